"""Values of `+ - * / %`, CAST, comparisons and date_part at the edges of their types, from each of the four evaluators, against the
exact reference tests/expr_ref.py (itself held to the oracle and to Python's calendar by tests/test_expr_reference.py): bit for bit,
a computed NaN as "is NaN", an error by its message prefix.  No tolerance appears in this file.

The evaluators, each proven to have run: column-at-a-time (`ops.project`, `ops.filter`, and `ops.aggregate` with fusion off:
fused_updates == 0), the register program (`register`: jit = 0 under GROUP BY row, an Int64 key whose groups are interned by hashing,
which is k_agg_fused with the register file in VGPRs: fused_updates > 0, nothing compiled), the tile program (`tile`: jit = 0 under
GROUP BY two UInt8 columns, which is k_agg_fused_tile with the register file in LDS: fused_updates > 0, nothing compiled, and
"agg_fused_tile" in the profile) and the source specialised with hiprtc (`specialised`: jit = 1: fused_updates > 0 and one more node
compiled; the on-disk code-object cache is off here so that a warm cache cannot serve the node and leave that count where it was).
A value leaves a fused node with one row per group: MAX(expr) carries an Int32 / Int64 / Float64 by its bits, SUM(expr) a Decimal128
by its 128-bit word (a one-row wrapping sum is the value), COUNT(expr) its NULL-ness.  The groups are the rows: GROUP BY row, and for
`tile` GROUP BY k0 = row & 0xFF, k1 = row >> 8 (4097 one-row groups: past the kernel's 256 local slots, into its key-indexed partials).
Predicates are read both as values (tests.expr_cases.truth) and as the node's predicate, by the rows that come back.  date_part as
the group key is not a `tile` case: that node's keys are plain UInt8 columns.

Division and the casts the row programs decline (Decimal128 scale-down, Decimal128 <-> Float64) are column-at-a-time by design: a fused
node holding one must fall back (fused_updates == 0) with the same values."""
import re

import numpy as np
import pyarrow as pa
import pytest

from tests import edge_values as E
from tests import expr_cases as C
from tests import expr_ref as R

pytestmark = pytest.mark.gpu

EVALUATORS = ("column", "register", "specialised")
NODE_EVALUATORS = EVALUATORS + ("tile",)
MAX_AGGS = 16               # accumulators of one aggregate node (csrc/aggregate.hip)
# what one tile node holds (csrc/aggregate.hip agg_update_small_single_pass): SM_MAX_CELLS LDS cells per group, a SUM(Decimal128) taking
# 3; and per lane (TILE_LDS_BUDGET - 4096) / BLOCK = 240 bytes of LDS register file, a Decimal128 / UInt64 register taking 16, any other 8
TILE_CELLS, TILE_REGFILE = 48, 240
SPECIALISED = dict(jit="1", jit__min_rows="0", jit__strict="1", jit__cache="0")
_compiled_nodes = set()     # (family, what) whose specialised node this process has built already


def _dev(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


def _aggregate(table, group_by, aggs, evaluator, predicate=None, fused=True, node=None) -> pa.Table:
    """ops.aggregate on one evaluator, with the proof that it was that one"""
    from datafusion_amd import ops
    info = {}
    try:
        if evaluator == "column":
            ops.set_fusion(False)
        else:
            ops.set_options(**(SPECIALISED if evaluator == "specialised" else dict(jit="0")))
        if evaluator == "tile":
            ops.profile_enable(True)
            ops.profile_reset()
        before = ops.jit_stats()[0]
        out = ops.aggregate(_dev(table), group_by, aggs, "Single", predicate=predicate, info=info).to_arrow()
        compiled = ops.jit_stats()[0] - before
        stats = ops.profile_stats() if evaluator == "tile" else {}
    finally:
        if evaluator == "tile":
            ops.profile_enable(False)
        ops.reset_options()
        ops.set_fusion(True)
    if evaluator == "tile":
        assert "agg_fused_tile" in stats, (sorted(stats), info)
        assert info["fused_updates"] > 0 and compiled == 0, (info, compiled)
        return out
    if evaluator == "column" or not fused:
        assert info["fused_updates"] == 0, (evaluator, info)
        assert compiled == 0
    else:
        assert info["fused_updates"] > 0, (evaluator, info)
        if evaluator == "register":
            assert compiled == 0
        elif node is not None and node not in _compiled_nodes:
            _compiled_nodes.add(node)
            assert compiled >= 1, f"{node}: no specialised node was compiled"
    return out


def _by_row(out: pa.Table) -> pa.Table:
    return out.take(pa.array(np.argsort(np.asarray(out.column("row"), dtype=np.int64), kind="stable")))


KEY_BYTES = ("k0", "k1")


def _with_key_bytes(table: pa.Table) -> pa.Table:
    """the table with its row number as two plain UInt8 columns: the keys of a tile node"""
    rows = np.arange(table.num_rows)
    return table.append_column("k0", pa.array((rows & 0xFF).astype(np.uint8))).append_column("k1", pa.array((rows >> 8).astype(np.uint8)))


def _by_key_bytes(out: pa.Table) -> pa.Table:
    """the groups of a tile node in row order, with the row rebuilt from (k1, k0)"""
    rows = np.asarray(out.column("k1"), dtype=np.int64) * 256 + np.asarray(out.column("k0"), dtype=np.int64)
    return out.append_column("row", pa.array(rows)).take(pa.array(np.argsort(rows, kind="stable")))


def _is_wide(typ):
    return pa.types.is_decimal128(typ) or typ == pa.uint64()


def _tile_nodes(f, ref) -> list:
    """the family's value names split over as few tile nodes as hold them, each value with its COUNT beside it.  A node is filled while
    (a) its accumulators stay within MAX_AGGS, (b) its cells within TILE_CELLS, (c) its lane registers within TILE_REGFILE: the table's
    columns and the two keys, 16 bytes per value (a Decimal128; or a Float64 with the ordered key MAX takes beside it), and 64 bytes for
    the temporaries of one expression (two wide, four narrow: the deepest are `nest` and `truth`)."""
    fixed = sum(16 if _is_wide(c.type) else 8 for c in f.table.drop_columns(["row"]).schema) + 2 * 8 + 64
    nodes, accs, cells, regs = [[]], 0, 0, fixed
    for nm, _ in f.values:
        c = (3 if pa.types.is_decimal128(ref[nm].typ) else 1) + 1
        if accs + 2 > MAX_AGGS or cells + c > TILE_CELLS or regs + 16 > TILE_REGFILE:
            nodes.append([])
            accs, cells, regs = 0, 0, fixed
        nodes[-1].append(nm)
        accs, cells, regs = accs + 2, cells + c, regs + 16
    assert all(nodes) and sorted(nm for node in nodes for nm in node) == sorted(nm for nm, _ in f.values)
    return nodes


def _values_through_tile_nodes(f, ref):
    """every value expression of the family through k_agg_fused_tile, GROUP BY (k0, k1)"""
    from datafusion_amd.expr import col
    table, exprs = _with_key_bytes(f.table), dict(f.values)
    for names in _tile_nodes(f, ref):
        aggs = [(_carrier(ref[nm].typ), exprs[nm], nm) for nm in names] + [("count", exprs[nm], nm + "__n") for nm in names]
        out = _by_key_bytes(_aggregate(table, [(col(k), k) for k in KEY_BYTES], aggs, "tile"))
        assert out.column("row").to_pylist() == list(range(table.num_rows))
        for nm in names:
            _check(out.column(nm), ref[nm], f"{f.name}.{nm} [tile]", carried=True)
            assert out.column(nm + "__n").to_pylist() == [0 if v is None else 1 for v in ref[nm].vals], f"{f.name}.{nm} [tile]: COUNT"


def _carrier(typ):
    return "sum" if pa.types.is_decimal128(typ) else "max"


def _check(got_col, want: R.Val, what, carried=False):
    typ = got_col.type
    if carried and pa.types.is_decimal128(want.typ):
        assert typ == pa.decimal128(min(38, want.typ.precision + 10), want.typ.scale), (what, typ)   # SUM's return type; the word is the value
        typ = want.typ
    diff = R.same(R.Val(typ, R.column_values(got_col)), want)
    assert diff is None, f"{what}: {diff}"


def _values_through_a_node(f, evaluator, table=None, ref=None):
    """every value expression of the family as one aggregate node, GROUP BY row"""
    from datafusion_amd.expr import col
    table, ref = f.table if table is None else table, C.reference(f.name) if ref is None else ref
    if evaluator == "tile":
        return _values_through_tile_nodes(f, ref)
    assert len(f.values) < MAX_AGGS
    counted = [nm for nm, _ in f.values][:MAX_AGGS - len(f.values)]          # COUNT(expr) beside as many values as the node has room for
    aggs = [(_carrier(ref[nm].typ), e, nm) for nm, e in f.values] + [("count", e, nm + "__n") for nm, e in f.values if nm in counted]
    node = None if f.name.startswith("int32_") else (f.name, "values")     # (the 63 / 64 / 65-row tables can share one node)
    out = _by_row(_aggregate(table, [(col("row"), "row")], aggs, evaluator, fused=f.fused, node=node))
    assert out.column("row").to_pylist() == list(range(table.num_rows))
    for nm, _ in f.values:
        _check(out.column(nm), ref[nm], f"{f.name}.{nm} [{evaluator}]", carried=True)
    for nm in counted:
        assert out.column(nm + "__n").to_pylist() == [0 if v is None else 1 for v in ref[nm].vals], f"{f.name}.{nm} [{evaluator}]: COUNT"


def _rows_under_the_node_predicate(f, evaluator):
    from datafusion_amd.expr import col
    nm, pred = f.node_pred
    want = [i for i, v in enumerate(C.reference(f.name)[nm].vals) if v is True]
    assert 0 < len(want) < f.table.num_rows
    if evaluator == "tile":
        out = _by_key_bytes(_aggregate(_with_key_bytes(f.table), [(col(k), k) for k in KEY_BYTES], [("count", None, "n")], evaluator, predicate=pred))
    else:
        out = _by_row(_aggregate(f.table, [(col("row"), "row")], [("count", None, "n")], evaluator, predicate=pred, node=(f.name, "predicate")))
    assert out.column("row").to_pylist() == want, f"{f.name}.{nm} [{evaluator}]: rows under the node's predicate"
    assert out.column("n").to_pylist() == [1] * len(want)


# ------------------------------------------------------------------------------------------------------------- the fused families
@pytest.mark.parametrize("evaluator", NODE_EVALUATORS)
@pytest.mark.parametrize("name", C.FUSED)
def test_values_and_predicates(name, evaluator):
    from datafusion_amd import ops
    f, ref = C.family(name), C.reference(name)
    if evaluator == "column":
        d = _dev(f.table)
        exprs = f.values + f.tris
        out = ops.project(d, [(e, nm) for nm, e in exprs]).to_arrow()
        for nm, _ in exprs:
            _check(out.column(nm), ref[nm], f"{name}.{nm} [project]")
        for nm, pred in f.preds:
            rows = ops.filter(d, pred, ["row"]).to_arrow().column("row").to_pylist()
            assert rows == [i for i, v in enumerate(ref[nm].vals) if v is True], f"{name}.{nm} [filter]"
    _values_through_a_node(f, evaluator)
    if f.node_pred is not None:
        _rows_under_the_node_predicate(f, evaluator)


# ------------------------------------------------------------------------- division and the declined casts: column-at-a-time by design
@pytest.mark.parametrize("name", C.DECLINED)
def test_division_and_declined_casts_fall_back_with_the_same_values(name):
    from datafusion_amd import ops
    f, ref = C.family(name), C.reference(name)
    assert not f.fused
    d = _dev(f.table)
    exprs = f.values + f.tris
    out = ops.project(d, [(e, nm) for nm, e in exprs]).to_arrow()
    for nm, _ in exprs:
        _check(out.column(nm), ref[nm], f"{name}.{nm} [project]")
    for nm, pred in f.preds:
        rows = ops.filter(d, pred, ["row"]).to_arrow().column("row").to_pylist()
        assert rows == [i for i, v in enumerate(ref[nm].vals) if v is True], f"{name}.{nm} [filter]"
    for evaluator in EVALUATORS:
        _values_through_a_node(f, evaluator)       # asserts fused_updates == 0 for all three


@pytest.mark.parametrize("kind", C.ERROR_KINDS)
def test_one_offending_row_raises_the_references_error_and_a_null_there_does_not(kind):
    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    from tests.util import to_oracle_expr
    for pos in C.ERROR_POSITIONS:
        bad, null_left, null_right, e, prefix = C.error_tables(kind, pos)
        with pytest.raises(_lib.DfgpuError, match="^" + re.escape(prefix)):
            ops.project(_dev(bad), [(e, "v")])
        for t in (null_left, null_right):
            out = ops.project(_dev(t), [(e, "v")]).to_arrow()
            _check(out.column("v"), R.evaluate(to_oracle_expr(e), t), f"{kind} at {pos}, NULL there")
    # the same through an aggregate node asked to fuse: it falls back, and the error is the column kernels'
    bad, null_left, _, e, prefix = C.error_tables(kind, 64)
    for evaluator in ("register", "specialised"):
        with pytest.raises(_lib.DfgpuError, match="^" + re.escape(prefix)):
            _aggregate(bad, [(col("row"), "row")], [("count", e, "n")], evaluator, fused=False)
        out = _by_row(_aggregate(null_left, [(col("row"), "row")], [("count", e, "n")], evaluator, fused=False))
        assert out.column("n").to_pylist() == [0 if i == 64 else 1 for i in range(C.N)]


@pytest.mark.parametrize("name", list(C.CAST_ERRORS))
def test_one_value_beyond_a_casts_range_raises_the_references_error(name):
    from datafusion_amd import _lib, ops
    from tests.util import to_oracle_expr
    for pos in C.ERROR_POSITIONS:
        bad, null, e, prefix = C.cast_error_tables(name, pos)
        with pytest.raises(_lib.DfgpuError, match="^" + re.escape(prefix)):
            ops.project(_dev(bad), [(e, "v")])
        out = ops.project(_dev(null), [(e, "v")]).to_arrow()
        _check(out.column("v"), R.evaluate(to_oracle_expr(e), null), f"{name} at {pos}, NULL there")


# ------------------------------------------------------------------------------------------------------------------------ date_part
@pytest.mark.parametrize("evaluator", EVALUATORS)
def test_date_part_as_the_group_key_of_the_node(evaluator):
    from datafusion_amd.expr import col, date_part
    f = C.family("date")
    days = R.column_values(f.table.column("dt"))
    want = {}
    for i, d in enumerate(days):
        y = None if d is None else R.ymd(d)[0]
        n, top, last = want.get(y, (0, None, -1))
        want[y] = (n + 1, d if top is None or (d is not None and d > top) else top, i)
    out = _aggregate(f.table, [(date_part("year", col("dt")), "y")], [("count", None, "n"), ("max", col("dt"), "top"), ("max", col("row"), "last")],
                     evaluator, node=("date", "group key"))
    assert out.schema.field("y").type == pa.int32()
    got = {y: (n, top, last) for y, n, top, last in zip(out.column("y").to_pylist(), out.column("n").to_pylist(),
                                                        R.column_values(out.column("top")), out.column("last").to_pylist())}
    assert len(got) == out.num_rows and got == want


# ------------------------------------------------------------------------------------------------------- inside the join's probe
@pytest.mark.parametrize("pred_in_counts", ["0", "1"])
def test_a_wrapping_sum_compared_inside_the_join_probe(pred_in_counts):
    """`a + b < c` over Int32 sums that wrap, as the predicate of a probe over unique build keys: the rows that join are the rows the
    reference keeps"""
    from datafusion_amd import ops
    f = C.family("int32")
    nm, pred = f.node_pred
    keep = [i for i, v in enumerate(C.reference("int32")[nm].vals) if v is True and i % 2 == 0]
    build = pa.table({"k": pa.array(np.arange(0, C.N, 2, dtype=np.int64)), "bv": pa.array(np.arange(0, C.N, 2, dtype=np.int64) * 3)})
    ops.set_options(join__pred_in_counts=pred_in_counts)
    ht = ops.JoinHashTable(_dev(build), ["k"])
    try:
        got = ht.probe(_dev(f.table), ["row"], "Inner", predicate=pred).to_arrow()
    finally:
        ht.free()
    got = _by_row(got)
    assert got.column("row").to_pylist() == keep and got.column("bv").to_pylist() == [3 * i for i in keep]
    for c in "abc":
        w, v = E.words_of(f.table.column(c))
        gw, gv = E.words_of(got.column(c))
        assert np.array_equal(w[keep], gw) and np.array_equal(v[keep], gv), c


# ------------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("typ", [pa.uint8(), pa.uint32(), pa.uint64()], ids=str)
def test_arithmetic_over_unsigned_columns_is_refused_everywhere(typ):
    """never a sign-extended answer: the projection and the aggregate node, interpreted or specialised, all raise"""
    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    top = {pa.uint8(): 255, pa.uint32(): 2**32 - 1, pa.uint64(): 2**64 - 1}[typ]
    t = C.with_row({"u": pa.array([top, top - 1, 1, 0] * 20, type=typ), "w": pa.array([1, top, top, 2] * 20, type=typ)})
    refusal = "arithmetic on .* is not supported on the GPU path"
    for e in (col("u") + col("w"), col("u") * col("w"), col("u") - col("w")):
        with pytest.raises(_lib.DfgpuError, match=refusal):
            ops.project(_dev(t), [(e, "v")])
        for evaluator in EVALUATORS:
            with pytest.raises(_lib.DfgpuError, match=refusal):
                _aggregate(t, [(col("row"), "row")], [("max", e, "v")], evaluator, fused=False)

"""Every operator at the edges of its value types, on every path it can be forced onto, against the oracle (itself checked at the same
edges by tests/test_edge_values_oracle.py).  Columns come from tests/edge_values.py: the extremes of each integer type, unsigned
values at and above 2^31 / 2^63, decimals beyond 64 bits, and the floats where order-preserving keys go wrong (both zeros, both
infinities, NaN of either sign and with a payload, subnormals, ±DBL_MAX).  Key columns of joins, aggregates and sorts also take
spans of exactly 2^k - 1, 2^k and 2^k + 1, where the range gates switch paths.  Results are compared with tests.edge_values.assert_exact:
moved floats by their bits, computed ones with NaN = NaN and signed zeros."""
import math

import numpy as np
import pyarrow as pa
import pytest

from tests import edge_values as E
from tests import variance_ref as V

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 4095, 4096, 4097, 70_000]
DESC_NULLS = [(False, False), (False, True), (True, False), (True, True)]


def _dev(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


def _opts(**kv):
    from datafusion_amd import ops
    if kv:
        ops.set_options(**kv)


def _with_rows(cols: dict, n: int) -> pa.Table:
    return pa.table({**cols, "row": pa.array(np.arange(n, dtype=np.int64))})


# ------------------------------------------------------------------------------------------------------------------------ sort

SORT_TYPES = [pa.int32(), pa.int64(), pa.date32(), pa.uint32(), pa.uint64(), pa.float64(), pa.decimal128(18, 2), pa.decimal128(38, 0)]
SORT_PATHS = {"default": {}, "no_small": {"sort__small": "0"}}
SORT_CASES = [("default", n) for n in ROWS] + [("no_small", n) for n in (65, 4097)]


def _check_sorted(got: pa.Table, exp: pa.Table, table: pa.Table, keys):
    """the key columns exactly as the oracle orders them (bits), and every output row is the input row it claims to be (ties may
    come out in another order: the sort is not stable)"""
    E.assert_exact(got.select(keys), exp.select(keys), ordered=True)
    rows = np.asarray(got.column("row"), dtype=np.int64)
    assert len(np.unique(rows)) == len(rows)
    for name in table.column_names:
        w, v = E.words_of(table.column(name))
        gw, gv = E.words_of(got.column(name))
        assert np.array_equal(w[rows], gw) and np.array_equal(v[rows], gv), name


@pytest.mark.parametrize("typ", SORT_TYPES, ids=str)
@pytest.mark.parametrize("path, n", SORT_CASES)
def test_sort_one_key(typ, path, n):
    from datafusion_amd import ops
    from oracle import oracle
    rng = np.random.default_rng(n * 31 + SORT_TYPES.index(typ))
    t = _with_rows({"k": E.edge_array(rng, n, typ, 0.3, 0.1), "p": E.edge_array(rng, n, pa.float64(), 0.5)}, n)
    _opts(**SORT_PATHS[path])
    d = _dev(t)
    for desc, nf in DESC_NULLS:
        keys = [("k", desc, nf)]
        _check_sorted(ops.sort(d, keys).to_arrow(), oracle.sort(t, keys), t, ["k"])
    for i, fetch in enumerate(sorted({0, 1, max(n - 1, 0), n, n + 5})):
        keys = [("k",) + DESC_NULLS[i % 4]]
        _check_sorted(ops.sort(d, keys, fetch=fetch).to_arrow(), oracle.sort(t, keys, fetch=fetch), t, ["k"])


# carried / LSD sorts read the key columns back out of the packed key: NULL-free integer keys at the edges of their types, a 16-byte
# payload (p, row), and the kernel that must have run
CARRIED_PATHS = {
    "lsd": ({"sort__carried_min_rows": "0"}, "sort_lsd_pass_out"),
    "carried_onesweep": ({"sort__carried": "onesweep", "sort__carried_min_rows": "0", "sort__lsd": "0"}, "sort_onesweep_pass"),
    "carried_ids": ({"sort__carried": "ids", "sort__carried_min_rows": "0", "sort__lsd": "0"}, "sort_build_records"),
    "carried_passes": ({"sort__carried": "passes", "sort__carried_min_rows": "0", "sort__lsd": "0"}, "sort_carried_pass"),
}
# (type, lowest key, span): spans up to 2^32 for the LSD sort (the product of its digit ranges), 2^62 for the carried ones
CARRIED_KEYS = {
    "i32_full": (pa.int32(), E.I32_MIN, 2**32 - 1), "date_full": (pa.date32(), E.I32_MIN, 2**32 - 1), "u32_full": (pa.uint32(), 0, 2**32 - 1),
    "i64_min": (pa.int64(), E.I64_MIN, None), "i64_max": (pa.int64(), None, None), "u64_2_63": (pa.uint64(), 2**63 - 2**20, None),
    "u64_max": (pa.uint64(), None, None),
}


def _carried_key(rng, n, name, path):
    typ, low, span = CARRIED_KEYS[name]
    if span is None:
        span = 2**31 if path == "lsd" else 2**62
    hi_t = E.type_range(typ)[1]
    if low is None:
        low = hi_t - span          # the top of the type: INT64_MAX / UINT64_MAX is the largest key
    return E.span_array(rng, n, typ, span, low)


@pytest.mark.parametrize("name", list(CARRIED_KEYS))
@pytest.mark.parametrize("path", list(CARRIED_PATHS))
def test_sort_carried_and_lsd_paths_rebuild_edge_keys(name, path):
    from datafusion_amd import ops
    from oracle import oracle
    n = 70_000
    rng = np.random.default_rng(n + list(CARRIED_KEYS).index(name) * 5 + len(path))
    t = _with_rows({"k": _carried_key(rng, n, name, path), "p": E.edge_array(rng, n, pa.float64(), 0.5)}, n)
    opts, kernel = CARRIED_PATHS[path]
    ops.set_options(**opts)
    d = _dev(t)
    for desc in (False, True):
        keys = [("k", desc, False)]
        ops.profile_enable(True)
        ops.profile_reset()
        try:
            got = ops.sort(d, keys).to_arrow()
            stats = ops.profile_stats()
        finally:
            ops.profile_enable(False)
        assert kernel in stats, sorted(stats)       # the sort under test ran
        _check_sorted(got, oracle.sort(t, keys), t, ["k"])


@pytest.mark.parametrize("spans, narrow", [((2**31 - 1, 2**32 - 1), True), ((2**31 - 1, 2**32 - 2), True), ((2**62 - 2, 1), True),
                                           ((2**31, 2**32 - 1), False), ((2**31 - 1, 2**32), False), ((2**62, 1), False),
                                           ((2**64 - 1, 2**32 - 1), False)])
@pytest.mark.parametrize("n", [4097, 70_000])
@pytest.mark.parametrize("nulls", [0.0, 0.05])
def test_sort_two_keys_around_the_mixed_radix_limit(spans, narrow, n, nulls):
    """sort.hip packs the keys mixed-radix into one word when the product of the key ranges (span + 1, doubled by a NULL flag) is at
    most 2^63, into bit fields otherwise: products at, just below and just above 2^63; with NULLs every case is wide"""
    from datafusion_amd import ops
    from oracle import oracle
    assert ((spans[0] + 1) * (spans[1] + 1) * (4 if nulls else 1) <= 2**63) == (narrow and not nulls)
    rng = np.random.default_rng(n + int(narrow) + int(nulls * 100))
    a = E.span_array(rng, n, pa.int64(), spans[0], null_frac=nulls)
    b = E.span_array(rng, n, pa.int64() if spans[1] < 2**63 else pa.uint64(), spans[1], null_frac=nulls)
    # few distinct values of the first key so the second one decides
    t = _with_rows({"a": a, "b": b}, n)
    d = _dev(t)
    for desc, nf in DESC_NULLS:
        keys = [("a", desc, nf), ("b", not desc, not nf)]
        _check_sorted(ops.sort(d, keys).to_arrow(), oracle.sort(t, keys), t, ["a", "b"])
        _check_sorted(ops.sort(d, keys, fetch=100).to_arrow(), oracle.sort(t, keys, fetch=100), t, ["a", "b"])


def test_sort_float_and_unsigned_keys_together():
    from datafusion_amd import ops
    from oracle import oracle
    rng = np.random.default_rng(5)
    for n in (4095, 70_000):
        t = _with_rows({"f": E.edge_array(rng, n, pa.float64(), 0.7, 0.05), "u": E.edge_array(rng, n, pa.uint64(), 0.7, 0.05),
                        "d": E.edge_array(rng, n, pa.decimal128(19, 0), 0.7)}, n)
        d = _dev(t)
        for desc, nf in DESC_NULLS:
            keys = [("f", desc, nf), ("u", desc, not nf)]
            _check_sorted(ops.sort(d, keys).to_arrow(), oracle.sort(t, keys), t, ["f", "u"])
            keys = [("u", desc, nf), ("d", not desc, nf)]     # 65 + 66 bits (a third such key would pass the 192-bit limit)
            _check_sorted(ops.sort(d, keys).to_arrow(), oracle.sort(t, keys), t, ["u", "d"])


def test_sort_three_full_span_decimal38_keys_is_refused_and_stays_on_the_cpu():
    """3 x 129 bits of Decimal128(38) keys are beyond the 192-bit packed key: the library refuses them with the documented error, and
    GpuOffloadRule keeps the SortExec on the CPU"""
    from datafusion_amd import _lib, ops
    from datafusion_amd import physical_plan as P
    rng = np.random.default_rng(8)
    typ = pa.decimal128(38, 0)
    t = _with_rows({c: E.span_array(rng, 500, typ, 2 * (10**38 - 1)) for c in "abc"}, 500)
    keys = [("a", False, False), ("b", True, False), ("c", False, True)]
    with pytest.raises(_lib.DfgpuError, match="packed sort key longer than 192 bits is not supported on the GPU path"):
        ops.sort(_dev(t), keys).to_arrow()
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.SortExec(keys, P.MemoryExec(_dev(t), "t")))
    assert getattr(out, "kept_on_cpu", False) and "192" in rule.declined[0][1], rule.declined


# ------------------------------------------------------------------------------------------------------------ filter / projection

CMP = ["=", "!=", "<", "<=", ">", ">="]
FILTER_TYPES = [pa.int32(), pa.int64(), pa.uint32(), pa.uint64(), pa.float64(), pa.decimal128(38, 0), pa.date32()]


def _pexpr(op, a, b):
    from datafusion_amd.expr import BinaryExpr
    return BinaryExpr(a, op, b)


def _edge_literals(typ):
    """every edge of the type as a literal (Date32: an Int32 day number cast to Date32, the extremes have no datetime.date)"""
    from datafusion_amd.expr import lit
    if pa.types.is_date32(typ):
        return [lit(v, pa.int32()).cast(pa.date32()) for v in E.edges_of(typ)]
    return [lit(E.from_raw([raw], typ)[0].as_py(), typ) for raw in E.edges_of(typ)]


def _filter_table(typ, n):
    rng = np.random.default_rng(n + FILTER_TYPES.index(typ) * 7)
    return _with_rows({"a": E.edge_array(rng, n, typ, 0.5, 0.05), "b": E.edge_array(rng, n, typ, 0.5, 0.05),
                       "p": E.edge_array(rng, n, pa.float64(), 0.5)}, n)


@pytest.mark.parametrize("typ", FILTER_TYPES, ids=str)
@pytest.mark.parametrize("n", [63, 4097, 70_000])
def test_filter_and_projection_compare_by_total_order(typ, n):
    """FilterExec and ProjectionExec (evaluated column-at-a-time): column against column and against every edge literal, floats by
    totalOrder (NaN = NaN, -0.0 < +0.0), unsigned as unsigned"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    from oracle import oracle
    from tests.util import to_oracle_expr
    t = _filter_table(typ, n)
    d = _dev(t)
    preds = [_pexpr(op, col("a"), col("b")) for op in CMP] + [_pexpr(op, col("a"), v) for v in _edge_literals(typ) for op in ("<", "=", ">=")]
    for pred in preds:
        exp = oracle.filter(t, to_oracle_expr(pred), ["a", "p", "row"])
        E.assert_exact(ops.filter(d, pred, ["a", "p", "row"]).to_arrow(), exp, ordered=True)
    proj = [(col("a"), "a"), (col("p"), "p"), (_pexpr("<", col("a"), col("b")), "lt"), (_pexpr("=", col("p"), col("p")), "self_eq")]
    exp = oracle.project(t, [(to_oracle_expr(e), nm) for e, nm in proj])
    E.assert_exact(ops.project(d, proj).to_arrow(), exp, ordered=True)


@pytest.mark.parametrize("typ", FILTER_TYPES, ids=str)
@pytest.mark.parametrize("path", ["specialised", "register"])
def test_fused_filter_node_compares_by_total_order(typ, path):
    """the same comparisons as the predicate of the fused FilterExec -> AggregateExec node, specialised (hiprtc) and as the register
    program: GROUP BY the row number shows exactly which rows passed, MAX carries a float payload through by its bits"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    from oracle import oracle
    from tests.util import to_oracle_expr
    n = 4097
    t = _filter_table(typ, n)
    d = _dev(t)
    ops.set_options(**({"jit": "1", "jit__min_rows": "0", "jit__strict": "1"} if path == "specialised" else {"jit": "0"}))
    group_by, aggs = [(col("row"), "row")], [("count", None, "c"), ("max", col("p"), "p")]
    preds = [_pexpr(op, col("a"), col("b")) for op in CMP] + [_pexpr("<", col("a"), v) for v in _edge_literals(typ)]
    for pred in preds:
        info = {}
        got = ops.aggregate(d, group_by, aggs, "Single", predicate=pred, info=info).to_arrow()
        assert info["fused_updates"] > 0, "the fused node did not take the predicate"
        exp = _oracle_agg(oracle.filter(t, to_oracle_expr(pred)), group_by, aggs)
        E.assert_exact(got, exp, ordered=False)


@pytest.mark.parametrize("pred_in_counts", ["1", "0"])
@pytest.mark.parametrize("typ", [pa.float64(), pa.uint64(), pa.int64()], ids=str)
def test_predicate_inside_the_join_probe(pred_in_counts, typ):
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    from oracle import oracle
    from tests.util import to_oracle_expr
    rng = np.random.default_rng(len(str(typ)) + int(pred_in_counts))
    nb, npr = 3000, 70_000
    build = pa.table({"k": pa.array(rng.integers(0, 2000, nb), pa.int64()), "bv": E.edge_array(rng, nb, pa.float64(), 0.5)})
    probe = _with_rows({"k": pa.array(rng.integers(0, 2500, npr), pa.int64()), "a": E.edge_array(rng, npr, typ, 0.5, 0.05),
                        "b": E.edge_array(rng, npr, typ, 0.5, 0.05)}, npr)
    ops.set_options(join__pred_in_counts=pred_in_counts)
    for op in ("<", "=", ">="):
        pred = _pexpr(op, col("a"), col("b"))
        fp = oracle.filter(probe, to_oracle_expr(pred))
        for jt in ("Inner", "RightSemi", "RightAnti", "Left"):
            ht = ops.JoinHashTable(_dev(build), ["k"])
            got = ht.probe(_dev(probe), ["k"], jt, predicate=pred)
            if jt == "Left":
                tail = ht.emit_unmatched(jt, None, ops.tail_probe_schema(_dev(probe), jt))
                got = ops.concat_tables([got, tail])
            ht.free()
            E.assert_exact(got.to_arrow(), oracle.hash_join(build, fp, [("k", "k")], jt), ordered=False)


# ------------------------------------------------------------------------------------------------------------ aggregate

AGG_PATHS = {
    "default": ({}, False),
    "specialised": ({"jit": "1", "jit__min_rows": "0", "jit__strict": "1"}, True),
    "interpreted": ({"jit": "0"}, True),
    "column": (None, True),
    "partitioned": ({"agg__partitioned_min_rows": "1"}, False),
    "no_grouped_move": ({"agg__grouped_move": "0"}, False),
    "no_gather_emit": ({"agg__gather_emit": "0"}, False),
    "no_records": ({"group__records": "0"}, False),
}
KEY_SHAPES = {
    "i32_i32": [pa.int32(), pa.int32()],     # 64 bits of key (the keyed table when NULL-free: test_group_by_keyed_table_at_64_bits_of_key)
    "i64_i32": [pa.int64(), pa.int32()],     # 96 bits
    "u64": [pa.uint64()],
    "f64": [pa.float64()],
    "date_dec": [pa.date32(), pa.decimal128(19, 0)],
}
FLOAT_SUM_EDGES = [E.f64_bits(x) for x in (0.0, -0.0, math.inf, -math.inf)] + [E.QNAN_BITS, E.NEG_QNAN_BITS]


def _agg_table(rng, n, key_types, null_frac=0.05, key_edge_frac=0.3, key_null_frac=None):
    key_null_frac = null_frac if key_null_frac is None else key_null_frac
    cols = {f"k{i}": E.edge_array(rng, n, t, key_edge_frac, key_null_frac) for i, t in enumerate(key_types)}
    cols.update({
        "i": E.edge_array(rng, n, pa.int64(), 0.3, null_frac),
        "u": E.edge_array(rng, n, pa.uint64(), 0.3, null_frac),
        "f": E.edge_array(rng, n, pa.float64(), 0.3, null_frac),
        "fs": E.edge_array(rng, n, pa.float64(), 0.1, null_frac, edges=FLOAT_SUM_EDGES),   # sums of these do not depend on the order
        "d": E.edge_array(rng, n, pa.decimal128(18, 2), 0.3, null_frac),
        "w": E.edge_array(rng, n, pa.decimal128(38, 0), 0.3, null_frac, edges=[0, 2**63 - 1, -2**63, -(2**63 - 1), 1, -1]),
    })
    return _with_rows(cols, n)


def _agg_list():
    from datafusion_amd.expr import col
    return [("count", None, "cnt"), ("count", col("f"), "cf"), ("sum", col("i"), "si"), ("sum", col("u"), "su"), ("min", col("i"), "mini"),
            ("max", col("i"), "maxi"), ("min", col("f"), "minf"), ("max", col("f"), "maxf"), ("sum", col("fs"), "sf"), ("avg", col("fs"), "af"),
            ("sum", col("d"), "sd"), ("min", col("d"), "mind"), ("max", col("d"), "maxd"), ("min", col("w"), "minw"), ("max", col("w"), "maxw")]


COMPUTED = ("sf", "af")


def _oracle_agg(t, group_by, aggs):
    from oracle import oracle
    from tests.util import to_oracle_expr
    return oracle.aggregate(t, [(to_oracle_expr(e), nm) for e, nm in group_by], [(f, None if e is None else to_oracle_expr(e), nm) for f, e, nm in aggs])


def _run_agg(t, group_by, aggs, path, mode="Single"):
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    opts, with_pred = AGG_PATHS[path]
    pred = (col("row") >= lit(0, pa.int64())) if with_pred else None     # true on every row: what makes the fused node take the aggregate
    if opts is None:
        ops.set_fusion(False)
    else:
        _opts(**opts)
    try:
        if mode == "Single":
            return ops.aggregate(_dev(t), group_by, aggs, "Single", predicate=pred).to_arrow()
        n = t.num_rows
        cuts = sorted({0, n // 3, n // 3 + 1, n})
        parts = [ops.aggregate(_dev(t.slice(a, b - a)), group_by, aggs, "Partial", predicate=pred).to_arrow() for a, b in zip(cuts, cuts[1:])]
        state = pa.concat_tables(parts)
        if mode == "PartialReduce":
            half = len(parts) // 2 or 1
            state = pa.concat_tables([ops.aggregate(_dev(pa.concat_tables(parts[:half])), group_by, aggs, "PartialReduce").to_arrow()] + parts[half:])
        rt = ops.aggregate_return_types(_dev(t), aggs)
        return ops.aggregate(_dev(state), group_by, aggs, "Final", return_types=rt).to_arrow()
    finally:
        ops.set_fusion(True)


AGG_CASES = [(s, "default", n, "Single") for s in KEY_SHAPES for n in ROWS] + \
    [(s, p, n, "Single") for s in KEY_SHAPES for p in AGG_PATHS if p != "default" for n in (4097, 70_000)] + \
    [(s, "default", n, m) for s in KEY_SHAPES for n in (4097, 70_000) for m in ("PartialFinal", "PartialReduce")]


@pytest.mark.parametrize("shape, path, n, mode", AGG_CASES)
def test_group_by_at_the_edges(shape, path, n, mode):
    """GROUP BY edge keys (64-bit keyed, 96-bit, UInt64 above 2^63, Float64 with both zeros and both NaNs as distinct groups, Date32 with
    a Decimal128(19)) with COUNT, SUM over Int64 that wraps and over UInt64, MIN / MAX by total order over floats and over decimals of
    64 bits, SUM / AVG over the float specials"""
    from datafusion_amd.expr import col
    rng = np.random.default_rng(n * 13 + list(KEY_SHAPES).index(shape))
    t = _agg_table(rng, n, KEY_SHAPES[shape])
    group_by = [(col(f"k{i}"), f"k{i}") for i in range(len(KEY_SHAPES[shape]))]
    aggs = _agg_list()
    exp = _oracle_agg(t, group_by, aggs)
    got = _run_agg(t, group_by, aggs, path, "Single" if mode == "Single" else ("Partial" if mode == "PartialFinal" else "PartialReduce"))
    E.assert_exact(got, exp, ordered=False, computed=COMPUTED)


def _profiled(fn):
    from datafusion_amd import ops
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        out = fn()
        return out, ops.profile_stats()
    finally:
        ops.profile_enable(False)


@pytest.mark.parametrize("shape, keyed", [("i32_i32", True), ("i64_i32", False)])
@pytest.mark.parametrize("n", [65_536, 70_000])
def test_group_by_keyed_table_at_64_bits_of_key(shape, keyed, n):
    """NULL-free keys of 64 bits together (two full-range Int32) take the keyed table, 96 bits (Int64 + Int32) the generic one"""
    from datafusion_amd.expr import col
    rng = np.random.default_rng(n + keyed)
    t = _agg_table(rng, n, KEY_SHAPES[shape], key_null_frac=0.0)
    group_by = [(col(f"k{i}"), f"k{i}") for i in range(2)]
    aggs = _agg_list()
    got, stats = _profiled(lambda: _run_agg(t, group_by, aggs, "default"))
    assert ("agg_intern_claim_keyed" in stats) == keyed and ("agg_intern_claim" in stats) == (not keyed), sorted(stats)
    E.assert_exact(got, _oracle_agg(t, group_by, aggs), ordered=False, computed=COMPUTED)


@pytest.mark.parametrize("typ", [pa.int32(), pa.date32(), pa.uint32()], ids=str)
def test_group_by_ordered_keys_take_the_runs_node(typ):
    """ordered NULL-free keys reaching the extremes of their type (no predicate: the runs node takes the aggregate itself)"""
    from datafusion_amd.expr import col
    n = 70_000
    rng = np.random.default_rng(31 + len(str(typ)))
    raw = sorted(E.edge_raw(rng, n, typ, 0.3))
    t = _agg_table(rng, n, [])
    t = t.add_column(0, "k", E.from_raw(raw, typ))
    group_by = [(col("k"), "k")]
    aggs = [("count", None, "cnt"), ("sum", col("i"), "si"), ("count", col("f"), "cf"), ("min", col("i"), "mini"), ("max", col("i"), "maxi"),
            ("sum", col("d"), "sd"), ("sum", col("fs"), "sf"), ("avg", col("fs"), "af")]
    from datafusion_amd import ops
    ops.set_options(jit="1", jit__min_rows="0", jit__strict="1", agg__runs="1")
    got, stats = _profiled(lambda: _run_agg(t, group_by, aggs, "default"))
    assert "agg_runs_accumulate" in stats, sorted(stats)
    E.assert_exact(got, _oracle_agg(t, group_by, aggs), ordered=False, computed=("sf", "af"))


def _span_low(typ, span):
    lo, hi = E.type_range(typ)
    return max(lo, min(-(span // 2), hi - span))


@pytest.mark.parametrize("span", [4095, 4096, 4097, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**64 - 1])
@pytest.mark.parametrize("path", ["default", "partitioned", "specialised", "column"])
def test_group_by_key_spans(span, path):
    """one Int64 key whose max - min sits on each side of the dense-range limit (4096), of 32 bits and of the wrapping 64-bit span"""
    from datafusion_amd.expr import col
    rng = np.random.default_rng(span % 1000 + len(path))
    n = 70_000
    t = _agg_table(rng, n, [])
    t = t.add_column(0, "k", E.span_array(rng, n, pa.int64(), span, null_frac=0.02))
    group_by = [(col("k"), "k")]
    aggs = _agg_list()
    E.assert_exact(_run_agg(t, group_by, aggs, path), _oracle_agg(t, group_by, aggs), ordered=False, computed=COMPUTED)


def test_group_by_at_a_full_pass_of_rows():
    """rows_worth_a_pass() rows or more (num_cus x 16384): paths no option lowers, the direct table among them; a small key range with
    the Int64 / UInt64 / Float64 edges in the arguments"""
    import torch
    from datafusion_amd.expr import col
    n = torch.cuda.get_device_properties(0).multi_processor_count * 16384 + 4097
    rng = np.random.default_rng(11)

    def column(typ, edges):
        bits = {pa.float64(): np.uint64}.get(typ)
        ordinary = rng.integers(-1000, 1000, n)
        vals = (ordinary.astype(np.float64) / 8).view(np.uint64) if bits is not None else ordinary.astype(np.int64).view(np.uint64)
        e = np.array(edges, dtype=np.uint64)
        vals = np.where(rng.random(n) < 0.2, e[rng.integers(0, len(e), n)], vals)
        vals[:len(e)] = e
        arr = pa.Array.from_buffers(typ, n, [None, pa.py_buffer(vals.tobytes())])
        return arr
    t = pa.table({"k": pa.array(rng.integers(-300, 300, n).astype(np.int32)),
                  "i": column(pa.int64(), [v & (2**64 - 1) for v in E.INT_EDGES[pa.int64()]]),
                  "u": column(pa.uint64(), E.INT_EDGES[pa.uint64()]),
                  "f": column(pa.float64(), E.F64_EDGE_BITS)})
    aggs = [("count", None, "cnt"), ("sum", col("i"), "si"), ("sum", col("u"), "su"), ("min", col("i"), "mini"), ("max", col("i"), "maxi"),
            ("min", col("f"), "minf"), ("max", col("f"), "maxf")]
    group_by = [(col("k"), "k")]
    exp = _oracle_agg(t, group_by, aggs)
    for path in ("default", "no_records"):
        E.assert_exact(_run_agg(t, group_by, aggs, path), exp, ordered=False)
    E.assert_exact(_run_agg(t, [], aggs, "default"), _oracle_agg(t, [], aggs), ordered=True)


@pytest.mark.parametrize("path", list(AGG_PATHS))
def test_min_max_over_decimal38_beyond_64_bits_is_refused(path):
    """MIN / MAX over Decimal128(38) compare 64-bit words: values of 64 bits go through every path, a value beyond them is the
    documented error (never a wrong answer), and GpuOffloadRule keeps such a node on the CPU"""
    from datafusion_amd import _lib
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    rng = np.random.default_rng(21)
    n = 5000
    typ = pa.decimal128(38, 0)
    t = _with_rows({"g": pa.array(rng.integers(0, 50, n).astype(np.int32)), "w": E.edge_array(rng, n, typ, 0.3, 0.05)}, n)
    aggs = [("min", col("w"), "lo"), ("max", col("w"), "hi")]
    with pytest.raises(_lib.DfgpuError, match="does not fit in 64 bits"):
        _run_agg(t, [(col("g"), "g")], aggs, path)
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.AggregateExec("Single", [(col("g"), "g")], aggs, P.MemoryExec(_dev(t), "t")))
    assert getattr(out, "kept_on_cpu", False) and "64-bit" in rule.declined[0][1], rule.declined


@pytest.mark.parametrize("func", ["min", "max"])
def test_min_max_over_uint64_is_refused_and_stays_on_the_cpu(func):
    """MIN / MAX compare signed 64-bit words on the device, which would misorder UInt64 values at and above 2^63: the library refuses
    the type with the documented error, and GpuOffloadRule keeps such a node on the CPU (SUM over UInt64 wraps and runs: above)"""
    from datafusion_amd import _lib
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    rng = np.random.default_rng(22)
    t = _with_rows({"g": pa.array(rng.integers(0, 50, 3000).astype(np.int32)), "u": E.edge_array(rng, 3000, pa.uint64(), 0.3)}, 3000)
    aggs = [(func, col("u"), "a")]
    with pytest.raises(_lib.DfgpuError, match="aggregate over UInt64 is not supported on the GPU path"):
        _run_agg(t, [(col("g"), "g")], aggs, "default")
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.AggregateExec("Single", [(col("g"), "g")], aggs, P.MemoryExec(_dev(t), "t")))
    assert getattr(out, "kept_on_cpu", False) and "UInt64" in rule.declined[0][1], rule.declined


def _var_groups(overflowing_sum=False):
    """(key, values) groups whose VAR does not depend on the order of the updates: ordinary dyadic values, a group per float special,
    groups of ±DBL_MAX alone and repeated, single values.  overflowing_sum: the repeated ±DBL_MAX groups are long enough for their sum
    to overflow (variance.rs keeps a running mean and gives 0.0; the device sums such a group again about one of its values)"""
    rng = np.random.default_rng(4)
    groups = []
    for g in range(40):
        groups.append((g, [float(v) / 8 for v in rng.integers(-8000, 8000, int(rng.integers(1, 300)))]))
    specials = [math.inf, -math.inf, float("nan"), E.f64_from_bits(E.NEG_QNAN_BITS)]
    for j, s in enumerate(specials):
        groups.append((100 + j, [float(v) for v in rng.integers(-50, 50, 200)] + [s]))
        groups.append((200 + j, [s]))
    groups.append((300, [math.inf, -math.inf]))
    for j, m in enumerate((E.DBL_MAX, -E.DBL_MAX)):
        groups.append((400 + j, [m] * (300 if overflowing_sum else 1)))
        groups.append((420 + j, [m / 4] * 2))
        groups.append((410 + j, [m]))
    groups.append((500, [-0.0, -0.0]))
    groups.append((501, [None, None]))
    return groups


@pytest.mark.parametrize("overflowing_sum", [False, True])
@pytest.mark.parametrize("path", ["default", "specialised", "interpreted", "column", "partitioned"])
@pytest.mark.parametrize("mode", ["Single", "PartialFinal"])
def test_variance_over_infinities_nans_and_dbl_max(path, mode, overflowing_sum):
    from datafusion_amd.expr import col
    groups = _var_groups(overflowing_sum)
    keys, xs = [], []
    for g, vals in groups:
        keys += [g] * len(vals)
        xs += vals
    perm = np.random.default_rng(3).permutation(len(xs))
    keys, xs = [keys[i] for i in perm], [xs[i] for i in perm]
    t = _with_rows({"g": pa.array(keys, pa.int32()), "x": pa.array(xs, pa.float64())}, len(xs))
    aggs = [(f, col("x"), f) for f in V.FUNCS]
    got = _run_agg(t, [(col("g"), "g")], aggs, path, "Single" if mode == "Single" else "Partial")
    want = {}
    for g, vals in groups:
        st = V.state_of(vals)
        want[g] = [V.finish(st, f) for f in V.FUNCS]
    order = sorted(want)
    exp = pa.table({"g": pa.array(order, pa.int32()), **{f: pa.array([want[g][j] for g in order], pa.float64()) for j, f in enumerate(V.FUNCS)}})
    got = got.take(pa.array(np.argsort(np.asarray(got.column("g")), kind="stable")))
    E.assert_exact(got, exp, ordered=True, computed=V.FUNCS)


# ------------------------------------------------------------------------------------------------------------------- join

JOIN_TYPES = ["Inner", "Left", "Right", "Full", "LeftSemi", "RightSemi", "LeftAnti", "RightAnti", "LeftMark", "RightMark"]
JOIN_SPANS = [1023, 1024, 1025, 2**34 - 1, 2**40 - 1, 2**40, 2**40 + 1, 2**64 - 1]


def _join_sides(rng, typ, span, nb=3000, npr=6000, null_frac=0.03):
    low = _span_low(typ, span)
    braw = E.span_raw(rng, nb, typ, span, low)
    lo_t, hi_t = E.type_range(typ)
    outside = [v for v in (low - 2, low - 1, low + span + 1, low + span + 2) if lo_t <= v <= hi_t]
    praw = [braw[int(i)] for i in rng.integers(0, nb, npr)]
    pick = rng.random(npr)
    for i in range(npr):
        if pick[i] < 0.15 and outside:
            praw[i] = outside[int(rng.integers(0, len(outside)))]
        elif pick[i] < 0.3:
            praw[i] = low + int(rng.random() * span)
    build = pa.table({"k": E.from_raw(braw, typ, rng.random(nb) < null_frac), "bf": E.edge_array(rng, nb, pa.float64(), 0.5),
                      "bd": E.edge_array(rng, nb, pa.decimal128(38, 0), 0.3)})
    probe = _with_rows({"k": E.from_raw(praw, typ, rng.random(npr) < null_frac), "pf": E.edge_array(rng, npr, pa.float64(), 0.5, 0.05)}, npr)
    return build, probe


def _join_all_types(build, probe, on, ne="NullEqualsNothing", d_build=None, strict=False, **build_opts):
    from datafusion_amd import _lib, ops
    from oracle import oracle
    db = _dev(build) if d_build is None else d_build
    dp = _dev(probe)
    for jt in JOIN_TYPES:
        exp = oracle.hash_join(build, probe, on, jt, ne)
        try:
            got = ops.hash_join(db, dp, on, jt, ne, **build_opts).to_arrow()
        except _lib.DfgpuError as err:
            if strict:
                raise
            # a table kind asked for by name that does not apply to these keys says so; an answer is never wrong
            assert build_opts.get("table_mode") in (2, 3, 5), err
            assert any(w in str(err) for w in ("not applicable", "pack", "not unique")), err
            return False
        E.assert_exact(got, exp, ordered=False)
    return True


@pytest.mark.parametrize("typ", [pa.int64(), pa.uint64()], ids=str)
@pytest.mark.parametrize("span", JOIN_SPANS)
@pytest.mark.parametrize("table_mode", [0, 1, 2, 3, 4, 5])
def test_join_key_spans(typ, span, table_mode):
    """build keys whose span sits on each side of the small-build threshold (1024), of the ArrayMap guard (2^34), of the rank map's
    2^40 and of the full wrapping span; probe keys just outside the build's range at both ends; all 10 join types per table kind"""
    rng = np.random.default_rng(span % 9973 + table_mode)
    build, probe = _join_sides(rng, typ, span)
    ran = _join_all_types(build, probe, [("k", "k")], table_mode=table_mode)
    if table_mode in (0, 1, 4):
        assert ran


@pytest.mark.parametrize("span, table_mode, runs", [(2**20, 2, True), (2**34, 2, False), (2**34 + 1, 2, False), (2**32, 3, True), (2**40, 3, False),
                                                    (2**40 + 1, 3, False), (2**40 - 1, 0, True), (2**40 + 1, 0, True)])
def test_join_direct_tables_at_their_range_limits(span, table_mode, runs):
    """unique Int64 build keys for the ArrayMap (table_mode 2, range < 2^34) and the rank map (table_mode 3, range < 2^40): the forced
    table builds and answers every join type inside its limit, and is refused at the limit and above it.  (The accepted spans stay
    well inside: a table one below the limit is a 64 GiB slot array or a 128 GiB bitmap.)"""
    from datafusion_amd import _lib
    rng = np.random.default_rng(span % 9973 + table_mode)
    build, probe = _join_sides(rng, pa.int64(), span, null_frac=0.0)
    keys = np.asarray(build.column("k"))
    build = build.take(pa.array(np.unique(keys, return_index=True)[1]))
    assert int(np.max(keys)) - int(np.min(keys)) == span
    if runs:
        assert _join_all_types(build, probe, [("k", "k")], table_mode=table_mode)
    else:
        with pytest.raises(_lib.DfgpuError, match="not applicable"):
            _join_all_types(build, probe, [("k", "k")], table_mode=table_mode, strict=True)


@pytest.mark.parametrize("span", [1023, 2**40 - 1, 2**64 - 1])
@pytest.mark.parametrize("probe_mode", [0, 1, 2, 3, 4])
def test_join_probe_modes(span, probe_mode):
    from datafusion_amd import ops
    from oracle import oracle
    rng = np.random.default_rng(span % 101 + probe_mode)
    build, probe = _join_sides(rng, pa.int64(), span)
    # unique build keys: the single-match probe strategies apply
    build = build.take(pa.array(np.unique(np.asarray(build.column("k").fill_null(0)), return_index=True)[1]))
    build = build.filter(build.column("k").is_valid())
    probe = probe.filter(probe.column("k").is_valid()).select(["k", "row"])     # non-nullable output columns: what the single-pass probes need
    db, dp = _dev(build), _dev(probe)
    for jt in ("Inner", "RightSemi", "RightAnti"):
        got = ops.hash_join(db, dp, [("k", "k")], jt, probe_mode=probe_mode).to_arrow()
        E.assert_exact(got, oracle.hash_join(build, probe, [("k", "k")], jt), ordered=False)


@pytest.mark.parametrize("span", [1024, 2**40 - 1, 2**40 + 1, 2**64 - 1])
@pytest.mark.parametrize("cached", ["1", "0"])
def test_join_cached_key_stats_second_build_and_slices(span, cached):
    """join.cached_key_stats: a second build over the same key column reads the statistics the first one left on it; a build over a
    slice of that column (a view of the same buffer with another range of keys) must not take them for its own"""
    from datafusion_amd import ops
    rng = np.random.default_rng(span % 977 + int(cached))
    ops.set_options(join__cached_key_stats=cached)
    build, probe = _join_sides(rng, pa.int64(), span, nb=6000, null_frac=0.0)
    order = np.argsort(np.asarray(build.column("k")), kind="stable")
    sorted_build = build.take(pa.array(order))        # ascending keys: the statistics also say so
    for b in (build, sorted_build):
        db = _dev(b)
        for _ in range(2):
            assert _join_all_types(b, probe, [("k", "k")], d_build=db)
        for off, ln in ((0, 1000), (2500, 3000), (5999, 1), (1, 5998)):
            assert _join_all_types(b.slice(off, ln), probe, [("k", "k")], d_build=db.slice(off, ln))
        assert _join_all_types(b, probe, [("k", "k")], d_build=db)


@pytest.mark.parametrize("keys", ["f64", "u64_i32", "dec38", "date_i64"])
@pytest.mark.parametrize("ne", ["NullEqualsNothing", "NullEqualsNull"])
@pytest.mark.parametrize("table_mode", [0, 1, 4, 5])
def test_join_edge_keys(keys, ne, table_mode):
    """edge values as join keys: Float64 keys equal by their bits (-0.0 and +0.0, the two NaN signs and a NaN payload are
    different keys), UInt64 above 2^63 beside Int32 extremes, Decimal128(38) beyond 64 bits, Date32 extremes with Int64 extremes"""
    types = {"f64": [pa.float64()], "u64_i32": [pa.uint64(), pa.int32()], "dec38": [pa.decimal128(38, 0)], "date_i64": [pa.date32(), pa.int64()]}[keys]
    rng = np.random.default_rng(len(keys) * 3 + table_mode + len(ne))
    nb, npr = 2500, 6000
    build = pa.table({**{f"k{i}": E.edge_array(rng, nb, t, 0.5, 0.03) for i, t in enumerate(types)}, "bf": E.edge_array(rng, nb, pa.float64(), 0.5)})
    probe = _with_rows({f"k{i}": E.edge_array(rng, npr, t, 0.5, 0.03) for i, t in enumerate(types)}, npr)
    ran = _join_all_types(build, probe, [(f"k{i}", f"k{i}") for i in range(len(types))], ne, table_mode=table_mode)
    if table_mode in (0, 1, 4):
        assert ran


# ------------------------------------------------------------------------------------------------------------------ partition

@pytest.mark.parametrize("typ", [pa.int32(), pa.int64(), pa.uint32(), pa.uint64(), pa.float64(), pa.decimal128(38, 0), pa.date32()], ids=str)
@pytest.mark.parametrize("nparts", [1, 3, 16])
@pytest.mark.parametrize("n", [65, 4097, 70_000])
def test_partition(typ, nparts, n):
    """RepartitionExec Hash over edge keys: every row in the oracle's partition (floats route by their bits: -0.0 apart from +0.0),
    in input order inside it"""
    from datafusion_amd import ops
    from oracle import oracle
    rng = np.random.default_rng(n + nparts + len(str(typ)))
    t = _with_rows({"k": E.edge_array(rng, n, typ, 0.4, 0.05), "k2": E.edge_array(rng, n, pa.int64(), 0.4, 0.05)}, n)
    for keys in (["k"], ["k", "k2"]):
        exp, _ = oracle.hash_partition(t, keys, nparts)
        got = ops.partition(_dev(t), keys, nparts)
        assert len(got) == nparts
        for g, e in zip(got, exp):
            E.assert_exact(g.to_arrow(), e, ordered=True)

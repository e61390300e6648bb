"""bit_and / bit_or / bit_xor and bool_and / bool_or of the GPU AggregateExec against tests/bitwise_ref.py, bit for bit: on every
accumulation site (the plans of tests/test_gpu_float_sums.py, whose profile name must show in ops.profile_stats()), over every
argument type with its edge values, in every mode, and through the offload rule.  The inputs are the reference's witness families
(tests/test_bitwise_reference.py shows which mistakes they catch); beside the new aggregates every site test carries COUNT(*) and SUM of
an Int64 companion column, so a row lost or counted twice shows there as well."""
import functools

import numpy as np
import pyarrow as pa
import pytest

from tests import bitwise_ref as B
from tests.test_gpu_float_sums import INTERPRETED, PARTITIONED, PLANS, SPECIALISED, _shape  # noqa: F401  (import only: the plans and their shapes)

pytestmark = pytest.mark.gpu


def _dev(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


def gpu(t, gb, aggs, mode="Single", predicate=None):
    from datafusion_amd import ops
    return ops.aggregate(_dev(t), gb, aggs, mode, predicate=predicate).to_arrow()


def _keys(names):
    from datafusion_amd.expr import col
    return [(col(k), k) for k in names]


class Spec:
    """one new aggregate of a test: output name, function, argument type, the argument's values and validity"""

    def __init__(self, name, func, typ, values, valid):
        self.name, self.func, self.typ, self.values, self.valid = name, func, typ, values, valid

    def arrow(self):
        return B.to_arrow(self.values, self.valid, self.typ)


def _family_specs(gids, null_frac, which, seed=0):
    """which: [(name, func, type)] -> Specs over the reference's family for that function and type"""
    out = []
    for name, func, typ in which:
        values, valid, _ = B.family(func, typ, gids, null_frac, seed)
        out.append(Spec(name, func, typ, values, valid))
    return out


def _want(key_rows, specs, extra=None):
    """{key tuple: (one result per spec ..., extra columns' values ...)}; extra = {name: (fn over the rows' indices of a group)}"""
    ids = {}
    gids = np.array([ids.setdefault(k, len(ids)) for k in key_rows], np.int64)
    if not ids:
        ids = {(): 0}                   # no GROUP BY over no rows: one row of NULLs
    cols = [B.reduce_groups(s.func, gids, s.values, s.valid, s.typ) for s in specs]
    rows = {k: tuple(c.get(g) for c in cols) for k, g in ids.items()}
    if extra:
        order = np.argsort(gids, kind="stable")
        bounds = np.r_[0, np.cumsum(np.bincount(gids, minlength=len(ids)))]
        for k, g in ids.items():
            idx = order[bounds[g]:bounds[g + 1]]
            rows[k] = rows[k] + tuple(fn(idx) for fn in extra.values())
    return rows


def _check(got, key_names, want, specs, extra_names=(), label=""):
    names = [s.name for s in specs] + list(extra_names)
    assert got.column_names == list(key_names) + names, (label, got.column_names)
    for s in specs:
        assert got.schema.field(s.name).type == s.typ, (label, s.name, got.schema.field(s.name).type)      # the result is of the argument's type
    keys = list(zip(*[got.column(k).to_pylist() for k in key_names])) if key_names else [()] * got.num_rows
    assert len(keys) == len(set(keys)) and set(keys) == set(want), (label, "group keys differ", len(keys), len(want))
    cols = [got.column(c).to_pylist() for c in names]
    for i, kt in enumerate(keys):
        row = tuple(c[i] for c in cols)
        assert row == want[kt], f"{label}: group {kt}: {dict(zip(names, row))}, want {dict(zip(names, want[kt]))}"


# ------------------------------------------------------------------------------ 1. known answers and NULL rules
def test_known_answers_and_null_rules():
    from datafusion_amd.expr import col
    t = pa.table({"k": pa.array([1, 1, 1, 2, 2, 3, 4], pa.int32()),
                  "i": pa.array([0b1100, 0b1010, None, 7, None, None, -1], pa.int32()),
                  "u": pa.array([0xF0, 0x3C, None, 0, None, None, 255], pa.uint8()),
                  "b": pa.array([True, False, None, True, True, None, None], pa.bool_())})
    aggs = [("bit_and", col("i"), "ia"), ("bit_or", col("i"), "io"), ("bit_xor", col("i"), "ix"), ("bit_and", col("u"), "ua"), ("bit_or", col("u"), "uo"),
            ("bit_xor", col("u"), "ux"), ("bool_and", col("b"), "ba"), ("bool_or", col("b"), "bo")]
    got = gpu(t, _keys(["k"]), aggs).sort_by("k")
    assert got.to_pydict() == {"k": [1, 2, 3, 4],
                               "ia": [0b1000, 7, None, -1], "io": [0b1110, 7, None, -1], "ix": [0b0110, 7, None, -1],
                               "ua": [0x30, 0, None, 255], "uo": [0xFC, 0, None, 255], "ux": [0xCC, 0, None, 255],
                               "ba": [False, True, None, None], "bo": [True, True, None, None]}
    assert [got.schema.field(n).type for n in ("ia", "io", "ix", "ua", "uo", "ux", "ba", "bo")] == [pa.int32()] * 3 + [pa.uint8()] * 3 + [pa.bool_()] * 2
    # without GROUP BY: one row; NULLs are skipped, not read as 0 / false
    whole = gpu(t, [], aggs)
    assert whole.to_pydict() == {"ia": [0], "io": [-1], "ix": [(0b0110 ^ 7) ^ -1], "ua": [0], "uo": [255], "ux": [0xCC ^ 255], "ba": [False], "bo": [True]}
    # ... and over no rows at all: one row of NULLs, of the arguments' types
    empty = gpu(t.slice(0, 0), [], aggs)
    assert empty.num_rows == 1 and all(v == [None] for v in empty.to_pydict().values()), empty.to_pydict()
    assert empty.schema.types == whole.schema.types


# ------------------------------------------------------------------------------ 2. every accumulation site
SITE_AGGS = [("a64", "bit_and", pa.int64()), ("o64", "bit_or", pa.int64()), ("x64", "bit_xor", pa.int64()),
             ("a32", "bit_and", pa.uint32()), ("o32", "bit_or", pa.uint32()), ("x32", "bit_xor", pa.uint32())]
BOOL_AGGS = [("ba", "bool_and", pa.bool_()), ("bo", "bool_or", pa.bool_())]


@functools.lru_cache(maxsize=4)
def _site_case(shape, n, null_frac, kind):
    """the input table of a (shape, size): the key columns, one argument column per aggregate, the Int64 companion `c` and the row number"""
    rng = np.random.default_rng([n, sum(map(ord, shape))])
    gids, keys = _shape(shape, n, rng)
    n = len(gids)
    comp = rng.integers(-2**50, 2**50, n)
    key_rows = list(zip(*[keys[k].to_pylist() for k in keys])) if keys else [()] * n
    if kind == "bits":
        specs = _family_specs(gids, null_frac, SITE_AGGS)
        cols = {s.name + "_in": s.arrow() for s in specs}
    else:
        # bool_and / bool_or over a Boolean column and over a comparison: `x < 0` of an Int64 column that is negative where the Boolean is true
        specs = _family_specs(gids, null_frac, BOOL_AGGS) + _family_specs(gids, null_frac, [("ca", "bool_and", pa.bool_()), ("co", "bool_or", pa.bool_())], seed=1)
        cols = {s.name + "_in": s.arrow() for s in specs[:2]}
        for s in specs[2:]:
            mag = rng.integers(1, 2**40, n)
            cols[s.name + "_in"] = B.to_arrow(np.where(s.values, -mag, mag - 1), s.valid, pa.int64())
    want = _want(key_rows, specs, {"rows": len, "sc": lambda idx: int(comp[idx].sum())})
    table = pa.table({**keys, **cols, "c": pa.array(comp), "row": pa.array(np.arange(n, dtype=np.int64))})
    return table, list(keys), specs, want


def _run_plan(plan, table, key_names, aggs):
    """the aggregate through the plan's path -> (result, profile_stats)"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    pred = (col("row") >= lit(0, pa.int64())) if plan.pred else None
    ops.set_options(**plan.opts)
    ops.set_fusion(plan.fusion)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        got = ops.aggregate(_dev(table), _keys(key_names), aggs, "Single", predicate=pred).to_arrow()
        return got, ops.profile_stats()
    finally:
        ops.profile_enable(False)
        ops.set_fusion(True)


SITE_CASES = sorted({(p.shape, n, nf, name) for name, p in PLANS.items() for n in p.sizes for nf in B.NULL_FRACTIONS})


@pytest.mark.parametrize("shape, n, null_frac, plan", SITE_CASES)
def test_bit_aggregates_on_every_accumulation_site(shape, n, null_frac, plan):
    """no site declines an integer argument: the plan's own site must run (with NULLs the site the plan names for them)"""
    from datafusion_amd.expr import col
    p = PLANS[plan]
    table, key_names, specs, want = _site_case(shape, n, null_frac, "bits")
    aggs = [(s.func, col(s.name + "_in"), s.name) for s in specs] + [("count", None, "rows"), ("sum", col("c"), "sc")]
    got, stats = _run_plan(p, table, key_names, aggs)
    label = f"{plan} / nulls {null_frac} / {table.num_rows} rows"
    site = p.kernel_nulls if null_frac > 0 else p.kernel
    assert site in stats, (label, "the accumulation site did not run", sorted(stats))
    for k in key_names:
        assert got.schema.field(k).type == table.schema.field(k).type, (label, k)
    _check(got, key_names, want, specs, ("rows", "sc"), label)


# A bit-packed Boolean argument has no bytes of its own that could be moved with its row, so the sites that move rows decline it,
# explicitly, and the site named here takes it: the dense node's partitioned accumulation -> the dense accumulate (dense_accumulate_partitioned),
# the fused node's partitioned accumulation -> the fused kernel's global atomics (fused_general_partitioned).  The column-at-a-time
# node's partitioned accumulation reads the rows where they lie (one LDS window of 3000 groups) and takes the Boolean column.
BOOL_SITE = {name: "agg_dense_accumulate" for name in PLANS if name.startswith("dense_partitioned")}
BOOL_SITE["two_keys_partitioned"] = "agg_fused_global"
BOOL_PROVEN = {"agg_accumulate_lds", "agg_accumulate_global", "agg_fused_lds", "agg_fused_global", "agg_fused_tile", "agg_fused_jit", "agg_runs_accumulate",
               "agg_dense_accumulate", "agg_dense_accumulate_partitioned"}
BOOL_CASES = sorted({(p.shape, 4097 if 4097 in p.sizes else p.sizes[0], nf, name) for name, p in PLANS.items() for nf in B.NULL_FRACTIONS})


def _bool_site(name, null_frac):
    p = PLANS[name]
    return p.kernel_nulls if null_frac > 0 else BOOL_SITE.get(name, p.kernel)


def test_the_boolean_cases_cover_the_sites_they_must():
    assert {_bool_site(name, nf) for _, _, nf, name in BOOL_CASES} == BOOL_PROVEN


@pytest.mark.parametrize("shape, n, null_frac, plan", BOOL_CASES)
def test_bool_aggregates_on_every_accumulation_site(shape, n, null_frac, plan):
    from datafusion_amd.expr import col, lit
    p = PLANS[plan]
    table, key_names, specs, want = _site_case(shape, n, null_frac, "bools")
    aggs = [(s.func, col(s.name + "_in"), s.name) for s in specs[:2]] + [(s.func, col(s.name + "_in") < lit(0, pa.int64()), s.name) for s in specs[2:]]
    got, stats = _run_plan(p, table, key_names, aggs + [("count", None, "rows"), ("sum", col("c"), "sc")])
    label = f"{plan} / nulls {null_frac} / {table.num_rows} rows"
    assert _bool_site(plan, null_frac) in stats, (label, "the accumulation site did not run", sorted(stats))
    _check(got, key_names, want, specs, ("rows", "sc"), label)


@pytest.mark.parametrize("groups", [1, 63, 64, 65, 4097])
def test_boolean_results_are_packed_words(groups):
    """the packed emit's last word partial, full and one past full; every third group has no value"""
    from datafusion_amd.expr import col
    rng = np.random.default_rng(groups)
    gids = rng.permutation(np.repeat(np.arange(groups), 3))
    values = rng.random(len(gids)) < 0.7
    valid = (gids % 3 != 1) & (rng.random(len(gids)) < 0.9)
    specs = [Spec("ba", "bool_and", pa.bool_(), values, valid), Spec("bo", "bool_or", pa.bool_(), ~values, valid)]
    t = pa.table({"k": pa.array(gids * 3 - 7), "ba_in": specs[0].arrow(), "bo_in": specs[1].arrow()})
    for mode in ("Single", "Partial"):
        got = gpu(t, _keys(["k"]), [(s.func, col(s.name + "_in"), s.name) for s in specs], mode)
        assert got.num_rows == groups
        _check(got, ["k"], _want([(int(k),) for k in gids * 3 - 7], specs), specs, label=f"{groups} groups, {mode}")


# ------------------------------------------------------------------------------ 3. argument types
@pytest.mark.parametrize("tname", list(B.INT_TYPES))
def test_argument_types_and_their_edge_values(tname):
    from datafusion_amd.expr import col
    typ = B.INT_TYPES[tname]
    e = B.edge_values(typ)          # 0, all ones, the sign bit alone, the largest positive
    groups = {0: e, 1: [e[1], e[2]], 2: [e[0]], 3: [e[1]], 4: [e[2], e[3]], 5: [e[2]], 6: [None, None], 7: [e[3], None, e[2], e[1]]}
    k = [g for g, vs in groups.items() for _ in vs]
    vals = [v for vs in groups.values() for v in vs]
    t = pa.table({"k": pa.array(k, pa.int32()), "v": pa.array(vals, typ)})
    valid = np.array([v is not None for v in vals])
    values = np.array([0 if v is None else v for v in vals], B.np_dtype(typ))
    specs = [Spec(f, f, typ, values, valid) for f in B.BIT_FUNCS]
    got = gpu(t, _keys(["k"]), [(f, col("v"), f) for f in B.BIT_FUNCS])
    _check(got, ["k"], _want([(g,) for g in k], specs), specs, label=tname)
    by_k = {r["k"]: r for r in got.to_pylist()}
    assert by_k[1] == {"k": 1, "bit_and": e[2], "bit_or": e[1], "bit_xor": e[3]}          # all ones and the sign bit
    assert by_k[4] == {"k": 4, "bit_and": 0, "bit_or": e[1], "bit_xor": e[1]}             # the sign bit and the largest positive
    assert by_k[5] == {"k": 5, "bit_and": e[2], "bit_or": e[2], "bit_xor": e[2]} and by_k[6] == {"k": 6, "bit_and": None, "bit_or": None, "bit_xor": None}


# ------------------------------------------------------------------------------ 4. modes
MODE_AGGS = [("a", "bit_and", pa.int64()), ("o", "bit_or", pa.uint32()), ("x", "bit_xor", pa.int32()), ("u", "bit_xor", pa.uint64()), ("m", "bit_or", pa.uint8()),
             ("ba", "bool_and", pa.bool_()), ("bo", "bool_or", pa.bool_())]
CUTS = [0, 7000, 7001, 25000]


@functools.lru_cache(maxsize=1)
def _mode_case():
    rng = np.random.default_rng(4)
    n = 40_000
    gids = rng.integers(0, 300, n)
    specs = _family_specs(gids, 0.1, MODE_AGGS)
    t = pa.table({"k": pa.array(gids.astype(np.int32)), **{s.name + "_in": s.arrow() for s in specs}})
    return t, gids, specs


def _mode_aggs(specs):
    from datafusion_amd.expr import col
    return [(s.func, col(s.name + "_in"), s.name) for s in specs]


def _partials(t, aggs):
    cuts = CUTS + [t.num_rows]
    return [gpu(t.slice(lo, hi - lo), _keys(["k"]), aggs, "Partial") for lo, hi in zip(cuts, cuts[1:])]


def test_partial_schema_is_one_state_column_of_the_arguments_type():
    t, gids, specs = _mode_case()
    parts = _partials(t, _mode_aggs(specs))
    for p in parts:
        assert [(f.name, f.type) for f in p.schema] == [("k", pa.int32())] + [(s.name, s.typ) for s in specs]
    # a partial state is the reference's result over the cut, NULL where the group saw no value
    _check(parts[1], ["k"], _want([(int(gids[7000]),)], [Spec(s.name, s.func, s.typ, s.values[7000:7001], s.valid[7000:7001]) for s in specs]), specs, label="one-row cut")


@pytest.mark.parametrize("final", ["Final", "FinalPartitioned"])
def test_partial_then_final_equals_single(final):
    t, gids, specs = _mode_case()
    aggs = _mode_aggs(specs)
    want = _want([(int(g),) for g in gids], specs)
    _check(gpu(t, _keys(["k"]), aggs), ["k"], want, specs, label="Single")
    _check(gpu(pa.concat_tables(_partials(t, aggs)), _keys(["k"]), aggs, final), ["k"], want, specs, label=final)


def test_partial_reduce_keeps_the_partial_schema_and_merges():
    t, gids, specs = _mode_case()
    aggs = _mode_aggs(specs)
    parts = _partials(t, aggs)
    reduced = gpu(pa.concat_tables(parts[:3]), _keys(["k"]), aggs, "PartialReduce")
    assert reduced.schema.remove_metadata() == parts[0].schema.remove_metadata()
    got = gpu(pa.concat_tables([reduced, parts[3]]), _keys(["k"]), aggs, "Final")
    _check(got, ["k"], _want([(int(g),) for g in gids], specs), specs, label="Partial -> PartialReduce -> Final")


def test_update_batches_and_a_real_predicate():
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    t, gids, specs = _mode_case()
    aggs = _mode_aggs(specs)
    cuts = CUTS + [t.num_rows]
    for fusion in (True, False):
        ops.set_fusion(fusion)
        try:
            a = ops.GroupedAggregate("Single", t.column_names, _keys(["k"]), aggs)
            for lo, hi in zip(cuts, cuts[1:]):
                a.update(_dev(t.slice(lo, hi - lo)))
            got = a.emit().to_arrow()
            a.free()
            _check(got, ["k"], _want([(int(g),) for g in gids], specs), specs, label=f"four batches, fusion {fusion}")
            # update_filtered: the rows the predicate drops neither make groups nor reach a cell
            keep = (gids > 10) & (gids < 250)
            pred = (col("k") > lit(10, pa.int32())).and_(col("k") < lit(250, pa.int32()))
            sub = [Spec(s.name, s.func, s.typ, s.values[keep], s.valid[keep]) for s in specs]
            _check(gpu(t, _keys(["k"]), aggs, predicate=pred), ["k"], _want([(int(g),) for g in gids[keep]], sub), specs, label=f"predicate, fusion {fusion}")
        finally:
            ops.set_fusion(True)


def test_rollup_through_grouping_sets():
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    rng = np.random.default_rng(6)
    n = 20_000
    ka, kb = rng.integers(0, 4, n), rng.integers(0, 3, n)
    gids = ka * 3 + kb
    specs = _family_specs(gids, 0.1, MODE_AGGS)
    t = pa.table({"ka": pa.array(ka.astype(np.int32)), "kb": pa.array(kb.astype(np.int32)), **{s.name + "_in": s.arrow() for s in specs}})
    groups = [[False, False], [False, True], [True, True]]
    want = {}
    for s in groups:
        gid = (2 if s[0] else 0) | (1 if s[1] else 0)
        rows = [(None if s[0] else int(a), None if s[1] else int(b), gid) for a, b in zip(ka, kb)]
        want.update(_want(rows, specs))
    got = ops.aggregate_grouping_sets(_dev(t), _keys(["ka", "kb"]), [lit(None, pa.int32()), lit(None, pa.int32())], groups, _mode_aggs(specs), "Single").to_arrow()
    _check(got, ["ka", "kb", "__grouping_id"], want, specs, label="rollup")


def test_reference_states_fed_to_a_gpu_final():
    """states made by tests/bitwise_ref.py — NULL where a part has no value for the group — merge on the device to the reference's results"""
    t, gids, specs = _mode_case()
    cuts = CUTS + [len(gids)]
    rows = {"k": []}
    for lo, hi in zip(cuts, cuts[1:]):
        states = [B.reduce_groups(s.func, gids[lo:hi], s.values[lo:hi], s.valid[lo:hi], s.typ) for s in specs]
        for g in states[0]:
            rows["k"].append(g)
            for s, st in zip(specs, states):
                rows.setdefault(s.name, []).append(st[g])
    st = pa.table({"k": pa.array(rows["k"], pa.int32()), **{s.name: pa.array(rows[s.name], s.typ) for s in specs}})
    assert any(v is None for v in rows["a"])
    got = gpu(st, _keys(["k"]), _mode_aggs(specs), "Final")
    _check(got, ["k"], _want([(int(g),) for g in gids], specs), specs, label="reference states -> Final")


# ------------------------------------------------------------------------------ 5. key types
@pytest.mark.parametrize("keys", ["two_columns", "utf8", "boolean", "null_keys"])
def test_key_types(keys):
    rng = np.random.default_rng(8)
    n = 30_000
    a, b = rng.integers(0, 9, n), rng.integers(0, 4, n)
    if keys == "two_columns":
        kc = {"ka": pa.array(a, pa.int32()), "kb": pa.array(b, pa.int64())}
        gids = a * 4 + b
    elif keys == "utf8":
        kc, gids = {"ka": pa.array([f"key-{v}" for v in a])}, a
    elif keys == "boolean":
        kc, gids = {"ka": pa.array((a % 2 == 0).tolist(), pa.bool_(), mask=a == 3)}, np.where(a == 3, 2, a % 2)
    else:
        kc, gids = {"ka": pa.array(a, pa.int64(), mask=a == 5)}, a
    specs = _family_specs(gids, 0.1, MODE_AGGS)
    t = pa.table({**kc, **{s.name + "_in": s.arrow() for s in specs}})
    names = list(kc)
    got = gpu(t, _keys(names), _mode_aggs(specs))
    _check(got, names, _want(list(zip(*[t.column(c).to_pylist() for c in names])), specs), specs, label=keys)


# ------------------------------------------------------------------------------ 6. the node's other aggregates
@pytest.mark.parametrize("with_predicate", [False, True])
@pytest.mark.parametrize("shape", ["few", "many"])
def test_other_aggregates_are_unchanged_beside_a_bit_xor(shape, with_predicate):
    from decimal import Decimal

    from datafusion_amd.expr import col, lit
    rng = np.random.default_rng(17)
    n = 60_000
    t = pa.table({"k": pa.array(rng.integers(0, 20 if shape == "few" else 4000, n), pa.int64()), "i": pa.array(rng.integers(-1000, 1000, n), pa.int64()),
                  "d": pa.array([Decimal(int(v)).scaleb(-2) for v in rng.integers(0, 10**7, n)], pa.decimal128(15, 2)),
                  "f": pa.array(rng.integers(0, 2**62, n), pa.int64(), mask=rng.random(n) < 0.1)})
    base = [("sum", col("i"), "s"), ("avg", col("d"), "a"), ("count", None, "c"), ("count", col("f"), "cf"), ("min", col("d"), "mn"), ("max", col("i"), "mx"), ("sum", col("d"), "sd")]
    pred = (col("i") > lit(-500, pa.int64())) if with_predicate else None
    plain = gpu(t, _keys(["k"]), base, predicate=pred).sort_by("k")
    withx = gpu(t, _keys(["k"]), base[:3] + [("bit_xor", col("f"), "x")] + base[3:], predicate=pred).sort_by("k")
    assert withx.drop(["x"]).equals(plain)
    keep = (np.asarray(t.column("i")) > -500) if with_predicate else np.ones(n, bool)
    f = t.column("f").combine_chunks()
    spec = Spec("x", "bit_xor", pa.int64(), f.fill_null(0).to_numpy()[keep], np.asarray(f.is_valid())[keep])
    _check(withx.select(["k", "x"]), ["k"], _want([(int(v),) for v in np.asarray(t.column("k"))[keep]], [spec]), [spec], label=shape)


# ------------------------------------------------------------------------------ 7. plan layer
def _plan_table():
    from decimal import Decimal
    rng = np.random.default_rng(15)
    n = 20_000
    gids = rng.integers(0, 200, n)
    specs = _family_specs(gids, 0.1, [("flags", "bit_or", pa.uint32())])
    q = rng.integers(1, 60, n)
    return pa.table({"k": pa.array(gids.astype(np.int32)), "flags": specs[0].arrow(), "q": pa.array(q, pa.int64()), "x": pa.array(rng.normal(size=n)),
                     "d": pa.array([Decimal(int(v)).scaleb(-2) for v in rng.integers(0, 10**5, n)], pa.decimal128(15, 2)), "b": pa.array(q % 2 == 0),
                     "i": pa.array(q.astype(np.int32))}), gids, specs[0], q


def test_offload_rule_runs_bit_or_and_bool_and_in_the_fused_node():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    t, gids, flags, q = _plan_table()
    leaf = P.MemoryExec(_dev(t), "t")
    inp = P.ProjectionExec([(col("k"), "k"), (col("flags"), "flags"), (col("q"), "q")], P.FilterExec(col("k") > lit(10, pa.int32()), leaf))
    plan = P.AggregateExec("Single", [(col("k"), "k")], [("bit_or", col("flags"), "any_flag"), ("bool_and", col("q") < lit(50, pa.int64()), "all_small"),
                                                         ("sum", col("q"), "sq")], inp)
    rule = P.GpuOffloadRule()
    opt = rule.optimize(plan)
    assert not rule.declined and isinstance(opt, P.GpuFusedAggregateExec), P.displayable(opt)
    got = P.collect(opt).to_arrow()
    assert got.schema.remove_metadata() == P.plan_schema(opt) == pa.schema([("k", pa.int32()), ("any_flag", pa.uint32()), ("all_small", pa.bool_()), ("sq", pa.int64())])
    keep = gids > 10
    specs = [Spec("any_flag", "bit_or", pa.uint32(), flags.values[keep], flags.valid[keep]), Spec("all_small", "bool_and", pa.bool_(), (q < 50)[keep], None)]
    _check(got, ["k"], _want([(int(g),) for g in gids[keep]], specs, {"sq": lambda idx: int(q[keep][idx].sum())}), specs, ("sq",), "offload rule")
    # the Partial twin's schema is the state: one column per aggregate, named like it
    part = P.AggregateExec("Partial", [(col("k"), "k")], [("bit_or", col("flags"), "any_flag"), ("bool_or", col("b"), "any_even")], leaf)
    pgot = P.collect(P.GpuOffloadRule().optimize(part)).to_arrow()
    assert pgot.schema.remove_metadata() == P.plan_schema(part) == pa.schema([("k", pa.int32()), ("any_flag", pa.uint32()), ("any_even", pa.bool_())])


@pytest.mark.parametrize("func, column, offloaded", [("bit_and", "x", False), ("bit_and", "d", False), ("bit_and", "b", False), ("bool_or", "i", False), ("min", "b", False),
                                                     ("bit_and", "i", True), ("bit_and", "flags", True), ("bool_or", "b", True)])
def test_argument_types_without_a_device_form_are_declined(func, column, offloaded):
    """(`min` over Boolean is the one case here that the parent commit passes as well: it pins that Boolean arguments enter through the
    two new functions only)"""
    from datafusion_amd import _lib, physical_plan as P
    from datafusion_amd.expr import col
    t = _plan_table()[0]
    plan = P.AggregateExec("Single", [(col("k"), "k")], [(func, col(column), "v"), ("count", None, "n")], P.MemoryExec(_dev(t), "t"))
    rule = P.GpuOffloadRule()
    out = rule.optimize(plan)
    if offloaded:
        assert not rule.declined and not getattr(out, "kept_on_cpu", False), rule.declined
        assert P.collect(out).to_arrow().schema.field("v").type == t.schema.field(column).type
        return
    assert getattr(out, "kept_on_cpu", False) and len(rule.declined) == 1 and "not supported" in rule.declined[0][1], rule.declined
    if func != "min":
        # the run-time twin of the plan-time decline: the library refuses the argument with the same words
        with pytest.raises(_lib.DfgpuError, match="is not supported on the GPU path"):
            gpu(t, _keys(["k"]), [(func, col(column), "v")])

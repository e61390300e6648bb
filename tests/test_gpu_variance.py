"""VAR / VAR_POP / STDDEV / STDDEV_POP on the GPU AggregateExec against a restatement of the reference's accumulator
(tests/variance_ref.py: Welford's update and the pairwise merge of variance.rs) and exact arithmetic: the NULL rules, accuracy on data
where the one-pass sum-of-squares formula cancels, every argument type and grouping dispatch, the Partial / Final / PartialReduce state
and grouping sets, and the plan layer."""
import math
from decimal import Decimal

import numpy as np
import pyarrow as pa
import pytest

from tests import variance_ref as V

pytestmark = pytest.mark.gpu
REL = 1e-6
FUNCS = V.FUNCS


def _aggs(arg, funcs=FUNCS):
    return [(f, arg, f) for f in funcs]


def gpu(table, group_by, aggs, mode="Single", predicate=None):
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    t = table if isinstance(table, DeviceTable) else DeviceTable.from_arrow(table)
    return ops.aggregate(t, group_by, aggs, mode, predicate=predicate).to_arrow()


def _close(got, want):
    if want is None or got is None:
        return got is None and want is None
    if math.isnan(want):
        return math.isnan(got)
    return math.isclose(got, want, rel_tol=REL, abs_tol=1e-9)


def expected(keys, xs, funcs=FUNCS, exact=False):
    """{key tuple: [value per func]} by the restatement (exact=True: exact rational arithmetic over the same Float64 inputs)"""
    groups = {}
    for k, x in zip(keys, xs):
        groups.setdefault(k, []).append(x)
    out = {}
    for k, vals in groups.items():
        if exact and not any(x is not None and not math.isfinite(x) for x in vals):
            out[k] = [V.exact_variance(vals, f) for f in funcs]
        else:
            st = V.state_of(vals)
            out[k] = [V.finish(st, f) for f in funcs]
    return out


def check(got, key_names, exp, funcs=FUNCS):
    assert got.num_rows == len(exp), (got.num_rows, len(exp))
    cols = [got.column(n).to_pylist() for n in key_names]
    vals = [got.column(f).to_pylist() for f in funcs]
    for f in funcs:
        assert got.schema.field(f).type == pa.float64()
    for r in range(got.num_rows):
        k = tuple(c[r] for c in cols)
        want = exp[k]
        for j, f in enumerate(funcs):
            assert _close(vals[j][r], want[j]), (f, k, vals[j][r], want[j])


# ------------------------------------------------------------------------------ 1. known answers
def test_known_answers_and_null_rules():
    from datafusion_amd.expr import col
    k = [1, 1, 1, 1, 2, 3, 3, 4, 4, 4]
    x = [1.0, 2.0, 3.0, 4.0, 7.0, None, None, 1.0, float("nan"), 2.0]
    got = gpu(pa.table({"k": pa.array(k, pa.int32()), "x": pa.array(x, pa.float64())}), [(col("k"), "k")], _aggs(col("x")))
    by = {r["k"]: r for r in got.to_pylist()}
    assert [by[1][f] for f in FUNCS] == [1.6666666666666667, 1.25, 1.2909944487358056, 1.118033988749895]
    assert [by[2][f] for f in FUNCS] == [None, 0.0, None, 0.0]
    assert [by[3][f] for f in FUNCS] == [None, None, None, None]
    assert all(math.isnan(by[4][f]) for f in FUNCS)


def test_no_group_by_over_empty_input_is_one_null_row():
    from datafusion_amd.expr import col
    got = gpu(pa.table({"x": pa.array([], pa.float64())}), [], _aggs(col("x")))
    assert got.num_rows == 1 and all(got.column(f).to_pylist() == [None] for f in FUNCS)


# ------------------------------------------------------------------------------ 2. accuracy
@pytest.mark.parametrize("data", ["offset_1e9", "mixed_magnitudes", "outlier_first"])
def test_accuracy_against_exact_values(data):
    from datafusion_amd.expr import col
    rng = np.random.default_rng(11)
    n, g = 20_000, 40
    k = rng.integers(0, g, n)
    if data == "offset_1e9":          # Σx² - (Σx)²/n loses every digit here
        x = 1e9 + rng.random(n)
    elif data == "mixed_magnitudes":
        x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 6, n)
    else:                              # each group's first-seen row is far from the rest
        x = rng.random(n) * 10.0
        _, first = np.unique(k, return_index=True)
        x[first] = 1e7
    got = gpu(pa.table({"k": pa.array(k, pa.int64()), "x": pa.array(x)}), [(col("k"), "k")], _aggs(col("x")))
    check(got, ["k"], expected([(int(a),) for a in k], x.tolist(), exact=True))


# ------------------------------------------------------------------------------ 3. argument types
@pytest.mark.parametrize("typ", ["float64", "int32", "int64", "decimal_cast"])
def test_argument_types(typ):
    from datafusion_amd.expr import col
    rng = np.random.default_rng(3)
    n = 5000
    k = rng.integers(0, 7, n).astype(np.int32)
    raw = rng.integers(-10**6, 10**6, n)
    mask = rng.random(n) < 0.1
    if typ == "float64":
        arr, xs, arg = pa.array(raw / 7.0, mask=mask), raw / 7.0, col("x")
    elif typ == "int32":
        arr, xs, arg = pa.array(raw.astype(np.int32), mask=mask), raw.astype(np.float64), col("x")
    elif typ == "int64":
        arr, xs, arg = pa.array(raw * 10**9, mask=mask), (raw * 10**9).astype(np.float64), col("x")
    else:                              # what the planner hands over: CAST(Decimal128(15,2) AS Float64)
        arr = pa.array([None if m else Decimal(int(v)).scaleb(-2) for v, m in zip(raw, mask)], pa.decimal128(15, 2))
        xs, arg = raw / 100.0, col("x").cast(pa.float64())
    got = gpu(pa.table({"k": pa.array(k), "x": arr}), [(col("k"), "k")], _aggs(arg))
    vals = [None if m else float(v) for v, m in zip(xs, mask)]
    check(got, ["k"], expected([(int(a),) for a in k], vals))


# ------------------------------------------------------------------------------ 4. dispatch
def _np_groups(keys, x):
    """{key: (n, m2)} by a two-pass sum in np.longdouble"""
    order = np.argsort(keys, kind="stable")
    ks, xs = keys[order], x[order].astype(np.longdouble)
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    cnt = np.diff(np.r_[starts, len(ks)])
    mean = np.add.reduceat(xs, starts) / cnt
    m2 = np.add.reduceat((xs - np.repeat(mean, cnt)) ** 2, starts)
    return ks[starts], cnt, m2


def _check_np(got, keys, x):
    uk, cnt, m2 = _np_groups(keys, x)
    g = got.sort_by("k")
    assert g.num_rows == len(uk) and np.array_equal(g.column("k").to_numpy(), uk)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = {"var": m2 / (cnt - 1), "var_pop": m2 / cnt}
    want["stddev"], want["stddev_pop"] = np.sqrt(want["var"]), np.sqrt(want["var_pop"])
    for f in FUNCS:
        col = g.column(f)
        null = ~col.is_valid().to_numpy(zero_copy_only=False)
        assert np.array_equal(null, cnt <= (1 if f in ("var", "stddev") else 0)), f
        v = col.to_numpy(zero_copy_only=False)[~null].astype(np.float64)
        w = want[f][~null].astype(np.float64)
        assert np.all(np.abs(v - w) <= REL * np.abs(w) + 1e-9), f


def test_no_group_by():
    from datafusion_amd.expr import col
    rng = np.random.default_rng(5)
    x = 1e9 + rng.random(300_000)
    got = gpu(pa.table({"x": pa.array(x)}), [], _aggs(col("x")))
    _, cnt, m2 = _np_groups(np.zeros(len(x), np.int64), x)
    assert math.isclose(got.column("var").to_pylist()[0], float(m2[0] / (cnt[0] - 1)), rel_tol=REL)
    assert math.isclose(got.column("stddev_pop").to_pylist()[0], math.sqrt(float(m2[0] / cnt[0])), rel_tol=REL)


@pytest.mark.parametrize("ngroups, n", [(3, 400_000), (50_000, 600_000)])
def test_group_counts(ngroups, n):
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    rng = np.random.default_rng(ngroups)
    keys = rng.integers(0, ngroups, n).astype(np.int64) * 3
    x = rng.normal(50.0, 20.0, n)
    ops.profile_enable(True)
    ops.profile_reset()
    got = gpu(pa.table({"k": pa.array(keys), "x": pa.array(x)}), [(col("k"), "k")], _aggs(col("x")))
    stats = ops.profile_stats()
    ops.profile_enable(False)
    assert "agg_var_m2" in stats, sorted(stats)
    _check_np(got, keys, x)


def test_millions_of_groups_take_the_partitioned_first_pass():
    """>= 2 M groups over more rows than agg.partitioned_min_rows: pass 1 moves the rows by group number, pass 2 adds in HBM"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    ops.set_options(agg__partitioned_min_rows="1000000")
    rng = np.random.default_rng(21)
    g = 2_100_000
    keys = rng.permutation(np.r_[np.arange(g), np.arange(g), rng.integers(0, g, 200_000)]).astype(np.int64) * 7 + 1
    x = rng.uniform(-100.0, 100.0, len(keys))
    ops.profile_enable(True)
    ops.profile_reset()
    got = gpu(pa.table({"k": pa.array(keys), "x": pa.array(x)}), [(col("k"), "k")], _aggs(col("x")))
    stats = ops.profile_stats()
    ops.profile_enable(False)
    assert "agg_var_m2" in stats and "agg_accumulate_lds" not in stats and "agg_accumulate_global" not in stats, sorted(stats)
    _check_np(got, keys, x)


@pytest.mark.parametrize("keys", ["two_columns", "utf8", "boolean", "null_keys"])
def test_key_types(keys):
    from datafusion_amd.expr import col
    rng = np.random.default_rng(8)
    n = 30_000
    a = rng.integers(0, 9, n)
    b = rng.integers(0, 4, n)
    x = rng.normal(0.0, 1e3, n)
    xmask = rng.random(n) < 0.05
    if keys == "two_columns":
        kc = {"a": pa.array(a, pa.int32()), "b": pa.array(b, pa.int64())}
    elif keys == "utf8":
        kc = {"a": pa.array([f"key-{v}" for v in a])}
    elif keys == "boolean":
        kc = {"a": pa.array((a % 2 == 0).tolist(), pa.bool_(), mask=a == 3)}
    else:
        kc = {"a": pa.array(a, pa.int64(), mask=a == 5)}
    t = pa.table({**kc, "x": pa.array(x, mask=xmask)})
    names = list(kc)
    got = gpu(t, [(col(c), c) for c in names], _aggs(col("x")))
    key_rows = list(zip(*[t.column(c).to_pylist() for c in names]))
    check(got, names, expected(key_rows, t.column("x").to_pylist()))


# ------------------------------------------------------------------------------ 5. modes
def _mode_table(seed=4, n=40_000):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 300, n).astype(np.int32)
    x = 1e6 + rng.normal(0.0, 3.0, n)
    return pa.table({"k": pa.array(k), "x": pa.array(x, mask=rng.random(n) < 0.02)})


def _single_rows(t):
    from datafusion_amd.expr import col
    return expected([(v,) for v in t.column("k").to_pylist()], t.column("x").to_pylist())


@pytest.mark.parametrize("final", ["Final", "FinalPartitioned"])
def test_partial_slices_then_final_equals_single(final):
    from datafusion_amd.expr import col
    t = _mode_table()
    gb, aggs = [(col("k"), "k")], _aggs(col("x"))
    cuts = [0, 7_000, 7_001, 25_000, t.num_rows]
    parts = [gpu(t.slice(a, b - a), gb, aggs, "Partial") for a, b in zip(cuts, cuts[1:])]
    out = gpu(pa.concat_tables(parts), gb, aggs, final)
    check(out, ["k"], _single_rows(t))
    check(gpu(t, gb, aggs, "Single"), ["k"], _single_rows(t))


def test_partial_reduce_then_final():
    from datafusion_amd.expr import col
    t = _mode_table(seed=6)
    gb, aggs = [(col("k"), "k")], _aggs(col("x"))
    parts = [gpu(t.slice(a, 10_000), gb, aggs, "Partial") for a in range(0, t.num_rows, 10_000)]
    reduced = gpu(pa.concat_tables(parts[:2]), gb, aggs, "PartialReduce")
    assert reduced.schema == parts[0].schema
    out = gpu(pa.concat_tables([reduced] + parts[2:]), gb, aggs, "Final")
    check(out, ["k"], _single_rows(t))


def test_rollup_grouping_sets():
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(12)
    n = 20_000
    t = pa.table({"a": pa.array(rng.integers(0, 4, n), pa.int64()), "b": pa.array(rng.integers(0, 3, n), pa.int32()),
                  "x": pa.array(rng.normal(10.0, 2.0, n))})
    groups = [[False, False], [False, True], [True, True]]
    got = ops.aggregate_grouping_sets(DeviceTable.from_arrow(t), [(col("a"), "a"), (col("b"), "b")], [lit(None, pa.int64()), lit(None, pa.int32())],
                                      groups, _aggs(col("x")), "Single").to_arrow()
    a, b, x = t.column("a").to_pylist(), t.column("b").to_pylist(), t.column("x").to_pylist()
    exp = {}
    for s in groups:
        gid = (2 if s[0] else 0) | (1 if s[1] else 0)
        keys = [(None if s[0] else p, None if s[1] else q, gid) for p, q in zip(a, b)]
        exp.update(expected(keys, x))
    check(got, ["a", "b", "__grouping_id"], exp)


def test_several_updates_equal_one_update_over_the_concatenation():
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    t = _mode_table(seed=9)
    gb, aggs = [(col("k"), "k")], _aggs(col("x"))
    a = ops.GroupedAggregate("Single", t.column_names, gb, aggs)
    for lo in range(0, t.num_rows, 9_000):
        a.update(DeviceTable.from_arrow(t.slice(lo, 9_000)))
    out = a.emit().to_arrow()
    a.free()
    check(out, ["k"], _single_rows(t))


# ------------------------------------------------------------------------------ 6. state compatibility
def test_partial_state_schema_and_python_merge():
    from datafusion_amd.expr import col
    t = _mode_table(seed=2)
    gb, aggs = [(col("k"), "k")], [("var", col("x"), "v")]
    p1, p2 = (gpu(t.slice(a, 20_000), gb, aggs, "Partial") for a in (0, 20_000))
    assert [(f.name, f.type) for f in p1.schema] == [("k", pa.int32()), ("v[count]", pa.uint64()), ("v[mean]", pa.float64()), ("v[m2]", pa.float64())]
    states = {}
    for p in (p1, p2):
        for r in p.to_pylist():
            states[r["k"]] = V.merge(states.get(r["k"], (0, 0.0, 0.0)), (r["v[count]"], r["v[mean]"], r["v[m2]"]))
    exp = _single_rows(t)
    for k, st in states.items():
        assert _close(V.finish(st, "var"), exp[(k,)][0]), k


def test_restatement_states_fed_to_gpu_final():
    from datafusion_amd.expr import col
    rng = np.random.default_rng(13)
    ks, xs, rows = [], [], []
    for part in range(4):
        for k in range(50):
            vals = [] if (k + part) % 7 == 0 else list(rng.normal(k, 1.0 + k, int(rng.integers(1, 30))))
            ks += [k] * len(vals)
            xs += vals
            rows.append((k,) + V.state_of(vals))     # count-0 rows included
    st = pa.table({"k": pa.array([r[0] for r in rows], pa.int32()), "v[count]": pa.array([r[1] for r in rows], pa.uint64()),
                   "v[mean]": pa.array([r[2] for r in rows], pa.float64()), "v[m2]": pa.array([r[3] for r in rows], pa.float64())})
    aggs = [(f, col("x"), f) for f in FUNCS]
    # one state triple per aggregate: the same states four times
    wide = st.select(["k"])
    for f in FUNCS:
        wide = wide.append_column(f"{f}[count]", st.column("v[count]")).append_column(f"{f}[mean]", st.column("v[mean]")).append_column(f"{f}[m2]", st.column("v[m2]"))
    got = gpu(wide, [(col("k"), "k")], aggs, "Final")
    check(got, ["k"], expected([(k,) for k in ks], xs))


# ------------------------------------------------------------------------------ 7. no regression of the node's other aggregates
@pytest.mark.parametrize("with_predicate", [False, True])
def test_other_aggregates_are_unchanged_beside_a_variance(with_predicate):
    """integer and decimal arguments: their sums are exact whatever the order of the atomics, so the columns must be bit-identical
    whether the node runs fused (no variance) or column-at-a-time (with one)"""
    from datafusion_amd.expr import col, lit
    rng = np.random.default_rng(17)
    n = 200_000
    t = pa.table({"k": pa.array(rng.integers(0, 20, n), pa.int64()), "i": pa.array(rng.integers(-1000, 1000, n), pa.int64()),
                  "d": pa.array([Decimal(int(v)).scaleb(-2) for v in rng.integers(0, 10**7, n)], pa.decimal128(15, 2)),
                  "x": pa.array(rng.normal(0.0, 1.0, n))})
    base = [("sum", col("i"), "s"), ("avg", col("d"), "a"), ("count", None, "c"), ("min", col("d"), "mn"), ("max", col("i"), "mx"), ("avg", col("i"), "ai")]
    pred = (col("i") > lit(-500, pa.int64())) if with_predicate else None
    gb = [(col("k"), "k")]
    plain = gpu(t, gb, base, predicate=pred).sort_by("k")
    withv = gpu(t, gb, base + [("stddev", col("x"), "sd")], predicate=pred).sort_by("k")
    assert withv.drop(["sd"]).equals(plain)
    host = t.filter(np.asarray(t.column("i")) > -500) if with_predicate else t
    exp = expected([(v,) for v in host.column("k").to_pylist()], host.column("x").to_pylist(), ["stddev"])
    for r in withv.to_pylist():
        assert _close(r["sd"], exp[(r["k"],)][0]), r


# ------------------------------------------------------------------------------ 8. plan layer
def test_offload_rule_runs_a_variance_node():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    from datafusion_amd.table import DeviceTable
    t = _mode_table(seed=15)
    leaf = P.MemoryExec(DeviceTable.from_arrow(t), "t")
    inp = P.ProjectionExec([(col("k"), "k"), (col("x"), "x")], P.FilterExec(col("k") > lit(10, pa.int32()), leaf))
    plan = P.AggregateExec("Single", [(col("k"), "k")], [("var", col("x"), "v"), ("stddev_pop", col("x"), "sp")], inp)
    rule = P.GpuOffloadRule()
    opt = rule.optimize(plan)
    assert not rule.declined and isinstance(opt, P.GpuFusedAggregateExec), P.displayable(opt)
    got = P.collect(opt).to_arrow()
    assert got.schema.remove_metadata() == P.plan_schema(opt)
    host = t.filter(np.asarray(t.column("k")) > 10)
    exp = expected([(v,) for v in host.column("k").to_pylist()], host.column("x").to_pylist(), ["var", "stddev_pop"])
    for r in got.to_pylist():
        assert _close(r["v"], exp[(r["k"],)][0]) and _close(r["sp"], exp[(r["k"],)][1]), r


def test_partial_plan_schema_is_the_state():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    t = _mode_table(seed=16)
    plan = P.AggregateExec("Partial", [(col("k"), "k")], [("var_pop", col("x"), "v")], P.MemoryExec(DeviceTable.from_arrow(t), "t"))
    got = P.collect(P.GpuOffloadRule().optimize(plan)).to_arrow()
    assert got.schema.remove_metadata() == P.plan_schema(plan)
    assert got.column_names == ["k", "v[count]", "v[mean]", "v[m2]"]


def test_variance_over_utf8_is_declined():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    t = pa.table({"g": pa.array([1, 2, 1], pa.int32()), "s": pa.array(["a", "b", "c"])})
    plan = P.AggregateExec("Single", [(col("g"), "g")], [("stddev", col("s"), "v")], P.MemoryExec(DeviceTable.from_arrow(t), "t"))
    rule = P.GpuOffloadRule()
    out = rule.optimize(plan)
    assert getattr(out, "kept_on_cpu", False) and len(rule.declined) == 1 and "not supported" in rule.declined[0][1], rule.declined


# ------------------------------------------------------------------------------ 9. size
def test_sf10_lineitem_stddev_of_the_price():
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    li = ops.tpch_lineitem(10, float_money=True)
    gb = [(col("l_returnflag"), "l_returnflag"), (col("l_linestatus"), "l_linestatus")]
    got = ops.aggregate(li, gb, [("stddev", col("l_extendedprice"), "sd")], "Single").to_arrow()
    host = li.select(["l_returnflag", "l_linestatus", "l_extendedprice"]).to_arrow()
    li.free()
    rf, ls = host.column(0).to_numpy(), host.column(1).to_numpy()
    price = host.column(2).to_numpy()
    assert got.num_rows == 4
    for r in got.to_pylist():
        x = price[(rf == r["l_returnflag"]) & (ls == r["l_linestatus"])].astype(np.longdouble)
        m = x.sum() / len(x)
        want = float(np.sqrt(((x - m) ** 2).sum() / (len(x) - 1)))
        assert math.isclose(r["sd"], want, rel_tol=REL), (r, want)

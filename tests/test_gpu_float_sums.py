"""Float64 SUM / AVG on every accumulation path of the AggregateExec against the exact sums of tests/float_sum_ref.py, inside the derived
bound gamma_m * S and nothing wider (tests/test_float_sum_reference.py shows what that bound lets through and what it does not).

A PLAN is a group-key shape plus the options that steer it onto one accumulation site; the kernel of that site must show in
ops.profile_stats(), or the test fails.  Every input family of the reference runs through every plan, without NULLs and with about
10 %.  Beside SUM(x) and AVG(x) every call carries COUNT(*), COUNT(x) and SUM of an Int64 companion column, compared bit for bit: a row
lost or counted twice shows there even where its float value is below the rounding of its group.  Group keys, NULL results (a group
without a value) and the result types are compared exactly.

m, the additions a value can pass through, is n_g - 1 + 1 for a Single aggregate and grows by one per partial state merged: three for
Partial -> Final over three cuts, four for Partial -> PartialReduce (two states) -> Final (two states), four for four update() batches."""
import functools

import numpy as np
import pyarrow as pa
import pytest

from tests import float_sum_ref as R

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 4095, 4096, 4097, 70_000]
SPECIALISED = {"jit": "1", "jit__min_rows": "0", "jit__strict": "1"}
INTERPRETED = {"jit": "0"}
PARTITIONED = {**SPECIALISED, "agg__partitioned_min_rows": "1"}


class Plan:
    """shape: the group keys (_shape); opts: ops.set_options; pred: an always-true predicate, which hands the aggregate to the fused
    FilterExec + AggregateExec node; fusion=False: column-at-a-time evaluation; kernel: the profile name of the accumulation site;
    kernel_nulls: the site that takes over when the argument has NULLs (the partitioned accumulation moves NULL-free columns only)"""

    def __init__(self, shape, opts, kernel, pred=True, fusion=True, kernel_nulls=None, sizes=(4097, 70_000)):
        self.shape, self.opts, self.kernel, self.pred, self.fusion, self.sizes = shape, opts, kernel, pred, fusion, sizes
        self.kernel_nulls = kernel_nulls or kernel


PLANS = {
    # no GROUP BY: the three evaluators of the fused node
    "scalar_specialised": Plan("none", SPECIALISED, "agg_fused_jit", sizes=ROWS),
    "scalar_interpreted": Plan("none", INTERPRETED, "agg_fused_tile", sizes=ROWS),
    "scalar_column": Plan("none", {}, "agg_accumulate_lds", fusion=False, sizes=ROWS),
    # a handful of groups under two UInt8 flag keys (Q1): LDS cells per workgroup, merged by key
    "flags_specialised": Plan("flags", SPECIALISED, "agg_fused_jit", sizes=ROWS),
    "flags_small_tile": Plan("flags", INTERPRETED, "agg_fused_tile", sizes=ROWS),
    "flags_column": Plan("flags", {}, "agg_accumulate_lds", fusion=False, sizes=ROWS),
    # a handful of groups under an Int64 key: hash interning, the interpreted fused kernel's replicated LDS cells
    "few_lds_cells": Plan("few_i64", INTERPRETED, "agg_fused_lds"),
    # an ordered key in runs: the runs node.  word-edge runs (63 .. 130 rows and one of 3000) take the plain stores, the rows of
    # the next word (`ext`) and the atomics of long runs; short runs (<= 64 rows) have no long run, so the cells are never
    # initialised and every one must be covered by a plain store
    "runs_word_edges": Plan("ordered_long", {**SPECIALISED, "agg__runs": "1"}, "agg_runs_accumulate", pred=False),
    "runs_short": Plan("ordered_short", {**SPECIALISED, "agg__runs": "1"}, "agg_runs_accumulate", pred=False),
    # the same runs through the dense-key node (segmented adds inside a wave, atomics between waves): the runs node switched off,
    # and runs whose keys are in no order
    "dense_ordered_runs": Plan("ordered_long", {**SPECIALISED, "agg__runs": "0"}, "agg_dense_accumulate", pred=False),
    "dense_clustered_runs": Plan("clustered", SPECIALISED, "agg_dense_accumulate", pred=False),
    # a dense integer key in no order: rank interning and the dense accumulate, then the partitioned one: a range of 5000 keys is
    # accumulated where the rows lie (one LDS window), 200 000 take one move into 64 windows, 1 000 000 the grouped move, which is
    # where the A/B switches act
    "dense_rank": Plan("dense", SPECIALISED, "agg_dense_accumulate", pred=False, sizes=(70_000,)),
    "dense_partitioned": Plan("dense", PARTITIONED, "agg_dense_accumulate_partitioned", pred=False, kernel_nulls="agg_dense_accumulate", sizes=(70_000,)),
    "dense_partitioned_mid": Plan("dense_mid", PARTITIONED, "agg_dense_accumulate_partitioned", pred=False, kernel_nulls="agg_dense_accumulate", sizes=(70_000,)),
    "dense_partitioned_wide": Plan("dense_wide", PARTITIONED, "agg_dense_accumulate_partitioned", pred=False, kernel_nulls="agg_dense_accumulate", sizes=(70_000,)),
    "dense_partitioned_no_grouped_move": Plan("dense_wide", {**PARTITIONED, "agg__grouped_move": "0"}, "agg_dense_accumulate_partitioned", pred=False,
                                              kernel_nulls="agg_dense_accumulate", sizes=(70_000,)),
    "dense_partitioned_no_gather_emit": Plan("dense_wide", {**PARTITIONED, "agg__gather_emit": "0"}, "agg_dense_accumulate_partitioned", pred=False,
                                             kernel_nulls="agg_dense_accumulate", sizes=(70_000,)),
    "dense_partitioned_no_records": Plan("dense_wide", {**PARTITIONED, "group__records": "0"}, "agg_dense_accumulate_partitioned", pred=False,
                                         kernel_nulls="agg_dense_accumulate", sizes=(70_000,)),
    # two key columns: hash interning, global atomics; the partitioned accumulation by group number when it is forced (it evaluates an
    # argument expression only without a predicate)
    "two_keys_global": Plan("two_keys", {}, "agg_fused_global"),
    "two_keys_column": Plan("two_keys", {}, "agg_accumulate_global", fusion=False),
    "two_keys_partitioned": Plan("two_keys", {"agg__partitioned_min_rows": "1"}, "agg_dense_accumulate_partitioned", pred=False, kernel_nulls="agg_fused_global"),
    "two_keys_column_partitioned": Plan("two_keys", {"agg__partitioned_min_rows": "1"}, "agg_dense_accumulate_partitioned", pred=False, fusion=False,
                                        kernel_nulls="agg_accumulate_global"),
}
MODE_PLANS = ["scalar_interpreted", "flags_specialised", "flags_small_tile", "few_lds_cells", "runs_word_edges", "dense_rank", "two_keys_global", "two_keys_column"]
MODES = {"PartialFinal": 3, "PartialReduce": 4, "Streaming": 4}      # mode: partial states a value's sum is merged through


def _shape(shape, n, rng):
    """(group number per row, {key column: array}): the key columns are an invertible image of the group numbers"""
    if shape == "none":
        return np.zeros(n, np.int64), {}
    if shape in ("flags", "four_flags"):
        g = rng.integers(0, 4 if shape == "four_flags" else 6, n)
        if shape == "flags" and n >= 8:
            g[n // 2] = 6                                   # a group of one row
        return g, {"k0": pa.array((g // 2).astype(np.uint8)), "k1": pa.array((g % 2).astype(np.uint8))}
    if shape == "few_i64":
        g = rng.integers(0, 5, n)
        g[n // 2] = 5
        return g, {"k": pa.array(g * 2**40 - 2**41)}
    if shape in ("ordered_long", "ordered_short", "clustered"):
        g = R.short_runs(n) if shape == "ordered_short" else R.word_edge_runs(n, long_run=3000 if n >= 20_000 else 300)
        keys = rng.permutation(int(g.max()) + 1)[g] if shape == "clustered" else g * 7 - 50_000
        return g, {"k": pa.array(keys.astype(np.int64))}
    if shape in ("dense", "dense_mid", "dense_wide"):
        g = rng.integers(0, 5000, n)
        g[:2] = (0, 4999)
        return g, {"k": pa.array((g * {"dense": 1, "dense_mid": 40, "dense_wide": 200}[shape] - 2500).astype(np.int64))}
    if shape == "two_keys":
        g = rng.integers(0, 3000, n)
        return g, {"k0": pa.array((g // 50).astype(np.int64) << 33), "k1": pa.array((g % 50 - 25).astype(np.int32))}
    if shape == "two_i32":
        g = rng.integers(0, 12, n)
        return g, {"ka": pa.array((g // 3).astype(np.int32)), "kb": pa.array((g % 3).astype(np.int32))}
    raise KeyError(shape)


@functools.lru_cache(maxsize=3)
def _case(shape, n, family, null_frac):
    """the input table of a (shape, family) and its truth: {key tuple: (GroupSum, Int64 companion sum)}"""
    rng = np.random.default_rng([n, sum(map(ord, shape))])
    gids, keys = _shape(shape, n, rng)
    n = len(gids)
    cols = R.family(family, gids, null_frac, seed=7)
    ref = R.family_reference(family, gids, cols)
    comp = rng.integers(-2**50, 2**50, n)
    uniq, inv = np.unique(gids, return_inverse=True)
    isum = np.zeros(len(uniq), np.int64)
    np.add.at(isum, inv, comp)
    first = np.zeros(len(uniq), np.int64)
    first[inv[::-1]] = np.arange(n)[::-1]
    key_rows = list(zip(*[keys[k].take(pa.array(first)).to_pylist() for k in keys])) if keys else [()]
    truth = {kt: (ref[int(g)], int(s)) for kt, g, s in zip(key_rows, uniq, isum)}
    assert len(truth) == len(uniq)
    data = {"price": R.f64_array(cols["price"], cols["valid"]), "disc": R.f64_array(cols["disc"]), "tax": R.f64_array(cols["tax"])} \
        if family == "money_expr" else {"x": R.f64_array(cols["x"], cols["valid"])}
    table = pa.table({**keys, **data, "c": pa.array(comp), "row": pa.array(np.arange(n, dtype=np.int64))})
    return table, list(keys), truth


def _aggs(family):
    from datafusion_amd.expr import col, lit
    one = lit(1.0, pa.float64())
    arg = col("price") * (one - col("disc")) * (one + col("tax")) if family == "money_expr" else col("x")
    return [("count", None, "rows"), ("count", arg, "cx"), ("sum", col("c"), "sc"), ("sum", arg, "s"), ("avg", arg, "a")]


def _dev(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


def _run(plan, table, key_names, family, mode="Single"):
    """the aggregate through the plan's path in the given mode -> (result, profile_stats)"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    gb, aggs = [(col(k), k) for k in key_names], _aggs(family)
    pred = (col("row") >= lit(0, pa.int64())) if plan.pred else None
    n = table.num_rows
    ops.set_options(**plan.opts)
    ops.set_fusion(plan.fusion)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        if mode == "Single":
            got = ops.aggregate(_dev(table), gb, aggs, "Single", predicate=pred).to_arrow()
        elif mode == "Streaming":
            cuts = [0, n // 5, n // 5 + 1, n // 2, n]
            a = ops.GroupedAggregate("Single", table.column_names, gb, aggs)
            for lo, hi in zip(cuts, cuts[1:]):
                a.update(_dev(table.slice(lo, hi - lo)), pred)
            got = a.emit().to_arrow()
            a.free()
        else:
            cuts = [0, n // 3, n // 3 + 1, n]
            parts = [ops.aggregate(_dev(table.slice(lo, hi - lo)), gb, aggs, "Partial", predicate=pred).to_arrow() for lo, hi in zip(cuts, cuts[1:])]
            if mode == "PartialReduce":
                parts = [ops.aggregate(_dev(pa.concat_tables(parts[:2])), gb, aggs, "PartialReduce").to_arrow(), parts[2]]
            got = ops.aggregate(_dev(pa.concat_tables(parts)), gb, aggs, "Final").to_arrow()
        return got, ops.profile_stats()
    finally:
        ops.profile_enable(False)
        ops.set_fusion(True)


def _check(got, table, key_names, truth, partial_states, label, record=None):
    """keys, counts, the Int64 sum and the NULLs exactly; SUM and AVG inside gamma_m * S of the exact value"""
    assert got.column_names == key_names + ["rows", "cx", "sc", "s", "a"], got.column_names
    for k in key_names:
        assert got.schema.field(k).type == table.schema.field(k).type, (label, k)
    assert [got.schema.field(c).type for c in ("rows", "cx", "sc", "s", "a")] == [pa.int64(), pa.int64(), pa.int64(), pa.float64(), pa.float64()], (label, got.schema)
    keys = list(zip(*[got.column(k).to_pylist() for k in key_names])) if key_names else [()] * got.num_rows
    assert len(keys) == len(set(keys)) and set(keys) == set(truth), (label, "group keys differ", len(keys), len(truth))
    worst = 0.0
    for kt, rows, cx, sc, s, a in zip(keys, *[got.column(c).to_pylist() for c in ("rows", "cx", "sc", "s", "a")]):
        g, isum = truth[kt]
        assert (rows, cx, sc) == (g.rows, g.n, isum), f"{label}: group {kt}: COUNT(*), COUNT(x), SUM(c) = {(rows, cx, sc)}, want {(g.rows, g.n, isum)}"
        if g.n == 0:
            assert s is None and a is None, f"{label}: group {kt} has no value: SUM {s!r}, AVG {a!r}, want NULL"
            continue
        assert s is not None and a is not None, f"{label}: group {kt} of {g.n} values: SUM {s!r}, AVG {a!r}"
        for what, value, exact, bound in (("SUM", s, g.exact, g.sum_bound(partial_states)), ("AVG", a, g.exact_avg(), g.avg_bound(partial_states))):
            r = R.ratio(value, exact, bound)
            worst = max(worst, r)
            assert R.within(value, exact, bound), (f"{label}: group {kt} ({g.n} addends, m = {g.additions(partial_states)}): {what} = {value!r}, exact {float(exact)!r}, "
                                                   f"|error| / (gamma_m S) = {r:.6g}")
    if record is not None:
        record.user_properties.append(("worst_ratio", worst))      # lands in a --junitxml report: how profiles/float_sum_bound.md was made


def _kernel(plan, null_frac):
    return plan.kernel_nulls if null_frac > 0 else plan.kernel


SINGLE_CASES = sorted({(p.shape, n, f, nf, name) for name, p in PLANS.items() for n in p.sizes for f in R.FAMILIES for nf in R.NULL_FRACTIONS})


@pytest.mark.parametrize("shape, n, family, null_frac, plan", SINGLE_CASES)
def test_single_aggregate_sums_within_the_bound(shape, n, family, null_frac, plan, request):
    p = PLANS[plan]
    table, key_names, truth = _case(shape, n, family, null_frac)
    got, stats = _run(p, table, key_names, family)
    label = f"{plan} / {family} / nulls {null_frac} / {table.num_rows} rows"
    assert _kernel(p, null_frac) in stats, (label, "the accumulation site did not run", sorted(stats))
    _check(got, table, key_names, truth, 0, label, request.node)


MODE_CASES = sorted({(PLANS[name].shape, f, nf, name, mode) for name in MODE_PLANS for mode in MODES for f in R.FAMILIES for nf in R.NULL_FRACTIONS})


@pytest.mark.parametrize("shape, family, null_frac, plan, mode", MODE_CASES)
def test_merged_states_and_batches_sum_within_the_bound(shape, family, null_frac, plan, mode, request):
    """Partial -> Final over three uneven cuts (one of them a single row), Partial -> PartialReduce -> Final, and four update() batches
    into one GroupedAggregate: the partial inputs go through the plan's path, the states merge column-at-a-time"""
    p = PLANS[plan]
    table, key_names, truth = _case(shape, 70_000, family, null_frac)
    got, stats = _run(p, table, key_names, family, mode)
    label = f"{plan} / {mode} / {family} / nulls {null_frac}"
    assert _kernel(p, null_frac) in stats, (label, "the accumulation site did not run", sorted(stats))
    if mode != "Streaming":
        assert "agg_accumulate_lds" in stats or "agg_accumulate_global" in stats, (label, "no merge of states ran", sorted(stats))
    _check(got, table, key_names, truth, MODES[mode], label, request.node)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("null_frac", R.NULL_FRACTIONS)
@pytest.mark.parametrize("with_pred", [False, True])
def test_grouping_sets_sum_within_the_bound(family, null_frac, with_pred, request):
    """ROLLUP (ka, kb): every row is an addend of three groups, one per grouping set"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    table, key_names, truth = _case("two_i32", 20_000, family, null_frac)
    n = table.num_rows
    gids = np.asarray(table.column("ka")) * 3 + np.asarray(table.column("kb"))
    cols = R.family(family, gids, null_frac, seed=7)             # the columns _case built the table from
    comp = np.asarray(table.column("c"))
    groups = [[False, False], [False, True], [True, True]]
    want = dict()
    for s in groups:
        gid = (2 if s[0] else 0) | (1 if s[1] else 0)
        level = gids if gid == 0 else gids // 3 if gid == 1 else np.zeros(n, np.int64)
        ref = R.family_reference(family, level, cols)
        for g, r in ref.items():
            kt = (None if s[0] else int(g // 3 if gid == 0 else g), None if s[1] else int(g % 3), gid)
            want[kt] = (r, int(comp[level == g].sum()))
    assert all(want[(a, b, 0)][0].exact == truth[(a, b)][0].exact for a, b in truth)
    pred = (col("row") >= lit(0, pa.int64())) if with_pred else None
    got = ops.aggregate_grouping_sets(_dev(table), [(col("ka"), "ka"), (col("kb"), "kb")], [lit(None, pa.int32()), lit(None, pa.int32())], groups, _aggs(family),
                                      "Single", predicate=pred).to_arrow()
    assert got.schema.field("__grouping_id").type == pa.uint8()
    table = table.append_column("__grouping_id", pa.array(np.zeros(n, np.uint8)))
    _check(got, table, ["ka", "kb", "__grouping_id"], want, 0, f"grouping sets / {family} / nulls {null_frac} / predicate {with_pred}", request.node)


@pytest.mark.parametrize("plan", ["flags_specialised", "flags_small_tile"])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("null_frac", R.NULL_FRACTIONS)
def test_five_million_rows_in_four_groups_sum_within_the_bound(plan, family, null_frac, request):
    """about 1.25 M addends per group: every workgroup's LDS cells merge into the same four totals; the reference is math.fsum (the
    subnormal family stays exact: its sums do not round; money_expr is held to fsum of its rounded rows)"""
    p = PLANS[plan]
    table, key_names, truth = _case("four_flags", 5_000_000, family, null_frac)
    assert all(g.n > 10**6 and (g.fsum_used or family == "subnormal") for g, _ in truth.values())
    got, stats = _run(p, table, key_names, family)
    label = f"{plan} / {family} / nulls {null_frac} / 5 M rows"
    assert p.kernel in stats, (label, sorted(stats))
    _check(got, table, key_names, truth, 0, label, request.node)

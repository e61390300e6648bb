"""Aggregates with FILTER (WHERE ...) on the GPU AggregateExec against tests/agg_filter_ref.py, value by value and without any
tolerance: integers, decimals and Booleans by equality, Float64 by bits (the inputs are integer-valued doubles whose partial sums
stay below 2^53, so every order of additions is exact).  tests/test_agg_filter_reference.py holds that reference to the oracle on
the same tables and shows which mistakes they catch.

Every function and argument type, every mode, the node predicate together with aggregate filters, and every accumulation site: a
site either honours the filter (its profile name or counter must show) or declines the node (then the test asserts the decline,
the site that took the node instead, and the same values)."""
import functools
import struct
from decimal import Decimal

import pyarrow as pa
import pytest

from tests import agg_filter_ref as R
from tests.test_agg_filter_reference import ARROW

pytestmark = pytest.mark.gpu

ARROW = dict(ARROW, f0=pa.uint8(), f1=pa.uint8(), kf=pa.int64(), kd=pa.int64(), ka=pa.int64(), kb=pa.int32(), q=pa.bool_(), w=pa.decimal128(38, 4), x=pa.float64())
SPECIALISED = {"jit": "1", "jit__min_rows": "0", "jit__strict": "1"}
INTERPRETED = {"jit": "0"}


def _dev(table, names=None):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(pa.table({c: pa.array(table[c], ARROW[c]) for c in (names or table)}))


def _e(aggs):
    """the reference's aggregates (columns by name) as the library's: (func, arg, name, filter) over Column expressions"""
    from datafusion_amd.expr import col
    return [(f, None if a is None else col(a), n, None if p is None else col(p)) for f, a, n, p in aggs]


def _keys(names):
    from datafusion_amd.expr import col
    return [(col(k), k) for k in names]


def _same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return struct.pack("<d", a) == struct.pack("<d", b)           # by bits
    return type(a) is type(b) and a == b


def _check(got, keys, aggs, want, label=""):
    """got: the device's table; want: the reference's rows.  The same groups, once each, and every value the same."""
    names = [a[2] for a in aggs]
    assert got.column_names == list(keys) + names, (label, got.column_names)
    rows = got.to_pylist()
    assert len(rows) == len(want), (label, "group count", len(rows), len(want))
    by_key = {tuple(r[k] for k in keys): r for r in rows}
    assert len(by_key) == len(rows), (label, "a group came out twice")
    for w in want:
        g = by_key.get(tuple(w[k] for k in keys))
        assert g is not None, (label, "missing group", {k: w[k] for k in keys})
        bad = {n: (g[n], w[n]) for n in names if not _same(g[n], w[n])}
        assert not bad, f"{label}: group { {k: w[k] for k in keys} }: (got, want) = {bad}"


class _options:
    """ops.set_options / set_fusion for the length of a `with`, the profile switched on; every option set is restored on the way out"""

    def __init__(self, opts=None, fusion=True):
        self.opts, self.fusion = dict(opts or {}), fusion

    def __enter__(self):
        from datafusion_amd import ops
        ops.set_options(**self.opts)
        ops.set_fusion(self.fusion)
        ops.profile_enable(True)
        ops.profile_reset()
        return ops

    def __exit__(self, *exc):
        from datafusion_amd import ops
        ops.profile_enable(False)
        ops.set_fusion(True)
        ops.set_options(**{k: None for k in self.opts})


@functools.lru_cache(maxsize=None)
def _table(n):
    return R.make_table(n)


# The aggregates of R.main_aggs() in sets one node takes (16 accumulators, an AVG is two): per argument type its five functions
# under the filter p beside COUNT(*) FILTER (the same filter: shared), COUNT(*) and SUM without one; then the bitwise and Boolean
# ones and the all-FALSE / all-TRUE filters.
def _agg_sets():
    main = R.main_aggs()
    by_name = {a[2]: a for a in main}
    shared = [by_name["cnt"], by_name["plain_cnt"], by_name["plain_sum"]]
    sets = [[a for a in main if a[1] == typ and a[3] == "p" and a[0] in ("sum", "min", "max", "count", "avg")] + shared for typ in ("i32", "i64", "f64", "dec")]
    rest = [a for a in main if not any(a in s for s in sets)]
    sets.append(rest + [by_name["plain_cnt"]])
    assert {a[2] for s in sets for a in s} == {a[2] for a in main} and all(len(s) + sum(a[0] == "avg" for a in s) <= 16 for s in sets)
    return sets


AGG_SETS = _agg_sets()


# ------------------------------------------------------------------------------ 1. every function, size and both evaluators
@pytest.mark.parametrize("path", ["column", "fused"])
@pytest.mark.parametrize("keys", [("k",), ()], ids=["group_by_k", "no_group_by"])
@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_every_function_under_a_filter(n, keys, path):
    table = _table(n)
    with _options(fusion=path == "fused") as ops:
        for aggs in AGG_SETS:
            info = {}
            got = ops.aggregate(_dev(table), _keys(keys), _e(aggs), "Single", info=info).to_arrow()
            _check(got, keys, aggs, R.aggregate(table, list(keys), aggs), f"{path}, {n} rows, {[a[2] for a in aggs][:3]}")
            if n > 0:       # (an update over no rows is nobody's)
                assert (info["fused_updates"] > 0) == (path == "fused"), (path, info)
        stats = ops.profile_stats()
    if n > 0 and path == "column":
        assert "agg_filter_validity" in stats, sorted(stats)         # the validity AND ran; no value column was rewritten
    if n > 0 and path == "fused":
        assert "agg_filter_validity" not in stats, sorted(stats)
    # the result types are the unfiltered aggregates'
    plain = ops.aggregate(_dev(table), _keys(keys), [a[:3] for a in _e(AGG_SETS[3])], "Single").to_arrow()
    assert plain.schema.remove_metadata() == ops.aggregate(_dev(table), _keys(keys), _e(AGG_SETS[3]), "Single").to_arrow().schema.remove_metadata()


def test_three_tuples_and_four_tuples_mix_and_none_is_no_filter():
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    table = _table(65)
    aggs = [("sum", col("i64"), "a"), ("sum", col("i64"), "b", None), ("sum", col("i64"), "c", col("pt")), ("sum", col("i64"), "d", col("p"))]
    got = ops.aggregate(_dev(table), _keys(["k"]), aggs, "Single").to_arrow()
    assert got.column("a") == got.column("b") == got.column("c") and got.column("a") != got.column("d")
    with pytest.raises(ValueError, match="an aggregate is"):
        ops.aggregate(_dev(table), _keys(["k"]), [("sum", col("i64"))], "Single")


def test_everything_filtered_out_without_group_by():
    from datafusion_amd import ops
    aggs = [("sum", "i64", "s", "pf"), ("count", None, "c", "pf"), ("count", "i64", "cx", "pf"), ("avg", "dec", "a", "pf"), ("min", "f64", "m", "pf"), ("bool_and", "b", "ba", "pf"),
            ("count", None, "rows", None)]
    for n in (0, 65, 4097):
        for fusion in (True, False):
            with _options(fusion=fusion):
                got = ops.aggregate(_dev(_table(n)), [], _e(aggs), "Single").to_arrow()
            assert got.to_pylist() == [{"s": None, "c": 0, "cx": 0, "a": None, "m": None, "ba": None, "rows": n}], (n, fusion)


def test_variance_and_stddev_under_a_filter():
    from datafusion_amd import ops
    t = R.variance_table()
    aggs = [("var_samp", "x", "vs", "p"), ("stddev_pop", "x", "sp", "p"), ("var_pop", "x", "vp", "p"), ("count", "x", "n", "p"), ("count", "x", "n_all", None)]
    got = ops.aggregate(_dev(t), _keys(["k"]), _e(aggs), "Single").to_arrow()
    _check(got, ["k"], aggs, R.aggregate(t, ["k"], aggs), "VAR / STDDEV")
    by_k = {r["k"]: r for r in got.to_pylist()}
    assert by_k[3]["vs"] is None and by_k[3]["vp"] == 0.0 and by_k[4]["n"] == 0 and by_k[4]["vp"] is None and by_k[2]["vs"] == 20.0 / 3.0


# ------------------------------------------------------------------------------ 2. modes
MODE_AGGS = [("sum", "dec", "sd", "p"), ("avg", "dec", "ad", "p"), ("avg", "i64", "ai", "p"), ("sum", "f64", "sf", "p"), ("min", "i32", "mn", "p"), ("max", "f64", "mx", "p"),
             ("count", None, "cnt", "p"), ("count", "i64", "cx", "p"), ("bit_xor", "u", "x", "p"), ("bool_and", "b", "ba", "p"), ("count", None, "plain_cnt", None),
             ("sum", "i64", "plain_sum", None), ("count", None, "none_cnt", "pf")]
CUTS = [0, 1300, 1301, 2600, 4097]


def _slice(table, lo, hi):
    return {c: v[lo:hi] for c, v in table.items()}


@pytest.mark.parametrize("fusion", [True, False], ids=["fused", "column"])
@pytest.mark.parametrize("mode", ["PartialFinal", "PartialReduceFinal", "Batched"])
def test_modes(mode, fusion):
    table = _table(4097)
    aggs, keys = _e(MODE_AGGS), _keys(["k"])
    want = R.aggregate(table, ["k"], MODE_AGGS)
    with _options(fusion=fusion) as ops:
        if mode == "Batched":
            # two update() calls on one handle; the second batch continues one group of the first and creates every other of its groups
            a = ops.GroupedAggregate("Single", list(table), keys, aggs)
            assert table["k"][2599] == table["k"][2600] and len(set(table["k"][2600:]) - set(table["k"][:2600])) > 10
            for lo, hi in ((0, 2600), (2600, 4097)):
                a.update(_dev(_slice(table, lo, hi)))
            got = a.emit().to_arrow()
            a.free()
        else:
            rt = ops.aggregate_return_types(_dev(table), aggs)
            parts = [ops.aggregate(_dev(_slice(table, lo, hi)), keys, aggs, "Partial").to_arrow() for lo, hi in zip(CUTS, CUTS[1:])]
            # the state schema of a filtered aggregate is the unfiltered one's
            unfiltered = ops.aggregate(_dev(_slice(table, 0, 1300)), keys, [a[:3] for a in aggs], "Partial").to_arrow()
            assert parts[0].schema.remove_metadata() == unfiltered.schema.remove_metadata()
            if mode == "PartialReduceFinal":
                reduced = ops.aggregate(_dev_arrow(pa.concat_tables(parts[:3])), keys, aggs, "PartialReduce", return_types=rt).to_arrow()
                assert reduced.schema.remove_metadata() == parts[0].schema.remove_metadata()
                parts = [reduced, parts[3]]
            # (the Final node is handed the filters too: it ignores them, like the arguments)
            got = ops.aggregate(_dev_arrow(pa.concat_tables(parts)), keys, aggs, "Final", return_types=rt).to_arrow()
    _check(got, ["k"], MODE_AGGS, want, f"{mode}, fusion {fusion}")


def _dev_arrow(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


@pytest.mark.parametrize("fusion", [True, False], ids=["fused", "column"])
def test_grouping_sets(fusion):
    from datafusion_amd.expr import lit
    table = dict(_table(4097))
    table["f0"] = [(r // 7) % 3 for r in table["row"]]
    table["f1"] = [(r // 3) % 2 for r in table["row"]]
    sets = [[False, False], [False, True]]                      # (f0, f1) and (f0)
    want = [dict(r, __grouping_id=0) for r in R.aggregate(table, ["f0", "f1"], MODE_AGGS)]                    # bit n-1-g set = column g is NULLed out
    want += [dict(r, f1=None, __grouping_id=1) for r in R.aggregate(table, ["f0"], MODE_AGGS)]
    with _options(fusion=fusion) as ops:
        got = ops.aggregate_grouping_sets(_dev(table), _keys(["f0", "f1"]), [lit(None, pa.uint8()), lit(None, pa.uint8())], sets, _e(MODE_AGGS), "Single").to_arrow()
    _check(got, ["f0", "f1", "__grouping_id"], MODE_AGGS, want, f"grouping sets, fusion {fusion}")


# ------------------------------------------------------------------------------ 3. the node predicate together with aggregate filters
@pytest.mark.parametrize("fusion", [True, False], ids=["fused", "column"])
@pytest.mark.parametrize("keys", [("k",), ()], ids=["group_by_k", "no_group_by"])
@pytest.mark.parametrize("n", [65, 4097])
def test_node_predicate_and_aggregate_filters(n, keys, fusion):
    from datafusion_amd.expr import col
    table = _table(n)
    with _options(fusion=fusion) as ops:
        info = {}
        got = ops.aggregate(_dev(table), _keys(keys), _e(MODE_AGGS), "Single", predicate=col("np_"), info=info).to_arrow()
    assert (info["fused_updates"] > 0) == fusion
    want = R.aggregate(table, list(keys), MODE_AGGS, predicate="np_")
    if n == 4097 and keys:
        assert len(want) < len(R.aggregate(table, list(keys), MODE_AGGS))               # the predicate does drop whole groups; no filter does
    _check(got, keys, MODE_AGGS, want, f"predicate + filters, {n} rows, fusion {fusion}")


# ------------------------------------------------------------------------------ 4. every accumulation site
SITE_ROWS = 20_000
# (a second, distinct filter beside p: the expression i64 > 0, whose truth the table carries in q for the reference)
SITE_AGGS = [("sum", "dec", "sd", "p"), ("avg", "i64", "ai", "p"), ("sum", "f64", "sf", "p"), ("count", None, "cnt", "p"), ("count", "i64", "cx", "p"), ("bit_xor", "u", "x", "p"),
             ("bool_or", "b", "bo", "p"), ("count", None, "plain_cnt", None), ("sum", "i64", "plain_sum", None), ("max", "dec", "q_max", "q"), ("count", None, "q_cnt", "q")]


@functools.lru_cache(maxsize=1)
def _site_table():
    import random
    t = dict(R.make_table(SITE_ROWS))
    rng = random.Random(11)
    n = SITE_ROWS
    t["f0"] = [rng.randrange(3) for _ in range(n)]                        # two UInt8 flags: the small-domain nodes
    t["f1"] = [rng.randrange(2) for _ in range(n)]
    t["kf"] = [rng.randrange(5) * 2**40 - 2**41 for _ in range(n)]        # a handful of Int64 keys: hash interning, LDS cells
    t["kd"] = [rng.randrange(5000) - 2500 for _ in range(n)]              # a dense Int64 key in no order: rank interning
    t["kd"][:2] = [-2500, 2499]
    g = [rng.randrange(3000) for _ in range(n)]                           # two keys, 3000 groups: hash interning, global cells
    t["ka"] = [(v // 50) << 33 for v in g]
    t["kb"] = [v % 50 - 25 for v in g]
    t["q"] = [None if v is None else v > 0 for v in t["i64"]]
    return t


def _site_aggs():
    from datafusion_amd.expr import col, lit
    out = []
    for f, a, name, p in SITE_AGGS:
        flt = None if p is None else (col("i64") > lit(0, pa.int64())) if p == "q" else col(p)
        out.append((f, None if a is None else col(a), name, flt))
    return out


# site: (key columns, options, fusion, the profile names that must show, the names that must NOT show, a site that declines the filter?)
PARTITIONED = {"agg__partitioned_min_rows": "1"}
SITES = {
    "column_lds": (("f0", "f1"), {}, False, ["agg_accumulate_lds", "agg_filter_validity"], [], None),
    "column_global": (("ka", "kb"), {}, False, ["agg_accumulate_global", "agg_filter_validity"], [], None),
    "tile_program": (("f0", "f1"), INTERPRETED, True, ["agg_fused_tile"], [], None),
    "specialised_small_domain": (("f0", "f1"), SPECIALISED, True, ["agg_fused_jit"], [], None),
    "specialised_no_group_by": ((), SPECIALISED, True, ["agg_fused_jit"], [], None),
    "register_program_lds": (("kf",), INTERPRETED, True, ["agg_fused_lds"], [], None),
    "register_program_global": (("ka", "kb"), {}, True, ["agg_fused_global"], [], None),
    "register_program_global_no_direct_table": (("ka", "kb"), {"agg__direct_table": "0"}, True, ["agg_fused_global"], [], None),
    "sorted_runs": (("k",), {**SPECIALISED, "agg__runs": "1"}, True, ["agg_runs_accumulate"], [], None),
    "dense_key": (("kd",), {**SPECIALISED, "agg__runs": "0"}, True, ["agg_dense_accumulate"], [], None),
    # the partitioned accumulations read argument columns as they lie, without asking a validity: they decline a filtered aggregate,
    # and the site beside them that does ask takes the node — with the same values
    "dense_partitioned_declines": (("kd",), {**SPECIALISED, **PARTITIONED}, True, ["agg_dense_accumulate"], ["agg_dense_accumulate_partitioned"], "agg_dense_accumulate_partitioned"),
    "dense_partitioned_no_grouped_move_declines": (("kd",), {**SPECIALISED, **PARTITIONED, "agg__grouped_move": "0"}, True, ["agg_dense_accumulate"],
                                                   ["agg_dense_accumulate_partitioned"], "agg_dense_accumulate_partitioned"),
    "fused_partitioned_declines": (("ka", "kb"), PARTITIONED, True, ["agg_fused_global"], ["agg_dense_accumulate_partitioned"], "agg_dense_accumulate_partitioned"),
    "column_partitioned_declines": (("ka", "kb"), PARTITIONED, False, ["agg_accumulate_global", "agg_filter_validity"], ["agg_dense_accumulate_partitioned"],
                                    "agg_dense_accumulate_partitioned"),
}


@pytest.mark.parametrize("site", list(SITES))
def test_accumulation_sites(site):
    keys, opts, fusion, must, must_not, declined = SITES[site]
    table = _site_table()
    want = R.aggregate(table, list(keys), SITE_AGGS)
    names = list(keys) + ["dec", "i64", "f64", "u", "b", "p"]
    with _options(opts, fusion) as ops:
        info = {}
        got = ops.aggregate(_dev(table, names), _keys(keys), _site_aggs(), "Single", info=info).to_arrow()
        stats = ops.profile_stats()
        compiled = ops.jit_stats()[0] + ops.jit_cache_stats()["disk_hits"]
        if declined:
            # over an argument without NULLs of its own (the partitioned accumulations take no others): the node without its filters does
            # take the site, the node with them does not — the decline is the filter's doing — and gives the reference's values
            small = [("sum", "row", "s", "p"), ("count", None, "c", "p"), ("sum", "row", "plain", None)]
            ops.profile_reset()
            ops.aggregate(_dev(table, list(keys) + ["row", "p"]), _keys(keys), [a[:3] for a in _e(small)], "Single").to_arrow()
            assert declined in ops.profile_stats(), (site, sorted(ops.profile_stats()))
            ops.profile_reset()
            got_small = ops.aggregate(_dev(table, list(keys) + ["row", "p"]), _keys(keys), _e(small), "Single").to_arrow()
            assert declined not in ops.profile_stats(), (site, sorted(ops.profile_stats()))
            _check(got_small, keys, small, R.aggregate(table, list(keys), small), site + " (declined)")
    for name in must:
        assert name in stats, (site, "did not run", name, sorted(stats))
    for name in must_not:
        assert name not in stats, (site, "ran", name, sorted(stats))
    assert (info["fused_updates"] > 0) == fusion, (site, info)
    if opts.get("jit") == "1":
        # (jit.strict: a node that does not compile is an error, not a fall-back) hiprtc compiled a node, or the code-object cache had it
        assert compiled >= 1, (site, "no node was specialised")
    _check(got, keys, SITE_AGGS, want, site)


def test_a_forest_that_does_not_fit_the_row_program_takes_the_column_path():
    """eleven input columns are one more than a row program loads: the node falls back, with the reference's values"""
    table = _table(4097)
    aggs = [("sum", "i32", "a", "p"), ("sum", "i64", "b", "p"), ("sum", "f64", "c", "p"), ("sum", "dec", "d", "p"), ("bit_xor", "u", "e", "p"), ("bool_or", "b", "f", "p"),
            ("count", None, "g", "pt"), ("count", None, "h", "pf"), ("sum", "row", "i", "np_")]
    with _options() as ops:
        info = {}
        got = ops.aggregate(_dev(table), _keys(["k"]), _e(aggs), "Single", info=info).to_arrow()
        stats = ops.profile_stats()
    assert info["fused_updates"] == 0 and "agg_filter_validity" in stats
    _check(got, ["k"], aggs, R.aggregate(table, ["k"], aggs), "too many columns")


# ------------------------------------------------------------------------------ 5. MIN / MAX over a wide Decimal128
def test_wide_max_looks_only_at_the_rows_that_survive_the_filter():
    from datafusion_amd import _lib, ops
    big = Decimal(2**70).scaleb(-4)
    table = {"k": [1, 1, 2, 2, 2, 3], "w": [Decimal("1.5000"), big, Decimal("-7.2500"), -big, Decimal("3.0000"), big], "p": [True, False, True, None, True, False]}
    aggs = [("max", "w", "mx", "p"), ("min", "w", "mn", "p"), ("count", None, "n", None)]
    got = ops.aggregate(_dev(table), _keys(["k"]), _e(aggs), "Single").to_arrow()
    assert got.schema.field("mx").type == pa.decimal128(38, 4)
    _check(got, ["k"], aggs, R.aggregate(table, ["k"], aggs), "wide MAX under a filter")
    assert {r["k"]: r["mx"] for r in got.to_pylist()} == {1: Decimal("1.5000"), 2: Decimal("3.0000"), 3: None}
    with pytest.raises(_lib.DfgpuError, match="a value does not fit in 64 bits"):
        ops.aggregate(_dev(table), _keys(["k"]), [a[:3] for a in _e(aggs)], "Single")


def test_a_filter_that_is_not_boolean_is_an_error_that_names_the_aggregate():
    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    table = _table(65)
    for fusion in (True, False):
        with _options(fusion=fusion):
            with pytest.raises(_lib.DfgpuError, match="aggregate total.*FILTER expression must be Boolean"):
                ops.aggregate(_dev(table), _keys(["k"]), [("sum", col("i64"), "total", col("i32"))], "Single")


# ------------------------------------------------------------------------------ 6. plan layer
def _plan_aggs():
    from datafusion_amd.expr import col, lit
    return ([("sum", col("v"), "s", col("flag")), ("count", None, "c", col("v") > lit(0, pa.int64())), ("avg", col("d"), "a", col("flag")), ("count", None, "n")],
            [("sum", "i64", "s", "p"), ("count", None, "c", "q"), ("avg", "dec", "a", "p"), ("count", None, "n", None)])


def test_offload_rule_offloads_a_filtered_aggregate():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    table = dict(_table(4097))
    table["q"] = [None if v is None else v > 0 for v in table["i64"]]
    leaf = P.MemoryExec(_dev(table, ["k", "i64", "dec", "p"]), "t")
    proj = P.ProjectionExec([(col("k"), "k"), (col("i64"), "v"), (col("dec"), "d"), (col("p"), "flag")], leaf)
    aggs, ref_aggs = _plan_aggs()
    plan = P.AggregateExec("Single", [(col("k"), "k")], aggs, proj)
    assert "s FILTER (WHERE" in plan.detail() and "n FILTER" not in plan.detail()                 # detail() shows the filter
    rule = P.GpuOffloadRule()
    opt = rule.optimize(plan)
    assert not rule.declined and isinstance(opt, P.GpuFusedAggregateExec), P.displayable(opt)
    # the projection's names are resolved inside the filters too
    assert "flag" not in P.displayable(opt) and "s FILTER (WHERE" in opt.detail()
    got = P.collect(opt).to_arrow()
    assert got.schema.remove_metadata() == P.plan_schema(opt)
    _check(got, ["k"], ref_aggs, R.aggregate(table, ["k"], ref_aggs), "offload rule")


def test_offload_rule_fuses_over_projection_and_filter():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    table = dict(_table(4097))
    table["q"] = [None if v is None else v > 0 for v in table["i64"]]
    leaf = P.MemoryExec(_dev(table, ["k", "i64", "dec", "p", "np_"]), "t")
    proj = P.ProjectionExec([(col("k"), "k"), (col("i64"), "v"), (col("dec"), "d"), (col("p"), "flag")], P.FilterExec(col("np_"), leaf))
    aggs, ref_aggs = _plan_aggs()
    rule = P.GpuOffloadRule()
    opt = rule.optimize(P.AggregateExec("Single", [(col("k"), "k")], aggs, proj))
    assert not rule.declined and isinstance(opt, P.GpuFusedAggregateExec) and isinstance(opt.input, P.MemoryExec), P.displayable(opt)
    _check(P.collect(opt).to_arrow(), ["k"], ref_aggs, R.aggregate(table, ["k"], ref_aggs, predicate="np_"), "fused over ProjectionExec(FilterExec)")


def test_offload_rule_keeps_a_node_with_an_int32_filter_on_the_cpu():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    leaf = P.MemoryExec(_dev(_table(65), ["k", "i64", "i32"]), "t")
    plan = P.AggregateExec("Single", [(col("k"), "k")], [("count", None, "n"), ("sum", col("i64"), "total", col("i32"))], leaf)
    rule = P.GpuOffloadRule()
    out = rule.optimize(plan)
    assert getattr(out, "kept_on_cpu", False) and len(rule.declined) == 1, rule.declined
    reason = rule.declined[0][1]
    assert "total" in reason and "not Boolean" in reason, reason


def test_plan_schema_of_a_filtered_partial_node_is_the_unfiltered_ones():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col
    leaf = P.MemoryExec(_dev(_table(65), ["k", "i64", "dec", "f64", "b", "p"]), "t")
    aggs = [("sum", col("dec"), "s", col("p")), ("avg", col("dec"), "a", col("p")), ("count", None, "c", col("p")), ("var_pop", col("f64"), "v", col("p")),
            ("bool_or", col("b"), "bo", col("p")), ("min", col("i64"), "m", col("p"))]
    for mode in ("Partial", "Single"):
        filtered = P.plan_schema(P.AggregateExec(mode, [(col("k"), "k")], aggs, leaf))
        assert filtered is not None and filtered == P.plan_schema(P.AggregateExec(mode, [(col("k"), "k")], [a[:3] for a in aggs], leaf))
    got = P.collect(P.GpuOffloadRule().optimize(P.AggregateExec("Partial", [(col("k"), "k")], aggs, leaf))).to_arrow()
    assert [f.type for f in got.schema] == [f.type for f in P.plan_schema(P.AggregateExec("Partial", [(col("k"), "k")], aggs, leaf))]


# ------------------------------------------------------------------------------ 7. the FILTER form and the CASE form
@pytest.mark.parametrize("fusion", [True, False], ids=["fused", "column"])
def test_filter_form_and_case_form_give_the_same_table(fusion):
    """a cross-check of two device paths against each other; the yardstick stays the reference"""
    from datafusion_amd.expr import case, col, lit
    table = _table(4097)
    ref_aggs = [("sum", "dec", "sd", "p"), ("min", "i64", "mn", "p"), ("avg", "f64", "af", "p"), ("count", "i32", "cx", "p"), ("count", None, "cnt", "p"), ("max", "i32", "plain", None)]
    p = col("p")
    case_aggs = [("sum", case([(p, col("dec"))]), "sd"), ("min", case([(p, col("i64"))]), "mn"), ("avg", case([(p, col("f64"))]), "af"), ("count", case([(p, col("i32"))]), "cx"),
                 ("count", case([(p, lit(1, pa.int64()))]), "cnt"), ("max", col("i32"), "plain")]
    with _options(fusion=fusion) as ops:
        a = ops.aggregate(_dev(table), _keys(["k"]), _e(ref_aggs), "Single").to_arrow()
        b = ops.aggregate(_dev(table), _keys(["k"]), case_aggs, "Single").to_arrow()
    assert a.equals(b)
    _check(a, ["k"], ref_aggs, R.aggregate(table, ["k"], ref_aggs), f"FILTER form, fusion {fusion}")

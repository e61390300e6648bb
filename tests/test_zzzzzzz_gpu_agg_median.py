"""MEDIAN(x) of the GPU AggregateExec against tests/median_ref.py: every group's value compared exactly — integers and decimals by value,
Float64 by its bits — row by row in first-seen group order.  tests/test_agg_median_reference.py holds that restatement to hand-worked
answers, to `statistics` and to numpy, and shows which mistakes its tables catch.

The one leniency: where the RESTATEMENT's result is a NaN made by the even count's addition (a NaN middle, +inf + -inf) any NaN is
taken, because which NaN an addition gives is the hardware's business.  Such rows exist only in the one test built for them; every
other test asserts that the restatement made none.

Shapes are the smallest that can still go wrong: row counts around the 64-row words and one block, every argument type at its edge
values, groups of 1 to 4 rows and an all-NULL group, run boundaries inside and across the radix passes' tiles (100 000 rows, 1 000
groups, one of them half the rows), every route of the group keys, a store that grows several times, several updates on one node, the
fused node's fallback, every refusal, and the collapsed plan."""
import functools

import pyarrow as pa
import pytest

from tests import edge_values as E
from tests import median_ref as R

pytestmark = pytest.mark.gpu

KERNELS = ("agg_median_append", "agg_median_count", "agg_median_pick", "radix_sort_pass")
ALL_AGGS = [("median", t, f"m_{t}", None) for t in R.MEDIAN_TYPES]
FILTERED = [("median", t, f"mp_{t}", "p") for t in ("i32", "u8", "f64", "dec")]
B = R.f64_bits


def _dev(table, types):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(R.to_arrow(table, types))


def _e(aggs):
    from datafusion_amd.expr import col
    return [(f, None if a is None else col(a), n, None if p is None else col(p)) for f, a, n, p in aggs]


def _keys(names):
    from datafusion_amd.expr import col
    return [(col(k), k) for k in names]


def _check(got, keys, aggs, want, types, label="", computed_nan=False):
    """got: the device's table; want: the restatement's rows.  Row by row, in first-seen group order, every value the same"""
    assert got.column_names == list(keys) + [a[2] for a in aggs], (label, got.column_names)
    assert got.num_rows == len(want), (label, "group count", got.num_rows, len(want))
    for k in keys:
        assert got.column(k).to_pylist() == [w[k] for w in want], (label, "key", k)
    made = 0
    for f, a, n, _ in aggs:
        field = got.schema.field(n)
        assert field.type == R.PA[types[a]], (label, n, field.type)                     # the argument's type
        values = R.raw_column(got.column(n), types[a])
        for i, (g, w) in enumerate(zip(values, want)):
            made += w[n] is R.COMPUTED_NAN
            shown = (hex(g) if isinstance(g, int) and types[a] == "f64" else g, hex(w[n]) if isinstance(w[n], int) and types[a] == "f64" else w[n])
            assert R.same(g, w[n]), f"{label}: column {n}, group {i}: (got, want) = {shown}"
    assert (made > 0) == computed_nan, (label, "NaNs made by an addition in the restatement", made)


class _profiled:
    """options for the length of a `with`, the profile switched on and reset; everything restored on the way out"""

    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        from datafusion_amd import ops
        ops.set_options(**self.opts)
        ops.profile_enable(True)
        ops.profile_reset()
        return ops

    def __exit__(self, *exc):
        from datafusion_amd import ops
        ops.profile_enable(False)
        ops.set_options(**{k: None for k in self.opts})


def _ran(stats, *names):
    for n in names:
        assert n in stats and stats[n]["calls"] > 0, (n, sorted(stats))


@functools.lru_cache(maxsize=None)
def _table(n):
    return R.make_table(n)


def _stored(table, aggs):
    """the rows each aggregate's store holds"""
    return [sum(v is not None and R.passes(table, p, i) for i, v in enumerate(table[a])) for _, a, _, p in aggs]


def _run(table, types, keys, aggs, label, computed_nan=False, **opts):
    with _profiled(**opts) as ops:
        info = {}
        got = ops.aggregate(_dev(table, types), _keys(keys), _e(aggs), "Single", info=info).to_arrow()
        stats = ops.profile_stats()
    _check(got, keys, aggs, R.aggregate(table, list(keys), aggs, types), types, label, computed_nan)
    assert info["fused_updates"] == 0, (label, info)                                    # the fused update declines the node
    most = max(_stored(table, aggs))
    if most > 0:                                                                        # every case that stores a value: the kernels ran
        _ran(stats, "agg_median_append", "agg_median_count", "agg_median_pick")
    if most > 1:
        _ran(stats, "radix_sort_pass")
    if most > 0 and keys and got.num_rows > 1:
        _ran(stats, "agg_median_gid_keys")
    return stats


# ------------------------------------------------------------------------------ 1. every type, the row counts, with and without GROUP BY
@pytest.mark.parametrize("keys", [("k",), ()], ids=["group_by_k", "no_group_by"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4097])
def test_every_argument_type_at_its_edge_values(n, keys):
    table = _table(n)
    _run(table, R.TYPES, keys, ALL_AGGS, f"{n} rows, all types")
    _run(table, R.TYPES, keys, FILTERED, f"{n} rows, filtered")
    if n == 4097 and keys:
        sizes = sorted({len(rows) for _, rows in R.groups_of(table, ["k"])})
        assert sizes[:4] == [1, 2, 3, 4]
        want = R.aggregate(table, ["k"], ALL_AGGS, R.TYPES)
        assert any(all(w[a[2]] is None for a in ALL_AGGS) for w in want)                # the all-NULL group


# ------------------------------------------------------------------------------ 2. the wrap cases of the contract, and the NaNs an addition makes
WRAPS = {"i32": ([2**31 - 1, 2**31 - 1], -1), "u8": ([200, 200], 72), "i64": ([-3, 0], -1), "u32": ([2**32 - 1, 2**32 - 1], 2**31 - 1), "u64": ([2**64 - 1, 1], 0),
         "dec": ([10**38 - 1, 10**38 - 1], 10**38 - 1 - 2**127), "f64": ([B(1e308), B(1e308)], B(float("inf")))}


@pytest.mark.parametrize("t", sorted(WRAPS))
def test_the_sum_wraps_at_the_types_width_and_the_division_truncates(t):
    pair, answer = WRAPS[t]
    # group 1: the pair; group 2: the pair and a NULL between; group 3: the pair's first value alone; and the same without GROUP BY over the pair
    table = {"k": [1, 1, 2, 2, 2, 3], "x": pair + [pair[0], None, pair[1]] + [pair[0]]}
    types = {"k": "i64", "x": t}
    want = R.aggregate(table, ["k"], [("median", "x", "m", None)], types)
    assert [w["m"] for w in want] == [answer, answer, pair[0]]
    _run(table, types, ("k",), [("median", "x", "m", None)], f"wrap {t}")
    _run({"x": pair}, {"x": t}, (), [("median", "x", "m", None)], f"wrap {t}, no GROUP BY")
    if t in ("i32", "i64", "dec"):                                                      # truncation toward zero on every signed type
        neg = {"k": [1, 1, 2, 2], "x": [-3, 0, -1, 0]}
        assert [w["m"] for w in R.aggregate(neg, ["k"], [("median", "x", "m", None)], types)] == [-1, 0]
        _run(neg, types, ("k",), [("median", "x", "m", None)], f"truncation {t}")


def test_float64_total_order_bits_and_the_nans_an_addition_makes():
    inf, nz, pz = B(float("inf")), B(-0.0), B(0.0)
    groups = [[pz, nz, pz], [nz, nz, pz], [E.PAYLOAD_NAN_BITS], [B(1.0), E.QNAN_BITS, E.PAYLOAD_NAN_BITS], [E.NEG_QNAN_BITS, B(-5.0), B(7.0)], [nz, pz], [nz, nz],
              [B(5e-324), B(5e-324)], [B(5e-324), pz], [B(1e308), B(1e308)], [B(-1e308), B(-1e308)], [E.NEG_QNAN_BITS, E.QNAN_BITS, nz, pz, B(-float("inf")), inf, B(3.0)]]
    table = {"k": [g for g, vs in enumerate(groups) for _ in vs], "x": [v for vs in groups for v in vs]}
    types = {"k": "i64", "x": "f64"}
    aggs = [("median", "x", "m", None)]
    want = [w["m"] for w in R.aggregate(table, ["k"], aggs, types)]
    assert want == [pz, nz, E.PAYLOAD_NAN_BITS, E.QNAN_BITS, B(-5.0), pz, nz, B(5e-324), pz, inf, B(-float("inf")), pz]
    _run(table, types, ("k",), aggs, "total order")
    # the one case with NaNs made by the addition: any NaN is taken there, everything else stays exact
    made = [[inf, B(-float("inf"))], [B(1.0), E.QNAN_BITS], [E.QNAN_BITS, E.PAYLOAD_NAN_BITS], [E.NEG_QNAN_BITS, E.NEG_QNAN_BITS, B(2.0), B(4.0)], [B(2.0), B(4.0)]]
    table = {"k": [g for g, vs in enumerate(made) for _ in vs], "x": [v for vs in made for v in vs]}
    want = [w["m"] for w in R.aggregate(table, ["k"], aggs, types)]
    assert want == [R.COMPUTED_NAN] * 4 + [B(3.0)]
    _run(table, types, ("k",), aggs, "NaNs made by the addition", computed_nan=True)


# ------------------------------------------------------------------------------ 3. 100 000 rows, 1 000 groups
@functools.lru_cache(maxsize=None)
def _skewed():
    """group 0 holds half the rows, groups 1..300 one row each, the rest is spread over groups 301..999; `dup`: 16 different values,
    `uniq` / `fu`: all different (Int64 / Float64)"""
    n = 100_000
    k = [0] * n
    odd = [i for i in range(n) if i % 2]
    for g, i in enumerate(odd[:300], start=1):
        k[i] = g
    for j, i in enumerate(odd[300:]):
        k[i] = 301 + (j * 7919) % 699
    table = {"k": [g * 1000003 - 5 for g in k],
             "dup": [None if i % 11 == 0 else (i * 2654435761) % 16 - 8 for i in range(n)],
             "uniq": [(i * 2654435761) % 2**40 * 2**20 + i - 2**59 for i in range(n)],
             "fu": [None if i % 13 == 0 else B(((i * 2654435761) % 2**32 - 2**31) / 64.0 + i * 2.0**-20) for i in range(n)]}
    return table


def test_a_hundred_thousand_rows_a_thousand_groups():
    table = _skewed()
    types = {"k": "i64", "dup": "i64", "uniq": "i64", "fu": "f64"}
    sizes = sorted(len(rows) for _, rows in R.groups_of(table, ["k"]))
    assert len(sizes) == 1000 and sizes[-1] == 50_000 and sizes.count(1) == 300
    assert len({v for v in table["dup"] if v is not None}) == 16 and len(set(table["uniq"])) == 100_000
    aggs = [("median", "dup", "md", None), ("median", "uniq", "mu", None), ("median", "fu", "mf", None)]
    _run(table, types, ("k",), aggs, "100000 rows, 1000 groups")
    _run(table, types, (), aggs, "100000 rows, no GROUP BY")


# ------------------------------------------------------------------------------ 4. the group keys' routes
def _key_table(n):
    t = dict(R.make_table(n))
    t["kd"] = [i * 3 % 11 for i in range(n)]                                        # dense Int32: the direct route of lookup_gid
    t["ks"] = [None if i % 13 == 0 else f"key-{i * 5 % 9}" for i in range(n)]       # strings
    t["kb"] = [None if i % 17 == 0 else i % 3 == 0 for i in range(n)]               # Boolean
    return t


KEY_TYPES = dict(R.TYPES, kd="i32", ks="str", kb="bool")


@pytest.mark.parametrize("keys", [("kd",), ("k",), ("k", "k2"), ("k2",), ("ks",), ("dict:ks",), ("kb",), ("kb", "ks")], ids=lambda k: "+".join(k).replace(":", "_"))
def test_group_key_routes(keys):
    from datafusion_amd.table import DeviceTable
    table = _key_table(4097)
    encode = keys[0].startswith("dict:")
    keys = tuple(k.split(":")[-1] for k in keys)
    aggs = [("median", "i64", "a", None), ("median", "f64", "b", "p"), ("median", "dec", "c", None), ("median", "u8", "d", None)]
    arrow = R.to_arrow(table, KEY_TYPES)
    if encode:                                                                       # a dictionary-encoded string key
        arrow = arrow.set_column(arrow.schema.get_field_index("ks"), "ks", arrow.column("ks").combine_chunks().dictionary_encode())
    with _profiled() as ops:
        got = ops.aggregate(DeviceTable.from_arrow(arrow), _keys(keys), _e(aggs), "Single").to_arrow()
        _ran(ops.profile_stats(), *KERNELS, "agg_median_gid_keys")
    if encode:
        got = got.set_column(0, "ks", got.column("ks").cast(pa.string()))
    _check(got, keys, aggs, R.aggregate(table, list(keys), aggs, KEY_TYPES), KEY_TYPES, f"keys {keys}")


# ------------------------------------------------------------------------------ 5. several updates, growth
def test_three_updates_equal_one_update_over_the_concatenation():
    from datafusion_amd import ops
    base = _table(4097)
    cuts = [(0, 0), (0, 1500), (1500, 1563), (1563, 4097)]                             # a first batch of zero rows
    parts = [{c: v[a:b] for c, v in base.items()} for a, b in cuts]
    nulls = {c: (v[:65] if c in ("k", "k2", "p") else [None] * 65) for c, v in base.items()}   # and a first batch that is all NULL
    for label, batches in (("empty first", parts), ("all-NULL first", [nulls] + parts[1:])):
        whole = R.concat(batches)
        for keys in (("k",), ()):
            with _profiled() as o:
                a = ops.GroupedAggregate("Single", list(base), _keys(keys), _e(ALL_AGGS + FILTERED))
                for part in batches:
                    a.update(_dev(part, R.TYPES))
                got = a.emit().to_arrow()
                again = a.emit().to_arrow()                                             # emitting is repeatable: the cells are made from the store each time
                a.free()
                _ran(o.profile_stats(), *KERNELS)
                once = o.aggregate(_dev(whole, R.TYPES), _keys(keys), _e(ALL_AGGS + FILTERED), "Single").to_arrow()
            _check(got, keys, ALL_AGGS + FILTERED, R.aggregate(whole, list(keys), ALL_AGGS + FILTERED, R.TYPES), R.TYPES, f"{label}, keys {keys}")
            assert again.equals(got) and once.equals(got), (label, keys)
    # the argument's type is held between updates
    a = ops.GroupedAggregate("Single", ["k", "x"], _keys(["k"]), _e([("median", "x", "m", None)]))
    a.update(_dev({"k": [1, 2], "x": [1, 2]}, {"k": "i64", "x": "i64"}))
    with pytest.raises(Exception, match="aggregate m: the argument's type changed between updates"):
        a.update(_dev({"k": [1, 2], "x": [1, 2]}, {"k": "i64", "x": "i32"}))
    a.free()


def test_a_small_store_grows_several_times_and_nothing_changes():
    from datafusion_amd import ops
    n = 10_000
    table = {"k": [i % 5 for i in range(n)], "i64": [None if i % 9 == 0 else (i * 7919) % 10007 - 5000 for i in range(n)]}
    table["dec"] = [None if v is None else v * (2**64 + 1) for v in table["i64"]]      # both words carry the value
    types = {"k": "i64", "i64": "i64", "dec": "dec"}
    aggs = [("median", "i64", "a", None), ("median", "dec", "b", None)]
    want = R.aggregate(table, ["k"], aggs, types)
    parts = [{c: v[a:a + 1000] for c, v in table.items()} for a in range(0, n, 1000)]
    outs = []
    for opts in (dict(agg__median_rows=64), dict()):
        with _profiled(**opts) as o:
            a = ops.GroupedAggregate("Single", list(table), _keys(["k"]), _e(aggs))
            for p in parts:
                a.update(_dev(p, types))
            outs.append(a.emit().to_arrow())
            a.free()
            _ran(o.profile_stats(), *KERNELS)
        _check(outs[-1], ("k",), aggs, want, types, f"grown {opts}")
    assert outs[0].equals(outs[1])
    _run(table, types, ("k",), aggs, "64 rows to start with, one update", agg__median_rows=64)


# ------------------------------------------------------------------------------ 6. beside the other aggregates, and under the fused node
def _mixed_table(n):
    t = dict(_table(n))
    t["a"] = [None if i % 10 == 0 else (i * 31) % 1000 - 500 for i in range(n)]
    t["u"] = [None if i % 7 == 0 else (i * 17) % 100 for i in range(n)]
    t["au"] = [None if a is None or u is None else a + u for a, u in zip(t["a"], t["u"])]
    return t


MIXED_TYPES = dict(R.TYPES, a="i64", u="i64", au="i64")


def test_one_node_with_plain_distinct_and_median_aggregates():
    from datafusion_amd.expr import col
    table = _mixed_table(4097)
    plain = [("sum", col("a"), "s"), ("avg", col("i32"), "avg"), ("count_distinct", col("u"), "cd")]     # (exact in any order: compared by value below)
    types = MIXED_TYPES
    medians = [("median", "a", "m1", None), ("median", "a", "m2", None), ("median", "a", "mp", "p"), ("median", "au", "me", None)]
    lowered = _e(medians[:3]) + [("median", col("a") + col("u"), "me", None)]
    for keys in (("k",), ()):
        with _profiled() as o:
            both = o.aggregate(_dev(table, types), _keys(keys), plain + lowered, "Single").to_arrow()
            stats = o.profile_stats()
            alone = o.aggregate(_dev(table, types), _keys(keys), plain, "Single").to_arrow()
        _ran(stats, *KERNELS)
        assert stats["agg_median_append"]["calls"] == 3, stats["agg_median_append"]     # m1 and m2 share one store; the filter and the expression have their own
        assert stats["agg_median_pick"]["calls"] == 3, stats["agg_median_pick"]         # and are sorted once
        for c in list(keys) + [p[2] for p in plain]:
            assert both.column(c).equals(alone.column(c)) and both.schema.field(c) == alone.schema.field(c), c
        _check(both.select(list(keys) + [m[2] for m in medians]), keys, medians, R.aggregate(table, list(keys), medians, types), types, "mixed node")
        assert both.column("m1").equals(both.column("m2"))


def test_the_fused_node_with_a_predicate_falls_back():
    from datafusion_amd.expr import col, lit
    table = _table(4097)
    kept = [i for i, v in enumerate(table["i32"]) if v is not None and v > 0]
    filtered = {c: [v[i] for i in kept] for c, v in table.items()}
    assert 0 < len(kept) < 4097
    aggs = [("median", "i64", "a", None), ("median", "dec", "b", "p"), ("median", "f64", "c", None)]
    for keys in (("k",), ()):
        with _profiled() as o:
            info = {}
            got = o.aggregate(_dev(table, R.TYPES), _keys(keys), _e(aggs), "Single", predicate=col("i32") > lit(0, pa.int32()), info=info).to_arrow()
            _ran(o.profile_stats(), *KERNELS)
        assert info["fused_updates"] == 0
        _check(got, keys, aggs, R.aggregate(filtered, list(keys), aggs, R.TYPES), R.TYPES, "fused node")


# ------------------------------------------------------------------------------ 7. refusals, in the library's words, and the rule
def test_every_refusal_by_its_message_and_the_rule_keeps_the_plan_on_the_cpu():
    from datafusion_amd import _lib, ops, physical_plan as P
    from datafusion_amd.expr import col, lit
    from datafusion_amd.table import DeviceTable
    table = dict(_table(65))
    table["d32"] = [None if v is None else v % 1000 for v in table["i64"]]
    table["s"] = [None if v is None else f"s{v % 5}" for v in table["i64"]]
    types = dict(R.TYPES, d32="d32", s="str")
    arrow = R.to_arrow(table, types)
    arrow = arrow.append_column("ds", arrow.column("s").combine_chunks().dictionary_encode())
    dev = DeviceTable.from_arrow(arrow)
    leaf = P.MemoryExec(dev, "t")
    cases = [("Single", ("median", col("d32"), "x"), "MEDIAN over Date32 is not supported on the GPU path"),
             ("Single", ("median", col("p"), "x"), "MEDIAN over Boolean is not supported on the GPU path"),
             ("SinglePartitioned", ("median", col("s"), "x"), "MEDIAN over Utf8 is not supported on the GPU path"),
             ("Single", ("median", col("ds"), "x"), "MEDIAN over Utf8 is not supported on the GPU path"),
             ("Single", ("median", None, "x"), "MEDIAN (aggregate x) needs an argument")]
    for mode in ("Partial", "Final", "FinalPartitioned", "PartialReduce"):
        cases.append((mode, ("median", col("i64"), "x"), f"MEDIAN (aggregate x) is not supported in mode {mode} on the GPU path: its partial state is a List column"))
        cases.append((mode, ("median", col("f64"), "x", col("p")), f"MEDIAN (aggregate x) is not supported in mode {mode} on the GPU path: its partial state is a List column"))
    for mode, agg, message in cases:
        with pytest.raises(_lib.DfgpuError) as err:
            ops.aggregate(dev, _keys(["k"]), [("count", None, "n"), agg], mode)
        assert message in str(err.value), (mode, agg, str(err.value))
        rule = P.GpuOffloadRule(world_size=2)                                # (two ranks: nothing is collapsed, every node is asked by itself)
        out = rule.optimize(P.AggregateExec(mode, _keys(["k"]), [("count", None, "n"), agg], leaf))
        assert type(out) is P.AggregateExec and getattr(out, "kept_on_cpu", False) and rule.declined == [(out, message)], (mode, agg, rule.declined)
    # on one rank a Single node is asked the same way, and a staged pair over a refused type stays as it was
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.AggregateExec("Single", _keys(["k"]), [cases[0][1]], leaf))
    assert getattr(out, "kept_on_cpu", False) and rule.declined == [(out, cases[0][2])]
    partial = P.AggregateExec("Partial", _keys(["k"]), [("median", col("d32"), "m")], leaf)
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.AggregateExec("FinalPartitioned", _keys(["k"]), [("median", col("m"), "m")], P.RepartitionExec(partial, ["k"], 4)))
    below = P._partial_below(out.input)
    assert out.mode == "FinalPartitioned" and getattr(out, "kept_on_cpu", False) and below.mode == "Partial" and getattr(below, "kept_on_cpu", False)
    assert rule.declined[0] == (out, "MEDIAN over Date32 is not supported on the GPU path")
    # grouping sets
    with pytest.raises(_lib.DfgpuError, match=r"grouping sets: MEDIAN \(aggregate x\) is not supported on the GPU path"):
        ops.aggregate_grouping_sets(dev, _keys(["k", "k2"]), [lit(None, pa.int64()), lit(None, pa.int32())], [[False, False], [False, True]], [("median", col("i64"), "x")])
    # the plan layer types the column as the argument's type, nullable
    schema = P.plan_schema(P.AggregateExec("Single", _keys(["k"]), [("median", col("f64"), "mw"), ("median", col("dec"), "mm"), ("median", col("u8"), "mb")], leaf))
    assert [(f.name, f.type, f.nullable) for f in schema][1:] == [("mw", pa.float64(), True), ("mm", R.PA["dec"], True), ("mb", pa.uint8(), True)]
    # and the node beside them is untouched: the accepted spelling still runs
    _run(table, types, ("k",), [("median", "i64", "c", None)], "after the refusals")


# ------------------------------------------------------------------------------ 8. the collapsed plan
def test_the_collapsed_plan_runs_through_collect():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    table = _table(4097)
    leaf = P.MemoryExec(_dev(table, R.TYPES), "t")
    proj = P.ProjectionExec([(col("k"), "k"), (col("f64"), "v"), (col("i32"), "w"), (col("u32"), "u"), (col("p"), "p")], P.FilterExec(col("i32") > lit(0, pa.int32()), leaf))
    aggs = [("median", col("v"), "med"), ("stddev", col("w"), "sd"), ("median", col("u"), "mu", col("p"))]
    partial = P.AggregateExec("Partial", [(col("k"), "k")], aggs, proj)
    final = P.AggregateExec("FinalPartitioned", [(col("k"), "k")], [(a[0], col(a[2]), a[2]) for a in aggs], P.CoalesceBatchesExec(P.RepartitionExec(partial, ["k"], 4)))
    rule = P.GpuOffloadRule()
    plan = rule.optimize(final)
    assert type(plan) is P.GpuFusedAggregateExec and plan.mode == "Single" and not rule.declined
    assert "aggr=[med, sd, mu FILTER (WHERE p@None)]" in P.displayable(plan).split("\n")[0]
    with _profiled() as o:
        got = P.collect(plan).to_arrow()
        _ran(o.profile_stats(), *KERNELS)
    kept = [i for i, v in enumerate(table["i32"]) if v is not None and v > 0]
    filtered = {c: [v[i] for i in kept] for c, v in table.items()}
    medians = [("median", "f64", "med", None), ("median", "u32", "mu", "p")]
    assert got.column_names == ["k", "med", "sd", "mu"]
    _check(got.select(["k", "med", "mu"]), ("k",), medians, R.aggregate(filtered, ["k"], medians, R.TYPES), R.TYPES, "collapsed plan")
    plain = P.collect(P.GpuOffloadRule().optimize(P.AggregateExec("Single", [(col("k"), "k")], aggs[1:2], proj))).to_arrow()
    # (STDDEV adds Float64 with atomics, in an order that differs from run to run: the suite's tolerance for computed floats)
    assert got.column("k").equals(plain.column("k"))
    for x, y in zip(got.column("sd").to_pylist(), plain.column("sd").to_pylist()):
        assert (x is None and y is None) or (x is not None and y is not None and x == pytest.approx(y, rel=E.REL)), (x, y)

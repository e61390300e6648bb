"""The GPU WindowAggExec (dfgpu_window) against tests/window_ref.py, value by value: every function, frame and argument type over
partitions that straddle the 64-row words and the scan's tile (T = ops.WINDOW_TILE rows per workgroup), NULL and dictionary and
Decimal128 keys, the Float64 families of tests/float_sum_ref.py, a plan through GpuOffloadRule, and the refusals.

Integers, decimals, dates, counts and ranks are compared exactly, Float64 MIN / MAX by their bits.  A Float64 SUM must lie within
gamma_(m-1) * S of the exact rational sum of its frame (m non-NULL values, S the sum of their magnitudes: any tree of m - 1 double
additions stays inside, Higham §4.2; joining an identity 0.0 is exact) — tests/float_sum_ref.py's gamma / within, no tolerance beside
it.  AVG = sum / m adds the rounding of one division: u * |avg|, or 2^-1075 where the quotient is subnormal.  money_expr's argument is
an expression of k = 4 float operations evaluated per row first: (gamma_k + gamma_(m-1) (1 + gamma_k)) * S, float_sum_ref's rule.
Every case asserts the `window_` kernels it must have run (ops.profile_stats())."""
import ctypes as C
import functools
import struct
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from tests import float_sum_ref as R
from tests import window_cases as WC
from tests import window_ref as W

pytestmark = pytest.mark.gpu

RANKS = [("row_number", None, "rn", None), ("rank", None, "rk", None), ("dense_rank", None, "dr", None)]
SCAN_OF = {("sum", "int32"): "add_u64", ("sum", "int64"): "add_u64", ("sum", "float64"): "add_f64", ("sum", "decimal"): "add_i128",
           ("avg", "int32"): "add_f64", ("avg", "int64"): "add_f64", ("avg", "float64"): "add_f64", ("avg", "decimal"): "add_i128",
           ("min", "decimal"): "min_i128", ("max", "decimal"): "max_i128"}


def _scan_name(func, tag):
    if func == "count":
        return "window_scan_count"
    t = "decimal" if isinstance(tag, tuple) else tag
    return "window_scan_" + SCAN_OF.get((func, t), f"{func}_i64")


def _tile():
    from datafusion_amd import ops
    return ops.WINDOW_TILE


def run(table, partition_by, order_by, exprs):
    """ops.window over an Arrow table -> (result as Arrow, {profile name: stats})"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    dev = DeviceTable.from_arrow(table)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        out = ops.window(dev, partition_by, order_by, exprs)
        got = out.to_arrow()
        out.free()
        return got, {k: v for k, v in ops.profile_stats().items() if k.startswith("window_")}
    finally:
        ops.profile_enable(False)
        dev.free()


def _exprs(specs):
    from datafusion_amd.expr import col
    return [(f, None if a is None else col(a), n, fr) for f, a, n, fr in specs]


def _bits(x):
    return None if x is None else struct.pack("<d", x)


def hold(label, func, want, got, k=0, record=None):
    """one value against the restatement's"""
    if isinstance(want, W.FloatSum):
        assert got is not None, label
        gk = R.gamma(k)
        bound = (gk + R.gamma(want.m - 1) * (1 + gk)) * want.S
        exact = want.exact
        if func == "avg":
            exact = want.exact / want.m
            bound = bound / want.m + (R.U * abs(exact) if abs(exact) >= Fraction(1, 2**1022) else Fraction(1, 2**1075))
        if record is not None:
            record[0] = max(record[0], R.ratio(got, exact, bound))
        assert R.within(got, exact, bound), (label, got, float(exact), R.ratio(got, exact, bound))
    elif isinstance(want, float) and func in ("min", "max"):
        assert _bits(got) == _bits(want), (label, got, want)
    else:
        assert got == want and type(got) is type(want), (label, got, want)


def check(got, table, cols, types, partition_by, order_by, specs, label=""):
    """the input's columns first and unchanged, then one column per expression: types and every value"""
    names = table.column_names
    assert got.column_names == names + [s[2] for s in specs], got.column_names
    for c in names:      # (Float64 by their bits: a NaN equals itself here)
        a, b = got.column(c).to_pylist(), table.column(c).to_pylist()
        assert (list(map(_bits, a)) == list(map(_bits, b))) if pa.types.is_floating(table.schema.field(c).type) else a == b, f"the input column {c} changed"
    want = W.window(cols, types, partition_by, order_by, specs)
    for func, arg, name, frame in specs:
        tag = "uint64" if func in W.RANKING else WC.result_tag(func, None if arg is None else types[arg])
        assert got.schema.field(name).type == WC.arrow_type(tag), (label, name, got.schema.field(name).type)
        if func in W.RANKING or func == "count":
            assert got.column(name).null_count == 0
        col = WC.from_array(got.column(name), tag)
        for i, (w, g) in enumerate(zip(want[name], col)):
            hold((label, name, i), func, w, g)


# ------------------------------------------------------------------------------------------------------------------------ the shapes
@functools.lru_cache(maxsize=None)
def shape_keys():
    """partition lengths that straddle the 64-row words (float_sum_ref's runs) and the tile (T - 1, T, T + 1 and 3T + 5: a whole tile
    without a head), peer groups of three rows — of 700 in the long partitions, so that peer groups cross tile edges too"""
    T = _tile()
    lengths = list(R.WORD_EDGE_RUNS) + list(R.SHORT_RUNS) + [T - 1, T, T + 1, 3 * T + 5, 1, 1, 7]
    p, o = [], []
    for g, length in enumerate(lengths):
        p += [g // 2 if g % 5 else None] * length                     # pairs of partitions share p (and one in five has a NULL p) ...
        o += [(j // (700 if length >= T - 1 else 3)) for j in range(length)]
    q = [g for g, length in enumerate(lengths) for _ in range(length)]   # ... so that only q changes at every other boundary
    starts = np.cumsum([0] + lengths[:-1]).tolist()
    long_peers = [(a + k, min(a + length, a + k + 700) - 1) for a, length in zip(starts, lengths) if length >= T - 1 for k in range(0, length, 700)]
    assert sum(1 for s, e in long_peers if s // T != e // T) >= 4          # peer groups that cross a tile edge
    assert any(a % T == 0 or (a + length) % T != 0 for a, length in zip(starts, lengths))
    return lengths, p, q, o


def shape_table(arg_cols: dict, arg_types: dict, fill=None):
    lengths, p, q, o = shape_keys()
    cols = dict({"p": p, "q": q, "o": o}, **arg_cols)
    types = dict({"p": "int32", "q": "int64", "o": "int32"}, **arg_types)
    return cols, types, WC.to_arrow(cols, types, fill)


def _nulled(rng, values, null_frac):
    return [None if null_frac and rng.random() < null_frac else v for v in values]


def _arguments(kind, n, null_frac):
    """{column: values}, {column: type tag}, {column: functions} of one argument type"""
    rng = np.random.default_rng([7, n, int(null_frac * 100), len(kind)])
    if kind == "int32":
        return {"x": _nulled(rng, rng.integers(-10**6, 10**6, n).tolist(), null_frac)}, {"x": "int32"}, {"x": ("sum", "count", "min", "max", "avg")}
    if kind == "int64":
        return {"x": _nulled(rng, rng.integers(-10**12, 10**12, n).tolist(), null_frac)}, {"x": "int64"}, {"x": ("sum", "count", "min", "max", "avg")}
    if kind == "date32":
        return {"x": _nulled(rng, rng.integers(-40000, 40000, n).tolist(), null_frac)}, {"x": "date32"}, {"x": ("count", "min", "max")}
    if kind == "float64":
        finite = np.ldexp(rng.uniform(-1, 1, n), rng.integers(-30, 30, n)).tolist()
        edges = [WC.EDGE_FLOATS[i] for i in rng.integers(0, len(WC.EDGE_FLOATS), n)]
        return ({"x": _nulled(rng, finite, null_frac), "xe": _nulled(rng, edges, null_frac)}, {"x": "float64", "xe": "float64"},
                {"x": ("sum", "count", "avg"), "xe": ("min", "max")})
    if kind == "decimal128":
        money = rng.integers(-10**13, 10**13, n).tolist()
        wide = [int(a) * 10**19 + int(b) for a, b in zip(rng.integers(-10**18, 10**18, n), rng.integers(0, 10**18, n))]   # up to 10^37: sums wrap
        return ({"x": _nulled(rng, money, null_frac), "xw": _nulled(rng, wide, null_frac)}, {"x": ("decimal", 15, 2), "xw": ("decimal", 38, 0)},
                {"x": ("sum", "count", "min", "max", "avg"), "xw": ("sum", "min", "max")})
    raise KeyError(kind)


@pytest.mark.parametrize("null_frac", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["int32", "int64", "date32", "float64", "decimal128"])
def test_every_function_and_frame_over_partitions_around_words_and_tiles(kind, null_frac):
    n = sum(shape_keys()[0])
    arg_cols, arg_types, funcs = _arguments(kind, n, null_frac)
    cols, types, table = shape_table(arg_cols, arg_types, fill={"x": R.NULL_FILLER if kind == "float64" else 77})
    specs = list(RANKS)
    for frame in W.FRAMES:
        specs += [(f, a, f"{f}_{a}_{frame}", frame) for a, fs in funcs.items() for f in fs] + [("count", None, f"n_{frame}", frame)]
    got, prof = run(table, ["p", "q"], ["o"], _exprs(specs))
    check(got, table, cols, types, ["p", "q"], ["o"], specs, label=f"{kind} nulls={null_frac}")
    expect = {"window_heads", "window_starts", "window_ends", "window_rank", "window_dense_rank", "window_peer_popcount", "window_finish", "window_pick",
              "window_scan_count"} | {_scan_name(f, arg_types[a]) for a, fs in funcs.items() for f in fs}
    assert set(prof) == expect, sorted(set(prof) ^ expect)
    assert prof["window_heads"]["calls"] == 1 and prof["window_starts"]["calls"] == 2 and prof["window_ends"]["calls"] == 2     # made once, shared
    n_aggs = len(specs) - 3
    assert prof["window_pick"]["calls"] == 2 * n_aggs // 3 and prof["window_finish"]["calls"] == n_aggs // 3


def test_zero_rows_one_row_and_zero_expressions():
    from datafusion_amd.expr import col
    types = {"p": "int32", "o": "int32", "x": "int64", "d": ("decimal", 15, 2)}
    specs = RANKS + [("sum", "x", "s", None), ("avg", "d", "a", "rows_to_current"), ("count", None, "c", "partition"), ("min", "x", "lo", "partition")]
    for cols in ({"p": [], "o": [], "x": [], "d": []}, {"p": [5], "o": [1], "x": [41], "d": [1234]}, {"p": [None], "o": [None], "x": [None], "d": [None]}):
        table = WC.to_arrow(cols, types)
        got, prof = run(table, ["p"], ["o"], _exprs(specs))
        check(got, table, cols, types, ["p"], ["o"], specs, label=str(cols))
        assert bool(prof) == bool(cols["p"])          # no rows: nothing is launched
    table = WC.to_arrow({"p": [1, 1, 2], "o": [1, 2, 3], "x": [1, 2, 3], "d": [1, 2, 3]}, types)
    got, prof = run(table, ["p"], ["o"], [])
    assert got.equals(table) and not prof
    got, _ = run(table, [], [], [("sum", col("x") + col("x"), "twice", "rows_to_current")])      # the argument is an expression
    assert got.column("twice").to_pylist() == [2, 6, 12]


@pytest.mark.parametrize("partition_by, order_by", [([], ["o"]), (["p"], []), ([], [])])
def test_without_partition_keys_without_order_keys_and_without_both(partition_by, order_by):
    rng = np.random.default_rng(3)
    n = 2 * _tile() + 77
    p = sorted(rng.integers(0, 9, n).tolist())
    o = sorted(rng.integers(0, 400, n).tolist())       # (with partition keys there are no order keys here: any order inside a partition serves)
    cols = {"p": p, "o": o, "x": _nulled(rng, rng.integers(-10**9, 10**9, n).tolist(), 0.1)}
    types = {"p": "int32", "o": "int32", "x": "int64"}
    table = WC.to_arrow(cols, types)
    specs = RANKS + [(f, "x", f"{f}_{fr}", fr) for f in ("sum", "count", "min", "avg") for fr in W.FRAMES]
    got, prof = run(table, partition_by, order_by, _exprs(specs))
    check(got, table, cols, types, partition_by, order_by, specs, label=f"{partition_by} {order_by}")
    assert {"window_heads", "window_pick", "window_finish", "window_scan_add_u64"} <= set(prof)


def test_a_unique_order_key_skips_the_peer_pick():
    lengths = [3, 64, 65, 2000, 700]
    p = [g for g, length in enumerate(lengths) for _ in range(length)]
    o = [j for length in lengths for j in range(length)]
    rng = np.random.default_rng(5)
    cols = {"p": p, "o": o, "x": _nulled(rng, rng.integers(-10**9, 10**9, len(p)).tolist(), 0.1)}
    types = {"p": "int32", "o": "int64", "x": "int64"}
    table = WC.to_arrow(cols, types)
    specs = [("sum", "x", "s", "range_to_current"), ("max", "x", "hi", None), ("rank", None, "rk", None)]
    got, prof = run(table, ["p"], ["o"], _exprs(specs))
    check(got, table, cols, types, ["p"], ["o"], specs)
    assert "window_pick" not in prof and prof["window_finish"]["calls"] == 2 and prof["window_peer_popcount"]["calls"] == 1 and "window_ends" not in prof
    with_peers = dict(cols, o=[j // 2 for j in o])
    table2 = WC.to_arrow(with_peers, types)
    got2, prof2 = run(table2, ["p"], ["o"], _exprs(specs))
    check(got2, table2, with_peers, types, ["p"], ["o"], specs)
    assert prof2["window_pick"]["calls"] == 2 and "window_finish" not in prof2 and prof2["window_ends"]["calls"] == 1


# ------------------------------------------------------------------------------------------------------------------------------ keys
KEY_SPECS = RANKS + [("sum", "x", "s", None), ("sum", "x", "r", "rows_to_current"), ("count", "x", "c", "partition")]


def test_null_keys_beside_keys_that_hold_the_same_buffer_value():
    """the slot under a NULL key holds the value of its non-NULL neighbour: bits alone would merge them; two NULLs with different
    slots are still one partition / one peer group"""
    p = [None] * 70 + [9] * 60 + [None] * 5 + [9] * 3
    o = ([None] * 3 + [4] * 3 + [None] * 2 + [4] * 62) + ([4] * 30 + [None] * 30) + [None, None, 4, None, None] + [4, None, 4]
    cols = {"p": p, "o": o, "x": list(range(1, len(p) + 1))}
    types = {"p": "int64", "o": "int32", "x": "int64"}
    table = WC.to_arrow(cols, types, fill={"p": 9, "o": 4})
    got, _ = run(table, ["p"], ["o"], _exprs(KEY_SPECS))
    check(got, table, cols, types, ["p"], ["o"], KEY_SPECS)
    slots = np.where(np.arange(len(p)) % 2 == 0, 9, 123456)                                    # NULL = NULL whatever lies under them
    arr = pa.Array.from_buffers(pa.int64(), len(p), [WC.to_array(p, "int64").buffers()[0], pa.py_buffer(np.where([v is None for v in p], slots, 9).astype(np.int64).tobytes())])
    table2 = table.set_column(0, "p", arr)
    got2, _ = run(table2, ["p"], ["o"], _exprs(KEY_SPECS))
    check(got2, table2, cols, types, ["p"], ["o"], KEY_SPECS)


def test_dictionary_encoded_string_keys_and_decimal_keys():
    lengths = [5, 64, 1, 130, 63, 2]
    words = ["apple", None, "pear", "fig", "apple", "kiwi"]          # "apple" twice, apart: runs, not values, make partitions
    s = [w for w, length in zip(words, lengths) for _ in range(length)]
    d = [(j // 4) * 10**20 + 7 if j % 11 else None for length in lengths for j in range(length)]   # differs in the HIGH word only
    rng = np.random.default_rng(11)
    x = rng.integers(-1000, 1000, len(s)).tolist()
    cols = {"k": s, "d": d, "x": x}
    types = {"d": ("decimal", 38, 0), "x": "int64"}
    sa = pa.array(s, type=pa.string()).dictionary_encode()
    table = pa.table({"k": sa, "d": WC.to_array(d, types["d"]), "x": WC.to_array(x, "int64")})
    got, prof = run(table, ["k"], ["d"], _exprs(KEY_SPECS))
    assert pa.types.is_dictionary(got.schema.field("k").type) and got.column("k").to_pylist() == s      # the dictionary is handed on
    want = W.window(cols, types, ["k"], ["d"], KEY_SPECS)
    for _, _, name, _ in KEY_SPECS:
        assert got.column(name).to_pylist() == want[name], name
    assert got.column("d").to_pylist() == table.column("d").to_pylist() and "window_heads" in prof
    # the decimal as the partition key, the dictionary as the order key
    order = sorted(range(len(s)), key=lambda i: (d[i] is None, d[i] or 0))
    cols2 = {k: [v[i] for i in order] for k, v in cols.items()}
    table2 = table.take(pa.array(order))
    got2, _ = run(table2, ["d"], ["k"], _exprs(KEY_SPECS))
    want2 = W.window(cols2, types, ["d"], ["k"], KEY_SPECS)
    for _, _, name, _ in KEY_SPECS:
        assert got2.column(name).to_pylist() == want2[name], name


# -------------------------------------------------------------------------------------------------- more tiles than one carry round
def test_int64_over_more_tiles_than_the_carry_scan_takes_in_a_round():
    """the carry kernel is ONE workgroup of 256 threads that takes 256 tiles per round: 300 + 600 000 + ... rows put a partition across the
    round's edge (tile 256).  Compared with vectorised numpy (wrapping Int64 sums by cumsum differences — exact for integers)."""
    T = _tile()
    rng = np.random.default_rng(17)
    lengths = [300, 600_000] + rng.integers(1, 4000, 60).tolist()
    n = int(sum(lengths))
    assert n > 256 * T + T and 300 < 256 * T < 600_300
    part = np.repeat(np.arange(len(lengths)), lengths)
    o = (np.arange(n) - np.repeat(np.cumsum([0] + lengths[:-1]), lengths)) // 5          # peer groups of five rows
    x = rng.integers(-2**62, 2**62, n)
    valid = rng.random(n) >= 0.05
    table = pa.table({"p": pa.array(part, type=pa.int64()), "o": pa.array(o, type=pa.int64()), "x": pa.array(x, type=pa.int64(), mask=~valid)})
    specs = RANKS + [("sum", "x", "s_rows", "rows_to_current"), ("sum", "x", "s_range", None), ("sum", "x", "s_part", "partition"), ("count", "x", "c_range", None),
                     ("max", "x", "hi_rows", "rows_to_current")]
    got, prof = run(table, ["p"], ["o"], _exprs(specs))
    idx = np.arange(n)
    head = np.r_[True, part[1:] != part[:-1]]
    peer = head | np.r_[True, o[1:] != o[:-1]]
    start = np.maximum.accumulate(np.where(head, idx, 0))
    peer_start = np.maximum.accumulate(np.where(peer, idx, 0))
    part_end = np.minimum.accumulate(np.where(np.r_[head[1:], True], idx, n)[::-1])[::-1]
    peer_end = np.minimum.accumulate(np.where(np.r_[peer[1:], True], idx, n)[::-1])[::-1]
    xv = np.where(valid, x, 0)
    with np.errstate(over="ignore"):
        cs = np.r_[0, np.cumsum(xv)]
    cc = np.r_[0, np.cumsum(valid)]

    def col(name):
        return got.column(name).combine_chunks()

    def nullable(name, values, count):
        a = col(name)
        assert np.array_equal(np.asarray(a.is_valid()), count > 0), name
        assert np.array_equal(a.fill_null(0).to_numpy()[count > 0], values[count > 0]), name
    assert np.array_equal(col("rn").to_numpy(), (idx - start + 1).astype(np.uint64))
    assert np.array_equal(col("rk").to_numpy(), (peer_start - start + 1).astype(np.uint64))
    dense = np.cumsum(peer)
    assert np.array_equal(col("dr").to_numpy(), (dense - dense[start] + 1).astype(np.uint64))
    for name, end in (("s_rows", idx), ("s_range", peer_end), ("s_part", part_end)):
        nullable(name, cs[end + 1] - cs[start], cc[end + 1] - cc[start])
    assert np.array_equal(col("c_range").to_numpy(), cc[peer_end + 1] - cc[start])
    run_max = np.empty(n, np.int64)
    lo = np.iinfo(np.int64).min
    for a, b in zip(np.flatnonzero(head), np.r_[np.flatnonzero(head)[1:], n]):
        run_max[a:b] = np.maximum.accumulate(np.where(valid[a:b], x[a:b], lo))
    nullable("hi_rows", run_max, cc[idx + 1] - cc[start])
    assert {"window_scan_add_u64", "window_scan_count", "window_scan_max_i64", "window_pick", "window_finish"} <= set(prof)


# ------------------------------------------------------------------------------------------------------------------- Float64 families
@functools.lru_cache(maxsize=None)
def _family_gids():
    T = _tile()
    lengths = list(R.WORD_EDGE_RUNS) + [T + 1] + list(R.SHORT_RUNS)      # a run longer than a tile between runs around the 64-row words
    return R.run_lengths_gids(lengths)


@pytest.mark.parametrize("null_frac", R.NULL_FRACTIONS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_float64_sums_and_averages_stay_inside_the_derived_bound(family, null_frac, record_property):
    from datafusion_amd.expr import col, lit
    gids = _family_gids()
    n = len(gids)
    assert n <= 70_000
    fam = R.family(family, gids, null_frac, seed=1)
    o = (np.arange(n) // 3).tolist()
    valid = fam["valid"]
    if family == "money_expr":
        exact, _ = R.money_rows(fam)
        x = [e if v else None for e, v in zip(exact, valid.tolist())]                     # the expression's exact value per row (a Fraction)
        table = pa.table({"p": pa.array(gids), "o": pa.array(o, type=pa.int64()), "price": R.f64_array(fam["price"], valid),
                          "disc": pa.array(fam["disc"]), "tax": pa.array(fam["tax"])})
        one = lit(1.0, pa.float64())
        arg, k = col("price") * (one - col("disc")) * (one + col("tax")), R.MONEY_K
    else:
        x = [float(v) if ok else None for v, ok in zip(fam["x"].tolist(), valid.tolist())]
        table = pa.table({"p": pa.array(gids), "o": pa.array(o, type=pa.int64()), "x": R.f64_array(fam["x"], valid)})     # NULL_FILLER under the NULLs
        arg, k = col("x"), 0
    cols = {"p": gids.tolist(), "o": o, "x": x}
    specs = [(f, "x", f"{f}_{fr}", fr) for f in ("sum", "avg") for fr in W.FRAMES] + [("count", "x", "c", None), ("count", None, "rows", "partition")]
    got, prof = run(table, ["p"], ["o"], [(f, None if a is None else arg, nm, fr) for f, a, nm, fr in specs])
    want = W.window(cols, {"x": "float64"}, ["p"], ["o"], specs)
    worst = {}
    for func, a, name, frame in specs:
        col_ = got.column(name).to_pylist()
        for i, (w, g) in enumerate(zip(want[name], col_)):
            hold((family, name, i), func, w, g, k=k, record=worst.setdefault(frame or "range_to_current", [0.0]))
    for frame, (ratio,) in worst.items():
        record_property(f"worst_ratio_{frame}", ratio)
        print(f"window float bound: family={family} nulls={null_frac} frame={frame} worst |error| / bound = {ratio:.4g}")
    assert {"window_scan_add_f64", "window_pick", "window_finish"} <= set(prof) and prof["window_scan_add_f64"]["calls"] == 6


# ------------------------------------------------------------------------------------------------------------------------- the plan
def test_top_three_per_partition_through_the_rule():
    """SortExec -> WindowAggExec -> FilterExec(rank <= 3) over unsorted rows: offloaded as it stands, compared with the restatement
    over the rows in (g, v) order"""
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(23)
    n = 5000
    g = rng.integers(0, 40, n).tolist()
    v = rng.integers(0, 300, n).tolist()                       # ties: ranks repeat
    pay = list(range(n))
    table = pa.table({"g": pa.array(g, type=pa.int32()), "v": pa.array(v, type=pa.int64()), "pay": pa.array(pay, type=pa.int64())})
    leaf = P.MemoryExec(DeviceTable.from_arrow(table), "t")
    wexpr = [("rank", None, "rk", None), ("sum", col("v"), "running", None)]
    plan = P.FilterExec(col("rk") <= lit(3, pa.uint64()), P.WindowAggExec(wexpr, ["g"], [("v", False, False)], P.SortExec([("g", False, False), ("v", False, False)], leaf)))
    rule = P.GpuOffloadRule()
    opt = rule.optimize(plan)
    assert not rule.declined and [type(x).__name__ for x in (opt, opt.input, opt.input.input)] == ["FilterExec", "WindowAggExec", "SortExec"]
    assert P.plan_schema(opt.input).names == ["g", "v", "pay", "rk", "running"] and P.plan_schema(opt.input).types[3:] == [pa.uint64(), pa.int64()]
    out = P.collect(opt)
    got = out.to_arrow()
    out.free()
    order = sorted(range(n), key=lambda i: (g[i], v[i]))
    cols = {"g": [g[i] for i in order], "v": [v[i] for i in order]}
    want = W.window(cols, {"v": "int64"}, ["g"], ["v"], [("rank", None, "rk", None), ("sum", "v", "running", None)])
    keep = [i for i in range(n) if want["rk"][i] <= 3]
    assert got.column("g").to_pylist() == [cols["g"][i] for i in keep] and got.column("v").to_pylist() == [cols["v"][i] for i in keep]
    assert got.column("rk").to_pylist() == [want["rk"][i] for i in keep] and got.column("running").to_pylist() == [want["running"][i] for i in keep]
    assert sorted(got.column("pay").to_pylist()) == sorted(pay[order[i]] for i in keep)      # (ties may arrive in either order)


# ------------------------------------------------------------------------------------------------------------------------- declines
def _decline_table():
    from decimal import Decimal
    return pa.table({"i": pa.array([1, 1, 2], type=pa.int32()), "f": pa.array([1.0, 1.0, 2.0]), "b": pa.array([True, True, False]),
                     "s": pa.array(["a", "a", "b"]), "wide": pa.array([Decimal("1.00"), Decimal("2.50"), Decimal("3.25")], type=pa.decimal128(30, 2)),
                     "ok": pa.array([Decimal("1.00"), Decimal("2.50"), Decimal("3.25")], type=pa.decimal128(15, 2))})


@pytest.mark.parametrize("partition_by, order_by, wexpr, needle", [
    (["f"], ["i"], None, "Float64 window keys are not supported on the GPU path"),
    (["i"], ["f"], None, "Float64 window keys are not supported on the GPU path"),
    (["b"], ["i"], None, "Boolean window keys are not supported on the GPU path"),
    (["i"], ["s"], None, "Utf8 window keys are not supported on the GPU path"),
    (["i"], ["i"], ("avg", "wide"), "Decimal256"),
    (["i"], ["i"], ("sum", "b"), "SUM(a) over bool is not supported on the GPU path"),
])
def test_what_the_device_does_not_take_stays_on_the_cpu_and_the_library_refuses_it_too(partition_by, order_by, wexpr, needle):
    from datafusion_amd import _lib, ops, physical_plan as P
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    dev = DeviceTable.from_arrow(_decline_table())
    leaf = P.MemoryExec(dev, "t")
    exprs = [("rank", None, "rk", None)] + ([(wexpr[0], col(wexpr[1]), "a", None)] if wexpr else [])
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.WindowAggExec(exprs, partition_by, order_by, leaf))
    assert isinstance(out, P.WindowAggExec) and getattr(out, "kept_on_cpu", False)
    assert len(rule.declined) == 1 and needle in rule.declined[0][1], rule.declined
    with pytest.raises(_lib.DfgpuError, match="not supported on the GPU path") as err:          # the run-time twin
        ops.window(dev, partition_by, order_by, exprs)
    if wexpr is None:
        assert str(err.value) == rule.declined[0][1]
    # the same plan over supported columns next to them is taken, and runs
    good = [("rank", None, "rk", None), ("avg", col("ok"), "a", None), ("min", col("wide"), "lo", "partition")]
    rule2 = P.GpuOffloadRule()
    opt = rule2.optimize(P.WindowAggExec(good, ["i"], ["i"], leaf))
    assert not getattr(opt, "kept_on_cpu", False) and not rule2.declined
    res = P.collect(opt)
    from decimal import Decimal
    assert res.to_arrow().column("a").to_pylist() == [Decimal("1.750000"), Decimal("1.750000"), Decimal("3.250000")]
    assert res.to_arrow().column("lo").to_pylist() == [Decimal("1.00"), Decimal("1.00"), Decimal("3.25")]
    res.free()
    dev.free()


def test_the_c_abi_refuses_an_unsupported_key_with_the_same_message():
    from datafusion_amd import _lib, physical_plan as P
    from datafusion_amd.table import DeviceTable
    lib = _lib.init()
    dev = DeviceTable.from_arrow(_decline_table())
    spec = _lib.WindowSpec()
    spec.func, spec.name = 0, b"rn"
    for key, other in ((1, 0), (2, 0), (3, 0)):
        for part, order in (((key,), (other,)), ((other,), (key,))):
            out = C.c_void_p()
            rc = lib.dfgpu_window(dev.handle, (C.c_int * 1)(*part), 1, (C.c_int * 1)(*order), 1, C.byref(spec), 1, C.byref(out))
            assert rc != 0 and not out.value
            message = lib.dfgpu_last_error().decode()
            names = dev.column_names
            rule = P.GpuOffloadRule()
            rule.optimize(P.WindowAggExec([("row_number", None, "rn", None)], [names[part[0]]], [names[order[0]]], P.MemoryExec(dev, "t")))
            assert message == rule.declined[0][1], (message, rule.declined)
    out = C.c_void_p()
    assert lib.dfgpu_window(dev.handle, (C.c_int * 1)(9), 1, None, 0, C.byref(spec), 1, C.byref(out)) != 0           # a column the table does not have
    assert "out of range" in lib.dfgpu_last_error().decode()
    dev.free()

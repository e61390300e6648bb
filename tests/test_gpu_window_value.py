"""percent_rank, cume_dist, ntile and first_value / last_value / nth_value of the GPU WindowAggExec (ABI 18) against
tests/window_value_ref.py, value by value and exactly: Float64 results and Float64 arguments by their bits, every other type by ==.
These functions take a row's positions from the 64-row words of the two head bitmaps plus one number per word and direction
(window_word_starts / window_word_ends), so the shapes sit around the words, around the scan's tile (T = ops.WINDOW_TILE) counted in
ROWS and counted in WORDS (a partition of more than 2 * 64 * T rows leaves a whole tile of the word scan without a head), and at the
ends of the input.  Output types, null counts and the unchanged input columns are checked; every case asserts the `window_` kernels it
ran — never window_starts / window_ends, the n * 8 position arrays of the older functions."""
import ctypes as C
import functools
import struct

import numpy as np
import pyarrow as pa
import pytest

from tests import float_sum_ref as R
from tests import window_cases as WC
from tests import window_ref as W
from tests import window_value_ref as V

pytestmark = pytest.mark.gpu

DIST_TYPE = {"percent_rank": pa.float64(), "cume_dist": pa.float64(), "ntile": pa.uint64()}
NTILES = (1, 3, 4, 10, 2**40)
NTHS = (1, 2, 3, -1, -2, 5000)


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


def _fname(func):
    return func[0] if isinstance(func, tuple) else func


def _bits(x):
    return None if x is None else struct.pack("<d", x)


def _same(a, b, floating):
    return list(map(_bits, a)) == list(map(_bits, b)) if floating else a == b


def _launches(specs):
    """(window_dist launches, window_value launches) of these expressions: last_value over rows_to_current is the argument itself"""
    dist = sum(1 for f, _, _, _ in specs if _fname(f) in V.DIST)
    value = sum(1 for f, _, _, fr in specs if _fname(f) in V.VALUE and not (_fname(f) == "last_value" and fr == "rows_to_current"))
    return dist, value


def check(got, table, cols, types, partition_by, order_by, specs, label=""):
    """the input's columns first and unchanged, then one column per expression: its type, its null count and every value"""
    names = table.column_names
    assert got.column_names == names + [s[2] for s in specs], got.column_names
    for c in names:
        assert _same(got.column(c).to_pylist(), table.column(c).to_pylist(), pa.types.is_floating(table.schema.field(c).type)), f"the input column {c} changed"
    want = V.window(cols, partition_by, order_by, specs)
    for func, arg, name, frame in specs:
        f = _fname(func)
        field, column = got.schema.field(name), got.column(name)
        if f in V.DIST:
            assert field.type == DIST_TYPE[f] and column.null_count == 0, (label, name, field)
            values = column.to_pylist()
            assert all(type(v) is (int if f == "ntile" else float) for v in values), (label, name)
        else:
            tag = types[arg]
            assert field.type == WC.arrow_type(tag), (label, name, field.type)
            assert column.null_count == sum(v is None for v in want[name]), (label, name, column.null_count)
            values = WC.from_array(column, tag)
        floating = f in ("percent_rank", "cume_dist") or (arg is not None and types[arg] == "float64")
        if not _same(values, want[name], floating):
            bad = [i for i, (g, w) in enumerate(zip(values, want[name])) if not _same([g], [w], floating)]
            raise AssertionError((label, name, f"{len(bad)} rows differ, the first at {bad[0]}: {values[bad[0]]!r} != {want[name][bad[0]]!r}"))


# ------------------------------------------------------------------------------------------------------------------------ the shapes
@functools.lru_cache(maxsize=None)
def shape_keys():
    """test_gpu_window.py's recipe: partition lengths that straddle the 64-row words and the tile (T - 1, T, T + 1 and 3T + 5), peer
    groups of three rows — of 700 in the long partitions —, one partition in five with a NULL p, and every other boundary one at which
    only the second key changes"""
    T = _tile()
    lengths = list(R.WORD_EDGE_RUNS) + list(R.SHORT_RUNS) + [T - 1, T, T + 1, 3 * T + 5, 1, 1, 7]
    p, o = [], []
    for g, length in enumerate(lengths):
        p += [g // 2 if g % 5 else None] * length
        o += [(j // (700 if length >= T - 1 else 3)) for j in range(length)]
    q = [g for g, length in enumerate(lengths) for _ in range(length)]
    return lengths, p, q, o


def _nulled(rng, values, null_frac):
    return [None if null_frac and rng.random() < null_frac else v for v in values]


def test_every_function_over_partitions_around_words_and_tiles():
    lengths, p, q, o = shape_keys()
    n = len(p)
    rng = np.random.default_rng(41)
    cols = {"p": p, "q": q, "o": o, "x": _nulled(rng, rng.integers(-10**12, 10**12, n).tolist(), 0.1)}
    types = {"p": "int32", "q": "int64", "o": "int32", "x": "int64"}
    table = WC.to_arrow(cols, types, fill={"x": 7777777})
    specs = [("percent_rank", None, "pr", None), ("cume_dist", None, "cd", None)] + [(("ntile", k), None, f"q{k}", None) for k in NTILES]
    for frame in V.FRAMES:
        specs += [("first_value", "x", f"first_{frame}", frame), ("last_value", "x", f"last_{frame}", frame)]
        specs += [(("nth_value", k), "x", f"nth_{k}_{frame}".replace("-", "m"), frame) for k in NTHS]
    got, prof = run(table, ["p", "q"], ["o"], _exprs(specs))
    check(got, table, cols, types, ["p", "q"], ["o"], specs)
    assert set(prof) == {"window_heads", "window_word_starts", "window_word_ends", "window_dist", "window_value"}, sorted(prof)   # no window_starts / window_ends
    # one summary per bitmap and direction, however many functions asked: starts of partitions and peers (percent_rank), ends of both
    assert prof["window_heads"]["calls"] == 1 and prof["window_word_starts"]["calls"] == 2 and prof["window_word_ends"]["calls"] == 2
    assert (prof["window_dist"]["calls"], prof["window_value"]["calls"]) == _launches(specs) == (2 + len(NTILES), 3 * (2 + len(NTHS)) - 1)


@pytest.mark.parametrize("funcs, starts, ends", [
    ([(("ntile", 3), None, "q", None)], 1, 1),                                             # never the peer bitmap
    ([("percent_rank", None, "pr", None)], 2, 1),
    ([("cume_dist", None, "cd", None)], 1, 2),
    ([("first_value", "x", "f", "partition")], 1, 0),
    ([("last_value", "x", "l", "partition")], 0, 1),
    ([("last_value", "x", "l", None), (("nth_value", -1), "x", "m", None)], 1, 1),          # peer ends; nth_value needs the start too
    ([(("nth_value", 2), "x", "n2", "rows_to_current")], 1, 0),
    ([("last_value", "x", "l", "rows_to_current")], 0, 0),                                  # the argument itself
])
def test_a_call_scans_only_the_summaries_its_functions_read(funcs, starts, ends):
    lengths = [3, 64, 65, 200, 61]
    p = [g for g, length in enumerate(lengths) for _ in range(length)]
    o = [j // 4 for length in lengths for j in range(length)]
    rng = np.random.default_rng(43)
    cols = {"p": p, "o": o, "x": _nulled(rng, rng.integers(-1000, 1000, len(p)).tolist(), 0.2)}
    types = {"p": "int32", "o": "int64", "x": "int32"}
    table = WC.to_arrow(cols, types)
    got, prof = run(table, ["p"], ["o"], _exprs(funcs))
    check(got, table, cols, types, ["p"], ["o"], funcs)
    dist, value = _launches(funcs)
    want = {"window_heads": 1, "window_word_starts": starts, "window_word_ends": ends, "window_dist": dist, "window_value": value}
    assert {k: v["calls"] for k, v in prof.items()} == {k: v for k, v in want.items() if v}, prof


def test_a_tile_of_the_word_scan_without_a_head():
    """a partition of 2 * 64 * T + 130 rows that starts in the middle of a word: words 2048 .. 4095 — the second tile of the scans over
    the partition bitmap's words — hold no head at all, so their last_upto / first_from come through the carry alone"""
    T = _tile()
    lengths = [5, 64, 37] + [63] * 60 + [2 * 64 * T + 130] + [3, 70, 1] + [65] * 60
    n = sum(lengths)
    start = sum(lengths[:63])
    assert 268_000 < n < 272_000 and start % 64 and (start + lengths[63]) // 64 > 2 * T > T > start // 64 + 1
    part = np.repeat(np.arange(len(lengths)), lengths)
    within = np.arange(n) - np.repeat(np.cumsum([0] + lengths[:-1]), lengths)
    o = within // 1000
    rng = np.random.default_rng(47)
    x = rng.integers(-2**62, 2**62, n)
    valid = rng.random(n) >= 0.1
    table = pa.table({"p": pa.array(part, type=pa.int32()), "o": pa.array(o, type=pa.int64()), "x": pa.array(x, type=pa.int64(), mask=~valid)})
    cols = {"p": part.tolist(), "o": o.tolist(), "x": [int(v) if ok else None for v, ok in zip(x.tolist(), valid.tolist())]}
    types = {"p": "int32", "o": "int64", "x": "int64"}
    specs = [(("ntile", 7), None, "q7", None), ("percent_rank", None, "pr", None), ("cume_dist", None, "cd", None), ("first_value", "x", "fv", None),
             ("last_value", "x", "lv", None), (("nth_value", -3), "x", "m3", None)]
    got, prof = run(table, ["p"], ["o"], _exprs(specs))
    check(got, table, cols, types, ["p"], ["o"], specs)
    assert set(prof) == {"window_heads", "window_word_starts", "window_word_ends", "window_dist", "window_value"}
    assert prof["window_word_starts"]["calls"] == 2 and prof["window_word_ends"]["calls"] == 2


# ------------------------------------------------------------------------------------------------------------- the ends of the input
END_SPECS = [("percent_rank", None, "pr", None), ("cume_dist", None, "cd", None), (("ntile", 4), None, "q4", None), (("ntile", 1), None, "q1", None),
             ("first_value", "x", "fv", None), ("last_value", "x", "lv", None), ("last_value", "x", "lv_part", "partition"),
             ("last_value", "x", "lv_rows", "rows_to_current"), (("nth_value", 2), "x", "n2", "rows_to_current"), (("nth_value", -2), "x", "m2", "partition"),
             (("nth_value", -1), "x", "m1", None)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128])
def test_the_ends_of_the_input(n):
    """no partition keys (one partition), no order keys (every row a peer), neither, and both — with partitions of 64 rows, so that the
    last one ends exactly on a word edge (n = 64, 128) or is the one row past it (n = 65)"""
    rng = np.random.default_rng(53 + n)
    cols = {"p": [j // 64 for j in range(n)], "o": [j // 3 for j in range(n)], "x": _nulled(rng, rng.integers(-10**6, 10**6, n).tolist(), 0.2)}
    types = {"p": "int32", "o": "int32", "x": "int64"}
    table = WC.to_arrow(cols, types)
    for partition_by, order_by in (([], ["o"]), (["p"], []), ([], []), (["p"], ["o"])):
        got, prof = run(table, partition_by, order_by, _exprs(END_SPECS))
        check(got, table, cols, types, partition_by, order_by, END_SPECS, label=f"n={n} {partition_by} {order_by}")
        if n == 0:
            assert not prof            # no rows: nothing is launched
        else:
            assert set(prof) == {"window_heads", "window_word_starts", "window_word_ends", "window_dist", "window_value"}, sorted(prof)
            assert (prof["window_dist"]["calls"], prof["window_value"]["calls"]) == _launches(END_SPECS)


# ---------------------------------------------------------------------------------------------------------------- the argument types
TYPE_LENGTHS = (5, 64, 1, 130, 63, 2, 70)
VALUE_SPECS = [("first_value", "x", "fv", None), ("last_value", "x", "lv", None), ("last_value", "x", "lv_part", "partition"),
               (("nth_value", 2), "x", "n2", "rows_to_current"), (("nth_value", -2), "x", "m2", "partition"), (("nth_value", 3), "x", "n3", None)]
FILL = {"int32": -123456, "int64": 7777777, "uint8": 201, "uint32": 4000000000, "uint64": 2**63 + 5, "date32": 12345, "float64": R.NULL_FILLER, "decimal": 10**30 + 1}
NUMPY_OF = {"int32": np.int32, "int64": np.int64, "uint8": np.uint8, "uint32": np.uint32, "uint64": np.uint64, "date32": np.int32, "float64": np.uint64}


def _type_keys():
    p = [g for g, length in enumerate(TYPE_LENGTHS) for _ in range(length)]
    o = [j // 3 for length in TYPE_LENGTHS for j in range(length)]
    return p, o


def _values(kind, rng, n):
    if kind == "int32":
        return rng.integers(-2**31, 2**31, n).tolist(), "int32"
    if kind == "int64":
        return rng.integers(-2**63, 2**63 - 1, n).tolist(), "int64"
    if kind == "uint8":
        return rng.integers(0, 256, n).tolist(), "uint8"
    if kind == "uint32":
        return rng.integers(0, 2**32, n).tolist(), "uint32"
    if kind == "uint64":
        return [int(v) for v in rng.integers(0, 2**64 - 1, n, dtype=np.uint64)], "uint64"
    if kind == "date32":
        return rng.integers(-40000, 40000, n).tolist(), "date32"
    if kind == "float64":
        return [WC.EDGE_FLOATS[i] for i in rng.integers(0, len(WC.EDGE_FLOATS), n)], "float64"
    if kind == "decimal":
        return [int(a) * 10**19 + int(b) for a, b in zip(rng.integers(-10**18, 10**18, n), rng.integers(0, 10**18, n))], ("decimal", 38, 0)
    raise KeyError(kind)


@pytest.mark.parametrize("null_frac", [0.0, 0.3])
@pytest.mark.parametrize("kind", ["int32", "int64", "uint8", "uint32", "uint64", "date32", "float64", "decimal"])
def test_value_functions_over_every_fixed_width_type(kind, null_frac):
    p, o = _type_keys()
    n = len(p)
    rng = np.random.default_rng([59, len(kind), int(null_frac * 10)])
    values, tag = _values(kind, rng, n)
    cols = {"p": p, "o": o, "x": _nulled(rng, values, null_frac)}
    types = {"p": "int32", "o": "int32", "x": tag}
    table = WC.to_arrow(cols, types, fill={"x": FILL[kind]})       # what lies under a NULL argument must never show
    got, prof = run(table, ["p"], ["o"], _exprs(VALUE_SPECS))
    check(got, table, cols, types, ["p"], ["o"], VALUE_SPECS, label=f"{kind} nulls={null_frac}")
    assert set(prof) == {"window_heads", "window_word_starts", "window_word_ends", "window_value"} and prof["window_value"]["calls"] == len(VALUE_SPECS)
    if kind != "decimal":                                          # the value slot under a NULL result is 0
        for _, _, name, _ in VALUE_SPECS:
            arr = got.column(name).combine_chunks()
            if arr.null_count:
                slots = np.frombuffer(arr.buffers()[1], dtype=NUMPY_OF[kind])[arr.offset:arr.offset + n]
                assert not slots[~np.asarray(arr.is_valid())].any(), (name, "a value slot under a NULL is not zero")


def test_dictionary_encoded_strings_an_expression_and_the_old_functions_beside_them():
    from datafusion_amd.expr import col, lit
    p, o = _type_keys()
    n = len(p)
    rng = np.random.default_rng(61)
    words = ["apple", "pear", "fig", "kiwi", "plum", "lime"]
    s = _nulled(rng, [words[i] for i in rng.integers(0, len(words), n)], 0.2)
    i64 = _nulled(rng, rng.integers(-10**9, 10**9, n).tolist(), 0.2)
    cols = {"p": p, "o": o, "s": s, "i64": i64, "plus": [None if v is None else v + 1 for v in i64]}
    table = pa.table({"p": pa.array(p, type=pa.int32()), "o": pa.array(o, type=pa.int32()), "s": pa.array(s, type=pa.string()).dictionary_encode(),
                      "i64": WC.to_array(i64, "int64")})
    new = [("first_value", "s", "s_first", None), ("last_value", "s", "s_last", None), (("nth_value", -2), "s", "s_m2", "partition"),
           ("last_value", "s", "s_rows", "rows_to_current"), (("ntile", 3), None, "q3", None), ("percent_rank", None, "pr", None)]
    plus = [("last_value", "plus", "e_last", None), (("nth_value", 2), "plus", "e_n2", "rows_to_current")]
    old = [("rank", None, "rk", None), ("sum", "i64", "running", None)]
    exprs = (_exprs(new[:2]) + [("rank", None, "rk", None)] + _exprs(new[2:]) + [("sum", col("i64"), "running", None)]
             + [(f, col("i64") + lit(1), name, fr) for f, _, name, fr in plus])
    got, prof = run(table, ["p"], ["o"], exprs)
    assert got.column_names == ["p", "o", "s", "i64", "s_first", "s_last", "rk", "s_m2", "s_rows", "q3", "pr", "running", "e_last", "e_n2"]
    want = V.window(cols, ["p"], ["o"], new + plus)
    for name in ("s_first", "s_last", "s_m2", "s_rows"):
        assert pa.types.is_dictionary(got.schema.field(name).type), name                                # the codes are picked, the dictionary handed on
        assert got.column(name).to_pylist() == want[name] and got.column(name).null_count == sum(v is None for v in want[name]), name
    assert got.column("s").to_pylist() == s and got.column("i64").to_pylist() == i64
    assert got.column("q3").to_pylist() == want["q3"] and _same(got.column("pr").to_pylist(), want["pr"], True)
    for name in ("e_last", "e_n2"):
        assert got.schema.field(name).type == pa.int64() and got.column(name).to_pylist() == want[name], name
    was = W.window(cols, {"i64": "int64"}, ["p"], ["o"], old)                                            # the old functions beside them, unchanged
    assert got.schema.field("rk").type == pa.uint64() and got.column("rk").to_pylist() == was["rk"]
    assert got.schema.field("running").type == pa.int64() and got.column("running").to_pylist() == was["running"]
    assert {"window_starts", "window_rank", "window_scan_add_u64", "window_pick", "window_word_starts", "window_word_ends", "window_dist", "window_value"} <= set(prof)
    assert prof["window_word_starts"]["calls"] == 2 and prof["window_word_ends"]["calls"] == 2 and prof["window_starts"]["calls"] == 2


# ------------------------------------------------------------------------------------------------------------------------- the plan
def test_the_first_quartile_per_partition_through_the_rule():
    """SortExec -> WindowAggExec -> FilterExec(q == 1) over unsorted rows: offloaded as it stands, compared with the restatement over the
    rows in (g, v) order"""
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(67)
    n = 5000
    g = rng.integers(0, 40, n).tolist()
    v = rng.integers(0, 300, n).tolist()                       # ties: peers
    table = pa.table({"g": pa.array(g, type=pa.int32()), "v": pa.array(v, type=pa.int64())})
    leaf = P.MemoryExec(DeviceTable.from_arrow(table), "t")
    wexpr = [(("ntile", 4), None, "q", None), ("first_value", col("v"), "lowest", None), ("percent_rank", None, "pr", None)]
    plan = P.FilterExec(col("q").eq(lit(1, pa.uint64())), P.WindowAggExec(wexpr, ["g"], [("v", False, False)], P.SortExec([("g", False, False), ("v", False, False)], leaf)))
    rule = P.GpuOffloadRule()
    opt = rule.optimize(plan)
    assert not rule.declined and [type(x).__name__ for x in (opt, opt.input, opt.input.input)] == ["FilterExec", "WindowAggExec", "SortExec"]
    schema = P.plan_schema(opt.input)
    assert schema.names == ["g", "v", "q", "lowest", "pr"] and schema.types[2:] == [pa.uint64(), pa.int64(), pa.float64()]
    assert [schema.field(k).nullable for k in ("q", "lowest", "pr")] == [False, True, False]
    out = P.collect(opt)
    got = out.to_arrow()
    out.free()
    order = sorted(range(n), key=lambda i: (g[i], v[i]))
    cols = {"g": [g[i] for i in order], "v": [v[i] for i in order]}
    want = V.window(cols, ["g"], ["v"], [(("ntile", 4), None, "q", None), ("first_value", "v", "lowest", None), ("percent_rank", None, "pr", None)])
    keep = [i for i in range(n) if want["q"][i] == 1]
    assert 0 < len(keep) < n
    assert got.column("g").to_pylist() == [cols["g"][i] for i in keep] and got.column("v").to_pylist() == [cols["v"][i] for i in keep]
    assert got.column("q").to_pylist() == [1] * len(keep) and got.column("lowest").to_pylist() == [want["lowest"][i] for i in keep]
    assert _same(got.column("pr").to_pylist(), [want["pr"][i] for i in keep], True)


# ------------------------------------------------------------------------------------------------------------------------- refusals
def _refusal_table():
    return pa.table({"i": pa.array([1, 1, 2], type=pa.int32()), "b": pa.array([True, None, False]), "s": pa.array(["a", "a", "b"]),
                     "x": pa.array([5, None, 7], type=pa.int64())})


@pytest.mark.parametrize("func, arg, message", [
    ("first_value", "b", "FIRST_VALUE(a) over Boolean is not supported on the GPU path"),
    ("last_value", "s", "LAST_VALUE(a) over Utf8 is not supported on the GPU path"),
    (("nth_value", 2), "b", "NTH_VALUE(a) over Boolean is not supported on the GPU path"),
    (("nth_value", -1), "s", "NTH_VALUE(a) over Utf8 is not supported on the GPU path"),
])
def test_boolean_and_utf8_arguments_stay_on_the_cpu_and_the_library_says_the_same(func, arg, message):
    from datafusion_amd import _lib, ops, physical_plan as P
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    dev = DeviceTable.from_arrow(_refusal_table())
    leaf = P.MemoryExec(dev, "t")
    exprs = [(("ntile", 2), None, "q", None), (func, col(arg), "a", "rows_to_current")]
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.WindowAggExec(exprs, ["i"], ["i"], leaf))
    assert isinstance(out, P.WindowAggExec) and getattr(out, "kept_on_cpu", False)
    assert len(rule.declined) == 1 and rule.declined[0][1] == message, rule.declined
    with pytest.raises(_lib.DfgpuError) as err:
        ops.window(dev, ["i"], ["i"], exprs)
    assert str(err.value) == message
    # the same functions over a column the device takes are offloaded, and run
    good = [(("ntile", 2), None, "q", None), (func, col("x"), "a", "partition")]
    rule2 = P.GpuOffloadRule()
    opt = rule2.optimize(P.WindowAggExec(good, ["i"], ["i"], leaf))
    assert not getattr(opt, "kept_on_cpu", False) and not rule2.declined
    res = P.collect(opt)
    cols = {"i": [1, 1, 2], "x": [5, None, 7]}
    want = V.window(cols, ["i"], ["i"], [(("ntile", 2), None, "q", None), (func, "x", "a", "partition")])
    assert res.to_arrow().column("q").to_pylist() == want["q"] and res.to_arrow().column("a").to_pylist() == want["a"]
    res.free()
    dev.free()


def test_the_c_abi_checks_the_parameters_itself():
    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    lib = _lib.init()
    dev = DeviceTable.from_arrow(_refusal_table())
    lowered = ops.lower(col("x"), dev.column_names, dev)

    def call(func, n, has_arg, frame=0):
        spec = _lib.WindowSpec()
        spec.func, spec.has_arg, spec.frame, spec.name, spec.n = func, has_arg, frame, b"a", n
        if has_arg:
            spec.arg = lowered.c
        out = C.c_void_p()
        ops.profile_enable(True)
        ops.profile_reset()
        try:
            rc = lib.dfgpu_window(dev.handle, (C.c_int * 1)(0), 1, (C.c_int * 1)(0), 1, C.byref(spec), 1, C.byref(out))
            ran = {k for k in ops.profile_stats() if k.startswith("window_")}
        finally:
            ops.profile_enable(False)
        if rc == 0:
            t = DeviceTable(out)
            got = t.to_arrow().column("a").to_pylist()
            t.free()
            return None, got, ran
        assert not out.value
        return lib.dfgpu_last_error().decode(), None, ran
    D, VF = ops.WINDOW_DIST_FUNCS, ops.WINDOW_VALUE_FUNCS
    assert call(D["ntile"], 0, 0)[::2] == ("NTILE needs a positive number of buckets", set())
    assert call(D["ntile"], -1, 0)[::2] == ("NTILE needs a positive number of buckets", set())
    assert call(VF["nth_value"], 0, 1)[::2] == ("NTH_VALUE needs a non-zero n", set())
    for name in ("first_value", "last_value", "nth_value"):
        assert call(VF[name], 1, 0)[::2] == (f"{name.upper()} needs an argument", set())
    message, _, ran = call(14, 0, 0)
    assert "14" in message and "dfgpu_window_func" in message and not ran                  # an unknown function: before anything runs
    assert "dfgpu_window_frame" in call(VF["first_value"], 0, 1, frame=3)[0]
    # and what it accepts, through the same door: n is read by NTILE and NTH_VALUE and by nobody else
    assert call(D["ntile"], 2, 0)[1] == [1, 2, 1]
    assert call(D["ntile"], 2**62, 0)[1] == [1, 2, 1]
    assert call(VF["nth_value"], 1, 1, frame=2)[1] == [5, 5, 7] and call(VF["nth_value"], -1, 1, frame=1)[1] == [5, None, 7]
    assert call(VF["first_value"], -99, 1)[1] == [5, 5, 7] and call(D["cume_dist"], -99, 0)[1] == [1.0, 1.0, 1.0]
    assert call(ops.WINDOW_FUNCS["row_number"], -99, 0)[1] == [1, 2, 1]
    dev.free()

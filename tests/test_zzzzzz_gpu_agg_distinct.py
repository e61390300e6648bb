"""COUNT(DISTINCT x) / SUM(DISTINCT x) of the GPU AggregateExec against tests/agg_distinct_ref.py: every value compared exactly, row by
row in first-seen group order, nothing with a tolerance.  tests/test_agg_distinct_reference.py holds that restatement to hand-worked
answers and to the oracle and shows which mistakes its tables catch.

Shapes are the smallest that can still go wrong: row counts around the 64-row words and one block, more groups than the 2 048 LDS
cells, every argument type at its edge values, duplicates that race inside one wave (64 equal rows) and across waves (4 096), a table
that has to grow several times, several updates on one node, the fused node's fallback, every refusal, and the collapsed plan."""
import functools

import pyarrow as pa
import pytest

from tests import agg_distinct_ref as R

pytestmark = pytest.mark.gpu

KERNELS = ("agg_distinct_insert", "agg_distinct_reduce")
ALL_AGGS = [("count_distinct", t, f"cd_{t}", None) for t in R.COUNT_TYPES] + [("sum_distinct", t, f"sd_{t}", None) for t in R.SUM_BITS]
FILTERED = [("count_distinct", t, f"cdp_{t}", "p") for t in ("i64", "dec", "f64", "str")] + [("sum_distinct", t, f"sdp_{t}", "p") for t in ("i32", "u64", "dec")]


def _dev(table, types=None, names=None):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(R.to_arrow(table, types, names))


def _e(aggs):
    from datafusion_amd.expr import col
    return [(f, None if a is None else col(a), n, None if p is None else col(p)) for f, a, n, p in aggs]


def _keys(names):
    from datafusion_amd.expr import col
    return [(col(k), k) for k in names]


def _check(got, keys, aggs, want, types, label=""):
    """got: the device's table; want: the restatement's rows.  Row by row, in first-seen group order, every value equal."""
    names = [a[2] for a in aggs]
    assert got.column_names == list(keys) + names, (label, got.column_names)
    for f, a, n, _ in aggs:
        t = got.schema.field(n).type
        assert t == (pa.int64() if f == "count_distinct" else {"dec": pa.decimal128(38, R.DEC[1]), "u32": pa.uint64(), "u64": pa.uint64()}.get(types[a], pa.int64())), (label, n, t)
    rows = got.to_pylist()
    assert len(rows) == len(want), (label, "group count", len(rows), len(want))
    for i, (g, w) in enumerate(zip(rows, want)):
        g = {c: R.from_arrow_value(v, None) for c, v in g.items()}
        assert all(type(g[c]) is type(w[c]) for c in g), (label, i, g, w)
        assert g == w, f"{label}: row {i}: (got, want) = { {c: (g[c], w[c]) for c in g if g[c] != w[c]} }"


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
def _table(n, groups=7):
    return R.make_table(n, groups=groups)


def _run(table, types, keys, aggs, label, inserts=True, **opts):
    with _profiled(**opts) as ops:
        info = {}
        got = ops.aggregate(_dev(table, types), _keys(keys), _e(aggs), "Single", info=info).to_arrow()
        stats = ops.profile_stats()
    _check(got, keys, aggs, R.aggregate(table, list(keys), aggs, types), types, label)
    assert info["fused_updates"] == 0, (label, info)             # the fused update declines the node
    if inserts:
        _ran(stats, *KERNELS)
    return stats


# ------------------------------------------------------------------------------ 1. every type, the row counts, with and without GROUP BY
@pytest.mark.parametrize("keys", [("k",), ()], ids=["group_by_k", "no_group_by"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4097])
def test_every_argument_type_at_its_edge_values(n, keys):
    table = _table(n)
    _run(table, R.TYPES, keys, ALL_AGGS, f"{n} rows, all types", inserts=n > 0)
    _run(table, R.TYPES, keys, FILTERED, f"{n} rows, filtered", inserts=n > 0)


@pytest.mark.parametrize("keys", [("k",), ()], ids=["group_by_k", "no_group_by"])
def test_a_hundred_thousand_rows(keys):
    aggs = [a for a in ALL_AGGS + FILTERED if a[1] in ("i64", "dec", "f64", "str")]
    _run(_table(100_003), R.TYPES, keys, aggs, "100003 rows")


# ------------------------------------------------------------------------------ 2. duplicates and cardinalities
def _shaped(n, key, value, null_every=0):
    t = {"k": [key(i) for i in range(n)], "i64": [None if null_every and i % null_every == 0 else value(i) for i in range(n)]}
    t["dec"] = [None if v is None else v * (2**64 + 1) for v in t["i64"]]           # both words carry the value
    return t


SHAPES = {
    "64_equal_rows": lambda: _shaped(64, lambda i: 5, lambda i: -9),                                        # one wave, one pair
    "4096_equal_rows": lambda: _shaped(4096, lambda i: 5, lambda i: -9),                                    # many waves, one pair
    "all_rows_distinct": lambda: _shaped(4097, lambda i: i % 7, lambda i: i * 7919 - 2**40),
    "one_value_in_every_group": lambda: _shaped(4097, lambda i: i % 7, lambda i: 42 if i % 2 else i),
    "5000_groups": lambda: _shaped(20_003, lambda i: (i * 31) % 5000 - 2500, lambda i: i % 3, null_every=10),  # more groups than LDS cells
    "5000_groups_all_distinct": lambda: _shaped(20_003, lambda i: (i * 31) % 5000, lambda i: i),
    "one_group": lambda: _shaped(4095, lambda i: 1, lambda i: i % 100, null_every=9),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_duplicates_and_cardinalities(shape):
    table = SHAPES[shape]()
    aggs = [("count_distinct", "i64", "c", None), ("sum_distinct", "i64", "s", None), ("count_distinct", "dec", "cd", None), ("sum_distinct", "dec", "sd", None)]
    _run(table, R.TYPES, ("k",), aggs, shape)
    if shape in ("64_equal_rows", "all_rows_distinct"):
        _run(table, R.TYPES, (), aggs, shape + ", no GROUP BY")


# ------------------------------------------------------------------------------ 3. the group keys' routes
def _key_table(n):
    t = R.make_table(n)
    t["kd"] = [i * 3 % 11 for i in range(n)]                                        # dense Int32: the direct route of lookup_gid
    t["ks"] = [None if i % 13 == 0 else f"key-{i * 5 % 9}" for i in range(n)]       # Utf8, interned on entry
    t["kb"] = [None if i % 17 == 0 else i % 3 == 0 for i in range(n)]               # Boolean
    return t


KEY_TYPES = dict(R.TYPES, kd="i32", ks="str", kb="bool")


@pytest.mark.parametrize("keys", [("kd",), ("k",), ("k", "k2"), ("k2",), ("ks",), ("kb",), ("kb", "ks")], ids=lambda k: "+".join(k))
def test_group_key_routes(keys):
    table = _key_table(4097)
    aggs = [("count_distinct", "i64", "c", None), ("sum_distinct", "u64", "s", "p"), ("count_distinct", "f64", "cf", None), ("count_distinct", "str", "cs", "p")]
    _run(table, KEY_TYPES, keys, aggs, f"keys {keys}")


# ------------------------------------------------------------------------------ 4. strings
def test_a_dictionary_encoded_and_a_plain_utf8_column():
    """through the host import, which takes no dictionary that repeats a value (the device import does: the next test)"""
    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    n = 4097
    values = ["b", "a", "", None, "zz", "c"]                                         # unsorted, the empty string and a NULL value
    codes = [None if i % 10 == 0 else (i * 5) % len(values) for i in range(n)]
    strings = [None if c is None else values[c] for c in codes]
    k = [i % 7 for i in range(n)]
    want = R.aggregate({"k": k, "str": strings}, ["k"], [("count_distinct", "str", "c", None)], R.TYPES)
    assert {r["c"] for r in want} == {5} and len(want) == 7                          # "b", "a", "", "zz", "c"
    encoded = pa.DictionaryArray.from_arrays(pa.array(codes, pa.int32()), pa.array(values, pa.string()))
    with pytest.raises(_lib.DfgpuError, match="duplicate dictionary value"):
        DeviceTable.from_arrow(pa.table({"str": pa.DictionaryArray.from_arrays(pa.array([0, 1, 2], pa.int32()), pa.array(["b", "a", "b"], pa.string()))}))
    for label, column in (("dictionary", encoded), ("plain", pa.array(strings, pa.string()))):
        with _profiled() as o:
            got = o.aggregate(DeviceTable.from_arrow(pa.table({"k": pa.array(k, pa.int64()), "str": column})), _keys(["k"]),
                              [("count_distinct", col("str"), "c")], "Single").to_arrow()
            _ran(o.profile_stats(), *KERNELS)
        assert got.to_pylist() == want, label
    # a second update with another dictionary is refused in the words of the group keys' check; with the same one it is taken
    a = ops.GroupedAggregate("Single", ["k", "str"], _keys(["k"]), [("count_distinct", col("str"), "c")])
    t1 = DeviceTable.from_arrow(pa.table({"k": pa.array(k, pa.int64()), "str": encoded}))
    a.update(t1)
    a.update(t1)
    assert a.emit().to_arrow().to_pylist() == want
    other = pa.DictionaryArray.from_arrays(pa.array([0, 1], pa.int32()), pa.array(["x", "y"], pa.string()))
    with pytest.raises(Exception, match="aggregate c: the dictionary changed between updates"):
        a.update(DeviceTable.from_arrow(pa.table({"k": pa.array([1, 2], pa.int64()), "str": other})))
    a.free()


class _DeviceDictionaryTable:
    """k: Int64, s: Dictionary(Int32, Utf8) in HBM, handed to the library as an ArrowDeviceArray over torch tensors — the Arrow C Device
    import, which takes a producer's dictionary as it is, repeated values included.  Keeps the producer's memory and structs alive."""

    def __init__(self, k, codes, values):
        import ctypes as C

        import numpy as np
        import torch

        from datafusion_amd.table import ARROW_DEVICE_ROCM, ArrowArray, ArrowDeviceArray, ArrowSchema, DeviceTable
        n = len(k)
        bits = lambda flags: np.packbits(np.concatenate([np.asarray(flags, bool), np.zeros((-len(flags)) % 64 + 64, bool)]), bitorder="little").copy()
        raw = [b"" if v is None else v.encode() for v in values]
        offsets = np.cumsum([0] + [len(r) for r in raw]).astype(np.int32)
        host = [np.asarray(k, np.int64), np.asarray([0 if c is None else c for c in codes], np.int32), bits([c is not None for c in codes]),
                bits([v is not None for v in values]), offsets, np.frombuffer(b"".join(raw) + b"\0" * 8, np.uint8).copy()]
        self.dev = [torch.from_numpy(x).to("cuda:0") for x in host]
        torch.cuda.synchronize()
        ptr = [x.data_ptr() for x in self.dev]
        self.released = []
        self._release = C.CFUNCTYPE(None, C.POINTER(ArrowArray))(self._on_release)
        self.keep = k_buf, s_buf, d_buf, root_buf = (C.c_void_p * 2)(None, ptr[0]), (C.c_void_p * 2)(ptr[2], ptr[1]), (C.c_void_p * 3)(ptr[3], ptr[4], ptr[5]), (C.c_void_p * 1)(None)
        self.dict_arr = ArrowArray(length=len(values), null_count=sum(v is None for v in values), offset=0, n_buffers=3, n_children=0, buffers=d_buf)
        self.dict_sch = ArrowSchema(format=b"u", name=b"", flags=2)
        self.kids = [ArrowArray(length=n, null_count=0, offset=0, n_buffers=2, n_children=0, buffers=k_buf),
                     ArrowArray(length=n, null_count=sum(c is None for c in codes), offset=0, n_buffers=2, n_children=0, buffers=s_buf, dictionary=C.pointer(self.dict_arr))]
        self.skids = [ArrowSchema(format=b"l", name=b"k", flags=2), ArrowSchema(format=b"i", name=b"str", flags=2, dictionary=C.pointer(self.dict_sch))]
        self.kid_ptrs = (C.POINTER(ArrowArray) * 2)(*[C.pointer(x) for x in self.kids])
        self.skid_ptrs = (C.POINTER(ArrowSchema) * 2)(*[C.pointer(x) for x in self.skids])
        arr = ArrowDeviceArray(device_id=0, device_type=ARROW_DEVICE_ROCM, sync_event=None)
        arr.array = ArrowArray(length=n, null_count=0, offset=0, n_buffers=1, n_children=2, buffers=root_buf, children=self.kid_ptrs, release=C.cast(self._release, C.c_void_p))
        sch = ArrowSchema(format=b"+s", name=b"", flags=0, n_children=2, children=self.skid_ptrs)
        self.table = DeviceTable.from_device(arr, sch)

    def _on_release(self, a):
        self.released.append(1)
        a.contents.release = None


def test_a_device_dictionary_whose_values_repeat():
    """"b" and "a" have three and two codes, one dictionary value is NULL: the codes are counted after the dictionary has been made unique"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    n = 4097
    values = ["b", "a", "b", "", "a", None, "zz", "b"]
    k = [i % 7 for i in range(n)]
    codes = [None if i % 10 == 0 else (i * 3) % len(values) for i in range(n)]
    strings = [None if c is None else values[c] for c in codes]
    aggs = [("count_distinct", "str", "c", None)]
    want = R.aggregate({"k": k, "str": strings}, ["k"], aggs, R.TYPES)
    by_codes = R.aggregate({"k": k, "str": [None if c is None else str(c) for c in codes]}, ["k"], aggs, R.TYPES)
    assert {r["c"] for r in want} == {4} and {r["c"] for r in by_codes} == {8}          # "b", "a", "", "zz": counting the codes would give 8
    src = _DeviceDictionaryTable(k, codes, values)
    assert src.table.dictionary_size("str") == len(values)                                # the dictionary came in as it is
    with _profiled() as o:
        got = o.aggregate(src.table, _keys(["k"]), [("count_distinct", col("str"), "c")], "Single").to_arrow()
        _ran(o.profile_stats(), *KERNELS)
    assert got.to_pylist() == want
    # several updates with the same dictionary: three thirds of the rows, each arriving through an import of its own
    cuts = [(0, 1500), (1500, 1563), (1563, n)]
    parts = [_DeviceDictionaryTable(k[a:b], codes[a:b], values) for a, b in cuts]
    a = ops.GroupedAggregate("Single", ["k", "str"], _keys(["k"]), [("count_distinct", col("str"), "c")])
    for p in parts:
        a.update(p.table)
    assert a.emit().to_arrow().to_pylist() == want
    # without GROUP BY, and a dictionary that differs only in where it repeats is another dictionary
    (whole,) = ops.aggregate(src.table, [], [("count_distinct", col("str"), "c")], "Single").to_arrow().to_pylist()
    assert whole == {"c": 4}
    other = _DeviceDictionaryTable(k[:10], codes[:10], ["b", "a", "a", "", "a", None, "zz", "b"])
    with pytest.raises(Exception, match="aggregate c: the dictionary changed between updates"):
        a.update(other.table)
    a.free()
    for t in [src, other] + parts:
        t.table.free()


def test_an_empty_first_batch_does_not_bind_a_utf8_argument():
    """an update over no rows, or over rows without a value, leaves nothing counted by a dictionary's codes: the next batch brings its own"""
    from datafusion_amd import ops
    table = _table(4097)
    empty = {c: v[:0] for c, v in table.items()}
    nulls = dict({c: v[:65] for c, v in table.items()}, str=[None] * 65)
    rest = {c: v[65:] for c, v in table.items()}
    aggs = [("count_distinct", "str", "c", None), ("count_distinct", "i64", "ci", "p")]
    for keys in (("k",), ()):
        a = ops.GroupedAggregate("Single", list(table), _keys(keys), _e(aggs))
        for part in (empty, nulls, rest):
            a.update(_dev(part))
        got = a.emit().to_arrow()
        a.free()
        _check(got, keys, aggs, R.aggregate(R.concat([nulls, rest]), list(keys), aggs, R.TYPES), R.TYPES, f"empty first batch, keys {keys}")


# ------------------------------------------------------------------------------ 5. growth
def test_a_small_table_grows_several_times_and_nothing_changes():
    from datafusion_amd import ops
    parts = [_shaped(1000, lambda i: i % 5, lambda i, u=u: (u * 1000 + i) * 3) for u in range(6)]            # all distinct, 6 updates
    whole = R.concat(parts)
    aggs = [("count_distinct", "i64", "c", None), ("sum_distinct", "i64", "s", None), ("count_distinct", "dec", "cd", None), ("sum_distinct", "dec", "sd", None)]
    want = R.aggregate(whole, ["k"], aggs, R.TYPES)
    assert sum(r["c"] for r in want) == 6000
    with _profiled(agg__distinct_slots=64) as o:
        a = ops.GroupedAggregate("Single", list(parts[0]), _keys(["k"]), _e(aggs))
        for p in parts:
            a.update(_dev(p))
        got = a.emit().to_arrow()
        a.free()
        stats = o.profile_stats()
    _check(got, ("k",), aggs, want, R.TYPES, "grown")
    _ran(stats, "agg_distinct_grow", *KERNELS)
    assert stats["agg_distinct_grow"]["calls"] >= 2 * 3, stats["agg_distinct_grow"]                              # two sets, three growths each
    # one update, the derived size: the same values, and nothing to grow
    with _profiled() as o:
        once = o.aggregate(_dev(whole), _keys(["k"]), _e(aggs), "Single").to_arrow()
        assert "agg_distinct_grow" not in o.profile_stats()
    assert once.equals(got)
    # long probe runs: 64 slots for 30 pairs that all start at few slots' distance is what 64 slots and one group give
    small = _shaped(30, lambda i: 0, lambda i: i)
    _run(small, R.TYPES, ("k",), aggs[:2], "64 slots, 30 pairs", agg__distinct_slots=64)


# ------------------------------------------------------------------------------ 6. three updates on one node
def test_three_updates_equal_one_update_over_the_concatenation():
    from datafusion_amd import ops
    base = _table(4097)
    cut = {c: v[:1500] for c, v in base.items()}, {c: v[1500:1563] for c, v in base.items()}, {c: v[1563:] for c, v in base.items()}
    key = lambda g: g * 1000003 - 2 * 1000003                               # (make_table's keys)
    late = {key(3): 1, key(5): 2}                                           # groups that first appear in the second and in the third update
    for u, part in enumerate(cut):
        part["k"] = [key(0) if late.get(k, 0) > u else k for k in part["k"]]
    whole = R.concat(list(cut))
    first_seen = {}
    for u, part in enumerate(cut):
        for k in part["k"]:
            first_seen.setdefault(k, u)
    assert sorted(set(first_seen.values())) == [0, 1, 2]
    aggs = [a for a in ALL_AGGS if a[1] != "str"] + [("count_distinct", "i64", "cdp", "p")]          # (a Utf8 argument takes one update per node)
    with _profiled() as o:
        a = ops.GroupedAggregate("Single", list(whole), _keys(["k"]), _e(aggs))
        for part in cut:
            a.update(_dev(part))
        got = a.emit().to_arrow()
        again = a.emit().to_arrow()                                          # emitting is repeatable: the cells are made from the set each time
        a.free()
        _ran(o.profile_stats(), *KERNELS)
    _check(got, ("k",), aggs, R.aggregate(whole, ["k"], aggs, R.TYPES), R.TYPES, "three updates")
    assert again.equals(got)
    a = ops.GroupedAggregate("Single", list(whole), _keys(["k"]), _e([("count_distinct", "str", "c", None)]))
    a.update(_dev(cut[0]))
    with pytest.raises(Exception, match="aggregate c: the dictionary changed between updates"):
        a.update(_dev(dict(cut[2], str=["another string"] * len(cut[2]["k"]))))
    a.free()


# ------------------------------------------------------------------------------ 7. beside the other aggregates, and under the fused node
def test_one_node_with_plain_and_distinct_aggregates():
    from datafusion_amd.expr import col
    table = _table(4097)
    plain = [("sum", col("i64"), "s"), ("avg", col("i32"), "m"), ("count", col("f64"), "n"), ("count", None, "star")]
    distinct = [("count_distinct", "i64", "cda", None), ("sum_distinct", "i64", "sda", None), ("count_distinct", "u32", "cdb", "p")]
    for keys in (("k",), ()):
        with _profiled() as o:
            both = o.aggregate(_dev(table), _keys(keys), plain + _e(distinct), "Single").to_arrow()
            _ran(o.profile_stats(), *KERNELS)
            assert o.profile_stats()["agg_distinct_insert"]["calls"] == 2                      # cda and sda share one set
            alone = o.aggregate(_dev(table), _keys(keys), plain, "Single").to_arrow()
        for c in list(keys) + [p[2] for p in plain]:
            assert both.column(c).equals(alone.column(c)) and both.schema.field(c) == alone.schema.field(c), c
        _check(both.select(list(keys) + [d[2] for d in distinct]), keys, distinct, R.aggregate(table, list(keys), distinct, R.TYPES), R.TYPES, "mixed node")


def test_the_fused_node_with_a_predicate_falls_back():
    from datafusion_amd.expr import col, lit
    table = _table(4097)
    kept = [i for i, v in enumerate(table["i32"]) if v is not None and v > 0]
    filtered = {c: [v[i] for i in kept] for c, v in table.items()}
    assert 0 < len(kept) < 4097
    aggs = [("count_distinct", "i64", "c", None), ("sum_distinct", "dec", "s", "p"), ("count_distinct", "str", "cs", None)]
    for keys in (("k",), ()):
        with _profiled() as o:
            info = {}
            got = o.aggregate(_dev(table), _keys(keys), _e(aggs), "Single", predicate=col("i32") > lit(0, pa.int32()), info=info).to_arrow()
            _ran(o.profile_stats(), *KERNELS)
        assert info["fused_updates"] == 0
        _check(got, keys, aggs, R.aggregate(filtered, list(keys), aggs, R.TYPES), R.TYPES, "fused node")


# ------------------------------------------------------------------------------ 8. refusals, in the library's words, and the rule
def test_every_refusal_by_its_message_and_the_rule_keeps_the_plan_on_the_cpu():
    from datafusion_amd import _lib, ops, physical_plan as P
    from datafusion_amd.expr import col, lit
    table = _table(65)
    table = dict(table, b=[None if p is None else not p for p in table["p"]])
    types = dict(R.TYPES, b="bool")
    dev = _dev(table, types)
    leaf = P.MemoryExec(dev, "t")
    cases = [("Single", ("sum_distinct", col("f64"), "x"), "SUM(DISTINCT) over Float64 is not supported on the GPU path"),
             ("Single", ("count_distinct", col("b"), "x"), "COUNT(DISTINCT) over Boolean is not supported on the GPU path"),
             ("SinglePartitioned", ("sum_distinct", col("b"), "x"), "SUM(DISTINCT) over Boolean is not supported on the GPU path"),
             ("Single", ("sum_distinct", col("str"), "x"), "SUM(DISTINCT) over Utf8 is not supported on the GPU path"),
             ("Single", ("sum_distinct", col("d32"), "x"), "SUM(DISTINCT) over Date32 is not supported on the GPU path"),
             ("Single", ("count_distinct", None, "x"), "COUNT(DISTINCT) (aggregate x) needs an argument"),
             ("Single", ("sum_distinct", None, "x"), "SUM(DISTINCT) (aggregate x) needs an argument")]
    for mode in ("Partial", "Final", "FinalPartitioned", "PartialReduce"):
        cases.append((mode, ("count_distinct", col("i64"), "x"), f"COUNT(DISTINCT) (aggregate x) is not supported in mode {mode} on the GPU path: its partial state is a List column"))
        cases.append((mode, ("sum_distinct", col("i64"), "x", col("p")), f"SUM(DISTINCT) (aggregate x) is not supported in mode {mode} on the GPU path: its partial state is a List column"))
    for mode, agg, message in cases:
        with pytest.raises(_lib.DfgpuError) as err:
            ops.aggregate(dev, _keys(["k"]), [("count", None, "n"), agg], mode)
        assert message in str(err.value), (mode, agg, str(err.value))
        rule = P.GpuOffloadRule(world_size=2)                                # (two ranks: nothing is collapsed, every node is asked by itself)
        out = rule.optimize(P.AggregateExec(mode, _keys(["k"]), [("count", None, "n"), agg], leaf))
        assert type(out) is P.AggregateExec and getattr(out, "kept_on_cpu", False) and rule.declined == [(out, message)], (mode, agg, rule.declined)
    # on one rank a Single node is asked the same way
    rule = P.GpuOffloadRule()
    out = rule.optimize(P.AggregateExec("Single", _keys(["k"]), [cases[0][1]], leaf))
    assert getattr(out, "kept_on_cpu", False) and rule.declined == [(out, cases[0][2])]
    # grouping sets
    with pytest.raises(_lib.DfgpuError, match=r"grouping sets: COUNT\(DISTINCT\) \(aggregate x\) is not supported on the GPU path"):
        ops.aggregate_grouping_sets(dev, _keys(["k", "k2"]), [lit(None, pa.int64()), lit(None, pa.int32())], [[False, False], [False, True]],
                                    [("count_distinct", col("i64"), "x")])
    # and the node beside them is untouched: the accepted spelling still runs
    _run(table, types, ("k",), [("count_distinct", "i64", "c", None)], "after the refusals")


# ------------------------------------------------------------------------------ 9. the collapsed plan
def test_the_collapsed_plan_runs_through_collect():
    from datafusion_amd import physical_plan as P
    from datafusion_amd.expr import col, lit
    table = _table(4097)
    leaf = P.MemoryExec(_dev(table), "t")
    proj = P.ProjectionExec([(col("k"), "k"), (col("i64"), "a"), (col("u32"), "u"), (col("i32"), "w"), (col("p"), "p")],
                            P.FilterExec(col("i32") > lit(0, pa.int32()), leaf))
    aggs = [("sum", col("u"), "s"), ("avg", col("w"), "m"), ("count_distinct", col("a"), "d", col("p")), ("sum_distinct", col("u"), "sd")]
    partial = P.AggregateExec("Partial", [(col("k"), "k")], aggs, proj)
    final = P.AggregateExec("FinalPartitioned", [(col("k"), "k")], [(a[0], col(a[2]), a[2]) for a in aggs], P.CoalesceBatchesExec(P.RepartitionExec(partial, ["k"], 4)))
    rule = P.GpuOffloadRule()
    plan = rule.optimize(final)
    assert type(plan) is P.GpuFusedAggregateExec and plan.mode == "Single" and not rule.declined
    with _profiled() as o:
        got = P.collect(plan).to_arrow()
        _ran(o.profile_stats(), *KERNELS)
    kept = [i for i, v in enumerate(table["i32"]) if v is not None and v > 0]
    filtered = {c: [v[i] for i in kept] for c, v in table.items()}
    distinct = [("count_distinct", "i64", "d", "p"), ("sum_distinct", "u32", "sd", None)]
    assert got.column_names == ["k", "s", "m", "d", "sd"]
    _check(got.select(["k", "d", "sd"]), ("k",), distinct, R.aggregate(filtered, ["k"], distinct, R.TYPES), R.TYPES, "collapsed plan")
    # the plain aggregates of the node are those of the same plan without the DISTINCT ones
    plain = P.collect(P.GpuOffloadRule().optimize(P.AggregateExec("Single", [(col("k"), "k")], aggs[:2], proj))).to_arrow()
    assert got.select(["k", "s", "m"]).equals(plain)

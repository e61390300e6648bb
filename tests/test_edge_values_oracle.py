"""The oracle at the edges of its value types, against plain Python exact arithmetic: every GPU edge-value test
(tests/test_gpu_edge_values.py) compares the device with the oracle, so the oracle is checked first.  Floats are held to their bit
patterns: f64::total_cmp orders -NaN < -inf < -0.0 < +0.0 < +inf < +NaN; integers and decimals wrap as add_wrapping does."""
import math

import numpy as np
import pyarrow as pa
import pytest

from oracle import oracle
from tests import edge_values as E
from tests import partition_cases as PC

def total_key(bits: int) -> int:
    """f64::total_cmp as an integer key: positive floats by their bits, negative ones reversed below them (-0.0 just below +0.0)"""
    return bits if bits < 2**63 else -(bits - 2**63) - 1


def raw_of(arr: pa.Array) -> list:
    """raw integers of a column as edge_values builds them (None for NULL): float bits, day numbers, unscaled decimals"""
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    valid = arr.is_valid().to_pylist()
    t = arr.type
    if pa.types.is_float64(t):
        vals = [int(b) for b in np.frombuffer(arr.buffers()[1], np.uint64, len(arr) + arr.offset)[arr.offset:]]
    elif pa.types.is_decimal128(t):
        w = np.frombuffer(arr.buffers()[1], np.uint64, 2 * (len(arr) + arr.offset))[2 * arr.offset:].reshape(-1, 2)
        vals = [E.unscaled(int(lo), int(hi)) for lo, hi in w]
    elif pa.types.is_date32(t):
        vals = arr.cast(pa.int32()).to_pylist()
    else:
        vals = arr.to_pylist()
    return [v if ok else None for v, ok in zip(vals, valid)]


def order_key(typ):
    return total_key if pa.types.is_float64(typ) else (lambda v: v)


SORT_TYPES = [pa.int32(), pa.int64(), pa.date32(), pa.uint32(), pa.uint64(), pa.float64()] + [pa.decimal128(p, 0) for p in E.DECIMAL_PRECISIONS]


@pytest.mark.parametrize("typ", SORT_TYPES, ids=str)
@pytest.mark.parametrize("desc, nulls_first", [(False, False), (False, True), (True, False), (True, True)])
def test_sort_follows_the_total_order(typ, desc, nulls_first):
    rng = np.random.default_rng(SORT_TYPES.index(typ) * 4 + 2 * desc + nulls_first)
    n = 600
    t = pa.table({"k": E.edge_array(rng, n, typ, 0.5, 0.1), "row": pa.array(np.arange(n, dtype=np.int64))})
    got = oracle.sort(t, [("k", desc, nulls_first)]).column("row").to_pylist()
    key, raw = order_key(typ), raw_of(t.column("k"))
    # stable: equal keys keep their input order; NULLs placed by nulls_first whatever the direction
    nulls = [i for i in range(n) if raw[i] is None]
    vals = sorted((i for i in range(n) if raw[i] is not None), key=lambda i: -key(raw[i]) if desc else key(raw[i]))
    want = nulls + vals if nulls_first else vals + nulls
    assert got == want


def test_sort_places_nan_by_its_sign_and_unsigned_above_2_63():
    bits = [E.QNAN_BITS, E.f64_bits(0.0), E.NEG_QNAN_BITS, E.f64_bits(-0.0), E.f64_bits(math.inf), E.f64_bits(-math.inf), E.f64_bits(-1.0)]
    t = pa.table({"f": E.from_raw(bits, pa.float64()), "u": E.from_raw([2**63, 1, 2**64 - 1, 0, 2**63 - 1, 5, 2**63 + 1], pa.uint64())})
    got = raw_of(oracle.sort(t, [("f", False, False)]).column("f"))
    assert got == [E.NEG_QNAN_BITS, E.f64_bits(-math.inf), E.f64_bits(-1.0), E.f64_bits(-0.0), E.f64_bits(0.0), E.f64_bits(math.inf), E.QNAN_BITS]
    assert oracle.sort(t, [("u", False, False)]).column("u").to_pylist() == [0, 1, 5, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1]


CMP_OPS = {"=": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
           ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}


@pytest.mark.parametrize("typ", [pa.int64(), pa.uint32(), pa.uint64(), pa.float64(), pa.decimal128(38, 0), pa.date32()], ids=str)
@pytest.mark.parametrize("op", list(CMP_OPS))
def test_comparisons_follow_the_total_order(typ, op):
    """arrow-ord's cmp kernels: floats by totalOrder (NaN = NaN, -0.0 < +0.0), unsigned values as unsigned; NULL rows drop"""
    rng = np.random.default_rng(len(op) * 7 + len(str(typ)))
    n = 800
    t = pa.table({"a": E.edge_array(rng, n, typ, 0.6, 0.05), "b": E.edge_array(rng, n, typ, 0.6, 0.05), "row": pa.array(np.arange(n))})
    got = oracle.filter(t, ("bin", op, ("col", "a"), ("col", "b")), ["row"]).column("row").to_pylist()
    key, ra, rb = order_key(typ), raw_of(t.column("a")), raw_of(t.column("b"))
    want = [i for i in range(n) if ra[i] is not None and rb[i] is not None and CMP_OPS[op](key(ra[i]), key(rb[i]))]
    assert got == want


def test_float_comparison_known_answers():
    bits = [E.QNAN_BITS, E.NEG_QNAN_BITS, E.f64_bits(-0.0), E.f64_bits(0.0)]
    t = pa.table({"a": E.from_raw(bits, pa.float64()), "b": E.from_raw([E.QNAN_BITS, E.QNAN_BITS, E.f64_bits(0.0), E.f64_bits(-0.0)], pa.float64()),
                  "row": pa.array([0, 1, 2, 3])})
    assert oracle.filter(t, ("bin", "=", ("col", "a"), ("col", "b")), ["row"]).column("row").to_pylist() == [0]      # NaN = NaN; -NaN != +NaN
    assert oracle.filter(t, ("bin", "<", ("col", "a"), ("col", "b")), ["row"]).column("row").to_pylist() == [1, 2]   # -NaN < NaN, -0.0 < 0.0


def _wrap(v, typ):
    """two's complement wrap of an exact sum into the accumulator's width (add_wrapping)"""
    bits = 128 if pa.types.is_decimal128(typ) else 64
    v &= (1 << bits) - 1
    return v - (1 << bits) if (not pa.types.is_unsigned_integer(typ) and v >= 1 << (bits - 1)) else v


AGG_TYPES = [pa.int32(), pa.int64(), pa.uint32(), pa.uint64(), pa.decimal128(18, 0), pa.decimal128(38, 0), pa.float64()]


@pytest.mark.parametrize("typ", AGG_TYPES, ids=str)
def test_sum_min_max_count_against_exact_arithmetic(typ):
    rng = np.random.default_rng(len(str(typ)))
    n = 3000
    g = rng.integers(0, 40, n).astype(np.int32)
    t = pa.table({"g": pa.array(g), "x": E.edge_array(rng, n, typ, 0.4, 0.1)})
    aggs = [("sum", ("col", "x"), "s"), ("min", ("col", "x"), "lo"), ("max", ("col", "x"), "hi"), ("count", ("col", "x"), "c")]
    if pa.types.is_float64(typ):
        aggs = aggs[1:]    # float SUM rounds: test_float_sum_specials
    out = oracle.aggregate(t, [(("col", "g"), "g")], aggs)
    raw = raw_of(t.column("x"))
    key = order_key(typ)
    sum_t = oracle.sum_result_type(typ)
    res = {name: (raw_of(out.column(name)) if name in ("lo", "hi") or pa.types.is_float64(typ) else out.column(name).to_pylist()) for _, _, name in aggs}
    if "s" in res:
        res["s"] = raw_of(out.column("s"))
    for r, gv in enumerate(out.column("g").to_pylist()):
        vals = [raw[i] for i in range(n) if g[i] == gv and raw[i] is not None]
        assert res["c"][r] == len(vals)
        if not vals:
            assert all(res[k][r] is None for k in res if k != "c")
            continue
        if "s" in res:
            assert out.schema.field("s").type == sum_t
            assert res["s"][r] == _wrap(sum(vals), sum_t), (gv, vals)
        assert res["lo"][r] == min(vals, key=key) and res["hi"][r] == max(vals, key=key), (gv, vals)


def test_sum_wraps_like_add_wrapping():
    t = pa.table({"i": pa.array([E.I64_MAX, 1, 5], pa.int64()), "u": pa.array([2**64 - 1, 2, 0], pa.uint64()),
                  "d": E.from_raw([10**38 - 1, 10**38 - 1, 0], pa.decimal128(38, 0))})
    out = oracle.aggregate(t, [], [("sum", ("col", c), c) for c in "iud"])
    assert out.column("i").to_pylist() == [E.I64_MIN + 5]
    assert out.column("u").to_pylist() == [1]
    assert raw_of(out.column("d")) == [_wrap(2 * (10**38 - 1), pa.decimal128(38, 0))]


def test_min_max_follow_the_total_order():
    """MAX over values that include NaN is NaN, MIN(-0.0, 0.0) is -0.0, MIN over a negative NaN is that NaN, whatever the row order"""
    cases = [([0.0, -0.0], -0.0, 0.0), ([-0.0, 0.0], -0.0, 0.0), ([1.0, float("nan"), 2.0], 1.0, "nan"), ([math.inf, 3.0], 3.0, math.inf),
             ([-math.inf, E.f64_from_bits(E.NEG_QNAN_BITS), 7.0], "-nan", 7.0), ([math.inf], math.inf, math.inf),
             ([E.f64_from_bits(E.PAYLOAD_NAN_BITS)], "payload", "payload")]
    named = {"nan": E.QNAN_BITS, "-nan": E.NEG_QNAN_BITS, "payload": E.PAYLOAD_NAN_BITS}
    bits, gids = [], []
    for gi, (xs, _, _) in enumerate(cases):
        for x in xs:
            bits.append(named["-nan"] if (isinstance(x, float) and math.isnan(x) and math.copysign(1, x) < 0) else
                        named["payload"] if x is not None and E.f64_bits(x) == E.PAYLOAD_NAN_BITS else
                        named["nan"] if math.isnan(x) else E.f64_bits(x))
            gids.append(gi)
    t = pa.table({"g": pa.array(gids, pa.int32()), "x": E.from_raw(bits, pa.float64())})
    out = oracle.aggregate(t, [(("col", "g"), "g")], [("min", ("col", "x"), "lo"), ("max", ("col", "x"), "hi")])
    want = lambda v: named[v] if isinstance(v, str) else E.f64_bits(v)
    assert raw_of(out.column("lo")) == [want(lo) for _, lo, _ in cases]
    assert raw_of(out.column("hi")) == [want(hi) for _, _, hi in cases]


def test_float_sum_specials():
    """SUM over Float64 starts at +0.0 (sum.rs: the accumulator's default): SUM(-0.0) is +0.0; inf + -inf and NaN give NaN"""
    groups = [[-0.0], [-0.0, -0.0], [math.inf, 1.0], [math.inf, -math.inf], [float("nan"), 2.0], [-math.inf, -1.0], [0.5, 0.25]]
    t = pa.table({"g": pa.array([i for i, xs in enumerate(groups) for _ in xs], pa.int32()), "x": pa.array([x for xs in groups for x in xs], pa.float64())})
    out = oracle.aggregate(t, [(("col", "g"), "g")], [("sum", ("col", "x"), "s")])
    got = raw_of(out.column("s"))
    assert got[:3] == [E.f64_bits(0.0), E.f64_bits(0.0), E.f64_bits(math.inf)]
    assert math.isnan(E.f64_from_bits(got[3])) and math.isnan(E.f64_from_bits(got[4]))
    assert got[5:] == [E.f64_bits(-math.inf), E.f64_bits(0.75)]


def test_group_keys_are_equal_by_their_bits():
    """-0.0 and +0.0 are two groups, so are +NaN and -NaN and a NaN with another payload; equal bits are one group"""
    bits = [E.f64_bits(0.0), E.f64_bits(-0.0), E.QNAN_BITS, E.NEG_QNAN_BITS, E.PAYLOAD_NAN_BITS, E.f64_bits(0.0), E.QNAN_BITS, E.f64_bits(-0.0)]
    t = pa.table({"k": E.from_raw(bits, pa.float64()), "x": pa.array(range(8), pa.int64())})
    out = oracle.aggregate(t, [(("col", "k"), "k")], [("count", None, "c"), ("sum", ("col", "x"), "s")])
    assert raw_of(out.column("k")) == bits[:5]
    assert out.column("c").to_pylist() == [2, 2, 2, 1, 1]
    assert out.column("s").to_pylist() == [0 + 5, 1 + 7, 2 + 6, 3, 4]


@pytest.mark.parametrize("typ", [pa.float64(), pa.uint64(), pa.int64(), pa.decimal128(38, 0)], ids=str)
def test_group_keys_at_the_edges(typ):
    rng = np.random.default_rng(3)
    t = pa.table({"k": E.edge_array(rng, 2000, typ, 0.5, 0.05), "x": pa.array(np.ones(2000, np.int64))})
    out = oracle.aggregate(t, [(("col", "k"), "k")], [("count", None, "c")])
    raw = raw_of(t.column("k"))
    first, counts = {}, {}
    for v in raw:
        first.setdefault(v, len(first))
        counts[v] = counts.get(v, 0) + 1
    assert raw_of(out.column("k")) == list(first)       # first-seen order, one group per distinct bit pattern / value, NULL one group
    assert out.column("c").to_pylist() == [counts[v] for v in first]


def test_hash_routing_follows_the_float_bits():
    """hash_utils.rs hashes a float by its bits (hash_float_value): the hash of a Float64 value is the hash of the UInt64 with the same
    bits, -0.0 and +0.0 hash apart, and so do the two NaN signs"""
    bits = E.F64_EDGE_BITS
    f = oracle.create_hashes([E.from_raw(bits, pa.float64())], 0)
    u = oracle.create_hashes([pa.array(bits, pa.uint64())], 0)
    assert list(f) == list(u)
    assert f[0] != f[1] and f[4] != f[5]
    # routing = hash % partitions, rows of one bit pattern always together
    rng = np.random.default_rng(9)
    t = pa.table({"k": E.edge_array(rng, 3000, pa.float64(), 0.5, 0.05)})
    for nparts in (1, 3, 16):
        _, part = oracle.hash_partition(t, ["k"], nparts)
        hashes = oracle.create_hashes([t.column("k")], 0)
        raw = raw_of(t.column("k"))
        for i in range(t.num_rows):
            assert part[i] == (0 if raw[i] is None else int(hashes[i]) % nparts)


_ROUTING = {}


def _routing_reference():
    """the edge-value table of the check above with a second, Int64 key (NULLs in both), and the hashes of its rows over one key and
    over both in Python integers (tests/partition_cases.py row_hashes), made once"""
    if not _ROUTING:
        rng = np.random.default_rng(9)
        t = pa.table({"k": E.edge_array(rng, 3000, pa.float64(), 0.5, 0.05), "k2": E.edge_array(rng, 3000, pa.int64(), 0.5, 0.05)})
        raws, types = [raw_of(t.column("k")), raw_of(t.column("k2"))], [pa.float64(), pa.int64()]
        assert None in raws[0] and None in raws[1] and any(a is None and b is None for a, b in zip(*raws))
        _ROUTING.update(table=t, one=PC.row_hashes(raws[:1], types[:1]), two=PC.row_hashes(raws, types))
    return _ROUTING


@pytest.mark.parametrize("nparts", PC.ALL_COUNTS)
def test_hash_routing_is_the_hash_modulo_every_partition_count(nparts):
    """every count the device partitions into (1..64; tests/test_gpu_partition.py compares with the oracle at each of them): a row goes
    to hash % nparts as Python integers compute it, over one key and over two, a NULL key leaving the hash as it was (0 for a row of NULLs
    only); the partitions hold their rows in input order"""
    ref = _routing_reference()
    t = ref["table"]
    for keys, hashes in ((["k"], ref["one"]), (["k", "k2"], ref["two"])):
        parts, part = oracle.hash_partition(t, keys, nparts)
        assert [int(h) for h in oracle.create_hashes([t.column(k) for k in keys], 0)] == hashes
        assert part.tolist() == [h % nparts for h in hashes]
        assert len(parts) == nparts and sum(p.num_rows for p in parts) == t.num_rows
        for p, tab in enumerate(parts):
            E.assert_exact(tab, t.take(pa.array([i for i, h in enumerate(hashes) if h % nparts == p], pa.int64())), ordered=True)


@pytest.mark.parametrize("kind", list(PC.KEY_KINDS))
def test_hashes_of_every_partition_key_kind_in_python_integers(kind):
    """the key kinds of the partition tests: signed 32-bit values hash as their sign-extended 64-bit word, unsigned ones zero-extended,
    floats by their bits, a Decimal128 by both words, a second key re-seeds with the first one's hash.  The columns carry the values
    the tests name: UInt64 at and above 2^63, both zeros and both NaN signs"""
    t, keys = PC.key_table(kind, PC.N)
    types = [typ for _, typ, _ in PC.KEY_KINDS[kind]]
    raws = [raw_of(t.column(k)) for k in keys]
    assert [int(h) for h in oracle.create_hashes([t.column(k) for k in keys], 0)] == PC.row_hashes(raws, types)
    assert (None in raws[0]) == (kind == "int64_nullable")
    if kind == "uint64":
        assert {2**63, 2**64 - 1} <= set(raws[0])
    if kind == "float64":
        assert {E.f64_bits(0.0), E.f64_bits(-0.0), E.QNAN_BITS, E.NEG_QNAN_BITS} <= set(raws[0])
    for nparts in (3, 17, 64):
        assert PC.reference(t, keys, nparts)[1].tolist() == [h % nparts for h in PC.row_hashes(raws, types)]


def test_partition_cases_are_the_shapes_they_claim():
    """the case lists of tests/partition_cases.py: the sizes around one tile, the table that needs a second trip through the tile loop,
    the column counts on both sides of a scatter launch, and view tables whose partitions start off every 16-byte boundary"""
    assert PC.N == 4099 and PC.N % 4 == 3 and PC.TWO_TRIPS == 2048 * 1024 + 1025
    assert PC.ceil_div(PC.TWO_TRIPS, PC.TILE) == PC.TILE_GRID + 2 and PC.ceil_div(PC.TWO_TRIPS - PC.TILE - 1, PC.TILE) == PC.TILE_GRID
    cases = PC.kind_cases()
    assert len(cases) == len(set(cases)) == 5 * 56 + 5 * 21
    for kind in PC.KEY_KINDS:
        assert {(p, n) for k, p, n in cases if k == kind} >= {(p, PC.N) for p in PC.KERNEL_COUNTS} | {(p, n) for p in (3, 17) for n in PC.SIZES}
    for ncols, key_last in PC.WIDE_CASES:
        t = PC.wide_table(ncols, key_last)
        assert t.num_columns == ncols and t.column_names.index("k") == (ncols - 1 if key_last else 0)
        assert {f.type.bit_width // 8 for f in t.schema} == {1, 4, 8, 16}
    for name, sizes in PC.VIEW_SIZES.items():
        t = PC.view_source(name)
        exp, part = PC.reference(t, [PC.VIEW_KEY], 3)
        assert [e.num_rows for e in exp] == list(sizes)
        for e in exp[1:]:      # (the views used) input order is kept, so the ascending columns still ascend, densely enough for the one-pass rank map
            for c in ("a64", "a32"):
                a = np.asarray(e.column(c)).astype(np.int64)
                assert (np.diff(a) > 0).all() and len(a) >= 0.15 * (a[-1] - a[0] + 1)
    s = PC.VIEW_SIZES
    assert s["odd"][0] % 2 == 1 and (s["odd"][0] + s["odd"][1]) % 2 == 1
    assert s["mod4"][0] % 4 == 1 and (s["mod4"][0] + s["mod4"][1]) % 4 == 2
    assert s["blocks"][1] == s["blocks"][2] == 2 * 4096 + 3 and s["blocks"][0] % 2 == 1


def test_byte_hash_of_string_keys_known_answers():
    """strings.hip hash_bytes as tests/partition_cases.py restates it: the length seeds it, whole little-endian words first, a partial
    last word zero-padded and marked, so "12345678" and "123456789" and a prefix with a trailing NUL differ"""
    h = PC.hash_bytes
    assert h(b"") == PC.fmix64(PC.SEED_BYTES)
    assert h(b"a") == PC.fmix64(PC.fmix64(1 ^ PC.SEED_BYTES) ^ 0x61 ^ PC.GOLDEN)
    assert h(b"12345678") == PC.fmix64(PC.fmix64(8 ^ PC.SEED_BYTES) ^ int.from_bytes(b"12345678", "little"))
    assert len({h(b"12345678"), h(b"123456789"), h(b"a"), h(b"a\0"), h(b"")}) == 5
    t = PC.odd_key_table("utf8")
    exp, part = PC.reference(t, ["k"], 17)
    home = {}
    for s, p in zip(t.column("k").to_pylist(), part.tolist()):
        assert home.setdefault(s, p) == p
    assert home[None] == 0 and len(set(home.values())) > 3


def test_span_columns_have_the_exact_span():
    rng = np.random.default_rng(1)
    for typ in (pa.int64(), pa.uint64()):
        for span in E.spans():
            a = E.span_raw(rng, 50, typ, span)
            assert max(a) - min(a) == span and E.type_range(typ)[0] <= min(a) and max(a) <= E.type_range(typ)[1]
    full = E.span_raw(rng, 50, pa.int64(), 2**64 - 1)
    assert min(full) == E.I64_MIN and max(full) == E.I64_MAX


def test_edge_columns_carry_every_edge():
    rng = np.random.default_rng(2)
    for typ in SORT_TYPES:
        arr = E.edge_array(rng, 200, typ, 0.1)
        assert set(E.edges_of(typ)) <= set(raw_of(arr))
    assert E.decimal_edges(19) == sorted({0, 10**19 - 1, -(10**19 - 1), 2**63 - 1, -(2**63 - 1), 2**63, -2**63})


def test_exact_helper_sees_bits_and_signed_zeros():
    a = pa.table({"f": E.from_raw([E.f64_bits(0.0), E.QNAN_BITS], pa.float64())})
    b = pa.table({"f": E.from_raw([E.f64_bits(-0.0), E.NEG_QNAN_BITS], pa.float64())})
    with pytest.raises(AssertionError):
        E.assert_exact(a, b, ordered=True)
    with pytest.raises(AssertionError):                   # as a computed value: the zero's sign still counts
        E.assert_exact(a, b, ordered=True, computed=("f",))
    c = pa.table({"f": E.from_raw([E.f64_bits(0.0), E.NEG_QNAN_BITS], pa.float64())})
    E.assert_exact(a, c, ordered=True, computed=("f",))  # computed NaN matches NaN
    E.assert_exact(a, a.take([1, 0]), ordered=False)
    with pytest.raises(AssertionError):
        E.assert_exact(a, a.take([1, 0]), ordered=True)

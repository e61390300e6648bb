"""Edge-value columns and an exact comparison for the edge-value tests (tests/test_edge_values_oracle.py, tests/test_gpu_edge_values.py).

The kernels turn values into encoded keys (order-preserving float keys, mixed-radix sort keys, key ranges of joins and aggregates), and
each encoding has a boundary: the extremes of a type, the sign bit of a float, a span of 2^k.  `edge_array` mixes ordinary random
values with those edges at a chosen fraction; `span_array` builds a key column whose max - min is exactly a given span.
`assert_exact` compares floats an operator only moves or selects by bit pattern (NaN sign and payload, the sign of zero), and
floats it computes by value with NaN = NaN, exact infinities and signed zeros."""
import math
import struct

import numpy as np
import pyarrow as pa

REL = 1e-6    # the suite's relative tolerance for computed floats

I32_MIN, I32_MAX = -2**31, 2**31 - 1
I64_MIN, I64_MAX = -2**63, 2**63 - 1
DBL_MAX = 1.7976931348623157e308


def f64_from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b & (2**64 - 1)))[0]


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


QNAN_BITS, NEG_QNAN_BITS, PAYLOAD_NAN_BITS = 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF800000000BEEF
F64_EDGE_BITS = [f64_bits(x) for x in (0.0, -0.0, math.inf, -math.inf)] + [QNAN_BITS, NEG_QNAN_BITS, PAYLOAD_NAN_BITS] + \
    [f64_bits(x) for x in (5e-324, -5e-324, DBL_MAX, -DBL_MAX, 1.0, math.nextafter(1.0, 2.0), math.nextafter(1.0, 0.0))]

INT_EDGES = {
    pa.int32(): [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX],
    pa.int64(): [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX],
    pa.date32(): [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX],
    pa.uint32(): [0, 2**31 - 1, 2**31, 2**32 - 1],
    pa.uint64(): [0, 2**63 - 1, 2**63, 2**64 - 1],
}
DECIMAL_PRECISIONS = (9, 18, 19, 38)


def decimal_edges(precision: int) -> list:
    """unscaled edges of Decimal128(precision, s) that the precision can hold: ±(10^p - 1), ±(2^63 - 1), ±2^63, ±2^64, 0"""
    top = 10**precision - 1
    mags = [top, 2**63 - 1, 2**63, 2**64]
    return sorted({0} | {s * m for m in mags if m <= top for s in (1, -1)})


def edges_of(typ: pa.DataType) -> list:
    """the edge values of a type as raw integers: values, unscaled decimals, day numbers, or float bit patterns"""
    if pa.types.is_float64(typ):
        return list(F64_EDGE_BITS)
    if pa.types.is_decimal128(typ):
        return decimal_edges(typ.precision)
    return list(INT_EDGES[typ])


def _ordinary(rng, n, typ):
    """the ordinary values beside the edges, as raw integers (Float64: small dyadic values, whose sums are exact in any order)"""
    if pa.types.is_float64(typ):
        return [f64_bits(float(v) / 8.0) for v in rng.integers(-8000, 8000, n)]
    if pa.types.is_unsigned_integer(typ):
        return [int(v) for v in rng.integers(0, 1000, n)]
    return [int(v) for v in rng.integers(-1000, 1000, n)]


def unscaled(lo: int, hi: int) -> int:
    """the signed 128-bit integer of a Decimal128 value's two little-endian words"""
    v = lo | hi << 64
    return v - 2**128 if v >= 2**127 else v


def from_raw(raw, typ: pa.DataType, mask=None) -> pa.Array:
    """an Arrow array of `typ` from raw integers (values, day numbers, unscaled decimals, float bit patterns), bit-exact"""
    n = len(raw)
    valid = None if mask is None else ~np.asarray(mask, dtype=bool)
    if pa.types.is_decimal128(typ):
        words = np.empty((n, 2), np.uint64)
        for i, v in enumerate(raw):
            u = v & (2**128 - 1)
            words[i, 0], words[i, 1] = u & (2**64 - 1), u >> 64
        data = words
    elif pa.types.is_float64(typ):
        data = np.array(raw, dtype=np.uint64)
    else:
        width = {pa.int32(): np.int32, pa.date32(): np.int32, pa.int64(): np.int64, pa.uint32(): np.uint32, pa.uint64(): np.uint64}[typ]
        data = np.array(raw, dtype=object).astype(width)
    vbuf, nulls = None, 0
    if valid is not None and not valid.all():
        vbuf = pa.py_buffer(np.packbits(valid.astype(np.uint8), bitorder="little").tobytes())
        nulls = int(n - valid.sum())
    return pa.Array.from_buffers(typ, n, [vbuf, pa.py_buffer(np.ascontiguousarray(data).tobytes())], null_count=nulls)


def edge_raw(rng, n, typ, edge_frac=0.25, edges=None) -> list:
    """n raw values: each one an edge of the type with probability edge_frac, an ordinary value otherwise; every edge appears at least
    once when n allows (so a small column still crosses every boundary)"""
    edges = edges_of(typ) if edges is None else list(edges)
    raw = _ordinary(rng, n, typ)
    pick = rng.random(n) < edge_frac
    which = rng.integers(0, len(edges), n)
    for i in range(n):
        if pick[i]:
            raw[i] = edges[which[i]]
    if n >= len(edges):
        pos = rng.choice(n, len(edges), replace=False)
        for p, e in zip(pos, edges):
            raw[p] = e
    return raw


def edge_array(rng, n, typ, edge_frac=0.25, null_frac=0.0, edges=None) -> pa.Array:
    raw = edge_raw(rng, n, typ, edge_frac, edges)
    mask = rng.random(n) < null_frac if null_frac > 0 else None
    return from_raw(raw, typ, mask)


def edge_table(rng, n, spec, edge_frac=0.25, null_frac=0.0) -> pa.Table:
    """spec: {name: pa type}"""
    return pa.table({name: edge_array(rng, n, typ, edge_frac, null_frac) for name, typ in spec.items()})


SPAN_KS = (12, 32, 40, 63, 64)


def spans() -> list:
    """the key spans (max - min) where range gates switch paths: 2^k - 1, 2^k, 2^k + 1 for k in SPAN_KS, and the full wrapping span
    (MIN..MAX of a 64-bit key, 2^64 - 1) once"""
    out = []
    for k in SPAN_KS:
        out += [2**k - 1, 2**k, 2**k + 1]
    return sorted(s for s in set(out) if s <= 2**64 - 1)


def type_range(typ: pa.DataType):
    if pa.types.is_decimal128(typ):
        top = 10**typ.precision - 1
        return -top, top
    return {pa.int32(): (I32_MIN, I32_MAX), pa.date32(): (I32_MIN, I32_MAX), pa.int64(): (I64_MIN, I64_MAX),
            pa.uint32(): (0, 2**32 - 1), pa.uint64(): (0, 2**64 - 1)}[typ]


def span_raw(rng, n, typ, span, low=None) -> list:
    """n raw integer keys whose min is `low` and max is low + span exactly (low defaults to the lowest start that keeps the span inside
    the type, centred on 0 where it fits); the other rows are drawn near both ends and at random in between"""
    lo_t, hi_t = type_range(typ)
    assert span <= hi_t - lo_t and n >= 2, (span, typ)
    if low is None:
        low = max(lo_t, min(-(span // 2), hi_t - span))
    high = low + span
    assert lo_t <= low and high <= hi_t
    raw = []
    for i in range(n):
        r = rng.random()
        if r < 0.3:
            raw.append(low + int(rng.integers(0, 8)) if span >= 8 else low)
        elif r < 0.6:
            raw.append(high - int(rng.integers(0, 8)) if span >= 8 else high)
        else:
            raw.append(low + int(rng.random() * span))
    raw = [min(max(v, low), high) for v in raw]
    pos = rng.choice(n, 2, replace=False)
    raw[pos[0]], raw[pos[1]] = low, high
    return raw


def span_array(rng, n, typ, span, low=None, null_frac=0.0) -> pa.Array:
    mask = rng.random(n) < null_frac if null_frac > 0 else None
    return from_raw(span_raw(rng, n, typ, span, low), typ, mask)


# --------------------------------------------------------------------------------------------------------- exact comparison

def words_of(col):
    """(raw 64-bit words of each row, shape (n, k); validity): float bit patterns, sign-extended integers, the two words of a
    Decimal128, day numbers; NULL rows are all-zero words"""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    n, t = len(col), col.type
    valid = np.asarray(col.is_valid(), dtype=bool) if col.null_count else np.ones(n, bool)
    if pa.types.is_boolean(t):
        w = np.asarray(col.fill_null(False), dtype=bool).astype(np.uint64).reshape(n, 1)
    elif pa.types.is_decimal128(t):
        w = np.frombuffer(col.buffers()[1], np.uint64, 2 * (n + col.offset))[2 * col.offset:].reshape(n, 2).copy() if n else np.zeros((0, 2), np.uint64)
    else:
        width = {1: (np.int8, np.uint8), 4: (np.int32, np.uint32), 8: (np.int64, np.uint64)}[t.bit_width // 8]
        raw = np.frombuffer(col.buffers()[1], width[1] if pa.types.is_unsigned_integer(t) else width[0], n + col.offset)[col.offset:] if n else np.zeros(0, width[0])
        w = raw.astype(np.int64).view(np.uint64).reshape(n, 1) if raw.dtype.itemsize < 8 else raw.view(np.uint64).reshape(n, 1)
    w = np.where(valid[:, None], w, np.uint64(0))
    return w, valid


def _computed_match(a, av, e, ev):
    """NaN = NaN, infinities and zeros exactly (with their sign), other values within REL; NULL = NULL"""
    with np.errstate(invalid="ignore", over="ignore"):
        both_nan = np.isnan(a) & np.isnan(e)
        exact = (a == e) & (np.signbit(a) == np.signbit(e))
        special = ~np.isfinite(a) | ~np.isfinite(e) | (a == 0) | (e == 0)
        close = np.abs(a - e) <= REL * np.maximum(np.abs(a), np.abs(e))
    ok = both_nan | exact | (~special & close)
    return np.where(av | ev, (av == ev) & ok, True)


def _describe(col, r):
    v = col.slice(r, 1).to_pylist()[0] if not pa.types.is_date32(col.type) else col.cast(pa.int32())[r].as_py()
    if pa.types.is_float64(col.type) and v is not None:
        return f"{v!r} (bits 0x{f64_bits(v):016x})"
    return repr(v)


def assert_exact(actual: pa.Table, expected: pa.Table, ordered: bool, computed=()):
    """actual == expected with floats held to their bits.  `computed` names the Float64 columns an operator computes (SUM, AVG, VAR):
    those match when both are NaN, or are the same infinity, or the same signed zero, or are within REL of each other.  Every other
    column (sort output, join payload, group keys, MIN / MAX, filter and partition output: floats included) must carry the same bits.
    ordered=False compares the rows as a multiset: both sides are sorted by their exact columns, then by the computed ones."""
    assert actual.column_names == expected.column_names, (actual.column_names, expected.column_names)
    for fa, fe in zip(actual.schema, expected.schema):
        assert fa.type == fe.type, f"type mismatch {fa} vs {fe}"
    assert actual.num_rows == expected.num_rows, (actual.num_rows, expected.num_rows)
    n, names = actual.num_rows, actual.column_names
    comp = [nm in computed for nm in names]
    for nm, c in zip(names, comp):
        assert not c or pa.types.is_float64(actual.schema.field(nm).type), nm
    acols = [words_of(actual.column(i)) for i in range(len(names))]
    ecols = [words_of(expected.column(i)) for i in range(len(names))]
    ia, ie = np.arange(n), np.arange(n)
    if not ordered and n > 1:
        def perm(cols):
            keys = []
            for i in [i for i in range(len(names)) if not comp[i]] + [i for i in range(len(names)) if comp[i]]:
                w, v = cols[i]
                keys += [v] + [w[:, j] for j in range(w.shape[1])]
            return np.lexsort(keys[::-1])
        ia, ie = perm(acols), perm(ecols)
    for i in range(len(names)):
        (aw, av), (ew, ev) = acols[i], ecols[i]
        aw, av, ew, ev = aw[ia], av[ia], ew[ie], ev[ie]
        if comp[i]:
            bad = ~_computed_match(aw[:, 0].view(np.float64), av, ew[:, 0].view(np.float64), ev)
        else:
            bad = (av != ev) | (aw != ew).any(axis=1)
        if bad.any():
            r = int(np.flatnonzero(bad)[0])
            ra, re = int(ia[r]), int(ie[r])
            raise AssertionError(f"{'row' if ordered else 'sorted row'} {r} of {n}, column {names[i]!r}: got {_describe(actual.column(i), ra)}, "
                                 f"want {_describe(expected.column(i), re)}; rows {actual.slice(ra, 1).to_pylist()} vs {expected.slice(re, 1).to_pylist()}")

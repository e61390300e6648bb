"""MEDIAN(x) restated in plain Python: the contract of include/dfgpu.h (calculate_median of the reference's median.rs), nothing shared
with the library.  tests/test_agg_median_reference.py holds it to hand-worked answers, to `statistics` and to numpy, and shows which
mistakes its tables catch; tests/test_zzzzzzz_gpu_agg_median.py holds the GPU AggregateExec to it exactly.

Values are RAW integers throughout: the value of an integer type, the unscaled integer of a Decimal128, the 64-bit pattern of a Float64
(so NaN payloads and the sign of zero are ordinary data).  NULL is None.  A table is {column: [raw | None, ...]}."""
import math
import struct

import numpy as np
import pyarrow as pa

from tests import edge_values as E

DEC = (38, 2)
PA = {"i32": pa.int32(), "i64": pa.int64(), "u8": pa.uint8(), "u32": pa.uint32(), "u64": pa.uint64(), "f64": pa.float64(), "dec": pa.decimal128(*DEC),
      "d32": pa.date32(), "bool": pa.bool_(), "str": pa.string()}
BITS = {"i32": 32, "i64": 64, "u8": 8, "u32": 32, "u64": 64, "dec": 128}
SIGNED = frozenset(("i32", "i64", "dec"))
MEDIAN_TYPES = ("i32", "i64", "u8", "u32", "u64", "f64", "dec")
EDGES = {"i32": E.INT_EDGES[pa.int32()], "i64": E.INT_EDGES[pa.int64()], "u8": [0, 1, 127, 128, 254, 255], "u32": E.INT_EDGES[pa.uint32()],
         "u64": E.INT_EDGES[pa.uint64()], "f64": list(E.F64_EDGE_BITS), "dec": E.decimal_edges(DEC[0])}


class _ComputedNaN:
    """the result of an even count whose IEEE addition made a NaN (a NaN middle, +inf + -inf): which NaN is the hardware's business"""

    def __repr__(self):
        return "ComputedNaN"


COMPUTED_NAN = _ComputedNaN()


def wrap(v: int, t: str) -> int:
    """v reduced to the type's width: what add_wrapping leaves"""
    bits = BITS[t]
    v &= (1 << bits) - 1
    return v - (1 << bits) if t in SIGNED and v >> (bits - 1) else v


def div2(v: int) -> int:
    """v / 2 truncating toward zero (div_wrapping by 2 cannot overflow)"""
    return -((-v) // 2) if v < 0 else v // 2


def f64(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def is_nan_bits(bits: int) -> bool:
    return (bits >> 52) & 0x7FF == 0x7FF and bits & ((1 << 52) - 1) != 0


def total_order_key(bits: int) -> int:
    """IEEE totalOrder as an unsigned integer: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN"""
    return bits ^ 0xFFFFFFFFFFFFFFFF if bits >> 63 else bits | 1 << 63


def ordered(values, t: str):
    return sorted(values, key=total_order_key) if t == "f64" else sorted(values)


def middle(v, t: str):
    """the median of the ascending non-NULL values v"""
    c = len(v)
    if c == 0:
        return None
    if c % 2:
        return v[c // 2]
    lo, hi = v[c // 2 - 1], v[c // 2]
    if t == "f64":
        s = f64(lo) + f64(hi)                         # one IEEE addition, rounded once
        if math.isnan(s):
            return COMPUTED_NAN
        return f64_bits(s / 2.0)                      # one IEEE division
    return wrap(div2(wrap(lo + hi, t)), t)


def median(values, t: str):
    """values: raw, None = NULL"""
    return middle(ordered([x for x in values if x is not None], t), t)


def passes(table, flt, i) -> bool:
    return flt is None or table[flt][i] is True


def groups_of(table, keys):
    """[(key tuple, [row numbers])] in first-seen order; without keys one group, also over no rows"""
    n = len(next(iter(table.values()))) if table else 0
    if not keys:
        return [((), list(range(n)))]
    seen = {}
    for i in range(n):
        seen.setdefault(tuple(table[k][i] for k in keys), []).append(i)
    return list(seen.items())


def aggregate(table, keys, aggs, types):
    """aggs: [("median", argument column, output name, filter column | None)].  Rows in first-seen group order: {key..., name: raw | None}"""
    out = []
    for key, rows in groups_of(table, keys):
        row = dict(zip(keys, key))
        for func, arg, name, flt in aggs:
            assert func == "median"
            row[name] = median([table[arg][i] for i in rows if passes(table, flt, i)], types[arg])
        out.append(row)
    return out


def concat(parts):
    return {c: [x for p in parts for x in p[c]] for c in parts[0]}


# ------------------------------------------------------------------------------------------------ Arrow in and out
def column(raw, t: str) -> pa.Array:
    typ = PA[t]
    if t in ("bool", "str"):
        return pa.array(raw, typ)
    mask = np.array([x is None for x in raw], bool)
    filled = [0 if x is None else x for x in raw]
    if t == "u8":
        return pa.array(np.array(filled, np.uint8), typ, mask=mask) if len(raw) else pa.array([], typ)
    return E.from_raw(filled, typ, mask if mask.any() else None)


def to_arrow(table, types) -> pa.Table:
    return pa.table({c: column(v, types[c]) for c, v in table.items()})


def raw_column(col, t: str):
    """an Arrow column back as raw values (None = NULL)"""
    words, valid = E.words_of(col)
    out = []
    for w, ok in zip(words.tolist(), valid.tolist()):
        if not ok:
            out.append(None)
        elif t == "dec":
            out.append(E.unscaled(w[0], w[1]))
        elif t in SIGNED:
            out.append(wrap(w[0], "i64"))
        else:
            out.append(w[0])
    return out


def same(got, want) -> bool:
    """got: a raw value from the device; want: the restatement's"""
    if want is COMPUTED_NAN:
        return got is not None and is_nan_bits(got)
    return got == want and type(got) is type(want)


# ------------------------------------------------------------------------------------------------ tables
def make_table(n, seed=7, groups=7, null_frac=0.15):
    """k: Int64 keys (group g of `groups`, spread so that they hash), k2: Int32, p: a nullable Boolean filter, and one column per MEDIAN
    type: the type's edge values crossed with each other at the front (every pair of edges is some group's two middles once the groups
    are small), ordinary values behind.  The first rows are laid out so that groups of 1, 2, 3 and 4 rows and an all-NULL group exist."""
    rng = np.random.default_rng(seed + n)
    # groups 100..104: sizes 1, 2, 3, 4 and an all-NULL group of 3 — present whenever n allows
    fixed = [100] + [101] * 2 + [102] * 3 + [103] * 4 + [104] * 3
    key = lambda g: g * 1000003 - 2 * 1000003
    t = {"k": [], "k2": [], "p": []}
    gs = (fixed + [int(g) for g in rng.integers(0, groups, max(0, n - len(fixed)))])[:n]
    t["k"] = [key(g) for g in gs]
    t["k2"] = [g % 3 - 1 for g in gs]
    t["p"] = [None if r < 0.1 else bool(r < 0.7) for r in rng.random(n)]
    for name in MEDIAN_TYPES:
        edges = EDGES[name]
        pairs = [e for a in edges for b in edges for e in (a, b)]
        typ = PA[name]
        raw = pairs[:n] + (E._ordinary(rng, n - len(pairs), typ if name != "u8" else pa.uint32()) if n > len(pairs) else [])
        if name == "u8":
            raw = [v & 0xFF for v in raw]
        nulls = rng.random(n) < null_frac
        t[name] = [None if nulls[i] or gs[i] == 104 else raw[i] for i in range(n)]
    return t


TYPES = dict({name: name for name in MEDIAN_TYPES}, k="i64", k2="i32", p="bool")

"""The tables and expressions of the expression-value tests, shared by tests/test_expr_reference.py (reference against the oracle, on
the CPU) and tests/test_gpu_expr_edges.py (every evaluator against the reference).

A family is one table of N = 4097 rows (64-row validity words, the 256-thread block, k_cmp's four-word unroll and a ragged tail) and
the expressions evaluated over it.  The first rows of a table hold the full cross product of the edge values of its first two
columns, all valid, so that every ordered pair of edges meets in some row (`assert_head` checks that); the rest mixes edges (one
half) with ordinary values and has 5 % NULLs.  Edges and raw-value arrays come from tests.edge_values; the mixing is done here
because several families need ordinary values of their own (uniform mantissas, ties, magnitudes beyond 2^53, non-zero divisors).
`reference(name)` evaluates a family once with tests.expr_ref and keeps the result."""
import functools
import math
from decimal import Decimal

import numpy as np
import pyarrow as pa

from datafusion_amd.expr import case, col, date_part, lit
from tests import edge_values as E
from tests import expr_ref as R
from tests.util import to_oracle_expr

N = 4097
I32, I64, F64 = pa.int32(), pa.int64(), pa.float64()
D38, D38_4, D18, D12, D15 = pa.decimal128(38, 0), pa.decimal128(38, 4), pa.decimal128(18, 2), pa.decimal128(12, 4), pa.decimal128(15, 2)
I128_MIN, I128_MAX = -2**127, 2**127 - 1
EDGES = {
    I32: E.INT_EDGES[I32], I64: E.INT_EDGES[I64], F64: E.F64_EDGE_BITS,
    D38: E.decimal_edges(38) + [I128_MIN, I128_MAX],
    D38_4: E.decimal_edges(38) + [I128_MIN, I128_MAX],
    D18: [-(10**18 - 1), -5 * 10**17, -1, 0, 1, 5 * 10**17, 10**18 - 1],
    D12: [-(10**12 - 1), -100, -1, 0, 1, 100, 10**12 - 1],
    D15: [-(10**15 - 1), -1, 0, 1, 100, 10**15 - 1],
}


def truth(pred):
    """a predicate read out as an Int32 value: 1 where it is TRUE, 0 where it is FALSE or NULL (six row-program instructions)"""
    return case([(pred, lit(1, I32))], lit(0, I32))


def tri(pred):
    """a predicate's three values as an Int32: 1 TRUE, 0 FALSE, -1 NULL (twice the instructions: column-at-a-time only)"""
    return case([(pred, lit(1, I32)), (pred.is_null(), lit(-1, I32))], lit(0, I32))


class Family:
    """values: [(name, expr)] read out as values by every evaluator, to which `truth` of the predicates named in `truths` is added as
    "is_<name>"; preds: [(name, Boolean expr)] checked by the rows they keep (and as `tri` values, "tri_<name>") column-at-a-time;
    node_pred: the predicate the fused node is also run under; fused: whether the row programs take the value expressions (False:
    they decline and the node runs column-at-a-time).  The value expressions of a fused family fit one row program (RP_MAX_INS = 56
    instructions, RP_MAX_COLS = 10 columns)."""

    def __init__(self, name, table, values, preds=(), truths=(), node_pred=None, fused=True, head=None):
        self.name, self.table, self.preds, self.fused, self.head = name, table, list(preds), fused, head
        by_name = dict(self.preds)
        self.values = list(values) + [("is_" + n, truth(by_name[n])) for n in truths]
        self.tris = [("tri_" + n, tri(p)) for n, p in self.preds]
        self.node_pred = None if node_pred is None else (node_pred, by_name[node_pred])


def mixed(rng, n, edges, ordinary, edge_frac=0.5) -> list:
    """n raw values: an edge with probability edge_frac, else ordinary(rng); every edge at least once when n allows"""
    raw = [edges[int(rng.integers(0, len(edges)))] if rng.random() < edge_frac else ordinary(rng) for _ in range(n)]
    if n >= len(edges):
        for p, e in zip(rng.choice(n, len(edges), replace=False), edges):
            raw[int(p)] = e
    return raw


def small(rng):
    return int(rng.integers(-1000, 1000))


def column(rng, n, typ, head=(), edges=None, ordinary=small, null_frac=0.05, edge_frac=0.5) -> pa.Array:
    edges = EDGES[typ] if edges is None else edges
    head = list(head)[:n]
    m = n - len(head)
    raw = head + mixed(rng, m, edges, ordinary, edge_frac)
    mask = [False] * len(head) + [bool(x) for x in (rng.random(m) < null_frac)]
    return E.from_raw(raw, typ, mask)


def cross(ea, eb):
    pairs = [(x, y) for x in ea for y in eb]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def with_row(cols: dict) -> pa.Table:
    n = len(next(iter(cols.values())))
    return pa.table({**cols, "row": pa.array(np.arange(n, dtype=np.int64))})


def assert_head(f: Family):
    """every ordered pair of the two columns' edges occurs in a row where both are valid"""
    if f.head is None:
        return
    (na, ea), (nb, eb) = f.head
    a, b = R.column_values(f.table.column(na)), R.column_values(f.table.column(nb))
    have = {(x, y) for x, y in zip(a, b) if x is not None and y is not None}
    missing = [(x, y) for x in ea for y in eb if (x, y) not in have]
    assert not missing, (f.name, missing[:3])


# ------------------------------------------------------------------------------------------------------------------------ integers
def _int_family(name, typ, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = E.type_range(typ)
    ha, hb = cross(EDGES[typ], EDGES[typ])
    t = with_row({"a": column(rng, n, typ, ha), "b": column(rng, n, typ, hb), "c": column(rng, n, typ)})
    a, b, c = col("a"), col("b"), col("c")
    L = lambda v: lit(v, typ)
    values = [("add", a + b), ("sub", a - b), ("mul", a * b),
              ("add_lit", a + L(hi)), ("lit_sub", L(lo) - a), ("mul_lit", a * L(-1)), ("lit_mul", L(hi) * a),
              ("fold", a + (L(hi) + L(1))), ("fold_mul", a - (L(lo) * L(-1))),
              ("nest_add", (a * b) + a), ("nest_mul", (a + b) * (a - b))]
    if typ == I32:   # the 32-bit wrap must happen before the widening
        values.append(("widen", (a + b).cast(I64) * b.cast(I64)))
    preds = [("sum_lt", a + b < c), ("mul_ge_lit", a * b >= L(hi - 1))]
    return Family(name, t, values, preds, truths=["sum_lt", "mul_ge_lit"], node_pred="sum_lt" if name == "int32" else None, head=(("a", EDGES[typ]), ("b", EDGES[typ])))


# ------------------------------------------------------------------------------------------------------------------------ decimals
def _dec38_family():
    rng = np.random.default_rng(38)
    ha, hb = cross(EDGES[D38], EDGES[D38])
    t = with_row({"a": column(rng, N, D38, ha), "b": column(rng, N, D38, hb), "e": column(rng, N, D38_4)})
    a, b, e = col("a"), col("b"), col("e")
    values = [("add", a + b), ("sub", a - b), ("mul", a * b),                     # products leave 128 bits and wrap
              ("add_scales", a + e), ("sub_scales", e - b), ("mul_scales", a * e),   # the rescale of `a` by 10^4 itself wraps
              ("nest", (a * b) + a)]
    return Family("dec38", t, values, [("lt_scales", a < e)], truths=["lt_scales"], head=(("a", EDGES[D38]), ("b", EDGES[D38])))


def _decmix_family():
    rng = np.random.default_rng(1812)
    hd, he = cross(EDGES[D18], EDGES[D12])
    wide = lambda rng: int(rng.integers(-10**15, 10**15))
    t = with_row({"d": column(rng, N, D18, hd, ordinary=wide), "e": column(rng, N, D12, he), "f": column(rng, N, D15)})
    d, e, f = col("d"), col("e"), col("f")
    one = lit(1, pa.decimal128(20, 0))
    values = [("add", d + e), ("sub", d - e), ("mul", d * e), ("one_minus", one - f), ("q1", f * (one - f)),
              ("add_lit", f + lit(Decimal("0.05"), D15)), ("lit_mul", lit(Decimal("-99999.99"), D15) * f),
              ("fold", f * (lit(2, pa.decimal128(20, 0)) + lit(3, pa.decimal128(20, 0))))]
    preds = [("lt_scales", d < e), ("eq_scales", (d * lit(Decimal("1.00"), D15)).eq(d * lit(Decimal("1.0000"), D12)))]
    return Family("decmix", t, values, preds, truths=["lt_scales", "eq_scales"], head=(("d", EDGES[D18]), ("e", EDGES[D12])))


# -------------------------------------------------------------------------------------------------------------------------- floats
def _float_bits(sign, mant, exp):
    return E.f64_bits(math.ldexp(mant, exp) * (-1.0 if sign else 1.0))


@functools.lru_cache(maxsize=None)
def _float_table():
    """ordinary values with uniform 53-bit mantissas and exponents spread over +-30; c is drawn a few binades below a * b, where a
    multiply-add that rounds once differs most often from a product and a sum that round twice"""
    rng = np.random.default_rng(53)
    ha, hb = cross(EDGES[F64], EDGES[F64])
    m = N - len(ha)
    uni = lambda rng: _float_bits(rng.random() < 0.5, 1.0 + rng.random(), int(rng.integers(-30, 31)))
    a = ha + mixed(rng, m, EDGES[F64], uni)
    b = hb + mixed(rng, m, EDGES[F64], uni)
    c, d = [], []
    for x, y in zip(a, b):
        p = E.f64_from_bits(x) * E.f64_from_bits(y)
        e = math.frexp(p)[1] if (math.isfinite(p) and p != 0.0) else int(rng.integers(-30, 31))
        c.append(_float_bits(rng.random() < 0.5, 1.0 + rng.random(), e - int(rng.integers(1, 30))))
        d.append(_float_bits(rng.random() < 0.5, 1.0 + rng.random(), int(rng.integers(-3, 4))))
    pick = rng.random(N) < 0.25
    for i in np.flatnonzero(pick):
        c[i] = EDGES[F64][int(rng.integers(0, len(EDGES[F64])))]
    mask = lambda: [False] * len(ha) + [bool(x) for x in (rng.random(m) < 0.05)]
    return with_row({"a": E.from_raw(a, F64, mask()), "b": E.from_raw(b, F64, mask()), "c": E.from_raw(c, F64, mask()), "d": E.from_raw(d, F64, mask())})


def _float_family(preds_only=False):
    t = _float_table()
    a, b, c, d = col("a"), col("b"), col("c"), col("d")
    values = [("add", a + b), ("sub", a - b), ("mul", a * b), ("fma", a * b + c), ("fms2", a * b - c * d), ("sum_mul", (a + b) * c),
              ("mul_lit", a * lit(2.0)), ("lit_sub", lit(math.inf) - a), ("fold", a + lit(E.DBL_MAX) * lit(2.0)), ("c_plus", c + a * b)]
    # which NaN an operation returns is the platform's choice and the total order puts the two at opposite ends: the predicates keep
    # the rows whose value cannot be NaN (finite a, b, c; |d| < 1 so that c * d stays finite)
    finite = lambda x: (x > lit(-math.inf)).and_(x < lit(math.inf))
    guard = finite(a).and_(finite(b)).and_(finite(c))
    preds = [("fma_gt", guard.and_(a * b + c > lit(0.0))), ("fms2_le", guard.and_(d > lit(-1.0)).and_(d < lit(1.0)).and_(a * b - c * d <= lit(-0.0)))]
    if preds_only:   # MAX(Float64) spends an instruction per value on the ordered key and every literal one more: two nodes
        return Family("float_preds", t, [], preds, truths=["fma_gt", "fms2_le"], node_pred="fma_gt")
    return Family("float", t, values, head=(("a", EDGES[F64]), ("b", EDGES[F64])))


# --------------------------------------------------------------------------------------------------------------------- comparisons
def _cmp_family():
    """decimal comparisons across scales, and comparisons between two Float64 literals (folded on the host for every evaluator): by
    total order NaN = NaN and -0.0 < +0.0.  (`a + b < c` over wrapping integer sums is in the integer families.)"""
    rng = np.random.default_rng(77)
    hd, he = cross(EDGES[D18], EDGES[D12])
    t = with_row({"d": column(rng, N, D18, hd), "e": column(rng, N, D12, he),
                  "x": column(rng, N, F64, ordinary=lambda rng: E.f64_bits(float(rng.integers(-8000, 8000)) / 8.0))})
    d, e, x = col("d"), col("e"), col("x")
    nan, pnan = lit(math.nan), lit(E.f64_from_bits(E.PAYLOAD_NAN_BITS))
    lits_all = nan.eq(nan).and_(lit(-0.0) < lit(0.0)).and_(lit(-0.0).eq(lit(0.0)).not_()).and_(lit(math.inf) < nan).and_(nan.ne(pnan))
    preds = [("dec_lt", d < e), ("dec_eq", (d * lit(Decimal("1.00"), D15)).eq(d * lit(Decimal("1.0000"), D12))), ("dec_ne", d.ne(e)),
             ("nan_eq_nan", nan.eq(nan)), ("nan_lt_nan", nan < nan), ("nan_ne_payload", nan.ne(pnan)),
             ("zero_lt", lit(-0.0) < lit(0.0)), ("zero_eq", lit(-0.0).eq(lit(0.0))), ("zero_ge", lit(-0.0) >= lit(0.0)),
             ("inf_lt_nan", lit(math.inf) < nan), ("lits_all", lits_all),
             ("x_and_fold", (x > lit(0.0)).and_(nan.eq(nan))), ("x_or_fold", (x > lit(0.0)).or_(lit(-0.0) < lit(0.0)))]
    return Family("cmp", t, [], preds, truths=["dec_lt", "dec_eq", "lits_all", "x_and_fold", "x_or_fold"], node_pred="x_and_fold",
                  head=(("d", EDGES[D18]), ("e", EDGES[D12])))


# --------------------------------------------------------------------------------------------------------------------------- casts
def _big64(rng):
    """Int64 magnitudes beyond 2^53 with random low bits: the conversion to double must round"""
    v = int(rng.integers(2**53, 2**63 - 1)) | 1
    return -v if rng.random() < 0.5 else v


I64_CAST_EDGES = [2**53 - 1, 2**53, 2**53 + 1, -(2**53 + 1), 2**53 + 2, 2**53 + 3, 2**54 + 2, 2**54 + 6, 2**63 - 1, -2**63, 0, -1, 2**62 + 2**8, 2**62 + 2**8 + 1]


def _casts_fused_family():
    rng = np.random.default_rng(64)
    u8 = pa.array([None if rng.random() < 0.05 else int(v) for v in rng.integers(0, 256, N)], type=pa.uint8())
    u32 = column(rng, N, pa.uint32(), edges=E.INT_EDGES[pa.uint32()], ordinary=lambda rng: int(rng.integers(0, 2**32)))
    t = with_row({"a": column(rng, N, I32), "p": column(rng, N, I64, edges=I64_CAST_EDGES, ordinary=_big64, edge_frac=0.25), "u8": u8, "u32": u32,
                  "d": column(rng, N, D15, ordinary=lambda rng: int(rng.integers(-10**14, 10**14)))})
    a, p, d = col("a"), col("p"), col("d")
    values = [("i32_i64", a.cast(I64)), ("u8_i64", col("u8").cast(I64)), ("u32_i64", col("u32").cast(I64)),
              ("i32_f64", a.cast(F64)), ("i64_f64", p.cast(F64)), ("i64_f64_half", p.cast(F64) * lit(0.5)),
              ("i32_dec", a.cast(pa.decimal128(20, 2))), ("i64_dec_wraps", p.cast(pa.decimal128(38, 20))), ("u8_dec", col("u8").cast(pa.decimal128(10, 2))),
              ("dec_up", d.cast(pa.decimal128(38, 25))), ("dec_up_add", d.cast(pa.decimal128(20, 4)) + lit(Decimal("0.0001"), pa.decimal128(20, 4)))]
    return Family("casts_fused", t, values, [("i64_f64_gt", p.cast(F64) > lit(2.0**62))], truths=["i64_f64_gt"])


F64_CAST_EDGES = [E.f64_bits(x) for x in (
    0.49999999999999994, -0.49999999999999994, 0.5, -0.5, 2.5, -2.5, 1.5, -1.5, 0.0, -0.0, 2.0**52 - 0.5, -(2.0**52 - 0.5), 2.0**51 + 0.5, 2.0**52 + 1.0,
    2.0**53 + 2.0, 1e18, -1e18, 1e38, -1e38, 5e-324, 1e-30)]
F64_CAST_EDGES_S2 = [E.f64_bits(x) for x in (0.005, -0.005, 0.015, 0.025, -0.025, 1.005, 2.675, 0.49999999999999994, 0.0, -0.0, 999999999999999.9, -999999999999999.9,
                                               1e-320, 0.125, -0.125, 0.375)]


def _ties(rng):
    k = int(rng.integers(-3000, 3000))
    return E.f64_bits(k + 0.5)


def _casts_declined_family():
    """the casts the row programs leave to the column kernels: Float64 -> Decimal128, Decimal128 -> Float64 (scales <= 22) and the
    Decimal128 scale-down; a clean table (no value beyond a target precision)"""
    rng = np.random.default_rng(22)
    dec38 = [10**38 - 1, -(10**38 - 1), 2**53 + 1, -(2**53 + 1), 2**53, 2**64 + 1, 2**100 + 2**40 + 1, 0, 1, -1, 123456789012345678901234567890123]
    wide = lambda rng: int(rng.integers(-2**62, 2**62)) * int(rng.integers(1, 2**40)) + int(rng.integers(0, 1000))
    k_edges = [5, -5, 15, -15, 25, -25, 14, -14, 16, 45, 55, 999995, -999995, 10**14 - 6, -(10**14 - 6), 10**18 - 5001, -(10**18 - 5001), 0]
    t = with_row({"f0": column(rng, N, F64, edges=F64_CAST_EDGES, ordinary=_ties, edge_frac=0.25),
                  "f2": column(rng, N, F64, edges=F64_CAST_EDGES_S2, ordinary=lambda rng: E.f64_bits(int(rng.integers(-10**6, 10**6)) / 1000.0 + 0.005), edge_frac=0.25),
                  "g": column(rng, N, pa.decimal128(38, 2), edges=dec38, ordinary=wide), "h": column(rng, N, pa.decimal128(38, 22), edges=dec38, ordinary=wide),
                  "k": column(rng, N, pa.decimal128(18, 4), edges=k_edges, ordinary=lambda rng: int(rng.integers(-10**6, 10**6)) * 10 + 5)})
    values = [("f_dec0", col("f0").cast(D38)), ("f_dec2", col("f2").cast(pa.decimal128(20, 2))), ("f_dec22", col("f2").cast(pa.decimal128(38, 22))),
              ("dec2_f", col("g").cast(F64)), ("dec22_f", col("h").cast(F64)),
              ("down1", col("k").cast(pa.decimal128(18, 3))), ("down_limit", col("k").cast(pa.decimal128(14, 0))), ("down_all", col("g").cast(D38))]
    return Family("casts_declined", t, values, [("f_dec_gt", col("f0").cast(D38) > lit(2, D38))], fused=False)


# ----------------------------------------------------------------------------------------------------------------------- date_part
DATE_EDGES = sorted({E.I32_MIN, E.I32_MAX, -719469, -719468, -719163, -719162, -1, 0, 59, 60, 2932896, 2932897} |
                    {base + k * 146097 + o for base in (-719468, -719162) for k in range(-10, 11) for o in (-1, 0, 1)})


def _date_family():
    rng = np.random.default_rng(1970)
    anyday = lambda rng: int(rng.integers(E.I32_MIN, E.I32_MAX + 1))
    t = with_row({"dt": column(rng, N, pa.date32(), DATE_EDGES, edges=DATE_EDGES, ordinary=anyday, edge_frac=0.1)})
    dt = col("dt")
    values = [(p, date_part(p, dt)) for p in ("year", "month", "day")] + [("ym", date_part("year", dt) * lit(100, I32) + date_part("month", dt))]
    preds = [("year_lt", date_part("year", dt) < lit(1, I32)), ("leap_day", date_part("month", dt).eq(lit(2, I32)).and_(date_part("day", dt).eq(lit(29, I32))))]
    return Family("date", t, values, preds, truths=["year_lt", "leap_day"], node_pred="leap_day")


# ---------------------------------------------------------------------------------------------------------------------- div and mod
def _nonzero(edges):
    return [e for e in edges if e != 0]


def _div_int_family(name, typ, seed):
    """a clean table: no zero divisor; `bd` is `b` with the one divisor that overflows MIN / -1 replaced, `b` keeps it for MIN % -1"""
    rng = np.random.default_rng(seed)
    lo, hi = E.type_range(typ)
    nz = lambda rng: small(rng) or 7
    ha, hb = cross(EDGES[typ], _nonzero(EDGES[typ]))
    a = column(rng, N, typ, ha)
    b = column(rng, N, typ, hb, edges=_nonzero(EDGES[typ]), ordinary=nz)
    av, bv = R.column_values(a), R.column_values(b)
    bd = E.from_raw([1 if (x == lo and y == -1) else (y or 0) for x, y in zip(av, bv)], typ, [y is None for y in bv])
    t = with_row({"a": a, "b": b, "bd": bd})
    a, b, bd = col("a"), col("b"), col("bd")
    L = lambda v: lit(v, typ)
    values = [("div", a / bd), ("mod", a % b), ("div_lit", a / L(7)), ("mod_lit", a % L(-1)), ("mod_min", a % L(lo)), ("lit_div", L(hi) / b), ("lit_mod", L(lo) % b),
              ("fold_mod", a + (L(lo) % L(-1))), ("fold_div", a + (L(lo) / L(1)) % L(hi)), ("nest", (a / bd) * bd + a % bd)]
    return Family(name, t, values, [("mod_eq", (a % b).eq(L(0)))], fused=False, head=(("a", EDGES[typ]), ("b", _nonzero(EDGES[typ]))))


G_FIT = (2**127 - 1) // 10**4      # the largest Decimal128(38, 0) whose rescale by 10^4 for `/` stays inside 128 bits


def _div_dec_family():
    rng = np.random.default_rng(154)
    hd, he = cross(EDGES[D15], _nonzero(EDGES[D12]))
    g_edges = [G_FIT, -G_FIT, G_FIT - 1, 10**30, -1, 0, 1, 7]
    t = with_row({"d": column(rng, N, D15, hd, ordinary=lambda rng: int(rng.integers(-10**9, 10**9))),
                  "e": column(rng, N, D12, he, edges=_nonzero(EDGES[D12]), ordinary=lambda rng: small(rng) or 3),
                  "g": column(rng, N, D38, edges=g_edges), "gd": column(rng, N, D38, edges=[1, -1, 3, -7, 10**20, G_FIT], ordinary=lambda rng: small(rng) or 9)})
    d, e, g, gd = col("d"), col("e"), col("g"), col("gd")
    values = [("div", d / e), ("mod", d % e), ("div_lit", d / lit(Decimal("-3.00"), D15)), ("mod_lit", d % lit(Decimal("0.07"), D15)),
              ("lit_div", lit(Decimal("1000.00"), D15) / e), ("lit_mod", lit(Decimal("1000.00"), D15) % e),
              ("div_rescale_edge", g / gd), ("mod38", g % gd)]
    return Family("div_dec", t, values, [("div_gt", d / e > lit(0, pa.decimal128(23, 6)))], fused=False, head=(("d", EDGES[D15]), ("e", _nonzero(EDGES[D12]))))


def _div_float_family():
    rng = np.random.default_rng(754)
    ha, hb = cross(EDGES[F64], EDGES[F64])
    dy = lambda rng: E.f64_bits(float(rng.integers(-8000, 8000)) / 8.0)
    t = with_row({"a": column(rng, N, F64, ha, ordinary=dy), "b": column(rng, N, F64, hb, ordinary=dy)})
    a, b = col("a"), col("b")
    values = [("div", a / b), ("mod", a % b), ("div_zero", a / lit(0.0)), ("div_neg_zero", a / lit(-0.0)), ("mod_inf", a % lit(math.inf)),
              ("zero_mod", lit(-0.0) % b), ("fold", a + lit(1.0) / lit(-0.0))]
    finite = lambda x: (x > lit(-math.inf)).and_(x < lit(math.inf))
    guard = finite(a).and_(finite(b)).and_(b.ne(lit(0.0))).and_(b.ne(lit(-0.0)))        # the quotient of these rows is never NaN
    return Family("div_float", t, values, [("div_lt", guard.and_(a / b < lit(0.0)))], fused=False, head=(("a", EDGES[F64]), ("b", EDGES[F64])))


BUILDERS = {
    "int32": lambda: _int_family("int32", I32, N, 32), "int64": lambda: _int_family("int64", I64, N, 64),
    "int32_63": lambda: _int_family("int32_63", I32, 63, 163), "int32_64": lambda: _int_family("int32_64", I32, 64, 164),
    "int32_65": lambda: _int_family("int32_65", I32, 65, 165),
    "dec38": _dec38_family, "decmix": _decmix_family, "float": _float_family, "float_preds": lambda: _float_family(True), "cmp": _cmp_family, "casts_fused": _casts_fused_family,
    "casts_declined": _casts_declined_family, "date": _date_family,
    "div_int32": lambda: _div_int_family("div_int32", I32, 3232), "div_int64": lambda: _div_int_family("div_int64", I64, 6464),
    "div_dec": _div_dec_family, "div_float": _div_float_family,
}
FUSED = ["int32", "int64", "int32_63", "int32_64", "int32_65", "dec38", "decmix", "float", "float_preds", "cmp", "casts_fused", "date"]
DECLINED = ["casts_declined", "div_int32", "div_int64", "div_dec", "div_float"]


@functools.lru_cache(maxsize=None)
def family(name) -> Family:
    f = BUILDERS[name]()
    assert_head(f)
    return f


@functools.lru_cache(maxsize=None)
def reference(name) -> dict:
    """{expression name: expr_ref.Val} of a family's values and predicates, computed once and left unchanged"""
    f = family(name)
    return {nm: R.evaluate(to_oracle_expr(e), f.table) for nm, e in f.values + f.tris + f.preds}


# ---------------------------------------------------------------------------------------------------------------------- error tables
ERROR_POSITIONS = (0, 63, 64, 4096)


def error_table(kind, pos):
    """(table, expression, the reference's error prefix): a clean table except for row `pos`"""
    rng = np.random.default_rng(pos + len(kind))
    nz = lambda rng: small(rng) or 5
    if kind in ("int32_zero", "int64_min_by_minus_one", "int32_mod_zero"):
        typ = I32 if "int32" in kind else I64
        a, b = R.column_values(column(rng, N, typ, edges=[1, 2], null_frac=0)), R.column_values(column(rng, N, typ, edges=[1, 2], ordinary=nz, null_frac=0))
        a[pos], b[pos] = (E.type_range(typ)[0], -1) if "min" in kind else (5, 0)
        e = col("a") % col("b") if "mod" in kind else col("a") / col("b")
        prefix = R.OVERFLOW if "min" in kind else R.DIV_ZERO
    elif kind == "dec_zero":
        typ = D15
        a, b = R.column_values(column(rng, N, typ, null_frac=0)), R.column_values(column(rng, N, typ, edges=[1, -1], ordinary=nz, null_frac=0))
        b[pos] = 0
        e, prefix = col("a") / col("b"), R.DIV_ZERO
    else:   # dec_rescale_overflow: the dividend times 10^4 leaves 128 bits in one row
        typ = D38
        a, b = R.column_values(column(rng, N, typ, edges=[G_FIT, -G_FIT], null_frac=0)), R.column_values(column(rng, N, typ, edges=[1, -1], ordinary=nz, null_frac=0))
        a[pos] = G_FIT + 1
        e, prefix = col("a") / col("b"), R.OVERFLOW
    return (a, b, typ), e, prefix


def error_tables(kind, pos):
    """the offending table, and the same table with the one row NULL on the left and on the right (those must not raise)"""
    (a, b, typ), e, prefix = error_table(kind, pos)
    mk = lambda na, nb: with_row({"a": E.from_raw(a, typ, [i == pos and na for i in range(N)]), "b": E.from_raw(b, typ, [i == pos and nb for i in range(N)])})
    return mk(False, False), mk(True, False), mk(False, True), e, prefix


ERROR_KINDS = ("int32_zero", "int32_mod_zero", "int64_min_by_minus_one", "dec_zero", "dec_rescale_overflow")

# Float64 -> Decimal128 and the scale-down, one offending value each: (value column type, raw value, target type, error prefix)
CAST_ERRORS = {
    "nan": (F64, E.QNAN_BITS, D38, R.CAST_OVERFLOW), "inf": (F64, E.f64_bits(math.inf), pa.decimal128(20, 2), R.CAST_OVERFLOW),
    "neg_inf": (F64, E.f64_bits(-math.inf), D38, R.CAST_OVERFLOW), "beyond_i128": (F64, E.f64_bits(2e38), D38, R.CAST_OVERFLOW),
    "beyond_precision": (F64, E.f64_bits(math.nextafter(1e38, math.inf)), D38, R.TOO_LARGE), "beyond_precision_scaled": (F64, E.f64_bits(-1e18), pa.decimal128(20, 2), R.TOO_LARGE),
    "down_beyond_precision": (pa.decimal128(18, 4), 10**18 - 5000, pa.decimal128(14, 0), R.TOO_LARGE),
    "down_rounds_beyond": (pa.decimal128(18, 4), -(10**18 - 5000), pa.decimal128(14, 0), R.TOO_LARGE),
}


def cast_error_tables(name, pos):
    typ, bad, to, prefix = CAST_ERRORS[name]
    rng = np.random.default_rng(pos)
    raw = [E.f64_bits(float(v)) if typ == F64 else int(v) for v in rng.integers(-1000, 1000, N)]
    raw[pos] = bad
    mk = lambda null: with_row({"v": E.from_raw(raw, typ, [i == pos and null for i in range(N)])})
    return mk(False), mk(True), col("v").cast(to), prefix

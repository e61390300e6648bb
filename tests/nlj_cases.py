"""The inputs of the nested-loop join tests: tables, filters and options, shared by the CPU test that holds the reference
(tests/test_nlj_reference.py) and the GPU test that holds the operator to it (tests/test_gpu_nlj.py).

Shapes are the smallest at which the kernel can go wrong, not workload sizes.  k_nlj gives a lane one right row (BLOCK = 256 per
workgroup) and stages the left rows in tiles of TL = 256, so the row counts come from 0, 1, a wave and its neighbours (63, 64, 65),
BLOCK / TL and their neighbours (255, 256, 257), 2 * TL + 3 = 515, and 700 rows against one with `nlj.left_chunk_rows` giving three
chunks and a ragged last one.  The largest case has 257 x 255 pairs: the Python reference of all cases together takes seconds, and
it is computed once per process (`passing`).

A case's `kind` says what holds by construction: "mixed" (both a matched and an unmatched row on every side that has two rows or more —
asserted from the reference in tests/test_nlj_reference.py), or "empty" / "all_match" / "no_match"."""
import functools
from decimal import Decimal

import numpy as np
import pyarrow as pa

BLOCK = TL = 256


class Case:
    def __init__(self, name, left, right, flt, kind="mixed", options=None, path="rowprog", ref_filter=None):
        self.name, self.left, self.right, self.filter, self.kind = name, left, right, flt, kind
        self.options = options or {}          # dfgpu options (dots as double underscores)
        self.path = path                      # "rowprog" (nlj_flags / nlj_count + nlj_emit) or "cartesian" (nlj_cartesian)
        self._ref_filter = ref_filter         # the filter in the reference's form when tests.util.to_oracle_expr cannot make it

    @property
    def ref_filter(self):
        if self.filter is None:
            return None
        if self._ref_filter is not None:
            return (self._ref_filter, self.filter[1])
        from tests.util import to_oracle_expr
        return (to_oracle_expr(self.filter[0]), self.filter[1])

    def __repr__(self):
        return self.name


def _X():
    from datafusion_amd import expr as X
    return X


# ------------------------------------------------------------------------------------------------------------------------ tables
def band_tables(nl, nr, width=7, seed=0):
    """left bands [10 i, 10 i + width) in shuffled order, right points: some inside a band, some in the gap behind it, some beyond
    every band; about one match per right row.  Payload columns ride along."""
    rng = np.random.default_rng(1000 * nl + nr + seed)
    order = rng.permutation(nl)
    lo = order * 10
    left = pa.table({"lo": pa.array(lo, type=pa.int64()), "hi": pa.array(lo + width, type=pa.int64()),
                     "tag": pa.array(np.arange(nl) * 3 - 5, type=pa.int32())})
    # every third band is left without a point, every fourth point falls into a gap, every ninth beyond the last band
    x = []
    for j in range(nr):
        band = (j * 5) % max(nl, 1)
        band += 1 if band % 3 == 0 and nl > 1 else 0
        band %= max(nl, 1)
        v = band * 10 + (j % 7 if width >= 7 else 0)
        if j % 4 == 1:
            v = band * 10 + 8                       # the gap behind a band of width 7
        if j % 9 == 2:
            v = nl * 10 + 5 + j                     # beyond every band
        x.append(v)
    right = pa.table({"x": pa.array(x, type=pa.int64()), "w": pa.array(np.arange(nr) / 4.0 - 3.0, type=pa.float64())})
    return left, right


def band_filter():
    X = _X()
    return (X.col("f0") <= X.col("f2")).and_(X.col("f2") < X.col("f1")), [(0, "Left"), (1, "Left"), (0, "Right")]


def null_tables(nl, nr, left_all_null=False, right_all_null=False):
    rng = np.random.default_rng(7 * nl + nr)
    a = rng.integers(0, 50, size=nl)
    x = rng.integers(-5, 45, size=nr)
    a[: max(1, nl // 8)] = 60                      # larger than every x: unmatched left rows
    x[: max(1, nr // 8)] = -9                      # smaller than every a: unmatched right rows
    am = (np.arange(nl) % 5 == 3) | left_all_null
    xm = (np.arange(nr) % 4 == 2) | right_all_null
    left = pa.table({"a": pa.array(a, type=pa.int64(), mask=am), "p": pa.array(np.arange(nl), type=pa.int32())})
    right = pa.table({"x": pa.array(x, type=pa.int64(), mask=xm), "q": pa.array(np.arange(nr) * 2, type=pa.int64())})
    return left, right


def decimal_tables(nl, nr):
    rng = np.random.default_rng(nl * 31 + nr)
    price = [Decimal(int(v)).scaleb(-2) for v in rng.integers(100, 100000, size=nl)]
    price[0] = Decimal("0.01")                     # times any factor stays below the literal
    factor = [Decimal(int(v)).scaleb(-2) for v in rng.integers(1, 300, size=nr)]
    factor[0] = Decimal("0.00")                    # times any price stays below the literal
    left = pa.table({"price": pa.array(price, type=pa.decimal128(15, 2), mask=np.arange(nl) % 11 == 5),
                     "d": pa.array(rng.integers(0, 20000, size=nl).astype(np.int32), type=pa.int32()).cast(pa.date32())})
    m = rng.integers(1, 13, size=nr).astype(np.int32)
    m[0] = 0                                       # no month is smaller
    right = pa.table({"factor": pa.array(factor, type=pa.decimal128(4, 2)), "m": pa.array(m, type=pa.int32(), mask=np.arange(nr) % 7 == 3)})
    return left, right


def float_tables(nl, nr):
    nan, inf = float("nan"), float("inf")
    special = [nan, -0.0, 0.0, inf, -inf, 1.5, -1.5, 5e-324, -nan]
    rng = np.random.default_rng(nl + 13 * nr)
    f = [special[i % len(special)] if i % 2 == 0 else float(rng.integers(-20, 20)) / 4 for i in range(nl)]
    g = [special[(i * 2 + 1) % len(special)] if i % 3 == 0 else float(rng.integers(-20, 20)) / 4 for i in range(nr)]
    left = pa.table({"f": pa.array(f, type=pa.float64(), mask=np.arange(nl) % 10 == 9), "i": pa.array(np.arange(nl), type=pa.int64())})
    right = pa.table({"g": pa.array(g, type=pa.float64(), mask=np.arange(nr) % 8 == 7), "j": pa.array(np.arange(nr), type=pa.int64())})
    return left, right


def dict_tables(nl, nr):
    """a dictionary-encoded left column whose LIKE '%green%' matches 20 separate runs of the dictionary: more than LikeExpr.MAX_RUNS,
    so the pattern reaches the library as a LIKE node"""
    values = [f"{'green' if i % 2 == 0 else 'red'} part {i:02d}" for i in range(40)]
    rng = np.random.default_rng(nl * 3 + nr)
    codes = rng.integers(0, 40, size=nl).astype(np.int32)
    left = pa.table({"name": pa.DictionaryArray.from_arrays(pa.array(codes, mask=np.arange(nl) % 9 == 4), pa.array(values)),
                     "v": pa.array(rng.integers(0, 100, size=nl), type=pa.int64())})
    y = rng.integers(0, 100, size=nr)
    y[0] = -1                                      # below every v
    right = pa.table({"y": pa.array(y, type=pa.int64())})
    return left, right


def eleven_tables(nl, nr):
    rng = np.random.default_rng(nl * 17 + nr)
    lcols = {f"c{k}": pa.array(rng.integers(0, 30, size=nl), type=pa.int32()) for k in range(6)}
    rcols = {f"d{k}": pa.array(rng.integers(10, 40, size=nr) + (100 if k else 0), type=pa.int32()) for k in range(5)}
    left, right = pa.table(lcols), pa.table(rcols)
    left = left.set_column(0, "c0", pa.array(np.where(np.arange(nl) % 6 == 0, 99, rng.integers(0, 30, size=nl)), type=pa.int32()))
    right = right.set_column(0, "d0", pa.array(np.where(np.arange(nr) % 5 == 0, -1, rng.integers(10, 40, size=nr)), type=pa.int32()))
    return left, right


def payload_tables(nl, nr):
    """the band tables with a dictionary-encoded and a Utf8 payload column on each side (not in the filter)"""
    left, right = band_tables(nl, nr)
    words = ["alpha", "beta", None, "gamma", ""]
    left = left.append_column("ls", pa.array([words[i % 5] for i in range(nl)], type=pa.string()))
    left = left.append_column("ld", pa.array([words[(i + 1) % 5] for i in range(nl)], type=pa.string()).dictionary_encode())
    right = right.append_column("rs", pa.array([None if i % 6 == 0 else f"r{i}" for i in range(nr)], type=pa.string()))
    right = right.append_column("rd", pa.array([words[(i + 3) % 5] for i in range(nr)], type=pa.string()).dictionary_encode())
    return left, right


# ------------------------------------------------------------------------------------------------------------------------- cases
BAND_SHAPES = [(63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (515, 65), (65, 515)]


def band_cases():
    out = [Case(f"band_{nl}x{nr}", *band_tables(nl, nr), band_filter()) for nl, nr in BAND_SHAPES]
    out.append(Case("band_700x1_three_chunks", *band_tables(700, 1), band_filter(), "mixed", {"nlj__left_chunk_rows": 300}))
    out.append(Case("band_1x700", *band_tables(1, 700), band_filter()))
    out.append(Case("band_515x63_ragged_chunks", *band_tables(515, 63), band_filter(), "mixed", {"nlj__left_chunk_rows": 200}))
    out.append(Case("band_700x3_seven_chunks", *band_tables(700, 3), band_filter(), "mixed", {"nlj__left_chunk_rows": 100}))
    out.append(Case("band_1x1", *band_tables(1, 1), band_filter(), "all_match"))
    out.append(Case("band_0x0", *band_tables(0, 0), band_filter(), "empty"))
    out.append(Case("band_0x65", *band_tables(0, 65), band_filter(), "empty"))
    out.append(Case("band_65x0", *band_tables(65, 0), band_filter(), "empty"))
    return out


def family_cases():
    X = _X()
    f0, f1, f2 = X.col("f0"), X.col("f1"), X.col("f2")
    lr = [(0, "Left"), (0, "Right")]
    out = []
    # (b) NULLs on both sides, and a side that is all NULL
    out.append(Case("nulls_65x257", *null_tables(65, 257), (f0 < f1, lr)))
    out.append(Case("nulls_257x65", *null_tables(257, 65), (f0 < f1, lr)))
    out.append(Case("nulls_left_all_null", *null_tables(65, 64, left_all_null=True), (f0 < f1, lr), "no_match"))
    out.append(Case("nulls_right_all_null", *null_tables(64, 65, right_all_null=True), (f0 < f1, lr), "no_match"))
    # (c) Decimal128 arithmetic across the sides; Int32 against date_part of a Date32
    out.append(Case("decimal_65x257", *decimal_tables(65, 257), ((f0 * f1) > X.lit(Decimal("900.0000"), pa.decimal128(20, 4)), lr)))
    out.append(Case("date_part_257x65", *decimal_tables(257, 65), (X.date_part("month", f0) < f1, [(1, "Left"), (1, "Right")])))
    # (d) Float64: NaN, +-0.0, infinities (the total order)
    out.append(Case("float_lt_65x257", *float_tables(65, 257), (f0 < f1, lr)))
    out.append(Case("float_eq_257x65", *float_tables(257, 65), (f0.eq(f1), lr)))
    # (e) one side only; literals only
    out.append(Case("left_only_65x64", *null_tables(65, 64), (f0 > X.lit(25), [(0, "Left")]), "one_sided"))
    out.append(Case("right_only_64x65", *null_tables(64, 65), (f0 > X.lit(20), [(0, "Right")]), "one_sided"))
    out.append(Case("literal_true_65x64", *null_tables(65, 64), (X.lit(True), []), "all_match"))
    out.append(Case("literal_false_65x64", *null_tables(65, 64), (X.lit(False), []), "no_match"))
    out.append(Case("literal_null_65x64", *null_tables(65, 64), (X.lit(None, pa.bool_()), []), "no_match"))
    # (f) no filter
    out.append(Case("cross_65x64", *null_tables(65, 64), None, "all_match", path="cartesian"))
    out.append(Case("cross_0x5", *null_tables(0, 5), None, "empty", path="cartesian"))
    out.append(Case("cross_5x0", *null_tables(5, 0), None, "empty", path="cartesian"))
    # (g) filters the row-program compiler declines
    dl, dr = null_tables(65, 257)
    dr = dr.set_column(1, "q", pa.array(np.arange(257) % 7 + 1, type=pa.int64()))       # no zero divisor
    out.append(Case("division_65x257", dl, dr, ((f0 / f2) > f1, [(0, "Left"), (0, "Right"), (1, "Right")]), path="cartesian"))
    out.append(Case("like_dictionary_65x64", *dict_tables(65, 64), (f0.like("%green%").and_(f1 < f2), [(0, "Left"), (1, "Left"), (0, "Right")]),
                    path="cartesian", ref_filter=("bin", "and", ("like", "f0", "%green%"), ("bin", "<", ("col", "f1"), ("col", "f2")))))
    e = X.col("f0") < X.col("f6")
    for k in range(1, 5):
        e = e.and_(X.col(f"f{k}") < X.col(f"f{6 + k}"))
    e = e.and_(X.col("f5") >= X.lit(0, pa.int32()))
    out.append(Case("eleven_columns_65x64", *eleven_tables(65, 64), (e, [(k, "Left") for k in range(6)] + [(k, "Right") for k in range(5)]), path="cartesian"))
    # the band join on the materialising path, in pieces whose boundaries fall inside a right row's run of matches
    out.append(Case("band_materialised_257x255", *band_tables(257, 255), band_filter(), options={"nlj__rowprog": 0}, path="cartesian"))
    out.append(Case("band_wide_materialised_pieces_65x63", *band_tables(65, 63, width=35), band_filter(),
                    options={"nlj__rowprog": 0, "nlj__chunk_pairs": 101}, path="cartesian"))
    out.append(Case("band_wide_65x63", *band_tables(65, 63, width=35), band_filter()))
    return out


@functools.lru_cache(maxsize=None)
def _all_cases():
    return tuple(band_cases() + family_cases())


def all_cases():
    """every case, built once per process"""
    return list(_all_cases())


def by_name(name):
    return next(c for c in _all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def pair_values(name):
    """tests.nlj_ref.pair_values of a case, computed once per process and shared by every test that needs it"""
    from tests import nlj_ref
    c = by_name(name)
    return tuple(nlj_ref.pair_values(c.left, c.right, c.ref_filter))


@functools.lru_cache(maxsize=None)
def passing(name):
    """the pairs of a case whose filter value is TRUE, in right-row-major order (the same for every join type)"""
    return tuple((l, r) for l, r, v in pair_values(name) if v is True)

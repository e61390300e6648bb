"""The inputs of the range join tests, shared by the CPU test that holds the reference (tests/test_range_join_reference.py) and the GPU
test that holds dfgpu_range_join to it (tests/test_zzzz_gpu_range_join.py).

Shapes are the smallest at which the kernels can go wrong, not workload sizes.  The bounds kernel gives a lane one left row (BLOCK = 256
per workgroup, validity words of 64 rows) and the sort works on the non-NULL x; the expand kernel gives a workgroup T =
RANGE_JOIN_TILE consecutive output slots, finds the slots' left rows in LDS when the tile spans at most T rows and in the offsets
themselves when it spans more.  So there are the nested-loop join's band shapes under all eight condition shapes, runs of equal x of
1, 63, 64, 65 and 130 rows with bounds on, below and above them, NULLs in each of the three columns, outputs of T - 1, T and T + 1
rows, one left row over three tiles, 300 and T + 5 left rows without a match between rows with many, and every key type opening with
its edge values.

A case's `kind` says what holds by construction: "mixed" (both a matched and an unmatched row on every side that has two rows or more —
asserted from the reference in tests/test_range_join_reference.py), or "empty" / "all_match" / "no_match".  `small` cases (at most
257 x 255 pairs) are also held to the pair-space reference there; the skew cases are held to tests/range_join_ref.py alone, whose
cost is linear in the output."""
import functools

import numpy as np
import pyarrow as pa

from datafusion_amd.ops import RANGE_JOIN_TILE as T
from tests import edge_values as E
from tests import nlj_cases as NC

# (lower inclusive, upper inclusive), None = the bound is absent
CONDITIONS = {"le_lt": (True, False), "le_le": (True, True), "lt_lt": (False, False), "lt_le": (False, True),
              "le_only": (True, None), "lt_only": (False, None), "only_le": (None, True), "only_lt": (None, False)}
KEY_TYPES = {"int32": pa.int32(), "int64": pa.int64(), "date32": pa.date32(), "uint32": pa.uint32(), "uint64": pa.uint64(), "float64": pa.float64()}


class Case:
    def __init__(self, name, left, right, cond, kind="mixed", small=True, x="x", a="lo", b="hi"):
        li, ui = CONDITIONS[cond]
        self.name, self.left, self.right, self.cond, self.kind, self.small = name, left, right, cond, kind, small
        self.x = x
        self.lower = None if li is None else (a, li)
        self.upper = None if ui is None else (b, ui)

    def _filter(self, col, cmp, conj):
        """the equivalent JoinFilter: columns f0.. = the bounds that are present, then x"""
        cols, parts = [], []
        n = (self.lower is not None) + (self.upper is not None)
        if self.lower is not None:
            cols.append((self.left.schema.get_field_index(self.lower[0]), "Left"))
            parts.append(cmp(col(f"f{len(cols) - 1}"), "<=" if self.lower[1] else "<", col(f"f{n}")))
        if self.upper is not None:
            cols.append((self.left.schema.get_field_index(self.upper[0]), "Left"))
            parts.append(cmp(col(f"f{n}"), "<=" if self.upper[1] else "<", col(f"f{len(cols) - 1}")))
        cols.append((self.right.schema.get_field_index(self.x), "Right"))
        return (parts[0] if len(parts) == 1 else conj(parts[0], parts[1])), cols

    @property
    def filter(self):
        """for ops.nested_loop_join / NestedLoopJoinExec"""
        from datafusion_amd import expr as X
        return self._filter(X.col, lambda l, op, r: X.BinaryExpr(l, op, r), lambda p, q: p.and_(q))

    @property
    def ref_filter(self):
        """for tests.nlj_ref (the oracle's tuple form)"""
        return self._filter(lambda n: ("col", n), lambda l, op, r: ("bin", op, l, r), lambda p, q: ("bin", "and", p, q))

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------------------------------ tables
def edged_band_tables(nl, nr):
    """nlj_cases.band_tables with an unmatched row on each side under EVERY condition shape: left row 0 is the reversed interval
    [10^9, -10^9] (its lower bound lies above every point, its upper bound below), right row 0 lies below every band and the points
    beyond every band lie above every upper bound"""
    left, right = NC.band_tables(nl, nr)
    if nl > 1:
        lo, hi = left.column("lo").to_pylist(), left.column("hi").to_pylist()
        lo[0], hi[0] = 10**9, -10**9
        left = left.set_column(0, "lo", pa.array(lo, type=pa.int64())).set_column(1, "hi", pa.array(hi, type=pa.int64()))
    if nr > 1:
        x = right.column("x").to_pylist()
        x[0] = -5
        right = right.set_column(0, "x", pa.array(x, type=pa.int64()))
    return left, right


RUNS = ((10, 1), (20, 63), (30, 64), (40, 65), (50, 130))      # (value, rows) of x: in sorted order the runs cross the 64-row words


def tie_tables():
    """x in runs of equal values, in shuffled row order (equal x must come out by ascending right row); a left row for every (a, b) with
    a and b one below, on and one above each run value — a == b and a > b among them — and intervals over several runs.  The run of
    three rows at 500 is touched by [500, 500] and the reversed [501, 499] only; -100 and 1000 lie in no interval."""
    rng = np.random.default_rng(11)
    x = [v for v, n in RUNS for _ in range(n)] + [500, 500, 500, -100, 1000]
    x = [x[i] for i in rng.permutation(len(x))]
    ab = [(v + da, v + db) for v, _ in RUNS for da in (-1, 0, 1) for db in (-1, 0, 1)]
    ab += [(10, 50), (20, 40), (21, 49), (500, 500), (501, 499), (60, 400)]
    ab = [ab[i] for i in rng.permutation(len(ab))]
    left = pa.table({"lo": pa.array([a for a, _ in ab], type=pa.int32()), "hi": pa.array([b for _, b in ab], type=pa.int32()),
                     "tag": pa.array(range(len(ab)), type=pa.int64())})
    right = pa.table({"x": pa.array(x, type=pa.int32()), "w": pa.array(np.arange(len(x)) / 2.0, type=pa.float64())})
    return left, right


def null_tables(nl=130, nr=150, a_null=None, b_null=None, x_null=None):
    """NULLs in a, b and x with partly set validity words (130 and 150 rows); under every condition shape there are unmatched rows on
    both sides: a = 60 lies above every x, b = -20 below, x = -40 below every a and x = 100 above every b.  *_null = "all": the column
    is all NULL; "none": it has no NULL."""
    rng = np.random.default_rng(5 * nl + nr)
    a = rng.integers(0, 50, size=nl)
    b = a + rng.integers(0, 20, size=nl)
    x = rng.integers(-5, 45, size=nr)
    k = max(1, nl // 8)
    a[:k], b[:k] = 60, 70
    a[k:2 * k], b[k:2 * k] = -30, -20
    j = max(1, nr // 8)
    x[:j] = -40
    x[j:2 * j] = 100
    mask = lambda n, every, at, mode: np.ones(n, bool) if mode == "all" else np.zeros(n, bool) if mode == "none" else np.arange(n) % every == at
    left = pa.table({"lo": pa.array(a, type=pa.int64(), mask=mask(nl, 5, 3, a_null)), "hi": pa.array(b, type=pa.int64(), mask=mask(nl, 7, 2, b_null)),
                     "p": pa.array(np.arange(nl), type=pa.int32())})
    right = pa.table({"x": pa.array(x, type=pa.int64(), mask=mask(nr, 4, 2, x_null)), "q": pa.array(np.arange(nr) * 2, type=pa.int64())})
    return left, right


def group_tables(groups):
    """left row g matches exactly groups[g] right rows under `lo <= x AND x <= hi` (0: none): group g's points all equal 10 g + 10, its
    interval is [10 g + 10, 10 g + 10] (a row without a match gets the empty gap [10 g + 5, 10 g + 6]).  The right rows are shuffled
    and one point at -7 lies in no interval."""
    rng = np.random.default_rng(len(groups) * 7 + sum(groups))
    x = [10 * g + 10 for g, n in enumerate(groups) for _ in range(n)] + [-7]
    x = [x[i] for i in rng.permutation(len(x))]
    lo = [10 * g + 10 if n else 10 * g + 5 for g, n in enumerate(groups)]
    hi = [10 * g + 10 if n else 10 * g + 6 for g, n in enumerate(groups)]
    left = pa.table({"lo": pa.array(lo, type=pa.int64()), "hi": pa.array(hi, type=pa.int64()), "tag": pa.array(range(len(groups)), type=pa.int32())})
    right = pa.table({"x": pa.array(x, type=pa.int64()), "w": pa.array(np.arange(len(x)) * 0.5, type=pa.float64())})
    return left, right


def one_each_tables(n):
    """n left rows [i, i + 1) with exactly one point each (the points in shuffled order), then one left row and one point without a match"""
    rng = np.random.default_rng(n)
    pts = rng.permutation(n)
    left = pa.table({"lo": pa.array(list(range(n)) + [-9], type=pa.int64()), "hi": pa.array(list(range(1, n + 1)) + [-8], type=pa.int64()),
                     "tag": pa.array(range(n + 1), type=pa.int32())})
    right = pa.table({"x": pa.array(list(pts) + [n + 5], type=pa.int64()), "w": pa.array(np.arange(n + 1) * 0.25, type=pa.float64())})
    return left, right


def typed_tables(typ, nl=70, nr=90):
    """bounds and points that open with the type's edge values (tests/edge_values.py) and go on with a mix of edges and ordinary values,
    a tenth of each column NULL.  Left row 0 is [minimum, maximum]; the points hold the type's minimum and maximum, which lie in no
    interval with an exclusive end on their side."""
    rng = np.random.default_rng(nl * 3 + nr + typ.bit_width)
    edges = E.edges_of(typ)
    if pa.types.is_date32(typ):
        # nlj_ref's comparison reads a Date32 cell as a Python date, which spans 0001-01-01 .. 9999-12-31: the ends of that span stand in
        # for the Int32 extremes (which the Int32 case holds; Date32 takes the same code path in the library)
        edges = [-719162, -719161, -1, 0, 1, 2932895, 2932896]
    if pa.types.is_float64(typ):
        from tests.expr_ref import total_key
        edges = sorted(edges, key=total_key)
    else:
        edges = sorted(edges)
    a = [edges[0]] + edges + E.edge_raw(rng, nl - len(edges) - 1, typ, edges=edges)
    b = [edges[-1]] + edges[::-1] + E.edge_raw(rng, nl - len(edges) - 1, typ, edges=edges)
    x = edges + E.edge_raw(rng, nr - len(edges), typ, edges=edges)
    null = lambda n, every: [i > len(edges) and i % every == 0 for i in range(n)]
    left = pa.table({"lo": E.from_raw(a, typ, null(nl, 9)), "hi": E.from_raw(b, typ, null(nl, 11)), "tag": pa.array(range(nl), type=pa.int32())})
    right = pa.table({"x": E.from_raw(x, typ, null(nr, 10)), "w": pa.array(np.arange(nr) * 1.5, type=pa.float64())})
    return left, right


def payload_tables(nl=65, nr=63):
    """the band tables with Utf8, dictionary-encoded and Decimal128 payload columns (none of them a key)"""
    from decimal import Decimal
    left, right = NC.payload_tables(nl, nr)
    left = left.append_column("ldec", pa.array([None if i % 7 == 3 else Decimal(i * 1001 - 5000).scaleb(-2) for i in range(nl)], type=pa.decimal128(20, 2)))
    right = right.append_column("rdec", pa.array([Decimal(-i * 77).scaleb(-4) for i in range(nr)], type=pa.decimal128(38, 4)))
    return left, right


# ------------------------------------------------------------------------------------------------------------------------- cases
def band_cases():
    out = [Case(f"band_{nl}x{nr}", *NC.band_tables(nl, nr), "le_lt") for nl, nr in NC.BAND_SHAPES]
    others = [c for c in CONDITIONS if c != "le_lt"]
    for k, (nl, nr) in enumerate(NC.BAND_SHAPES):          # every shape under the band condition and under one other; every condition somewhere
        cond = others[k % len(others)]
        out.append(Case(f"band_{cond}_{nl}x{nr}", *edged_band_tables(nl, nr), cond))
    out.append(Case("band_le_lt_edged_257x255", *edged_band_tables(257, 255), "le_lt"))
    out.append(Case("band_1x700", *NC.band_tables(1, 700), "le_lt"))
    out.append(Case("band_700x1", *NC.band_tables(700, 1), "le_lt"))
    out.append(Case("band_1x1", *NC.band_tables(1, 1), "le_lt", "all_match"))
    out.append(Case("band_0x0", *NC.band_tables(0, 0), "le_lt", "empty"))
    out.append(Case("band_0x65", *NC.band_tables(0, 65), "only_lt", "empty"))
    out.append(Case("band_65x0", *NC.band_tables(65, 0), "le_only", "empty"))
    return out


def tie_cases():
    return [Case(f"ties_{cond}", *tie_tables(), cond) for cond in ("le_lt", "le_le", "lt_lt", "lt_le")]


def null_cases():
    out = [Case(f"nulls_{cond}", *null_tables(), cond) for cond in ("le_lt", "lt_le")]
    out.append(Case("nulls_a_all_null", *null_tables(a_null="all"), "le_lt", "no_match"))
    out.append(Case("nulls_b_all_null", *null_tables(b_null="all"), "le_le", "no_match"))
    out.append(Case("nulls_x_all_null", *null_tables(x_null="all"), "lt_lt", "no_match"))
    out.append(Case("nulls_x_all_null_lower_only", *null_tables(x_null="all"), "le_only", "no_match"))
    # a bound that is absent: the NULLs of its column must not matter
    out.append(Case("nulls_lower_only_b_all_null", *null_tables(b_null="all"), "le_only"))
    out.append(Case("nulls_lower_only_b_some_null", *null_tables(x_null="none"), "lt_only"))
    out.append(Case("nulls_upper_only_a_all_null", *null_tables(a_null="all"), "only_lt"))
    out.append(Case("nulls_upper_only_a_some_null", *null_tables(), "only_le"))
    return out


def skew_cases():
    out = []
    rng = np.random.default_rng(2)
    n = 2 * T + 3
    out.append(Case(f"skew_1x{n}_all_match", pa.table({"lo": pa.array([0], type=pa.int64()), "hi": pa.array([10], type=pa.int64()), "tag": pa.array([7], type=pa.int32())}),
                    pa.table({"x": pa.array(rng.integers(0, 10, size=n), type=pa.int64()), "w": pa.array(np.arange(n) * 1.0, type=pa.float64())}),
                    "le_lt", "all_match", small=False))
    out.append(Case(f"skew_{T + 1}_rows_one_match_each", *one_each_tables(T + 1), "le_lt", small=False))
    out.append(Case("skew_300_rows_without_a_match_between_heavy_rows", *group_tables([1500] + [0] * 300 + [1500]), "le_le", small=False))
    out.append(Case(f"skew_{T + 5}_rows_without_a_match_in_one_tile", *group_tables([10] + [0] * (T + 5) + [10, 0, 3]), "le_le", small=False))
    out.append(Case("skew_one_row_over_three_tiles", *group_tables([T // 2, 0, 1, 2 * T + 100, 0, 1]), "le_le", small=False))
    for total in (T - 1, T, T + 1):
        out.append(Case(f"skew_total_{total}", *group_tables([total - 100, 0, 100]), "le_le", small=False))
    return out


def type_cases():
    out = []
    for name, typ in KEY_TYPES.items():
        out.append(Case(f"type_{name}_le_lt", *typed_tables(typ), "le_lt"))
        out.append(Case(f"type_{name}_lt_le", *typed_tables(typ), "lt_le"))
    out.append(Case("type_float64_lt_only", *typed_tables(pa.float64()), "lt_only"))
    out.append(Case("type_int64_only_lt", *typed_tables(pa.int64()), "only_lt"))
    return out


@functools.lru_cache(maxsize=None)
def _all_cases():
    return tuple(band_cases() + tie_cases() + null_cases() + skew_cases() + type_cases() + [Case("payload_65x63", *payload_tables(), "le_lt")])


def all_cases():
    """every case, built once per process"""
    return list(_all_cases())


def small_cases():
    return [c for c in _all_cases() if c.small]


def by_name(name):
    return next(c for c in _all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def pairs(name):
    """tests.range_join_ref.matching_pairs of a case, computed once per process and shared by every test that needs it"""
    from tests import range_join_ref
    c = by_name(name)
    return tuple(range_join_ref.matching_pairs(c.left, c.right, c.x, c.lower, c.upper))

"""The truth the Float64 SUM / AVG tests compare with: exact per-group sums (rationals) and the derived bound on what any
double-precision accumulation of them may return, plus the seeded input families built to make a sum round.

The bound is the one for recursive summation in any order and any association (Higham, Accuracy and Stability of Numerical Algorithms,
2nd ed., §4.2):  |computed - exact| <= gamma_m * S,  gamma_m = m u / (1 - m u),  u = 2^-53,  S = sum |x_i|,  m = the number of additions a
value can pass through.  It is a worst case, no constant in it is fitted: a correct accumulation passes it whatever its order; a
float32 temporary, a neighbour's row, a flushed subnormal or a lost partial does not, on the family built for it (tests/test_float_sum_reference.py
shows both).  Additions whose operands and result are multiples of 2^-1074 below 2^-1021 do not round at all, so a group whose S is
below 2^-1021 (the subnormal family) has the bound 0.

AVG = sum / n adds the rounding of one division, u * |exact avg|.  (The division rounds sum_computed / n, not sum / n: the u * bound / n
this leaves out is covered by what gamma_m has over the (1 + u)^m - 1 that m additions can reach, term by term for m >= 1.)  A
quotient below 2^-1022 is rounded to a multiple of 2^-1074 instead: half of that, 2^-1075, is its error there.

A SUM over an expression of k float operations (price * (1 - disc) * (1 + tax): k = 4) is held to the exact value of the expression
per row; every row carries (1 + d)^k <= 1 + gamma_k against its exact magnitude M_i, and the rounded rows are then summed:
|computed - exact| <= (gamma_k + gamma_m (1 + gamma_k)) * sum M_i.  A contracted multiply-add rounds less often and stays inside.
Where the rows are too many for rationals, the reference is math.fsum of the rows as numpy's double arithmetic rounds them (`rounded_rows`):
it is itself within gamma_k * sum M_i of the exact value, and sum M_i <= sum |rounded row| / (1 - gamma_k), which gives
|computed - fsum| <= (2 gamma_k + gamma_m (1 + gamma_k)) * sum |rounded row| / (1 - gamma_k), plus fsum's own half ulp."""
import math
from fractions import Fraction

import numpy as np

U = Fraction(1, 2**53)
DBL_MAX = 1.7976931348623157e308
FSUM_ABOVE = 100_000           # addends per group above which math.fsum stands in for the rational sum
EXACT_BELOW = Fraction(1, 2**1021)
NULL_FILLER = 7.0e295          # what the value buffer holds under a NULL: a sum that reads it is far outside every bound

FAMILIES = ("wide_range", "cancelling", "giant_neighbours", "subnormal", "tenths", "money_expr")
NULL_FRACTIONS = (0.0, 0.1)


def gamma(m: int) -> Fraction:
    assert m >= 0 and m * U < 1
    return m * U / (1 - m * U)


def exact_sum(xs) -> Fraction:
    """the exact sum of finite doubles: every double is an integer times a power of two"""
    xs = np.asarray(xs, dtype=np.float64)
    if len(xs) == 0:
        return Fraction(0)
    assert np.isfinite(xs).all() and len(xs) < 2**26
    mant, exp = np.frexp(xs)
    ints = (mant * 2.0**53).astype(np.int64)          # exact: |mant| < 1 has 53 bits
    exps, which = np.unique(exp.astype(np.int64) - 53, return_inverse=True)
    # per exponent, the integers summed in two 27-bit halves: each half's sum stays below 2^53, where float64 weights are exact
    lo = np.bincount(which, weights=(ints & (2**27 - 1)).astype(np.float64))
    hi = np.bincount(which, weights=(ints >> 27).astype(np.float64))
    low = int(exps[0])
    total = sum(((int(h) << 27) + int(l)) << (int(e) - low) for e, l, h in zip(exps, lo, hi))
    return Fraction(total) * Fraction(2) ** low


class GroupSum:
    """one group's truth: `exact` (a Fraction; with `fsum_used` the correctly rounded sum, within u * |exact| of it), `n` non-NULL addends,
    `S` = sum |x_i| (with `fsum_used` an upper bound of it), `rows` = COUNT(*), `k` = float operations in the argument expression,
    `rounded_rows`: exact and S are those of the expression's rows after their k roundings, not of its exact values"""
    __slots__ = ("exact", "n", "S", "rows", "fsum_used", "k", "rounded_rows")

    def __init__(self, exact, n, S, rows, fsum_used=False, k=0, rounded_rows=False):
        self.exact, self.n, self.S, self.rows, self.fsum_used, self.k, self.rounded_rows = exact, n, S, rows, fsum_used, k, rounded_rows

    def additions(self, partial_states=0) -> int:
        """m: n - 1 additions of the group's values, one per partial state merged, one for an accumulator that starts at 0.0"""
        return max(self.n - 1, 0) + partial_states + 1

    def sum_bound(self, partial_states=0) -> Fraction:
        if self.k == 0 and not self.fsum_used and self.S < EXACT_BELOW:
            return Fraction(0)
        gm = gamma(self.additions(partial_states))
        gk = gamma(self.k)
        if self.k == 0:
            b = gm * self.S
        elif not self.rounded_rows:
            b = (gk + gm * (1 + gk)) * self.S
        else:
            b = (2 * gk + gm * (1 + gk)) * self.S / (1 - gk)
        return b + (U * abs(self.exact) if self.fsum_used else 0)

    def exact_avg(self) -> Fraction:
        return self.exact / self.n

    def avg_bound(self, partial_states=0) -> Fraction:
        avg = abs(self.exact_avg())
        division = U * avg if avg >= Fraction(1, 2**1022) else Fraction(1, 2**1075)
        return self.sum_bound(partial_states) / self.n + division


def group_slices(keys):
    """{key: row indices} for an integer key array or a list of hashable keys (a dict is taken for the slices themselves)"""
    if isinstance(keys, dict):
        return keys
    if isinstance(keys, np.ndarray) and keys.ndim == 1:
        order = np.argsort(keys, kind="stable")
        ks = keys[order]
        cuts = np.flatnonzero(np.diff(ks)) + 1
        starts = np.concatenate([[0], cuts])
        ends = np.concatenate([cuts, [len(ks)]])
        return {int(ks[a]): order[a:b] for a, b in zip(starts, ends)} if len(ks) else {}
    out = {}
    for i, k in enumerate(keys):
        out.setdefault(k, []).append(i)
    return {k: np.array(v) for k, v in out.items()}


def exact_group_sums(keys, values, valid=None, fsum_above=FSUM_ABOVE, k=0) -> dict:
    """{key: GroupSum} of Float64 `values` grouped by `keys` (an integer array, or any hashable per row); NULL where `valid` is False.
    Groups of more than `fsum_above` addends take math.fsum (not where the magnitudes sum to less than 2^-1021: those stay exact).
    k > 0: the values are the rows of an expression of k float operations as double arithmetic rounded them (`rounded_rows`).
    Asserts what the bound rests on: finite addends and S < DBL_MAX / 2 in every group, so that no order of the additions overflows."""
    values = np.asarray(values, dtype=np.float64)
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, dtype=bool)
    out = {}
    for key, idx in group_slices(keys).items():
        xs = values[idx][valid[idx]]
        assert np.isfinite(xs).all(), "non-finite addends belong to the edge-value tests"
        if len(xs) > fsum_above and math.fsum(np.abs(xs)) >= 2.0**-1021:
            exact, S = Fraction(math.fsum(xs)), Fraction(math.fsum(np.abs(xs))) / (1 - U)
            g = GroupSum(exact, len(xs), S, len(idx), fsum_used=True, k=k, rounded_rows=k > 0)
        else:
            g = GroupSum(exact_sum(xs), len(xs), exact_sum(np.abs(xs)), len(idx), k=k, rounded_rows=k > 0)
        assert g.S < Fraction(DBL_MAX) / 2, "a group's sum of magnitudes could overflow in some order"
        out[key] = g
    return out


def exact_group_sums_expr(keys, row_exact, row_mag, valid, k) -> dict:
    """the same for a SUM over an expression: `row_exact` the expression's exact value per row and `row_mag` its exact magnitude bound
    (Fractions), `k` the float operations in it"""
    valid = np.asarray(valid, dtype=bool)
    out = {}
    for key, idx in group_slices(keys).items():
        live = [int(i) for i in idx if valid[i]]
        g = GroupSum(sum((row_exact[i] for i in live), Fraction(0)), len(live), sum((row_mag[i] for i in live), Fraction(0)), len(idx), k=k)
        assert g.S < Fraction(DBL_MAX) / 2
        out[key] = g
    return out


def ratio(computed: float, exact: Fraction, bound: Fraction) -> float:
    """|computed - exact| / bound as a float for messages and records (0 / 0 = 0, x / 0 = inf; inf for a computed infinity or NaN)"""
    if not math.isfinite(computed):
        return math.inf
    err = abs(Fraction(computed) - exact)
    if err == 0:
        return 0.0
    if bound == 0:
        return math.inf
    r = err / bound
    return float(r) if r < 10**300 else math.inf


def within(computed: float, exact: Fraction, bound: Fraction) -> bool:
    """the comparison itself, in rationals: no tolerance beside the bound"""
    return math.isfinite(computed) and abs(Fraction(computed) - exact) <= bound


# --------------------------------------------------------------------------------------------------------------- input families

def _mantissas(rng, n):
    """random 53-bit mantissas in [1, 2) with random signs"""
    m = (rng.integers(2**52, 2**53, n).astype(np.float64)) / 2.0**52
    return np.where(rng.random(n) < 0.5, -m, m)


def run_lengths_gids(lengths) -> np.ndarray:
    """group numbers 0, 1, 2, ... in contiguous runs of the given lengths"""
    return np.repeat(np.arange(len(lengths), dtype=np.int64), np.asarray(lengths, dtype=np.int64))


WORD_EDGE_RUNS = (63, 64, 65, 127, 128, 129, 1, 62, 66, 2, 126, 130, 64, 64, 63, 1, 65, 128, 127, 129, 3)


SHORT_RUNS = (63, 64, 1, 62, 2, 64, 63, 3, 61, 64, 33, 31, 64, 60, 5)     # 676 rows: the starts move through the word as it repeats


def short_runs(n_min: int) -> np.ndarray:
    """runs of at most 64 rows: every 64-row word holds a run head, so no run is 'long'; most of them still cross a word boundary"""
    lengths = []
    while sum(lengths) < n_min:
        lengths += list(SHORT_RUNS)
    return run_lengths_gids(lengths)


def word_edge_runs(n_min: int, long_run: int = 0) -> np.ndarray:
    """group numbers in runs that start, end and straddle at 63 / 64 / 65 / 127 / 128 / 129 rows (the 64-row words a wave of the
    runs node and of the dense-runs source walks), repeated to at least `n_min` rows; `long_run` > 0 puts one run of that many rows
    (longer than a workgroup's tile: the atomic leg) into the middle"""
    lengths = []
    while sum(lengths) < n_min:
        lengths += list(WORD_EDGE_RUNS)
    if long_run:
        lengths.insert(len(lengths) // 2, long_run)
    return run_lengths_gids(lengths)


def family(name: str, gids, null_frac: float, seed: int) -> dict:
    """the columns of one family over rows whose groups are `gids` (integer group numbers; a family that shapes its values by group
    reads them): {"x": Float64 values, "valid": bool} — money_expr: {"price", "disc", "tax", "valid"} (valid = price's validity).
    Value slots under a NULL hold NULL_FILLER."""
    gids = np.asarray(gids, dtype=np.int64)
    n = len(gids)
    rng = np.random.default_rng([seed, FAMILIES.index(name), int(null_frac * 100), n])
    valid = rng.random(n) >= null_frac if null_frac > 0 else np.ones(n, bool)
    if name == "money_expr":
        price = np.round(rng.uniform(900.0, 105_000.0, n), 2)
        disc = rng.integers(0, 11, n).astype(np.float64) / 100.0
        tax = rng.integers(0, 9, n).astype(np.float64) / 100.0
        return {"price": np.where(valid, price, NULL_FILLER), "disc": disc, "tax": tax, "valid": valid}
    if name == "wide_range":
        x = np.ldexp(_mantissas(rng, n), rng.integers(-200, 201, n))
    elif name == "cancelling":
        # inside each group, in a random order of its non-NULL rows: (v, -v) pairs of 2^60 .. 2^80; the first pair and an unpaired
        # last row are small residues instead, so the exact sum is ~1e-3 under an S of ~1e24
        big = np.ldexp(_mantissas(rng, n), rng.integers(60, 81, n))
        small = rng.uniform(-1e-3, 1e-3, n)
        x = np.zeros(n)
        live = np.flatnonzero(valid)
        order = live[np.lexsort((rng.random(len(live)), gids[live]))]
        g = gids[order]
        start = np.concatenate([[True], g[1:] != g[:-1]]) if len(g) else np.zeros(0, bool)
        first = np.maximum.accumulate(np.where(start, np.arange(len(g)), 0)) if len(g) else np.zeros(0, np.int64)
        rank = np.arange(len(g)) - first
        size = np.diff(np.concatenate([np.flatnonzero(start), [len(g)]]))[np.cumsum(start) - 1] if len(g) else np.zeros(0, np.int64)
        v = big[order]
        odd = rank % 2 == 1
        v[odd] = -v[np.flatnonzero(odd) - 1]
        residue = (rank < 2) | ((rank % 2 == 0) & (rank == size - 1))
        v[residue] = small[order][residue]
        x[order] = v
    elif name == "giant_neighbours":
        x = np.ldexp(_mantissas(rng, n), np.where(gids % 2 == 0, 900, -900))
    elif name == "subnormal":
        # multiples of 2^-1074 small enough that a whole group stays below 2^-1021: no addition of them rounds
        biggest = max(int(np.bincount(gids - gids.min()).max()), 1) if n else 1
        top = max(2, 2**52 // (biggest + 1))
        k = rng.integers(1, top, n)
        x = np.ldexp(np.where(rng.random(n) < 0.5, -1.0, 1.0) * k.astype(np.float64), -1074)
        assert (np.abs(x) < 2.0**-1022).all() and (x != 0).all()
    elif name == "tenths":
        x = np.where((gids + seed) % 2 == 0, 0.1, 1.0 / 3.0)
    else:
        raise KeyError(name)
    return {"x": np.where(valid, x, NULL_FILLER), "valid": valid}


MONEY_K = 4     # 1 - disc, price * that, 1 + tax, the product


def money_rows(cols):
    """exact value and magnitude per row of price * (1 - disc) * (1 + tax); all factors are positive, so the magnitude is the value"""
    exact = [Fraction(p) * (1 - Fraction(d)) * (1 + Fraction(t)) if v else Fraction(0)
             for p, d, t, v in zip(cols["price"].tolist(), cols["disc"].tolist(), cols["tax"].tolist(), cols["valid"].tolist())]
    return exact, exact


def family_reference(name, gids, cols, fsum_above=FSUM_ABOVE) -> dict:
    """{group number: GroupSum} of a family's SUM argument (money_expr over more than `fsum_above` rows: of its rounded rows)"""
    if name == "money_expr" and len(gids) > fsum_above:
        return exact_group_sums(np.asarray(gids), family_values(name, cols), cols["valid"], fsum_above, k=MONEY_K)
    if name == "money_expr":
        exact, mag = money_rows(cols)
        return exact_group_sums_expr(np.asarray(gids), exact, mag, cols["valid"], MONEY_K)
    return exact_group_sums(np.asarray(gids), cols["x"], cols["valid"], fsum_above)


def family_values(name, cols) -> np.ndarray:
    """the SUM argument per row as double arithmetic gives it (what an honest summation adds up)"""
    if name == "money_expr":
        return cols["price"] * (1.0 - cols["disc"]) * (1.0 + cols["tax"])
    return cols["x"]


def f64_array(values, valid=None):
    """a Float64 Arrow array over exactly these value slots (what lies under a NULL included)"""
    import pyarrow as pa
    vbuf = None if valid is None or valid.all() else pa.py_buffer(np.packbits(np.asarray(valid).astype(np.uint8), bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.float64(), len(values), [vbuf, pa.py_buffer(np.ascontiguousarray(values, dtype=np.float64).tobytes())])

"""The Float64 SUM / AVG reference and its bound (tests/float_sum_ref.py), checked without a GPU: honest double-precision summations in
any order stay inside the bound on every input family — the oracle, which the rest of the suite trusts, among them — and each wrong
summation the GPU tests are meant to catch violates it on the family built for it."""
import math
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from tests import float_sum_ref as R

N = 20_000


def _gids(family, layout, seed=1):
    rng = np.random.default_rng(seed)
    if layout == "runs":
        return R.word_edge_runs(N, long_run=3000)
    g = rng.integers(0, 6, N)
    g[N // 2] = 6            # one group of a single row
    return g


CASES = [(f, nf, "interleaved") for f in R.FAMILIES for nf in R.NULL_FRACTIONS] + [("giant_neighbours", nf, "runs") for nf in R.NULL_FRACTIONS]


def _case(family, null_frac, layout):
    gids = _gids(family, layout)
    cols = R.family(family, gids, null_frac, seed=3)
    return gids, cols, R.family_reference(family, gids, cols), R.family_values(family, cols)


def _per_group(gids, vals, valid, summer):
    """{group: summer(the group's non-NULL values in row order)}"""
    return {k: summer(vals[idx][valid[idx]]) for k, idx in R.group_slices(np.asarray(gids)).items()}


def _sequential(xs):
    return float(np.cumsum(xs)[-1]) if len(xs) else 0.0


def _wave_tree(xs):
    """a 64-wide tree per wave, the waves' totals combined one after the other"""
    pad = np.concatenate([xs, np.zeros(-len(xs) % 64)]).reshape(-1, 64)
    w = 64
    while w > 1:
        w //= 2
        pad = pad[:, :w] + pad[:, w:2 * w]
    return _sequential(pad[:, 0])


def _honest_summers():
    out = {"row_order": _sequential, "reverse": lambda xs: _sequential(xs[::-1]), "numpy_pairwise": lambda xs: float(np.sum(xs)) if len(xs) else 0.0,
           "wave_tree": _wave_tree}
    for p in range(5):
        out[f"permutation_{p}"] = lambda xs, p=p: _sequential(xs[np.random.default_rng(100 + p).permutation(len(xs))])
    return out


def _violations(ref, sums, partial_states=0, counts=None):
    """[(group, ratio)] of the groups whose SUM (and AVG = sum / count) leave the bound"""
    bad = []
    for k, g in ref.items():
        if g.n == 0:
            continue
        s = sums[k]
        if not R.within(s, g.exact, g.sum_bound(partial_states)):
            bad.append((k, "sum", R.ratio(s, g.exact, g.sum_bound(partial_states))))
        with np.errstate(all="ignore"):
            avg = float(np.float64(s) / np.float64(g.n if counts is None else counts[k]))
        if not R.within(avg, g.exact_avg(), g.avg_bound(partial_states)):
            bad.append((k, "avg", R.ratio(avg, g.exact_avg(), g.avg_bound(partial_states))))
    return bad


# ------------------------------------------------------------------------------------------------------------ the reference itself

def test_exact_sum_is_the_rational_sum():
    rng = np.random.default_rng(0)
    for xs in (np.ldexp(rng.uniform(-1, 1, 500), rng.integers(-1070, 1000, 500)), np.array([5e-324, -1.5e-323, 2.0**-1022]), np.array([0.1] * 10),
               np.array([R.DBL_MAX / 4, -R.DBL_MAX / 4, 1.0]), np.zeros(3), np.zeros(0)):
        assert R.exact_sum(xs) == sum((Fraction(float(x)) for x in xs), Fraction(0))


def test_gamma_and_the_counts_of_additions():
    assert R.gamma(0) == 0 and R.gamma(1) == R.U / (1 - R.U)
    g = R.GroupSum(Fraction(3), 3, Fraction(3), 4)
    assert g.additions() == 3 and g.additions(partial_states=3) == 6
    assert g.sum_bound() == R.gamma(3) * 3 and g.avg_bound() == R.gamma(3) + R.U
    tiny = R.GroupSum(Fraction(3, 2**1074), 3, Fraction(5, 2**1074), 3)
    assert tiny.sum_bound() == 0 and tiny.avg_bound() == Fraction(1, 2**1075)     # additions exact; the division rounds to a subnormal
    e = R.GroupSum(Fraction(10), 2, Fraction(10), 2, k=4)
    assert e.sum_bound() == (R.gamma(4) + R.gamma(2) * (1 + R.gamma(4))) * 10


def test_rounded_rows_reference_agrees_with_the_exact_rows():
    """money_expr against fsum of its rounded rows (how the large cases take it) and against the exact rows: an honest sum is inside both,
    and the rounded-rows bound is the wider one"""
    gids = np.random.default_rng(5).integers(0, 4, 6000)
    cols = R.family("money_expr", gids, 0.1, seed=1)
    exact, rounded = R.family_reference("money_expr", gids, cols), R.family_reference("money_expr", gids, cols, fsum_above=1000)
    sums = _per_group(gids, R.family_values("money_expr", cols), cols["valid"], _sequential)
    for k in exact:
        assert rounded[k].rounded_rows and rounded[k].fsum_used and not exact[k].rounded_rows
        assert rounded[k].sum_bound() > exact[k].sum_bound()
        assert abs(rounded[k].exact - exact[k].exact) <= R.gamma(R.MONEY_K) * exact[k].S + R.U * abs(exact[k].exact)
    assert not _violations(exact, sums) and not _violations(rounded, sums)


def test_short_runs_have_a_head_in_every_word():
    g = R.short_runs(20_000)
    heads = np.concatenate([[True], np.diff(g) != 0])
    words = np.add.reduceat(heads, np.arange(0, len(g), 64))
    assert (words > 0).all() and (np.flatnonzero(heads) % 64 != 0).sum() > len(words) // 2


def test_a_computed_infinity_or_nan_is_outside_every_bound():
    for bad in (math.inf, -math.inf, math.nan):
        assert not R.within(bad, Fraction(1), Fraction(10**400)) and R.ratio(bad, Fraction(1), Fraction(1)) == math.inf
    assert R.ratio(1.0, Fraction(1), Fraction(0)) == 0.0 and R.ratio(1.5, Fraction(1), Fraction(0)) == math.inf


def test_the_reference_refuses_what_the_bound_does_not_cover():
    with pytest.raises(AssertionError):
        R.exact_group_sums(np.zeros(3, np.int64), np.array([R.DBL_MAX / 2, R.DBL_MAX / 4, R.DBL_MAX / 4]))    # S >= DBL_MAX / 2
    with pytest.raises(AssertionError):
        R.exact_group_sums(np.zeros(2, np.int64), np.array([1.0, math.inf]))


def test_fsum_stands_in_above_the_limit_with_its_half_ulp_in_the_bound():
    rng = np.random.default_rng(2)
    xs = rng.uniform(-1, 1, 3000)
    exact = R.exact_group_sums(np.zeros(3000, np.int64), xs)[0]
    approx = R.exact_group_sums(np.zeros(3000, np.int64), xs, fsum_above=1000)[0]
    assert approx.fsum_used and not exact.fsum_used
    assert abs(approx.exact - exact.exact) <= R.U * abs(exact.exact) and approx.S >= exact.S
    assert approx.sum_bound() >= exact.sum_bound()


@pytest.mark.parametrize("family, null_frac, layout", CASES)
def test_the_families_are_what_they_say(family, null_frac, layout):
    gids, cols, ref, vals = _case(family, null_frac, layout)
    valid = cols["valid"]
    assert abs((~valid).mean() - null_frac) < 0.02 and (null_frac > 0) == (not valid.all())
    live = vals[valid]
    assert np.isfinite(live).all()
    assert any(g.rows == 1 for g in ref.values())                  # a group of one row
    if family == "wide_range":
        e = np.frexp(live)[1]
        assert e.min() < -150 and e.max() > 150
    if family == "cancelling":
        big = [g for g in ref.values() if g.n >= 4]
        assert big and all(abs(g.exact) < g.S / 2**60 for g in big)
    if family == "giant_neighbours":
        mags = {k: float(g.S / g.n) for k, g in ref.items() if g.n}
        assert all((m > 2.0**899) == (k % 2 == 0) and (m > 2.0**899 or m < 2.0**-898) for k, m in mags.items())
        if layout == "runs":
            assert (np.diff(gids) >= 0).all()
            lengths = np.bincount(gids)
            assert set(lengths) >= {63, 64, 65, 127, 128, 129} and lengths.max() >= 3000
            starts = np.cumsum(lengths) - lengths
            assert {0, 1, 63} <= set(starts % 64) and {0, 1, 63} <= set((starts + lengths) % 64)
    if family == "subnormal":
        assert (np.abs(live) < 2.0**-1022).all() and (live != 0).all() and (live > 0).any() and (live < 0).any()
        assert all(g.sum_bound() == 0 for g in ref.values())
    if family == "tenths":
        assert set(np.unique(live)) == {0.1, 1.0 / 3.0}


# --------------------------------------------------------------------------------------------- honest summations are inside the bound

@pytest.mark.parametrize("family, null_frac, layout", CASES)
def test_honest_summations_stay_inside_the_bound(family, null_frac, layout):
    gids, cols, ref, vals = _case(family, null_frac, layout)
    for name, summer in _honest_summers().items():
        sums = _per_group(gids, vals, cols["valid"], summer)
        assert not _violations(ref, sums), (name, _violations(ref, sums)[:3])


def _arrow_table(family, gids, cols):
    f64 = R.f64_array
    t = {"g": pa.array(np.asarray(gids, dtype=np.int64))}
    if family == "money_expr":
        t.update(price=f64(cols["price"], cols["valid"]), disc=f64(cols["disc"]), tax=f64(cols["tax"]))
    else:
        t["x"] = f64(cols["x"], cols["valid"])
    return pa.table(t)


def _oracle_arg(family):
    if family != "money_expr":
        return ("col", "x")
    one = ("lit", 1.0, pa.float64())
    return ("bin", "*", ("bin", "*", ("col", "price"), ("bin", "-", one, ("col", "disc"))), ("bin", "+", one, ("col", "tax")))


@pytest.mark.parametrize("family, null_frac, layout", CASES)
def test_the_oracle_stays_inside_the_bound(family, null_frac, layout):
    """oracle.aggregate is the reference of every other Float64 SUM / AVG assertion in the suite: Single, and Partial -> Final over three
    uneven cuts (three partial states merged)"""
    from oracle import oracle
    gids, cols, ref, _ = _case(family, null_frac, layout)
    t = _arrow_table(family, gids, cols)
    gb, aggs = [(("col", "g"), "g")], [("sum", _oracle_arg(family), "s"), ("avg", _oracle_arg(family), "a"), ("count", _oracle_arg(family), "c")]
    cuts = sorted({0, N // 3, N // 3 + 1, t.num_rows})
    state = pa.concat_tables([oracle.aggregate(t.slice(a, b - a), gb, aggs, "Partial") for a, b in zip(cuts, cuts[1:])])
    for got, states in ((oracle.aggregate(t, gb, aggs, "Single"), 0), (oracle.aggregate(state, gb, aggs, "Final"), 3)):
        assert got.num_rows == len(ref)
        for k, s, a, c in zip(*(got.column(c).to_pylist() for c in ("g", "s", "a", "c"))):
            g = ref[k]
            assert c == g.n
            if g.n == 0:
                assert s is None and a is None
                continue
            assert R.within(s, g.exact, g.sum_bound(states)), (k, s, R.ratio(s, g.exact, g.sum_bound(states)))
            assert R.within(a, g.exact_avg(), g.avg_bound(states)), (k, a, R.ratio(a, g.exact_avg(), g.avg_bound(states)))


# ------------------------------------------------------------------------------------------- wrong summations leave the bound

def _f32_accumulator(xs):
    return float(np.cumsum(xs, dtype=np.float32)[-1]) if len(xs) else 0.0


def _f32_partials(xs):
    """double accumulation inside 256-row tiles, the tiles' partials kept in 32 bits"""
    tiles = [np.float32(_sequential(xs[i:i + 256])) for i in range(0, len(xs), 256)]
    return _sequential(np.array(tiles, dtype=np.float64))


def _flush_subnormals(xs):
    return _sequential(np.where(np.abs(xs) < 2.0**-1022, 0.0, xs))


@pytest.mark.parametrize("family", ["tenths", "money_expr"])
@pytest.mark.parametrize("mutant", [_f32_accumulator, _f32_partials], ids=["accumulator", "partials"])
def test_mutant_a_float32_storage_leaves_the_bound(family, mutant):
    gids, cols, ref, vals = _case(family, 0.0, "interleaved")
    sums = _per_group(gids, vals, cols["valid"], mutant)
    bad = _violations(ref, sums)
    assert bad, "a 32-bit accumulator went unnoticed"
    honest = _per_group(gids, vals, cols["valid"], _sequential)
    if mutant is _f32_partials:
        assert all(abs(sums[k] - honest[k]) <= 1e-6 * abs(honest[k]) for k in sums)       # what the 1e-6 comparison lets through


def _runs_case(null_frac):
    gids, cols, ref, vals = _case("giant_neighbours", null_frac, "runs")
    v = np.where(cols["valid"], vals, 0.0)
    lengths = np.bincount(gids)
    ends = np.cumsum(lengths)
    return gids, cols, ref, v, ends - lengths, ends


@pytest.mark.parametrize("null_frac", R.NULL_FRACTIONS)
def test_mutant_b_prefix_differences_leave_the_bound(null_frac):
    """run totals as inclusive prefix [last row] - inclusive prefix [row before the run]: the small groups drown in their neighbours"""
    gids, cols, ref, v, starts, ends = _runs_case(null_frac)
    prefix = np.concatenate([[0.0], np.cumsum(v)])
    sums = {k: float(prefix[ends[k]] - prefix[starts[k]]) for k in ref}
    bad = _violations(ref, sums)
    assert {k for k, _, _ in bad} >= {k for k, g in ref.items() if k % 2 == 1 and g.exact != 0}         # every 2^-900 group
    assert sum(k % 2 == 1 and g.exact != 0 for k, g in ref.items()) > len(ref) // 4


@pytest.mark.parametrize("null_frac", R.NULL_FRACTIONS)
@pytest.mark.parametrize("mutant", ["takes_the_next_runs_first_row", "loses_its_last_row"])
def test_mutant_c_a_boundary_one_row_off_leaves_the_bound(null_frac, mutant):
    gids, cols, ref, v, starts, ends = _runs_case(null_frac)
    valid = cols["valid"]
    sums, checked = {}, {}
    for k in ref:
        a, b = int(starts[k]), int(ends[k])
        b2 = min(b + 1, len(v)) if mutant == "takes_the_next_runs_first_row" else b - 1
        moved = b if b2 > b else b2                   # the row wrongly added or dropped
        if b2 == b or not valid[moved]:
            continue                                  # the last run has no neighbour; a NULL row changes nothing
        sums[k] = _sequential(v[a:b2]) if b2 > a else 0.0
        checked[k] = ref[k]
    bad = {k for k, what, _ in _violations(checked, sums) if what == "sum"}
    if mutant == "loses_its_last_row":
        assert bad == set(checked)                    # a lost addend is seen in every group
    else:
        assert bad == {k for k in checked if k % 2 == 1}     # a 2^900 row in a 2^-900 group; the reverse is below the giant's rounding:
        assert len(bad) > len(ref) // 4                      # the GPU tests see that one through COUNT and the Int64 companion


@pytest.mark.parametrize("null_frac", R.NULL_FRACTIONS)
def test_mutant_d_flushed_subnormals_leave_the_bound(null_frac):
    gids, cols, ref, vals = _case("subnormal", null_frac, "interleaved")
    sums = _per_group(gids, vals, cols["valid"], _flush_subnormals)
    assert {k for k, _, _ in _violations(ref, sums)} == {k for k, g in ref.items() if g.exact != 0}
    assert sum(g.exact != 0 for g in ref.values()) >= 6


@pytest.mark.parametrize("mutant", ["dropped", "doubled"])
def test_mutant_e_a_partial_state_dropped_or_doubled_in_the_merge_leaves_the_bound(mutant):
    """1.2 M times 0.1 in one group, cut as the suite cuts its Partial inputs (n // 3, n // 3 + 1): the middle state is one row, less
    than 1e-6 of the total"""
    n = 1_200_000
    gids = np.zeros(n, np.int64)
    cols = R.family("tenths", gids, 0.0, seed=0)
    ref = R.family_reference("tenths", gids, cols)
    assert ref[0].fsum_used
    cuts = [0, n // 3, n // 3 + 1, n]
    parts = [_sequential(cols["x"][a:b]) for a, b in zip(cuts, cuts[1:])]
    honest = _sequential(np.array(parts))
    assert not _violations(ref, {0: honest}, partial_states=3)
    wrong = _sequential(np.array([parts[0], parts[2]] if mutant == "dropped" else [parts[0], parts[1], parts[1], parts[2]]))
    assert abs(wrong - honest) <= 1e-6 * honest                  # invisible at 1e-6
    assert _violations(ref, {0: wrong}, partial_states=3)


@pytest.mark.parametrize("family", ["wide_range", "giant_neighbours", "subnormal", "tenths", "money_expr"])
def test_mutant_f_avg_over_the_row_count_leaves_the_bound(family):
    gids, cols, ref, vals = _case(family, 0.1, "interleaved")
    sums = _per_group(gids, vals, cols["valid"], _sequential)
    assert not _violations(ref, sums)
    bad = _violations(ref, sums, counts={k: g.rows for k, g in ref.items()})
    assert {k for k, what, _ in bad if what == "avg"} == {k for k, g in ref.items() if g.n and g.rows != g.n and g.exact != 0}
    assert len(bad) >= 6

"""The reference of the expression-value tests (tests/expr_ref.py) held against the CPU oracle on every table of tests/expr_cases.py and
against Python's own calendar, and the tables held to their purpose: each wrong evaluator below (a few lines of Python) must differ
from the reference on at least 100 non-NULL rows of the table built to catch it, or in its error outcome.  The 100 rows are a
condition on the inputs, not a tolerance: a table that stops meeting it no longer tests what it was built for.  No GPU is used."""
import datetime
import math
from fractions import Fraction

import pyarrow as pa
import pytest

from tests import edge_values as E
from tests import expr_cases as C
from tests import expr_ref as R
from tests.util import to_oracle_expr


def _oracle(expr, table) -> R.Val:
    from oracle import oracle
    arr = oracle.evaluate(to_oracle_expr(expr), table).to_array(table.num_rows)
    return R.Val(arr.type, R.column_values(arr))


def _outcome(fn):
    """('ok', value) or ('error', the reference's message prefix)"""
    try:
        return "ok", fn()
    except (R.ExprError, ZeroDivisionError, OverflowError) as e:
        prefix = R.error_prefix(str(e))
        assert prefix is not None, repr(e)
        return "error", prefix


# ------------------------------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("name", list(C.BUILDERS))
def test_reference_agrees_with_the_oracle(name):
    f, ref = C.family(name), C.reference(name)
    for nm, e in f.values + f.tris + f.preds:
        diff = R.same(_oracle(e, f.table), ref[nm])
        assert diff is None, f"{name}.{nm}: oracle against reference: {diff}"


@pytest.mark.parametrize("kind", C.ERROR_KINDS)
def test_reference_raises_the_oracles_errors_and_visits_no_null_row(kind):
    for pos in C.ERROR_POSITIONS:
        bad, null_left, null_right, e, prefix = C.error_tables(kind, pos)
        oe = to_oracle_expr(e)
        assert _outcome(lambda: R.evaluate(oe, bad)) == ("error", prefix)
        assert _outcome(lambda: _oracle(e, bad)) == ("error", prefix)
        for t in (null_left, null_right):
            want = R.evaluate(oe, t)
            assert want.vals[pos] is None and sum(v is None for v in want.vals) == 1
            assert R.same(_oracle(e, t), want) is None


@pytest.mark.parametrize("name", list(C.CAST_ERRORS))
def test_reference_raises_the_oracles_cast_errors(name):
    for pos in (0, 4096):
        bad, null, e, prefix = C.cast_error_tables(name, pos)
        assert _outcome(lambda: R.evaluate(to_oracle_expr(e), bad)) == ("error", prefix)
        assert _outcome(lambda: _oracle(e, bad)) == ("error", prefix)
        assert R.same(_oracle(e, null), R.evaluate(to_oracle_expr(e), null)) is None


def test_scales_beyond_22_are_left_out():
    t = pa.table({"d": E.from_raw([1], pa.decimal128(38, 23)), "f": E.from_raw([E.f64_bits(1.0)], pa.float64())})
    with pytest.raises(NotImplementedError):
        R.evaluate(("cast", ("col", "d"), pa.float64()), t)
    with pytest.raises(NotImplementedError):
        R.evaluate(("cast", ("col", "f"), pa.decimal128(38, 23)), t)


# ------------------------------------------------------------------------------------------ the reference against Python's calendar
def test_date_part_agrees_with_datetime_date():
    """every seventh day of years 1 to 9999, and the first and last day of every month"""
    first, last = datetime.date(1, 1, 1).toordinal(), datetime.date(9999, 12, 31).toordinal()
    ordinals = set(range(first, last + 1, 7)) | {last}
    for y in range(1, 10000):
        for m in range(1, 13):
            o = datetime.date(y, m, 1).toordinal()
            ordinals.add(o)
            ordinals.add(max(o - 1, first))
    epoch = datetime.date(1970, 1, 1).toordinal()
    for o in ordinals:
        d = datetime.date.fromordinal(o)
        assert R.ymd(o - epoch) == (d.year, d.month, d.day), o
    assert R.ymd(0) == (1970, 1, 1) and R.ymd(-719163) == (0, 12, 31) and R.ymd(-719468) == (0, 3, 1) and R.ymd(-719469) == (0, 2, 29)
    assert R.ymd(2932897) == (10000, 1, 1) and R.ymd(E.I32_MIN) == (-5877641, 6, 23) and R.ymd(E.I32_MAX) == (5881580, 7, 11)


# --------------------------------------------------------------------------------------------------------------- wrong evaluators
def _cols(name, *names):
    t = C.family(name).table
    return [R.column_values(t.column(n)) for n in names]


def _differs(name, expr_name, wrong, *cols) -> int:
    """rows, valid in every input, where the reference's value is not what `wrong(*inputs)` gives"""
    ref = C.reference(name)[expr_name].vals
    rows = 0
    for i, args in enumerate(zip(*_cols(name, *cols))):
        if any(a is None for a in args):
            continue
        assert ref[i] is not None
        rows += ref[i] != wrong(*args)
    return rows


F = lambda bits: Fraction(E.f64_from_bits(bits))
_finite = lambda *bits: all(math.isfinite(E.f64_from_bits(b)) for b in bits)


def _once(q: Fraction) -> int:
    """an exact value rounded to a double once"""
    try:
        return R.bits_of(float(q))
    except OverflowError:
        return E.f64_bits(math.inf if q > 0 else -math.inf)


def test_float_table_tells_a_fused_multiply_add_from_two_roundings():
    ref = C.reference("float")
    rows = {"fma": 0, "fms2": 0, "c_plus": 0}
    for i, (a, b, c, d) in enumerate(zip(*_cols("float", "a", "b", "c", "d"))):
        if None in (a, b, c, d) or not _finite(a, b, c, d):
            continue
        exact = F(a) * F(b)
        if exact + F(c) != 0:   # (an exact zero's sign depends on the operands' signs, not on the roundings)
            rows["fma"] += ref["fma"].vals[i] != _once(exact + F(c))
            rows["c_plus"] += ref["c_plus"].vals[i] != _once(exact + F(c))
        if exact - F(c) * F(d) != 0:
            rows["fms2"] += ref["fms2"].vals[i] != _once(exact - F(c) * F(d))
    assert min(rows.values()) >= 100, rows


def test_int32_table_tells_a_result_left_at_64_bits():
    for nm, op in (("add", lambda a, b: a + b), ("sub", lambda a, b: a - b), ("mul", lambda a, b: R.wrap(a * b, 64))):
        assert _differs("int32", nm, op, "a", "b") >= 100, nm
    # widened without the 32-bit wrap first
    assert _differs("int32", "widen", lambda a, b: R.wrap((a + b) * b, 64), "a", "b") >= 100


def test_int64_table_tells_arithmetic_done_in_doubles():
    def in_doubles(op):
        def f(a, b):
            r = op(float(a), float(b))
            return R.wrap(int(r), 64)
        return f
    for nm, op in (("add", lambda x, y: x + y), ("sub", lambda x, y: x - y), ("mul", lambda x, y: x * y)):
        assert _differs("int64", nm, in_doubles(op), "a", "b") >= 100, nm


def test_decimal_table_tells_an_addition_that_forgets_to_rescale():
    assert _differs("decmix", "add", lambda d, e: R.wrap(d + e, 128), "d", "e") >= 100
    assert _differs("dec38", "add_scales", lambda a, e: R.wrap(a + e, 128), "a", "e") >= 100


@pytest.mark.parametrize("name", ["div_int32", "div_int64"])
def test_division_tables_tell_a_remainder_with_the_divisors_sign(name):
    assert _differs(name, "mod", lambda a, b: a % b, "a", "b") >= 100          # Python's % floors: the divisor's sign


def test_cast_table_tells_the_wrong_float_to_decimal_roundings():
    up = lambda f: math.floor(F(f) + Fraction(1, 2))                            # floor(x + 0.5), exactly
    even = lambda f: round(F(f))                                                 # Python rounds a Fraction half to even
    assert _differs("casts_declined", "f_dec0", up, "f0") >= 100
    assert _differs("casts_declined", "f_dec0", even, "f0") >= 100


def test_cast_table_tells_a_truncating_int64_to_float64():
    def trunc(p):
        m = abs(p)
        shift = max(m.bit_length() - 53, 0)
        return R.bits_of(math.copysign(float((m >> shift) << shift), p))
    assert _differs("casts_fused", "i64_f64", trunc, "p") >= 100


def test_cmp_table_tells_ieee_from_total_order_between_literals():
    ref = C.reference("cmp")
    n = C.N
    ieee = {"nan_eq_nan": math.nan == math.nan, "nan_lt_nan": False, "zero_lt": -0.0 < 0.0, "zero_eq": -0.0 == 0.0, "zero_ge": -0.0 >= 0.0, "inf_lt_nan": math.inf < math.nan}
    total = {"nan_eq_nan": True, "nan_lt_nan": False, "zero_lt": True, "zero_eq": False, "zero_ge": False, "inf_lt_nan": True, "nan_ne_payload": True}
    for nm, want in total.items():
        assert ref[nm].vals == [want] * n, nm
    assert sum(ieee[nm] != total[nm] for nm in ieee) >= 4
    assert ref["lits_all"].vals == [True] * n
    x = _cols("cmp", "x")[0]
    assert sum(1 for v, r in zip(x, ref["x_and_fold"].vals) if v is not None and r is True) >= 100      # IEEE: no row at all


def test_min_mod_minus_one_is_zero_and_min_div_minus_one_overflows():
    for typ, lo in ((pa.int32(), E.I32_MIN), (pa.int64(), E.I64_MIN), (pa.decimal128(38, 0), C.I128_MIN)):
        t = pa.table({"a": E.from_raw([lo], typ), "b": E.from_raw([-1], typ)})
        assert _outcome(lambda: R.evaluate(("bin", "%", ("col", "a"), ("col", "b")), t).vals) == ("ok", [0])
        assert _outcome(lambda: R.evaluate(("bin", "/", ("col", "a"), ("col", "b")), t).vals) == ("error", R.OVERFLOW)
    a, b = _cols("div_int32", "a", "b")
    assert sum(1 for x, y in zip(a, b) if x == E.I32_MIN and y == -1) >= 1       # the clean table holds the pair (an evaluator that raises fails it)


def test_date_table_tells_a_truncating_era_division():
    def truncating(days, part):
        div = lambda x, y: int(x / y) if abs(x) < 2**52 else None     # C's `/`: toward zero
        z = days + 719468
        era = div(z, 146097)
        doe = z - era * 146097
        yoe = div(doe - div(doe, 1460) + div(doe, 36524) - div(doe, 146096), 365)
        doy = doe - (365 * yoe + div(yoe, 4) - div(yoe, 100))
        mp = div(5 * doy + 2, 153)
        d, m = doy - div(153 * mp + 2, 5) + 1, (mp + 3 if mp < 10 else mp - 9)
        return {"year": yoe + era * 400 + (1 if m <= 2 else 0), "month": m, "day": d}[part]
    for part in ("year", "month", "day"):
        assert _differs("date", part, lambda d, part=part: truncating(d, part), "dt") >= 100, part
    # and the same formula with the floor it needs is the reference: the difference above is the truncation alone
    t = C.family("date").table
    for d in R.column_values(t.column("dt"))[:200]:
        if d is not None and d + 719468 >= 0:
            assert tuple(truncating(d, p) for p in ("year", "month", "day")) == R.ymd(d)

"""The truth the expression-value tests compare with: `+ - * / %`, CAST, comparisons, date_part, Kleene logic and CASE over columns
of Python values, one exact result per row.

An expression is the oracle's tuple form (oracle/oracle.py; tests.util.to_oracle_expr produces it), a table is a pyarrow Table.  Inside,
a column is a list of raw Python values with None for NULL: Python ints for Int32 / Int64 / Date32 / UInt8 / UInt32 and for the unscaled
value of a Decimal128, the 64-bit pattern for a Float64, bool for a Boolean.  Nothing here is numpy arithmetic or a call into C:
integers are Python integers wrapped to their width by hand, decimals wrap at 128 bits (the contract stated at the top of
csrc/expr.hip), a Float64 node is one Python float operation (IEEE double, one rounding per node), roundings of casts go through
fractions.Fraction, and the calendar counts 400 / 100 / 4 / 1-year cycles from 0001-01-01.

A Float64 result that is NaN is kept as NAN, which is no 64-bit pattern: `same` compares it as "is NaN" and everything else by its
bits.  Which NaN an operation returns (0 * inf is a negative NaN on x86 and a positive one on the GPU) is the platform's choice, and the
total order puts the two at opposite ends: a comparison that reads a computed NaN is AMBIGUOUS.  Kleene AND / OR absorb it where
the other side decides (FALSE AND x, TRUE OR x), so a predicate can guard it away; an AMBIGUOUS that reaches a result, a CASE condition
or a filter is an error of the test that wrote the expression.

Errors are ExprError with the reference's message prefix (`.prefix`): a zero divisor in a row that is valid on both sides, MIN / -1 or a
decimal operand times its power of ten leaving 128 bits, a Float64 that does not reach an i128 or the target precision, a decimal
beyond the target precision after a scale-down.  NULL rows are never visited.  MIN % -1 is 0.

Left out on purpose: Decimal128 -> Float64 from a source scale above 22, and Float64 -> Decimal128 to one.  Up to 22, 10^s is exact in a
double, so `pow`, `powi` and Python agree on the divisor; above it they may not, and nothing here decides between them: `evaluate`
raises NotImplementedError."""
import datetime
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import pyarrow as pa

from tests import edge_values as E

NAN = -1                      # a computed NaN (as bits for an operand: an all-ones pattern, itself a NaN)


class _Ambiguous:
    def __repr__(self):
        return "AMBIGUOUS"


AMBIGUOUS = _Ambiguous()
DIV_ZERO = "Arrow error: Divide by zero error"
OVERFLOW = "Arrow error: Arithmetic overflow"
CAST_OVERFLOW = "Arrow error: Cast error: Cannot cast to"
TOO_LARGE = "Arrow error: Invalid argument error"
PREFIXES = (DIV_ZERO, OVERFLOW, CAST_OVERFLOW, TOO_LARGE)
MAX_FLOAT_SCALE = 22


class ExprError(Exception):
    def __init__(self, prefix, detail=""):
        super().__init__(prefix + detail)
        self.prefix = prefix


def error_prefix(message: str):
    """which of the reference's errors a message is, or None"""
    return next((p for p in PREFIXES if str(message).startswith(p)), None)


class Val:
    """a typed column of raw values (None = NULL)"""

    def __init__(self, typ, vals):
        self.typ, self.vals = typ, vals


def wrap(v: int, bits: int) -> int:
    """two's complement: v modulo 2^bits as a signed integer"""
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def width(typ) -> int:
    if pa.types.is_decimal128(typ):
        return 128
    if pa.types.is_int32(typ) or pa.types.is_date32(typ):
        return 32
    if pa.types.is_int64(typ):
        return 64
    raise TypeError(f"no signed integer arithmetic on {typ}")


def bits_of(x: float) -> int:
    return NAN if x != x else E.f64_bits(x)


def total_key(bits: int) -> int:
    """f64::total_cmp: the pattern as a signed integer, the magnitude bits flipped under a set sign"""
    b = wrap(bits, 64)
    return b ^ 0x7FFFFFFFFFFFFFFF if b < 0 else b


def _dec(p, s):
    return pa.decimal128(min(38, p), min(38, s))


def result_type(op, lt, rt):
    """csrc/expr.hip arith_result_type"""
    if pa.types.is_decimal128(lt) and pa.types.is_decimal128(rt):
        p1, s1, p2, s2 = lt.precision, lt.scale, rt.precision, rt.scale
        if op == "/":
            s = min(38, s1 + 4)
            return _dec(s - s1 + s2 + p1, s)
        if op == "%":
            s = max(s1, s2)
            return _dec(s + min(p1 - s1, p2 - s2), s)
        if op == "*":
            return _dec(p1 + p2 + 1, s1 + s2)
        s = max(s1, s2)
        return _dec(s + max(p1 - s1, p2 - s2) + 1, s)
    if lt != rt:
        raise TypeError(f"arithmetic operand types differ: {lt} vs {rt}")
    if not (pa.types.is_int32(lt) or pa.types.is_int64(lt) or pa.types.is_float64(lt)):
        raise TypeError(f"arithmetic on {lt}")
    return lt


# ------------------------------------------------------------------------------------------------------------------- Float64 nodes
def float_op(op, xb: int, yb: int) -> int:
    x, y = E.f64_from_bits(xb), E.f64_from_bits(yb)
    if op == "+":
        r = x + y
    elif op == "-":
        r = x - y
    elif op == "*":
        r = x * y
    elif op == "/":
        if y == 0.0:
            r = math.nan if (x == 0.0 or x != x) else math.copysign(math.inf, x) * math.copysign(1.0, y)
        else:
            r = x / y
    else:
        r = math.nan if (x != x or y != y or math.isinf(x) or y == 0.0) else math.fmod(x, y)
    return bits_of(r)


# ------------------------------------------------------------------------------------------------------------------------ div, mod
def int_divmod(op, x: int, y: int, bits: int, la: int = 1, lb: int = 1) -> int:
    """arrow-arith div / rem of one valid row: operands first taken to the common scale (checked), truncation toward zero"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    x, y = x * la, y * lb
    if not (lo <= x <= hi and lo <= y <= hi):
        raise ExprError(OVERFLOW)
    if y == 0:
        raise ExprError(DIV_ZERO)
    if x == lo and y == -1:
        if op == "/":
            raise ExprError(OVERFLOW)
        return 0
    q = abs(x) // abs(y)
    q = -q if (x < 0) != (y < 0) else q
    return q if op == "/" else x - q * y


# --------------------------------------------------------------------------------------------------------------------------- casts
def round_half_away(q: Fraction) -> int:
    n = math.floor(abs(q) + Fraction(1, 2))
    return -n if q < 0 else n


def cast_value(v, frm, to):
    """one valid value"""
    if frm == to:
        return v
    f_dec, t_dec = pa.types.is_decimal128(frm), pa.types.is_decimal128(to)
    f_int = pa.types.is_int32(frm) or pa.types.is_int64(frm) or pa.types.is_uint8(frm) or pa.types.is_uint32(frm) or pa.types.is_date32(frm)
    if pa.types.is_int64(to) and (pa.types.is_int32(frm) or pa.types.is_uint8(frm) or pa.types.is_uint32(frm)):
        return v
    if (pa.types.is_int32(to) or pa.types.is_date32(to)) and (pa.types.is_int32(frm) or pa.types.is_date32(frm)):
        return v
    if pa.types.is_float64(to) and (pa.types.is_int32(frm) or pa.types.is_int64(frm)):
        return bits_of(float(v))                           # int -> float rounds to nearest, ties to even
    if pa.types.is_float64(to) and f_dec:
        if frm.scale > MAX_FLOAT_SCALE:
            raise NotImplementedError(f"cast {frm} -> Float64: scales above {MAX_FLOAT_SCALE} are left out")
        return bits_of(float(v) / float(10 ** frm.scale))
    if t_dec and pa.types.is_float64(frm):
        if to.scale > MAX_FLOAT_SCALE:
            raise NotImplementedError(f"cast Float64 -> {to}: scales above {MAX_FLOAT_SCALE} are left out")
        m = E.f64_from_bits(v) * float(10 ** to.scale)     # the product is a double, as in (v * 10^scale).round()
        if m != m or math.isinf(m) or not -2.0 ** 127 <= m < 2.0 ** 127:
            raise ExprError(CAST_OVERFLOW)
        d = round_half_away(Fraction(m))
        if abs(d) >= 10 ** to.precision:
            raise ExprError(TOO_LARGE)
        return d
    if t_dec and (f_dec or (f_int and not pa.types.is_uint32(frm) and not pa.types.is_date32(frm))):
        fs = frm.scale if f_dec else 0
        if to.scale >= fs:
            return wrap(v * 10 ** (to.scale - fs), 128)
        d = round_half_away(Fraction(v, 10 ** (fs - to.scale)))
        if abs(d) >= 10 ** to.precision:
            raise ExprError(TOO_LARGE)
        return d
    raise NotImplementedError(f"cast {frm} -> {to}")


# ------------------------------------------------------------------------------------------------------------------------ calendar
_DAYS_BEFORE = (0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334)


def ymd(days: int) -> tuple:
    """(year, month, day) of the proleptic Gregorian date `days` after 1970-01-01 (year 0 = 1 BC, astronomical numbering)"""
    n = days + 719162                                      # days after 0001-01-01
    n400, n = divmod(n, 146097)                            # Python's divmod floors: n is in [0, 146097) for any sign of days
    n100 = min(n // 36524, 3)
    n -= n100 * 36524
    n4, n = divmod(n, 1461)
    n1 = min(n // 365, 3)
    n -= n1 * 365
    year = 400 * n400 + 100 * n100 + 4 * n4 + n1 + 1
    leap = year % 4 == 0 and (year % 100 != 0 or year % 400 == 0)
    month = 12
    while n < _DAYS_BEFORE[month - 1] + (1 if leap and month > 2 else 0):
        month -= 1
    return year, month, n - _DAYS_BEFORE[month - 1] - (1 if leap and month > 2 else 0) + 1


def date_part(part: str, days: int) -> int:
    return ymd(days)[("year", "month", "day").index(part)]


# ------------------------------------------------------------------------------------------------------------------------- columns
def column_values(col) -> list:
    """a pyarrow column as raw values"""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    t = col.type
    if pa.types.is_boolean(t):
        return col.to_pylist()
    if pa.types.is_uint8(t):
        return col.to_pylist()
    w, valid = E.words_of(col)
    rows, ok = w.tolist(), valid.tolist()
    if pa.types.is_decimal128(t):
        return [E.unscaled(lo, hi) if v else None for (lo, hi), v in zip(rows, ok)]
    if pa.types.is_float64(t) or pa.types.is_unsigned_integer(t):
        return [r[0] if v else None for r, v in zip(rows, ok)]
    return [wrap(r[0], 64) if v else None for r, v in zip(rows, ok)]


def literal_value(value, typ):
    if value is None:
        return None
    if pa.types.is_boolean(typ):
        return bool(value)
    if pa.types.is_float64(typ):
        return E.f64_bits(float(value))                    # a literal is moved, not computed: its own bits
    if pa.types.is_decimal128(typ):
        with localcontext() as ctx:
            ctx.prec = 100
            return int(Decimal(str(value)).scaleb(typ.scale).to_integral_value())
    if pa.types.is_date32(typ) and isinstance(value, datetime.date):
        return (value - datetime.date(1970, 1, 1)).days
    return int(value)


def to_arrow(v: Val) -> pa.Array:
    if pa.types.is_boolean(v.typ) or pa.types.is_uint8(v.typ):
        return pa.array(_decided(v.vals, "a Boolean column"), type=v.typ)
    mask = [x is None for x in v.vals]
    return E.from_raw([0 if x is None else E.QNAN_BITS if x == NAN else x for x in v.vals], v.typ, mask if any(mask) else None)


def same(got: Val, want: Val):
    """None when the two columns agree in type, validity and bits (a NaN against any NaN), else a description of the first difference"""
    if got.typ != want.typ:
        return f"type {got.typ} != {want.typ}"
    if len(got.vals) != len(want.vals):
        return f"{len(got.vals)} rows != {len(want.vals)}"
    is_f = pa.types.is_float64(want.typ)
    nan = lambda b: (b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000
    _decided(want.vals, "the expected column")
    for i, (g, w) in enumerate(zip(got.vals, want.vals)):
        if g == w or (is_f and g is not None and w == NAN and nan(g)):
            continue
        fmt = (lambda b: None if b is None else f"{E.f64_from_bits(b)!r} (0x{b & (2**64 - 1):016x})") if is_f else repr
        return f"row {i}: got {fmt(g)}, want {fmt(w)}"
    return None


# ---------------------------------------------------------------------------------------------------------------------- evaluation
def _compare(op, x, y) -> bool:
    return {"=": x == y, "!=": x != y, "<": x < y, "<=": x <= y, ">": x > y, ">=": x >= y}[op]


def _kleene(op, a, b):
    if op == "and":
        if a is False or b is False:
            return False
        if a is AMBIGUOUS or b is AMBIGUOUS:
            return AMBIGUOUS
        return None if (a is None or b is None) else True
    if a is True or b is True:
        return True
    if a is AMBIGUOUS or b is AMBIGUOUS:
        return AMBIGUOUS
    return None if (a is None or b is None) else False


def _decided(vals, what):
    if any(v is AMBIGUOUS for v in vals):
        raise ValueError(f"{what} reads the order of a computed NaN")
    return vals


def evaluate(expr, table: pa.Table) -> Val:
    n = table.num_rows
    kind = expr[0]
    if kind == "col":
        c = table.column(expr[1])
        return Val(c.type, column_values(c))
    if kind == "lit":
        return Val(expr[2], [literal_value(expr[1], expr[2])] * n)
    if kind == "cast":
        a, to = evaluate(expr[1], table), expr[2]
        return Val(to, [None if v is None else cast_value(v, a.typ, to) for v in a.vals])
    if kind == "date_part":
        a = evaluate(expr[2], table)
        if not pa.types.is_date32(a.typ):
            raise TypeError(f"date_part over {a.typ}")
        return Val(pa.int32(), [None if v is None else date_part(expr[1], v) for v in a.vals])
    if kind == "is_null":
        return Val(pa.bool_(), [v is None for v in evaluate(expr[1], table).vals])
    if kind == "not":
        return Val(pa.bool_(), [v if (v is None or v is AMBIGUOUS) else not v for v in evaluate(expr[1], table).vals])
    if kind == "case":
        c, a = evaluate(expr[1], table), evaluate(expr[2], table)
        b = evaluate(expr[3], table) if expr[3] is not None else Val(a.typ, [None] * n)
        if a.typ != b.typ:
            raise TypeError(f"CASE branch types differ: {a.typ} vs {b.typ}")
        return Val(a.typ, [x if w is True else y for w, x, y in zip(_decided(c.vals, "a CASE condition"), a.vals, b.vals)])
    if kind != "bin":
        raise NotImplementedError(repr(expr))
    _, op, le, re_ = expr
    a, b = evaluate(le, table), evaluate(re_, table)
    if op in ("and", "or"):
        return Val(pa.bool_(), [_kleene(op, x, y) for x, y in zip(a.vals, b.vals)])
    both = lambda f: [None if (x is None or y is None) else f(x, y) for x, y in zip(a.vals, b.vals)]
    a_dec, b_dec = pa.types.is_decimal128(a.typ), pa.types.is_decimal128(b.typ)
    if op in ("=", "!=", "<", "<=", ">", ">="):
        if a_dec and b_dec:
            s = max(a.typ.scale, b.typ.scale)
            la, lb = 10 ** (s - a.typ.scale), 10 ** (s - b.typ.scale)
            return Val(pa.bool_(), both(lambda x, y: _compare(op, wrap(x * la, 128), wrap(y * lb, 128))))
        if pa.types.is_float64(a.typ) and pa.types.is_float64(b.typ):
            return Val(pa.bool_(), both(lambda x, y: AMBIGUOUS if NAN in (x, y) else _compare(op, total_key(x), total_key(y))))
        same_kind = a.typ == b.typ or {str(a.typ), str(b.typ)} == {"int32", "date32[day]"}
        if not same_kind or pa.types.is_floating(a.typ):
            raise TypeError(f"comparison operand types differ: {a.typ} vs {b.typ}")
        return Val(pa.bool_(), both(lambda x, y: _compare(op, x, y)))
    rt = result_type(op, a.typ, b.typ)
    if pa.types.is_float64(rt):
        return Val(rt, both(lambda x, y: float_op(op, x, y)))
    bits = width(rt)
    la = lb = 1
    if op in ("/", "%"):
        if a_dec:
            if op == "/":
                k = rt.scale - a.typ.scale + b.typ.scale
                la, lb = (10 ** k, 1) if k >= 0 else (1, 10 ** -k)
            else:
                la, lb = 10 ** (rt.scale - a.typ.scale), 10 ** (rt.scale - b.typ.scale)
        return Val(rt, both(lambda x, y: int_divmod(op, x, y, bits, la, lb)))
    if a_dec and op in "+-":
        la, lb = 10 ** (rt.scale - a.typ.scale), 10 ** (rt.scale - b.typ.scale)
    f = {"+": lambda x, y: x * la + y * lb, "-": lambda x, y: x * la - y * lb, "*": lambda x, y: x * y}[op]
    return Val(rt, both(lambda x, y: wrap(f(x, y), bits)))


def project(table: pa.Table, exprs) -> pa.Table:
    """exprs = [(expr, name)], as oracle.project"""
    return pa.Table.from_arrays([to_arrow(evaluate(e, table)) for e, _ in exprs], names=[nm for _, nm in exprs])


def filter_rows(table: pa.Table, predicate) -> list:
    """the indices of the rows a FilterExec keeps: the predicate is TRUE (NULL rows are dropped)"""
    return [i for i, v in enumerate(_decided(evaluate(predicate, table).vals, "a filter")) if v is True]

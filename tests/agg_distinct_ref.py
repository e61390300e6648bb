"""COUNT(DISTINCT x) / SUM(DISTINCT x) restated in plain Python: per group a set of the non-NULL values, the count its size, the sum
its members added up and wrapped like SUM's result type.  A FILTER makes the argument NULL where it is not TRUE; groups come in
first-seen order and exist whether any of their rows passes or not.

A table is {column: [python values]} with a type tag per column (TYPES / `types`): integers are Python ints, Decimal128 values are
their UNSCALED ints, Date32 values are day numbers, Float64 values are floats and are told apart by their BITS (the reference's
Hashable<T>: +0.0 and -0.0 are two values, two NaN payloads are two values, the same NaN is one), strings are str.

tests/test_agg_distinct_reference.py holds this file to hand-worked answers and to the oracle and shows which mistakes its case
tables catch; tests/test_zzzzzz_gpu_agg_distinct.py holds the GPU AggregateExec to it, exactly."""
import struct

DISTINCT = ("count_distinct", "sum_distinct")
# SUM's result type per argument type (sum.rs): signed 64 bits, unsigned 64 bits, or Decimal128's 128
SUM_BITS = {"i32": (64, True), "i64": (64, True), "u8": (64, True), "u32": (64, False), "u64": (64, False), "dec": (128, True)}
COUNT_TYPES = ("i32", "i64", "u8", "u32", "u64", "d32", "dec", "f64", "str")
DEC = (38, 2)                                         # the Decimal128 type of every "dec" column here
NAN_A = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NAN_B = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000001))[0]


def bits(v):
    """what makes two values of a column the same value"""
    return struct.pack("<d", v) if isinstance(v, float) else v


def wrap(total, typ):
    nbits, signed = SUM_BITS[typ]
    total &= (1 << nbits) - 1
    return total - (1 << nbits) if signed and total >> (nbits - 1) else total


def concat(tables):
    return {c: [v for t in tables for v in t[c]] for c in tables[0]}


def aggregate(table, keys, aggs, types):
    """aggs = [(func, arg, name, filter | None)], func in DISTINCT -> [{key..., name...}] in first-seen group order"""
    n = len(next(iter(table.values()))) if table else 0
    groups = {}
    for i in range(n):
        groups.setdefault(tuple(bits(table[k][i]) for k in keys), []).append(i)
    if not keys and not groups:
        groups[()] = []                                # no GROUP BY: one row even over no rows
    out = []
    for rows in groups.values():
        row = {k: table[k][rows[0]] for k in keys}
        for func, arg, name, flt in aggs:
            assert func in DISTINCT, func
            seen = {}
            for i in rows:
                v = table[arg][i]
                if v is None or (flt is not None and table[flt][i] is not True):
                    continue
                seen.setdefault(bits(v), v)
            if func == "count_distinct":
                row[name] = len(seen)
            else:
                row[name] = wrap(sum(seen.values()), types[arg]) if seen else None
        out.append(row)
    return out


def to_arrow(table, types=None, names=None):
    """the table as pyarrow: Decimal128 from the unscaled ints, Date32 from the day numbers"""
    import decimal

    import pyarrow as pa
    types = types or TYPES
    plain = {"i32": pa.int32(), "i64": pa.int64(), "u8": pa.uint8(), "u32": pa.uint32(), "u64": pa.uint64(), "f64": pa.float64(), "str": pa.string(), "bool": pa.bool_()}
    cols = {}
    for c in names or table:
        t = types[c]
        if t == "dec":
            with decimal.localcontext() as ctx:
                ctx.prec = 60
                cols[c] = pa.array([None if v is None else decimal.Decimal(v).scaleb(-DEC[1]) for v in table[c]], pa.decimal128(*DEC))
        elif t == "d32":
            cols[c] = pa.array(table[c], pa.int32()).cast(pa.date32())
        else:
            cols[c] = pa.array(table[c], plain[t])
    return pa.table(cols)


def from_arrow_value(v, typ):
    """a value of to_pylist() back in this file's terms"""
    import datetime
    import decimal
    if isinstance(v, decimal.Decimal):
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            return int(v.scaleb(DEC[1]))
    if isinstance(v, datetime.date):
        return (v - datetime.date(1970, 1, 1)).days
    return v


# ------------------------------------------------------------------------------------- case tables
I32, I64, U32, U64 = (-2**31, 2**31 - 1), (-2**63, 2**63 - 1), (0, 2**32 - 1), (0, 2**64 - 1)
EDGES = {
    "i32": [I32[0], I32[1], 0, -1, 1, 65536, 65537],
    "i64": [I64[0], I64[1], 0, -1, 5, 5 + 2**32, 5 + 2**33, -1 - 2**32],                 # pairs that agree in the low 32 bits only
    "u8": [0, 255, 1, 128],
    "u32": [0, U32[1], 1, 2**31, 2**31 + 1],
    "u64": [0, U64[1], 2**63, 2**63 + 1, 7, 7 + 2**32],                                   # above 2^63; low 32 bits shared
    "d32": [I32[0], I32[1], 0, -1, 19000],
    "dec": [0, -1, 10**37, -10**37, 3, 3 + 2**64, 3 + 2**65, 2**64, 2**64 + 1, -2**64 + 3],   # differ in the high word only / the low word only
    "f64": [0.0, -0.0, NAN_A, NAN_B, 1.5, -1.5, float("inf"), float("-inf"), 5e-324, 1.7976931348623157e308],
    "str": ["", "a", "b", "ab", "a" * 40, "é"],
}
TYPES = {"k": "i64", "k2": "i32", "p": "bool", "row": "i64", **{t: t for t in EDGES}}


def make_table(n, groups=7, seed=1):
    """n rows: key k cycles unevenly over `groups` values (so equal (group, value) pairs are rarely adjacent), every typed column walks
    its edge values with about 10 % NULLs, p is TRUE / FALSE / NULL, and group 3 (when it exists) has no row that passes p."""
    t = {c: [] for c in ["k", "k2", "p", "row"] + list(EDGES)}
    state = seed * 2654435761 % 2**32
    for i in range(n):
        state = (state * 1103515245 + 12345) % 2**31
        r = state >> 8
        k = (i * 5 + r % 3) % groups
        t["k"].append(k * 1000003 - 2 * 1000003)                  # sparse Int64 keys, some negative
        t["k2"].append(None if r % 11 == 0 else r % 2)
        t["row"].append(i)
        p = (True, True, False, None)[(r >> 3) % 4]
        t["p"].append(False if k == 3 and p is True else p)
        for c, edges in EDGES.items():
            t[c].append(None if (r >> 5) % 10 == 0 else edges[(r >> 9) % len(edges)])
    return t


def hand_table():
    """a few rows whose answers are worked by hand in the tests"""
    return {"k": [1, 2, 1, 1, 2, 3, 1, 3],
            "i64": [5, 5, None, 5 + 2**32, 7, None, 5, None],
            "f64": [0.0, 1.0, -0.0, 0.0, NAN_A, NAN_B, NAN_A, None],
            "dec": [3, 3 + 2**64, 3 + 2**64, 3, 10**37, None, 3, None],
            "u64": [2**63, 2**64 - 1, 2**63, 1, 2**64 - 1, None, 2**64 - 1, None],
            "p": [True, False, True, None, True, None, True, False]}


# the tables tests/test_agg_distinct_reference.py compares with the oracle and shows the mistakes on: (table, keys)
def case_tables():
    return {"hand": (hand_table(), ["k"]),
            "one_group": (make_table(65, groups=1), ["k"]),
            "seven_groups": (make_table(4097, groups=7), ["k"]),
            "two_keys": (make_table(4095, groups=7, seed=3), ["k", "k2"]),
            "no_group_by": (make_table(63, seed=5), []),
            "no_rows": (make_table(0), ["k"]),
            "no_rows_no_group_by": (make_table(0), [])}

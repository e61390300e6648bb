"""Inputs of the window tests in the plain form tests/window_ref.py reads ({name: list}, None = NULL, type tags), and their Arrow
form with a chosen value slot under every NULL.  `reference_table()` is the ~200-row table tests/test_window_reference.py holds the
restatement to the oracle on; it is built so that every mistake listed there changes a result."""
import datetime
from decimal import Decimal

import numpy as np
import pyarrow as pa

NP = {"int32": np.int32, "int64": np.int64, "uint8": np.uint8, "uint32": np.uint32, "uint64": np.uint64, "date32": np.int32, "float64": np.float64}
PA = {"int32": pa.int32(), "int64": pa.int64(), "uint8": pa.uint8(), "uint32": pa.uint32(), "uint64": pa.uint64(), "date32": pa.date32(),
      "float64": pa.float64()}


def arrow_type(tag):
    return pa.decimal128(tag[1], tag[2]) if isinstance(tag, tuple) else PA[tag]


def to_array(values, tag, fill=None):
    """an Arrow array over exactly these value slots: `fill` (default 77) is what lies under a NULL"""
    n = len(values)
    valid = np.array([v is not None for v in values], bool)
    fill = 77 if fill is None else fill
    slots = [fill if v is None else v for v in values]
    if isinstance(tag, tuple):
        data = b"".join(int(v).to_bytes(16, "little", signed=True) for v in slots)
    else:
        data = np.array(slots, dtype=NP[tag]).tobytes()
    vbuf = None if valid.all() else pa.py_buffer(np.packbits(valid.astype(np.uint8), bitorder="little").tobytes())
    return pa.Array.from_buffers(arrow_type(tag), n, [vbuf, pa.py_buffer(data)])


def to_arrow(cols, types, fill=None):
    return pa.table({k: to_array(v, types[k], (fill or {}).get(k)) for k, v in cols.items()})


def from_array(arr, tag):
    """an Arrow column back in the plain form: unscaled ints for decimals, days for dates"""
    arr = arr.combine_chunks() if isinstance(arr, pa.ChunkedArray) else arr
    if isinstance(tag, tuple):
        return [None if v is None else unscaled(v, tag[2]) for v in arr.to_pylist()]
    if tag == "date32":
        return arr.cast(pa.int32()).to_pylist()
    return arr.to_pylist()


def result_tag(func, tag):
    """the result's type tag: the GPU AggregateExec's rules"""
    if func == "count" or tag is None:
        return "int64"
    dec = isinstance(tag, tuple)
    if func == "sum":
        return ("decimal", min(38, tag[1] + 10), tag[2]) if dec else "float64" if tag == "float64" else "uint64" if tag in ("uint32", "uint64") else "int64"
    if func == "avg":
        return ("decimal", min(38, tag[1] + 4), min(38, tag[2] + 4)) if dec else "float64"
    return tag


# ---------------------------------------------------------------------------------------------------------------- the reference table
PARTITION_LENGTHS = (5, 59, 64, 1, 3, 40, 28)            # heads at rows 0, 5, 64, 128, 129, 132, 172: two of them on 64-row word edges
PARTITION_KEYS = ((None, None), (None, 3), (1, 3), (1, None), (1, 4), (2, 4), (2, 5))   # at rows 5, 128, 129 and 172 only p2 changes
ALL_NULL_PARTITION = 4                                    # its three rows carry no argument value at all
TYPES = {"p1": "int32", "p2": "int64", "o": "int32", "i32": "int32", "i64": "int64", "u32": "uint32", "d32": "date32", "f": "float64",
         "fe": "float64", "dec": ("decimal", 15, 2)}
ARGS = ("i32", "i64", "u32", "d32", "f", "fe", "dec")
FUNCS_OF = {"i32": ("sum", "count", "min", "max", "avg"), "i64": ("sum", "count", "min", "max", "avg"), "u32": ("sum", "count", "min", "max"),
            "d32": ("count", "min", "max"), "f": ("sum", "count", "avg"), "fe": ("count", "min", "max"), "dec": ("sum", "count", "min", "max", "avg")}
EDGE_FLOATS = (0.0, -0.0, float("nan"), -float("nan"), float("inf"), -float("inf"), 1.5, -1.5, 5e-324, -5e-324)


def reference_table(seed=20):
    """(cols, types): 200 rows in (p1, p2, o) order, NULLs in keys and arguments"""
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in TYPES}
    for part, (length, (p1, p2)) in enumerate(zip(PARTITION_LENGTHS, PARTITION_KEYS)):
        o = None if length > 2 else 0          # longer partitions begin with a peer group of NULL order keys
        for j in range(length):
            if j >= 2 and o is None:
                o = 0
            elif o is not None and rng.random() < 0.5:
                o += 1
            cols["p1"].append(p1)
            cols["p2"].append(p2)
            cols["o"].append(o)
            dead = part == ALL_NULL_PARTITION

            def put(name, v):
                cols[name].append(None if dead or rng.random() < 0.2 else v)
            put("i32", int(rng.integers(-1000, 1000)))
            put("i64", int(rng.integers(-10**12, 10**12)))
            put("u32", int(rng.integers(0, 2**32)))
            put("d32", int(rng.integers(-30000, 30000)))
            put("f", float(np.ldexp(rng.uniform(-1, 1), int(rng.integers(-40, 40)))))
            put("fe", EDGE_FLOATS[int(rng.integers(0, len(EDGE_FLOATS)))])
            put("dec", int(rng.integers(-10**13, 10**13)))
    return cols, dict(TYPES)


def frames(cols, partition_lengths, order_by):
    """(start, rows end, range end, partition end) per row from the partition lengths the table was built with; peers by == with
    None == None"""
    out, a = [], 0
    for length in partition_lengths:
        b = a + length
        for i in range(a, b):
            e = i
            while e + 1 < b and all(cols[k][e + 1] == cols[k][i] for k in order_by):
                e += 1
            out.append((a, i, e, b - 1))
        a = b
    return out


def days(d):
    return (d - datetime.date(1970, 1, 1)).days


def unscaled(d: Decimal, scale: int) -> int:
    """exact at any width (Decimal.scaleb would round to the context's 28 digits)"""
    sign, digits, exponent = d.as_tuple()
    assert exponent + scale >= 0
    v = int("".join(map(str, digits)) or "0") * 10 ** (exponent + scale)
    return -v if sign else v

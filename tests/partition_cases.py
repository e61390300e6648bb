"""Inputs of the partition tests (tests/test_gpu_partition.py on the device, tests/test_edge_values_oracle.py for the reference): every
partition count 1..64, the key kinds that choose between partition.hip's three counting kernels, tables wider than one scatter launch
takes, the second trip of the tile loop, skewed and empty inputs, the payloads that leave the zero-copy path, and the tables whose
partitions become the unaligned views fed to the other operators.  Tables are seeded and cached: the CPU and the GPU tests see the same
rows.  `reference` routes like the oracle (hash % nparts, input order kept) and restates what the library does to keys the oracle has
no type for: a Boolean key is hashed as one byte, a string key as a UInt64 hash of its bytes (strings.hip hash_bytes)."""
import functools

import numpy as np
import pyarrow as pa

from tests import edge_values as E

TILE = 1024                                   # rows per workgroup tile of both passes (partition.hip PT_TILE)
TILE_GRID = 2048                              # workgroups at most: more tiles than this and a workgroup takes a second one
N = 4 * TILE + 3                              # four full tiles and a three-row tail
TWO_TRIPS = TILE_GRID * TILE + TILE + 1       # the smallest input at which a workgroup takes a second tile, plus a one-row tail tile
SCATTER_COLS = 12                             # columns per scatter launch (PART_MAX_COLS)
ALL_COUNTS = tuple(range(1, 65))
KERNEL_COUNTS = (3, 8, 9, 16, 17, 33, 64)     # both sides of 8 | 9 (two or four packed counters) and of 16 | 17 (ballot counting), the end
SIZES = (1, 3, 4, 5, TILE - 1, TILE, TILE + 1, N)
MASK64 = 2**64 - 1
GOLDEN = 0x9E3779B97F4A7C15
SEED_BYTES = 0x51D7348D9B2F63A5               # device.hpp SEED_AGG: what hash_bytes starts from


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def _rows(n):
    return pa.array(np.arange(n, dtype=np.int64))


def _u8(rng, n):
    return pa.array(rng.integers(0, 256, n).astype(np.uint8))


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------- hashing in Python integers
def fmix64(x: int) -> int:
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & MASK64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & MASK64
    return x ^ x >> 33


def hash_raw(raw: int, typ: pa.DataType, seed: int) -> int:
    """one value's hash from its raw integer as edge_values builds it (float bits, day number, unscaled decimal): signed 32-bit values are
    sign-extended to a 64-bit word, a Decimal128 folds its high word in behind the low one"""
    h = fmix64((raw & MASK64) ^ seed ^ GOLDEN)
    return fmix64(((raw >> 64) & MASK64) ^ h) if pa.types.is_decimal128(typ) else h


def row_hashes(raws, types, seed=0) -> list:
    """create_hashes over key columns given as raw integers (None = NULL): the first column takes the seed, every later one the hash so
    far; a NULL leaves the hash as it is, and it starts at 0"""
    out = [0] * len(raws[0])
    for c, (col, typ) in enumerate(zip(raws, types)):
        for i, v in enumerate(col):
            if v is not None:
                out[i] = hash_raw(v, typ, seed if c == 0 else out[i])
    return out


def hash_bytes(b: bytes) -> int:
    """strings.hip hash_bytes: the length, then the bytes eight at a time as little-endian words, a zero-padded last word marked apart"""
    h = fmix64(len(b) ^ SEED_BYTES)
    k = 0
    while k + 8 <= len(b):
        h = fmix64(h ^ int.from_bytes(b[k:k + 8], "little"))
        k += 8
    if k < len(b):
        h = fmix64(h ^ int.from_bytes(b[k:], "little") ^ GOLDEN)
    return h


def _routing_column(col):
    """the column the routing hash is taken of: itself, or what the library puts in the place of a Boolean or string key"""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    t = col.type
    if pa.types.is_boolean(t):
        return col.cast(pa.uint8())
    if pa.types.is_dictionary(t):
        col, t = col.cast(pa.string()), pa.string()
    if pa.types.is_string(t):
        vals = col.to_pylist()
        return pa.array([0 if v is None else hash_bytes(v.encode()) for v in vals], pa.uint64(), mask=np.array([v is None for v in vals], dtype=bool))
    return col


def reference(table: pa.Table, keys, nparts: int):
    """(the nparts partitions in input order, the partition of every row) by the oracle's routing"""
    from oracle import oracle
    routed = pa.table({f"k{i}": _routing_column(table.column(k)) for i, k in enumerate(keys)})
    _, part = oracle.hash_partition(routed, routed.column_names, nparts)
    return [oracle.take(table, np.nonzero(part == p)[0].astype(np.int64)) for p in range(nparts)], part


# ------------------------------------------------------------------------------------------------------------ every count
@functools.lru_cache(maxsize=None)
def count_table(n=N):
    """an Int64 key at the edges of its type without NULLs (the typed kernel up to 16 partitions) and the row number"""
    return pa.table({"k": E.edge_array(_rng(1, n), n, pa.int64(), 0.4), "row": _rows(n)})


# -------------------------------------------------------------------------------------------------------------- key kinds
KEY_KINDS = {      # name: ((column, type, NULL fraction), ...)
    "int64": (("k", pa.int64(), 0.0),),
    "uint64": (("k", pa.uint64(), 0.0),),
    "int32": (("k", pa.int32(), 0.0),),
    "date32": (("k", pa.date32(), 0.0),),
    "uint32": (("k", pa.uint32(), 0.0),),
    "int64_nullable": (("k", pa.int64(), 0.1),),
    "int32_int64": (("k", pa.int32(), 0.0), ("k2", pa.int64(), 0.0)),
    "float64": (("k", pa.float64(), 0.0),),
    "decimal38": (("k", pa.decimal128(38, 0), 0.0),),
    "uint8": (("k", pa.uint8(), 0.0),),
}
TYPED_KINDS = ("int64", "uint64", "int32", "date32")          # one NULL-free column of 64 or of signed 32 bits: k_part_count2<.., KT_I64 / KT_I32>
FULL_CROSS = TYPED_KINDS + ("int64_nullable",)                # every count x every size; the other kinds hash row by row whatever the size


@functools.lru_cache(maxsize=None)
def key_table(kind, n):
    """(table of the kind's key columns and the row number, the key names)"""
    rng = _rng(2, list(KEY_KINDS).index(kind), n)
    cols = {}
    for name, typ, nulls in KEY_KINDS[kind]:
        cols[name] = _u8(rng, n) if typ == pa.uint8() else E.edge_array(rng, n, typ, 0.4, nulls)
    cols["row"] = _rows(n)
    return pa.table(cols), [name for name, _, _ in KEY_KINDS[kind]]


def kind_cases():
    """(kind, nparts, n): every kind at every kernel count with N rows and at every size with 3 and 17 partitions; the kinds that choose
    a kernel by their type or their NULLs at every count x size"""
    return [(kind, nparts, n) for kind in KEY_KINDS for nparts in KERNEL_COUNTS for n in SIZES if kind in FULL_CROSS or n == N or nparts in (3, 17)]


# -------------------------------------------------------------------------------------------------- more columns than a launch
WIDTH_TYPES = (pa.uint8(), pa.int32(), pa.int64(), pa.decimal128(38, 0), pa.float64(), pa.date32(), pa.uint64(), pa.uint32())   # 1, 4, 8, 16, 8, 4, 8, 4 bytes
WIDE_CASES = ((12, False), (13, False), (13, True), (24, False), (25, False), (25, True))      # (columns in all, the key is the last one)


@functools.lru_cache(maxsize=None)
def wide_table(ncols, key_last, n=N):
    """an Int64 key and ncols - 1 NULL-free payload columns of 1, 4, 8 and 16 bytes in turn, every column with values of its own"""
    rng = _rng(3, ncols, key_last, n)
    key = E.edge_array(rng, n, pa.int64(), 0.4)
    cols = {} if key_last else {"k": key}
    for i in range(ncols - 1):
        typ = WIDTH_TYPES[i % len(WIDTH_TYPES)]
        cols[f"p{i}"] = _u8(rng, n) if typ == pa.uint8() else E.edge_array(rng, n, typ, 0.3)
    if key_last:
        cols["k"] = key
    assert len(cols) == ncols
    return pa.table(cols)


# ------------------------------------------------------------------------------------------------------- the second tile
@functools.lru_cache(maxsize=None)
def two_trip_columns(n=TWO_TRIPS):
    """an Int32 key over its whole range (the extremes included) as numpy"""
    key = _rng(4, n).integers(E.I32_MIN, E.I32_MAX + 1, n).astype(np.int32)
    key[[0, n // 2, n - 1]] = (E.I32_MIN, E.I32_MAX, -1)
    return key


# ------------------------------------------------------------------------------------------------------ skew and empties
SKEWS = ("constant", "few_distinct", "all_null", "no_rows")
FEW = (E.I64_MIN, -1, 0, 7, E.I64_MAX)


@functools.lru_cache(maxsize=None)
def skew_table(shape, n=N):
    rng = _rng(5, SKEWS.index(shape))
    if shape == "no_rows":
        n = 0
    if shape == "constant":
        key = pa.array(np.full(n, 7, dtype=np.int64))
    elif shape == "all_null":
        key = pa.array(np.full(n, 7, dtype=np.int64), mask=np.ones(n, dtype=bool))
    else:
        key = pa.array(np.array(FEW, dtype=np.int64)[rng.integers(0, len(FEW), n)])
    return pa.table({"k": key, "row": _rows(n), "d": E.edge_array(rng, n, pa.decimal128(38, 0), 0.3), "c": _u8(rng, n)})


# --------------------------------------------------------------------------------------- payloads that leave the zero-copy path
WORDS = ("", "a", "pear", "12345678", "123456789", "Customer#000000001", "Zürich", "x" * 40)
FALLBACK_KINDS = ("nullable_int64", "boolean", "utf8", "dictionary", "all")
FALLBACK_SIZES = (65, N)


def _strings(rng, n, null_frac):
    pick, null = rng.integers(0, len(WORDS), n), rng.random(n) < null_frac
    return pa.array([None if m else WORDS[i] for i, m in zip(pick, null)], pa.string())


@functools.lru_cache(maxsize=None)
def fallback_table(kind, n):
    """an Int64 key, the row number and the payload(s) of the kind, every one with NULLs: a validity bitmap, a bit-packed Boolean or
    variable-length strings cannot be sliced at a row, so the partitions are compacted out one by one"""
    rng = _rng(6, FALLBACK_KINDS.index(kind), n)
    cols = {"k": E.edge_array(rng, n, pa.int64(), 0.4), "row": _rows(n)}
    if kind in ("nullable_int64", "all"):
        cols["ni"] = E.edge_array(rng, n, pa.int64(), 0.3, 0.1)
    if kind in ("boolean", "all"):
        cols["b"] = pa.array(rng.random(n) < 0.4, mask=rng.random(n) < 0.1)
    if kind in ("utf8", "all"):
        cols["s"] = _strings(rng, n, 0.1)
    if kind in ("dictionary", "all"):
        cols["ds"] = _strings(rng, n, 0.1).dictionary_encode()
    return pa.table(cols)


@functools.lru_cache(maxsize=None)
def odd_key_table(kind, n=N):
    """a Utf8 or a Boolean KEY with NULLs beside the row number and a NULL-free payload"""
    rng = _rng(7, len(kind), n)
    key = _strings(rng, n, 0.05) if kind == "utf8" else pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.05)
    return pa.table({"k": key, "row": _rows(n), "v": E.edge_array(rng, n, pa.float64(), 0.3)})


# ------------------------------------------------------------------------------------- tables whose partitions become views
VIEW_KEY = "pk"
VIEW_SIZES = {            # rows of partitions 0, 1, 2 -> partition 1 starts at row sizes[0], partition 2 at sizes[0] + sizes[1]
    "odd": (1003, 1002, 1001),          # starts 1003 and 2005: every column narrower than 16 bytes off its 16-byte boundary
    "mod4": (1001, 1001, 1000),         # starts 1001 = 1 (mod 4) and 2002 = 2 (mod 4): 4-byte columns 4 and 8 bytes off
    "blocks": (7, 8195, 8195),          # views of two 4096-row workgroups and a three-row tail, at rows 7 and 8202
}


@functools.lru_cache(maxsize=None)
def routed_values(nparts=3):
    """Int64 values by the partition the oracle routes them to: what a table with chosen partition sizes draws its key from"""
    from oracle import oracle
    cand = np.arange(-500, 500, dtype=np.int64)
    _, part = oracle.hash_partition(pa.table({"k": pa.array(cand)}), ["k"], nparts)
    out = [cand[part == p] for p in range(nparts)]
    assert all(len(v) > 100 for v in out)
    return out


def view_table(sizes, seed=0, wide=True):
    """rows for the operators behind a repartition, `sizes[p]` of them routed to partition p of 3 by the Int64 key `pk`, in mixed order:
      f, s, d     UInt8, UInt8, Date32 group keys of 3 x 2 x 40 values (the aggregate's direct table)
      a64, a32    strictly ascending NULL-free Int64 / Int32 (one-pass rank map builds, the window's order key), ~0.8 of their range used
      r64, r32    probe keys: values from the range of a64 / a32 and a little beyond it
      x32, xf, xd Int32, finite Float64 and Decimal128(15, 2) payloads (wide=False: x32 and xf only); row: the row number"""
    n = int(sum(sizes))
    rng = _rng(8, seed, n)
    values = routed_values(len(sizes))
    owner = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    pk = np.empty(n, np.int64)
    for p, vals in enumerate(values):
        pk[owner == p] = vals[rng.integers(0, len(vals), int(sizes[p]))]
    a64 = np.cumsum(1 + (rng.random(n) < 0.25)).astype(np.int64) - 1_000_037
    a32 = (np.cumsum(1 + (rng.random(n) < 0.25)) - 20_011).astype(np.int32)
    cols = {
        "f": pa.array(np.frombuffer(b"ANR", dtype=np.uint8)[rng.integers(0, 3, n)]),
        "s": pa.array(np.frombuffer(b"FO", dtype=np.uint8)[rng.integers(0, 2, n)]),
        "d": pa.array((8000 + rng.integers(0, 40, n)).astype(np.int32), pa.date32()),
        "a64": pa.array(a64), "a32": pa.array(a32),
        "r64": pa.array(rng.integers(a64[0] - 50, a64[-1] + 50, n)), "r32": pa.array(rng.integers(int(a32[0]) - 50, int(a32[-1]) + 50, n).astype(np.int32)),
        "x32": pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32)),
        "xf": pa.array(np.ldexp(rng.uniform(-1, 1, n), rng.integers(-20, 21, n))),
    }
    if wide:
        cols["xd"] = E.from_raw([int(v) for v in rng.integers(-10**12, 10**12, n)], pa.decimal128(15, 2))
    cols["row"] = _rows(n)
    cols[VIEW_KEY] = pa.array(pk)
    return pa.table(cols)


@functools.lru_cache(maxsize=None)
def view_source(name):
    return view_table(VIEW_SIZES[name], seed=list(VIEW_SIZES).index(name))

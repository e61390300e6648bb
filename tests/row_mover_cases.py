"""Inputs and references of the row-mover tests (tests/test_row_mover_reference.py on the CPU, tests/test_gpu_row_movers.py on the GPU):
filter compaction, take, slice and concat are held to pyarrow - Table.filter (a NULL mask slot drops the row), Table.take (a NULL id
gives a NULL row), Table.slice and pa.concat_tables - bit for bit.

Here: the "every type" table (a nullable and a NULL-free column of every type the library moves, built straight from buffers so that
the bits are what the builder says), the named selection patterns, the sizes at which the kernels change their path, the record-take
layouts with the record sizes they must get, and the exact comparison.  No GPU is needed to import or to check any of it."""
import functools

import numpy as np
import pyarrow as pa

# ---------------------------------------------------------------------------------------------------------------- sizes
# one lane, each side of one 64-row mask word, each side of one COMPACT_UNROLL group of four words (256 rows), and a ragged tail past
# 4096 rows (more than one workgroup of k_compact: a workgroup takes 16 words = 1024 rows)
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
# grid_for caps a launch at 2048 workgroups: the kernels that take one row per thread or one mask word per wave wrap their loop above
# 2048 * 256 = 524 288 rows, k_compact (four words per wave) above 2048 * 16 * 64 = 2 097 152 rows
WRAP_ROWS = 524_288 + 65
WRAP_COMPACT_ROWS = 2_097_152 + 65
WRAP_COLUMNS = ("b_n", "s_n", "i32", "v")               # at WRAP_ROWS
WRAP_COMPACT_COLUMNS = ("dec", "i64_n", "v")            # at WRAP_COMPACT_ROWS
MAX_COLS = 12          # filter.hip: byte-addressable columns per k_compact launch
GM_MAX = 16            # filter.hip: plain columns per k_gather_many launch
SMALL_TAKE_ROWS = 65_536   # filter.hip gather_columns: up to here a take of plain columns is one k_gather_many launch
PACK_MAX_COLS = 8      # records.hpp: fields per record
RECORD_MAX_BYTES = 64

F64_SPECIAL_BITS = (0x0000000000000000, 0x8000000000000000,        # +0.0, -0.0
                    0x7FF0000000000000, 0xFFF0000000000000,        # +inf, -inf
                    0x7FF8000000000123, 0xFFF80000DEADBEEF,        # quiet NaNs of both signs, each with a payload
                    0x7FF0000000000001)                            # a signalling NaN
STRINGS = ("", "a", "8 bytes!", "héllo wörld", "日本語テキスト", "x" * 257, "\U0001F642\U0001F642", "seven b",
           "nine byte", "0123456789abcdef0123456789abcdef")
DICT_WORDS = ("delta", "alpha", "", "écho", "charlie", "bravo", "zulu")     # (not in order: the indices are not ranks)

TYPES = {"i32": pa.int32(), "i64": pa.int64(), "u8": pa.uint8(), "u32": pa.uint32(), "u64": pa.uint64(), "d32": pa.date32(),
         "f64": pa.float64(), "dec": pa.decimal128(38, 0), "b": pa.bool_(), "s": pa.string(),
         "ds": pa.dictionary(pa.int32(), pa.string())}
NULLABLE_TYPES = dict(TYPES, ds=pa.dictionary(pa.uint8(), pa.string()))     # (the nullable dictionary column has UInt8 indices)
WIDTH = {"i32": 4, "i64": 8, "u8": 1, "u32": 4, "u64": 8, "d32": 4, "f64": 8, "dec": 16, "ds": 4, "v": 8}
# every column of the every-type table: `x` is NULL-free (imported without a validity buffer), `x_n` holds about 20 % NULLs
EVERY_TYPE_COLUMNS = tuple(k + sfx for k in TYPES for sfx in ("", "_n")) + ("v",)
# the byte-addressable ones (neither bit-packed nor Utf8): 9 types twice and the row number = 19 > MAX_COLS, so one filter over the
# whole table takes TWO k_compact launches (12 + 7 columns)
BYTE_ADDRESSABLE = tuple(c for c in EVERY_TYPE_COLUMNS if c.split("_")[0] not in ("b", "s"))
assert len(EVERY_TYPE_COLUMNS) == 23 and len(BYTE_ADDRESSABLE) == 19 and MAX_COLS < len(BYTE_ADDRESSABLE) <= 2 * MAX_COLS
# 18 NULL-free byte-addressable columns (> GM_MAX): a small take moves 16 of them in one k_gather_many launch, the rest one by one
PLAIN_18 = tuple(f"p{i}_{k}" for i, k in enumerate(("i64", "i32", "u8", "dec", "u64", "f64", "u32", "d32", "i64") * 2))


def _rng(*seed):
    return np.random.default_rng([abs(hash_name(s)) if isinstance(s, str) else int(s) for s in seed])


def hash_name(s):
    """a seed from a column name that does not change between processes (hash() of a str does)"""
    h = 0
    for ch in s.encode():
        h = (h * 131 + ch) % (2**31 - 1)
    return h


def _bitmap(bits):
    return pa.py_buffer(np.packbits(np.asarray(bits, dtype=bool), bitorder="little").tobytes())


def from_numpy(values, typ, null=None):
    """an Arrow array over exactly these bytes (no conversion looks at the values); null: Boolean numpy array, True = NULL; the value
    bytes (or bits) under a NULL stay what `values` holds"""
    n = len(values)
    data = _bitmap(values) if pa.types.is_boolean(typ) else pa.py_buffer(np.ascontiguousarray(values).tobytes())
    if null is None or not null.any():
        return pa.Array.from_buffers(typ, n, [None, data], null_count=0)
    return pa.Array.from_buffers(typ, n, [_bitmap(~null), data], null_count=int(null.sum()))


def decimal_halves(n, rng):
    """(n, 2) uint64: the low and high word of n Decimal128(38, 0) values, drawn independently; |value| < 2^125 < 10^38, and no high
    word is the sign extension of its low word (a mover that rebuilt the high word from the low one would be wrong on EVERY row)"""
    lo = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    hi = rng.integers(-2**61, 2**61, size=n, dtype=np.int64)
    ext = np.where(lo >> np.uint64(63) != 0, np.int64(-1), np.int64(0))
    hi = np.where(hi == ext, np.int64(5), hi)
    return np.stack([lo, hi.view(np.uint64)], axis=1)


def _values(kind, n, rng):
    if kind == "i32":
        v = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
        v[:2] = (-2**31, 2**31 - 1)[:n]
        return v
    if kind == "i64" or kind == "v":
        v = rng.integers(-2**63, 2**63 - 1, size=n, dtype=np.int64)
        v[:2] = (-2**63, 2**63 - 1)[:n]
        return v
    if kind == "u8":
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    if kind == "u32":
        v = rng.integers(0, 2**32, size=n, dtype=np.uint32)
        v[:1] = (2**32 - 1,)[:n]
        return v
    if kind == "u64":   # half of the values at and above 2^63
        v = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        v[:2] = (2**63, 2**64 - 1)[:n]
        return v
    if kind == "d32":
        return rng.integers(-200_000, 200_000, size=n, dtype=np.int64).astype(np.int32)
    if kind == "f64":   # any bit pattern, the special ones in the first rows and scattered after them
        bits = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        k = len(F64_SPECIAL_BITS)
        bits[:k] = np.array(F64_SPECIAL_BITS, dtype=np.uint64)[:n]
        at = np.arange(k, n, 11)
        bits[at] = np.array(F64_SPECIAL_BITS, dtype=np.uint64)[(at // 11) % k]
        return bits
    if kind == "dec":
        return decimal_halves(n, rng)
    if kind == "b":
        return rng.random(n) < 0.5
    raise KeyError(kind)


def _cycle_then_random(n, k, rng):
    """indices into k values: 0..k-1 first (every value is there once n >= k), then at random"""
    idx = rng.integers(0, k, size=n)
    idx[:k] = np.arange(k)[:n]
    return idx


def _validity_word_mix(n, rng):
    """True = NULL for about 20 % of the rows, with one whole 64-row word of NULLs and one without any where the table is long enough
    (a validity word of all zeros / all ones)"""
    null = rng.random(n) < 0.2
    if n >= 192:
        null[64:128] = True
        null[128:192] = False
    return null


@functools.lru_cache(maxsize=None)
def column(name, n, seed=0):
    """column `name` of the every-type table of n rows: the same values whichever other columns are built beside it"""
    if name == "v":
        return pa.array(np.arange(n, dtype=np.int64))
    parts = name.split("_")
    if parts[0][0] == "p" and parts[0][1:].isdigit():      # PLAIN_18: p<i>_<kind>, NULL-free
        return from_numpy(_values(parts[1], n, _rng(seed, n, name)), TYPES[parts[1]])
    kind, nullable = parts[0], name.endswith("_n")
    rng = _rng(seed, n, name)
    null = _validity_word_mix(n, rng) if nullable else None
    if kind == "s":
        words = pa.array(STRINGS, pa.string())
        out = words.take(pa.array(_cycle_then_random(n, len(STRINGS), rng), mask=null))
        return out if out.null_count else pa.Array.from_buffers(pa.string(), n, [None] + out.buffers()[1:], null_count=0, offset=out.offset)
    if kind == "ds":
        typ = (NULLABLE_TYPES if nullable else TYPES)["ds"]
        idx = from_numpy(_cycle_then_random(n, len(DICT_WORDS), rng).astype(np.uint8 if nullable else np.int32), typ.index_type, null)
        return pa.DictionaryArray.from_arrays(idx, pa.array(DICT_WORDS, pa.string()))
    return from_numpy(_values(kind, n, rng), TYPES[kind], null)


def table_of(columns, n, seed=0):
    return pa.Table.from_arrays([column(c, n, seed) for c in columns], names=list(columns))


def every_type_table(n, seed=0):
    return table_of(EVERY_TYPE_COLUMNS, n, seed)


# ---------------------------------------------------------------------------------------------------------------- selection patterns
# name -> n -> (selected, null): two Boolean numpy arrays; a row is kept where selected & ~null
def _only(*rows):
    def f(n):
        sel = np.zeros(n, bool)
        for r in rows:
            r = n + r if r < 0 else r
            if 0 <= r < n:
                sel[r] = True
        return sel, None
    return f


def _by_row(pred):
    return lambda n: (pred(np.arange(n)), None)


def _random(frac, seed):
    return lambda n: (_rng(seed, n).random(n) < frac, None)


def _half_with_nulls(n):
    """10 % of the slots are NULL and every one of them sits over a TRUE value: a mover that ignores mask_valid keeps them all"""
    rng = _rng(77, n)
    sel = rng.random(n) < 0.5
    null = sel & (rng.random(n) < 0.2)
    return sel, null


PATTERNS = {
    "none": _by_row(lambda i: i < 0),
    "all": _by_row(lambda i: i >= 0),
    "first_only": _only(0),
    "last_only": _only(-1),
    "row_63_only": _only(63),                                     # the last lane of the first mask word
    "row_64_only": _only(64),                                     # the first lane of the second
    "last_word_only": lambda n: (np.arange(n) >= ((n - 1) // 64) * 64, None),      # the ragged tail alone
    "alternate_rows": _by_row(lambda i: i % 2 == 0),
    "one_per_word": _by_row(lambda i: i % 64 == (i // 64 * 13) % 64),             # lane 13 w mod 64 of word w
    "alternate_words": _by_row(lambda i: (i // 64) % 2 == 0),
    "fourth_word_of_each_256": _by_row(lambda i: i % 256 >= 192),                # one word of each COMPACT_UNROLL group
    "sparse": _random(0.001, 71),
    "dense": _random(0.999, 72),
    "half": _random(0.5, 73),
    "half_with_nulls": _half_with_nulls,
}


def pattern_mask(name, n):
    """the pattern as a Boolean Arrow array; the value bit under a NULL slot is kept as the pattern sets it (TRUE)"""
    sel, null = PATTERNS[name](n)
    return from_numpy(sel, pa.bool_(), null)


def pattern_rows(name, n):
    """row numbers the pattern keeps, ascending"""
    sel, null = PATTERNS[name](n)
    return np.flatnonzero(sel if null is None else sel & ~null)


def with_masks(table, names=tuple(PATTERNS)):
    """the table with one Boolean column m_<pattern> per pattern"""
    for name in names:
        table = table.append_column("m_" + name, pattern_mask(name, table.num_rows))
    return table


# ---------------------------------------------------------------------------------------------------------------- record layouts
# (name, column kinds, (fields, bytes, record size) of every record the take must build - the widest columns go first, a record holds
#  at most 64 bytes and PACK_MAX_COLS fields, and a column left alone is taken by the per-column gather)
LAYOUTS = (
    ("r16", ("i64", "i32", "u8"), ((3, 13, 16),)),
    ("r32", ("dec", "i64", "i32"), ((3, 28, 32),)),
    ("r48", ("dec", "i64", "i64", "i64", "i32"), ((5, 44, 48),)),
    ("r64_exactly", ("dec",) * 4, ((4, 64, 64),)),
    ("r64_and_a_lone_column", ("dec",) * 5, ((4, 64, 64),)),                       # the fifth Decimal128 goes alone
    ("ten_u8", ("u8",) * 10, ((8, 8, 16), (2, 2, 16))),                             # split at PACK_MAX_COLS
    ("mixed", ("i64", "i64_n", "b", "s", "u32", "s_n", "u8"), ((3, 13, 16),)),      # nullable, Boolean, Utf8 stay out of the record
)
LAYOUT_NAMES = tuple(l[0] for l in LAYOUTS)


def layout(name):
    return next(l for l in LAYOUTS if l[0] == name)


def layout_columns(name):
    """[(column name of the layout's table, kind)]"""
    return [(f"c{i}_{k}", k) for i, k in enumerate(layout(name)[1])]


def packable(kind):
    return not kind.endswith("_n") and kind not in ("b", "s")


def record_groups(kinds):
    """what gather_columns must build for plain columns of these kinds (the others are skipped): [(fields, bytes, record size)];
    a restatement of its grouping from the comment above it, not of its code"""
    widths = sorted((WIDTH[k] for k in kinds if packable(k)), reverse=True)
    if len(widths) < 2:
        return []
    groups, at = [], 0
    while at < len(widths):
        fields = size = 0
        while at < len(widths) and fields < PACK_MAX_COLS and size + widths[at] <= RECORD_MAX_BYTES:
            size += widths[at]
            fields += 1
            at += 1
        if fields >= 2:
            groups.append((fields, size, (size + 15) // 16 * 16))
    return groups


@functools.lru_cache(maxsize=None)
def layout_table(name, n, seed=0):
    cols = []
    for cname, kind in layout_columns(name):
        if kind.endswith("_n") or kind in ("b", "s"):
            cols.append(column(kind, n, seed + 1 + len(cols)))
        else:
            cols.append(from_numpy(_values(kind, n, _rng(seed, n, name, cname)), TYPES[kind]))
    return pa.Table.from_arrays(cols, names=[c for c, _ in layout_columns(name)])


def drop_validity(table):
    """the same buffers without the validity buffers: every slot that was NULL now holds whatever bytes lay under it"""
    def plain(col):
        col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
        if pa.types.is_dictionary(col.type):
            return pa.DictionaryArray.from_arrays(plain(col.indices), col.dictionary)
        return pa.Array.from_buffers(col.type, len(col), [None] + col.buffers()[1:], null_count=0, offset=col.offset)
    return pa.Table.from_arrays([plain(c) for c in table.columns], names=table.column_names)


def permutation(n, seed=0, dtype=np.int32):
    return _rng(seed, n, "p").permutation(n).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- references
def ref_filter(table, mask):
    """arrow-select filter_record_batch: a FALSE or NULL mask slot drops the row"""
    return table.filter(mask, null_selection_behavior="drop")


def ref_take(table, ids):
    """arrow `take`: ids is a numpy array, a negative id stands for a NULL index and gives a row of NULLs"""
    ids = np.asarray(ids, dtype=np.int64)
    return table.take(pa.array(ids, mask=ids < 0))


def loop_filter(table, mask):
    """the same by a plain loop over Python values: {column: list}"""
    keep = [i for i, m in enumerate(mask.to_pylist()) if m is True]
    return {name: [vals[i] for i in keep] for name, vals in ((n, table.column(n).to_pylist()) for n in table.column_names)}


def loop_take(table, ids):
    return {name: [None if i < 0 else vals[i] for i in ids] for name, vals in ((n, table.column(n).to_pylist()) for n in table.column_names)}


# ---------------------------------------------------------------------------------------------------------------- exact comparison
def _plain(col):
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if pa.types.is_dictionary(col.type):
        return col.cast(pa.string())
    if pa.types.is_large_string(col.type):
        return col.cast(pa.string())
    return col


def bits_of(col):
    """(values, validity) as numpy arrays that compare bit for bit: Float64 by its 64-bit pattern, Decimal128 by both words, strings
    (dictionary columns decoded) as Python objects; the slots under a NULL are zeroed"""
    col = _plain(col)
    n, t = len(col), col.type
    valid = np.asarray(col.is_valid().to_numpy(zero_copy_only=False), dtype=bool) if n else np.zeros(0, bool)
    if pa.types.is_string(t):
        v = np.array(col.to_pylist(), dtype=object).reshape(n, 1)
        return v, valid
    if pa.types.is_boolean(t):
        v = np.asarray(col.fill_null(False).to_numpy(zero_copy_only=False), dtype=np.uint64).reshape(n, 1)
    elif pa.types.is_decimal128(t):
        v = np.frombuffer(col.buffers()[1], np.uint64, 2 * (n + col.offset))[2 * col.offset:].reshape(n, 2).copy()
    else:
        dt = {1: np.uint8, 4: np.uint32, 8: np.uint64}[t.bit_width // 8]
        v = np.frombuffer(col.buffers()[1], dt, n + col.offset)[col.offset:].astype(np.uint64).reshape(n, 1)
    return np.where(valid[:, None], v, np.uint64(0)), valid


def assert_same_bits(got, exp, what=""):
    """got == exp, in order: names, types (a dictionary column stays one and is compared as its strings), row count, the null_count of
    every column, and every value by its bits - never through `==` on floats"""
    assert got.column_names == exp.column_names, (what, got.column_names, exp.column_names)
    assert got.num_rows == exp.num_rows, (what, got.num_rows, exp.num_rows)
    for name in exp.column_names:
        g, e = got.column(name), exp.column(name)
        gt, et = g.type, e.type
        assert pa.types.is_dictionary(gt) == pa.types.is_dictionary(et), (what, name, gt, et)
        assert _plain(g).type == _plain(e).type, (what, name, gt, et)
        assert g.null_count == e.null_count, f"{what} column {name!r}: null_count {g.null_count}, want {e.null_count}"
        if not pa.types.is_floating(et) and _plain(g).equals(_plain(e)):
            continue     # (Arrow's equality is exact for everything but floats; what it rejects is worded below)
        (gv, gvalid), (ev, evalid) = bits_of(g), bits_of(e)
        bad = (gvalid != evalid) | (gv != ev).any(axis=1)
        if bad.any():
            r = int(np.flatnonzero(bad)[0])
            show = lambda v, ok: None if not ok[r] else [x if isinstance(x, str) else hex(int(x)) for x in v[r]]
            raise AssertionError(f"{what} column {name!r} row {r} of {len(bad)} ({int(bad.sum())} rows differ): got {show(gv, gvalid)}, want {show(ev, evalid)}")

"""Hand-built Parquet pages (tests/parquet_pages.py) at the bit widths, run shapes and byte positions at which csrc/parquet.hip takes
another branch — cases pyarrow's writer never produces: an index width that is not the minimal one (0..32), bit-packed runs at width 0,
600 run headers in a page (PQ_RB = 128), a bit-packed run longer than the LDS window (PQ_WIN = 8192), DELTA miniblocks of every width
0..64, 400 of them in a page and 128 of them in one block (PQ_DM = 64), definition levels that start anywhere in a 64-row word, v2 pages that clear is_compressed.

A case = the file's bytes, the column's values (Python ints; DOUBLE as its 64-bit patterns; str for strings; None for NULL — the values
the pages were BUILT from, not a decode of them) and the counts the host half must report.  NAMES lists them; case(name) builds one
(cached).  tests/test_parquet_page_reference.py holds pyarrow and the host half to them, tests/test_zzzzz_gpu_parquet_pages.py the GPU."""
import functools
import random
from dataclasses import dataclass, field

from tests import parquet_pages as W
from tests.parquet_pages import BOOLEAN, BYTE_ARRAY, DOUBLE, FIXED_LEN_BYTE_ARRAY, INT32, INT64, Chunk

I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2**31, 2**31 - 1, -2**63, 2**63 - 1


@dataclass
class Case:
    name: str
    data: bytes
    values: list
    counts: dict
    optional: bool = False
    kind: str = "fixed"        # fixed: a fixed-width target (device kernels) | bool | utf8 (host-planned) | dict_utf8 (indices on the device)
    codec: str = "none"
    widths: list = field(default_factory=list)   # DELTA: the width bytes the writer emitted


_BUILDERS = {}


def _case(name, **kw):
    def deco(fn):
        assert name not in _BUILDERS, name
        _BUILDERS[name] = functools.partial(fn, **kw)
        return fn
    return deco


def _finish(name, chunk: Chunk, values, kind="fixed", widths=None) -> Case:
    assert len(values) == chunk.counts["values"] and sum(v is None for v in values) == chunk.counts["nulls"], name
    return Case(name, chunk.file(), values, dict(chunk.counts), chunk.optional, kind, chunk.codec, widths or [])


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return _BUILDERS[name](name)


# ------------------------------------------------------------------------------------------------- dictionaries by type
# (physical type, kwargs of Chunk, PLAIN encoder, eight values: the type's extremes first)
F64 = [0x7FF8000000000001, 0xFFF0000000000000, 0x8000000000000000, 0x0000000000000001, 0x7FF0000000000000, 0xFFF800000000BEEF, 0x3FF0000000000000,
       0x800FFFFFFFFFFFFF]   # NaN with a payload, -inf, -0.0, the smallest subnormal, +inf, a negative NaN with a payload, 1.0, the largest negative subnormal


def flba_precision(length: int) -> int:
    """the most decimal digits `length` bytes of two's complement always hold"""
    p = 1
    while 10 ** (p + 1) - 1 <= 2 ** (8 * length - 1) - 1:
        p += 1
    return p


def flba_pool(length: int) -> list:
    lo, hi = -2 ** (8 * length - 1), 2 ** (8 * length - 1) - 1
    return [lo, hi, -1, 0, 1, hi // 3, lo // 3, hi - 1]


TYPES = {
    "int32": (INT32, {}, W.plain_int32, [I32_MIN, I32_MAX, 0, -1, 1, 123456789, -987654321, 0x00FF00FF]),
    "date32": (INT32, dict(converted=W.DATE), W.plain_int32, [I32_MIN, I32_MAX, 0, -1, 1, 8035, 19000, -719162]),
    "uint8": (INT32, dict(converted=W.UINT_8), W.plain_int32, [0, 255, 1, 127, 128, 200, 2, 254]),
    "uint32": (INT32, dict(converted=W.UINT_32), W.plain_int32, [0, 2**32 - 1, 2**31, 2**31 - 1, 1, 2**31 + 12345, 4000000000, 7]),
    "dec9": (INT32, dict(converted=W.DECIMAL, scale=2, precision=9), W.plain_int32, [-999999999, 999999999, 0, -1, 1, -12345, 31415926, -100]),
    "int64": (INT64, {}, W.plain_int64, [I64_MIN, I64_MAX, 0, -1, 1, 2**40 + 3, -(2**52) - 1, 0x0102030405060708]),
    "uint64": (INT64, dict(converted=W.UINT_64), W.plain_int64, [0, 2**64 - 1, 2**63, 2**63 - 1, 1, 2**63 + 987654321, 18000000000000000000, 9]),
    "dec18": (INT64, dict(converted=W.DECIMAL, scale=2, precision=18), W.plain_int64, [-(10**18) + 1, 10**18 - 1, 0, -1, 1, -123456789012, 31415926535897, -100]),
    "double": (DOUBLE, {}, W.plain_double_bits, F64),
}
for _l in range(1, 17):
    TYPES[f"flba{_l}"] = (FIXED_LEN_BYTE_ARRAY, dict(type_length=_l, converted=W.DECIMAL, scale=2 if _l > 1 else 0, precision=flba_precision(_l)),
                          functools.partial(W.plain_flba, length=_l), flba_pool(_l))


def _runs_for(shape, rng, limit):
    """shape = [("packed", n) | ("rle", n)] -> a run list with random indices below `limit`"""
    return [("rle", rng.randrange(limit), n) if k == "rle" else ("packed", [rng.randrange(limit) for _ in range(n)]) for k, n in shape]


PADDED_SHAPE = lambda n: [("packed", 16), ("rle", 2), ("packed", 504), ("rle", 300), ("packed", n - 822)]


# ------------------------------------------------------------------------------------------ A. dictionary index width
def _a_padded(name, bw, type_name="int32", rle_only=False):
    physical, kw, plain, pool = TYPES[type_name]
    rng = random.Random(1000 + bw)
    entries = pool[:min(7, 2 ** bw)]
    n = 1000 + bw
    runs = [("rle", 0, n)] if rle_only else _runs_for(PADDED_SHAPE(n), rng, len(entries))
    c = Chunk(physical, **kw)
    c.dictionary(plain(entries), len(entries))
    c.dict_page(runs, bw)
    return _finish(name, c, [entries[i] for i in W.expand_runs(runs)])


for _bw in range(33):
    _case(f"A_padded_w{_bw:02d}", bw=_bw)(_a_padded)
_case("A_padded_w00_rle_only", bw=0, rle_only=True)(_a_padded)
for _t in ("int64", "double", "flba7"):
    for _bw in (1, 7, 8, 9, 31, 32):
        _case(f"A_padded_{_t}_w{_bw:02d}", bw=_bw, type_name=_t)(_a_padded)


def _a_full(name, bw):
    import numpy as np
    size = 2 ** bw
    entries = (np.random.default_rng(bw).permutation(size).astype(np.int64) * 4093 - 2**31)      # distinct, inside Int32
    rng = random.Random(2000 + bw)
    runs = _runs_for([("packed", 64), ("rle", 5), ("packed", 934)], rng, size)
    runs[0][1][3], runs[0][1][4], runs[2][1][-1], runs[2][1][-2] = 0, size - 1, size - 1, 0      # both ends of the index range
    c = Chunk(INT32)
    c.dictionary(entries.astype("<i4").tobytes(), size)
    c.dict_page(runs, bw)
    return _finish(name, c, [int(entries[i]) for i in W.expand_runs(runs)])


for _bw in range(1, 21):
    _case(f"A_full_w{_bw:02d}", bw=_bw)(_a_full)


# --------------------------------------------------------------------------------------------------- B. run-stream shape
def _int32_dictionary(size, seed):
    rng = random.Random(seed)
    return [rng.randrange(I32_MIN, I32_MAX + 1) for _ in range(size)]


def _b(name, bw, dict_size, pages):
    """pages = [(width or None for bw, run list)]"""
    entries = _int32_dictionary(dict_size, 7)
    c = Chunk(INT32)
    c.dictionary(W.plain_int32(entries), dict_size)
    values = []
    for width, runs in pages:
        c.dict_page(runs, bw if width is None else width)
        values += [entries[i] for i in W.expand_runs(runs)]
    return _finish(name, c, values)


@_case("B1_600_run_headers")
def _b1(name):
    rng = random.Random(31)
    return _b(name, 13, 2**13, [(None, _runs_for([("packed", 8), ("rle", 3)] * 300, rng, 2**13))])


@_case("B2_packed_run_longer_than_the_window")
def _b2(name):
    rng = random.Random(32)
    return _b(name, 20, 70_000, [(None, _runs_for([("packed", 4096), ("rle", 500), ("packed", 77)], rng, 70_000))])


@_case("B3_seeded_run_list")
def _b3(name):
    rng = random.Random(33)
    shape, n = [], 0
    while n < 20_000:
        if rng.random() < 0.5:
            k = ("rle", rng.choice([1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513]))
        else:
            k = ("packed", 8 * rng.choice([1, 2, 63, 64, 65]))
        k = (k[0], min(k[1], 20_000 - n))
        shape.append(k)
        n += k[1]
    return _b(name, 13, 2**13, [(None, _runs_for(shape, rng, 2**13))])


@_case("B4_rle_counts_of_two_and_three_varint_bytes")
def _b4(name):
    rng = random.Random(34)
    return _b(name, 3, 7, [(None, _runs_for([("rle", 200), ("packed", 8), ("rle", 20_000), ("packed", 5)], rng, 7))])


@_case("B5_one_value_rle")
def _b5a(name):
    return _b(name, 3, 7, [(None, [("rle", 5, 1)])])


@_case("B5_one_value_packed")
def _b5b(name):
    return _b(name, 3, 7, [(None, [("packed", [6])])])


@_case("B6_three_pages_three_widths")
def _b6(name):
    rng = random.Random(36)
    return _b(name, None, 2**13, [(3, _runs_for([("packed", 40), ("rle", 21)], rng, 8)), (5, _runs_for([("packed", 3)], rng, 32)),
                                  (13, _runs_for([("rle", 100), ("packed", 900)], rng, 2**13))])


# -------------------------------------------------------------------------------------------------- C. definition levels
def _scattered(rng, n):
    bits = [int(rng.random() < 0.7) for _ in range(n)]
    bits[0], bits[-1] = 0, 1
    return bits


def _c_levels(rng):
    """[(rows, level runs)]: pages that start on and off 64-row words (rows before: 0, 61, 128, 129, 258, 770)"""
    return [
        (61, [("packed", _scattered(rng, 61))]),                                                   # a final packed group with padding
        (67, [("rle", 1, 30), ("rle", 0, 7), ("packed", _scattered(rng, 24)), ("rle", 1, 6)]),
        (1, [("rle", 1, 1)]),
        (129, [("rle", 0, 129)]),                                                                  # an all-NULL page between two others
        (512, [("rle", 1, 35), ("rle", 0, 200), ("packed", _scattered(rng, 64)), ("rle", 1, 213)]),   # 258 + 35 = 293 = 4 * 64 + 37
        (237, [("rle", 1, 100), ("rle", 0, 70), ("packed", _scattered(rng, 64)), ("rle", 1, 3)]),
    ]


def _c(name, encoding, version, all_valid=False):
    rng = random.Random(41)
    entries = [I32_MIN, I32_MAX, 0, -1, 1, 77, -77]
    c = Chunk(INT64 if encoding == "plain" else INT32, optional=True)
    if encoding == "dict":
        c.dictionary(W.plain_int32(entries), len(entries))
    values = []
    for rows, levels in ([(300, None)] if all_valid else _c_levels(rng)):
        valid = W.expand_runs(levels)[:rows] if levels else [1] * rows
        k = sum(valid)
        if encoding == "plain":
            dense = [rng.randrange(I64_MIN, I64_MAX + 1) for _ in range(k)]
            c.page(rows, W.PLAIN, W.plain_int64(dense), version=version, levels=levels)
        else:
            runs = _runs_for([("rle", k // 3), ("packed", k - k // 3)] if k >= 3 else [("packed", k)] if k else [], rng, len(entries))
            dense = [entries[i] for i in W.expand_runs(runs)]
            c.dict_page(runs, 3, num_rows=rows, version=version, levels=levels)
        it = iter(dense)
        values += [next(it) if v else None for v in valid]
    return _finish(name, c, values)


for _enc in ("plain", "dict"):
    for _v in (1, 2):
        _case(f"C_levels_{_enc}_v{_v}", encoding=_enc, version=_v)(_c)
_case("C_all_valid_plain_v1", encoding="plain", version=1, all_valid=True)(_c)
_case("C_all_valid_dict_v2", encoding="dict", version=2, all_valid=True)(_c)


# ------------------------------------------------------------------------------------------------ D. DELTA_BINARY_PACKED
def _delta(name, physical, pages, block=128, minis=4, optional=False, version=1, want_widths=None):
    """pages = [values with None for NULL]"""
    bits = 32 if physical == INT32 else 64
    c = Chunk(physical, optional=optional)
    values, widths = [], []
    for page in pages:
        dense = [v for v in page if v is not None]
        enc, w = W.delta_binary_packed(dense, block, minis, bits)
        widths += w
        levels = [("packed", [int(v is not None) for v in page])] if optional else None
        c.page(len(page), W.DELTA_BINARY_PACKED, enc, version=version, levels=levels)
        values += page
    if want_widths is not None:
        assert widths == want_widths, (name, widths, want_widths)      # the page holds the miniblocks it was built for
    return _finish(name, c, values, widths=widths)


def _delta_values_of_widths(widths, bits, rng, per=32, minis=4):
    """values whose miniblocks of `per` deltas come out at exactly `widths`: per block a min delta (the most negative number of the
    type where a miniblock needs every bit), per miniblock deltas above it with the width's top bit set in one and a zero in another"""
    mask = (1 << bits) - 1
    lo = -(1 << (bits - 1))
    values = [rng.randrange(lo, -lo)]
    for b in range(0, len(widths), minis):
        blk = widths[b:b + minis]
        md = lo if max(blk) == bits else -5
        for k, w in enumerate(blk):
            adj = [rng.randrange(1 << w) for _ in range(per)]
            if w:
                adj[1] |= 1 << (w - 1)
            if k == 0:
                adj[0] = 0                      # the block's min delta itself
            for a in adj:
                v = (values[-1] + md + a) & mask
                values.append(v - (1 << bits) if v >> (bits - 1) else v)
    return values


def _d_widths(name, physical, reverse):
    bits = 32 if physical == INT32 else 64
    widths = list(range(bits + 1))
    if reverse:
        widths.reverse()
    values = _delta_values_of_widths(widths, bits, random.Random(50 + bits + reverse))
    return _delta(name, physical, [values], want_widths=widths + [0] * (-len(widths) % 4))


for _p, _n in ((INT64, "int64"), (INT32, "int32")):
    _case(f"D_widths_{_n}_ascending", physical=_p, reverse=False)(_d_widths)
    _case(f"D_widths_{_n}_descending", physical=_p, reverse=True)(_d_widths)


def _delta_walk(rng, n, bits=64):
    lo = -(1 << (bits - 1))
    out = [rng.randrange(lo // 2, -lo // 2)]
    for i in range(n - 1):
        out.append(out[-1] + rng.randrange(-1000, 1 << rng.choice([3, 11, 20])))
    return out


def _d_shape(name, block, minis, count):
    return _delta(name, INT64, [_delta_walk(random.Random(block + minis + count), count)], block, minis)


for _block, _minis in ((128, 1), (128, 4), (256, 8), (2048, 64), (4096, 64)):
    for _label, _count in (("1", 1), ("2", 2), ("block", _block), ("block_plus_1", _block + 1), ("block_plus_2", _block + 2),
                           ("three_blocks_one_miniblock_one", 1 + 3 * _block + _block // _minis + 1)):
        _case(f"D_shape_{_block}_{_minis}_count_{_label}", block=_block, minis=_minis, count=_count)(_d_shape)


@_case("D_padded_partial_last_miniblock")
def _d_partial(name):
    return _delta(name, INT64, [_delta_walk(random.Random(61), 1 + 128 + 32 + 8)])


@_case("D_400_miniblocks")
def _d_400(name):
    return _delta(name, INT64, [_delta_walk(random.Random(62), 1 + 100 * 128)])


@_case("D_128_miniblocks_in_a_block")
def _d_128(name):
    """more miniblocks in ONE block than a batch of the device decoder holds (PQ_DM = 64): a block, a miniblock of the next, one more value"""
    return _delta(name, INT64, [_delta_walk(random.Random(65), 1 + 4096 + 32 + 1)], block=4096, minis=128)


@_case("D_block_of_two_million_values")
def _d_huge_block(name):
    """a declared block far larger than the page: 40 values of one delta, so every miniblock in use has width 0 and no bytes"""
    return _delta(name, INT64, [[100 + 7 * i for i in range(40)]], block=1 << 21, minis=64, want_widths=[0] * 64)


@_case("D_alternating_extremes_int64")
def _d_ext64(name):
    return _delta(name, INT64, [[I64_MIN if i % 2 else I64_MAX for i in range(300)]])


@_case("D_alternating_extremes_int32")
def _d_ext32(name):
    return _delta(name, INT32, [[I32_MIN if i % 2 else I32_MAX for i in range(300)]])


@_case("D_two_pages")
def _d_two(name):
    rng = random.Random(63)
    return _delta(name, INT64, [_delta_walk(rng, 200), _delta_walk(rng, 333)])


def _d_optional(name, version):
    rng = random.Random(64)
    pages = []
    for rows in (150, 1, 77):
        walk = iter(_delta_walk(rng, rows, 32))
        pages.append([None if rng.random() < 0.3 else next(walk) for _ in range(rows)])
    pages[1] = [12345]
    return _delta(name, INT32, pages, optional=True, version=version)


_case("D_optional_v1", version=1)(_d_optional)
_case("D_optional_v2", version=2)(_d_optional)


# ----------------------------------------------------------------- E. fixed-width PLAIN, dictionary and BYTE_STREAM_SPLIT
def _e(name, type_name, encoding):
    physical, kw, plain, pool = TYPES[type_name]
    rng = random.Random(sum(map(ord, type_name)))
    n = 257
    c = Chunk(physical, **kw)
    if encoding == "dict":
        runs = _runs_for([("packed", 96), ("rle", 57), ("packed", 104)], rng, len(pool))
        runs[0][1][:8] = range(8)
        values = [pool[i] for i in W.expand_runs(runs)]
        c.dictionary(plain(pool), len(pool))
        c.dict_page(runs, 3)
    else:
        lo, hi = (0, 2**64 - 1) if type_name == "double" else (min(pool), max(pool))
        values = list(pool) + [rng.randrange(lo, hi + 1) for _ in range(n - 8)]      # (DOUBLE: any 64-bit pattern)
        raw = plain(values)
        width = len(raw) // n
        c.page(n, W.PLAIN if encoding == "plain" else W.BYTE_STREAM_SPLIT, raw if encoding == "plain" else W.byte_stream_split(raw, width))
    return _finish(name, c, values)


for _t in TYPES:
    _case(f"E_{_t}_plain", type_name=_t, encoding="plain")(_e)
    _case(f"E_{_t}_dictionary_w3", type_name=_t, encoding="dict")(_e)
for _t in ("double", "int32", "int64", "flba7"):
    _case(f"E_{_t}_byte_stream_split", type_name=_t, encoding="bss")(_e)


# ------------------------------------------------------------------------------- F. v2 pages and the compression flag
def _f(name, codec, encoding):
    """an optional column in a compressed chunk: a compressed dictionary page, v2 pages with is_compressed true / false / true / false,
    levels (never compressed) in front of each"""
    rng = random.Random(71)
    entries = [I32_MIN, I32_MAX, 0, -1, 1, 77, -77]
    c = Chunk(INT32 if encoding == "dict" else INT64, optional=True, codec=codec)
    if encoding == "dict":
        c.dictionary(W.plain_int32(entries * 40), len(entries) * 40)      # (repeats: a page the codec does shrink)
    values = []
    for rows, flag in ((700, True), (300, False), (1, True), (513, False), (900, True)):
        levels = [("rle", 1, rows // 2), ("packed", _scattered(rng, rows - rows // 2))] if rows > 1 else [("rle", 1, 1)]
        valid = W.expand_runs(levels)[:rows]
        k = sum(valid)
        if encoding == "dict":
            runs = _runs_for([("rle", k // 3), ("packed", k - k // 3)] if k >= 3 else [("packed", k)], rng, len(entries) * 40)
            dense = [(entries * 40)[i] for i in W.expand_runs(runs)]
            c.dict_page(runs, 9, num_rows=rows, version=2, levels=levels, is_compressed=flag)
        else:
            dense = [rng.choice([5, 5, 5, 2**40, -3]) for _ in range(k)]
            c.page(rows, W.PLAIN, W.plain_int64(dense), version=2, levels=levels, is_compressed=flag)
        it = iter(dense)
        values += [next(it) if v else None for v in valid]
    return _finish(name, c, values)


for _codec in ("snappy", "zstd"):
    for _enc in ("plain", "dict"):
        _case(f"F_{_codec}_{_enc}_mixed_is_compressed", codec=_codec, encoding=_enc)(_f)


# -------------------------------------------------------------------------------------------------------- G. BOOLEAN
@_case("G_boolean_plain_pages_of_13_and_70")
def _g_plain(name):
    rng = random.Random(81)
    c = Chunk(BOOLEAN)
    values = []
    for rows in (13, 70):
        page = [rng.randrange(2) for _ in range(rows)]
        c.page(rows, W.PLAIN, W.plain_boolean(page))
        values += page
    return _finish(name, c, values, kind="bool")


@_case("G_boolean_rle_packed_rle_packed")
def _g_rle(name):
    rng = random.Random(82)
    runs = [("packed", [rng.randrange(2) for _ in range(24)]), ("rle", 1, 100), ("packed", [rng.randrange(2) for _ in range(13)])]
    c = Chunk(BOOLEAN)
    c.page(137, W.RLE, W.rle_boolean(runs), version=2, index_runs=runs)
    return _finish(name, c, W.expand_runs(runs), kind="bool")


@_case("G_boolean_optional")
def _g_optional(name):
    rng = random.Random(83)
    c = Chunk(BOOLEAN, optional=True)
    values = []
    for rows in (70, 61):
        levels = [("rle", 1, 9), ("rle", 0, 20), ("packed", _scattered(rng, rows - 29))]
        page = [rng.randrange(2) if v else None for v in W.expand_runs(levels)[:rows]]
        c.page(rows, W.PLAIN, W.plain_boolean([v for v in page if v is not None]), levels=levels)
        values += page
    return _finish(name, c, values, kind="bool")


# ----------------------------------------------------------------------------------------------------- H. BYTE_ARRAY
STRINGS = ["zebra", "", "żółw", "alpha", "日本語", "mid", "Alpha", "zz top"]      # not ascending; "" and multi-byte UTF-8


def _h_dict(name, bw):
    rng = random.Random(90 + bw)
    limit = min(len(STRINGS), 2 ** bw)
    n = 1000 + bw
    runs = _runs_for(PADDED_SHAPE(n), rng, limit)
    c = Chunk(BYTE_ARRAY, converted=W.UTF8)
    c.dictionary(W.plain_byte_array(STRINGS), len(STRINGS))
    c.dict_page(runs, bw)
    return _finish(name, c, [STRINGS[i] for i in W.expand_runs(runs)], kind="dict_utf8")


for _bw in (1, 3, 8, 17):
    _case(f"H_string_dictionary_w{_bw:02d}", bw=_bw)(_h_dict)


@_case("H_plain_strings_read_as_utf8")
def _h_plain(name):
    rng = random.Random(95)
    c = Chunk(BYTE_ARRAY, converted=W.UTF8)
    values = []
    for rows in (61, 200):
        page = [rng.choice(STRINGS) + ("" if rng.random() < 0.5 else str(rng.randrange(1000))) for _ in range(rows)]
        c.page(rows, W.PLAIN, W.plain_byte_array(page))
        values += page
    return _finish(name, c, values, kind="utf8")


NAMES = list(_BUILDERS)


# ------------------------------------------------------------------------------------- an Arrow column as the cases' values
def column_values(col) -> list:
    """an Arrow (chunked) array as a case spells its values: ints; Float64 as bit patterns; Decimal128 as its unscaled integer; Date32 as
    days; Boolean as 0 / 1; strings as str (a dictionary-encoded column decoded first); None for NULL"""
    import numpy as np
    import pyarrow as pa
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if pa.types.is_dictionary(arr.type):
        arr = arr.cast(arr.type.value_type)
    t = arr.type
    valid = arr.is_valid().to_pylist()
    if pa.types.is_float64(t) or pa.types.is_decimal128(t):
        buf = arr.buffers()[1]
        if pa.types.is_float64(t):
            raw = np.frombuffer(buf, dtype="<u8", count=len(arr), offset=arr.offset * 8).tolist()
        else:
            b = buf.to_pybytes()[arr.offset * 16:(arr.offset + len(arr)) * 16]
            raw = [int.from_bytes(b[i:i + 16], "little", signed=True) for i in range(0, len(b), 16)]
        return [v if ok else None for v, ok in zip(raw, valid)]
    if pa.types.is_date32(t):
        arr = arr.cast(pa.int32())
    if pa.types.is_boolean(t):
        return [None if v is None else int(v) for v in arr.to_pylist()]
    return arr.to_pylist()

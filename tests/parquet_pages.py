"""A spec-level Parquet writer for tests: every byte of a page is chosen by the caller — the declared bit width of an index stream (which
need not be the minimal one), its run list, the DELTA block shape, the page version, the per-page `is_compressed` flag — where a
production writer picks them itself and so reaches a handful of the decoders' branches.  Plain Python over the format documents
(parquet.thrift, Encodings.md, the Thrift compact protocol); imports nothing of the library under test.  pyarrow's reader is the judge
of what is written here (tests/test_parquet_page_reference.py); pyarrow.Codec compresses page bodies.

    c = Chunk(INT32, optional=True)
    c.dictionary(plain_int32([7, 8, 9]), 3)
    c.dict_page([("packed", [0, 1, 2, 2, 1]), ("rle", 0, 40)], width=5, version=2, levels=[("rle", 1, 45), ("rle", 0, 3)])
    open(path, "wb").write(c.file())         # c.counts = what a reader's page walk must have counted
"""
import struct

BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY = range(8)
PLAIN, PLAIN_DICTIONARY, RLE, BIT_PACKED, DELTA_BINARY_PACKED, RLE_DICTIONARY, BYTE_STREAM_SPLIT = 0, 2, 3, 4, 5, 8, 9
UTF8, DECIMAL, DATE, UINT_8, UINT_16, UINT_32, UINT_64 = 0, 5, 6, 11, 12, 13, 14       # ConvertedType
CODECS = {"none": 0, "snappy": 1, "zstd": 6}                                         # CompressionCodec
PAGE_DATA, PAGE_DICTIONARY, PAGE_DATA_V2 = 0, 2, 3

# ------------------------------------------------------------------------------------------------ Thrift compact protocol
T_TRUE, T_FALSE, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_SET, T_MAP, T_STRUCT = range(1, 13)


def varint(v: int) -> bytes:
    assert v >= 0
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v: int) -> bytes:
    """a signed integer of up to 64 bits"""
    assert -(1 << 63) <= v < (1 << 63)
    return varint(((v << 1) ^ (v >> 63)) & ((1 << 64) - 1))


def _thrift_value(t: int, v) -> bytes:
    if t in (T_I16, T_I32, T_I64):
        return zigzag(v)
    if t == T_BYTE:
        return struct.pack("<b", v)
    if t == T_BINARY:
        v = v.encode() if isinstance(v, str) else bytes(v)
        return varint(len(v)) + v
    if t == T_STRUCT:
        return thrift_struct(v)
    if t == T_LIST:
        et, items = v
        head = bytes([(len(items) << 4) | et]) if len(items) < 15 else bytes([0xF0 | et]) + varint(len(items))
        return head + b"".join(bytes([1 if x else 2]) if et in (T_TRUE, T_FALSE) else _thrift_value(et, x) for x in items)
    raise ValueError(f"thrift type {t}")


def thrift_struct(fields) -> bytes:
    """fields = [(id, type, value)] in ascending id order; a bool is (id, T_TRUE, True / False); value None = field absent"""
    out, last = bytearray(), 0
    for fid, t, v in fields:
        if v is None:
            continue
        if t in (T_TRUE, T_FALSE):
            t = T_TRUE if v else T_FALSE
        assert fid > last
        out += bytes([((fid - last) << 4) | t]) if fid - last <= 15 else bytes([t]) + zigzag(fid)
        if t not in (T_TRUE, T_FALSE):
            out += _thrift_value(t, v)
        last = fid
    return bytes(out) + b"\x00"


# ----------------------------------------------------------------------------------------------------------- page headers
def dictionary_page_header(uncompressed: int, compressed: int, num_values: int, encoding: int = PLAIN) -> bytes:
    return thrift_struct([(1, T_I32, PAGE_DICTIONARY), (2, T_I32, uncompressed), (3, T_I32, compressed),
                          (7, T_STRUCT, [(1, T_I32, num_values), (2, T_I32, encoding)])])


def data_page_header(uncompressed: int, compressed: int, num_values: int, encoding: int) -> bytes:
    return thrift_struct([(1, T_I32, PAGE_DATA), (2, T_I32, uncompressed), (3, T_I32, compressed),
                          (5, T_STRUCT, [(1, T_I32, num_values), (2, T_I32, encoding), (3, T_I32, RLE), (4, T_I32, RLE)])])


def data_page_header_v2(uncompressed: int, compressed: int, num_values: int, num_nulls: int, encoding: int, def_bytes: int, is_compressed: bool) -> bytes:
    return thrift_struct([(1, T_I32, PAGE_DATA_V2), (2, T_I32, uncompressed), (3, T_I32, compressed),
                          (8, T_STRUCT, [(1, T_I32, num_values), (2, T_I32, num_nulls), (3, T_I32, num_values), (4, T_I32, encoding),
                                         (5, T_I32, def_bytes), (6, T_I32, 0), (7, T_TRUE, is_compressed)])])


# ------------------------------------------------------------------------------------------------------------ encodings
def pack_bits(values, width: int) -> bytes:
    """values of `width` bits each, LSB first, in ceil(len * width / 8) bytes"""
    acc = 0
    for i, v in enumerate(values):
        assert 0 <= v < (1 << width) or (width == 0 and v == 0), (v, width)
        acc |= v << (i * width)
    return acc.to_bytes((len(values) * width + 7) // 8, "little")


def hybrid(runs, width: int) -> bytes:
    """RLE / bit-packed hybrid: runs = [("rle", value, count) | ("packed", values)]; the last packed run is padded with zeros to whole
    groups of eight; `width` is the declared bit width (a run of width 0 has a header and no bytes)"""
    out = bytearray()
    for k, r in enumerate(runs):
        if r[0] == "rle":
            _, value, count = r
            assert count > 0 and 0 <= value < max(1 << width, 1)
            out += varint(count << 1) + value.to_bytes((width + 7) // 8, "little")
        else:
            vals = list(r[1])
            assert vals and (len(vals) % 8 == 0 or k == len(runs) - 1)       # padding inside a stream would be read as values
            groups = (len(vals) + 7) // 8
            out += varint((groups << 1) | 1) + pack_bits(vals + [0] * (groups * 8 - len(vals)), width)
    return bytes(out)


def expand_runs(runs) -> list:
    out = []
    for r in runs:
        out += [r[1]] * r[2] if r[0] == "rle" else list(r[1])
    return out


def count_runs(runs) -> tuple:
    """(RLE runs, bit-packed runs)"""
    return sum(r[0] == "rle" for r in runs), sum(r[0] == "packed" for r in runs)


def definition_levels(runs, version: int) -> bytes:
    """max definition level 1: bit width 1; a 4-byte length in front in a v1 page, the bare stream in v2"""
    s = hybrid(runs, 1)
    return struct.pack("<I", len(s)) + s if version == 1 else s


def plain_boolean(values) -> bytes:
    return pack_bits([int(bool(v)) for v in values], 1)


def plain_int32(values) -> bytes:
    return b"".join(struct.pack("<I", v & 0xFFFFFFFF) for v in values)


def plain_int64(values) -> bytes:
    return b"".join(struct.pack("<Q", v & 0xFFFFFFFFFFFFFFFF) for v in values)


plain_double_bits = plain_int64        # DOUBLE as its 64-bit patterns


def plain_flba(values, length: int) -> bytes:
    """big-endian two's complement in `length` bytes"""
    return b"".join(v.to_bytes(length, "big", signed=True) for v in values)


def plain_byte_array(values) -> bytes:
    raw = [v.encode() if isinstance(v, str) else bytes(v) for v in values]
    return b"".join(struct.pack("<I", len(b)) + b for b in raw)


def rle_boolean(runs) -> bytes:
    """BOOLEAN values with the RLE encoding: <4-byte length> hybrid runs of bit width 1"""
    s = hybrid(runs, 1)
    return struct.pack("<I", len(s)) + s


def delta_binary_packed(values, block: int = 128, minis: int = 4, bits: int = 64):
    """-> (bytes, the bit width bytes emitted, block after block).  Arithmetic modulo 2^bits (the physical type's width): a delta
    is the wrapped signed difference, a block's min delta the smallest of them, a miniblock's width the widest (delta - min delta).
    The last miniblock in use is padded to its full length; the miniblocks behind it have width 0 and no bytes."""
    assert block % 128 == 0 and block % minis == 0 and (block // minis) % 32 == 0 and values
    mask, per = (1 << bits) - 1, block // minis

    def signed(x):
        x &= mask
        return x - (1 << bits) if x >> (bits - 1) else x
    out = bytearray(varint(block) + varint(minis) + varint(len(values)) + zigzag(signed(values[0])))
    deltas = [signed(values[i + 1] - values[i]) for i in range(len(values) - 1)]
    emitted = []
    for b in range(0, len(deltas), block):
        blk = deltas[b:b + block]
        md = min(blk)
        adj = [d - md for d in blk]
        widths, body = [], bytearray()
        for m in range(minis):
            mb = adj[m * per:(m + 1) * per]
            if not mb:
                widths.append(0)
                continue
            w = max(x.bit_length() for x in mb)
            assert w <= bits
            widths.append(w)
            body += pack_bits(mb + [0] * (per - len(mb)), w)
        out += zigzag(md) + bytes(widths) + body
        emitted += widths
    return bytes(out), emitted


def byte_stream_split(plain: bytes, width: int) -> bytes:
    """PLAIN values of `width` bytes each -> byte k of every value, stream after stream"""
    assert len(plain) % width == 0
    return b"".join(plain[k::width] for k in range(width))


def compress(codec: str, body: bytes) -> bytes:
    if codec == "none":
        return body
    import pyarrow as pa
    return pa.Codec(codec).compress(body, asbytes=True)


# --------------------------------------------------------------------------------------------------- a one-column file
class Chunk:
    """One column chunk, page by page, and the file around it (one row group, one column).  `counts` follows what is added: what the
    walk of a reader over these pages must find."""

    def __init__(self, physical: int, *, type_length: int = 0, optional: bool = False, converted=None, scale: int = 0, precision: int = 0,
                 codec: str = "none", name: str = "c"):
        self.physical, self.type_length, self.optional, self.converted = physical, type_length, optional, converted
        self.scale, self.precision, self.codec, self.name = scale, precision, codec, name
        self.pages, self.encodings = [], {RLE}
        self.uncompressed_total = 0
        self.counts = dict(values=0, nulls=0, dictionary_values=0, n_dictionary_pages=0, n_data_pages_v1=0, n_data_pages_v2=0, n_plain_pages=0,
                           n_dictionary_encoded_pages=0, n_runs_rle=0, n_runs_bitpacked=0)

    def _add(self, header: bytes, body: bytes, uncompressed: int):
        self.pages.append(header + body)
        self.uncompressed_total += len(header) + uncompressed

    def dictionary(self, plain: bytes, num_values: int):
        body = compress(self.codec, plain)
        self._add(dictionary_page_header(len(plain), len(body), num_values), body, len(plain))
        self.encodings.add(PLAIN)
        self.counts["dictionary_values"] = num_values
        self.counts["n_dictionary_pages"] += 1

    def page(self, num_rows: int, encoding: int, values: bytes, *, version: int = 1, levels=None, is_compressed: bool = True, index_runs=None):
        """one data page of `num_rows` rows.  levels = the definition levels' run list (optional columns; None = every row valid, as
        one RLE run); values = the encoded non-null values; index_runs = the run list of a dictionary index / RLE Boolean stream, for
        the run counts alone"""
        nulls = 0
        lv = b""
        if self.optional:
            levels = levels or [("rle", 1, num_rows)]
            bits = expand_runs(levels)[:num_rows]            # (a packed run's padding is not rows)
            assert len(bits) == num_rows and sum(len(r[1]) if r[0] == "packed" else r[2] for r in levels[:-1]) < num_rows
            nulls = num_rows - sum(bits)
            lv = definition_levels(levels, version)
        else:
            assert levels is None
        if version == 1:
            raw = lv + values
            body = compress(self.codec, raw)
            self._add(data_page_header(len(raw), len(body), num_rows, encoding), body, len(raw))
            self.counts["n_data_pages_v1"] += 1
        else:
            packed = compress(self.codec, values) if is_compressed else values
            self._add(data_page_header_v2(len(lv) + len(values), len(lv) + len(packed), num_rows, nulls, encoding, len(lv), is_compressed),
                      lv + packed, len(lv) + len(values))
            self.counts["n_data_pages_v2"] += 1
        self.encodings.add(encoding)
        self.counts["values"] += num_rows
        self.counts["nulls"] += nulls
        self.counts["n_dictionary_encoded_pages" if encoding in (RLE_DICTIONARY, PLAIN_DICTIONARY) else "n_plain_pages"] += 1
        if index_runs is not None:
            r, p = count_runs(index_runs)
            self.counts["n_runs_rle"] += r
            self.counts["n_runs_bitpacked"] += p

    def dict_page(self, index_runs, width: int, num_rows=None, **kw):
        """a dictionary-encoded data page: the width byte, then the index runs; no runs (an all-NULL page) = the width byte alone in a
        v1 page and an empty value section in a v2 page"""
        n = len(expand_runs(index_runs))
        if index_runs:
            values = bytes([width]) + hybrid(index_runs, width)
        else:
            values = bytes([width]) if kw.get("version", 1) == 1 else b""
        self.page(n if num_rows is None else num_rows, RLE_DICTIONARY, values, index_runs=index_runs, **kw)

    def file(self) -> bytes:
        """"PAR1", the pages, FileMetaData, its length, "PAR1" """
        has_dict = self.counts["n_dictionary_pages"] > 0
        first_data = 4 + (len(self.pages[0]) if has_dict else 0)
        total = sum(len(p) for p in self.pages)
        column_meta = [(1, T_I32, self.physical), (2, T_LIST, (T_I32, sorted(self.encodings))), (3, T_LIST, (T_BINARY, [self.name])),
                       (4, T_I32, CODECS[self.codec]), (5, T_I64, self.counts["values"]), (6, T_I64, self.uncompressed_total), (7, T_I64, total),
                       (9, T_I64, first_data), (11, T_I64, 4 if has_dict else None)]
        leaf = [(1, T_I32, self.physical), (2, T_I32, self.type_length or None), (3, T_I32, 1 if self.optional else 0), (4, T_BINARY, self.name),
                (6, T_I32, self.converted), (7, T_I32, self.scale if self.converted == DECIMAL else None),
                (8, T_I32, self.precision if self.converted == DECIMAL else None)]
        root = [(4, T_BINARY, "schema"), (5, T_I32, 1)]
        row_group = [(1, T_LIST, (T_STRUCT, [[(2, T_I64, 4 + total), (3, T_STRUCT, column_meta)]])), (2, T_I64, self.uncompressed_total),
                     (3, T_I64, self.counts["values"])]
        footer = thrift_struct([(1, T_I32, 1), (2, T_LIST, (T_STRUCT, [root, leaf])), (3, T_I64, self.counts["values"]),
                                (4, T_LIST, (T_STRUCT, [row_group])), (6, T_BINARY, "tests/parquet_pages.py")])
        return b"PAR1" + b"".join(self.pages) + footer + struct.pack("<I", len(footer)) + b"PAR1"

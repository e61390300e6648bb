"""The references and case builders of the row-mover tests (tests/row_mover_cases.py), checked without a GPU: every selection pattern
selects the rows its name says, pyarrow's filter and take agree with a plain loop over Python values (NULLs included), the every-type
table holds the bit patterns it promises, every record layout has the size its case claims, and the exact comparison tells apart what
`==` does not."""
import struct

import numpy as np
import pyarrow as pa
import pytest

from tests import row_mover_cases as RC

SMALL = [n for n in RC.SIZES if n <= 257]


# ------------------------------------------------------------------------------------------------------------------ patterns
def _expected_rows(name, n):
    """the rows each name stands for, written out independently of RC.PATTERNS (None: a random pattern, held to its density below)"""
    rows = range(n)
    return {
        "none": [],
        "all": list(rows),
        "first_only": [0],
        "last_only": [n - 1],
        "row_63_only": [63] if n > 63 else [],
        "row_64_only": [64] if n > 64 else [],
        "last_word_only": [i for i in rows if i // 64 == (n - 1) // 64],
        "alternate_rows": [i for i in rows if i % 2 == 0],
        "one_per_word": [w * 64 + (13 * w) % 64 for w in range((n + 63) // 64) if w * 64 + (13 * w) % 64 < n],
        "alternate_words": [i for i in rows if (i // 64) % 2 == 0],
        "fourth_word_of_each_256": [i for i in rows if 192 <= i % 256 <= 255],
    }.get(name)


@pytest.mark.parametrize("n", RC.SIZES)
@pytest.mark.parametrize("name", list(RC.PATTERNS))
def test_pattern_selects_the_rows_its_name_says(name, n):
    mask = RC.pattern_mask(name, n)
    assert mask.type == pa.bool_() and len(mask) == n
    kept = [i for i, m in enumerate(mask.to_pylist()) if m is True]
    assert kept == RC.pattern_rows(name, n).tolist()
    want = _expected_rows(name, n)
    if want is not None:
        assert kept == want and mask.null_count == 0
    if name == "last_word_only":
        assert 1 <= len(kept) <= 64 and kept[-1] == n - 1 and kept[0] % 64 == 0
    if name == "one_per_word":
        assert len({i // 64 for i in kept}) == len(kept) >= n // 64      # one row of every full word, never two


@pytest.mark.parametrize("name, frac", [("sparse", 0.001), ("dense", 0.999), ("half", 0.5)])
def test_random_patterns_have_their_density(name, frac):
    n = RC.WRAP_ROWS
    k = len(RC.pattern_rows(name, n))
    assert abs(k - frac * n) <= 5 * (n * frac * (1 - frac)) ** 0.5, (name, k)     # five standard deviations of the binomial
    assert 0 < k < n
    assert RC.pattern_rows(name, 4097).tolist() == RC.pattern_rows(name, 4097).tolist()   # seeded: the same rows every time


@pytest.mark.parametrize("n", [65, 257, 4097, RC.WRAP_ROWS])
def test_half_with_nulls_has_its_nulls_over_true_values(n):
    mask = RC.pattern_mask("half_with_nulls", n)
    valid = np.unpackbits(np.frombuffer(mask.buffers()[0], np.uint8), bitorder="little")[:n].astype(bool)
    value = np.unpackbits(np.frombuffer(mask.buffers()[1], np.uint8), bitorder="little")[:n].astype(bool)
    assert mask.null_count == int((~valid).sum()) > 0
    assert value[~valid].all(), "a NULL slot over a FALSE value would be dropped by a mover that ignores the validity too"
    if n >= 4097:
        assert 0.08 * n < mask.null_count < 0.12 * n
    kept = RC.pattern_rows("half_with_nulls", n)
    assert kept.tolist() == np.flatnonzero(value & valid).tolist() and len(kept) < int(value.sum())


# ------------------------------------------------------------------------------------------------------------------ the table
def test_every_type_table_has_a_nullable_and_a_null_free_column_of_every_type():
    t = RC.every_type_table(4097)
    assert tuple(t.column_names) == RC.EVERY_TYPE_COLUMNS and t.num_columns == 23
    for kind, typ in RC.TYPES.items():
        plain, nullable = t.column(kind).chunk(0), t.column(kind + "_n").chunk(0)
        assert plain.type == typ and nullable.type == RC.NULLABLE_TYPES[kind], kind
        assert plain.null_count == 0 and plain.buffers()[0] is None, kind        # imported without a validity buffer
        assert 0.1 * 4097 < nullable.null_count < 0.3 * 4097, kind
        assert nullable.slice(64, 64).null_count == 64 and nullable.slice(128, 64).null_count == 0, kind
    assert t.column("v").to_pylist() == list(range(4097))
    # more byte-addressable columns than one k_compact launch takes, and no more than two launches take
    byte_addressable = [f.name for f in t.schema if not (pa.types.is_boolean(f.type) or pa.types.is_string(f.type))]
    assert tuple(byte_addressable) == RC.BYTE_ADDRESSABLE and RC.MAX_COLS < len(byte_addressable) == 19 <= 2 * RC.MAX_COLS
    assert t.column("ds").type.index_type == pa.int32() and t.column("ds_n").type.index_type == pa.uint8()
    for n in RC.SIZES:
        RC.every_type_table(n).validate(full=True)
        assert RC.every_type_table(n).num_rows == n


def test_a_column_is_the_same_whichever_columns_are_built_beside_it():
    assert RC.table_of(RC.WRAP_COLUMNS, 4097).column("s_n").equals(RC.every_type_table(4097).column("s_n"))
    assert RC.table_of(("dec",), 257).column("dec").equals(RC.every_type_table(257).column("dec"))
    assert not RC.column("i64", 257).equals(RC.column("i64_n", 257).fill_null(0))


@pytest.mark.parametrize("n", [1, 257, 4097])
@pytest.mark.parametrize("name", ["dec", "dec_n"])
def test_no_decimal_has_a_high_half_that_is_the_sign_extension_of_its_low_half(name, n):
    col = RC.column(name, n)
    words = np.frombuffer(col.buffers()[1], np.uint64, 2 * n).reshape(n, 2)
    lo, hi = words[:, 0], words[:, 1].view(np.int64)
    ext = np.where(lo >> np.uint64(63) != 0, -1, 0)
    assert (hi != ext).all()
    assert len(set(hi.tolist())) > n // 2 or n == 1                         # and the high halves are drawn on their own
    py = col.to_pylist()
    for i in range(min(n, 50)):                                              # the bytes ARE the value pyarrow reads
        if py[i] is not None:
            assert int(py[i]) == (int(hi[i]) << 64) + int(lo[i]) and abs(int(py[i])) < 10**38


def test_the_float_column_holds_the_special_bit_patterns():
    for name in ("f64", "f64_n"):
        col = RC.column(name, 257)
        bits = np.frombuffer(col.buffers()[1], np.uint64, 257)
        for b in RC.F64_SPECIAL_BITS:
            assert int((bits == np.uint64(b)).sum()) >= 2, hex(b)
        assert bits[:len(RC.F64_SPECIAL_BITS)].tolist() == list(RC.F64_SPECIAL_BITS)
    vals = [struct.unpack("<d", struct.pack("<Q", b))[0] for b in RC.F64_SPECIAL_BITS]
    assert str(vals[0]) == "0.0" and str(vals[1]) == "-0.0" and vals[2] == float("inf") and vals[3] == float("-inf")
    assert all(v != v for v in vals[4:])
    got = RC.column("f64", 257).to_pylist()[:4]
    assert [struct.pack("<d", v) for v in got] == [struct.pack("<Q", b) for b in RC.F64_SPECIAL_BITS[:4]]


def test_the_other_columns_hold_their_edges():
    t = RC.every_type_table(257)
    assert min(t.column("u64").to_pylist()) < 2**63 <= t.column("u64")[0].as_py() and t.column("u64")[1].as_py() == 2**64 - 1
    assert sum(v >= 2**63 for v in t.column("u64").to_pylist()) > 64
    assert t.column("i64").to_pylist()[:2] == [-2**63, 2**63 - 1] and t.column("i32").to_pylist()[:2] == [-2**31, 2**31 - 1]
    s = t.column("s").to_pylist()
    assert set(s) == set(RC.STRINGS) and "" in s and "x" * 257 in s and any(len(x.encode()) == 8 for x in s)
    assert any(len(x.encode()) > len(x) for x in s)                          # multi-byte characters
    assert set(t.column("ds").cast(pa.string()).to_pylist()) == set(RC.DICT_WORDS)
    assert set(t.column("b").to_pylist()) == {True, False} and set(t.column("b_n").to_pylist()) == {True, False, None}


def test_the_18_plain_columns():
    t = RC.table_of(RC.PLAIN_18, 257)
    assert t.num_columns == 18 > RC.GM_MAX
    assert all(c.null_count == 0 and c.chunk(0).buffers()[0] is None for c in t.columns)
    assert {str(f.type) for f in t.schema} >= {"int64", "int32", "uint8", "decimal128(38, 0)", "uint64", "double", "uint32", "date32[day]"}
    assert not t.column("p0_i64").equals(t.column("p8_i64"))


def test_the_wrap_tables():
    """the reduced column sets of the two sizes at which a grid-stride loop goes round again (built from buffers: well under a second)"""
    a = RC.with_masks(RC.table_of(RC.WRAP_COLUMNS, RC.WRAP_ROWS), ("half_with_nulls", "sparse"))
    b = RC.with_masks(RC.table_of(RC.WRAP_COMPACT_COLUMNS, RC.WRAP_COMPACT_ROWS), ("half_with_nulls", "sparse"))
    assert a.num_rows == 524_288 + 65 > 2048 * 256 and b.num_rows == 2_097_152 + 65 > 2048 * 16 * 64
    assert [str(f.type) for f in a.schema][:4] == ["bool", "string", "int32", "int64"] and a.column("b_n").null_count > 0 < a.column("s_n").null_count
    assert [str(f.type) for f in b.schema][:3] == ["decimal128(38, 0)", "int64", "int64"] and b.column("i64_n").null_count > 0 == b.column("dec").null_count


# ------------------------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("n", SMALL)
def test_pyarrow_filter_is_the_plain_loop(n):
    t = RC.every_type_table(n)
    for name in RC.PATTERNS:
        mask = RC.pattern_mask(name, n)
        got = RC.ref_filter(t, mask)
        assert got.num_rows == len(RC.pattern_rows(name, n))
        want = RC.loop_filter(t, mask)
        for c in t.column_names:
            col = got.column(c)
            vals = col.cast(pa.string()).to_pylist() if pa.types.is_dictionary(col.type) else col.to_pylist()
            exp = t.column(c).cast(pa.string()).to_pylist() if pa.types.is_dictionary(col.type) else None
            exp = want[c] if exp is None else [exp[i] for i in RC.pattern_rows(name, n)]
            assert _same_python_values(vals, exp), (name, c)
        RC.assert_same_bits(got, RC.ref_take(t, RC.pattern_rows(name, n)), name)      # the two references agree with each other


@pytest.mark.parametrize("n", SMALL)
def test_pyarrow_take_is_the_plain_loop(n):
    t = RC.every_type_table(n).drop_columns(["ds", "ds_n"])
    rng = np.random.default_rng(n)
    ids = rng.integers(-1, n, size=3 * n + 5)          # -1: a NULL index
    ids[0] = -1
    got = RC.ref_take(t, ids)
    want = RC.loop_take(t, ids.tolist())
    for c in t.column_names:
        assert _same_python_values(got.column(c).to_pylist(), want[c]), c
        assert got.column(c).null_count == sum(v is None for v in want[c])
    assert got.column("v").null_count == int((ids < 0).sum()) > 0


def _same_python_values(a, b):
    """lists equal with floats held to their bits (NaN payloads, signed zeros)"""
    key = lambda v: struct.pack("<d", v) if isinstance(v, float) else v
    return [key(v) for v in a] == [key(v) for v in b]


def test_slice_and_concat_references():
    t = RC.every_type_table(5000)
    cuts = (0, 0, 1, 64, 127, 257, 257, 4097, 5000)
    parts = [t.slice(a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert [p.num_rows for p in parts] == [0, 1, 63, 63, 130, 0, 3840, 903]
    RC.assert_same_bits(pa.concat_tables(parts).combine_chunks(), t)


# ------------------------------------------------------------------------------------------------------------------ record layouts
@pytest.mark.parametrize("name", RC.LAYOUT_NAMES)
def test_record_layout_has_the_size_its_case_claims(name):
    _, kinds, groups = RC.layout(name)
    assert RC.record_groups(kinds) == list(groups)
    widths = sorted((RC.WIDTH[k] for k in kinds if RC.packable(k)), reverse=True)
    assert sum(g[1] for g in groups) <= sum(widths)
    for fields, size, rec in groups:
        assert 2 <= fields <= RC.PACK_MAX_COLS and size <= rec <= RC.RECORD_MAX_BYTES and rec in (16, 32, 48, 64) and rec - size < 16
    t = RC.layout_table(name, 300)
    for (cname, kind), field in zip(RC.layout_columns(name), t.schema):
        assert field.name == cname
        if RC.packable(kind):
            assert field.type.bit_width // 8 == RC.WIDTH[kind] and t.column(cname).null_count == 0
        else:
            assert t.column(cname).null_count > 0 or pa.types.is_boolean(field.type) or pa.types.is_string(field.type)


def test_the_layouts_cover_every_record_size_and_split():
    sizes = {g[2] for l in RC.LAYOUTS for g in l[2]}
    assert sizes == {16, 32, 48, 64}
    assert RC.layout("r64_exactly")[2] == ((4, 64, 64),)
    kinds = RC.layout("r64_and_a_lone_column")[1]
    assert sum(RC.WIDTH[k] for k in kinds) > 64 and sum(g[0] for g in RC.record_groups(kinds)) == len(kinds) - 1      # one goes alone
    assert [g[0] for g in RC.record_groups(RC.layout("ten_u8")[1])] == [RC.PACK_MAX_COLS, 2]
    mixed = RC.layout("mixed")[1]
    assert {"i64_n", "b", "s", "s_n"} <= set(mixed) and RC.record_groups(mixed)[0][0] == sum(RC.packable(k) for k in mixed)
    # with a 4-byte sort key taken beside them (ops.sort takes every column), the sizes and splits are all still there
    with_key = {name: RC.record_groups(kinds + ("i32",)) for name, kinds, _ in RC.LAYOUTS}
    assert with_key == {"r16": [(4, 17, 32)], "r32": [(4, 32, 32)], "r48": [(6, 48, 48)], "r64_exactly": [(4, 64, 64)],
                        "r64_and_a_lone_column": [(4, 64, 64), (2, 20, 32)], "ten_u8": [(8, 11, 16), (3, 3, 16)], "mixed": [(4, 17, 32)]}


# ------------------------------------------------------------------------------------------------------------------ the comparison
def test_the_exact_comparison_tells_bits_apart():
    f = lambda bits: RC.from_numpy(np.array(bits, dtype=np.uint64), pa.float64())
    base = pa.table({"x": f([RC.F64_SPECIAL_BITS[4], 0])})
    RC.assert_same_bits(base, pa.table({"x": f([RC.F64_SPECIAL_BITS[4], 0])}))                 # NaN equals the same NaN
    for other in ([RC.F64_SPECIAL_BITS[5], 0], [RC.F64_SPECIAL_BITS[4] + 1, 0], [RC.F64_SPECIAL_BITS[4], 1 << 63]):
        with pytest.raises(AssertionError, match="row"):
            RC.assert_same_bits(base, pa.table({"x": f(other)}))                                # another NaN, another zero
    d = RC.decimal_halves(4, np.random.default_rng(1))
    swapped = d[:, ::-1].copy()
    with pytest.raises(AssertionError, match="row 0"):
        RC.assert_same_bits(pa.table({"d": RC.from_numpy(d, RC.TYPES["dec"])}), pa.table({"d": RC.from_numpy(swapped, RC.TYPES["dec"])}))
    a = pa.table({"i": pa.array([1, None, 3])})
    RC.assert_same_bits(a, pa.table({"i": RC.from_numpy(np.array([1, 99, 3]), pa.int64(), np.array([False, True, False]))}))   # under a NULL: anything
    with pytest.raises(AssertionError, match="null_count"):
        RC.assert_same_bits(a, pa.table({"i": pa.array([1, 0, 3])}))
    with pytest.raises(AssertionError):
        RC.assert_same_bits(pa.table({"s": ["a", "b"]}), pa.table({"s": ["a", "c"]}))
    words = pa.array(["a", "b"])
    one = pa.table({"s": pa.DictionaryArray.from_arrays(pa.array([0, 1], pa.int32()), words)})
    other = pa.table({"s": pa.DictionaryArray.from_arrays(pa.array([1, 0], pa.uint8()), pa.array(["b", "a"]))})
    RC.assert_same_bits(one, other)                                                              # dictionary columns: as their strings
    with pytest.raises(AssertionError):
        RC.assert_same_bits(one, pa.table({"s": words}))                                         # but a dictionary column stays one

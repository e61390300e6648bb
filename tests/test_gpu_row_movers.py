"""The kernels that move rows - filter compaction (k_compact, k_compact_bits, k_pack_bytes, k_str_mask_ids / k_str_lengths / k_str_copy),
the takes (k_gather, k_gather_bits, k_gather_many, k_widen_ids, the record take k_pack_rows / k_gather_rows over records.hpp) and
slice / concat (k_bitmap_extract, k_bitmap_place, k_remap_indices, k_str_rebase) - against pyarrow's filter, take, slice and
concat_tables, bit for bit and in order, over a nullable and a NULL-free column of every type (tests/row_mover_cases.py; the
references and builders are checked in tests/test_row_mover_reference.py).  A test that claims a path asserts it by the names in
ops.profile_stats(); concat and slice launch under no profile name and are held by their results alone."""
import functools

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests import row_mover_cases as RC

pytestmark = pytest.mark.gpu

SORT_CARRIED = ("sort_local_emit", "sort_lsd_pass_out", "sort_carried_pass", "sort_onesweep_pass")
RECORD_TAKE = ("take_pack_rows", "take_gather_rows")


def _dev(t):
    from datafusion_amd.table import DeviceTable
    return DeviceTable.from_arrow(t)


def _profiled(fn):
    from datafusion_amd import ops
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        out = fn()
        return out, ops.profile_stats()
    finally:
        ops.profile_enable(False)


def _is_utf8(t):
    return pa.types.is_string(t)


def _is_bool(t):
    return pa.types.is_boolean(t)


# ================================================================================================================ filter compaction
@functools.lru_cache(maxsize=None)
def _filter_input(n):
    t = RC.with_masks(RC.every_type_table(n))
    return t, _dev(t)


REORDERED = ("s_n", "v", "dec_n", "b", "u8", "f64_n", "ds", "i32_n", "u64", "b_n", "d32", "s", "dec")   # 13 columns, 9 byte-addressable


def check_filter(t, dev, pred, mask, projection, what):
    """ops.filter against Table.filter with NULL slots dropped; the launches: ceil(byte-addressable columns / 12) of k_compact, and
    the bitmaps of every Boolean column and every nullable column packed from bytes"""
    from datafusion_amd import ops
    out, stats = _profiled(lambda: ops.filter(dev, pred, list(projection)))
    got = out.to_arrow()
    exp = RC.ref_filter(t.select(list(projection)), mask)
    RC.assert_same_bits(got, exp, what)
    wide = [c for c in projection if c in RC.BYTE_ADDRESSABLE]
    if exp.num_rows == 0:
        assert "compact" not in stats and "pack_bytes" not in stats and "take_string_bytes" not in stats, (what, sorted(stats))
    else:
        assert stats["compact"]["calls"] == -(-len(wide) // RC.MAX_COLS), (what, stats["compact"])
        strings = [c for c in projection if c.split("_")[0] == "s"]
        bools = [c for c in projection if c.split("_")[0] == "b"]
        nullable = [c for c in projection if t.column(c).null_count]     # (a column without a NULL has no validity buffer)
        calls = lambda name: stats.get(name, {"calls": 0})["calls"]
        assert calls("take_string_lengths") == calls("take_string_bytes") == len(strings), (what, sorted(stats))
        assert calls("pack_bytes") == len(bools) + len(nullable), (what, sorted(stats))
    assert not set(stats) & {"gather", *RECORD_TAKE}, (what, sorted(stats))
    return got


@pytest.mark.parametrize("n", RC.SIZES)
@pytest.mark.parametrize("pattern", list(RC.PATTERNS))
def test_filter_every_pattern_every_size_every_type(pattern, n):
    """a bare Boolean column is the predicate: its values are the mask, its validity mask_valid.  n: one lane, each side of one mask
    word and of one COMPACT_UNROLL group, a ragged tail behind more than one workgroup.  The 19 byte-addressable columns of the table
    take two k_compact launches; the reordered projection one"""
    from datafusion_amd.expr import col
    t, dev = _filter_input(n)
    mask = t.column("m_" + pattern)
    got = check_filter(t, dev, col("m_" + pattern), mask, RC.EVERY_TYPE_COLUMNS, f"{pattern} n={n}")
    assert got.column("v").to_pylist() == RC.pattern_rows(pattern, n).tolist()
    check_filter(t, dev, col("m_" + pattern), mask, REORDERED, f"{pattern} n={n} reordered")
    # NOT m: the complement (a NULL slot stays NULL and drops its row), through a mask that a kernel computed
    check_filter(t, dev, col("m_" + pattern).not_(), pc.invert(mask), REORDERED, f"not {pattern} n={n}")


@pytest.mark.parametrize("pattern", ["all", "last_only", "half_with_nulls", "last_word_only"])
def test_filter_of_a_table_imported_at_an_offset(pattern):
    """the Arrow arrays start at row 3 of longer buffers: at the source, the bits behind the last row of the mask (and of every
    bitmap) are other rows' bits, not zeros"""
    from datafusion_amd.expr import col
    whole = RC.with_masks(RC.every_type_table(300), ("all", "half_with_nulls"))
    t = whole.slice(3, 257)
    extra = {"last_only": RC.pattern_mask("last_only", 257), "last_word_only": RC.pattern_mask("last_word_only", 257)}
    for name, m in extra.items():   # (their own rows sliced out of a longer all-TRUE array: ones behind the end as well)
        sel = np.concatenate([np.ones(3, bool), np.asarray(m.to_numpy(zero_copy_only=False), dtype=bool), np.ones(40, bool)])
        t = t.append_column("m_" + name, RC.from_numpy(sel, pa.bool_()).slice(3, 257))
    assert t.column("m_all").chunk(0).offset == 3 and t.column("m_" + pattern).chunk(0).offset == 3
    dev = _dev(t)
    RC.assert_same_bits(dev.to_arrow(), t.combine_chunks(), "import at an offset")
    got = check_filter(t, dev, col("m_" + pattern), t.column("m_" + pattern), RC.EVERY_TYPE_COLUMNS, f"{pattern} at an offset")
    assert got.num_rows == {"all": 257, "last_only": 1, "last_word_only": 1}.get(pattern, got.num_rows)


@pytest.mark.parametrize("pattern", ["half_with_nulls", "sparse"])
@pytest.mark.parametrize("n, columns", [(RC.WRAP_ROWS, RC.WRAP_COLUMNS), (RC.WRAP_COMPACT_ROWS, RC.WRAP_COMPACT_COLUMNS)],
                         ids=["wrap_word_per_wave", "wrap_k_compact"])
def test_filter_beyond_one_trip_of_the_grid_stride_loop(pattern, n, columns):
    """a launch has at most 2048 workgroups.  524 288 + 65 rows: k_compact_bits, k_pack_bytes, k_str_mask_ids and the string take go
    round their loop a second time (Boolean, Utf8, Int32); 2 097 152 + 65 rows: k_compact does (Decimal128, nullable Int64)"""
    from datafusion_amd.expr import col
    t, dev = _wrap_input(n, columns)
    got = check_filter(t, dev, col("m_" + pattern), t.column("m_" + pattern), columns, f"{pattern} n={n}")
    assert np.array_equal(got.column("v").to_numpy(), RC.pattern_rows(pattern, n))


@functools.lru_cache(maxsize=None)
def _wrap_input(n, columns):
    t = RC.with_masks(RC.table_of(columns, n), ("half_with_nulls", "sparse"))
    return t, _dev(t)


# ================================================================================================================ take by 32-bit ids
def _with_key(t):
    return t.append_column("p", pa.array(RC.permutation(t.num_rows)))


@functools.lru_cache(maxsize=None)
def _sort_input(columns, n):
    """columns + a key `p`, a random permutation of 0..n-1 (Int32): the sorted table is t.take(argsort(p))"""
    names = {"one": (), "plain18": RC.PLAIN_18, "every": RC.EVERY_TYPE_COLUMNS, "wrap": RC.WRAP_COLUMNS}[columns]
    t = _with_key(RC.table_of(names, n)) if names else pa.table({"p": pa.array(RC.permutation(n))})
    order = np.argsort(t.column("p").to_numpy(), kind="stable")
    return t, _dev(t), order


def expected_gather_calls(t, n_out):
    """launches under the name `gather` of one gather_columns call (filter.hip): up to 65 536 rows, GM_MAX plain columns in ONE
    launch and the others one by one; above, every column on its own.  Utf8 columns run under the string take's names"""
    plain = [f.name for f in t.schema if t.column(f.name).null_count == 0 and not _is_bool(f.type) and not _is_utf8(f.type)]
    others = [f.name for f in t.schema if f.name not in plain and not _is_utf8(f.type)]
    if n_out <= RC.SMALL_TAKE_ROWS and t.num_columns >= 2:
        return (1 if plain else 0) + max(0, len(plain) - RC.GM_MAX) + len(others)
    return len(plain) + len(others)


SORT_TAKES = [(c, n) for c in ("one", "plain18", "every") for n in (2, 4096, RC.SMALL_TAKE_ROWS, RC.SMALL_TAKE_ROWS + 1)] + [("wrap", RC.WRAP_ROWS)]


@pytest.mark.parametrize("fetch", ["all", "half", "ten"])
@pytest.mark.parametrize("columns, n", SORT_TAKES)
def test_take_by_sorted_ids(columns, n, fetch):
    """SortExec by a permutation key: the row ids of a full sort are 32-bit and taken as they are (k_gather_many reads them, the
    per-column kernels take them widened by k_widen_ids); n = 2 and 4096 sort in LDS, 65 536 / 65 537 lie each side of the
    k_gather_many limit, 524 288 + 65 wraps the grid-stride loops of k_gather, k_gather_bits, k_widen_ids and the string take.
    fetch = n / 2 is no TopK: the first ids only; fetch = 10 above 4096 rows is a TopK: 64-bit ids.  One column alone never takes
    k_gather_many; of 19 plain ones (18 and the key) 16 go in one launch"""
    from datafusion_amd import ops
    t, dev, order = _sort_input(columns, n)
    k = {"all": None, "half": n // 2, "ten": 10}[fetch]
    out, stats = _profiled(lambda: ops.sort(dev, [("p", False, False)], k))
    n_out = n if k is None else min(k, n)
    RC.assert_same_bits(out.to_arrow(), RC.ref_take(t, order[:n_out]), f"sort {columns} n={n} fetch={k}")
    topk = k is not None and n > 4096 and n_out < n // 4
    assert any(name.startswith("topk_") for name in stats) == topk, sorted(stats)
    assert not set(stats) & {*SORT_CARRIED, *RECORD_TAKE}, sorted(stats)
    want = expected_gather_calls(t, n_out)
    if topk:   # (the radix select takes its survivors' key words by the same kernel: one launch per key word; the sampled limit none)
        assert want <= stats["gather"]["calls"] <= want + 2, (stats["gather"], want)
    else:
        assert stats["gather"]["calls"] == want, (stats["gather"], want)
    strings = sum(_is_utf8(f.type) for f in t.schema)
    assert stats.get("take_string_bytes", {"calls": 0})["calls"] == strings, sorted(stats)


# ================================================================================================================ record take
PACK_ROWS = 70_000    # above the small take's 65 536 rows


def _record_ledger(groups, n_in, n_out):
    """{name: [calls, bytes]} of the record take: one k_pack_rows over the input and one k_gather_rows over the output per record"""
    return {"take_pack_rows": [len(groups), sum(n_in * (size + rec) for _, size, rec in groups)],
            "take_gather_rows": [len(groups), sum(n_out * (8 + rec + size) for _, size, rec in groups)]}


def _ledger(stats, names=RECORD_TAKE):
    return {k: [stats[k]["calls"], stats[k]["bytes"]] for k in names if k in stats}


@pytest.mark.parametrize("layout", RC.LAYOUT_NAMES)
def test_record_take_by_32_bit_ids(layout):
    """take.pack_min_bytes = 0: the sort's take packs the plain columns (the layout's and the 4-byte key) into records and takes whole
    records by the sort's own 32-bit ids: k_gather_rows<R, uint32_t> at every R, past 64 bytes, past PACK_MAX_COLS fields, with a
    column left alone, and with nullable / Boolean / Utf8 columns that stay outside.  The record sizes are read off the ledger"""
    from datafusion_amd import ops
    t = _with_key(RC.layout_table(layout, PACK_ROWS))
    order = np.argsort(t.column("p").to_numpy(), kind="stable")
    dev = _dev(t)
    groups = RC.record_groups(RC.layout(layout)[1] + ("i32",))
    keys = [("p", False, False)]
    try:
        ops.set_options(take__pack_min_bytes="0")
        out, stats = _profiled(lambda: ops.sort(dev, keys))
        packed = out.to_arrow()
        assert _ledger(stats) == _record_ledger(groups, PACK_ROWS, PACK_ROWS), (stats, groups)
        assert not set(stats) & set(SORT_CARRIED), sorted(stats)
        RC.assert_same_bits(packed, RC.ref_take(t, order), f"{layout} packed")
        # a TopK's ten rows do not repay a pass over 70 000: declined (n * 4 < rows), still right
        out10, stats10 = _profiled(lambda: ops.sort(dev, keys, 10))
        assert not set(stats10) & set(RECORD_TAKE) and "gather" in stats10, sorted(stats10)
        RC.assert_same_bits(out10.to_arrow(), RC.ref_take(t, order[:10]), f"{layout} fetch=10")
    finally:
        ops.set_options(take__pack_min_bytes=None)
    out, stats = _profiled(lambda: ops.sort(dev, keys))
    assert not set(stats) & set(RECORD_TAKE) and "gather" in stats, sorted(stats)      # the default: column by column at this size
    plain = out.to_arrow()
    RC.assert_same_bits(plain, packed, f"{layout} column by column")


@pytest.mark.parametrize("layout", RC.LAYOUT_NAMES)
def test_record_take_by_64_bit_ids(layout):
    """the general M:N join path takes the build side by 64-bit ids: k_gather_rows<R, int64_t> over exactly the layout's columns.
    Every build key occurs twice (no unique-key path), every probe row matches both rows: 140 000 output rows of a 70 000-row build side"""
    from datafusion_amd import ops
    lt = RC.layout_table(layout, PACK_ROWS)
    names = lt.column_names
    build = lt.append_column("k", pa.array(np.arange(PACK_ROWS, dtype=np.int64) // 2))
    rng = np.random.default_rng(5)
    pk = rng.integers(0, PACK_ROWS // 2, size=PACK_ROWS)
    probe = pa.table({"pk": pa.array(pk), "q": pa.array(np.arange(PACK_ROWS, dtype=np.int64))})
    bdev, pdev = _dev(build), _dev(probe)
    groups = list(RC.layout(layout)[2])
    try:
        ops.set_options(take__pack_min_bytes="0")
        out, stats = _profiled(lambda: ops.hash_join(bdev, pdev, [("k", "pk")], "Inner", build_cols=names, probe_cols=["q"]))
    finally:
        ops.set_options(take__pack_min_bytes=None)
    got = out.to_arrow()
    assert "join_probe_emit" in stats and not set(stats) & {"join_probe_fused", "join_probe_placed", "join_probe_materialize"}, sorted(stats)
    assert _ledger(stats) == _record_ledger(groups, PACK_ROWS, 2 * PACK_ROWS), (stats, groups)
    ids = np.stack([2 * pk, 2 * pk + 1], axis=1).ravel()
    exp = RC.ref_take(lt, ids).append_column("q", pa.array(np.repeat(np.arange(PACK_ROWS, dtype=np.int64), 2)))
    assert got.num_rows == 2 * PACK_ROWS >= PACK_ROWS // 4
    # the two partners of a probe row come in no promised order: both sides ordered by q, then by the plain columns
    by = [("q", "ascending")] + [(c, "ascending") for c, kind in RC.layout_columns(layout) if RC.packable(kind)]
    RC.assert_same_bits(got.sort_by(by), exp.sort_by(by), f"{layout} join")


# ================================================================================================================ take with NULL ids
N_BUILD, N_PROBE = 5_000, 70_000


@functools.lru_cache(maxsize=None)
def _outer_join_input():
    """build: the every-type table, every key twice.  probe: a nullable key; a third of the keys are absent from the build side (and
    a fifth of the build keys from the probe side: Full has unmatched build rows)"""
    build = RC.every_type_table(N_BUILD).append_column("k", pa.array(np.arange(N_BUILD, dtype=np.int64) // 2))
    rng = np.random.default_rng(11)
    r = rng.integers(0, N_BUILD // 2 * 3 // 2, size=N_PROBE)
    pk = np.where(r % 5 == 0, r + 1_000_000, r)
    null = rng.random(N_PROBE) < 0.05
    probe = pa.table({"pk": pa.array(pk, mask=null), "q": pa.array(np.arange(N_PROBE, dtype=np.int64))})
    hit = ~null & (pk < N_BUILD // 2)
    # (build row, probe row) pairs in probe order; -1: no partner
    b = np.where(hit[:, None], np.stack([2 * pk, 2 * pk + 1], axis=1), -1)
    keep = np.stack([np.ones(N_PROBE, bool), hit], axis=1)          # a miss gives ONE row
    ids_b, ids_p = b[keep], np.repeat(np.arange(N_PROBE), 2).reshape(-1, 2)[keep]
    seen = np.zeros(N_BUILD, bool)
    seen[ids_b[ids_b >= 0]] = True
    return build, probe, ids_b, ids_p, np.flatnonzero(~seen)


@pytest.mark.parametrize("join_type", ["Right", "Full"])
def test_take_with_null_ids(join_type):
    """Right / Full joins on the general M:N path take the build side with NULL ids: every type - the Boolean, Utf8 and dictionary
    columns as well, the NULL-free ones too - comes out NULL for a probe row without a partner (k_gather, k_gather_bits, k_str_lengths
    with idx < 0), and the values under a NULL of the source stay NULL"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    build, probe, ids_b, ids_p, unmatched = _outer_join_input()
    assert (ids_b < 0).sum() > N_PROBE // 3 and len(unmatched) > N_BUILD // 10
    bdev, pdev = _dev(build), _dev(probe)
    bcols = list(RC.EVERY_TYPE_COLUMNS)

    def join():
        ht = ops.JoinHashTable(bdev, ["k"])
        parts = [ht.probe(pdev, ["pk"], join_type, bcols, ["q", "pk"])]
        if join_type == "Full":
            parts.append(ht.emit_unmatched("Full", bcols, ops.tail_probe_schema(pdev, "Full", ["q", "pk"])))
            assert parts[1].num_rows == len(unmatched)
        return parts[0] if len(parts) == 1 else DeviceTable.concat(parts)     # (never ops.concat_tables: it falls back to the host)
    out, stats = _profiled(join)
    got = out.to_arrow()
    assert "join_probe_emit" in stats and "join_probe_count" in stats and not set(stats) & set(RECORD_TAKE), sorted(stats)
    # one launch per fixed-width build column under `gather`, the strings under their own names
    assert stats["gather"]["calls"] >= sum(not _is_utf8(f.type) for f in build.select(bcols).schema), stats["gather"]
    assert stats["take_string_bytes"]["calls"] >= 2, sorted(stats)
    exp = RC.ref_take(build.select(bcols), ids_b)
    ptake = RC.ref_take(probe.select(["q", "pk"]), ids_p)
    if join_type == "Full":
        exp = pa.concat_tables([exp, build.select(bcols).take(pa.array(unmatched))])
        ptake = pa.concat_tables([ptake, RC.ref_take(probe.select(["q", "pk"]), np.full(len(unmatched), -1))])
    for c in ("q", "pk"):
        exp = exp.append_column(c, ptake.column(c))
    exp = exp.combine_chunks()
    misses = int((ids_b < 0).sum())
    for c in bcols:
        assert exp.column(c).null_count >= misses, c
    by = [("q", "ascending"), ("v", "ascending")]
    RC.assert_same_bits(got.sort_by(by), exp.sort_by(by), join_type)


# ================================================================================================================ slice and concat
CUTS = (0, 0, 1, 64, 127, 257, 257, 4097, 5000)      # part lengths 0, 1, 63, 63, 130, 0, 3840, 903


def test_slices_and_their_concat():
    """dev.slice of every part against Table.slice (k_bitmap_extract at bit offsets 0, 1, 64, 127, 257, 4097 for the Boolean values
    and every validity bitmap; k_str_rebase), then the concat of the slices against the table: Boolean values and validity bits are
    placed at bit offsets that are no multiples of 64 (k_bitmap_place with and without the carry from the next source word), parts
    of no rows among them"""
    from datafusion_amd.table import DeviceTable
    t = RC.every_type_table(5000)
    dev = _dev(t)
    parts = []
    for a, b in zip(CUTS, CUTS[1:]):
        parts.append(dev.slice(a, b - a))
        assert parts[-1].num_rows == b - a
        RC.assert_same_bits(parts[-1].to_arrow(), t.slice(a, b - a).combine_chunks(), f"slice [{a}, {b})")
    assert [p.num_rows for p in parts] == [0, 1, 63, 63, 130, 0, 3840, 903]
    RC.assert_same_bits(DeviceTable.concat(parts).to_arrow(), t, "concat of the slices")
    # the same parts imported one by one (validity buffers that start at bit 0 of their own words)
    again = [_dev(t.slice(a, b - a)) for a, b in zip(CUTS, CUTS[1:])]
    RC.assert_same_bits(DeviceTable.concat(again).to_arrow(), t, "concat of imported parts")
    # a slice of a slice, and a slice of the concat
    RC.assert_same_bits(parts[6].slice(61, 131).to_arrow(), t.slice(257 + 61, 131).combine_chunks(), "slice of a slice")


def test_concat_with_a_part_that_has_no_validity_buffers():
    """the middle part's nullable columns carry no NULL and arrive without validity buffers: its rows must come out all valid between
    parts whose bitmaps are placed around them (k_bitmap_place with src == nullptr), at bit offsets 100 and 100 + 77"""
    from datafusion_amd.table import DeviceTable
    t = RC.every_type_table(400)
    a, b, c = t.slice(0, 100).combine_chunks(), RC.drop_validity(t.slice(100, 77)), t.slice(177, 223).combine_chunks()
    assert all(col.null_count == 0 and col.chunk(0).buffers()[0] is None for col in b.columns) and a.column("i64_n").null_count > 0
    for parts in ([a, b, c], [b, a], [a, b]):
        got = DeviceTable.concat([_dev(p) for p in parts]).to_arrow()
        RC.assert_same_bits(got, pa.concat_tables(parts).combine_chunks(), "concat")
    n_ab = pa.concat_tables([a, b])
    assert n_ab.column("b_n").null_count == a.column("b_n").null_count > 0


def _dict_part(rng, n, words8, words32, null_frac):
    def one(words, index_type):
        idx = rng.integers(0, len(words), size=n).astype(index_type.to_pandas_dtype())
        null = rng.random(n) < null_frac
        return pa.DictionaryArray.from_arrays(RC.from_numpy(idx, index_type, null if null_frac else None), pa.array(words, pa.string()))
    return pa.table({"d8": one(words8, pa.uint8()), "d32": one(words32, pa.int32()), "v": pa.array(np.arange(n, dtype=np.int64))})


def test_concat_of_parts_with_different_dictionaries():
    """every part was encoded on its own: the dictionaries differ in content and order, so the indices of every part are rewritten
    into one merged dictionary (k_remap_indices at UInt8 and at Int32 width; the UInt8 one merges to 150 <= 256 values, the Int32
    one to more than 256)"""
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(21)
    pool8 = [f"w{i:03d}é" for i in range(150)]
    pool32 = [f"{i * 7919 % 1000:04d}-word" for i in range(1000)]
    parts = [_dict_part(rng, 1000, pool8[:100], pool32[:400], 0.1),
             _dict_part(rng, 0, pool8[:3], pool32[:3], 0.0),
             _dict_part(rng, 257, pool8[50:150][::-1], pool32[300:700][::-1], 0.0),
             _dict_part(rng, 70, pool8[::-3], pool32[600:], 0.3)]
    got = DeviceTable.concat([_dev(p) for p in parts]).to_arrow()
    plain = pa.schema([("d8", pa.string()), ("d32", pa.string()), ("v", pa.int64())])
    exp = pa.concat_tables([p.cast(plain) for p in parts]).combine_chunks()          # the strings themselves
    for name, index_type in (("d8", pa.uint8()), ("d32", pa.int32())):
        col = got.column(name).chunk(0)
        assert pa.types.is_dictionary(col.type) and col.type.index_type == index_type, col.type
        merged = col.dictionary.to_pylist()
        assert merged == sorted(set(merged), key=lambda s: s.encode()), name          # distinct and ascending (byte order)
        assert set(exp.column(name).drop_null().to_pylist()) <= set(merged)
        assert all(merged != p.column(name).chunk(0).dictionary.to_pylist() for p in parts if p.num_rows)
        assert got.column(name).null_count == exp.column(name).null_count > 0
        assert got.column(name).cast(pa.string()).combine_chunks().equals(exp.column(name).combine_chunks()), name
    assert len(got.column("d8").chunk(0).dictionary) <= 256 < len(got.column("d32").chunk(0).dictionary)
    assert got.column("v").equals(exp.column("v"))
    # parts that share one dictionary keep it: nothing is rewritten
    same = [parts[0].slice(0, 10).combine_chunks(), parts[0].slice(500, 77).combine_chunks()]
    got = DeviceTable.concat([_dev(p) for p in same]).to_arrow()
    RC.assert_same_bits(got, pa.concat_tables(same).combine_chunks(), "one dictionary")
    assert got.column("d8").chunk(0).dictionary.to_pylist() == pool8[:100]


def test_concat_of_one_part_and_of_empty_parts():
    from datafusion_amd.table import DeviceTable
    t = RC.every_type_table(257)
    dev = _dev(t)
    RC.assert_same_bits(DeviceTable.concat([dev]).to_arrow(), t, "one part")
    empty = [dev.slice(0, 0), _dev(t.slice(0, 0)), dev.slice(257, 0)]
    for parts in (empty, empty[:1]):
        got = DeviceTable.concat(parts).to_arrow()
        RC.assert_same_bits(got, t.slice(0, 0).combine_chunks(), "empty parts")
    RC.assert_same_bits(DeviceTable.concat([empty[0], dev, empty[2]]).to_arrow(), t, "empty parts around one")

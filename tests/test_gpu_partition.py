"""RepartitionExec(Hash) on the device (partition.hip) at every partition count, on each of its three counting kernels, through every
scatter launch of a wide table, on the second trip of the tile loop and on the mask-and-compact fallback, against the oracle's routing
(hash % nparts in input order; tests/test_edge_values_oracle.py holds that to Python integers at every count 1..64) - and the partitions
themselves, which are zero-copy views that start wherever the rows before them end, as the input of every other operator: the result
over a view must be the result over an aligned copy of it, and the oracle's.  Inputs: tests/partition_cases.py.

Moved values are compared by their bits (tests/edge_values.py assert_exact), strings as strings; a Float64 SUM is held to the exact sum
and the bound of tests/float_sum_ref.py, never to another run."""
import ctypes as C
import datetime
import functools
import itertools

import numpy as np
import pyarrow as pa
import pytest

from tests import edge_values as E
from tests import float_sum_ref as R
from tests import partition_cases as PC
from tests import window_ref as W

pytestmark = pytest.mark.gpu

REFUSAL = "dfgpu_partition supports 1..64 partitions"
ONEPASS = "join_build_rank_tab_onepass"


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


def _is_string(t):
    return pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_dictionary(t)


def assert_same(got: pa.Table, exp: pa.Table, ordered=True):
    """names, types and every value: strings (plain or dictionary-encoded, which stay what they were) as strings, the rest by its bits"""
    assert got.column_names == exp.column_names, (got.column_names, exp.column_names)
    strings = [f.name for f in exp.schema if _is_string(f.type)]
    for name in strings:
        assert pa.types.is_dictionary(got.schema.field(name).type) == pa.types.is_dictionary(exp.schema.field(name).type), name
        assert ordered and got.column(name).cast(pa.string()).to_pylist() == exp.column(name).cast(pa.string()).to_pylist(), name
    rest = [n for n in exp.column_names if n not in strings]
    E.assert_exact(got.select(rest), exp.select(rest), ordered=ordered)


def check_partition(table, keys, nparts, simple=None, dev=None):
    """ops.partition against the reference: nparts outputs, every row once, each partition the reference's rows in input order.
    simple = True: the zero-copy path ran (one count launch, one scatter launch per 12 columns, nothing compacted); False: the fallback"""
    from datafusion_amd import ops
    d = _dev(table) if dev is None else dev
    parts, stats = _profiled(lambda: ops.partition(d, keys, nparts))
    exp, part = PC.reference(table, keys, nparts)
    assert len(parts) == nparts == len(exp)
    got = [p.to_arrow() for p in parts]
    assert sum(g.num_rows for g in got) == table.num_rows
    for p, (g, e) in enumerate(zip(got, exp)):
        assert g.num_rows == e.num_rows, (p, g.num_rows, e.num_rows)
        assert_same(g, e)
    if table.num_rows == 0:
        assert "partition_count" not in stats and "partition_scatter" not in stats, sorted(stats)
    elif simple is not None:
        assert stats["partition_count"]["calls"] == 1, sorted(stats)
        if simple:
            assert stats["partition_scatter"]["calls"] == PC.ceil_div(table.num_columns, PC.SCATTER_COLS) and "compact" not in stats, stats
        else:
            assert "partition_scatter" not in stats and "compact" in stats, sorted(stats)
    return parts, got, part


# ------------------------------------------------------------------------------------------------------------ every count
@pytest.mark.parametrize("nparts", PC.ALL_COUNTS)
def test_every_partition_count(nparts):
    """1..64 partitions of four tiles and a three-row tail: 1..8 and 9..16 on the packed counters (typed: one NULL-free Int64 key),
    17..64 on the ballot counting, every divisor through the fast remainder (a mask for the powers of two)"""
    check_partition(PC.count_table(), ["k"], nparts, simple=True)


@pytest.mark.parametrize("nparts", [0, 65])
@pytest.mark.parametrize("rows", ["rows", "no_rows"])
def test_counts_outside_1_to_64_are_refused(nparts, rows):
    from datafusion_amd import _lib, ops
    lib = _lib.init()
    d = _dev(PC.count_table() if rows == "rows" else PC.skew_table("no_rows"))
    outs = (C.c_void_p * max(nparts, 1))()
    rc = lib.dfgpu_partition(d.handle, (C.c_int * 1)(0), 1, nparts, outs)
    assert rc != 0 and REFUSAL in lib.dfgpu_last_error().decode()
    assert all(h is None for h in outs)                      # no table is handed out
    with pytest.raises(_lib.DfgpuError, match=REFUSAL):
        ops.partition(d, ["k"], nparts)
    assert len(ops.partition(d, ["k"], 64)) == 64            # and the library goes on


# ------------------------------------------------------------------------------------------------ key kinds x counting kernels
@pytest.mark.parametrize("kind, nparts, n", PC.kind_cases())
def test_key_kinds_on_each_counting_kernel(kind, nparts, n):
    """the typed kernels take one NULL-free Int64 / UInt64 (values at and above 2^63) or Int32 / Date32 key up to 16 partitions; a
    UInt32 key has no typed kernel and takes KT_ANY, the row-by-row hash, as do a nullable Int64 (NULLs route by a hash of 0), two keys
    together, Float64 (by its bits: both zeros, both NaN signs), Decimal128(38, 0) (both words) and UInt8; above 16 partitions every
    kind takes the ballot-counting kernel.  Sizes: below, at and above one 1024-row tile, and 1, 3, 4, 5 rows - a thread stores the
    partition ids of four rows as one word, or byte by byte in a ragged tail"""
    table, keys = PC.key_table(kind, n)
    check_partition(table, keys, nparts, simple=table.column("k").null_count == 0)


# -------------------------------------------------------------------------------------------------- more columns than a launch
@pytest.mark.parametrize("nparts", [3, 17])
@pytest.mark.parametrize("ncols, key_last", PC.WIDE_CASES)
def test_tables_wider_than_one_scatter_launch(ncols, key_last, nparts):
    """12 columns go in one scatter launch, 13 and 24 in two, 25 in three, all by the one `part` / `prefix`; payloads of 1, 4, 8 and 16
    bytes side by side; the key as the last column lies in the last launch.  Every column of every partition is compared"""
    check_partition(PC.wide_table(ncols, key_last), ["k"], nparts, simple=True)


# ------------------------------------------------------------------------------------------------------- the second tile
@pytest.mark.parametrize("nparts", [3, 17])
def test_second_trip_of_the_tile_loop(nparts):
    """2048 x 1024 + 1025 rows are 2050 tiles for 2048 workgroups: workgroups 0 and 1 take a second tile (a full one and one row) and
    set their LDS counters up again.  Row numbers per partition are np.nonzero(part == p) of the oracle's routing, keys the rows' keys"""
    from datafusion_amd import ops
    from oracle import oracle
    key = PC.two_trip_columns()
    n = len(key)
    assert PC.ceil_div(n, PC.TILE) == PC.TILE_GRID + 2
    table = pa.table({"k": pa.array(key), "row": pa.array(np.arange(n, dtype=np.int64))})
    _, part = oracle.hash_partition(table.select(["k"]), ["k"], nparts)
    parts, stats = _profiled(lambda: ops.partition(_dev(table), ["k"], nparts))
    assert stats["partition_count"]["calls"] == 1 and stats["partition_scatter"]["calls"] == 1
    assert len(parts) == nparts and sum(p.num_rows for p in parts) == n
    for p, dp in enumerate(parts):
        got = dp.to_arrow()
        rows = np.nonzero(part == p)[0]
        assert got.column_names == ["k", "row"] and got.schema.types == [pa.int32(), pa.int64()]
        assert np.array_equal(got.column("row").to_numpy(), rows), p
        assert np.array_equal(got.column("k").to_numpy(), key[rows]), p


# ------------------------------------------------------------------------------------------------------ skew and empties
@pytest.mark.parametrize("nparts", [16, 17, 64])
@pytest.mark.parametrize("shape", PC.SKEWS)
def test_skewed_and_empty_inputs(shape, nparts):
    """one key value (everything in one partition), five key values (most partitions empty), a key of NULLs only (hash 0: partition
    0; the validity takes the table off the zero-copy path) and a table without rows: the empty partitions are zero-row tables of the
    full schema"""
    table = PC.skew_table(shape)
    parts, got, part = check_partition(table, ["k"], nparts, simple=shape != "all_null")
    sizes = [g.num_rows for g in got]
    if shape == "constant":
        assert sorted(sizes)[-1] == table.num_rows and sizes.count(0) == nparts - 1
    elif shape == "few_distinct":
        assert 1 < sum(1 for s in sizes if s) <= len(PC.FEW) < nparts
    elif shape == "all_null":
        assert sizes[0] == table.num_rows
    else:
        assert sizes == [0] * nparts


# --------------------------------------------------------------------------------------------------------- the fallback
@pytest.mark.parametrize("n", PC.FALLBACK_SIZES)
@pytest.mark.parametrize("nparts", [3, 17, 64])
@pytest.mark.parametrize("kind", PC.FALLBACK_KINDS)
def test_payloads_that_are_compacted_partition_by_partition(kind, nparts, n):
    """a nullable Int64, a Boolean with NULLs, a Utf8 with NULLs, a dictionary-encoded string with NULLs, and all four together: no
    scatter, one mask and one compaction per partition, up to 64 of them; values, NULLs and strings in input order"""
    check_partition(PC.fallback_table(kind, n), ["k"], nparts, simple=False)


@pytest.mark.parametrize("nparts", [17, 64])
@pytest.mark.parametrize("kind", ["utf8", "boolean"])
def test_string_and_boolean_keys_at_large_counts(kind, nparts):
    """a Utf8 key is routed on a UInt64 hash of its bytes carried as an extra column, a Boolean key as one byte per row; NULL keys go to
    partition 0; the extra column is dropped from the partitions"""
    from datafusion_amd import ops
    table = PC.odd_key_table(kind)
    parts, got, part = check_partition(table, ["k"], nparts)
    assert got[0].column("k").null_count == table.column("k").null_count > 0
    if kind == "utf8":
        enc = _dev(table).dictionary_encode(["k"])
        for g, e in zip(got, [p.to_arrow() for p in ops.partition(enc, ["k"], nparts)]):      # the same routing whatever the encoding
            assert pa.types.is_dictionary(e.schema.field("k").type)
            assert_same(pa.table({"k": e.column("k").cast(pa.string()), "row": e.column("row"), "v": e.column("v")}), g)


# ------------------------------------------------------------------------------------------------------------- the views
VIEWS = [(name, p) for name in ("odd", "mod4") for p in (1, 2)]
VIEW_IDS = [f"{name}_{p}" for name, p in VIEWS]


@functools.lru_cache(maxsize=None)
def _views(name):
    """(the source, its three partitions on the device - views of one buffer per column -, the reference's partitions as Arrow, aligned
    device copies of the views)"""
    from datafusion_amd import ops
    table = PC.view_source(name)
    parts = ops.partition(_dev(table), [PC.VIEW_KEY], 3)
    exp, _ = PC.reference(table, [PC.VIEW_KEY], 3)
    copies = [_dev(p.to_arrow()) for p in parts]
    return table, parts, exp, copies


def _offsets(dev):
    """{column: its data address modulo 16}"""
    views = [dev.column_view(i) for i in range(dev.num_columns)]
    return {v.name.decode(): int(v.data or 0) % 16 for v in views}


def _width(t):
    return t.bit_width // 8


@pytest.mark.parametrize("name", list(PC.VIEW_SIZES))
def test_partitions_are_views_off_the_16_byte_boundaries(name):
    """what the tests below rest on: partitions 1 and 2 start at rows the reference's sizes put off every 16-byte boundary, the device
    columns really start there, the aligned copies really are aligned, and the views hold the reference's rows"""
    table, parts, exp, copies = _views(name)
    sizes = [e.num_rows for e in exp]
    assert sizes == list(PC.VIEW_SIZES[name]) == [p.num_rows for p in parts]
    starts = [0, sizes[0], sizes[0] + sizes[1]]
    assert starts[1] % 16 != 0 and starts[2] % 16 != 0
    widths = {f.name: _width(f.type) for f in table.schema}
    for p in (1, 2):
        off = _offsets(parts[p])
        assert off == {c: starts[p] * w % 16 for c, w in widths.items()}, (p, off)     # one buffer per column, sliced at the row
        assert all(v == 0 for v in _offsets(copies[p]).values())
        E.assert_exact(parts[p].to_arrow(), exp[p], ordered=True)
        E.assert_exact(copies[p].to_arrow(), exp[p], ordered=True)
    narrow = [c for c, w in widths.items() if w in (1, 4, 8)]
    if name == "odd":
        assert all(_offsets(parts[p])[c] != 0 for p in (1, 2) for c in narrow)
    elif name == "mod4":
        assert _offsets(parts[1])["x32"] == 4 and _offsets(parts[2])["x32"] == 8 and _offsets(parts[1])["f"] == 1001 % 16
    else:
        assert all(_offsets(parts[1])[c] != 0 for c in narrow) and _offsets(parts[2])["a32"] == 8 and _offsets(parts[2])["f"] != 0


def _group_by():
    from datafusion_amd.expr import col
    return [(col(c), c) for c in ("f", "s", "d")]


def _aggs(wide=True):
    from datafusion_amd.expr import col
    out = [("count", None, "cnt"), ("sum", col("x32"), "s32"), ("min", col("x32"), "lo32"), ("max", col("x32"), "hi32"),
           ("min", col("xf"), "lof"), ("max", col("xf"), "hif"), ("count", col("xf"), "cf")]
    return out + ([("sum", col("xd"), "sd")] if wide else []) + [("sum", col("xf"), "sf")]


def _oracle_agg(t, group_by, aggs):
    from oracle import oracle
    from tests.util import to_oracle_expr
    return oracle.aggregate(t, [(to_oracle_expr(e), nm) for e, nm in group_by], [(f, None if e is None else to_oracle_expr(e), nm) for f, e, nm in aggs])


def _group_number(t):
    return (np.asarray(t.column("f")).astype(np.int64) << 40) | (np.asarray(t.column("s")).astype(np.int64) << 32) | np.asarray(t.column("d").cast(pa.int32())).astype(np.int64)


def _check_aggregate(got, arrow, exp, truth):
    """everything but the Float64 SUM equals the oracle's; the Float64 SUM lies within the derived bound of its group's exact sum"""
    E.assert_exact(got.drop(["sf"]), exp, ordered=False)
    for g, s in zip(_group_number(got).tolist(), got.column("sf").to_pylist()):
        assert R.within(s, truth[g].exact, truth[g].sum_bound()), (g, s, float(truth[g].exact), R.ratio(s, truth[g].exact, truth[g].sum_bound()))


@pytest.mark.parametrize("path", ["default", "partitioned"])
@pytest.mark.parametrize("name, p", VIEWS, ids=VIEW_IDS)
def test_aggregate_over_a_view(name, p, path):
    """GROUP BY (UInt8, UInt8, Date32) with COUNT / SUM / MIN / MAX over Int32, Float64 and Decimal128 payloads: the view and its aligned
    copy give the same table (groups in first-seen order), the oracle's; also with the partitioned paths forced"""
    from datafusion_amd import ops
    _, parts, exp, copies = _views(name)
    if path == "partitioned":
        ops.set_options(agg__partitioned_min_rows="1")
    gb, aggs = _group_by(), _aggs()
    want = _oracle_agg(exp[p], gb, aggs[:-1])
    truth = R.exact_group_sums(_group_number(exp[p]), np.asarray(exp[p].column("xf")))
    got_v = ops.aggregate(parts[p], gb, aggs, "Single").to_arrow()
    got_c = ops.aggregate(copies[p], gb, aggs, "Single").to_arrow()
    _check_aggregate(got_v, exp[p], want, truth)
    _check_aggregate(got_c, exp[p], want, truth)
    E.assert_exact(got_v.drop(["sf"]), got_c.drop(["sf"]), ordered=True)


def test_direct_table_claim_and_presence_scan_over_an_unaligned_view():
    """the aggregate's direct table is considered from (compute units x 16384) rows on, and no option lowers that: this view has that
    many rows and two 4096-row blocks and a three-row tail more, and starts at row 5 of its buffers (UInt8 keys 5 bytes, the Date32 key
    4 bytes off a 16-byte boundary), so k_intern_claim_direct takes its row-by-row loads and the UInt8 presence scan its bytewise head;
    the aligned copy takes the 16-byte loads.  Both must run, agree and equal the oracle; the keyed / generic table (agg.direct_table=0)
    and the partitioned paths over the same view as well"""
    import torch
    from datafusion_amd import ops
    rows = torch.cuda.get_device_properties(0).multi_processor_count * 16384 + 2 * 4096 + 3
    cols = ["f", "s", "d", "x32", "xf", PC.VIEW_KEY]
    table = PC.view_table((5, rows, 3), seed=9, wide=False).select(cols)
    parts = ops.partition(_dev(table), [PC.VIEW_KEY], 3)
    assert [q.num_rows for q in parts] == [5, rows, 3]
    view = parts[1]
    arrow = view.to_arrow()
    copy = _dev(arrow)
    assert _offsets(view) == {"f": 5, "s": 5, "d": 4, "x32": 4, "xf": 8, PC.VIEW_KEY: 8} and not any(_offsets(copy).values())
    owner = PC.reference(table.select([PC.VIEW_KEY]), [PC.VIEW_KEY], 3)[1]
    E.assert_exact(arrow, table.take(pa.array(np.nonzero(owner == 1)[0])), ordered=True)
    gb, aggs = _group_by(), _aggs(wide=False)[:-1]      # (a Float64 SUM over millions of rows belongs to tests/test_gpu_float_sums.py)
    want = _oracle_agg(arrow, gb, aggs)
    assert want.num_rows == 3 * 2 * 40
    got = {}
    for which, dev in (("view", view), ("copy", copy)):
        out, stats = _profiled(lambda: ops.aggregate(dev, gb, aggs, "Single").to_arrow())
        assert stats["agg_intern_claim_direct"]["calls"] == 1 and "column_u8_presence" in stats, (which, sorted(stats))
        E.assert_exact(out, want, ordered=False)
        got[which] = out
    E.assert_exact(got["view"], got["copy"], ordered=True)
    for opts in ({"agg__direct_table": "0"}, {"agg__partitioned_min_rows": "1"}):
        ops.set_options(**opts)
        out, stats = _profiled(lambda: ops.aggregate(view, gb, aggs, "Single").to_arrow())
        if "agg__direct_table" in opts:
            assert "agg_intern_claim_direct" not in stats, sorted(stats)
        E.assert_exact(out, want, ordered=False)
        ops.reset_options()


@pytest.mark.parametrize("probe_mode", [2, 1], ids=["single_pass", "two_pass"])
@pytest.mark.parametrize("key, probe_key", [("a64", "r64"), ("a32", "r32")])
@pytest.mark.parametrize("build_view", [1, 2])
def test_one_pass_rank_map_build_over_a_view(build_view, key, probe_key, probe_mode):
    """the rank map (table_mode 3) of a strictly ascending Int64 / Int32 key column that is a view of two 4096-row blocks and three
    rows: k_rank_tab_onepass loads four keys per lane, 16 bytes at a time where the column's address allows - view 1 starts 7 rows in
    (row by row), view 2 at row 8202 (Int64 aligned, Int32 8 bytes off).  Probed from the other view, Inner / RightSemi / RightAnti,
    single-pass and two-pass: the same rows in the same order as over aligned copies, and the oracle's rows"""
    from datafusion_amd import ops
    from oracle import oracle
    _, parts, exp, copies = _views("blocks")
    bcols, pcols = [key, "x32", "xd"], [probe_key, "row"]
    b_arrow, p_arrow = exp[build_view].select(bcols), exp[3 - build_view].select(pcols)
    got = {}
    for which, tabs in (("view", parts), ("copy", copies)):
        build, probe = tabs[build_view].select(bcols), tabs[3 - build_view].select(pcols)
        if which == "view":
            assert _offsets(build)[key] == (7 if build_view == 1 else 8202) * _width(b_arrow.schema.field(key).type) % 16
        ht, stats = _profiled(lambda: ops.JoinHashTable(build, [key], table_mode=3, probe_mode=probe_mode))
        assert ONEPASS in stats and "join_build_speculation_missed" not in stats, (which, sorted(stats))
        for jt in ("Inner", "RightSemi", "RightAnti"):
            got[which, jt] = ht.probe(probe, [probe_key], jt).to_arrow()
        ht.free()
    for jt in ("Inner", "RightSemi", "RightAnti"):
        want = oracle.hash_join(b_arrow, p_arrow, [(key, probe_key)], jt)
        assert 0 < want.num_rows < p_arrow.num_rows
        E.assert_exact(got["view", jt], want, ordered=False)
        E.assert_exact(got["view", jt], got["copy", jt], ordered=True)


@pytest.mark.parametrize("name, p", VIEWS, ids=VIEW_IDS)
def test_sort_and_topk_over_a_view(name, p):
    from datafusion_amd import ops
    from oracle import oracle
    _, parts, exp, copies = _views(name)
    keys = [("d", True, False), ("a64", False, False)]       # a64 is unique: one order only
    for fetch in (None, 10):
        want = oracle.sort(exp[p], keys, fetch)
        got_v, got_c = ops.sort(parts[p], keys, fetch).to_arrow(), ops.sort(copies[p], keys, fetch).to_arrow()
        E.assert_exact(got_v, want, ordered=True)
        E.assert_exact(got_c, got_v, ordered=True)


@pytest.mark.parametrize("name, p", VIEWS, ids=VIEW_IDS)
def test_filter_and_projection_over_a_view(name, p):
    """a comparison, a Kleene AND of two comparisons (Float64 and Date32), and Decimal128 arithmetic"""
    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    from oracle import oracle
    from tests.util import to_oracle_expr
    _, parts, exp, copies = _views(name)
    day = lit(datetime.date(1970, 1, 1) + datetime.timedelta(days=8020), pa.date32())
    for pred in (col("x32") > lit(0, pa.int32()), (col("xf") < lit(0.0, pa.float64())).and_(col("d") >= day)):
        want = oracle.filter(exp[p], to_oracle_expr(pred))
        assert 0 < want.num_rows < exp[p].num_rows
        got_v, got_c = ops.filter(parts[p], pred).to_arrow(), ops.filter(copies[p], pred).to_arrow()
        E.assert_exact(got_v, want, ordered=True)
        E.assert_exact(got_c, got_v, ordered=True)
        E.assert_exact(ops.filter(parts[p], pred, ["s", "xd", "row"]).to_arrow(), want.select(["s", "xd", "row"]), ordered=True)
    one = lit(1, pa.decimal128(20, 0))
    proj = [(col("xd") * (one - col("xd")), "e"), (col("xd") + col("xd"), "twice"), (col("x32") > lit(0, pa.int32()), "pos"), (col("f"), "f"), (col("row"), "row")]
    want = oracle.project(exp[p], [(to_oracle_expr(e), nm) for e, nm in proj])
    got_v, got_c = ops.project(parts[p], proj).to_arrow(), ops.project(copies[p], proj).to_arrow()
    E.assert_exact(got_v, want, ordered=True)
    E.assert_exact(got_c, got_v, ordered=True)


WINDOW_SPECS = [("row_number", None, "rn", None), ("sum", "x32", "running", "rows_to_current"), ("sum", "x32", "to_peers", None), ("max", "a32", "hi", "rows_to_current")]


def _window(dev, partition_by, order_by):
    from datafusion_amd import ops
    from datafusion_amd.expr import col
    return ops.window(dev, partition_by, order_by, [(f, None if a is None else col(a), nm, fr) for f, a, nm, fr in WINDOW_SPECS]).to_arrow()


def _check_window(got, rows: pa.Table, partition_by, order_by):
    cols = {c: rows.column(c).to_pylist() for c in ("f", "a64", "x32", "a32")}
    want = W.window(cols, {"f": "uint8", "a64": "int64", "x32": "int32", "a32": "int32"}, partition_by, order_by, WINDOW_SPECS)
    E.assert_exact(got.select(rows.column_names), rows, ordered=True)          # the input's columns first, unchanged
    assert got.column_names == rows.column_names + [s[2] for s in WINDOW_SPECS]
    assert got.schema.field("rn").type == pa.uint64() and got.schema.field("running").type == pa.int64() and got.schema.field("hi").type == pa.int32()
    for _, _, name, _ in WINDOW_SPECS:
        assert got.column(name).to_pylist() == want[name], name


@pytest.mark.parametrize("name, p", VIEWS, ids=VIEW_IDS)
def test_window_over_a_view(name, p):
    """row_number and running sums against tests/window_ref.py: over the view sorted by (UInt8, Int64) first, and directly over the view
    ordered by its ascending column (one partition, no peers)"""
    from datafusion_amd import ops
    from oracle import oracle
    _, parts, exp, copies = _views(name)
    keys = [("f", False, False), ("a64", False, False)]
    rows = oracle.sort(exp[p], keys)
    got_v, got_c = _window(ops.sort(parts[p], keys), ["f"], ["a64"]), _window(ops.sort(copies[p], keys), ["f"], ["a64"])
    _check_window(got_v, rows, ["f"], ["a64"])
    E.assert_exact(got_c, got_v, ordered=True)
    got_v, got_c = _window(parts[p], [], ["a64"]), _window(copies[p], [], ["a64"])
    _check_window(got_v, exp[p], [], ["a64"])
    E.assert_exact(got_c, got_v, ordered=True)


@pytest.mark.parametrize("nparts", [3, 17])
@pytest.mark.parametrize("name, p", VIEWS, ids=VIEW_IDS)
def test_partition_of_a_view(name, p, nparts):
    """a partition as the input of the next repartition: by its ascending Int64 (the typed kernel at 3) and by (UInt8, Date32)"""
    _, parts, exp, copies = _views(name)
    for keys in (["a64"], ["f", "d"]):
        _, got_v, _ = check_partition(exp[p], keys, nparts, simple=True, dev=parts[p])
        _, got_c, _ = check_partition(exp[p], keys, nparts, simple=True, dev=copies[p])
        for a, b in zip(got_v, got_c):
            E.assert_exact(a, b, ordered=True)


@pytest.mark.parametrize("name, p", VIEWS, ids=VIEW_IDS)
def test_slices_concatenation_and_batches_of_a_view(name, p):
    """slice (a view of a view), concat of two views and export_batch at 1, 63 and 64 rows a batch, against pyarrow's slices"""
    from datafusion_amd.table import DeviceTable
    _, parts, exp, copies = _views(name)
    n = exp[p].num_rows
    for off, length in ((0, 0), (0, n), (1, 5), (3, n - 3), (n - 1, 1), (64, 63), (n, 0)):
        E.assert_exact(parts[p].slice(off, length).to_arrow(), exp[p].slice(off, length), ordered=True)
    E.assert_exact(parts[p].slice(5, 200).slice(3, 100).to_arrow(), exp[p].slice(8, 100), ordered=True)
    both = DeviceTable.concat([parts[p], parts[3 - p]])
    E.assert_exact(both.to_arrow(), pa.concat_tables([exp[p], exp[3 - p]]), ordered=True)
    E.assert_exact(DeviceTable.concat([parts[p].slice(1, 70), copies[p].slice(0, 1)]).to_arrow(), pa.concat_tables([exp[p].slice(1, 70), exp[p].slice(0, 1)]), ordered=True)
    for rows, batches in ((1, 130), (63, None), (64, None)):
        seen = 0
        for i, batch in enumerate(itertools.islice(parts[p].to_batches(rows), batches)):
            E.assert_exact(pa.Table.from_batches([batch]), exp[p].slice(i * rows, rows), ordered=True)
            seen += batch.num_rows
        assert seen == (n if batches is None else batches * rows)

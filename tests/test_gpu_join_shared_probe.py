"""The foreign-key probe that shares its probe columns (k_join_probe_shared): when every probe row finds exactly one build row and the
output is in probe order, the output's probe-side columns ARE the probe table's columns (same device buffers, second owners) and the
kernel writes the build-side columns only.  Checked against the CPU oracle; `join.share_probe_min_rows` forces the path at small
sizes, the profile record `join_probe_shared_columns` tells which path ran, `column_view().data` tells who owns what."""
from decimal import Decimal

import numpy as np
import pyarrow as pa
import pytest

from tests.util import assert_tables_equal

pytestmark = pytest.mark.gpu

KIND_CODE = {"array": 1, "rank": 2, "flat": 4, "flat16": 5}       # dfgpu_join_info.table_kind
TABLE_MODE = {"array": 2, "rank": 3, "flat": 5, "flat16": 5}      # dfgpu_join_options.table_mode that forces the kind
GROUP_ROWS = 256                                                  # rows whose 4-byte values the shared kernel stores together
BLOCK_ROWS = 2048                                                 # probe rows per workgroup of the shared kernel
TILE_ROWS = 2048                                                  # probe rows per tile of the fused kernels
KEY_TYPES = {"Int64": pa.int64(), "Int32": pa.int32(), "UInt8": pa.uint8()}
PAYLOAD = {1: ("b_u8", pa.uint8()), 4: ("b_i32", pa.int32()), 8: ("b_i64", pa.int64()), 16: ("b_dec", pa.decimal128(15, 2))}


def _build_table(kind, key_type, nb, rng):
    """unique build keys that the forced table kind accepts, and one payload column of every width"""
    if key_type == "UInt8":
        nb = min(nb, 80)
    keys = np.arange(nb, dtype=np.int64) * 3 + 2
    cols = {"bk": pa.array(keys, type=KEY_TYPES[key_type])}
    if kind == "flat16":    # two key columns: 16 packed bytes
        cols["bk2"] = pa.array(keys * 5 - 1, type=pa.int64())
    cols["b_u8"] = pa.array(rng.integers(0, 256, nb).astype(np.uint8))
    cols["b_i32"] = pa.array(rng.integers(-2**31, 2**31, nb).astype(np.int32))
    cols["b_i64"] = pa.array(rng.integers(-2**62, 2**62, nb).astype(np.int64))
    cols["b_dec"] = pa.array([Decimal(int(v)).scaleb(-2) for v in rng.integers(-10**12, 10**12, nb)], type=pa.decimal128(15, 2))
    return pa.table(cols)


def _probe_table(build, kind, npr, rng):
    """a foreign-key probe: every probe key is some build key (not clustered: any build row, any number of times)"""
    fk = rng.integers(0, build.num_rows, npr)
    cols = {"pk": build.column("bk").take(pa.array(fk))}
    if kind == "flat16":
        cols["pk2"] = build.column("bk2").take(pa.array(fk))
    cols["p_i64"] = pa.array(rng.integers(-2**62, 2**62, npr).astype(np.int64))
    cols["p_i32"] = pa.array(np.arange(npr, dtype=np.int32))
    return pa.table(cols)


def _on(kind):
    return [("bk", "pk"), ("bk2", "pk2")] if kind == "flat16" else [("bk", "pk")]


def _oracle(build, probe, on, join_type, build_cols, probe_cols):
    from oracle import oracle
    exp = oracle.hash_join(build, probe, on, join_type)
    if join_type in ("RightSemi", "RightAnti"):
        return exp.select(probe_cols)
    return exp.select(list(build_cols) + list(probe_cols))


def _pointers(table):
    return [table.column_view(i).data for i in range(table.num_columns)]


class _Forced:
    """the shared path at any size, the profile on; options and profile back to their defaults afterwards"""

    def __init__(self, **opts):
        self.opts = {"join__share_probe_min_rows": 1, **opts}

    def __enter__(self):
        from datafusion_amd import ops
        ops.set_options(**self.opts)
        ops.profile_enable(True)
        ops.profile_reset()
        return self

    def __exit__(self, *exc):
        from datafusion_amd import ops
        ops.profile_enable(False)
        ops.set_options(**{k: None for k in self.opts})


def _probe(build, probe, kind, probe_mode, join_type, build_cols, probe_cols, predicate=None, **force):
    """(device output, profile names, device probe table, device build table, join table): the caller frees them"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    db, dp = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    with _Forced(**force):
        ht = ops.JoinHashTable(db, [l for l, _ in _on(kind)], table_mode=TABLE_MODE[kind], probe_mode=probe_mode)
        out = ht.probe(dp, [r for _, r in _on(kind)], join_type, build_cols, probe_cols, predicate=predicate)
        stats = ops.profile_stats()
    return out, stats, dp, db, ht


def _check_shared(out, stats, dp, probe_cols, n_build_cols):
    assert "join_probe_shared_columns" in stats, sorted(stats)
    assert "join_probe_speculation_missed" not in stats and "join_probe_tile_counts" not in stats, sorted(stats)
    inputs = _pointers(dp)
    got = _pointers(out)
    for i, name in enumerate(probe_cols):   # the probe side of the output IS the input
        assert got[n_build_cols + i] == inputs[dp.index_of(name)], (name, got, inputs)
    for i in range(n_build_cols):           # the build side is new
        assert got[i] not in inputs, (i, got, inputs)


def _check_not_shared(out, stats, dp):
    assert "join_probe_shared_columns" not in stats, sorted(stats)
    inputs = _pointers(dp)
    assert not [p for p in _pointers(out) if p in inputs], "an output column shares a buffer with the probe table"


CASES = [(kind, kt) for kind in ("rank", "array") for kt in ("Int64", "Int32", "UInt8")] + [("flat", "Int64"), ("flat", "Int32"), ("flat16", "Int64")]


@pytest.mark.parametrize("width", [1, 4, 8, 16])
@pytest.mark.parametrize("probe_mode", [0, 3, 4])
@pytest.mark.parametrize("kind,key_type", CASES, ids=[f"{k}-{t}" for k, t in CASES])
def test_all_hit_probe_shares_probe_columns(kind, key_type, probe_mode, width):
    """every table kind the path serves x the probe modes it serves x key types x one build payload column of each width: the oracle's
    rows in probe order, probe-side columns are the input's buffers, the build-side column is new"""
    rng = np.random.default_rng(7 * width + probe_mode)
    build = _build_table(kind, key_type, 3_000, rng)
    probe = _probe_table(build, kind, 5_000, rng)
    bcols, pcols = [PAYLOAD[width][0]], ["pk", "p_i64", "p_i32"]
    out, stats, dp, db, ht = _probe(build, probe, kind, probe_mode, "Inner", bcols, pcols)
    try:
        assert ht.info().table_kind == KIND_CODE[kind]
        assert ("join_probe_placed" if probe_mode == 0 else "join_probe_fused") in stats, sorted(stats)
        _check_shared(out, stats, dp, pcols, 1)
        assert_tables_equal(out.to_arrow(), _oracle(build, probe, _on(kind), "Inner", bcols, pcols), ordered=True)
    finally:
        for t in (out, ht, dp, db):
            t.free()


@pytest.mark.parametrize("npr", [1, 2, 3, 5, 63, 64, 65, GROUP_ROWS - 1, GROUP_ROWS, GROUP_ROWS + 1, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, TILE_ROWS - 1, TILE_ROWS,
                                 TILE_ROWS + 1, 5 * TILE_ROWS + 777, 5 * TILE_ROWS + GROUP_ROWS - 2])
@pytest.mark.parametrize("kind", ["rank", "flat"])
def test_row_counts_off_the_word_and_tile_grid(kind, npr):
    """all four payload widths at once, at row counts around the 64-row word, the 256-row group of the 16-byte stores, the kernel's
    workgroup and the fused kernels' tile"""
    rng = np.random.default_rng(npr)
    build = _build_table(kind, "Int64", 700, rng)
    probe = _probe_table(build, kind, npr, rng)
    bcols, pcols = ["b_u8", "b_i32", "b_i64", "b_dec"], ["p_i32", "pk"]
    out, stats, dp, db, ht = _probe(build, probe, kind, 0, "Inner", bcols, pcols)
    try:
        _check_shared(out, stats, dp, pcols, 4)
        assert out.num_rows == npr
        assert_tables_equal(out.to_arrow(), _oracle(build, probe, _on(kind), "Inner", bcols, pcols), ordered=True)
    finally:
        for t in (out, ht, dp, db):
            t.free()


def test_probe_table_that_is_a_view_into_a_larger_buffer():
    """the output partitions of dfgpu_partition are views (non-zero data_offset) of one buffer per column: the shared output columns
    point at base + offset and read back right"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(3)
    build = _build_table("rank", "Int64", 2_000, rng)
    probe = _probe_table(build, "rank", 40_000, rng)
    db, whole = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    parts = ops.partition(whole, ["pk"], 4)
    bases = [p.column_view(0).data for p in parts]
    assert len(set(bases)) == 4     # four windows of one buffer: at least three start at a non-zero offset
    bcols, pcols = ["b_i32", "b_dec"], ["pk", "p_i64"]
    try:
        for part in parts:
            with _Forced():
                ht = ops.JoinHashTable(db, ["bk"], table_mode=3, probe_mode=3)
                out = ht.probe(part, ["pk"], "Inner", bcols, pcols)
                stats = ops.profile_stats()
            _check_shared(out, stats, part, pcols, 2)
            assert_tables_equal(out.to_arrow(), _oracle(build, part.to_arrow(), _on("rank"), "Inner", bcols, pcols), ordered=True)
            out.free()
            ht.free()
    finally:
        for t in parts + [whole, db]:
            t.free()


def _foreign_key_5m(flaw):
    """the 5 M-row foreign-key probe of test_probe_order_speculation_every_row_finds_its_key with one kind of miss in it"""
    rng = np.random.default_rng(31)
    nb, npr = 500_000, 5_000_000
    okeys = (np.arange(nb, dtype=np.int64) // 8) * 32 + np.arange(nb) % 8 + 1
    fk = np.sort(rng.integers(0, nb, npr))
    pk = okeys[fk].copy()
    pay = rng.integers(0, 10**6, npr).astype(np.int64)
    null_at = None
    if flaw == "between_samples":
        pk[[70_001, 2_345_679, 4_999_998]] = -5       # none of them on a sampled word
    elif flaw == "first_row":
        pk[0] = -5
    elif flaw == "last_row":
        pk[npr - 1] = -5
    elif flaw == "null_key":
        null_at = 2_345_679
    mask = None
    if null_at is not None:
        mask = np.zeros(npr, bool)
        mask[null_at] = True
    build = pa.table({"o_orderkey": pa.array(okeys), "o_flag": pa.array((np.arange(nb) % 7).astype(np.int32))})
    probe = pa.table({"l_orderkey": pa.array(pk, mask=mask), "l_pay": pa.array(pay)})
    keep = pk > 0 if mask is None else ~mask
    return build, probe, fk, pk, pay, keep


@pytest.mark.parametrize("probe_mode", [0, 3])
@pytest.mark.parametrize("flaw", ["between_samples", "first_row", "last_row", "null_key"])
def test_a_probe_row_without_partner_falls_back_to_the_counted_probe(flaw, probe_mode):
    """a dangling key the sample does not see (between the sampled words, in the last row, a NULL key) makes the kernel raise its flag:
    `join_probe_speculation_missed`, then the counted / unordered probe; the first row lies on a sampled word, so there the sample
    itself sends the probe down the counted path and no speculation is recorded.  Either way: the oracle's rows, nothing shared."""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    build, probe, fk, pk, pay, keep = _foreign_key_5m(flaw)
    pcols = ["l_pay"] if flaw == "null_key" else ["l_orderkey", "l_pay"]     # (a nullable payload column would leave the fused paths)
    db, dp = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        ht = ops.JoinHashTable(db, ["o_orderkey"], probe_mode=probe_mode)
        out = ht.probe(dp, ["l_orderkey"], "Inner", ["o_flag"], pcols)
        stats = ops.profile_stats()
    finally:
        ops.profile_enable(False)
    try:
        assert ("join_probe_speculation_missed" in stats) == (flaw != "first_row"), sorted(stats)
        _check_not_shared(out, stats, dp)
        got = out.to_arrow()
        assert got.num_rows == int(keep.sum())
        exp = {"o_flag": (fk[keep] % 7).astype(np.int32), "l_orderkey": pk[keep], "l_pay": pay[keep]}
        names = ["o_flag"] + pcols
        if probe_mode == 0:     # probe order
            for n in names:
                assert np.array_equal(got.column(n).to_numpy(), exp[n]), n
        else:                   # any order: the same multiset of rows
            a = np.stack([got.column(n).to_numpy().astype(np.int64) for n in names])
            e = np.stack([exp[n].astype(np.int64) for n in names])
            assert np.array_equal(a[:, np.lexsort(a)], e[:, np.lexsort(e)])
    finally:
        for t in (out, ht, dp, db):
            t.free()


def test_missed_speculation_against_the_oracle_at_small_size():
    """small enough for the oracle: every word of a probe this small is sampled, so the sample itself finds the dangling keys and the
    counted path runs: the oracle's rows, nothing shared"""
    rng = np.random.default_rng(5)
    build = _build_table("rank", "Int64", 900, rng)
    probe = _probe_table(build, "rank", 7_000, rng)
    pk = probe.column("pk").to_numpy().copy()
    pk[[0, 3_333, 6_999]] = 1          # 1 is not a build key (build keys are 3 i + 2)
    probe = probe.set_column(0, "pk", pa.array(pk))
    bcols, pcols = ["b_i64"], ["pk", "p_i32"]
    out, stats, dp, db, ht = _probe(build, probe, "rank", 0, "Inner", bcols, pcols)
    try:
        _check_not_shared(out, stats, dp)
        assert_tables_equal(out.to_arrow(), _oracle(build, probe, _on("rank"), "Inner", bcols, pcols), ordered=True)
    finally:
        for t in (out, ht, dp, db):
            t.free()


@pytest.mark.parametrize("case", ["duplicate_build_keys", "fused_predicate", "nullable_payload", "right_anti", "lookback_mode"])
def test_shapes_that_must_not_take_the_shared_path(case):
    from datafusion_amd.expr import col, lit
    rng = np.random.default_rng(11)
    build = _build_table("flat", "Int64", 1_500, rng)
    probe = _probe_table(build, "flat", 9_000, rng)
    join_type, bcols, pcols, predicate, mode, kind = "Inner", ["b_i32", "b_i64"], ["pk", "p_i64"], None, 0, "flat"
    exp_probe = probe
    if case == "duplicate_build_keys":
        build = pa.concat_tables([build, build.slice(0, 10)])
    elif case == "fused_predicate":
        predicate = col("p_i32") >= lit(0, pa.int32())       # true of every row: still a mask
    elif case == "nullable_payload":
        m = np.zeros(probe.num_rows, bool)
        m[17] = True
        probe = exp_probe = probe.set_column(probe.schema.get_field_index("p_i64"), "p_i64", pa.array(probe.column("p_i64").to_numpy(), mask=m))
    elif case == "right_anti":
        join_type, bcols = "RightAnti", []
        pk = probe.column("pk").to_numpy().copy()
        pk[::50] = 1
        probe = exp_probe = probe.set_column(0, "pk", pa.array(pk))
    elif case == "lookback_mode":
        mode, kind = 2, "rank"
    out, stats, dp, db, ht = _probe(build, probe, kind, mode, join_type, bcols, pcols, predicate=predicate)
    try:
        _check_not_shared(out, stats, dp)
        exp = _oracle(build, exp_probe, _on(kind), join_type, bcols, pcols)
        assert_tables_equal(out.to_arrow(), exp, ordered=case != "duplicate_build_keys")
    finally:
        for t in (out, ht, dp, db):
            t.free()


@pytest.mark.parametrize("kind", ["rank", "array", "flat", "flat16"])
def test_right_semi_all_hit_hands_back_the_probe_columns(kind):
    """no build column to write: the kernel reads the keys, verifies, and every output column is the probe's"""
    rng = np.random.default_rng(13)
    build = _build_table(kind, "Int64", 1_200, rng)
    probe = _probe_table(build, kind, 6_001, rng)
    pcols = ["p_i64", "pk", "p_i32"]
    out, stats, dp, db, ht = _probe(build, probe, kind, 4, "RightSemi", [], pcols)
    try:
        _check_shared(out, stats, dp, pcols, 0)
        assert out.num_columns == 3
        assert_tables_equal(out.to_arrow(), _oracle(build, probe, _on(kind), "RightSemi", [], pcols), ordered=True)
    finally:
        for t in (out, ht, dp, db):
            t.free()


def test_output_outlives_its_inputs_and_the_probe_table_outlives_the_output():
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(17)
    build = _build_table("rank", "Int64", 2_500, rng)
    probe = _probe_table(build, "rank", 30_000, rng)
    bcols, pcols = ["b_dec", "b_u8"], ["pk", "p_i64", "p_i32"]
    exp = _oracle(build, probe, _on("rank"), "Inner", bcols, pcols)
    # inputs freed first, buffers churned, then the output is read
    out, stats, dp, db, ht = _probe(build, probe, "rank", 3, "Inner", bcols, pcols)
    _check_shared(out, stats, dp, pcols, 2)
    for t in (dp, ht, db):
        t.free()
    churn = [DeviceTable.from_arrow(_probe_table(build, "rank", 30_000, rng)) for _ in range(4)]   # whatever the pool got back is written over
    assert_tables_equal(out.to_arrow(), exp, ordered=True)
    out.free()
    for t in churn:
        t.free()
    # output freed first, then the probe table is read
    out, stats, dp, db, ht = _probe(build, probe, "rank", 3, "Inner", bcols, pcols)
    _check_shared(out, stats, dp, pcols, 2)
    out.free()
    churn = [DeviceTable.from_arrow(_probe_table(build, "rank", 30_000, rng)) for _ in range(4)]
    assert_tables_equal(dp.to_arrow(), probe, ordered=True)
    for t in churn + [dp, ht, db]:
        t.free()


@pytest.mark.parametrize("probe_mode", [0, 3])
def test_switched_off_gives_the_copying_path_and_the_same_rows(probe_mode):
    rng = np.random.default_rng(19)
    build = _build_table("rank", "Int64", 2_000, rng)
    probe = _probe_table(build, "rank", 20_000, rng)
    bcols, pcols = ["b_i32", "b_i64"], ["pk", "p_i64"]
    out, stats, dp, db, ht = _probe(build, probe, "rank", probe_mode, "Inner", bcols, pcols, join__share_probe=0)
    try:
        _check_not_shared(out, stats, dp)
        assert ("join_probe_placed" if probe_mode == 0 else "join_probe_fused") in stats, sorted(stats)
        assert_tables_equal(out.to_arrow(), _oracle(build, probe, _on("rank"), "Inner", bcols, pcols), ordered=probe_mode == 0)
    finally:
        for t in (out, ht, dp, db):
            t.free()


@pytest.mark.parametrize("dangling", [False, True])
def test_the_samples_answer_is_remembered_per_pair_of_key_buffers(dangling):
    """the all-hit sample (a kernel and a blocking read-back) is asked once per (build key buffer, probe key buffer): a second probe of the
    same tables takes the shared path again without it; after a miss the kernel found (row 69: word 1, the sample of a 200 K-row probe
    looks at every third word) the answer is corrected and the second probe does not speculate again.  Same rows every time."""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    rng = np.random.default_rng(23)
    build = _build_table("rank", "Int64", 4_000, rng)
    probe = _probe_table(build, "rank", 200_000, rng)
    if dangling:
        pk = probe.column("pk").to_numpy().copy()
        pk[69] = 1          # not a build key
        probe = probe.set_column(0, "pk", pa.array(pk))
    bcols, pcols = ["b_i32", "b_u8"], ["pk", "p_i32"]
    exp = _oracle(build, probe, _on("rank"), "Inner", bcols, pcols)
    db, dp = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    try:
        for attempt in range(2):
            with _Forced():
                ht = ops.JoinHashTable(db, ["bk"], table_mode=3, probe_mode=0)     # a new join table over the same build table each time
                out = ht.probe(dp, ["pk"], "Inner", bcols, pcols)
                stats = ops.profile_stats()
            if dangling:
                _check_not_shared(out, stats, dp)
                assert ("join_probe_speculation_missed" in stats) == (attempt == 0), (attempt, sorted(stats))
            else:
                _check_shared(out, stats, dp, pcols, 2)
            assert_tables_equal(out.to_arrow(), exp, ordered=True)
            out.free()
            ht.free()
    finally:
        dp.free()
        db.free()

"""What the join step no longer launches between its two kernels.

The foreign-key probe that shares its probe columns (k_join_probe_shared) reports a row without a partner into a word of pinned host
memory of the calling thread: no fill of a device control word in front of the kernel, no copy behind it (`runtime.pinned_readback`
off, or `join.probe_host_flag` off, keeps the device word and its copy).  `join_probe_shared_columns` in the profile is a label without
device events.

The one-pass build of the rank map's table (k_rank_tab_onepass) leaves its table unzeroed when the key column's statistics say that no
workgroup's words exceed its LDS window; the verifying build of a column (>= 4 Mi rows, no statistics yet) establishes that, the builds
after it read it (`join_build_rank_tab_no_fill` in the profile names the form that ran).  Every build here is made over pool memory
that was filled with 0xFF just before.

Everything is compared with the CPU oracle.  The oracle's tables of the big probe are computed once and shared."""
import functools
import threading

import numpy as np
import pyarrow as pa
import pytest

from tests.util import assert_tables_equal

pytestmark = pytest.mark.gpu

ROWS = 4096            # rows per workgroup of the build kernel
WINDOW = 1024          # table words it stages in LDS
SPECULATE = 1 << 22    # builds of at least this many rows guess their statistics and verify them (and establish the fit)
SHARE_MIN = 1 << 22    # join.share_probe_min_rows: from here on the all-hit sample is asked
SHARED = "join_probe_shared_columns"
MISSED = "join_probe_speculation_missed"
ONEPASS = "join_build_rank_tab_onepass"
NO_FILL = "join_build_rank_tab_no_fill"


def tpch_keys(n):
    i = np.arange(n, dtype=np.int64)
    return (i // 8) * 32 + i % 8 + 1


# ------------------------------------------------------------------------------------------------ the miss flag in host memory
NB = (1 << 20) + 3
NP = SHARE_MIN + 65                                  # the last word holds one row
# sampled words of the all-hit sample at this size: 1024 words, every 64th, from word 0 (k_sample_all_hit)
MIDDLE = 2_345_679
DANGLING = {
    # the issue's three rows.  Row 0 lies on a sampled word: the SAMPLE finds it and the counted path runs without a speculation
    "first_last_middle": [0, MIDDLE, NP - 1],
    # the same with the first row of the first word the sample does not look at: the KERNEL finds all three
    "unsampled_first_last_middle": [64, MIDDLE, NP - 1],
}
PCOLS = ["pk", "row"]
BCOLS = ["flag", "pay"]


def _sampled(row):
    every = ((NP + 63) // 64) // 1024
    w = row // 64
    return w % every == 0 and w // every < 1024


assert _sampled(0) and not _sampled(64) and not _sampled(MIDDLE) and not _sampled(NP - 1)


@functools.lru_cache(maxsize=None)
def _fk_pair(dangling, seed=0):
    """(build, probe, oracle's Inner join) of the foreign-key probe; `dangling` names the rows whose key no build row has"""
    from oracle import oracle
    rng = np.random.default_rng(41 + seed)
    keys = tpch_keys(NB) - 77_001 * (seed + 1)
    fk = np.sort(rng.integers(0, NB, NP))
    pk = keys[fk].copy()
    if dangling:
        pk[DANGLING[dangling]] = keys[0] - 5
    build = pa.table({"k": pa.array(keys), "flag": pa.array((np.arange(NB) % 7).astype(np.int32)), "pay": pa.array(np.arange(NB, dtype=np.int64) * 7 + 3)})
    probe = pa.table({"pk": pa.array(pk), "row": pa.array(np.arange(NP, dtype=np.int64))})
    exp = oracle.hash_join(build, probe, [("k", "pk")], "Inner").select(BCOLS + PCOLS)
    assert exp.num_rows == NP - (len(DANGLING[dangling]) if dangling else 0)
    return build, probe, exp


class _Options:
    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        from datafusion_amd import ops
        ops.set_options(**self.opts)

    def __exit__(self, *exc):
        from datafusion_amd import ops
        ops.set_options(**{k: None for k in self.opts})


def _host_flag_options(host_flag):
    return {} if host_flag else {"runtime__pinned_readback": 0}


def _probe_once(dangling, probe_mode, seed=0):
    """fresh device tables, a fresh join table, one probe with the profile on: (profile, output as Arrow)"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    build, probe, _ = _fk_pair(dangling, seed)
    db, dp = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    ht = ops.JoinHashTable(db, ["k"], probe_mode=probe_mode)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        out = ht.probe(dp, ["pk"], "Inner", BCOLS, PCOLS)
        stats = ops.profile_stats()
    finally:
        ops.profile_enable(False)
    got = out.to_arrow()
    for t in (out, ht, dp, db):
        t.free()
    return stats, got


def _check_all_hit(stats, got, probe_mode, seed=0):
    assert SHARED in stats and stats[SHARED]["calls"] == 1 and stats[SHARED]["total_ms"] == 0, stats.get(SHARED)
    assert MISSED not in stats and "join_probe_tile_counts" not in stats, sorted(stats)
    assert_tables_equal(got, _fk_pair(None, seed)[2], ordered=True)      # (the shared flavour writes in probe order in every mode)


def _check_dangling(stats, got, dangling, probe_mode):
    assert SHARED not in stats, sorted(stats)
    # a dangling row on a sampled word is the sample's find: no speculation was tried; otherwise the kernel raised its flag
    assert (MISSED in stats) == (not any(_sampled(r) for r in DANGLING[dangling])), (dangling, sorted(stats))
    assert_tables_equal(got, _fk_pair(dangling)[2], ordered=probe_mode == 0)


@pytest.mark.parametrize("host_flag", [True, False], ids=["host_flag", "pinned_readback_off"])
@pytest.mark.parametrize("probe_mode", [0, 3])
def test_all_hit_probe_reports_nothing(probe_mode, host_flag):
    with _Options(**_host_flag_options(host_flag)):
        stats, got = _probe_once(None, probe_mode)
    _check_all_hit(stats, got, probe_mode)


@pytest.mark.parametrize("host_flag", [True, False], ids=["host_flag", "pinned_readback_off"])
@pytest.mark.parametrize("probe_mode", [0, 3])
@pytest.mark.parametrize("dangling", sorted(DANGLING))
@pytest.mark.parametrize("order", ["miss_then_hit", "hit_then_miss"])
def test_dangling_keys_and_the_next_probe_of_the_thread(order, dangling, probe_mode, host_flag):
    """three probe rows without a partner: the oracle's rows through the counted probe; the probe of a fresh all-hit pair that follows
    on the same thread (its flag word is the same word) takes the shared path and is right; and the other way round"""
    with _Options(**_host_flag_options(host_flag)):
        for what in order.split("_then_"):
            if what == "miss":
                stats, got = _probe_once(dangling, probe_mode)
                _check_dangling(stats, got, dangling, probe_mode)
            else:
                stats, got = _probe_once(None, probe_mode, seed=1)
                _check_all_hit(stats, got, probe_mode, seed=1)


@pytest.mark.parametrize("host_flag", [True, False], ids=["host_flag", "pinned_readback_off"])
def test_four_threads_probe_one_join_table(host_flag):
    """each thread has its own stream and its own flag word: three threads' all-hit probes of one shared join table never see the
    flag that the fourth thread's dangling key raises, 20 probes each"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    build, probe, exp = _fk_pair(None)
    _, probe_d, exp_d = _fk_pair("unsampled_first_last_middle")
    cols = ["flag", "row"]       # (one build-side and one probe-side column: 80 outputs are read back)
    want = {False: [exp.column(n).to_numpy() for n in cols], True: [exp_d.column(n).to_numpy() for n in cols]}
    db = DeviceTable.from_arrow(build)
    # every thread probes a table of its own (the remembered answer of the sample belongs to a pair of key buffers)
    probes = [DeviceTable.from_arrow(probe_d if w == 3 else probe) for w in range(4)]
    errors, shared_calls = [], []
    with _Options(**_host_flag_options(host_flag)):
        ht = ops.JoinHashTable(db, ["k"], probe_mode=0)
        start = threading.Barrier(4)

        def worker(w):
            try:
                start.wait()
                for it in range(20):
                    out = ht.probe(probes[w], ["pk"], "Inner", ["flag"], ["row"])
                    got = out.to_arrow()
                    out.free()
                    for n, e in zip(cols, want[w == 3]):
                        assert np.array_equal(got.column(n).to_numpy(), e), (w, it, n)
            except BaseException as e:      # noqa: BLE001
                errors.append((w, e))
        ops.profile_enable(True)
        ops.profile_reset()
        try:
            threads = [threading.Thread(target=worker, args=(w,)) for w in range(4)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            stats = ops.profile_stats()
        finally:
            ops.profile_enable(False)
        shared_calls.append(stats.get(SHARED, {}).get("calls", 0))
    for t in probes + [ht, db]:
        t.free()
    assert not errors, errors
    assert shared_calls == [60], (shared_calls, sorted(stats))      # the three all-hit threads, every time
    assert stats[MISSED]["calls"] == 1, stats[MISSED]               # the fourth thread's first probe; its answer is remembered


# ------------------------------------------------------------------------------------------------ the build without the table fill
def _dirty_pool(nbytes):
    """pool blocks of the table's size (and of the sizes around it) filled with 0xFF and given back: the next table lands on them"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    held = [DeviceTable.from_arrow(pa.table({"x": pa.array(np.full(max(64, n), 0xFF, dtype=np.uint8))})) for n in (nbytes, nbytes - 4096, nbytes + 4096)]
    ops.sync()
    for t in held:
        t.free()


def _build_table(keys, key_type):
    n = len(keys)
    k = pa.array(np.asarray(keys).astype(np.int32 if key_type == pa.int32() else np.int64))
    return pa.table({"k": k, "pay": pa.array(np.arange(n, dtype=np.int64) * 7 + 3)})      # the payload names the build ROW


def _probe_table(keys, absent, key_type):
    """every build key once, the `absent` values, and values just outside the range"""
    keys = np.asarray(keys, dtype=np.int64)
    pk = np.concatenate([keys, np.asarray(absent, dtype=np.int64), np.array([keys[0] - 1, keys[-1] + 1, keys[0] - 64, keys[-1] + 64], dtype=np.int64)])
    assert not np.isin(pk[len(keys):], keys).any()
    return pa.table({"pk": pa.array(pk.astype(np.int32 if key_type == pa.int32() else np.int64)), "row": pa.array(np.arange(len(pk), dtype=np.int64))})


def _empty_words(keys):
    """one value in every 64-value word of the key range that holds no key"""
    idx = np.asarray(keys, dtype=np.int64) - int(keys[0])
    n_words = int(idx[-1] >> 6) + 1
    has = np.zeros(n_words, bool)
    has[idx >> 6] = True
    w = np.flatnonzero(~has).astype(np.int64)
    return int(keys[0]) + w * 64 + (w * 37) % 64


def _two_builds(keys, absent, fits, key_type=pa.int64()):
    """the same join twice over one device table: the first build guesses and verifies (and zeroes its table), the second reads the
    column's statistics and leaves the fill out exactly when `fits`; both over freshly dirtied pool memory, both the oracle's rows"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    from oracle import oracle
    keys = np.asarray(keys, dtype=np.int64)
    assert len(keys) >= SPECULATE and np.all(np.diff(keys) > 0) and len(keys) >= 0.15 * (keys[-1] - keys[0] + 1)
    build, probe = _build_table(keys, key_type), _probe_table(keys, absent, key_type)
    exp = oracle.hash_join(build, probe, [("k", "pk")], "Inner").select(["pay", "pk", "row"])
    assert exp.num_rows == len(keys)
    table_bytes = (int(keys[-1] - keys[0]) // 64 + 1) * 16
    db, dp = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    try:
        for n in range(2):
            _dirty_pool(table_bytes)
            ops.profile_enable(True)
            ops.profile_reset()
            try:
                got = ops.hash_join(db, dp, [("k", "pk")], "Inner", build_cols=["pay"], probe_cols=["pk", "row"]).to_arrow()
                stats = ops.profile_stats()
            finally:
                ops.profile_enable(False)
            assert ONEPASS in stats and "join_build_speculation_missed" not in stats and "join_build_rank_map" not in stats, (n, sorted(stats))
            assert (NO_FILL in stats) == (n == 1 and fits), (n, fits, sorted(stats))
            assert_tables_equal(got, exp)
    finally:
        dp.free()
        db.free()


@pytest.mark.parametrize("key_type", [pa.int64(), pa.int32()], ids=["int64", "int32"])
def test_dense_ascending_keys_build_without_the_fill(key_type):
    """TPC-H order keys (8 of every 32 values: every word holds keys, 256 words per workgroup), 4 Mi + 1 rows, a negative minimum that
    is no multiple of 64; probed with every key and with values no row has"""
    nb = SPECULATE + 1
    keys = tpch_keys(nb) - 1_000_003
    rng = np.random.default_rng(5)
    absent = np.setdiff1d(rng.integers(keys[0], keys[-1], 300_000), keys)
    _two_builds(keys, absent, fits=True, key_type=key_type)


def test_one_locally_sparse_stretch_keeps_the_fill():
    """one gap of 200 000 values inside a workgroup's rows: its 4096 rows span more than 65536 values, so its words exceed the window
    and go to the table one by one — into zeroed memory: the statistic says so and the second build fills as the first did"""
    nb = SPECULATE + 5 * ROWS + 77
    keys = tpch_keys(nb)
    r = 300 * ROWS + 1234
    keys[r:] += 200_000
    assert keys[301 * ROWS - 1] - keys[300 * ROWS] > 65536
    gap = np.arange(keys[r - 1] + 1, keys[r], 61)
    _two_builds(keys, np.concatenate([gap, _empty_words(keys)[::7]]), fits=False)


@pytest.mark.parametrize("words", [WINDOW, WINDOW + 1], ids=["exactly_the_window", "one_word_more"])
def test_a_workgroup_whose_words_just_fit_the_window(words):
    """consecutive keys (64 aligned words per workgroup) with one jump in front of a workgroup's last row: that workgroup owns exactly
    `words` words, all but 65 of them empty.  1024 fit (the kernel writes every one of them, the empty ones as {0, 0}, over 0xFF),
    1025 do not (the fill stays).  Probed with a value in every empty word."""
    nb = SPECULATE + 3 * ROWS
    keys = np.arange(nb, dtype=np.int64) - 64 * 1000          # key - min = row: workgroup b starts word 64 b
    last = 500 * ROWS + ROWS - 1
    keys[last:] += (words - 64) * 64
    idx = keys - keys[0]
    assert (idx[last] >> 6) - ((idx[500 * ROWS - 1] >> 6) + 1) + 1 == words
    empty = _empty_words(keys)
    assert len(empty) == words - 65                           # (64 words of the rows before the jump, and the one the last row opens)
    _two_builds(keys, empty, fits=words <= WINDOW)


@pytest.mark.parametrize("last_key", ["in_the_word_before", "in_a_word_of_its_own"])
def test_a_last_workgroup_of_one_row(last_key):
    """4096 k + 1 rows: the last workgroup has one row, whose key lies in its predecessor's last word (the workgroup owns no word and
    writes nothing) or opens the table's last word (it owns exactly that one)"""
    nb = 1025 * ROWS + 1
    keys = tpch_keys(nb)                  # row nb - 1 = 8 j: the first key of a group of 8, 25 values behind the key before it
    assert keys[-1] - keys[-2] == 25
    if last_key == "in_the_word_before":
        keys[-1] = keys[-2] + 1
        assert (keys[-1] - keys[0]) >> 6 == (keys[-2] - keys[0]) >> 6
    else:
        keys[-1] = keys[-2] + 64
        assert (keys[-1] - keys[0]) >> 6 == ((keys[-2] - keys[0]) >> 6) + 1
    rng = np.random.default_rng(len(last_key))
    absent = np.setdiff1d(np.concatenate([rng.integers(keys[0], keys[-1], 100_000), np.arange(keys[-2] - 70, keys[-1] + 1)]), keys)
    _two_builds(keys, absent, fits=True)


def test_the_bitmap_made_from_a_table_that_was_never_zeroed():
    """a probe of which 10 % of the rows hit takes the counts pass, which streams the keys through the bitmap: made from the table
    (ensure_rank_bits), here from a table built without the fill over 0xFF"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    from oracle import oracle
    rng = np.random.default_rng(77)
    nb, npr = SPECULATE + 1, 2_000_000
    keys = np.arange(nb, dtype=np.int64) * 4 - 4_000_001       # one value in four is a key
    keys[2_000_000:] += 64 * 700                                # and 700 words without any (256 + 700 still fit the window)
    build = _build_table(keys, pa.int64())
    span = int(keys[-1] - keys[0])
    pk = rng.integers(keys[0] - 3 * span // 4, keys[-1] + 3 * span // 4, npr)
    empty = _empty_words(keys)
    assert 690 <= len(empty) <= 700
    pk[:len(empty)] = empty
    probe = pa.table({"pk": pa.array(pk), "row": pa.array(np.arange(npr, dtype=np.int64))})
    exp = oracle.hash_join(build, probe, [("k", "pk")], "Inner").select(["pay", "pk", "row"])
    assert 0.05 < exp.num_rows / npr < 0.15
    db, dp = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    try:
        ops.JoinHashTable(db, ["k"]).free()                     # the verifying build: the column's statistics
        _dirty_pool((span // 64 + 1) * 16)
        ops.profile_enable(True)
        ops.profile_reset()
        try:
            ht = ops.JoinHashTable(db, ["k"])
            out = ht.probe(dp, ["pk"], "Inner", ["pay"], ["pk", "row"])
            stats = ops.profile_stats()
        finally:
            ops.profile_enable(False)
        assert NO_FILL in stats and "join_build_rank_deinterleave" in stats and "join_probe_tile_counts" in stats, sorted(stats)
        assert_tables_equal(out.to_arrow(), exp)
        out.free()
        ht.free()
    finally:
        dp.free()
        db.free()

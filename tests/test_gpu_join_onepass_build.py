"""The one-pass build of the rank map's interleaved table (k_rank_tab_onepass): strictly ascending build keys without NULLs at a key
density >= 0.15.  A workgroup takes 4096 consecutive build rows, owns the bitmap words whose first key lies among them, stages
1024 words in LDS and writes runs beyond that window directly; >= 4 Mi rows without cached statistics build on a guess that the
same pass verifies.  Every case is the same join three ways: the CPU oracle, the GPU's chained hash table (table_mode 1, which
shares nothing with the rank map) and the default table, whose profile must name the one-pass build.  The payload is gathered, so
a wrong prefix shows as a wrong build row and not only as a wrong hit."""
import threading

import numpy as np
import pyarrow as pa
import pytest

from tests.util import assert_tables_equal

pytestmark = pytest.mark.gpu

ROWS = 4096          # rows per workgroup of the build kernel
WINDOW = 1024        # bitmap words it stages in LDS
SPECULATE = 1 << 22  # builds of at least this many rows guess their statistics
JOIN_TYPES = ("Inner", "Left", "RightSemi")
ONEPASS = "join_build_rank_tab_onepass"


def tpch_keys(n):
    i = np.arange(n, dtype=np.int64)
    return (i // 8) * 32 + i % 8 + 1


def build_table(keys, key_type=pa.int64()):
    n = len(keys)
    k = pa.array(np.asarray(keys).astype(np.int32 if key_type != pa.int64() else np.int64))
    if key_type != k.type:
        k = k.cast(key_type)
    # the payload names the build ROW: a rank that is off by one gathers another row's value
    return pa.table({"k": k, "pay": pa.array(np.arange(n, dtype=np.int64) * 7 + 3), "pay32": pa.array((np.arange(n) % 100_003).astype(np.int32))})


def probe_table(keys, extra, rng, key_type=pa.int64(), n_random=200_000):
    """probe keys: `extra` (the case's own edge keys), a sample of build keys, keys drawn from the whole range and a little beyond it"""
    keys = np.asarray(keys, dtype=np.int64)
    lo, hi = int(keys.min()), int(keys.max())
    parts = [np.asarray(extra, dtype=np.int64), keys[rng.integers(0, len(keys), n_random)], rng.integers(lo - 200, hi + 200, n_random)]
    parts.append(np.array([lo, hi, lo - 1, hi + 1, lo - 64, hi + 64], dtype=np.int64))
    pk = np.concatenate(parts)
    rng.shuffle(pk)
    k = pa.array(pk.astype(np.int32 if key_type != pa.int64() else np.int64))
    if key_type != k.type:
        k = k.cast(key_type)
    return pa.table({"pk": k, "row": pa.array(np.arange(len(pk), dtype=np.int64))})


def check_joins(build, probe, expect_missed=False, expect_stats_pass=None):
    """Inner / Left / RightSemi over fresh device tables (no cached statistics on the first build, cached ones afterwards)"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    from oracle import oracle
    b, p = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    for n, jt in enumerate(JOIN_TYPES):
        bcols = [] if jt == "RightSemi" else ["k", "pay", "pay32"]
        exp = oracle.hash_join(build, probe, [("k", "pk")], jt).select(bcols + ["pk", "row"])
        ops.profile_enable(True)
        ops.profile_reset()
        got = ops.hash_join(b, p, [("k", "pk")], jt, build_cols=bcols, probe_cols=["pk", "row"]).to_arrow()
        stats = ops.profile_stats()
        ops.profile_enable(False)
        if expect_missed:
            # the flawed column is never ascending: the first build guesses and misses, later ones read the measured statistics
            assert ("join_build_speculation_missed" in stats) == (n == 0), (jt, sorted(stats))
            assert (ONEPASS in stats) == (n == 0), (jt, sorted(stats))
        else:
            assert ONEPASS in stats and "join_build_speculation_missed" not in stats, (jt, sorted(stats))
            assert "join_build_rank_map" not in stats, (jt, sorted(stats))          # no bitmap pass (and so no scan of one)
            if expect_stats_pass is not None:
                assert ("join_build_key_stats" in stats) == (expect_stats_pass and n == 0), (jt, sorted(stats))
        assert_tables_equal(got, exp)
        chained = ops.hash_join(b, p, [("k", "pk")], jt, build_cols=bcols, probe_cols=["pk", "row"], table_mode=1).to_arrow()
        assert_tables_equal(got, chained)


@pytest.mark.parametrize("nb", [1, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1, 5 * ROWS - 64, 5 * ROWS - 63])
@pytest.mark.parametrize("shape", ["consecutive", "tpch", "stride6"])
def test_build_sizes_around_the_row_block(nb, shape):
    """just below, at and above one workgroup's rows; a last workgroup of one row; density 1 (one word per 64 rows), TPC-H order keys
    (8 of every 32), stride 6 (0.17)"""
    rng = np.random.default_rng(nb * 3 + len(shape))
    keys = {"consecutive": np.arange(nb, dtype=np.int64) + 5, "tpch": tpch_keys(nb), "stride6": np.arange(nb, dtype=np.int64) * 6 - 77}[shape]
    build = build_table(keys)
    check_joins(build, probe_table(keys, keys[-130:], rng, n_random=20_000), expect_stats_pass=True)


@pytest.mark.parametrize("nb", [SPECULATE - 1, SPECULATE, SPECULATE + 1])
def test_build_sizes_around_the_speculation_threshold(nb):
    """below 4 Mi rows the statistics are measured first and the plain form of the kernel runs; from 4 Mi on the first build guesses
    them and the verifying form runs; the builds after it read what the column has cached"""
    rng = np.random.default_rng(nb)
    keys = tpch_keys(nb) - 1_000_003
    edge = np.concatenate([keys[:70], keys[-70:], keys[ROWS - 3:ROWS + 3]])
    check_joins(build_table(keys), probe_table(keys, edge, rng), expect_stats_pass=nb < SPECULATE)


@pytest.mark.parametrize("before", [0, 1, 32, 63])
def test_a_word_that_straddles_two_row_blocks(before):
    """consecutive keys: `before` keys of a bitmap word are the last rows of one workgroup, the other 64 - `before` the first rows of
    the next (0: word and block boundaries coincide); the minimum key is negative and no multiple of 64"""
    rng = np.random.default_rng(before)
    nb = 7 * ROWS + 17
    keys = np.arange(nb, dtype=np.int64) - 1_000_037
    keys[100:] += before          # key - min of row r >= 100 is r + before: row 4096 k is key number `before` of its word
    idx = keys - keys[0]
    for blk in range(1, 7):
        w = idx[blk * ROWS] >> 6
        assert int(((idx[:blk * ROWS] >> 6) == w).sum()) == before and int(((idx[blk * ROWS:] >> 6) == w).sum()) == 64 - before
    edge = np.concatenate([keys[b * ROWS - 70:b * ROWS + 70] for b in range(1, 7)] + [np.arange(keys[99] - 3, keys[100] + 3)])
    check_joins(build_table(keys), probe_table(keys, edge, rng, n_random=50_000))


@pytest.mark.parametrize("key_type", [pa.int32(), pa.date32(), pa.int64()], ids=["int32", "date32", "int64"])
def test_key_types_and_a_negative_minimum(key_type):
    rng = np.random.default_rng(9)
    nb = 3 * ROWS + 1000
    keys = tpch_keys(nb) - 20_011
    assert keys[0] < 0 and keys[0] % 64 != 0
    edge = np.concatenate([keys[ROWS - 40:ROWS + 40], keys[:40], keys[-40:]])
    check_joins(build_table(keys, key_type), probe_table(keys, edge, rng, key_type, n_random=50_000))


def sparse_keys(run_rows, gaps, tail_rows=0):
    """dense runs (consecutive keys) of `run_rows` rows separated by `gaps` unused key values; returns keys, first and last key of each run"""
    runs, start = [], 11
    for g in list(gaps) + [0]:
        runs.append(np.arange(start, start + run_rows, dtype=np.int64))
        start += run_rows + g
    if tail_rows:
        runs.append(np.arange(start, start + tail_rows, dtype=np.int64))
    keys = np.concatenate(runs)
    return keys, np.array([r[0] for r in runs]), np.array([r[-1] for r in runs])


@pytest.mark.parametrize("case", ["one_word", "beyond_the_window", "millions_of_words"])
def test_locally_sparse_builds(case):
    """dense runs separated by gaps of one word, of more words than a workgroup stages in LDS (the runs behind such a gap inside one
    workgroup's rows go to the table directly, and their words are split between waves because the gap is no multiple of 64), and
    of millions of words; still >= 0.15 dense overall.  Probes land in the gaps and on the first and last key of every run."""
    rng = np.random.default_rng(len(case))
    if case == "one_word":
        keys, first, last = sparse_keys(1000, [64] * 40)
    elif case == "beyond_the_window":
        gap = (WINDOW + 2000) * 64 + 17
        keys, first, last = sparse_keys(1500, [gap, gap + 5, 64 * WINDOW - 1, gap, 3 * gap], tail_rows=4_000_000)
        assert len(keys) < SPECULATE
    else:
        gap = 2_000_001 * 64 + 29
        keys, first, last = sparse_keys(700, [gap, 64, 123_457 * 64 + 1], tail_rows=24_000_000)
        assert len(keys) >= SPECULATE
    assert len(keys) >= 0.15 * (keys[-1] - keys[0] + 1)
    assert np.all(np.diff(keys) > 0)
    edge = np.concatenate([first, last, first - 1, last + 1, first + 1, last - 1, (first[1:] + last[:-1]) // 2])
    check_joins(build_table(keys), probe_table(keys, edge, rng))


def _not_sampled(nb, rows):
    """the build's guess samples 4096 neighbour pairs (i * (nb // 4096), + 1): the flaw must lie between them, or nothing is speculated"""
    every = nb // 4096
    sampled = set()
    for i in range(4096):
        sampled.update((i * every, i * every + 1))
    return not (sampled & set(int(r) for r in rows))


@pytest.mark.parametrize("where", ["block_boundary", "interior"])
@pytest.mark.parametrize("flaw", ["swapped_pair", "repeated_key", "last_key_small"])
def test_a_guess_that_does_not_hold(flaw, where):
    """>= 4 Mi rows without cached statistics: one swapped pair, one repeated key, a last key below an interior key (and so a range
    guessed too small), across a workgroup's boundary and inside one: the verifying pass raises the flag, the table is built again
    from measured statistics and the join is the oracle's"""
    rng = np.random.default_rng(len(flaw) + len(where))
    if flaw == "last_key_small":
        nb = 1025 * ROWS + (1 if where == "block_boundary" else 1700)      # the last row opens a workgroup / lies inside one
        keys = tpch_keys(nb)
        keys[-1] = keys[-1000] + 12       # a value no other row has, below the 999 keys before it
        touched = [nb - 2, nb - 1]
        assert keys[-1] - keys[0] + 1 >= nb
    else:
        nb = SPECULATE + 5000
        keys = tpch_keys(nb)
        r = 300 * ROWS if where == "block_boundary" else 300 * ROWS + 1234     # rows r - 1 and r
        if flaw == "swapped_pair":
            keys[[r - 1, r]] = keys[[r, r - 1]]
        else:
            keys[r] = keys[r - 1]
        touched = [r - 1, r]
    assert nb >= SPECULATE and _not_sampled(nb, touched)
    edge = np.concatenate([keys[touched[0] - 70:touched[1] + 70], keys[:10], keys[-10:]])
    check_joins(build_table(keys), probe_table(keys, edge, rng), expect_missed=True)


def test_probes_that_want_the_bitmap_alone_after_a_one_pass_build():
    """the one-pass build leaves the interleaved table only; a probe whose counts pass streams every key through the bitmap (10 % of
    the probe keys exist; a probe with a row mask) makes the bitmap from the table, once, also when two threads ask together"""
    import pyarrow.compute as pc

    from datafusion_amd import ops
    from datafusion_amd.expr import col, lit
    from datafusion_amd.table import DeviceTable
    from oracle import oracle
    rng = np.random.default_rng(77)
    nb, npr = 600_000, 2_000_000
    keys = tpch_keys(nb) - 4_000_001
    build = build_table(keys)
    span = int(keys[-1] - keys[0])
    pk = rng.integers(keys[0] - 3 * span // 4, keys[-1] + 3 * span // 4, npr)      # 1 / 4 of the range's values are keys: ~ 10 % hits
    probe = pa.table({"pk": pa.array(pk), "row": pa.array(np.arange(npr, dtype=np.int64)), "q": pa.array(rng.integers(0, 50, npr).astype(np.int32))})
    b, p = DeviceTable.from_arrow(build), DeviceTable.from_arrow(probe)
    exp = oracle.hash_join(build, probe, [("k", "pk")], "Inner").select(["pay", "pay32", "pk", "row"])
    assert 0.05 < exp.num_rows / npr < 0.15
    n_words = (span >> 6) + 1

    ht = ops.JoinHashTable(b, ["k"])
    assert ht.info().table_bytes == n_words * 16                       # the table and nothing else
    results, errors = {}, []

    def worker(w):
        try:
            results[w] = ht.probe(p, ["pk"], "Inner", ["pay", "pay32"], ["pk", "row"]).to_arrow()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    ops.profile_enable(True)
    ops.profile_reset()
    threads = [threading.Thread(target=worker, args=(w,)) for w in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    stats = ops.profile_stats()
    ops.profile_enable(False)
    assert not errors, errors
    assert stats["join_build_rank_deinterleave"]["calls"] == 1 and "join_probe_tile_counts" in stats, sorted(stats)
    assert ht.info().table_bytes == n_words * 24                       # + the bitmap, made once
    for w in range(2):
        assert_tables_equal(results[w], exp)
    # a FilterExec fused below the probe side: its row mask rides through the counts pass
    kept = probe.filter(pc.less(probe.column("q"), 20))
    exp_kept = oracle.hash_join(build, kept, [("k", "pk")], "Inner").select(["pay", "pay32", "pk", "row"])
    got = ht.probe(p, ["pk"], "Inner", ["pay", "pay32"], ["pk", "row"], predicate=col("q") < lit(20, pa.int32())).to_arrow()
    assert_tables_equal(got, exp_kept)
    for jt in ("RightSemi", "RightAnti"):
        got = ht.probe(p, ["pk"], jt, [], ["pk", "row"]).to_arrow()
        assert_tables_equal(got, oracle.hash_join(build, probe, [("k", "pk")], jt).select(["pk", "row"]))
    ht.free()
    # the row-masked probe as the FIRST one of a fresh table, against the chained table as well
    for mode in (0, 1):
        ht = ops.JoinHashTable(b, ["k"], table_mode=mode)
        got = ht.probe(p, ["pk"], "Inner", ["pay", "pay32"], ["pk", "row"], predicate=col("q") < lit(20, pa.int32())).to_arrow()
        assert_tables_equal(got, exp_kept)
        ht.free()

"""Inputs of the sort route ledger (tests/test_gpu_sort_routes.py): one named case per branch of sort.hip's host half — the edges, one
workgroup in LDS, the two-level id sort and its skewed fallback, the carried sorts in their three modes, the LSD record sort, the two
TopK narrowings — each at the smallest shape that still reaches its branch.  A case is a table (seeded), the sort keys, the fetch and
the options it runs under; tests/golden/sort_routes.json holds what ops.profile_stats() recorded for it as {name: [calls, bytes]}."""
import functools
from collections import namedtuple

import numpy as np
import pyarrow as pa

Case = namedtuple("Case", "name table keys fetch options")   # table: () -> pa.Table; keys: [(column, descending, nulls_first)]
CARRIED = {"sort__carried_min_rows": "0", "sort__lsd": "0"}   # the carried sorts on small tables, the LSD record sort out of their way
LSD = {"sort__carried_min_rows": "0"}


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _ids(n):
    return pa.array(np.arange(n, dtype=np.int64))


def _date(values):
    return pa.array(values.astype(np.int32), pa.int32()).cast(pa.date32())


@functools.lru_cache(maxsize=None)
def spread(n, seed=1):
    """one Int64 key spread over 2^41 values, the row number as payload"""
    return pa.table({"a": pa.array(_rng(n, seed).integers(-2**40, 2**40, size=n)), "v": _ids(n)})


@functools.lru_cache(maxsize=None)
def constant(n):
    return pa.table({"a": pa.array(np.full(n, 7, dtype=np.int64)), "v": _ids(n)})


@functools.lru_cache(maxsize=None)
def skewed(n):
    """three values hold the top bits: a bucket of the two-level sort holds a third of the rows"""
    rng = _rng(n, 2)
    return pa.table({"a": pa.array((rng.integers(0, 3, size=n) << 40) + rng.integers(0, 2**20, size=n)), "v": _ids(n)})


@functools.lru_cache(maxsize=None)
def mixed(n, null_frac=0.1):
    """Decimal128, Float64 and Int32 keys with NULLs (a packed key of two words), UInt8 and Date32 beside them"""
    rng = _rng(n, 3)
    mask = lambda: rng.random(n) < null_frac
    return pa.table({"d": pa.array([int(x) for x in rng.integers(-10**6, 10**6, n)], pa.decimal128(15, 2), mask=mask()),
                     "f": pa.array(rng.uniform(-100, 100, n), mask=mask()), "q": pa.array(rng.integers(-5, 5, n).astype(np.int32), mask=mask()),
                     "c": pa.array(rng.integers(0, 4, n).astype(np.uint8)), "dt": _date(rng.integers(9000, 9100, n)), "v": _ids(n)})


@functools.lru_cache(maxsize=None)
def payload_20_bytes(n):
    rng = _rng(n, 4)
    return pa.table({"a": pa.array(rng.integers(-2**40, 2**40, size=n)), "v": _ids(n), "w": pa.array(rng.integers(0, 9, n)),
                     "x": pa.array(rng.integers(0, 9, n).astype(np.int32))})


@functools.lru_cache(maxsize=None)
def nullable_key(n):
    rng = _rng(n, 5)
    return pa.table({"a": pa.array(rng.integers(-2**40, 2**40, size=n), mask=rng.random(n) < 0.01), "v": _ids(n)})


@functools.lru_cache(maxsize=None)
def orders(n):
    """a date and a key that is strictly ascending in row order (which leaves the LSD sort's key), 12 bytes of payload"""
    rng = _rng(n, 6)
    return pa.table({"o_orderkey": pa.array(np.cumsum(rng.integers(1, 9, n)).astype(np.int64)), "o_custkey": pa.array(rng.integers(1, 10**6, n)),
                     "o_orderdate": _date(rng.integers(8035, 10441, n)), "o_shippriority": pa.array(rng.integers(0, 3, n).astype(np.int32))})


@functools.lru_cache(maxsize=None)
def u8_key(n):
    rng = _rng(n, 7)
    return pa.table({"c": pa.array(rng.integers(3, 200, n).astype(np.uint8)), "v": _ids(n), "w": pa.array(rng.integers(0, 2**31, n).astype(np.int32))})


@functools.lru_cache(maxsize=None)
def record_32_bytes(n):
    """two keys of 13 + 11 bits (three passes); Int64, UInt8 and Decimal128 payload: 25 bytes and the key word"""
    rng = _rng(n, 8)
    return pa.table({"d": pa.array(rng.integers(-3000, 3000, n).astype(np.int32)), "e": pa.array(rng.integers(0, 1500, n)), "x": pa.array(rng.integers(-2**62, 2**62, n)),
                     "y": pa.array(rng.integers(0, 255, n).astype(np.uint8)), "dec": pa.array([int(v) for v in rng.integers(-10**15, 10**15, n)], pa.decimal128(30, 2))})


@functools.lru_cache(maxsize=None)
def ties(n):
    rng = _rng(n, 9)
    return pa.table({"a": pa.array(rng.integers(0, 5, n)), "v": _ids(n), "row": pa.array(np.arange(n, dtype=np.int64) * 3)})


@functools.lru_cache(maxsize=None)
def record_over_32_bytes(n):
    rng = _rng(n, 10)
    return pa.table({"a": pa.array(rng.integers(0, 4000, n)), "v": _ids(n), "w": pa.array(rng.integers(0, 9, n)), "x": pa.array(rng.integers(0, 9, n)),
                     "y": pa.array(rng.integers(0, 9, n))})


@functools.lru_cache(maxsize=None)
def key_over_32_bits(n):
    return pa.table({"a": pa.array(_rng(n, 11).integers(0, 2**33, n)), "v": _ids(n)})


@functools.lru_cache(maxsize=None)
def small_key(n):
    return pa.table({"a": pa.array(_rng(n, 12).integers(0, 4000, n)), "v": _ids(n)})


@functools.lru_cache(maxsize=None)
def nearly_equal_keys(n):
    """one row in a thousand differs: a one-bit key, nearly every row lies under any sampled limit"""
    return pa.table({"a": pa.array((_rng(n, 13).random(n) < 0.001).astype(np.uint8)), "v": pa.array(np.arange(n, dtype=np.int32))})


def _case(name, table, *args, keys, fetch=None, options=None):
    return Case(name, functools.partial(table, *args), keys, fetch, dict(options or {}))


A = [("a", False, False)]
A_DESC = [("a", True, False)]
THREE_KEYS = [("d", True, False), ("f", False, True), ("q", True, True)]
N_TOPK = 1_300_003

CASES = [
    # ---- edges
    _case("empty", spread, 0, keys=A),
    _case("one_row", spread, 1, keys=A),
    _case("constant_key", constant, 100, keys=A),                       # no digits: ids are positions
    # ---- one workgroup in LDS
    _case("lds_100", mixed, 100, keys=THREE_KEYS),
    _case("lds_4096", spread, 4096, keys=A),
    _case("rows_4097", spread, 4097, keys=A),                           # one row too many for the LDS route
    _case("rows_4097_fetch_10", spread, 4097, keys=A, fetch=10),        # narrowed first, then the LDS route
    _case("lds_100_switched_off", mixed, 100, keys=THREE_KEYS, options={"sort__small": "0"}),
    # ---- two-level ids
    _case("two_level_spread", spread, 70_000, keys=A),
    _case("two_level_skewed", skewed, 70_000, keys=A_DESC),             # a bucket beyond LS_CAP: keys packed again, radix passes finish
    _case("three_keys_two_words", mixed, 30_000, keys=THREE_KEYS),      # straight to the radix passes
    # ---- carried sorts
    _case("carried_onesweep_one_top_pass", spread, 5000, keys=A, options=CARRIED),
    _case("carried_onesweep_two_top_passes", spread, 700_000, keys=A, options=CARRIED),
    _case("carried_ids", spread, 5000, keys=A, options={**CARRIED, "sort__carried": "ids"}),
    _case("carried_passes", spread, 5000, keys=A, options={**CARRIED, "sort__carried": "passes"}),
    _case("carried_one_bucket_onesweep", spread, 1500, keys=A_DESC, options=CARRIED),
    _case("carried_one_bucket_ids", spread, 1500, keys=A_DESC, options={**CARRIED, "sort__carried": "ids"}),
    _case("carried_one_bucket_passes", spread, 1500, keys=A_DESC, options={**CARRIED, "sort__carried": "passes"}),
    _case("carried_declines_skewed_ids", skewed, 70_000, keys=A_DESC, options={**CARRIED, "sort__carried": "ids"}),   # clobbers, declines, re-pack
    _case("carried_declines_payload_20_bytes", payload_20_bytes, 5000, keys=A, options=CARRIED),
    _case("carried_declines_nullable_key", nullable_key, 5000, keys=[("a", False, True)], options=CARRIED),
    # ---- LSD record sort
    _case("lsd_date_then_ascending_key_asc", orders, 300_001, keys=[("o_orderdate", False, False), ("o_orderkey", False, False)], options=LSD),
    _case("lsd_date_then_ascending_key_desc", orders, 300_001, keys=[("o_orderdate", False, False), ("o_orderkey", True, False)], options=LSD),
    _case("lsd_look_back_asc", orders, 300_001, keys=[("o_orderdate", False, False), ("o_orderkey", False, False)], options={**LSD, "sort__lsd_ahead": "0"}),
    _case("lsd_look_back_desc", orders, 300_001, keys=[("o_orderdate", False, False), ("o_orderkey", True, False)], options={**LSD, "sort__lsd_ahead": "0"}),
    _case("lsd_one_pass_u8_key", u8_key, 20_000, keys=[("c", True, False)], options=LSD),
    _case("lsd_three_passes_32_byte_record", record_32_bytes, 20_000, keys=[("e", False, False), ("d", True, False)], options=LSD),
    _case("lsd_ragged_last_tile_ties", ties, 2048 * 5 + 3, keys=[("a", True, False), ("row", True, False), ("v", False, False)], options=LSD),
    _case("lsd_declines_record_over_32_bytes", record_over_32_bytes, 20_000, keys=A, options=LSD),
    _case("lsd_declines_key_over_32_bits", key_over_32_bits, 20_000, keys=A, options=LSD),
    _case("lsd_declines_key_listed_twice", small_key, 20_000, keys=[("a", False, False), ("a", True, False)], options=LSD),
    # ---- TopK
    _case("topk_sampled_limit_fetch_10", spread, N_TOPK, keys=A, fetch=10),             # ~1400 rows under the limit: straight to the LDS sort
    _case("topk_sampled_limit_no_second_narrowing", spread, N_TOPK, keys=A, fetch=10, options={"sort__topk_second_narrowing": "0"}),
    _case("topk_sampled_limit_fetch_2000", spread, N_TOPK, keys=A, fetch=2000),         # ~5400 under the limit, the second narrowing leaves ~4000 to the LDS sort
    _case("topk_sampled_limit_fetch_5000", spread, N_TOPK, keys=A, fetch=5000),         # more than the LDS sort holds: the radix passes sort who passed
    _case("topk_equal_keys", constant, N_TOPK, keys=[("a", True, True)], fetch=10),     # a key of no bits: nothing to narrow by
    _case("topk_too_many_under_the_limit", nearly_equal_keys, (1 << 22) + 100_000, keys=A, fetch=10),   # more than 2^22 pass: the radix select takes over
    _case("topk_two_word_key", mixed, 100_000, keys=[("d", True, False), ("f", False, True)], fetch=10),   # the radix select directly
]
BY_NAME = {c.name: c for c in CASES}


def run(case):
    """the case on the GPU -> (sorted table as Arrow, {profile name: [calls, bytes]} of everything that ran inside ops.sort)"""
    from datafusion_amd import ops
    from datafusion_amd.table import DeviceTable
    dev = DeviceTable.from_arrow(case.table())
    ops.set_options(**case.options)
    ops.profile_enable(True)
    ops.profile_reset()
    try:
        out = ops.sort(dev, case.keys, case.fetch)
        ledger = {k: [v["calls"], v["bytes"]] for k, v in ops.profile_stats().items()}
        got = out.to_arrow()
        out.free()
        return got, ledger
    finally:
        ops.profile_enable(False)
        ops.reset_options()
        dev.free()


if __name__ == "__main__":   # python -m tests.sort_route_cases OUT.json: records the ledger of the commit it runs at
    import json
    import sys
    with open(sys.argv[1], "w") as f:
        json.dump({c.name: dict(sorted(run(c)[1].items())) for c in CASES}, f, indent=1)
        f.write("\n")

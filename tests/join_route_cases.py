"""Inputs of the join route ledger (tests/test_zzz_gpu_join_routes.py): one named case per branch of join_probe's host code in join.hip —
the radix table, counts + placed over every table kind, the listed emits, the shared columns and the speculated placed probe, the
single-pass flavours, the grouped keys and the returned lookup, first match, the pairs in one pass, the general pairs, the null-aware
anti joins and the argument errors — each at the smallest shape that still reaches its branch.  A case is a seeded build and probe
table, the join options, the probe call and the options it runs under; tests/golden/join_routes.json holds what the probe recorded:
{"profile": {name: [calls, bytes]}, "info": [probe_rows, output_rows]} or {"error": message}.

Shapes: N = two 2048-row fused tiles and a ragged word of one row; the first probe row hits and the last one misses unless the case
says otherwise.  Three thresholds have no test hook: the clustered-keys sample answers "clustered" below 2^16 rows (the grouped and the
returned cases use N16 = 2^16 + 65), the pairs in one pass need 2^16 rows, the narrow-row rule 2^22."""
import functools
from collections import namedtuple
from decimal import Decimal

import numpy as np
import pyarrow as pa

Case = namedtuple("Case", "name build probe on join_type build_cols probe_cols join call predicate options probes probe_slice ordered null_equality")
N = 2 * 2048 + 65
N16 = (1 << 16) + 65
N17 = (1 << 17) + 65
N22 = (1 << 22) + 65
TABLE_MODE = {"auto": 0, "chained": 1, "array": 2, "rank": 3, "radix": 4, "flat": 5}
SHARE = {"join__share_probe_min_rows": "1"}
UNCLUSTERED = {"join__beyond_cache_bytes": "0", "join__grouped_min_rows": "0", "join__grouped_bits": "3", "join__near_window": "1000"}


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def _dec(values):
    return pa.array([Decimal(int(v)).scaleb(-2) for v in values], type=pa.decimal128(15, 2))


@functools.lru_cache(maxsize=None)
def build(nb=1500, step=3, order="ascending", dup=1, extra="", seed=1):
    """build keys step * i + 2 (unique unless dup > 1: every key `dup` times), one payload column of every width; extra: "nullable" (a
    payload column with NULLs), "utf8", "wide" (four Decimal128 columns: 64 bytes), "two_keys" (a second key column), "null_keys",
    "many" (13 Int32 columns)"""
    rng = _rng(nb, step, dup, seed)
    keys = np.repeat(np.arange(nb // dup, dtype=np.int64) * step + 2, dup)
    if order == "shuffled":
        rng.shuffle(keys)
    nb = len(keys)
    cols = {"bk": pa.array(keys, mask=(rng.random(nb) < 0.05) if extra == "null_keys" else None)}
    if extra == "two_keys":
        cols["bk2"] = pa.array(keys * 5 - 1)
    cols["b_i32"] = pa.array((keys % 1000).astype(np.int32))
    cols["b_i64"] = pa.array(keys * 11)
    cols["b_u8"] = pa.array((keys % 251).astype(np.uint8))
    cols["b_dec"] = _dec(keys * 7)
    if extra == "nullable":
        cols["b_n"] = pa.array(keys * 13, mask=rng.random(nb) < 0.1)
    if extra == "utf8":
        cols["b_s"] = pa.array([f"s{k}" for k in keys])
    if extra == "wide":
        for i in range(3):
            cols[f"b_dec{i}"] = _dec(keys * (3 + i))
    if extra == "many":
        for i in range(13):
            cols[f"m{i}"] = pa.array(((keys + i) % 97).astype(np.int32))
    return pa.table(cols)


@functools.lru_cache(maxsize=None)
def probe(npr=N, hit=0.6, nb=1500, step=3, miss_rows=(-1,), extra="", seed=2, sorted_keys=False, matches_by_parity=0):
    """probe keys: a build key with probability `hit`, else a key between two build keys, below the range or above it; `miss_rows` miss
    whatever was drawn and row 0 hits (with hit = 1 every other row hits).  p_i32 is the row number, p_f is uniform in [0, 100)"""
    rng = _rng(npr, nb, step, seed)
    at = rng.integers(0, nb, npr)
    if sorted_keys:
        at = np.sort(at)
    keys = at.astype(np.int64) * step + 2
    miss = rng.random(npr) >= hit
    off = rng.integers(0, 3, npr)
    keys = np.where(miss, np.where(off == 0, keys + 1, np.where(off == 1, -5 - at, nb * step + 7 + at)), keys)
    if npr:
        keys[0] = 2
        for r in miss_rows:
            keys[r] = 3
    if matches_by_parity:   # even rows: the first `nb // 2` keys (one build row each), odd rows: the others (`matches_by_parity` build rows each)
        keys = np.where(np.arange(npr) % 2 == 0, (at % (nb // 2)) * step + 2, (nb // 2 + at % (nb // 2)) * step + 2).astype(np.int64)
    cols = {"pk": pa.array(keys, mask=(rng.random(npr) < 0.03) if extra == "null_keys" else None)}
    if extra == "two_keys":
        cols["pk2"] = pa.array(keys * 5 - 1)
    cols["p_i64"] = pa.array(rng.integers(-2**62, 2**62, npr))
    cols["p_i32"] = pa.array(np.arange(npr, dtype=np.int32))
    cols["p_f"] = pa.array(rng.integers(0, 100, npr).astype(np.int32))
    if extra == "nullable":
        cols["p_n"] = pa.array(rng.integers(0, 9, npr), mask=rng.random(npr) < 0.1)
    if extra == "key_copy":
        cols["pk_copy"] = cols["pk"]
    return pa.table(cols)


@functools.lru_cache(maxsize=None)
def build_by_parity(nb_keys=2000, many=8):
    """the first half of the keys once, the second half `many` times each"""
    keys = np.arange(nb_keys, dtype=np.int64) * 3 + 2
    keys = np.concatenate([keys[:nb_keys // 2], np.repeat(keys[nb_keys // 2:], many)])
    return pa.table({"bk": pa.array(keys), "b_i32": pa.array(np.arange(len(keys), dtype=np.int32))})


def simple_pred(below):
    from datafusion_amd.expr import col, lit
    return col("p_f") < lit(below, pa.int32())


def other_pred():
    from datafusion_amd.expr import col
    return col("p_f") < col("p_i32")   # a comparison of two columns: a mask


CASES = []


def _case(name, b, p, join_type="Inner", build_cols=("b_i32",), probe_cols=("pk", "p_i64"), mode="auto", probe_mode=0, null_aware=False, call="plain",
          predicate=None, options=None, probes=1, probe_slice=None, ordered=True, on=(("bk", "pk"),), null_equality="NullEqualsNothing"):
    join = {"table_mode": TABLE_MODE[mode], "probe_mode": probe_mode, "null_aware": null_aware}
    CASES.append(Case(name, b, p, list(on), join_type, list(build_cols), list(probe_cols), join, call, predicate, dict(options or {}), probes, probe_slice, ordered,
                      null_equality))


B = functools.partial(functools.partial, build)
P = functools.partial(functools.partial, probe)
TWO = (("bk", "pk"), ("bk2", "pk2"))

# ---- radix table
_case("radix_inner_fused_emit", B(), P(), mode="radix", ordered=False)
_case("radix_left_goes_on_to_the_filter_path", B(), P(), "Left", mode="radix", ordered=False)
_case("radix_predicate_not_consumed", B(), P(), mode="radix", call="predicate", predicate=functools.partial(simple_pred, 50), ordered=False)
# ---- counts + placed
_case("placed_array", B(), P(), mode="array")
_case("placed_rank", B(), P(), mode="rank")
_case("placed_flat", B(), P(), mode="flat")
_case("placed_flat16", B(extra="two_keys"), P(extra="two_keys"), mode="flat", on=TWO, probe_cols=("pk", "pk2", "p_i64"))
_case("placed_chained_two_keys", B(extra="two_keys"), P(extra="two_keys"), mode="chained", on=TWO, probe_cols=("pk", "pk2", "p_i64"))
_case("placed_right_semi", B(), P(), "RightSemi", mode="rank")
_case("placed_right_anti", B(), P(), "RightAnti", mode="rank")
_case("placed_payload_without_the_key", B(), P(), mode="rank", probe_cols=("p_i64", "p_i32"))
_case("placed_rank_shuffled_build_builds_the_permutation", B(order="shuffled"), P(), mode="rank")
_case("placed_rank_shuffled_build_key_only_right_semi", B(order="shuffled"), P(), "RightSemi", mode="rank", probe_cols=("pk",))
_case("placed_first_row_misses_last_row_hits", B(), P(miss_rows=(0,)), mode="array")
# ---- listed
_case("listed_sparse_emit", B(step=10), P(hit=0.02, step=10), mode="rank")
_case("listed_sparse_emit_switched_off", B(step=10), P(hit=0.02, step=10), mode="rank", options={"join__listed_sparse_den": "0"})
_case("listed_dense_emit", B(step=10), P(hit=0.1, step=10), mode="rank")
_case("listed_dense_emit_array", B(step=10), P(hit=0.1, step=10), mode="array")
_case("listed_guess_dropped_after_the_counts", B(step=10), P(hit=0.6, step=10), mode="rank")
_case("listed_predicate_in_counts", B(), P(), mode="rank", call="predicate", predicate=functools.partial(simple_pred, 20))
_case("listed_predicate_in_counts_switched_off", B(), P(), mode="rank", call="predicate", predicate=functools.partial(simple_pred, 20),
      options={"join__pred_in_counts": "0"})
_case("listed_predicate_of_another_shape", B(), P(), mode="rank", call="predicate", predicate=other_pred)
_case("listed_predicate_in_counts_dropped_words_become_the_mask", B(), P(hit=0.9), mode="rank", call="predicate", predicate=functools.partial(simple_pred, 90))
_case("listed_predicate_right_anti", B(), P(), "RightAnti", mode="array", call="predicate", predicate=functools.partial(simple_pred, 20))
_case("listed_counts_without_nt_loads", B(step=10), P(hit=0.1, step=10), mode="rank", options={"join__counts_nt": "0"})
# ---- shared columns
for _pm in (0, 3, 4):
    _case(f"shared_all_hit_probe_mode_{_pm}", B(), P(hit=1.0, miss_rows=()), mode="rank", probe_mode=_pm, options=SHARE)
_case("shared_all_hit_flat", B(), P(hit=1.0, miss_rows=()), mode="flat", options=SHARE)
_case("shared_right_semi", B(), P(hit=1.0, miss_rows=()), "RightSemi", mode="array", probe_mode=4, options=SHARE)
_case("shared_second_probe_takes_the_remembered_hint", B(), P(hit=1.0, miss_rows=()), mode="rank", options=SHARE, probes=2)
_case("shared_miss_on_a_sampled_word", B(), P(hit=1.0), mode="rank", options=SHARE)
_case("shared_miss_on_an_unsampled_word", B(), P(npr=200_000, hit=1.0, miss_rows=(69,)), mode="rank", options=SHARE)   # every third word is sampled
_case("shared_miss_on_an_unsampled_word_probe_mode_3", B(), P(npr=200_000, hit=1.0, miss_rows=(69,)), mode="rank", probe_mode=3, options=SHARE, ordered=False)
_case("shared_device_flag", B(), P(hit=1.0, miss_rows=()), mode="rank", options={**SHARE, "join__probe_host_flag": "0"})
_case("shared_device_flag_miss_on_an_unsampled_word", B(), P(npr=200_000, hit=1.0, miss_rows=(69,)), mode="rank", options={**SHARE, "join__probe_host_flag": "0"})
# ---- speculated placed
NO_SHARE = {**SHARE, "join__share_probe": "0"}
_case("speculated_placed_all_hit", B(), P(hit=1.0, miss_rows=()), mode="rank", options=NO_SHARE)
_case("speculated_placed_miss_on_an_unsampled_word", B(), P(npr=200_000, hit=1.0, miss_rows=(69,)), mode="rank", options=NO_SHARE)
# ---- single pass
_case("single_pass_look_back", B(), P(), mode="rank", probe_mode=2)
_case("single_pass_unordered_probe_mode_3", B(), P(), mode="rank", probe_mode=3, ordered=False)
_case("single_pass_unordered_probe_mode_4_flat", B(), P(), mode="flat", probe_mode=4, ordered=False)
_case("single_pass_unordered_chained_two_keys", B(extra="two_keys"), P(extra="two_keys"), mode="chained", probe_mode=4, on=TWO, ordered=False)
_case("single_pass_probe_mode_3_not_applicable", B(dup=2), P(), mode="chained", probe_mode=3)
_case("single_pass_narrow_rows_take_counts_and_placed", B(), P(npr=N22, sorted_keys=True), "RightSemi", mode="rank", probe_mode=3, probe_cols=("pk",))
# ---- grouped keys only
_case("grouped_keys_rank_inner", B(), P(npr=N16), build_cols=(), probe_cols=("pk",), mode="rank", probe_mode=4, options=UNCLUSTERED, ordered=False)
_case("grouped_keys_rank_right_semi", B(order="shuffled"), P(npr=N16), "RightSemi", probe_cols=("pk",), mode="rank", probe_mode=4, options=UNCLUSTERED, ordered=False)
_case("grouped_keys_rank_right_anti", B(), P(npr=N16), "RightAnti", probe_cols=("pk",), mode="rank", probe_mode=4, options=UNCLUSTERED, ordered=False)
_case("grouped_keys_array", B(), P(npr=N16), build_cols=(), probe_cols=("pk",), mode="array", probe_mode=4, options=UNCLUSTERED, ordered=False)
_case("grouped_keys_sliced_key_column", B(), P(npr=N16 + 640), build_cols=(), probe_cols=("pk",), mode="array", probe_mode=4, options=UNCLUSTERED, ordered=False,
      probe_slice=(576, N16))
_case("grouped_keys_switched_off", B(), P(npr=N16), build_cols=(), probe_cols=("pk",), mode="rank", probe_mode=4, options={**UNCLUSTERED, "join__grouped_probe": "0"},
      ordered=False)
# ---- returned lookup
_case("returned_every_row_hits", B(), P(npr=N16, hit=1.0, miss_rows=()), mode="rank", options=UNCLUSTERED)
_case("returned_misses_probe_mode_0", B(), P(npr=N16), mode="rank", build_cols=("b_i32", "b_dec", "b_u8"), options=UNCLUSTERED)
_case("returned_misses_probe_mode_4", B(), P(npr=N16), mode="rank", probe_mode=4, options=UNCLUSTERED, ordered=False)
_case("returned_shuffled_build_packed_records", B(order="shuffled"), P(npr=N16), mode="rank", build_cols=("b_i32", "b_i64"), options=UNCLUSTERED)
_case("returned_shuffled_build_payload_by_column", B(order="shuffled"), P(npr=N16), mode="rank", build_cols=("b_dec", "b_i64"), options=UNCLUSTERED)
_case("returned_with_a_row_mask", B(), P(npr=N16), mode="rank", call="predicate", predicate=functools.partial(simple_pred, 50), options=UNCLUSTERED)
_case("returned_right_anti", B(), P(npr=N16), "RightAnti", mode="rank", options=UNCLUSTERED)
_case("returned_lookup_declines_wide_records", B(extra="wide"), P(npr=N16), mode="rank", build_cols=("b_dec", "b_dec0", "b_dec1", "b_dec2", "b_i32"), options=UNCLUSTERED)
# ---- first match
_case("first_match_nullable_payload_right_semi", B(), P(extra="nullable"), "RightSemi", mode="rank", probe_cols=("pk", "p_n"))
_case("first_match_nullable_payload_right_anti", B(), P(extra="nullable"), "RightAnti", mode="rank", probe_cols=("pk", "p_n"))
_case("first_match_utf8_payload_inner_takes_the_pairs", B(extra="utf8"), P(), mode="rank", build_cols=("b_s",))
_case("first_match_left_semi_unique_keys", B(), P(), "LeftSemi", mode="rank", ordered=False)
_case("first_match_left_anti_unique_keys", B(), P(), "LeftAnti", mode="rank", ordered=False)
_case("first_match_left_mark_unique_keys", B(), P(), "LeftMark", mode="rank", ordered=False)
_case("first_match_inner_13_columns_materialise", B(extra="many"), P(), mode="rank", build_cols=tuple(f"m{i}" for i in range(13)))
# (more than MAX_JOIN_COLS columns leave the first-match route for the pairs: only an Inner probe WITHOUT output columns takes lookup -> scan)
_case("first_match_inner_no_output_columns", B(), P(), mode="rank", build_cols=(), probe_cols=())
_case("first_match_right_semi_row_mask", B(), P(extra="nullable"), "RightSemi", mode="rank", probe_cols=("pk", "p_n"), call="predicate",
      predicate=functools.partial(simple_pred, 50))
_case("first_match_left_semi_row_mask_not_consumed", B(), P(), "LeftSemi", mode="rank", call="predicate", predicate=functools.partial(simple_pred, 50), ordered=False)
_case("first_match_inner_13_columns_row_mask", B(extra="many"), P(), mode="rank", build_cols=tuple(f"m{i}" for i in range(13)), call="predicate", predicate=other_pred)
# ---- pairs in one pass
_case("pairs_single_capacity_holds", B(nb=3000, dup=2), P(npr=N16), mode="flat", probe_mode=4, ordered=False)
# (at 2^16 + 65 rows every row is sampled, so the capacity always holds: the case beside it has every second row sampled)
_case("pairs_single_sampled_rows_one_match_others_many", build_by_parity, P(npr=N16, nb=2000, matches_by_parity=8), mode="flat", probe_mode=4, ordered=False)
_case("pairs_single_capacity_does_not_hold", build_by_parity, P(npr=N17, nb=2000, matches_by_parity=8), mode="flat", probe_mode=4, ordered=False)
# ---- general pairs
for _jt in ("Inner", "Left", "Right", "Full", "LeftSemi", "LeftAnti", "RightSemi", "RightAnti", "LeftMark", "RightMark"):
    _case(f"pairs_duplicate_keys_{_jt}", B(dup=3), P(), _jt, ordered=False)
_case("pairs_flat_duplicate_keys", B(dup=3), P(), mode="flat", ordered=False)
_case("pairs_null_keys_equal_nothing", B(dup=3, extra="null_keys"), P(extra="null_keys"), "Full", ordered=False)
_case("pairs_null_keys_equal_null", B(dup=3, extra="null_keys"), P(extra="null_keys"), "Full", ordered=False, null_equality="NullEqualsNull")
_case("pairs_empty_probe", B(dup=3), P(npr=0), "Right", ordered=False)
_case("pairs_empty_build", B(nb=0), P(), "Right", ordered=False)
_case("pairs_empty_probe_unique_keys", B(), P(npr=0), mode="rank")
_case("pairs_predicate_not_consumed", B(dup=3), P(), call="predicate", predicate=functools.partial(simple_pred, 50), ordered=False)
# ---- null-aware anti joins
_case("null_aware_right_anti_build_has_null", B(extra="null_keys"), P(), "RightAnti", null_aware=True, ordered=False)
_case("null_aware_right_anti_masks_null_probe_keys", B(), P(extra="null_keys"), "RightAnti", null_aware=True, probe_cols=("p_i64", "p_i32"), mode="rank")
_case("null_aware_right_anti_masks_null_probe_keys_radix", B(), P(extra="null_keys"), "RightAnti", null_aware=True, probe_cols=("p_i64", "p_i32"), mode="radix", ordered=False)
_case("null_aware_right_anti_proceeds", B(), P(), "RightAnti", null_aware=True, mode="rank")
_case("null_aware_left_anti", B(), P(extra="null_keys"), "LeftAnti", null_aware=True, ordered=False)
# ---- argument errors
_case("error_build_output_column_out_of_range", B(), P(), mode="rank", call="bad_build_col")
_case("error_probe_output_column_out_of_range", B(), P(), mode="rank", call="bad_probe_col")
_case("error_probe_output_column_out_of_range_radix", B(), P(), mode="radix", call="bad_probe_col")

BY_NAME = {c.name: c for c in CASES}
LEFT_TYPES = ("Left", "Full", "LeftSemi", "LeftAnti", "LeftMark")


def expected(case):
    """the oracle's rows of the whole join (the probe's output and, for the join types that have one, the tail of unmatched build rows)"""
    from oracle import oracle
    from tests.util import to_oracle_expr
    b, p = case.build(), case.probe()
    if case.probe_slice:
        p = p.slice(*case.probe_slice)
    if case.predicate is not None:
        p = oracle.filter(p, to_oracle_expr(case.predicate()), p.column_names)
    exp = oracle.hash_join(b, p, case.on, case.join_type, null_equality=case.null_equality, null_aware=case.join["null_aware"])
    mark = ["mark"] if case.join_type in ("LeftMark", "RightMark") else []
    if case.join_type in ("RightSemi", "RightAnti", "RightMark"):
        return exp.select(case.probe_cols + mark)
    if case.join_type in ("LeftSemi", "LeftAnti", "LeftMark"):
        return exp.select(case.build_cols + mark)
    if not case.build_cols + case.probe_cols:   # no column to compare: the row count
        return pa.table({"rows": [exp.num_rows]})
    return exp.select(case.build_cols + case.probe_cols)


def run(case):
    """the case on the GPU -> (the join's rows as Arrow, {profile name: [calls, bytes]} of the last probe, [probe_rows, output_rows]); an error of
    the probe comes back as (None, {"error": message}, None).  Fresh device tables and a fresh join table: no hint on a key buffer is left
    from another case"""
    import ctypes as C

    from datafusion_amd import _lib, ops
    from datafusion_amd.table import DeviceTable
    db, whole = DeviceTable.from_arrow(case.build()), DeviceTable.from_arrow(case.probe())
    dp = whole.slice(*case.probe_slice) if case.probe_slice else whole
    ops.set_options(**case.options)
    ops.profile_enable(True)
    ht = None
    try:
        ht = ops.JoinHashTable(db, [l for l, _ in case.on], case.null_equality, **case.join)
        on_right = [r for _, r in case.on]
        out = None
        try:
            for _ in range(case.probes):
                if out is not None:
                    out.free()
                ops.profile_reset()
                if case.call in ("bad_build_col", "bad_probe_col"):
                    lib, handle = _lib.load(), C.c_void_p()
                    bc, pc = ([99], [0]) if case.call == "bad_build_col" else ([0], [99])
                    _lib.check(lib.dfgpu_join_probe(ht._h, dp.handle, ops._ints([dp.index_of(k) for k in on_right]), ops.JOIN_TYPES[case.join_type], ops._ints(bc), 1,
                                                    ops._ints(pc), 1, C.byref(handle)))
                    raise AssertionError("the probe accepted a column that does not exist")
                out = ht.probe(dp, on_right, case.join_type, case.build_cols, case.probe_cols, predicate=case.predicate() if case.predicate else None)
        except _lib.DfgpuError as e:
            return None, {"error": str(e)}, None
        ops.sync()
        ledger = {k: [v["calls"], v["bytes"]] for k, v in ops.profile_stats().items()}
        info = ht.info()
        counters = [info.probe_rows, info.output_rows]
        if case.join_type in LEFT_TYPES:
            tail = ht.emit_unmatched(case.join_type, case.build_cols, ops.tail_probe_schema(dp, case.join_type, case.probe_cols))
            out = ops.concat_tables([out, tail]) if case.join_type in ("Left", "Full") else tail
        got = out.to_arrow() if out.num_columns else pa.table({"rows": [out.num_rows]})
        out.free()
        return got, ledger, counters
    finally:
        ops.profile_enable(False)
        ops.reset_options()
        if ht is not None:
            ht.free()
        if dp is not whole:
            dp.free()
        whole.free()
        db.free()


def record(case):
    got, ledger, counters = run(case)
    return ledger if got is None else {"profile": dict(sorted(ledger.items())), "info": counters}


if __name__ == "__main__":   # python -m tests.join_route_cases OUT.json: records the ledger of the commit it runs at
    import json
    import sys
    with open(sys.argv[1], "w") as f:
        json.dump({c.name: record(c) for c in CASES}, f, indent=1)
        f.write("\n")

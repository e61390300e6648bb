#!/usr/bin/env python3
"""NestedLoopJoinExec on the device: the band join `l.lo <= r.x AND r.x < l.hi` with about one match per right row (left bands
[10 i, 10 i + 7) in shuffled order, right points uniform over the bands' range: 70 % fall into a band, 30 % into a gap).

Per shape |L| x |R|: Inner (nlj_count + nlj_emit) and RightSemi (nlj_flags, with and without the early exit) — wall ms of the call and,
per launch the library recorded (ops.profile_launches), its ms and the pair evaluations per second that comes to.  With --hash-join
the same join through the only device route there was before: ops.hash_join on a constant key column with the same JoinFilter, which
materialises all |L| x |R| pairs (only shapes whose pairs fit).  Inputs are resident in HBM; one JSON object per line.

  python scripts/bench_nlj.py [--shapes 2048x65536,16384x1048576,1x16777216,16777216x1] [--hash-join 2048x65536] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NLJ_LAUNCHES = ("nlj_flags", "nlj_count", "nlj_emit", "nlj_cartesian")


def tables(nl, nr, with_key=False):
    import numpy as np
    import pyarrow as pa
    rng = np.random.default_rng(nl * 7 + nr)
    lo = rng.permutation(nl).astype(np.int64) * 10
    left = {"lo": pa.array(lo), "hi": pa.array(lo + 7), "tag": pa.array(np.arange(nl, dtype=np.int64))}
    right = {"x": pa.array(rng.integers(0, nl * 10, size=nr).astype(np.int64)), "row": pa.array(np.arange(nr, dtype=np.int64))}
    if with_key:
        left["k"] = pa.array(np.ones(nl, dtype=np.int32))
        right["k"] = pa.array(np.ones(nr, dtype=np.int32))
    return pa.table(left), pa.table(right)


def stats(ms):
    return {"best": round(min(ms), 3), "median": round(sorted(ms)[len(ms) // 2], 3), "worst": round(max(ms), 3)}


def timed(fn, rounds, pairs, ops):
    fn().free()            # warm-up: code objects, the memory pool
    wall, launches, rows = [], {}, 0
    for _ in range(rounds):
        ops.profile_enable(True)
        ops.profile_reset()
        ops.sync()
        t0 = time.perf_counter()
        out = fn()
        ops.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        rows = out.num_rows
        out.free()
        ops.profile_stats()
        launches = {}
        for k in NLJ_LAUNCHES:
            rec = ops.profile_launches(k)
            if rec:
                launches[k] = [{"ms": round(ms, 4), "pair_evaluations_per_s": round(pairs / (ms * 1e-3), 0) if ms > 0 else None} for ms, _ in rec]
        ops.profile_enable(False)
    return {"wall_ms": stats(wall), "output_rows": rows, "launches_last_round": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x65536,16384x1048576,1x16777216,16777216x1")
    ap.add_argument("--hash-join", default="2048x65536")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    _lib.init(0)
    flt = ((col("f0") <= col("f2")).and_(col("f2") < col("f1")), [(0, "Left"), (1, "Left"), (0, "Right")])
    shape = lambda s: tuple(int(v) for v in s.split("x"))
    for nl, nr in [shape(s) for s in args.shapes.split(",") if s]:
        left, right = tables(nl, nr)
        dl, dr = DeviceTable.from_arrow(left), DeviceTable.from_arrow(right)
        legs = [("Inner", "Inner", {}), ("RightSemi", "RightSemi", {}), ("RightSemi, no early exit", "RightSemi", {"nlj__early_exit": 0})]
        for name, jt, options in legs:
            if options:
                ops.set_options(**options)
            res = timed(lambda: ops.nested_loop_join(dl, dr, jt, flt), args.rounds, nl * nr, ops)
            if options:
                ops.set_options(**{k: None for k in options})
            print(json.dumps(dict({"leg": name, "left_rows": nl, "right_rows": nr, "pairs": nl * nr}, **res)), flush=True)
        dl.free()
        dr.free()
    for nl, nr in [shape(s) for s in args.hash_join.split(",") if s]:
        left, right = tables(nl, nr, with_key=True)
        dl, dr = DeviceTable.from_arrow(left), DeviceTable.from_arrow(right)
        lc, rc = ["lo", "hi", "tag"], ["x", "row"]
        for jt in ("Inner", "RightSemi"):
            new = timed(lambda: ops.nested_loop_join(dl, dr, jt, flt, lc, rc), args.rounds, nl * nr, ops)
            old = timed(lambda: ops.hash_join(dl, dr, [("k", "k")], jt, build_cols=lc, probe_cols=rc, join_filter=flt), args.rounds, nl * nr, ops)
            assert new["output_rows"] == old["output_rows"], (new["output_rows"], old["output_rows"])
            print(json.dumps({"leg": f"{jt}: nested loop join against the constant-key hash join", "left_rows": nl, "right_rows": nr, "pairs": nl * nr,
                              "nested_loop_join": new, "constant_key_hash_join": old,
                              "hash_join_ms_over_nested_loop_ms": round(old["wall_ms"]["median"] / new["wall_ms"]["median"], 2)}), flush=True)
        dl.free()
        dr.free()


if __name__ == "__main__":
    main()

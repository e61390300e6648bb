#!/usr/bin/env python3
"""The range join on the device against the nested-loop join, in one process: the band join `l.lo <= r.x AND r.x < l.hi` of
scripts/bench_nlj.py (the same tables(): left bands [10 i, 10 i + 7) in shuffled order, right points uniform over the bands' range,
about 0.7 matches per right row).

Per shape |L| x |R|: Inner and RightSemi through ops.range_join and through ops.nested_loop_join — wall ms of the call and, per
launch the library recorded (ops.profile_launches), its ms — and a check that the two results are equal as multisets (the pair order
differs by contract).  Then one single-inequality shape whose output is large, `l.lo <= r.x` (about half the pair space), with row-id
sized output columns: the expand kernel's rate in output bytes per second, to set against the copy ceiling of profiles/.  There only
the range join runs, and the check is the row count against the count of pairs computed on the host.  Inputs are resident in HBM;
one JSON object per line.

  python scripts/bench_range_join.py [--shapes 2048x65536,16384x1048576,1x16777216,16777216x1] [--lower-only 4096x65536] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_nlj import stats, tables  # noqa: E402

LAUNCHES = ("rangejoin_keys", "rangejoin_bounds", "rangejoin_cover", "rangejoin_expand", "nlj_flags", "nlj_count", "nlj_emit", "nlj_cartesian")


def timed(fn, rounds, ops, keep=False):
    """-> (wall ms statistics, launches of the last round, output rows, the last output when `keep`)"""
    fn().free()            # warm-up: code objects, the memory pool, the key column's cached statistics
    wall, launches, rows, out = [], {}, 0, None
    for i in range(rounds):
        ops.profile_enable(True)
        ops.profile_reset()
        ops.sync()
        t0 = time.perf_counter()
        out = fn()
        ops.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
        rows = out.num_rows
        if not (keep and i == rounds - 1):
            out.free()
            out = None
        ops.profile_stats()
        launches = {}
        for k in LAUNCHES:
            rec = ops.profile_launches(k)
            if rec:
                launches[k] = [round(ms, 4) for ms, _ in rec]
        ops.profile_enable(False)
    return {"wall_ms": stats(wall), "output_rows": rows, "launch_ms_last_round": launches}, out


def same_multiset(a, b):
    """two device tables hold the same rows: sorted by every column on the host, then compared"""
    import pyarrow.compute as pc
    ta, tb = a.to_arrow(), b.to_arrow()
    if ta.column_names != tb.column_names or ta.num_rows != tb.num_rows:
        return False
    keys = [(n, "ascending") for n in ta.column_names]
    if not keys:
        return True
    ta, tb = ta.take(pc.sort_indices(ta, sort_keys=keys)), tb.take(pc.sort_indices(tb, sort_keys=keys))
    return ta.equals(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x65536,16384x1048576,1x16777216,16777216x1")
    ap.add_argument("--lower-only", default="4096x65536")
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
        for jt in ("Inner", "RightSemi"):
            rj, a = timed(lambda: ops.range_join(dl, dr, "x", ("lo", True), ("hi", False), jt), args.rounds, ops, keep=True)
            nlj, b = timed(lambda: ops.nested_loop_join(dl, dr, jt, flt), args.rounds, ops, keep=True)
            equal = same_multiset(a, b)
            a.free()
            b.free()
            print(json.dumps({"leg": jt, "left_rows": nl, "right_rows": nr, "pairs": nl * nr, "range_join": rj, "nested_loop_join": nlj,
                              "equal_as_multisets": equal,
                              "nested_loop_ms_over_range_join_ms": round(nlj["wall_ms"]["median"] / rj["wall_ms"]["median"], 2)}), flush=True)
            assert equal, (jt, nl, nr)
        dl.free()
        dr.free()
    for nl, nr in [shape(s) for s in args.lower_only.split(",") if s]:
        import numpy as np
        left, right = tables(nl, nr)
        want = int(np.searchsorted(np.sort(left.column("lo").to_numpy()), right.column("x").to_numpy(), side="right").sum())   # pairs with lo <= x
        dl, dr = DeviceTable.from_arrow(left), DeviceTable.from_arrow(right)
        rj, _ = timed(lambda: ops.range_join(dl, dr, "x", ("lo", True), None, "Inner", ["tag"], ["row"]), args.rounds, ops)
        ms = rj["launch_ms_last_round"].get("rangejoin_expand", [None])[0]
        print(json.dumps({"leg": "Inner, lo <= x only, output columns tag and row", "left_rows": nl, "right_rows": nr, "pairs": nl * nr, "range_join": rj,
                          "row_count_as_computed_on_the_host": rj["output_rows"] == want,
                          "expand_output_bytes": rj["output_rows"] * 16,
                          "expand_output_bytes_per_s": round(rj["output_rows"] * 16 / (ms * 1e-3), 0) if ms else None}), flush=True)
        assert rj["output_rows"] == want, (rj["output_rows"], want)
        dl.free()
        dr.free()


if __name__ == "__main__":
    main()

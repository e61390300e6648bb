#!/usr/bin/env python3
"""bit_or beside MAX and bit_xor beside SUM(Int64) over the GROUP BY shapes of scripts/bench_ops.py: the new kinds move the bytes of
the kinds beside them, so each pair should take the same time.  The four legs of a shape run in turn, `--rounds` times over, in one
process (inputs resident in HBM, the stream drained on both sides of the timed region); per leg the best, the median and the worst wall
time and the kernels the library recorded.  One JSON object per line on stdout.

  python scripts/bench_bitwise.py [--sf 100] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    _lib.init(0)
    li = ops.tpch_lineitem(args.sf)
    orders = ops.tpch_orders(args.sf)
    shapes = [
        ("GROUP BY l_orderkey", li.select(["l_orderkey"]), ["l_orderkey"], "l_orderkey"),
        ("GROUP BY o_custkey", orders.select(["o_custkey", "o_orderkey"]), ["o_custkey"], "o_orderkey"),
        ("GROUP BY l_returnflag, l_linestatus, l_shipdate", li.select(["l_returnflag", "l_linestatus", "l_shipdate", "l_orderkey"]),
         ["l_returnflag", "l_linestatus", "l_shipdate"], "l_orderkey"),
        ("GROUP BY l_returnflag, l_linestatus", li.select(["l_returnflag", "l_linestatus", "l_orderkey"]), ["l_returnflag", "l_linestatus"], "l_orderkey"),
    ]
    for name, t, keys, arg in shapes:
        gb = [(col(k), k) for k in keys]
        legs = ["max", "bit_or", "sum", "bit_xor"]
        times = {f: [] for f in legs}
        kernels = {}
        groups = 0
        for f in legs:      # warm-up: code objects, the memory pool, the key columns' cached statistics
            o = ops.aggregate(t, gb, [(f, col(arg), "v")], "Single")
            groups = o.num_rows
            o.free()
        for _ in range(args.rounds):
            for f in legs:
                ops.profile_enable(True)
                ops.profile_reset()
                ops.sync()
                t0 = time.perf_counter()
                o = ops.aggregate(t, gb, [(f, col(arg), "v")], "Single")
                ops.sync()
                times[f].append(time.perf_counter() - t0)
                o.free()
                kernels[f] = {k: round(v["total_ms"], 3) for k, v in sorted(ops.profile_stats().items(), key=lambda kv: -kv[1]["total_ms"])[:4]}
                ops.profile_enable(False)
        print(json.dumps({"shape": f"{name} SF{args.sf:g}", "rows": t.num_rows, "groups": groups, "argument": arg,
                          "ms": {f: {"best": round(min(v) * 1e3, 3), "median": round(sorted(v)[len(v) // 2] * 1e3, 3), "worst": round(max(v) * 1e3, 3)}
                                 for f, v in times.items()},
                          "kernels_ms_last_round": kernels}), flush=True)
        t.free()
    li.free()
    orders.free()


if __name__ == "__main__":
    main()

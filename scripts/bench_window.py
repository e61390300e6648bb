#!/usr/bin/env python3
"""WindowAggExec over TPC-H `orders` sorted by (o_custkey, o_orderdate): row_number + rank, a running sum(o_totalprice) over the
default RANGE frame, sum over the whole partition, and the functions that take positions from the bitmap words (ntile + percent_rank +
cume_dist; first_value + last_value over the default frame; nth_value(2) over the ROWS frame) — each beside the SortExec below it, from
the same run.  Per `window_` launch the
library recorded (ops.profile_launches): its ms, its algorithmic bytes, and the fraction of the measured copy ceiling (6.29 TB/s, the
ceiling bench.py and the profiles use) those bytes per that time come to.  Inputs are resident in HBM; one JSON object per line.
The device generator of `orders` makes no o_totalprice: the column here is CAST(o_orderkey AS Decimal128(15, 2)) — the type and the
width of the real one (what a bandwidth-bound scan is timed by), not its values.

  python scripts/bench_window.py [--sf 100] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_CEILING_GBS = 6290.0   # bench.py: the measured float4 copy ceiling of the MI355X
WINDOW_LAUNCHES = ("window_heads", "window_peer_popcount", "window_starts", "window_ends", "window_rank", "window_dense_rank", "window_scan_add_u64",
                   "window_scan_add_i128", "window_scan_add_f64", "window_scan_count", "window_scan_min_i64", "window_scan_max_i64", "window_scan_min_i128",
                   "window_scan_max_i128", "window_finish", "window_pick", "window_word_starts", "window_word_ends", "window_dist", "window_value")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    from datafusion_amd import _lib, ops
    import pyarrow as pa

    from datafusion_amd.expr import CastExpr, col
    _lib.init(0)
    orders = ops.tpch_orders(args.sf)
    src = ops.project(orders, [(col("o_custkey"), "o_custkey"), (col("o_orderdate"), "o_orderdate"),
                               (CastExpr(col("o_orderkey"), pa.decimal128(15, 2)), "o_totalprice")])
    keys = [("o_custkey", False, False), ("o_orderdate", False, False)]
    ops.sync()
    sort_ms = []
    for r in range(args.rounds + 1):          # (the first is the warm-up: code objects, the memory pool, cached statistics)
        ops.sync()
        t0 = time.perf_counter()
        sorted_t = ops.sort(src, keys)
        ops.sync()
        sort_ms.append((time.perf_counter() - t0) * 1e3)
        if r < args.rounds:
            sorted_t.free()
    sort_ms = sort_ms[1:]
    legs = [
        ("row_number + rank", [("row_number", None, "rn", None), ("rank", None, "rk", None)]),
        ("sum(o_totalprice) range_to_current", [("sum", col("o_totalprice"), "running", "range_to_current")]),
        ("sum(o_totalprice) partition", [("sum", col("o_totalprice"), "total", "partition")]),
        ("ntile(4) + percent_rank + cume_dist", [(("ntile", 4), None, "q", None), ("percent_rank", None, "pr", None), ("cume_dist", None, "cd", None)]),
        ("first_value + last_value(o_totalprice) range_to_current", [("first_value", col("o_totalprice"), "first", None), ("last_value", col("o_totalprice"), "last", None)]),
        ("nth_value(o_totalprice, 2) rows_to_current", [(("nth_value", 2), col("o_totalprice"), "second", "rows_to_current")]),
    ]
    for name, exprs in legs:
        ops.window(sorted_t, ["o_custkey"], ["o_orderdate"], exprs).free()     # warm-up
        wall, launches = [], {}
        for _ in range(args.rounds):
            ops.profile_enable(True)
            ops.profile_reset()
            ops.sync()
            t0 = time.perf_counter()
            out = ops.window(sorted_t, ["o_custkey"], ["o_orderdate"], exprs)
            ops.sync()
            wall.append((time.perf_counter() - t0) * 1e3)
            out.free()
            ops.profile_stats()           # collects the recorded launches
            launches = {}
            for k in WINDOW_LAUNCHES:
                rec = ops.profile_launches(k)
                if rec:
                    launches[k] = [{"ms": round(ms, 4), "algorithmic_bytes": nb,
                                    "frac_vs_copy_ceiling": round(nb / (ms * 1e-3) / 1e9 / HBM_COPY_CEILING_GBS, 4) if ms > 0 else None} for ms, nb in rec]
            ops.profile_enable(False)
        print(json.dumps({"leg": name, "sf": args.sf, "rows": sorted_t.num_rows,
                          "window_ms": {"best": round(min(wall), 3), "median": round(sorted(wall)[len(wall) // 2], 3), "worst": round(max(wall), 3)},
                          "sort_below_ms": {"best": round(min(sort_ms), 3), "median": round(sorted(sort_ms)[len(sort_ms) // 2], 3), "worst": round(max(sort_ms), 3)},
                          "launches_last_round": launches}), flush=True)
    sorted_t.free()
    src.free()
    orders.free()


if __name__ == "__main__":
    main()

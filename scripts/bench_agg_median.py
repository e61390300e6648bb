#!/usr/bin/env python3
"""MEDIAN(v) through the GPU AggregateExec's row store (ABI 22), beside the two things that bound it, in the same process on the same
tables:

  median   `MEDIAN(v) GROUP BY k`, one Single node: append the rows, then at emit count, sort by (group, value), pick
  min      the same node with MIN in place of MEDIAN: what the node costs without the store and the emit
  sort     ops.sort of the two-column table (k, v) by (k, v): the work an exact median cannot go below with this design

Shapes, 16 M rows unless --rows says otherwise:

  g8, g10k, g1m   Float64 v at 8, 10 000 (the H2O group-by question 6 shape) and 1 M groups
  dec             Decimal128(21, 2) v at 10 000 groups
  q6              `MEDIAN(v), STDDEV(v) GROUP BY k1, k2` at 100 x 100 groups, beside the same node with MIN and STDDEV

Tables are generated from a seed, live in HBM before anything is timed, and every timed call ends in a device synchronise.  Per shape:
`--warmup` untimed runs of every route, then `--steps` timed ones with the routes ALTERNATING (profile off: wall milliseconds, min and
median), then `--steps` more per route with the library's profile on for the per-kernel event times and the algorithmic bytes the
kernels declare.  One JSON object per line; `--md FILE` also writes the figures as the tables of profiles/agg_median.md.

  python scripts/bench_agg_median.py [--rows 16000000] [--steps 7] [--warmup 2] [--shapes g8,g10k,g1m,dec,q6] [--md profiles/agg_median.md]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"g8": "Float64, 8 groups", "g10k": "Float64, 10 000 groups (H2O q6's)", "g1m": "Float64, 1 M groups", "dec": "Decimal128(21, 2), 10 000 groups",
          "q6": "median(v), stddev(v) GROUP BY k1, k2 (100 x 100)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--md", default=None, help="write the figures as a Markdown report to this file")
    ap.add_argument("--root", default=ROOT, help="the tree whose datafusion_amd package is measured")
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import numpy as np
    import pyarrow as pa

    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import col
    from datafusion_amd.table import DeviceTable
    _lib.init(0)
    n = args.rows
    rng = np.random.default_rng(22)

    def table(shape):
        if shape == "q6":
            return pa.table({"k1": pa.array(rng.integers(0, 100, n).astype(np.int32)), "k2": pa.array(rng.integers(0, 100, n).astype(np.int32)),
                             "v": pa.array(rng.random(n) * 100.0)})
        groups = {"g8": 8, "g10k": 10_000, "g1m": 1_000_000, "dec": 10_000}[shape]
        k = pa.array(rng.integers(0, groups, n).astype(np.int64))
        if shape == "dec":
            return pa.table({"k": k, "v": pa.array(rng.integers(-10**9, 10**9, n).astype(np.int64)).cast(pa.decimal128(21, 2))})
        return pa.table({"k": k, "v": pa.array(rng.random(n) * 100.0)})

    def timed(fn):
        ops.sync()
        t0 = time.perf_counter()
        out = fn()
        ops.sync()
        ms = (time.perf_counter() - t0) * 1e3
        out.free()
        return ms

    def profiled(fn):
        ops.sync()
        ops.profile_enable(True)
        ops.profile_reset()
        for _ in range(args.steps):
            fn().free()
        ops.sync()
        stats = ops.profile_stats()
        ops.profile_enable(False)
        return {k: {"ms": round(v["total_ms"] / args.steps, 4), "bytes": v["bytes"] // args.steps, "calls": v["calls"] // args.steps}
                for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])}

    results = []
    for shape in [s for s in args.shapes.split(",") if s]:
        t = DeviceTable.from_arrow(table(shape))
        keys = ["k1", "k2"] if shape == "q6" else ["k"]
        gk = [(col(k), k) for k in keys]
        extra = [("stddev", col("v"), "sd")] if shape == "q6" else []
        routes = {"median": lambda: ops.aggregate(t, gk, [("median", col("v"), "m")] + extra, "Single"),
                  "min": lambda: ops.aggregate(t, gk, [("min", col("v"), "m")] + extra, "Single"),
                  "sort": lambda: ops.sort(t, [(k, False, False) for k in keys] + [("v", False, False)])}
        # the median of every group from the sorted table, on the host: the node's answer is checked before anything is timed
        got = routes["median"]().to_arrow().sort_by([(k, "ascending") for k in keys])
        s = routes["sort"]().to_arrow()
        kcols = [s.column(k).to_numpy() for k in keys]
        vc = s.column("v").combine_chunks()
        # (Decimal128: the unscaled low words; the values are small, and so is every sum of two)
        v = np.frombuffer(vc.buffers()[1], np.int64, 2 * (n + vc.offset))[2 * vc.offset::2] if shape == "dec" else vc.to_numpy(zero_copy_only=False)
        start = np.flatnonzero(np.concatenate([[True], np.any([c[1:] != c[:-1] for c in kcols], axis=0)]))
        count = np.diff(np.concatenate([start, [n]]))
        lo, hi = v[start + (count - 1) // 2], v[start + count // 2]
        if shape == "dec":
            want = [a if c % 2 else int((a + b) / 2) for a, b, c in zip(lo.tolist(), hi.tolist(), count.tolist())]       # (int(): toward zero)
            mine = [int(x.scaleb(2)) for x in got.column("m").to_pylist()]
        else:
            want = [a if c % 2 else (a + b) / 2 for a, b, c in zip(lo.tolist(), hi.tolist(), count.tolist())]
            mine = got.column("m").to_pylist()
        assert got.num_rows == len(start) and mine == want, f"{shape}: the node's medians differ from those of the sorted table"
        for fn in routes.values():
            for _ in range(args.warmup):
                fn().free()
        times = {r: [] for r in routes}
        for _ in range(args.steps):                      # the routes alternate inside the timed window
            for r, fn in routes.items():
                times[r].append(timed(fn))
        for r, fn in routes.items():
            ts = sorted(times[r])
            results.append({"shape": shape, "route": r, "rows": n, "groups": got.num_rows, "ms_min": round(ts[0], 3), "ms_median": round(ts[len(ts) // 2], 3),
                            "ms_steps": [round(x, 3) for x in times[r]], "kernels": profiled(fn)})
            print(json.dumps(results[-1]), flush=True)
        t.free()
    if args.md:
        write_md(args, results)


def write_md(args, results):
    by = {(r["shape"], r["route"]): r for r in results}
    shapes = [s for s in SHAPES if (s, "median") in by]
    out = ["# MEDIAN through the node's row store, beside MIN and a sort of (k, v) (ABI 22)", "",
           f"Written by `python scripts/bench_agg_median.py --rows {args.rows} --steps {args.steps} --warmup {args.warmup} --md ...` on one MI355X, one process.",
           f"{args.rows / 1e6:g} M rows resident in HBM, generated from a seed.  Per shape the three routes were warmed up {args.warmup} times, then timed {args.steps} times",
           "ALTERNATING, every call ending in a device synchronise, profile off: the wall figures (min / median).  Then the same number of calls per",
           "route with the library's profile on: per-kernel event times and the algorithmic bytes the kernels declare.  The node's medians were",
           "compared with those read off the sorted table (equal) before anything was timed.  One call on one machine; machines of a pool differ by a few percent.", "",
           "* **median**: `MEDIAN(v) GROUP BY k`, one Single node (DESIGN §4.2.2).",
           "* **min**: the same node with `MIN(v)`: what the node costs without the store and the emit.",
           "* **sort**: `ops.sort` of the table by (k, v): the work an exact median cannot go below with this design.", "",
           "| shape | groups | median, ms | min, ms | sort, ms | median - (min + sort), ms |", "|---|---|---|---|---|---|"]
    for s in shapes:
        m, a, b = (by[(s, r)] for r in ("median", "min", "sort"))
        out.append(f"| {s}: {SHAPES[s]} | {m['groups']:,} | {m['ms_min']:.2f} / {m['ms_median']:.2f} | {a['ms_min']:.2f} / {a['ms_median']:.2f} | "
                   f"{b['ms_min']:.2f} / {b['ms_median']:.2f} | {m['ms_median'] - a['ms_median'] - b['ms_median']:+.2f} |")
    out += ["", "## Per kernel (event time per call, declared bytes, bytes / time; kernels below 0.05 ms left out)", "", "| shape, route | kernel | calls | ms | bytes | GB/s |", "|---|---|---|---|---|---|"]
    for s in shapes:
        for r in ("median", "min", "sort"):
            first = True
            for k, v in by[(s, r)]["kernels"].items():
                if v["ms"] < 0.05:
                    continue
                out.append(f"| {s + ', ' + r if first else ''} | {k} | {v['calls']} | {v['ms']:.2f} | {v['bytes'] / 1e6:.1f} M | {v['bytes'] / v['ms'] / 1e6:.0f} |")
                first = False
    text = "\n".join(out) + "\n"
    if os.path.exists(args.md):                          # what was written by hand below the marker stays
        old = open(args.md).read()
        mark = "\n## Reading the figures\n"
        if mark in old:
            text += old[old.index(mark):]
    with open(args.md, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

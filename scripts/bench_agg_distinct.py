#!/usr/bin/env python3
"""COUNT(DISTINCT x) through the GPU AggregateExec's set (ABI 21) against the only device route there was before it, the two-level
spelling through the same node — GROUP BY (k, x) with aggr=[], then COUNT(x) GROUP BY k — on the same tables, results compared:

  few_groups    8 groups x many values          (COUNT(DISTINCT o_custkey)-like per a handful of keys)
  many_groups   rows / 16 groups x 16 values
  all_distinct  1 024 groups, every row another value
  mixed         SUM(a), AVG(w), COUNT(DISTINCT u) GROUP BY r in ONE node (100 groups, 100 000 values).  Before ABI 21 such a node was
                declined and ran on the CPU; here it is timed beside the same node without its DISTINCT aggregate and beside the
                two-level route for the DISTINCT aggregate alone.

Tables are generated from a seed, live in HBM before anything is timed, and every timed call ends in a device synchronise.  Per shape
and route: `--warmup` untimed runs, then `--steps` timed ones with the two routes ALTERNATING (profile off: wall milliseconds, min and
median), then `--steps` more with the library's profile on for the per-kernel event times and the algorithmic bytes its kernels
declare.  One JSON object per line.

  python scripts/bench_agg_distinct.py [--rows 16000000] [--steps 7] [--warmup 2] [--shapes few_groups,many_groups,all_distinct,mixed]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="few_groups,many_groups,all_distinct,mixed")
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
    rng = np.random.default_rng(21)

    def table(shape):
        if shape == "few_groups":
            return {"k": rng.integers(0, 8, n).astype(np.int64), "x": rng.integers(0, max(1, n // 4), n).astype(np.int64)}
        if shape == "many_groups":
            return {"k": rng.integers(0, max(1, n // 16), n).astype(np.int64), "x": rng.integers(0, 16, n).astype(np.int64)}
        if shape == "all_distinct":
            return {"k": (np.arange(n, dtype=np.int64) * 7) % 1024, "x": rng.permutation(n).astype(np.int64)}
        return {"k": rng.integers(0, 100, n).astype(np.int32), "a": rng.integers(-1000, 1000, n).astype(np.int64), "w": rng.random(n), "x": rng.integers(0, 100_000, n).astype(np.int64)}

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

    for shape in [s for s in args.shapes.split(",") if s]:
        host = table(shape)
        t = DeviceTable.from_arrow(pa.table({c: pa.array(v) for c, v in host.items()}))
        gk = [(col("k"), "k")]

        def distinct():
            return ops.aggregate(t, gk, [("count_distinct", col("x"), "c")], "Single")

        def two_level():
            inner = ops.aggregate(t, gk + [(col("x"), "x")], [], "Single")
            try:
                return ops.aggregate(inner, gk, [("count", col("x"), "c")], "Single")
            finally:
                inner.free()

        routes = {"distinct": distinct, "two_level": two_level}
        if shape == "mixed":
            plain = [("sum", col("a"), "s"), ("avg", col("w"), "m")]
            routes["mixed_node"] = lambda: ops.aggregate(t, gk, plain + [("count_distinct", col("x"), "c")], "Single")
            routes["mixed_node_without_distinct"] = lambda: ops.aggregate(t, gk, plain, "Single")
        a, b = (routes[r]().to_arrow().sort_by("k") for r in ("distinct", "two_level"))
        assert a.equals(b), f"{shape}: the set and the two-level spelling differ"
        if shape == "mixed":
            m = routes["mixed_node"]().to_arrow().sort_by("k")
            assert m.column("c").equals(a.column("c")) and m.select(["k", "s"]).equals(routes["mixed_node_without_distinct"]().to_arrow().sort_by("k").select(["k", "s"]))
        groups, pairs = a.num_rows, int(sum(a.column("c").to_pylist()))
        for fn in routes.values():
            for _ in range(args.warmup):
                fn().free()
        times = {r: [] for r in routes}
        for _ in range(args.steps):                      # the routes alternate inside the timed window
            for r, fn in routes.items():
                times[r].append(timed(fn))
        for r, fn in routes.items():
            ts = sorted(times[r])
            print(json.dumps({"shape": shape, "route": r, "rows": n, "groups": groups, "distinct_pairs": pairs, "ms_min": round(ts[0], 3), "ms_median": round(ts[len(ts) // 2], 3),
                              "ms_steps": [round(x, 3) for x in times[r]], "kernels": profiled(fn)}), flush=True)
        t.free()


if __name__ == "__main__":
    main()

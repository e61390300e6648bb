#!/usr/bin/env python3
"""A Q1-shaped pivot over lineitem, written with per-aggregate FILTER and with the CASE workaround:

    SELECT l_returnflag, l_linestatus,
           SUM(l_extendedprice) FILTER (WHERE p1), COUNT(*) FILTER (WHERE p1),
           SUM(l_extendedprice) FILTER (WHERE p2), COUNT(*) FILTER (WHERE p2)
    FROM lineitem GROUP BY l_returnflag, l_linestatus

  filter form : the four aggregates carry their filter (dfgpu_agg_spec.has_filter / filter)
  case form   : SUM(CASE WHEN p THEN l_extendedprice END), COUNT(CASE WHEN p THEN 1 END) — what a user writes without FILTER

p1 = l_shipdate < DATE '1995-01-01', p2 = l_shipdate >= DATE '1997-01-01': two distinct predicates over one 4-byte column (the
lineitem generator of the library has no l_shipmode column; the shape — four aggregates over two predicates — is the pivot's).

Each (form, path) is warmed up and then timed `--steps` times with the input resident in HBM and the stream drained on both sides;
one JSON object per line: min and median milliseconds, every step's time, and the library's per-kernel breakdown with the algorithmic
bytes its kernels declare.  Paths: column (expression fusion off), fused (the tile program: jit = 0), specialised (hiprtc node).
The two forms must give the same table; the script checks that before it times anything.

  python scripts/bench_agg_filter.py [--sf 10] [--steps 7] [--warmup 2] [--forms case,filter] [--paths column,fused,specialised] [--label X]
"""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--forms", default="case,filter")
    ap.add_argument("--paths", default="column,fused,specialised")
    ap.add_argument("--label", default="")
    ap.add_argument("--root", default=ROOT, help="the tree whose datafusion_amd package is measured")
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import pyarrow as pa

    from datafusion_amd import _lib, ops
    from datafusion_amd.expr import case, col, lit
    _lib.init(0)
    lineitem = ops.tpch_lineitem(args.sf)
    rows = lineitem.num_rows
    gb = [(col("l_returnflag"), "l_returnflag"), (col("l_linestatus"), "l_linestatus")]
    p1 = col("l_shipdate") < lit(datetime.date(1995, 1, 1), pa.date32())
    p2 = col("l_shipdate") >= lit(datetime.date(1997, 1, 1), pa.date32())
    price, one = col("l_extendedprice"), lit(1, pa.int64())
    forms = {
        "filter": [("sum", price, "s1", p1), ("count", None, "c1", p1), ("sum", price, "s2", p2), ("count", None, "c2", p2)],
        "case": [("sum", case([(p1, price)]), "s1"), ("count", case([(p1, one)]), "c1"), ("sum", case([(p2, price)]), "s2"), ("count", case([(p2, one)]), "c2")],
    }
    paths = {"column": (False, {}), "fused": (True, {"jit": "0"}), "specialised": (True, {"jit": "1", "jit__strict": "1"})}
    want_forms = [f for f in args.forms.split(",") if f]
    want_paths = [p for p in args.paths.split(",") if p]

    def run(form):
        return ops.aggregate(lineitem, gb, forms[form], "Single")

    if len(want_forms) == 2:
        a, b = (run(f).to_arrow().sort_by([("l_returnflag", "ascending"), ("l_linestatus", "ascending")]) for f in ("filter", "case"))
        assert a.equals(b), "the FILTER form and the CASE form differ"
    for path in want_paths:
        fusion, opts = paths[path]
        ops.set_options(**opts)
        ops.set_fusion(fusion)
        for form in want_forms:
            for _ in range(args.warmup):
                run(form).free()
            ops.sync()
            ops.profile_enable(True)
            ops.profile_reset()
            times = []
            for _ in range(args.steps):
                ops.sync()
                t0 = time.perf_counter()
                out = run(form)
                ops.sync()
                times.append((time.perf_counter() - t0) * 1e3)
                out.free()
            stats = ops.profile_stats()
            ops.profile_enable(False)
            kernels = {k: {"ms": round(v["total_ms"] / args.steps, 3), "bytes": v["bytes"] // args.steps} for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])}
            print(json.dumps({"label": args.label, "form": form, "path": path, "sf": args.sf, "rows": rows, "ms_min": round(min(times), 3),
                              "ms_median": round(sorted(times)[len(times) // 2], 3), "ms_steps": [round(t, 3) for t in times],
                              "kernel_bytes_per_step": sum(k["bytes"] for k in kernels.values()), "kernels": kernels}), flush=True)
        ops.set_fusion(True)
        ops.set_options(**{k: None for k in opts})


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One profiled measurement of a bench.py workload on the GPU box (run through gpurun): writes gpurun_out/<tag>/

  bench.json        the plain bench line (no profiler attached)
  stats/            rocprofv3 --kernel-trace --stats of the same command; the bench line printed INSIDE that process is kept as
                    stats_bench.json, so the HIP-event average of the dominant kernel and rocprofv3's average come from the same launches
  agreement.json    per try: HIP-event avg vs rocprofv3 avg of the dominant kernel; a try whose two averages differ by more than 3 % is
                    repeated (up to 3 tries) — VERDICT r4 "next" 1(a)
  pmc_fetch/ pmc_write/   separate --pmc passes (FETCH_SIZE, WRITE_SIZE), as MI355X_MICROARCH.md prescribes
  clocks.json       rocm-smi clocks / power / temperature before and after every pass

usage: python scripts/profile_run.py <tag> [--skip-pmc] [--skip-plain] -- <bench.py args>
then (in the container): python scripts/summarize_profile.py gpurun_out/<tag> profiles/<tag>"""
import json
import os
import re
import sqlite3
import subprocess
import sys
import time

R = os.environ.get("GRAFT_REPO_ROOT", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)


def smi():
    """what the clocks were: sclk / mclk / power / cap / temperature as rocm-smi reports them (json when it can, text otherwise)"""
    for cmd in (["rocm-smi", "--showclocks", "--showpower", "--showmaxpower", "--showperflevel", "--showtemp", "--json"],
                ["rocm-smi", "--showclocks", "--showpower", "--showperflevel"]):
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=30).stdout
            try:
                return json.loads(out)
            except ValueError:
                if out.strip():
                    return {"text": out[-3000:]}
        except (OSError, subprocess.TimeoutExpired):
            continue
    return None


def last_json_line(text):
    for ln in reversed(text.splitlines()):
        if ln.startswith("{"):
            try:
                return json.loads(ln)
            except ValueError:
                continue
    return None


def short(name):
    return name.replace("void ", "").split("(")[0].replace("dfgpu::", "")


def rocprof_avg_ms(db, line):
    """rocprofv3's average duration of the device kernel behind the bench line's dominant ProfileScope"""
    from bench import DEVICE_KERNEL_OF
    roof = line.get("roofline") or {}
    scope = roof.get("kernel")
    prefix = DEVICE_KERNEL_OF.get(scope)
    if prefix is None:
        return None, None
    con = sqlite3.connect(db)
    rows = [(short(n), c, tot, avg) for n, c, tot, avg in con.execute("select name,total_calls,total_duration,average from top_kernels")]
    con.close()
    cand = [r for r in rows if r[0].startswith(prefix)]
    if scope in ("join_probe_fused", "join_probe_placed"):   # <KIND, KT, W, MODE, KEYREG>: MODE 0 = single pass, 2 = placed by tile offsets
        want = "0" if scope == "join_probe_fused" else "2"
        def mode(n):
            a = [x.strip().replace("(dfgpu::FusedMode)", "") for x in n[n.index("<") + 1:].rstrip(">").split(",")] if "<" in n else []
            return a[3] if len(a) >= 4 else ""
        # ... or k_join_probe_shared (the foreign-key probe that shares its probe columns), recorded under either scope: whichever
        # of the two took the time is the kernel behind the scope
        cand = [r for r in cand if mode(r[0]) == want] + [r for r in rows if r[0].startswith("k_join_probe_shared")]
    if not cand:
        return None, None
    best = max(cand, key=lambda r: r[2])
    # a roofline quoted on "launch k of n in a step" (one kernel over unlike inputs): compare with rocprofv3's average of THAT grid size —
    # launch positions matched to grid sizes by duration order, as scripts/summarize_profile.py does
    m = re.match(r"launch (\d+) of (\d+)", str(roof.get("launch") or ""))
    if m and int(m.group(2)) > 1:
        con = sqlite3.connect(db)
        per = [(g, c, avg) for n, g, c, avg in con.execute("select name, grid_x, count(*), avg(duration) from kernels group by 1, 2")
               if short(n) == best[0] and c > 1]
        con.close()
        per_launch = roof.get("per_launch_avg_ms")
        if len(per) == int(m.group(2)):
            per.sort(key=lambda r: r[2])
            if per_launch and len(per_launch) == len(per):
                order = sorted(range(len(per_launch)), key=lambda i: per_launch[i])
                rank = order.index(int(m.group(1)) - 1)
            else:
                rank = len(per) - 1      # the quoted launch is the dominant (longest) one
            g, c, avg = per[rank]
            return avg / 1e6, f"{best[0]} [grid {g}]"      # the kernels table's durations are nanoseconds
    return best[3] / 1e3, best[0]     # the top_kernels view's durations are microseconds (traffic.json: avg_launch_us_rocprof)


def main():
    tag = sys.argv[1]
    rest = sys.argv[2:]
    flags = rest[:rest.index("--")] if "--" in rest else []
    bargs = rest[rest.index("--") + 1:] if "--" in rest else rest
    out = os.path.join(R, "gpurun_out", tag)
    os.makedirs(out, exist_ok=True)
    clocks = []
    env = dict(os.environ, TMPDIR="/tmp")

    def run(label, cmd, log, timeout):
        before = smi()
        t0 = time.time()
        p = subprocess.run(cmd, capture_output=True, text=True, cwd="/tmp", env=env, timeout=timeout)
        clocks.append({"pass": label, "seconds": round(time.time() - t0, 1), "rc": p.returncode, "before": before, "after": smi()})
        open(os.path.join(out, log), "w").write(p.stdout[-20000:] + "\n--- stderr ---\n" + p.stderr[-6000:])
        return p

    bench = ["python", os.path.join(R, "bench.py")] + bargs
    if "--skip-plain" not in flags:
        p = run("plain", bench, "bench.log", 1500)
        line = last_json_line(p.stdout)
        open(os.path.join(out, "bench.json"), "w").write(json.dumps(line) + "\n")
    tries = []
    for k in range(3):
        d = os.path.join(out, "stats")
        subprocess.run(["rm", "-rf", d])
        p = run(f"kernel_trace_try{k}", ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "trace", "--"] + bench + ["--no-cpu"], "stats.log", 1500)
        line = last_json_line(p.stdout)
        if line is None:
            tries.append({"try": k, "error": "no bench line under rocprofv3", "rc": p.returncode})
            continue
        open(os.path.join(out, "stats_bench.json"), "w").write(json.dumps(line) + "\n")
        if "--skip-plain" in flags:
            open(os.path.join(out, "bench.json"), "w").write(json.dumps(line) + "\n")
        try:
            rp_ms, dev = rocprof_avg_ms(os.path.join(d, "trace_results.db"), line)
        except sqlite3.Error as e:
            tries.append({"try": k, "error": str(e)})
            continue
        hip_ms = (line.get("roofline") or {}).get("avg_launch_ms")
        rel = abs(rp_ms - hip_ms) / hip_ms if rp_ms and hip_ms else None
        tries.append({"try": k, "scope": (line.get("roofline") or {}).get("kernel"), "device_kernel": dev, "hip_event_avg_ms": hip_ms,
                      "rocprof_avg_ms": None if rp_ms is None else round(rp_ms, 4), "relative_difference": None if rel is None else round(rel, 4),
                      "ms_per_step": line.get("ms_per_step"), "agree_within_3pct": rel is not None and rel <= 0.03})
        if rel is None or rel <= 0.03:
            break
    json.dump({"tries": tries}, open(os.path.join(out, "agreement.json"), "w"), indent=1)
    if "--skip-pmc" not in flags:
        short_args = [a for a in bargs]
        for i, a in enumerate(short_args):   # two timed steps are enough for counters
            if a in ("--steps", "--warmup") and i + 1 < len(short_args):
                short_args[i + 1] = "2" if a == "--steps" else "1"
        if "--steps" not in short_args:
            short_args += ["--steps", "2", "--warmup", "1"]
        pb = ["python", os.path.join(R, "bench.py")] + short_args + ["--no-cpu"]
        run("pmc_fetch", ["rocprofv3", "--pmc", "FETCH_SIZE", "-d", os.path.join(out, "pmc_fetch"), "-o", "pmc", "--"] + pb, "pmc_fetch.log", 1500)
        run("pmc_write", ["rocprofv3", "--pmc", "WRITE_SIZE", "-d", os.path.join(out, "pmc_write"), "-o", "pmc", "--"] + pb, "pmc_write.log", 1500)
    json.dump(clocks, open(os.path.join(out, "clocks.json"), "w"), indent=1)
    # keep only what the 64 MiB merge cap allows: the sqlite summaries stay, multi-MB csv traces go
    subprocess.run(f"find {out} -name '*.csv' -size +8M -delete", shell=True)
    print(json.dumps({"tag": tag, "agreement": tries}, indent=1))


if __name__ == "__main__":
    main()

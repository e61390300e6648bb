"""bench.py's contract, on the GPU: every workload prints ONE JSON line that carries the fields the driver parses — metric / value / unit /
n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload — plus the `roofline`
object (dominant kernel, algorithmic bytes per launch over its HIP-event duration, against the 8 TB/s peak) and the `cpu_baseline` object
(the oracle timed on the host's cores, on a bounded sample).  Small scale factors: the line's shape is what is tested, not its numbers (at SF1 the
longest kernel of Q3 is a small one)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("workload, metric", [("join", "tpch_q3_hash_join_rows_per_sec"), ("q1", "tpch_q1_rows_per_sec"), ("q3", "tpch_q3_rows_per_sec")])
def test_bench_line_carries_roofline_and_cpu_baseline(workload, metric):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--sf", "1", "--cpu-sf", "1", "--steps", "3", "--warmup", "1", "--full"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, (k, sorted(line))
    assert line["metric"] == metric and line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["vs_baseline"] is None and line["data"] == "synthetic" and "workload" in line["config"]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and 0 <= r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3, r
    assert "traffic" in r and r["kernel"]
    c = line["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("port", "reference") and c["sample"] and c["unit"] == line["unit"], c
    if workload in ("q1", "q3"):
        # configs 4 / 5: the CPU leg runs the GPU leg's own tables at its scale factor, and its result is the GPU leg's (the oracle as checker)
        assert c["same_workload_as_gpu_leg"] is True and c["result_equals_gpu_leg"] is True and line["speedup_vs_cpu_port"] > 0, c
        assert line["hbm_frac_whole_step"] == pytest.approx(line["kernel_algorithmic_bytes_per_step"] / (line["ms_per_step"] * 1e-3) / 1e9 / 8000.0, rel=1e-2, abs=2e-4)
        assert line["survey_8d_formula"]["bytes_per_step"] > 0
    if workload == "q3":
        assert c["intermediate_rows_equal_gpu_leg"] is True, c


def test_default_line_also_carries_configs_4_and_5():
    """the single-GPU --full line carries BASELINE configs 4 and 5 under `also`, each from its own process after the
    headline's timed region: ms_per_step, roofline, whole-step fraction, the CPU leg on the same tables and the oracle's verdict on the result
    (small scale factors here: the shape of the line, not its numbers)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--sf", "1", "--cpu-sf", "1", "--steps", "3", "--warmup", "1", "--also", "q1:1,q3:1", "--full"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    line = json.loads(lines[0])
    assert line["metric"] == "tpch_q3_hash_join_rows_per_sec" and set(line["also"]) == {"q1", "q3"}
    for w, d in line["also"].items():
        assert "error" not in d, d
        assert d["metric"] == f"tpch_{w}_rows_per_sec" and d["ms_per_step"] > 0 and d["roofline"]["bound"] == "hbm" and 0 < d["hbm_frac_whole_step"] < 1, d
        assert d["cpu_baseline"]["same_workload_as_gpu_leg"] is True and d["cpu_baseline"]["result_equals_gpu_leg"] is True, d["cpu_baseline"]


def test_plain_line_is_the_headline_and_dump_outputs_is_the_join_output(tmp_path):
    """a plain run measures the headline and nothing else (no CPU leg, no ordered_output, no `also`); --dump-outputs writes the last timed
    step's join output as float64 .npy files, under 64 MB, the same files from a second run, and at SF0.1 (every row in the sample) they
    are the oracle's join in canonical order, with the whole output's row count and column sums beside them"""
    import numpy as np
    import pyarrow as pa

    from datafusion_amd import tpch
    from oracle import oracle
    names = ["l_orderkey", "o_orderdate", "o_shippriority", "l_extendedprice", "l_discount"]   # the canonical order: the sampling key first
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--sf", "0.1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
        line = json.loads(lines[0])
        assert line["metric"] == "tpch_q3_hash_join_rows_per_sec" and line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"]
        assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert not {"cpu_baseline", "speedup_vs_cpu_port", "ordered_output", "also"} & set(line), sorted(line)
        files = sorted(os.listdir(d))
        assert files == sorted([f"join_{n}.npy" for n in names] + ["join_totals.npy"]), files
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        dumps.append({f[len("join_"):-len(".npy")]: np.load(d / f) for f in files})
    a, b = dumps
    assert all(a[k].dtype == np.float64 and np.array_equal(a[k], b[k]) for k in a)
    exp = oracle.hash_join(tpch.orders(0.1), tpch.lineitem(0.1), [("o_orderkey", "l_orderkey")], "Inner")

    def unscaled(name):
        c = exp.column(name).combine_chunks()
        if pa.types.is_decimal(c.type):   # the Q3 payload's decimals are positive and below 2^63: the low word is the value
            return np.frombuffer(c.buffers()[1], dtype=np.int64)[2 * c.offset:2 * (c.offset + len(c))].reshape(-1, 2)[:, 0]
        return (c.cast(pa.int32()) if pa.types.is_date32(c.type) else c).to_numpy().astype(np.int64)
    scale = {"l_extendedprice": 100.0, "l_discount": 100.0}
    want = {n: unscaled(n) for n in names}
    order = np.lexsort([want[n] for n in reversed(names)])
    assert line["config"]["output_rows"] == exp.num_rows == len(a["l_orderkey"])
    for n in names:
        assert np.array_equal(a[n], want[n][order].astype(np.float64) / scale.get(n, 1.0)), n
    table_order = ["o_orderdate", "o_shippriority", "l_orderkey", "l_extendedprice", "l_discount"]   # build columns, then probe columns
    assert a["totals"].tolist() == [float(exp.num_rows)] + [float(int(want[n].sum())) / scale.get(n, 1.0) for n in table_order]

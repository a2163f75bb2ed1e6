"""bench.py's output contract, on a small batch: one JSON line on stdout with every field the
driver and the judge read (metric and unit from BASELINE.json, value = problems / wall time,
roofline with achieved / peak / frac / traffic, cpu_baseline with value / unit / cores /
kind / sample, numa records), and a value consistent with its own ms_per_step."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_line_contract():
    n, steps, warm = 200_000, 10, 2
    r = subprocess.run([sys.executable, "bench.py", "--problems-per-gpu", str(n), "--steps", str(steps),
                        "--warmup", str(warm), "--full", "--no-extras"],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"]
    for k in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline",
              "launch_stats", "baseline_configs"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warm
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and "workload" in d["config"]
    # value = problems x steps / wall, i.e. n / ms_per_step
    assert abs(d["value"] - n / d["ms_per_step"] / 1e3) / d["value"] < 0.01
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert rf["algorithmic_bytes_per_launch"] == n * 100
    assert rf["traffic"] is None  # the committed PMC figure is for the 10 M launch only
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "reference" and cb["cores"] >= 1 and cb["all_core_output_bit_exact"]
    assert d["numa"]["per_rank"][0]["rank"] == 0


def test_plain_run_is_headline_only_and_dumps_last_step(pkg, dev, tmp_path):
    """Without --full the line is the headline alone (none of the sections that take runs of
    their own), and --dump-outputs writes the last timed step's H: float32, the fixed seeded
    sample of rows (the batch is past DUMP_MAX_BYTES), bit for bit what pkg.solve gives on the
    same inputs."""
    import numpy as np
    import torch

    import bench
    n, steps, warm = 1_500_000, 3, 1
    assert n * 36 > bench.DUMP_MAX_BYTES
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--problems-per-gpu", str(n),
                        "--steps", str(steps), "--warmup", str(warm), "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "M homographies/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["steps"] == steps
    assert abs(d["value"] - n / d["ms_per_step"] / 1e3) / d["value"] < 0.01
    for k in ("launch_stats", "reference_statistic", "sks", "ge_baseline", "tensor_aca_rect",
              "ransac", "host_boundary", "cpu_baseline", "baseline_configs", "extras_error"):
        assert k not in d, k
    assert sorted(os.listdir(tmp_path)) == ["H.npy"]
    got = np.load(tmp_path / "H.npy")
    rows = bench.dump_rows(n, 36)
    assert got.dtype == np.float32 and got.shape == (len(rows), 9) and got.nbytes <= 64 << 20
    assert d["dumped_outputs"]["shape"] == [len(rows), 9]
    assert np.array_equal(rows, bench.dump_rows(n, 36)) and np.all(np.diff(rows) > 0)
    src, tar = bench.rank_block_inputs(pkg, dev, n, n, 0)
    want = pkg.solve("aca", src, tar, normalize=True)[torch.from_numpy(rows).to(dev)].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("algo,layout,dtype,bpp", [("sks", "aos", "f32", 100), ("gpt", "soa", "f64", 200)])
def test_bench_headline_selection(algo, layout, dtype, bpp):
    """--algo / --layout / --dtype / --seed pick the headline (SURVEY 5's bench flags): the
    line names the workload, its dtype, layout and algorithmic bytes, and the value still
    follows from its own ms_per_step."""
    n, steps = 100_000, 5
    r = subprocess.run([sys.executable, "bench.py", "--problems-per-gpu", str(n), "--steps", str(steps),
                        "--warmup", "2", "--no-extras", "--no-cpu", "--algo", algo, "--layout", layout,
                        "--dtype", dtype, "--seed", "3"],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert d["dtype"] == dtype and d["config"]["algo"] == algo and d["config"]["layout"] == layout
    assert algo.upper() in d["config"]["workload"] and "seed 3" in d["data"]
    assert d["roofline"]["algorithmic_bytes_per_launch"] == n * bpp
    assert abs(d["value"] - n / d["ms_per_step"] / 1e3) / d["value"] < 0.01

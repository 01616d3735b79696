"""bench.py's plain run and --dump-outputs: the plain line carries the contract and none of the --full legs, --steps is
the number of timed steps, and the dumped arrays are what the timed step computed (the same under eager launches and
under HIP-graph replay) within the 64 MB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_budget_and_fixed_sample():
    import bench
    g = torch.Generator().manual_seed(3)
    got = {"big": torch.randn(3_000_000, generator=g), "small": torch.randn(2, 3, 4, generator=g),
           "scalar": torch.tensor(1.5)}
    limit = 4 * 2 ** 20
    a, b = bench.dump_outputs(got, limit_bytes=limit), bench.dump_outputs(dict(got), limit_bytes=limit)
    assert set(a) == set(got)
    assert sum(x.nbytes + 128 for x in a.values()) <= limit
    assert a["small"].shape == (2, 3, 4) and np.array_equal(a["small"], got["small"].numpy())
    assert a["scalar"].shape == () and float(a["scalar"]) == 1.5
    assert a["big"].dtype == np.float32 and 0 < a["big"].size < got["big"].numel()
    assert np.array_equal(a["big"], b["big"])                                      # the same positions every time
    assert np.isin(a["big"], got["big"].numpy()).all()


def _bench(tmp_path, tag, *extra):
    out_dir = tmp_path / tag
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "2", "--batch", "2", "--height", "64",
           "--width", "128", "--planes", "9", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    arrays = {f[:-4]: np.load(str(out_dir / f)) for f in os.listdir(str(out_dir)) if f.endswith(".npy")}
    return res, arrays


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    eager, a = _bench(tmp_path, "eager", "--launch", "eager")
    graph, b = _bench(tmp_path, "graph", "--launch", "graph")
    for res in (eager, graph):
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in res, k
        assert res["steps"] == 7 and res["ms_per_step"] > 0
        assert abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) <= 5e-3 * res["value"]   # (ms_per_step has 4 decimals)
        for k in ("roofline", "kernels", "cpu_baseline", "next_rows", "fast_rows_option", "ddp_step", "hbm_copy_measured"):
            assert k not in res, k
        assert res["windows"] is None and res["pre_timed_steps"]["in_step_kernel_timing_steps"] == 0
    assert graph["launch"].startswith("HIP graph") and eager["launch"].startswith("eager")
    assert {"rgb_rec_r", "ph_map_r", "ph_mean_r", "g_logits", "g_sigma", "g_disp_pp"} <= set(a)
    assert set(a) == set(b) and set(a) == set(eager["dumped_outputs"]["arrays"])
    assert sum(x.nbytes for x in a.values()) <= 64 * 2 ** 20
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert a[k].shape == b[k].shape, k
        scale = max(float(np.abs(a[k]).max()), 1e-30)
        assert float(np.abs(a[k] - b[k]).max()) <= 1e-5 * scale, k   # graph replay computes what the eager step does

"""bench.py end to end on a small scene: a plain run times exactly --steps steps and nothing else, and two runs with the
same arguments write the same outputs (the training backward rounds fp64 sums, gsr_render_backward's acc64)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--gaussians", "60000", "--width", "320", "--height", "192"]


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_exactly_steps_and_dumps_reproducible_outputs(device, tmp_path):
    d1 = _run(tmp_path / "a")
    assert d1["steps"] == 4 and d1["warmup"] == 2 and d1["timing"]["repeats"] == 1
    assert d1["optimizer"]["fused_steps"] == 4 + 2  # every optimizer step of the run: the warmup and the timed ones
    for k in ("kernels", "roofline", "cpu_baseline", "extra_workloads", "rendered_views"):
        assert k not in d1, k
    assert d1["ms_per_step"] > 0 and abs(d1["value"] - 1e3 / d1["ms_per_step"]) <= 0.01 * d1["value"]
    _run(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["features_dc.npy", "features_rest.npy", "images.npy", "loss.npy", "opacity.npy", "rotation.npy",
                     "scaling.npy", "xyz.npy"]
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape
        assert np.array_equal(x, y), f"{n}: max |difference| {float(np.abs(x.astype(np.float64) - y).max())}"

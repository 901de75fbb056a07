"""GPU: a plain `bench.py` run end to end at a tiny batch -- the contract fields of its line, --steps as the number of
timed steps, nothing of --full in it -- and --dump-outputs: two runs with the same arguments compute on the same
inputs, so their dumped outputs agree."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "2", "--seq", "128", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_line_and_dumped_outputs(cuda, tmp_path):
    a = _run(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in a, k
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["dtype"] == "bf16"
    assert abs(a["value"] - 2 * 128 / (a["ms_per_step"] * 1e-3)) < 2e-3 * a["value"]
    assert "ppo" not in a and "cpu_baseline" not in a and a["roofline"] is None and a["kernels"] == {}
    names = ("losses", "grad_norm", "params_sample", "grads_sample")
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in names}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert got["losses"].shape == (7,) and got["params_sample"].shape == (1 << 20,)
    assert abs(got["losses"][-1] - a["final_loss"]) < 1e-3
    b = _run(tmp_path / "b")
    assert abs(b["final_loss"] - a["final_loss"]) < 1e-3
    for k in names:
        other = np.load(tmp_path / "b" / (k + ".npy"))
        np.testing.assert_allclose(other, got[k], rtol=1e-3, atol=1e-5, err_msg=k)

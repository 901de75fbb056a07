"""CPU: bench.py's command line (a plain run measures the headline only; --full adds the rest) and --dump-outputs'
writer (bench.dump_outputs) on a CPU model: float32 files, a fixed seeded sample, the 64 MB cap."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default_and_full_is_opt_in():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    b = bench.parse_args(["--full", "--dump-outputs", "out", "--no-ppo"])
    assert b.full is True and b.dump_outputs == "out" and b.no_ppo is True


def _net_after_a_step(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(64, 300), torch.nn.GELU(), torch.nn.Linear(300, 6))
    x = torch.randn(32, 64)
    out = net(x)
    losses = [out[:, i].pow(2).mean() for i in range(6)]
    (sum(losses) / 6).backward()
    norm = torch.nn.utils.clip_grad_norm_(net.parameters(), 3.0)
    return net, losses, norm


def test_dump_writes_float32_arrays_with_a_fixed_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    net, losses, norm = _net_after_a_step()
    n = sum(p.numel() for p in net.parameters())
    shapes = bench.dump_outputs(str(tmp_path / "a"), net.parameters(), losses, norm, sample=1000)
    assert shapes == {"losses": (7,), "grad_norm": (1,), "params_sample": (1000,), "grads_sample": (1000,)}
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in shapes}
    assert all(a.dtype == np.float32 for a in got.values())
    want = np.array([l.item() for l in losses] + [sum(l.item() for l in losses) / 6], dtype=np.float32)
    np.testing.assert_allclose(got["losses"], want, rtol=1e-6)
    assert got["grad_norm"][0] == pytest.approx(norm.item(), rel=1e-6)
    # the sample is the seeded one, in ascending flat index over the parameters in registration order
    flat_p = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    flat_g = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(bench.DUMP_SEED))[:1000].sort().values
    np.testing.assert_array_equal(got["params_sample"], flat_p[idx].numpy())
    np.testing.assert_array_equal(got["grads_sample"], flat_g[idx].numpy())
    # the same state dumps the same files; a sample as large as the model is the whole model
    bench.dump_outputs(str(tmp_path / "b"), net.parameters(), losses, norm, sample=1000)
    for k in shapes:
        np.testing.assert_array_equal(got[k], np.load(tmp_path / "b" / (k + ".npy")))
    whole = bench.dump_outputs(str(tmp_path / "c"), net.parameters(), losses, norm, sample=n)
    assert whole["params_sample"] == (n,)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "params_sample.npy"), flat_p.numpy())


def test_dump_refuses_more_than_64_mb(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    net, losses, norm = _net_after_a_step()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    with pytest.raises(ValueError, match="cap"):
        bench.dump_outputs(str(tmp_path / "big"), net.parameters(), losses, norm, sample=1000)
    assert not os.path.exists(tmp_path / "big")
    # the default sample of the repo-dims model (38 982 227 parameters) stays far below the real cap
    assert 2 * 4 * bench.DUMP_SAMPLE + 4 * 8 <= 64 << 20

"""GPU: the row-batched decode step (csrc/decode_gemm.hip) -- its f32 MFMA GEMM against torch f32, bitwise batch
invariance, and DecodeSession(kernel="gemm") against the GEMV step and the reference-recorded fixture."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]
REPO_CLASS = [56, 135, 18, 87, 18, 25]
# (K, n_out) of every projection of the step: repo dims, then the small fixture's (d_model 128)
SHAPES = [(1216, 512), (512, 1536), (512, 512), (512, 2048), (2048, 512), (512, 339),
          (1216, 128), (128, 384), (128, 128), (128, 2048), (2048, 128), (128, 339)]


def _small_model(cuda):
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": 2, "N_HEAD": 2})
    try:
        net = model.LinearTransformer(N_CLASS, is_training=False)
    finally:
        config.AgentConfig.update(old)
    return fill_params(net, seed=int(FIX["fill_seed"])).to(cuda).eval()


def _repo_model(cuda):
    from rlmg_amd.dqn_policy import model
    net = fill_params(model.LinearTransformer(REPO_CLASS, is_training=False), seed=5).to(cuda).eval()
    assert net.d_model == 512 and net.n_layer == 12 and net.compute_dtype == torch.float32
    return net


def _tokens(n_class, n, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, c, (n, T), generator=g) for c in n_class], -1).numpy()     # (n, T, 6)


def test_decode_gemm_building_block(cuda):
    """prologue LayerNorm(s), bias / GELU / residual epilogue, strided rows: the GEMM against torch f32."""
    g = torch.Generator().manual_seed(5)
    for K, n_out in SHAPES:
        w = (torch.randn(n_out, K, generator=g) / K ** 0.5).to(cuda)
        b = torch.randn(n_out, generator=g).to(cuda)
        ln = (1 + 0.1 * torch.randn(K, generator=g)).to(cuda), (0.1 * torch.randn(K, generator=g)).to(cuda)
        ln2 = (1 + 0.1 * torch.randn(K, generator=g)).to(cuda), (0.1 * torch.randn(K, generator=g)).to(cuda)
        for M in (1, 7, 64, 257, 1024):
            big = torch.randn(M, K + 20, generator=g).to(cuda)
            x = big[:, 8:8 + K]                                       # strided rows (ld = K + 20)
            res = torch.randn(M, n_out, generator=g).to(cuda)
            tag = (K, n_out, M)
            assert (ops.decode_gemm(w, b, x) - F.linear(x, w, b)).abs().max().item() < 2e-5, tag
            assert (ops.decode_gemm(w, None, x, res=res) - (F.linear(x, w) + res)).abs().max().item() < 2e-5, tag
            x1 = F.layer_norm(x, (K,), ln[0], ln[1], 1e-5)
            got, xn = ops.decode_gemm(w, b, x, ln=ln, act="gelu", want_normed=True)
            assert (xn - x1).abs().max().item() < 2e-5, tag
            assert (got - F.gelu(F.linear(x1, w, b))).abs().max().item() < 2e-5, tag
            x2 = F.layer_norm(x1, (K,), ln2[0], ln2[1], 1e-5)
            got, xn = ops.decode_gemm(w, b, x, ln=ln, ln2=ln2, res=res, want_normed=True)
            assert (xn - x2).abs().max().item() < 2e-5, tag
            assert (got - (F.linear(x2, w, b) + res)).abs().max().item() < 3e-5, tag
            # a prologue without x_out normalises into the scratch
            assert (ops.decode_gemm(w, b, x, ln=ln) - F.linear(x1, w, b)).abs().max().item() < 2e-5, tag


def test_decode_gemm_batch_invariance(cuda):
    """Each row of an M = 1024 call is bitwise the row computed alone and in a row-permuted call."""
    g = torch.Generator().manual_seed(6)
    for K, n_out in SHAPES:
        w = (torch.randn(n_out, K, generator=g) / K ** 0.5).to(cuda)
        b = torch.randn(n_out, generator=g).to(cuda)
        ln = (1 + 0.1 * torch.randn(K, generator=g)).to(cuda), (0.1 * torch.randn(K, generator=g)).to(cuda)
        x = torch.randn(1024, K, generator=g).to(cuda)
        res = torch.randn(1024, n_out, generator=g).to(cuda)
        perm = torch.randperm(1024, generator=g).to(cuda)
        for kw in ({}, {"ln": ln, "act": "gelu", "res": res}):
            full = ops.decode_gemm(w, b, x, **kw)
            pk = dict(kw, res=res[perm]) if "res" in kw else kw
            assert torch.equal(ops.decode_gemm(w, b, x[perm], **pk), full[perm]), (K, n_out)
            for r in (0, 1, 63, 64, 500, 1023):
                rk = dict(kw, res=res[r:r + 1]) if "res" in kw else kw
                assert torch.equal(ops.decode_gemm(w, b, x[r:r + 1], **rk)[0], full[r]), (K, n_out, r)


def _teacher_forced(net, toks, kernel, graph=False):
    sess = generation.DecodeSession(net, n_songs=toks.shape[0], kernel=kernel, graph=graph)
    logits, hidden = [], []
    for t in range(toks.shape[1]):
        logits.append(np.array(sess.step(toks[:, t]), copy=True).reshape(toks.shape[0], -1))
        hidden.append(sess.hidden.clone())
    return np.stack(logits, 1), torch.stack(hidden, 1)


@pytest.mark.parametrize("dims", ["small", "repo"])
def test_gemm_step_matches_gemv_step(cuda, dims):
    net = _small_model(cuda) if dims == "small" else _repo_model(cuda)
    N = 5 if dims == "small" else 64
    toks = _tokens(N_CLASS if dims == "small" else REPO_CLASS, N, 16, 3)
    a, ha = _teacher_forced(net, toks, "gemv")
    b, hb = _teacher_forced(net, toks, "gemm")
    worst = float(np.abs(a - b).max())
    print("%s dims, %d songs: worst |gemm - gemv| logit difference %.3g" % (dims, N, worst))
    assert worst < 1e-5, worst
    assert (ha - hb).abs().max().item() < 1e-5


def test_gemm_session_matches_reference_fixture(cuda):
    net = _small_model(cuda)
    for graph in (False, True):
        sess = generation.DecodeSession(net, graph=graph, kernel="gemm")
        for t in range(len(FIX["logits"])):
            got = sess.step(FIX["tokens"][t])
            assert np.abs(got - FIX["logits"][t]).max() < 1e-4, (graph, t)
        if graph:
            assert sess.use_graph and sess.census.get("memset", 0) == 0, sess.census


def test_gemm_session_modes(cuda):
    """Eager == graph replay bitwise; GEMM steps after a ragged prefill match GEMV steps; reset() sees new weights."""
    net = _small_model(cuda)
    toks = _tokens(N_CLASS, 6, 12, 8)
    eager, he = _teacher_forced(net, toks, "gemm", graph=False)
    replay, hr = _teacher_forced(net, toks, "gemm", graph=True)
    assert np.array_equal(eager, replay) and torch.equal(he, hr)
    # ragged prefill, then steps: the state buffers are shared with whichever step kernel runs
    prompt = _tokens(N_CLASS, 6, 20, 9)
    lens = [20, 1, 7, 13, 20, 2]
    out = {}
    for kernel in ("gemv", "gemm"):
        sess = generation.DecodeSession(net, n_songs=6, kernel=kernel, graph=True)
        first = sess.prefill(prompt, lengths=lens).copy()
        out[kernel] = [first] + [sess.step(toks[:, t]).copy() for t in range(6)]
    for t, (a, b) in enumerate(zip(out["gemv"], out["gemm"])):
        assert np.abs(a - b).max() < 1e-5, t
    # weights changed between songs are picked up by reset(), in the captured graph too
    sess = generation.DecodeSession(net, n_songs=2, kernel="gemm", graph=True)
    before = [sess.step(toks[:2, t]).copy() for t in range(3)]
    with torch.no_grad():
        net.proj_pitch.bias.add_(1.0)
        net.transformer_encoder.layers[0].attention.query_projection.weight.mul_(1.5)
    try:
        sess.reset()
        after = [sess.step(toks[:2, t]).copy() for t in range(3)]
        ref = generation.DecodeSession(net, n_songs=2, kernel="gemv", graph=False)
        want = [ref.step(toks[:2, t]).copy() for t in range(3)]
    finally:
        with torch.no_grad():
            net.proj_pitch.bias.sub_(1.0)
            net.transformer_encoder.layers[0].attention.query_projection.weight.div_(1.5)
    assert np.abs(after[2] - before[2]).max() > 1e-3
    for a, b in zip(after, want):
        assert np.abs(a - b).max() < 1e-5


def test_gemm_session_refusals(cuda):
    net = _small_model(cuda)
    with pytest.raises(ValueError):
        generation.DecodeSession(net, kernel="gemmx")
    with pytest.raises(RuntimeError):
        generation.DecodeSession(net, kernel="gemm", fused=False)

"""GPU: the packed train step (CWTrunk.train_step_packed: songs of different lengths end to end, no padded rows) through
every layer -- input front with positions from a table, encoder layers with the packed scan forward and backward, heads.

Model: the repo's layer shape (d_model 512, 8 heads, d_ff 2048), 2 layers, a small vocabulary; songs of 1, 63, 64, 65, 130,
200 and 257 rows (R = 780); f32 and bf16, dropout off and on.

Losses and gradients.  The six losses and every parameter gradient against oracle.step_f64, song by song: each song is a
(1, L) batch of its own whose dropout rows start at row0 = cu[s] (the kernels key dropout by the packed row) and whose loss
share is divided by the GLOBAL mask sum.  Bound: the expression of tests/test_bf16_regimes_gpu.py / tests/test_model_gpu.py
restated for this depth -- 4 sqrt(n) 2^-9 / sqrt(3) of each tensor's own norm with n = 2 (10 n_layers + 5) bf16 roundings
between the input and a parameter gradient (10 per layer each way; embedding, in_linear, positions, final norm, logits),
the floor of 1e-4 of the rms gradient norm for a gradient that is nearly zero, and the same fraction of the largest loss.
The Q and K projection gradients take that file's two measured factors, per layer and from the f64 reference itself
(oracle/step_f64.normaliser_terms / row_terms, summed over the songs): 4 sqrt(n + 3 G^2) U C with G the normaliser gain
and C >= 1 the cancellation of the rows in the parameter gradient.
The f32 runs are held to the same bounds (they sit far inside them; the ratios are printed).

Isolation through the stack (p = 0): changing one song's tokens leaves every other song's hidden rows bitwise unchanged.
Packed against padded (p = 0): both runs are within the bound of the same f64 losses, so they differ by at most the sum
of the two bounds -- a consequence of the first check, asserted as such.
Entry scripts: one packed step of each pretraining script runs, gives finite losses and changes the parameters; with the
option unset the loop launches no packed entry point (asserted on the log of C-ABI calls).
"""
import os
import sys

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import data as cwdata, ops  # noqa: E402
from oracle import step_f64  # noqa: E402

pytestmark = pytest.mark.gpu
N_CLASS = [9, 12, 7, 11, 6, 8]
LENS = [1, 63, 64, 65, 130, 200, 257]
N_LAYER = 2
U = 2.0 ** -9 / 3 ** 0.5
N_ROUNDINGS = 2 * (N_LAYER * 10 + 5)
BOUND = 4 * N_ROUNDINGS ** 0.5 * U
EMB_SIZES = (128, 256, 64, 512, 128, 128)
REAL_CALL = ops._call


def build_net(cuda, dtype, p):
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 512, "N_LAYER": N_LAYER, "N_HEAD": 8})
    try:
        net = fill_params(model.LinearTransformer(N_CLASS), seed=77).to(cuda).train()
    finally:
        config.AgentConfig.update(old)
    net.compute_dtype = dtype
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p
    return net


def songs(T=None, seed=5):
    """x, y (N, T, 6), mask (N, T): song n live on its first LENS[n] rows, with two holes inside songs."""
    g = torch.Generator().manual_seed(seed)
    N, T = len(LENS), T or max(LENS)
    x = torch.stack([torch.randint(0, n, (N, T), generator=g) for n in N_CLASS], -1).numpy()
    y = torch.stack([torch.randint(0, n, (N, T), generator=g) for n in N_CLASS], -1).numpy()
    mask = np.zeros((N, T), dtype=np.float32)
    for n, L in enumerate(LENS):
        mask[n, :L] = 1
    mask[5, 17:23] = 0
    mask[6, 0] = 0
    return x, y, mask


def record_seeds(monkeypatch):
    seeds = []
    real = ops.next_seed

    def next_seed():
        s = real()
        seeds.append(s)
        return s

    monkeypatch.setattr(ops, "next_seed", next_seed)
    return seeds


def song_losses(P, pe, tokens, target, mask, msum, p, seeds, row0, taps):
    """oracle.step_f64.step_losses for one song (its arithmetic, line for line), with the encoder's taps handed out."""
    T = tokens.shape[1]
    embs = torch.cat([P["word_emb_%s.lut.weight" % a][tokens[..., i]] * math.sqrt(d)
                      for i, (a, d) in enumerate(zip(step_f64.ATTRS, EMB_SIZES))], -1)
    e = F.linear(embs, P["in_linear.weight"], P["in_linear.bias"]) + pe[:T]
    e = step_f64.dropout.dropout(e, p, seeds[0], row0)
    h = step_f64.encoder_forward(e, P, N_LAYER, 8, p, seeds[1:], row0, "transformer_encoder.", taps=taps)
    m = mask.reshape(-1).to(h.dtype)
    losses = []
    for i, (a, nt) in enumerate(zip(step_f64.ATTRS, N_CLASS)):
        logits = F.linear(h, P["proj_%s.weight" % a], P["proj_%s.bias" % a]).reshape(-1, nt)
        losses.append((F.cross_entropy(logits, target[..., i].reshape(-1), reduction="none") * m).sum() / msum)
    return torch.stack(losses)


def reference(net, batch, p, seeds, gains=None):
    """oracle.step_f64 song by song: row0 = cu[s], the global mask sum -> (losses (6,), {name: grad}); gains receives
    the per-layer dicts of step_f64.encoder_vjp (normaliser gains and uncancelled row norms), summed over the songs."""
    params = dict(net.named_parameters())
    dev = batch.tokens.device
    P = step_f64._leaves(params, torch.float64, dev)
    pe = net.pos_emb.pe.reshape(-1, 512).to(device=dev, dtype=torch.float64)
    msum = batch.mask.double().sum()
    total = torch.zeros(6, dtype=torch.float64, device=dev)
    cu = batch.cu_host
    sums = [[0.0] * 8 for _ in range(N_LAYER)]
    for s in range(len(cu) - 1):
        sl = slice(cu[s], cu[s + 1])
        taps = []
        ls = song_losses(P, pe, batch.tokens[sl][None], batch.target[sl][None], batch.mask[sl][None], msum, p, seeds,
                         cu[s], taps)
        (ls.sum() / 6).backward()
        total += ls.detach()
        for i, (x2, q, k, a) in enumerate(taps):
            t = step_f64.normaliser_terms(q, k, a) + step_f64.row_terms(x2, q) + step_f64.row_terms(x2, k)
            sums[i] = [u + w for u, w in zip(sums[i], t)]
    if gains is not None:
        gains.extend({"query": (v[0] / v[1]) ** 0.5, "key": (v[2] / v[3]) ** 0.5,
                      "query_rows": (v[4] ** 0.5, v[5] ** 0.5), "key_rows": (v[6] ** 0.5, v[7] ** 0.5)} for v in sums)
    return total, {k: v.grad for k, v in P.items()}


def bounds_for(norms, gains):
    """tests/test_bf16_regimes_gpu.py::_bounds at this model's depth: BOUND for every tensor; the Q / K projection
    gradients of layer i with its normaliser gain, times the cancellation of their row sums (at least one)."""
    b = {k: BOUND for k in norms}
    for i, gd in enumerate(gains):
        for part in ("query", "key"):
            for j, sfx in enumerate(("bias", "weight")):
                name = "transformer_encoder.layers.%d.attention.%s_projection.%s" % (i, part, sfx)
                b[name] = (4 * (N_ROUNDINGS + 3 * gd[part] ** 2) ** 0.5 * U
                           * max(1.0, gd[part + "_rows"][j] / max(norms[name], 1e-300)))
    return b


@pytest.mark.parametrize("dtype,p,front", [(torch.float32, 0.0, "embed"), (torch.float32, 0.1, "proj"),
                                           (torch.bfloat16, 0.0, "proj"), (torch.bfloat16, 0.1, "embed")],
                         ids=["f32-p0", "f32-p0.1", "bf16-p0", "bf16-p0.1"])
def test_losses_and_gradients_against_f64_song_by_song(cuda, monkeypatch, dtype, p, front):
    if front == "proj":
        monkeypatch.setattr(ops, "EMBED_PROJ_MIN_ROWS", 1)       # the one-pass front with its position table
    names_called = []
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: (names_called.append(name), REAL_CALL(name, *a, **kw))[1])
    net = build_net(cuda, dtype, p)
    x, y, mask = songs()
    batch = cwdata.pack_songs(x, y, mask, list(range(len(LENS))), device=cuda)
    assert batch.rows == sum(LENS) == 780 and batch.songs == [6, 5, 4, 3, 2, 1, 0]
    seeds = record_seeds(monkeypatch)
    torch.manual_seed(99)
    lg = net.train_step_packed(batch)
    (sum(lg) / 6).backward()
    torch.cuda.synchronize()
    assert ops._seed_base() is None
    assert len(seeds) == (1 + 3 * N_LAYER if p > 0 else 0)
    bf = dtype == torch.bfloat16
    assert names_called.count("cwlt_causal_linear_fwd_packed") == N_LAYER and "cwlt_causal_linear_fwd" not in names_called
    assert "cwlt_encoder_fwd" not in names_called and "cwlt_encoder_layer_fwd" not in names_called
    assert names_called.count("cwlt_causal_linear_bwd_sweep_packed") == (N_LAYER if bf else 0)
    assert names_called.count("cwlt_causal_linear_bwd_dkdv_packed") == (0 if bf else N_LAYER)
    assert ("cwlt_cw_embed_proj_fwd_pos" in names_called) == (front == "proj")
    assert ("cwlt_posenc_dropout_pos" in names_called) == (front == "embed")
    gains = []
    l64, ref = reference(net, batch, p, seeds if p > 0 else [0] * (1 + 3 * N_LAYER), gains)
    print("normaliser gains (q, k) per layer:", ", ".join("(%.2f, %.2f)" % (gd["query"], gd["key"]) for gd in gains))
    got_l = torch.tensor([l.item() for l in lg], dtype=torch.float64)
    l64 = l64.cpu()
    lr = (got_l - l64).abs().max().item() / l64.abs().max().item()
    print("losses %s f64 %s  ratio to bound %.4f" % (got_l.tolist(), l64.tolist(), lr / BOUND))
    params = dict(net.named_parameters())
    names = [n for n in params if ref[n] is not None]
    assert all(params[n].grad is None for n in params if ref[n] is None)
    norms = {n: ref[n].norm().item() for n in names}
    floor = 1e-4 * (sum(v ** 2 for v in norms.values()) / len(names)) ** 0.5
    r = {n: (params[n].grad.double() - ref[n]).norm().item() / max(norms[n], floor) for n in names}
    b = bounds_for(norms, gains)
    for n in sorted(r, key=lambda n: r[n] / b[n], reverse=True):
        print("    %-62s %.5f  (%.3f of the bound %.5f)" % (n, r[n], r[n] / b[n], b[n]))
    assert all(torch.isfinite(params[n].grad).all() for n in names)
    assert lr <= BOUND, (lr, BOUND)
    worst = max(r, key=lambda n: r[n] / b[n])
    assert r[worst] <= b[worst], (worst, r[worst], b[worst])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_songs_are_isolated_through_the_stack_and_packed_equals_padded(cuda, monkeypatch, dtype):
    net = build_net(cuda, dtype, 0.0)
    x, y, mask = songs()
    batch = cwdata.pack_songs(x, y, mask, list(range(len(LENS))), device=cuda)
    cu = ops.SeqOffsets(batch.cu, host=batch.cu_host)
    with torch.no_grad():
        h0 = net.forward_hidden_packed(batch.tokens, cu, batch.pos)
        j = 2                                                     # packed song 2 = dataset song 4, 130 rows
        a, z = batch.cu_host[j], batch.cu_host[j + 1]
        tok = batch.tokens.clone()
        tok[a:z] = (tok[a:z] + 1) % torch.tensor(N_CLASS, device=cuda)
        h1 = net.forward_hidden_packed(tok, cu, batch.pos)
    bits = lambda t: t.contiguous().view(torch.uint8)
    with torch.no_grad():
        assert torch.equal(bits(net.forward_hidden_packed(batch.tokens, cu)), bits(h0))       # pos built from the offsets
    with pytest.raises(ValueError, match="position table"):                                   # a pos that is not cu's
        net.forward_hidden_packed(batch.tokens, cu, torch.roll(batch.pos, 1))
    assert h0.shape == (780, 512) and torch.isfinite(h0.float()).all()
    assert torch.equal(bits(h0[:a]), bits(h1[:a])) and torch.equal(bits(h0[z:]), bits(h1[z:]))
    assert not torch.equal(bits(h0[a:z]), bits(h1[a:z]))
    # the padded batch of the same songs defines the same loss: both within BOUND of the f64 losses
    lp = net.train_step_packed(batch)
    lr = net.train_step(torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(mask).to(cuda))
    l64, _ = reference(net, batch, 0.0, [0] * (1 + 3 * N_LAYER))
    lp, lr, l64 = (torch.stack([v.detach().double() for v in t]).cpu() for t in (lp, lr, l64))
    scale = l64.abs().max().item()
    print("packed %s\npadded %s\nf64    %s" % (lp.tolist(), lr.tolist(), l64.tolist()))
    assert (lp - l64).abs().max().item() <= BOUND * scale and (lr - l64).abs().max().item() <= BOUND * scale
    assert (lp - lr).abs().max().item() <= 2 * BOUND * scale


SMALL = {"D_MODEL": 128, "N_LAYER": 2, "N_HEAD": 2}


def call_log(monkeypatch):
    names = []
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: (names.append(name), REAL_CALL(name, *a, **kw))[1])
    return names


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unset"])
def test_dqn_pretrain_script_takes_one_packed_step(cuda, tmp_path, monkeypatch, packed):
    monkeypatch.chdir(tmp_path)
    from rlmg_amd.dqn_policy import agent_pretrain as A, config
    for k, v in SMALL.items():
        monkeypatch.setitem(config.AgentConfig, k, v)
    real_load = cwdata.load_dqn
    monkeypatch.setattr(cwdata, "load_dqn", lambda a, b, **kw: real_load(a, b, n_seq=4, T=256))   # 2 x 230 + 2 x 256 rows
    made = []

    class Recorded(A.TransformerModel):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append((self, {k: v.detach().clone() for k, v in self.state_dict().items()}))

    monkeypatch.setattr(A, "TransformerModel", Recorded)
    if packed:
        monkeypatch.setenv("CWLT_PACKED_ROWS", "1024")            # the environment form of packed_rows=1024
    else:
        monkeypatch.delenv("CWLT_PACKED_ROWS", raising=False)
    names = call_log(monkeypatch)
    loss = A.train(n_epoch=1, log=lambda *a: None)
    assert loss == loss and 0 < loss < 10
    net, init = made[0]
    changed = [k for k, v in net.state_dict().items() if not torch.equal(v.cpu(), init[k].cpu())]
    assert any(k.startswith("transformer_encoder.layers.0.attention") for k in changed) and "in_linear.weight" in changed
    n_packed = sum(n.endswith("_packed") for n in names)
    if packed:
        assert names.count("cwlt_causal_linear_fwd_packed") == 2 and "cwlt_causal_linear_fwd" not in names   # one step
        assert "cwlt_posenc_dropout_pos" in names
    else:
        assert n_packed == 0 and "cwlt_posenc_dropout_pos" not in names and "cwlt_cw_embed_proj_fwd_pos" not in names
        assert names.count("cwlt_causal_linear_fwd") == 2                                   # one rectangular batch of 4


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unset"])
def test_ppo_pretrain_script_takes_one_packed_step(cuda, tmp_path, monkeypatch, packed):
    monkeypatch.chdir(tmp_path)
    from rlmg_amd.ppo_policy import config, my_pretrain as M
    for c in (config.ActorConfig, config.CriticConfig, config.DiscriConfig):
        for k, v in SMALL.items():
            monkeypatch.setitem(c, k, v)
    monkeypatch.setattr(M, "BATCH_SIZE", 4)
    monkeypatch.setattr(M, "Init_lr", 1e-3)
    monkeypatch.delenv("CWLT_PACKED_ROWS", raising=False)
    (e2w, _), ds = cwdata.load_ppo("missing", "missing", n_seq=4, T=256)
    model = M.LinearTransformer([len(e2w[k]) + 1 for k in e2w], is_training=True).to(cuda).train()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = ops.graph_adam(model.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[500], gamma=0.1)
    os.makedirs("ckpt")
    names = call_log(monkeypatch)
    rec = M.pretrain(model, ds, opt, sched, False, "config_log.txt", "ckpt", num_epoch=1, log=lambda *a: None,
                     packed_rows=1024 if packed else None)
    assert len(rec) == 1 and np.isfinite(rec[0])
    assert any(not torch.equal(v, init[k]) for k, v in model.state_dict().items() if k.startswith("transformer_encoder."))
    if packed:
        assert names.count("cwlt_causal_linear_fwd_packed") == 2 and "cwlt_causal_linear_fwd" not in names
        with pytest.raises(ValueError, match="agent"):
            M.pretrain(model, ds, opt, sched, True, "config_log.txt", "ckpt", num_epoch=1, packed_rows=1024)
    else:
        assert not any(n.endswith("_packed") or n.endswith("_pos") for n in names)
        assert names.count("cwlt_causal_linear_fwd") == 2

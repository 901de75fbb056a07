"""CPU: the f64 references of the bf16 GPU tests (oracle/dropout.py, oracle/step_f64.py) checked on their own.

* the torch restatement of the kernels' dropout keep mask against a scalar restatement of csrc/cwlt_common.h in Python
  integers, at chosen element indices: even and odd elements, pair indices past 2^32 (the hash's `hi` word);
* with dropout off, the layer-stack and train-step references against oracle/ft_encoder.py and oracle/cw_model.py in f64:
  forward and every gradient;
* evaluation in slabs of whole sequences equals whole-batch evaluation, dropout on.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

from oracle import cw_model, dropout, ft_encoder, step_f64  # noqa: E402

M32 = 0xFFFFFFFF
N_CLASS = [56, 135, 18, 87, 18, 25]


# ---- the keep mask ------------------------------------------------------------------------------------------------
def _hash32(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def _keep(seed, idx, p):
    """dropout_keep(seed, idx, drop_thresh(p)) of csrc/cwlt_common.h, one element, Python integers."""
    pair = idx >> 1
    lo, hi = pair & M32, (pair >> 32) & M32
    key = (seed & M32) ^ (((seed >> 32) * 0x9E3779B9) & M32) ^ ((hi * 0x85EBCA6B) & M32)
    r = _hash32(((lo * 0x9E3779B1) & M32) ^ key)
    bits = (r >> 16) if idx & 1 else (r & 0xFFFF)
    return bits >= int(p * 65536 + 0.5)


SEEDS = [0, 1, 0x2545F4914F6CDD1D & ((1 << 62) - 1), (1 << 62) - 1, 0x123456789]


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_matches_the_scalar_restatement(p):
    g = torch.Generator().manual_seed(3)
    idx = [0, 1, 2, 3, 4094, 4095, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1,
           (1 << 33) - 2, (1 << 33) - 1, 1 << 33, (1 << 33) + 1, (1 << 33) + 2, (1 << 40) + 7, (1 << 62) + 1, (1 << 62) + 2]
    idx += torch.randint(0, 1 << 62, (200,), generator=g).tolist()
    idx += torch.randint(0, 1 << 30, (200,), generator=g).tolist()
    assert sum(i >> 1 >= 1 << 32 for i in idx) > 100 and {i & 1 for i in idx} == {0, 1}
    t = torch.tensor(idx, dtype=torch.int64)
    for seed in SEEDS:
        got = dropout.keep_flags(seed, p, t).tolist()
        want = [_keep(seed, i, p) for i in idx]
        assert got == want, seed
    # a site's tensor: element row * cols + col, shifted by whole rows in a slab
    m = dropout.site_mask(SEEDS[2], p, 3, 10, row0=(1 << 31) + 5)
    start = ((1 << 31) + 5) * 10
    assert m.flatten().tolist() == [_keep(SEEDS[2], start + j, p) for j in range(30)]


def test_keep_rate_and_scale():
    m = dropout.site_mask(12345, 0.1, 256, 1024)
    assert abs(1.0 - m.double().mean().item() - 6554 / 65536) < 3e-3
    assert dropout.thresh16(0.1) == 6554 and dropout.thresh16(0.0) == 0 and dropout.thresh16(0.5) == 32768
    assert dropout.keep_scale(0.1) == 65536 / (65536 - 6554) and dropout.keep_scale(0.0) == 1.0
    x = torch.ones(4, 6, dtype=torch.float64)
    y = dropout.dropout(x, 0.5, 7, row0=3)
    assert torch.equal(y != 0, dropout.site_mask(7, 0.5, 4, 6, row0=3)) and set(y.unique().tolist()) <= {0.0, 2.0}
    assert torch.equal(dropout.dropout(x, 0.0, 7), x)


# ---- the references at p = 0 against the module oracles -----------------------------------------------------------
def _ft_encoder(n_layers, seed):
    enc = ft_encoder.TransformerEncoderBuilder.from_kwargs(
        n_layers=n_layers, n_heads=2, query_dimensions=64, value_dimensions=64, feed_forward_dimensions=256,
        activation="gelu", dropout=0.1, attention_type="causal-linear").get()
    return fill_params(enc, seed=seed).double().eval()


def _leaf_grads(module):
    return {n: q.grad for n, q in module.named_parameters()}


@pytest.mark.parametrize("L", [37, 300])
def test_encoder_reference_matches_ft_encoder_without_dropout(L):
    """Two layers + final norm; L = 300 takes oracle/cla.py's chunked form, L = 37 the quadratic one."""
    enc = _ft_encoder(2, 5)
    g = torch.Generator().manual_seed(L)
    x = torch.randn(3, L, 128, generator=g, dtype=torch.float64)
    dy = torch.randn(3, L, 128, generator=g, dtype=torch.float64)
    xin = x.clone().requires_grad_(True)
    y = enc(xin, ft_encoder.TriangularCausalMask(L))
    y.backward(dy)
    params = dict(enc.named_parameters())
    yr, dxr, gr = step_f64.encoder_vjp(params, x, dy, 2, 2, 0.0, [0] * 6)
    assert torch.allclose(yr, y.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(dxr, xin.grad, rtol=0, atol=1e-11)
    want = _leaf_grads(enc)
    assert gr.keys() == want.keys()
    for n in want:
        assert torch.allclose(gr[n], want[n], rtol=0, atol=1e-10 * max(1.0, want[n].abs().max().item())), n


def _cw_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([torch.randint(0, n, (B, T), generator=g) for n in N_CLASS], -1)
    y = torch.stack([torch.randint(0, n, (B, T), generator=g) for n in N_CLASS], -1)
    mask = torch.ones(B, T)
    mask[0, T - 7:] = 0
    mask[B - 1, :3] = 0
    return x, y, mask


def test_step_reference_matches_cw_model_without_dropout():
    ref = fill_params(cw_model.CWLinearTransformer(N_CLASS, 128, 2, 2, d_inner=256, variant="dqn"), seed=7)
    ref = ref.double().eval()
    x, y, mask = _cw_inputs(3, 40, 1)
    lr = ref.train_step(x, y, mask.double())
    (sum(lr) / 6).backward()
    params = dict(ref.named_parameters())
    losses, grads = step_f64.step_grads(params, ref.pos_emb.pe, x, y, mask, N_CLASS, 2, 2, 0.0, [0] * 7)
    assert torch.allclose(losses, torch.stack([l.detach() for l in lr]), rtol=0, atol=1e-12)
    want = _leaf_grads(ref)
    assert grads.keys() == want.keys()
    for n in want:
        if want[n] is None:                                     # project_concat_type: declared, never used
            assert grads[n] is None and n.startswith("project_concat_type"), n
            continue
        assert torch.allclose(grads[n], want[n], rtol=0, atol=1e-10 * max(1.0, want[n].abs().max().item())), n


def test_normaliser_terms_split_the_attention_gradient():
    """normaliser_terms' second sums are what the first sums lose to the normaliser: dphi(q_i) + c_i z_i and
    dphi(k_j) + sum_{i>=j} c_i phi(q_i) equal the numerator-only sums, written here from the quadratic form."""
    from oracle import cla
    g = torch.Generator().manual_seed(4)
    n, L, H, E = 2, 33, 2, 64
    q, k, v, dout = (torch.randn(n, L, H, E, generator=g, dtype=torch.float64) for _ in range(4))
    q.requires_grad_(True)
    k.requires_grad_(True)
    out = cla.cla_quadratic(q, k, v)
    out.retain_grad()
    out.backward(dout)
    tq2, dq2, tk2, dk2 = step_f64.normaliser_terms(q, k, out)
    Q, K = cla.feature_map(q.detach()), cla.feature_map(k.detach())
    tril = torch.tril(torch.ones(L, L, dtype=torch.float64))
    den = torch.einsum("nihe,njhe->nhij", Q, K) * tril
    den = den.sum(-1).permute(0, 2, 1)[..., None] + cla.EPS                              # (n, L, H, 1)
    w = torch.einsum("njhm,nihm->nhij", v, dout) * tril                                  # v_j . dout_i, j <= i
    first_q = torch.einsum("nhij,njhe->nihe", w, K) / den
    first_k = torch.einsum("nhij,nihe->njhe", w / den.permute(0, 2, 1, 3), Q)
    c = (out.detach() * dout).sum(-1, keepdim=True) / den
    dphi_q = q.grad / step_f64._dphi(q.detach())
    dphi_k = k.grad / step_f64._dphi(k.detach())
    assert torch.allclose(dphi_q + c * K.cumsum(1), first_q, rtol=1e-10, atol=1e-12)
    assert torch.allclose(dphi_k + (c * Q).flip(1).cumsum(1).flip(1), first_k, rtol=1e-10, atol=1e-12)
    assert abs(tq2 - (c * K.cumsum(1)).square().sum().item()) <= 1e-9 * tq2
    assert abs(dq2 - dphi_q.square().sum().item()) <= 1e-9 * dq2 and dk2 > 0 and tk2 > 0


# ---- slabs ---------------------------------------------------------------------------------------------------------
def test_encoder_slabs_equal_the_whole_batch_with_dropout():
    enc = _ft_encoder(2, 6)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 70, 128, generator=g, dtype=torch.float64)
    dy = torch.randn(5, 70, 128, generator=g, dtype=torch.float64)
    params = dict(enc.named_parameters())
    seeds = [11, 12, 13, 21, 22, 23]
    whole = step_f64.encoder_vjp(params, x, dy, 2, 2, 0.1, seeds)
    slabs = step_f64.encoder_vjp(params, x, dy, 2, 2, 0.1, seeds, slab=2)
    assert torch.allclose(whole[0], slabs[0], rtol=0, atol=1e-12)
    assert torch.allclose(whole[1], slabs[1], rtol=0, atol=1e-12)
    for n in whole[2]:
        assert torch.allclose(whole[2][n], slabs[2][n], rtol=1e-12, atol=1e-13), n
    # the masks did act, and the slabs kept their global rows: a slab evaluated as if it started the batch differs
    nodrop = step_f64.encoder_vjp(params, x, dy, 2, 2, 0.0, seeds)
    assert (whole[0] - nodrop[0]).abs().max().item() > 0.1
    local = step_f64.encoder_vjp(params, x[2:4], dy[2:4], 2, 2, 0.1, seeds)
    assert (local[0] - whole[0][2:4]).abs().max().item() > 0.1


def test_step_slabs_equal_the_whole_batch_with_dropout():
    ref = fill_params(cw_model.CWLinearTransformer(N_CLASS, 128, 2, 2, d_inner=256, variant="dqn"), seed=8)
    x, y, mask = _cw_inputs(5, 24, 2)
    params = dict(ref.named_parameters())
    seeds = [5, 11, 12, 13, 21, 22, 23]
    lw, gw = step_f64.step_grads(params, ref.pos_emb.pe, x, y, mask, N_CLASS, 2, 2, 0.1, seeds)
    ls, gs = step_f64.step_grads(params, ref.pos_emb.pe, x, y, mask, N_CLASS, 2, 2, 0.1, seeds, slab=2)
    assert torch.allclose(lw, ls, rtol=0, atol=1e-12)
    for n in gw:
        if gw[n] is None:
            assert gs[n] is None
            continue
        assert torch.allclose(gw[n], gs[n], rtol=1e-11, atol=1e-13), n
    l0, _ = step_f64.step_grads(params, ref.pos_emb.pe, x, y, mask, N_CLASS, 2, 2, 0.0, seeds)
    assert (lw - l0).abs().max().item() > 1e-3                   # dropout did act

"""CPU: pins oracle/disc_f64.py, the f64 reference of the two Longformer discriminators with the kernels' dropout that
tests/test_disc_f64_gpu.py holds the kernels to.

With p = 0 it must reproduce the four fixtures recorded from the reference's own classes (to the tolerances
test_oracle_golden.py, test_oracle_disc_grads.py and test_oracle_reward_grads.py use for oracle/discriminator.py) and
agree with oracle/discriminator.py at repo dims; with p = 0.1 its attention mask keeps 1 - p of the band and nothing
outside and its mean over seeds approaches the p = 0 output; its band attention passes gradcheck with a mask and
dropout; and every wrong ingredient of the GPU test's teeth moves the f64 result by at least 2 x TEETH x the bound that
the GPU comparison of that quantity uses, so that a teeth failure there means a blind comparison, not a harmless
ingredient.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

from oracle import disc_f64, dropout  # noqa: E402
from oracle import discriminator as odisc  # noqa: E402

N_CLASS = [56, 135, 18, 87, 18, 25]
TEETH = 5.0
ROOM = 2.0


def _load(name):
    return np.load(os.path.join(HERE, "golden", name), allow_pickle=False)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _airl(n_class, seed, dims=(128, 2, 2)):
    import rlmg_amd  # noqa: F401  (host classes only, as parameter containers)
    from rlmg_amd.dqn_policy import AIRL_model
    old = (AIRL_model.D_MODEL, AIRL_model.N_LAYER, AIRL_model.N_HEAD)
    AIRL_model.D_MODEL, AIRL_model.N_LAYER, AIRL_model.N_HEAD = dims
    try:
        return fill_params(AIRL_model.LongFormer(n_class), seed=seed)
    finally:
        AIRL_model.D_MODEL, AIRL_model.N_LAYER, AIRL_model.N_HEAD = old


def _reward(n_token, seed, dims=(128, 2, 2)):
    import rlmg_amd  # noqa: F401
    from rlmg_amd.ppo_policy import config as pcfg, model as pmodel
    old = dict(pcfg.DiscriConfig)
    pcfg.DiscriConfig.update({"D_MODEL": dims[0], "N_LAYER": dims[1], "N_HEAD": dims[2]})
    try:
        return fill_params(pmodel.LongFormer(n_token), seed=seed)
    finally:
        pcfg.DiscriConfig.update(old)


def _f64(net):
    return {k: v.detach().double() for k, v in net.state_dict().items()}


STATS = (torch.linspace(-0.2, 0.2, 128).double(), torch.linspace(0.5, 1.5, 128).double())


def test_reproduces_the_airl_score_fixture():
    fx = _load("airl_small.npz")
    P = _f64(_airl(fx["n_class"].tolist(), 41))
    got, stats, _ = disc_f64.airl_forward(P, STATS, _t(fx["x"]), _t(fx["mask"]), 2, 2, 25, False)
    assert (got - _t(fx["score"])).abs().max().item() < 1e-5
    assert stats is STATS                                           # eval mode leaves the running statistics alone


def test_reproduces_the_airl_loss_and_gradient_fixture():
    fx = _load("airl_grads_small.npz")
    P = _f64(_airl(fx["n_class"].tolist(), 43))
    names = fx["names"].tolist()
    for k in names:
        P[k].requires_grad_(True)
    x_exp, x_ag, mask = (_t(fx[k]) for k in ("x_exp", "x_agent", "mask"))
    (e, a, c), _ = disc_f64.airl_train_loss(P, STATS, x_exp, x_ag, mask, 2, 2, 25, batch_stats=False)
    assert np.allclose([e.item(), a.item(), c.item()], fx["losses"], atol=2e-5)
    (e + (a + c)).backward()
    for k, want_norm in zip(names, fx["norms"]):
        g = P[k].grad
        assert g is not None, k
        assert abs(g.norm().item() - want_norm) < 2e-5 + 1e-4 * want_norm, k
        want = _t(fx["grad." + k]).double()
        got = g[:8] if g.numel() > 4096 else g
        assert (got - want).abs().max().item() < 2e-5, k


def test_reproduces_the_reward_fixture():
    fx = _load("ppo_reward_small.npz")
    P = _f64(_reward(fx["n_token"].tolist(), 31))
    got, _ = disc_f64.ppo_token_forward(P, _t(fx["x"]), _t(fx["mask"]), 2, 2, 64)
    assert (got - _t(fx["reward"])).abs().max().item() < 1e-5


def test_reproduces_the_reward_gradient_fixture():
    fx = _load("ppo_reward_grads_small.npz")
    P = _f64(_reward(fx["n_token"].tolist(), 33))
    names = fx["names"].tolist()
    for k in names:
        P[k].requires_grad_(True)
    score, _ = disc_f64.ppo_token_forward(P, _t(fx["x"]), _t(fx["mask"]), 2, 2, 64)
    assert (score.detach() - _t(fx["score"]).double()).abs().max().item() < 2e-6
    (score * _t(fx["w"]).double()).sum().backward()
    for k, want_norm in zip(names, fx["norms"]):
        g = P[k].grad
        if g is None:           # HF embeds its window PADDING through word_embeddings: a defined, all-zero gradient
            assert want_norm == 0.0, k
            continue
        assert abs(g.norm().item() - want_norm) < 1e-6 + 1e-4 * want_norm, k
        want = _t(fx["grad." + k]).double()
        got = g[:8] if g.numel() > 4096 else g
        assert (got - want).abs().max().item() < 1e-6 + 1e-4 * want.abs().max().item(), k


def _tokens(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n, (B, L), generator=g) for n in N_CLASS], -1)


@pytest.mark.timeout(300)
def test_agrees_with_the_dense_oracle_at_repo_dims():
    """AIRL at 512 / 10 / 8, window 50, and the reward model at 512 / 12 / 8, window 512, on 3 x 50 tokens with a padded
    tail: oracle/discriminator.py takes the softmax in f32 (6e-8 per probability), hence 1e-6 and not 1e-12."""
    x = _tokens(3, 50, 8)
    mask = torch.ones(3, 50, dtype=torch.long)
    mask[1, 33:] = 0
    net = _airl(N_CLASS, 5, (512, 10, 8))
    P = _f64(net)
    stats = (P["score_classifier.1.running_mean"], P["score_classifier.1.running_var"])
    with torch.no_grad():
        for bs in (False, True):
            got, _, _ = disc_f64.airl_forward(P, stats, x, mask, 10, 8, 25, bs)
            want = odisc.airl_forward(P, x, mask, 10, 8, 50, batch_stats=bs)
            assert (got - want).abs().max().item() < 1e-6
        P = _f64(_reward(N_CLASS, 6, (512, 12, 8)))
        got, _ = disc_f64.ppo_token_forward(P, x, mask, 12, 8, 256)
        assert (got - odisc.ppo_reward_forward(P, x, mask, 12, 8, 512)).abs().max().item() < 1e-6


def _qkv(B, L, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, 3, H, 64, generator=g, dtype=torch.float64)


def test_attention_mask_keeps_one_minus_p_of_the_band_and_nothing_outside():
    """v = identity rows makes the output row i the dropped probabilities Pd_i.: zero outside the band and on masked keys,
    kept with frequency 1 - p inside (n = 2 x 4 x 1 930 flags: 4 sigma of a binomial), kept ones scaled by keep_scale."""
    B, L, H, w, p = 2, 64, 4, 20, 0.1
    qkv = _qkv(B, L, H, 3)
    qkv[:, :, 2] = torch.eye(64, dtype=torch.float64)[None, :, None, :]
    mask = torch.ones(B, L)
    mask[1, 50:] = 0
    idx = torch.arange(L)
    band = ((idx[:, None] - idx[None, :]).abs() <= w)[None, None] & (mask != 0)[:, None, None, :] \
        & (mask != 0)[:, None, :, None]
    band = band.expand(B, H, L, L)
    p0, _ = disc_f64.band_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, w)
    pd, _ = disc_f64.band_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, w, p, 12345)
    p0, pd = (t.view(B, L, H, L).permute(0, 2, 1, 3) for t in (p0, pd))
    assert (p0[~band] == 0).all() and (pd[~band] == 0).all() and (p0[band] > 0).all()
    kept = pd[band] != 0
    n = kept.numel()
    assert abs(kept.double().mean().item() - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5
    assert torch.allclose(pd[band][kept], p0[band][kept] * dropout.keep_scale(p), rtol=1e-14, atol=0)
    # the flags are the kernels' own: index ((b H + h) L + i) L + j
    flags = dropout.keep_flags(12345, p, torch.arange(B * H * L * L).view(B, H, L, L))
    assert torch.equal(pd != 0, flags & band)


def test_mean_over_seeds_approaches_the_output_without_dropout():
    """E[Pd] = P: the mean output over 64 seeds deviates from the p = 0 output by 1 / 8 of what one seed does (1.5x
    allowed: the 64 x 2 x 50 x 512 elements make both figures sharp)."""
    qkv = _qkv(2, 50, 8, 4)
    mask = torch.ones(2, 50)
    mask[0, 40:] = 0
    args = (qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, 25)
    o0, _ = disc_f64.band_attention(*args)
    outs = torch.stack([disc_f64.band_attention(*args, 0.1, 1000 + 7 * s)[0] for s in range(64)])
    one = (outs - o0).square().sum((1, 2, 3)).mean().sqrt().item()
    mean = (outs.mean(0) - o0).norm().item()
    print("deviation of one seed %.4f, of the mean of 64 %.4f (of |out| = %.4f)" % (one, mean, o0.norm().item()))
    assert one > 0.05 * o0.norm().item()
    assert mean < 1.5 * one / 8


def test_band_attention_gradcheck_with_mask_and_dropout():
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(2, 7, 2, 4, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(3))
    mask = torch.ones(2, 7)
    mask[0, 5:] = 0
    mask[1, 0] = 0
    fn = lambda q, k, v: disc_f64.band_attention(q, k, v, mask, 2, 0.25, 77)[0]       # noqa: E731
    assert torch.autograd.gradcheck(fn, (q, k, v), eps=1e-6, atol=1e-7)
    lse = lambda q, k: torch.nan_to_num(disc_f64.band_attention(q, k, v, mask, 2)[1], posinf=0.0)   # noqa: E731
    assert torch.autograd.gradcheck(lse, (q, k), eps=1e-6, atol=1e-7)


def test_rows_without_an_admissible_key_are_zero_and_carry_no_gradient():
    qkv = _qkv(3, 20, 2, 5).requires_grad_(True)
    mask = torch.ones(3, 20)
    mask[1] = 0                                                     # a window masked entirely
    mask[2, :] = 0
    mask[2, 4] = 1                                                  # a single valid key
    out, lse = disc_f64.band_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, 3)
    assert (out[1] == 0).all() and torch.isinf(lse[1]).all()
    assert torch.equal(out[2, 4].view(2, 64), qkv[2, 4, 2].detach())
    assert (lse[2, :, 4] - (qkv[2, 4, 0].detach() * qkv[2, 4, 1].detach()).sum(-1) / 8).abs().max().item() < 1e-14
    assert (out[2, :4] == 0).all() and (out[2, 5:] == 0).all()
    out.square().sum().backward()
    assert torch.isfinite(qkv.grad).all() and (qkv.grad[1] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# the teeth of tests/test_disc_f64_gpu.py: how far each wrong ingredient moves the f64 result
# ----------------------------------------------------------------------------------------------------------------------
def _row_rel(a, b, rows):
    """Per row of (.., rows-of-64..) tensors viewed as (-1, rows): |a - b| / max(|b|, rms |b| / 4)."""
    a, b = a.reshape(-1, rows), b.reshape(-1, rows)
    nb = b.norm(dim=1)
    return (a - b).norm(dim=1) / torch.maximum(nb, nb.square().mean().sqrt() / 4)


def swapped_flags(L):
    """keep_flags with the query and the key index of ((b H + h) L + i) L + j exchanged."""
    def keep(seed, p, idx):
        j, i, bh = idx % L, (idx // L) % L, idx // (L * L)
        return dropout.keep_flags(seed, p, (bh * L + j) * L + i)
    return keep


def test_attention_teeth_move_the_f64_rows_beyond_the_bf16_kernel_bound():
    """At the product shape (L = 50, w = 25, H = 8), p = 0.1, a padded tail and a hole: the rows a wrong window, a shifted
    key mask or swapped keep flags feed move, in the rms over those rows (the GPU test's teeth measure: a far key that a wider window admits may carry
    next to no probability in one row, never in most), by at least 2 x 5 x the bound of the bf16 MFMA kernel's rows,
    4 sqrt(2) 2^-9 / sqrt(3) = 6.4e-3 (the largest kernel-level forward bound; the f32 one is 5 000 times smaller)."""
    bound = 4 * 2 ** 0.5 * 2.0 ** -9 / 3 ** 0.5
    B, L, H, w, p, seed = 4, 50, 8, 25, 0.1, 4242
    qkv = _qkv(B, L, H, 6)
    mask = torch.ones(B, L)
    mask[1, 37:] = 0
    mask[2, 11] = 0
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    good, _ = disc_f64.band_attention(q, k, v, mask, w, p, seed)
    idx = torch.arange(L)
    shifted = torch.roll(mask, 1, 1)
    fed = {
        "window + 1": ((idx[:, None] - idx[None, :]).abs() == w + 1).any(1)[None, :, None].expand(B, L, H)
        & (mask != 0)[:, :, None],
        "key mask shifted by one": ((mask != shifted).any(1) & True)[:, None, None].expand(B, L, H)
        & (mask != 0)[:, :, None] & (shifted != 0)[:, :, None],
        "keep flags with i and j swapped": (mask != 0)[:, :, None].expand(B, L, H),
    }
    wrong = {
        "window + 1": disc_f64.band_attention(q, k, v, mask, w + 1, p, seed)[0],
        "key mask shifted by one": disc_f64.band_attention(q, k, v, shifted, w, p, seed)[0],
        "keep flags with i and j swapped": disc_f64.band_attention(q, k, v, mask, w, p, seed, keep=swapped_flags(L))[0],
    }
    for label, bad in wrong.items():
        r = _row_rel(bad, good, 64).view(B, L, H)
        rows = fed[label]
        if label == "key mask shifted by one":                     # rows whose band holds a key that changed sides
            changed = (mask != shifted)
            near = torch.stack([changed[:, max(0, i - w):i + w + 1].any(1) for i in range(L)], 1)
            rows = rows & near[:, :, None]
        assert rows.any()
        print("%s: %d rows fed, moved by %.3f .. %.3f (needed %.3f)" % (label, rows.sum().item(), r[rows].min().item(),
                                                                      r[rows].max().item(), ROOM * TEETH * bound))
        rms = r[rows].square().mean().sqrt().item()
        print("    rms %.3f, rows beyond %.3f: %.0f %%" % (rms, TEETH * bound, 100 * (r[rows] >= TEETH * bound).double().mean()))
        assert rms >= ROOM * TEETH * bound, label


@pytest.mark.timeout(300)
def test_hidden_dropout_seed_tooth_is_resolved_in_f32_and_not_in_bf16():
    """The attention-output dropout of the LAST layer drawn with the output-dense seed, AIRL at repo dims, 4 x 50, p = 0.1:
    the hidden rows move by a few per cent.  That is thousands of times the f32 bound of the GPU test and BELOW 5 x its
    bf16 bound for ten layers (4 sqrt(136) 2^-9 / sqrt(3) = 5.3e-2): the GPU test therefore asks this tooth of the f32
    runs only, and says so."""
    x = _tokens(4, 50, 10)
    mask = torch.ones(4, 50, dtype=torch.long)
    mask[2, 41:] = 0
    P = _f64(_airl(N_CLASS, 5, (512, 10, 8)))
    seeds = [900 + 13 * i for i in range(disc_f64.n_seeds(10))]
    bad = list(seeds)
    bad[-2] = seeds[-1]
    with torch.no_grad():
        h = disc_f64.hidden(P, x, mask, 10, 8, 25, 0.1, 0.1, seeds)
        hb = disc_f64.hidden(P, x, mask, 10, 8, 25, 0.1, 0.1, bad)
    r = _row_rel(hb, h, 512)
    f32_bound = 4 * 5700 ** 0.5 * 2.0 ** -24
    bf16_bound = 4 * 136 ** 0.5 * 2.0 ** -9 / 3 ** 0.5
    print("rows moved by %.4f .. %.4f; 5 x f32 bound %.2e, 5 x bf16 bound %.3f" % (
        r.min().item(), r.max().item(), TEETH * f32_bound, TEETH * bf16_bound))
    assert r.min().item() >= ROOM * TEETH * f32_bound
    assert r.max().item() < TEETH * bf16_bound

"""CPU pin of oracle/heads_rl_f64.py, the reference, inputs, measures and bounds of tests/test_heads_f64_gpu.py and
tests/test_rl_f64_gpu.py: the f64 forms equal torch's own functions and oracle/rl_math.py, every input maker has the
properties it promises, the share of skipped argmax pairs is below 0.1 %, torch's f32 chain on the CPU (a stand-in for the
kernels: the same formulas, other summation orders) stays inside every bound, and every "teeth" mutant falls outside its
bound by TEETH = 5.  No kernel runs here.  Run with -s for the figures."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import heads_rl_f64 as o
from oracle import rl_math

BF16, F32 = torch.bfloat16, torch.float32
EDGES = (9, 8, 7, 1, 65, 64, 63)
SLOTS = (1, 63, 64, 65, 128, 129, 255)


def emulate(logits, n_class, target, mask, w=None, out_dtype=F32):
    """The kernels' formulas in torch f32 on the CPU -> loss sums, argmax, pmax, probs, (p - onehot) * w."""
    x = logits.float()
    off = o.offsets(n_class)
    t = o.clamp_targets(target, n_class)
    loss, am, pm, pr, dl = [], [], [], [], []
    for f, n in enumerate(n_class):
        seg = x[:, off[f]:off[f] + n]
        mx = seg.max(1).values
        e = torch.exp(seg - mx[:, None])
        s = e.sum(1)
        p = e / s[:, None]
        nll = (torch.log(s) + mx) - seg.gather(1, t[:, f:f + 1])[:, 0]
        loss.append((mask * nll).sum())
        am.append(o.first_argmax(p))
        pm.append(p.max(1).values)
        pr.append(p)
        if w is not None:
            dl.append(((e * (1.0 / s)[:, None] - F.one_hot(t[:, f], n).float()) * w[:, f:f + 1]).to(out_dtype))
    return torch.stack(loss), torch.stack(am, 1), torch.stack(pm, 1), torch.cat(pr, 1), (torch.cat(dl, 1) if dl else None)


# ----------------------------------------------------------------------------------------------------------------------
# heads: the reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_class,ld", [(o.REPO, 384), (EDGES, 256), (SLOTS, 768)])
def test_heads_reference_equals_torch(n_class, ld):
    rows = 37
    x = o.make_logits("x3", rows, n_class, ld).double().requires_grad_(True)
    tgt = o.make_targets(rows, n_class, out_of_range=True)
    mask = o.make_mask("p80", rows).double()
    ref = o.heads_reference(x.detach(), n_class, tgt)
    off = o.offsets(n_class)
    tc = o.clamp_targets(tgt, n_class)
    assert ((tgt < 0) | (tgt >= torch.tensor(n_class))).any() and (tc >= 0).all() and (tc < torch.tensor(n_class)).all()
    coef = torch.rand(len(n_class), dtype=torch.float64) + 0.5
    g = torch.randn(rows, len(n_class), dtype=torch.float64)
    total = 0
    for f, n in enumerate(n_class):
        seg = x[:, off[f]:off[f] + n]
        ls = torch.log_softmax(seg, 1)
        nll = F.nll_loss(ls, tc[:, f], reduction="none")
        assert (nll.detach() - ref["nll"][:, f]).abs().max().item() < 1e-12 * ref["scale"][:, f].max().item()
        assert (ls.exp().detach() - ref["p"][:, off[f]:off[f] + n]).abs().max().item() < 1e-14
        assert torch.equal(ref["argmax"][:, f], o.first_argmax(ls.detach()))
        total = total + (nll * mask).sum() * coef[f]
    (gx,) = torch.autograd.grad(total, x)
    gx = torch.nan_to_num(gx)
    dl, w = o.ce_dlogits(ref, n_class, mask, coef, ld)
    assert (dl - gx).abs().max().item() < 1e-14 and (dl[:, off[-1]:] == 0).all()
    lp = torch.stack([torch.log_softmax(x[:, off[f]:off[f] + n], 1).gather(1, tc[:, f:f + 1])[:, 0] for f, n in enumerate(n_class)], 1)
    (gx,) = torch.autograd.grad((lp * g).sum(), x)
    assert (o.logp_dlogits(ref, n_class, g, ld) - torch.nan_to_num(gx)).abs().max().item() < 1e-14
    assert torch.allclose(o.loss_sums(ref, mask), (ref["nll"] * mask[:, None]).sum(0))


def test_first_argmax_takes_the_lowest_tied_index():
    p = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, 1.0, 2.0, 2.0]])
    assert o.first_argmax(p).tolist() == [1, 0, 2]


# ----------------------------------------------------------------------------------------------------------------------
# heads: the input makers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_input_makers_keep_their_promises(dtype):
    rows, n_class, ld = 64, SLOTS, 768
    off = o.offsets(n_class)
    x3 = o.make_logits("x3", rows, n_class, ld, dtype)
    assert x3.dtype == dtype and x3.shape == (rows, ld) and torch.isnan(x3[:, off[-1]:].float()).all()
    assert not torch.isnan(x3[:, :off[-1]].float()).any() and 2.5 < x3[:, :off[-1]].float().std().item() < 3.5
    pk = o.make_logits("peaked", rows, n_class, ld, dtype)
    tg = o.make_targets(rows, n_class, logits=pk)
    ref = o.heads_reference(pk, n_class, tg)
    assert (ref["mx"] == 50).all()
    on_peak = ref["xt"] == 50
    big = [f for f, n in enumerate(n_class) if n >= 63]
    assert on_peak[:, big].any() and (~on_peak[:, big]).any() and (ref["nll"][~on_peak] > 40).all()
    assert (ref["nll"][on_peak] < 1e-15).all()
    sh = o.make_logits("shifted", rows, n_class, ld, dtype)
    assert sh[:, :off[-1]].float().min().item() > 290
    bad = o.heads_reference(sh, n_class, tg, mutant="nomax")
    assert not torch.isfinite(bad["nll"]).any(), "exp(300) overflows f32: the max subtraction is needed"
    assert torch.isfinite(o.heads_reference(sh, n_class, tg)["nll"]).all()
    ti = o.make_logits("ties", rows, n_class, ld, dtype)
    ref = o.heads_reference(ti, n_class)
    seen = set()
    for f, n in enumerate(n_class):
        seg = ti[:, off[f]:off[f] + n].double()
        for r in range(rows):
            cols = torch.nonzero(seg[r] == seg[r].max())[:, 0].tolist()
            assert ref["argmax"][r, f].item() == cols[0]
            if n > 1:
                assert len(cols) >= 2 or n - cols[0] == 1, (r, f, cols)
            if r % 4 == 3:
                assert cols == list(range(n))
                seen.add("all")
            elif r % 4 == 1 and n >= 9:
                assert cols == [7, 8]
                seen.add("unroll")
            elif r % 4 == 2 and n >= 65:
                assert cols[1] - cols[0] == 64
                seen.add("slot")
            elif len(cols) > 1:
                assert cols[0] // 8 == cols[-1] // 8 and cols == list(range(cols[0], cols[-1] + 1))
                seen.add("group")
    assert seen == {"all", "unroll", "slot", "group"}
    assert (ref["gap"] == 0)[:, [f for f, n in enumerate(n_class) if n > 2]].float().mean().item() > 0.9
    t5 = o.make_targets(rows, n_class, out_of_range=True)
    assert (t5 == -5).any() and all((t5[:, f] == n + 3).any() for f, n in enumerate(n_class))
    for kind, ones in (("ones", rows), ("last", 1), ("tail", 32)):
        m = o.make_mask(kind, rows)
        assert m.sum().item() == ones and m[-1] == 1
    assert o.make_mask("tail", 33).tolist() == [0.0] * 32 + [1.0] and 0.6 < o.make_mask("p80", 1000).mean().item() < 0.95


def test_argmax_skip_share_is_small():
    """f32 randn x 3 at 32 801 rows, class counts 7 .. 256: pairs whose top two softmax values are closer than 1e-5 (relative)
    are about 1e-5 of all; bf16 inputs have exact ties (not skipped) or gaps far above 1e-5."""
    n_class = (7, 9, 63, 65, 129, 255, 256)
    for dtype in (F32, BF16):
        x = o.make_logits("x3", 32801, n_class, sum(n_class), dtype)
        ref = o.heads_reference(x, n_class)
        skip = ((ref["gap"] > 0) & (ref["gap"] < o.GAP)).double().mean(0)
        ties = (ref["gap"] == 0).double().mean(0)
        print("    %s skipped share per attribute %s  exact ties %s" % (dtype, skip.tolist(), ties.tolist()))
        assert skip.max().item() <= o.SKIP_SHARE
        if dtype == BF16:
            assert skip.max().item() == 0 and ties.max().item() < 0.03
        else:
            assert skip.max().item() < 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# heads: bounds and teeth
# ----------------------------------------------------------------------------------------------------------------------
def test_bound_pieces():
    assert abs(o.LOG2E_C - 0.225) < 0.01
    assert o.n_sum(256, True) == 256 / 3 and o.n_sum(65, True, 1363) == 1363 / 3 and o.n_sum(256, False) == 3 + 6 and o.n_sum(1, False) == 0
    assert o.n_sum(65, False) == 1 + 6 and o.n_sum(7, False) == 3
    # tiled: one tile per block up to 32 768 rows, two in the first blocks above; wave: two rows per wave above 4 096
    assert o.tree_count(32801, True) - o.tree_count(32768, True) == pytest.approx(1 / 6)
    assert o.tree_count(4101, False) - o.tree_count(4096, False) == pytest.approx(1 / 6)
    assert o.heads_blocks(1) == 1 and o.heads_blocks(4097) == 1024 and o.heads_blocks(5) == 2


@pytest.mark.parametrize("kind", o.KINDS)
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n_class,ld,tiled", [(o.REPO, 384, True), (SLOTS, 768, False), (EDGES, 256, True)])
def test_f32_chain_is_inside_every_heads_bound(kind, dtype, n_class, ld, tiled):
    rows = 1031
    bf = dtype == BF16
    x = o.make_logits(kind, rows, n_class, ld, dtype)
    tgt = o.make_targets(rows, n_class, out_of_range=True, logits=x if kind == "peaked" else None)
    mask = o.make_mask("p80", rows)
    coef = torch.rand(len(n_class)) + 0.5
    w = mask[:, None] * coef[None, :]
    loss, am, pm, pr, dl = emulate(x, n_class, tgt, mask, w, dtype)
    ref = o.heads_reference(x, n_class, tgt)
    r = o.heads_ratios(ref, n_class, tiled, bf, mask, loss, pmax=pm, probs=pr)
    want, wd = o.ce_dlogits(ref, n_class, mask, coef, sum(n_class))
    r["dlogits"], exact = o.rows_ratio(dl, want, wd.abs(), o.dlogits_bound(ref, n_class, tiled, bf, 2), n_class)
    bad, share = o.argmax_check(am, ref)
    print("    %-8s %-5s %-28s %s  skipped %.1e" % (kind, "bf16" if bf else "f32", n_class[:3], "  ".join("%s %.2f" % kv for kv in r.items()), share))
    assert exact and bad == 0 and share <= o.SKIP_SHARE
    assert all(v <= 1 for v in r.values()), r


def test_heads_mutants_fall_outside():
    rows, n_class, ld = 1031, o.REPO, 384
    mask = o.make_mask("p80", rows)
    tgt = o.make_targets(rows, n_class)
    x = o.make_logits("x3", rows, n_class, ld)
    ref = o.heads_reference(x, n_class, tgt)
    b, D = o.loss_bound(ref, n_class, mask, True, False)
    good = o.loss_sums(ref, mask)
    for name, mut in (("target+1", o.loss_sums(o.heads_reference(x, n_class, tgt, mutant="target+1"), mask)),
                      ("mask ignored", o.loss_sums(ref, None)),
                      ("last tile dropped", o.loss_sums(ref, o.make_mask("ones", rows), drop_from=1024) - o.loss_sums(ref, o.make_mask("ones", rows)) + good)):
        m = o.miss(mut, good, D * b)
        print("    teeth %-18s %.1f x the bound" % (name, m))
        assert m >= o.TEETH
    sh = o.make_logits("shifted", rows, n_class, ld)
    assert o.miss(o.loss_sums(o.heads_reference(sh, n_class, tgt, mutant="nomax"), mask),
                  o.loss_sums(o.heads_reference(sh, n_class, tgt), mask), D * b) == float("inf")
    ti = o.make_logits("ties", rows, n_class, ld)
    a, z = o.heads_reference(ti, n_class), o.heads_reference(ti, n_class, mutant="lastmax")
    assert (a["argmax"] != z["argmax"]).float().mean().item() > 0.9 and o.argmax_check(z["argmax"], a)[0] > 0
    # coef not divided by sum(mask): every live row of dlogits is off by the factor sum(mask)
    coef = torch.ones(len(n_class))
    want, w = o.ce_dlogits(ref, n_class, mask, coef / mask.sum(), ld)
    mut, _ = o.ce_dlogits(ref, n_class, mask, coef, ld)
    r, _ = o.rows_ratio(mut, want, w.abs(), o.dlogits_bound(ref, n_class, True, True, 2), n_class)
    assert r >= o.TEETH


# ----------------------------------------------------------------------------------------------------------------------
# RL: the f64 forms equal oracle/rl_math.py where it is defined
# ----------------------------------------------------------------------------------------------------------------------
def _fused(ys):
    return torch.cat(ys, -1)


def test_rl_forms_equal_rl_math():
    g = torch.Generator().manual_seed(1)
    B, T, NA = 4, 50, 25
    ys = [torch.randn(B, T, n, generator=g, dtype=torch.float64) * 2 for n in o.REPO]
    ps = [torch.softmax(y, -1) for y in ys]
    ids = torch.stack([p.argmax(-1) for p in ps], -1)
    probs = _fused(ps)
    a0, _ = o.rollout_gather(ids[:1], None, o.REPO, NA, 0)
    assert torch.equal(a0[0], rl_math.dqn_choose_action([y[:1] for y in ys], NA))
    a1, l1 = o.rollout_gather(ids[:1], probs[:1], o.REPO, NA, 1)
    wa, wl = rl_math.ppo_choose_action([y[:1] for y in ys], NA)
    assert torch.equal(a1[0], wa) and (l1[0] - wl).abs().max().item() < 1e-12
    a2, l2 = o.rollout_gather(ids, probs, o.REPO, NA, 2)
    wa, wl = rl_math.ppo_select_update(ys, NA)
    assert torch.equal(a2[-1], wa) and (l2[-1] - wl).abs().max().item() < 1e-12
    # returns / advantages (rl_math builds its returns in f32)
    rewards, values = torch.rand(30, generator=g), torch.randn(30, 1, generator=g)
    for norm in (True, False):
        wr = rl_math.ppo_returns([x for x in rewards], 0.99, normalize=norm)
        wa = rl_math.ppo_advantages(wr, values, normalize=norm)
        ret, adv, V = o.ppo_returns_adv(rewards, values, 0.99, norm)
        assert (ret - wr[:, 0]).abs().max().item() < 2e-6 * wr.abs().max().item()
        assert (adv - wa[:, 0]).abs().max().item() < 4e-6 * wa.abs().max().item()
    assert o.ppo_returns_adv(torch.tensor([1.0, 2.0, 3.0]), torch.zeros(3), 0.5, False)[0].tolist() == [4.25, 2.5, 1.0]
    # surrogate
    new = (torch.randn(NA, 6, generator=g, dtype=torch.float64) * 0.3 - 0.5).requires_grad_(True)
    old = (torch.randn(30, NA, 6, generator=g) * 1.2 - 0.8).long()
    adv = torch.randn(30, 1, generator=g, dtype=torch.float64)
    want = rl_math.ppo_policy_loss(new, old, adv, 0.2)
    (gw,) = torch.autograd.grad(want, new)
    ref = o.ppo_policy_loss(new.detach(), old, adv, 0.2)
    assert abs(ref["loss"].item() - want.item()) < 1e-14 and (ref["grad"] - gw).abs().max().item() < 1e-15
    # TD loss
    B, T, NA = 5, 12, 7
    y = [(torch.randn(B, T, n, generator=g, dtype=torch.float64) * 2).requires_grad_(True) for n in o.REPO]
    yt = [torch.randn(B, T, n, generator=g, dtype=torch.float64) * 2 for n in o.REPO]
    action = torch.stack([torch.randint(0, n, (B, NA), generator=g) for n in o.REPO], -1)
    reward, done = torch.rand(B, 1, generator=g, dtype=torch.float64), torch.randint(0, 2, (B, 1), generator=g)
    total, losses = rl_math.dqn_td_loss(y, yt, action, reward, done, o.f32v(0.9), NA)
    gw = torch.rand(6, dtype=torch.float64) + 0.5
    gy = torch.autograd.grad(sum(l * w for l, w in zip(losses, gw)), y)
    ref = o.dqn_td(_fused([t.detach() for t in y]), _fused(yt), action, reward, done, o.REPO, 0.9)
    assert (ref["mse"] - torch.stack(losses).detach()).abs().max().item() < 1e-13
    dy, bound = o.dqn_td_dy(ref, action, o.REPO, gw, (B, T, sum(o.REPO)))
    assert (dy - _fused(gy)).abs().max().item() < 1e-14 and (dy[1:] == 0).all() and (dy[0, B:] == 0).all()
    assert ((bound > 0) == (dy[0] != 0)).all()
    assert (ref["dq"] - 2 * ref["d"] / (B * NA * 6)).abs().max().item() == 0


# ----------------------------------------------------------------------------------------------------------------------
# RL: bounds and teeth
# ----------------------------------------------------------------------------------------------------------------------
def _returns_f32(rewards, values, gamma, normalize):
    r = rewards.float()
    E = r.numel()
    ret = torch.zeros(E)
    R = torch.zeros(())
    gm = torch.tensor(gamma, dtype=F32)
    for t in range(E):
        R = r[t] + R * gm
        ret[E - 1 - t] = R
    if normalize:
        ret = (ret - ret.mean()) / ret.std()
    adv = ret - values.float()
    if normalize:
        adv = (adv - adv.mean()) / adv.std()
    return ret, adv


@pytest.mark.parametrize("E", [2, 63, 64, 65, 1000, 8192])
@pytest.mark.parametrize("gamma", [0.5, 0.99, 1.0])
@pytest.mark.parametrize("normalize", [True, False])
def test_f32_chain_is_inside_the_returns_bound(E, gamma, normalize):
    g = torch.Generator().manual_seed(E)
    rewards, values = torch.rand(E, generator=g), torch.randn(E, generator=g)
    ret, adv, V = o.ppo_returns_adv(rewards, values, gamma, normalize)
    br, ba = o.ppo_returns_adv_bounds(rewards, values, gamma, normalize)
    gr, ga = _returns_f32(rewards, values, gamma, normalize)
    rr, ra = o.miss(gr, ret, br), o.miss(ga, adv, ba)
    print("    E %5d gamma %.2f norm %d  returns %.2f  adv %.2f  (bound / |ref| max %.1e)" % (E, gamma, normalize, rr, ra, (br / ret.abs().clamp_min(1e-30)).median().item()))
    assert rr <= 1 and ra <= 1
    for mutant in ("textbook",) + (("biased",) if normalize and E <= 1000 else ()):
        mr, ma, _ = o.ppo_returns_adv(rewards, values, gamma, normalize, mutant=mutant)
        if E >= 63:
            assert o.miss(mr, ret, br) >= o.TEETH, mutant


def test_returns_bound_grows_with_E():
    g = torch.Generator().manual_seed(0)
    r, v = torch.rand(8192, generator=g), torch.randn(8192, generator=g)
    rel = []
    for E in (64, 1000, 8192):
        ret, _, _ = o.ppo_returns_adv(r[:E], v[:E], 1.0, False)
        rel.append((o.ppo_returns_adv_bounds(r[:E], v[:E], 1.0, False)[0][0] / ret[0]).item())
    assert rel[0] < rel[1] < rel[2] and rel[2] < 1e-4


def ppo_case(E, NA, A, seed=6):
    """new (NA, A), old (E, NA, A) int64 through .long(), adv (E) of both signs; ratios on both sides of both clip edges."""
    g = torch.Generator().manual_seed(seed)
    new = torch.randn(NA, A, generator=g) * 0.3 - 0.5
    old = (torch.randn(E, NA, A, generator=g) * 1.2 - 0.8).long()
    adv = torch.randn(E, generator=g)
    if E == 1:
        adv = -adv.abs()
    return new, old, adv


@pytest.mark.parametrize("E,NA,A", [(1, 1, 1), (30, 43, 6), (64, 512, 6)])
def test_f32_chain_is_inside_the_surrogate_bound(E, NA, A):
    new, old, adv = ppo_case(E, NA, A)
    ref = o.ppo_policy_loss(new, old, adv, 0.2)
    if E > 1:
        r = ref["ratio"]
        assert (r < 0.8).any() and ((r > 0.8) & (r < 1.2)).any() and (r > 1.2).any() and (adv > 0).any() and (adv < 0).any()
        assert (ref["grad"] != 0).any()
    lb, gb = o.ppo_policy_loss_bounds(ref)
    nl = new.clone().requires_grad_(True)
    got = rl_math.ppo_policy_loss(nl, old, adv.view(E, 1), 0.2)
    (gg,) = torch.autograd.grad(got, nl)
    rl_, rg = o.miss(got.detach(), ref["loss"], lb), o.miss(gg, ref["grad"], gb.clamp_min(1e-300))
    print("    surrogate E %d NA %d A %d  loss %.2f  grad %.2f" % (E, NA, A, rl_, rg))
    assert rl_ <= 1 and rg <= 1
    if E > 1:
        mut = o.ppo_policy_loss(new, old, adv, 0.2, mutant="ratioA")
        assert o.miss(mut["loss"], ref["loss"], lb) >= o.TEETH


def td_case(B, T, NA, n_class, done="mixed", seed=7):
    """Fused logits (B, T, W) whose target-net rows repeat their per-position maxima (values rounded to 1 / 4: ties in the
    top-k), actions in range with duplicates, rewards, done flags."""
    g = torch.Generator().manual_seed(seed)
    W = sum(n_class) + (-sum(n_class)) % 64
    y = torch.randn(B, T, W, generator=g) * 2
    yt = (torch.randn(B, T, W, generator=g) * 8).round() / 4
    action = torch.stack([torch.randint(0, n, (B, NA), generator=g) for n in n_class], -1)
    if NA > 1:
        action[:, 1] = action[:, 0]                                                # a duplicate in every (j, f)
    reward = torch.rand(B, generator=g)
    dn = {"mixed": torch.randint(0, 2, (B,), generator=g).float(), "zero": torch.zeros(B), "one": torch.ones(B)}[done]
    return y, yt, action, reward, dn


@pytest.mark.parametrize("B,T,NA", [(1, 1, 1), (30, 50, 25), (65, 65, 65), (5, 129, 70)])
@pytest.mark.parametrize("n_class", [o.REPO, (5,)])
def test_f32_chain_is_inside_the_td_bound(B, T, NA, n_class):
    A = len(n_class)
    y, yt, action, reward, dn = td_case(B, T, NA, n_class)
    ref = o.dqn_td(y, yt, action, reward, dn, n_class, 0.9)
    if T > 1:
        nxt = yt[:, :, :n_class[0]].max(2).values
        assert any(len(set(row.tolist())) < T for row in nxt), "ties among the next-state maxima"
    mb, qb = o.dqn_td_bounds(ref, B, NA, A)
    off = o.offsets(n_class)
    ys = [y[..., off[f]:off[f] + n].clone().requires_grad_(True) for f, n in enumerate(n_class)]
    losses = []
    for f, n in enumerate(n_class):                                                 # rl_math.dqn_td_loss for any A, in f32
        q = ys[f].gather(2, action[:, :, f].unsqueeze(0)).squeeze(0)
        top, _ = yt[..., off[f]:off[f] + n].max(2)[0].topk(NA, dim=1)
        losses.append(F.mse_loss(q, reward.view(B, 1) + 0.9 * (1 - dn.view(B, 1)) * top))
    gw = torch.rand(A) + 0.5
    gy = torch.autograd.grad(sum(l * w for l, w in zip(losses, gw)), ys)
    rm = o.miss(torch.stack(losses).detach(), ref["mse"], mb)
    dy, bound = o.dqn_td_dy(ref, action, n_class, gw, y.shape)
    got = torch.zeros_like(dy)
    got[..., :off[-1]] = torch.cat(gy, -1)
    live = bound > 0
    rd = o.miss(got[0][live], dy[0][live], bound[live])
    print("    td (%d, %d, %d) A %d  mse %.2f  dy %.2f" % (B, T, NA, A, rm, rd))
    assert rm <= 1 and rd <= 1 and (got[0][~live] == 0).all() and (got[1:] == 0).all()
    if B > 1:
        for mutant in ("ascending", "batch_j"):
            mut = o.dqn_td(y, yt, action, reward, dn, n_class, 0.9, mutant=mutant)
            assert o.miss(mut["dq"], ref["dq"], qb) >= o.TEETH, mutant

"""GPU: the RL arithmetic kernels (csrc/rl.hip) past the first wrap of every loop, element by element against the f64 forms of
oracle/heads_rl_f64.py (pinned, with every bound below and against oracle/rl_math.py, by tests/test_oracle_heads_rl_f64_cpu.py).

cwlt_ppo_returns_adv   one wave striding over E: E = 2, 63, 64, 65, 1 000, 8 192; gamma 0.5, 0.99, 1.0; normalised or not.  The
                       bound grows with E through the serial recursion and passes through the two normalisations.
cwlt_ppo_policy_loss   (E, NA, A) = (1, 1, 1), (30, 43, 6) (KF = 258: the second trip of the 256-thread loop), (64, 512, 6);
                       advantages of both signs, stored log-probs through .long(), ratios on both sides of both clip edges;
                       loss and gradient per element, the gradient also through autograd with an upstream factor.
cwlt_dqn_td_fwd / bwd  through rl_ops.dqn_td_mse: B = T and NA = T on and next to a power of two, npad from 64 to 1 024 (the
                       bitonic network's pair loop runs up to 8 times per lane, padding beside real values), NA > 64; target
                       logits with repeated maxima (ties in the top-k); done all 0, all 1, mixed; 1 and 8 attributes.
cwlt_rollout_gather    the edges: mode 0 at NA = T, modes 1 and 2 at NA = T - 1, R = 3, T = 2.
Action indices and ids stay inside their attribute (the precondition stated in include/cwlt.h).  Refusals are argument checks
that return before any launch (rl.hip's entry points, read before they were added here).

Teeth (TEETH = 5): the textbook (reversed) return recursion, the biased std, surrogate 1 as ratio x A, the top-k ascending,
the q gather from batch element j instead of 0.  Measured on an MI355X: profiles/heads_rl_f64_ratios.txt.
"""
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import _lib, rl_ops
from oracle import heads_rl_f64 as o

pytestmark = pytest.mark.gpu
N8 = (56, 135, 18, 87, 18, 25, 7, 64)


def say(label, **ratios):
    print("    %-52s %s" % (label, "  ".join("%s %.2f" % kv for kv in ratios.items())))
    assert all(v <= 1 for v in ratios.values()), (label, ratios)


# ----------------------------------------------------------------------------------------------------------------------
# returns and advantages
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("gamma", [0.5, 0.99, 1.0])
@pytest.mark.parametrize("E", [2, 63, 64, 65, 1000, 8192])
def test_returns_and_advantages(cuda, E, gamma, normalize):
    g = torch.Generator().manual_seed(E)
    rewards, values = torch.rand(E, generator=g), torch.randn(E, generator=g)
    ret, adv, _ = o.ppo_returns_adv(rewards, values, gamma, normalize)
    br, ba = o.ppo_returns_adv_bounds(rewards, values, gamma, normalize)
    gr, ga = rl_ops.ppo_returns_adv(rewards.to(cuda), values.to(cuda), gamma, normalize)
    assert gr.shape == (E, 1) and ga.shape == (E, 1)
    gr, ga = gr[:, 0].cpu(), ga[:, 0].cpu()
    inside = {"returns": o.miss(gr, ret, br), "adv": o.miss(ga, adv, ba)}
    say("returns E %5d gamma %.2f %s" % (E, gamma, "norm" if normalize else "raw "), **inside)
    if E == 65:
        for mutant in ("textbook",) + (("biased",) if normalize else ()):
            mr, ma, _ = o.ppo_returns_adv(rewards, values, gamma, normalize, mutant=mutant)
            # the rows the ingredient feeds: every one but a few where the two recursions cross
            m = ((gr.double() - mr).abs() / br).median().item()
            print("    teeth %-9s E 65 gamma %.2f returns  inside %.2f, the mutant %.1f x the bound" % (mutant, gamma, inside["returns"], m))
            assert m >= o.TEETH


def test_returns_refusals(cuda):
    """E < 2 and E > 8 192 are refused by the argument check, before the launch."""
    for E in (1, 8193):
        x = torch.zeros(E, device=cuda)
        with pytest.raises(RuntimeError, match="1001"):
            rl_ops.ppo_returns_adv(x, x, 0.9)


# ----------------------------------------------------------------------------------------------------------------------
# the surrogate
# ----------------------------------------------------------------------------------------------------------------------
def ppo_case(E, NA, A, seed=6):
    g = torch.Generator().manual_seed(seed)
    new = torch.randn(NA, A, generator=g) * 0.3 - 0.5
    stored = torch.randn(E, NA, A, generator=g) * 1.2 - 0.8
    old = stored.long()                                       # the buffer hands stored log-probs back through .long()
    adv = torch.randn(E, generator=g)
    if E == 1:
        adv = -adv.abs()                                      # the one element carries a gradient
    return new, old, adv


@pytest.mark.parametrize("E,NA,A", [(1, 1, 1), (30, 43, 6), (64, 512, 6)])
def test_policy_loss_and_gradient(cuda, E, NA, A):
    new, old, adv = ppo_case(E, NA, A)
    assert old.dtype == torch.int64 and torch.tensor([-0.3, -1.7]).long().tolist() == [0, -1]
    ref = o.ppo_policy_loss(new, old, adv, 0.2)
    if E > 1:
        r = ref["ratio"]
        assert (r < 0.8).any() and ((r > 0.8) & (r < 1.0)).any() and ((r > 1.0) & (r < 1.2)).any() and (r > 1.2).any()
        assert (adv > 0).any() and (adv < 0).any() and NA * A > 256
    lb, gb = o.ppo_policy_loss_bounds(ref)
    _, gba = o.ppo_policy_loss_bounds(ref, autograd=True)
    nd = new.to(cuda).requires_grad_(True)
    loss = rl_ops.ppo_policy_loss(nd, old.to(cuda), adv.to(cuda).view(E, 1), 0.2)
    (loss * 1.75).backward()
    grad_up = nd.grad.cpu()
    # the gradient as the kernel wrote it: an upstream factor of exactly 1
    nd2 = new.to(cuda).requires_grad_(True)
    rl_ops.ppo_policy_loss(nd2, old.to(cuda), adv.to(cuda), 0.2).backward()
    live = gb > 0
    ratios = {"loss": o.miss(loss.detach().cpu(), ref["loss"], lb),
              "grad": o.miss(nd2.grad.cpu()[live], ref["grad"][live], gb[live]),
              "grad x 1.75": o.miss(grad_up[live], 1.75 * ref["grad"][live], 1.75 * gba[live])}
    assert (nd2.grad.cpu()[~live] == 0).all() and (grad_up[~live] == 0).all()
    say("surrogate E %d NA %d A %d (KF %d)" % (E, NA, A, NA * A), **ratios)
    if E > 1:
        mut = o.ppo_policy_loss(new, old, adv, 0.2, mutant="ratioA")
        m = o.miss(loss.detach().cpu(), mut["loss"], lb)
        print("    teeth ratio x A  E %d  loss  inside %.2f, the mutant %.1f x the bound" % (E, ratios["loss"], m))
        assert m >= o.TEETH


# ----------------------------------------------------------------------------------------------------------------------
# the TD loss
# ----------------------------------------------------------------------------------------------------------------------
def td_case(B, T, NA, n_class, done, seed=7):
    """Target-net logits on a grid of 1 / 4 (repeated maxima: ties in the top-k); actions inside their attribute, one
    duplicated in every (j, f)."""
    g = torch.Generator().manual_seed(seed)
    W = sum(n_class) + (-sum(n_class)) % 64
    y = torch.randn(B, T, W, generator=g) * 2
    yt = (torch.randn(B, T, W, generator=g) * 8).round() / 4
    action = torch.stack([torch.randint(0, n, (B, NA), generator=g) for n in n_class], -1)
    if NA > 1:
        action[:, 1] = action[:, 0]
    reward = torch.rand(B, generator=g)
    dn = {"mixed": torch.randint(0, 2, (B,), generator=g).float(), "zero": torch.zeros(B), "one": torch.ones(B)}[done]
    return y, yt, action, reward, dn


@pytest.mark.parametrize("n_class", [(25,), N8], ids=["A1", "A8"])
@pytest.mark.parametrize("B,T,NA,done", [(1, 1, 1, "zero"), (30, 50, 25, "mixed"), (64, 64, 64, "mixed"), (65, 65, 65, "one"),
                                         (30, 100, 100, "zero"), (5, 129, 70, "mixed"), (3, 1000, 512, "mixed"),
                                         (2, 1024, 1024, "mixed")])
def test_td_loss_and_gradient(cuda, B, T, NA, done, n_class):
    A = len(n_class)
    y, yt, action, reward, dn = td_case(B, T, NA, n_class, done)
    n = torch.tensor(n_class)
    assert (action >= 0).all() and (action < n).all(), "the precondition of cwlt_dqn_td_fwd / _bwd"
    if T > 1:
        nxt = yt[:, :, :n_class[0]].max(2).values
        assert all(len(set(row.tolist())) < T for row in nxt), "ties among the next-state maxima"
    yd, ytd, ad, rd, dd = y.to(cuda), yt.to(cuda), action.to(cuda), reward.to(cuda), dn.to(cuda)
    ref = o.dqn_td(yd, ytd, ad, rd, dd, n_class, 0.9)
    mb, qb = o.dqn_td_bounds(ref, B, NA, A)
    gw = (torch.rand(A, generator=torch.Generator().manual_seed(3)) + 0.5).to(cuda)
    yg = yd.clone().requires_grad_(True)
    mse = rl_ops.dqn_td_mse(yg, ytd, ad, rd.view(B, 1), dd.view(B, 1), n_class, 0.9)
    assert mse.shape == (A,)
    (mse * gw).sum().backward()
    torch.cuda.synchronize()
    dy, bound = o.dqn_td_dy(ref, ad, n_class, gw, y.shape)
    got = yg.grad
    live = bound > 0
    assert (got[1:] == 0).all(), "the gradient lives in batch element 0's rows only"
    assert (got[0][~live] == 0).all() and (got[0, B:] == 0).all() and int(live.sum()) > 0
    # dq as the kernel wrote it
    part = torch.empty((B, A), device=cuda)
    dq = torch.empty((B, NA, A), device=cuda)
    rl_ops._call("cwlt_dqn_td_fwd", _lib.dev(yd), _lib.dev(ytd), _lib.int_array(n_class), A, _lib.dev(ad),
                 _lib.dev(rd), _lib.dev(dd), _lib.dev(part), _lib.dev(dq), B, T, NA, y.shape[2], 0.9,
                 _lib.stream_ptr())
    torch.cuda.synchronize()
    inside = {"mse": o.miss(mse.detach(), ref["mse"], mb), "dq": o.miss(dq, ref["dq"], qb),
              "dy": o.miss(got[0][live], dy[0][live], bound[live])}
    say("td (%d, %d, %d) A %d done %s" % (B, T, NA, A, done), **inside)
    if NA > 1:      # duplicates of an action across k are summed: the duplicated pair's two terms land on one element
        j, f = 0, 0
        col = o.offsets(n_class)[f] + int(action[j, 0, f])
        same = (action[j, :, f] == action[j, 0, f]).nonzero()[:, 0]
        assert len(same) >= 2
        want = (ref["d"][j, same, f] * 2 / (B * NA) * gw[f].double()).sum()
        assert abs(got[0, j, col].double() - want) <= bound[j, col]
    if B > 1 and done != "one":
        for mutant in ("ascending", "batch_j"):
            mut = o.dqn_td(yd, ytd, ad, rd, dd, n_class, 0.9, mutant=mutant)
            fed = (mut["dq"] != ref["dq"])
            if mutant == "batch_j":
                fed[0] = False                                           # batch element 0 gathers from itself either way
            m = ((dq.double() - mut["dq"]).abs() / qb)[fed].median().item()
            print("    teeth %-9s td (%d, %d, %d) A %d  dq  inside %.2f, the mutant %.1f x the bound"
                  % (mutant, B, T, NA, A, inside["dq"], m))
            assert m >= o.TEETH


def test_td_refusals(cuda):
    """B > T, NA > T and T > 8 192 are refused by the argument check of cwlt_dqn_td_fwd, before the launch."""
    n_class = (5,)

    def run(B, T, NA):
        y = torch.zeros(B, T, 64, device=cuda)
        a = torch.zeros(B, NA, 1, dtype=torch.int64, device=cuda)
        z = torch.zeros(B, 1, device=cuda)
        return rl_ops.dqn_td_mse(y, y, a, z, z, n_class, 0.9)

    assert run(2, 2, 2).shape == (1,)
    for B, T, NA in ((3, 2, 2), (2, 4, 5), (1, 8193, 1)):
        with pytest.raises(RuntimeError, match="1001"):
            run(B, T, NA)


# ----------------------------------------------------------------------------------------------------------------------
# the gather's edges
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,T,NA", [(0, 50, 50), (1, 50, 49), (2, 50, 49), (0, 2, 2), (1, 2, 1), (2, 2, 1)])
def test_rollout_gather_edges(cuda, mode, T, NA):
    R, n_class = 3, o.REPO
    g = torch.Generator().manual_seed(11)
    ids = torch.stack([torch.randint(0, n, (R, T), generator=g) for n in n_class], -1)
    probs = torch.rand(R, T, sum(n_class), generator=g) * 0.9 + 0.05
    assert (ids >= 0).all() and (ids < torch.tensor(n_class)).all(), "the precondition of cwlt_rollout_gather"
    wa, wl = o.rollout_gather(ids, probs, n_class, NA, mode)
    ga, gl = rl_ops.rollout_gather(ids.to(cuda), None if mode == 0 else probs.to(cuda), n_class, NA, mode)
    assert torch.equal(ga.cpu(), wa) and ga.shape == (R, NA, 6)
    if mode == 0:
        assert gl is None and torch.equal(wa[:, 0], ids[:, 0]) and torch.equal(wa[:, -1], ids[:, T - NA + 1 if NA > 1 else 0])
        return
    if mode == 1:       # tempo and chord read the class chosen at position +idx: up to position NA = T - 1
        assert NA == T - 1
    r = o.miss(gl.cpu(), wl, 8 * o.U32 * wl.abs())
    say("gather mode %d T %d NA %d R %d" % (mode, T, NA, R), logp=r)


def test_rollout_gather_refusals(cuda):
    ids = torch.zeros(1, 4, 6, dtype=torch.int64, device=cuda)
    probs = torch.ones(1, 4, 339, device=cuda)
    for mode, NA in ((0, 5), (1, 4), (2, 4)):
        with pytest.raises(RuntimeError, match="1001"):
            rl_ops.rollout_gather(ids, probs, o.REPO, NA, mode)

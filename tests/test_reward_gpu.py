"""GPU: reward terms in the particles' weights -- the three kernels of csrc/reward.hip one by one, bitwise
against numpy, then generation.generate_particles(reward=) end to end on the small fixture model (128 / 2 layers / 2
heads) and a small AIRL discriminator (128 / 2 layers / 2 heads).

1. cwlt_reward_push: rows 1 / 65 / 257, A 6 / 8, W 1 / 2 / 50, the counter at 0, W - 1 and past the wrap, done flags 0 / 1
   / 2 mixed; only slot counter % W of sentinel-filled rings changes.
2. cwlt_reward_window: filled 1 and W, live flags set in slots >= filled (stale: ignored), flags that are no prefix, a
   row with no live slot (any 0, mask[n, 0] = 1, tokens 0); every output buffer starts from a sentinel.
3. cwlt_reward_apply against sampling.reward_apply_f32: rows 1 / 257, NaN and +-inf rewards in rows without a live
   slot, beta negative, zero, large.
4. End to end: (i) beta = 0 is the run without a reward, bit for bit, graph and eager; (ii) a 0 / 1 reward at beta = 100
   -- ancestors, recorded rewards, weights and evidence; (iii) the evidence in the linear domain against plain Monte
   Carlo; (iv) WindowReward on the discriminator; (v) refusals and generate(particles=, reward=).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops, sampling  # noqa: E402
from rlmg_amd.generation import Constraint  # noqa: E402

from test_blend_gpu import FIX, N_CLASS, _bits, _same, _small_model, _word2event  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -1234567


def _d(cuda, x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(cuda)


# ---- 1. push -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 65, 257])
@pytest.mark.parametrize("n_attr", [6, 8])
def test_push_against_numpy(cuda, rows, n_attr):
    rng = np.random.default_rng(rows + n_attr)
    for W in (1, 2, 50):
        for counter in (0, W - 1, 2 * W + 1):
            tok = rng.integers(0, 2 ** 40, (rows, n_attr)).astype(np.int64)
            done = (rng.random(rows) < 0.4).astype(np.int64) * rng.integers(1, 3, rows)
            if rows > 1:
                done[0], done[1] = 0, 2
            recent = np.full((rows, W, n_attr), SENTINEL, dtype=np.int64)
            live = np.full((rows, W), SENTINEL, dtype=np.int64)
            tok_d, done_d, recent_d, live_d = _d(cuda, tok), _d(cuda, done), _d(cuda, recent), _d(cuda, live)
            cnt = torch.tensor([counter], dtype=torch.int64, device=cuda)
            ops.reward_push(tok_d, done_d, cnt, recent_d, live_d)
            s = counter % W
            recent[:, s] = tok
            live[:, s] = done == 0
            assert np.array_equal(recent_d.cpu().numpy(), recent), (rows, n_attr, W, counter)
            assert np.array_equal(live_d.cpu().numpy(), live), (rows, n_attr, W, counter)
            assert torch.equal(tok_d, _d(cuda, tok)) and torch.equal(done_d, _d(cuda, done))
            assert int(cnt.item()) == counter


# ---- 2. window -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n_attr", [(1, 6), (65, 8), (257, 6)])
def test_window_against_numpy(cuda, rows, n_attr):
    rng = np.random.default_rng(rows)
    for W in (1, 2, 50):
        for filled in sorted({1, W}):
            recent = rng.integers(1, 2 ** 40, (rows, W, n_attr)).astype(np.int64)
            live = (rng.random((rows, W)) < 0.6).astype(np.int64) * rng.integers(1, 3, (rows, W))
            live[:, filled:] = 1                                        # stale flags past the window
            dead = np.arange(rows) % 3 == 1
            live[dead, :filled] = 0                                     # rows with no live slot
            if rows > 2:
                live[2, 0] = 1
                assert dead[1] and not dead[2]
            win = torch.full((rows, W, n_attr), SENTINEL, dtype=torch.int64, device=cuda)
            mask = torch.full((rows, W), SENTINEL, dtype=torch.int64, device=cuda)
            any_d = torch.full((rows,), SENTINEL, dtype=torch.int64, device=cuda)
            recent_d, live_d = _d(cuda, recent), _d(cuda, live)
            ops.reward_window(recent_d, live_d, filled, win, mask, any_d)
            on = (live != 0) & (np.arange(W)[None, :] < filled)
            want_any = on.any(1)
            want_mask = on.astype(np.int64)
            want_mask[~want_any, 0] = 1
            assert np.array_equal(win.cpu().numpy(), np.where(on[..., None], recent, 0)), (rows, W, filled)
            assert np.array_equal(mask.cpu().numpy(), want_mask), (rows, W, filled)
            assert np.array_equal(any_d.cpu().numpy(), want_any.astype(np.int64)), (rows, W, filled)
            assert torch.equal(recent_d, _d(cuda, recent)) and torch.equal(live_d, _d(cuda, live))
            if rows > 2:
                assert any_d[1].item() == 0 and mask[1, 0].item() == 1 and int(win[1].abs().sum().item()) == 0
                assert int(mask.sum(1).min().item()) >= 1               # no empty window


# ---- 3. apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 257])
def test_apply_against_f32_restatement(cuda, rows):
    rng = np.random.default_rng(rows)
    for beta in (1.0, -2.5, 0.0, 100.0, 0.3):
        for dead_fill in (np.nan, np.inf, -np.inf):
            lw = rng.normal(0, 30, rows).astype(np.float32)
            r = (rng.normal(0, 1, rows) * 10.0 ** rng.integers(-3, 3, rows)).astype(np.float32)
            on = (rng.random(rows) < 0.6).astype(np.int64) * rng.integers(1, 3, rows)
            if rows > 1:
                on[0], on[1] = 1, 0
            r[on == 0] = dead_fill
            lw_d = _d(cuda, lw)
            h_r = torch.full((rows,), float(SENTINEL), dtype=torch.float32, device=cuda)
            ops.reward_apply(_d(cuda, r), _d(cuda, on), beta, lw_d, h_r)
            want, rec = sampling.reward_apply_f32(lw, r, on, beta)
            got, got_r = lw_d.cpu().numpy(), h_r.cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (rows, beta, dead_fill)
            assert np.array_equal(got_r.view(np.int32), rec.view(np.int32)), (rows, beta, dead_fill)
            assert np.array_equal(got[on == 0].view(np.int32), lw[on == 0].view(np.int32))
            assert (got_r[on == 0] == 0).all() and np.isfinite(got).all()


def test_binding_refusals(cuda):
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=cuda)     # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=cuda)   # noqa: E731
    with pytest.raises(ValueError, match="recent must be"):
        ops.reward_push(i64(4, 6), i64(4), i64(1), i64(4, 5, 6), i64(4, 4))
    with pytest.raises(TypeError, match="reward_push takes"):
        ops.reward_push(i64(3, 6), i64(4), i64(1), i64(4, 5, 6), i64(4, 5))
    with pytest.raises(TypeError, match="counter"):
        ops.reward_push(i64(4, 6), i64(4), f32(1), i64(4, 5, 6), i64(4, 5))
    with pytest.raises(TypeError, match="reward_window takes"):
        ops.reward_window(i64(4, 5, 6), i64(4, 5), 5, i64(4, 5, 6), i64(4, 4), i64(4))
    for filled in (0, 6):
        with pytest.raises(RuntimeError):                               # the C entry's 1001
            ops.reward_window(i64(4, 5, 6), i64(4, 5), filled, i64(4, 5, 6), i64(4, 5), i64(4))
    with pytest.raises(TypeError, match="reward_apply takes"):
        ops.reward_apply(f32(4), i64(4), 1.0, f32(5), f32(5))
    with pytest.raises(TypeError, match="int64 any"):
        ops.reward_apply(f32(4), f32(4), 1.0, f32(4), f32(4))


# ---- 4. end to end -------------------------------------------------------------------------------------------------------
N, K, SEED, EPS23 = 3, 4, 21, 2.0 ** -23


@pytest.fixture(scope="module")
def world(cuda):
    seed = int(FIX["fill_seed"])
    w2e = _word2event()
    w = {"net": _small_model(cuda, seed), "w2e": w2e, "cuda": cuda}
    w["tight"] = Constraint(w2e, per_bar={"pitch": [[5, 6, 7], [20, 21, 22], [40, 41, 42]]}, cycle=True)
    return w


def _parity(windows, mask):
    """0 / 1: the parity of the pitch class of the window's first row."""
    return (windows[:, 0, 3] % 2).float()


def _particles(w, n=N, k=K, **kw):
    torch.manual_seed(SEED)
    kw.setdefault("bar_cond", 4)
    kw.setdefault("max_tokens", 48)
    kw.setdefault("chunk", 16)
    return generation.generate_particles(w["net"], w["w2e"], n, k, **kw)


def _same_sets(a, b, rewards=True):
    f = lambda x: x.view(np.int32)                                      # noqa: E731
    ok = (_same(a.songs, b.songs) and _bits(a.logprobs, b.logprobs) and np.array_equal(f(a.log_weights), f(b.log_weights))
          and a.log_evidence == b.log_evidence and np.array_equal(f(a.ess), f(b.ess)) and
          np.array_equal(a.resampled, b.resampled) and np.array_equal(a.ancestors, b.ancestors) and
          np.array_equal(f(a.event_log_weights), f(b.event_log_weights)))
    if rewards:
        ok = ok and _bits(a.rewards, b.rewards) and np.array_equal(f(a.event_rewards), f(b.event_rewards))
    return ok


def test_beta_zero_is_the_run_without_a_reward(world, monkeypatch):
    """(i) beta = 0 with a reward callable: songs, log-probs, weights, evidence and ancestors of the run without one, bit
    for bit, on the graph and eager; reward_window 5 against resample_every 4 and a ring of 16 rows."""
    w = world
    kw = dict(ess=1.0, resample_every=4, constraints=w["tight"], sampler="categorical")
    plain = _particles(w, **kw)
    assert any(ps.resampled.any() for ps in plain) and all(ps.rewards is None and ps.event_rewards is None for ps in plain)
    for graphs in (True, False):
        monkeypatch.setattr(ops, "GRAPHS_ENABLED", graphs)
        calls = []

        def fn(windows, mask):
            calls.append(tuple(windows.shape) + tuple(mask.shape))
            return _parity(windows, mask) * 7.5 - 3.0

        got = _particles(w, reward=fn, reward_window=5, beta=0.0, **kw)
        assert all(_same_sets(a, b, rewards=False) for a, b in zip(got, plain)), graphs
        assert calls and set(calls) == {(N * K, 5, 6, N * K, 5)}
        for ps in got:
            assert len(ps.rewards) == K
            for k in range(K):
                assert ps.rewards[k].dtype == np.float32 and len(ps.rewards[k]) == -(-(len(ps.songs[k]) - 1) // 5)
    monkeypatch.undo()


def _host_parity(song, W):
    drawn = song[1:]
    return np.array([drawn[j, 3] % 2 for j in range(0, len(drawn), W)], dtype=np.float32)


def _recompute(ps, R, W, beta, k_particles):
    """Weights and evidence of one set in float64 from its recorded pairs, rewards and ancestors -> the worst
    |difference| / bound of (weights, evidence).  The bound of a weight is events x 2^-23 x max |lw|: the updates
    (token rows and reward events) since the weight was last reset, and the largest running sum among them."""
    E = len(ps.resampled)
    line = generation.particle_lineage(ps.ancestors, k_particles)
    resets = (np.nonzero(ps.resampled)[0] + 1) * R                      # the steps after which the weights were 0
    worst_w = 0.0

    def weight(k, since, upto):
        """Particle k's updates after step `since` up to step `upto` (None: to the end, the closing partial event
        included), in the order they were made -> (sum, events, max |running sum|)."""
        pairs = ps.logprobs[k].astype(np.float64)
        terms = []
        for t in range(len(pairs)):                                     # row t is weighed at step t + 1
            if t + 1 > since and (upto is None or t + 1 <= upto):
                terms.append((t + 1, 0, float((pairs[t, :, 0] - pairs[t, :, 1]).sum())))
        for j, r in enumerate(ps.rewards[k]):                           # window j's event follows step (j + 1) W; when
            step = (j + 1) * W                                          # the run ends before, it follows every other
            if step > since and (upto is None or step <= upto):         # event
                terms.append((step, 1, beta * float(r)))
        terms.sort(key=lambda x: x[:2])
        run = np.cumsum([x[2] for x in terms]) if terms else np.zeros(1)
        return float(run[-1]), len(terms), float(np.abs(run).max())

    for e in range(E):
        step = (e + 1) * R
        since = int(resets[resets < step].max()) if (resets < step).any() else 0
        for k in range(k_particles):
            want, events, top = weight(k, since, step)
            seen = float(ps.event_log_weights[e, line[e, k]])
            bound = events * EPS23 * top
            assert abs(seen - want) <= bound, (e, k, seen, want, bound)
            worst_w = max(worst_w, abs(seen - want) / bound if bound else 0.0)
    since = int(resets.max()) if len(resets) else 0
    for k in range(k_particles):
        want, events, top = weight(k, since, None)
        bound = events * EPS23 * top
        assert abs(float(ps.log_weights[k]) - want) <= bound, (k, float(ps.log_weights[k]), want, bound)
        worst_w = max(worst_w, abs(float(ps.log_weights[k]) - want) / bound if bound else 0.0)
    hits = np.nonzero(ps.resampled)[0]
    want = sum(sampling.logmeanexp(ps.event_log_weights[e]) for e in hits) + sampling.logmeanexp(ps.log_weights)
    top = max([float(np.abs(ps.event_log_weights[e]).max()) for e in hits] + [float(np.abs(ps.log_weights).max())])
    bound = (len(hits) + 1) * EPS23 * top
    print("evidence %.6f against %.6f, bound %.3g" % (ps.log_evidence, want, bound))
    assert abs(ps.log_evidence - want) <= bound, (ps.log_evidence, want, bound)
    return worst_w, abs(ps.log_evidence - want) / bound if bound else 0.0


@pytest.mark.parametrize("W", [4, 7])
def test_synthetic_reward(world, monkeypatch, W):
    """(ii) r = the parity of the first row's pitch, beta = 100, resample_every 4, ess 1, a three-pitch per-bar constraint
    (songs end at different steps), 47 drawn rows at most (a partial last window for W 4 and 7 alike).  W = 4: reward and
    resampling events coincide.  W = 7: resample_every does not divide it, so windows cross resampling events."""
    w = world
    R, beta, cap = 4, 100.0, 48
    kw = dict(ess=1.0, resample_every=R, constraints=w["tight"], sampler="categorical", reward=_parity,
              reward_window=W, beta=beta, bar_cond=9, max_tokens=cap, chunk=cap)
    sets = _particles(w, **kw)
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    eager = _particles(w, **kw)
    monkeypatch.undo()
    assert all(_same_sets(a, b) for a, b in zip(sets, eager))
    lens = [len(s) - 1 for ps in sets for s in ps.songs]
    moved = sum(int((ps.ancestors != np.arange(K)).any(1).sum()) for ps in sets)
    print("W = %d: drawn rows %s, %d events moved rows" % (W, lens, moved))
    assert (cap - 1) % W and min(lens) < cap - 1 and len(set(lens)) > 1 and moved >= 1
    assert max(lens) > 2 * W                                            # a lineage with several windows
    worst = [0.0, 0.0]
    for ps in sets:
        # the recorded rewards are the callable's on the windows of the returned songs (0 / 1: exact)
        for k in range(K):
            assert np.array_equal(ps.rewards[k], _host_parity(ps.songs[k], W)), k
        assert set(np.unique(ps.event_rewards)) <= {0.0, 1.0}
        if W == R:                                                      # event e of either kind follows step (e + 1) R
            checked = 0
            for e in range(min(len(ps.ancestors), len(ps.event_rewards), (cap - 1) // W)):
                rewarded = ps.event_rewards[e] == 1
                if rewarded.any():
                    assert rewarded[ps.ancestors[e]].all(), (e, ps.event_rewards[e], ps.ancestors[e])
                    checked += 1
            assert checked >= 1
        a, b = _recompute(ps, R, W, beta, K)
        worst = [max(worst[0], a), max(worst[1], b)]
    print("W = %d: worst |weight - f64| / bound = %.3g, worst |evidence - f64| / bound = %.3g" % (W, worst[0], worst[1]))


def test_right_target(world):
    """(iii) sampler="categorical" without constraints: the proposal is the model, every weight is the reward term alone,
    and exp(log_evidence) is an unbiased estimate of E[exp(beta sum r)] under the model.  16 songs x 64 particles of 6
    drawn rows, windows of 2 rows, r = the share of odd pitches in the window (bounded in [0, 1]), beta 1.5, ess 1
    (every event resamples).  The mean of exp(log_evidence) over the songs against the plain Monte Carlo mean over 2048
    generate_batch songs of the same model: within 5 combined standard errors, each from its own sample's spread."""
    w = world
    W, beta, songs_n, k, rows = 2, 1.5, 16, 64, 6

    def share(windows, mask):
        return ((windows[:, :, 3] % 2) * mask).sum(1).float() / W

    sets = _particles(w, n=songs_n, k=k, ess=1.0, resample_every=W, sampler="categorical", reward=share,
                      reward_window=W, beta=beta, bar_cond=17, max_tokens=rows + 1, chunk=8)
    assert all(len(s) == rows + 1 for ps in sets for s in ps.songs) and any(ps.resampled.any() for ps in sets)
    z = np.exp(np.array([ps.log_evidence for ps in sets], dtype=np.float64))
    torch.manual_seed(SEED + 1)
    plain = generation.generate_batch(w["net"], w["w2e"], 2048, bar_cond=17, max_tokens=rows + 1, sampler="categorical",
                                      chunk=8)
    assert all(len(s) == rows + 1 for s in plain)
    f = np.exp(beta * np.array([(s[1:, 3] % 2).sum() / W for s in plain], dtype=np.float64))
    se = np.sqrt(z.var(ddof=1) / len(z) + f.var(ddof=1) / len(f))
    print("right target: SMC mean Z %.4f (se %.4f) against Monte Carlo %.4f (se %.4f): %.2f combined standard errors"
          % (z.mean(), np.sqrt(z.var(ddof=1) / len(z)), f.mean(), np.sqrt(f.var(ddof=1) / len(f)),
             abs(z.mean() - f.mean()) / se))
    assert f.std() > 0.1 * f.mean()                                     # the reward does tilt the target
    assert abs(z.mean() - f.mean()) <= 5 * se


def _small_disc(cuda):
    from rlmg_amd.dqn_policy import AIRL_model
    old = (AIRL_model.D_MODEL, AIRL_model.N_LAYER, AIRL_model.N_HEAD)
    AIRL_model.D_MODEL, AIRL_model.N_LAYER, AIRL_model.N_HEAD = 128, 2, 2
    try:
        net = fill_params(AIRL_model.LongFormer(N_CLASS), seed=41)
    finally:
        AIRL_model.D_MODEL, AIRL_model.N_LAYER, AIRL_model.N_HEAD = old
    with torch.no_grad():
        net.score_classifier[1].running_mean.copy_(torch.linspace(-0.2, 0.2, 128))
        net.score_classifier[1].running_var.copy_(torch.linspace(0.5, 1.5, 128))
    return net.to(cuda)


@pytest.fixture(scope="module")
def disc_world(world):
    """The discriminator, left in train() mode, and the three-song run every discriminator test reads."""
    w = dict(world)
    w["disc"] = _small_disc(w["cuda"]).train()
    w["kw"] = dict(ess=1.0, resample_every=16, constraints=w["tight"], sampler="categorical", bar_cond=17,
                   max_tokens=121, chunk=64)
    bn = w["disc"].score_classifier[1]
    w["before"] = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked.item()))
    w["reward"] = generation.WindowReward(w["disc"])
    w["sets"] = _particles(w, reward=w["reward"], **w["kw"])
    return w


def test_window_reward_on_the_discriminator(disc_world):
    """(iv) default reward_window (the discriminator's 50), 120 drawn rows at most: two whole windows and a partial one.
    The recorded rewards against the wrapper on the windows rebuilt from the returned songs, one (N K, 50, 6) batch per
    window index as in the run: |difference| <= 1e-4 / (D (1 - D)), the f32 parity figure of the score D carried through
    the log-odds.  The module is still in train() mode and its BatchNorm statistics are untouched."""
    w = disc_world
    W, disc, sets = 50, w["disc"], w["sets"]
    bn = disc.score_classifier[1]
    assert disc.training and all(m.training for m in disc.modules())
    assert torch.equal(bn.running_mean, w["before"][0]) and torch.equal(bn.running_var, w["before"][1])
    assert int(bn.num_batches_tracked.item()) == w["before"][2]
    songs = [s for ps in sets for s in ps.songs]
    rewards = [r for ps in sets for r in ps.rewards]
    n_windows = [len(r) for r in rewards]
    print("discriminator: drawn rows %s, windows %s" % ([len(s) - 1 for s in songs], n_windows))
    assert max(n_windows) == 3 and all(n == -(-(len(s) - 1) // W) for n, s in zip(n_windows, songs))
    worst = 0.0
    for j in range(max(n_windows)):
        win = np.zeros((len(songs), W, 6), dtype=np.int64)
        mask = np.zeros((len(songs), W), dtype=np.int64)
        for n, s in enumerate(songs):
            rows = s[1:][j * W:(j + 1) * W]
            win[n, :len(rows)] = rows
            mask[n, :len(rows)] = 1
            if not len(rows):
                mask[n, 0] = 1                                          # what a row without a live slot is shown
        r = w["reward"](_d(w["cuda"], win), _d(w["cuda"], mask)).cpu().numpy().astype(np.float64)
        for n in range(len(songs)):
            if j < n_windows[n]:
                d = 1.0 / (1.0 + np.exp(-r[n]))
                tol = 1e-4 / (d * (1.0 - d))
                err = abs(float(rewards[n][j]) - r[n])
                assert err <= tol, (n, j, float(rewards[n][j]), r[n], tol)
                worst = max(worst, err / tol)
    print("discriminator: worst |recorded - rebuilt| / tolerance = %.3g" % worst)
    assert disc.training and torch.equal(bn.running_mean, w["before"][0])
    # the forms, on one batch: log_odds = log D - log(1 - D), log = log D, score = D
    x, m = _d(w["cuda"], win), _d(w["cuda"], mask)
    score = generation.WindowReward(disc, form="score")(x, m)
    assert score.shape == (len(songs),) and score.dtype == torch.float32 and bool(((score > 0) & (score < 1)).all())
    c = score.clamp(1e-6, 1 - 1e-6)
    assert torch.equal(generation.WindowReward(disc, form="log")(x, m), torch.log(c))
    assert torch.equal(w["reward"](x, m), torch.log(c) - torch.log(1 - c))
    clamped = generation.WindowReward(lambda a, b: torch.tensor([[0.0], [1.0]], device=w["cuda"]), eps=1e-3)(x, m)
    assert torch.allclose(clamped, torch.tensor([-6.906755, 6.906755], device=w["cuda"]), atol=1e-4)


def test_song_zero_alone_with_the_discriminator(disc_world):
    """Song 0's set does not depend on the other songs of the pool: in eval() mode a window's score is its own."""
    w = disc_world
    one = _particles(w, n=1, reward=w["reward"], **w["kw"])
    three = w["sets"]
    diff = max(float(np.abs(a - b).max()) for a, b in zip(one[0].rewards, three[0].rewards)
               if a.shape == b.shape and len(a))
    print("song 0 alone against song 0 of three: worst |reward difference| = %.3g" % diff)
    assert len(one) == 1 and _same_sets(one[0], three[0])


def test_refusals_and_generate(world, tmp_path):
    """(v)"""
    w = world
    net, w2e = w["net"], w["w2e"]
    with pytest.raises(TypeError, match="reward must be a callable"):
        generation.generate_particles(net, w2e, 3, 4, reward=3)
    for kw, msg in ((dict(reward_window=0), "reward_window"), (dict(beta=float("nan")), "beta must be finite"),
                    (dict(beta=float("inf")), "beta must be finite")):
        with pytest.raises(ValueError, match=msg):
            generation.generate_particles(net, w2e, 3, 4, reward=_parity, **kw)
    for kw in (dict(), dict(batch_size=3), dict(slots=4)):
        with pytest.raises(ValueError, match="pass particles="):
            generation.generate(net, w2e, n_songs=3, reward=_parity, path_gendir=str(tmp_path), **kw)
    with pytest.raises(TypeError, match="must return"):                # a callable that returns the wrong thing
        _particles(w, reward=lambda x, m: torch.zeros(len(x), 1, device=x.device), reward_window=4)
    with pytest.raises(TypeError, match="must return"):
        _particles(w, reward=lambda x, m: [0.0] * len(x), reward_window=4)
    kw = dict(constraints=w["tight"], ess=1.0, resample_every=4, reward=_parity, reward_window=4, beta=100.0)
    torch.manual_seed(SEED)
    sets = generation.generate_particles(net, w2e, 3, 4, bar_cond=4, max_tokens=48, **kw)
    torch.manual_seed(SEED)
    stats = generation.generate(net, w2e, n_songs=3, bar_cond=4, max_tokens=48, batch_size=3, particles=4,
                                path_gendir=str(tmp_path), stats_path=None, log=lambda s: None, **kw)
    assert len(stats["words_len_list"]) == 3
    for i, ps in enumerate(sets):
        song = np.load(os.path.join(str(tmp_path), "get_%d.npy" % i))
        assert any(song.shape == s.shape and (song == s).all() for s in ps.songs)
        assert ps.rewards is not None and len(song) == stats["words_len_list"][i]
    # the reward did steer: against the same run without it, more windows open on an odd pitch
    torch.manual_seed(SEED)
    plain = generation.generate_particles(net, w2e, 3, 4, bar_cond=4, max_tokens=48,
                                          **{k: v for k, v in kw.items() if k not in ("reward", "reward_window", "beta")})
    odd = lambda group: np.mean([_host_parity(s, 4).mean() for ps in group for s in ps.songs])   # noqa: E731
    print("share of windows that open on an odd pitch: %.2f with the reward, %.2f without" % (odd(sets), odd(plain)))
    assert odd(sets) > odd(plain)

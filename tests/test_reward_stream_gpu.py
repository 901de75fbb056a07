"""GPU: reward-guided particles on the stream and a reward weight per song -- cwlt_reward_apply_keyed
bitwise against its numpy restatement, then generation.generate_particles(slots=, reward=) end to end on the small
fixture model (128 / 2 layers / 2 heads) against the lock-step pool.

1. cwlt_reward_apply_keyed: rows 1 / 257 / 2050 x particles 2 / 7 / 64; key NULL, the identity, a permutation with -1
   entries, ids whose song has no table entry; betas with 0, a negative one and 100; NaN / +-inf in off rows; the
   weights of off rows and sentinel-filled memory around both output buffers unchanged; the binding's refusals.
2. Stream equals lock-step: 7 songs x 4 particles, ess = 1, the "all on" configuration, r = the parity of the window's
   first pitch at beta = 100, (R, W, chunk) = (4, 8, 16), (8, 4, 16), (4, 6, 24): slots 7, 3 and 1 give the pool's sets
   bit for bit, rewards and event_rewards included; with one shared prompt against prefill="gemm"; graph equals eager;
   the 3-slot run's own record shows the comparison is not vacuous.
3. A beta per song: a constant list is the scalar run; a song with beta 0 is the song without a reward; pool equals
   stream; weights and evidence against float64 with each song's own beta.
4. beta = 0 on the stream; WindowReward on the small discriminator at W = 50, R = 10, chunk = 100; generate().
5. The launch sequence of both particle loops, with and without a reward, against patterns written out from the
   loops' docstrings: 3 songs x 2 particles, (R, W, chunk) = (2, 4, 4), max_tokens 8, bar_cond 4, graphs off.

bar_cond 9 and max_tokens 48 (tests/test_reward_gpu.py's): the particles draw 30 .. 39 rows at (R, W, chunk) = (4, 8, 16),
19 .. 40 at (8, 4, 16) and 30 .. 43 at (4, 6, 24) (the test prints them), three or more windows each, and at 3 slots
four songs start late, at two or more different multiples of B.  With these values every non-vacuity assertion of
test 2 holds for (R, W, chunk) = (4, 8, 16) and (4, 6, 24); for (8, 4, 16), where every R boundary is a B boundary and
no window crosses an event, those that can.  (At bar_cond 4 the songs have one or two windows and every lineage's
rewards are equal.)
"""
import os

import numpy as np
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, ops, sampling
from rlmg_amd.generation import Constraint, Grammar, Preference

from test_blend_gpu import FIX, _bits, _same, _small_model, _word2event
from test_reward_gpu import _recompute, _small_disc

pytestmark = pytest.mark.gpu
SENT = -1234567.0
GUARD = 64


def _d(cuda, x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(cuda)


# ---- 1. keyed apply ------------------------------------------------------------------------------------------------------
def _guarded(cuda, values):
    """values inside a sentinel-filled buffer, GUARD floats on either side -> (the whole buffer, the view on values)."""
    whole = torch.full((len(values) + 2 * GUARD,), SENT, dtype=torch.float32, device=cuda)
    view = whole[GUARD:GUARD + len(values)]
    view.copy_(_d(cuda, values))
    return whole, view


@pytest.mark.parametrize("rows", [1, 257, 2050])
@pytest.mark.parametrize("K", [2, 7, 64])
def test_keyed_apply_against_restatement(cuda, rows, K):
    rng = np.random.default_rng([rows, K])
    songs = -(-rows // K)
    perm = rng.permutation(rows).astype(np.int64)
    perm[rng.random(rows) < 0.3] = -1
    if rows > 1:
        perm[0], perm[-1] = -1, 0
    keys = {"null": (None, songs), "identity": (np.arange(rows, dtype=np.int64), songs), "permutation": (perm, songs),
            "no entry": (np.arange(rows, dtype=np.int64) + K * (songs // 2), max(1, songs // 2 + 1))}
    for name, (key, n_beta) in keys.items():
        for dead_fill in (np.nan, np.inf, -np.inf):
            beta = rng.normal(0, 3, n_beta).astype(np.float32)
            beta[:3] = np.float32([0.0, -2.5, 100.0])[:n_beta][::-1]      # rows 0 .. are on in every key but the permutation
            lw = rng.normal(0, 30, rows).astype(np.float32)
            r = (rng.normal(0, 1, rows) * 10.0 ** rng.integers(-3, 3, rows)).astype(np.float32)
            on = (rng.random(rows) < 0.7).astype(np.int64) * rng.integers(1, 3, rows)
            ids = np.arange(rows) if key is None else key
            off = (on == 0) | (ids < 0) | (np.where(ids >= 0, ids // K, 0) >= n_beta)
            r[off] = dead_fill
            lw_all, lw_d = _guarded(cuda, lw)
            hr_all, hr_d = _guarded(cuda, np.full(rows, SENT, np.float32))
            ops.reward_apply_keyed(_d(cuda, r), _d(cuda, on), _d(cuda, beta), None if key is None else _d(cuda, key), K,
                                   lw_d, hr_d)
            want, rec = sampling.reward_apply_keyed_f32(lw, r, on, beta, key, K)
            got, got_r = lw_d.cpu().numpy(), hr_d.cpu().numpy()
            where = (rows, K, name, dead_fill)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), where
            assert np.array_equal(got_r.view(np.int32), rec.view(np.int32)), where
            assert np.array_equal(got[off].view(np.int32), lw[off].view(np.int32)) and (got_r[off] == 0).all(), where
            assert np.isfinite(got).all() and (name != "no entry" or rows == 1 or off[-1]), where
            for whole in (lw_all, hr_all):
                edge = torch.cat([whole[:GUARD], whole[-GUARD:]])
                assert bool((edge == SENT).all()), where
            if name == "identity":                                      # the identity key is the NULL key
                lw2, hr2 = _d(cuda, lw), torch.zeros(rows, dtype=torch.float32, device=cuda)
                ops.reward_apply_keyed(_d(cuda, r), _d(cuda, on), _d(cuda, beta), None, K, lw2, hr2)
                assert torch.equal(lw2.view(torch.int32), lw_d.view(torch.int32)) and \
                    torch.equal(hr2.view(torch.int32), hr_d.view(torch.int32))


def test_keyed_apply_equal_table_is_the_scalar_kernel(cuda):
    rng = np.random.default_rng(8)
    rows, K = 257, 7
    lw = rng.normal(0, 30, rows).astype(np.float32)
    r = rng.normal(0, 5, rows).astype(np.float32)
    on = rng.integers(0, 2, rows).astype(np.int64)
    for beta in (100.0, -2.5, 0.3, 0.0):
        a, b = _d(cuda, lw), _d(cuda, lw)
        ha, hb = (torch.zeros(rows, dtype=torch.float32, device=cuda) for _ in range(2))
        ops.reward_apply(_d(cuda, r), _d(cuda, on), beta, a, ha)
        ops.reward_apply_keyed(_d(cuda, r), _d(cuda, on), _d(cuda, np.full(37, beta, np.float32)), None, K, b, hb)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ha.view(torch.int32),
                                                                                     hb.view(torch.int32))


def test_keyed_binding_refusals(cuda):
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=cuda)     # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=cuda)   # noqa: E731
    with pytest.raises(TypeError, match="reward_apply_keyed takes contiguous f32"):
        ops.reward_apply_keyed(f32(4), i64(4), f32(2), None, 2, f32(5), f32(5))
    with pytest.raises(TypeError, match="int64 any"):
        ops.reward_apply_keyed(f32(4), f32(4), f32(2), None, 2, f32(4), f32(4))
    with pytest.raises(TypeError, match="beta table"):
        ops.reward_apply_keyed(f32(4), i64(4), i64(2), None, 2, f32(4), f32(4))
    with pytest.raises(TypeError, match="beta table"):
        ops.reward_apply_keyed(f32(4), i64(4), f32(0), None, 2, f32(4), f32(4))
    with pytest.raises(TypeError, match="int64 key"):
        ops.reward_apply_keyed(f32(4), i64(4), f32(2), i64(3), 2, f32(4), f32(4))
    with pytest.raises(TypeError, match="int64 key"):
        ops.reward_apply_keyed(f32(4), i64(4), f32(2), f32(4), 2, f32(4), f32(4))
    with pytest.raises(ValueError, match="particles must be"):
        ops.reward_apply_keyed(f32(4), i64(4), f32(2), None, 0, f32(4), f32(4))


# ---- 2. the stream against the lock-step pool ----------------------------------------------------------------------------
N, K4, BAR_COND, CAP, SEED, BETA = 7, 4, 9, 48, 21, 100.0
CONFIGS = [(4, 8, 16), (8, 4, 16), (4, 6, 24)]                          # (resample_every, reward_window, chunk)


def _parity(windows, mask):
    """0 / 1: the parity of the pitch class of the window's first row (a live row, when the window has one)."""
    return (windows[:, 0, 3] % 2).float()


def _host_parity(song, W, P=1):
    drawn = song[P:]
    return np.array([drawn[j, 3] % 2 for j in range(0, len(drawn), W)], dtype=np.float32)


def _make_world(cuda):
    seed = int(FIX["fill_seed"])
    w2e = _word2event()
    w = {"net": _small_model(cuda, seed), "ref": _small_model(cuda, seed + 1), "w2e": w2e, "cuda": cuda, "lock": {}}
    w["tight"] = Constraint(w2e, per_bar={"pitch": [[5, 6, 7], [20, 21, 22], [40, 41, 42]]}, cycle=True)
    w["all on"] = dict(constraints=w["tight"], grammar=Grammar(w2e), reference=w["ref"], alpha=0.7,
                       preferences=Preference(w2e, repeat={"pitch": (0.5, 0.5)}, decay=0.9), sampler="categorical")
    return w


@pytest.fixture(scope="module")
def world(cuda):
    return _make_world(cuda)


def _particles(w, config, **kw):
    R, W, chunk = config
    torch.manual_seed(SEED)
    kw.setdefault("reward", _parity)
    kw.setdefault("beta", BETA)
    return generation.generate_particles(w["net"], w["w2e"], N, K4, bar_cond=BAR_COND, max_tokens=CAP, chunk=chunk,
                                         resample_every=R, reward_window=W, ess=1.0, **w["all on"], **kw)


def _lock(w, config):
    """The lock-step pool of all 7 songs under the reward, made once per configuration."""
    if config not in w["lock"]:
        w["lock"][config] = _particles(w, config)
    return w["lock"][config]


def _same_sets(a, b, rewards=True):
    f = lambda x: x.view(np.int32)                                      # noqa: E731
    ok = (_same(a.songs, b.songs) and _bits(a.logprobs, b.logprobs) and np.array_equal(f(a.log_weights), f(b.log_weights))
          and a.log_evidence == b.log_evidence and np.array_equal(f(a.ess), f(b.ess)) and
          np.array_equal(a.resampled, b.resampled) and np.array_equal(a.ancestors, b.ancestors) and
          np.array_equal(f(a.event_log_weights), f(b.event_log_weights)))
    if rewards:
        ok = ok and _bits(a.rewards, b.rewards) and a.event_rewards.shape == b.event_rewards.shape and \
            np.array_equal(f(a.event_rewards), f(b.event_rewards)) and a.beta == b.beta
    return ok


def _differ(a, b, rewards=True):
    assert len(a) == len(b)
    return [i for i, (x, y) in enumerate(zip(a, b)) if not _same_sets(x, y, rewards)]


def _stream3_with_stats(w, config, beta=BETA):
    """The 3-slot run through _run_particle_stream, which hands back the run's own record."""
    R, W, chunk = config
    kw = w["all on"]
    torch.manual_seed(SEED)
    heads, caps, plan = generation._particle_setup("generate_particles", w["net"], w["w2e"], N, K4, R, 1.0, BAR_COND,
                                                   CAP, None, "categorical", chunk, "blas", kw["constraints"],
                                                   kw["grammar"], w["ref"], 0.7, kw["preferences"], pool=3)
    stats = {}
    sets = generation._run_particle_stream(w["net"], w["w2e"], heads, caps, plan, N, K4, 3, R, 1.0, BAR_COND, chunk, None,
                                           None, stats=stats, reward=generation._reward_spec(_parity, W, beta, N))
    return sets, stats


@pytest.mark.parametrize("config", CONFIGS)
def test_stream_is_the_lock_step_run(world, config):
    """Slots 7, 3 and 1: all 7 sets are the lock-step pool's, field by field and bit for bit, rewards included; and the
    recorded rewards are the callable's on the windows of the returned songs (0 / 1: exact)."""
    w = world
    R, W, chunk = config
    B = R * W // np.gcd(R, W)
    lock = _lock(w, config)
    assert len(lock) == N and any(ps.resampled.any() for ps in lock)
    three, stats = _stream3_with_stats(w, config)
    assert _differ(three, lock) == []
    for slots in (7, 1):
        assert _differ(_particles(w, config, slots=slots), lock) == [], slots
    for ps in three:
        assert ps.beta == BETA and set(np.unique(ps.event_rewards)) <= {0.0, 1.0}
        for k in range(K4):
            assert np.array_equal(ps.rewards[k], _host_parity(ps.songs[k], W)), k
    starts, lens = stats["start_steps"], [[len(s) - 1 for s in ps.songs] for ps in three]
    print("reward stream (R, W, chunk) = %s at 3 slots: starts %s, %d steps, %d events, %d reward events, waiting %d "
          "(beyond the next R boundary: %d) and idle %d group-steps, lengths %s"
          % (config, starts, stats["steps"], stats["events"], stats["reward_events"], stats["wait_group_steps"],
             stats["boundary_wait_group_steps"], stats["idle_group_steps"], lens))
    assert sorted(starts[:3]) == [0, 0, 0] and all(s > 0 for s in starts[3:]) and all(s % B == 0 for s in starts)
    assert stats["events"] * R == stats["steps"] and stats["reward_events"] * W == stats["steps"]
    # the comparison is not vacuous (on this run's own record; bar_cond 9, max_tokens 48):
    late = [ps for ps, s in zip(three, starts) if s > 0]
    assert any((ps.ancestors != np.arange(K4)).any() for ps in late)     # a late song has an event that moved rows
    assert any(n % W for per in lens for n in per)                      # a particle ends inside a window
    if R % W:                                                           # B > R, and events off the windows' grid
        assert stats["boundary_wait_group_steps"] > 0                   # a group waited past an R boundary that is no B's
        assert any(ps.resampled[e] and (e + 1) * R % W for ps in three for e in range(len(ps.resampled)))  # a window
        #                                                                 straddles a resampling that happened
    assert any(len(np.unique(np.concatenate(ps.rewards))) > 1 for ps in three)   # rewards that are not all equal
    assert any(len(r) > 1 for ps in late for r in ps.rewards)           # a late lineage with several windows


@pytest.mark.parametrize("config", CONFIGS)
def test_shared_prompt(world, config):
    """One shared prompt, prefilled once, against the lock-step pool with prefill="gemm" and the prompt for every song."""
    w = world
    W = config[1]
    song = _lock(w, config)[0].songs[0]
    P = 5
    while P > 2 and 1 + sum(w["w2e"]["bar-beat"][int(r[2])] == "Bar" for r in song[1:P]) >= BAR_COND - 1:
        P -= 1
    prompt = song[:P].copy()
    want = _particles(w, config, prompts=prompt, prefill="gemm")
    got = _particles(w, config, prompts=prompt, slots=3)
    assert _differ(got, want) == []
    for slots in (7, 1):
        assert _differ(_particles(w, config, prompts=prompt, slots=slots), want) == [], slots
    assert all((s[:P] == prompt).all() for ps in got for s in ps.songs) and any(ps.resampled.any() for ps in got)
    for ps in got:
        for k in range(K4):
            assert np.array_equal(ps.rewards[k], _host_parity(ps.songs[k], W, P)), k


def test_graph_is_eager(world, monkeypatch):
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    eager = _particles(world, CONFIGS[0], slots=3)
    monkeypatch.undo()
    assert _differ(eager, _lock(world, CONFIGS[0])) == []


# ---- 3. a beta per song --------------------------------------------------------------------------------------------------
BETAS = [0.0, 100.0, 0.3, -2.5, 100.0, 1.0, 30.0]


def test_per_song_beta(world):
    w, config = world, CONFIGS[0]
    R, W, _ = config
    # a constant list is the scalar run, in the pool and on the stream (beta itself is recorded as the song's float)
    lock = _lock(w, config)
    assert _differ(_particles(w, config, beta=[BETA] * N), lock) == []
    assert _differ(_particles(w, config, beta=[BETA] * N, slots=3), lock) == []
    # a list: song 0 (beta 0) is song 0 of the run without a reward; the pool is the stream
    pool = _particles(w, config, beta=BETAS)
    plain = _particles(w, config, reward=None)
    assert _same_sets(pool[0], plain[0], rewards=False) and pool[0].rewards is not None and plain[0].rewards is None
    assert [ps.beta for ps in pool] == BETAS and all(ps.beta is None for ps in plain)
    assert not _same_sets(pool[1], plain[1], rewards=False)             # beta 100 does steer song 1
    assert _same_sets(pool[1], lock[1]) and _same_sets(pool[4], lock[4])        # and a song is its own beta's alone
    stream = _particles(w, config, beta=BETAS, slots=3)
    assert _differ(stream, pool) == []
    # weights and evidence in float64 from the recorded pairs, rewards and ancestors, each song with its own beta
    worst = [0.0, 0.0]
    for ps in stream:
        a, b = _recompute(ps, R, W, ps.beta, K4)
        worst = [max(worst[0], a), max(worst[1], b)]
    print("per-song beta: worst |weight - f64| / bound = %.3g, worst |evidence - f64| / bound = %.3g"
          % (worst[0], worst[1]))


# ---- 4. beta = 0, the discriminator, generate() ----------------------------------------------------------------------------
def test_beta_zero_on_the_stream(world):
    w, config = world, CONFIGS[0]
    calls = []

    def fn(windows, mask):
        calls.append(tuple(windows.shape) + tuple(mask.shape))
        return _parity(windows, mask) * 7.5 - 3.0

    plain = _particles(w, config, reward=None, slots=3)
    got = _particles(w, config, reward=fn, beta=0.0, slots=3)
    assert _differ(got, plain, rewards=False) == []
    assert calls and set(calls) == {(3 * K4, config[1], 6, 3 * K4, config[1])}  # all S K rows, every event
    assert all(ps.rewards is not None and ps.beta == 0.0 for ps in got) and all(ps.rewards is None for ps in plain)


def test_window_reward_on_the_stream(world):
    """WindowReward on the small AIRL discriminator, W = 50, R = 10, chunk = 100, 3 songs on 2 slots, 120 drawn rows at
    most: the recorded rewards against the wrapper on the windows rebuilt from the returned songs, within
    1e-4 / (D (1 - D)) (tests/test_reward_gpu.py's figure).  The module's modes and BatchNorm statistics are unchanged."""
    w = world
    W, disc = 50, _small_disc(w["cuda"]).train()
    bn = disc.score_classifier[1]
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked.item()))
    reward = generation.WindowReward(disc)
    torch.manual_seed(SEED)
    sets = generation.generate_particles(w["net"], w["w2e"], 3, K4, ess=1.0, resample_every=10, constraints=w["tight"],
                                         sampler="categorical", bar_cond=17, max_tokens=121, chunk=100, reward=reward,
                                         reward_window=W, slots=2)
    assert disc.training and all(m.training for m in disc.modules())
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
    assert int(bn.num_batches_tracked.item()) == before[2]
    songs = [s for ps in sets for s in ps.songs]
    rewards = [r for ps in sets for r in ps.rewards]
    n_windows = [len(r) for r in rewards]
    print("discriminator on the stream: drawn rows %s, windows %s" % ([len(s) - 1 for s in songs], n_windows))
    assert max(n_windows) >= 2 and all(n == -(-(len(s) - 1) // W) for n, s in zip(n_windows, songs))
    assert len(np.unique(np.concatenate(rewards))) > len(songs)         # scores of their own windows, not one clamp value
    worst = 0.0
    for j in range(max(n_windows)):
        win = np.zeros((len(songs), W, 6), dtype=np.int64)
        mask = np.zeros((len(songs), W), dtype=np.int64)
        for n, s in enumerate(songs):
            rows = s[1:][j * W:(j + 1) * W]
            win[n, :len(rows)] = rows
            mask[n, :len(rows)] = 1
            if not len(rows):
                mask[n, 0] = 1
        r = reward(_d(w["cuda"], win), _d(w["cuda"], mask)).cpu().numpy().astype(np.float64)
        for n in range(len(songs)):
            if j < n_windows[n]:
                d = 1.0 / (1.0 + np.exp(-r[n]))
                tol = 1e-4 / (d * (1.0 - d))
                err = abs(float(rewards[n][j]) - r[n])
                assert err <= tol, (n, j, float(rewards[n][j]), r[n], tol)
                worst = max(worst, err / tol)
    print("discriminator on the stream: worst |recorded - rebuilt| / tolerance = %.3g" % worst)
    assert disc.training and torch.equal(bn.running_mean, before[0])


def test_generate_passes_the_reward_through(world, tmp_path, monkeypatch):
    w = world
    net, w2e = w["net"], w["w2e"]
    kw = dict(constraints=w["tight"], ess=1.0, resample_every=16, reward=_parity, reward_window=32,
              beta=[100.0, 0.0, 30.0, 100.0, 1.0])
    torch.manual_seed(SEED)
    sets = generation.generate_particles(net, w2e, 5, K4, bar_cond=BAR_COND, max_tokens=CAP, slots=2, **kw)
    torch.manual_seed(SEED)
    stats = generation.generate(net, w2e, n_songs=5, bar_cond=BAR_COND, max_tokens=CAP, slots=2, particles=K4,
                                path_gendir=str(tmp_path), stats_path=None, log=lambda s: None, **kw)
    assert len(stats["words_len_list"]) == 5 and [ps.beta for ps in sets] == kw["beta"]
    for i, ps in enumerate(sets):
        song = np.load(os.path.join(str(tmp_path), "get_%d.npy" % i))
        assert any(song.shape == s.shape and (song == s).all() for s in ps.songs)
        assert ps.rewards is not None and len(song) == stats["words_len_list"][i]
    # the batch_size path cuts the list per group, like every per-song entry; its first pool is generate_particles' on
    # the first three songs and their betas
    kw.update(reward_window=4, resample_every=4)
    torch.manual_seed(SEED)
    first = generation.generate_particles(net, w2e, 3, K4, bar_cond=BAR_COND, max_tokens=CAP,
                                          **dict(kw, beta=kw["beta"][:3]))
    seen, run = [], generation._run_particles
    monkeypatch.setattr(generation, "_run_particles", lambda *a, **k: seen.append(k["reward"][2]) or run(*a, **k))
    torch.manual_seed(SEED)
    stats = generation.generate(net, w2e, n_songs=5, bar_cond=BAR_COND, max_tokens=CAP, batch_size=3, particles=K4,
                                path_gendir=str(tmp_path / "pools"), stats_path=None, log=lambda s: None, **kw)
    monkeypatch.undo()
    assert seen == [(100.0, 0.0, 30.0), (100.0, 1.0)] and len(stats["words_len_list"]) == 5
    for i, ps in enumerate(first):
        song = np.load(os.path.join(str(tmp_path / "pools"), "get_%d.npy" % i))
        assert any(song.shape == s.shape and (song == s).all() for s in ps.songs) and ps.beta == kw["beta"][i]
    with pytest.raises(ValueError, match="reward= with slots="):        # generate's chunk is 128: W = 50 stays refused
        generation.generate(net, w2e, n_songs=5, slots=2, particles=K4, path_gendir=str(tmp_path), reward=_parity)


# ---- 5. the launch sequence ----------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """Every ops._call of the test by entry name, the call itself forwarded unchanged; graphs off."""
    seen, real = [], ops._call

    def recording(name, *args, **kw):
        seen.append(name)
        return real(name, *args, **kw)

    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    monkeypatch.setattr(ops, "_call", recording)
    return seen


# "all on": S and Z of the model and of the reference, then tok, bar, beat, seen, len, done, cap; a reward adds recent, live
FAMILIES = 4 + 7
WINDOW = ["cwlt_reward_window", "cwlt_reward_apply"]
RELEASE = ["cwlt_particle_release", "cwlt_particle_fill", "cwlt_particle_fill"]   # the release, then beat and seen


def _watched(names):
    return [n for n in names if n.startswith(("cwlt_particle_", "cwlt_reward_")) or n in ("cwlt_stream_refill",
                                                                                         "cwlt_count_bars")]


def _lock_step_launches(T, R, W, reward):
    """_ParticleLoop's docstring for T tokens: per token the bar count, under a reward the push, the weigh; after every
    W-th token the reward event, ahead of the resampling event after every R-th: the resampling, then every family to
    scratch and back; a run that ends inside a window closes it with one more reward event."""
    gathers = ["cwlt_particle_gather"] * (2 * (FAMILIES + (2 if reward else 0)))
    out = []
    for t in range(1, T + 1):
        out += ["cwlt_count_bars"] + ["cwlt_reward_push"] * reward + ["cwlt_particle_weigh"]
        if reward and t % W == 0:
            out += WINDOW
        if t % R == 0:
            out += ["cwlt_particle_resample"] + gathers
    return out + (WINDOW if reward and T % W else [])


def _stream_launches(T, R, W, reward):
    """_ParticleStreamLoop's docstring for T steps: the first release; per token the refill of the model's pool and of
    the reference's, the bar count, under a reward the push, the weigh, the advance; after every W-th token the reward
    event, ahead of the event after every R-th: the keyed resampling, every family to scratch and back and, at
    multiples of R -- of lcm(R, W) under a reward --, the release and its fills."""
    gathers = ["cwlt_particle_gather"] * (2 * (FAMILIES + (2 if reward else 0)))
    hand = R * W // int(np.gcd(R, W)) if reward else R
    out = list(RELEASE)
    for t in range(1, T + 1):
        out += ["cwlt_stream_refill"] * 2 + ["cwlt_count_bars"] + ["cwlt_reward_push"] * reward
        out += ["cwlt_particle_weigh", "cwlt_particle_advance"]
        if reward and t % W == 0:
            out += WINDOW
        if t % R == 0:
            out += ["cwlt_particle_resample_keyed"] + gathers + (RELEASE if t % hand == 0 else [])
    return out


def test_launch_sequences(world, calls):
    """3 songs x 2 particles, "all on", (R, W, chunk) = (2, 4, 4), max_tokens 8 (7 drawn rows at most), bar_cond 4: the
    lock-step pool and the 2-slot stream, each with and without a reward, launch what their docstrings say, in that
    order; T is read off the run (the weigh launches) and must be a length the run can have."""
    w = world
    R, W, chunk = 2, 4, 4
    for slots in (None, 2):
        for reward in (None, _parity):
            del calls[:]
            torch.manual_seed(SEED)
            sets = generation.generate_particles(w["net"], w["w2e"], 3, 2, bar_cond=4, max_tokens=8, chunk=chunk,
                                                 resample_every=R, reward_window=W, ess=1.0, reward=reward, beta=BETA,
                                                 slots=slots, **w["all on"])
            got = _watched(calls)
            T = got.count("cwlt_particle_weigh")
            print("launch sequence, slots %s, reward %s: %d tokens, %d launches" % (slots, reward is not None, T, len(got)))
            assert len(sets) == 3 and max(len(s) for ps in sets for s in ps.songs) <= 8
            if slots is None:
                assert T in (4, 7)                                      # one chunk, or the cap
                want = _lock_step_launches(T, R, W, reward is not None)
            else:
                assert T >= 2 * chunk and T % chunk == 0               # whole chunks, one enqueued past the end
                want = _stream_launches(T, R, W, reward is not None)
            assert got == want, (slots, reward is not None, T)
            assert reward is not None or not any(n.startswith("cwlt_reward_") for n in got)

"""GPU: per-song prompts on the particle stream and the shared prefill of the lock-step pool -- the two
kernels bitwise against numpy and against the kernels they stand in for, then generate_particles(slots=, prompts=[...],
bank=) end to end on the small fixture model.

1. cwlt_particle_refill_bank against numpy: groups 1, 3, 130 x K 2, 7, 64 and (2 groups, K 1024); 2 layers; bank 1, 3 and
   groups + 1 (entries wrap); fresh patterns none, all, some groups, a group with only some rows fresh, fresh rows with
   id -1, and a group whose rows ask for different entries.  Sentinel-filled state and logits change only in the fresh
   rows, the padding columns past n_logits keep the sentinel; with whole groups fresh the result is
   cwlt_stream_refill_bank's given song = id // K.  State sizes with one and with several workgroups.
2. cwlt_particle_release_bank against sampling.particle_release_bank on the group shapes of
   tests/test_particles_stream_gpu.py: ready 0 (everything parks, ctl[1] unmoved), ready inside the candidates,
   ready >= n_songs; bar and cap from the tables; with ready >= n_songs and constant tables every array is
   cwlt_particle_release's.
3. End to end, 7 songs x 4 particles, resample_every 4, chunk 16, bar_cond 9, max_tokens 48, everything on at ess 1,
   prompts the first 1, 2, 3, 5, 8, 12 and 17 rows of seven songs of generate_batch: (i) - (viii) below.
"""
import os

import numpy as np
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, ops, sampling
from rlmg_amd.generation import Constraint, Grammar, Preference

from test_blend_gpu import FIX, _bits, _same, _small_model, _word2event

pytestmark = pytest.mark.gpu
SENT = -1234567


def _d(cuda, x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(cuda)


def _i32(x):
    return x.view(np.int32)


# ---- 1. the refill -------------------------------------------------------------------------------------------------------
LAYERS, N_LOGITS, LD, LD_BANK = 2, 37, 41, 40
PATTERNS = ("none", "all", "some groups", "partial", "no id", "mixed")


def _split(flat, n, sf, zf):
    """The (LAYERS, n, sf) S rows and (LAYERS, n, zf) Z rows of a flat state of n slots (views)."""
    per = flat.reshape(LAYERS, n * (sf + zf))
    return per[:, :n * sf].reshape(LAYERS, n, sf), per[:, n * sf:].reshape(LAYERS, n, zf)


def _pattern(rng, how, groups, K, bank):
    """-> (fresh, id) of groups * K rows.  Every group holds a song of its own (so entries wrap at bank <= groups)."""
    rows = groups * K
    song = rng.permutation(groups + 40)[:groups].astype(np.int64)
    pid = (song[:, None] * K + np.arange(K)).reshape(-1)
    fresh = np.zeros(rows, dtype=np.int64)
    pick = rng.random(groups) < 0.5
    pick[rng.integers(groups)] = True                                   # at least one group
    if how == "all":
        fresh[:] = 1
    elif how == "some groups":
        fresh[np.repeat(pick, K)] = rng.integers(1, 4, int(pick.sum()) * K)     # any non-zero flag counts
    elif how == "partial":                                              # some rows of the picked groups, the last row of
        fresh[np.repeat(pick, K) & (rng.random(rows) < 0.5)] = 1        # the pool among them
        fresh[-1] = 1
    elif how == "no id":                                                # fresh rows without a particle: not written
        fresh[:] = 1
        last = pid[-1]
        pid[rng.random(rows) < 0.4] = -1
        pid[0], pid[-1] = -1, last
    elif how == "mixed":                                                # rows of one group that ask for several entries
        fresh[:] = 1
        pid = (rng.integers(0, groups + 40, rows) * K + np.tile(np.arange(K), groups)).astype(np.int64)
    return fresh, pid


@pytest.mark.parametrize("groups,K", [(g, k) for g in (1, 3, 130) for k in (2, 7, 64)] + [(2, 1024)])
def test_refill_bank_against_numpy(cuda, groups, K):
    rows = groups * K
    sf, zf = (16, 8) if rows > 1000 and K != 1024 else (512, 136)       # one workgroup, or 324 float4: two
    rng = np.random.default_rng([groups, K])
    state0 = np.full(LAYERS * rows * (sf + zf), SENT, dtype=np.float32)
    logits0 = np.full((rows, LD), SENT, dtype=np.float32)
    d_state0, d_logits0 = _d(cuda, state0), _d(cuda, logits0)
    for bank in (1, 3, groups + 1):
        bank_state = rng.normal(0, 3, LAYERS * bank * (sf + zf)).astype(np.float32)
        bank_logits = rng.normal(0, 3, (bank, LD_BANK)).astype(np.float32)
        d_bank, d_blogits = _d(cuda, bank_state), _d(cuda, bank_logits)
        bS, bZ = _split(bank_state, bank, sf, zf)
        for how in PATTERNS:
            fresh, pid = _pattern(rng, how, groups, K, bank)
            d_fresh, d_pid = _d(cuda, fresh), _d(cuda, pid)
            state, logits = d_state0.clone(), d_logits0.clone()
            ops.particle_refill_bank(state, d_bank, LAYERS, sf, zf, logits, d_blogits[:, :N_LOGITS], d_fresh, d_pid, K)
            hit = (fresh != 0) & (pid >= 0)
            e = np.where(hit, pid // K % bank, 0)
            want = state0.copy()
            S, Z = _split(want, rows, sf, zf)
            S[:, hit], Z[:, hit] = bS[:, e[hit]], bZ[:, e[hit]]
            want_logits = logits0.copy()
            want_logits[hit, :N_LOGITS] = bank_logits[e[hit], :N_LOGITS]
            where = (groups, K, bank, how)
            assert np.array_equal(_i32(state.cpu().numpy()), _i32(want)), where
            assert np.array_equal(_i32(logits.cpu().numpy()), _i32(want_logits)), where
            assert hit.any() == (how != "none")
            if how in ("none", "all", "some groups"):                   # whole groups: the per-row kernel, row by row
                state2, logits2 = d_state0.clone(), d_logits0.clone()
                ops.stream_refill_bank(state2, d_bank, LAYERS, sf, zf, logits2, d_blogits[:, :N_LOGITS], d_fresh,
                                       torch.div(d_pid, K, rounding_mode="floor"))
                assert torch.equal(state.view(torch.int32), state2.view(torch.int32)), where
                assert torch.equal(logits.view(torch.int32), logits2.view(torch.int32)), where


def test_refill_bank_binding_refusals(cuda):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=cuda)       # noqa: E731
    fresh, pid = z(8, dt=torch.int64), z(8, dt=torch.int64)
    good = dict(state=z(2 * 8 * 24), bank_state=z(2 * 3 * 24), n_layer=2, s_floats=16, z_floats=8, logits=z(8, 12),
                bank_logits=z(3, 10), fresh=fresh, pid=pid, particles=4)
    ops.particle_refill_bank(**good)
    for kw, err in ((dict(particles=3), ValueError), (dict(state=z(2 * 8 * 24 + 4)), ValueError),
                    (dict(bank_state=z(2 * 2 * 24)), ValueError), (dict(pid=z(7, dt=torch.int64)), TypeError),
                    (dict(fresh=z(8, dt=torch.int32)), TypeError), (dict(logits=z(8, 9)), ValueError),
                    (dict(state=z(2 * 8 * 24, dt=torch.float64)), TypeError)):
        args = dict(good)
        args.update(kw)
        with pytest.raises(err):
            ops.particle_refill_bank(**args)


# ---- 2. the release ------------------------------------------------------------------------------------------------------
NAMES = ("pos", "bar", "cap", "length", "fresh")


def _release_inputs(groups, K, rng):
    assigned0 = groups + 5
    song = rng.permutation(assigned0)[:groups].astype(np.int64)         # unique songs below the assigned counter
    song[rng.random(groups) < 0.2] = -1
    done = (rng.random((groups, K)) < 0.5).astype(np.int64) * rng.integers(1, 3, (groups, K))
    done[rng.random(groups) < 0.4] = 1
    done[-1] = 1                                                        # the last group is a candidate
    done[song < 0] = 1
    n_cand = int(((song < 0) | (done != 0).all(1)).sum())
    rows = groups * K
    c = dict(groups=groups, K=K, assigned0=assigned0, song=song, done=done.reshape(-1), n_cand=n_cand,
             n_songs=assigned0 + n_cand + 5,
             pid=np.where(song[:, None] >= 0, song[:, None] * K + np.arange(K), -1).astype(np.int64).reshape(-1),
             pos=rng.integers(0, 90, rows), bar=rng.integers(1, 5, rows), cap=rng.integers(40, 50, rows),
             length=rng.integers(1, 40, rows), fresh=rng.integers(0, 2, rows),
             lw=rng.normal(0, 9, rows).astype(np.float32), log_z=rng.normal(0, 9, groups).astype(np.float32))
    c["bar0_all"] = rng.integers(1, 6, c["n_songs"]).astype(np.int64)
    c["cap_all"] = rng.integers(20, 60, c["n_songs"]).astype(np.int64)
    return c


def _release(cuda, c, ready=None, bar0_all=None, cap_all=None, scalars=None):
    """One release on the device -> every array it may write, by name.  scalars (bar0, cap0): cwlt_particle_release."""
    K, n_songs = c["K"], c["n_songs"]
    dev = {k: _d(cuda, c[k]) for k in NAMES + ("song", "pid", "done", "lw", "log_z")}
    dev["out_lw"] = torch.full((n_songs * K,), float(SENT), dtype=torch.float32, device=cuda)
    dev["out_len"] = torch.full((n_songs * K,), SENT, dtype=torch.int64, device=cuda)
    dev["out_logz"] = torch.full((n_songs,), float(SENT), dtype=torch.float32, device=cuda)
    tail = (dev["song"], dev["pid"], dev["pos"], dev["bar"], dev["cap"], dev["length"], dev["done"], dev["fresh"],
            dev["lw"], dev["log_z"])
    outs = (dev["out_lw"], dev["out_len"], dev["out_logz"])
    if scalars is not None:
        dev["ctl"] = _d(cuda, np.array([77, c["assigned0"], 3], dtype=np.int64))
        ops.particle_release(K, n_songs, scalars[0], scalars[1], *tail, dev["ctl"], *outs)
    else:
        dev["ctl"] = _d(cuda, np.array([77, c["assigned0"], 3, ready], dtype=np.int64))
        ops.particle_release_bank(K, n_songs, _d(cuda, bar0_all), _d(cuda, cap_all), *tail, dev["ctl"], *outs)
    return {k: v.cpu().numpy() for k, v in dev.items()}


@pytest.mark.parametrize("groups,K", [(1, 2), (3, 64), (130, 7), (1025, 2), (4096, 2)])
def test_release_bank_against_restatement(cuda, groups, K):
    rng = np.random.default_rng([groups, K, 36])
    c = _release_inputs(groups, K, rng)
    n_songs, a0 = c["n_songs"], c["assigned0"]
    song, pid, lw, log_z = c["song"], c["pid"], c["lw"], c["log_z"]
    for ready in (0, a0 + c["n_cand"] // 2, n_songs, n_songs + 9):
        got = _release(cuda, c, ready, c["bar0_all"], c["cap_all"])
        take, rel, assigned, finished = sampling.particle_release_bank(song, c["done"], K, a0, 3, ready, n_songs)
        where = (groups, K, ready)
        if ready == 0:
            assert (take[take != -2] == -1).all() and assigned == a0
        elif ready < n_songs:
            assert (take >= 0).sum() == c["n_cand"] // 2 and take[-1] == -1, where
        else:
            assert (take != -1).all() and (take >= 0).any() and assigned == a0 + c["n_cand"], where
        cand_r, hand_r, rel_r = np.repeat(take != -2, K), np.repeat(take >= 0, K), np.repeat(rel, K)
        took = np.repeat(np.maximum(take, 0), K)
        w_lw, w_len, w_lz = np.full(n_songs * K, SENT, np.float32), np.full(n_songs * K, SENT, np.int64), \
            np.full(n_songs, SENT, np.float32)
        w_lw[pid[rel_r]], w_len[pid[rel_r]] = lw[rel_r], c["length"][rel_r]
        w_lz[song[rel]] = log_z[rel]
        # a finished song's outputs are written whether or not its group got a new song
        assert np.array_equal(_i32(got["out_lw"]), _i32(w_lw)) and np.array_equal(got["out_len"], w_len), where
        assert np.array_equal(_i32(got["out_logz"]), _i32(w_lz)), where
        assert np.array_equal(got["song"], np.where(take != -2, take, song)), where
        assert np.array_equal(got["pid"], np.where(hand_r, took * K + np.tile(np.arange(K), groups),
                                                   np.where(cand_r, -1, pid))), where
        assert np.array_equal(got["ctl"], [77, assigned, finished, ready]), where
        for name, value in (("pos", 0), ("bar", c["bar0_all"][took]), ("cap", c["cap_all"][took]), ("length", 0),
                            ("fresh", 1)):
            assert np.array_equal(got[name], np.where(hand_r, value, c[name])), (where, name)
        assert np.array_equal(got["done"], np.where(hand_r, 0, np.where(cand_r, 1, c["done"]))), where
        assert np.array_equal(_i32(got["lw"]), _i32(np.where(hand_r, np.float32(0), lw))), where
        assert np.array_equal(_i32(got["log_z"]), _i32(np.where(take >= 0, np.float32(0), log_z))), where
    # the songs run out below the gate: n_songs is the limit
    c2 = dict(c, n_songs=a0 + c["n_cand"] - 1, bar0_all=c["bar0_all"][:a0 + c["n_cand"] - 1],
              cap_all=c["cap_all"][:a0 + c["n_cand"] - 1])
    got = _release(cuda, c2, c2["n_songs"] + 3, c2["bar0_all"], c2["cap_all"])
    take, _, assigned, finished = sampling.particle_release_bank(song, c["done"], K, a0, 3, c2["n_songs"] + 3,
                                                                 c2["n_songs"])
    assert take[-1] == -1 and np.array_equal(got["song"], np.where(take != -2, take, song))
    assert np.array_equal(got["ctl"], [77, assigned, finished, c2["n_songs"] + 3]) and assigned == c2["n_songs"]


@pytest.mark.parametrize("groups,K", [(1, 2), (3, 64), (130, 7), (1025, 2), (4096, 2)])
def test_release_bank_open_gate_is_the_plain_release(cuda, groups, K):
    rng = np.random.default_rng([groups, K, 37])
    c = _release_inputs(groups, K, rng)
    for n_songs in (c["n_songs"], c["assigned0"] + c["n_cand"] - 1, c["assigned0"] + c["n_cand"] // 2):
        c = dict(c, n_songs=n_songs)
        want = _release(cuda, c, scalars=(2, 45))
        for ready in (n_songs, n_songs + 100):
            got = _release(cuda, c, ready, np.full(n_songs, 2, np.int64), np.full(n_songs, 45, np.int64))
            for name in want:
                a, b = got[name], want[name]
                if name == "ctl":
                    a = a[:3]
                assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32)), (groups, K, ready, name)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------
N, K4, BAR_COND, CAP, EVERY, CHUNK, SEED = 7, 4, 9, 48, 4, 16, 21
P_ROWS = (1, 2, 3, 5, 8, 12, 17)
ONE_BLOCK = dict(bank=2, prefill_rows=2 * 17)                           # blocks of 2 songs, a bank of one block


def _parity(windows, mask):
    """0 / 1: the parity of the pitch class of the window's first row (tests/test_reward_stream_gpu.py)."""
    return (windows[:, 0, 3] % 2).float()


@pytest.fixture(scope="module")
def world(cuda):
    seed = int(FIX["fill_seed"])
    w2e = _word2event()
    w = {"net": _small_model(cuda, seed), "ref": _small_model(cuda, seed + 1), "w2e": w2e}
    w["tight"] = Constraint(w2e, per_bar={"pitch": [[5, 6, 7], [20, 21, 22], [40, 41, 42]]}, cycle=True)
    w["plain"] = dict(constraints=w["tight"], grammar=Grammar(w2e), sampler="categorical")
    w["all on"] = dict(reference=w["ref"], alpha=0.7, preferences=Preference(w2e, repeat={"pitch": (0.5, 0.5)}, decay=0.9),
                       **w["plain"])
    # the prompts: prefixes of seven songs drawn under the same constraints and grammar, the longest prefix of the
    # longest song
    torch.manual_seed(5)
    songs = generation.generate_batch(w["net"], w2e, N, bar_cond=BAR_COND, max_tokens=CAP, **w["plain"])
    by_length = sorted(songs, key=len, reverse=True)
    assert all(len(s) > p for s, p in zip(by_length, sorted(P_ROWS, reverse=True)))
    w["prompts"] = [by_length[N - 1 - i][:p].copy() for i, p in enumerate(P_ROWS)]
    bars = [1 + sum(w2e["bar-beat"][int(r[2])] == "Bar" for r in p[1:]) for p in w["prompts"]]
    assert len(set(bars)) >= 2, bars                                    # at least two distinct prompt bar counts
    w["bars"] = bars
    return w


def _particles(w, config="all on", **kw):
    torch.manual_seed(SEED)
    kw.setdefault("ess", 1.0)
    return generation.generate_particles(w["net"], w["w2e"], N, K4, bar_cond=BAR_COND, max_tokens=CAP, chunk=CHUNK,
                                         resample_every=EVERY, prompts=w["prompts"], **w[config], **kw)


def _same_sets(a, b, rewards=False):
    ok = (_same(a.songs, b.songs) and _bits(a.logprobs, b.logprobs) and
          np.array_equal(_i32(a.log_weights), _i32(b.log_weights)) and a.log_evidence == b.log_evidence and
          np.array_equal(_i32(a.ess), _i32(b.ess)) and np.array_equal(a.resampled, b.resampled) and
          np.array_equal(a.ancestors, b.ancestors) and
          np.array_equal(_i32(a.event_log_weights), _i32(b.event_log_weights)))
    if rewards:
        ok = ok and _bits(a.rewards, b.rewards) and a.event_rewards.shape == b.event_rewards.shape and \
            np.array_equal(_i32(a.event_rewards), _i32(b.event_rewards)) and a.beta == b.beta
    return ok


def _differ(a, b, rewards=False):
    assert len(a) == len(b) == N
    return [i for i, (x, y) in enumerate(zip(a, b)) if not _same_sets(x, y, rewards)]


@pytest.fixture(scope="module")
def lock(world):
    """The lock-step pool, every row prefilled: the parent's path."""
    return _particles(world, prefill="gemm", share_prefill=False)


def _with_stats(w, slots, config="all on", reward=None, **bank):
    kw = w[config]
    torch.manual_seed(SEED)
    heads, caps, plan = generation._particle_setup("generate_particles", w["net"], w["w2e"], N, K4, EVERY, 1.0, BAR_COND,
                                                   CAP, w["prompts"], "categorical", CHUNK, "blas", kw["constraints"],
                                                   kw["grammar"], kw.get("reference"), kw.get("alpha"),
                                                   kw.get("preferences"), pool=slots)
    stats = {}
    sets = generation._run_particle_stream(w["net"], w["w2e"], heads, caps, plan, N, K4, slots, EVERY, 1.0, BAR_COND,
                                           CHUNK, None, heads[0], stats=stats, reward=reward, **bank)
    return sets, stats


@pytest.fixture(scope="module")
def stream3(world):
    return _with_stats(world, 3, **ONE_BLOCK)


def test_preconditions_of_the_one_block_run(world, lock, stream3):
    """(i) 3 slots on a bank of one block of two songs: the run equals the pool, groups were parked by the gate, entries
    were reused, and the comparison is not vacuous."""
    sets, stats = stream3
    assert _differ(sets, lock) == []
    starts = stats["start_steps"]
    print("particle bank stream at 3 slots, bank 2: starts %s, %d steps, block %d, %d blocks, gated chunks %d, gate wait "
          "%d, waiting %d and idle %d group-steps, prompt bars %s, lengths %s"
          % (starts, stats["steps"], stats["block"], stats["prefill_blocks"], stats["gated_chunks"],
             stats["gate_wait_group_steps"], stats["wait_group_steps"], stats["idle_group_steps"], world["bars"],
             [max(len(s) for s in ps.songs) for ps in sets]))
    assert stats["block"] == 2 and stats["bank"] == 2 and stats["prefill_blocks"] == 4
    assert stats["gate_wait_group_steps"] > 0 and stats["gated_chunks"] > 0
    assert sorted(starts[:2]) == [0, 0] and all(s > 0 and s % EVERY == 0 for s in starts[2:])
    late = [ps for ps, s in zip(sets, starts) if s > 0]
    assert any((ps.ancestors != np.arange(K4)).any() for ps in late)     # an event moves rows in a song started later
    assert all((s[:p] == h).all() for ps, h, p in zip(sets, world["prompts"], P_ROWS) for s in ps.songs)
    assert [len(h) for h in world["prompts"]] == list(P_ROWS)


@pytest.mark.parametrize("slots", [7, 3, 1])
def test_stream_is_the_lock_step_run(world, lock, slots):
    """(ii) slots 7, 3 and 1, on the one-block bank and on stream_bank_plan's: the pool's sets, bit for bit."""
    assert _differ(_particles(world, slots=slots, **ONE_BLOCK), lock) == []
    assert _differ(_particles(world, slots=slots, bank="auto"), lock) == []


def test_ess_zero_is_generate_batch(world):
    """(iii) ess = 0: no row ever moves, and the songs and pairs are generate_batch's on 28 rows with the prompts
    repeated (a path this change leaves alone)."""
    w = world
    sets = _particles(w, ess=0, slots=3, **ONE_BLOCK)
    torch.manual_seed(SEED)
    songs, lps = generation.generate_batch(w["net"], w["w2e"], N * K4, bar_cond=BAR_COND, max_tokens=CAP, chunk=CHUNK,
                                           prompts=[p for p in w["prompts"] for _ in range(K4)], prefill="gemm",
                                           return_logprobs=True, **w["all on"])
    assert _same([s for ps in sets for s in ps.songs], songs)
    assert _bits([l for ps in sets for l in ps.logprobs], lps)
    assert all(not ps.resampled.any() and (ps.ancestors == np.arange(K4)).all() for ps in sets)


def test_graph_is_eager(world, stream3, monkeypatch):
    """(iv)"""
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    eager = _particles(world, slots=3, **ONE_BLOCK)
    monkeypatch.undo()
    assert _differ(eager, stream3[0]) == []


def test_without_a_reference(world):
    """(v) one bank, not two: constraints and grammar only."""
    want = _particles(world, "plain", prefill="gemm", share_prefill=False)
    assert _differ(_particles(world, "plain", slots=3, **ONE_BLOCK), want) == []
    assert _differ(_particles(world, "plain", slots=2, bank="auto"), want) == []


def test_reward_on_the_bank_stream(world):
    """(vi) a 0 / 1 reward at reward_window 8, resample_every 4: rewards, event_rewards and beta included."""
    kw = dict(reward=_parity, reward_window=8, beta=100.0)
    want = _particles(world, prefill="gemm", share_prefill=False, **kw)
    assert any(ps.resampled.any() for ps in want)
    for bank in (ONE_BLOCK, dict(bank="auto")):
        got = _particles(world, slots=3, **bank, **kw)
        assert _differ(got, want, rewards=True) == [], bank
        for ps, p in zip(got, P_ROWS):
            for k in range(K4):
                drawn = ps.songs[k][p:]
                assert np.array_equal(ps.rewards[k], np.float32([drawn[j, 3] % 2 for j in range(0, len(drawn), 8)]))


@pytest.mark.parametrize("config", ["all on", "plain"])
def test_pool_shares_the_prefill(world, config):
    """(vii) the lock-step pool: share_prefill=None is False bit for bit, with and without a reference, and prefills the
    songs' prompts, not the rows'."""
    w = world
    kw = w[config]
    out = {}
    for share in (False, True):
        torch.manual_seed(SEED)
        heads, caps, plan = generation._particle_setup("generate_particles", w["net"], w["w2e"], N, K4, EVERY, 1.0,
                                                       BAR_COND, CAP, w["prompts"], "categorical", CHUNK, "gemm",
                                                       kw["constraints"], kw["grammar"], kw.get("reference"),
                                                       kw.get("alpha"), kw.get("preferences"))
        stats = {}
        out[share] = generation._run_particles(w["net"], w["w2e"], heads, caps, plan, K4, EVERY, 1.0, BAR_COND, CHUNK,
                                               None, "gemm", stats=stats, share_prefill=share), stats
    assert out[False][1]["prefilled_prompts"] == N * K4 and out[True][1]["prefilled_prompts"] == N
    assert _differ(out[True][0], out[False][0]) == []
    assert _differ(_particles(w, config, prefill="gemm"), out[False][0]) == []          # None shares under "gemm"
    assert _differ(_particles(w, config, prefill="gemm", share_prefill=True), out[False][0]) == []
    assert any(ps.resampled.any() for ps in out[False][0])


def test_songs_score_and_generate(world, stream3, tmp_path):
    """(viii) score_songs reproduces the drawn pairs within the 1e-4 the stream tests use; generate(slots=, particles=,
    prompts=[...], bank="auto") writes the songs of generate_particles."""
    w, kw = world, world["all on"]
    songs = [s for ps in stream3[0] for s in ps.songs]
    lps = [l for ps in stream3[0] for l in ps.logprobs]
    scored = generation.score_songs(w["net"], w["w2e"], songs, **kw)
    worst = 0.0
    for s, lp, sc, p in zip(songs, lps, scored, np.repeat(P_ROWS, K4)):
        assert lp.shape == (len(s) - p, 6, 2) and np.isfinite(lp).all()
        worst = max(worst, float(np.abs(lp - sc[p - 1:]).max()))
    print("particle bank stream: generated against scored log-probs, worst |difference| = %.3g" % worst)
    assert worst <= 1e-4
    net, w2e = w["net"], w["w2e"]
    free = torch.cuda.memory_allocated()
    for bad, msg in ((dict(bank=3, prefill_rows=34), "multiple of the prefill block"), (dict(bank=0), "bank must be"),
                     (dict(), "one shared")):
        with pytest.raises(ValueError, match=msg):
            generation.generate_particles(net, w2e, N, K4, slots=3, resample_every=EVERY, chunk=CHUNK,
                                          prompts=w["prompts"], **bad)
    assert torch.cuda.memory_allocated() == free                        # nothing was made on the device
    opts = dict(constraints=w["tight"], grammar=kw["grammar"], ess=1.0, resample_every=EVERY)
    torch.manual_seed(SEED)
    sets = generation.generate_particles(net, w2e, N, K4, bar_cond=BAR_COND, max_tokens=CAP, slots=2,
                                         prompts=w["prompts"], bank="auto", **opts)
    torch.manual_seed(SEED)
    stats = generation.generate(net, w2e, n_songs=N, bar_cond=BAR_COND, max_tokens=CAP, slots=2, particles=K4,
                                prompts=w["prompts"], bank="auto", path_gendir=str(tmp_path),
                                stats_path=str(tmp_path / "stats.json"), log=lambda s: None, logprobs=True, **opts)
    assert len(stats["words_len_list"]) == N
    for i, ps in enumerate(sets):
        song = np.load(os.path.join(str(tmp_path), "get_%d.npy" % i))
        lp = np.load(os.path.join(str(tmp_path), "get_%d_logp.npy" % i))
        hits = [k for k in range(K4) if song.shape == ps.songs[k].shape and (song == ps.songs[k]).all()]
        assert hits and len(song) == stats["words_len_list"][i] and (song[:P_ROWS[i]] == w["prompts"][i]).all()
        assert any(np.array_equal(lp.view(np.int32), ps.logprobs[k].view(np.int32)) for k in hits)

"""GPU: particle generation on the stream -- the kernels one by one, bitwise against numpy or the
lock-step kernels, then generation.generate_particles(slots=) end to end on the small fixture model.

1. cwlt_particle_resample_keyed against cwlt_particle_resample: groups 1, 3, 130 x K 2, 7, 64, 65, 1024 x the weight
   cases of tests/test_particles_cpu.py.  Identity songs and clocks (e + 1) R: every output equal.  Songs permuted over
   the groups and clocks that differ per group: group j's outputs are the plain kernel's for group song[j] at event
   pos[j] // R - 1 on the same weights.  Groups with song -1 and sentinel-filled lw / log_z: untouched, anc the identity.
2. cwlt_particle_release and cwlt_particle_fill against sampling.particle_release: (groups, K) = (1, 2), (3, 64),
   (130, 7), (1025, 2) -- the last a second chunk of the one workgroup -- with n_songs such that the songs run out inside
   the first chunk, at the last candidate (inside the second chunk at 1025 groups) and not at all; sentinel-filled output
   arrays change only at released ids; beat (1 int64) and seen (the small model's sum n_class floats) rows of handed
   groups equal their beat0 / seen0 rows.
3. cwlt_particle_advance against numpy: rows 1, 65, 2050, 6 and 8 attributes, the ring row across the wrap, rows
   without a song.
4. End to end, 7 songs x 4 particles, resample_every 4, chunk 16, bar_cond 4, max_tokens 48: (i) - (vi) below.
"""
import os

import numpy as np
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, ops, sampling
from rlmg_amd.generation import Constraint, Grammar, Preference

from test_blend_gpu import FIX, N_CLASS, _bits, _same, _small_model, _word2event
from test_particles_cpu import CASES, resample_case

pytestmark = pytest.mark.gpu
SENT = -1234567
GROUPS, KS, R = (1, 3, 130), (2, 7, 64, 65, 1024), 4


def _d(cuda, x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(cuda)


# ---- 1. keyed resample ---------------------------------------------------------------------------------------------------
def _outs(cuda, groups, K):
    return (torch.full((groups * K,), -7, dtype=torch.int64, device=cuda),
            torch.full((groups,), -1.0, dtype=torch.float32, device=cuda),
            torch.full((groups,), -1.0, dtype=torch.float32, device=cuda),
            torch.full((groups,), -1, dtype=torch.int32, device=cuda))


def _plain(cuda, lw, done, K, seed, event, log_z0):
    groups = lw.shape[0]
    lw_d, lz = _d(cuda, lw.reshape(-1)), _d(cuda, log_z0)
    anc, u, ess, res = _outs(cuda, groups, K)
    ops.particle_resample(lw_d, _d(cuda, done.reshape(-1)), K, 1.0, seed, event, anc, u, ess, res, lz)
    return [t.cpu().numpy() for t in (anc, u, ess, res, lz, lw_d)]


def _keyed(cuda, lw, done, K, seed, song, pos, log_z0, stride):
    groups = lw.shape[0]
    lw_d, lz = _d(cuda, lw.reshape(-1)), _d(cuda, log_z0)
    anc, u, ess, res = _outs(cuda, groups, K)
    ops.particle_resample_keyed(lw_d, _d(cuda, done.reshape(-1)), K, 1.0, seed, _d(cuda, song), _d(cuda, pos), R, anc, u,
                                ess, res, lz, pos_stride=stride)
    return [t.cpu().numpy() for t in (anc, u, ess, res, lz, lw_d)]


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32 if a.itemsize == 4 else np.int64),
                                                                         b.view(np.int32 if b.itemsize == 4 else np.int64))


@pytest.mark.parametrize("K", KS)
def test_keyed_resample_is_the_plain_kernel(cuda, K):
    for groups in GROUPS:
        for case in CASES:
            lw, done = resample_case(case, groups, K, seed=groups)
            rng = np.random.default_rng([K, groups, CASES.index(case)])
            log_z0 = rng.normal(0, 5, groups).astype(np.float32)
            where = (case, groups)
            # identity songs, every clock (e + 1) R, the clocks per row (the default stride)
            want = _plain(cuda, lw, done, K, 99, 3, log_z0)
            got = _keyed(cuda, lw, done, K, 99, np.arange(groups), np.full(groups * K, 4 * R, dtype=np.int64), log_z0,
                         None)
            assert all(_eq(a, b) for a, b in zip(got, want)), where
            # permuted songs, two clocks (one off a boundary: the index is the floor), one group without a song
            song = rng.permutation(groups).astype(np.int64)
            ev = rng.integers(0, 2, groups) * 3 + 2                     # event 2 or 5
            pos = (ev + 1) * R + rng.integers(0, R, groups)
            none = groups - 1 if groups > 1 else None
            lw_in, lz_in, song_in = lw.copy(), log_z0.copy(), song.copy()
            if none is not None:
                song_in[none] = -1
                lw_in[none], lz_in[none] = SENT, SENT
            got = _keyed(cuda, lw_in, done, K, 99, song_in, pos.astype(np.int64), lz_in, 1)
            event, skip = sampling.particle_event_keys(song_in, pos, R)
            assert np.array_equal(event, ev) and skip.sum() == (none is not None)
            perm_lw, perm_done = np.empty_like(lw), np.empty_like(done)
            perm_lw[song], perm_done[song] = lw, done                   # plain group song[j] holds group j's weights
            perm_lz = np.empty_like(log_z0)
            perm_lz[song] = log_z0
            plain = {e: _plain(cuda, perm_lw, perm_done, K, 99, int(e), perm_lz) for e in np.unique(ev)}
            g_anc, g_lw = got[0].reshape(groups, K), got[5].reshape(groups, K)
            for j in range(groups):
                if j == none:
                    assert (g_anc[j] == j * K + np.arange(K)).all() and got[3][j] == 0 and got[1][j] == 0
                    assert (g_lw[j] == SENT).all() and got[4][j] == SENT, where
                    continue
                p, s = plain[ev[j]], int(song[j])
                assert np.array_equal(g_anc[j] - j * K, p[0].reshape(groups, K)[s] - s * K), (where, j)
                for i in (1, 2, 3, 4):
                    assert _eq(got[i][j:j + 1], p[i][s:s + 1]), (where, j, i)
                assert _eq(g_lw[j], p[5].reshape(groups, K)[s]), (where, j)
    # a lone group without a song
    lw, done = resample_case("normal3", 1, K, seed=1)
    got = _keyed(cuda, np.full_like(lw, SENT), done, K, 99, np.array([-1]), np.array([8]), np.float32([SENT]), 1)
    assert (got[0] == np.arange(K)).all() and got[3][0] == 0 and (got[5] == SENT).all() and got[4][0] == SENT


# ---- 2. release and fill -------------------------------------------------------------------------------------------------
W = int(sum(N_CLASS))


def _release_case(cuda, groups, K, how, rng):
    assigned0 = groups + 5
    song = rng.permutation(assigned0)[:groups].astype(np.int64)         # unique songs below the assigned counter
    song[rng.random(groups) < 0.2] = -1
    done = (rng.random((groups, K)) < 0.5).astype(np.int64) * rng.integers(1, 3, (groups, K))
    done[rng.random(groups) < 0.4] = 1
    done[-1] = 1                                                        # the last group is a candidate
    done[song < 0] = 1
    n_cand = int(((song < 0) | (done != 0).all(1)).sum())
    n_songs = assigned0 + {"enough": n_cand + 5, "last": n_cand - 1, "middle": n_cand // 2}[how]
    pid = np.where(song[:, None] >= 0, song[:, None] * K + np.arange(K), -1).astype(np.int64)
    rows = groups * K
    st = dict(pos=rng.integers(0, 90, rows), bar=rng.integers(1, 5, rows), cap=rng.integers(40, 50, rows),
              length=rng.integers(1, 40, rows), fresh=rng.integers(0, 2, rows))
    lw = rng.normal(0, 9, rows).astype(np.float32)
    log_z = rng.normal(0, 9, groups).astype(np.float32)
    ctl = np.array([77, assigned0, 3], dtype=np.int64)
    beat0 = rng.integers(-1, 16, n_songs * K).astype(np.int64)
    seen0 = rng.random((n_songs * K, W)).astype(np.float32)
    beat, seen = rng.integers(-1, 16, rows).astype(np.int64), rng.random((rows, W)).astype(np.float32)
    dev = {k: _d(cuda, v) for k, v in st.items()}
    d_song, d_pid, d_done, d_lw, d_lz, d_ctl = (_d(cuda, x) for x in (song, pid.reshape(-1), done.reshape(-1), lw, log_z,
                                                                   ctl))
    out_lw = torch.full((n_songs * K,), float(SENT), dtype=torch.float32, device=cuda)
    out_len = torch.full((n_songs * K,), SENT, dtype=torch.int64, device=cuda)
    out_lz = torch.full((n_songs,), float(SENT), dtype=torch.float32, device=cuda)
    ops.particle_release(K, n_songs, 2, 45, d_song, d_pid, dev["pos"], dev["bar"], dev["cap"], dev["length"], d_done,
                         dev["fresh"], d_lw, d_lz, d_ctl, out_lw, out_len, out_lz)
    d_beat, d_seen = _d(cuda, beat), _d(cuda, seen)
    ops.particle_fill(d_beat, _d(cuda, beat0), dev["fresh"], d_pid)
    ops.particle_fill(d_seen, _d(cuda, seen0), dev["fresh"], d_pid)
    # the restatement
    take, rel, assigned, finished = sampling.particle_release(song, done.reshape(-1), K, assigned0, 3, n_songs)
    cand_r, hand_r, rel_r = np.repeat(take != -2, K), np.repeat(take >= 0, K), np.repeat(rel, K)
    new_pid = np.where(hand_r, np.repeat(take, K) * K + np.tile(np.arange(K), groups),
                       np.where(cand_r, -1, pid.reshape(-1)))
    w_lw, w_len, w_lz = np.full(n_songs * K, SENT, np.float32), np.full(n_songs * K, SENT, np.int64), \
        np.full(n_songs, SENT, np.float32)
    w_lw[pid.reshape(-1)[rel_r]], w_len[pid.reshape(-1)[rel_r]] = lw[rel_r], st["length"][rel_r]
    w_lz[song[rel]] = log_z[rel]
    where = (groups, K, how)
    assert _eq(out_lw.cpu().numpy(), w_lw) and np.array_equal(out_len.cpu().numpy(), w_len), where
    assert _eq(out_lz.cpu().numpy(), w_lz), where
    assert np.array_equal(d_song.cpu().numpy(), np.where(take != -2, take, song)), where
    assert np.array_equal(d_pid.cpu().numpy(), new_pid), where
    assert np.array_equal(d_ctl.cpu().numpy(), [77, assigned, finished]), where
    for name, value in (("pos", 0), ("bar", 2), ("cap", 45), ("length", 0), ("fresh", 1)):
        assert np.array_equal(dev[name].cpu().numpy(), np.where(hand_r, value, st[name])), (where, name)
    assert np.array_equal(d_done.cpu().numpy(), np.where(hand_r, 0, np.where(cand_r, 1, done.reshape(-1)))), where
    assert _eq(d_lw.cpu().numpy(), np.where(hand_r, np.float32(0), lw)), where
    assert _eq(d_lz.cpu().numpy(), np.where(take >= 0, np.float32(0), log_z)), where
    # the fill: rows flagged fresh (the handed ones, and whatever was flagged before) with an id take that id's row
    fresh = np.where(hand_r, 1, st["fresh"]) != 0
    fill = fresh & (new_pid >= 0)
    safe = np.where(fill, new_pid, 0)
    assert np.array_equal(d_beat.cpu().numpy(), np.where(fill, beat0[safe], beat)), where
    assert _eq(d_seen.cpu().numpy(), np.where(fill[:, None], seen0[safe], seen)), where
    got_beat, got_seen = d_beat.cpu().numpy(), d_seen.cpu().numpy()
    assert (got_beat[hand_r] == beat0[new_pid[hand_r]]).all() and (got_seen[hand_r] == seen0[new_pid[hand_r]]).all()
    if how == "enough":
        assert (take != -1).all() and hand_r.any()
    else:
        assert take[-1] == -1                                           # the songs ran out at or before the last group
    if how == "last":
        assert (take[:-1] != -1).all()


@pytest.mark.parametrize("groups,K", [(1, 2), (3, 64), (130, 7), (1025, 2), (4096, 2)])
def test_release_against_restatement(cuda, groups, K):
    rng = np.random.default_rng([groups, K])
    for how in ("enough", "last", "middle"):
        _release_case(cuda, groups, K, how, rng)


# ---- 3. advance ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 65, 2050])
@pytest.mark.parametrize("A", [6, 8])
def test_advance_against_numpy(cuda, rows, A):
    rng = np.random.default_rng([rows, A])
    ring_rows = 5
    for t in (3, 4, 5, 12):                                             # the last row, the wrap, past it
        tok = rng.integers(0, 300, (rows, A)).astype(np.int64)
        pid = rng.integers(0, 1 << 20, rows).astype(np.int64)
        pid[rng.random(rows) < 0.3] = -1
        if rows > 1:
            pid[0], pid[-1] = -1, 5
        done = (rng.random(rows) < 0.5).astype(np.int64) * rng.integers(1, 3, rows)
        pos, fresh = rng.integers(0, 1 << 33, rows).astype(np.int64), rng.integers(0, 2, rows).astype(np.int64)
        ctl = np.array([t, 11, 7], dtype=np.int64)
        ring = torch.full((ring_rows, rows, A + 2), SENT, dtype=torch.int64, device=cuda)
        d_pos, d_fresh, d_ctl = _d(cuda, pos), _d(cuda, fresh), _d(cuda, ctl)
        ops.particle_advance(_d(cuda, tok), _d(cuda, pid), _d(cuda, done), d_pos, d_fresh, d_ctl, ring)
        want = np.full((ring_rows, rows, A + 2), SENT, dtype=np.int64)
        want[t % ring_rows, :, 0] = np.where(pid >= 0, pid, -1)
        want[t % ring_rows, :, 1:1 + A] = tok
        want[t % ring_rows, :, A + 1] = (pid >= 0) & (done != 0)
        assert np.array_equal(ring.cpu().numpy(), want), (rows, A, t)
        assert np.array_equal(d_pos.cpu().numpy(), pos + (pid >= 0)) and not d_fresh.any().item()
        assert np.array_equal(d_ctl.cpu().numpy(), [t + 1, 11, 7])


# ---- 4. end to end -------------------------------------------------------------------------------------------------------
N, K4, BAR_COND, CAP, EVERY, CHUNK, SEED = 7, 4, 4, 48, 4, 16, 21


@pytest.fixture(scope="module")
def world(cuda):
    seed = int(FIX["fill_seed"])
    w2e = _word2event()
    w = {"net": _small_model(cuda, seed), "ref": _small_model(cuda, seed + 1), "w2e": w2e}
    w["range"] = Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(5, 12)},
                            per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7]]}, cycle=True)
    w["tight"] = Constraint(w2e, per_bar={"pitch": [[5, 6, 7], [20, 21, 22], [40, 41, 42]]}, cycle=True)
    w["all on"] = dict(constraints=w["tight"], grammar=Grammar(w2e), reference=w["ref"], alpha=0.7,
                       preferences=Preference(w2e, repeat={"pitch": (0.5, 0.5)}, decay=0.9), sampler="categorical")
    return w


def _particles(w, **kw):
    torch.manual_seed(SEED)
    return generation.generate_particles(w["net"], w["w2e"], N, K4, bar_cond=BAR_COND, max_tokens=CAP, chunk=CHUNK,
                                         resample_every=EVERY, **kw)


def _same_sets(a, b):
    return (_same(a.songs, b.songs) and _bits(a.logprobs, b.logprobs) and
            np.array_equal(a.log_weights.view(np.int32), b.log_weights.view(np.int32)) and
            a.log_evidence == b.log_evidence and np.array_equal(a.ess.view(np.int32), b.ess.view(np.int32)) and
            np.array_equal(a.resampled, b.resampled) and np.array_equal(a.ancestors, b.ancestors) and
            np.array_equal(a.event_log_weights.view(np.int32), b.event_log_weights.view(np.int32)))


def _differ(a, b):
    return [i for i, (x, y) in enumerate(zip(a, b)) if not _same_sets(x, y)]


@pytest.fixture(scope="module")
def lock(world):
    """The lock-step pool of all 7 songs in the "all on" configuration, ess = 1."""
    return _particles(world, ess=1.0, **world["all on"])


@pytest.fixture(scope="module")
def stream3(world):
    return _particles(world, ess=1.0, slots=3, **world["all on"])


def test_stream_is_the_lock_step_run(world, lock, stream3):
    """(i) all 7 sets from slots = 7, 3 and 1 are the lock-step pool's, field by field and bit for bit."""
    w = world
    assert len(lock) == N and len(stream3) == N
    assert _differ(stream3, lock) == []
    for slots in (7, 1):
        assert _differ(_particles(w, ess=1.0, slots=slots, **w["all on"]), lock) == [], slots
    # at 3 slots songs 3 .. 6 start at a boundary > 0 (the run's own record of it), and events move rows in them
    torch.manual_seed(SEED)
    heads, caps, plan = generation._particle_setup("generate_particles", w["net"], w["w2e"], N, K4, EVERY, 1.0, BAR_COND,
                                                   CAP, None, "categorical", CHUNK, "blas", w["tight"],
                                                   w["all on"]["grammar"], w["ref"], 0.7,
                                                   w["all on"]["preferences"], pool=3)
    stats = {}
    again = generation._run_particle_stream(w["net"], w["w2e"], heads, caps, plan, N, K4, 3, EVERY, 1.0, BAR_COND, CHUNK,
                                            None, None, stats=stats)
    assert _differ(again, lock) == []
    starts = stats["start_steps"]
    print("particle stream at 3 slots: starts %s, %d steps, %d events, waiting %d and idle %d group-steps, lengths %s"
          % (starts, stats["steps"], stats["events"], stats["wait_group_steps"], stats["idle_group_steps"],
             [max(len(s) for s in ps.songs) for ps in again]))
    assert sorted(starts[:3]) == [0, 0, 0] and all(s > 0 and s % EVERY == 0 for s in starts[3:])
    late = [ps for ps, s in zip(stream3, starts) if s > 0]
    assert any((ps.ancestors != np.arange(K4)).any() for ps in late)
    # a song's rows cross a chunk boundary of the ring
    ends = [s + max(len(x) for x in ps.songs) - 1 for ps, s in zip(stream3, starts)]
    assert any(s // CHUNK != (e - 1) // CHUNK for s, e in zip(starts, ends))
    assert stats["events"] * EVERY == stats["steps"]


def test_shared_prompt(world, lock):
    """(ii) one shared prompt, prefilled once: the lock-step pool with prefill="gemm" and the prompt for every song."""
    w = world
    song = lock[0].songs[0]
    P = 5
    while P > 2 and 1 + sum(w["w2e"]["bar-beat"][int(r[2])] == "Bar" for r in song[1:P]) >= BAR_COND - 1:
        P -= 1
    prompt = song[:P].copy()
    want = _particles(w, ess=1.0, prompts=prompt, prefill="gemm", **w["all on"])
    got = _particles(w, ess=1.0, prompts=prompt, slots=3, **w["all on"])
    assert _differ(got, want) == []
    assert all((s[:P] == prompt).all() for ps in got for s in ps.songs)
    assert any(ps.resampled.any() for ps in got)


def test_ess_zero_is_generate_stream(world):
    """(iii) ess = 0: no row ever moves, and the songs and pairs are generate_stream's on S K slots."""
    w = world
    cons = [w["range"], None, w["tight"], w["range"], None, w["tight"], w["range"]]
    sets = _particles(w, ess=0, slots=3, constraints=cons)
    torch.manual_seed(SEED)
    songs, lps = generation.generate_stream(w["net"], w["w2e"], N * K4, slots=3 * K4, bar_cond=BAR_COND, max_tokens=CAP,
                                            chunk=CHUNK, return_logprobs=True,
                                            constraints=[c for c in cons for _ in range(K4)])
    assert _same([s for ps in sets for s in ps.songs], songs)
    assert _bits([l for ps in sets for l in ps.logprobs], lps)
    for ps in sets:
        assert not ps.resampled.any() and (ps.ancestors == np.arange(K4)).all()
        for k in range(K4):
            lw = np.zeros(1, dtype=np.float32)
            for row in ps.logprobs[k]:
                lw = sampling.particle_weigh_f32(lw, row[None])
            assert lw.view(np.int32)[0] == ps.log_weights[k:k + 1].view(np.int32)[0]
        assert abs(ps.log_evidence - sampling.logmeanexp(ps.log_weights)) < 1e-12


def test_graph_is_eager(world, stream3, monkeypatch):
    """(iv)"""
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    eager = _particles(world, ess=1.0, slots=3, **world["all on"])
    monkeypatch.undo()
    assert _differ(eager, stream3) == []


def _host_ends(song, w2e, cap):
    cnt = 1
    for t in range(1, len(song)):
        cnt += w2e["bar-beat"][int(song[t, 2])] == "Bar"
        if cnt == BAR_COND:
            return t == len(song) - 1
    return len(song) == cap


def test_songs_are_consistent(world, stream3):
    """(v) the constraint, the grammar, the host's bar rule; and score_songs reproduces the pairs within the project's
    1e-4: a state the release or the gather failed to carry breaks exactly this."""
    w, kw = world, world["all on"]
    songs = [s for ps in stream3 for s in ps.songs]
    lps = [l for ps in stream3 for l in ps.logprobs]
    for s in songs:
        assert kw["constraints"].violations(s[1:], 1) == [] and kw["grammar"].violations(s, 1) == []
        assert _host_ends(s, w["w2e"], CAP), len(s)
    scored = generation.score_songs(w["net"], w["w2e"], songs, **kw)
    worst = max(float(np.abs(lp - sc).max()) for lp, sc in zip(lps, scored))
    print("particle stream: generated against scored log-probs, worst |difference| = %.3g" % worst)
    assert all(np.isfinite(lp).all() and lp.shape == (len(s) - 1, 6, 2) for s, lp in zip(songs, lps))
    assert worst <= 1e-4


def test_generate_and_refusals(world, tmp_path):
    """(vi)"""
    w = world
    net, w2e = w["net"], w["w2e"]
    fn = lambda windows, mask: torch.zeros(len(windows), device=windows.device)      # noqa: E731
    free = torch.cuda.memory_allocated()
    for kw, msg in ((dict(reward=fn), "reward= with slots="), (dict(prompts=[np.zeros((1, 6), np.int64)] * N), "shared"),
                    (dict(slots=0), "slots must be"), (dict(slots=1025), "at most 4096"),
                    (dict(n_songs=(1 << 20) // 4 + 1), r"2\*\*20"), (dict(chunk=18), "multiple of resample_every"),
                    (dict(particles=1), "particles must be"), (dict(ess=2), "ess must"),
                    (dict(sampler="greedy"), "sampler must"), (dict(reference=w["ref"]), "needs alpha=")):
        args = dict(n_songs=N, particles=K4, slots=3, resample_every=EVERY, chunk=CHUNK)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            generation.generate_particles(net, w2e, **args)
    assert torch.cuda.memory_allocated() == free                        # nothing was made on the device
    kw = dict(constraints=w["tight"], grammar=w["all on"]["grammar"], ess=1.0, resample_every=EVERY)
    torch.manual_seed(SEED)
    sets = generation.generate_particles(net, w2e, N, K4, bar_cond=BAR_COND, max_tokens=CAP, slots=2, **kw)
    torch.manual_seed(SEED)
    stats = generation.generate(net, w2e, n_songs=N, bar_cond=BAR_COND, max_tokens=CAP, slots=2, particles=K4,
                                path_gendir=str(tmp_path), stats_path=str(tmp_path / "stats.json"), log=lambda s: None,
                                logprobs=True, **kw)
    assert len(stats["words_len_list"]) == N
    for i, ps in enumerate(sets):
        song = np.load(os.path.join(str(tmp_path), "get_%d.npy" % i))
        lp = np.load(os.path.join(str(tmp_path), "get_%d_logp.npy" % i))
        hits = [k for k in range(K4) if song.shape == ps.songs[k].shape and (song == ps.songs[k]).all()]
        assert hits and len(song) == stats["words_len_list"][i]
        assert any(np.array_equal(lp.view(np.int32), ps.logprobs[k].view(np.int32)) for k in hits)

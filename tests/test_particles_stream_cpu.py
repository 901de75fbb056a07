"""CPU: particle generation on the stream -- the numpy restatements, the ParticleSet rebuild on a
hand-written trace, the four C-ABI entries' presence and refusals, and the Python-level refusals.  No GPU.

1. sampling.particle_release on hand-written cases: groups all done, partly done and without a song; songs running out
   in the middle of the ranking; the counters; groups that are no candidates marked -2 (nothing of them is written).
   sampling.particle_event_keys: the song's own event index and the groups the keyed resampling leaves alone.
2. generation.particle_stream_sets on a hand-written trace: two groups, three songs, K = 3, R = 2, eight steps.  Song 0
   has one event with a swap inside its group and a row that dies out; song 2 starts at the second boundary, in the
   group song 0 left, which then idles; song 1 runs through all four events of the run.
3. cwlt_particle_resample_keyed / _advance / _release / _fill are declared, bound and exported at ABI > 33 and refuse
   with 1001, before any launch: null pointers and sizes out of range.
4. generate_particles(slots=) / generate(slots=, particles=) refuse, before the model is looked at: a reward, per-song
   prompt lists, slots < 1, slots x particles > 4096, n_songs x particles > 2**20, a chunk that is no multiple of
   resample_every; then the lock-step refusals, with their messages.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cwlt_particle_resample_keyed", "cwlt_particle_advance", "cwlt_particle_release", "cwlt_particle_fill")


# ---- 1. the restatements -------------------------------------------------------------------------------------------------
def test_release_restatement_hand_cases():
    K = 2
    #          g0 all done   g1 partly    g2 no song   g3 all done   g4 running
    song = [4, 5, -1, 6, 7]
    done = [1, 1, 1, 0, 1, 1, 1, 2, 0, 0]
    take, rel, assigned, finished = sampling.particle_release(song, done, K, 8, 3, 100)
    assert take.tolist() == [8, -2, 9, 10, -2] and rel.tolist() == [True, False, False, True, False]
    assert (assigned, finished) == (11, 5)
    # songs run out in the middle of the ranking: the first candidate takes the last song, the others are parked
    take, rel, assigned, finished = sampling.particle_release(song, done, K, 8, 3, 9)
    assert take.tolist() == [8, -2, -1, -1, -2] and rel.tolist() == [True, False, False, True, False]
    assert (assigned, finished) == (9, 5)
    # none left at all; a parked group stays a candidate and stays parked, and counts as no finished song
    take, rel, assigned, finished = sampling.particle_release([-1, -1, 3], [1, 1, 1, 1, 1, 1], K, 9, 8, 9)
    assert take.tolist() == [-1, -1, -1] and rel.tolist() == [False, False, True] and (assigned, finished) == (9, 9)
    # the start of a run: no group has a song, the first n_songs groups take one
    take, rel, assigned, finished = sampling.particle_release([-1] * 4, [1] * 12, 3, 0, 0, 3)
    assert take.tolist() == [0, 1, 2, -1] and not rel.any() and (assigned, finished) == (3, 0)
    # nothing to do
    take, rel, assigned, finished = sampling.particle_release([0, 1], [0, 1, 1, 0], K, 2, 0, 5)
    assert take.tolist() == [-2, -2] and not rel.any() and (assigned, finished) == (2, 0)
    # a counter that came in above n_songs: every candidate parks and the counter is clamped down to n_songs
    take, rel, assigned, finished = sampling.particle_release(song, done, K, 12, 3, 9)
    assert take.tolist() == [-1, -2, -1, -1, -2] and rel.tolist() == [True, False, False, True, False]
    assert (assigned, finished) == (9, 5)


def test_event_keys_restatement():
    event, skip = sampling.particle_event_keys([3, -1, 0, 7], [8, 8, 4, 3], 4)
    assert event.tolist() == [1, 1, 0, -1] and skip.tolist() == [False, True, False, True]


# ---- 2. the rebuild ------------------------------------------------------------------------------------------------------
K, R, A, T = 3, 2, 2, 8


def _trace():
    rows = np.zeros((T, 2 * K, A + 2), dtype=np.int64)
    lps = np.zeros((T, 2 * K, A, 2), dtype=np.float32)
    for t in range(T):
        for n in range(2 * K):
            rows[t, n, 1:1 + A] = (100 * t + n, 7)
            lps[t, n] = -(10 * t + n) - np.arange(A * 2).reshape(A, 2) / 8.0
    g0 = np.array([0] * 4 + [2] * 2 + [-1] * 2)                          # group 0: song 0, song 2, then idle
    for k in range(K):
        rows[:, k, 0] = np.where(g0 >= 0, g0 * K + k, -1)
        rows[:, K + k, 0] = 1 * K + k                                   # group 1: song 1 throughout
    ident = np.arange(2 * K)
    h_anc = np.tile(ident, (4, 1))
    h_anc[0, :K] = [1, 0, 0]                                            # song 0, event 0: rows 0 / 1 swap, row 2 dies out
    h_anc[1, K:] = K + np.array([0, 1, 1])                              # song 1, its event 1
    h_res = np.array([[1, 0], [0, 1], [0, 0], [0, 0]], dtype=np.int32)
    h_ess = (np.arange(8, dtype=np.float32).reshape(4, 2) + 1) / 4
    h_lw = -np.arange(4 * 2 * K, dtype=np.float32).reshape(4, 2 * K) / 16
    out_len = np.array([4, 3, 4, 7, 8, 5, 2, 1, 2], dtype=np.int64)     # by particle id: songs 0, 1, 2
    out_lw = -np.arange(9, dtype=np.float32) / 4
    out_logz = np.array([-1.5, -2.5, 0.0], dtype=np.float32)
    return rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz


def test_rebuild_hand_trace():
    rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz = _trace()
    head = np.array([[0, 9]], dtype=np.int64)
    stats = {}
    sets = generation.particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz, K, R, 3,
                                           head, stats)
    assert len(sets) == 3 and all(len(ps.songs) == K for ps in sets)
    # (step, pool row) of every drawn row, by hand
    want = {0: [[(0, 1), (1, 1), (2, 0), (3, 0)], [(0, 0), (1, 0), (2, 1)], [(0, 0), (1, 0), (2, 2), (3, 2)]],
            1: [[(t, 3) for t in range(7)], [(t, 4) for t in range(8)],
                [(0, 4), (1, 4), (2, 4), (3, 4), (4, 5)]],
            2: [[(4, 0), (5, 0)], [(4, 1)], [(4, 2), (5, 2)]]}
    for s, ps in enumerate(sets):
        for k in range(K):
            toks = np.array([[100 * t + n, 7] for t, n in want[s][k]], dtype=np.int64)
            assert np.array_equal(ps.songs[k], np.concatenate([head, toks])), (s, k)
            assert np.array_equal(ps.logprobs[k], np.stack([lps[t, n] for t, n in want[s][k]])), (s, k)
            assert ps.logprobs[k].dtype == np.float32 and ps.logprobs[k].shape == (len(toks), A, 2)
        assert np.array_equal(ps.log_weights, out_lw[s * K:(s + 1) * K]) and ps.log_weights.dtype == np.float32
        assert ps.log_evidence == float(out_logz[s]) + sampling.logmeanexp(out_lw[s * K:(s + 1) * K])
    # song 0: the group's events 0 and 1 passed while it held the group; the song was live only up to event 0
    assert np.array_equal(sets[0].ancestors, [[1, 0, 0]]) and sets[0].resampled.tolist() == [True]
    assert np.array_equal(sets[0].ess, h_ess[:1, 0]) and np.array_equal(sets[0].event_log_weights, h_lw[:1, :K])
    # song 1: rows up to 8 -> events after rows 2, 4, 6 (the one after row 8 is not its own)
    assert np.array_equal(sets[1].ancestors, [[0, 1, 2], [0, 1, 1], [0, 1, 2]])
    assert sets[1].resampled.tolist() == [False, True, False]
    assert np.array_equal(sets[1].ess, h_ess[:3, 1]) and np.array_equal(sets[1].event_log_weights, h_lw[:3, K:])
    # song 2 started at the second boundary and ended before its first event
    assert sets[2].ancestors.shape == (0, K) and len(sets[2].ess) == 0 and sets[2].event_log_weights.shape == (0, K)
    assert stats == {"wait_group_steps": 0, "idle_group_steps": 2, "start_steps": [0, 0, 4]}


def test_rebuild_counts_waiting_and_refuses_gaps():
    rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz = _trace()
    out_len[:3] = [2, 1, 2]                                             # song 0 ended at its row 2, released at step 4
    h_res[0, 0] = 0
    h_anc[0, :K] = [0, 1, 2]
    stats = {}
    sets = generation.particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz, K, R, 3,
                                           np.zeros((1, A), np.int64), stats)
    assert stats["wait_group_steps"] == 2 and len(sets[0].ess) == 0
    with pytest.raises(RuntimeError, match="no rows of songs"):
        generation.particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, np.zeros(12, np.float32),
                                        np.ones(12, np.int64), np.zeros(4, np.float32), K, R, 4,
                                        np.zeros((1, A), np.int64))
    rows[3, :K, 0] = 2 * K + np.arange(K)                               # song 2 would start at step 3, off a boundary
    with pytest.raises(RuntimeError, match="inconsistent"):
        generation.particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz, K, R, 3,
                                        np.zeros((1, A), np.int64))


# ---- 3. ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rlmg_amd import _lib
    return _lib


def test_entries_declared_bound_exported(built):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cwlt.h")).read(), flags=re.S)
    lib = built.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in built._SIGNATURES and hasattr(lib, name)
        assert name in built.exported_names()
    assert built.ABI_VERSION > 33 and lib.cwlt_abi_version() == built.ABI_VERSION
    from rlmg_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("particle_resample_keyed", "particle_advance", "particle_release",
                                                    "particle_fill"))


def test_refusals_without_gpu(built):
    lib = built.load()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    keyed = lib.cwlt_particle_resample_keyed
    good = [buf, buf, 3, 4, 0.5, 7, buf, buf, 4, 16, buf, buf, buf, buf, buf]
    for at in (0, 1, 6, 7, 10, 11, 12, 13, 14):
        args = list(good)
        args[at] = null
        assert keyed(*args, null) == 1001, at
    for at, bad in ((2, 0), (3, 1), (3, 1025), (2, (1 << 20) // 4 + 1), (4, 1.5), (4, -0.1), (8, 0), (9, 0), (9, -4)):
        args = list(good)
        args[at] = bad
        assert keyed(*args, null) == 1001, (at, bad)
    advance = lib.cwlt_particle_advance
    good = [buf, 6, 8, buf, buf, buf, buf, buf, buf, 32]
    for at in (0, 3, 4, 5, 6, 7, 8):
        args = list(good)
        args[at] = null
        assert advance(*args, null) == 1001, at
    for at, bad in ((1, 0), (1, 9), (2, 0), (2, (1 << 20) + 1), (9, 0)):
        args = list(good)
        args[at] = bad
        assert advance(*args, null) == 1001, (at, bad)
    release = lib.cwlt_particle_release
    good = [4, 3, 10, 1, 48] + [buf] * 14
    for at in range(5, 19):
        args = list(good)
        args[at] = null
        assert release(*args, null) == 1001, at
    for at, bad in ((0, 0), (0, 4097), (1, 1), (1, 1025), (2, -1), (2, (1 << 20) // 3 + 1), (4, 0)):
        args = list(good)
        args[at] = bad
        assert release(*args, null) == 1001, (at, bad)
    fill = lib.cwlt_particle_fill
    good = [buf, ctypes.c_void_p(8192), buf, buf, 8, 20, 16, 16, 16]
    for at in (0, 1, 2, 3):
        args = list(good)
        args[at] = null
        assert fill(*args, null) == 1001, at
    assert fill(buf, buf, buf, buf, 8, 20, 16, 16, 16, null) == 1001    # in place
    assert fill(ctypes.c_void_p(4098), ctypes.c_void_p(8192), buf, buf, 8, 20, 16, 16, 16, null) == 1001
    for at, bad in ((4, 0), (5, 0), (6, 0), (6, 6), (7, 12), (8, 8), (7, 18)):
        args = list(good)
        args[at] = bad
        assert fill(*args, null) == 1001, (at, bad)


# ---- 4. Python-level refusals ------------------------------------------------------------------------------------------
def test_stream_refusals_come_first(tmp_path):
    """Made before the model is looked at (no GPU, no model needed)."""
    w2e = {"bar-beat": {0: 0, 1: "Bar"}}
    fn = lambda windows, mask: None                                     # noqa: E731
    gp = generation.generate_particles
    with pytest.raises(ValueError, match="reward= with slots="):
        gp(None, w2e, 8, 4, slots=2, reward=fn)
    with pytest.raises(ValueError, match="one shared"):
        gp(None, w2e, 2, 4, slots=2, prompts=[np.zeros((1, 6), np.int64)] * 2)
    for slots in (0, -3):
        with pytest.raises(ValueError, match="slots must be >= 1"):
            gp(None, w2e, 8, 4, slots=slots)
    with pytest.raises(ValueError, match="at most 4096"):
        gp(None, w2e, 5000, 4, slots=1025)
    with pytest.raises(ValueError, match=r"2\*\*20"):
        gp(None, w2e, (1 << 20) // 4 + 1, 4, slots=8)
    with pytest.raises(ValueError, match="multiple of resample_every"):
        gp(None, w2e, 8, 4, slots=2, chunk=16, resample_every=5)
    # then the lock-step refusals, with their messages
    for kw, msg in ((dict(particles=1), "particles must be"), (dict(resample_every=0), "resample_every must be"),
                    (dict(ess=1.5), "ess must lie")):
        args = dict(n_songs=8, particles=4, slots=2)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            gp(None, w2e, **args)
    with pytest.raises(TypeError, match="reward must be a callable"):   # the reward's own refusals stay first
        gp(None, w2e, 8, 4, slots=2, reward=1.5)
    gen = generation.generate
    with pytest.raises(ValueError, match="pass batch_size"):
        gen(None, w2e, n_songs=2, particles=4, path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="not both"):
        gen(None, w2e, n_songs=2, particles=4, batch_size=2, slots=2, path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="reward= with slots="):
        gen(None, w2e, n_songs=2, particles=4, slots=2, reward=fn, path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="one shared prompt"):
        gen(None, w2e, n_songs=2, particles=4, slots=2, prompts=[np.zeros((1, 6), np.int64)] * 2,
            path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="slots must be >= 1"):
        gen(None, w2e, n_songs=2, particles=4, slots=0, path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="multiple of resample_every"):
        gen(None, w2e, n_songs=2, particles=4, slots=2, resample_every=5, path_gendir=str(tmp_path))
    import inspect
    assert inspect.signature(gp).parameters["slots"].default is None

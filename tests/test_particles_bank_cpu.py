"""CPU: per-song prompts on the particle stream and the shared prefill of the lock-step pool -- the numpy
restatement of the gated release, the two C-ABI entries' presence and refusals, the ParticleSet rebuild with a head per
song, and the Python-level refusals.  No GPU.

1. sampling.particle_release_bank on hand-written cases: ready 0 (everything parks, the assigned counter does not move),
   ready inside the candidates, ready >= n_songs equal to sampling.particle_release; the counter never decreases.
2. cwlt_particle_refill_bank / cwlt_particle_release_bank are declared, bound and exported at ABI >= 36 and refuse with
   1001, before any launch: every null pointer and every size out of range.
3. generation.particle_stream_sets with per-song heads on a hand-written trace: two groups, three songs with heads of
   1, 2 and 3 rows, K = 3, R = 2, eight steps; group 0 is parked by the gate for one boundary between songs 0 and 2 and
   idles at the tail -- the two are counted apart.
4. generate_particles / generate refuse with model=None: the old "one shared" refusals still fire without bank=, bank= or
   prefill_rows= without a prompt list or without slots=, what stream_bank_plan and the prompts' checks refuse, and
   share_prefill=True with the blas prefill.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, sampling

from test_particles_stream_cpu import A, K, R, T, _trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cwlt_particle_refill_bank", "cwlt_particle_release_bank")


# ---- 1. the restatement --------------------------------------------------------------------------------------------------
def test_release_bank_restatement_hand_cases():
    #          g0 all done   g1 partly    g2 no song   g3 all done   g4 running
    song = [4, 5, -1, 6, 7]
    done = [1, 1, 1, 0, 1, 1, 1, 2, 0, 0]
    # ready 0, and ready at the assigned counter: every candidate parks, finished songs are still released
    for ready in (0, 8):
        take, rel, assigned, finished = sampling.particle_release_bank(song, done, 2, 8, 3, ready, 100)
        assert take.tolist() == [-1, -2, -1, -1, -2] and rel.tolist() == [True, False, False, True, False]
        assert (assigned, finished) == (8, 5)                           # the counter is not pulled down to `ready`
    # ready inside the candidates: the first two take songs 8 and 9, the third parks
    take, rel, assigned, finished = sampling.particle_release_bank(song, done, 2, 8, 3, 10, 100)
    assert take.tolist() == [8, -2, 9, -1, -2] and (assigned, finished) == (10, 5)
    # the parked group is a candidate again at the next boundary, without a second release of its old song
    take, rel, assigned, finished = sampling.particle_release_bank([8, 5, 9, -1, 7], [0, 0, 1, 0, 0, 0, 1, 1, 0, 0], 2, 10,
                                                                   5, 12, 100)
    assert take.tolist() == [-2, -2, -2, 10, -2] and not rel.any() and (assigned, finished) == (11, 5)
    # ready >= n_songs: particle_release, on its own hand-written cases
    for args in ((song, done, 2, 8, 3, 100), (song, done, 2, 8, 3, 9), ([-1, -1, 3], [1] * 6, 2, 9, 8, 9),
                 ([-1] * 4, [1] * 12, 3, 0, 0, 3), ([0, 1], [0, 1, 1, 0], 2, 2, 0, 5)):
        want = sampling.particle_release(*args)
        for ready in (args[-1], args[-1] + 7):
            got = sampling.particle_release_bank(*args[:5], ready, args[5])
            assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2:] == want[2:]
    # the gate below n_songs, the songs running out above it
    take, _, assigned, _ = sampling.particle_release_bank([-1] * 4, [1] * 8, 2, 0, 0, 5, 3)
    assert take.tolist() == [0, 1, 2, -1] and assigned == 3
    # a counter that came in above n_songs: every candidate parks, as in particle_release, but the counter stays
    for ready in (5, 9, 100):
        take, rel, assigned, finished = sampling.particle_release_bank(song, done, 2, 12, 3, ready, 9)
        assert take.tolist() == [-1, -2, -1, -1, -2] and rel.tolist() == [True, False, False, True, False]
        assert (assigned, finished) == (12, 5)


# ---- 2. ABI ----------------------------------------------------------------------------------------------------------------
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
    assert built.ABI_VERSION >= 36 and lib.cwlt_abi_version() == built.ABI_VERSION
    from rlmg_amd import ops
    assert callable(ops.particle_refill_bank) and callable(ops.particle_release_bank)


def test_refusals_without_gpu(built):
    lib = built.load()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    refill = lib.cwlt_particle_refill_bank
    #       state bank_state bank layers s  z  logits bank_logits n  ld  ld_bank fresh id  rows K
    good = [buf, buf, 3, 2, 16, 8, buf, buf, 10, 12, 12, buf, buf, 8, 4]
    for at in (0, 1, 6, 7, 11, 12):
        args = list(good)
        args[at] = null
        assert refill(*args, null) == 1001, at
    for at in (0, 1):                                                   # 16-byte alignment of the two states
        args = list(good)
        args[at] = ctypes.c_void_p(4104)
        assert refill(*args, null) == 1001, at
    for at, bad in ((2, 0), (3, 0), (4, 0), (4, 6), (5, 0), (5, 6), (8, 0), (9, 8), (10, 8), (13, 0),
                    (13, (1 << 20) + 4), (13, 10), (14, 1), (14, 1025)):
        args = list(good)
        args[at] = bad
        assert refill(*args, null) == 1001, (at, bad)
    release = lib.cwlt_particle_release_bank
    good = [4, 3, 10] + [buf] * 16
    for at in range(3, 19):
        args = list(good)
        args[at] = null
        assert release(*args, null) == 1001, at
    for at, bad in ((0, 0), (0, 4097), (1, 1), (1, 1025), (2, -1), (2, (1 << 20) // 3 + 1)):
        args = list(good)
        args[at] = bad
        assert release(*args, null) == 1001, (at, bad)
    good = [4096, 1024, 10] + [buf] * 16                                # groups x particles past 2**20
    assert release(*good, null) == 1001


# ---- 3. the rebuild with a head per song ---------------------------------------------------------------------------------
def _gated_trace():
    """tests/test_particles_stream_cpu.py's trace with group 0: song 0 for steps 0 - 1, parked by the gate for steps
    2 - 3 (song 2's entry was not written at the boundary after step 2), song 2 for steps 4 - 5, idle for 6 - 7."""
    rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz = _trace()
    g0 = np.array([0] * 2 + [-1] * 2 + [2] * 2 + [-1] * 2)
    for k in range(K):
        rows[:, k, 0] = np.where(g0 >= 0, g0 * K + k, -1)
    out_len[:3] = [2, 1, 2]
    h_res[0, 0] = 0
    h_anc[0, :K] = [0, 1, 2]
    return rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz


def test_rebuild_per_song_heads_and_gate_wait():
    rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz = _gated_trace()
    heads = [np.arange(2 * (s + 1), dtype=np.int64).reshape(s + 1, A) + 1000 * s for s in range(3)]
    stats = {}
    sets = generation.particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz, K, R, 3,
                                           heads, stats)
    # (step, pool row) of every drawn row, by hand
    want = {0: [[(0, 0), (1, 0)], [(0, 1)], [(0, 2), (1, 2)]],
            1: [[(t, 3) for t in range(7)], [(t, 4) for t in range(8)], [(0, 4), (1, 4), (2, 4), (3, 4), (4, 5)]],
            2: [[(4, 0), (5, 0)], [(4, 1)], [(4, 2), (5, 2)]]}
    for s, ps in enumerate(sets):
        for k in range(K):
            toks = np.array([[100 * t + n, 7] for t, n in want[s][k]], dtype=np.int64)
            assert np.array_equal(ps.songs[k], np.concatenate([heads[s], toks])), (s, k)
            assert len(ps.songs[k]) == s + 1 + len(toks)
            assert np.array_equal(ps.logprobs[k], np.stack([lps[t, n] for t, n in want[s][k]])), (s, k)
        assert np.array_equal(ps.log_weights, out_lw[s * K:(s + 1) * K])
    assert len(sets[0].ess) == 0 and len(sets[2].ess) == 0
    assert np.array_equal(sets[1].ancestors, [[0, 1, 2], [0, 1, 1], [0, 1, 2]])
    assert stats == {"gate_wait_group_steps": 2, "wait_group_steps": 0, "idle_group_steps": 2, "start_steps": [0, 0, 4]}
    # one shared head: the same trace reads as four idle group-steps, and no gate is reported
    stats = {}
    generation.particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz, K, R, 3, heads[0],
                                    stats)
    assert stats == {"wait_group_steps": 0, "idle_group_steps": 4, "start_steps": [0, 0, 4]}
    with pytest.raises(ValueError, match="2 arrays for 3 songs"):
        generation.particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz, K, R, 3,
                                        heads[:2])
    assert T == 8


# ---- 4. Python-level refusals ------------------------------------------------------------------------------------------
def test_refusals_come_before_the_model(tmp_path):
    w2e = {k: {0: 0, 1: "Bar"} for k in ("tempo", "chord", "bar-beat", "type", "pitch", "duration")}
    one = np.zeros((1, 6), np.int64)
    gp, gen = generation.generate_particles, generation.generate
    # the old refusals, where and as they were, with the closing clause
    with pytest.raises(ValueError, match=r"one shared \(P, 6\) prompt.*would need a prompt bank.*bank=\"auto\""):
        gp(None, w2e, 2, 4, slots=2, prompts=[one] * 2)
    with pytest.raises(ValueError, match=r"one shared prompt \(prompt=\), not per-song prompts.*bank=\"auto\""):
        gen(None, w2e, n_songs=2, particles=4, slots=2, prompts=[one] * 2, path_gendir=str(tmp_path))
    # bank / prefill_rows without slots= and a prompt list
    for kw in (dict(bank="auto"), dict(bank=2), dict(prefill_rows=64), dict(bank="auto", slots=2),
               dict(bank=4, prompts=[one] * 2), dict(bank="auto", slots=2, prompts=one),
               dict(prefill_rows=64, slots=2)):
        with pytest.raises(ValueError, match="bank and prefill_rows belong to slots="):
            gp(None, w2e, 2, 4, **kw)
    with pytest.raises(ValueError, match="one shared"):                 # prefill_rows alone does not opt in
        gp(None, w2e, 2, 4, slots=2, prompts=[one] * 2, prefill_rows=64)
    for kw in (dict(bank="auto"), dict(bank="auto", slots=2, particles=4), dict(bank="auto", batch_size=2, particles=4,
                                                                               prompts=[one] * 2)):
        with pytest.raises(ValueError, match="bank belongs to slots="):
            gen(None, w2e, n_songs=2, path_gendir=str(tmp_path), **kw)
    # what stream_bank_plan and the prompts' checks refuse
    args = dict(slots=2, prompts=[one] * 2)
    with pytest.raises(ValueError, match="bank must be >= 1"):
        gp(None, w2e, 2, 4, bank=0, **args)
    with pytest.raises(ValueError, match="bank must be \"auto\""):
        gp(None, w2e, 2, 4, bank="big", **args)
    with pytest.raises(ValueError, match="prefill_rows must be >= 1"):
        gp(None, w2e, 2, 4, bank="auto", prefill_rows=0, **args)
    with pytest.raises(ValueError, match="must be a multiple of the prefill block"):
        gp(None, w2e, 5, 4, bank=3, prefill_rows=2, slots=2, prompts=[one] * 5)
    with pytest.raises(ValueError, match="3 arrays for 2 songs"):
        gp(None, w2e, 2, 4, bank="auto", slots=2, prompts=[one] * 3)
    with pytest.raises(ValueError, match="empty prompt"):
        gp(None, w2e, 2, 4, bank="auto", slots=2, prompts=[one, one[:0]])
    with pytest.raises(ValueError, match="already reaches bar"):
        gp(None, w2e, 2, 4, bank="auto", slots=2, bar_cond=2, prompts=[one, np.array([[0, 0, 1, 0, 0, 0]] * 2)])
    with pytest.raises(ValueError, match="leaves no room"):
        gp(None, w2e, 2, 4, bank="auto", slots=2, max_tokens=1, prompts=[one] * 2)
    with pytest.raises(ValueError, match="3 arrays for 2 songs"):
        gen(None, w2e, n_songs=2, particles=4, slots=2, bank="auto", prompts=[one] * 3, path_gendir=str(tmp_path))
    # the stream's own refusals still come first
    with pytest.raises(ValueError, match="slots must be >= 1"):
        gp(None, w2e, 2, 4, bank="auto", slots=0, prompts=[one] * 2)
    with pytest.raises(ValueError, match="multiple of resample_every"):
        gp(None, w2e, 2, 4, bank="auto", slots=2, prompts=[one] * 2, chunk=16, resample_every=5)
    # then the lock-step refusals (the model is looked at only after all of the above)
    with pytest.raises(ValueError, match="particles must be"):
        gp(None, w2e, 2, 1, bank="auto", slots=2, prompts=[one] * 2)
    # the shared prefill needs the batch-invariant prefill
    for kw in (dict(), dict(prefill="blas"), dict(prompts=[one] * 2, prefill="blas")):
        with pytest.raises(ValueError, match="share_prefill=True needs prefill=\"gemm\""):
            gp(None, w2e, 2, 4, share_prefill=True, **kw)
    import inspect
    sig = inspect.signature(gp).parameters
    assert sig["bank"].default is None and sig["prefill_rows"].default is None and sig["share_prefill"].default is None
    assert list(sig)[:4] == ["model", "word2event", "n_songs", "particles"]
    assert inspect.signature(gen).parameters["bank"].default is None
    names = list(inspect.signature(generation.particle_stream_sets).parameters)
    assert names == ["rows", "logps", "h_anc", "h_lw", "h_ess", "h_res", "out_lw", "out_len", "out_logz", "particles",
                     "every", "n_songs", "head", "stats", "h_r", "window"]

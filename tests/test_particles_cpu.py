"""CPU: particle generation -- the float64 restatement of the resampling event, the lineage of the final
rows, and the three C-ABI entries' presence and refusals.  No GPU.

1. sampling.systematic_resample for K in {2, 7, 64}: ancestors never decrease; row i is copied floor(K w_i) or
   ceil(K w_i) times; equal weights are kept (the identity, resampled 0) even at ess_frac 1; one dominant weight takes
   every copy; a group whose rows are all done is kept; the evidence estimate log_z + logmeanexp(lw) is the same before
   and after an event.
2. The cases the GPU test feeds cwlt_particle_resample (resample_case, shared with tests/test_particles_gpu.py): a numpy
   float32 emulation of the kernel's arithmetic (f32 exp, sequential f32 prefix sums, f32 thresholds), u on a grid,
   disagrees with the float64 restatement only where a threshold lies within (K + 2) 2^-23 s of a prefix-sum boundary,
   and on fewer than 1 % of the entries of each K: the seeds leave the GPU comparison that room.
3. generation.particle_lineage on a hand-written three-event ancestry with a swap and a row that dies out.
3b. generation.particle_pool_sets on a hand-written lock-step trace: two songs, K = 3, R = 2, seven steps; two final
   particles that share a prefix, a song whose events are cut by its last resampling, a pool without an event; the same
   trace, one step longer, through generation.particle_stream_sets gives the same sets bit for bit.
4. cwlt_particle_weigh / _resample / _gather are declared, bound and exported, and refuse bad arguments with 1001.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 7, 64)
NAMES = ("cwlt_particle_weigh", "cwlt_particle_resample", "cwlt_particle_gather")
CASES = ("equal", "dominant", "normal3", "shifted", "done")
GPU_KS = (2, 7, 64, 65, 256, 1024)
GPU_GROUPS = (1, 3, 130)


def resample_case(case, groups, K, seed):
    """The log-weights (groups, K) f32 and done flags (groups, K) int64 of one resampling case, from `seed`."""
    rng = np.random.default_rng([seed, groups, K, CASES.index(case)])
    done = np.zeros((groups, K), dtype=np.int64)
    if case == "equal":
        lw = np.repeat(rng.normal(0, 3, (groups, 1)), K, axis=1)
    elif case == "dominant":
        lw = rng.normal(-1000, 1, (groups, K))
        lw[np.arange(groups), rng.integers(0, K, groups)] = rng.normal(0, 1, groups)
    elif case == "normal3":
        lw = 3 * rng.normal(0, 1, (groups, K))
    elif case == "shifted":
        lw = rng.normal(0, 1, (groups, K)) - 5000
    else:                                                               # every other group is all done
        lw = 3 * rng.normal(0, 1, (groups, K))
        done[::2] = 1
        done[1::2, 0] = 1                                               # one done row does not stop a group
    return lw.astype(np.float32), done


def near_boundary(res, K):
    """Per entry j: a prefix-sum boundary lies within (K + 2) 2^-23 s of threshold j (float64 restatement `res`)."""
    delta = (K + 2) * 2.0 ** -23 * res.s
    return np.abs(res.prefix[None, :] - res.thresholds[:, None]).min(1) <= delta


def _resample_f32(lw, u, ess_frac, done):
    """The kernel's arithmetic in numpy float32 -> (anc, resampled)."""
    f = np.float32
    x = lw.astype(f)
    K = len(x)
    e = np.exp(x - x.max()).astype(f)
    c = np.cumsum(e, dtype=f)
    s = c[-1]
    ess = f(s * s) / f((e * e).sum(dtype=f))
    if (done != 0).all() or ess >= f(ess_frac) * f(K):
        return np.arange(K), 0
    t = ((np.arange(K).astype(f) + f(u)) / f(K)).astype(f) * s
    return np.minimum(np.searchsorted(c, t.astype(f), side="right"), K - 1), 1


# ---- 1. restatement invariants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_ancestors_and_copy_counts(K):
    rng = np.random.default_rng(K)
    hit = 0
    for trial in range(200):
        lw = rng.normal(0, rng.choice([0.3, 1.0, 3.0]), K)
        u = rng.random()
        r = sampling.systematic_resample(lw, u, 1.0)
        w = np.exp(lw - lw.max())
        w /= w.sum()
        assert r.resampled == 1 and (np.diff(r.anc) >= 0).all()
        counts = np.bincount(r.anc, minlength=K)
        assert counts.sum() == K
        lo, hi = np.floor(K * w - 1e-9), np.ceil(K * w + 1e-9)
        assert ((counts >= lo) & (counts <= hi)).all(), (trial, counts, K * w)
        assert (r.lw == 0).all() and abs(r.ess - 1.0 / (w * w).sum()) <= 1e-9 * K
        # the decision is the threshold's: just above ess / K nothing moves, at or below it the group is resampled
        frac = r.ess / K
        kept = sampling.systematic_resample(lw, u, frac * (1 - 1e-9))
        assert kept.resampled == 0 and (kept.anc == np.arange(K)).all() and (kept.lw == lw).all() and kept.log_z == 0
        hit += sampling.systematic_resample(lw, u, min(1.0, frac * (1 + 1e-9))).resampled
    assert hit >= 190                                                   # (frac (1 + 1e-9) > 1 is clipped for a few)


@pytest.mark.parametrize("K", KS)
def test_equal_dominant_done_and_evidence(K):
    rng = np.random.default_rng(100 + K)
    for u in (0.0, 0.25, 0.999999):
        eq = sampling.systematic_resample(np.full(K, -3.25), u, 1.0)
        assert eq.resampled == 0 and (eq.anc == np.arange(K)).all() and eq.ess == K and eq.log_z == 0.0
        assert sampling.logmeanexp(eq.lw) + eq.log_z == -3.25           # unchanged by the (kept) event
        for at in (0, K // 2, K - 1):
            lw = np.full(K, -1000.0)
            lw[at] = 2.5
            dom = sampling.systematic_resample(lw, u, 1.0)
            assert dom.resampled == 1 and (dom.anc == at).all() and abs(dom.ess - 1.0) < 1e-12
            assert abs(dom.log_z - (2.5 - np.log(K))) < 1e-12
        lw = rng.normal(0, 3, K)
        done = np.ones(K, dtype=np.int64)
        skipped = sampling.systematic_resample(lw, u, 1.0, done=done)
        assert skipped.resampled == 0 and (skipped.anc == np.arange(K)).all() and (skipped.lw == lw).all()
        done[K // 2] = 0                                                # one live particle: the group takes part
        r = sampling.systematic_resample(lw, u, 1.0, done=done)
        assert r.resampled == 1
        assert abs((r.log_z + sampling.logmeanexp(r.lw)) - sampling.logmeanexp(lw)) < 1e-12
    with pytest.raises(ValueError):
        sampling.systematic_resample(np.zeros(K), 1.0, 0.5)
    with pytest.raises(ValueError):
        sampling.systematic_resample(np.zeros(1), 0.5, 0.5)


def test_weigh_restatement_is_sequential_f32():
    rng = np.random.default_rng(5)
    pairs = (rng.normal(-3, 2, (9, 6, 2)) * 10.0 ** rng.integers(-3, 3, (9, 6, 2))).astype(np.float32)
    lw = rng.normal(0, 50, 9).astype(np.float32)
    done = np.array([0, 1, 0, 0, 2, 0, 0, 0, 0])
    got = sampling.particle_weigh_f32(lw, pairs, done)
    assert got.dtype == np.float32
    for n in range(9):
        s = np.float32(0)
        for a in range(6):
            s = np.float32(s + np.float32(pairs[n, a, 0] - pairs[n, a, 1]))
        want = lw[n] if done[n] else np.float32(lw[n] + s)
        assert got[n].view(np.int32) == np.float32(want).view(np.int32)
    assert sampling.logmeanexp([-np.inf, -np.inf]) == -np.inf
    assert abs(sampling.logmeanexp([0.0, np.log(3.0)]) - np.log(2.0)) < 1e-15


# ---- 2. the GPU test's cases leave it room -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", GPU_KS)
def test_f32_arithmetic_stays_within_the_excuse(K):
    entries = excused = 0
    for groups in GPU_GROUPS:
        for case in CASES:
            lw, done = resample_case(case, groups, K, seed=groups)
            for g in range(0, groups, max(1, groups // 8)):
                for u in (np.arange(4) + 0.37) / 4:
                    want = sampling.systematic_resample(lw[g], np.float32(u), 1.0, done=done[g])
                    anc, res = _resample_f32(lw[g], u, 1.0, done[g])
                    assert res == want.resampled, (case, groups, g, u)
                    bad = anc != want.anc
                    assert not (bad & ~near_boundary(want, K)).any(), (case, groups, g, u)
                    entries += K
                    excused += int(bad.sum())
    print("K = %d: %d of %d entries differ between f32 and f64 arithmetic" % (K, excused, entries))
    assert excused <= 0.01 * entries


# ---- 3. lineage ------------------------------------------------------------------------------------------------------------
def test_particle_lineage_by_hand():
    """Four rows, three events.  Event 0 swaps rows 0 and 1; event 1 copies row 0 over row 1 (old row 1's song -- row
    0's before the swap -- dies out) and row 3 over row 2; event 2 copies row 2 over row 3."""
    anc = np.array([[1, 0, 2, 3],
                    [0, 0, 3, 3],
                    [0, 1, 2, 2]])
    line = generation.particle_lineage(anc)
    assert line.dtype == np.int64 and line.shape == (4, 4)
    assert line[3].tolist() == [0, 1, 2, 3]                             # after the last event: the rows themselves
    assert line[2].tolist() == [0, 1, 2, 2]                             # between events 1 and 2
    assert line[1].tolist() == [0, 0, 3, 3]                             # between events 0 and 1
    assert line[0].tolist() == [1, 1, 3, 3]                             # before event 0: through the swap
    assert 0 not in line[0] and 2 not in line[0]                        # rows 0 and 2 of segment 0 have no descendant
    assert 1 not in line[1] and 2 not in line[1]                        # the swapped-in row 1 died at event 1
    assert generation.particle_lineage(np.zeros((0, 5), dtype=np.int64)).tolist() == [[0, 1, 2, 3, 4]]
    assert generation.particle_lineage([], rows=3).tolist() == [[0, 1, 2]]
    with pytest.raises(ValueError):
        generation.particle_lineage([[0, 4, 1, 2]])


def test_particle_set_weights_and_draw():
    songs = [np.full((2, 6), k) for k in range(3)]
    lw = np.array([0.0, np.log(3.0), -np.inf], dtype=np.float32)
    ps = generation.ParticleSet(songs, [None] * 3, lw, 1.5, np.zeros(0, np.float32), np.zeros(0, bool),
                                np.zeros((0, 3), np.int64))
    w = ps.weights()
    assert w.dtype == np.float64 and np.allclose(w, [0.25, 0.75, 0.0]) and ps.log_evidence == 1.5
    rng = np.random.default_rng(0)
    picks = [ps.draw(rng, return_index=True)[1] for _ in range(400)]
    assert 2 not in picks and 250 < picks.count(1) < 350
    assert ps.draw(np.random.default_rng(1)) is songs[ps.draw(np.random.default_rng(1), return_index=True)[1]]


# ---- 3b. the lock-step rebuild -------------------------------------------------------------------------------------------
POOL_K, POOL_R, POOL_W, POOL_A = 3, 2, 4, 2


def pool_trace(T=7):
    """A lock-step pool of two songs x 3 particles as the device leaves it after T steps, R = 2, W = 4: T // 2 events and
    ceil(T / 4) reward events (at T = 7 the last one closes a window of 3 rows).  Song 0 (pool rows 0, 1, 2) drew 7, 5
    and 3 rows and was resampled at event 1, ancestors [0, 0, 2]; song 1 (rows 3, 4, 5) drew 2, 2 and 1 rows and its
    only resampling, event 0, copied row 4 over row 3.  Shared with tests/test_reward_cpu.py."""
    K, R, W, A, N = POOL_K, POOL_R, POOL_W, POOL_A, 2 * POOL_K
    rows = np.zeros((T, N, A), dtype=np.int64)
    lps = np.zeros((T, N, A, 2), dtype=np.float32)
    for t in range(T):
        for n in range(N):
            rows[t, n] = (100 * t + n, 7)
            lps[t, n] = -(10 * t + n) - np.arange(A * 2).reshape(A, 2) / 8.0
    E = T // R
    h_anc = np.tile(np.arange(N), (E, 1))
    h_res = np.zeros((E, 2), dtype=np.int32)
    h_anc[1, :K], h_res[1, 0] = [0, 0, 2], 1
    h_anc[0, K:], h_res[0, 1] = K + np.array([1, 1, 2]), 1
    song_heads = [np.array([[0, 9]], dtype=np.int64), np.array([[1, 9], [2, 9]], dtype=np.int64)]
    return {"heads": [h for h in song_heads for _ in range(K)], "song_heads": song_heads, "rows": rows, "logps": lps,
            "lens": np.array([7, 5, 3, 2, 2, 1], dtype=np.int64), "lw": -np.arange(N, dtype=np.float32) / 4,
            "log_z": np.array([-1.5, -2.5], dtype=np.float32), "h_anc": h_anc,
            "h_lw": -np.arange(E * N, dtype=np.float32).reshape(E, N) / 16,
            "h_ess": (np.arange(2 * E, dtype=np.float32).reshape(E, 2) + 1) / 4, "h_res": h_res,
            "h_r": (10 * np.arange(-(-T // W))[:, None] + np.arange(N)[None, :] + 0.5).astype(np.float32)}


def pool_sets(tr, reward):
    return generation.particle_pool_sets(tr["heads"], tr["rows"], tr["logps"], tr["lens"], tr["lw"], tr["log_z"],
                                         tr["h_anc"], tr["h_lw"], tr["h_ess"], tr["h_res"], POOL_K, POOL_R,
                                         h_r=tr["h_r"] if reward else None, window=POOL_W if reward else None)


def check_pool_sets(sets, tr):
    """Every field of the two sets but the rewards against the values written out by hand."""
    K = POOL_K
    assert len(sets) == 2 and all(len(ps.songs) == K and ps.beta is None for ps in sets)
    # (step, pool row) of every drawn row: song 0's particle 1 shares particle 0's first four rows, drawn in row 0
    # before event 1; song 1's particles 0 and 1 are both row 4's two rows
    want = [[[(t, 0) for t in range(7)], [(0, 0), (1, 0), (2, 0), (3, 0), (4, 1)], [(0, 2), (1, 2), (2, 2)]],
            [[(0, 4), (1, 4)], [(0, 4), (1, 4)], [(0, 5)]]]
    for s, ps in enumerate(sets):
        for k in range(K):
            toks = np.array([[100 * t + n, 7] for t, n in want[s][k]], dtype=np.int64)
            assert np.array_equal(ps.songs[k], np.concatenate([tr["song_heads"][s], toks])), (s, k)
            assert np.array_equal(ps.logprobs[k], np.stack([tr["logps"][t, n] for t, n in want[s][k]])), (s, k)
            assert ps.logprobs[k].dtype == np.float32 and ps.logprobs[k].shape == (len(toks), POOL_A, 2)
        w = tr["lw"][s * K:(s + 1) * K]
        assert np.array_equal(ps.log_weights, w) and ps.log_weights.dtype == np.float32
        assert ps.log_evidence == float(tr["log_z"][s]) + sampling.logmeanexp(w)
    # song 0: its longest particle drew 7 rows: the events after rows 2, 4 and 6 are its own
    assert sets[0].ancestors.tolist() == [[0, 1, 2], [0, 0, 2], [0, 1, 2]] and sets[0].ancestors.dtype == np.int64
    assert sets[0].resampled.tolist() == [False, True, False] and sets[0].resampled.dtype == bool
    assert np.array_equal(sets[0].ess, tr["h_ess"][:3, 0]) and np.array_equal(sets[0].event_log_weights,
                                                                             tr["h_lw"][:3, :K])
    # song 1: no event e has (e + 1) R < 2, its longest particle; event 0 is its own because it resampled the song
    assert sets[1].ancestors.tolist() == [[1, 1, 2]] and sets[1].resampled.tolist() == [True]
    assert np.array_equal(sets[1].ess, tr["h_ess"][:1, 1]) and np.array_equal(sets[1].event_log_weights,
                                                                             tr["h_lw"][:1, K:])
    assert all(ps.ess.dtype == np.float32 and ps.event_log_weights.dtype == np.float32 for ps in sets)


def test_pool_sets_hand_trace():
    """generation.particle_pool_sets without a reward: two songs, K = 3, R = 2, seven steps, three events."""
    tr = pool_trace()
    sets = pool_sets(tr, reward=False)
    check_pool_sets(sets, tr)
    assert all(ps.rewards is None and ps.event_rewards is None for ps in sets)
    # h_r without a window, or a window without h_r, is the run without a reward
    args = [tr[k] for k in ("heads", "rows", "logps", "lens", "lw", "log_z", "h_anc", "h_lw", "h_ess", "h_res")]
    assert generation.particle_pool_sets(*args, POOL_K, POOL_R, window=POOL_W)[0].rewards is None
    assert generation.particle_pool_sets(*args, POOL_K, POOL_R, h_r=tr["h_r"])[0].rewards is None
    # a pool with no event at all: one step
    tr.update(rows=tr["rows"][:1], logps=tr["logps"][:1], lens=np.ones(6, dtype=np.int64),
              **{k: tr[k][:0] for k in ("h_anc", "h_lw", "h_ess", "h_res")})
    sets = pool_sets(tr, reward=False)
    assert all(ps.ancestors.shape == (0, POOL_K) and len(ps.ess) == 0 and [len(s) for s in ps.songs] == [p] * 3
               for ps, p in zip(sets, (2, 3)))


def stream_sets(tr, reward):
    """The trace as a particle stream's: ring ids = the row index (group g holds song g from step 0 on), the release's
    outputs = the pool's finals, a head per song."""
    T, N = tr["rows"].shape[:2]
    ring = np.concatenate([np.tile(np.arange(N)[None, :, None], (T, 1, 1)), tr["rows"],
                           np.zeros((T, N, 1), dtype=np.int64)], axis=2)
    return generation.particle_stream_sets(ring, tr["logps"], tr["h_anc"], tr["h_lw"], tr["h_ess"], tr["h_res"], tr["lw"],
                                           tr["lens"], tr["log_z"], POOL_K, POOL_R, 2, tr["song_heads"],
                                           h_r=tr["h_r"] if reward else None, window=POOL_W if reward else None)


def same_sets(a, b):
    """Field by field and bit for bit, dtypes and shapes included."""
    def same(x, y):
        if isinstance(x, list):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if x is None or y is None:
            return x is None and y is None
        return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    fields = ("songs", "logprobs", "log_weights", "ess", "resampled", "ancestors", "event_log_weights", "rewards",
              "event_rewards")
    return a.log_evidence == b.log_evidence and a.beta == b.beta and all(same(getattr(a, f), getattr(b, f))
                                                                         for f in fields)


def test_pool_trace_as_a_stream_trace():
    """Eight steps, so that every window closes: the stream's rebuild gives the pool's sets."""
    tr = pool_trace(T=8)
    pool = pool_sets(tr, reward=False)
    check_pool_sets(pool, tr)                                           # the eighth step and fourth event change nothing
    stream = stream_sets(tr, reward=False)
    assert len(stream) == 2 and all(same_sets(a, b) for a, b in zip(stream, pool))


# ---- 4. ABI ----------------------------------------------------------------------------------------------------------------
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
    assert built.ABI_VERSION > 31 and lib.cwlt_abi_version() == built.ABI_VERSION
    from rlmg_amd import ops
    assert all(hasattr(ops, n) for n in ("particle_weigh", "particle_resample", "particle_gather"))
    assert callable(generation.generate_particles)


def test_refusals_without_gpu(built):
    lib = built.load()
    null, buf, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    assert lib.cwlt_particle_weigh(null, null, 1, 1, 6, null, 4, null, null, null, null, null) == 1001
    assert lib.cwlt_particle_weigh(buf, buf, 4, 0, 6, buf, 4, buf, buf, buf, buf, null) == 1001          # no rows
    assert lib.cwlt_particle_weigh(buf, buf, 4, (1 << 20) + 1, 6, buf, 4, buf, buf, buf, buf, null) == 1001
    assert lib.cwlt_particle_weigh(buf, buf, 4, 8, 9, buf, 4, buf, buf, buf, buf, null) == 1001          # n_attr
    assert lib.cwlt_particle_weigh(buf, null, 4, 8, 6, buf, 4, buf, buf, buf, buf, null) == 1001         # ring, no counter
    assert lib.cwlt_particle_resample(null, null, 1, 2, 0.5, 0, 0, null, null, null, null, null, null) == 1001
    args = (buf, buf, buf, buf, buf, buf)
    for K in (1, 1025):
        assert lib.cwlt_particle_resample(buf, buf, 1, K, 0.5, 0, 0, *args[:5], null) == 1001
    assert lib.cwlt_particle_resample(buf, buf, 0, 4, 0.5, 0, 0, *args[:5], null) == 1001
    assert lib.cwlt_particle_resample(buf, buf, 1, 4, 1.5, 0, 0, *args[:5], null) == 1001
    assert lib.cwlt_particle_resample(buf, buf, 1, 4, -0.1, 0, 0, *args[:5], null) == 1001
    assert lib.cwlt_particle_resample(buf, buf, 1, 4, float("nan"), 0, 0, *args[:5], null) == 1001
    assert lib.cwlt_particle_resample(buf, buf, 1, 4, 0.5, 0, -1, *args[:5], null) == 1001
    assert lib.cwlt_particle_resample(buf, buf, 2048, 1024, 0.5, 0, 0, *args[:5], null) == 1001          # > 2^20 rows
    assert lib.cwlt_particle_gather(null, null, null, 1, 8, 1, 0, 0, null) == 1001
    other = ctypes.c_void_p(8192)
    assert lib.cwlt_particle_gather(buf, buf, buf, 4, 8, 1, 0, 0, null) == 1001                         # in place
    assert lib.cwlt_particle_gather(buf, other, buf, 4, 6, 1, 0, 0, null) == 1001                       # row_bytes % 4
    assert lib.cwlt_particle_gather(buf, other, buf, 4, 0, 1, 0, 0, null) == 1001
    assert lib.cwlt_particle_gather(odd, other, buf, 4, 8, 1, 0, 0, null) == 1001                       # alignment
    assert lib.cwlt_particle_gather(buf, other, buf, 4, 8, 3, 16, 0, null) == 1001                      # blocks overlap
    assert lib.cwlt_particle_gather(buf, other, buf, 4, 8, 0, 0, 0, null) == 1001
    assert lib.cwlt_particle_gather(buf, other, buf, 4, 8, 1, 0, 2, null) == 1001                       # copy_back
    assert lib.cwlt_particle_gather(buf, other, buf, 0, 8, 1, 0, 0, null) == 1001


def test_generate_particles_refusals_come_first():
    """The particle refusals are made before the model is looked at (no GPU, no model needed)."""
    w2e = {"bar-beat": {0: 0, 1: "Bar"}}
    for kw, msg in ((dict(particles=1), "particles must be"), (dict(particles=1025), "particles must be"),
                    (dict(particles=8, n_songs=513), "at most 4096"),
                    (dict(particles=4, resample_every=0), "resample_every"),
                    (dict(particles=4, ess=1.5), "ess must"), (dict(particles=4, ess=-0.1), "ess must")):
        args = dict(n_songs=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            generation.generate_particles(None, w2e, **args)
    with pytest.raises(ValueError, match="pass batch_size"):
        generation.generate(None, w2e, n_songs=2, particles=4)

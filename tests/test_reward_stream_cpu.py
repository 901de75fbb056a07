"""CPU: reward-guided particles on the stream and a reward weight per song -- the float32 restatement of
the keyed weight update, the ParticleSet rebuild with rewards on a hand-written trace, the new C-ABI entry's presence and
refusals, and the Python-level refusals.  No GPU.

1. sampling.reward_apply_keyed_f32 against hand-computed float32 values: product then sum (a case where an fma would
   differ), key None against an explicit arange, rows without an id or without a table entry (weight kept bit for bit,
   0 recorded, NaN / +-inf in r), a table of equal entries against reward_apply_f32.
2. generation.particle_stream_sets(h_r=, window=) on a hand-written trace: two groups, three songs, K = 3, R = 2, W = 4
   (B = 4), twelve steps.  Song 0 ends inside its only window and waits for the boundary; song 1 runs through all twelve
   steps, with a swap inside its second window and a partial last window; song 2 starts at the second B boundary (step
   4) with a swap at its own second event.  A song that starts at a multiple of R but not of B, and a group released
   before its song's window closed, raise.
3. cwlt_reward_apply_keyed is declared, bound and exported at ABI >= 35 and refuses with 1001 before any launch.
4. _particle_stream_refusals / generate_particles / generate with model=None: the lcm rule, the beta list.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# ---- 1. the restatement --------------------------------------------------------------------------------------------------
def test_keyed_restatement_hand_values():
    f = np.float32
    # K = 2, three songs' betas; rows 0 .. 5 are songs 0, 0, 1, 1, 2, 2
    beta = [2.0, -0.5, 0.0]
    lw = f([1.0, -3.0, 0.25, 8.0, -7.5, 0.0])
    r = f([0.5, 4.0, 3.0, -2.0, 123.0, -9.0])
    got, rec = sampling.reward_apply_keyed_f32(lw, r, [1, 1, 1, 0, 1, 1], beta, None, 2)
    assert got.dtype == np.float32 and rec.dtype == np.float32
    assert np.array_equal(_bits(got), _bits([2.0, 5.0, -1.25, 8.0, -7.5, 0.0]))
    assert np.array_equal(_bits(rec), _bits([0.5, 4.0, 3.0, 0.0, 123.0, -9.0]))
    # key None is the identity key
    again = sampling.reward_apply_keyed_f32(lw, r, [1, 1, 1, 0, 1, 1], beta, np.arange(6), 2)
    assert np.array_equal(_bits(again[0]), _bits(got)) and np.array_equal(_bits(again[1]), _bits(rec))
    # a permuted key: row n takes the beta of song key[n] // 2
    got, rec = sampling.reward_apply_keyed_f32(lw, r, np.ones(6), beta, [4, 5, 0, 1, 2, 3], 2)
    assert np.array_equal(_bits(got), _bits([1.0, -3.0, 6.25, 4.0, -69.0, 4.5]))
    assert np.array_equal(_bits(rec), _bits(r))
    # where one rounding (an fma) and two differ: beta r = 1 + 2^-22 + 2^-46 exactly; rounded first it loses the 2^-46
    b = f(1 + 2.0 ** -23)
    got, _ = sampling.reward_apply_keyed_f32(f([7.0, -1.0]), [b, b], [1, 1], [0.0, b], [0, 3], 3)
    assert float(got[0]) == 7.0 and float(got[1]) == 2.0 ** -22 and float(b) * float(b) - 1.0 != float(got[1])


def test_keyed_restatement_off_rows_and_equal_table():
    lw = np.float32([1.5, -2.25, 0.0, 7.0, -0.0, 3.0])
    bad = np.float32([np.nan, np.inf, -np.inf, 3.0, np.nan, np.inf])
    # K = 2, two table entries: key -1 (no id), keys 4 and 5 (song 2 >= n_beta), any = 0; only row 3 is on
    got, rec = sampling.reward_apply_keyed_f32(lw, bad, [1, 1, 1, 1, 0, 1], [1.0, -1.0], [-1, 4, 5, 2, 0, -7], 2)
    assert np.array_equal(_bits(got), _bits([1.5, -2.25, 0.0, 4.0, -0.0, 3.0]))
    assert np.array_equal(_bits(rec), _bits([0, 0, 0, 3.0, 0, 0]))
    rng = np.random.default_rng(5)
    lw = rng.normal(0, 30, 96).astype(np.float32)
    r = (rng.normal(0, 1, 96) * 10.0 ** rng.integers(-3, 3, 96)).astype(np.float32)
    on = rng.integers(0, 2, 96)
    for beta in (1.0, 0.3, -2.5, 100.0, 0.0):
        want = sampling.reward_apply_f32(lw, r, on, beta)
        for key in (None, rng.permutation(96)):
            got = sampling.reward_apply_keyed_f32(lw, r, on, [beta] * 24, key, 4)
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))


# ---- 2. the rebuild ------------------------------------------------------------------------------------------------------
K, R, W, A, T = 3, 2, 4, 2, 12


def _trace():
    rows = np.zeros((T, 2 * K, A + 2), dtype=np.int64)
    lps = np.zeros((T, 2 * K, A, 2), dtype=np.float32)
    for t in range(T):
        for n in range(2 * K):
            rows[t, n, 1:1 + A] = (100 * t + n, 7)
            lps[t, n] = -(10 * t + n) - np.arange(A * 2).reshape(A, 2) / 8.0
    g0 = np.array([0] * 4 + [2] * 8)                                    # group 0: song 0, then song 2 from step 4 = B
    for k in range(K):
        rows[:, k, 0] = g0 * K + k
        rows[:, K + k, 0] = 1 * K + k                                   # group 1: song 1 throughout
    E = T // R
    h_anc = np.tile(np.arange(2 * K), (E, 1))
    h_res = np.zeros((E, 2), dtype=np.int32)
    h_anc[0, :K], h_res[0, 0] = [1, 0, 2], 1                            # song 0, its event 0 (after its row 2)
    h_anc[2, K:], h_res[2, 1] = K + np.array([1, 0, 2]), 1              # song 1, event 2: after row 6, inside window 1
    h_anc[3, :K], h_res[3, 0] = [1, 0, 2], 1                            # song 2, its own event 1: after its row 4
    h_ess = (np.arange(2 * E, dtype=np.float32).reshape(E, 2) + 1) / 4
    h_lw = -np.arange(E * 2 * K, dtype=np.float32).reshape(E, 2 * K) / 16
    h_r = (10 * np.arange(T // W)[:, None] + np.arange(2 * K)[None, :] + 0.5).astype(np.float32)
    out_len = np.array([2, 2, 1, 11, 12, 5, 6, 8, 1], dtype=np.int64)   # by particle id: songs 0, 1, 2
    out_lw = -np.arange(9, dtype=np.float32) / 4
    out_logz = np.array([-1.5, -2.5, 0.0], dtype=np.float32)
    return [rows, lps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz], h_r


def test_rebuild_rewards_hand_trace():
    args, h_r = _trace()
    head = np.array([[0, 9]], dtype=np.int64)
    stats = {}
    sets = generation.particle_stream_sets(*args, K, R, 3, head, stats, h_r=h_r, window=W)
    f = lambda *v: np.float32(v)                                        # noqa: E731
    # song 0: one window, closed at step 4 by run event 0, every lineage in its own row by then
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(sets[0].rewards, (f(0.5), f(1.5), f(2.5))))
    assert np.array_equal(_bits(sets[0].event_rewards), _bits([[0.5, 1.5, 2.5]]))
    # song 1 (pool rows 3, 4, 5): final particle 0 lived in row 4 up to the swap after row 6, particle 1 in row 3; window
    # 0 closed before the swap, so particle 0's first reward is row 4's.  11 and 5 rows: a partial last window each
    want = (f(4.5, 13.5, 23.5), f(3.5, 14.5, 24.5), f(5.5, 15.5))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(sets[1].rewards, want)), sets[1].rewards
    assert [len(x) for x in sets[1].rewards] == [3, 3, 2]
    assert np.array_equal(_bits(sets[1].event_rewards), _bits(h_r[:, K:]))
    # song 2 (pool rows 0, 1, 2 from step 4): the run's reward events 1 and 2; its swap follows its own row 4, after
    # window 0 closed: particle 0's first reward is row 1's
    want = (f(11.5, 20.5), f(10.5, 21.5), f(12.5))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(sets[2].rewards, want)), sets[2].rewards
    assert np.array_equal(_bits(sets[2].event_rewards), _bits(h_r[1:3, :K]))
    assert all(x.dtype == np.float32 for ps in sets for x in ps.rewards)
    assert all(ps.event_rewards.dtype == np.float32 for ps in sets)
    # the token rows follow the same lineage: song 1's particle 0 was drawn by row 4, then by row 3
    assert sets[1].songs[0][1:, 0].tolist() == [100 * t + (4 if t < 6 else 3) for t in range(11)]
    assert sets[2].songs[0][1:, 0].tolist() == [100 * (4 + t) + (1 if t < 4 else 0) for t in range(6)]
    assert sets[2].ancestors.tolist() == [[0, 1, 2], [1, 0, 2], [0, 1, 2]] and sets[2].resampled.tolist() == [0, 1, 0]
    # song 0 ended at its row 2 and waited for step 4: two steps, both beyond the next multiple of R
    assert stats == {"wait_group_steps": 2, "idle_group_steps": 0, "start_steps": [0, 0, 4],
                     "boundary_wait_group_steps": 2}
    # without the reward's arguments nothing changes: no rewards, no new key
    stats = {}
    plain = generation.particle_stream_sets(*args, K, R, 3, head, stats)
    assert all(ps.rewards is None and ps.event_rewards is None and ps.beta is None for ps in plain)
    assert sorted(stats) == ["idle_group_steps", "start_steps", "wait_group_steps"]
    for a, b in zip(plain, sets):
        assert all(np.array_equal(x, y) for x, y in zip(a.songs, b.songs)) and a.log_evidence == b.log_evidence


def test_rebuild_refuses_starts_off_the_lcm_and_open_windows():
    args, h_r = _trace()
    head = np.zeros((1, A), np.int64)
    args[0][4:6, :K, 0] = -1                                            # song 2 starts at step 6: a multiple of R, not of B
    args[7][6:9] = [4, 6, 1]
    assert len(generation.particle_stream_sets(*args, K, R, 3, head)) == 3
    with pytest.raises(RuntimeError, match="inconsistent: song 2 starts at step 6"):
        generation.particle_stream_sets(*args, K, R, 3, head, h_r=h_r, window=W)
    args, h_r = _trace()
    args[0][2:4, :K, 0] = -1                                            # song 0's group released at step 2, its window open
    assert len(generation.particle_stream_sets(*args, K, R, 3, head)) == 3
    with pytest.raises(RuntimeError, match="inconsistent: song 0 held its group for 2 steps"):
        generation.particle_stream_sets(*args, K, R, 3, head, h_r=h_r, window=W)
    args, h_r = _trace()                                                # fewer reward events than the songs' windows
    with pytest.raises(RuntimeError, match="inconsistent"):
        generation.particle_stream_sets(*args, K, R, 3, head, h_r=h_r[:2], window=W)


# ---- 3. ABI ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from rlmg_amd import _lib
    return _lib


def test_entry_declared_bound_exported(built):
    name = "cwlt_reward_apply_keyed"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cwlt.h")).read(), flags=re.S)
    lib = built.load()
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert name in built._SIGNATURES and hasattr(lib, name) and name in built.exported_names()
    assert built.ABI_VERSION >= 35 and lib.cwlt_abi_version() == built.ABI_VERSION
    from rlmg_amd import ops
    assert callable(ops.reward_apply_keyed) and callable(sampling.reward_apply_keyed_f32)


def test_entry_refusals_without_gpu(built):
    apply_ = built.load().cwlt_reward_apply_keyed
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    for at in (0, 1, 2, 7, 8):                                          # each of r, any, beta, lw, h_r null
        args = [buf, buf, buf, 3, buf, 4, 8, buf, buf]
        args[at] = null
        assert apply_(*args, null) == 1001, at
    for key in (buf, null):                                             # with and without a key
        assert apply_(buf, buf, buf, 3, key, 4, 0, buf, buf, null) == 1001      # rows
        assert apply_(buf, buf, buf, 3, key, 4, -5, buf, buf, null) == 1001
        assert apply_(buf, buf, buf, 3, key, 4, (1 << 20) + 1, buf, buf, null) == 1001
        assert apply_(buf, buf, buf, 0, key, 4, 8, buf, buf, null) == 1001      # n_beta
        assert apply_(buf, buf, buf, -1, key, 4, 8, buf, buf, null) == 1001
        assert apply_(buf, buf, buf, 3, key, 0, 8, buf, buf, null) == 1001      # particles
        assert apply_(buf, buf, buf, 3, key, -2, 8, buf, buf, null) == 1001


# ---- 4. Python-level refusals ------------------------------------------------------------------------------------------
def test_stream_reward_refusals_come_first(tmp_path):
    """Made before the model is looked at (no GPU, no model needed)."""
    w2e = {"bar-beat": {0: 0, 1: "Bar"}}
    fn = lambda windows, mask: None                                     # noqa: E731
    refuse = generation._particle_stream_refusals
    for every, window, chunk in ((4, 8, 16), (8, 4, 16), (4, 6, 24)):
        assert refuse(8, 4, 2, every, chunk, None, fn, window) is None
        assert refuse(8, 4, 2, every, chunk, None, fn, reward_window=window) is None
    for every, window, chunk, lcm in ((4, 6, 16, 12), (16, 50, 128, 400)):
        with pytest.raises(ValueError, match="reward= with slots=") as e:
            refuse(8, 4, 2, every, chunk, None, fn, window)
        assert "lcm" in str(e.value) and " %d" % lcm in str(e.value) and "for example" in str(e.value)
    assert refuse(8, 4, 2, 4, 16, None, None, 6) is None                # no reward: the window is of no account
    gp = generation.generate_particles
    with pytest.raises(ValueError, match=r"reward= with slots=.* = 400"):
        gp(None, w2e, 8, 4, slots=2, reward=fn)                         # the defaults: R 16, W 50, chunk 128
    with pytest.raises(ValueError, match="particles must be"):          # the lcm rule holds: the next refusal is met
        gp(None, w2e, 8, 1, slots=2, reward=fn, resample_every=4, reward_window=8, chunk=16)
    # the callable check still comes first, then the window, then beta
    with pytest.raises(TypeError, match="reward must be a callable"):
        gp(None, w2e, 8, 4, slots=2, reward=1.5, beta=[1.0], reward_window=0)
    with pytest.raises(ValueError, match="reward_window"):
        gp(None, w2e, 8, 4, slots=2, reward=fn, beta=[1.0], reward_window=0)
    for slots in (None, 2):
        kw = dict(slots=slots, reward=fn, resample_every=4, reward_window=8, chunk=16)
        with pytest.raises(ValueError, match="beta: 2 entries for 3 songs"):
            gp(None, w2e, 3, 4, beta=[1.0, 2.0], **kw)
        with pytest.raises(ValueError, match="entry of beta must be finite"):
            gp(None, w2e, 3, 4, beta=[1.0, float("nan"), 2.0], **kw)
        with pytest.raises(ValueError, match="entry of beta must be finite"):
            gp(None, w2e, 3, 4, beta=(1.0, 2.0, float("inf")), **kw)
        with pytest.raises(ValueError, match="beta must be finite, got nan"):   # a scalar: the message as it was
            gp(None, w2e, 3, 4, beta=float("nan"), **kw)
        with pytest.raises(ValueError, match="particles must be"):      # a good list passes on to the next refusal
            gp(None, w2e, 3, 1, beta=np.float32([1.0, 0.0, -2.0]), **kw)
    gen = generation.generate
    with pytest.raises(ValueError, match=r"reward= with slots=.*lcm\(16, 50\) = 400"):
        gen(None, w2e, n_songs=2, particles=4, slots=2, reward=fn, path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="beta: 3 entries for 2 songs"):
        gen(None, w2e, n_songs=2, particles=4, slots=2, reward=fn, reward_window=32, beta=[1.0, 2.0, 3.0],
            path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="particles must be"):          # R 16, W 32 at generate's chunk of 128: accepted
        gen(None, w2e, n_songs=2, particles=1, slots=2, reward=fn, reward_window=32, beta=[1.0, 2.0],
            path_gendir=str(tmp_path))
    # without a reward beta is not used, and a sequence is not looked at: the next refusal is met
    for slots in (None, 2):
        with pytest.raises(ValueError, match="particles must be"):
            gp(None, w2e, 3, 1, slots=slots, beta=[1.0, float("nan")])
    assert generation._reward_spec(None, 4, [float("nan")], 3) is None
    ps = generation.ParticleSet([], [], np.zeros(0, np.float32), 0.0, None, None, None)
    assert ps.beta is None and ps.rewards is None
    assert generation._reward_spec(fn, 4, [1, 2.5], 2) == (fn, 4, (1.0, 2.5))
    assert generation._reward_spec(fn, 4, 3) == (fn, 4, 3.0) and generation._reward_spec(None, 4, [1.0]) is None

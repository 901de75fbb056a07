"""CPU: reward terms in the particles' weights -- the float32 restatement of the weight update, the three
C-ABI entries' presence and refusals, and the Python-level refusals.  No GPU.

1. sampling.reward_apply_f32: the product is rounded before the sum (a case where an fma would differ is included); a
   row without a live slot keeps its weight bit for bit and records 0 whatever its reward holds (NaN, +-inf); beta = 0
   leaves every weight bit for bit; negative beta.
1b. generation.particle_pool_sets(h_r=, window=) on the hand-written lock-step trace of tests/test_particles_cpu.py: a
   window reward read from the ancestor's row, a run that ends inside a window, a song whose events are cut by its last
   resampling; the same trace, one step longer, through generation.particle_stream_sets.
2. cwlt_reward_push / _window / _apply are declared, bound and exported at ABI > 32, and refuse with 1001, before any
   launch: null pointers, W < 1, filled outside 1 .. W, n_attr outside 1 .. 8, rows < 1.
3. generate_particles / generate / WindowReward refuse, before the model is looked at: a reward that is not callable,
   reward_window < 1, a beta that is not finite, a reward without particles, an unknown form.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, sampling

from test_particles_cpu import check_pool_sets, pool_sets, pool_trace, same_sets, stream_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cwlt_reward_push", "cwlt_reward_window", "cwlt_reward_apply")


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# ---- 1. the restatement --------------------------------------------------------------------------------------------------
def test_apply_restatement_rounds_product_then_sum():
    rng = np.random.default_rng(3)
    lw = (rng.normal(0, 30, 64)).astype(np.float32)
    r = (rng.normal(0, 1, 64) * 10.0 ** rng.integers(-3, 3, 64)).astype(np.float32)
    on = rng.integers(0, 2, 64)
    on[:2] = (1, 0)
    for beta in (1.0, 0.3, -2.5, 100.0):
        got, rec = sampling.reward_apply_f32(lw, r, on, beta)
        assert got.dtype == np.float32 and rec.dtype == np.float32
        for n in range(64):
            want = np.float32(lw[n] + np.float32(np.float32(beta) * r[n])) if on[n] else lw[n]
            assert _bits(got[n]) == _bits(want)
            assert _bits(rec[n]) == _bits(r[n] if on[n] else np.float32(0))
    # where one rounding (an fma) and two differ: beta r = 1 + 2^-22 + 2^-46 exactly; rounded first it loses the 2^-46,
    # and the sum with -1 is 2^-22; an fma would give 2^-22 + 2^-46
    b = np.float32(1 + 2.0 ** -23)
    got, _ = sampling.reward_apply_f32(np.float32([-1.0]), [b], [1], b)
    assert float(got[0]) == 2.0 ** -22 and float(b) * float(b) - 1.0 != float(got[0])


def test_apply_restatement_dead_rows_and_beta_zero():
    lw = np.float32([1.5, -2.25, 0.0, 7.0, -0.0])
    bad = np.float32([np.nan, np.inf, -np.inf, 3.0, np.nan])
    got, rec = sampling.reward_apply_f32(lw, bad, np.zeros(5, np.int64), 2.0)
    assert np.array_equal(_bits(got), _bits(lw)) and np.array_equal(_bits(rec), _bits(np.zeros(5)))
    got, rec = sampling.reward_apply_f32(lw, bad, [0, 0, 0, 1, 0], -1.0)
    assert np.array_equal(_bits(got), _bits([1.5, -2.25, 0.0, 4.0, -0.0]))
    assert np.array_equal(_bits(rec), _bits([0, 0, 0, 3.0, 0]))
    rng = np.random.default_rng(4)
    lw = np.concatenate([rng.normal(0, 100, 200), [0.0]]).astype(np.float32)
    r = rng.normal(0, 1000, 201).astype(np.float32)
    got, rec = sampling.reward_apply_f32(lw, r, np.ones(201, np.int64), 0.0)
    assert np.array_equal(_bits(got), _bits(lw)) and np.array_equal(_bits(rec), _bits(r))


# ---- 1b. the lock-step rebuild with rewards ------------------------------------------------------------------------------
def test_pool_sets_rewards_hand_trace():
    """generation.particle_pool_sets(h_r=, window=) on tests/test_particles_cpu.py's trace: W = 4 over seven steps, one
    whole window and a last one of 3 rows, closed by the run's second reward event (h_r[i, n] = 10 i + n + 0.5)."""
    tr = pool_trace()
    sets = pool_sets(tr, reward=True)
    check_pool_sets(sets, tr)
    f = lambda *v: np.float32(v)                                        # noqa: E731
    # song 0: window 0 closed after row 4, when final particle 1's lineage still lived in row 0 (event 1 had copied row
    # 0 over row 1, the swap shows from row 5 on); the partial window closed after row 7, every lineage in its own row
    want = (f(0.5, 10.5), f(0.5, 11.5), f(2.5))
    assert [len(r) for r in sets[0].rewards] == [2, 2, 1]
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(sets[0].rewards, want)), sets[0].rewards
    assert sets[0].event_rewards.shape == (2, 3) and np.array_equal(_bits(sets[0].event_rewards), _bits(tr["h_r"][:, :3]))
    # song 1: 2, 2 and 1 rows, one window each, read after event 0 in the rows themselves; the run's second reward
    # event came after the song's last particle and its last resampling: not its own
    want = (f(3.5), f(4.5), f(5.5))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(sets[1].rewards, want)), sets[1].rewards
    assert sets[1].event_rewards.shape == (1, 3) and np.array_equal(_bits(sets[1].event_rewards), _bits(tr["h_r"][:1, 3:]))
    assert all(r.dtype == np.float32 for ps in sets for r in ps.rewards)
    assert all(ps.event_rewards.dtype == np.float32 and ps.beta is None for ps in sets)
    # the other fields are those of the run without a reward
    for a, b in zip(sets, pool_sets(tr, reward=False)):
        a.rewards = a.event_rewards = None
        assert same_sets(a, b)


def test_pool_trace_with_rewards_as_a_stream_trace():
    """Eight steps, so that the second window closes inside the run: the stream's rebuild gives the pool's sets, rewards
    and event_rewards included, and both give the seven-step run's rewards."""
    tr = pool_trace(T=8)
    pool, stream = pool_sets(tr, reward=True), stream_sets(tr, reward=True)
    check_pool_sets(pool, tr)
    assert len(stream) == 2 and all(same_sets(a, b) for a, b in zip(stream, pool))
    for a, b in zip(pool, pool_sets(pool_trace(), reward=True)):
        assert same_sets(a, b)


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
    assert built.ABI_VERSION > 32 and lib.cwlt_abi_version() == built.ABI_VERSION
    from rlmg_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("reward_push", "reward_window", "reward_apply"))
    assert callable(sampling.reward_apply_f32) and callable(generation.WindowReward)


def test_refusals_without_gpu(built):
    lib = built.load()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    push = lib.cwlt_reward_push
    for at in range(3):                                                # each of tok, done, counter null
        ptrs = [buf] * 3
        ptrs[at] = null
        assert push(*ptrs, 4, 6, 50, buf, buf, null) == 1001
    assert push(buf, buf, buf, 4, 6, 50, null, buf, null) == 1001
    assert push(buf, buf, buf, 4, 6, 50, buf, null, null) == 1001
    assert push(buf, buf, buf, 0, 6, 50, buf, buf, null) == 1001        # rows
    assert push(buf, buf, buf, -1, 6, 50, buf, buf, null) == 1001
    assert push(buf, buf, buf, 4, 0, 50, buf, buf, null) == 1001        # n_attr
    assert push(buf, buf, buf, 4, 9, 50, buf, buf, null) == 1001
    assert push(buf, buf, buf, 4, 6, 0, buf, buf, null) == 1001         # W
    assert push(buf, buf, buf, 4, 6, -3, buf, buf, null) == 1001
    window = lib.cwlt_reward_window
    for at in (0, 1, 6, 7, 8):
        args = [buf, buf, 4, 6, 50, 50, buf, buf, buf]
        args[at] = null
        assert window(*args, null) == 1001
    assert window(buf, buf, 0, 6, 50, 50, buf, buf, buf, null) == 1001  # rows
    assert window(buf, buf, 4, 0, 50, 50, buf, buf, buf, null) == 1001  # n_attr
    assert window(buf, buf, 4, 9, 50, 50, buf, buf, buf, null) == 1001
    assert window(buf, buf, 4, 6, 0, 1, buf, buf, buf, null) == 1001    # W
    assert window(buf, buf, 4, 6, 50, 0, buf, buf, buf, null) == 1001   # filled
    assert window(buf, buf, 4, 6, 50, 51, buf, buf, buf, null) == 1001
    assert window(buf, buf, 4, 6, 50, -1, buf, buf, buf, null) == 1001
    apply_ = lib.cwlt_reward_apply
    for at in (0, 1, 4, 5):
        args = [buf, buf, 1.0, 4, buf, buf]
        args[at] = null
        assert apply_(*args, null) == 1001
    assert apply_(buf, buf, 1.0, 0, buf, buf, null) == 1001             # rows
    assert apply_(buf, buf, 1.0, -5, buf, buf, null) == 1001


# ---- 3. Python-level refusals ------------------------------------------------------------------------------------------
def test_reward_refusals_come_first():
    """Made before the model is looked at (no GPU, no model needed)."""
    w2e = {"bar-beat": {0: 0, 1: "Bar"}}
    fn = lambda windows, mask: None                                     # noqa: E731
    with pytest.raises(TypeError, match="reward must be a callable"):
        generation.generate_particles(None, w2e, 3, 4, reward=1.5)
    for kw, msg in ((dict(reward_window=0), "reward_window"), (dict(reward_window=-2), "reward_window"),
                    (dict(beta=float("nan")), "beta must be finite"), (dict(beta=float("inf")), "beta must be finite"),
                    (dict(beta=-float("inf")), "beta must be finite")):
        with pytest.raises(ValueError, match=msg):
            generation.generate_particles(None, w2e, 3, 4, reward=fn, **kw)
    # the particle refusals still come, after the reward's
    with pytest.raises(ValueError, match="particles must be"):
        generation.generate_particles(None, w2e, 3, 1, reward=fn)
    # a reward on an entry that is not the particle path
    for kw in (dict(), dict(batch_size=2), dict(slots=4)):
        with pytest.raises(ValueError, match="pass particles="):
            generation.generate(None, w2e, n_songs=2, reward=fn, **kw)
    with pytest.raises(ValueError, match="pass batch_size"):
        generation.generate(None, w2e, n_songs=2, particles=4, reward=fn)
    with pytest.raises(TypeError, match="reward must be a callable"):
        generation.generate(None, w2e, n_songs=2, batch_size=2, particles=4, reward="disc")
    with pytest.raises(ValueError, match="reward_window"):
        generation.generate(None, w2e, n_songs=2, batch_size=2, particles=4, reward=fn, reward_window=0)


def test_window_reward_refusals_and_defaults():
    disc = lambda windows, mask: None                                   # noqa: E731
    wr = generation.WindowReward(disc)
    assert wr.form == "log_odds" and wr.eps == 1e-6 and callable(wr)
    for form in ("log_odds", "log", "score"):
        assert generation.WindowReward(disc, form=form).form == form
    with pytest.raises(ValueError, match="form must be"):
        generation.WindowReward(disc, form="logit")
    with pytest.raises(TypeError, match="disc must be"):
        generation.WindowReward(None)
    with pytest.raises(ValueError, match="eps must"):
        generation.WindowReward(disc, eps=0.5)
    import inspect
    sig = inspect.signature(generation.generate_particles).parameters
    assert sig["reward"].default is None and sig["reward_window"].default == 50 and sig["beta"].default == 1.0
    ps = generation.ParticleSet([], [], np.zeros(0, np.float32), 0.0, None, None, None)
    assert ps.rewards is None and ps.event_log_weights is None

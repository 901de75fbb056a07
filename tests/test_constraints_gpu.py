"""GPU: constrained generation -- the masked sampler (cwlt_sample_categorical_masked) against the unmasked entries and an
exact numpy model of its draw, and generate_stream(constraints=...) against generate_batch(constraints=...): bitwise
equal songs, no violations, permissive constraints equal to no constraint, graph equal to eager, generate() and the
refusals."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]


def _small_model(cuda):
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": 2, "N_HEAD": 2})
    try:
        net = model.LinearTransformer(N_CLASS, is_training=False)
    finally:
        config.AgentConfig.update(old)
    return fill_params(net, seed=int(FIX["fill_seed"])).to(cuda).eval()


def _word2event():
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(KEYS, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    w2e["bar-beat"][9] = "Bar"
    return w2e


def _constraints(w2e):
    """A fixed tempo, a pitch range and a cycled chord progression; a bar-beat schedule; a permissive one."""
    musical = generation.Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(5, 12)},
                                    per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7], ["chord_4"]]},
                                    cycle=True)
    beats = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar", "bar-beat_3"], ["Bar", "bar-beat_4", 5]],
                                                "velocity": [[2], [3, 4], [5]]}, keep_neutral=False)
    return musical, beats


def _prompts(lengths, seed, max_bars=2):
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        p = np.stack([rng.integers(0, c, n) for c in N_CLASS], 1).astype(np.int64)
        p[:, 2] = np.where(p[:, 2] == 9, 0, p[:, 2])
        bars = np.nonzero(p[1:, 2] == 1)[0] + 1
        p[bars[max_bars - 1:], 2] = 0
        out.append(p)
    return out


def _bar0(w2e, p):
    return 1 + sum(w2e["bar-beat"][int(r[2])] == "Bar" for r in p[1:])


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def _no_violations(w2e, songs, cons, heads):
    for k, (s, p) in enumerate(zip(songs, heads)):
        c = cons[k] if isinstance(cons, (list, tuple)) else cons
        if c is not None:
            assert c.violations(s[len(p):], bar0=_bar0(w2e, p)) == [], k


def _device_table(cons, n, bar_cond, bar0s, cuda):
    sched, masks = generation.compile_constraints(cons, n, N_CLASS, bar_cond, bar0s, 1000)
    return (torch.as_tensor(sched, device=cuda),
            torch.as_tensor(np.ascontiguousarray(masks).view(np.int32), device=cuda), masks)


# ---- 1. all-ones masks: bitwise the unmasked draw --------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_all_ones_mask_is_unmasked(cuda, sampler):
    rows, W, A = 24, sum(N_CLASS), len(N_CLASS)
    g = torch.Generator(device=cuda).manual_seed(3)
    L = torch.randn(rows, W, device=cuda, generator=g) * 3
    temp, top_p = (generation.DQN_TEMPERATURE, generation.DQN_TOP_P) if sampler == "dqn" else (None, None)
    w2e = _word2event()
    sched, masks, _ = _device_table(generation.Constraint(w2e), rows, 17, [1] * rows, cuda)
    rng = np.random.default_rng(1)
    bar = torch.as_tensor(rng.integers(1, 20, rows), device=cuda)
    key = torch.as_tensor(rng.permutation(rows), device=cuda)
    step = torch.as_tensor(rng.choice([0, 5, 77, 4000], rows), device=cuda)
    want = torch.zeros(rows, A, dtype=torch.int64, device=cuda)
    ops.sample_categorical_keyed(L, N_CLASS, want, 99, key, step, temperature=temp, top_p=top_p)
    got = torch.zeros_like(want)
    ops.sample_categorical_masked(L, N_CLASS, got, 99, bar, sched, masks, key=key, step=step, temperature=temp,
                                  top_p=top_p)
    assert torch.equal(got, want)
    for c in (0, 9, 123):
        cnt = torch.tensor([c], device=cuda)
        want = torch.zeros(rows, A, dtype=torch.int64, device=cuda)
        ops.sample_categorical(L, N_CLASS, want, 99, counter=cnt, temperature=temp, top_p=top_p, slot_keys=True)
        got = torch.zeros_like(want)
        ops.sample_categorical_masked(L, N_CLASS, got, 99, bar, sched, masks, counter=cnt, temperature=temp,
                                      top_p=top_p)
        assert torch.equal(got, want), c
    # every song constrained to class 3: rows with a negative key (idle -1 / waiting -2 stream slots) draw unmasked
    tight = generation.Constraint(w2e, allow={k: [3] for k in KEYS}, keep_neutral=False)
    sched, masks, _ = _device_table(tight, rows, 17, [1] * rows, cuda)
    neg = key.clone()
    neg[0::2] = -1
    neg[1::4] = -2
    want = torch.zeros(rows, A, dtype=torch.int64, device=cuda)
    ops.sample_categorical_keyed(L, N_CLASS, want, 99, neg, step, temperature=temp, top_p=top_p)
    got = torch.zeros_like(want)
    ops.sample_categorical_masked(L, N_CLASS, got, 99, bar, sched, masks, key=neg, step=step, temperature=temp,
                                  top_p=top_p)
    idle = neg < 0
    assert torch.equal(got[idle], want[idle])
    assert (got[~idle] == 3).all()


# ---- 2. exact model of the masked draw -------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def _hash32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def _rng_pair(seed, idx):
    lo, hi = idx & M32, (idx >> 32) & M32
    key = (seed & M32) ^ (((seed >> 32) * 0x9e3779b9) & M32) ^ ((hi * 0x85ebca6b) & M32)
    return _hash32(((lo * 0x9e3779b1) & M32) ^ key)


def _model_pick(x, allowed, inv_t, top_p, u):
    """-> (pick, ambiguous): the masked temperature / nucleus draw in float64."""
    v = np.where(allowed, x.astype(np.float64) * inv_t, -np.inf)
    e = np.where(allowed, np.exp(v - v[allowed].max()), 0.0)
    tot = e.sum()
    amb = False
    if top_p < 1.0:
        idx = np.arange(len(e))
        ahead = np.array([e[(e > e[i]) | ((e == e[i]) & (idx > i))].sum() for i in range(len(e))])
        limit = top_p * tot * (1 + 1e-5)
        amb = bool((np.abs(ahead[allowed] - limit) <= 1e-5 * tot).any())
        e = np.where(ahead <= limit, e, 0.0)
    cum = np.cumsum(e)
    total = cum[-1]
    target = u * total
    pick = int(np.nonzero((cum > target) & (e > 0))[0][0]) if (cum > target).any() else int(np.nonzero(e > 0)[0][-1])
    amb = amb or bool((np.abs(cum[e > 0] - target) <= 1e-5 * total).any())
    return pick, amb


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_masked_draw_model(cuda, sampler):
    rows, A = 64, len(N_CLASS)
    off = np.cumsum([0] + N_CLASS)
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((rows, off[-1])) * 2).astype(np.float32)
    temp, top_p = (generation.DQN_TEMPERATURE, generation.DQN_TOP_P) if sampler == "dqn" else (None, None)
    inv_t = [1.0 if temp is None else np.float32(1.0) / np.float32(t) for t in (temp or [1.0] * A)]
    tps = [1.0 if top_p is None or p is None else p for p in (top_p or [None] * A)]
    # one mask row per song: random sets, single classes, and allowed logits 100 below a disallowed maximum
    allowed = np.zeros((rows, off[-1]), dtype=bool)
    for n in range(rows):
        for a in range(A):
            seg = slice(off[a], off[a + 1])
            kind = n % 3
            if kind == 0:
                allowed[n, seg] = rng.random(N_CLASS[a]) < 0.4
                allowed[n, off[a] + rng.integers(N_CLASS[a])] = True
            elif kind == 1:
                allowed[n, off[a] + rng.integers(N_CLASS[a])] = True
            else:
                ok = rng.random(N_CLASS[a]) < 0.5
                ok[rng.integers(N_CLASS[a])] = True
                ok[-1] = False
                allowed[n, seg] = ok
                x[n, seg] = np.where(ok, x[n, seg] - 100.0, x[n, seg])
                x[n, off[a + 1] - 1] = 5.0                         # the disallowed maximum
    W = -(-off[-1] // 32)
    bits = np.zeros((rows, W * 32), dtype=bool)
    bits[:, :off[-1]] = allowed
    masks = np.packbits(bits, axis=1, bitorder="little").view("<u4")
    # song k uses mask row k, reached through a 2-row schedule at bar 2 (row first + 1): first = k - 1
    sched = np.stack([np.arange(rows) - 1, np.full(rows, 2)], 1).astype(np.int64)
    masks_dev = torch.as_tensor(np.concatenate([masks, masks[:1]]).view(np.int32), device=cuda)
    sched[0] = (rows, 1)                                               # row 0's copy sits at the end, one-row schedule
    key = rng.permutation(rows)
    step = rng.integers(0, 5000, rows)
    L = torch.as_tensor(x[key], device=cuda)
    got = torch.zeros(rows, A, dtype=torch.int64, device=cuda)
    ops.sample_categorical_masked(L, N_CLASS, got, 4242, torch.full((rows,), 2, dtype=torch.int64, device=cuda),
                                  torch.as_tensor(sched, device=cuda), masks_dev,
                                  key=torch.as_tensor(key, device=cuda), step=torch.as_tensor(step, device=cuda),
                                  temperature=temp, top_p=top_p)
    got = got.cpu().numpy()
    checked = 0
    for n in range(rows):
        k = int(key[n])
        for a in range(A):
            r = _rng_pair(4242, ((k << 40) + int(step[n])) * 8 + a)
            u = (r >> 8) * (1.0 / 16777216.0)
            seg = slice(off[a], off[a + 1])
            pick, amb = _model_pick(x[k, seg], allowed[k, seg], inv_t[a], tps[a], u)
            assert allowed[k, off[a] + got[n, a]], (n, a, got[n, a])
            if not amb:
                assert got[n, a] == pick, (n, a, got[n, a], pick)
                checked += 1
    assert checked > rows * A * 0.9


# ---- 3-5. stream == batch under constraints, no violations, permissive == unconstrained -----------------------------
@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_stream_equals_batch_constrained(cuda, sampler):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    n = 20
    per_song = [musical if i % 3 == 0 else beats if i % 3 == 1 else None for i in range(n)]
    heads = [generation.INIT_CW[0][None]] * n
    for cons in (musical, per_song):
        torch.manual_seed(21)
        ref = generation.generate_batch(net, w2e, n, bar_cond=5, max_tokens=160, sampler=sampler, chunk=32,
                                        constraints=cons)
        _no_violations(w2e, ref, cons, heads)
        for slots in (1, 7, 40):
            torch.manual_seed(21)
            got = generation.generate_stream(net, w2e, n, slots=slots, bar_cond=5, max_tokens=160, sampler=sampler,
                                             chunk=16, constraints=cons)
            assert _same(got, ref), slots
    # a constraint that allows every class: the unconstrained songs, bitwise
    torch.manual_seed(22)
    free_b = generation.generate_batch(net, w2e, n, bar_cond=5, max_tokens=160, sampler=sampler)
    torch.manual_seed(22)
    free_s = generation.generate_stream(net, w2e, n, slots=7, bar_cond=5, max_tokens=160, sampler=sampler)
    everything = generation.Constraint(w2e, allow={k: list(range(c)) for k, c in zip(KEYS, N_CLASS)})
    for cons in (generation.Constraint(w2e), everything):
        torch.manual_seed(22)
        assert _same(generation.generate_batch(net, w2e, n, bar_cond=5, max_tokens=160, sampler=sampler,
                                               constraints=cons), free_b)
        torch.manual_seed(22)
        assert _same(generation.generate_stream(net, w2e, n, slots=7, bar_cond=5, max_tokens=160, sampler=sampler,
                                                constraints=cons), free_s)
    assert _same(free_b, free_s)


def test_stream_prompts_equal_batch_constrained(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    prompts = _prompts([3, 17, 1, 40, 9, 25, 2, 30, 12, 5, 8, 21], seed=3)
    n = len(prompts)
    per_song = [beats if i % 2 else musical for i in range(n)]
    per_song[5] = None
    for cons in (musical, per_song):
        torch.manual_seed(31)
        ref = generation.generate_batch(net, w2e, n, bar_cond=6, max_tokens=150, prompts=prompts, prefill="gemm",
                                        chunk=32, constraints=cons)
        _no_violations(w2e, ref, cons, prompts)
        for slots in (1, 7, 40):
            torch.manual_seed(31)
            got = generation.generate_stream(net, w2e, n, slots=slots, bar_cond=6, max_tokens=150, prompts=prompts,
                                             chunk=16, bank=4, prefill_rows=64, constraints=cons)
            assert _same(got, ref), slots
    # no max_tokens: songs end by the bar rule under a schedule that keeps a Bar class in every bar
    torch.manual_seed(32)
    ref = generation.generate_batch(net, w2e, n, bar_cond=4, prompts=prompts, prefill="gemm", constraints=beats)
    torch.manual_seed(32)
    got = generation.generate_stream(net, w2e, n, slots=5, bar_cond=4, prompts=prompts, constraints=beats)
    assert _same(got, ref)
    _no_violations(w2e, got, beats, prompts)


# ---- 6. graph replay == eager ----------------------------------------------------------------------------------------
def test_constrained_graph_equals_eager(cuda, monkeypatch):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    cons = [musical, beats, None] * 4
    torch.manual_seed(5)
    graphed, st = generation._generate_stream(net, w2e, 12, slots=5, bar_cond=4, max_tokens=120, chunk=8,
                                              constraints=cons)
    assert st["graph"]
    torch.manual_seed(5)
    batch_g = generation.generate_batch(net, w2e, 12, bar_cond=4, max_tokens=120, chunk=8, constraints=cons)
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    torch.manual_seed(5)
    eager, st = generation._generate_stream(net, w2e, 12, slots=5, bar_cond=4, max_tokens=120, chunk=8,
                                            constraints=cons)
    assert not st["graph"]
    torch.manual_seed(5)
    batch_e = generation.generate_batch(net, w2e, 12, bar_cond=4, max_tokens=120, chunk=8, constraints=cons)
    assert _same(graphed, eager) and _same(batch_g, batch_e) and _same(graphed, batch_g)


# ---- 7. generate() and the refusals ----------------------------------------------------------------------------------
def test_generate_with_constraints(cuda, tmp_path):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    cons = [musical, None, beats, musical, beats]
    for mode, kw in (("slots", {"slots": 2}), ("batch", {"batch_size": 2})):
        d = tmp_path / mode
        torch.manual_seed(41)
        stats = generation.generate(net, w2e, n_songs=5, bar_cond=3, path_gendir=str(d), max_tokens=100,
                                    stats_path=str(tmp_path / ("%s.json" % mode)), log=lambda *a: None,
                                    constraints=cons, **kw)
        assert len(stats["song_time"]) == 5
        for i in range(5):
            s = np.load(d / ("get_%d.npy" % i))
            assert s.shape == (stats["words_len_list"][i], 6)
            if cons[i] is not None:
                assert cons[i].violations(s[1:]) == [], (mode, i)
    # batch groups of 2 slice the list: the songs are those of one generate_batch per group
    torch.manual_seed(41)
    g0 = generation.generate_batch(net, w2e, 2, bar_cond=3, max_tokens=100, constraints=cons[:2])
    assert all((np.load(tmp_path / "batch" / ("get_%d.npy" % i)) == g0[i]).all() for i in range(2))


def test_constraint_refusals_gpu(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, _ = _constraints(w2e)
    no_bar = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar"], ["bar-beat_3"]]})
    with pytest.raises(ValueError, match="never"):
        generation.generate_stream(net, w2e, 3, slots=2, bar_cond=4, constraints=no_bar)
    with pytest.raises(ValueError, match="never"):
        generation.generate_batch(net, w2e, 3, bar_cond=4, constraints=no_bar)
    with pytest.raises(ValueError, match="never"):
        generation.generate_stream(net, w2e, 2, slots=2, bar_cond=4, prompts=_prompts([4, 6], 1),
                                   constraints=no_bar)
    with pytest.raises(ValueError, match="2 entries for 3 songs"):
        generation.generate_stream(net, w2e, 3, slots=2, bar_cond=4, max_tokens=50, constraints=[musical, None])
    with pytest.raises(ValueError, match="2 entries for 3 songs"):
        generation.generate_batch(net, w2e, 3, bar_cond=4, max_tokens=50, constraints=[musical, None])
    with pytest.raises(ValueError, match="generate_batch\\(n_songs=1"):
        generation.generate(net, w2e, n_songs=1, bar_cond=3, stats_path=None, log=lambda *a: None,
                            device_sampling=True, constraints=musical)
    other = {k: dict(v) for k, v in w2e.items()}
    other["pitch"][len(other["pitch"])] = "extra"
    with pytest.raises(ValueError, match="classes"):
        generation.generate_batch(net, w2e, 2, bar_cond=4, max_tokens=50,
                                  constraints=generation.Constraint(other, allow={"pitch": ["extra"]}))


# ---- 8. repo dims --------------------------------------------------------------------------------------------------
def test_constraints_repo_dims(cuda):
    from rlmg_amd import data
    from rlmg_amd.dqn_policy import model
    w2e = {k: v for k, v in data.synthetic_cp_vocabulary().items() if k != "type"}
    n_class = [len(v) for v in w2e.values()]
    net = fill_params(model.LinearTransformer(n_class, is_training=False), seed=5).to(cuda).eval()
    musical = generation.Constraint(w2e, allow={"tempo": ["Tempo_110"],
                                                "pitch": ["Note_Pitch_%d" % p for p in range(55, 80)]},
                                    per_bar={"chord": [["C_M"], ["A_m"], ["F_M"], ["G_7"]]}, cycle=True)
    torch.manual_seed(7)
    ref = generation.generate_batch(net, w2e, 512, bar_cond=5, max_tokens=256, constraints=musical)
    torch.manual_seed(7)
    got = generation.generate_stream(net, w2e, 512, slots=256, bar_cond=5, max_tokens=256, chunk=64,
                                     constraints=musical)
    assert _same(got, ref)
    assert sum(len(musical.violations(s[1:])) for s in got) == 0
    # the constraint did bite: chord and tempo ids are only neutral or allowed ones
    rows = np.concatenate([s[1:] for s in got])
    assert set(np.unique(rows[:, 0]).tolist()) <= {0, 1, [k for k, e in w2e["tempo"].items() if e == "Tempo_110"][0]}

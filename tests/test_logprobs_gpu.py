"""GPU: song log-likelihoods -- the log-prob sampler (cwlt_sample_categorical_logp) against the existing
entries and a float64 restatement, the scorer (cwlt_score_categorical) bitwise against the sampler, score_songs against
the reference fixture, its batch invariance and constraint masks, and return_logprobs on generate_batch /
generate_stream: the same songs, stream == batch bitwise, generated == scored, and the refusals."""
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
from rlmg_amd.sampling import logprobs_f64  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
OFF = np.concatenate([[0], np.cumsum(N_CLASS)])
DQN = (generation.DQN_TEMPERATURE, generation.DQN_TOP_P)


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


def _songs(lengths, seed, max_bars=3):
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        p = np.stack([rng.integers(0, c, n) for c in N_CLASS], 1).astype(np.int64)
        p[:, 2] = np.where(p[:, 2] == 9, 0, p[:, 2])
        bars = np.nonzero(p[1:, 2] == 1)[0] + 1
        p[bars[max_bars - 1:], 2] = 0
        out.append(p)
    return out


def _constraints(w2e):
    musical = generation.Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(5, 12)},
                                    per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7], ["chord_4"]]},
                                    cycle=True)
    beats = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar", "bar-beat_3"], ["Bar", "bar-beat_4", 5]],
                                                "velocity": [[2], [3, 4], [5]]}, keep_neutral=False)
    return musical, beats


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)
                                    for x, y in zip(a, b))


def _ratio(logits, temperature, top_p, allowed=None):
    """Per class, the nucleus test value ahead / total / (1 + 1e-5) of logprobs_f64 (float64)."""
    x = np.asarray(logits, dtype=np.float64) / temperature
    ok = np.ones(len(x), dtype=bool) if allowed is None else allowed
    m = x[ok].max()
    e = np.where(ok, np.exp(np.where(ok, x, m) - m), 0.0)
    order = np.lexsort((-np.arange(len(x)), -e))
    ahead = np.empty(len(x))
    ahead[order] = np.concatenate([[0.0], np.cumsum(e[order])[:-1]])
    return ahead / e.sum() / (1.0 + 1e-5)


def _near_boundary(logits, temperature, top_p, allowed=None, tol=1e-5):
    return top_p is not None and np.abs(_ratio(logits, temperature, top_p, allowed) - top_p).min() < tol


def _check_f64(logits, tokens, lp, settings, allowed=None, tol=1e-5):
    """lp (rows, A, 2) within tol of logprobs_f64; an entry off by more must sit at a nucleus boundary."""
    temps, tops = settings
    for n in range(len(tokens)):
        for a in range(len(N_CLASS)):
            x = logits[n, OFF[a]:OFF[a + 1]]
            t = 1.0 if temps is None else temps[a]
            p = None if tops is None else tops[a]
            al = None if allowed is None else allowed[n][a]
            want = logprobs_f64(x, tokens[n, a], t, p, al)
            assert abs(lp[n, a, 0] - want[0]) <= tol, (n, a, lp[n, a], want)
            if np.isinf(want[1]) or np.isinf(lp[n, a, 1]) or abs(lp[n, a, 1] - want[1]) > tol:
                if not (np.isinf(want[1]) and np.isinf(lp[n, a, 1])):
                    assert _near_boundary(x, t, p, al), (n, a, lp[n, a], want)


# ---- 1-2. score_songs against the reference fixture --------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["gemm", "blas"])
def test_fixture_model_logprobs(cuda, kernel):
    net = _small_model(cuda)
    toks = FIX["tokens"]
    got = generation.score_songs(net, _word2event(), [toks], kernel=kernel)[0]
    assert got.shape == (len(toks) - 1, 6, 2) and got.dtype == np.float32
    for t in range(len(toks) - 1):
        lg = FIX["logits"][t].astype(np.float64)
        for a in range(6):
            x = lg[OFF[a]:OFF[a + 1]]
            want = x[toks[t + 1, a]] - x.max() - np.log(np.exp(x - x.max()).sum())
            assert abs(got[t, a, 0] - want) < 1e-4, (t, a)
    # categorical without a constraint: q is the model softmax
    assert np.abs(got[..., 1] - got[..., 0]).max() < 1e-6


def test_fixture_dqn_sampler_logprobs(cuda):
    net = _small_model(cuda)
    toks = FIX["tokens"]
    got = generation.score_songs(net, _word2event(), [toks], sampler="dqn")[0]
    assert np.isfinite(got).all()                   # the reference's own samplers drew these tokens
    for t in range(len(toks) - 1):
        for a in range(6):
            x = FIX["logits"][t][OFF[a]:OFF[a + 1]]
            want = logprobs_f64(x, toks[t + 1, a], DQN[0][a], DQN[1][a])
            assert abs(got[t, a, 1] - want[1]) < 1e-4 and abs(got[t, a, 0] - want[0]) < 1e-4, (t, a)


# ---- 3-4. the log-prob sampler and the scorer ------------------------------------------------------------------------
def _random_logits(cuda, rows, seed, ld_pad=5):
    g = torch.Generator().manual_seed(seed)
    W = int(OFF[-1])
    lg = 2.5 * torch.randn(rows, W + ld_pad, generator=g)
    lg[:rows // 4, :W] = torch.round(lg[:rows // 4, :W])          # ties in the first quarter
    return lg.to(cuda)[:, :W]                                    # a row stride != W


def _table(cuda, rows, seed):
    """A random constraint table: 5 songs' schedules over 7 mask rows, one song without rows."""
    rng = np.random.default_rng(seed)
    W = -(-int(OFF[-1]) // 32)
    bits = rng.random((7, W * 32)) < 0.6
    for r in range(7):                                            # keep every attribute non-empty
        for a in range(6):
            bits[r, OFF[a] + rng.integers(0, N_CLASS[a])] = True
    masks = np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(7, W)
    sched = np.array([[0, 3], [3, 1], [4, 3], [0, 0], [2, 5]], dtype=np.int64)
    bar = rng.integers(0, 6, rows).astype(np.int64)
    return sched, masks, bar, bits


def _allowed(sched, bits, bar, keys):
    out = []
    for n, k in enumerate(keys):
        al = [np.ones(c, dtype=bool) for c in N_CLASS]
        if 0 <= k < len(sched) and sched[k, 1] > 0:
            r = sched[k, 0] + min(max(bar[n] - 1, 0), sched[k, 1] - 1)
            al = [bits[r, OFF[a]:OFF[a + 1]].copy() for a in range(6)]
        out.append(al)
    return out


@pytest.mark.parametrize("settings", [DQN, (None, None)], ids=["dqn", "categorical"])
def test_logp_sampler_forms(cuda, settings):
    rows = 96
    logits = _random_logits(cuda, rows, 3)
    host = logits.cpu().numpy()
    temps, tops = settings
    sched, masks, bar, bits = _table(cuda, rows, 4)
    d_sched = torch.as_tensor(sched).to(cuda)
    d_masks = torch.as_tensor(masks.view(np.int32)).to(cuda)
    d_bar = torch.as_tensor(bar).to(cuda)
    key = torch.as_tensor(np.random.default_rng(5).integers(-1, 7, rows)).to(cuda)
    step = torch.as_tensor(np.random.default_rng(6).integers(0, 1000, rows)).to(cuda)
    counter = torch.tensor([17], dtype=torch.int64, device=cuda)
    seed = 1234
    new = lambda: torch.full((rows, 6), -7, dtype=torch.int64, device=cuda)
    for form in ("slots", "keyed", "masked", "masked_keyed"):
        ref = new()
        masked = form.startswith("masked")
        keyed = form.endswith("keyed")
        kw = dict(temperature=temps, top_p=tops)
        if form == "slots":
            ops.sample_categorical(logits, N_CLASS, ref, seed, counter=counter, slot_keys=True, **kw)
        elif form == "keyed":
            ops.sample_categorical_keyed(logits, N_CLASS, ref, seed, key, step, **kw)
        else:
            ops.sample_categorical_masked(logits, N_CLASS, ref, seed, d_bar, d_sched, d_masks,
                                          counter=None if keyed else counter, key=key if keyed else None,
                                          step=step if keyed else None, **kw)
        # a 3-row ring at out_counter 5 -> row 2; rows 0 and 1 stay untouched
        ring = torch.full((3, rows, 6, 2), 7.0, dtype=torch.float32, device=cuda)
        got = new()
        m = dict(bar=d_bar, sched=d_sched, masks=d_masks) if masked else {}
        ops.sample_categorical_logp(logits, N_CLASS, got, seed, ring, counter=None if keyed else counter,
                                    key=key if keyed else None, step=step if keyed else None,
                                    out_counter=torch.tensor([5], dtype=torch.int64, device=cuda), **m, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), form
        assert (ring[:2] == 7.0).all()
        lp = ring[2].cpu().numpy()
        toks = got.cpu().numpy()
        keys = key.cpu().numpy() if keyed else np.arange(rows)
        allowed = _allowed(sched, bits, bar, keys) if masked else None
        assert np.isfinite(lp[..., 0]).all()
        assert np.isfinite(lp[..., 1]).all()            # a drawn class is always inside the kept set
        _check_f64(host, toks, lp, settings, allowed)
        # the scorer on the same logits at the drawn classes: the sampler's bits; padding rows untouched
        tgt = got.clone()
        tgt[::7] = -1
        out = torch.full((rows, 6, 2), 3.0, dtype=torch.float32, device=cuda)
        ops.score_categorical(logits, N_CLASS, tgt, key=key if (masked and keyed) else None,
                              out=out, **m, **kw)
        sc = out.cpu().numpy()
        pad = np.zeros(rows, dtype=bool)
        pad[::7] = True
        assert (sc[pad] == 3.0).all()
        assert np.array_equal(sc[~pad].view(np.int32), lp[~pad].view(np.int32)), form


def test_scorer_any_class(cuda):
    """Forced classes outside the kept set or the mask get -inf sampler log-probs; every class is checked in f64."""
    rows = 40
    logits = _random_logits(cuda, rows, 8)
    host = logits.cpu().numpy()
    rng = np.random.default_rng(9)
    toks = np.stack([rng.integers(0, c, rows) for c in N_CLASS], 1).astype(np.int64)
    sched, masks, bar, bits = _table(cuda, rows, 10)
    for settings in (DQN, (None, None)):
        for masked in (False, True):
            m = dict(bar=torch.as_tensor(bar).to(cuda), sched=torch.as_tensor(sched).to(cuda),
                     masks=torch.as_tensor(masks.view(np.int32)).to(cuda)) if masked else {}
            lp = ops.score_categorical(logits, N_CLASS, torch.as_tensor(toks).to(cuda), temperature=settings[0],
                                       top_p=settings[1], **m).cpu().numpy()
            allowed = _allowed(sched, bits, bar, np.arange(rows)) if masked else None
            _check_f64(host, toks, lp, settings, allowed)


# ---- 5-6. score_songs: batch invariance, blas against gemm, constraints ----------------------------------------------
def test_score_batch_invariance(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    songs = _songs([30, 7, 1, 55, 12, 2, 41, 19], seed=11)
    for sampler in ("dqn", "categorical"):
        full = generation.score_songs(net, w2e, songs, sampler=sampler)
        assert [x.shape for x in full] == [(len(s) - 1, 6, 2) for s in songs]
        alone = [generation.score_songs(net, w2e, [s], sampler=sampler)[0] for s in songs]
        assert _same(full, alone)
        perm = [5, 2, 7, 0, 3, 6, 1, 4]
        got = generation.score_songs(net, w2e, [songs[i] for i in perm], sampler=sampler)
        assert _same(got, [full[i] for i in perm])
        for rows in (64, 100):
            assert _same(generation.score_songs(net, w2e, songs, sampler=sampler, prefill_rows=rows), full)
        # the dataset-array form: padded to T with garbage past each song, mask marks the song
        T = max(len(s) for s in songs) + 3
        x = np.stack([np.concatenate([s, np.tile(s[:1], (T - len(s), 1))]) for s in songs])
        mask = np.stack([(np.arange(T) < len(s)).astype(np.float32) for s in songs])
        assert _same(generation.score_songs(net, w2e, x, sampler=sampler, mask=mask), full)
    assert full[2].shape == (0, 6, 2)
    blas = generation.score_songs(net, w2e, songs, kernel="blas")
    gemm = generation.score_songs(net, w2e, songs, kernel="gemm")
    for b, g in zip(blas, gemm):
        assert np.isfinite(b).all() and np.abs(b - g).max(initial=0) < 1e-4


def test_score_constraint_violations(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    songs = _songs([40, 25, 33], seed=12)
    for cons in (musical, [beats, None, musical]):
        got = generation.score_songs(net, w2e, songs, constraints=cons)
        free = generation.score_songs(net, w2e, songs)
        per = [cons] * 3 if isinstance(cons, generation.Constraint) else cons
        for s, g, f, c in zip(songs, got, free, per):
            assert np.abs(g[..., 0] - f[..., 0]).max() < 1e-6 and np.isfinite(g[..., 0]).all()
            if c is None:
                assert _same([g], [f])
                continue
            bars = generation.song_bar_counts(s, w2e)
            bad = np.array([[not c.allowed(b)[a][s[t + 1, a]] for a in range(6)] for t, b in enumerate(bars)])
            assert bad.any() and not bad.all()
            assert np.isneginf(g[..., 1][bad]).all()
            assert np.isfinite(g[..., 1][~bad]).all()
            assert sorted(set(np.nonzero(bad.any(1))[0])) == c.violations(s[1:], 1)


# ---- 7-8. generation with return_logprobs ----------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_batch_flag_keeps_songs(cuda, sampler):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    prompts = _songs([3, 17, 1, 9, 25], seed=13, max_bars=2)
    for kw in (dict(), dict(prompts=prompts, prefill="gemm"), dict(constraints=[musical, beats, None, beats, musical]),
               dict(prompts=prompts, constraints=musical)):
        torch.manual_seed(41)
        ref = generation.generate_batch(net, w2e, 5, bar_cond=5, max_tokens=150, sampler=sampler, chunk=32, **kw)
        torch.manual_seed(41)
        got, lps = generation.generate_batch(net, w2e, 5, bar_cond=5, max_tokens=150, sampler=sampler, chunk=32,
                                             return_logprobs=True, **kw)
        assert _same(got, ref)
        heads = kw.get("prompts", [generation.INIT_CW[0][None]] * 5)
        for s, lp, h in zip(got, lps, heads):
            assert lp.shape == (len(s) - len(h), 6, 2) and lp.dtype == np.float32
            assert np.isfinite(lp).all()


def _stream_cases(w2e):
    musical, beats = _constraints(w2e)
    prompts = _songs([3, 17, 1, 40, 9, 25, 2, 30, 12, 5], seed=14, max_bars=2)
    return [("scratch", dict(), dict()),
            ("prompts", dict(prompts=prompts, prefill="gemm"), dict(prompts=prompts, bank=4, prefill_rows=64)),
            ("constraints", dict(constraints=[musical, beats, None, musical, beats] * 2),
             dict(constraints=[musical, beats, None, musical, beats] * 2)),
            ("prompts+constraints", dict(prompts=prompts, prefill="gemm", constraints=beats),
             dict(prompts=prompts, constraints=beats))]


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_stream_logprobs_equal_batch(cuda, sampler):
    net = _small_model(cuda)
    w2e = _word2event()
    n = 10
    for name, bkw, skw in _stream_cases(w2e):
        torch.manual_seed(51)
        ref, ref_lp = generation.generate_batch(net, w2e, n, bar_cond=5, max_tokens=140, sampler=sampler, chunk=32,
                                                return_logprobs=True, **bkw)
        for slots in (1, 3, n + 5):
            torch.manual_seed(51)
            got, lp = generation.generate_stream(net, w2e, n, slots=slots, bar_cond=5, max_tokens=140,
                                                 sampler=sampler, chunk=16, return_logprobs=True, **skw)
            assert _same(got, ref), (name, slots)
            assert _same(lp, ref_lp), (name, slots)
            torch.manual_seed(51)
            plain = generation.generate_stream(net, w2e, n, slots=slots, bar_cond=5, max_tokens=140, sampler=sampler,
                                               chunk=16, **skw)
            assert _same(plain, got), (name, slots)


def test_stream_logprobs_shared_prompt(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    prompt = FIX["tokens"][:6]
    outs = []
    for slots in (1, 3, 15):
        torch.manual_seed(61)
        outs.append(generation.generate_stream(net, w2e, 10, slots=slots, bar_cond=4, max_tokens=120, prompt=prompt,
                                               chunk=16, return_logprobs=True))
    for s, lp in outs[1:]:
        assert _same(s, outs[0][0]) and _same(lp, outs[0][1])
    # song 0 starts from the same one-song prefill as a one-song batch
    torch.manual_seed(61)
    one, one_lp = generation.generate_batch(net, w2e, 1, bar_cond=4, max_tokens=120, prompts=prompt,
                                            return_logprobs=True)
    assert _same(one, outs[0][0][:1]) and _same(one_lp, outs[0][1][:1])


def test_stream_logprobs_graph_equals_eager(cuda, monkeypatch):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    prompts = _songs([3, 17, 1, 40, 9, 25, 2], seed=15, max_bars=2)
    runs = {}
    for graph in (True, False):
        if not graph:
            monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
        for name, kw in (("shared", dict()), ("prompts", dict(prompts=prompts, constraints=musical))):
            torch.manual_seed(71)
            (songs, lps), st = generation._generate_stream(net, w2e, 7, slots=3, bar_cond=4, max_tokens=90, chunk=8,
                                                           return_logprobs=True, **kw)
            assert st["graph"] == graph
            runs[graph, name] = songs, lps
    for name in ("shared", "prompts"):
        assert _same(runs[True, name][0], runs[False, name][0]) and _same(runs[True, name][1], runs[False, name][1])
    torch.manual_seed(71)
    got, lp = generation.generate_batch(net, w2e, 7, bar_cond=4, max_tokens=90, chunk=8, prompts=prompts,
                                        prefill="gemm", constraints=musical, return_logprobs=True)
    assert _same(got, runs[False, "prompts"][0]) and _same(lp, runs[False, "prompts"][1])


# ---- 9. generated against scored -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,constrained", [("categorical", False), ("categorical", True), ("dqn", False),
                                                 ("dqn", True)])
def test_generated_equals_scored(cuda, sampler, constrained):
    net = _small_model(cuda)
    w2e = _word2event()
    musical, beats = _constraints(w2e)
    prompts = _songs([3, 17, 1, 40, 9, 25, 2, 30], seed=16, max_bars=2)
    cons = [musical, beats, None, musical] * 2 if constrained else None
    torch.manual_seed(81)
    songs, lps = generation.generate_batch(net, w2e, 8, bar_cond=6, max_tokens=200, prompts=prompts, prefill="gemm",
                                           sampler=sampler, constraints=cons, return_logprobs=True)
    scored = generation.score_songs(net, w2e, songs, sampler=sampler, constraints=cons)
    total = flipped = 0
    for k, (s, p, lp, sc) in enumerate(zip(songs, prompts, lps, scored)):
        part = sc[len(p) - 1:]
        assert part.shape == lp.shape
        assert np.abs(part[..., 0] - lp[..., 0]).max() < 1e-4, k
        d = np.abs(part[..., 1] - lp[..., 1])
        d[np.isneginf(part[..., 1]) & np.isneginf(lp[..., 1])] = 0
        total += d.size
        if sampler == "categorical":
            assert d.max() < 1e-4, k
            continue
        bad = np.argwhere(~(d < 1e-4))
        if len(bad) == 0:
            continue
        flipped += len(bad)
        n = len(s)
        memory = [[torch.zeros((1, 2, 64, 64), device=cuda), torch.zeros((1, 2, 64), device=cuda)] for _ in range(2)]
        with torch.no_grad():
            lg = net.prefill_hidden(torch.as_tensor(s[None]).to(cuda), memory, [n], kernel="gemm",
                                    logits="all")[0].cpu().numpy()
        bars = generation.song_bar_counts(s, w2e)
        for t, a in bad:
            row = len(p) - 1 + t
            al = None if cons is None or cons[k] is None else cons[k].allowed(bars[row])[a]
            assert DQN[1][a] is not None, (k, t, a)
            assert _near_boundary(lg[row, OFF[a]:OFF[a + 1]], DQN[0][a], DQN[1][a], al, tol=1e-4), (k, t, a)
    assert flipped <= 1e-3 * total


# ---- 10. refusals ----------------------------------------------------------------------------------------------------
def test_logprob_refusals(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    song = FIX["tokens"][:10]
    with pytest.raises(ValueError):
        generation.score_songs(net, w2e, [song], sampler="greedy")
    with pytest.raises(ValueError):
        generation.score_songs(net, w2e, [song], kernel="gemv")
    with pytest.raises(ValueError):
        generation.score_songs(net, w2e, [song, song[:0]])
    bad = song.copy()
    bad[4, 3] = N_CLASS[3]
    with pytest.raises(ValueError):
        generation.score_songs(net, w2e, [bad])
    with pytest.raises(ValueError):
        generation.score_songs(net, w2e, [song], mask=np.ones((1, 10)))
    net.train()
    with pytest.raises(RuntimeError):
        generation.score_songs(net, w2e, [song])
    net.eval()
    net.compute_dtype = torch.bfloat16
    with pytest.raises(RuntimeError):
        generation.score_songs(net, w2e, [song])
    net.compute_dtype = torch.float32
    with pytest.raises(ValueError):
        generation.inference_from_scratch(net, w2e, 3, max_tokens=20, return_logprobs=True)
    with pytest.raises(ValueError):
        generation.inference_from_prompt(net, w2e, song[:3], 3, max_tokens=20, return_logprobs=True)
    with pytest.raises(ValueError):
        generation.categorical_rollout(net, 5, return_logprobs=True)
    with pytest.raises(ValueError):
        generation.generate(net, w2e, 1, bar_cond=3, max_tokens=20, logprobs=True, stats_path=None, log=lambda *a: 0)


def test_generate_saves_logprobs(cuda, tmp_path):
    net = _small_model(cuda)
    w2e = _word2event()
    for kw in (dict(slots=3), dict(batch_size=2)):
        out = tmp_path / ("slots" if "slots" in kw else "batch")
        torch.manual_seed(91)
        generation.generate(net, w2e, 4, bar_cond=3, max_tokens=60, path_gendir=str(out), logprobs=True,
                            stats_path=str(out / "stats.json"), log=lambda *a: 0, **kw)
        for i in range(4):
            s, lp = np.load(out / ("get_%d.npy" % i)), np.load(out / ("get_%d_logp.npy" % i))
            assert lp.shape == (len(s) - 1, 6, 2) and np.isfinite(lp).all()
            sc = generation.score_songs(net, w2e, [s], sampler="dqn")[0]
            assert np.abs(sc[..., 0] - lp[..., 0]).max() < 1e-4

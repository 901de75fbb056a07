"""CPU: the float64 restatement of the sampler's log-probs (sampling.logprobs_f64) against a brute-force walk of the
reference's nucleus rule, the per-row bar counts of score_songs against generation's bar rule, the host-side refusals
of the log-prob flags, and the argument checks of the two new entry points (no launch: there is no GPU here)."""
import ctypes

import numpy as np
import pytest

import rlmg_amd  # noqa: F401
from rlmg_amd import generation
from rlmg_amd.sampling import logprobs_f64

N_CLASS = [56, 135, 18, 87, 18, 25]
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]


def _word2event():
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(KEYS, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    w2e["bar-beat"][9] = "Bar"
    return w2e


def _brute(logits, target, temperature, top_p, allowed):
    """The reference's sampler walked literally in float64: softmax with temperature over the allowed classes,
    probs / (sum + 1e-5), classes visited in descending probability (ties: larger index first, argsort()[::-1]),
    each visited class kept until the running mass exceeds top_p, then renormalised."""
    x = np.asarray(logits, dtype=np.float64)
    n = len(x)
    ok = np.ones(n, dtype=bool) if allowed is None else allowed
    v = x / temperature
    e = np.zeros(n)
    e[ok] = np.exp(v[ok] - v[ok].max())
    probs = e / e.sum()
    kept = [i for i in range(n) if ok[i]]
    if top_p is not None and top_p < 1:
        p2 = probs / (probs.sum() + 1e-5)
        walk = sorted(range(n), key=lambda i: (-p2[i], -i))
        kept, run = [], 0.0
        for i in walk:
            kept.append(i)
            run += p2[i]
            if run > top_p:
                break
        kept = [i for i in kept if ok[i]]
    lm = x[target] - np.log(np.exp(x - x.max()).sum()) - x.max()
    if target not in kept:
        return lm, -np.inf
    return lm, np.log(probs[target] / probs[kept].sum())


@pytest.mark.parametrize("seed", range(6))
def test_restatement_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        n = int(rng.integers(1, 140))
        x = rng.normal(0, 2.0, n)
        if rng.random() < 0.5:
            x = np.round(x)                                  # ties
        t = float(rng.choice([1.0, 1.2, 2.0, 5.0]))
        p = [None, 0.9, 0.99, 0.5, 0.3][int(rng.integers(0, 5))]
        allowed = None
        if rng.random() < 0.5:
            allowed = rng.random(n) < 0.6
            allowed[int(rng.integers(0, n))] = True
        for c in range(n):
            got = logprobs_f64(x, c, t, p, allowed)
            want = _brute(x, c, t, p, allowed)
            assert abs(got[0] - want[0]) < 1e-12
            assert (np.isneginf(got[1]) and np.isneginf(want[1])) or abs(got[1] - want[1]) < 1e-12, (c, got, want)
        if p is None and allowed is None:                   # q is the tempered softmax
            assert abs(np.logaddexp.reduce([logprobs_f64(x, c, t, p)[1] for c in range(n)])) < 1e-9


def test_restatement_kept_mass():
    """The kept set is the smallest head of the ranking whose mass passes top_p: dropping its last class leaves at most
    top_p, and the kept probabilities sum to one after renormalising."""
    rng = np.random.default_rng(7)
    for _ in range(50):
        x = np.round(rng.normal(0, 1.5, 40) * 2) / 2
        q = np.exp([logprobs_f64(x, c, 1.0, 0.8)[1] for c in range(40)])
        assert abs(q.sum() - 1) < 1e-9
        probs = np.exp(x - x.max())
        probs /= probs.sum()
        kept = q > 0
        assert probs[kept].sum() / (1 + 1e-5) > 0.8 or kept.all()
        assert probs[kept].sum() - probs[kept].min() <= 0.8 * (1 + 1e-5) + 1e-12


def test_song_bar_counts_follow_the_bar_rule():
    w2e = _word2event()
    rng = np.random.default_rng(3)
    for L in (1, 2, 3, 17, 60):
        song = np.stack([rng.integers(0, c, L) for c in N_CLASS], 1).astype(np.int64)
        song[:, 2] = rng.choice([0, 1, 4, 9], L)
        bars = generation.song_bar_counts(song, w2e)
        assert bars.shape == (L - 1,) and bars.dtype == np.int64
        for t in range(L - 1):
            # row t + 1 continues the prompt song[:t + 1]: the count generation starts that prompt's draws from
            _, bar0s, _ = generation._check_prompts([song[:t + 1]], 1, w2e, N_CLASS, 10 ** 6, None)
            assert bars[t] == bar0s[0]
        for b in range(1, int(bars.max(initial=1)) + 1):
            cut = generation.cut_prompt(song, w2e, b)
            assert (bars[:len(cut) - 1] <= b).all()         # cut_prompt's first b bars are drawn under counts <= b


def test_host_paths_refuse_logprobs():
    w2e = _word2event()
    with pytest.raises(ValueError):
        generation.inference_from_scratch(None, w2e, 3, return_logprobs=True)
    with pytest.raises(ValueError):
        generation.inference_from_prompt(None, w2e, np.zeros((2, 6), dtype=np.int64), 3, return_logprobs=True)
    with pytest.raises(ValueError):
        generation.categorical_rollout(None, 4, return_logprobs=True)
    with pytest.raises(ValueError):
        generation.generate(None, w2e, 2, logprobs=True, stats_path=None, log=lambda *a: 0)


def test_entry_points_refuse_bad_arguments():
    import __graft_entry__ as g
    g.build()
    from rlmg_amd import _lib
    lib = _lib.load()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    nc = (ctypes.c_int * 6)(*N_CLASS)
    W = sum(N_CLASS)
    words = -(-W // 32)

    def logp(logits=buf, n_class=nc, rows=4, ld=W, counter=buf, key=null, step=null, bar=null, sched=null,
             masks=null, mask_words=words, tokens=buf, out=buf, out_counter=buf, out_rows=2):
        return lib.cwlt_sample_categorical_logp(logits, n_class, None, None, 6, rows, ld, 0, counter, key, step, bar,
                                                sched, 2, masks, 3, mask_words, tokens, out, out_counter, out_rows,
                                                null)

    assert logp(out=null) == 1001                                   # no output
    assert logp(rows=(1 << 20) + 1) == 1001
    assert logp(out_rows=0) == 1001
    assert logp(out_counter=null) == 1001                           # a ring needs its counter
    assert logp(counter=null) == 1001                               # neither key nor counter
    assert logp(key=buf) == 1001                                    # key without step
    assert logp(bar=buf, sched=buf) == 1001                         # a partial mask table
    assert logp(bar=buf, sched=buf, masks=buf, mask_words=words - 1) == 1001
    assert logp(ld=W - 1) == 1001
    assert logp(n_class=(ctypes.c_int * 6)(56, 300, 18, 87, 18, 25), ld=W + 300) == 1001

    def score(logits=buf, rows=4, ld=W, targets=buf, key=null, bar=null, sched=null, masks=null, mask_words=words,
              out=buf):
        return lib.cwlt_score_categorical(logits, nc, None, None, 6, rows, ld, targets, key, bar, sched, 2, masks, 3,
                                          mask_words, out, null)

    assert score(targets=null) == 1001
    assert score(out=null) == 1001
    assert score(rows=(1 << 20) + 1) == 1001
    assert score(masks=buf) == 1001
    assert score(bar=buf, sched=buf, masks=buf, mask_words=words - 1) == 1001
    assert score(ld=W - 1) == 1001
    assert score(rows=0) == 1001

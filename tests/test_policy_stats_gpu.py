"""GPU: policy entropy and KL against a reference model (cwlt_policy_stats).

1. Every entry against the float64 restatement (sampling.policy_stats_f64): |dH| <= 1e-5 (1 + H), |dKL| <= 2e-5 + 1e-5
   sum_K q_j |l_j - l'_j|.  1e-5 is the tolerance of one sampler log-prob at this logit scale (tests/test_logprobs_gpu.py);
   H and KL are q-weighted sums of one or two of them.  An entry may miss only where the nucleus ratio of the logits or
   of the reference logits sits within 1e-5 of top_p (_near_boundary), at most 1 % of the entries.
2. The support is the sampler's, with no exemption: every class is scored by cwlt_score_categorical(_grammar) on the same
   rows; H(q) and KL(q || q') formed in float64 from the scorer's own f32 log-probs meet the same bounds on every entry,
   KL is +inf exactly where the scorer shows a kept class of q outside q''s kept set, NaN exactly where it keeps nothing.
3. Degenerate cases: the reference aliased to the logits, and the plain categorical distribution.
4. generation.policy_stats on the small fixture model against ops.policy_stats on hand-built rows, the recorded fixture
   logits, batch invariance, refusals.
Each case prints its worst ratio to each bound (pytest -s); measured on an MI355X: profiles/policy_stats_ratios.txt."""
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
from rlmg_amd.sampling import all_logprobs_f64, grammar_allowed_f64, policy_stats_f64  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
WIDE = [1, 2, 3, 4, 5, 64, 255, 256]                  # eight attributes, a full wave, a single class
ROWS = 96
FILL = 7.0
VARIANTS = ["unmasked", "masked", "grammar", "grammar+masked"]


def _settings(name, A):
    if name == "categorical":
        return None, None
    return ([generation.DQN_TEMPERATURE[a % 6] for a in range(A)], [generation.DQN_TOP_P[a % 6] for a in range(A)])


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _random_logits(cuda, rows, W, seed, ld_pad=5):
    g = torch.Generator().manual_seed(seed)
    lg = 2.5 * torch.randn(rows, W + ld_pad, generator=g)
    lg[:rows // 4, :W] = torch.round(lg[:rows // 4, :W])          # ties in the first quarter
    return lg.to(cuda)[:, :W]                                    # a row stride != W


def _reference_logits(cuda, logits, seed, ld_pad=9):
    """The logits plus {0, 0.3, 2.5} randn by thirds of the rows, with another row stride."""
    rows, W = logits.shape
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([0.0, 0.3, 2.5]).repeat_interleave(-(-rows // 3))[:rows, None]
    buf = torch.zeros(rows, W + ld_pad)
    buf[:, :W] = logits.cpu() + scale * torch.randn(rows, W, generator=g)
    return buf.to(cuda)[:, :W]


def _table(rows, seed, n_class):
    """The random constraint table of the log-prob test: 5 songs' schedules over 7 mask rows, one song without rows;
    row keys that include -1 and songs past the table."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(n_class)])
    W = -(-int(off[-1]) // 32)
    bits = rng.random((7, W * 32)) < 0.6
    for r in range(7):                                            # keep every attribute non-empty
        for a, c in enumerate(n_class):
            bits[r, off[a] + rng.integers(0, c)] = True
    masks = np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(7, W)
    sched = np.array([[0, 3], [3, 1], [4, 3], [0, 0], [2, 5]], dtype=np.int64)
    bar = rng.integers(0, 6, rows).astype(np.int64)
    key = rng.integers(-1, 7, rows).astype(np.int64)
    allowed = []
    for n, k in enumerate(key):
        al = [np.ones(c, dtype=bool) for c in n_class]
        if 0 <= k < len(sched) and sched[k, 1] > 0:
            r = sched[k, 0] + min(max(bar[n] - 1, 0), sched[k, 1] - 1)
            al = [bits[r, off[a]:off[a + 1]].copy() for a in range(len(n_class))]
        allowed.append(al)
    return sched, masks, bar, key, allowed


def _grammar_for(n_class):
    """A generation.Grammar over n_class -> (grammar, bar_attr): the fixture vocabulary's own, or for the wide list
    bar-beat = the 64-class attribute (0, Bar, Beat_0 .. Beat_61), the 4-class attribute metrical, the two widest note
    attributes; the rest carry no role."""
    if n_class == N_CLASS:
        w2e = {k: {i: "%s_%d" % (k, i) for i in range(c)} for k, c in zip(KEYS, n_class)}
        w2e["bar-beat"] = {0: 0, 1: "Bar", **{2 + k: "Beat_%d" % k for k in range(16)}}
        return generation.Grammar(w2e), 2
    w2e = {"a%d" % a: {i: "c%d" % i for i in range(c)} for a, c in enumerate(n_class)}
    w2e["a5"] = {0: 0, 1: "Bar", **{2 + k: "Beat_%d" % k for k in range(62)}}
    return generation.Grammar(w2e, bar_attr="a5", metrical=("a3",), note=("a6", "a7")), 5


class Case:
    """One (class list, settings, variant): the inputs on the device, the kernel's output and the allowed sets."""

    def __init__(self, cuda, n_class, setting, variant):
        self.n_class, self.A = n_class, len(n_class)
        self.off = np.concatenate([[0], np.cumsum(n_class)])
        W = int(self.off[-1])
        self.temps, self.tops = _settings(setting, self.A)
        self.logits = _random_logits(cuda, ROWS, W, 3)
        self.ref = _reference_logits(cuda, self.logits, 4)
        assert self.logits.stride(0) != W and self.ref.stride(0) not in (W, self.logits.stride(0))
        self.x, self.y = self.logits.cpu().numpy(), self.ref.cpu().numpy()
        rng = np.random.default_rng(5)
        masked, grammar = "masked" in variant.split("+"), variant.startswith("grammar")
        self.mask_kw, self.key, allowed = {}, None, [None] * ROWS
        self.bar_class = None
        if masked:
            sched, masks, bar, key, allowed = _table(ROWS, 6, n_class)
            self.key = torch.as_tensor(key).to(cuda)
            self.mask_kw = dict(bar=torch.as_tensor(bar).to(cuda), sched=torch.as_tensor(sched).to(cuda),
                                masks=torch.as_tensor(masks.view(np.int32)).to(cuda))
            self.bar_class = rng.integers(0, 2, ROWS).astype(np.int64)         # only the sign is read
        self.gram_kw = None
        if grammar:
            g, self.bar_attr = _grammar_for(n_class)
            nb = n_class[self.bar_attr]
            order, gram = g.tables()
            order[nb - 1] = -3                                        # a class the grammar never allows
            self.beat = rng.integers(-1, nb - 2, ROWS).astype(np.int64)
            self.bar_class = rng.integers(0, nb, ROWS).astype(np.int64)
            self.bar_class[5::11] = nb - 1                            # rows of the never-allowed class: no allowed set
            self.gram_kw = (torch.as_tensor(self.beat).to(cuda), torch.as_tensor(order).to(cuda),
                            torch.as_tensor(np.ascontiguousarray(gram).view(np.int32)).to(cuda), self.bar_attr)
            sets = [g.allowed(kind) for kind in (0, 1, 2)]
            allowed = [grammar_allowed_f64(self.bar_class[n], self.beat[n], order, sets, self.bar_attr, allowed[n])
                       for n in range(ROWS)]
        if self.bar_class is not None:
            self.bar_class[::7] = -1                                  # padding rows
        self.pad = np.zeros(ROWS, dtype=bool) if self.bar_class is None else self.bar_class < 0
        self.allowed = allowed
        self.d_bar_class = None if self.bar_class is None else torch.as_tensor(self.bar_class).to(cuda)
        out = torch.full((ROWS, self.A, 4), FILL, dtype=torch.float32, device=cuda)
        got = self.run(self.ref, out)
        assert got is out
        self.got = out.cpu().numpy()

    def run(self, ref, out=None):
        return ops.policy_stats(self.logits, self.n_class, ref, temperature=self.temps, top_p=self.tops, key=self.key,
                                bar_class=self.d_bar_class, grammar=self.gram_kw, out=out, **self.mask_kw)

    def setting(self, a):
        return (1.0 if self.temps is None else self.temps[a]), (None if self.tops is None else self.tops[a])

    def seg(self, z, n, a):
        return z[n, self.off[a]:self.off[a + 1]]

    def al(self, n, a):
        return None if self.allowed[n] is None else self.allowed[n][a]


_CASES = {}


def _case(cuda, classes, setting, variant):
    k = (classes, setting, variant)
    if k not in _CASES:
        _CASES[k] = Case(cuda, N_CLASS if classes == "fixture" else WIDE, setting, variant)
    return _CASES[k]


ALL = [(c, s, v) for c in ("fixture", "wide") for s in ("dqn", "categorical") for v in VARIANTS]
IDS = ["-".join(k) for k in ALL]


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


def _h_and_kl(l, r):
    """From log-probs l of a distribution and r of the reference (float64, -inf outside the kept sets) -> H, KL, and
    the sum of q |l - r| that scales the KL bound (inf with the KL)."""
    k = np.isfinite(l)
    q = np.exp(l[k])
    h = -(q * l[k]).sum()
    if np.isinf(r[k]).any():
        return h, np.inf, np.inf
    return h, (q * (l[k] - r[k])).sum(), (q * np.abs(l[k] - r[k])).sum()


def _miss(got, want, bound):
    """|got - want| / bound; 0 where both are +inf; inf where only one is, or one is NaN."""
    if np.isposinf(got) and np.isposinf(want):
        return 0.0
    if not (np.isfinite(got) and np.isfinite(want)):
        return np.inf
    return abs(got - want) / bound


# ---- 1. against float64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes,setting,variant", ALL, ids=IDS)
def test_against_f64(cuda, classes, setting, variant):
    c = _case(cuda, classes, setting, variant)
    got = c.got
    assert (got[c.pad] == FILL).all()                                 # padding rows keep their fill value
    worst = {"H(p)": 0.0, "H(q)": 0.0, "KL(p)": 0.0, "KL(q)": 0.0}
    entries = exempt = empty = inf = fin = 0
    for n in np.nonzero(~c.pad)[0]:
        for a in range(c.A):
            x, y, al = c.seg(c.x, n, a), c.seg(c.y, n, a), c.al(n, a)
            t, p = c.setting(a)
            want = policy_stats_f64(x, y, t, p, al)
            g = got[n, a].astype(np.float64)
            assert np.isfinite(g[0]) and np.isfinite(g[2]), (n, a, g)     # the model columns are always finite
            lp, lq = all_logprobs_f64(x, t, p, al)
            rp, rq = all_logprobs_f64(y, t, p, al)
            entries += 1
            miss = {"H(p)": _miss(g[0], want[0], 1e-5 * (1 + want[0])),
                    "KL(p)": _miss(g[2], want[2], 2e-5 + 1e-5 * _h_and_kl(lp, rp)[2])}
            if lq is None:                                            # no allowed class: NaN in the sampler columns only
                empty += 1
                assert np.isnan(g[1]) and np.isnan(g[3]) and np.isnan(want[1]) and np.isnan(want[3]), (n, a, g)
            else:
                scale = _h_and_kl(lq, rq)[2]
                miss["H(q)"] = _miss(g[1], want[1], 1e-5 * (1 + want[1]))
                miss["KL(q)"] = _miss(g[3], want[3], 2e-5 + 1e-5 * (scale if np.isfinite(scale) else 0.0))
                inf += np.isposinf(g[3])
                fin += np.isfinite(g[3])
            if max(miss.values()) > 1:
                assert miss["H(p)"] <= 1 and miss["KL(p)"] <= 1, (n, a, g, want)
                assert _near_boundary(x, t, p, al) or _near_boundary(y, t, p, al), (n, a, g, want, miss)
                exempt += 1
                continue
            for k, v in miss.items():
                worst[k] = max(worst[k], v)
    print("    %-36s %s  exempt %d of %d, empty %d, KL(q) inf %d finite %d"
          % ("-".join((classes, setting, variant)), "  ".join("%s %.3f" % kv for kv in worst.items()), exempt, entries,
             empty, inf, fin))
    assert exempt <= 0.01 * entries
    assert (empty > 0) == variant.startswith("grammar")
    if setting == "dqn":
        assert inf > 0 and fin > 0                                    # both outcomes of the sampler KL occur
    else:
        assert inf == 0                                               # masks and grammar do not depend on the model


# ---- 2. the support is the sampler's -----------------------------------------------------------------------------------
def _scorer_logprobs(c, logits):
    """The scorer's pairs for every class of every attribute -> (rows, A, max classes, 2) float32, -inf past an
    attribute's classes.  Under a grammar the kind of a row is that of its bar_class: the other attributes are scored
    with the bar-beat target held at bar_class, the bar-beat attribute itself in a call of its own."""
    top = max(c.n_class)
    out = np.full((ROWS, c.A, top, 2), -np.inf, dtype=np.float32)
    dev = logits.device
    kw = dict(temperature=c.temps, top_p=c.tops, key=c.key, **c.mask_kw)
    pad = torch.as_tensor(c.pad).to(dev)
    for cls in range(top):
        tgt = torch.full((ROWS, c.A), cls, dtype=torch.int64, device=dev)
        tgt[pad] = -1
        if c.gram_kw is None:
            lp = ops.score_categorical(logits, c.n_class, tgt, **kw).cpu().numpy()
        else:
            beat, order, gram, ba = c.gram_kw
            own = ops.score_categorical_grammar(logits, c.n_class, tgt, beat, order, gram, ba, **kw).cpu().numpy()
            tgt[:, ba] = c.d_bar_class
            lp = ops.score_categorical_grammar(logits, c.n_class, tgt, beat, order, gram, ba, **kw).cpu().numpy()
            lp[:, ba] = own[:, ba]
        for a, nc in enumerate(c.n_class):
            if cls < nc:
                out[:, a, cls] = lp[:, a]
    return out


@pytest.mark.parametrize("classes,setting,variant", ALL, ids=IDS)
def test_support_is_the_samplers(cuda, classes, setting, variant):
    c = _case(cuda, classes, setting, variant)
    sx = _scorer_logprobs(c, c.logits).astype(np.float64)
    sy = _scorer_logprobs(c, c.ref).astype(np.float64)
    worst = {"H(p)": 0.0, "H(q)": 0.0, "KL(p)": 0.0, "KL(q)": 0.0}
    for n in np.nonzero(~c.pad)[0]:
        for a, nc in enumerate(c.n_class):
            g = c.got[n, a].astype(np.float64)
            hp, kp, sp = _h_and_kl(sx[n, a, :nc, 0], sy[n, a, :nc, 0])
            miss = {"H(p)": _miss(g[0], hp, 1e-5 * (1 + hp)), "KL(p)": _miss(g[2], kp, 2e-5 + 1e-5 * sp)}
            kept = np.isfinite(sx[n, a, :nc, 1])
            if not kept.any():                                        # NaN exactly where the scorer keeps nothing
                assert np.isnan(g[1]) and np.isnan(g[3]), (n, a, g)
            else:
                hq, kq, sq = _h_and_kl(sx[n, a, :nc, 1], sy[n, a, :nc, 1])
                outside = (kept & ~np.isfinite(sy[n, a, :nc, 1])).any()
                assert np.isposinf(g[3]) == outside and np.isposinf(kq) == outside, (n, a, g, kq)
                miss["H(q)"] = _miss(g[1], hq, 1e-5 * (1 + hq))
                miss["KL(q)"] = _miss(g[3], kq, 2e-5 + 1e-5 * (sq if np.isfinite(sq) else 0.0))
            assert max(miss.values()) <= 1, (n, a, g, miss)           # no exemption: the kept sets are the same sets
            for k, v in miss.items():
                worst[k] = max(worst[k], v)
    print("    %-36s scorer  %s" % ("-".join((classes, setting, variant)), "  ".join("%s %.3f" % kv for kv in worst.items())))


# ---- 3. degenerate cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes,setting,variant", ALL, ids=IDS)
def test_degenerate_cases(cuda, classes, setting, variant):
    c = _case(cuda, classes, setting, variant)
    same = c.run(c.logits).cpu().numpy()[~c.pad]                      # the reference aliased to the logits
    kl = same[..., 2:]
    empty = np.isnan(same[..., 1])
    assert (np.abs(kl[..., 0]) <= 2e-5).all() and (np.abs(kl[..., 1][~empty]) <= 2e-5).all()
    assert np.isnan(kl[..., 1][empty]).all()
    assert np.array_equal(same[..., :2], c.got[~c.pad][..., :2], equal_nan=True)
    alone = c.run(None).cpu().numpy()                                 # no reference: the two entropies, the same bits
    assert alone.shape == (ROWS, c.A, 2)
    assert np.array_equal(alone[~c.pad], c.got[~c.pad][..., :2], equal_nan=True)
    if setting == "categorical" and variant == "unmasked":
        assert np.abs(c.got[..., 1] - c.got[..., 0]).max() <= 1e-6    # q is p
        assert np.abs(c.got[..., 3] - c.got[..., 2]).max() <= 1e-6
    one = [a for a, nc in enumerate(c.n_class) if nc == 1]
    for a in one:                                                     # a single class: nothing to be uncertain about
        v = c.got[~c.pad][:, a]
        assert (np.nan_to_num(v, nan=0.0) == 0).all()


# ---- 4. generation.policy_stats on the small fixture model -------------------------------------------------------------
def _small_model(cuda, seed):
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": 2, "N_HEAD": 2})
    try:
        net = model.LinearTransformer(N_CLASS, is_training=False)
    finally:
        config.AgentConfig.update(old)
    return fill_params(net, seed=seed).to(cuda).eval()


@pytest.fixture(scope="module")
def nets(cuda):
    return _small_model(cuda, int(FIX["fill_seed"])), _small_model(cuda, int(FIX["fill_seed"]) + 1)


def _word2event():
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(KEYS, N_CLASS)}
    for k in KEYS:
        w2e[k][0] = 0
    w2e["tempo"][1] = w2e["chord"][1] = "CONTI"
    w2e["bar-beat"] = {0: 0, 1: "Bar", **{2 + k: "Beat_%d" % k for k in range(16)}}
    return w2e


def _songs(lengths, seed, max_bars=3):
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        p = np.stack([rng.integers(0, c, n) for c in N_CLASS], 1).astype(np.int64)
        bars = np.nonzero(p[1:, 2] == 1)[0] + 1
        p[bars[max_bars - 1:], 2] = 0
        out.append(p)
    return out


def _constraints(w2e):
    musical = generation.Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(5, 12)},
                                    per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7], ["chord_4"]]},
                                    cycle=True)
    beats = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar", "Beat_0", "Beat_4", "Beat_8", "Beat_12"],
                                                             ["Bar", "Beat_0", "Beat_6", 9]],
                                                "velocity": [[2], [3, 4], [5]]})
    return musical, beats


def _bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and
                                    np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _all_logits(net, song, cuda):
    enc = net.transformer_encoder
    H = enc.layers[0].attention.n_heads
    d = net.d_model // H
    memory = [[torch.zeros((1, H, d, d), device=cuda), torch.zeros((1, H, d), device=cuda)] for _ in enc.layers]
    with torch.no_grad():
        return net.prefill_hidden(torch.as_tensor(song[None]).to(cuda), memory, [len(song)], kernel="gemm",
                                  logits="all")[0]


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_generation_equals_hand_built_rows(cuda, nets, sampler):
    net, ref = nets
    w2e = _word2event()
    g = generation.Grammar(w2e)
    order, gram = g.tables()
    d_order = torch.as_tensor(order).to(cuda)
    d_gram = torch.as_tensor(np.ascontiguousarray(gram).view(np.int32)).to(cuda)
    songs = _songs([2, 17, 33, 64], seed=21)
    musical, beats = _constraints(w2e)
    cons = [musical, None, beats, musical]
    temps, tops = (generation.DQN_TEMPERATURE, generation.DQN_TOP_P) if sampler == "dqn" else (None, None)
    W = -(-sum(N_CLASS) // 32)
    for constrained in (False, True):
        for grammar in (False, True):
            kw = dict(sampler=sampler, constraints=cons if constrained else None, grammar=g if grammar else None)
            pair = generation.policy_stats(net, w2e, songs, reference=ref, **kw)
            alone = generation.policy_stats(net, w2e, songs, **kw)
            assert [x.shape for x in pair] == [(len(s) - 1, 6, 4) for s in songs]
            assert [x.shape for x in alone] == [(len(s) - 1, 6, 2) for s in songs]
            assert all(x.dtype == np.float32 for x in pair + alone)
            assert _bits(alone, [x[..., :2].copy() for x in pair])
            for s, c, got in zip(songs, cons, pair):
                L = len(s)
                lg, rl = _all_logits(net, s, cuda)[:L - 1], _all_logits(ref, s, cuda)[:L - 1]
                m = {}
                if constrained and c is not None:                     # one mask row per song row, keyed by the row
                    rows = np.zeros((L - 1, W * 32), dtype=bool)
                    for t, b in enumerate(generation.song_bar_counts(s, w2e)):
                        rows[t, :sum(N_CLASS)] = np.concatenate(c.allowed(int(b)))
                    masks = np.packbits(rows, axis=1, bitorder="little").view("<u4").reshape(L - 1, W).view(np.int32)
                    m = dict(key=torch.arange(L - 1, device=cuda), bar=torch.ones(L - 1, dtype=torch.int64, device=cuda),
                             sched=torch.as_tensor(np.stack([np.arange(L - 1), np.ones(L - 1, dtype=np.int64)], 1)).to(cuda),
                             masks=torch.as_tensor(masks).to(cuda))
                gt = None
                if grammar:
                    gt = (torch.as_tensor(g.beat_states(s)[0][1:].copy()).to(cuda), d_order, d_gram, 2)
                want = ops.policy_stats(lg, N_CLASS, rl, temperature=temps, top_p=tops,
                                        bar_class=torch.as_tensor(s[1:, 2].copy()).to(cuda), grammar=gt, **m)
                assert _bits([got], [want.cpu().numpy()]), (constrained, grammar, L)
                assert np.isfinite(got[..., 0]).all() and np.isfinite(got[..., 2]).all()
                # every bar-beat class of this vocabulary has a kind, and compile_grammar keeps each kind a class under
                # the constraints: no allowed set is empty, however ill-formed the random rows are
                assert not np.isnan(got).any()


def test_fixture_song_entropy(cuda, nets):
    net, ref = nets
    toks = FIX["tokens"]
    off = np.concatenate([[0], np.cumsum(N_CLASS)])
    got = generation.policy_stats(net, _word2event(), [toks], reference=ref)[0]
    assert got.shape == (len(toks) - 1, 6, 4)
    for t in range(len(toks) - 1):
        lg = FIX["logits"][t].astype(np.float64)
        for a in range(6):
            h = policy_stats_f64(lg[off[a]:off[a + 1]])[0]
            assert abs(got[t, a, 0] - h) <= 1e-4 * (1 + h), (t, a)
    assert np.abs(got[..., 1] - got[..., 0]).max() <= 1e-6            # categorical, unconstrained: q is p
    assert (got[..., 2] > 0).all() and np.isfinite(got).all()         # another model: a positive, finite KL
    same = generation.policy_stats(net, _word2event(), [toks], reference=net)[0]
    assert np.abs(same[..., 2:]).max() <= 2e-5


def test_batch_invariance(cuda, nets):
    net, ref = nets
    w2e = _word2event()
    songs = _songs([2, 17, 33, 64], seed=22)
    musical, beats = _constraints(w2e)
    kw = dict(reference=ref, sampler="dqn", constraints=[musical, beats, None, beats], grammar=generation.Grammar(w2e))
    full = generation.policy_stats(net, w2e, songs, **kw)
    perm = [2, 0, 3, 1]
    got = generation.policy_stats(net, w2e, [songs[i] for i in perm],
                                  **{**kw, "constraints": [kw["constraints"][i] for i in perm]})
    assert _bits(got, [full[i] for i in perm])
    for i, s in enumerate(songs):
        assert _bits(generation.policy_stats(net, w2e, [s], **{**kw, "constraints": kw["constraints"][i]}), [full[i]])
    assert _bits(generation.policy_stats(net, w2e, songs, prefill_rows=64, **kw), full)
    assert generation.policy_stats(net, w2e, [], **kw) == []


def test_refusals(cuda, nets):
    net, ref = nets
    w2e = _word2event()
    song = FIX["tokens"][:10]
    with pytest.raises(ValueError):
        generation.policy_stats(net, w2e, [song], sampler="greedy")
    with pytest.raises(ValueError):
        generation.policy_stats(net, w2e, [song], kernel="gemv")
    with pytest.raises(ValueError):
        generation.policy_stats(net, w2e, [song, song[:0]])
    net.train()
    try:
        with pytest.raises(RuntimeError):
            generation.policy_stats(net, w2e, [song])
    finally:
        net.eval()
    ref.train()
    try:
        with pytest.raises(RuntimeError):
            generation.policy_stats(net, w2e, [song], reference=ref)
    finally:
        ref.eval()
    ref.compute_dtype = torch.bfloat16
    try:
        with pytest.raises(RuntimeError):
            generation.policy_stats(net, w2e, [song], reference=ref)
    finally:
        ref.compute_dtype = torch.float32
    ref._recurrent = False
    try:
        with pytest.raises(RuntimeError):
            generation.policy_stats(net, w2e, [song], reference=ref)
    finally:
        ref._recurrent = True
    n_token = ref.n_token
    ref.n_token = list(N_CLASS[:-1]) + [N_CLASS[-1] + 1]
    try:
        with pytest.raises(ValueError):
            generation.policy_stats(net, w2e, [song], reference=ref)
    finally:
        ref.n_token = n_token
    assert generation.policy_stats(net, w2e, [song], reference=ref)[0].shape == (9, 6, 4)

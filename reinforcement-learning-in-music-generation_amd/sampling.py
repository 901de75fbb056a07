"""Host-side (numpy) token samplers used at generation time -- dqn_policy/model.py:19-55,
ppo_policy/model.py:28-64.  They consume `np.random` exactly as the reference does (one uniform double per draw,
in the reference's order of draws) and do its float32 arithmetic step for step, so a seeded run reproduces its
token stream bit for bit (tests/golden/dqn_generation_small.npz; tests/test_generation_cpu.py also checks them
against a line-by-line restatement on random logits).

They are on the critical path of host-sampled generation (one call per attribute per token), so the Python-level
loops of the reference are replaced by numpy calls with the SAME rounding:
  * `sum(x)` over a float32 array (sequential float32 adds)  ==  `np.cumsum(x)[-1]` (cumsum is sequential too);
  * `np.random.choice(a, size=1, p=p)`  ==  `a[searchsorted(cumsum(float64(p)) / total, random_sample(), 'right')]`,
    which is what RandomState.choice does after validating p; non-finite p goes to np.random.choice itself so
    that it raises what the reference raises.
"""
import numpy as np


def _seq_sum(x):
    """Python's sum() over a float32 vector: left-to-right float32 additions."""
    return x.cumsum()[-1]


def _choice(values, p):
    """np.random.choice(values, size=1, p=p)[0] without its argument validation (same draw, same result)."""
    cdf = p.astype(np.float64).cumsum()
    total = cdf[-1]
    if not abs(total - 1.0) <= 1e-4:                              # NaN / inf / not normalised (p >= 0: it is exp / sum)
        return np.random.choice(values, size=1, p=p)[0]          # let numpy raise / decide, as in the reference
    cdf /= total
    return values[cdf.searchsorted(np.random.random_sample(), side="right")]


def softmax_with_temperature(logits, temperature):
    e = np.exp(logits / temperature)
    return e / np.sum(e)


def weighted_sampling(probs):
    probs = probs / _seq_sum(probs)
    order = probs.argsort()[::-1]
    return _choice(order, probs[order])


def nucleus(probs, p):
    probs = probs / (_seq_sum(probs) + 1e-5)
    order = probs.argsort()[::-1]
    sorted_probs = probs[order]
    hit = (sorted_probs.cumsum() > p).nonzero()[0]
    cand = order[:hit[0] + 1] if hit.size else order
    cp = sorted_probs[:cand.size]
    cp = cp / _seq_sum(cp)
    return _choice(cand, cp)


def sampling(logit, p=None, t=1.0):
    if not isinstance(logit, np.ndarray):
        logit = logit.squeeze().detach().cpu().numpy()
    probs = softmax_with_temperature(logits=logit, temperature=t)
    if p is not None:
        return nucleus(probs, p=p)
    return weighted_sampling(probs)


def sample_cw(y):
    """Next CW token from the six logit vectors (tempo, chord, barbeat, pitch, duration, velocity) with the
    reference's per-attribute temperature / nucleus settings.  The DRAW order is tempo, barbeat, chord, pitch,
    duration, velocity (dqn_policy/model.py:281-286); the returned array is in attribute order (:289-296)."""
    tempo = sampling(y[0], t=1.2, p=0.9)
    barbeat = sampling(y[2], t=1.2)
    chord = sampling(y[1], p=0.99)
    pitch = sampling(y[3], p=0.9)
    duration = sampling(y[4], t=2, p=0.9)
    velocity = sampling(y[5], t=5)
    return np.array([tempo, chord, barbeat, pitch, duration, velocity])


def logprobs_f64(logits, target, temperature=1.0, top_p=None, allowed=None):
    """Float64 restatement of the device sampler's log-probs for one attribute: logits (n,), the class
    `target` -> (model log-prob, sampler log-prob).  The model log-prob is log_softmax(logits)[target].  The sampler's
    q: logits / temperature, classes outside `allowed` ((n,) bool, None = all) removed, then the nucleus kept set of
    `nucleus` above (top_p None or >= 1: every allowed class): classes ranked by probability (ties: the larger index
    first, as argsort()[::-1] orders them), a class kept when the mass ranked ahead of it is <= top_p in units of
    probs / (sum + 1e-5); renormalised over the kept classes.  -inf outside the kept set."""
    x = np.asarray(logits, dtype=np.float64)
    n = len(x)
    target = int(target)
    mx = x.max()
    lm = x[target] - mx - np.log(np.exp(x - mx).sum())
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    if not ok[target]:
        return lm, -np.inf
    v = x / float(temperature)
    m, e, keep = _kept_set_f64(v, ok, top_p)
    if not keep[target]:
        return lm, -np.inf
    return lm, (v[target] - m) - np.log(e[keep].sum())


def _kept_set_f64(v, ok, top_p):
    """The support of the sampler's q over tempered logits v with allowed classes ok (at least one) -> (m, e, keep): the
    allowed max, exp(v - m) on the allowed classes (0 elsewhere), the kept set of logprobs_f64's nucleus rule."""
    n = len(v)
    m = v[ok].max()
    e = np.where(ok, np.exp(np.where(ok, v, m) - m), 0.0)
    keep = ok.copy()
    if top_p is not None and top_p < 1.0:
        order = np.lexsort((-np.arange(n), -e))                  # probability descending, ties: larger index first
        ahead = np.empty(n)
        ahead[order] = np.concatenate([[0.0], np.cumsum(e[order])[:-1]])
        keep &= ahead / e.sum() / (1.0 + 1e-5) <= top_p
    return m, e, keep


def all_logprobs_f64(logits, temperature=1.0, top_p=None, allowed=None):
    """logprobs_f64 for every class at once: logits (n,) -> (model log-probs (n,), sampler log-probs (n,), -inf outside
    the kept set; None when `allowed` leaves no class)."""
    x = np.asarray(logits, dtype=np.float64)
    lm = (x - x.max()) - np.log(np.exp(x - x.max()).sum())
    ok = np.ones(len(x), dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    if not ok.any():
        return lm, None
    v = x / float(temperature)
    m, e, keep = _kept_set_f64(v, ok, top_p)
    return lm, np.where(keep, (v - m) - np.log(e[keep].sum()), -np.inf)


def policy_stats_f64(logits, ref_logits=None, temperature=1.0, top_p=None, allowed=None):
    """Float64 restatement of cwlt_policy_stats for one attribute: logits (n,) -> [H(p), H(q)], with
    ref_logits (n,) also [.., KL(p || p'), KL(q || q')], in nats.  p = softmax(logits), p' = softmax(ref_logits); q and q'
    the sampler's distributions of logprobs_f64 on each (temperature, `allowed`, the nucleus kept set, renormalised).
    Sums run term by term over the kept set, on log-probabilities formed from the logits.  KL(q || q') is +inf when q's
    kept set is not inside q''s; with no allowed class the q entries are NaN."""
    def dists(z):
        return all_logprobs_f64(z, temperature, top_p, allowed)

    def entropy(l):
        k = np.isfinite(l)
        return float(-(np.exp(l[k]) * l[k]).sum())

    def kl(l, r):
        k = np.isfinite(l)
        if np.isinf(r[k]).any():
            return np.inf
        return float((np.exp(l[k]) * (l[k] - r[k])).sum())

    lp, lq = dists(logits)
    out = [entropy(lp), np.nan if lq is None else entropy(lq)]
    if ref_logits is not None:
        rp, rq = dists(ref_logits)
        out += [kl(lp, rp), np.nan if lq is None else kl(lq, rq)]
    return np.array(out, dtype=np.float64)


def blend_logits_f64(logits, ref_logits, n_class, alpha):
    """Float64 restatement of cwlt_blend_logits: logits, ref_logits (rows, >= sum n_class) -> (rows, sum
    n_class) float64, attribute a's columns alpha[n, a] x + (1 - alpha[n, a]) r, the logits of pi^alpha pi_ref^(1 -
    alpha).  alpha: (1, A) (every row) or (rows, A), ALREADY rounded to f32 -- the alpha the kernel sees; 1 - alpha is
    then formed exactly here and rounded once in the kernel."""
    x = np.asarray(logits, dtype=np.float64)
    r = np.asarray(ref_logits, dtype=np.float64)
    al = np.asarray(alpha)
    if al.dtype != np.float32:
        raise TypeError("blend_logits_f64 takes alpha already rounded to float32, got %s" % al.dtype)
    A, W = len(n_class), int(sum(n_class))
    if x.ndim != 2 or r.ndim != 2 or len(r) != len(x) or x.shape[1] < W or r.shape[1] < W:
        raise ValueError("logits and ref_logits must be (rows, >= %d)" % W)
    if al.ndim != 2 or al.shape[1] != A or al.shape[0] not in (1, len(x)):
        raise ValueError("alpha must be (1, %d) or (%d, %d)" % (A, len(x), A))
    w = np.repeat(al.astype(np.float64), [int(n) for n in n_class], axis=1)         # (1 | rows, W): alpha per column
    return w * x[:, :W] + (1.0 - w) * r[:, :W]


def prefer_logits_f32(logits, n_class, bias_row=None, pen=None, seen=None):
    """Numpy float32 restatement of cwlt_prefer_logits for the rows of ONE song: logits (rows, >= sum
    n_class) or (sum n_class,) -> float32 of the same leading shape, ((x + b) - f s) - (s > 0 ? p : 0) with every
    operation rounded on its own, as the kernel rounds it: the result is bitwise the kernel's.  bias_row: (sum n_class,)
    or one row per row of logits, None: no b is added; pen: Preference.penalties(), (2 A + 1,) {frequency, presence,
    decay}; seen: the state per row, shaped like the result, None: no penalty.  Class 0 of every attribute is never
    penalised."""
    A, W = len(n_class), int(sum(n_class))
    x = np.asarray(logits, dtype=np.float32)[..., :W]
    out = x.copy()
    if bias_row is not None:
        out = out + np.asarray(bias_row, dtype=np.float32)[..., :W]
    if seen is None:
        return out
    pen = np.asarray(pen, dtype=np.float32).reshape(2 * A + 1)
    f = np.repeat(pen[:A], [int(n) for n in n_class])
    p = np.repeat(pen[A:2 * A], [int(n) for n in n_class])
    first = np.concatenate([[0], np.cumsum(n_class)[:-1]]).astype(np.int64)
    f[first], p[first] = 0.0, 0.0
    s = np.asarray(seen, dtype=np.float32)[..., :W]
    with np.errstate(over="ignore", invalid="ignore"):
        out = out - f * s
        out = out - np.where(s > 0, p, np.float32(0.0))
    return out.astype(np.float32, copy=False)


def grammar_allowed_f64(bar_class, beat, order, gram, bar_attr, allowed=None):
    """The allowed sets of one row under the row grammar -> list of (n,) bool arrays, one per attribute.
    order: per class of attribute bar_attr, -2 class 0 (a note row), -1 a Bar class, k >= 0 Beat_k, -3 never allowed;
    beat: the song's position before the row (-1 after a Bar row, k after Beat_k); gram[kind][a]: the (n,) bool classes
    a row of kind 0 NOTE / 1 BAR / 2 BEAT may carry in attribute a; allowed: the row's constraint sets (None = all).
    Attribute bar_attr gets the position rule (a Bar class always, Beat_k when k > beat, class 0 when beat >= 0); every
    other attribute gets the gram row of the kind of `bar_class`, the row's bar_attr class (no class at all when
    bar_class is outside the attribute or never allowed)."""
    o = np.asarray(order, dtype=np.int64)
    b = int(beat)
    c = int(bar_class)
    kind = None
    if 0 <= c < len(o) and o[c] != -3:
        kind = 0 if o[c] == -2 else 1 if o[c] == -1 else 2
    out = []
    for a in range(len(gram[0])):
        if a == bar_attr:
            ok = (o == -1) | ((o >= 0) & (o > b)) | ((o == -2) & (b >= 0))
        elif kind is None:
            ok = np.zeros(len(gram[0][a]), dtype=bool)
        else:
            ok = np.asarray(gram[kind][a], dtype=bool)
        out.append(ok.copy() if allowed is None else ok & np.asarray(allowed[a], dtype=bool))
    return out


def grammar_logprobs_f64(logits, target, beat, order, gram, bar_attr, temperature=None, top_p=None, allowed=None):
    """Float64 restatement of the grammar draw's log-probs for one row: logits (one (n,) vector per attribute), target
    (one class per attribute) -> (A, 2) float64, [a] = logprobs_f64 of attribute a under the distribution the device
    draws it from: bar_attr given the position `beat`, every other attribute given the kind of target[bar_attr]
    (grammar_allowed_f64).  The model column is unchanged by the grammar; an ill-formed target has -inf in the sampler
    column of the offending attribute."""
    sets = grammar_allowed_f64(target[bar_attr], beat, order, gram, bar_attr, allowed)
    A = len(sets)
    out = np.zeros((A, 2))
    for a in range(A):
        t = 1.0 if temperature is None else temperature[a]
        p = None if top_p is None else top_p[a]
        out[a] = logprobs_f64(logits[a], target[a], t, p, sets[a])
    return out


def particle_weigh_f32(lw, pairs, done=None):
    """Numpy float32 restatement of cwlt_particle_weigh's weight update for one token: lw (rows,) and the
    token's log-prob pairs (rows, A, 2) -> the new (rows,) float32 weights, bitwise the kernel's.  Per row the
    differences model - sampler are added in attribute order from 0, then the row's sum is added to lw, every
    operation rounded on its own.  done (rows,), optional: rows with done != 0 keep their weight."""
    lw = np.asarray(lw, dtype=np.float32)
    p = np.asarray(pairs, dtype=np.float32)
    s = np.zeros(lw.shape, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for a in range(p.shape[-2]):
            s = (s + (p[..., a, 0] - p[..., a, 1]).astype(np.float32)).astype(np.float32)
        out = (lw + s).astype(np.float32)
    return out if done is None else np.where(np.asarray(done) != 0, lw, out)


def reward_apply_f32(lw, r, any_live, beta):
    """Numpy float32 restatement of cwlt_reward_apply: lw, r (rows,), any_live (rows,) 0 / 1 -> (the new
    (rows,) float32 weights, the (rows,) float32 rewards recorded), both bitwise the kernel's.  A row with any_live != 0
    gets lw + (beta * r), the product rounded to float32 and then the sum, and records r; every other row keeps its
    weight and records 0 -- selected, not multiplied: r may be NaN or infinite there."""
    lw = np.asarray(lw, dtype=np.float32)
    r = np.asarray(r, dtype=np.float32)
    on = np.asarray(any_live) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        out = (lw + (np.float32(beta) * r).astype(np.float32)).astype(np.float32)
    return np.where(on, out, lw), np.where(on, r, np.float32(0))


def reward_apply_keyed_f32(lw, r, any_live, beta, key, particles):
    """Numpy float32 restatement of cwlt_reward_apply_keyed: reward_apply_f32 with the reward weight of
    the row's own song.  beta (n_beta,); key (rows,) particle ids, or None: the row indices; row n is of song
    s = key[n] // particles.  A row is on when any_live != 0, key >= 0 and s < n_beta: it gets lw + (beta[s] * r), the
    product rounded to float32 and then the sum, and records r.  Every other row keeps its weight and records 0 --
    selected: r may be NaN or infinite there, and no entry of beta is read for it.  Both outputs bitwise the kernel's."""
    lw = np.asarray(lw, dtype=np.float32)
    r = np.asarray(r, dtype=np.float32)
    table = np.asarray(beta, dtype=np.float32).reshape(-1)
    ids = np.arange(len(lw), dtype=np.int64) if key is None else np.asarray(key, dtype=np.int64).reshape(-1)
    song = np.where(ids >= 0, ids // int(particles), -1)
    on = (np.asarray(any_live) != 0) & (ids >= 0) & (song < len(table))
    b = table[np.where(on, song, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        out = (lw + (b * r).astype(np.float32)).astype(np.float32)
    return np.where(on, out, lw), np.where(on, r, np.float32(0))


def logmeanexp(x):
    """log(mean(exp(x))) of a vector in float64, by the max subtraction; -inf for all -inf."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return float(m) if not np.isfinite(m) else float(m + np.log(np.exp(x - m).mean()))


class Resampled:
    """What systematic_resample decides for one group: anc (K,) int64 in-group ancestors, ess, resampled (0 / 1), log_z
    (the evidence increment, 0.0 for a kept group), lw (K,) the weights after the event; and, for a comparison with
    float32 arithmetic, the scaled prefix sums `prefix` (K,), the thresholds (K,) they were searched with and s."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def systematic_resample(lw, u, ess_frac, done=None):
    """Float64 restatement of cwlt_particle_resample for ONE group: lw (K,) log-weights, u in [0, 1) ->
    Resampled.  m = max lw, e = exp(lw - m), s = sum e, ess = s^2 / sum e^2.  A group whose rows are all done, or with
    ess >= ess_frac * K, is kept: the identity, resampled 0, weights unchanged.  Otherwise ancestor j is the first row
    whose inclusive prefix sum of e exceeds (j + u) / K * s (the last row when none does), the increment of the log
    evidence is m + log(s / K) and every weight becomes 0."""
    x = np.asarray(lw, dtype=np.float64).reshape(-1)
    K = len(x)
    if K < 2:
        raise ValueError("a group has at least 2 particles, got %d" % K)
    if not 0.0 <= float(u) < 1.0:
        raise ValueError("u must lie in [0, 1), got %r" % (u,))
    m = x.max()
    e = np.exp(x - m) if np.isfinite(m) else np.zeros(K)
    prefix = np.cumsum(e)
    s = float(prefix[-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        ess = s * s / float((e * e).sum())
    thresholds = (np.arange(K) + float(u)) / K * s
    all_done = done is not None and bool(np.all(np.asarray(done) != 0))
    if all_done or not s > 0.0 or ess >= float(ess_frac) * K:
        return Resampled(anc=np.arange(K, dtype=np.int64), ess=ess, resampled=0, log_z=0.0, lw=x.copy(),
                         prefix=prefix, thresholds=thresholds, s=s)
    anc = np.minimum(np.searchsorted(prefix, thresholds, side="right"), K - 1).astype(np.int64)
    return Resampled(anc=anc, ess=ess, resampled=1, log_z=float(m + np.log(s / K)), lw=np.zeros(K), prefix=prefix,
                     thresholds=thresholds, s=s)


def _particle_release(song, done, particles, assigned, finished, limit, top):
    """The release's decision: songs are handed out below `limit`, and the counter of assigned songs stops at `top`."""
    song = np.asarray(song, dtype=np.int64).reshape(-1)
    K = int(particles)
    all_done = (np.asarray(done).reshape(len(song), K) != 0).all(1)
    cand = (song < 0) | all_done
    released = (song >= 0) & all_done
    idx = int(assigned) + np.cumsum(cand) - 1
    take = np.where(cand, np.where(idx < limit, idx, -1), -2).astype(np.int64)
    return take, released, min(int(assigned) + int(cand.sum()), top), int(finished) + int(released.sum())


def particle_release(song, done, particles, assigned, finished, n_songs):
    """Numpy restatement of cwlt_particle_release's decision.  song (groups,): each group's song, < 0
    none; done (groups * K,): the rows' end flags; assigned, finished: the counters before; n_songs: the run's songs.
    A group is a candidate when it has no song or all its K rows are done; a candidate with a song is finished.
    Candidate number r, in group order, takes song assigned + r while that is < n_songs, else none (-1).
    -> (take (groups,) int64: -2 for a group that is no candidate (nothing of it is written), else its new song or -1;
    released (groups,) bool: the finished groups, whose old song's outputs are written; assigned, finished after)."""
    return _particle_release(song, done, particles, assigned, finished, int(n_songs), int(n_songs))


def particle_release_bank(song, done, particles, assigned, finished, ready, n_songs):
    """Numpy restatement of cwlt_particle_release_bank's decision: particle_release under the gate of
    the bank.  ready: the songs whose bank entries are written (ctl[3]).  With limit = min(ready, n_songs), candidate
    number r takes song assigned + r only while that is < limit, else none (-1: parked, a candidate again at the next
    boundary); finished groups are released whether or not they take a song; assigned becomes
    min(assigned + candidates, max(limit, assigned)), so it never decreases.  -> particle_release's four values; with
    ready >= n_songs they are particle_release's."""
    limit = min(int(ready), int(n_songs))
    return _particle_release(song, done, particles, assigned, finished, limit, max(limit, int(assigned)))


def particle_event_keys(song, pos, every):
    """Numpy restatement of cwlt_particle_resample_keyed's bookkeeping: song (groups,) and the groups'
    clocks pos (groups,) -> (event (groups,) int64: the song's own event index pos // every - 1; skip (groups,) bool:
    groups the kernel leaves alone -- no song, or no whole segment yet).  Group g's u is cwlt_particle_resample's for
    (seed, event[g], song[g]) in place of (seed, the run's event, g)."""
    song = np.asarray(song, dtype=np.int64).reshape(-1)
    event = np.asarray(pos, dtype=np.int64).reshape(-1) // int(every) - 1
    return event, (song < 0) | (event < 0)


SONG_METRICS = 11


def _song_metrics(tok, mask, lengths, spec, weights, max_bars, exact):
    """song_metrics_f32 (exact False) and song_metrics_f64 (exact True): the walk and every integer are shared."""
    tok = np.asarray(tok, dtype=np.int64)
    N, L, _ = tok.shape
    MB = int(spec.max_bars if max_bars is None else max_bars)
    idx = np.arange(L, dtype=np.int64)
    live = np.ones((N, L), dtype=bool) if mask is None else np.asarray(mask).reshape(N, L) != 0
    if lengths is not None:
        live = live & (idx[None, :] < np.asarray(lengths, dtype=np.int64).reshape(N, 1))
    order, pitch = spec.order.astype(np.int64), spec.pitch.astype(np.int64)
    cb, cp = tok[:, :, spec.bar_attr], tok[:, :, spec.pitch_attr]
    inside = live & (cb >= 0) & (cb < len(order)) & (cp >= 0) & (cp < len(pitch))
    if spec.chord_attr >= 0:
        chord, cc = spec.chord.astype(np.int64), tok[:, :, spec.chord_attr]
        inside = inside & (cc >= 0) & (cc < len(chord))
    o = np.where(inside, order[np.where(inside, cb, 0)], -3)
    pit = np.where(inside, pitch[np.where(inside, cp, 0)], -1)
    ch = np.where(inside, chord[np.where(inside, cc, 0)], -1) if spec.chord_attr >= 0 else np.full((N, L), -1)

    def last_set(setter, value, start):
        # the value of the last setter at or before each row (Grammar.beat_states' max-scan), `start` without one
        last = np.maximum.accumulate(np.where(setter, idx[None, :], -1), axis=1)
        return np.where(last >= 0, np.take_along_axis(value, np.maximum(last, 0), axis=1), start)

    slot = np.cumsum(o == -1, axis=1)
    beat = last_set(o >= -1, o, -1)
    cur = last_set((o >= 0) & (ch >= 0), ch, 0)
    note = (o == -2) & (pit >= 0) & (pit < 128)
    head = (live & (slot == 0)).any(axis=1)
    keep = note & (slot < MB)

    ft = np.float64 if exact else np.float32
    T = None if exact else np.asarray(spec.xlog2x(L + 1), dtype=np.float32)

    def ent(c):
        # c (..., 12) integer counts -> the entropies in bits
        c = np.asarray(c, dtype=np.int64)
        n = c.sum(axis=-1)
        safe = np.maximum(n, 1)
        if exact:
            xl = lambda v: v * np.log2(np.maximum(v, 1).astype(np.float64))    # noqa: E731
            return np.where(n > 0, (xl(n) - xl(c).sum(axis=-1)) / safe, 0.0)
        s = np.zeros(n.shape, dtype=np.float32)
        for k in range(12):
            s = (s + T[c[..., k]]).astype(np.float32)
        return np.where(n > 0, ((T[n] - s).astype(np.float32) / safe.astype(np.float32)).astype(np.float32),
                        np.float32(0))

    def mean(values):
        if not len(values):
            return ft(0)
        total = values.sum() if exact else np.add.accumulate(values.astype(np.float32), dtype=np.float32)[-1]
        return ft(total / ft(len(values)))

    def ratio(a, b):
        return ft(ft(a) / ft(b)) if b else ft(0)

    feat = np.zeros((N, SONG_METRICS), dtype=ft)
    bars = np.zeros(N, dtype=np.int32)
    hist = np.zeros((N, MB, 12), dtype=np.int32)
    groove = np.zeros((N, MB), dtype=np.uint64)
    for n in range(N):
        k = np.nonzero(keep[n])[0]
        s_k, p_k, b_k, c_k = slot[n, k], pit[n, k], beat[n, k], cur[n, k]
        pc = p_k % 12
        np.add.at(hist[n], (s_k, pc), 1)
        on = (b_k >= 0) & (b_k < 64)
        np.bitwise_or.at(groove[n], s_k[on], np.uint64(1) << b_k[on].astype(np.uint64))
        c_bars = int(slot[n, -1])
        first = 0 if head[n] else 1
        B = c_bars + 1 - first
        hi = min(c_bars + 1, MB)
        Bk = max(hi - first, 0)
        bars[n] = B
        h = hist[n, first:hi].astype(np.int64)
        cnt = h.sum(axis=1)
        notes = int(cnt.sum())
        e1 = ent(h)
        feat[n, 0], feat[n, 1] = notes, B
        feat[n, 2] = mean(e1[cnt > 0])
        if Bk >= 4:
            h4 = h[:-3] + h[1:-2] + h[2:-1] + h[3:]
            feat[n, 3] = mean(ent(h4)[h4.sum(axis=1) > 0])
        feat[n, 4] = ent(h.sum(axis=0))
        P = Bk * (Bk - 1) // 2
        if P:
            bits = np.unpackbits(groove[n, first:hi].view(np.uint8).reshape(Bk, 8), axis=1).astype(np.int64)
            ones = bits.sum(axis=0)
            S = int((ones * (Bk - ones)).sum())
            feat[n, 5] = 1.0 - S / (P * spec.Q) if exact else np.float32(1) - ratio(S, P * spec.Q)
        under = c_k != 0
        feat[n, 6] = ratio(int((((c_k >> pc) & 1) != 0)[under].sum()), int(under.sum()))
        feat[n, 7] = int(p_k.max() - p_k.min()) if notes else 0
        feat[n, 8] = len(np.unique(p_k))
        feat[n, 9] = ratio(notes, Bk)
        feat[n, 10] = ratio(int((cnt == 0).sum()), Bk)
    reward = None
    if weights is not None:
        w = np.asarray(weights, dtype=ft).reshape(SONG_METRICS)
        reward = np.zeros(N, dtype=ft)
        with np.errstate(invalid="ignore", over="ignore"):
            for f in range(SONG_METRICS):
                reward = (reward + (w[f] * feat[:, f]).astype(ft)).astype(ft)
    return {"feat": feat, "reward": reward, "bars": bars, "hist": hist, "groove": groove.view(np.int64)}


def song_metrics_f32(tok, mask, lengths, spec, weights=None, max_bars=None):
    """Numpy float32 restatement of cwlt_song_metrics, bitwise what the kernel produces.  tok (N, L, A)
    int64; mask (N, L) or None (nonzero: live); lengths (N,) or None; spec a metrics.SongMetricSpec (its order, pitch and
    chord tables, its Q and its xlog2x table; max_bars: the spec's unless given).  -> a dict: feat (N, 11) float32 in
    metrics.METRICS' order, reward (N,) float32 (None without weights (11,)), bars (N,) int32, hist (N, max_bars, 12)
    int32 and groove (N, max_bars) int64, indexed by slot.
    The walk: a row that is not live is nothing; a live row with a class outside its table only counts as a live row;
    a Bar row opens the next slot and sets beat = -1; a Beat_k row sets beat = k and, unless its chord entry is -1, the
    chord mask; a class-0 row with a pitch is a note at (slot, beat, chord mask).  Slot 0 exists only when a live row
    precedes the first Bar row.  Every entropy is (T[n] - sum_k T[c_k]) / n with the float32 table T[c] = c log2 c, the
    sum taken from 0 in the order k = 0..11, each operation rounded on its own; means are sequential float32 sums in
    slot order divided once; the reward is r = r + (w[f] * feat[f]) for f = 0..10 from 0."""
    return _song_metrics(tok, mask, lengths, spec, weights, max_bars, False)


def song_metrics_f64(tok, mask, lengths, spec, weights=None, max_bars=None):
    """song_metrics_f32's definitions in float64: c log2 c evaluated in float64 (no table), exact divisions, float64
    sums.  The integers (bars, hist, groove, and the features that are counts) are the same arrays."""
    return _song_metrics(tok, mask, lengths, spec, weights, max_bars, True)

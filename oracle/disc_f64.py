"""f64 reference of the two Longformer discriminators WITH the kernels' dropout (TEST INFRASTRUCTURE; see
oracle/__init__.py).

Plain, device-agnostic torch (CPU, or f64 on the GPU), functions of a flat parameter dict keyed by the product modules'
own parameter names (dqn_policy/AIRL_model.LongFormer, ppo_policy/model.LongFormer), differentiable by autograd.  Every
dropout site is explicit (oracle/dropout.py: the kernels' keep flags and scale):

    band attention   P_ij = softmax_j of (q_i . k_j) / 8 over |i - j| <= w, key j unmasked -- in f64 throughout, its own
                     softmax (oracle/longformer.band_attention takes it in f32); masked query rows and rows with no
                     admissible key are zero; Pd_ij = keep(seed, p, ((b H + h) L + i) L + j) P_ij keep_scale(p)
    body             h = drop(LN(x + pos[2 : L + 2] + type[0]))                                       seeds[0]
    layer i          a = band attention of the three projections of h                                 seeds[1 + 3i]
                     h1 = LN(h + drop(dense(a)))                                                      seeds[2 + 3i]
                     h = LN(h1 + drop(dense(gelu(dense(h1)))))   exact-erf GELU, no dropout after it  seeds[3 + 3i]
    LayerNorm eps 1e-12.  The hidden sites index their (B * L, 512) tensor as row * 512 + col (csrc/ln.hip takes
    dropout_mask at off = row * D + column; cwlt_posenc_dropout is pinned element for element against
    oracle.dropout.site_mask by tests/test_bf16_regimes_gpu.py), which is oracle.dropout.dropout's convention.

`b0`: the global index of the first window, for a batch evaluated in slabs of windows (the attention mask is keyed by
the window, the hidden sites by the row b0 * L + ...).  `drop` (signature of oracle.dropout.dropout) and `keep`
(signature of oracle.dropout.keep_flags) are what the sites apply: tests hand in deliberately wrong ones.
"""
import math

import torch
import torch.nn.functional as F

from . import dropout

ATTRS = ("tempo", "chord", "barbeat", "pitch", "duration", "velocity")
LN_EPS = 1e-12
BN_EPS = 1e-5
BN_MOMENTUM = 0.1


def n_seeds(n_layer):
    return 1 + 3 * n_layer


def band_probs(q, k, mask, window):
    """The softmax of the admitted scores: q, k (B, L, H, D); mask (B, L) nonzero = attend, or None; window one-sided.
    -> P (B, H, L, L), zero outside the band, on masked keys and in the rows of masked queries; lse (B, H, L), the row
    log-sum-exp of the admitted scores, +inf where the row is forced to zero (masked query, no admissible key), which
    is the kernels' convention."""
    B, L, H, D = q.shape
    dev = q.device
    s = torch.einsum("blhd,bshd->bhls", q, k) / math.sqrt(D)
    idx = torch.arange(L, device=dev)
    allow = ((idx[:, None] - idx[None, :]).abs() <= window)[None, None].expand(B, H, L, L)
    qok = torch.ones(B, 1, L, dtype=torch.bool, device=dev)
    if mask is not None:
        valid = mask.reshape(B, L) != 0
        allow = allow & valid[:, None, None, :]
        qok = valid[:, None, :]
    live = allow.any(-1) & qok                                           # (B, H, L)
    zero = torch.zeros((), dtype=s.dtype, device=dev)
    sm = torch.where(allow, s, torch.full((), float("-inf"), dtype=s.dtype, device=dev))
    m = torch.where(live, sm.amax(-1), zero).detach()
    e = torch.where(allow, torch.exp(sm - m[..., None]), zero)
    l = e.sum(-1)
    lsafe = torch.where(live, l, torch.ones_like(l))
    pr = e / lsafe[..., None] * live[..., None].to(s.dtype)
    return pr, torch.where(live, m + torch.log(lsafe), torch.full_like(l, float("inf")))


def keep_factors(B, H, L, p, seed, b0=0, keep=dropout.keep_flags, device=None, dtype=torch.float64):
    """(B, H, L, L): keep_scale(p) where the attention-probability dropout keeps element ((b H + h) L + i) L + j of
    windows b0 .. b0 + B - 1, zero where it drops it."""
    idx = torch.arange(L, device=device)
    bh = (b0 + torch.arange(B, device=device))[:, None] * H + torch.arange(H, device=device)[None, :]
    eidx = ((bh[:, :, None] * L + idx[None, None, :])[..., None]) * L + idx
    return keep(seed, p, eidx).to(dtype) * dropout.keep_scale(p)


def band_attention(q, k, v, mask, window, p=0.0, seed=0, b0=0, keep=dropout.keep_flags):
    """q, k, v (B, L, H, D) f64 -> out (B, L, H * D), lse (B, H, L) (band_probs)."""
    B, L, H, D = q.shape
    pr, lse = band_probs(q, k, mask, window)
    if p > 0:
        pr = pr * keep_factors(B, H, L, p, seed, b0, keep, q.device, pr.dtype)
    return torch.einsum("bhls,bshd->blhd", pr, v).reshape(B, L, H * D), lse


def band_attention_row_terms(q, k, v, dout, mask, window, p=0.0, seed=0):
    """What the rows of dq and dk would measure if nothing in them cancelled.  With dp_ij = keep_ij (dO_i . v_j) and
    delta_i = sum_j P_ij dp_ij = dO_i . out_i the score gradient is dS_ij = P_ij (dp_ij - delta_i), a difference that
    vanishes identically for a row with one admissible key and nearly so for a row one key dominates, of two dot
    products that are sums of 64 terms of either sign themselves; dq_i = sum_j dS_ij k_j / 8, dk_j = sum_i dS_ij q_i / 8.
    Uncancelled: dpu_ij^2 = keep_ij^2 sum_d dO_id^2 v_jd^2, du_i^2 = sum_j P_ij^2 dpu_ij^2.
    -> (B, L, H) each: sqrt(sum_j P_ij^2 (dpu_ij^2 + du_i^2) |k_j|^2) / 8 and the same over i with |q_i|^2."""
    B, L, H, D = q.shape
    pr, _ = band_probs(q, k, mask, window)
    dpu2 = torch.einsum("blhd,bshd->bhls", dout.reshape(B, L, H, D).square(), v.square())
    if p > 0:
        dpu2 = dpu2 * keep_factors(B, H, L, p, seed, 0, dropout.keep_flags, q.device, pr.dtype).square()
    t = pr.square() * dpu2
    t = t + pr.square() * t.sum(-1, keepdim=True)
    uq = torch.einsum("bhls,bsh->blh", t, k.square().sum(-1)).sqrt() / math.sqrt(D)
    uk = torch.einsum("bhls,blh->bsh", t, q.square().sum(-1)).sqrt() / math.sqrt(D)
    return uq, uk


def body(P, x, mask, n_layer, n_head, window, ph=0.0, pa=0.0, seeds=None, b0=0, pre="longformer.",
         drop=dropout.dropout, keep=dropout.keep_flags, taps=None, attn_window=None, attn_mask=None):
    """The Longformer body: x (B, L, D) inputs_embeds -> last hidden state (B, L, D).  seeds: n_seeds(n_layer) of them in
    the order the model draws them (ignored where the site's p is 0).  taps: a list that receives, per layer, (input rows
    (B * L, D), q, k) with the gradients of q and k retained (row_terms).  attn_window / attn_mask: what the attention
    alone is given instead of window / mask (tests hand in wrong ones)."""
    B, L, D = x.shape
    seeds = [0] * n_seeds(n_layer) if seeds is None else seeds
    row0 = b0 * L
    g = lambda name: P[pre + name]                                       # noqa: E731

    def ln(t, name):
        return F.layer_norm(t, (D,), g(name + ".weight"), g(name + ".bias"), LN_EPS)

    h = x + g("embeddings.position_embeddings.weight")[2:2 + L] + g("embeddings.token_type_embeddings.weight")[0]
    h = drop(ln(h, "embeddings.LayerNorm").reshape(B * L, D), ph, seeds[0], row0)
    w_att = window if attn_window is None else attn_window
    m_att = mask if attn_mask is None else attn_mask
    for i in range(n_layer):
        lp = "encoder.layer.%d." % i
        sa, sb, sc = seeds[1 + 3 * i:4 + 3 * i]
        q, k, v = (F.linear(h, g(lp + "attention.self.%s.weight" % nm), g(lp + "attention.self.%s.bias" % nm))
                   .view(B, L, n_head, D // n_head) for nm in ("query", "key", "value"))
        if taps is not None:
            q.retain_grad()
            k.retain_grad()
            taps.append((h, q, k))
        a, _ = band_attention(q, k, v, m_att, w_att, pa, sa, b0, keep)
        o = F.linear(a.reshape(B * L, D), g(lp + "attention.output.dense.weight"), g(lp + "attention.output.dense.bias"))
        h1 = ln(h + drop(o, ph, sb, row0), lp + "attention.output.LayerNorm")
        it = F.gelu(F.linear(h1, g(lp + "intermediate.dense.weight"), g(lp + "intermediate.dense.bias")))
        y = F.linear(it, g(lp + "output.dense.weight"), g(lp + "output.dense.bias"))
        h = ln(h1 + drop(y, ph, sc, row0), lp + "output.LayerNorm")
    return h.view(B, L, D)


def row_terms(x2, t):
    """oracle/step_f64.row_terms: from a tap after the backward, (sum_r |dt_r|^2, sum_r |dt_r|^2 |x_r|^2): the squared
    norms a projection's bias and weight gradient would have if their rows added up without cancelling."""
    g2 = t.grad.reshape(x2.shape[0], -1).square().sum(1)
    return g2.sum().item(), (g2 * x2.detach().square().sum(1)).sum().item()


def embed_proj(P, data):
    """CW embedding x sqrt(d) of the six attributes, concatenated -> proj: (B, L, 6) int64 -> (B, L, D)."""
    embs = [P["word_emb_%s.lut.weight" % a][data[..., i]] * math.sqrt(P["word_emb_%s.lut.weight" % a].shape[1])
            for i, a in enumerate(ATTRS)]
    return F.linear(torch.cat(embs, -1), P["proj.weight"], P["proj.bias"])


def hidden(P, data, mask, n_layer, n_head, window, ph=0.0, pa=0.0, seeds=None, slab=None, **kw):
    """The last hidden state (B, L, D) of either model, `slab` windows at a time (the dense (B, H, L, L) scores of
    L = 1 024 are 67 MB a window)."""
    B = data.shape[0]
    slab = slab or B
    out = [body(P, embed_proj(P, data[s:s + slab]), None if mask is None else mask[s:s + slab], n_layer, n_head, window,
                ph, pa, seeds, b0=s, **kw) for s in range(0, B, slab)]
    return out[0] if len(out) == 1 else torch.cat(out)


def _same(t, n32, n16=0):
    return t


def score_classifier(P, m, stats, batch_stats, tap=None, jitter=None):
    """AIRL's score classifier on the window means m (B, D).  stats = (running_mean, running_var).  batch_stats:
    BatchNorm1d in train mode (this batch's biased variance normalises, the running statistics move by momentum 0.1 with
    the unbiased one); else on the running statistics.  -> (score (B, 1), (running_mean, running_var) afterwards).
    tap (batch_stats only): a list that receives (m, zn, sigma), zn the normalised first Linear's output with its gradient
    retained, sigma the batch's standard deviations (classifier_row_terms).
    jitter(t, n32, n16=0) -> t with the rounding errors of n32 f32 operations (and n16 bf16 roundings where the product
    keeps that stage in bf16): tests propagate the product's own roundings through the reference with it."""
    j = jitter or _same
    z = j(F.linear(m, P["score_classifier.0.weight"], P["score_classifier.0.bias"]), m.shape[-1] / 6 + 1)
    rm, rv = stats
    if batch_stats:
        n = z.shape[0]
        mu, var = j(z.mean(0), n / 6 + 1), j(z.var(0, unbiased=False), n / 6 + 3)
        zn = (z - mu) / torch.sqrt(var + BN_EPS)
        if tap is not None:
            zn.retain_grad()
            tap.append((m, zn, torch.sqrt(var + BN_EPS).detach()))
        stats = (j((1 - BN_MOMENTUM) * rm + BN_MOMENTUM * mu.detach(), 2),
                 j((1 - BN_MOMENTUM) * rv + BN_MOMENTUM * var.detach() * (n / max(n - 1, 1)), 3))
    else:
        zn = (z - rm) / torch.sqrt(rv + BN_EPS)
    y = j(torch.tanh(j(zn, 3) * P["score_classifier.1.weight"] + P["score_classifier.1.bias"]), 4)
    y = j(torch.tanh(j(F.linear(y, P["score_classifier.3.weight"], P["score_classifier.3.bias"]), 128 / 6 + 1)), 2)
    return j(torch.sigmoid(j(F.linear(y, P["score_classifier.5.weight"], P["score_classifier.5.bias"]), 64 / 6 + 1)),
             2), stats


def classifier_row_terms(m, zn, sigma, gamma):
    """What the gradients of the score classifier's first Linear and of its BatchNorm weight would measure without the
    cancellation inside the BatchNorm's backward, from a tap after the backward.  With g = d loss / d zn, the gradient
    w.r.t. the Linear's output is dz_b = (g_b - mean_b g - zn_b mean_b(g zn)) / sigma: a BCE against one label gives every
    window nearly the same g, so the first two terms cancel to a few per cent, and sum_b dz_b = 0 on top.  The BatchNorm
    weight's gradient is sum_b (g_b / gamma) zn_b with sum_b zn_b = 0.
    -> squared norms: (bias: sum u^2, weight: sum_b |u_b|^2 |m_b|^2, BatchNorm weight: sum (g zn / gamma)^2), where
    u^2 = (g^2 + (mean g)^2 + zn^2 (mean g zn)^2) / sigma^2."""
    g, z = zn.grad, zn.detach()
    u2 = (g.square() + g.mean(0).square() + z.square() * (g * z).mean(0).square()) / sigma.square()
    return (u2.sum().item(), (u2.sum(1) * m.detach().square().sum(1)).sum().item(),
            (g * z / gamma.detach()).square().sum().item())


def airl_forward(P, stats, data, mask, n_layer, n_head, window, batch_stats, ph=0.0, pa=0.0, seeds=None, ztap=None,
                 **kw):
    """dqn_policy/AIRL_model.LongFormer.forward -> (score (B, 1), running statistics afterwards, hidden (B, L, D))."""
    h = hidden(P, data, mask, n_layer, n_head, window, ph, pa, seeds, **kw)
    score, stats = score_classifier(P, h.mean(1), stats, batch_stats, ztap)
    return score, stats, h


def token_ce(P, h, target, jitter=None):
    """The six mean cross entropies of the proj_* heads on hidden rows h (B, L, D) against target (B, L, 6) -> (6,).
    jitter: as in score_classifier (logits in the compute dtype, the cross entropy and its mean in f32)."""
    j = jitter or _same
    out = []
    for i, a in enumerate(ATTRS):
        y = j(F.linear(h, P["proj_%s.weight" % a], P["proj_%s.bias" % a]), h.shape[-1] / 6 + 1, 2)
        nll = j(F.cross_entropy(y.reshape(-1, y.shape[-1]), target[..., i].reshape(-1), reduction="none"),
                y.shape[-1] / 6 + 3)
        out.append(j(nll.mean(), nll.numel() / 6 + 1))
    return torch.stack(out)


def bce(score, label, jitter=None):
    """nn.BCELoss of scores (B, 1) against the constant label."""
    j = jitter or _same
    e = j(F.binary_cross_entropy(score, torch.full_like(score, label), reduction="none"), 3)
    return j(e.mean(), e.numel() / 6 + 1)


def airl_token_forward(P, data, target, mask, n_layer, n_head, window, ph=0.0, pa=0.0, seeds=None, **kw):
    """AIRL_model.LongFormer.token_forward: the mean of the six CEs (compute_CEloss is the plain mean)."""
    return token_ce(P, hidden(P, data, mask, n_layer, n_head, window, ph, pa, seeds, **kw), target).mean()


def airl_losses(P, stats, h_exp, h_ce, h_ag, target, batch_stats=True, ztap=None, jitter=None, pool=None):
    """The three losses of one discriminator batch from the hidden rows of its three passes, in the product's order (expert
    score, token CE, agent score: the BatchNorm's running statistics move twice).  pool: the window mean (tests hand in a
    jittered one).  -> ((BCE(expert, 1), BCE(agent, 0), CE), running statistics afterwards)."""
    j = jitter or _same
    pool = pool or (lambda h: h.mean(1))
    s_exp, stats = score_classifier(P, pool(h_exp), stats, batch_stats, ztap, jitter)
    ce = j(token_ce(P, h_ce, target, jitter).mean(), 2)
    s_ag, stats = score_classifier(P, pool(h_ag), stats, batch_stats, ztap, jitter)
    return (bce(s_exp, 1.0, jitter), bce(s_ag, 0.0, jitter), ce), stats


def airl_train_loss(P, stats, x_exp, x_agent, mask, n_layer, n_head, window, ph=0.0, pa=0.0, seeds3=(None, None, None),
                    batch_stats=True, ztap=None, **kw):
    """One batch of dqn_policy/AIRL.py:113-128 in train mode: expert score, token CE of the agent windows against the
    expert windows, agent score -- three passes in that order, each with its own seeds (seeds3: three lists), the
    BatchNorm on batch statistics twice (batch_stats=False: on the running statistics, the mode the reference-recorded
    fixture was taken in).  -> ((BCE(expert, 1), BCE(agent, 0), CE), running statistics afterwards); the loss that is
    back-propagated is e + (a + c)."""
    hs = [hidden(P, d, mask, n_layer, n_head, window, ph, pa, sd, **kw)
          for d, sd in ((x_exp, seeds3[0]), (x_agent, seeds3[1]), (x_agent, seeds3[2]))]
    return airl_losses(P, stats, hs[0], hs[1], hs[2], x_exp, batch_stats, ztap)


def ppo_reward(P, h, jitter=None):
    """ppo_policy/model.LongFormer.token_forward from the hidden rows: the mean over the six attributes of
    sigmoid(eval_f(mean over the window of proj_f(h))) -> (B, 1).  jitter: as in score_classifier (the product takes the
    logits in its compute dtype, everything after them in f32)."""
    j = jitter or _same
    total = 0
    for a in ATTRS:
        y = j(F.linear(h, P["proj_%s.weight" % a], P["proj_%s.bias" % a]), h.shape[-1] / 6 + 1, 2)
        y = j(y.mean(1), y.shape[1] / 6 + 1)
        total = total + j(torch.sigmoid(j(F.linear(y, P["eval_%s.weight" % a], P["eval_%s.bias" % a]),
                                          y.shape[-1] / 6 + 1)), 2)
    return j(total / len(ATTRS), len(ATTRS) / 6 + 1)


def ppo_token_forward(P, data, mask, n_layer, n_head, window, ph=0.0, pa=0.0, seeds=None, **kw):
    """-> (reward (B, 1), hidden (B, L, D))."""
    h = hidden(P, data, mask, n_layer, n_head, window, ph, pa, seeds, **kw)
    return ppo_reward(P, h), h


def ppo_train_step(P, data, target, mask, n_layer, n_head, window, ph=0.0, pa=0.0, seeds=None, **kw):
    """ppo_policy/model.LongFormer.train_step: the six mean token CEs -> (6,)."""
    return token_ce(P, hidden(P, data, mask, n_layer, n_head, window, ph, pa, seeds, **kw), target)


def leaves(params, device=None, dtype=torch.float64):
    """name -> a detached `dtype` copy that requires grad."""
    return {k: v.detach().to(device=device or v.device, dtype=dtype).requires_grad_(True) for k, v in params.items()}

"""Loss heads (csrc/heads.hip) and RL arithmetic (csrc/rl.hip) in f64 (TEST INFRASTRUCTURE; see oracle/__init__.py): the
references, input makers, measures and error bounds of tests/test_heads_f64_gpu.py and tests/test_rl_f64_gpu.py, pinned by
tests/test_oracle_heads_rl_f64_cpu.py.  Plain torch, any device, none of the project's kernels.

Heads.  logits (rows, ld), attribute f in columns [off_f, off_f + n_f), off_f = sum_{g<f} n_g; columns >= sum n are padding.
    mx = max_j x_j;  e_j = exp(x_j - mx);  s = sum_j e_j;  p_j = e_j / s;  nll = (log s + mx) - x_t,  t = clamp(target, 0, n - 1)
    loss_sum_f = sum_r mask_r nll_rf;  argmax = FIRST index of the largest p_j;  pmax = p at argmax
    cwlt_heads_ce_bwd:   dlogits_j = (p_j - [j == t]) * (mask_r * coef_f), padding columns 0
    cwlt_heads_logp_bwd: dlogits_j = ([j == t] - p_j) * g_rf,             padding columns 0
The reference starts from the exact input values (the bf16 values of bf16 logits) in f64.

gamma is a `float` in the C ABI: the references use its f32 value (f32v), as rl_math's own f32 expressions do.

RL.  oracle/rl_math.py stays the literal restatement (six attributes, lists of tensors).  rollout_gather, ppo_returns_adv,
ppo_policy_loss and dqn_td below are the same formulas in f64 on the fused layouts the kernels take, for any R, T, NA, E, B,
attribute count and class counts; the CPU test asserts they equal rl_math where rl_math is defined.

Bounds.  u = 2^-24 per f32 operation, U = 2^-9 / sqrt(3) rms per bf16 rounding, errors independent, a serial sum of n terms
counts n / 6 (relative to the sum of |terms|), a level of a reduction tree counts 1, the bound 4 x the predicted rms.  Operation
counts, read off the source:

  softmax sum (both families).  d_j = |x_j - mx|.  e_j carries the rounding of its argument (f32: the subtraction, bf16: the
      product with log2(e) inside __expf; the difference of two bf16 values is exact), a relative error u d_j, and the
      exponential itself: expf at 2 ulp (n_exp = 4), the hardware exp2 of __expf at 1 ulp (n_exp = 1).  The sum s then has the
      relative variance  S = sum_j p_j^2 (n_exp + d_j^2) + n_sum  [+ (c sum_j p_j d_j)^2 for __expf], where
      n_sum = n / 3 for the tiled kernels (row_sumexp adds serially; see below) and (slots - 1) + ceil(log2 min(n, 64)) for
      the wave-per-row kernels (a lane adds its <= 4 slots, then a butterfly; adding an exact zero does not round).
      n / 3, not the n / 6 of a sum whose partial sums grow with the terms (CORRECTED after the second GPU run: with n / 6
      the tiled bf16 pmax of 32 801 x 6 pairs of randn x 3 sat at 1.08, f32 at 0.84).  The partial sums of a softmax row do
      not grow evenly: once the largest class is in, every later partial sum is about s, and each of the remaining
      roundings is uniform within half an ulp of s: variance u^2 s^2 / 3 each, n u^2 s^2 / 3 at most for the row.
      Equal values (CORRECTED after the first GPU run: bf16 randn + 300 takes five values, 296 .. 304; the tiled bf16 pmax
      of (9, 8, 7, 1, 65, 64, 63) sat at 1.15 of the bound written for independent errors).  The m_l classes of a row that
      hold the same value (a "level" l) have the same e_j, hence the same errors: they add to the sum as P_l = m_l p_l, and
      S takes sum_l P_l^2 (n_exp + d_l^2) in place of the sum over j.  And a serial sum that adds the same addend again
      and again rounds the same way each time while the partial sum stays in one binade (the partial is a multiple of its
      ulp, the addend's remainder modulo that ulp is fixed): the m_l roundings of a level add linearly, so the tiled
      n_sum is sum_l m_l^2 / 3, which is n / 3 when all values differ.  The wave-per-row count is already one whole
      rounding per step of its 4 + 6 deep tree.  The kernel is right: a serial f32 sum is what it is meant to be.
  __expf (bf16 families, sm_exp).  __expf(y) = exp2(y * log2e_f32).  The product rounds once (relative u of the argument,
      so relative u d_j of e_j, counted above) and the f32 constant differs from log2(e) by c u, c = |log2e_f32 / log2(e)
      - 1| / u = 0.225: the same sign for every class, so it does not average: e_j is off by the factor exp(-c u d_j) and
      s by -c u sum_j p_j d_j <= c u log n relative, which enters S squared (LOG2E_C).
  nll.  log s: dS absolute from s and logf at 2 ulp of |log s|; (log s + mx) one rounding of at most |log s| + |mx|; - x_t one
      rounding of |nll| <= |mx| + |x_t| + |log s| = scale; the product with the mask one more:
      var(nll_r) = u^2 (S_r + 7 scale_r^2).
  loss sums.  measured relative to D_f = sum_r mask_r scale_rf:  the rows' errors add in quadrature,
      u^2 sum_r mask_r^2 (S_r + 7 scale_r^2) / D^2, plus the partial-sum tree relative to sum_r mask_r |nll_r| <= D:
      tiled  trips / 6 (a thread's acc over its tiles) + 32 / 6 (the 32 rows of red[slot]) + finalize
      wave   trips / 6 (a wave's acc over its rows) + 2 (the four waves, two levels) + finalize
      finalize (colsum_finalize_kernel over nb blocks, 16 waves x 16 chains): ceil(nb / 256) / 6 + 4 + 16 / 6.
      ops.heads_ce divides by sum(mask) (exact for 0/1 masks): + 1.
  probs, pmax.  p_j = e_j / s: relative variance n_exp + d_j^2 + S + 1 (the division).  Per row the measure is
      max_j |got_j - p_j| / pmax_row, and p_j / pmax = exp(-d_j), d^2 exp(-2d) <= exp(-2) = 0.135:
      bound = 4 u sqrt(n_exp + 1.135 + S) of pmax_row (pmax itself: the same, d = 0).
  dlogits.  p_j = e_j * (1 / s) (two roundings), minus the one-hot (one, of at most 1), times w (one) and w = mask * coef
      (one; coef = gloss / sum(mask) in ops.heads_ce one more; none for logp_bwd whose w is given):
      per row max_j |got_j - ref_j| / |w_r| <= 4 sqrt((n_exp + 5.135 + n_w + S) u^2 [+ U^2 for bf16 dlogits]).
      A row whose w is 0 must be exactly 0, padding columns must be exactly 0.
  argmax.  exact, except (row, attribute) pairs whose two largest softmax values differ by a relative gap in (0, 1e-5):
      those are skipped (GAP), their share asserted <= 0.1 % (SKIP_SHARE).  Exact ties are not skipped.

  rollout_gather.  action is a copy: exact.  logp = logf(probs[...]) of the given f32 probs: 2 ulp, 4 * 2 u |log p|.
  ppo_returns_adv.  R_t = r_t + gamma R_{t-1} (two roundings unless contracted): e_t = gamma e_{t-1} + delta_t,
      var(e_t) = V_t u^2, V_t = gamma^2 V_{t-1} + 2 R_t^2: grows with t, so with E.  normalize = 0: returns 4 u sqrt(V),
      adv = returns - values one more rounding.  A normalisation y = (x - mean) / sd of values with rms errors a_i:
          mean: the lane sums ceil(E / 64) values, a butterfly and a division: var = max a^2 + u^2 (m / 6 + 7) mean|x|^2
                (the a_i of a recursion are correlated: their mean is counted at their largest)
          sd:   d sd / sd <= sqrt(sum D_i^2) / sqrt(sum (x_i - mean)^2) (Cauchy-Schwarz), D_i^2 = a_i^2 + var(mean)
                + u^2 (x_i - mean)^2, plus squares, sum, division, root: u^2 (m / 6 + 11)
          y_i:  var = (a_i^2 + var(mean) + u^2 (x_i - mean)^2) / sd^2 + y_i^2 (var(sd) / sd^2 + u^2)
      applied twice (returns, then advantages = y - values with one more rounding of |adv|).
  ppo_policy_loss.  ratio = expf(new - old): relative variance 4 + d^2, d = |new - old|; times A_e one more; the clip edges are
      f32(1 -+ f32(clip)) in the kernel and 1 -+ clip here (as rl_math has them): one more, 6 + d^2.  Per thread a serial
      sum of E * ceil(KF / 256) terms, an 8-level tree, * 1 / (E KF) (two roundings):
          loss  4 u sqrt((6 + max d^2) (rss / sum)^2 + E trips / 6 + 10) * sum |terms| / (E KF)
          grad  per element kf: 4 u sqrt((6 + max d^2) + E / 6 + 2 [+ 1 through autograd]) * sum_e |A_e ratio| / (E KF), the sum over
                the e that pass the clip test; an element whose ratio is within EDGE = 16 u (1 + d) of a clip edge may fall on
                either side: |A_e ratio| / (E KF) of it is added to the bound.  l2 < l1 is A_e < 0 for any clip < 0.8: no edge.
  dqn_td.  next-state maxima and their order are exact (comparisons).  target = reward + (gamma (1 - done)) top: 4 roundings of at
      most |reward| + gamma |top|; d = q - target one of |d|: var(d) = 5 u^2 s^2, s = |q| + |reward| + gamma |top|.
          dq    d * (2 / (B NA A)): 4 more roundings:  4 u sqrt(9) s gscale
          mse_f sum_jk d^2 / (B NA): each d^2 errs by 2 |d| sqrt(5) u s (+ u d^2 for the square); the lane sum of ceil(NA / 64),
                a butterfly, torch's sum over B (counted B / 6) and the division:
                4 u sqrt(sum (2 d sqrt(5) s)^2 + (m / 6 + 9 + B / 6) (sum d^2)^2) / (B NA)
          dy    dq * (g_f A) (two roundings) scattered by serial adds over the duplicates of an action:
                4 u sqrt(11 + dup / 6) * sum |contributions| (with s in place of |d|); untouched elements exactly 0.
Measured on an MI355X: profiles/heads_rl_f64_ratios.txt.
"""
import math

import torch

U16 = 2.0 ** -9 / 3 ** 0.5
U32 = 2.0 ** -24
TEETH = 5.0
GAP = 1e-5
SKIP_SHARE = 1e-3
LOG2E_C = abs(float(torch.tensor(math.log2(math.e), dtype=torch.float32)) / math.log2(math.e) - 1) / U32
EDGE = 16 * U32

REPO = (56, 135, 18, 87, 18, 25)
PPO = (49, 19, 19, 89, 67, 25)
KINDS = ("x3", "peaked", "shifted", "ties")


def f32v(x):
    """The f32 value of a scalar argument (gamma is a `float` in the C ABI: the kernels never see the double)."""
    return float(torch.tensor(x, dtype=torch.float32))


def offsets(n_class):
    off = [0]
    for n in n_class:
        off.append(off[-1] + n)
    return off


def heads_blocks(rows):
    return max(1, min(1024, (rows + 3) // 4))


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def make_logits(kind, rows, n_class, ld, dtype=torch.float32, seed=1, pad=float("nan")):
    """(rows, ld) logits of `dtype`, padding columns = `pad`.
    x3       randn x 3
    peaked   randn with one class per (row, attribute) at +50
    shifted  randn + 300 (the max subtraction is needed: exp(300) overflows f32)
    ties     randn x 3 with exact ties of the maximum, by row % 4:  0 a block of up to 3 equal maxima inside one group of 8,
             1 classes 7 and 8 (across a group-of-8 boundary; n >= 9),  2 classes c and c + 64 (across the slot boundary;
             n >= 65),  3 the whole row equal.  Where n is too small for 1 or 2, form 0 is used."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), pad, dtype=torch.float64)
    off = offsets(n_class)
    for f, n in enumerate(n_class):
        seg = torch.randn(rows, n, generator=g, dtype=torch.float64)
        if kind in ("x3", "ties"):
            seg = seg * 3
        elif kind == "shifted":
            seg = seg + 300
        elif kind == "peaked":
            seg.scatter_(1, torch.randint(0, n, (rows, 1), generator=g), 50.0)
        elif kind != "randn":
            raise AssertionError(kind)
        if kind == "ties":
            seg = seg.to(dtype).double()
            top = seg.max(1).values + 1.0
            start = torch.randint(0, 1 << 30, (rows,), generator=g)
            for r in range(rows):
                for c in tie_columns(r, n, int(start[r])):
                    seg[r, c] = top[r]
        x[:, off[f]:off[f] + n] = seg
    return x.to(dtype)


def tie_columns(r, n, start):
    """Columns holding the tied maximum of row r of an attribute of n classes (make_logits 'ties')."""
    form = r % 4
    if form == 3:
        return list(range(n))
    if form == 1 and n >= 9:
        return [7, 8]
    if form == 2 and n >= 65:
        c = start % (n - 64)
        return [c, c + 64]
    g0 = 8 * (start % ((n + 7) // 8))
    return list(range(g0, min(g0 + 3, n, g0 + 8)))


def make_targets(rows, n_class, seed=2, out_of_range=False, logits=None):
    """(rows, A) int64 in range; out_of_range: a quarter of the entries -5, a quarter n + 3 (the kernels clamp them).
    With `logits` (the 'peaked' input): half the targets are the row's peak class, the rest any other (far below)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.stack([torch.randint(0, n, (rows,), generator=g) for n in n_class], 1)
    if logits is not None:
        off = offsets(n_class)
        for f, n in enumerate(n_class):
            peak = logits[:, off[f]:off[f] + n].double().argmax(1)
            t[:, f] = torch.where(torch.rand(rows, generator=g) < 0.5, peak, t[:, f])
    if out_of_range:
        pick = torch.randint(0, 4, t.shape, generator=g)
        t = torch.where(pick == 0, torch.full_like(t, -5), t)
        t = torch.where(pick == 1, torch.tensor(n_class).view(1, -1) + 3, t)
    return t


def make_mask(kind, rows, seed=3):
    """ones | p80 (random, 80 % ones) | last (a single 1 on the last row) | tail (ones only in the last partial tile of 32)."""
    if kind == "ones":
        return torch.ones(rows)
    if kind == "p80":
        return (torch.rand(rows, generator=torch.Generator().manual_seed(seed)) < 0.8).float()
    m = torch.zeros(rows)
    if kind == "last":
        m[-1] = 1
    elif kind == "tail":
        m[((rows - 1) // 32) * 32:] = 1
    else:
        raise AssertionError(kind)
    return m


# ----------------------------------------------------------------------------------------------------------------------
# heads: reference
# ----------------------------------------------------------------------------------------------------------------------
def clamp_targets(target, n_class):
    n = torch.tensor(n_class, device=target.device).view(1, -1)
    return torch.minimum(target.clamp_min(0), n - 1)


def first_argmax(p):
    """First index of the row maximum (torch.argmax does not promise which of several equal maxima it returns)."""
    n = p.shape[1]
    idx = torch.arange(n, device=p.device).expand_as(p)
    return torch.where(p == p.max(1, keepdim=True).values, idx, torch.full_like(idx, n)).min(1).values


def heads_reference(logits, n_class, target=None, mutant=None):
    """f64 per (row, attribute) pieces: mx, logs, xt, nll (with target), p (rows, sum n), argmax, pmax, gap (relative gap of
    the two largest softmax values, inf for n = 1), S-pieces for the bounds, by level of equal values (p2 = sum_l P_l^2, p2d2 = sum_l P_l^2 d_l^2, m2 = sum_l m_l^2) and pd = sum p d.
    mutant: 'nomax' (no max subtraction, in f32 as a kernel would), 'target+1', 'lastmax'."""
    x = logits.double()
    rows, A = x.shape[0], len(n_class)
    off = offsets(n_class)
    dev = x.device
    res = {k: torch.zeros(rows, A, dtype=torch.float64, device=dev) for k in ("mx", "logs", "pmax", "gap", "p2", "p2d2", "pd", "m2")}
    res["argmax"] = torch.zeros(rows, A, dtype=torch.int64, device=dev)
    res["p"] = torch.zeros(rows, off[-1], dtype=torch.float64, device=dev)
    if target is not None:
        t = clamp_targets(target.to(dev), n_class)
        if mutant == "target+1":
            t = (t + 1) % torch.tensor(n_class, device=dev).view(1, -1)
        res["t"] = t
        res["xt"] = torch.zeros(rows, A, dtype=torch.float64, device=dev)
    for f, n in enumerate(n_class):
        seg = x[:, off[f]:off[f] + n]
        mx = seg.max(1).values
        if mutant == "nomax":
            e = torch.exp(seg.float()).double()          # overflows where a kernel without the subtraction would
            s = e.sum(1)
            logs, d = torch.log(s) - mx, mx[:, None] - seg
        else:
            d = mx[:, None] - seg
            e = torch.exp(-d)
            s = e.sum(1)
            logs = torch.log(s)
        p = e / s[:, None]
        res["mx"][:, f], res["logs"][:, f] = mx, logs
        res["p"][:, off[f]:off[f] + n] = p
        if mutant == "lastmax":
            res["argmax"][:, f] = n - 1 - first_argmax(p.flip(1))
        else:
            res["argmax"][:, f] = first_argmax(p)
        res["pmax"][:, f] = p.max(1).values
        if n > 1:
            top = p.topk(2, dim=1).values
            res["gap"][:, f] = (top[:, 0] - top[:, 1]) / top[:, 0]
        else:
            res["gap"][:, f] = float("inf")
        # classes holding the same value have the same e_j and the same rounding errors: grouped by value (levels)
        ds, order = d.sort(1)
        gid = torch.cat([torch.zeros_like(ds[:, :1], dtype=torch.bool), ds[:, 1:] != ds[:, :-1]], 1).long().cumsum(1)
        P = torch.zeros_like(p).scatter_add_(1, gid, p.gather(1, order))            # P_l = m_l p_l, by level
        dl = torch.zeros_like(p).scatter_(1, gid, ds)
        m = torch.zeros_like(p).scatter_add_(1, gid, torch.ones_like(p))
        res["p2"][:, f] = (P * P).sum(1)
        res["p2d2"][:, f] = (P * P * dl * dl).sum(1)
        res["pd"][:, f] = (p * d).sum(1)
        res["m2"][:, f] = (m * m).sum(1)
        if target is not None:
            res["xt"][:, f] = seg.gather(1, res["t"][:, f:f + 1])[:, 0]
    if target is not None:
        res["nll"] = (res["logs"] + res["mx"]) - res["xt"]
        res["scale"] = res["mx"].abs() + res["xt"].abs() + res["logs"].abs()
    return res


def loss_sums(ref, mask=None, drop_from=None):
    """(A) sum_r mask_r nll_rf.  mask None = ones ('mask ignored'); drop_from: rows >= it are left out ('last tile dropped')."""
    nll = ref["nll"] if drop_from is None else ref["nll"][:drop_from]
    if mask is None:
        return nll.sum(0)
    m = mask.double().to(nll.device)
    return (nll * (m if drop_from is None else m[:drop_from])[:, None]).sum(0)


def expand(v, n_class):
    """(rows, A) -> (rows, sum n): each attribute's value on its columns."""
    return torch.repeat_interleave(v, torch.tensor(n_class, device=v.device), dim=1)


def onehot(ref, n_class):
    off = torch.tensor(offsets(n_class)[:-1], device=ref["t"].device).view(1, -1)
    return torch.zeros_like(ref["p"]).scatter_(1, ref["t"] + off, 1.0)


def ce_dlogits(ref, n_class, mask, coef, ld):
    """(rows, ld) f64: (p - onehot) mask_r coef_f, padding columns 0.  -> (dlogits, w (rows, A))."""
    w = mask.double().to(ref["p"].device)[:, None] * coef.double().to(ref["p"].device)[None, :]
    out = torch.zeros(ref["p"].shape[0], ld, dtype=torch.float64, device=ref["p"].device)
    out[:, :ref["p"].shape[1]] = (ref["p"] - onehot(ref, n_class)) * expand(w, n_class)
    return out, w


def logp_dlogits(ref, n_class, g, ld):
    """(rows, ld) f64: (onehot - p) g_rf, padding columns 0."""
    out = torch.zeros(ref["p"].shape[0], ld, dtype=torch.float64, device=ref["p"].device)
    out[:, :ref["p"].shape[1]] = (onehot(ref, n_class) - ref["p"]) * expand(g.double().to(ref["p"].device), n_class)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# heads: bounds and measures
# ----------------------------------------------------------------------------------------------------------------------
def n_exp(bf16):
    return 1.0 if bf16 else 4.0


def n_sum(n, tiled, m2=None):
    """m2 = sum over the levels of equal values of (copies)^2; n when all values differ."""
    if tiled:
        return (n if m2 is None else m2) / 3.0
    return ((n + 63) // 64 - 1) + math.ceil(math.log2(min(n, 64))) if n > 1 else 0.0


def sum_var(ref, n_class, tiled, bf16):
    """(rows, A): S, the relative variance of the softmax sum in units of u^2."""
    ns = ref["m2"] / 3.0 if tiled else \
        torch.tensor([n_sum(n, tiled) for n in n_class], dtype=torch.float64, device=ref["p2"].device)[None, :]
    S = n_exp(bf16) * ref["p2"] + ref["p2d2"] + ns
    if bf16:
        S = S + (LOG2E_C * ref["pd"]) ** 2
    return S


def tree_count(rows, tiled, through_ce=False):
    nb = heads_blocks(rows)
    if tiled:
        ntile = (rows + 31) // 32
        nb = min(nb, ntile)
        own = math.ceil(ntile / nb) / 6.0 + 32 / 6.0
    else:
        own = math.ceil(rows / (4 * nb)) / 6.0 + 2
    return own + math.ceil(nb / 256) / 6.0 + 4 + 16 / 6.0 + (1 if through_ce else 0)


def loss_bound(ref, n_class, mask, tiled, bf16, through_ce=False):
    """-> (bound (A) relative to D, D (A) = sum_r mask_r scale_rf)."""
    m = mask.double().to(ref["nll"].device)[:, None]
    D = (m * ref["scale"]).sum(0)
    rowvar = (m * m * (sum_var(ref, n_class, tiled, bf16) + 7 * ref["scale"] ** 2)).sum(0)
    return 4 * U32 * torch.sqrt(rowvar / D ** 2 + tree_count(ref["nll"].shape[0], tiled, through_ce)), D


def probs_bound(ref, n_class, tiled, bf16):
    """(rows, A): bound of max_j |got_j - p_j| / pmax (and of |pmax - ref| / pmax)."""
    return 4 * U32 * torch.sqrt(n_exp(bf16) + 1.135 + sum_var(ref, n_class, tiled, bf16))


def dlogits_bound(ref, n_class, tiled, bf16, n_w):
    """(rows, A): bound of max_j |got_j - ref_j| / |w_rf|.  n_w: roundings inside w (2 through ops.heads_ce, 0 for logp_bwd)."""
    v = (n_exp(bf16) + 5.135 + n_w + sum_var(ref, n_class, tiled, bf16)) * U32 ** 2
    if bf16:
        v = v + U16 ** 2
    return 4 * torch.sqrt(v)


def seg_max(err, n_class):
    """(rows, sum n) -> (rows, A): the largest entry of each attribute's columns."""
    off = offsets(n_class)
    return torch.stack([err[:, off[f]:off[f] + n].max(1).values for f, n in enumerate(n_class)], 1)


def rows_ratio(got, want, scale, bound, n_class):
    """Worst of (max over the attribute's columns of |got - want|) / (scale bound), over the (row, attribute) pairs with
    scale > 0; the others must be exactly equal (asserted by the caller through the returned flag).
    -> (worst ratio, all-equal-where-scale-is-0)."""
    err = seg_max((got.double() - want).abs(), n_class)
    live = scale > 0
    exact = bool((err[~live] == 0).all())
    if not live.any():
        return 0.0, exact
    return (err[live] / (scale[live] * bound[live])).max().item(), exact


def argmax_check(got, ref):
    """-> (mismatches outside the skipped pairs, share of skipped pairs)."""
    skip = (ref["gap"] > 0) & (ref["gap"] < GAP)
    bad = ((got.to(ref["argmax"].device) != ref["argmax"]) & ~skip).sum().item()
    return bad, skip.double().mean().item()


# ----------------------------------------------------------------------------------------------------------------------
# RL: references
# ----------------------------------------------------------------------------------------------------------------------
def rollout_gather(ids, probs, n_class, NA, mode, mutant=None):
    """ids (R, T, A) int64, probs (R, T, W) -> action (R, NA, A), logp (R, NA, A) f64 (modes 1, 2; None for mode 0)."""
    R, T, A = ids.shape
    off = offsets(n_class)
    k = torch.arange(NA, device=ids.device)
    pos = torch.where(k == 0, torch.zeros_like(k), T - k) if mode == 0 else T - (k + 1)
    action = ids[:, pos, :]
    if mode == 0:
        return action, None
    c = action.clone()
    if mode == 1:
        c[:, :, :2] = ids[:, k + 1, :2]
    col = c + torch.tensor(off[:-1], device=ids.device).view(1, 1, -1)
    logp = torch.log(probs.double()[:, pos, :].gather(2, col))
    return action, logp


def ppo_returns_adv(rewards, values, gamma, normalize=True, mutant=None):
    """rewards, values (E) -> returns (E), adv (E) f64, and V (E): the recursion's error variance in units of u^2.
    mutant: 'textbook' (the recursion from the last reward backwards), 'biased' (std with 1 / E)."""
    r, v = rewards.double().reshape(-1), values.double().reshape(-1)
    gamma = f32v(gamma)
    E = r.numel()
    ret = torch.zeros(E, dtype=torch.float64)
    V = torch.zeros(E, dtype=torch.float64)
    R = Vt = 0.0
    rl = r.tolist()
    if mutant == "textbook":
        for t in reversed(range(E)):
            R = rl[t] + R * gamma
            ret[t] = R
    else:
        for t in range(E):
            R = rl[t] + R * gamma
            Vt = gamma * gamma * Vt + 2 * R * R
            ret[E - 1 - t], V[E - 1 - t] = R, Vt
    ret = ret.to(r.device)
    corr = 0 if mutant == "biased" else 1
    if normalize:
        ret = (ret - ret.mean()) / ret.std(correction=corr)
    adv = ret - v
    if normalize:
        adv = (adv - adv.mean()) / adv.std(correction=corr)
    return ret, adv, V


def _normalise_err(x, a):
    """rms errors (absolute) of (x - mean) / sd (unbiased) given the values x (E) and their rms errors a (E)."""
    E = x.numel()
    m = math.ceil(E / 64)
    mean = x.mean()
    var_mean = a.max() ** 2 + U32 ** 2 * (m / 6 + 7) * x.abs().mean() ** 2
    c = x - mean
    D2 = a ** 2 + var_mean + U32 ** 2 * c ** 2
    sd = x.std()
    rel_sd2 = D2.sum() / (c ** 2).sum() + U32 ** 2 * (m / 6 + 11)
    y = c / sd
    return torch.sqrt(D2 / sd ** 2 + y ** 2 * (rel_sd2 + U32 ** 2))


def ppo_returns_adv_bounds(rewards, values, gamma, normalize=True):
    """-> (returns bound (E), adv bound (E)): absolute, 4 x rms."""
    r, v = rewards.double().reshape(-1), values.double().reshape(-1)
    ret, _, V = ppo_returns_adv(r, v, gamma, normalize=False)
    a = U32 * torch.sqrt(V)
    if not normalize:
        return 4 * a, 4 * torch.sqrt(a ** 2 + U32 ** 2 * (ret - v) ** 2)
    a1 = _normalise_err(ret, a)
    y = (ret - ret.mean()) / ret.std()
    adv = y - v
    a2 = _normalise_err(adv, torch.sqrt(a1 ** 2 + U32 ** 2 * adv ** 2))
    return 4 * a1, 4 * a2


def ppo_policy_loss(new_logp, old_int, adv, clip, mutant=None):
    """new_logp (NA, A), old_int (E, NA, A) int64, adv (E) -> dict loss, grad (NA, A), and the bounds' pieces.
    mutant: 'ratioA' (surrogate 1 as ratio * A, the textbook form)."""
    nl, a = new_logp.double(), adv.double().reshape(-1, 1, 1)
    d = nl[None] - old_int.double()
    ratio = torch.exp(d)
    l1 = ratio * a if mutant == "ratioA" else 0.2 * a
    l2 = ratio.clamp(1 - clip, 1 + clip) * a
    n = float(ratio.numel())
    term = torch.minimum(l1, l2)
    inside = (ratio > 1 - clip) & (ratio < 1 + clip)
    sel = (l2 < l1) & inside
    if mutant == "ratioA":
        gterm = torch.where(l1 <= l2, ratio * a, torch.where(inside, ratio * a, torch.zeros_like(ratio)))
    else:
        gterm = torch.where(sel, ratio * a, torch.zeros_like(ratio))
    near = ((ratio / (1 - clip) - 1).abs() < EDGE * (1 + d.abs())) | ((ratio / (1 + clip) - 1).abs() < EDGE * (1 + d.abs()))
    near = near & (a < 0)
    return {"loss": -term.sum() / n, "grad": -gterm.sum(0) / n, "term_abs": term.abs().sum(), "term_rss": (term ** 2).sum().sqrt(),
            "g_abs": gterm.abs().sum(0), "g_edge": torch.where(near, (ratio * a).abs(), torch.zeros_like(ratio)).sum(0),
            "dmax": d.abs().max(), "n": n, "ratio": ratio, "E": ratio.shape[0]}


def ppo_policy_loss_bounds(ref, autograd=False):
    """-> (loss bound (absolute), grad bound (NA, A) absolute)."""
    E, n = ref["E"], ref["n"]
    KF = n / E
    trips = math.ceil(KF / 256)
    per = 6 + ref["dmax"] ** 2
    lb = 4 * U32 * torch.sqrt(per * (ref["term_rss"] / ref["term_abs"].clamp_min(1e-300)) ** 2 + E * trips / 6 + 10) * ref["term_abs"] / n
    gb = 4 * U32 * torch.sqrt(per + E / 6 + 2 + (1 if autograd else 0)) * ref["g_abs"] / n + ref["g_edge"] / n
    return lb, gb


def dqn_td(y, yt, action, reward, done, n_class, gamma, mutant=None):
    """y, yt (B, T, W), action (B, NA, A), reward, done (B) -> dict mse (A), dq (B, NA, A), q, top, s (the scale of d) in f64.
    mutant: 'ascending' (the NA smallest next-state values, ascending), 'batch_j' (q from batch element j, not 0)."""
    B, T, W = y.shape
    NA, A = action.shape[1], action.shape[2]
    gamma = f32v(gamma)
    off = offsets(n_class)
    y64, yt64 = y.double(), yt.double()
    r, dn = reward.double().reshape(B, 1), done.double().reshape(B, 1)
    jj = torch.arange(B, device=y.device).view(B, 1).expand(B, NA)
    q = torch.zeros(B, NA, A, dtype=torch.float64, device=y.device)
    top = torch.zeros_like(q)
    src = y64[jj, jj] if mutant == "batch_j" else y64[0][jj]                        # (B, NA, W): row j of batch element 0
    for f, n in enumerate(n_class):
        q[:, :, f] = src.gather(2, (action[:, :, f] + off[f]).unsqueeze(2))[:, :, 0]
        nxt = yt64[:, :, off[f]:off[f] + n].max(2).values
        srt = nxt.sort(1, descending=mutant != "ascending").values
        top[:, :, f] = srt[:, :NA]
    tgt = r.unsqueeze(2) + gamma * (1 - dn).unsqueeze(2) * top
    d = q - tgt
    s = q.abs() + r.abs().unsqueeze(2) + gamma * top.abs()
    return {"mse": (d * d).mean((0, 1)), "dq": 2 * d / (B * NA * A), "d": d, "q": q, "top": top, "s": s, "tgt": tgt}


def dqn_td_dy(ref, action, n_class, gw, shape):
    """Gradient of sum_f gw_f mse_f w.r.t. y (B, T, W): batch element 0's rows j < B only, duplicates of an action summed.
    -> (dy, bound): bound (T, W) absolute for batch element 0's rows, 0 where nothing is scattered."""
    B, T, W = shape
    NA, A = action.shape[1], action.shape[2]
    dev = action.device
    off = torch.tensor(offsets(n_class)[:-1], device=dev).view(1, 1, -1)
    idx = (torch.arange(B, device=dev).view(B, 1, 1) * W + action + off).reshape(-1)
    w = gw.double().to(dev).view(1, 1, -1) * 2 / (B * NA)

    def scatter(v):
        return torch.zeros(T * W, dtype=torch.float64, device=dev).index_add_(0, idx, v.reshape(-1)).view(T, W)

    dy = torch.zeros(B, T, W, dtype=torch.float64, device=dev)
    dy[0] = scatter(ref["d"] * w)
    bound = 4 * U32 * torch.sqrt(11 + scatter(torch.ones_like(ref["d"])) / 6) * scatter(ref["s"] * w.abs())
    return dy, bound


def dqn_td_bounds(ref, B, NA, A):
    """-> (mse bound (A) absolute, dq bound (B, NA, A) absolute)."""
    m = math.ceil(NA / 64)
    d, s = ref["d"], ref["s"]
    var = ((2 * d * 5 ** 0.5 * s) ** 2).sum((0, 1)) + (m / 6 + 9 + B / 6) * (d * d).sum((0, 1)) ** 2
    return 4 * U32 * torch.sqrt(var) / (B * NA), 4 * U32 * 3 * s * 2 / (B * NA * A)


# ----------------------------------------------------------------------------------------------------------------------
# one place for the comparisons the CPU pin and the GPU tests both make
# ----------------------------------------------------------------------------------------------------------------------
def miss(got, want, denom):
    """max |got - want| / denom with a non-finite difference counted as infinite (a mutant that overflows has missed)."""
    r = (got.double() - want.double()).abs() / denom
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return r.max().item() if r.numel() else 0.0


def heads_ratios(ref, n_class, tiled, bf16, mask=None, loss=None, through_ce=False, pmax=None, probs=None):
    """Worst |error| / bound per group of the forward's outputs (loss given as the SUM over rows)."""
    out = {}
    if loss is not None:
        b, D = loss_bound(ref, n_class, mask, tiled, bf16, through_ce)
        out["loss"] = miss(loss, loss_sums(ref, mask), D * b)
    pb = probs_bound(ref, n_class, tiled, bf16)
    if pmax is not None:
        out["pmax"] = miss(pmax, ref["pmax"], ref["pmax"] * pb)
    if probs is not None:
        out["probs"], _ = rows_ratio(probs, ref["p"], ref["pmax"], pb, n_class)
    return out


def pair_ratios(got, want, scale, bound, n_class):
    """(rows, A): max over the attribute's columns of |got - want| / (scale bound); nan where scale is 0."""
    err = seg_max((got.double() - want).abs(), n_class)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(scale > 0, err / (scale * bound), torch.full_like(err, float("nan")))

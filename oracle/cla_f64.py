"""Causal linear attention scans in f64 (TEST INFRASTRUCTURE; see oracle/__init__.py): the reference with every buffer the
kernels write, the per-row "uncancelled" norms the GPU test divides by, an f64 emulation of nothing but the bf16 roundings
of the MFMA kernels (csrc/cla_bf16.hip), and the error bounds of tests/test_cla_f64_gpu.py.  Plain torch, any device.

Tensors use the package's layout: q, k, v, dout (N, L, H, 64).  On top of oracle/cla.py (the forward's three forms).

    Q = phi(q), K = phi(k), phi = elu + 1;  A_ij = Q_i . K_j (j <= i);  den_i = sum_j A_ij + eps;  z_i = 1 / den_i
    out_i = z_i sum_j A_ij v_j;  dden_i = -(dout_i . out_i) z_i;  c_ij = z_i dout_i . (v_j - out_i) = z_i dout_i . v_j + dden_i
    dv_j = sum_{i>=j} z_i A_ij dout_i;  dk_j = phi'(k_j) * sum_{i>=j} c_ij Q_i;  dq_i = phi'(q_i) * sum_{j<=i} c_ij K_j
    final state: S = sum_j K_j v_j^T (e x m), ksum = sum_j K_j.

Row terms (row_terms): the norm a row of 64 would have if the contributions of its tokens added without cancelling,
    T(out_i)^2 = sum_j |z_i A_ij v_j|^2                T(dv_j)^2 = sum_{i>=j} |z_i A_ij dout_i|^2
    T(dk_j)^2  = sum_{i>=j} |phi'(k_j) * Q_i c_ij|^2   T(dq_i)^2 = sum_{j<=i} |phi'(q_i) * K_j z_i dout_i.v_j|^2 + |phi'(q_i) * ksum_i dden_i|^2
(dq: the numerator part token by token and the normaliser part dden_i ksum_i as one term: the two nearly cancel where a row
averages over many tokens, oracle/step_f64.normaliser_terms).  One query chunk of 64 against all its keys at a time: O(L x 64)
memory per stream.

Rounding emulation (emulate_mfma), read off csrc/cla_bf16.hip with CWLT_STATE_LO = 0 (cwlt_mfma_bf16.h's default: running
states enter the MFMAs as ONE bf16 operand, no residual).  r() = round to bf16; everything else exact (f64):
    forward   Qr = r(phi(q)), Kr = r(phi(k)); score tile At = r(Qr Kr^T) masked; num = At v + Qr r(S); den = sum_j At +
              Qr . r(ksum) + eps (the same rounded tile in both); z = 1 / den (f32, stored); out = r(num z).  S, ksum
              accumulate Kr v^T and Kr unrounded.
    backward  g = r(dout z); dden = -(dout . out_stored) z (f32; the stored bf16 out).  A-tile At as above.
      pair    dkdv: W = r(g v^T + r(dden)) masked (dden enters through an MFMA operand); dkf = W^T Qr + r(R) v + r(r1);
              dk = r(r(dkf) min(Kr, 1)) (the dkf tile crosses LDS in bf16 and is rounded again after phi'); dv = r(At^T g +
              r(R)^T Kr); R = sum_later Qr g^T, r1 = sum_later Qr (hi + lo of dden).  dq: W = r(g v^T + dden) (f32 add);
              dqf = W Kr + r(S) g + r(ksum) r(dden); dq = r(dqf phi'(q)) with phi' from the raw q.
      sweep   one W = r(g v^T + r(dden)) for both groups; dk = r(dkf min(Kr, 1)) (one rounding); dq = r(dqf min(Qr, 1))
              (phi' from the rounded phi); S of the dq group = final state minus the chunks passed (exact here; its f32
              term is sweep_state_term()).
      segmented  the same roundings as the pair: a segment's start state is the f32 sum of the increments of the segments
              before it, rounded to bf16 at the same place.  Only the order of f32 additions differs, which is no bf16
              rounding; emulate_mfma therefore has no segmented variant and the segmented bounds are the pair's.
    column sums  pair: dq and dk columns sum the f32 values BEFORE the output rounding, dv the stored bf16; sweep: all
              three sum the stored bf16 values.

Bounds (row_bound and friends): u = 2^-24 per f32 operation, U = 2^-9 / sqrt(3) rms per bf16 rounding, errors independent,
a sum of n terms counts n / 6, the bound 4 x the predicted rms.  The measure of a row is |got - ref| / den, den =
max(|ref row|, T_row).  A rounding of a factor of one token's term errs the row by at most U T_row, a rounding of the whole
row by U |row|: these count into n_T.  A rounding made element by element BEFORE the contraction over the 64 value columns
(g, and the stored out inside dden) errs the row by U E_row (operand_terms), which is not bounded by den: where v has a
mean, dout_i . v_j and dout_i . out_i are cancelling sums of 64 and E / den reaches 30 at L = 1 024.  These count into n_E
and enter as a function of the row, computed from the reference:
        bound_row = 4 sqrt((n_T + n_E (E_row / den_row)^2) U^2 + (the same with the f32 counts) u^2)
(with n_T alone the emulation sits at 8 x the bound in its worst dq row of input 3; with both, at 0.6).  Counts, from the
source:
    z     phi(q), phi(k), score tile, r(ksum): 4 roundings of positive terms averaged over 64 features and the row's keys,
          counted 1 wherever z enters.
    out   phi(q) 1, phi(k) 1, score tile or r(S) 1, z 1, output 1                                    n_T = 5
    dv    g 1, z 1, phi(q) 1, phi(k) 1, A tile or r(R) 1, output 1 (g multiplies one dout row: no contraction)  n_T = 6
    dk    n_E = 6: g 1 and the stored out inside dden 5 (it carries the forward's n_T).  n_T: z 1, r(dden) 1, W tile or
          r(R) / r(r1) 1, Qr 1, min(Kr, 1) 1, output 1 = 6 (sweep); the pair rounds dkf once more = 7.
    dq    n_E = 6 as dk.  n_T: z 1, W tile or r(S) / r(ksum) 1, Kr 1, r(dden) beside ksum 1, output 1 = 5 (pair); the sweep
          also rounds dden inside the tile and takes phi' from the rounded phi(q) = 7.
    generic bf16 (cla.hip's templates on bf16: f32 arithmetic, bf16 loads and stores): out 1; dv 1; dq, dk n_T = 1 (output),
          n_E = 1 (the stored out inside dden), plus the f32 counts.
    mixed  the generic backward behind the MFMA forward (a dout view whose row stride is no multiple of 8): it reads the
          MFMA forward's z (1) and out (5): dv, dq, dk n_T = 2 (z, output), n_E = 5.
    f32   per row: phi (expf at 2 ulp) 4 + 4, score 64/6, the sum over the row's tokens P/6, normaliser 64/6 + P/6,
          reciprocal and product 2:  n32_fwd = 12 + 64/3 + P/3; the backward carries z and its own sums, as much again, and
          the product with phi' :  n32_bwd = 2 n32_fwd + 2 (n_T);  n_E = n32_fwd + 64/6 + 2 (out inside dden, the sum of 64
          products, the product with z).  The test takes P = L for every row (the largest count).
    zinv  MFMA: the 4 roundings above, each at most U of den since every term is positive: 4 sqrt(4) U of |ref|.
          f32 / generic: 4 sqrt(n32_fwd) u.
    dden  |dden - ref| <= z |dout| |out - ref out| + |dden| dz/z: relative to D_i = max(|ref|, z_i |dout_i| max(|out_i|,
          T(out_i))) (the Cauchy-Schwarz bound of the element's uncancelled sum) the out bound and the zinv bound add.
    final state  f32 accumulation of exact products of bf16 values: 4 sqrt(L/6) u of the sum of |terms|; the test's measure
          is relative to the root-sum-square of the L terms, so the bound per element is that times sum|t| / rss(t).
    column sums  f32 additions of L values: 4 sqrt(L/6 + 3) u of the column's sum of |terms|; where the kernel sums the
          f32 values before the output rounding (pair: dq, dk) the stored values the test can sum differ from them by L
          independent roundings: + 4 (2 U) rss(terms).  2 U: a value just above a power of two rounds with rms 2 U, one
          just below the next with U; the row bounds have other terms to share with, this sum of roundings has none (the
          emulation measures 1.37 U rss).
    phi   the MFMA kernels evaluate phi = exp(x) for x <= 0 (relative error); cla.hip (f32, generic) evaluates
          (exp(x) - 1) + 1 as the reference does: an absolute error u, which the f32 and generic bounds carry per row as
          4 sqrt(2) kappa_i (phi_abs_term), in quadrature.  Where eps decides a row (input 4, rows 0 .. 4) kappa is about
          1: those forms keep no significant digit there and the bound says so.
    sweep dq state  S_prev = final - passed chunks in f32: sqrt(chunks passed) u |final| / |prefix| relative error of
          the state operand of chunk c, added in quadrature (sweep_state_term), nothing for chunk 0 (an exact zero).
"""
import torch

from oracle import cla as ocla

EPS = ocla.EPS
C = 64
U16 = 2.0 ** -9 / 3 ** 0.5
U32 = 2.0 ** -24
TEETH = 5.0
N16_T = {
    "mfma":    {"out": 5, "dv": 6, "dk": 7, "dq": 5},      # forward; whole-sequence and segmented pair
    "sweep":   {"out": 5, "dv": 6, "dk": 6, "dq": 7},
    "generic": {"out": 1, "dv": 1, "dk": 1, "dq": 1},
    "mixed":   {"out": 5, "dv": 2, "dk": 2, "dq": 2},      # MFMA forward, generic backward (a dout view of odd stride)
    "f32":     {"out": 0, "dv": 0, "dk": 0, "dq": 0},
}
N16_E = {"mfma": 6, "sweep": 6, "generic": 1, "mixed": 5, "f32": 0}     # dq and dk only


def phi(x):
    """elu(x) + 1 without the cancellation of (exp(x) - 1) + 1, which costs f64 eight digits at x = -20."""
    return torch.where(x > 0, x + 1, torch.exp(x))


def dphi(x):
    return torch.where(x > 0, torch.ones_like(x), torch.exp(x))


def rb(x):
    """Round to bf16, keep f64."""
    return x.to(torch.bfloat16).to(torch.float64)


def _s(t):
    """(N, L, H, D) -> (N, H, L, D)."""
    return t.permute(0, 2, 1, 3)


# ----------------------------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------------------------
def n32_fwd(L):
    return 12 + 64 / 3 + L / 3


def n32_bwd(L):
    return 2 * n32_fwd(L) + 2


def n32_e(L):
    return n32_fwd(L) + 64 / 6 + 2


def row_bound(form, name, L, e_over_den=None):
    """Bound on |got - ref| / max(|ref row|, T_row) for the rows of `name` (out, dq, dk, dv) computed by `form`; dq and dk
    need e_over_den (N, L, H) = E_row / den_row and get a bound per row."""
    n16, n32 = N16_T[form][name], n32_fwd(L) if name == "out" else n32_bwd(L)
    if name in ("dq", "dk"):
        n16 = n16 + N16_E[form] * e_over_den ** 2
        n32 = n32 + n32_e(L) * e_over_den ** 2
    return 4 * (n16 * U16 ** 2 + n32 * U32 ** 2) ** 0.5


def zinv_bound(form, L):
    return 4 * 2 * U16 if form in ("mfma", "sweep", "mixed") else 4 * n32_fwd(L) ** 0.5 * U32


def dden_bound(form, L):
    return row_bound(form, "out", L) + zinv_bound(form, L)


def state_bound(L):
    """Of the sum of |terms| of an element of the final state."""
    return 4 * (L / 6) ** 0.5 * U32


def colsum_bound(L):
    """Of the sum of |terms| of a column: f32 additions of L values."""
    return 4 * (L / 6 + 3) ** 0.5 * U32


def sweep_state_term(ref, L):
    """(N, H, nch): relative f32 error of the sweep's dq prefix state in front of chunk c (see the module docstring)."""
    K, v = _s(phi(ref["k"])), _s(ref["v"])
    nch = (L + C - 1) // C
    out = torch.zeros(K.shape[0], K.shape[1], nch, dtype=torch.float64, device=K.device)
    S = torch.zeros(K.shape[0], K.shape[1], 64, 64, dtype=torch.float64, device=K.device)
    pre = []
    for c in range(nch):
        pre.append(S.flatten(2).norm(dim=-1))
        S = S + torch.einsum("nhje,nhjm->nhem", K[:, :, c * C:(c + 1) * C], v[:, :, c * C:(c + 1) * C])
    fin = S.flatten(2).norm(dim=-1)
    for c in range(1, nch):
        out[:, :, c] = (nch - c) ** 0.5 * U32 * fin / pre[c].clamp_min(1e-300)
    return out


def phi_abs_term(ref):
    """(N, L, H) kappa_i: the relative error of row i's normaliser where phi is evaluated as (exp(x) - 1) + 1 in f32, as
    cla.hip does to match the reference bit for bit: an ABSOLUTE error u in every phi(k_je), j <= i, and phi(q_ie),
    kappa_i = u sqrt((i + 1) |Q_i|^2 + |ksum_i|^2) / den_i.  1e-8 on ordinary rows; about 1 where eps decides the row
    (phi(-20) = 2e-9 evaluates to 0 in f32)."""
    Q, ksum = phi(ref["q"]), phi(ref["k"]).cumsum(1)
    i1 = torch.arange(1, Q.shape[1] + 1, dtype=torch.float64, device=Q.device)[None, :, None]
    return U32 * (i1 * (Q ** 2).sum(-1) + (ksum ** 2).sum(-1)).sqrt() * ref["zinv"]


def bounds(form, ref, terms, L):
    """{"out", "dq", "dk", "dv"}: the row bounds of `form` ("f32" | "generic" | "mfma" | "sweep"); terms = analyse(ref)."""
    res = {}
    for n in ("out", "dq", "dk", "dv"):
        eod = terms["E_" + n] / terms["den_" + n].clamp_min(1e-300) if n in ("dq", "dk") else None
        res[n] = row_bound(form, n, L, eod) * torch.ones_like(terms["den_" + n])
    if form in ("f32", "generic", "mixed"):
        # numerator and normaliser both: 4 sqrt(2) kappa; a key row j collects the query rows i >= j: the largest of them
        kap = 4 * 2 ** 0.5 * phi_abs_term(ref)
        rev = kap.flip(1).cummax(1).values.flip(1)
        for n, x in (("out", kap), ("dq", kap), ("dk", rev), ("dv", rev)):
            res[n] = (res[n] ** 2 + x ** 2) ** 0.5
    if form == "sweep":
        t = sweep_state_term(ref, L).repeat_interleave(C, dim=2)[:, :, :L].permute(0, 2, 1)
        res["dq"] = (res["dq"] ** 2 + (4 * t) ** 2) ** 0.5
    return res


# ----------------------------------------------------------------------------------------------------------------------
# reference
# ----------------------------------------------------------------------------------------------------------------------
def cla_chunked(q, k, v, eps=EPS, chunk=C):
    """oracle.cla.cla_chunked with this module's phi."""
    Q, K = _s(phi(q)), _s(phi(k))
    v = _s(v)
    S = torch.zeros(Q.shape[0], Q.shape[1], 64, 64, dtype=q.dtype, device=q.device)
    z = torch.zeros(Q.shape[0], Q.shape[1], 64, dtype=q.dtype, device=q.device)
    outs = []
    for c0 in range(0, Q.shape[2], chunk):
        Qc, Kc, Vc = Q[:, :, c0:c0 + chunk], K[:, :, c0:c0 + chunk], v[:, :, c0:c0 + chunk]
        A = torch.tril(Qc @ Kc.transpose(2, 3))
        den = A.sum(-1) + torch.einsum("nhie,nhe->nhi", Qc, z) + eps
        outs.append((A @ Vc + Qc @ S) / den[..., None])
        S = S + Kc.transpose(2, 3) @ Vc
        z = z + Kc.sum(2)
    return _s(torch.cat(outs, 2))


def reference(q, k, v, dout, eps=EPS, fn=cla_chunked, kf_round=None):
    """f64 out, zinv (N, L, H), dq, dk, dv, dden (N, L, H), fin_S (N, H, m, e) and fin_z (N, H, e) -- the layout of the
    kernels' final-state buffer -- by autograd through `fn`.  kf_round: applied to phi(k) for the final state (the MFMA
    forward sums the bf16-rounded phi(k))."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    out, dq, dk, dv = ocla.cla_grads(q, k, v, dout, fn=fn, eps=eps)
    Q, K = phi(q), phi(k)
    zinv = 1.0 / (torch.einsum("nlhe,nlhe->nlh", Q, K.cumsum(1)) + eps)
    dden = -(dout * out).sum(-1) * zinv
    Kf = K if kf_round is None else kf_round(K)
    return {"q": q, "k": k, "v": v, "dout": dout, "eps": eps, "out": out, "zinv": zinv, "dq": dq, "dk": dk, "dv": dv,
            "dden": dden, "fin_S": torch.einsum("nlhe,nlhm->nhme", Kf, v), "fin_z": Kf.sum(1),
            "fin_S_abs": torch.einsum("nlhe,nlhm->nhme", Kf, v.abs()), "fin_S_rss":
            torch.einsum("nlhe,nlhm->nhme", Kf ** 2, v ** 2).sqrt(), "fin_z_rss": (Kf ** 2).sum(1).sqrt()}


def explicit_grads(q, k, v, dout, eps=EPS):
    """out, dq, dk, dv from the formulas of the module docstring, L x L (the third reference form; small L only)."""
    q, k, v, dout = (_s(t.double()) for t in (q, k, v, dout))
    Q, K = phi(q), phi(k)
    L = q.shape[2]
    A = torch.tril(torch.einsum("nhie,nhje->nhij", Q, K))
    z = 1.0 / (A.sum(-1) + eps)
    out = torch.einsum("nhij,nhjm->nhim", A, v) * z[..., None]
    c = (torch.einsum("nhim,nhjm->nhij", dout, v) - (dout * out).sum(-1)[..., None]) * z[..., None]
    c = torch.tril(c)
    dv = torch.einsum("nhij,nhim->nhjm", A * z[..., None], dout)
    dk = dphi(k) * torch.einsum("nhij,nhie->nhje", c, Q)
    dq = dphi(q) * torch.einsum("nhij,nhje->nhie", c, K)
    return tuple(_s(t) for t in (out, dq, dk, dv))


def row_terms(ref):
    """{"out", "dq", "dk", "dv"}: (N, L, H) uncancelled row norms, plus "dden": the denominator D_i of the dden measure."""
    q, k, v, dout, out = (_s(ref[n]) for n in ("q", "k", "v", "dout", "out"))
    z, dden = ref["zinv"].permute(0, 2, 1), ref["dden"].permute(0, 2, 1)
    Q, K = phi(q), phi(k)
    N, H, L, _ = q.shape
    zero = lambda: torch.zeros(N, H, L, dtype=torch.float64, device=q.device)
    t_out, t_dq, t_dv = zero(), zero(), zero()
    t_dk = torch.zeros(N, H, L, 64, dtype=torch.float64, device=q.device)
    v2, g2, K2, Q2 = (v ** 2).sum(-1), (dout ** 2).sum(-1), K ** 2, Q ** 2
    dq2, dk2 = dphi(q) ** 2, dphi(k) ** 2
    ksum = K.cumsum(2)
    for c0 in range(0, L, C):
        i = slice(c0, min(L, c0 + C))
        j = slice(0, i.stop)
        mask = (torch.arange(i.start, i.stop, device=q.device)[:, None] >= torch.arange(0, i.stop, device=q.device))
        A = torch.einsum("nhie,nhje->nhij", Q[:, :, i], K[:, :, j]) * mask * z[:, :, i, None]        # z_i A_ij
        t_out[:, :, i] = torch.einsum("nhij,nhj->nhi", A ** 2, v2[:, :, j])
        t_dv[:, :, j] += torch.einsum("nhij,nhi->nhj", A ** 2, g2[:, :, i])
        gv = torch.einsum("nhim,nhjm->nhij", dout[:, :, i], v[:, :, j]) * z[:, :, i, None] * mask    # z_i dout_i . v_j
        cc = (gv + dden[:, :, i, None]) * mask                                                      # c_ij
        t_dk[:, :, j] += torch.einsum("nhij,nhie->nhje", cc ** 2, Q2[:, :, i])
        t_dq[:, :, i] = (dq2[:, :, i] * (torch.einsum("nhij,nhje->nhie", gv ** 2, K2[:, :, j]) +
                                          (ksum[:, :, i] * dden[:, :, i, None]) ** 2)).sum(-1)
    t_dk = (t_dk * dk2).sum(-1)
    res = {"out": t_out.sqrt(), "dq": t_dq.sqrt(), "dk": t_dk.sqrt(), "dv": t_dv.sqrt()}
    res["dden"] = torch.maximum(dden.abs(), z * g2.sqrt() * torch.maximum(out.norm(dim=-1), res["out"]))
    return {n: t.permute(0, 2, 1) for n, t in res.items()}


def operand_terms(ref):
    """{"dq", "dk"}: (N, L, H) norms of the rows if, in addition, the contraction over the 64 value columns did not cancel.
    g = r(dout z) and the stored out inside dden are rounded element by element BEFORE they are contracted with v, S or
    out over m, so their errors are relative to these, not to the row terms (where v has a mean, dout_i . v_j is a
    cancelling sum of 64 and S_em a coherent sum over the tokens):
        E(dq_i)^2 = sum_e phi'(q_ie)^2 z_i^2 [sum_m dout_im^2 (S_i,em^2 + sum_{j<=i} K_je^2 v_jm^2) + ksum_ie^2 sum_m dout_im^2 out_im^2]
        E(dk_j)^2 = sum_e phi'(k_je)^2 [sum_m v_jm^2 (R_j,em^2 + sum_{i>=j} Q_ie^2 z_i^2 dout_im^2) + sum_{i>=j} Q_ie^2 z_i^2 sum_m dout_im^2 out_im^2]
    with the inclusive states S_i = sum_{j<=i} K_j v_j^T and R_j = sum_{i>=j} z_i Q_i dout_i^T."""
    q, k, v, dout, out = (_s(ref[n]) for n in ("q", "k", "v", "dout", "out"))
    z = ref["zinv"].permute(0, 2, 1)[..., None]
    Q, K = phi(q), phi(k)
    N, H, L, _ = q.shape
    g = dout * z
    do2 = (g ** 2 * out ** 2).sum(-1, keepdim=True)                       # z_i^2 sum_m dout_im^2 out_im^2
    ksum = K.cumsum(2)
    e_dq = torch.zeros(N, H, L, dtype=torch.float64, device=q.device)
    e_dk = torch.zeros_like(e_dq)
    z4 = lambda: torch.zeros(N, H, 64, 64, dtype=torch.float64, device=q.device)
    S, S2 = z4(), z4()
    for c0 in range(0, L, C):
        i = slice(c0, min(L, c0 + C))
        Sc = S[:, :, None] + torch.einsum("nhje,nhjm->nhjem", K[:, :, i], v[:, :, i]).cumsum(2)
        S2c = S2[:, :, None] + torch.einsum("nhje,nhjm->nhjem", K[:, :, i] ** 2, v[:, :, i] ** 2).cumsum(2)
        t = torch.einsum("nhim,nhiem->nhie", g[:, :, i] ** 2, Sc ** 2 + S2c) + ksum[:, :, i] ** 2 * do2[:, :, i]
        e_dq[:, :, i] = (dphi(q[:, :, i]) ** 2 * t).sum(-1)
        S, S2 = Sc[:, :, -1], S2c[:, :, -1]
    R, R2, R3 = z4(), z4(), torch.zeros(N, H, 64, dtype=torch.float64, device=q.device)
    for c0 in range((L - 1) // C * C, -1, -C):
        i = slice(c0, min(L, c0 + C))
        rc = lambda x: x.flip(2).cumsum(2).flip(2)
        Rc = R[:, :, None] + rc(torch.einsum("nhie,nhim->nhiem", Q[:, :, i], g[:, :, i]))
        R2c = R2[:, :, None] + rc(torch.einsum("nhie,nhim->nhiem", Q[:, :, i] ** 2, g[:, :, i] ** 2))
        R3c = R3[:, :, None] + rc(Q[:, :, i] ** 2 * do2[:, :, i])
        t = torch.einsum("nhjm,nhjem->nhje", v[:, :, i] ** 2, Rc ** 2 + R2c) + R3c
        e_dk[:, :, i] = (dphi(k[:, :, i]) ** 2 * t).sum(-1)
        R, R2, R3 = Rc[:, :, 0], R2c[:, :, 0], R3c[:, :, 0]
    return {"dq": e_dq.sqrt().permute(0, 2, 1), "dk": e_dk.sqrt().permute(0, 2, 1)}


def analyse(ref):
    """row_terms and operand_terms of a reference, and den_<name> = max(|ref row|, T_row): everything the measure needs."""
    t = row_terms(ref)
    e = operand_terms(ref)
    res = dict(t)
    for n in ("out", "dq", "dk", "dv"):
        res["den_" + n] = torch.maximum(ref[n].norm(dim=-1), t[n])
    res["E_dq"], res["E_dk"] = e["dq"], e["dk"]
    res["E_out"], res["E_dv"] = res["den_out"], res["den_dv"]
    return res


def row_terms_brute(ref):
    """The same by the whole L x L x 64 tensors (to pin row_terms at small L)."""
    q, k, v, dout, out = (_s(ref[n]) for n in ("q", "k", "v", "dout", "out"))
    z, dden = ref["zinv"].permute(0, 2, 1), ref["dden"].permute(0, 2, 1)
    Q, K = phi(q), phi(k)
    L = q.shape[2]
    tril = torch.tril(torch.ones(L, L, dtype=torch.float64, device=q.device))
    w = torch.einsum("nhie,nhje->nhij", Q, K) * tril * z[..., None]
    t_out = (w[..., None] * v[:, :, None]).pow(2).sum((3, 4)).sqrt()                 # terms [i][j][m]
    t_dv = (w[..., None] * dout[:, :, :, None]).pow(2).sum((2, 4)).sqrt()
    gv = torch.einsum("nhim,nhjm->nhij", dout, v) * z[..., None] * tril
    cc = (gv + dden[..., None]) * tril
    t_dk = (cc[..., None] * Q[:, :, :, None] * dphi(k)[:, :, None]).pow(2).sum((2, 4)).sqrt()
    num = (gv[..., None] * K[:, :, None] * dphi(q)[:, :, :, None]).pow(2).sum((3, 4))
    nrm = (dphi(q) * K.cumsum(2) * dden[..., None]).pow(2).sum(-1)
    return {n: t.permute(0, 2, 1) for n, t in (("out", t_out), ("dq", (num + nrm).sqrt()), ("dk", t_dk), ("dv", t_dv))}


# ----------------------------------------------------------------------------------------------------------------------
# measures
# ----------------------------------------------------------------------------------------------------------------------
def row_ratio(got, ref_rows, den):
    """(N, L, H): |got - ref| / den, den = max(|ref row|, T_row) (analyse); 0 where the error is 0 (rows that are exactly
    zero in both have den = 0)."""
    err = (got.double() - ref_rows).norm(dim=-1)
    return torch.where(err == 0, torch.zeros_like(err), err / den.clamp_min(1e-300))


# ----------------------------------------------------------------------------------------------------------------------
# emulation of the bf16 roundings, and of kernels with one wrong ingredient
# ----------------------------------------------------------------------------------------------------------------------
def emulate_mfma(q, k, v, dout, form="pair", eps=EPS, r=rb, mutant=None, segments=1):
    """f64 arithmetic with the MFMA kernels' bf16 roundings (`r`; r = identity gives the exact chunked scan, which is how
    the mutants are built).  form: "pair" | "sweep".  -> dict out, zinv, dden, dq, dk, dv (package layout), fin_S, fin_z,
    cs (3, N, H, 64): what the kernels' column sums add up, per sequence.
    mutant: None | "diag" (score-tile diagonal dropped from chunk 2 on) | "stale" (state one chunk stale from chunk 4 on)
    | "seg" (with `segments` = P: segment 2 of the forward scans starts from the state segment 1 started from)."""
    q, k, v, dout = (_s(t.double()) for t in (q, k, v, dout))
    N, H, L, _ = q.shape
    dev = q.device
    Qr, Kr = r(phi(q)), r(phi(k))
    nch = (L + C - 1) // C
    cps = -(-nch // segments)
    sl = [slice(c * C, min(L, (c + 1) * C)) for c in range(nch)]
    tri = lambda n, c: torch.tril(torch.ones(n, n, dtype=torch.float64, device=dev), -1 if mutant == "diag" and c >= 2 else 0)
    z64 = lambda *s: torch.zeros(N, H, *s, dtype=torch.float64, device=dev)

    def stale(hist, c):
        """The state in front of chunk c out of hist[c] (the list of states in scan order)."""
        if mutant == "stale" and c >= 4:
            return hist[c - 1]
        if mutant == "seg" and c // cps == 2:
            return hist[c] - hist[2 * cps] + hist[cps]             # segment 2 run from segment 1's start state
        return hist[c]

    out, zinv = z64(L, 64), z64(L)
    S, ks, hS, hk = z64(64, 64), z64(64), [], []                    # S[e][m]
    for c, i in enumerate(sl):
        hS.append(S)
        hk.append(ks)
        S0, k0 = stale(hS, c), stale(hk, c)
        At = r(torch.einsum("nhie,nhje->nhij", Qr[:, :, i], Kr[:, :, i]) * tri(i.stop - i.start, c))
        num = At @ v[:, :, i] + Qr[:, :, i] @ r(S0)
        den = At.sum(-1) + torch.einsum("nhie,nhe->nhi", Qr[:, :, i], r(k0)) + eps
        zinv[:, :, i] = 1.0 / den
        out[:, :, i] = r(num / den[..., None])
        S = S + Kr[:, :, i].transpose(2, 3) @ v[:, :, i]
        ks = ks + Kr[:, :, i].sum(2)
    fin_S, fin_z = S, ks
    g = r(dout * zinv[..., None])
    dden = -(dout * out).sum(-1) * zinv
    sweep = form == "sweep"
    dq, dk, dv = z64(L, 64), z64(L, 64), z64(L, 64)
    cs = torch.zeros(3, N, H, 64, dtype=torch.float64, device=dev)
    # reverse scan: dk, dv
    R, r1, hR, h1 = z64(64, 64), z64(64), {}, {}                    # R[e][m]
    for c in range(nch - 1, -1, -1):
        i = sl[c]
        hR[c], h1[c] = R, r1
        if mutant == "stale" and c + 1 < nch and c >= 4:
            R0, r10 = hR[c + 1], h1[c + 1]
        else:
            R0, r10 = R, r1
        m = tri(i.stop - i.start, c)
        W = r((g[:, :, i] @ v[:, :, i].transpose(2, 3) + r(dden[:, :, i])[..., None]) * m)          # [i][j]
        At = r(torch.einsum("nhie,nhje->nhij", Qr[:, :, i], Kr[:, :, i]) * m)
        dkf = W.transpose(2, 3) @ Qr[:, :, i] + v[:, :, i] @ r(R0).transpose(2, 3) + r(r10)[:, :, None]
        x = (dkf if sweep else r(dkf)) * Kr[:, :, i].clamp(max=1.0)
        dk[:, :, i] = r(x)
        dv[:, :, i] = r(At.transpose(2, 3) @ g[:, :, i] + Kr[:, :, i] @ r(R0))
        cs[1] += (dk[:, :, i] if sweep else x).sum(2)
        cs[2] += dv[:, :, i].sum(2)
        R = R + Qr[:, :, i].transpose(2, 3) @ g[:, :, i]
        r1 = r1 + torch.einsum("nhie,nhi->nhe", Qr[:, :, i], dden[:, :, i])
    # forward scan: dq
    for c, i in enumerate(sl):
        S0, k0 = stale(hS, c), stale(hk, c)
        dd = dden[:, :, i]
        W = r((g[:, :, i] @ v[:, :, i].transpose(2, 3) + (r(dd) if sweep else dd)[..., None]) * tri(i.stop - i.start, c))
        dqf = W @ Kr[:, :, i] + g[:, :, i] @ r(S0).transpose(2, 3) + r(k0)[:, :, None] * r(dd)[..., None]
        x = dqf * (Qr[:, :, i].clamp(max=1.0) if sweep else dphi(q[:, :, i]))
        dq[:, :, i] = r(x)
        cs[0] += (dq[:, :, i] if sweep else x).sum(2)
    return {"out": _s(out), "zinv": zinv.permute(0, 2, 1), "dden": dden.permute(0, 2, 1), "dq": _s(dq), "dk": _s(dk),
            "dv": _s(dv), "fin_S": fin_S.transpose(2, 3), "fin_z": fin_z, "cs": cs}


def mutant_reference(q, k, v, dout, mutant, eps=EPS, segments=1):
    """The reference with one wrong ingredient (no roundings): "diag", "stale", "seg" (emulate_mfma), "eps0" (eps = 0),
    "tail" (dk and dv of the last 32 rows zero)."""
    ident = lambda x: x
    if mutant == "eps0":
        return emulate_mfma(q, k, v, dout, "sweep", 0.0, ident)
    if mutant == "tail":
        res = emulate_mfma(q, k, v, dout, "sweep", eps, ident)
        res["dk"][:, -32:] = 0
        res["dv"][:, -32:] = 0
        return res
    return emulate_mfma(q, k, v, dout, "sweep", eps, ident, mutant=mutant, segments=segments)


def make_inputs(kind, N, L, H, seed, dtype=torch.bfloat16):
    """q, k, v, dout (N, L, H, 64) as `dtype` values (CPU): "randn"; "x3" (q, k = 3 randn: a few keys dominate, phi spans
    0.05 to 10); "vmean" (x3 with v of mean 1: out rows do not cancel); "eps" (k = -20 on the first 5 tokens: their
    denominators are below eps).  Every sequence of the batch is drawn separately."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, d = (torch.randn(N, L, H, 64, generator=g) for _ in range(4))
    if kind in ("x3", "vmean"):
        q, k = 3 * q, 3 * k
    if kind == "vmean":
        v = v + 1
    if kind == "eps":
        k[:, :5] = -20.0
    return tuple(t.to(dtype) for t in (q, k, v, d))


MUTANTS = [  # mutant, input, (N, L, H), segments, the tensors it is asked on, the rows it feeds
    # the dropped diagonal is not asked on dq: one token's term of a row that sums 130 .. 200 of them is 1 to 2 x the
    # bound there (rms 1.8 x); out, dk and dv resolve it
    ("diag", "randn", (1, 200, 2), 1, ("out", "dk", "dv"), slice(128, 200)),
    ("stale", "randn", (1, 576, 1), 1, ("out", "dq", "dk", "dv"), slice(256, 512)),
    ("eps0", "eps", (1, 65, 1), 1, ("out",), slice(0, 5)),
    ("tail", "randn", (1, 1024, 2), 1, ("dk", "dv"), slice(992, 1024)),
    ("seg", "randn", (1, 576, 1), 3, ("out", "dq"), slice(384, 576)),
]


def teeth(got, mutant, den, bound, rows):
    """rms over `rows` (a slice of tokens) of the miss |got - mutant| / den in units of the bound."""
    r = row_ratio(got, mutant, den) / bound
    return r[:, rows].pow(2).mean().sqrt().item()

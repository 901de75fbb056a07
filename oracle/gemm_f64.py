"""The bf16 GEMM family (csrc/gemm_bf16.hip, gemm_nt.hip, gemm_ln.hip, gemm_small.hip, wgrad.hip) in f64 (TEST
INFRASTRUCTURE; see oracle/__init__.py): the references, input makers, measures and error bounds of
tests/test_gemm_f64_gpu.py, pinned by tests/test_oracle_gemm_f64_cpu.py.  Plain torch, any device, none of the project's
kernels.  Every comparison is PER ELEMENT (per row for the LayerNorm epilogue): a tolerance set by the largest element of a
matrix cannot see an error that is small beside that element.

Forms.  a (M, K), w (N, K), c0 (M, N), gd (M, N), x (M, N) bf16; bias, gamma, beta (N) f32.  Every reference starts from the
exact bf16 / f32 operand values in f64; prod = a w^T.
    plain     c = prod [+ c0] [+ bias]                                       one rounding to bf16
    EPI_MUL   c = bf16(prod) * gd                                            (two roundings: the product, then c)
              colsum_n = sum_r bf16(prod)_rn gd_rn                           the UNROUNDED products of the two bf16 factors
    EPI_GELU  pre = bf16(prod) + bias;  g = keep scale gelu(pre);  gd = keep scale gelu'(pre);  gelu(x) = x Phi(x) (exact erf)
    LN        o = bf16(prod) + bias;  s = x + keep scale o;  mean, rstd of the UNROUNDED s over the N = 512 columns;
              y = (s - mean) rstd gamma + beta  (from the unrounded s; s and y are each rounded once on their way out)
    wgrad     out (N1, N2) f32 [+]= A^T B
keep is the dropout stream keyed by (seed, row * N + column): the tests take it from ops.posenc_dropout(ones, None, 1, p, seed)
!= 0 (the same stream), never from the output under test; scale = drop_scale(p) = 65536 / (65536 - t), t = round(65536 p)
clamped to 1 .. 65535, as an f32 value: the reciprocal of the keep probability the stream's 16-bit threshold really has
(csrc/cwlt_common.h: drop_thresh, drop_scale).  CORRECTED after the first GPU run: with 1 / (1 - p), which differs from it by
up to 2^-17 relative (7.2e-6 at p = 0.1), the LayerNorm epilogue's s sat at 45 x its bound where x cancels scale o (the
bound there is u-sized, not 2^-8 |s|-sized), rstd at 3.7 x and mean at 1.4 x; every p = 0 case and every other kernel was
inside.  The kernel is right: its scale is the one that makes its own stream unbiased.

Bounds.  u = 2^-24 per f32 operation, errors independent, a serial sum of n terms counts n / 6 (relative to the sum of
|terms|), a level of a reduction tree counts 1, the bound 4 x the predicted rms; every result that is ONE round-to-nearest to
bf16 gets the hard half-ulp 2^-8 max(|ref|, |got|) on top.  The product of two bf16 values is exact in f32 (8 + 8 significant
bits), so only additions round.  With S = |a| |w|^T [+ |c0|] [+ |bias|] (f64, absolute values) per element:

    plain:   |got - ref| <= 2^-8 max(|ref|, |got|) + delta,    delta = 4 u sqrt(n) S

n, read off each kernel's summation order (an MFMA is counted as a balanced tree over its k products -- 5 levels for
v_mfma_f32_16x16x32_bf16, 4 for v_mfma_f32_32x32x16_bf16 -- plus the chain of the accumulator through the K / k MFMAs; the
hardware is not documented to do worse, and doing better only leaves slack):
    gemm_bf16_kernel (256 x 256, BK = 64, GB_MFMA4: two 16x16x32 per K-tile and accumulator)   (K / 32) / 6 + 5
        epilogue `v += c0` then `v += bias`: + 1 each
    gemm_small_kernel (whole K, one 16x16x32 per k-step of 32)                                   (K / 32) / 6 + 5, + 1 each
    gemm_small_splitk_kernel / _splitk64_kernel (wave w: k-steps [w K / 128, (w + 1) K / 128), then
        (red0 + red1) + (red2 + red3) through LDS: two tree levels)                              (K / 128) / 6 + 5 + 2, + 1 each
    gemm_nt_mul_kernel, gemm_ln_kernel (BK = 32, two 32x32x16 per step and accumulator)         (K / 16) / 6 + 4
    wgrad_kernel / wgrad_group_kernel (a slice of mslice rows in steps of 32 = two 32x32x16)    (mslice / 16) / 6 + 4
        wgrad_reduce_kernel: the S partials added serially: + S / 6; accumulate: + 1
        S = cwlt_wgrad_splits(M, N1, N2) and mslice as cwlt_wgrad_bf16 cuts them (restated below: wgrad_splits, wgrad_slices)
    The weight gradients are f32: no bf16 term, |got - ref| <= 4 u sqrt(n) (|A|^T |B| [+ |out0|]).
The provisional n = K / 192 + 8 of the issue is replaced by these (K / 192 + 5 .. 7 for the 256 x 256 kernel).

Inner rounding of the product (MUL, GELU, LN).  The kernel rounds its f32 accumulator q' = prod + e, |e| <= delta, to bf16.
r0 = bf16(prod), r1 = the bf16 neighbour of r0 on prod's side.  Three cases per element:
    no rounding boundary (a midpoint of two bf16 neighbours) within delta of prod:   the kernel's value is r0: compared with
        the reference built from r0;
    one boundary within delta (`amb`):   r0 or r1: the element passes if it meets its bound against EITHER reference;
    delta >= a quarter of the bf16 spacing at prod (`wide`: products that cancel, |prod| <~ 1e-3 S):  several boundaries may
        lie inside [prod - delta, prod + delta]; then |q - r0| <= |q - q'| + |q' - prod| + |prod - r0| <= delta + 2 . 2^-8
        (|prod| + delta) =: slack, which enters the element's bound through the epilogue's derivative (|gd| for MUL,
        scale max|gelu'| = 1.13 scale and scale max|gelu''| = 0.8 scale for GELU, keep scale for LN).
No element is skipped.

    EPI_MUL c:   r_k gd is exact in f32 (two bf16 factors), so c is one rounding of it:
                 |got - r_k gd| <= 2^-8 max(|r_k gd|, |got|) + |gd| slack      for k = 0 or (amb) 1
    colsum:      reference sum_r r0 gd; bound 4 u sqrt(n_cs) sum_r |r0 gd| + sum_r |gd| (amb ? |r1 - r0| : 0) + sum_r |gd| slack
                 n_cs: the terms are exact; 128 x 256 kernel: a thread's 8 rows serially (8 / 6), the 16 row groups of `red`
                 serially (16 / 6); 256 x 256 kernel: 8 rows per lane (8 / 6), four DPP levels (4), the two row halves (1);
                 then colsum_finalize_kernel over nb row tiles as counted in heads_rl_f64.py: ceil(nb / 256) / 6 + 4 + 16 / 6.
    EPI_GELU:    pre = r_k + bias is one f32 rounding (u |pre|, hard); the bf16 GELU of cwlt_gelu.h is within GELU_ABS = 1.5e-4
                 absolute of the exact-erf value and derivative in f32 arithmetic (include/cwlt.h), times scale:
                 |g - ref|  <= 2^-8 max(|ref|, |g|)  + scale (1.5e-4 + 1.13 (u |pre| + slack))
                 |gd - ref| <= 2^-8 max(|ref|, |gd|) + scale (1.5e-4 + 0.8  (u |pre| + slack));  dropped elements exactly 0.
    LN:          per element E = u (2 scale |o| + |s|) (the add of the bias, the product with scale, the add of x; hard)
                 + keep scale slack;  flip = keep scale |r1 - r0| where amb, else 0.
                 s:     |got - s_k| <= 2^-8 max(|s_k|, |got|) + E              k = 0 or (amb) 1;  dropped: s == x exactly
                 mean:  a lane's 8 values serially (8 / 6), six butterfly levels, the product with 1 / N:
                        |mean - ref| <= 4 u sqrt(8 / 6 + 7) mean_j |s| + mean_j (E + flip)
                 rstd:  var = sum d^2 / N, d = s - mean (one rounding each, squared: 2), fma chain of 8 (8 / 6), six levels, the
                        product with 1 / N, + eps, rsqrtf at 2 ulp (4): n_var = 8 / 6 + 6 + 2 + 1 + 1 + 4; the elements' own
                        errors move var by 2 sum |d| (E + flip + dmean) / N and rstd by half of that, relatively:
                        |rstd - ref| <= rstd (4 u sqrt(n_var) + sum_j |d_j| (E_j + flip_j + dmean) / (N (var + eps)))
                 y:     (s - mean) rstd gamma + beta: three more f32 roundings of at most |y - beta| and one of |y| (hard):
                        |y - ref| <= 2^-8 max(|ref|, |y|) + |gamma| (rstd (E + flip + dmean) + |d| drstd) + u (3 |y - beta| + |y|)
                 The measure is per row: the largest ratio over the row's 512 columns.
Exact zeros stay asserted exactly: dropped elements, everything outside an output view or outside [0, N) of a strided c
(the tests compare those regions with torch.equal).
Measured on an MI355X: profiles/gemm_f64_ratios.txt.
"""
import math

import torch

U32 = 2.0 ** -24
HALF = 2.0 ** -8
GELU_ABS = 1.5e-4
GELU_D1 = 1.13           # max |gelu'|  (1.1289 at x = 1.41)
GELU_D2 = 0.8            # max |gelu''| (2 phi(0) = 0.798)
LN_EPS = 1e-5
FORMS = ((False, False), (True, False), (False, True), (True, True))     # (bias, accumulate)


# the case lists of tests/test_gemm_f64_gpu.py (the CPU pin walks the same (N, K))
BIG_M, BIG_N, BIG_K = (1, 127, 129, 255, 256, 257, 513), (8, 248, 256, 264, 520), (128, 192, 256, 320, 576)
NT_M, NT_N, NT_K, NT_P = (1, 127, 128, 129, 1025), (256, 768), (64, 192, 512), (0.0, 0.1)
FFN_BIG_M, FFN_BIG_K = (1, 255, 257, 600), (128, 192, 512)
LN_M, LN_K, LN_N = (1, 127, 128, 129, 300), (64, 128, 192, 2048), 512
SMALL_K, SMALL_M, SMALL_N = (32, 96, 128, 256, 384, 512, 768, 1024, 1536), (1, 31, 32, 33, 255, 256, 257), (8, 24, 40, 64, 72)
SMALL_GELU_K = (128, 256, 512, 1024)
WG_M, WG_WIDTHS = (1, 31, 33, 255, 257, 2561, 4097), ((8, 8), (256, 256), (264, 8), (248, 520), (512, 256))


def big_cases():
    """40 (M, N, K, bias, accumulate) of the 256 x 256 kernel: every value of every axis meets every form at least once."""
    out = []
    for f, (bias, acc) in enumerate(FORMS):
        for i in range(10):
            out.append((BIG_M[i % 7], BIG_N[(i + f) % 5], BIG_K[(2 * i + f) % 5], bias, acc))
    return out


def drop_scale(p):
    """csrc/cwlt_common.h drop_scale restated: the f32 value of 1 / (keep probability of the 16-bit threshold)."""
    if p <= 0:
        return 1.0
    t = min(max(int(p * 65536.0 + 0.5), 1), 65535)
    return float(torch.tensor(65536.0 / (65536.0 - t), dtype=torch.float32))


def form_name(bias, acc):
    return ("bias" if bias else "plain") + ("+acc" if acc else "")


# ----------------------------------------------------------------------------------------------------------------------
# inputs (CPU tensors; a and w may be column blocks of wider tensors: lda / ldw are their row strides)
# ----------------------------------------------------------------------------------------------------------------------
def make_operands(M, N, K, seed, lda=None, ldw=None):
    """The maker of tests/test_gemm_bf16_gpu.py: randn a, w x 2 / sqrt(K), bias x 0.3 (f32), randn c0 (bf16).  The outputs
    spread over several binades."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, lda or K, generator=g).bfloat16()[:, :K]
    w = (torch.randn(N, ldw or K, generator=g) * (2.0 / K ** 0.5)).bfloat16()[:, :K]
    bias = torch.randn(N, generator=g) * 0.3
    c0 = torch.randn(M, N, generator=g).bfloat16()
    return a, w, bias, c0


def make_cancelling(M, N, K, seed):
    """Rows whose product is far smaller than sum_k |a_k w_k|: the second half of a row of `a` is minus its first half, the
    second half of a row of `w` its first half times (1 + randn / 64) before the rounding to bf16."""
    g = torch.Generator().manual_seed(seed)
    h = K // 2
    a1 = torch.randn(M, h, generator=g).bfloat16()
    w1 = torch.randn(N, h, generator=g) * (2.0 / K ** 0.5)
    w2 = w1 * (1 + torch.randn(N, h, generator=g) / 64)
    a = torch.cat([a1, -a1], 1).contiguous()
    w = torch.cat([w1, w2], 1).bfloat16().contiguous()
    bias = torch.randn(N, generator=g) * 0.01
    c0 = (torch.randn(M, N, generator=g) * 0.01).bfloat16()
    return a, w, bias, c0


def make_integers(M, N, K, seed):
    """The maker of test_exact_integers_and_an_asymmetric_weight: integers in [-3, 3], column 0 of w depends on the row:
    every product and sum is exact, results up to 256 are exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-3, 4, (N, K), generator=g).float()
    w[:, 0] = torch.arange(N).float() % 7 - 3
    return a.bfloat16(), w.bfloat16()


def make_gd(M, N, seed, p=0.0):
    """A factor like the forward's gd = keep scale gelu'(.): bf16 values in about [-0.2, 1.2 scale], a share p exactly 0."""
    g = torch.Generator().manual_seed(seed)
    gd = (torch.rand(M, N, generator=g) * 1.3 - 0.15) / (1 - p)
    if p > 0:
        gd = gd * (torch.rand(M, N, generator=g) >= p)
    return gd.bfloat16()


def make_ln(M, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g).bfloat16()
    return x, torch.randn(N, generator=g), torch.randn(N, generator=g)


def make_wgrad(M, N1, N2, seed, strided=False):
    """a (M, N1), b (M, N2) bf16 randn; strided: column slices of wider tensors (16-byte aligned starts), the neighbouring
    columns filled with 100 so that a leak shows."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, N1, generator=g).bfloat16()
    b = torch.randn(M, N2, generator=g).bfloat16()
    if strided:
        wa = torch.full((M, N1 + 24), 100.0).bfloat16()
        wb = torch.full((M, N2 + 72), 100.0).bfloat16()
        wa[:, 8:8 + N1] = a
        wb[:, 64:64 + N2] = b
        a, b = wa[:, 8:8 + N1], wb[:, 64:64 + N2]
    return a, b


# ----------------------------------------------------------------------------------------------------------------------
# operation counts
# ----------------------------------------------------------------------------------------------------------------------
def n_big(K, bias=False, acc=False):
    return K / 32 / 6 + 5 + bool(bias) + bool(acc)


def small_splitk(M, K, splitk=True):
    """Whether cwlt_gemm_bf16_small takes a split-K kernel (its own dispatch condition)."""
    return bool(splitk) and K % 128 == 0 and M <= 16384


def n_small(M, K, bias=False, acc=False, splitk=True):
    if small_splitk(M, K, splitk):
        return K / 128 / 6 + 5 + 2 + bool(bias) + bool(acc)
    return K / 32 / 6 + 5 + bool(bias) + bool(acc)


def n_small_gelu(K):
    return K / 128 / 6 + 5 + 2


def n_nt(K):
    return K / 16 / 6 + 4


def n_finalize(nb):
    return math.ceil(nb / 256) / 6 + 4 + 16 / 6


def n_colsum(M, big=False):
    if big:
        return 8 / 6 + 4 + 1 + n_finalize((M + 255) // 256)
    return 8 / 6 + 16 / 6 + n_finalize((M + 127) // 128)


def wgrad_splits(M, N1, N2):
    """cwlt_wgrad_splits restated."""
    tiles = ((N1 + 255) // 256) * ((N2 + 255) // 256)
    s = 256 // tiles // 8 * 8
    s = min(max(s, 8), 128)
    return min(s, max(M // 256, 1))


def wgrad_slices(M, N1, N2):
    """(S, rows per slice) as cwlt_wgrad_bf16 cuts the token rows."""
    S = wgrad_splits(M, N1, N2)
    ms = -(-M // S)
    return S, -(-ms // 32) * 32


def n_wgrad(M, N1, N2, acc=False):
    S, ms = wgrad_slices(M, N1, N2)
    return ms / 16 / 6 + 4 + S / 6 + bool(acc)


# ----------------------------------------------------------------------------------------------------------------------
# references and measures
# ----------------------------------------------------------------------------------------------------------------------
def product(a, w):
    """(a w^T, |a| |w|^T) in f64 from the exact bf16 values."""
    ad, wd = a.double(), w.double()
    return ad @ wd.t(), ad.abs() @ wd.abs().t()


def plain_reference(a, w, bias=None, c0=None):
    ref, S = product(a, w)
    if c0 is not None:
        ref, S = ref + c0.double(), S + c0.double().abs()
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    return ref, S


def _ratio(err, bound):
    """err / bound, 0 where both are 0 (an exact result with nothing to round), inf where only the bound is."""
    r = err / bound.clamp_min(1e-300)
    return torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r)


def plain_ratios(got, ref, S, n):
    """Per element |got - ref| / (2^-8 max(|ref|, |got|) + 4 u sqrt(n) S)."""
    got = got.double().cpu()
    return _ratio((got - ref).abs(), HALF * torch.maximum(ref.abs(), got.abs()) + 4 * U32 * math.sqrt(n) * S)


def f32_ratios(got, ref, S, n):
    """Per element |got - ref| / (4 u sqrt(n) S): f32 results (the weight gradients)."""
    return _ratio((got.double().cpu() - ref).abs(), 4 * U32 * math.sqrt(n) * S)


def wgrad_reference(a, b, out0=None):
    ad, bd = a.double(), b.double()
    ref, S = ad.t() @ bd, ad.abs().t() @ bd.abs()
    if out0 is not None:
        ref, S = ref + out0.double(), S + out0.double().abs()
    return ref, S


def bf16_step(r, away):
    """The bf16 neighbour of the (nonzero) bf16 values r, away from zero where `away`, else towards it.  f64 tensors."""
    m, e = torch.frexp(r.abs())                        # |r| = m 2^e, m in [0.5, 1): spacing above 2^(e - 8)
    ulp = torch.ldexp(torch.ones_like(m), e - 8)
    down = torch.where(m == 0.5, ulp / 2, ulp)         # the spacing below a power of two is half of the one above
    return torch.sign(r) * (r.abs() + torch.where(away, ulp, -down))


def bf16_neighbours(prod, delta):
    """r0 = bf16(prod), r1 = its bf16 neighbour on prod's side where `amb` (one rounding boundary within delta of prod), else
    r0, and slack (0, or for `wide` elements the distance the kernel's rounded product may lie from r0).  f64 tensors."""
    r0 = prod.float().bfloat16().double()
    zero = r0 == 0
    nb = torch.where(zero | (prod == r0), r0, bf16_step(r0, prod.abs() > r0.abs()))
    gap = (nb - r0).abs()
    spacing = torch.where(gap > 0, gap, (bf16_step(r0, torch.zeros_like(zero)) - r0).abs())
    wide = zero | (delta >= spacing / 4)
    amb = (~wide) & (gap > 0) & ((prod - (r0 + nb) / 2).abs() <= delta)
    slack = torch.where(wide, delta + 2 * HALF * (prod.abs() + delta), torch.zeros_like(prod))
    slack = torch.where(zero & (prod == 0) & (delta == 0), torch.zeros_like(prod), slack)
    return r0, torch.where(amb, nb, r0), amb, slack


def _best(got, refs, bound_of):
    """The smaller of the ratios against the candidate references."""
    out = None
    for ref in refs:
        r = _ratio((got - ref).abs(), bound_of(ref))
        out = r if out is None else torch.minimum(out, r)
    return out


def mul_ratios(got_c, got_cs, a, w, gd, n, n_cs):
    """EPI_MUL: per-element ratios of c and per-column ratios of the column sums (None when not wanted)."""
    prod, S = product(a, w)
    delta = 4 * U32 * math.sqrt(n) * S
    r0, r1, amb, slack = bf16_neighbours(prod, delta)
    g = gd.double()
    got = got_c.double().cpu()
    rc = _best(got, (r0 * g, r1 * g), lambda ref: HALF * torch.maximum(ref.abs(), got.abs()) + g.abs() * slack)
    rs = None
    if got_cs is not None:
        ref = (r0 * g).sum(0)
        bound = (4 * U32 * math.sqrt(n_cs) * (r0 * g).abs().sum(0) + (g.abs() * (r1 - r0).abs()).sum(0)
                 + (g.abs() * slack).sum(0))
        rs = _ratio((got_cs.double().cpu() - ref).abs(), bound)
    return rc, rs


def gelu64(x):
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return x * cdf, cdf + x * pdf


def gelu_ratios(got_g, got_gd, a, w, bias, keep, scale, n):
    """EPI_GELU: per-element ratios of g and gd (None when not wanted); inf where a dropped element is not exactly 0."""
    prod, S = product(a, w)
    delta = 4 * U32 * math.sqrt(n) * S
    r0, r1, amb, slack = bf16_neighbours(prod, delta)
    kd = keep.double()
    out = []
    for got, which, d in ((got_g, 0, GELU_D1), (got_gd, 1, GELU_D2)):
        if got is None:
            out.append(None)
            continue
        got = got.double().cpu()
        refs, pres = [], []
        for r in (r0, r1):
            pre = r + bias.double()
            refs.append(kd * scale * gelu64(pre)[which])
            pres.append(pre)
        best = None
        for ref, pre in zip(refs, pres):
            bound = HALF * torch.maximum(ref.abs(), got.abs()) + kd * scale * (GELU_ABS + d * (U32 * pre.abs() + slack))
            r = _ratio((got - ref).abs(), bound)
            best = r if best is None else torch.minimum(best, r)
        best = torch.where((kd == 0) & (got != 0), torch.full_like(best, float("inf")), best)
        out.append(best)
    return out


def ln_ratios(got_s, got_y, got_mean, got_rstd, a, w, bias, x, gamma, beta, keep, scale, n, eps=LN_EPS):
    """LN epilogue: per-row ratios {s, y, mean, rstd}; s is inf on a row where a dropped element differs from x."""
    prod, S = product(a, w)
    delta = 4 * U32 * math.sqrt(n) * S
    r0, r1, amb, slack = bf16_neighbours(prod, delta)
    kd, xd, N = keep.double(), x.double(), prod.shape[1]
    o0 = r0 + bias.double()
    s0, s1 = xd + kd * scale * o0, xd + kd * scale * (r1 + bias.double())
    E = U32 * (2 * scale * o0.abs() + s0.abs()) + kd * scale * slack
    flip = kd * scale * (r1 - r0).abs()
    gs = got_s.double().cpu()
    rs = _best(gs, (s0, s1), lambda ref: HALF * torch.maximum(ref.abs(), gs.abs()) + E)
    rs = torch.where((kd == 0) & (gs != xd), torch.full_like(rs, float("inf")), rs)
    mean = s0.mean(1)
    dmean = 4 * U32 * math.sqrt(8 / 6 + 7) * s0.abs().mean(1) + (E + flip).mean(1)
    d = s0 - mean[:, None]
    var = (d * d).mean(1)
    rstd = 1 / torch.sqrt(var + eps)
    n_var = 8 / 6 + 6 + 2 + 1 + 1 + 4
    drstd = rstd * (4 * U32 * math.sqrt(n_var) + (d.abs() * (E + flip + dmean[:, None])).sum(1) / (N * (var + eps)))
    gm, bt = gamma.double(), beta.double()
    y = d * rstd[:, None] * gm + bt
    gy = got_y.double().cpu()
    by = (HALF * torch.maximum(y.abs(), gy.abs()) + gm.abs() * (rstd[:, None] * (E + flip + dmean[:, None])
                                                                  + d.abs() * drstd[:, None])
          + U32 * (3 * (y - bt).abs() + y.abs()))
    return {"s": rs.max(1).values, "y": _ratio((gy - y).abs(), by).max(1).values,
            "mean": _ratio((got_mean.double().cpu() - mean).abs(), dmean),
            "rstd": _ratio((got_rstd.double().cpu() - rstd).abs(), drstd)}


def worst(r):
    """The largest ratio of a tensor (0 for an empty one; nan counts as inf)."""
    if r is None or r.numel() == 0:
        return 0.0
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))
    return float(r.max())


# ----------------------------------------------------------------------------------------------------------------------
# f32 emulations of the kernels' arithmetic on the CPU (the stand-ins of the CPU pin, and its mutants' starting point)
# ----------------------------------------------------------------------------------------------------------------------
def emulate_plain(a, w, bias=None, c0=None, mutate=None):
    """f32 product, `+= c0`, `+= bias`, one rounding to bf16.  mutate: bias_bf16 | splitk_bf16 | double_round | drop_k |
    c0_row | bias_col."""
    af, wf = a.float(), w.float()
    K = af.shape[1]
    if mutate == "drop_k":
        acc = af[:, :K - 1] @ wf[:, :K - 1].t()
    elif mutate == "splitk_bf16":
        h = K // 2
        acc = (af[:, :h] @ wf[:, :h].t()).bfloat16().float() + af[:, h:] @ wf[:, h:].t()
    else:
        acc = af @ wf.t()
    if c0 is not None:
        c = c0.float()
        if mutate == "c0_row":
            c = torch.roll(c, 1, 0)
        if mutate == "double_round":
            acc = acc.bfloat16().float()
        acc = acc + c
    if bias is not None:
        b = bias.float()
        if mutate == "bias_bf16":
            b = b.bfloat16().float()
        if mutate == "bias_col":
            b = torch.roll(b, 1, 0)
        acc = acc + b
    return acc.bfloat16()


def emulate_mul(a, w, gd, mutate=None):
    """bf16(a w^T) * gd rounded once more, and the f32 column sums of the unrounded products.  mutate: unrounded | drop_k."""
    af, wf = a.float(), w.float()
    if mutate == "drop_k":
        af, wf = af[:, :-1], wf[:, :-1]
    acc = af @ wf.t()
    t = (acc if mutate == "unrounded" else acc.bfloat16().float()) * gd.float()
    return t.bfloat16(), t.sum(0)


def emulate_gelu(a, w, bias, keep, scale):
    pre = (a.float() @ w.float().t()).bfloat16().float() + bias.float()
    g, gd = gelu64(pre.double())
    k = keep.float() * scale
    return (k * g.float()).bfloat16(), (k * gd.float()).bfloat16()


def emulate_ln(a, w, bias, x, gamma, beta, keep, scale, eps=LN_EPS):
    o = (a.float() @ w.float().t()).bfloat16().float() + bias.float()
    s = torch.where(keep, o * scale, torch.zeros_like(o)) + x.float()
    mean = s.mean(1)
    d = s - mean[:, None]
    rstd = torch.rsqrt((d * d).mean(1) + eps)
    y = d * rstd[:, None] * gamma.float() + beta.float()
    return s.bfloat16(), y.bfloat16(), mean, rstd


def emulate_wgrad(a, b, M_slices, out0=None, mutate=None):
    """The slices' f32 partial products added serially.  M_slices = (S, rows per slice).  mutate: drop_step (one 32-row step
    of one slice) | slice_twice."""
    S, ms = M_slices
    af, bf = a.float(), b.float()
    total = None
    for s in range(S):
        lo, hi = s * ms, min(af.shape[0], (s + 1) * ms)
        if hi <= lo:
            part = torch.zeros(af.shape[1], bf.shape[1])
        else:
            if mutate == "drop_step" and s == 0:
                lo = min(lo + 32, hi)
            part = af[lo:hi].t() @ bf[lo:hi]
            if mutate == "slice_twice" and s == 0:
                part = part + part
        total = part if total is None else total + part
    return total + out0.float() if out0 is not None else total

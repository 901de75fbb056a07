"""LayerNorm (csrc/ln.hip), FFN activation / posenc / colsum (csrc/ffn_act.hip, csrc/cwlt_gelu.h) and the un-projected CW
embedding (csrc/embed.hip) in f64 (TEST INFRASTRUCTURE; see oracle/__init__.py): the references, input makers, measures and
error bounds of tests/test_elementwise_f64_gpu.py and tests/test_embed_f64_gpu.py, pinned by
tests/test_oracle_elementwise_f64_cpu.py.  Plain torch, any device, none of the project's kernels.

References start from the exact input values (the bf16 values of bf16 inputs) in f64.  Masks and keep_scale come from
oracle/dropout.py only; its key arithmetic is on Python integers, so a device-resident seed offset is stated as
seed_key(seed, base) = (seed + base) mod 2^64, the uint64 sum the kernels form.  eps is a `float` in the C ABI: the
reference uses its f32 value.

    s = x + dropout(a);  mean = sum s / D;  var = sum (s - mean)^2 / D (biased);  rstd = 1 / sqrt(var + eps)
    y = (s - mean) rstd gamma + beta
    backward, on the STORED s, mean, rstd:  g = dy [+ dy2];  xh = (s - mean) rstd;  dx = g gamma;  m1 = mean dx;
        m2 = mean dx xh;  ds = rstd (dx - m1 - xh m2);  da = mask ks ds;  dgamma = colsum g xh;  dbeta = colsum g;
        dbias = colsum da
    x = h + b;  g = mask ks x Phi(x);  gd = mask ks (Phi(x) + x phi(x))  (exact erf);  dh = dg gd;  db1 = colsum dh
    posenc: mask ks (x + pe[r % T]);   embedding: table_f[clamp(id)] sqrt(w_f), concatenated; table gradients by index_add

Bounds.  u = 2^-24 per f32 operation, U = 2^-9 / sqrt(3) rms per bf16 rounding, errors independent, a serial sum of n terms
counts n / 6 (relative to the sum of |terms|), a level of a reduction tree counts 1, adding to an exact zero does not round,
the bound 4 x the predicted rms.  A quantity whose count is 0 must be exact.  Counts, read off the source:

  row sums (wave per row).  A lane adds its ceil(nchunk / 64) * V elements serially, then a 6-level butterfly (fewer when
      fewer than 64 lanes hold a chunk): cnt = ceil(nchunk / 64) V / 6 + ceil(log2 min(64, nchunk)).
  s.  a * ks: two roundings (ks itself is an f32 constant) when p > 0; + x one rounding of |s|:  es2 = 2 (a ks)^2 + s^2.
  mean.  the row sum, 1 / D rounded and the product: var = u^2 ((cnt + 2) (sum |s|)^2 + sum es2) / D^2.
  rstd.  d_i = s_i - mean one rounding, squared (2 d_i delta d_i), fma-accumulated, * 1 / D (2), + eps (1), v_rsq_f32 (1 ulp: 1):
      relative var = 1/4 (4 sum d^4 + 4 sum d^2 es2 + (cnt + 3) (sum d^2)^2) / (D (var + eps))^2 + 1, and the error of the
      mean enters squared (sum d_i = 0): + 1/2 bound(mean)^2 / (var + eps), added linearly (a bias).
  y.  gamma^2 rstd^2 (es2 + var(mean) + d^2) + (xh gamma)^2 (2 + relvar(rstd)) + y^2 [+ U^2 y^2].  The first term carries the
      |mean| / std amplification of a residual stream: the error of s_i and of the mean is relative to |s|, the result to d.
  ds.  g = dy + dy2 (n_g = 1 if dy2), dx = g gamma (1), xh two roundings, m1 and m2 as the mean (sum of dx, fma sum of
      dx xh): var(o) = rstd^2 ((n_g + 1) dx^2 + var(m1) + xh^2 var(m2) + 3 (xh m2)^2 + 2 (|dx| + |m1| + |xh m2|)^2) + o^2.
      da = o ks from the f32 o: ks^2 var(o) + 2 da^2.
  LayerNorm column sums.  A wave adds trips = ceil(rows / (4 blocks)) rows serially, the four waves in two levels, then
      colsum_finalize over `blocks` partials: per = ceil(blocks / 16) per wave, of which a[0] takes per // 16 + per % 16
      serial adds, a 4-level tree of the 16 chains when per >= 16, and the waves serially.  Terms: g xh (n_g + 2), g (n_g),
      da (its own variance).
  GELU f32.  x = h + b (1 if bias), z = x / sqrt 2 (1), erff 4 ulp (16, of |erf|; the ROCm device library's documented
      figure), 1 + erf (1):  var(Phi) = 1/4 ((erf'(z) z)^2 + 16 erf^2 + (1 + erf)^2);  g: ks^2 ((gelu'(x) x)^2 [bias] + x^2
      var(Phi)) + 3 g^2;  phi = c expf(-x^2 / 2): the argument rounds once (relative x^2 / 2 of phi), expf 2 ulp (4), c (1);
      gd: ks^2 ((gelu''(x) x)^2 [bias] + var(Phi) + (x phi)^2 (x^4 / 4 + 6) + gelu'^2) + 2 gd^2;  dh: dg^2 var(gd) + 2 dh^2.
  GELU bf16 (cwlt_gelu.h).  GELU_APPROX = 1.5e-4 times ks absolute (pinned against the f32 emulation below), the output
      rounding, and y = fma(|x|, us, c0 x): two terms of magnitude ks |x| / 2, the second rounded, which for x < 0 cancel and
      leave that rounding: u^2 ks^2 x^2 (1/4 + [bias]).  (COUNTED, beyond the approximation term and the output rounding: at
      x = -1e6 and ks = 1.1111 the formula returns 0.025 where gelu is -0, up to 2^-25 ks |x|; relative to the uncancelled
      magnitude that is one f32 rounding, and above |x| = 4.5e3 it exceeds GELU_APPROX.)  gd and dh: GELU_APPROX ks [|dg|] + rounding + u^2 ks^2 [dg^2] ((gelu'' x)^2 [bias] + 1).
  db1.  A thread adds per = ceil(rows / slabs) rows serially, then colsum_finalize over the slabs; bf16 terms carry their
      approximation error with one sign at worst: + sum_r |dg| GELU_APPROX ks, linearly.
  posenc.  x + pe (1 if pe), * ks (2 if p > 0) [+ U].     colsum.  Two interleaved chains of per / 2, their sum, finalize.
  embedding forward.  sqrtf(w) and one product: 1 ulp = 2 u |ref| (a hard bound) [bf16: 4 sqrt(U^2 + 2 u^2) |ref|].
  embedding backward.  Terms dout sqrt(w) (2); an id row of a split takes at most min(hits, rows per split) serial f32 adds
      (LDS read-modify-write, or the MFMA accumulator whose one-hot products are exact), then colsum_finalize over the splits.

The GELU domain.  Q(|x|) of cwlt_gelu.h overflows to -inf for |x| above about 1.8e8 while e = 0: NaN.  GELU_BF16_MAX_ABS =
2^26 is the largest magnitude anything here asserts on; outside it nothing is asserted.  gelu_scaled_f32 is the header's
formula in f32 (fma through f64), used by the CPU test only.
Measured on an MI355X: profiles/elementwise_f64_ratios.txt.
"""
import math

import torch

from . import dropout

U16 = 2.0 ** -9 / 3 ** 0.5
U32 = 2.0 ** -24
TEETH = 5.0
LN_EPS = 1e-5
GELU_APPROX = 1.5e-4
GELU_BF16_MAX_ABS = 2.0 ** 26
INF = float("inf")
LN_KINDS = ("randn", "mean100", "tiny", "const", "outlier", "mixed")
REPO_WIDTHS = (128, 256, 64, 512, 128, 128)
REPO_VOCAB = (56, 135, 18, 87, 18, 25)


def f32v(x):
    return float(torch.tensor(x, dtype=torch.float32))


def seed_key(seed, base=0):
    """The kernels' `seed += *seed_base` on uint64 (base may be a signed 64-bit value)."""
    return (int(seed) + int(base)) % (1 << 64)


def keep(seed, p, rows, cols, device=None, base=0, mut=None, row0=0):
    """(rows, cols) keep flags.  Mutants: "shift" (one element pair later), "swap" (the 16-bit halves of a pair exchanged),
    "nobase" (the seed offset ignored)."""
    key = seed_key(seed, 0 if mut == "nobase" else base)
    start = row0 * cols + (2 if mut == "shift" else 0)
    idx = torch.arange(start, start + rows * cols, dtype=torch.int64, device=device).view(rows, cols)
    if mut == "swap":
        idx = idx ^ 1
    return dropout.keep_flags(key, p, idx)


def ratio(got, ref, bound):
    """max |got - ref| / bound over every element; a zero bound demands equality; NaN / inf in `got` is infinite."""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, INF, 0.0).to(err.dtype))
    r = torch.nan_to_num(r, nan=INF, posinf=INF)
    return float(r.max()) if r.numel() else 0.0


def mask_exact(got, ref, bound, mask):
    """Dropped elements are exactly 0 and kept ones are non-zero wherever the reference exceeds its bound."""
    return bool((got[~mask] == 0).all()) and bool((got[mask & (ref.abs() > bound)] != 0).all())


def _z(x):
    return torch.zeros((), dtype=torch.float64, device=x.device)


# ----------------------------------------------------------------------------------------------------------------------
# launch geometry (restated from the launchers)
# ----------------------------------------------------------------------------------------------------------------------
def ln_blocks(rows):
    return max(1, min(1024, (rows + 3) // 4))


def rowslab_blocks(rows):
    return max(1, min(1024, (rows + 15) // 16))


def colsum_blocks(rows):
    return max(1, min(512, (rows + 63) // 64))


def embed_splits(rows):
    return max(1, min(512, (rows + 255) // 256))


def row_sum_count(D, bf):
    V = 8 if bf else 4
    nch = D // V
    return -(-nch // 64) * V / 6.0 + (math.ceil(math.log2(min(64, nch))) if nch > 1 else 0)


def finalize_count(nb):
    per = -(-nb // 16)
    waves = -(-nb // per)
    chain = per // 16 + per % 16
    return (chain / 6.0 if chain > 1 else 0) + (4 if per >= 16 else 0) + (waves / 6.0 if waves > 1 else 0)


def ln_col_count(rows):
    nb = ln_blocks(rows)
    trips = -(-rows // (4 * nb))
    return (trips / 6.0 if trips > 1 else 0) + math.ceil(math.log2(min(4, rows))) + finalize_count(nb)


def slab_col_count(rows, nb, chains=1):
    per = -(-rows // nb)
    link = -(-per // chains)
    return (link / 6.0 if link > 1 else 0) + (1 if chains > 1 and per > 1 else 0) + finalize_count(nb)


def ln_last_block_rows(rows, device=None):
    """bool (rows): the rows the last LayerNorm block handles (row r belongs to block (r // 4) % blocks)."""
    nb = ln_blocks(rows)
    r = torch.arange(rows, device=device)
    return (r // 4) % nb == nb - 1


def last_split_rows(rows, nb, device=None):
    """bool (rows): the rows of the last non-empty contiguous row split of `nb` splits."""
    per = -(-rows // nb)
    last = (rows - 1) // per
    r = torch.arange(rows, device=device)
    return r // per == last


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def make_ln_input(kind, rows, D, dtype=torch.float32, seed=1, residual=True):
    """-> x (or None), a of `dtype` whose sum has the property `kind` names (at p = 0):
    randn     standard normal
    mean100   row mean 100 x the row's std (std 1)
    tiny      std 1e-3, mean 0: var ~ eps / 10
    const     every element of a row the same dyadic value (exact in bf16, variance exactly 0)
    outlier   randn x 1e-3 with one element per row at 1 (1e3 x the rest)
    mixed     randn x (1, 10, 0.1) by row % 3"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, D, generator=g, dtype=torch.float64)
    r = torch.arange(rows)
    if kind == "randn":
        base = z
    elif kind == "mean100":
        base = z + 100.0 * torch.where(r % 2 == 0, 1.0, -1.0).double()[:, None]
    elif kind == "tiny":
        base = z * 1e-3
    elif kind == "const":
        base = (0.5 * (1 + r % 5).double() * torch.where(r % 2 == 0, 1.0, -1.0).double())[:, None].expand(rows, D).clone()
    elif kind == "outlier":
        base = z * 1e-3
        base[r, (r * 7) % D] = 1.0
    elif kind == "mixed":
        base = z * torch.tensor([1.0, 10.0, 0.1], dtype=torch.float64)[r % 3][:, None]
    else:
        raise ValueError(kind)
    if not residual:
        return None, base.to(dtype)
    a = (base * 0.5).to(dtype)
    x = (base - a.double()).to(dtype)
    return x, a


def make_affine(D, seed=2):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.25 * torch.randn(D, generator=g)).float(), (0.25 * torch.randn(D, generator=g)).float()


def gelu_ladder():
    """Magnitudes 1e-4 .. 2^26 in both signs, +-0, and the erf saturation points of test_bias_gelu_bf16_tails_and_zero."""
    mags = [1e-4, 1e-3, 1e-2, 0.1, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 5.5, 6.0, 8.0, 10.0, 12.0, 13.0, 14.0, 20.0, 30.0, 100.0,
            1e3, 4500.0, 1e4, 1e5, 1e6, 2.0 ** 24, 2.0 ** 25, 2.0 ** 26]
    v = [0.0, -0.0] + mags + [-m for m in mags]
    return torch.tensor(v, dtype=torch.float64)


def make_gelu_input(kind, rows, F, dtype=torch.float32, seed=3):
    """randn x 2, or the ladder tiled over the tensor (rotated by row so that every column sees every value)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "randn2":
        return (2 * torch.randn(rows, F, generator=g, dtype=torch.float64)).to(dtype)
    lad = gelu_ladder()
    idx = (torch.arange(rows)[:, None] * 5 + torch.arange(F)[None, :]) % lad.numel()
    return lad[idx].to(dtype)


def make_tables(widths, nrows, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, w, generator=g) for w, n in zip(widths, nrows)]


def make_tokens(rows, nrows, seed=5, oor=False, every=None, never=None):
    """(rows, A) int64 ids.  oor: some ids below 0 and >= n.  every / never: (attribute, id) hit by every / by no row."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.stack([torch.randint(0, n, (rows,), generator=g) for n in nrows], 1)
    if oor:
        r = torch.arange(rows)
        for f, n in enumerate(nrows):
            tok[:, f] = torch.where(r % 7 == f % 7, tok[:, f] - n - 3, tok[:, f])
            tok[:, f] = torch.where(r % 11 == f % 11, tok[:, f] + n + 2, tok[:, f])
    if never is not None:
        f, i = never
        tok[:, f] = torch.where(tok[:, f] == i, (i + 1) % nrows[f], tok[:, f])
    if every is not None:
        tok[:, every[0]] = every[1]
    return tok


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def ln_forward(x, a, gamma, beta, eps=LN_EPS, p=0.0, seed=0, base=0, mut=None):
    """Mutants: "eps6" (eps 1e-6), "unbiased", "mean_undropped", and the mask mutants of keep()."""
    rows, D = a.shape
    a64 = a.double()
    ks = dropout.keep_scale(p)
    m = keep(seed, p, rows, D, a.device, base, mut)
    ad = torch.where(m, a64 * ks, _z(a64))
    x64 = x.double() if x is not None else None
    s = ad + x64 if x is not None else ad
    e = 1e-6 if mut == "eps6" else f32v(eps)
    mean = s.mean(1)
    if mut == "mean_undropped":
        mean = (a64 + x64 if x is not None else a64).mean(1)
    d = s - mean[:, None]
    var = (d * d).sum(1) / (D - 1 if mut == "unbiased" else D)
    rstd = 1.0 / torch.sqrt(var + e)
    y = d * rstd[:, None] * gamma.double() + beta.double()
    return dict(s=s, mean=mean, rstd=rstd, y=y, var=var, mask=m, ks=ks, adrop=ad, eps=e, has_x=x is not None, p=p)


def ln_fwd_bounds(ref, gamma, bf):
    """-> dict of absolute bounds for s, mean, rstd, y (shapes of the quantities)."""
    s, mean, rstd, y, var = ref["s"], ref["mean"], ref["rstd"], ref["y"], ref["var"]
    D = s.shape[1]
    cnt = row_sum_count(D, bf)
    es2 = torch.zeros_like(s)
    if ref["p"] > 0:
        es2 = es2 + 2 * ref["adrop"] ** 2
    if ref["has_x"]:
        es2 = es2 + s * s
    vmu = ((cnt + 2) * s.abs().sum(1) ** 2 + es2.sum(1)) / D ** 2
    b_mean = 4 * U32 * torch.sqrt(vmu)
    d = s - mean[:, None]
    q = var + ref["eps"]
    d2 = d * d
    vrs = 0.25 * (4 * (d2 * d2).sum(1) + 4 * (d2 * es2).sum(1) + (cnt + 3) * d2.sum(1) ** 2) / (D * q) ** 2 + 1
    bias = 0.5 * b_mean ** 2 / q
    b_rstd = (4 * U32 * torch.sqrt(vrs) + bias) * rstd
    gm = gamma.double()
    xg = d * rstd[:, None] * gm
    vy = (gm * rstd[:, None]) ** 2 * (es2 + vmu[:, None] + d2) + xg ** 2 * (2 + vrs[:, None]) + y * y
    b_y = 4 * torch.sqrt(U32 ** 2 * vy + (U16 * y) ** 2 * bf) + xg.abs() * bias[:, None]
    b_s = 4 * torch.sqrt(U32 ** 2 * es2 + (U16 * s) ** 2 * bf)
    return dict(s=b_s, mean=b_mean, rstd=b_rstd, y=b_y)


def ln_backward(dy, dy2, s, gamma, mean, rstd, p=0.0, seed=0, base=0, mut=None, drop_rows=None):
    """On the stored s, mean, rstd.  Mutants: "no_dy2", the mask mutants; drop_rows: rows left out of the column sums."""
    rows, D = s.shape
    g = dy.double()
    if dy2 is not None and mut != "no_dy2":
        g = g + dy2.double()
    rs = rstd.double()[:, None]
    xh = (s.double() - mean.double()[:, None]) * rs
    dx = g * gamma.double()
    m1 = dx.mean(1, keepdim=True)
    m2 = (dx * xh).mean(1, keepdim=True)
    ds = rs * (dx - m1 - xh * m2)
    ks = dropout.keep_scale(p)
    m = keep(seed, p, rows, D, s.device, base, mut)
    da = torch.where(m, ds * ks, _z(ds))
    w = torch.ones(rows, 1, dtype=torch.float64, device=s.device)
    if drop_rows is not None:
        w = (~drop_rows).double()[:, None]
    return dict(ds=ds, da=da, dgamma=(g * xh * w).sum(0), dbeta=(g * w).sum(0), dbias=(da * w).sum(0), g=g, xh=xh, dx=dx,
                m1=m1, m2=m2, rs=rs, ks=ks, mask=m, n_g=1 if dy2 is not None else 0)


def ln_bwd_bounds(ref, bf):
    g, xh, dx, m1, m2, rs, ks, ds, da = (ref[k] for k in ("g", "xh", "dx", "m1", "m2", "rs", "ks", "ds", "da"))
    rows, D = ds.shape
    ng = ref["n_g"]
    cnt = row_sum_count(D, bf)
    vm1 = ((ng + 1) * (dx * dx).sum(1, keepdim=True) + (cnt + 2) * dx.abs().sum(1, keepdim=True) ** 2) / D ** 2
    t2 = dx * xh
    vm2 = ((ng + 3) * (t2 * t2).sum(1, keepdim=True) + (cnt + 2) * t2.abs().sum(1, keepdim=True) ** 2) / D ** 2
    xm = xh * m2
    vo = rs ** 2 * ((ng + 1) * dx * dx + vm1 + xh * xh * vm2 + 3 * xm * xm + 2 * (dx.abs() + m1.abs() + xm.abs()) ** 2) + ds * ds
    b_ds = 4 * torch.sqrt(U32 ** 2 * vo + (U16 * ds) ** 2 * bf)
    vda = torch.where(ref["mask"], ks * ks * vo + 2 * da * da, _z(da)) if ks != 1.0 else vo
    b_da = 4 * torch.sqrt(U32 ** 2 * vda + (U16 * da) ** 2 * bf)
    n = ln_col_count(rows)

    def col(t, vt):
        return 4 * U32 * torch.sqrt(vt.sum(0) + n * t.abs().sum(0) ** 2)

    tg = g * xh
    return dict(ds=b_ds, da=b_da, dgamma=col(tg, (ng + 2) * tg * tg), dbeta=col(g, ng * g * g), dbias=col(da, vda))


# ----------------------------------------------------------------------------------------------------------------------
# GELU, posenc, colsum
# ----------------------------------------------------------------------------------------------------------------------
def gelu_parts(x, tanh=False):
    """gelu(x), gelu'(x), gelu''(x) in f64 (exact erf; tanh = True: the tanh form, a teeth mutant)."""
    if tanh:
        xr = x.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            v = torch.nn.functional.gelu(xr, approximate="tanh")
            (dv,) = torch.autograd.grad(v.sum(), xr)
        return v.detach(), dv, torch.zeros_like(x)
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return x * cdf, cdf + x * pdf, pdf * (2 - x * x)


def gelu_forward(h, bias, p=0.0, seed=0, base=0, mut=None):
    rows, F = h.shape
    x = h.double() + bias.double() if bias is not None else h.double()
    val, der, der2 = gelu_parts(x, tanh=mut == "tanh")
    ks = dropout.keep_scale(p)
    m = keep(seed, p, rows, F, h.device, base, mut)
    zero = _z(x)
    return dict(g=torch.where(m, val * ks, zero), gd=torch.where(m, der * ks, zero), x=x, der=der, der2=der2, mask=m, ks=ks,
                has_bias=bias is not None)


def gelu_backward(dg, ref, drop_rows=None):
    dh = dg.double() * ref["gd"]
    w = 1.0 if drop_rows is None else (~drop_rows).double()[:, None]
    return dict(dh=dh, db1=(dh * w).sum(0), dg=dg.double())


def _gelu_var(ref):
    """f32 path: variances of g and gd in u^2 units (kept elements)."""
    x, ks, g, gd = ref["x"], ref["ks"], ref["g"], ref["gd"]
    nb = 1.0 if ref["has_bias"] else 0.0
    z = x / math.sqrt(2)
    erf = torch.erf(z)
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    vcdf = 0.25 * ((2 / math.sqrt(math.pi) * torch.exp(-z * z) * z) ** 2 + 16 * erf * erf + (1 + erf) ** 2)
    vg = ks * ks * (nb * (ref["der"] * x) ** 2 + x * x * vcdf) + 3 * g * g
    vgd = ks * ks * (nb * (ref["der2"] * x) ** 2 + vcdf + (x * pdf) ** 2 * (x ** 4 / 4 + 6) + ref["der"] ** 2) + 2 * gd * gd
    return vg, vgd


def gelu_fwd_bounds(ref, bf):
    x, ks, g, gd, m = ref["x"], ref["ks"], ref["g"], ref["gd"], ref["mask"].double()
    nb = 1.0 if ref["has_bias"] else 0.0
    if not bf:
        vg, vgd = _gelu_var(ref)
        return dict(g=4 * U32 * torch.sqrt(vg) * m, gd=4 * U32 * torch.sqrt(vgd) * m)
    b_g = GELU_APPROX * ks + 4 * torch.sqrt((U16 * g) ** 2 + (U32 * ks * x) ** 2 * (0.25 + nb))
    b_gd = GELU_APPROX * ks + 4 * torch.sqrt((U16 * gd) ** 2 + (U32 * ks) ** 2 * (nb * (ref["der2"] * x) ** 2 + 1))
    return dict(g=b_g * m, gd=b_gd * m)


def gelu_bwd_bounds(ref, bref, bf):
    x, ks, m = ref["x"], ref["ks"], ref["mask"].double()
    dg, dh = bref["dg"], bref["dh"]
    rows = dh.shape[0]
    nb = 1.0 if ref["has_bias"] else 0.0
    n = slab_col_count(rows, rowslab_blocks(rows))
    if not bf:
        _, vgd = _gelu_var(ref)
        vt = (dg * dg * vgd + 2 * dh * dh) * m
        return dict(dh=4 * U32 * torch.sqrt(vt), db1=4 * U32 * torch.sqrt(vt.sum(0) + n * dh.abs().sum(0) ** 2))
    vt = ((dg * ks) ** 2 * (nb * (ref["der2"] * x) ** 2 + 1) + dh * dh) * m
    ap = GELU_APPROX * ks * dg.abs() * m
    return dict(dh=ap + 4 * torch.sqrt((U16 * dh) ** 2 + U32 ** 2 * vt),
                db1=ap.sum(0) + 4 * U32 * torch.sqrt(vt.sum(0) + n * dh.abs().sum(0) ** 2))


def posenc_forward(x, pe, T, p=0.0, seed=0, base=0, mut=None):
    """Mutants: "no_mod" (pe[r] instead of pe[r % T]; needs a table of `rows` rows), the mask mutants."""
    rows, D = x.shape
    t = x.double()
    if pe is not None:
        r = torch.arange(rows, device=x.device)
        t = t + pe.double()[r if mut == "no_mod" else r % T]
    ks = dropout.keep_scale(p)
    m = keep(seed, p, rows, D, x.device, base, mut)
    return dict(y=torch.where(m, t * ks, _z(t)), t=t, mask=m, has_pe=pe is not None, p=p)


def posenc_bounds(ref, bf):
    y = ref["y"]
    v = (ref["t"] ** 2 if ref["has_pe"] else 0) + (2 * y * y if ref["p"] > 0 else 0)
    return 4 * torch.sqrt(U32 ** 2 * v + (U16 * y) ** 2 * bf) * ref["mask"].double()


def colsum_reference(x, drop_rows=None):
    x64 = x.double()
    w = 1.0 if drop_rows is None else (~drop_rows).double()[:, None]
    return (x64 * w).sum(0)


def colsum_bound(x):
    rows = x.shape[0]
    n = slab_col_count(rows, colsum_blocks(rows), chains=2)
    return 4 * U32 * math.sqrt(n) * x.double().abs().sum(0)


# ----------------------------------------------------------------------------------------------------------------------
# CW embedding
# ----------------------------------------------------------------------------------------------------------------------
def _ids(tok, n, wrap=False):
    return tok % n if wrap else tok.clamp(0, n - 1)


def embed_forward(tokens, tables, mut=None):
    """(rows, sum widths) f64.  Mutants: "neighbour" (sqrt(w) of the next table), "wrap" (ids wrapped, not clamped)."""
    A = len(tables)
    out = []
    for f, t in enumerate(tables):
        w = tables[(f + 1) % A].shape[1] if mut == "neighbour" else t.shape[1]
        out.append(t.double()[_ids(tokens[:, f], t.shape[0], mut == "wrap")] * math.sqrt(w))
    return torch.cat(out, 1)


def embed_fwd_bound(ref, bf):
    return ref.abs() * (4 * math.sqrt(U16 ** 2 + 2 * U32 ** 2) if bf else 2 * U32)


def embed_backward(tokens, dout, widths, nrows, mut=None, drop_rows=None, chunk=1 << 18):
    """-> per table (grad, bound), both (n_f, w_f) f64, from dout (rows, >= sum widths) (a row-strided view is fine)."""
    rows = tokens.shape[0]
    ns = embed_splits(rows)
    per = -(-rows // ns)
    nfin = finalize_count(ns)
    res, off = [], 0
    for f, (w, n) in enumerate(zip(widths, nrows)):
        sc = math.sqrt(w)
        # one f64 index_add_ per chunk of rows for the gradient, sum |terms|, sum terms^2 and the hit count together, spread
        # over G copies of the table (row r adds into copy r % G) so that a small vocabulary does not serialise the adds
        G = 256 if rows > 4096 else 1
        acc = torch.zeros(G * n, 3 * w + 1, dtype=torch.float64, device=dout.device)
        for r0 in range(0, rows, chunk):
            r1 = min(rows, r0 + chunk)
            ids = _ids(tokens[r0:r1, f], n, mut == "wrap") + n * (torch.arange(r0, r1, device=dout.device) % G)
            t = dout[r0:r1, off:off + w].double() * sc
            live = t if drop_rows is None else t * (~drop_rows[r0:r1]).double()[:, None]
            acc.index_add_(0, ids, torch.cat([live, t.abs(), t * t, torch.ones_like(t[:, :1])], 1))
        acc = acc.view(G, n, 3 * w + 1).sum(0)
        grad, sab, ssq, hits = acc[:, :w].contiguous(), acc[:, w:2 * w], acc[:, 2 * w:3 * w], acc[:, 3 * w]
        serial = hits.clamp(max=per)
        cnt = torch.where(serial > 1, serial / 6.0, torch.zeros_like(serial)) + nfin
        res.append((grad, 4 * U32 * torch.sqrt(2 * ssq + cnt[:, None] * sab ** 2)))
        off += w
    return res


def embed_bwd_form(dtype, nrows, rows, ldd, ptr):
    """The dispatch of cwlt_cw_embed_bwd, restated: ("mfma" | "slab", raised LDS limit) or None where it refuses."""
    maxr = max(nrows)
    if maxr * 64 * 4 > 160 * 1024:
        return None
    ns = embed_splits(rows)
    if dtype == torch.bfloat16 and maxr <= 160 and -(-rows // ns) <= 4096 and ldd % 8 == 0 and ptr % 16 == 0:
        return ("mfma", False)
    return ("slab", maxr * 64 * 4 > 64 * 1024)


# ----------------------------------------------------------------------------------------------------------------------
# cwlt_gelu.h in f32, emulated (CPU test only)
# ----------------------------------------------------------------------------------------------------------------------
GELU_Q = (-3.959011294e-01, 2.307531891e-01, -9.244854863e-02, 2.139916809e-02, -2.076792892e-03)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def gelu_scaled_f32(x, s=1.0):
    """gelu_scaled(x, gelu_consts(s)) of cwlt_gelu.h on an f32 tensor: the same operations in the same order, every fma a
    product and sum in f64 rounded once to f32, exp2 correctly rounded.  -> y, dy (f32)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    s = f(s)
    c0 = f(0.5) * s
    c = [f(q) * s for q in GELU_Q]
    pdfc = f(0.39894228040143267794) * s
    x = x.float()
    e = torch.exp2(((x * x) * f(-0.72134752044448170368)).double()).float()
    a = x.abs()
    q = _fma(a, c[4].expand_as(a), c[3].expand_as(a))
    for k in (c[2], c[1], c[0], c0):
        q = _fma(a, q, k.expand_as(a))
    us = _fma(-e, q, c0.expand_as(a))
    cdf = c0 + torch.copysign(us, x)
    y = _fma(a, us, c0 * x)
    dy = _fma(e * x, pdfc.expand_as(a), cdf)
    return y, dy

"""CPU pin of oracle/elementwise_f64.py, the reference, inputs, measures and bounds of tests/test_elementwise_f64_gpu.py and
tests/test_embed_f64_gpu.py: the f64 forms equal torch's own layer_norm / gelu / embedding and their autograd gradients,
every input maker has the property it names, torch's f32 chain on the CPU (a stand-in for the kernels: the same formulas,
other summation orders; rounded to bf16 for the bf16 cases) stays inside every bound while every bound stays below 8 x that
floor, every "teeth" mutant falls outside its bound by TEETH = 5, a 64-bit dropout key equals the C formula, and the f32
emulation of cwlt_gelu.h keeps the header's 1.5e-4 and is finite through GELU_BF16_MAX_ABS.  No kernel runs here.  Run with
-s for the figures."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import dropout
from oracle import elementwise_f64 as o

BF16, F32 = torch.bfloat16, torch.float32
NAME = {F32: "f32", BF16: "bf16"}
WORST = {}        # (quantity, dtype) -> worst ratio of the f32 chain, read by test_bounds_are_not_loose (last in the module)
LN_D = {F32: (8, 256, 264, 512, 520, 768, 776, 1024), BF16: (8, 504, 512, 520, 1024)}
LN_ROWS_SMALL = (1, 3, 4, 5, 61, 65)
LN_ROWS_BIG = (1021, 1025, 4097)
SEED = 0x2545F4914F6CDD1D & ((1 << 62) - 1)


def note(label, r, dtype):
    for k, v in r.items():
        WORST[(k, dtype)] = max(WORST.get((k, dtype), 0.0), v)
    print("    %-52s %s" % (label, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert all(v <= 1 for v in r.values()), (label, r)


# ----------------------------------------------------------------------------------------------------------------------
# the f32 chains
# ----------------------------------------------------------------------------------------------------------------------
def ks32(p):
    return torch.tensor(dropout.keep_scale(p), dtype=F32)


def ln_chain(x, a, gamma, beta, p, seed):
    rows, D = a.shape
    v = a.float()
    if p > 0:
        v = torch.where(o.keep(seed, p, rows, D), v * ks32(p), torch.zeros(()))
    if x is not None:
        v = v + x.float()
    mean = v.mean(1)
    d = v - mean[:, None]
    rstd = torch.rsqrt((d * d).mean(1) + torch.tensor(o.LN_EPS, dtype=F32))
    y = d * rstd[:, None] * gamma + beta
    return v.to(a.dtype), y.to(a.dtype), mean, rstd


def ln_bwd_chain(dy, dy2, s, gamma, mean, rstd, p, seed):
    rows, D = s.shape
    g = dy.float() + dy2.float() if dy2 is not None else dy.float()
    xh = (s.float() - mean[:, None]) * rstd[:, None]
    dx = g * gamma
    o_ = rstd[:, None] * (dx - dx.mean(1, keepdim=True) - xh * (dx * xh).mean(1, keepdim=True))
    m = torch.where(o.keep(seed, p, rows, D), o_ * ks32(p), torch.zeros(())) if p > 0 else o_
    return o_.to(s.dtype), m.to(s.dtype), (g * xh).sum(0), g.sum(0), m.sum(0)


def gelu_chain(h, bias, p, seed, dg=None):
    rows, Fd = h.shape
    x = h.float() + bias if bias is not None else h.float()
    m = o.keep(seed, p, rows, Fd)
    zero = torch.zeros(())
    if h.dtype == BF16:
        y, dy = o.gelu_scaled_f32(x, dropout.keep_scale(p))
    else:
        cdf = 0.5 * (1 + torch.erf(x * 0.70710678118654752440))
        pdf = 0.39894228040143267794 * torch.exp(-0.5 * x * x)
        y, dy = x * cdf * ks32(p), (cdf + x * pdf) * ks32(p)
    g, gd = torch.where(m, y, zero), torch.where(m, dy, zero)
    if dg is None:
        return g.to(h.dtype), gd.to(h.dtype)
    dh = dg.float() * gd
    return g.to(h.dtype), gd.to(h.dtype), dh.to(h.dtype), dh.sum(0)


# ----------------------------------------------------------------------------------------------------------------------
# the references are what torch computes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("residual,two", [(True, True), (False, False)])
def test_ln_reference_equals_torch(p, residual, two):
    rows, D = 37, 264
    x, a = o.make_ln_input("mixed", rows, D, F32, residual=residual)
    gamma, beta = o.make_affine(D)
    ref = o.ln_forward(x, a, gamma, beta, p=p, seed=SEED)
    a64 = a.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True) if residual else None
    m = ref["mask"].double() * dropout.keep_scale(p)
    assert (p == 0) == bool(ref["mask"].all())
    s = a64 * m + x64 if residual else a64 * m
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.layer_norm(s, (D,), g64, b64, ref["eps"])
    assert (ref["y"] - y).abs().max() < 1e-12 and (ref["s"] - s).abs().max() < 1e-12
    assert (ref["mean"] - s.mean(1)).abs().max() < 1e-12
    assert ((ref["rstd"] - 1 / torch.sqrt(s.var(1, unbiased=False) + ref["eps"])) / ref["rstd"]).abs().max() < 1e-12
    gen = torch.Generator().manual_seed(9)
    dy = torch.randn(rows, D, generator=gen)
    dy2 = torch.randn(rows, D, generator=gen) if two else None
    up = dy.double() + dy2.double() if two else dy.double()
    s2 = s.detach().requires_grad_(True)
    y2 = F.layer_norm(s2, (D,), g64, b64, ref["eps"])
    ds, dgm, dbt = torch.autograd.grad((y2 * up).sum(), [s2, g64, b64])
    b = o.ln_backward(dy, dy2, ref["s"], gamma, ref["mean"], ref["rstd"], p, SEED)
    scale = float(ds.abs().max())
    assert (b["ds"] - ds).abs().max() < 1e-12 * scale and (b["da"] - ds * m).abs().max() < 1e-12 * scale
    assert (b["dgamma"] - dgm).abs().max() < 1e-11 and (b["dbeta"] - dbt).abs().max() < 1e-11
    assert (b["dbias"] - (ds * m).sum(0)).abs().max() < 1e-11


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_posenc_reference_equals_torch(p):
    rows, Fd = 19, 72
    h = o.make_gelu_input("randn2", rows, Fd)
    bias = torch.randn(Fd)
    ref = o.gelu_forward(h, bias, p, SEED)
    m = ref["mask"].double() * dropout.keep_scale(p)
    x = (h.double() + bias.double()).requires_grad_(True)
    v = F.gelu(x)
    dg = torch.randn(rows, Fd, dtype=torch.float64)
    (dx,) = torch.autograd.grad((v * m * dg).sum(), x)
    b = o.gelu_backward(dg, ref)
    assert (ref["g"] - v * m).abs().max() < 1e-12 and (b["dh"] - dx).abs().max() < 1e-12
    assert (b["db1"] - dx.sum(0)).abs().max() < 1e-11
    pe = torch.randn(50, Fd)
    pr = o.posenc_forward(h, pe, 7, p, SEED)
    want = (h.double().view(-1) + pe.double()[torch.arange(rows) % 7].view(-1)) * m.view(-1)
    assert (pr["y"].view(-1) - want).abs().max() < 1e-12
    assert (o.colsum_reference(h) - h.double().sum(0)).abs().max() < 1e-12


def test_embed_reference_equals_torch():
    widths, nrows = (64, 128), (5, 9)
    tables = [t.double().requires_grad_(True) for t in o.make_tables(widths, nrows)]
    tok = o.make_tokens(41, nrows, oor=True)
    assert (tok < 0).any() and (tok >= torch.tensor(nrows)).any()
    want = torch.cat([F.embedding(tok[:, f].clamp(0, n - 1), t) * math.sqrt(w)
                      for f, (t, w, n) in enumerate(zip(tables, widths, nrows))], 1)
    ref = o.embed_forward(tok, [t.detach() for t in tables])
    assert (ref - want).abs().max() < 1e-12
    dout = torch.randn(41, 200, dtype=torch.float64)[:, :192]           # a row-strided view
    grads = torch.autograd.grad((want * dout).sum(), tables)
    for (g, bnd), w in zip(o.embed_backward(tok, dout, widths, nrows), grads):
        assert (g - w).abs().max() < 1e-11 and (bnd >= 0).all()


def test_seed_key_is_the_c_formula():
    """dropout.rng_pair on Python integers takes a full 64-bit key: equal to cwlt_common.h::rng_pair restated on scalars."""
    M = 0xFFFFFFFF

    def h32(v):
        v ^= v >> 16
        v = v * 0x7FEB352D & M
        v ^= v >> 15
        v = v * 0x846CA68B & M
        return v ^ (v >> 16)

    def c_rng_pair(seed, pair):
        lo, hi = pair & M, pair >> 32
        key = (seed & M) ^ ((seed >> 32) * 0x9E3779B9 & M) ^ (hi * 0x85EBCA6B & M)
        return h32((lo * 0x9E3779B1 & M) ^ key)

    step = 0x9E3779B97F4A7C15 - (1 << 64)
    assert o.seed_key(5, step) == 5 + 0x9E3779B97F4A7C15 and o.seed_key(SEED, -SEED - 1) == (1 << 64) - 1
    assert o.seed_key(SEED, (1 << 63) - 1) > (1 << 62) and o.seed_key((1 << 62) - 1, -(1 << 62)) == (1 << 64) - 1
    pairs = [0, 1, 77, (1 << 32) - 1, 1 << 32, (1 << 33) + 12345]
    for key in (0, SEED, o.seed_key(SEED, step), (1 << 64) - 1, o.seed_key(3, -7)):
        got = dropout.rng_pair(key, torch.tensor(pairs, dtype=torch.int64)).tolist()
        assert got == [c_rng_pair(key, q) for q in pairs], hex(key)
    a = o.keep(SEED, 0.1, 8, 64)
    assert not torch.equal(a, o.keep(SEED, 0.1, 8, 64, base=step)) and 0.8 < a.float().mean() < 0.97
    assert torch.equal(o.keep(SEED, 0.1, 8, 64, base=step, mut="nobase"), a)
    assert torch.equal(o.keep(SEED, 0.1, 8, 64, mut="swap").view(-1, 2).flip(1).reshape(8, 64), a)
    assert torch.equal(o.keep(SEED, 0.1, 8, 64, mut="shift").view(-1)[:-2], a.view(-1)[2:])


# ----------------------------------------------------------------------------------------------------------------------
# input makers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ln_input_makers(dtype):
    rows, D = 12, 520
    for residual in (True, False):
        st = {}
        for kind in o.LN_KINDS:
            x, a = o.make_ln_input(kind, rows, D, dtype, residual=residual)
            assert (x is None) == (not residual) and a.dtype == dtype
            s = a.double() + x.double() if residual else a.double()
            st[kind] = (s, s.mean(1), s.var(1, unbiased=False))
        s, mu, var = st["randn"]
        assert (mu.abs() < 0.3).all() and ((var > 0.7) & (var < 1.4)).all()
        s, mu, var = st["mean100"]
        assert ((mu.abs() / var.sqrt() > 80) & (mu.abs() / var.sqrt() < 125)).all() and (mu > 0).any() and (mu < 0).any()
        s, mu, var = st["tiny"]
        assert (var < o.LN_EPS / 5).all() and (var > o.LN_EPS / 20).all()
        s, mu, var = st["const"]
        assert (var == 0).all() and (s == s[:, :1]).all() and (s != 0).all() and len(set(s[:, 0].tolist())) > 4
        s, mu, var = st["outlier"]
        top = s.abs().max(1).values
        rest = s.abs().kthvalue(D - 1, 1).values
        assert (top > 200 * rest).all() and (s.abs().argmax(1) == (torch.arange(rows) * 7) % D).all()
        s, mu, var = st["mixed"]
        sd = var.sqrt()
        assert (sd[0::3] > 0.8).all() and (sd[0::3] < 1.2).all() and (sd[1::3] > 8).all() and (sd[2::3] < 0.12).all()


def test_gelu_and_token_makers():
    lad = o.gelu_ladder()
    assert lad.abs().max() == o.GELU_BF16_MAX_ABS and lad.abs()[2:].min() == 1e-4
    assert (lad == 0).sum() == 2 and torch.signbit(lad[:2]).tolist() == [False, True]
    assert set((-lad[2:]).tolist()) == set(lad[2:].tolist()) and {5.5, 13.0, -13.0} <= set(lad.tolist())
    for dtype in (F32, BF16):
        h = o.make_gelu_input("ladder", 64, 64, dtype)
        assert h.abs().max() == o.GELU_BF16_MAX_ABS and all((h[:, c].double() == 2.0 ** 26).any() for c in range(64))
    h = o.make_gelu_input("randn2", 64, 64)
    assert 1.8 < h.std() < 2.2
    tok = o.make_tokens(500, (33, 7), every=(1, 4), never=(0, 31))
    assert (tok[:, 1] == 4).all() and not (tok[:, 0] == 31).any() and (tok[:, 0] == 32).any()
    assert o.embed_bwd_form(BF16, (160,), 2097152, 64, 0) == ("mfma", False)
    assert o.embed_bwd_form(BF16, (160,), 2097153, 64, 0) == ("slab", False)
    assert o.embed_bwd_form(BF16, (161,), 5, 64, 0) == ("slab", False) == o.embed_bwd_form(BF16, (9,), 5, 68, 0)
    assert o.embed_bwd_form(BF16, (9,), 5, 64, 8) == ("slab", False) == o.embed_bwd_form(F32, (256,), 5, 64, 0)
    assert o.embed_bwd_form(F32, (257,), 5, 64, 0) == ("slab", True) == o.embed_bwd_form(BF16, (640,), 5, 64, 0)
    assert o.embed_bwd_form(F32, (641,), 5, 64, 0) is None
    assert o.ln_last_block_rows(4097).nonzero().view(-1).tolist() == [4092, 4093, 4094, 4095]
    assert o.last_split_rows(131073, 512).nonzero().view(-1).tolist() == list(range(510 * 257, 131073))
    assert [o.finalize_count(n) for n in (1, 2, 16)] == [0, 2 / 6.0, 16 / 6.0] and o.finalize_count(257) == 2 / 6.0 + 4 + 16 / 6.0


# ----------------------------------------------------------------------------------------------------------------------
# the f32 chain stays inside every bound
# ----------------------------------------------------------------------------------------------------------------------
def ln_case(dtype, kind, rows, D, p, residual, two, label):
    bf = dtype == BF16
    x, a = o.make_ln_input(kind, rows, D, dtype, residual=residual)
    gamma, beta = o.make_affine(D)
    ref = o.ln_forward(x, a, gamma, beta, p=p, seed=SEED)
    s, y, mean, rstd = ln_chain(x, a, gamma, beta, p, SEED)
    bnd = o.ln_fwd_bounds(ref, gamma, bf)
    r = {k: o.ratio(v, ref[k], bnd[k]) for k, v in (("s", s), ("y", y), ("mean", mean), ("rstd", rstd))}
    gen = torch.Generator().manual_seed(rows + D)
    dy = torch.randn(rows, D, generator=gen).abs().to(dtype)           # one sign: the column sums do not cancel
    dy2 = torch.randn(rows, D, generator=gen).to(dtype) if two else None
    bref = o.ln_backward(dy, dy2, s, gamma, mean, rstd, p, SEED)
    bb = o.ln_bwd_bounds(bref, bf)
    got = dict(zip(("ds", "da", "dgamma", "dbeta", "dbias"), ln_bwd_chain(dy, dy2, s, gamma, mean, rstd, p, SEED)))
    r.update({k: o.ratio(got[k], bref[k], bb[k]) for k in got})
    note(label, r, dtype)
    return x, a, gamma, beta, ref, bnd, (s, y, mean, rstd), (dy, dy2, bref, bb, got)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ln_chain_inside_bounds(dtype):
    i = 0
    for D in LN_D[dtype]:
        for rows in LN_ROWS_SMALL:
            kind = o.LN_KINDS[i % len(o.LN_KINDS)]
            p, residual, two = (0.1 if i % 2 else 0.0), i % 3 != 0, i % 4 < 2
            ln_case(dtype, kind, rows, D, p, residual, two, "ln %s %s %dx%d p%.1f x%d dy2%d" % (NAME[dtype], kind, rows, D, p,
                                                                                                residual, two))
            i += 1
    for rows in LN_ROWS_BIG:
        for kind in o.LN_KINDS:
            D = 256 if dtype == F32 else 512
            ln_case(dtype, kind, rows, D, 0.1 if i % 2 else 0.0, True, i % 4 < 2, "ln %s %s %dx%d" % (NAME[dtype], kind, rows, D))
            i += 1


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gelu_posenc_colsum_chain_inside_bounds(dtype):
    bf = dtype == BF16
    i = 0
    for Fd in (8, 64, 1016, 1024, 1032, 2048, 2056):
        for rows in ((1, 7, 8, 9, 15, 16, 17) if Fd != 64 else (1, 9, 17, 4099)):
            for kind in ("randn2", "ladder"):
                p = 0.1 if i % 2 else 0.0
                h = o.make_gelu_input(kind, rows, Fd, dtype)
                bias = torch.randn(Fd, generator=torch.Generator().manual_seed(i)) if i % 3 else None
                dg = torch.randn(rows, Fd, generator=torch.Generator().manual_seed(i + 1)).abs().to(dtype)
                ref = o.gelu_forward(h, bias, p, SEED)
                bref = o.gelu_backward(dg, ref)
                g, gd, dh, db1 = gelu_chain(h, bias, p, SEED, dg)
                assert torch.isfinite(g.float()).all() and torch.isfinite(gd.float()).all()
                fb, bb = o.gelu_fwd_bounds(ref, bf), o.gelu_bwd_bounds(ref, bref, bf)
                assert o.mask_exact(g, ref["g"], fb["g"], ref["mask"]) and o.mask_exact(gd, ref["gd"], fb["gd"], ref["mask"])
                r = dict(g=o.ratio(g, ref["g"], fb["g"]), gd=o.ratio(gd, ref["gd"], fb["gd"]),
                         dh=o.ratio(dh, bref["dh"], bb["dh"]), db1=o.ratio(db1, bref["db1"], bb["db1"]))
                note("gelu %s %s %dx%d p%.1f bias%d" % (NAME[dtype], kind, rows, Fd, p, bias is not None), r, dtype)
                i += 1
    for D, rows, T, p in ((8, 5, 1, 0.25), (128, 33, 7, 0.0), (512, 9, 9, 0.25), (128, 6, 11, 0.25)):
        x = torch.randn(rows, D).abs().to(dtype)
        pe = torch.randn(T + 3, D).abs()
        ref = o.posenc_forward(x, pe, T, p, SEED)
        t = x.float() + pe[torch.arange(rows) % T]
        y = torch.where(ref["mask"], t * ks32(p), torch.zeros(())).to(dtype) if p else t.to(dtype)
        note("posenc %s %dx%d T%d p%.2f" % (NAME[dtype], rows, D, T, p), dict(posenc=o.ratio(y, ref["y"], o.posenc_bounds(ref, bf))), dtype)
    for ncols in (8, 1536):
        for rows in (1, 63, 64, 65, 4099):
            x = torch.randn(rows, ncols + 8).abs().to(dtype)[:, :ncols]
            got = x.float().sum(0)
            note("colsum %s %dx%d" % (NAME[dtype], rows, ncols), dict(colsum=o.ratio(got, o.colsum_reference(x), o.colsum_bound(x))), dtype)


EMBED_SETS = {"one64": ((64,), (18,)), "repo": (o.REPO_WIDTHS, o.REPO_VOCAB), "w1408": ((512, 512, 384), (7, 33, 160)),
              "w2048": ((1024, 1024), (5, 3)), "attr8": ((64,) * 8, (3, 31, 32, 33, 1, 160, 9, 2))}


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_embed_chain_inside_bounds(dtype):
    bf = dtype == BF16
    for name, (widths, nrows) in EMBED_SETS.items():
        tables = o.make_tables(widths, nrows)
        for rows in (1, 15, 16, 17, 33, 513):
            tok = o.make_tokens(rows, nrows, oor=True)
            ref = o.embed_forward(tok, tables)
            got = torch.cat([t[tok[:, f].clamp(0, n - 1)] * torch.tensor(w, dtype=F32).sqrt()
                             for f, (t, w, n) in enumerate(zip(tables, widths, nrows))], 1).to(dtype)
            r = dict(embed=o.ratio(got, ref, o.embed_fwd_bound(ref, bf)))
            dout = torch.randn(rows, sum(widths)).abs().to(dtype)
            worst, off = 0.0, 0
            for f, (g, bnd) in enumerate(o.embed_backward(tok, dout, widths, nrows)):
                w, n = widths[f], nrows[f]
                acc = torch.zeros(n, w).index_add_(0, tok[:, f].clamp(0, n - 1), dout[:, off:off + w].float() * torch.tensor(w, dtype=F32).sqrt())
                worst = max(worst, o.ratio(acc, g, bnd))
                off += w
            r["dtable"] = worst
            note("embed %s %s rows %d" % (NAME[dtype], name, rows), r, dtype)


# ----------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------
def bite(label, got, ref, bound, need=o.TEETH):
    r = o.ratio(got, ref, bound)
    print("    tooth %-44s %.3g" % (label, r))
    assert r >= need, (label, r)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_teeth(dtype):
    bf = dtype == BF16
    rows, D, p = 65, 520, 0.1
    gamma, beta = o.make_affine(D)

    def fwd(kind, mut, keys, base=0, pp=p):
        x, a = o.make_ln_input(kind, rows, D, dtype)
        got = dict(zip(("s", "y", "mean", "rstd"), ln_chain(x, a, gamma, beta, pp, o.seed_key(SEED, base))))
        right = o.ln_forward(x, a, gamma, beta, p=pp, seed=SEED, base=base)
        bnd = o.ln_fwd_bounds(right, gamma, bf)
        assert all(o.ratio(got[k], right[k], bnd[k]) <= 1 for k in got)
        wrong = o.ln_forward(x, a, gamma, beta, p=pp, seed=SEED, base=base, mut=mut)
        for k in keys:
            bite("ln %s %s on %s" % (mut, k, kind), got[k], wrong[k], bnd[k])
        return x, a, got

    fwd("tiny", "eps6", ("rstd", "y"))
    fwd("randn", "unbiased", ("rstd", "y"))
    fwd("mean100", "mean_undropped", ("mean", "y"))
    fwd("randn", "shift", ("s", "y"))
    fwd("randn", "swap", ("s", "y"))
    fwd("randn", "nobase", ("s", "y"), base=0x9E3779B97F4A7C15 - (1 << 64))
    x, a, got = fwd("randn", "swap", ("s",))
    gen = torch.Generator().manual_seed(3)
    dy, dy2 = torch.randn(rows, D, generator=gen).abs().to(dtype), torch.randn(rows, D, generator=gen).to(dtype)
    chain = dict(zip(("ds", "da", "dgamma", "dbeta", "dbias"), ln_bwd_chain(dy, dy2, got["s"], gamma, got["mean"], got["rstd"], p, SEED)))
    right = o.ln_backward(dy, dy2, got["s"], gamma, got["mean"], got["rstd"], p, SEED)
    bb = o.ln_bwd_bounds(right, bf)
    assert all(o.ratio(chain[k], right[k], bb[k]) <= 1 for k in chain)
    for mut, drop, keys in (("no_dy2", None, ("ds", "da", "dgamma", "dbeta", "dbias")), ("swap", None, ("da", "dbias")),
                            (None, o.ln_last_block_rows(rows), ("dgamma", "dbeta", "dbias"))):
        wrong = o.ln_backward(dy, dy2, got["s"], gamma, got["mean"], got["rstd"], p, SEED, mut=mut, drop_rows=drop)
        for k in keys:
            bite("ln_bwd %s %s" % (mut or "last block dropped", k), chain[k], wrong[k], bb[k])
    # GELU, posenc, colsum
    h = o.make_gelu_input("randn2", 33, 1032, dtype)
    bias = torch.randn(1032)
    dg = torch.randn(33, 1032).abs().to(dtype)
    g, gd, dh, db1 = gelu_chain(h, bias, p, SEED, dg)
    ref = o.gelu_forward(h, bias, p, SEED)
    fb, bref = o.gelu_fwd_bounds(ref, bf), o.gelu_backward(dg, ref)
    bb = o.gelu_bwd_bounds(ref, bref, bf)
    for mut in ("tanh", "shift", "swap"):
        wrong = o.gelu_forward(h, bias, p, SEED, mut=mut)
        # the tanh form is at most 4.7e-4 from the erf form: 3.1 x the bf16 path's own allowance of GELU_APPROX, so in bf16
        # the mutant can only be asked to fall outside the bound (it does, by 2 to 3 x); f32 resolves it fully
        need = 1.0 if bf and mut == "tanh" else o.TEETH
        bite("gelu %s g" % mut, g, wrong["g"], fb["g"], need)
        bite("gelu %s gd" % mut, gd, wrong["gd"], fb["gd"], need)
        bite("gelu %s dh" % mut, dh, o.gelu_backward(dg, wrong)["dh"], bb["dh"], need)
    bite("gelu last slab dropped db1", db1, o.gelu_backward(dg, ref, o.last_split_rows(33, o.rowslab_blocks(33)))["db1"], bb["db1"])
    x = torch.randn(33, 128).to(dtype)
    pe = torch.randn(33, 128)
    ref = o.posenc_forward(x, pe, 7, p, SEED)
    y = torch.where(ref["mask"], (x.float() + pe[torch.arange(33) % 7]) * ks32(p), torch.zeros(())).to(dtype)
    assert o.ratio(y, ref["y"], o.posenc_bounds(ref, bf)) <= 1
    for mut in ("no_mod", "swap", "shift"):
        bite("posenc %s" % mut, y, o.posenc_forward(x, pe, 7, p, SEED, mut=mut)["y"], o.posenc_bounds(ref, bf))
    xs = torch.randn(65, 64).abs().to(dtype)
    bite("colsum last split dropped", xs.float().sum(0), o.colsum_reference(xs, o.last_split_rows(65, o.colsum_blocks(65))),
         o.colsum_bound(xs))
    # embedding
    widths, nrows = o.REPO_WIDTHS, o.REPO_VOCAB
    tables = o.make_tables(widths, nrows)
    tok = o.make_tokens(513, nrows, oor=True)
    ref = o.embed_forward(tok, tables)
    got = torch.cat([t[tok[:, f].clamp(0, n - 1)] * torch.tensor(w, dtype=F32).sqrt()
                     for f, (t, w, n) in enumerate(zip(tables, widths, nrows))], 1).to(dtype)
    for mut in ("neighbour", "wrap"):
        bite("embed %s" % mut, got, o.embed_forward(tok, tables, mut=mut), o.embed_fwd_bound(ref, bf))
    dout = torch.randn(513, sum(widths)).abs().to(dtype)
    right = o.embed_backward(tok, dout, widths, nrows)
    for label, kw in (("wrap", dict(mut="wrap")), ("last split dropped", dict(drop_rows=o.last_split_rows(513, o.embed_splits(513))))):
        wrong = o.embed_backward(tok, dout, widths, nrows, **kw)
        bite("embed_bwd %s" % label, torch.cat([g.view(-1) for g, _ in right]), torch.cat([g.view(-1) for g, _ in wrong]),
             torch.cat([b.view(-1) for _, b in right]))


# ----------------------------------------------------------------------------------------------------------------------
# cwlt_gelu.h in f32
# ----------------------------------------------------------------------------------------------------------------------
def test_gelu_emulation_accuracy_and_domain():
    x = torch.linspace(-12, 12, 2400001, dtype=torch.float64).float()
    val, der, _ = o.gelu_parts(x.double())
    for s in (1.0, dropout.keep_scale(0.1)):
        y, dy = o.gelu_scaled_f32(x, s)
        ev, ed = float((y.double() / s - val).abs().max()), float((dy.double() / s - der).abs().max())
        print("    gelu_scaled f32 emulation on [-12, 12], scale %.4f: worst |gelu| %.4e  |gelu'| %.4e" % (s, ev, ed))
        assert ev <= o.GELU_APPROX and ed <= o.GELU_APPROX
    lad = o.gelu_ladder().float()
    val, der, _ = o.gelu_parts(lad.double())
    for s in (1.0, dropout.keep_scale(0.1), dropout.keep_scale(0.25)):
        y, dy = o.gelu_scaled_f32(lad, s)
        assert torch.isfinite(y).all() and torch.isfinite(dy).all()
        big = lad.abs() >= 20
        # x / 0 / 1 / 0 within rounding: of the uncancelled magnitude |x| for the value, of 1 for the derivative
        assert ((y.double() - s * val).abs() <= o.GELU_APPROX * s + 4 * o.U32 * s * lad.abs().double()).all()
        assert ((dy.double() - s * der).abs() <= o.GELU_APPROX * s).all()
        assert (dy[big & (lad > 0)].double() - s).abs().max() <= 2 * o.U32 * s and (dy[big & (lad < 0)] == 0).all()
        assert ((y[big & (lad > 0)].double() - s * lad[big & (lad > 0)].double()).abs() <= 2 * o.U32 * s * lad[big & (lad > 0)].double()).all()
    # where the formula first returns NaN: the documented limit is a measured one
    grid = torch.tensor([2.0 ** 26 * 1.0005 ** k for k in range(4000)], dtype=torch.float64).float()
    y, dy = o.gelu_scaled_f32(grid)
    bad = torch.isnan(y) | torch.isnan(dy)
    first = float(grid[bad][0])
    print("    gelu_scaled f32 emulation: first NaN at |x| = %.4e (finite through %.4e; GELU_BF16_MAX_ABS = %.4e)"
          % (first, float(grid[~bad][-1]), o.GELU_BF16_MAX_ABS))
    assert not bad[0] and 1.5e8 < first < 2.1e8 and bad[grid >= first].all()
    yn, dyn = o.gelu_scaled_f32(-grid)
    assert torch.equal(torch.isnan(yn) | torch.isnan(dyn), bad)


def test_bounds_are_not_loose():
    """Every bound is below 8 x the floor the f32 chain sets at its worst case (runs after the chain tests of this module)."""
    want = [(k, d) for d in (F32, BF16) for k in ("s", "y", "mean", "rstd", "ds", "da", "dgamma", "dbeta", "dbias", "g", "gd", "dh",
                                                   "db1", "posenc", "colsum", "embed", "dtable")]
    missing = [k for k in want if k not in WORST]
    assert not missing, missing
    for k in want:
        print("    floor %-8s %-5s worst chain / bound %.3f" % (k[0], NAME[k[1]], WORST[k]))
    loose = {(k, NAME[d]): v for (k, d), v in WORST.items() if v < 0.125}
    assert not loose, loose

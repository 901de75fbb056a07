"""GPU: the LayerNorm kernels (csrc/ln.hip), the FFN activation, posenc and colsum kernels (csrc/ffn_act.hip, cwlt_gelu.h)
per element, row and column against the f64 references of oracle/elementwise_f64.py (pinned, with every bound below, by
tests/test_oracle_elementwise_f64_cpu.py).  The CW embedding is in tests/test_embed_f64_gpu.py.

Reference.  f64 on the GPU (plain torch, none of the project's kernels) from the very values the kernels are given (the bf16
values of bf16 inputs); the LayerNorm backward is evaluated on the s, mean and rstd the forward kernel stored.  Dropout masks
and keep_scale come from oracle/dropout.py.  Every output is compared at every element, each under its own bound (counts in
the oracle's docstring); dropped elements must be exactly 0.  Outputs, partial-sum workspaces and statistics live inside
sentinel-filled buffers whose margins must come back untouched; inputs must come back bit-identical.

Shapes.  LayerNorm: D f32 8, 256, 264, 512, 520, 768, 776, 1024 (NC 1, 2, 4; a dead chunk from 516 to 768; partial last
chunks), bf16 8, 504, 512, 520, 1024; rows 1, 3, 4, 5, 61, 65, 1021, 1025, 4095, 4096, 4097, 8195 (1, 16, 17, 256, 257, 1024
partial blocks of colsum_finalize, then the second and third grid pass); the rows from 1021 on at three (f32) / two (bf16)
widths.  Inputs: all of LN_KINDS, p 0 and 0.1, residual and dy2 present and absent, ds / da NULL, the plain-LayerNorm form.
GELU: F 8, 64, 1016, 1024, 1032, 2048, 2056, forward rows 1, 7, 8, 9 and (F = 64) 32768, 32769, backward rows 1, 15, 16, 17
and (F = 64) 16384, 16385, 32769; randn x 2 and the magnitude ladder through GELU_BF16_MAX_ABS; gd absent, separate and
aliasing h.  posenc: D 8, 128, 512, T 1, 7, rows, > rows, pe longer than T and NULL, 1048576 and 1048576 + 128 vectors.
colsum: 8 and 1536 columns, rows 1, 63, 64, 65, 32768, 32769, dense and row-strided.

Teeth (TEETH = 5): the reference with eps 1e-6 on `tiny` rows, and with the two 16-bit halves of each hash word exchanged,
must miss the KERNELS' results by 5 x the bound while the right reference is inside it (the dropped last split:
tests/test_embed_f64_gpu.py and the colsum case here).

Measured on an MI355X: profiles/elementwise_f64_ratios.txt (the -s output of this file).
"""
import math

import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import _lib, ops
from oracle import elementwise_f64 as o

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAME = {F32: "f32", BF16: "bf16"}
SENT = -7777.0
SEED = 0x2545F4914F6CDD1D & ((1 << 62) - 1)
WORST = {}
LN_D = {F32: (8, 256, 264, 512, 520, 768, 776, 1024), BF16: (8, 504, 512, 520, 1024)}
LN_D_BIG = {F32: (256, 776, 1024), BF16: (520, 1024)}
LN_ROWS = (1, 3, 4, 5, 61, 65)
LN_ROWS_BIG = (1021, 1025, 4095, 4096, 4097, 8195)


def note(label, r, dtype):
    for k, v in r.items():
        WORST[(k, NAME[dtype])] = max(WORST.get((k, NAME[dtype]), 0.0), v)
    print("    %-56s %s" % (label, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert all(v <= 1 for v in r.values()), (label, r)


class Guarded:
    """A tensor inside a sentinel-filled buffer (64 elements each side: the view stays 16-byte aligned)."""

    def __init__(self, shape, dtype, dev):
        n = math.prod(shape)
        self.buf = torch.full((n + 128,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[64:64 + n].view(shape)
        self.n = n

    def intact(self):
        return bool((self.buf[:64] == SENT).all()) and bool((self.buf[64 + self.n:] == SENT).all())


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def code(t):
    return _lib.dtype_code(t.dtype)


# ----------------------------------------------------------------------------------------------------------------------
# the entry points, on guarded buffers
# ----------------------------------------------------------------------------------------------------------------------
def ln_fwd(x, a, gamma, beta, p=0.0, seed=0, want_s=True, eps=o.LN_EPS):
    rows, D = a.shape
    dev = a.device
    s = Guarded((rows, D), a.dtype, dev) if want_s else None
    y, mean, rstd = Guarded((rows, D), a.dtype, dev), Guarded((rows,), F32, dev), Guarded((rows,), F32, dev)
    keep = [t.clone() for t in (a, gamma, beta)] + ([x.clone()] if x is not None else [])
    ops._call("cwlt_add_dropout_layernorm_fwd", _lib.opt(x), _lib.dev(a), _lib.dev(gamma), _lib.dev(beta),
              _lib.opt(s.t if s else None), _lib.dev(y.t), _lib.dev(mean.t), _lib.dev(rstd.t), rows, D, float(eps), float(p),
              int(seed), None, code(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert all(g.intact() for g in (s, y, mean, rstd) if g is not None)
    assert all(same(u, v) for u, v in zip(keep, [a, gamma, beta] + ([x] if x is not None else [])))
    return dict(s=s.t if s else None, y=y.t, mean=mean.t, rstd=rstd.t)


def ln_bwd(dy, dy2, s, gamma, mean, rstd, p=0.0, seed=0, want_ds=True, want_da=True):
    rows, D = s.shape
    dev = s.device
    nb = _lib.load().cwlt_ln_blocks(rows)
    assert nb == o.ln_blocks(rows)
    ds = Guarded((rows, D), s.dtype, dev) if want_ds else None
    da = Guarded((rows, D), s.dtype, dev) if want_da else None
    part, stats = Guarded((nb * 3 * D,), F32, dev), Guarded((3, D), F32, dev)
    keep = [t.clone() for t in (dy, s, gamma, mean, rstd)]
    ops._call("cwlt_add_dropout_layernorm_bwd", _lib.dev(dy), _lib.opt(dy2), _lib.dev(s), _lib.dev(gamma), _lib.dev(mean),
              _lib.dev(rstd), _lib.opt(ds.t if ds else None), _lib.opt(da.t if da else None), _lib.dev(part.t),
              _lib.dev(stats.t), rows, D, float(p), int(seed), None, code(s), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert all(g.intact() for g in (ds, da, part, stats) if g is not None)
    assert all(same(u, v) for u, v in zip(keep, (dy, s, gamma, mean, rstd)))
    return dict(ds=ds.t if ds else None, da=da.t if da else None, dgamma=stats.t[0], dbeta=stats.t[1], dbias=stats.t[2])


def gelu_fwd(h, bias, p=0.0, seed=0, gd="sep"):
    """gd: None, "sep" (its own buffer) or "alias" (h is overwritten: a copy of h is passed)."""
    rows, Fd = h.shape
    g = Guarded((rows, Fd), h.dtype, h.device)
    hh = Guarded((rows, Fd), h.dtype, h.device)
    hh.t.copy_(h)
    d = hh if gd == "alias" else (Guarded((rows, Fd), h.dtype, h.device) if gd == "sep" else None)
    ops._call("cwlt_bias_gelu_dropout_fwd", _lib.dev(hh.t), _lib.opt(bias), _lib.dev(g.t), _lib.opt(d.t if d else None), rows, Fd,
              float(p), int(seed), None, code(h), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert g.intact() and hh.intact() and (d is None or d.intact()) and (gd == "alias" or same(hh.t, h))
    return g.t, (d.t if d else None)


def gelu_bwd(dg, h, bias, p=0.0, seed=0, want_dbias=True):
    rows, Fd = h.shape
    nb = _lib.load().cwlt_rowslab_blocks(rows)
    assert nb == o.rowslab_blocks(rows)
    dh = Guarded((rows, Fd), h.dtype, h.device)
    part = Guarded((nb * Fd,), F32, h.device) if want_dbias else None
    db = Guarded((Fd,), F32, h.device) if want_dbias else None
    keep = (dg.clone(), h.clone())
    ops._call("cwlt_bias_gelu_dropout_bwd", _lib.dev(dg), _lib.dev(h), _lib.opt(bias), _lib.dev(dh.t),
              _lib.opt(part.t if part else None), _lib.opt(db.t if db else None), rows, Fd, float(p), int(seed), None, code(h),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert dh.intact() and (part is None or (part.intact() and db.intact())) and same(keep[0], dg) and same(keep[1], h)
    return dh.t, (db.t if db else None)


def posenc(x, pe, T, p=0.0, seed=0):
    rows, D = x.shape
    y = Guarded((rows, D), x.dtype, x.device)
    keep = x.clone()
    ops._call("cwlt_posenc_dropout", _lib.dev(x), _lib.opt(pe), _lib.dev(y.t), rows, int(T), D, float(p), int(seed), None, code(x),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert y.intact() and same(keep, x)
    return y.t


def colsum(x):
    rows, ncols = x.shape
    nb = _lib.load().cwlt_colsum_blocks(rows)
    assert nb == o.colsum_blocks(rows)
    part, out = Guarded((nb * ncols,), F32, x.device), Guarded((ncols,), F32, x.device)
    ops._call("cwlt_colsum", _lib.dev(x), _lib.dev(part.t), _lib.dev(out.t), rows, ncols, x.stride(0), code(x), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert part.intact() and out.intact()
    return out.t


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def ln_case(cuda, dtype, kind, rows, D, p, residual, two, nulls=False):
    bf = dtype == BF16
    x, a = o.make_ln_input(kind, rows, D, dtype, seed=rows + D, residual=residual)
    x, a = (x.to(cuda) if residual else None), a.to(cuda)
    gamma, beta = (t.to(cuda) for t in o.make_affine(D))
    label = "ln %s %-7s %5dx%-4d p%.1f x%d dy2%d" % (NAME[dtype], kind, rows, D, p, residual, two)
    got = ln_fwd(x, a, gamma, beta, p, SEED)
    again = ln_fwd(x, a, gamma, beta, p, SEED)
    assert all(same(got[k], again[k]) for k in got), label
    ref = o.ln_forward(x, a, gamma, beta, p=p, seed=SEED)
    bnd = o.ln_fwd_bounds(ref, gamma, bf)
    r = {k: o.ratio(got[k], ref[k], bnd[k]) for k in ("s", "y", "mean", "rstd")}
    if p > 0 and not residual:
        assert o.mask_exact(got["s"], ref["s"], bnd["s"], ref["mask"]), label
    gen = torch.Generator().manual_seed(rows * 3 + D)
    dy = torch.randn(rows, D, generator=gen).to(dtype).to(cuda)
    dy2 = torch.randn(rows, D, generator=gen).to(dtype).to(cuda) if two else None
    s, mean, rstd = got["s"], got["mean"], got["rstd"]
    b = ln_bwd(dy, dy2, s, gamma, mean, rstd, p, SEED, want_da=p > 0)
    again = ln_bwd(dy, dy2, s, gamma, mean, rstd, p, SEED, want_da=p > 0)
    assert all(same(b[k], again[k]) for k in b if b[k] is not None), label
    bref = o.ln_backward(dy, dy2, s, gamma, mean, rstd, p, SEED)
    bb = o.ln_bwd_bounds(bref, bf)
    if p == 0:
        b["da"] = b["ds"]                                  # da NULL at p = 0: dbias is still the column sum of ds
    r.update({k: o.ratio(b[k], bref[k], bb[k]) for k in ("ds", "da", "dgamma", "dbeta", "dbias")})
    if p > 0:
        assert o.mask_exact(b["da"], bref["da"], bb["da"], bref["mask"]), label
    if nulls:                                              # ds NULL and da NULL: the statistics do not depend on them
        n = ln_bwd(dy, dy2, s, gamma, mean, rstd, p, SEED, want_ds=False, want_da=False)
        assert all(same(n[k], b[k]) for k in ("dgamma", "dbeta", "dbias")), label
    note(label, r, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_layernorm_small_rows(cuda, dtype):
    i = 0
    for D in LN_D[dtype]:
        for rows in LN_ROWS:
            ln_case(cuda, dtype, o.LN_KINDS[i % 6], rows, D, 0.1 if (i // 6) % 2 else 0.0, i % 3 != 0, i % 4 < 2, nulls=i % 5 == 0)
            i += 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", o.LN_KINDS)
def test_layernorm_every_family_every_option(cuda, dtype, kind):
    D = 776 if dtype == F32 else 520
    for p in (0.0, 0.1):
        for residual in (True, False):
            for two in (True, False):
                ln_case(cuda, dtype, kind, 65, D, p, residual, two)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", LN_ROWS_BIG)
def test_layernorm_grid_passes(cuda, dtype, rows):
    for i, D in enumerate(LN_D_BIG[dtype]):
        j = i + rows
        ln_case(cuda, dtype, o.LN_KINDS[j % 6], rows, D, 0.1 if j % 2 else 0.0, True, j % 3 == 0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_layernorm_forms_and_refusals(cuda, dtype):
    bf = dtype == BF16
    rows, D = 65, 520
    x, a = o.make_ln_input("mixed", rows, D, dtype)
    x, a = x.to(cuda), a.to(cuda)
    gamma, beta = (t.to(cuda) for t in o.make_affine(D))
    # ops.ln_bwd: da is ds at p = 0, its own tensor at p > 0
    s, y, mean, rstd = ops.ln_fwd(x, a, gamma, beta, p=0.0, seed=SEED)
    dy = torch.randn(rows, D, device=cuda).to(dtype)
    ds, da, dgm, dbt, dbs = ops.ln_bwd(dy, None, s, gamma, mean, rstd, 0.0, SEED)
    assert da is ds
    ds1, da1 = ops.ln_bwd(dy, None, s, gamma, mean, rstd, 0.1, SEED)[:2]
    assert da1 is not ds1 and same(ds1, ds)
    # the plain-LayerNorm form: x NULL, p = 0: s is not written and `a` itself is returned
    s0, y0, mean0, rstd0 = ops.ln_fwd(None, a, gamma, beta)
    assert s0 is a
    raw = ln_fwd(None, a, gamma, beta, want_s=False)
    assert same(raw["y"], y0) and same(raw["mean"], mean0) and same(raw["rstd"], rstd0)
    ref = o.ln_forward(None, a, gamma, beta)
    bnd = o.ln_fwd_bounds(ref, gamma, bf)
    ar = a.detach().clone().requires_grad_(True)
    gp, bp = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yf = ops.layer_norm(ar, gp, bp)
    yf.backward(dy)
    bref = o.ln_backward(dy, None, a, gamma, mean0, rstd0)
    bb = o.ln_bwd_bounds(bref, bf)
    note("ln %s plain form (LayerNormFn)" % NAME[dtype],
         dict(y=o.ratio(yf.detach(), ref["y"], bnd["y"]), mean=o.ratio(mean0, ref["mean"], bnd["mean"]),
              rstd=o.ratio(rstd0, ref["rstd"], bnd["rstd"]), ds=o.ratio(ar.grad, bref["ds"], bb["ds"]),
              dgamma=o.ratio(gp.grad, bref["dgamma"], bb["dgamma"]), dbeta=o.ratio(bp.grad, bref["dbeta"], bb["dbeta"])), dtype)
    # a mixed batch: every row is bitwise what it is when run alone (p = 0: the mask depends on the row's offset)
    full = ln_fwd(x, a, gamma, beta)
    fb = ln_bwd(dy, None, full["s"], gamma, full["mean"], full["rstd"], want_da=False)
    for r in range(0, rows, 7):
        one = ln_fwd(x[r:r + 1].clone(), a[r:r + 1].clone(), gamma, beta)
        assert all(same(one[k], full[k][r:r + 1]) for k in one), r
        ob = ln_bwd(dy[r:r + 1].clone(), None, one["s"], gamma, one["mean"], one["rstd"], want_da=False)
        assert same(ob["ds"], fb["ds"][r:r + 1]), r
    # refusals
    for Dbad, p in ((1032, 0.0), (12, 0.0), (520, 1.0)):
        t = torch.zeros(4, Dbad, dtype=dtype, device=cuda)
        w = torch.ones(Dbad, device=cuda)
        with pytest.raises(RuntimeError, match="1001"):
            ln_fwd(None, t, w, w, p=p)
        with pytest.raises(RuntimeError, match="1001"):
            ln_bwd(t, None, t, w, torch.zeros(4, device=cuda), torch.ones(4, device=cuda), p=p)


# ----------------------------------------------------------------------------------------------------------------------
# the device-resident seed offset
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_seed_offset_masks(cuda, dtype, monkeypatch):
    """seed + *seed_base on uint64, eager (no graph): the masks of all five dropout sites equal the oracle's for the summed
    key, element for element, and differ from the un-offset mask."""
    monkeypatch.setattr(ops, "_USE_SEED_BASE", True)
    base_t = ops.seed_base_tensor(cuda)
    rows, D, p = 33, 264, 0.1
    ones = torch.ones(rows, D, dtype=dtype, device=cuda)
    w = torch.ones(D, device=cuda)
    dy = (torch.randn(rows, D, device=cuda).abs() + 0.5).to(dtype)
    s0, _, mean, rstd = ops.ln_fwd(None, torch.randn(rows, D, device=cuda).to(dtype), w, w)
    plain = o.keep(SEED, p, rows, D, cuda)
    wrap = -(SEED - 5)                                    # seed + base = 5 + 2^64: the uint64 sum wraps
    assert SEED + (wrap % (1 << 64)) >= 1 << 64 and o.seed_key(SEED, wrap) == 5
    try:
        for base in (0, 12345, ops._SEED_STEP, wrap, -1):
            base_t.fill_(base)
            want = o.keep(SEED, p, rows, D, cuda, base=base)
            assert torch.equal(want, plain) == (base == 0)
            got = {}
            got["ln_fwd"] = ops.ln_fwd(None, ones, w, w, p=p, seed=SEED)[0] != 0
            ds, da = ops.ln_bwd(dy, None, s0, w, mean, rstd, p, SEED)[:2]
            assert bool((ds != 0).all())
            got["ln_bwd"] = da != 0
            h = ones.clone()
            got["gelu_fwd"] = ops.gelu_fwd(h, None, p, SEED, gd_inplace=True) != 0
            got["gelu_fwd gd"] = h != 0
            got["gelu_bwd"] = ops.gelu_bwd(dy, ones, None, p, SEED)[0] != 0
            got["posenc"] = ops.posenc_dropout(ones, None, 7, p, SEED) != 0
            for k, m in got.items():
                assert torch.equal(m, want), (k, base)
    finally:
        base_t.fill_(0)
    print("    seed offset %s: 6 sites x 5 bases (0, 12345, _SEED_STEP, a wrapping sum, -1) equal the oracle" % NAME[dtype])


# ----------------------------------------------------------------------------------------------------------------------
# GELU
# ----------------------------------------------------------------------------------------------------------------------
def gelu_case(cuda, dtype, kind, rows, Fd, p, with_bias, forward=True, backward=True):
    bf = dtype == BF16
    h = o.make_gelu_input(kind, rows, Fd, dtype, seed=rows + Fd).to(cuda)
    bias = torch.randn(Fd, generator=torch.Generator().manual_seed(Fd)).to(cuda) if with_bias else None
    label = "gelu %s %-6s %5dx%-4d p%.1f bias%d" % (NAME[dtype], kind, rows, Fd, p, with_bias)
    ref = o.gelu_forward(h, bias, p, SEED)
    r = {}
    if forward:
        fb = o.gelu_fwd_bounds(ref, bf)
        g0, _ = gelu_fwd(h, bias, p, SEED, gd=None)
        g1, gd1 = gelu_fwd(h, bias, p, SEED, gd="sep")
        g2, gd2 = gelu_fwd(h, bias, p, SEED, gd="alias")
        assert same(g0, g1) and same(g0, g2) and same(gd1, gd2), label
        assert torch.isfinite(g0.float()).all() and torch.isfinite(gd1.float()).all(), label
        assert o.mask_exact(g0, ref["g"], fb["g"], ref["mask"]) and o.mask_exact(gd1, ref["gd"], fb["gd"], ref["mask"]), label
        r.update(g=o.ratio(g0, ref["g"], fb["g"]), gd=o.ratio(gd1, ref["gd"], fb["gd"]))
    if backward:
        dg = torch.randn(rows, Fd, generator=torch.Generator().manual_seed(rows)).to(dtype).to(cuda)
        bref = o.gelu_backward(dg, ref)
        bb = o.gelu_bwd_bounds(ref, bref, bf)
        dh, db1 = gelu_bwd(dg, h, bias, p, SEED)
        dh2, db2 = gelu_bwd(dg, h, bias, p, SEED)
        dh3, _ = gelu_bwd(dg, h, bias, p, SEED, want_dbias=False)
        assert same(dh, dh2) and same(db1, db2) and same(dh, dh3) and torch.isfinite(dh.float()).all(), label
        assert o.mask_exact(dh, bref["dh"], bb["dh"], ref["mask"]), label
        r.update(dh=o.ratio(dh, bref["dh"], bb["dh"]), db1=o.ratio(db1, bref["db1"], bb["db1"]))
    note(label, r, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Fd", [8, 64, 1016, 1024, 1032, 2048, 2056])
def test_gelu_widths_and_slab_edges(cuda, dtype, Fd):
    i = Fd // 8
    for rows in (1, 7, 8, 9, 15, 16, 17):
        for kind in ("randn2", "ladder"):
            gelu_case(cuda, dtype, kind, rows, Fd, 0.1 if i % 2 else 0.0, i % 3 != 0, forward=rows <= 9 or kind == "ladder",
                      backward=rows not in (7, 8, 9) or kind == "ladder")
            i += 1


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [16384, 16385, 32768, 32769])
def test_gelu_grid_caps(cuda, dtype, rows):
    """More than 4096 slabs x 8 rows forward, 1024 x 16 rows backward: a slab takes a second row range."""
    gelu_case(cuda, dtype, "randn2" if rows % 2 else "ladder", rows, 64, 0.1, True, forward=rows >= 32768, backward=rows != 32768)


# ----------------------------------------------------------------------------------------------------------------------
# posenc, colsum
# ----------------------------------------------------------------------------------------------------------------------
def posenc_case(cuda, dtype, rows, D, T, p, with_pe, extra=3):
    x = torch.randn(rows, D, generator=torch.Generator().manual_seed(rows + D)).to(dtype).to(cuda)
    pe = torch.randn(T + extra, D, generator=torch.Generator().manual_seed(T)).to(cuda) if with_pe else None
    y = posenc(x, pe, T, p, SEED)
    ref = o.posenc_forward(x, pe, T, p, SEED)
    bnd = o.posenc_bounds(ref, dtype == BF16)
    assert o.mask_exact(y, ref["y"], bnd, ref["mask"])
    assert same(y, posenc(x, pe, T, p, SEED))
    note("posenc %s %7dx%-3d T%-4d p%.2f pe%d" % (NAME[dtype], rows, D, T, p, with_pe), dict(posenc=o.ratio(y, ref["y"], bnd)), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_posenc(cuda, dtype):
    rows = 33
    i = 0
    for D in (8, 128, 512):
        for T in (1, 7, rows, rows + 9):
            posenc_case(cuda, dtype, rows, D, T, 0.25 if i % 2 else 0.0, True)
            i += 1
        posenc_case(cuda, dtype, rows, D, 7, 0.25, False)
        posenc_case(cuda, dtype, rows, D, 7, 0.0, False)
    nd = 8 // (8 if dtype == BF16 else 4)
    for vectors in (1048576, 1048576 + 128):              # 4096 blocks x 256 threads, then the grid-stride wrap
        posenc_case(cuda, dtype, vectors // nd, 8, 1000, 0.25, True)
    # the backward through PosEncDropoutFn: the same mask on dy, no pe
    N, T, D, p = 3, 11, 128, 0.25
    x = torch.randn(N, T, D, device=cuda).to(dtype).requires_grad_(True)
    pe = torch.randn(T + 5, D, device=cuda)
    y = ops.PosEncDropoutFn.apply(x, pe, p, SEED)
    dy = torch.randn(N, T, D, device=cuda).to(dtype)
    y.backward(dy)
    ref = o.posenc_forward(x.detach().view(N * T, D), pe, T, p, SEED)
    bref = o.posenc_forward(dy.view(N * T, D), None, T, p, SEED)
    bf = dtype == BF16
    note("posenc %s PosEncDropoutFn fwd + bwd" % NAME[dtype],
         dict(posenc=max(o.ratio(y.detach().view(N * T, D), ref["y"], o.posenc_bounds(ref, bf)),
                         o.ratio(x.grad.view(N * T, D), bref["y"], o.posenc_bounds(bref, bf)))), dtype)
    assert o.mask_exact(x.grad.view(N * T, D), bref["y"], o.posenc_bounds(bref, bf), bref["mask"])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ncols", [8, 1536])
def test_colsum(cuda, dtype, ncols):
    for rows in (1, 63, 64, 65, 32768, 32769):
        for ld in (ncols, ncols + 8):
            x = torch.randn(rows, ld, generator=torch.Generator(device=cuda).manual_seed(rows), device=cuda).to(dtype)[:, :ncols]
            got = colsum(x)
            assert same(got, colsum(x)) and same(got, ops.colsum(x))
            ref, bnd = o.colsum_reference(x), o.colsum_bound(x)
            note("colsum %s %5dx%-4d ld %d" % (NAME[dtype], rows, ncols, ld), dict(colsum=o.ratio(got, ref, bnd)), dtype)
            if rows == 65:                                # tooth: the last row split left out of the reference
                t = o.ratio(got, o.colsum_reference(x, o.last_split_rows(rows, o.colsum_blocks(rows), cuda)), bnd)
                print("    tooth colsum last split dropped %s: %.3g" % (NAME[dtype], t))
                assert t >= o.TEETH


# ----------------------------------------------------------------------------------------------------------------------
# teeth on the kernels' own results
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_teeth_on_the_kernels(cuda, dtype):
    bf = dtype == BF16
    rows, D, p = 65, 520, 0.1
    gamma, beta = (t.to(cuda) for t in o.make_affine(D))
    for kind, mut, keys in (("tiny", "eps6", ("rstd", "y")), ("randn", "swap", ("s", "y"))):
        x, a = (t.to(cuda) for t in o.make_ln_input(kind, rows, D, dtype))
        got = ln_fwd(x, a, gamma, beta, p, SEED)
        right = o.ln_forward(x, a, gamma, beta, p=p, seed=SEED)
        bnd = o.ln_fwd_bounds(right, gamma, bf)
        assert all(o.ratio(got[k], right[k], bnd[k]) <= 1 for k in got)
        wrong = o.ln_forward(x, a, gamma, beta, p=p, seed=SEED, mut=mut)
        for k in keys:
            t = o.ratio(got[k], wrong[k], bnd[k])
            print("    tooth ln %s %s %s: %.3g" % (mut, k, NAME[dtype], t))
            assert t >= o.TEETH, (mut, k, t)
    h = o.make_gelu_input("randn2", 33, 1032, dtype).to(cuda)
    dg = torch.randn(33, 1032, device=cuda).to(dtype)
    ref = o.gelu_forward(h, None, p, SEED)
    wrong = o.gelu_forward(h, None, p, SEED, mut="swap")
    fb = o.gelu_fwd_bounds(ref, bf)
    g, gd = gelu_fwd(h, None, p, SEED)
    dh, _ = gelu_bwd(dg, h, None, p, SEED)
    y = posenc(h, None, 7, p, SEED)
    pr, pw = o.posenc_forward(h, None, 7, p, SEED), o.posenc_forward(h, None, 7, p, SEED, mut="swap")
    bref = o.gelu_backward(dg, ref)
    for label, got_, w_, r_, b_ in (("gelu g", g, wrong["g"], ref["g"], fb["g"]), ("gelu gd", gd, wrong["gd"], ref["gd"], fb["gd"]),
                                    ("gelu dh", dh, o.gelu_backward(dg, wrong)["dh"], bref["dh"], o.gelu_bwd_bounds(ref, bref, bf)["dh"]),
                                    ("posenc", y, pw["y"], pr["y"], o.posenc_bounds(pr, bf))):
        assert o.ratio(got_, r_, b_) <= 1
        t = o.ratio(got_, w_, b_)
        print("    tooth %s swap %s: %.3g" % (label, NAME[dtype], t))
        assert t >= o.TEETH, (label, t)


def test_worst_ratios_summary(cuda):
    """The record of profiles/elementwise_f64_ratios.txt: worst measured / bound per quantity and dtype (runs last)."""
    for (k, d), v in sorted(WORST.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("    worst %-7s %-5s %.3f" % (k, d, v))
    assert all(v <= 1 for v in WORST.values())

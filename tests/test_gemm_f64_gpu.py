"""GPU: the bf16 GEMM family -- cwlt_gemm_bf16 (256 x 256 persistent tiles), the FFN epilogues cwlt_gemm_nt_mul /
cwlt_gemm_nt_bias_gelu_dropout on the 128 x 256 and on the 256 x 256 kernel, the LayerNorm epilogue
(cwlt_gemm_nt_bias_dropout_add_layernorm), cwlt_gemm_bf16_small / _small_gelu and the weight gradients cwlt_wgrad_bf16 /
_group -- PER ELEMENT against the f64 result of the same bf16 operands, under the bounds derived in
oracle/gemm_f64.py (pinned by tests/test_oracle_gemm_f64_cpu.py), at the smallest shapes that reach each tile edge and each
dispatch branch of the launchers.  The instantiations behind switches that are read once per process run in child
processes, one per set of switches.  Every figure is the worst |error| / bound of its case (<= 1 passes); run with -s for
the figures.  Measured on an MI355X: profiles/gemm_f64_ratios.txt."""
import os
import subprocess
import sys

import pytest
import torch

import rlmg_amd  # noqa: F401
from oracle import gemm_f64 as o
from rlmg_amd import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def note(label, ratios):
    print("    %-58s %s" % (label, "  ".join("%s %.2f" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (label, bad)


@pytest.fixture(autouse=True)
def _all_rows(monkeypatch):
    monkeypatch.setattr(ops, "GEMM_BF16_MIN_ROWS", 0)
    yield
    _lib.load().cwlt_gemm_bf16_tune(-1, None)


def keep_mask(M, N, p, seed, dev):
    """The dropout stream keyed by (seed, row * N + column), from another kernel: never from the output under test."""
    if p == 0:
        return torch.ones(M, N, dtype=torch.bool)
    return (ops.posenc_dropout(torch.ones(M, N, device=dev), None, 1, p=p, seed=seed) != 0).cpu()


# ----------------------------------------------------------------------------------------------------------------------
# plain forms: cwlt_gemm_bf16 and cwlt_gemm_bf16_small
# ----------------------------------------------------------------------------------------------------------------------
def run_plain(fn, count, dev, a, w, bias, c0, forms=o.FORMS):
    """fn(a, w, bias, out, accumulate) -> out on every form; count(bias, acc) -> n.  {form: worst ratio}."""
    ad, wd, bd = a.to(dev), w.to(dev), bias.to(dev)
    M, N = a.shape[0], w.shape[0]
    res = {}
    for has_bias, acc in forms:
        out = c0.to(dev) if acc else torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
        got = fn(ad, wd, bd if has_bias else None, out, acc)
        assert got.data_ptr() == out.data_ptr() and got.dtype == torch.bfloat16
        ref, S = o.plain_reference(a, w, bias if has_bias else None, c0 if acc else None)
        res[o.form_name(has_bias, acc)] = o.worst(o.plain_ratios(got, ref, S, count(has_bias, acc)))
    return res


def big_fn(a, w, bias, out, acc):
    return ops.gemm_bf16(a, w, bias, out=out, accumulate=acc)


def small_fn(a, w, bias, out, acc):
    return ops.gemm_bf16_small(a, w, bias, out=out, accumulate=acc)


@pytest.mark.parametrize("M,N,K,bias,acc", o.big_cases())
def test_gemm_bf16_per_element(cuda, M, N, K, bias, acc):
    a, w, b, c0 = o.make_operands(M, N, K, 7 * M + N + K)
    r = run_plain(big_fn, lambda hb, ac: o.n_big(K, hb, ac), cuda, a, w, b, c0, forms=((bias, acc),))
    note("gemm_bf16 %4d x %4d x %4d" % (M, N, K), r)


@pytest.mark.parametrize("K", [128, 576])
def test_gemm_bf16_cancelling_rows_and_exact_integers(cuda, K):
    M, N = 257, 264
    a, w, b, c0 = o.make_cancelling(M, N, K, K)
    prod, S = o.product(a, w)
    assert prod.abs().median() < 0.05 * S.median()                   # the maker cancels
    note("gemm_bf16 cancelling %d x %d x %d" % (M, N, K), run_plain(big_fn, lambda hb, ac: o.n_big(K, hb, ac), cuda, a, w, b, c0))
    a, w = o.make_integers(M, N, K, 11)
    ref = a.double() @ w.double().t()
    got = ops.gemm_bf16(a.to(cuda), w.to(cuda)).double().cpu()
    exact = ref.abs() <= 256
    assert exact.float().mean() > 0.9 and torch.equal(got[exact], ref[exact])


def test_gemm_bf16_last_float_of_the_bias_strip_and_the_limit(cuda):
    """N = 8192 is the bias strip's limit (the strip's last float belongs to the last column); N = 8200 is refused with a
    bias and right without one."""
    a, w, b, c0 = o.make_operands(1, 8192, 128, 3)
    r = run_plain(big_fn, lambda hb, ac: o.n_big(128, hb, ac), cuda, a, w, b, c0, forms=((True, False), (True, True)))
    note("gemm_bf16    1 x 8192 x  128", r)
    a, w, b, c0 = o.make_operands(129, 8200, 128, 4)
    with pytest.raises(RuntimeError):
        ops.gemm_bf16(a.to(cuda), w.to(cuda), b.to(cuda))
    r = run_plain(big_fn, lambda hb, ac: o.n_big(128, hb, ac), cuda, a, w, b, c0, forms=((False, False), (False, True)))
    note("gemm_bf16  129 x 8200 x  128", r)


@pytest.mark.parametrize("bias", [False, True])
def test_gemm_bf16_accumulates_into_a_column_block(cuda, bias):
    """The accumulating forms on an output view with ldc = 3 N; the neighbouring blocks stay untouched."""
    M, N, K = 257, 264, 192
    a, w, b, c0 = o.make_operands(M, N, K, 9, lda=3 * K, ldw=K + 64)
    big_a = torch.zeros(M, 3 * K, dtype=torch.bfloat16, device=cuda)
    big_a[:, K:2 * K] = a.to(cuda)
    big_w = torch.zeros(N, K + 64, dtype=torch.bfloat16, device=cuda)
    big_w[:, :K] = w.to(cuda)
    big_c = torch.full((M, 3 * N), 3.0, dtype=torch.bfloat16, device=cuda)
    big_c[:, N:2 * N] = c0.to(cuda)
    cv = big_c[:, N:2 * N]
    assert cv.stride(0) == 3 * N
    ops.gemm_bf16(big_a[:, K:2 * K], big_w[:, :K], b.to(cuda) if bias else None, out=cv, accumulate=True)
    ref, S = o.plain_reference(a, w, b if bias else None, c0)
    note("gemm_bf16 view ldc = 3 N", {o.form_name(bias, True): o.worst(o.plain_ratios(cv, ref, S, o.n_big(K, bias, True)))})
    assert torch.all(big_c[:, :N] == 3.0) and torch.all(big_c[:, 2 * N:] == 3.0)


@pytest.mark.parametrize("variant", [1 << 8])
@pytest.mark.parametrize("K", [128, 192])
def test_gemm_bf16_several_tiles_per_workgroup(cuda, variant, K):
    """8 workgroups: 9 row tiles padded to 16, three column tiles with the last one partial, six tiles per workgroup with
    padding tiles among them, all four forms."""
    M, N = 2049, 520
    a, w, b, c0 = o.make_operands(M, N, K, 100 + K)
    _lib.load().cwlt_gemm_bf16_tune(variant, None)
    note("gemm_bf16 variant %d  %d x %d x %d" % (variant, M, N, K),
         run_plain(big_fn, lambda hb, ac: o.n_big(K, hb, ac), cuda, a, w, b, c0))


@pytest.mark.parametrize("K", o.SMALL_K)
def test_gemm_bf16_small_per_element(cuda, K):
    """Whole-K (K % 128 != 0) and the split-K instantiations PD = 1, 2, 1, 4, 2, 8, 4; the rows bracket the switch from the
    32 x 32 to the 64 x 64 tile; strided operands and output."""
    res = {}
    for M in o.SMALL_M:
        for N in o.SMALL_N:
            a, w, b, c0 = o.make_operands(M, N, K, 13 * M + N + K, lda=K + 24, ldw=K + 8)
            wa = torch.zeros(M, K + 24, dtype=torch.bfloat16, device=cuda)
            wa[:, :K] = a.to(cuda)
            ww = torch.zeros(N, K + 8, dtype=torch.bfloat16, device=cuda)
            ww[:, :K] = w.to(cuda)
            ad, wd = (wa[:, :K], ww[:, :K]) if (M + N // 8) % 2 else (a.to(cuda), w.to(cuda))
            for hb, acc in o.FORMS:
                big = torch.full((M, N + 16), 7.0, dtype=torch.bfloat16, device=cuda)
                out = big[:, 8:8 + N]
                if acc:
                    out.copy_(c0.to(cuda))
                ops.gemm_bf16_small(ad, wd, b.to(cuda) if hb else None, out=out, accumulate=acc)
                ref, S = o.plain_reference(a, w, b if hb else None, c0 if acc else None)
                r = o.worst(o.plain_ratios(out, ref, S, o.n_small(M, K, hb, acc)))
                res[o.form_name(hb, acc)] = max(res.get(o.form_name(hb, acc), 0.0), r)
                assert torch.all(big[:, :8] == 7.0) and torch.all(big[:, 8 + N:] == 7.0)
    note("gemm_small K = %4d, M in %s, N in %s" % (K, o.SMALL_M, o.SMALL_N), res)


@pytest.mark.parametrize("M", [16384, 16385])
def test_gemm_bf16_small_at_the_split_k_row_limit(cuda, M):
    """The last split-K launch and the first whole-K launch with K % 128 == 0."""
    a, w, b, c0 = o.make_operands(M, 8, 128, M)
    note("gemm_small %d x 8 x 128" % M, run_plain(small_fn, lambda hb, ac: o.n_small(M, 128, hb, ac), cuda, a, w, b, c0))


def test_gemm_bf16_small_cancelling_rows(cuda):
    M, N, K = 257, 72, 768
    a, w, b, c0 = o.make_cancelling(M, N, K, 5)
    note("gemm_small cancelling %d x %d x %d" % (M, N, K),
         run_plain(small_fn, lambda hb, ac: o.n_small(M, K, hb, ac), cuda, a, w, b, c0))


@pytest.mark.parametrize("K", o.SMALL_GELU_K)
def test_gemm_bf16_small_gelu(cuda, K):
    """PD = 1, 2, 4, 8 of the GELU form: bit for bit the two-kernel chain, and against f64."""
    res = {}
    for M, N, p in ((1, 8, 0.0), (33, 72, 0.1), (255, 40, 0.1), (257, 64, 0.0)):
        a, w, b, _ = o.make_operands(M, N, K, 31 * M + K)
        ad, wd, bd = a.to(cuda), w.to(cuda), b.to(cuda)
        seed = 1234 + M
        g, gd = ops.gemm_bf16_small_gelu(ad, wd, bd, p, seed)
        g_only, none = ops.gemm_bf16_small_gelu(ad, wd, bd, p, seed, want_gd=False)
        assert none is None and torch.equal(g_only, g)
        if M <= 256:       # the chain's product comes from the same split-K 32 x 32 kernel below 256 rows
            h = ops.gemm_bf16_small(ad, wd)
            g_ref = ops.gelu_fwd(h, bd, p, seed, gd_inplace=True)       # h now holds gd
            assert torch.equal(g, g_ref) and torch.equal(gd, h)
        keep = keep_mask(M, N, p, seed, cuda)
        rg, rgd = o.gelu_ratios(g, gd, a, w, b, keep, o.drop_scale(p), o.n_small_gelu(K))
        res["g"] = max(res.get("g", 0.0), o.worst(rg))
        res["gd"] = max(res.get("gd", 0.0), o.worst(rgd))
    note("gemm_small_gelu K = %4d" % K, res)


# ----------------------------------------------------------------------------------------------------------------------
# FFN epilogues (128 x 256 kernel by default at these rows; the 256 x 256 persistent kernel under CWLT_FFN_BIG_MIN_ROWS=1)
# ----------------------------------------------------------------------------------------------------------------------
def nt_mul(a, w, g, c, want_colsum):
    """cwlt_gemm_nt_mul with the caller's c (its row stride is an argument)."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    part = cs = None
    if want_colsum:
        part = torch.empty(lib.cwlt_gemm_nt_tiles(M) * N, dtype=torch.float32, device=a.device)
        cs = torch.full((N,), float("nan"), dtype=torch.float32, device=a.device)
    ops._call("cwlt_gemm_nt_mul", _lib.dev(a), _lib.dev(w), _lib.dev(g), _lib.dev(c), _lib.opt(part), _lib.opt(cs), M, N, K,
              a.stride(0), w.stride(0), g.stride(0), c.stride(0), _lib.stream_ptr())
    return cs


def run_mul(dev, M, N, K, p, big=False, strided=False):
    a, w, _, _ = o.make_operands(M, N, K, 3 * M + N + K)
    gd = o.make_gd(M, N, M + K, p)
    ad, wd = a.to(dev), w.to(dev)
    res, first = {}, None
    for want in (True, False):
        if strided:
            gw = torch.full((M, N + 8), 9.0, dtype=torch.bfloat16, device=dev)
            gw[:, :N] = gd.to(dev)
            gv = gw[:, :N]
            cw = torch.full((M, 2 * N), 5.0, dtype=torch.bfloat16, device=dev)
            cv = cw[:, N:]
            cs = nt_mul(ad, wd, gv, cv, want)
            assert torch.all(cw[:, :N] == 5.0)
        else:
            out = ops.gemm_nt_mul(ad, wd, gd.to(dev), want_colsum=want)
            cv, cs = out if want else (out, None)
        if want:
            first = cv.clone()
            on_big = big and not strided                       # a strided g or c keeps the 128 x 256 kernel
            rc, rs = o.mul_ratios(cv, cs, a, w, gd, o.n_big(K) if on_big else o.n_nt(K), o.n_colsum(M, big=on_big))
            res = {"c": o.worst(rc), "colsum": o.worst(rs)}
        else:
            assert torch.equal(cv, first)                      # without the sums: the same c, bit for bit
    return res


def run_gelu(dev, M, N, K, p, big=False):
    a, w, b, _ = o.make_operands(M, N, K, 5 * M + N + K)
    seed = 777 + M + K
    g, gd = ops.ffn1_gelu_dropout(a.to(dev), w.to(dev), b.to(dev), p, seed)
    keep = keep_mask(M, N, p, seed, dev)
    if p > 0 and M * N >= 1 << 15:
        assert abs(1 - keep.float().mean().item() - p) < 0.02
    rg, rgd = o.gelu_ratios(g, gd, a, w, b, keep, o.drop_scale(p), o.n_big(K) if big else o.n_nt(K))
    return {"g": o.worst(rg), "gd": o.worst(rgd)}


def merge(into, res):
    for k, v in res.items():
        into[k] = max(into.get(k, 0.0), v)


def run_ffn_cases(dev, Ms, Ks, big, label):
    for M in Ms:
        mul, gelu, strd = {}, {}, {}
        for N in o.NT_N:
            for K in Ks:
                for p in o.NT_P:
                    merge(mul, run_mul(dev, M, N, K, p, big=big))
                    merge(gelu, run_gelu(dev, M, N, K, p, big=big))
                merge(strd, run_mul(dev, M, N, K, 0.1, big=big, strided=True))
        note("%s mul  M = %4d, N in %s, K in %s" % (label, M, o.NT_N, Ks), mul)
        note("%s mul, g and c strided%s  M = %4d" % (label, " (dispatched to the 128 x 256 kernel)" if big else "", M), strd)
        note("%s gelu M = %4d, N in %s, K in %s" % (label, M, o.NT_N, Ks), gelu)


@pytest.mark.parametrize("M", o.NT_M)
def test_ffn_epilogues_on_the_128_x_256_kernel(cuda, M):
    run_ffn_cases(cuda, (M,), o.NT_K, False, "gemm_nt 128x256")


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm epilogue
# ----------------------------------------------------------------------------------------------------------------------
def run_ln(dev, M, K, p, strided):
    N = o.LN_N
    a, w, b, _ = o.make_operands(M, N, K, 11 * M + K, lda=3 * K if strided else None, ldw=K + 64 if strided else None)
    x, gamma, beta = o.make_ln(M, N, M + K)
    if strided:
        wa = torch.zeros(M, 3 * K, dtype=torch.bfloat16, device=dev)
        wa[:, K:2 * K] = a.to(dev)
        ww = torch.zeros(N, K + 64, dtype=torch.bfloat16, device=dev)
        ww[:, :K] = w.to(dev)
        ad, wd = wa[:, K:2 * K], ww[:, :K]
    else:
        ad, wd = a.to(dev), w.to(dev)
    seed = 4000 + M + K
    s, y, mean, rstd = ops.linear_ln(ad, wd, b.to(dev), x.to(dev), gamma.to(dev), beta.to(dev), p=p, seed=seed)
    keep = keep_mask(M, N, p, seed, dev)
    r = o.ln_ratios(s, y, mean, rstd, a, w, b, x, gamma, beta, keep, o.drop_scale(p), o.n_nt(K))
    return {k: o.worst(v) for k, v in r.items()}


@pytest.mark.parametrize("K", o.LN_K)
def test_layernorm_epilogue_per_row(cuda, K):
    for strided in (False, True):
        for p in (0.0, 0.1):
            res = {}
            for M in o.LN_M:
                merge(res, run_ln(cuda, M, K, p, strided))
            note("gemm_ln K = %4d, p = %.1f, M in %s%s" % (K, p, o.LN_M, ", lda = 3 K, ldw = K + 64" if strided else ""), res)


# ----------------------------------------------------------------------------------------------------------------------
# weight gradients
# ----------------------------------------------------------------------------------------------------------------------
def run_wgrad(dev, M, N1, N2, strided):
    a, b = o.make_wgrad(M, N1, N2, M + N1 + N2, strided)
    if strided:
        wa = torch.empty(M, N1 + 24, dtype=torch.bfloat16, device=dev).copy_(a._base)
        wb = torch.empty(M, N2 + 72, dtype=torch.bfloat16, device=dev).copy_(b._base)
        ad, bd = wa[:, 8:8 + N1], wb[:, 64:64 + N2]
    else:
        ad, bd = a.to(dev), b.to(dev)
    got = ops.wgrad(ad, bd)
    assert torch.equal(got, ops.wgrad(ad, bd))                         # fixed summation order
    ref, S = o.wgrad_reference(a, b)
    res = {"plain": o.worst(o.f32_ratios(got, ref, S, o.n_wgrad(M, N1, N2, False)))}
    out0 = torch.randn(N1, N2, generator=torch.Generator().manual_seed(M))
    acc = out0.to(dev)
    ops.wgrad(ad, bd, out=acc, accumulate=True)
    ref, S = o.wgrad_reference(a, b, out0)
    res["acc"] = o.worst(o.f32_ratios(acc, ref, S, o.n_wgrad(M, N1, N2, True)))
    return res


@pytest.mark.parametrize("M", o.WG_M)
def test_wgrad_per_element(cuda, M):
    """M = 2561: S = 10 slices of 288 rows, the last one empty (plain slice order); M = 4097: S = 16 of 288, the last one
    empty (XCD order), for the 256 x 256 tilings with one tile; fewer rows than a 32-row step; widths of one 8-column chunk."""
    for strided in (False, True):
        res = {}
        for N1, N2 in o.WG_WIDTHS:
            merge(res, run_wgrad(cuda, M, N1, N2, strided))
        note("wgrad M = %4d%s" % (M, ", column slices" if strided else ""), res)
    if M in (2561, 4097):
        assert o.wgrad_slices(M, 256, 256)[0] * o.wgrad_slices(M, 256, 256)[1] - M >= o.wgrad_slices(M, 256, 256)[1]


@pytest.mark.parametrize("M", [2561, 4097])
def test_wgrad_group_with_an_empty_slice(cuda, M):
    """Bit for bit the separate launches, and within the f64 bound."""
    g = torch.Generator().manual_seed(M)
    mk = lambda n: torch.randn(M, n, generator=g).bfloat16()
    pairs = [(mk(256), mk(256)), (mk(512), mk(256)), (mk(256), mk(512))]
    dp = [(a.to(cuda), b.to(cuda)) for a, b in pairs]
    one = [ops.wgrad(a, b) for a, b in dp]
    grp = ops.wgrad_group(dp)
    res = {}
    for (a, b), x, y in zip(pairs, one, grp):
        assert torch.equal(x, y)
        ref, S = o.wgrad_reference(a, b)
        merge(res, {"group": o.worst(o.f32_ratios(y, ref, S, o.n_wgrad(M, a.shape[1], b.shape[1])))})
    outs = [torch.full_like(x, 0.5) for x in one]
    ops.wgrad_group(dp, accumulate=True, outs=outs)
    for x, y in zip(one, outs):
        assert torch.equal(x + 0.5, y)
    note("wgrad_group M = %d" % M, res)


# ----------------------------------------------------------------------------------------------------------------------
# instantiations behind switches that are read once per process: one child process per set of switches
# ----------------------------------------------------------------------------------------------------------------------
def child_ffn_big(dev):
    """CWLT_FFN_BIG_MIN_ROWS=1: the FFN forms on the 256 x 256 persistent kernel (ragged last row tile, column-sum partials
    of that tile), then several tiles per workgroup (the sums' LDS strip reused between a workgroup's tiles)."""
    run_ffn_cases(dev, o.FFN_BIG_M, o.FFN_BIG_K, True, "gemm_bf16 256x256 ffn")
    _lib.load().cwlt_gemm_bf16_tune(1 << 8, None)
    try:
        run_ffn_cases(dev, (2049,), o.FFN_BIG_K, True, "gemm_bf16 256x256 ffn, 8 workgroups")
    finally:
        _lib.load().cwlt_gemm_bf16_tune(-1, None)


def child_whole_k_small(dev):
    """CWLT_GEMM_SMALL_SPLITK=0: whole-K gemm_small at K % 128 == 0."""
    for K in (128, 256, 512, 1536):
        res = {}
        for M, N in ((1, 8), (33, 72), (257, 40)):
            a, w, b, c0 = o.make_operands(M, N, K, M + N + K)
            merge(res, run_plain(small_fn, lambda hb, ac: o.n_small(M, K, hb, ac, splitk=False), dev, a, w, b, c0))
        note("gemm_small whole K = %4d" % K, res)


CHILDREN = {
    "child_ffn_big": {"CWLT_FFN_BIG_MIN_ROWS": "1"},
    "child_whole_k_small": {"CWLT_GEMM_SMALL_SPLITK": "0"},
}


@pytest.mark.parametrize("name", sorted(CHILDREN))
def test_switched_instantiations_in_a_process_of_their_own(cuda, name):
    code = ("import sys\nsys.path[:0] = [%r, %r]\nimport torch\nimport test_gemm_f64_gpu as t\n"
            "t.%s(torch.device('cuda:0'))\nprint('ok')\n" % (ROOT, os.path.join(ROOT, "tests"), name))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **CHILDREN[name]), capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, end="")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr

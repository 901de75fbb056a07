"""CPU pin of oracle/gemm_f64.py, the references, inputs, measures and bounds of tests/test_gemm_f64_gpu.py: the f64 forms
equal torch's own functions, the input makers have the properties they promise, the slice arithmetic restated from
cwlt_wgrad_bf16 gives the empty slices the GPU cases are chosen for, torch's f32 chain on the CPU (a stand-in for the kernels:
the same formulas and rounding points, other summation orders) stays inside every bound at every (N, K) of the GPU case
lists, every mutant of that chain falls outside its bound at every K of the lists (2048 included), and the both-neighbours
rule accepts the product rounded either way and nothing else.  No kernel runs here.  Run with -s for the figures."""
import pytest
import torch
import torch.nn.functional as F

from oracle import gemm_f64 as o

ALL_K = sorted(set(o.BIG_K + o.SMALL_K + o.NT_K + o.LN_K + o.FFN_BIG_K))
PLAIN_MUTANTS = ("bias_bf16", "splitk_bf16", "double_round", "drop_k", "c0_row", "bias_col")


def say(label, **kv):
    print("    %-52s %s" % (label, "  ".join("%s %.2f" % i for i in kv.items())))


def keep_of(M, N, p, seed):
    return torch.rand(M, N, generator=torch.Generator().manual_seed(seed)) >= p


# ----------------------------------------------------------------------------------------------------------------------
# references, makers, counts
# ----------------------------------------------------------------------------------------------------------------------
def test_references_equal_torch():
    x = torch.randn(1000, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).mul(3).requires_grad_(True)
    y = F.gelu(x)
    (dy,) = torch.autograd.grad(y.sum(), x)
    g, gd = o.gelu64(x.detach())
    assert (g - y.detach()).abs().max() < 1e-14 and (gd - dy).abs().max() < 1e-14
    grid = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    d1 = o.gelu64(grid)[1]
    d2 = (d1[2:] - d1[:-2]) / (grid[2] - grid[0])
    assert d1.abs().max() <= o.GELU_D1 and d2.abs().max() <= o.GELU_D2
    M, K, N = 37, 128, o.LN_N
    a, w, b, _ = o.make_operands(M, N, K, 1)
    xr, gamma, beta = o.make_ln(M, N, 2)
    keep = keep_of(M, N, 0.1, 3)
    s, yy, mean, rstd = o.emulate_ln(a, w, b, xr, gamma, beta, keep, o.drop_scale(0.1))
    sref = xr.double() + keep.double() * o.drop_scale(0.1) * ((a.double() @ w.double().t()).float().bfloat16().double() + b.double())
    yref = F.layer_norm(sref, (N,), gamma.double(), beta.double(), o.LN_EPS)
    r = o.ln_ratios(yref * 0 + sref, yref, sref.mean(1), 1 / torch.sqrt(sref.var(1, unbiased=False) + o.LN_EPS), a, w, b, xr,
                    gamma, beta, keep, o.drop_scale(0.1), o.n_nt(K))
    assert all(o.worst(v) < 1e-6 for v in r.values()), {k: o.worst(v) for k, v in r.items()}     # the reference itself: 0


def test_makers_and_slice_arithmetic():
    a, w, b, c0 = o.make_operands(64, 72, 256, 5, lda=3 * 256, ldw=256 + 64)
    assert a.stride(0) == 768 and w.stride(0) == 320 and a.dtype == torch.bfloat16 and b.dtype == torch.float32
    ref, S = o.plain_reference(*o.make_operands(300, 264, 512, 6))
    hi, lo = ref.abs().quantile(0.99), ref.abs().quantile(0.05)
    assert hi / lo > 2 ** 5                                        # several binades: what makes a per-element bound bite
    a, w, b, c0 = o.make_cancelling(65, 72, 256, 7)
    prod, S = o.product(a, w)
    assert prod.abs().median() < 0.05 * S.median()
    a, w = o.make_integers(64, 64, 128, 11)
    ref = a.double() @ w.double().t()
    assert torch.equal(ref, ref.round()) and torch.equal(o.emulate_plain(a, w).double()[ref.abs() <= 256], ref[ref.abs() <= 256])
    a, bb = o.make_wgrad(40, 8, 264, 1, strided=True)
    assert a.stride(0) == 32 and bb.stride(0) == 336 and (a._base[:, :8] == 100).all() and a.storage_offset() % 8 == 0
    # the empty slices the GPU cases are chosen for (the issue's figures)
    assert o.wgrad_slices(2561, 256, 256)[:2] == (10, 288) and o.wgrad_slices(4097, 256, 256)[:2] == (16, 288)
    assert 9 * 288 >= 2561 and 15 * 288 >= 4097                  # slice 9 / slice 15 start past the last row
    assert o.wgrad_slices(31, 8, 8)[:2] == (1, 32)
    assert o.drop_scale(0.0) == 1.0 and o.drop_scale(0.1) == float(torch.tensor(65536.0 / (65536 - 6554), dtype=torch.float32))
    assert abs(o.drop_scale(0.1) * 0.9 - 1) < 2.0 ** -17 and o.drop_scale(0.5) == 2.0
    assert [o.small_splitk(M, 128) for M in (16384, 16385)] == [True, False] and not o.small_splitk(1, 96)


# ----------------------------------------------------------------------------------------------------------------------
# the f32 chain stays inside every bound
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", o.BIG_K)
def test_plain_emulation_inside_the_bound_big(K):
    res = {}
    for N in o.BIG_N + (8192,):
        M = 257 if N < 8192 else 3
        a, w, b, c0 = o.make_operands(M, N, K, 7 * M + N + K)
        for hb, acc in o.FORMS:
            ref, S = o.plain_reference(a, w, b if hb else None, c0 if acc else None)
            got = o.emulate_plain(a, w, b if hb else None, c0 if acc else None)
            r = o.worst(o.plain_ratios(got, ref, S, o.n_big(K, hb, acc)))
            res[o.form_name(hb, acc)] = max(res.get(o.form_name(hb, acc), 0), r)
    say("256 x 256 counts, K = %d" % K, **res)
    assert max(res.values()) <= 1


@pytest.mark.parametrize("K", o.SMALL_K)
def test_plain_emulation_inside_the_bound_small(K):
    res = {}
    for N in o.SMALL_N:
        for M in (33, 257):
            a, w, b, c0 = o.make_operands(M, N, K, 13 * M + N + K)
            for hb, acc in o.FORMS:
                ref, S = o.plain_reference(a, w, b if hb else None, c0 if acc else None)
                got = o.emulate_plain(a, w, b if hb else None, c0 if acc else None)
                for sk in (True, False):
                    r = o.worst(o.plain_ratios(got, ref, S, o.n_small(M, K, hb, acc, splitk=sk)))
                    res[o.form_name(hb, acc)] = max(res.get(o.form_name(hb, acc), 0), r)
    say("small-tile counts, K = %d" % K, **res)
    assert max(res.values()) <= 1


@pytest.mark.parametrize("K", [128, 576, 2048])
def test_plain_emulation_inside_the_bound_on_cancelling_rows(K):
    a, w, b, c0 = o.make_cancelling(257, 264, K, K)
    res = {}
    for hb, acc in o.FORMS:
        ref, S = o.plain_reference(a, w, b if hb else None, c0 if acc else None)
        got = o.emulate_plain(a, w, b if hb else None, c0 if acc else None)
        res[o.form_name(hb, acc)] = o.worst(o.plain_ratios(got, ref, S, o.n_big(K, hb, acc)))
    say("cancelling rows, K = %d" % K, **res)
    assert max(res.values()) <= 1


@pytest.mark.parametrize("K", sorted(set(o.NT_K + o.FFN_BIG_K)))
def test_ffn_emulations_inside_their_bounds(K):
    res = {}
    for N in o.NT_N:
        for p in o.NT_P:
            M = 300
            a, w, b, _ = o.make_operands(M, N, K, 3 * M + N + K)
            gd = o.make_gd(M, N, M + K, p)
            c, cs = o.emulate_mul(a, w, gd)
            for big in ((False, True) if K >= 128 else (False,)):
                rc, rs = o.mul_ratios(c, cs, a, w, gd, o.n_big(K) if big else o.n_nt(K), o.n_colsum(M, big))
                res["c"] = max(res.get("c", 0), o.worst(rc))
                res["colsum"] = max(res.get("colsum", 0), o.worst(rs))
                keep = keep_of(M, N, p, K)
                g, gdd = o.emulate_gelu(a, w, b, keep, o.drop_scale(p))
                rg, rgd = o.gelu_ratios(g, gdd, a, w, b, keep, o.drop_scale(p), o.n_big(K) if big else o.n_nt(K))
                res["g"] = max(res.get("g", 0), o.worst(rg))
                res["gd"] = max(res.get("gd", 0), o.worst(rgd))
    say("FFN epilogues, K = %d" % K, **res)
    assert max(res.values()) <= 1


@pytest.mark.parametrize("K", o.LN_K)
def test_layernorm_emulation_inside_its_bounds(K):
    M, N = 129, o.LN_N
    res = {}
    for p in (0.0, 0.1):
        a, w, b, _ = o.make_operands(M, N, K, 11 * M + K)
        x, gamma, beta = o.make_ln(M, N, M + K)
        keep = keep_of(M, N, p, K)
        s, y, mean, rstd = o.emulate_ln(a, w, b, x, gamma, beta, keep, o.drop_scale(p))
        r = o.ln_ratios(s, y, mean, rstd, a, w, b, x, gamma, beta, keep, o.drop_scale(p), o.n_nt(K))
        for k, v in r.items():
            res[k] = max(res.get(k, 0), o.worst(v))
        # a dropped element that is not exactly x, and a whole wrong row
        s2 = s.clone()
        if p > 0:
            i, j = (~keep).nonzero()[0].tolist()
            s2[i, j] = o.bf16_step(s2[i, j].double().reshape(1), torch.tensor([True])).bfloat16()[0] if s2[i, j] != 0 else 1.0
            assert o.worst(o.ln_ratios(s2, y, mean, rstd, a, w, b, x, gamma, beta, keep, o.drop_scale(p), o.n_nt(K))["s"]) == float("inf")
        # the mean without the last column, the unbiased variance
        sf = s.float()
        bad = o.ln_ratios(s, y, sf[:, :-1].sum(1) / N, torch.rsqrt(sf.var(1, unbiased=True) + o.LN_EPS), a, w, b, x, gamma, beta,
                          keep, o.drop_scale(p), o.n_nt(K))
        res["mean of 511"] = min(res.get("mean of 511", float("inf")), o.worst(bad["mean"]))
        res["unbiased"] = min(res.get("unbiased", float("inf")), o.worst(bad["rstd"]))
    say("LayerNorm epilogue, K = %d" % K, **res)
    assert res.pop("mean of 511") > 1 and res.pop("unbiased") > 1 and max(res.values()) <= 1


@pytest.mark.parametrize("M", o.WG_M)
def test_wgrad_emulation_inside_the_bound_and_its_mutants_outside(M):
    res = {}
    for N1, N2 in o.WG_WIDTHS:
        a, b = o.make_wgrad(M, N1, N2, M + N1 + N2, strided=(N1 == 264))
        out0 = torch.randn(N1, N2, generator=torch.Generator().manual_seed(M))
        sl = o.wgrad_slices(M, N1, N2)[:2]
        for acc in (False, True):
            ref, S = o.wgrad_reference(a, b, out0 if acc else None)
            n = o.n_wgrad(M, N1, N2, acc)
            r = o.worst(o.f32_ratios(o.emulate_wgrad(a, b, sl, out0 if acc else None), ref, S, n))
            res["inside"] = max(res.get("inside", 0), r)
            for mut in ("drop_step", "slice_twice"):
                r = o.worst(o.f32_ratios(o.emulate_wgrad(a, b, sl, out0 if acc else None, mutate=mut), ref, S, n))
                res[mut] = min(res.get(mut, float("inf")), r)
    say("weight gradients, M = %d" % M, **res)
    assert res["inside"] <= 1 and res["drop_step"] > 1 and res["slice_twice"] > 1


# ----------------------------------------------------------------------------------------------------------------------
# every mutant is outside, at every K of the case lists
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ALL_K)
def test_plain_mutants_outside_the_bound(K):
    """With the LARGEST count any kernel has at this K (whole-K chain + both epilogue adds + the split-K merge)."""
    M, N = 257, 264
    a, w, b, c0 = o.make_operands(M, N, K, 7 * M + N + K)
    ref, S = o.plain_reference(a, w, b, c0)
    n = max(o.n_big(K, True, True), o.n_small(M, K, True, True), o.n_nt(K) + 2)
    res = {"inside": o.worst(o.plain_ratios(o.emulate_plain(a, w, b, c0), ref, S, n))}
    for mut in PLAIN_MUTANTS:
        res[mut] = o.worst(o.plain_ratios(o.emulate_plain(a, w, b, c0, mutate=mut), ref, S, n))
    say("plain forms, K = %d" % K, **res)
    assert res.pop("inside") <= 1 and min(res.values()) > 1, res


@pytest.mark.parametrize("K", sorted(set(o.NT_K + o.FFN_BIG_K + (2048,))))
def test_mul_mutants_outside_the_bound(K):
    M, N = 300, 768
    a, w, _, _ = o.make_operands(M, N, K, 3 * M + N + K)
    gd = o.make_gd(M, N, M + K, 0.1)
    n = max(o.n_nt(K), o.n_big(K))
    res = {}
    for mut in (None, "unrounded", "drop_k"):
        c, cs = o.emulate_mul(a, w, gd, mutate=mut)
        rc, rs = o.mul_ratios(c, cs, a, w, gd, n, o.n_colsum(M))
        res["%s c" % (mut or "inside")] = o.worst(rc)
        res["%s colsum" % (mut or "inside")] = o.worst(rs)
    # the column sums of the ROUNDED c (what a kernel summing after its store would give)
    c, cs = o.emulate_mul(a, w, gd)
    res["sums of rounded c"] = o.worst(o.mul_ratios(c, c.float().sum(0), a, w, gd, n, o.n_colsum(M))[1])
    say("multiply form, K = %d" % K, **res)
    assert res["inside c"] <= 1 and res["inside colsum"] <= 1
    assert res["unrounded c"] > 1 and res["drop_k c"] > 1 and res["drop_k colsum"] > 1 and res["sums of rounded c"] > 1


# ----------------------------------------------------------------------------------------------------------------------
# the both-neighbours rule
# ----------------------------------------------------------------------------------------------------------------------
def test_both_neighbours_rule_accepts_either_rounding_and_nothing_else():
    M, N, K = 300, 768, 512
    a, w, _, _ = o.make_operands(M, N, K, 21)
    gd = torch.ones(M, N).bfloat16()
    prod, S = o.product(a, w)
    delta = 4 * o.U32 * o.n_nt(K) ** 0.5 * S
    r0, r1, amb, slack = o.bf16_neighbours(prod, delta)
    plain = (~amb) & (slack == 0)
    assert amb.sum() > 50 and plain.float().mean() > 0.95 and (r1[~amb] == r0[~amb]).all()
    assert ((r0 - prod).abs() <= (r1 - prod).abs() + o.U32 * prod.abs())[amb].all() and (r1[amb] != r0[amb]).all()
    # r0 and r1 are neighbours with prod between them
    lo, hi = torch.minimum(r0, r1)[amb], torch.maximum(r0, r1)[amb]
    assert ((lo <= prod[amb]) & (prod[amb] <= hi)).all() and (hi.float().bfloat16().double() == hi).all()
    assert (o.bf16_step(lo, lo > 0) == hi).all()
    ratio = lambda c: o.mul_ratios(c.bfloat16(), None, a, w, gd, o.n_nt(K), 1)[0]
    assert o.worst(ratio(r0)) <= 1                                       # the nearest value everywhere
    assert o.worst(ratio(torch.where(amb, r1, r0))) <= 1               # the other neighbour where the boundary is within delta
    # ... and nowhere else.  The hard term 2^-8 max(|ref|, |got|) is a half-ulp at the bottom of a binade and a whole ulp at its
    # top, so a whole-ulp miss is outside for every element in the lower half of its binade (and never below 0.99)
    away = o.bf16_step(r0, prod.abs() > r0.abs())
    sel = plain & (prod != r0)
    miss = ratio(torch.where(sel, away, r0))
    mant = torch.frexp(r0.abs())[0]
    low = sel & (mant > 0.5) & (mant < 0.7)                             # (a power of two has a half-sized step below it)
    assert low.sum() > 1000 and (miss[low] > 1).all() and (miss[sel] > 0.99).all()
    far = o.bf16_step(r0, ~(prod.abs() > r0.abs()))                     # the neighbour on the other side of r0: never
    nz = amb & (mant > 0.5) & (mant < 0.7)
    assert nz.sum() > 10 and (ratio(torch.where(nz, far, r0))[nz] > 1).all()
    # products that cancel: the kernel's rounded value may lie anywhere within slack of r0
    a, w, _, _ = o.make_cancelling(65, 72, 256, 7)
    prod, S = o.product(a, w)
    delta = 4 * o.U32 * o.n_nt(256) ** 0.5 * S
    r0, r1, amb, slack = o.bf16_neighbours(prod, delta)
    wide = slack > 0
    assert wide.any() and (slack[wide] >= delta[wide]).all()
    g1 = torch.ones(65, 72).bfloat16()
    got = (prod + delta * 0.99).float().bfloat16()
    assert o.worst(o.mul_ratios(got, None, a, w, g1, o.n_nt(256), 1)[0]) <= 1
    got = (prod + 40 * delta + 2.0 ** -6 * prod.abs()).float().bfloat16()
    assert o.worst(o.mul_ratios(got, None, a, w, g1, o.n_nt(256), 1)[0]) > 1

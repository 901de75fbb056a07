"""GPU: every form of the causal linear attention scan (csrc/cla.hip, csrc/cla_bf16.hip), row by row against the f64 reference
of oracle/cla_f64.py (pinned, with every bound below, by tests/test_oracle_cla_f64_cpu.py).

Reference.  oracle.cla_f64.reference in f64 on the GPU (plain torch, none of the project's kernels), started from the very
values the kernels are given (bf16 values for the bf16 forms).  out, zinv, dq, dk, dv, dden and the final state; the final
state sums the bf16-rounded phi(k), which is what the MFMA forward adds.

Measure.  Per row of 64 (query rows for out and dq, key rows for dk and dv): |got - ref| / max(|ref row|, T_row), T_row the
norm the row would have if its tokens' terms added without cancelling (oracle.cla_f64.row_terms).  No tensor-wide floor and
no floor for any row class: the denominator is positive on every row of every input (asserted on the CPU) except rows that
are exactly zero by construction, which must be exactly zero.  zinv per element relative to |ref|; dden per element relative
to D_i = max(|ref|, z_i |dout_i| max(|out_i|, T(out_i))); the final state per element relative to the root-sum-square of
its L terms; column sums against the f64 sums of the stored values, relative to the column's sum of |terms|.

Bounds.  u = 2^-24 per f32 operation, U = 2^-9 / sqrt(3) per bf16 rounding, errors independent, a sum of n terms counts
n / 6, the bound 4 x the predicted rms; the counts per form and tensor are read off the source in oracle/cla_f64.py's
docstring and evaluated by oracle.cla_f64.bounds / zinv_bound / dden_bound / state_bound / colsum_bound:
    bound_row = 4 sqrt((n_T + n_E (E_row / den_row)^2) U^2 + (n32_T + n32_E (E_row / den_row)^2) u^2 [+ per-row terms])
    n_T       out  dv  dk  dq    n_E (dq, dk)
    mfma        5   6   7   5    6          whole-sequence pair and segmented pair (same roundings, other f32 order)
    sweep       5   6   6   7    6          dq also takes 4 sqrt(chunks passed) u |final state| / |prefix state| (its state by
                                            subtraction), by the row's chunk, from the reference's states
    generic     1   1   1   1    1
    mixed       5   2   2   2    5          the generic backward behind the MFMA forward (dout view of row stride 132)
    f32         n32_fwd = 12 + 64/3 + L/3, n32_bwd = 2 n32_fwd + 2, n32_E = n32_fwd + 64/6 + 2
E_row (oracle.cla_f64.operand_terms) is the norm of a dq or dk row if the contraction over the 64 value columns did not
cancel either: g = r(dout z) and the stored out inside dden are rounded before that contraction.  The f32 and generic
forms evaluate phi as (exp(x) - 1) + 1, as the reference does: an absolute error u, carried per row as 4 sqrt(2) kappa_i
(oracle.cla_f64.phi_abs_term); where eps decides a row (input 4, rows 0 .. 4) kappa is about 1 and the assertion of those
forms there is finiteness: input 4 is given to them at L >= 257 only, so that the share of such rows stays below 2 %
(asserted).  Measured there at (2, 257, 3): the worst of dk rows 0 .. 4 at 5.8 x its denominator in f32 and 5.5 x in the
generic form (1.17 and 1.11 of a bound that is itself 5: the linear error model ends where kappa reaches 1); every other
row of those cases inside its bound.  The MFMA forms evaluate exp(x) and are held to their bound on those rows too.

Forms are asserted, not assumed: ops._call is wrapped and every case checks the entry points that ran, their dtype code,
row strides, segment count, final-state and dden arguments against the path it names.

Inputs (oracle.cla_f64.make_inputs): 1 randn; 2 randn x 3 for q and k; 3 the same with v of mean 1; 4 k = -20 on the
first 5 tokens.  5 and 6 (dout zero on a span; dout nonzero below t only) have exact-zero assertions of their own.

Teeth (TEETH = 5): the reference rebuilt with one wrong ingredient (oracle.cla_f64.MUTANTS) must miss the kernels' result,
in the rms over the rows the ingredient feeds, by 5 x the bound, while the kernel is inside the bound against the right
reference.  The dropped diagonal is asked on out, dk and dv: on dq, one token's term of a row of 130 to 200 is only
1.8 x the bound.

Measured on an MI355X: profiles/cla_f64_ratios.txt.
"""
import ctypes

import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import _lib, ops
from oracle import cla_f64 as o

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAMES = ("out", "dq", "dk", "dv")
REAL_CALL = ops._call
_CACHE = {}


def note(label, value, bound=1.0):
    """Prints a figure against its bound -> their ratio."""
    print("    %-72s %.3e  bound %.3e  (%.2f)" % (label, value, bound, value / bound))
    return value / bound


# ----------------------------------------------------------------------------------------------------------------------
# recording the entry points
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    log = []

    def spy(name, *args, **kw):
        a = args
        if name == "cwlt_causal_linear_fwd":
            log.append({"name": "fwd", "ld": tuple(a[9:12]), "P": a[14], "fin": a[16] is not None, "code": a[17]})
        elif name == "cwlt_causal_linear_bwd_dkdv":
            log.append({"name": "dkdv", "ld": tuple(a[15:18]) + (a[19],), "P": a[22], "dden": a[10] is not None,
                        "cs": a[8] is not None, "code": a[24]})
        elif name == "cwlt_causal_linear_bwd_dq":
            log.append({"name": "dq", "ld": tuple(a[13:16]) + (a[17],), "P": a[19], "dden": a[8] is not None,
                        "cs": a[7] is not None, "code": a[21]})
        elif name == "cwlt_causal_linear_bwd_sweep":
            log.append({"name": "sweep", "ld": tuple(a[17:20]) + (a[21],), "cs": a[10] is not None, "code": a[25]})
        return REAL_CALL(name, *args, **kw)

    monkeypatch.setattr(ops, "_call", spy)
    return log


def assert_route(log, route, P=1, colsum=False, fin=None):
    """The entry points that ran are those of `route`, on the kernels it names."""
    names = [c["name"] for c in log]
    code = _lib.dtype_code(F32 if route == "f32" else BF16)
    assert all(c["code"] == code for c in log), log
    mult8 = lambda c: all(x % 8 == 0 for x in c["ld"])
    fwd = log[0]
    assert fwd["name"] == "fwd"
    if route == "f32":
        assert names == ["fwd", "dkdv", "dq"] and not any(c.get("dden") or c.get("cs") for c in log[1:])
        assert fwd["P"] == 1 and not fwd["fin"]
    elif route == "generic":
        assert names == ["fwd", "dkdv", "dq"] and not any(mult8(c) for c in log), log
        assert not any(c.get("dden") or c.get("cs") for c in log[1:]) and fwd["P"] == 1 and not fwd["fin"]
    elif route == "mixed":
        assert names == ["fwd", "dkdv", "dq"] and mult8(fwd) and not mult8(log[1]) and not mult8(log[2]), log
        assert not any(c.get("dden") for c in log[1:]) and all(c["P"] == 1 for c in log)
    elif route in ("mfma", "seg"):
        assert names == ["fwd", "dkdv", "dq"] and all(mult8(c) for c in log), log
        assert all(c["P"] == P for c in log) and (P > 1) == (route == "seg"), (log, P)
        assert log[1]["dden"] and log[2]["dden"], "the dden hand-over between dkdv and dq"
        assert log[1]["cs"] == colsum and log[2]["cs"] == colsum
        assert fwd["fin"] == bool(fin)
    elif route == "sweep":
        assert names == ["fwd", "sweep"] and all(mult8(c) for c in log), log
        assert fwd["P"] == 1 and fwd["fin"] and log[1]["cs"] == colsum
    else:
        raise AssertionError(route)


# ----------------------------------------------------------------------------------------------------------------------
# running a route through the package
# ----------------------------------------------------------------------------------------------------------------------
def expected_segments(L, segs):
    nch = (L + 63) // 64
    cps = -(-nch // max(1, min(segs, nch)))
    return -(-nch // cps)


def strided(x, pad, fill=float("nan")):
    """q, k, v (N, L, H, 64) as column blocks of one buffer of row width 3 H 64 + pad whose gap columns hold `fill`."""
    q, k, v = x
    N, L, H, _ = q.shape
    buf = torch.full((N, L, 3 * H * 64 + pad), fill, dtype=q.dtype, device=q.device)
    views = []
    W = 3 * H * 64 + pad
    for i, t in enumerate((q, k, v)):
        view = buf.as_strided((N, L, H, 64), (L * W, W, 64, 1), i * H * 64)
        view.copy_(t)
        views.append(view)
    assert all(w.stride(1) == 3 * H * 64 + pad and w.data_ptr() % 16 == 0 for w in views)
    return views


def run(route, x, monkeypatch, log, segs=1, colsum=False, with_fin=None):
    """x = (q, k, v, dout) on the GPU.  -> dict out, zinv, dq, dk, dv [, dbias, fin] as the package returns them."""
    q, k, v, g = x
    N, L, H, _ = q.shape
    del log[:]
    monkeypatch.setenv("CWLT_SCAN_SEGMENTS", str(segs if route == "seg" else 1))
    P = 1
    if route == "generic":
        q, k, v = strided((q, k, v), 4)
    if route == "mixed":
        big = torch.full((N, L, H * 64 + 4), float("nan"), dtype=g.dtype, device=g.device)
        gv = big.as_strided((N, L, H, 64), (L * (H * 64 + 4), H * 64 + 4, 64, 1))
        gv.copy_(g)
        g = gv
        assert g.stride(1) == H * 64 + 4
    if route == "seg":
        P = expected_segments(L, segs)
        assert P > 1 and ops.scan_segments(N, H, L, BF16) == P
    res = {}
    if route == "sweep":
        q, k, v, out, zinv, fin = ops.cla_fwd(q, k, v, final_state=True)
        assert fin is not None
        back = ops.cla_bwd(q, k, v, out, zinv, g, want_colsum=colsum, final_state=fin)
        res["fin"] = fin
    else:
        if with_fin is None:
            q, k, v, out, zinv = ops.cla_fwd(q, k, v)
        else:
            q, k, v, out, zinv, fin = ops.cla_fwd(q, k, v, final_state=with_fin)
            assert (fin is not None) == bool(with_fin)
            res["fin"] = fin
        back = ops.cla_bwd(q, k, v, out, zinv, g, want_colsum=colsum and route in ("mfma", "seg"))
    torch.cuda.synchronize()
    assert_route(log, route, P, colsum, with_fin)
    dqkv = back[0] if isinstance(back, tuple) else back
    if isinstance(back, tuple):
        res["dbias"] = back[1]
    res.update(out=out, zinv=zinv, dq=dqkv[:, :, 0], dk=dqkv[:, :, 1], dv=dqkv[:, :, 2])
    return res


def case(kind, shape, dtype, cuda, seed=1):
    """Inputs on the GPU, their f64 reference and its row terms: computed once, shared, never modified."""
    key = (kind, shape, dtype, seed)
    if key not in _CACHE:
        x = tuple(t.to(cuda) for t in o.make_inputs(kind, *shape, seed, dtype))
        ref = o.reference(*x, kf_round=o.rb)
        _CACHE[key] = (x, ref, o.analyse(ref))
    return _CACHE[key]


def check(label, form, res, ref, t, L, rows=None):
    """Every row of out, dq, dk, dv and every zinv inside the bound of `form`; prints each worst figure as a ratio.
    Rows whose bound is above 1 (the error may exceed the row: no digit is promised) are held to finiteness only; they
    are the first token's dq and dk (c_00 = z dout . (v - out) = O(eps): the one term cancels within itself, E / den is
    1e8) and, for the f32 and generic forms, the rows eps decides; beyond token 0 their share is at most 2 %."""
    b = o.bounds(form, ref, t, L)
    worst = {}
    vacuous = 0.0
    for n in NAMES:
        assert torch.isfinite(res[n].float()).all(), (label, n)
        r = o.row_ratio(res[n], ref[n], t["den_" + n]) / b[n]
        loose = b[n] > 1
        worst[n] = torch.where(loose, torch.zeros_like(r), r).max().item()
        if n in ("dq", "dk"):
            loose = loose[:, 1:]
        vacuous = max(vacuous, loose.double().mean().item() if loose.numel() else 0.0)
    z = ((res["zinv"].double() - ref["zinv"]).abs() / ref["zinv"])
    assert torch.isfinite(res["zinv"]).all()
    kap = 4 * 2 ** 0.5 * o.phi_abs_term(ref) if form in ("f32", "generic") else 0.0
    worst["zinv"] = (z / (o.zinv_bound(form, L) ** 2 + kap ** 2) ** 0.5).max().item()
    print("    %-40s %s" % (label, "  ".join("%s %.2f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, (label, worst)
    assert vacuous <= 0.02, (label, "rows whose bound is above 1", vacuous)
    return worst


def check_colsum(label, res, L, preround):
    """dbias (3 H 64) against the f64 sums of the stored gradients over (N, L)."""
    N = res["dq"].shape[0]
    worst = 0.0
    for i, n in enumerate(("dq", "dk", "dv")):
        x = res[n].double()
        want, sabs, rss = x.sum((0, 1)).reshape(-1), x.abs().sum((0, 1)).reshape(-1), (x ** 2).sum((0, 1)).sqrt().reshape(-1)
        allow = o.colsum_bound(N * L) * sabs + (4 * 2 * o.U16 * rss if preround and n != "dv" else 0)
        got = res["dbias"].double().reshape(3, -1)[i]
        worst = max(worst, ((got - want).abs() / allow.clamp_min(1e-300)).max().item())
    print("    %-40s column sums %.2f" % (label, worst))
    assert worst <= 1.0, (label, worst)


def check_state(label, fin, ref, N, L, H):
    """The forward's final state, per element relative to the root-sum-square of its L terms."""
    fin = fin.view(N, H, 65, 64).double()
    S, zs = fin[:, :, :64], fin[:, :, 64]
    rS = ((S - ref["fin_S"]).abs() / ref["fin_S_rss"]) / (o.state_bound(L) * ref["fin_S_abs"] / ref["fin_S_rss"])
    rz = ((zs - ref["fin_z"]).abs() / ref["fin_z_rss"]) / (o.state_bound(L) * ref["fin_z"] / ref["fin_z_rss"])
    print("    %-40s final state S %.2f  ksum %.2f" % (label, rS.max().item(), rz.max().item()))
    assert rS.max().item() <= 1.0 and rz.max().item() <= 1.0, label


# ----------------------------------------------------------------------------------------------------------------------
# every form at the edge shapes
# ----------------------------------------------------------------------------------------------------------------------
# L: 1, 2, one short of / exactly / one past one and two chunks of 64, a ragged middle, 5 and 9 chunks, a ragged 16 and 16
# full chunks.  N: 1, 3, 8, 16 (N % 8 == 0 switches stream_of_block).  H: 1, 2, 3, 8.  At most 8 k rows per case.
SHAPES = [((1, 1, 1), "randn"), ((3, 2, 2), "x3"), ((1, 63, 3), "vmean"), ((16, 64, 2), "randn"), ((3, 65, 1), "x3"),
          ((1, 127, 8), "vmean"), ((2, 128, 1), "randn"), ((3, 129, 2), "x3"), ((8, 130, 3), "randn"),
          ((1, 200, 2), "vmean"), ((2, 257, 3), "eps"), ((1, 576, 2), "x3"), ((2, 1000, 1), "eps"),
          ((1, 1024, 8), "randn"), ((1, 1024, 2), "x3"), ((1, 1024, 2), "vmean"), ((1, 1024, 2), "eps"),
          ((3, 65, 1), "eps")]


@pytest.mark.parametrize("shape,kind", SHAPES)
@pytest.mark.parametrize("route", ["f32", "generic", "mfma", "sweep"])
def test_rows_against_f64(cuda, monkeypatch, calls, route, shape, kind):
    N, L, H = shape
    if route in ("f32", "generic") and kind == "eps" and L < 257:
        kind = "randn"          # input 4 at L >= 257 only for the forms that keep no digit where eps decides (docstring)
    x, ref, t = case(kind, shape, F32 if route == "f32" else BF16, cuda)
    colsum = route in ("mfma", "sweep") and (N + L) % 2 == 1
    with_fin = None if route != "mfma" else (False if L % 2 else None)
    res = run(route, x, monkeypatch, calls, colsum=colsum, with_fin=with_fin)
    label = "%s %s %s" % (route, shape, kind)
    check(label, route, res, ref, t, L)
    if colsum:
        check_colsum(label, res, L, preround=route == "mfma")
    if route == "sweep":
        check_state(label, res["fin"], ref, N, L, H)


SEG_CASES = [((1, 129, 2), 2, "randn"), ((3, 200, 2), 3, "vmean"), ((1, 257, 1), 2, "x3"), ((1, 257, 1), 8, "eps"),
             ((2, 576, 1), 3, "randn"), ((2, 576, 1), 4, "x3"), ((1, 1000, 2), 16, "vmean"), ((1, 1024, 2), 2, "randn"),
             ((1, 1024, 2), 3, "x3"), ((1, 1024, 2), 8, "eps"), ((1, 1024, 1), 16, "randn"), ((8, 130, 3), 2, "randn")]


@pytest.mark.parametrize("shape,segs,kind", SEG_CASES)
def test_segmented_rows_against_f64(cuda, monkeypatch, calls, shape, segs, kind):
    """The few-stream schedule: 9 chunks take 3 segments and refuse 4; a ragged last chunk ends the last segment; an
    uneven split (16 chunks in 3 runs: 6, 6, 4); one chunk per segment; N % 8 == 0."""
    N, L, H = shape
    x, ref, t = case(kind, shape, BF16, cuda)
    P = expected_segments(L, segs)
    assert {(576, 3): 3, (576, 4): 3, (1024, 3): 3, (1024, 16): 16, (1000, 16): 16}.get((L, segs), P) == P
    res = run("seg", x, monkeypatch, calls, segs=segs, colsum=True)
    label = "seg P=%d %s %s" % (P, shape, kind)
    check(label, "mfma", res, ref, t, L)
    check_colsum(label, res, L, preround=True)


def test_fused_qkv_views_and_the_autograd_function(cuda, monkeypatch, calls):
    """q, k, v as views of one (N, L, 3, H, 64) projection through causal_linear_attention: the forward hands over its
    final state and the backward is the sweep."""
    monkeypatch.setenv("CWLT_SCAN_SEGMENTS", "1")
    N, L, H = 2, 257, 3
    x, ref, t = case("x3", (N, L, H), BF16, cuda)
    qkv = torch.stack(x[:3], 2).requires_grad_(True)
    del calls[:]
    out = ops.causal_linear_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    out.backward(x[3])
    torch.cuda.synchronize()
    assert_route(calls, "sweep")
    assert calls[0]["ld"] == (3 * H * 64,) * 3
    res = {"out": out.detach(), "dq": qkv.grad[:, :, 0], "dk": qkv.grad[:, :, 1], "dv": qkv.grad[:, :, 2]}
    b = o.bounds("sweep", ref, t, L)
    for n in NAMES:
        assert (b[n] <= 1).all()
        assert note("autograd %s" % n, (o.row_ratio(res[n], ref[n], t["den_" + n]) / b[n]).max().item()) <= 1.0


def test_dout_view_with_row_stride_132(cuda, monkeypatch, calls):
    """H = 2, dout a view of row stride 132: the MFMA forward, then the generic dkdv + dq pair (form "mixed")."""
    shape = (2, 200, 2)
    x, ref, t = case("randn", shape, BF16, cuda)
    res = run("mixed", x, monkeypatch, calls)
    check("mixed %s" % (shape,), "mixed", res, ref, t, shape[1])


# ----------------------------------------------------------------------------------------------------------------------
# exact zeros
# ----------------------------------------------------------------------------------------------------------------------
BACKWARD_ROUTES = [("f32", 1), ("generic", 1), ("mfma", 1), ("seg", 2), ("seg", 3), ("sweep", 1)]


@pytest.mark.parametrize("route,segs", BACKWARD_ROUTES)
def test_dq_is_exactly_zero_where_dout_is(cuda, monkeypatch, calls, route, segs):
    """Input 5: dout zero on rows 60 .. 139 (across two chunk boundaries): dden_i = 0 and every product has a zero factor."""
    shape = (3, 200, 2)
    x, _, _ = case("randn", shape, F32 if route == "f32" else BF16, cuda)
    g = x[3].clone()
    g[:, 60:140] = 0
    res = run(route, x[:3] + (g,), monkeypatch, calls, segs=segs)
    assert (res["dq"][:, 60:140] == 0).all() and (res["dq"][:, :60] != 0).any() and (res["dq"][:, 140:] != 0).any()
    ref = o.reference(*x[:3], g)
    t = o.analyse(ref)
    check("%s dout zero on a span" % route, "mfma" if route == "seg" else route, res, ref, t, shape[1])


@pytest.mark.parametrize("route,segs", BACKWARD_ROUTES)
@pytest.mark.parametrize("L,t0", [(200, 1), (200, 100), (200, 128), (200, 199), (257, 192), (257, 256)])
def test_dk_dv_are_exactly_zero_from_the_last_live_query_on(cuda, monkeypatch, calls, route, segs, L, t0):
    """Input 6: dout nonzero on rows below t only, t = 1, inside a chunk, at a chunk boundary (128: also the segment
    boundary at L = 200; at L = 257, 192 is the boundary of 2 segments and 256 one of 3), L - 1: no query at or after t
    has a gradient, so no key there gets one.  dq is zero there as well (input 5)."""
    shape = (1, L, 2)
    x, _, _ = case("x3", shape, F32 if route == "f32" else BF16, cuda)
    g = x[3].clone()
    g[:, t0:] = 0
    res = run(route, x[:3] + (g,), monkeypatch, calls, segs=segs)
    for n in ("dk", "dv", "dq"):
        assert (res[n][:, t0:] == 0).all(), (n, route, t0)
        # (a lone first token's dq and dk are c_00 = z dout . (v - out) = O(eps): they may round to zero)
        assert (res[n][:, :t0] != 0).any() or (t0 == 1 and n != "dv"), (n, route, t0)


# ----------------------------------------------------------------------------------------------------------------------
# batch independence and determinism
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,segs", BACKWARD_ROUTES)
def test_sequences_do_not_see_each_other_and_runs_repeat(cuda, monkeypatch, calls, route, segs):
    """N = 3, L = 65 (129 segmented), sequences of magnitude 1, 10 and 0.1: each equals, bit for bit, the same sequence
    run alone, and a second run of the batch equals the first."""
    L = 129 if route == "seg" else 65
    dtype = F32 if route == "f32" else BF16
    x, _, _ = case("randn", (3, L, 2), dtype, cuda, seed=5)
    scale = torch.tensor([1.0, 10.0, 0.1], device=cuda).view(3, 1, 1, 1)
    x = tuple((t.float() * scale).to(dtype) for t in x)
    a = run(route, x, monkeypatch, calls, segs=segs, colsum=route in ("mfma", "seg", "sweep"))
    b = run(route, x, monkeypatch, calls, segs=segs, colsum=route in ("mfma", "seg", "sweep"))
    for n in a:
        assert torch.equal(a[n], b[n]), (route, n)
    for s in range(3):
        one = run(route, tuple(t[s:s + 1].contiguous() for t in x), monkeypatch, calls, segs=segs)
        for n in NAMES + ("zinv",):
            assert torch.equal(one[n][0], a[n][s]), (route, n, s)


def test_segmented_and_whole_sequence_agree_under_the_bound(cuda, monkeypatch, calls):
    """The one pair of forms that is not bit-identical: both inside the bound against the same reference, on every sequence
    of the magnitude-1 / 10 / 0.1 batch."""
    x, _, _ = case("randn", (3, 129, 2), BF16, cuda, seed=5)
    scale = torch.tensor([1.0, 10.0, 0.1], device=cuda).view(3, 1, 1, 1)
    x = tuple((t.float() * scale).bfloat16() for t in x)
    ref = o.reference(*x, kf_round=o.rb)
    t = o.analyse(ref)
    for route, segs in (("mfma", 1), ("seg", 2), ("seg", 3)):
        check("%s P=%d magnitudes" % (route, segs), "mfma", run(route, x, monkeypatch, calls, segs=segs), ref, t, 129)


# ----------------------------------------------------------------------------------------------------------------------
# tails and neighbours: the C entry points on buffers of our own
# ----------------------------------------------------------------------------------------------------------------------
def direct(route, x, P=1):
    """Runs `route` ("generic" | "mfma" | "seg" | "sweep") through the C entry points on strided inputs whose gap columns
    hold NaN and on outputs allocated inside larger buffers pre-filled with a sentinel.  -> results, and the list of
    (buffer, pristine copy, mask of what the kernels may write)."""
    q, k, v, g = x
    N, L, H, _ = q.shape
    dev, dt = q.device, q.dtype
    pad = 4 if route == "generic" else 8
    lib = _lib.load()
    q, k, v = strided((q, k, v), pad)
    gbuf = torch.full((N, L, H * 64 + pad), float("nan"), dtype=dt, device=dev)
    gv = gbuf.as_strided((N, L, H, 64), (L * (H * 64 + pad), H * 64 + pad, 64, 1))
    gv.copy_(g)
    ldi, ldg, W = 3 * H * 64 + pad, H * 64 + pad, 3 * H * 64 + pad
    SENT = 7776.0
    rows = N * L
    obuf = torch.full((rows + 3, H * 64), SENT, dtype=dt, device=dev)            # 3 rows past the last sequence
    zbuf = torch.full((rows * H + 1,), SENT, dtype=F32, device=dev)              # the float after zinv
    dbuf = torch.full((rows + 3, W), SENT, dtype=dt, device=dev)                 # strided dqkv with gap columns
    ddbuf = torch.full((rows * H + 1,), SENT, dtype=F32, device=dev)
    fbuf = torch.full((N * H * 65 * 64 + 1,), SENT, dtype=F32, device=dev)
    cbuf = torch.full((3 * N * P * H * 64 + 1,), SENT, dtype=F32, device=dev)
    cs = cbuf[:-1].view(3, N * P, H * 64)
    code, st = _lib.dtype_code(dt), _lib.stream_ptr()
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    col = lambda i: ctypes.c_void_p(dbuf.data_ptr() + i * H * 64 * dbuf.element_size())
    ws = lambda back: (torch.empty(int(lib.cwlt_scan_seg_floats(N, H, P, back)), dtype=F32, device=dev) if P > 1 else None)
    w0 = ws(0)
    fin = route == "sweep"
    REAL_CALL("cwlt_causal_linear_fwd", p(q), p(k), p(v), p(obuf), p(zbuf), N, H, L, 64, ldi, ldi, ldi, H * 64, o.EPS, P,
              _lib.opt(w0), p(fbuf) if fin else None, code, st)
    common = (p(q), p(k), p(v), p(obuf), p(zbuf), p(gv))
    fused = route != "generic"
    if route == "sweep":
        REAL_CALL("cwlt_causal_linear_bwd_sweep", *common, p(fbuf), col(0), col(1), col(2), p(cs[0]), p(cs[1]), p(cs[2]),
                  N, H, L, 64, ldi, ldi, ldi, H * 64, ldg, W, W, W, code, st)
    else:
        w1 = ws(1)
        REAL_CALL("cwlt_causal_linear_bwd_dkdv", *common, col(1), col(2), p(cs[1]) if fused else None,
                  p(cs[2]) if fused else None, p(ddbuf) if fused else None, N, H, L, 64, ldi, ldi, ldi, H * 64, ldg, W, W,
                  P, _lib.opt(w1), code, st)
        REAL_CALL("cwlt_causal_linear_bwd_dq", *common, col(0), p(cs[0]) if fused else None, p(ddbuf) if fused else None,
                  N, H, L, 64, ldi, ldi, ldi, H * 64, ldg, W, P, _lib.opt(w1), code, st)
    torch.cuda.synchronize()
    d = dbuf[:rows, :3 * H * 64].view(N, L, 3, H, 64)
    res = {"out": obuf[:rows].view(N, L, H, 64), "zinv": zbuf[:-1].view(N, L, H), "dq": d[:, :, 0], "dk": d[:, :, 1],
           "dv": d[:, :, 2], "dden": ddbuf[:-1].view(N, L, H), "fin": fbuf[:-1], "cs": cs}
    untouched = [("rows past L of out", obuf[rows:]), ("the float after zinv", zbuf[-1:]),
                 ("gap columns of dqkv", dbuf[:, 3 * H * 64:]), ("rows past L of dqkv", dbuf[rows:]),
                 ("the float after the column sums", cbuf[-1:])]
    if fused and route != "sweep":
        untouched.append(("the float after dden", ddbuf[-1:]))
    else:
        untouched.append(("dden (not written by this route)", ddbuf))
    if fin:
        untouched.append(("the float after the final state", fbuf[-1:]))
    else:
        untouched.append(("final state (not written by this route)", fbuf))
    if not fused:
        untouched.append(("column sums (not written by this route)", cbuf))
    for what, piece in untouched:
        assert (piece == SENT).all(), (route, what)
    return res


@pytest.mark.parametrize("route,P,shape", [("generic", 1, (2, 65, 2)), ("mfma", 1, (3, 65, 2)), ("mfma", 1, (8, 130, 1)),
                                           ("seg", 2, (2, 129, 2)), ("seg", 3, (1, 257, 1)), ("sweep", 1, (3, 65, 2)),
                                           ("sweep", 1, (8, 130, 1))])
def test_neighbours_untouched_nan_gaps_dden_and_column_sums(cuda, monkeypatch, calls, route, P, shape):
    """Outputs inside sentinel-filled buffers (gap columns of a strided dqkv, rows past L of the last sequence, the float
    after zinv / dden / the final state / the column sums: untouched); NaN in the gap columns of the strided inputs
    (results bit-identical to the package's run on dense copies); the dden the dkdv kernel hands to dq, and the column
    sums per (sequence, head), against f64."""
    N, L, H = shape
    x, ref, t = case("x3", shape, BF16, cuda, seed=3)
    res = direct(route, x, P)
    dense = run(route, x, monkeypatch, calls, segs=P, colsum=route != "generic")
    for n in NAMES + ("zinv",):
        assert torch.equal(res[n], dense[n]), (route, n)
    form = {"seg": "mfma"}.get(route, route)
    label = "direct %s P=%d %s" % (route, P, shape)
    check(label, form, res, ref, t, L)
    if route in ("mfma", "seg"):
        r = ((res["dden"].double() - ref["dden"]).abs() / t["dden"]).max().item()
        assert note(label + " dden", r, o.dden_bound(form, L)) <= 1.0
    if route != "generic":
        cs = res["cs"].view(3, N, P, H, 64).double().sum(2)                    # per (sequence, head)
        worst = 0.0
        for i, n in enumerate(("dq", "dk", "dv")):
            g = res[n].double()
            allow = o.colsum_bound(L) * g.abs().sum(1) + (4 * 2 * o.U16 * (g ** 2).sum(1).sqrt()
                                                          if route != "sweep" and n != "dv" else 0)
            worst = max(worst, ((cs[i] - g.sum(1)).abs() / allow.clamp_min(1e-300)).max().item())
        assert note(label + " column sums per (sequence, head)", worst) <= 1.0
        want = cs.sum(1).reshape(-1)
        assert (dense["dbias"].double() - want).abs().max().item() <= 4 * (N * P) ** 0.5 * o.U32 * want.abs().max().item()
    if route == "sweep":
        check_state(label, res["fin"], ref, N, L, H)


# ----------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant,kind,shape,segs,tensors,rows", o.MUTANTS)
def test_teeth(cuda, monkeypatch, calls, mutant, kind, shape, segs, tensors, rows):
    x, ref, t = case(kind, shape, BF16, cuda)
    L = shape[1]
    mut = o.mutant_reference(*x, mutant, segments=segs)
    routes = [("seg", segs)] if mutant == "seg" else [("mfma", 1), ("sweep", 1)] + ([("seg", 3)] if L >= 576 else [])
    for route, P in routes:
        res = run(route, x, monkeypatch, calls, segs=P)
        form = "sweep" if route == "sweep" else "mfma"
        b = o.bounds(form, ref, t, L)
        for n in tensors:
            inside = (o.row_ratio(res[n], ref[n], t["den_" + n]) / b[n]).max().item()
            miss = o.teeth(res[n], mut[n], t["den_" + n], b[n], rows)
            print("    teeth %-6s %-6s %-4s inside %.2f, the mutant %.1f x the bound" % (mutant, route, n, inside, miss))
            assert inside <= 1.0 and miss >= o.TEETH, (mutant, route, n, inside, miss)
        if mutant == "eps0":
            z = ((res["zinv"].double() - mut["zinv"]).abs() / mut["zinv"])[:, rows].max().item()
            assert z >= o.TEETH * o.zinv_bound(form, L)

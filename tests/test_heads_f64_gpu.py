"""GPU: both kernel families of the per-attribute heads (csrc/heads.hip), row by row against the f64 reference of
oracle/heads_rl_f64.py (pinned, with every bound below, by tests/test_oracle_heads_rl_f64_cpu.py).

Reference.  oracle.heads_rl_f64.heads_reference in f64 on the GPU (plain torch, none of the project's kernels), started from
the very values the kernels are given (the bf16 values of bf16 logits): per (row, attribute) nll, softmax, argmax, pmax; the
masked loss sums; dlogits of cwlt_heads_ce_bwd and of cwlt_heads_logp_bwd with padding columns zero.  Padding columns of the
logits hold NaN: a kernel that reads one into a softmax shows it.

Measure and bounds (u = 2^-24, U = 2^-9 / sqrt(3), 4 x the predicted rms; counts in the oracle's docstring).  Loss sums
relative to sum_r mask_r (|mx| + |x_t| + |log sum|) with the f32 term of the family's partial-sum tree; probs and pmax per
(row, attribute) relative to the row's pmax; dlogits per (row, attribute) relative to |mask coef| or |g|, one bf16 rounding
on top for bf16 dlogits, rows of weight 0 and padding columns exactly 0.  argmax exact except pairs whose two largest softmax
values differ by a relative gap in (0, 1e-5) (skipped, share asserted <= 0.1 %); exact ties must give the lowest index.

Families are asserted, not assumed: ops._call is wrapped, every case checks the entry point that ran, its dtype code and ld,
and that cwlt_heads_tiled (the launchers' own decision) names the family the case claims, for the very pointers passed.

Tiled: repo vocabularies (ld 384), PPO vocabularies (320), (9, 8, 7, 1, 65, 64, 63) (n_attr = 7: the backward's one idle slot
clears the padding; the 8-unroll edges; n = 1) and (256,).  Wave-per-row, one per trigger: n_attr = 8; ld >= 480; ld % vec != 0
(unpadded repo logits, 339 f32 / 340 bf16); a misaligned base (a column view, forward only: heads_ce copies it); the 64-lane
slot edges (1, 63, 64, 65, 128, 129, 255).  Rows 1, 31, 32, 33, 1 031 per family; 32 801 rows tiled (a second tile in the first
blocks, a 1-row last tile) and 4 101 rows wave-per-row (a second row in the first waves).  Masks: ones, random 80 %, a single 1
on the last row, ones only in the last partial tile.  Inputs: randn x 3, peaked (+50), shifted (+300), exact ties, targets
holding -5 and n + 3.

Teeth (TEETH = 5): the reference with one wrong ingredient must miss the kernels' result by 5 x the bound, in the rms over the
(row, attribute) pairs the ingredient feeds, while the kernel is inside the bound against the right reference.  (Not on every
pair: where the target's probability is 0.998, an ignored mask changes a bf16 dlogits row by 0.002 |w|, half its bound.)

Measured on an MI355X: profiles/heads_rl_f64_ratios.txt.
"""
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import _lib, ops, rl_ops
from oracle import heads_rl_f64 as o

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
REAL_CALL = ops._call
_CACHE = {}


class Layout:
    def __init__(self, name, n_class, ld, tiled, ld_bf16=None):
        self.name, self.n_class, self.tiled = name, tuple(n_class), tiled
        self.ld = {F32: ld, BF16: ld_bf16 or ld}

    def __repr__(self):
        return self.name


TILED = [Layout("repo", o.REPO, 384, True), Layout("ppo", o.PPO, 320, True),
         Layout("edges7", (9, 8, 7, 1, 65, 64, 63), 256, True), Layout("wide1", (256,), 256, True)]
WAVE = [Layout("attr8", (56, 135, 18, 87, 18, 25, 7, 64), 448, False), Layout("ld640", (256, 200, 135), 640, False),
        Layout("unpadded", o.REPO, 339, False, 340), Layout("slots", (1, 63, 64, 65, 128, 129, 255), 768, False)]
EDGES7, SLOTS = TILED[2], WAVE[3]
NAME = {F32: "f32", BF16: "bf16"}
RAN = {}          # (entry point, family, dtype) -> cases, asserted complete by the last test of the module


def note(label, ratios):
    print("    %-44s %s" % (label, "  ".join("%s %.2f" % kv for kv in ratios.items())))


# ----------------------------------------------------------------------------------------------------------------------
# recording the entry points
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    log = []
    where = {"cwlt_heads_fwd": (11, 13, None), "cwlt_heads_ce_bwd": (8, 9, 6), "cwlt_heads_logp_bwd": (7, 8, 5)}

    def spy(name, *args, **kw):
        if name in where:
            ld, code, dl = where[name]
            fam = _lib.load().cwlt_heads_tiled(args[1], args[2], args[ld], args[code], args[0], None if dl is None else args[dl])
            log.append({"name": name[len("cwlt_heads_"):], "ld": args[ld], "code": args[code], "tiled": fam,
                        "ptr": args[0].value, "rows": args[ld - 1]})
        return REAL_CALL(name, *args, **kw)

    monkeypatch.setattr(ops, "_call", spy)
    monkeypatch.setattr(rl_ops, "_call", spy)          # rl_ops binds the name at import
    return log


def assert_route(log, name, lay, dtype, x, rows):
    """One entry point ran: `name`, on `dtype` and the layout's ld and family; ops.heads_tiled says the same."""
    assert [c["name"] for c in log] == [name], log
    c = log[0]
    assert c["code"] == _lib.dtype_code(dtype) and c["ld"] == lay.ld[dtype] and c["rows"] == rows, (c, lay)
    assert c["tiled"] == (1 if lay.tiled else 0), (c, lay)
    assert ops.heads_tiled(x, lay.n_class) == lay.tiled
    RAN.setdefault((name, lay.tiled, dtype), []).append((lay.name, rows))
    del log[:]


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def case(cuda, lay, dtype, rows, kind, oor=False, seed=1):
    """Inputs on the GPU and their f64 reference: computed once, shared, never modified."""
    key = (lay.name, dtype, rows, kind, oor, seed)
    if key not in _CACHE:
        x = o.make_logits(kind, rows, lay.n_class, lay.ld[dtype], dtype, seed)
        tgt = o.make_targets(rows, lay.n_class, seed + 1, oor, logits=x if kind == "peaked" else None)
        x, tgt = x.to(cuda), tgt.to(cuda)
        _CACHE[key] = (x, tgt, o.heads_reference(x, lay.n_class, tgt))
        if len(_CACHE) > 6:
            del _CACHE[next(iter(_CACHE))]
    return _CACHE[key]


def forward(log, lay, dtype, x, tgt, ref, mask, label, full=True):
    """cwlt_heads_fwd through ops.heads_forward: loss sums [+ argmax, pmax, probs] against the reference."""
    rows = x.shape[0]
    bf = dtype == BF16
    before = x.clone()
    res = ops.heads_forward(x, lay.n_class, tgt, mask, want_argmax=full, want_pmax=full, want_probs=full)
    torch.cuda.synchronize()
    assert_route(log, "fwd", lay, dtype, x, rows)
    assert torch.equal(before.view(torch.int16 if bf else torch.int32), x.view(torch.int16 if bf else torch.int32))
    r = o.heads_ratios(ref, lay.n_class, lay.tiled, bf, mask, res["loss_sum"], pmax=res["pmax"], probs=res["probs"])
    if full:
        bad, share = o.argmax_check(res["argmax"], ref)
        assert bad == 0 and share <= o.SKIP_SHARE, (bad, share)
        assert res["probs"].shape == (rows, sum(lay.n_class))
    note(label, r)
    assert all(v <= 1 for v in r.values()), (label, r)
    return res, r


def ce_backward(log, lay, dtype, x, tgt, ref, mask, label):
    """ops.heads_ce: (A) losses and their gradient, upstream weights other than 1."""
    rows, A = x.shape[0], len(lay.n_class)
    bf = dtype == BF16
    used = sum(lay.n_class)
    gw = (torch.rand(A, generator=torch.Generator().manual_seed(5)) + 0.5).to(x.device)
    xg = x.clone().requires_grad_(True)
    loss = ops.heads_ce(xg, tgt, mask, lay.n_class)
    torch.cuda.synchronize()
    assert_route(log, "fwd", lay, dtype, x, rows)
    (loss * gw).sum().backward()
    torch.cuda.synchronize()
    assert_route(log, "ce_bwd", lay, dtype, x, rows)
    msum = mask.double().sum()
    b, D = o.loss_bound(ref, lay.n_class, mask, lay.tiled, bf, through_ce=True)
    r = {"ce loss": o.miss(loss.double() * msum, o.loss_sums(ref, mask), D * b)}
    want, w = o.ce_dlogits(ref, lay.n_class, mask, gw.double() / msum, lay.ld[dtype])
    got = xg.grad
    assert got.dtype == dtype and got.shape == x.shape
    assert (got[:, used:] == 0).all(), "padding columns of dlogits are exactly zero"
    bound = o.dlogits_bound(ref, lay.n_class, lay.tiled, bf, 2)
    r["dlogits"], exact = o.rows_ratio(got[:, :used], want[:, :used], w.abs(), bound, lay.n_class)
    assert exact, "rows of weight zero are exactly zero"
    note(label, r)
    assert all(v <= 1 for v in r.values()), (label, r)
    return got, want, w, bound


def logp_backward(log, lay, dtype, x, tgt, ref, label, g=None):
    """cwlt_heads_logp_bwd, called as rl_ops.LogPArgmaxFn.backward calls it, with the case's own targets."""
    rows, A = x.shape[0], len(lay.n_class)
    used = sum(lay.n_class)
    if g is None:
        g = torch.randn(rows, A, generator=torch.Generator().manual_seed(6))
        g[::7] = 0
    g = g.to(x.device)
    w = (-g).float().contiguous()
    dl = torch.full_like(x, float("nan"))
    ops._call("cwlt_heads_logp_bwd", _lib.dev(x), _lib.int_array(lay.n_class), A, _lib.dev(tgt), _lib.dev(w), _lib.dev(dl),
              rows, x.stride(0), _lib.dtype_code(dtype), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert_route(log, "logp_bwd", lay, dtype, x, rows)
    assert (dl[:, used:] == 0).all(), "padding columns of dlogits are exactly zero"
    want = o.logp_dlogits(ref, lay.n_class, g, lay.ld[dtype])
    r, exact = o.rows_ratio(dl[:, :used], want[:, :used], g.double().abs().expand(rows, A),
                            o.dlogits_bound(ref, lay.n_class, lay.tiled, dtype == BF16, 0), lay.n_class)
    assert exact
    note(label, {"logp dlogits": r})
    assert r <= 1, (label, r)


def whole_case(cuda, log, lay, dtype, rows, kind, mask_kind, oor=False):
    x, tgt, ref = case(cuda, lay, dtype, rows, kind, oor)
    label = "%-5s %-4s %-8s %6d %-7s" % ("tiled" if lay.tiled else "wave", NAME[dtype], lay.name, rows, kind)
    mask = o.make_mask(mask_kind, rows).to(cuda)
    forward(log, lay, dtype, x, tgt, ref, mask, label + " " + mask_kind)
    for other in ("ones", "last", "tail"):
        if other != mask_kind:
            forward(log, lay, dtype, x, tgt, ref, o.make_mask(other, rows).to(cuda), label + " " + other, full=False)
    ce_backward(log, lay, dtype, x, tgt, ref, mask, label + " " + mask_kind)
    logp_backward(log, lay, dtype, x, tgt, ref, label)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", TILED + WAVE, ids=repr)
def test_every_layout_at_1031_rows(cuda, calls, lay, dtype):
    whole_case(cuda, calls, lay, dtype, 1031, "x3", "p80")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 31, 32, 33])
@pytest.mark.parametrize("lay", [EDGES7, SLOTS], ids=repr)
def test_row_counts_around_a_tile(cuda, calls, lay, rows, dtype):
    whole_case(cuda, calls, lay, dtype, rows, "peaked", "last")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind,mask_kind", [("peaked", "ones"), ("shifted", "tail"), ("ties", "p80")])
@pytest.mark.parametrize("lay", [EDGES7, SLOTS, TILED[0], WAVE[0]], ids=repr)
def test_inputs_with_clamped_targets(cuda, calls, lay, kind, mask_kind, dtype):
    """Inputs 2, 3, 4 with targets holding -5 and n + 3 (input 5) on both families."""
    x, tgt, ref = case(cuda, lay, dtype, 1031, kind, True)
    n = torch.tensor(lay.n_class, device=tgt.device)
    assert (tgt < 0).any() and (tgt >= n).any() and (ref["t"] >= 0).all() and (ref["t"] < n).all()
    if kind == "ties":      # all but a group of 8 that holds a single class (the last of n = 8 k + 1) have a tied maximum
        assert (ref["gap"] == 0)[:, n > 1].float().mean().item() > 0.8
    whole_case(cuda, calls, lay, dtype, 1031, kind, mask_kind, oor=True)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["x3", "peaked"])
@pytest.mark.parametrize("lay,rows", [(TILED[0], 32801), (WAVE[2], 4101)], ids=["tiled-32801", "wave-4101"])
def test_loop_regimes(cuda, calls, lay, rows, kind, dtype):
    """The second trip: 1 026 tiles on 1 024 blocks (two tiles in blocks 0 and 1, a 1-row last tile) and 4 101 rows on 4 096
    waves (two rows in the first five)."""
    if lay.tiled:
        assert (rows + 31) // 32 > 1024 and rows % 32 == 1
    else:
        assert 4 * o.heads_blocks(rows) == 4096 < rows
    whole_case(cuda, calls, lay, dtype, rows, kind, "p80")
    x, tgt, ref = case(cuda, lay, dtype, rows, kind)
    ones = o.make_mask("ones", rows).to(cuda)
    res = ops.heads_forward(x, lay.n_class, tgt, ones)
    del calls[:]
    b, D = o.loss_bound(ref, lay.n_class, ones, lay.tiled, dtype == BF16)
    inside = o.miss(res["loss_sum"], o.loss_sums(ref, ones), D * b)
    dropped = o.miss(res["loss_sum"], o.loss_sums(ref, ones, drop_from=((rows - 1) // 32) * 32 if lay.tiled else 4096), D * b)
    print("    teeth %-5s %-4s %6d rows: second trip / last tile dropped  inside %.2f, the mutant %.1f x the bound"
          % ("tiled" if lay.tiled else "wave", NAME[dtype], rows, inside, dropped))
    assert inside <= 1 and dropped >= o.TEETH


# ----------------------------------------------------------------------------------------------------------------------
# a misaligned base; buffers around the outputs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_misaligned_base_goes_to_the_wave_family(cuda, calls, dtype):
    """A column view big[:, 1:1 + W]: ld a multiple of the vector width, the base pointer not 16-byte aligned."""
    rows, W = 1031, 384
    vec = 8 if dtype == BF16 else 4
    lay = Layout("misaligned", o.REPO, W + vec, False)
    dense = o.make_logits("x3", rows, o.REPO, W, dtype, 3).to(cuda)
    big = torch.full((rows, W + vec), float("nan"), dtype=dtype, device=cuda)
    view = big[:, 1:1 + W]
    view.copy_(dense)
    assert view.stride(0) % vec == 0 and view.data_ptr() % 16 != 0 and big.data_ptr() % 16 == 0
    tgt = o.make_targets(rows, o.REPO, 4).to(cuda)
    ref = o.heads_reference(dense, o.REPO, tgt)
    mask = o.make_mask("p80", rows).to(cuda)
    res, _ = forward(calls, lay, dtype, view, tgt, ref, mask, "wave  %-4s misaligned view" % NAME[dtype])
    # heads_ce makes its input contiguous: the tiled family on ld = W, and the very result of the dense input
    a = view.clone(memory_format=torch.preserve_format)
    assert not view.is_contiguous()
    got = []
    for inp in (view, dense):
        xg = inp.detach().requires_grad_(True)
        loss = ops.heads_ce(xg, tgt, mask, o.REPO)
        loss.sum().backward()
        torch.cuda.synchronize()
        assert [(c["name"], c["ld"], c["tiled"]) for c in calls] == [("fwd", W, 1), ("ce_bwd", W, 1)], calls
        del calls[:]
        got.append((loss.detach().clone(), xg.grad.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert torch.equal(torch.nan_to_num(a.float()), torch.nan_to_num(view.float()))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", [TILED[0], WAVE[1]], ids=repr)
def test_nothing_outside_the_output_views_is_written(cuda, calls, lay, dtype):
    """probs as a (rows, used) view inside a wider, taller buffer; dlogits between two guard rows."""
    rows, A, used, ld = 33, len(lay.n_class), sum(lay.n_class), lay.ld[dtype]
    x, tgt, ref = case(cuda, lay, dtype, rows, "x3")
    SENT = 12345.0
    ldp = used + 8
    pbuf = torch.full((rows + 2, ldp), SENT, device=cuda)
    ops._call("cwlt_heads_fwd", _lib.dev(x), _lib.int_array(lay.n_class), A, None, None, None, None, None, None,
              _lib.dev(pbuf[1:]), rows, ld, ldp, _lib.dtype_code(dtype), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert_route(calls, "fwd", lay, dtype, x, rows)
    assert (pbuf[0] == SENT).all() and (pbuf[-1] == SENT).all() and (pbuf[1:-1, used:] == SENT).all()
    r, _ = o.rows_ratio(pbuf[1:-1, :used], ref["p"], ref["pmax"], o.probs_bound(ref, lay.n_class, lay.tiled, dtype == BF16), lay.n_class)
    assert r <= 1
    mask = o.make_mask("ones", rows).to(cuda)
    coef = torch.ones(A, device=cuda)
    g = torch.ones(rows, A, device=cuda)
    for name, extra in (("cwlt_heads_ce_bwd", (_lib.dev(mask), _lib.dev(coef))), ("cwlt_heads_logp_bwd", (_lib.dev(g),))):
        dbuf = torch.full((rows + 2, ld), SENT, dtype=dtype, device=cuda)
        ops._call(name, _lib.dev(x), _lib.int_array(lay.n_class), A, _lib.dev(tgt), *extra, _lib.dev(dbuf[1:]), rows, ld,
                  _lib.dtype_code(dtype), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert ops.heads_tiled(x, lay.n_class, dbuf[1:]) == lay.tiled and calls[0]["tiled"] == int(lay.tiled)
        del calls[:]
        assert (dbuf[0] == SENT).all() and (dbuf[-1] == SENT).all() and (dbuf[1:-1, used:] == 0).all()
        assert torch.isfinite(dbuf[1:-1].float()).all() and (dbuf[1:-1, :used] != SENT).all()


# ----------------------------------------------------------------------------------------------------------------------
# rl_ops.logp_argmax
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [33, 1031])
@pytest.mark.parametrize("lay", [TILED[0], WAVE[2]], ids=repr)
def test_logp_argmax_forward_and_backward(cuda, calls, lay, rows, dtype):
    x, _, ref = case(cuda, lay, dtype, rows, "x3")
    bf = dtype == BF16
    A = len(lay.n_class)
    up = torch.randn(rows, A, generator=torch.Generator().manual_seed(8)).to(cuda)
    xg = x.clone().requires_grad_(True)
    lp, ids = rl_ops.logp_argmax(xg, lay.n_class)
    torch.cuda.synchronize()
    assert_route(calls, "fwd", lay, dtype, x, rows)
    bad, share = o.argmax_check(ids, ref)
    assert bad == 0 and share <= o.SKIP_SHARE
    # log(pmax): the pmax bound relative, plus torch's f32 log (2 ulp of |log pmax|)
    pb = o.probs_bound(ref, lay.n_class, lay.tiled, bf)
    want = torch.log(ref["pmax"])
    r = {"logp": o.miss(lp, want, torch.sqrt(pb ** 2 + (8 * o.U32 * want.abs()) ** 2) + 1e-300)}
    (lp * up).sum().backward()
    torch.cuda.synchronize()
    assert_route(calls, "logp_bwd", lay, dtype, x, rows)
    aref = dict(ref, t=ref["argmax"])
    wantg = o.logp_dlogits(aref, lay.n_class, up, lay.ld[dtype])
    used = sum(lay.n_class)
    r["dlogits"], exact = o.rows_ratio(xg.grad[:, :used], wantg[:, :used], up.double().abs(),
                                       o.dlogits_bound(ref, lay.n_class, lay.tiled, bf, 0), lay.n_class)
    note("logp_argmax %-5s %-4s %5d" % ("tiled" if lay.tiled else "wave", NAME[dtype], rows), r)
    assert exact and (xg.grad[:, used:] == 0).all() and all(v <= 1 for v in r.values()), r


# ----------------------------------------------------------------------------------------------------------------------
# teeth
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("lay", [TILED[0], WAVE[0]], ids=repr)
def test_teeth(cuda, calls, lay, dtype):
    rows, nc, bf = 1031, lay.n_class, dtype == BF16
    fam = "%-5s %-4s" % ("tiled" if lay.tiled else "wave", NAME[dtype])
    mask = o.make_mask("p80", rows).to(cuda)
    ones = o.make_mask("ones", rows).to(cuda)

    def say(name, what, inside, mutant):
        print("    teeth %-10s %s %-8s inside %.2f, the mutant %.1f x the bound" % (name, fam, what, inside, mutant))
        assert inside <= 1 and mutant >= o.TEETH, (name, what, inside, mutant)

    x, tgt, ref = case(cuda, lay, dtype, rows, "x3")
    res = ops.heads_forward(x, nc, tgt, mask)
    res1 = ops.heads_forward(x, nc, tgt, ones)
    del calls[:]
    b, D = o.loss_bound(ref, nc, mask, lay.tiled, bf)
    b1, D1 = o.loss_bound(ref, nc, ones, lay.tiled, bf)
    inside = o.miss(res["loss_sum"], o.loss_sums(ref, mask), D * b)
    off1 = o.heads_reference(x, nc, tgt, mutant="target+1")
    say("target+1", "loss", inside, o.miss(res["loss_sum"], o.loss_sums(off1, mask), D * b))
    say("no mask", "loss", inside, o.miss(res["loss_sum"], o.loss_sums(ref, None), D * b))
    say("tail", "loss", o.miss(res1["loss_sum"], o.loss_sums(ref, ones), D1 * b1),
        o.miss(res1["loss_sum"], o.loss_sums(ref, ones, drop_from=1024), D1 * b1))
    # gradients: per (row, attribute), the rms miss over the pairs the ingredient feeds
    def rms(t):
        return t.pow(2).mean().sqrt().item()

    got, want, w, bound = ce_backward(calls, lay, dtype, x, tgt, ref, mask, "teeth " + fam)
    used = sum(nc)
    gw = (torch.rand(len(nc), generator=torch.Generator().manual_seed(5)) + 0.5).to(cuda).double()
    msum = mask.double().sum()
    inside = o.pair_ratios(got[:, :used], want[:, :used], w.abs(), bound, nc)
    inside = inside[~torch.isnan(inside)].max().item()
    live = (w.abs() > 0) & (torch.tensor(nc, device=cuda) > 1)
    m1, _ = o.ce_dlogits(off1, nc, mask, gw / msum, lay.ld[dtype])
    say("target+1", "dlogits", inside, rms(o.pair_ratios(got[:, :used], m1[:, :used], w.abs(), bound, nc)[live]))
    m2, w2 = o.ce_dlogits(ref, nc, ones, gw / msum, lay.ld[dtype])
    dead = (w == 0)
    say("no mask", "dlogits", inside, rms(o.pair_ratios(got[:, :used], m2[:, :used], w2.abs(), bound, nc)[dead]))
    m3, _ = o.ce_dlogits(ref, nc, mask, gw, lay.ld[dtype])
    say("coef", "dlogits", inside, rms(o.pair_ratios(got[:, :used], m3[:, :used], w.abs(), bound, nc)[w.abs() > 0]))
    # input 3 without the max subtraction overflows; input 4 with the last tied index
    x, tgt, ref = case(cuda, lay, dtype, rows, "shifted")
    res = ops.heads_forward(x, nc, tgt, mask)
    b, D = o.loss_bound(ref, nc, mask, lay.tiled, bf)
    say("no max", "loss", o.miss(res["loss_sum"], o.loss_sums(ref, mask), D * b),
        o.miss(res["loss_sum"], o.loss_sums(o.heads_reference(x, nc, tgt, mutant="nomax"), mask), D * b))
    x, tgt, ref = case(cuda, lay, dtype, rows, "ties")
    res = ops.heads_forward(x, nc, want_argmax=True)
    last = o.heads_reference(x, nc, mutant="lastmax")
    bad, _ = o.argmax_check(res["argmax"], ref)
    badm, _ = o.argmax_check(res["argmax"], last)
    print("    teeth last index %s argmax mismatches: reference %d, the mutant %d of %d" % (fam, bad, badm, ref["argmax"].numel()))
    assert bad == 0 and badm > 0.9 * ref["argmax"].numel()


def test_both_families_ran_every_entry_point_in_both_types():
    """Runs last, over what the tests above recorded (nothing to say when they were deselected)."""
    if not RAN:
        pytest.skip("the tests of this module that record their routes were not run")
    for name in ("fwd", "ce_bwd", "logp_bwd"):
        for tiled in (True, False):
            for dtype in (F32, BF16):
                ran = RAN.get((name, tiled, dtype), [])
                assert ran, (name, tiled, dtype)
                assert any(rows == (32801 if tiled else 4101) for _, rows in ran), (name, tiled, dtype)

"""GPU: the bf16 encoder and the bf16 train step in every row-count regime, dropout on, against the f64 reference with
the kernels' own dropout masks (oracle/step_f64.py, oracle/dropout.py), with the dispatch thresholds as shipped.

Which kernels a bf16 encoder pass runs depends on its token rows R = N * L (ops.py, encoder.py, cw_transformer.py,
gemm_nt.hip):

    R <= 8 192        the whole stack as one host call (csrc/layer.hip, encoder._EncoderStackFn)
    8 193 - 16 383    per-op layer: hipBLASLt projections, FFN on gemm_nt's 128 x 256 kernel, NN input gradients
    16 384 - 32 767   + the transposed-weight cache (LayerCache.refresh_transposed), NT input gradients
    32 768 - 65 535   + cwlt_gemm_bf16 projections and accumulate forms, FFN on the 256 x 256 epilogue kernel
    >= 65 536         + linear_ln (out-projection, bias, dropout, residual and LayerNorm in one kernel)
    front, >= 8 192   embed_proj (embedding, in_linear, posenc and dropout in one pass)

Every case wraps the ops entry points and asserts the regime it names, so that a threshold change cannot move it off
that path unnoticed, and records the dropout seeds the layers draw (ops.next_seed / ops.next_seeds): the reference
runs on the same bf16 input and upstream gradient with the same seeds.  Launches stay eager (seed_base NULL).

Bound.  As tests/test_model_gpu.py::BF16_GRAD_REL: every activation that crosses HBM in bf16 carries a relative error
of rms u = 2^-9 / sqrt(3); one layer stores about 10 such tensors on the forward path and as many on the backward path,
the final norm one each way, so an encoder of n_l layers puts n = 2 * (10 * n_l + 1) roundings between its input and a
parameter gradient, and independent perturbations add up to sqrt(n) * u of a tensor's norm.  The tests allow 4x that,
4 * sqrt(n) * 2^-9 / sqrt(3), of each tensor's OWN norm (2.9 % for two layers, 2.1 % for one), with the model test's
floor of 1e-4 of the rms parameter-gradient norm for a gradient that is nearly zero.
The Q and K projection gradients are worse conditioned, in two ways the f64 reference measures per layer.  (1) The
attention backward forms d phi(q) and d phi(k) as differences of two sums whose second one, the normaliser term,
nearly cancels the first when a row averages over many tokens (oracle/step_f64.normaliser_terms); the scan kernels
build both from bf16 operands (dout, the attention output and g = dout * z), so those three roundings reach each row
multiplied by G = |normaliser term| / |gradient| (measured: about 10 for Q in the last of two layers at L = 1 000, below
1 for K).  (2) The output does not change when phi(q_i) or all phi(k_j) are scaled, so the rows of these gradients
largely cancel in the parameter gradients (their sums over rows); errors of the rows do not cancel with them, so the
relative error grows by C = |uncancelled row sum| / |parameter gradient| (oracle/step_f64.row_terms, taken as >= 1).
Their bound is 4 * sqrt(n + 3 G^2) * 2^-9 / sqrt(3) * C.

Teeth.  With p = 0.1 the reference is also built with one wrong ingredient -- the last layer's linear2 mask drawn with
its FFN-activation seed, or the first layer's FFN-activation mask shifted by one element pair -- and must then miss the
kernels' result by at least 5x the bound on the tensors that ingredient feeds.
"""
import collections
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import encoder, ops  # noqa: E402
from oracle import dropout, step_f64  # noqa: E402

pytestmark = pytest.mark.gpu
N_CLASS = [56, 135, 18, 87, 18, 25]
U = 2.0 ** -9 / 3 ** 0.5
TEETH = 5.0


def encoder_bound(n_layers, gain=0.0):
    return 4 * (2 * (10 * n_layers + 1) + 3 * gain ** 2) ** 0.5 * U


# tests/test_model_gpu.py derives it: 12 layers + embedding / in_linear / positional encoding / final norm / logits
BF16_GRAD_REL = 4 * (2 * (12 * 10 + 5)) ** 0.5 * U


class Spy:
    """Counts the calls of the ops entry points that tell the regimes apart, the accumulate forms of gemm_bf16, the
    final_state that reached each cla_bwd, and the dropout seeds drawn (one list entry per draw)."""

    NAMES = ("encoder_fwd", "linear_ln", "ffn1_gelu_dropout", "gemm_nt_mul", "gemm_bf16", "ln_fwd", "embed_proj")

    def __init__(self, monkeypatch):
        self.calls = collections.Counter()
        self.fin = []
        self.draws = []
        self.seeds = []
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        real_bwd, real_seed, real_seeds = ops.cla_bwd, ops.next_seed, ops.next_seeds

        def cla_bwd(*a, **kw):
            self.fin.append(kw.get("final_state") is not None)
            return real_bwd(*a, **kw)

        def next_seed():
            s = real_seed()
            self.draws.append(1)
            self.seeds.append(s)
            return s

        def next_seeds(k):
            s = real_seeds(k)
            self.draws.append(k)
            self.seeds.extend(s)
            return s

        monkeypatch.setattr(ops, "cla_bwd", cla_bwd)
        monkeypatch.setattr(ops, "next_seed", next_seed)
        monkeypatch.setattr(ops, "next_seeds", next_seeds)

    def _wrap(self, name, real):
        def f(*a, **kw):
            self.calls[name] += 1
            if name == "gemm_bf16" and kw.get("accumulate"):
                self.calls["gemm_bf16_acc"] += 1
            return real(*a, **kw)
        return f


def _encoder(cuda, n_layers, p, seed):
    """tests/test_layer_c_gpu.py::_encoder: repo layer shape, weights ~ 1 / sqrt(fan-in), LayerNorm weights around one."""
    enc = encoder.TransformerEncoderBuilder.from_kwargs(
        n_layers=n_layers, n_heads=8, query_dimensions=64, value_dimensions=64, feed_forward_dimensions=2048,
        activation="gelu", dropout=p, attention_type="causal-linear").get()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for q in enc.parameters():
            q.copy_(torch.randn(q.shape, generator=g) * (1.0 / q.shape[1] ** 0.5 if q.dim() == 2 else 0.2))
        for layer in enc.layers:
            layer.norm1.weight.add_(1.0)
            layer.norm2.weight.add_(1.0)
        enc.norm.weight.add_(1.0)
    return enc.to(cuda)


def _ratios(got, ref, names):
    """||got - ref|| / max(||ref||, 1e-4 x the rms norm of the parameter gradients `names`), per tensor."""
    norms = {k: ref[k].norm().item() for k in ref}
    floor = 1e-4 * (sum(norms[k] ** 2 for k in names) / len(names)) ** 0.5
    return {k: (got[k].double() - ref[k]).norm().item() / max(norms[k], floor) for k in ref}


def _report(label, r, bounds):
    """Prints every tensor's error against its bound; -> the tensor nearest to (or furthest past) its bound."""
    worst = max(r, key=lambda k: r[k] / bounds[k])
    print("%s: worst %s %.5f (bound %.5f)" % (label, worst, r[worst], bounds[worst]))
    for k in sorted(r, key=lambda k: r[k] / bounds[k], reverse=True):
        print("    %-58s %.5f  bound %.5f" % (k, r[k], bounds[k]))
    return worst


def _bounds(norms, n_layers, gains):
    """encoder_bound for every tensor of `norms` (name -> the reference's norm); the Q / K projection gradients of layer i
    with its normaliser gain, times the cancellation of their row sums (at least one)."""
    b = {k: encoder_bound(n_layers) for k in norms}
    for i, gd in enumerate(gains):
        for part in ("query", "key"):
            for j, s in enumerate(("bias", "weight")):
                name = "layers.%d.attention.%s_projection.%s" % (i, part, s)
                b[name] = encoder_bound(n_layers, gd[part]) * max(1.0, gd[part + "_rows"][j] / max(norms[name], 1e-300))
    return b


def _assert_regime(spy, enc, N, L, p, n_layers):
    R = N * L
    c = spy.calls
    seg1 = ops.scan_segments(N, 8, L, torch.bfloat16) == 1
    print("regime R=%d: calls %s, final_state %s, draws %s, tcache %s" % (R, dict(c), spy.fin, spy.draws,
                                                                          enc._tcache is not None))
    assert ops._seed_base() is None                                 # eager launches: the seeds are the keys
    if R <= ops.LAYER_C_MAX_ROWS:
        assert c["encoder_fwd"] == 1 and spy.fin == []
        assert c["linear_ln"] == c["ffn1_gelu_dropout"] == c["gemm_nt_mul"] == c["gemm_bf16"] == 0
        assert c["ln_fwd"] == 1                                     # the final norm
        assert spy.draws == ([3 * n_layers] if p > 0 else [])
        assert enc._tcache is None
        return
    assert c["encoder_fwd"] == 0
    assert spy.draws == ([1] * (3 * n_layers) if p > 0 else [])
    assert c["ffn1_gelu_dropout"] == n_layers and c["gemm_nt_mul"] == n_layers
    assert spy.fin == [seg1] * n_layers                              # one-sweep backward iff whole-sequence scans
    assert (enc._tcache is not None) == (R >= 16384)
    big = R >= ops.GEMM_BF16_MIN_ROWS
    fused = R >= ops.LINEAR_LN_MIN_ROWS
    assert c["linear_ln"] == (n_layers if fused else 0)
    assert c["ln_fwd"] == (1 if fused else 2) * n_layers + 1
    # forward: Q/K/V, [out-projection,] linear2; backward: the out-projection's input gradient, and linear1's and Q/K/V's
    # accumulated onto the residual gradients ds2 and ds1
    assert c["gemm_bf16_acc"] == (2 * n_layers if big else 0)
    assert c["gemm_bf16"] - c["gemm_bf16_acc"] == ((3 if fused else 4) * n_layers if big else 0)


def _run_encoder(enc, x, dy, monkeypatch):
    enc.train()
    for q in enc.parameters():
        q.grad = None
    spy = Spy(monkeypatch)
    torch.manual_seed(1234)                                         # ops.next_seed(): the dropout streams
    xin = x.clone().requires_grad_(True)
    y = enc(xin, attn_mask=encoder.TriangularCausalMask(x.shape[1], device=x.device))
    y.backward(dy)
    torch.cuda.synchronize()
    got = {"out": y.detach(), "dx": xin.grad.detach()}
    got.update({n: q.grad.detach() for n, q in enc.named_parameters()})
    del y, xin
    return spy, got


def _reference(enc, x, dy, n_layers, p, seeds, slab, drop=dropout.dropout, gains=None):
    y, dx, grads = step_f64.encoder_vjp(dict(enc.named_parameters()), x, dy, n_layers, 8, p, seeds, slab, drop=drop,
                                        gains=gains)
    ref = {"out": y, "dx": dx}
    ref.update(grads)
    return ref


def _shifted(seed):
    """The kernels' dropout, except that the site keyed by `seed` reads its mask one element pair further on."""
    def drop(x, p, s, row0=0):
        return dropout.dropout(x, p, s, row0, offset=2 if s == seed else 0)
    return drop


def _check_encoder(cuda, monkeypatch, N, L, p, n_layers, slab_rows=16384):
    enc = _encoder(cuda, n_layers, p, seed=21 + N)
    g = torch.Generator().manual_seed(N * 1000 + L)
    x = torch.randn(N, L, 512, generator=g).bfloat16().to(cuda)
    dy = (torch.randn(N, L, 512, generator=g) * 0.1).bfloat16().to(cuda)
    spy, got = _run_encoder(enc, x, dy, monkeypatch)
    _assert_regime(spy, enc, N, L, p, n_layers)
    seeds = spy.seeds if p > 0 else [0] * (3 * n_layers)
    assert len(seeds) == 3 * n_layers and (p == 0 or len(set(seeds)) == len(seeds))
    slab = max(1, slab_rows // L)
    names = [n for n, _ in enc.named_parameters()]
    bound = encoder_bound(n_layers)
    gains = []
    ref = _reference(enc, x, dy, n_layers, p, seeds, slab, gains=gains)
    r = _ratios(got, ref, names)
    bounds = _bounds({k: ref[k].norm().item() for k in ref}, n_layers, gains)
    del ref
    print("normaliser gains (q, k) per layer:", ", ".join("(%.2f, %.2f)" % (gd["query"], gd["key"]) for gd in gains))
    worst = _report("N=%d L=%d p=%g" % (N, L, p), r, bounds)
    assert r[worst] <= bounds[worst], (worst, r[worst], bounds[worst])
    if p == 0:
        return
    last = n_layers - 1
    wrong = [("linear2 mask of layer %d drawn with its FFN-activation seed" % last,
              seeds[:3 * last + 2] + [seeds[3 * last + 1]], dropout.dropout,
              ["out", "dx", "layers.%d.linear2.weight" % last, "layers.%d.linear1.weight" % last]),
             ("FFN-activation mask of layer 0 shifted by one element pair", seeds, _shifted(seeds[1]),
              ["out", "dx", "layers.0.linear1.weight", "layers.0.linear2.weight"])]
    for label, s, drop, affected in wrong:
        bad = _reference(enc, x, dy, n_layers, p, s, slab, drop)
        rb = _ratios(got, bad, names)
        del bad
        print("  teeth, %s: %s" % (label, ", ".join("%s %.4f" % (k, rb[k]) for k in affected)))
        for k in affected:
            assert rb[k] >= TEETH * bound, (label, k, rb[k], TEETH * bound)


@pytest.mark.parametrize("N,L", [(30, 50),        # 1 500 rows: one host call per stack
                                 (9, 1000),       # 9 000: per-op, hipBLASLt projections, NN input gradients
                                 (17, 1000),      # 17 000: + transposed-weight cache, NT input gradients
                                 (40, 1000),      # 40 000: + cwlt_gemm_bf16 and its accumulate forms, 256 x 256 FFN
                                 (64, 1024),      # 65 536: + linear_ln
                                 (66, 1000)])     # 66 000: ragged (L % 64, R % 256 != 0) at the bench's dispatch
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_encoder_regime_matches_the_f64_reference(cuda, monkeypatch, N, L, p):
    """A 2-layer repo-shape bf16 encoder (+ final norm) in train mode: output, input gradient and every parameter
    gradient against the f64 reference with the recorded seeds."""
    _check_encoder(cuda, monkeypatch, N, L, p, 2)


def test_one_layer_at_the_bench_rows_matches_the_f64_reference(cuda, monkeypatch):
    """B = 512 x T = 1024 = 524 288 rows, dropout on: the FFN masks' element indices reach 2^30 and byte offsets pass
    2^31.  Whole tensors are compared; the reference runs in slabs of 32 sequences."""
    _check_encoder(cuda, monkeypatch, 512, 1024, 0.1, 1, slab_rows=32768)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kernel_masks_equal_the_restatement(cuda, p):
    """The keep flags of a (R, 512) site (cwlt_posenc_dropout) and of a (R, 2048) one (cwlt_bias_gelu_dropout_fwd) equal
    oracle/dropout.py's, element for element, and the kept values carry its scale."""
    seed = 0x1F2E3D4C5B6A7988 & ((1 << 62) - 1)
    R = 1 << 17
    y = ops.posenc_dropout(torch.ones(R, 512, dtype=torch.bfloat16, device=cuda), None, 1, p, seed)
    assert torch.equal(y != 0, dropout.site_mask(seed, p, R, 512, device=cuda))
    assert (y[y != 0].float() == torch.tensor(dropout.keep_scale(p)).bfloat16().float().item()).all()
    del y
    R = 1 << 16
    h = torch.full((R, 2048), 3.0, dtype=torch.bfloat16, device=cuda)
    keep = ops.gelu_fwd(h, None, p, seed + 1) != 0
    assert torch.equal(keep, dropout.site_mask(seed + 1, p, R, 2048, device=cuda))


def test_train_step_at_the_bench_dispatch_matches_the_f64_reference(cuda, monkeypatch):
    """LinearTransformer at repo dims (12 layers), bf16, train mode with dropout 0.1, B = 64 x T = 1024 = 65 536 rows: the
    bench's own dispatch (embed_proj front, linear_ln in every layer, transposed-weight cache, whole-sequence scans with
    the one-sweep backward, never the one-call stack).  The 6 losses and every parameter gradient against the f64 step
    reference with the recorded seeds, under BF16_GRAD_REL."""
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 512, "N_LAYER": 12, "N_HEAD": 8})
    try:
        net = fill_params(model.LinearTransformer(N_CLASS), seed=61).to(cuda).train()
    finally:
        config.AgentConfig.update(old)
    net.compute_dtype = torch.bfloat16
    B, T = 64, 1024
    g = torch.Generator().manual_seed(14)
    x = torch.stack([torch.randint(0, n, (B, T), generator=g) for n in N_CLASS], -1).to(cuda)
    y = torch.stack([torch.randint(0, n, (B, T), generator=g) for n in N_CLASS], -1).to(cuda)
    mask = torch.ones(B, T)
    mask[3, 700:] = 0
    mask[40:44, 900:] = 0
    mask[63, :5] = 0
    mask = mask.to(cuda)
    spy = Spy(monkeypatch)
    torch.manual_seed(4321)
    lg = net.train_step(x, y, mask)
    (sum(lg) / 6).backward()
    torch.cuda.synchronize()
    c = spy.calls
    print("calls %s, final_state %s, draws %d" % (dict(c), spy.fin, len(spy.draws)))
    assert ops._seed_base() is None
    assert c["embed_proj"] == 1 and c["linear_ln"] == 12 and c["encoder_fwd"] == 0
    assert net.transformer_encoder._tcache is not None
    assert ops.scan_segments(B, 8, T, torch.bfloat16) == 1 and spy.fin == [True] * 12
    assert spy.draws == [1] * 37 and len(set(spy.seeds)) == 37     # the front, then 3 per layer
    params = {n: q for n, q in net.named_parameters()}
    l64, ref = step_f64.step_grads(params, net.pos_emb.pe, x, y, mask, N_CLASS, 12, 8, 0.1, spy.seeds, slab=16)
    l16 = torch.tensor([l.item() for l in lg], dtype=torch.float64)
    l64 = l64.cpu()
    print("losses bf16 %s f64 %s" % (l16.tolist(), l64.tolist()))
    assert (l16 - l64).abs().max().item() <= BF16_GRAD_REL * l64.abs().max().item()
    names = [n for n in params if ref[n] is not None]
    assert all(params[n].grad is None for n in params if ref[n] is None)
    assert all(n.startswith("project_concat_type") for n in params if ref[n] is None)
    got = {n: params[n].grad for n in names}
    assert all(got[n].dtype == torch.float32 and torch.isfinite(got[n]).all() for n in names)
    r = _ratios(got, {n: ref[n] for n in names}, names)
    worst = _report("train step B=64 T=1024 p=0.1", r, {n: BF16_GRAD_REL for n in names})
    assert r[worst] <= BF16_GRAD_REL, (worst, r[worst], BF16_GRAD_REL)

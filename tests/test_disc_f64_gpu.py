"""GPU: the band-attention kernels and both Longformer discriminators, f32 and bf16, dropout off and on, against the f64
reference with the kernels' own dropout masks (oracle/disc_f64.py, pinned by tests/test_oracle_disc_f64_cpu.py).

Reference.  oracle/disc_f64.py in f64 on the GPU (plain torch ops, none of the project's kernels), on the very values the
kernels are given (the bf16 kernels' inputs are bf16 values, so the reference of a bf16 case starts from the rounded
inputs; model parameters are the f32 masters in both).  Dropout seeds are recorded by wrapping ops.next_seed; launches
are eager (seed_base NULL), so the seeds are the keys.

Kernel level (csrc/band_attn.hip), fused (B, L, 3, H, 64) layout, forward and backward.
  Forms, asserted from the arguments that reach cwlt_band_attn_fwd (ops._call is wrapped): "f32" (FMA), "mfma" (bf16,
  every row stride a multiple of 8 and every pointer 16-byte aligned) and "generic" (band_attn_fwd_kernel<bf16_t>, any
  other bf16 view).  The generic form is reached through ops.band_attention by q, k, v that are column blocks of a buffer
  of row width 3 H 64 + 4 (stride a multiple of 4, not of 8).  Its pointer leg cannot be reached through the package:
  ops._row_stride copies every view whose base is not 16-byte aligned, so that leg is covered by calling
  cwlt_band_attn_fwd directly on a buffer that starts 8 bytes off (test_generic_form_by_a_misaligned_pointer).  The
  backward has one kernel per dtype and always sees the contiguous fused buffer.
  Measure: per query row of 64 (per key row for dk and dv), |got - ref| / max(|ref|, rms |ref| / 4): relative to the
  row's own norm, the floor a quarter of the tensor's rms row norm.  The rows of dq and dk are sums of
  dS_ij = P_ij (keep_ij dO_i.v_j - delta_i), a difference of two sums of 64 terms of either sign that vanishes identically
  where a row has one admissible key and nearly where one key dominates (there the kernels return rounding noise around
  an exact zero: emulating nothing but the bf16 roundings in f64 on the CPU puts the worst of 2 000 such rows at 12 U of
  its norm, 96 U with a single-key window), so their denominator is also at least the norm the row would have if nothing
  in it cancelled (oracle.disc_f64.band_attention_row_terms), as the regimes test does for the encoder's Q / K gradients;
  the same emulation then has its worst row at 3.4 U under the bound of 6.9 U.
  Rows that are zero by the mask alone (masked query; no admissible key; for dk / dv a masked key or a key no live query
  reaches) must be exactly zero, a fully masked window must leave dq = dk = dv = 0, and lse must be finite exactly on the
  other rows.
  Bounds, u = 2^-24 per f32 operation, U = 2^-9 / sqrt(3) rms per bf16 rounding, independent errors, 4x the predicted rms
  (the rule of tests/test_bf16_regimes_gpu.py and test_decode_f64_gpu.py; a sum of n terms counts n / 6):
    f32 forward   n_a = 64/6 x max(1, 2 ln K) (score) + 1 (q / 8) + 4 (s - m, expf at 2 ulp) + K/6 (row of P V, K =
                  min(2w + 1, L) keys) + 2 T (rescale of o and l per key tile, T = ceil(K / 64) + 1) + 2 (1 / l, product):
                  4 sqrt(n_a) u; 2.4e-6 at (L 50, w 25), 3.7e-6 at (L 1 024, w 256).  The score term: a sum of 64 products
                  errs by u sqrt(64/6) times the size of its partial sums, ABSOLUTELY, and that becomes the relative
                  error of the probability; the keys that carry a row are those with the largest of its K scores, about
                  sqrt(2 ln K) for scores of unit variance (randn q and k: q.k / 8 has variance one).  With 64/6 alone
                  the torch f32 chain on the CPU, no kernel involved, already sits at 0.76 of the bound in its worst row.
                  lse: the same bound, of max(1, |lse|).
    f32 backward  the forward's lse and out (delta = dO . out) feed it, 2 n_a; score, dO.v and delta are sums of 64, 3 x
                  64/6; expf, the difference, the products 8; the sum over K keys or queries K/6:
                  4 sqrt(2 n_a + 40 + K/6) u.
    bf16 forward  generic: f32 arithmetic on bf16 inputs, the output rounds once: 4 U = 4.5e-3.  mfma: the probabilities
                  round to bf16 as well: 4 sqrt(2) U = 6.4e-3 (q / 8 is exact in bf16).  Fed the same values, both forms
                  must sit inside their bounds.  lse is an f32 quantity in both: the generic form takes the f32 bound, the
                  mfma form, whose __expf multiplies the argument by log2(e) first (u |x|, |x| <= 4 where it counts),
                  4 sqrt(n_a + 16) u of max(1, |lse|), which replaces the 1e-3 of tests/test_discriminator_gpu.py.
    bf16 backward the forward's out carries two roundings into delta, the gradients round once: 4 sqrt(3) U = 7.8e-3.

Models at repo dims (fill_params weights, LayerNorm weights around one; masks with padded tails and one fully padded
window), hidden rows (B L rows of 512) relative to each row's norm, both schedules (no-grad scoring and autograd) held
to the same bound with the same seeds:
    bf16  per layer 9 activations cross HBM in bf16 (qkv, the MFMA kernel's probabilities, the attention output, the
          dense output, h1, the intermediate pre-activation, the GELU output, the output-dense output, h) and 4 weight
          matrices are rounded copies; the front has 5 (embedding, proj weight, inputs_embeds, their sum with the
          position row, the embedding LayerNorm) + 1 with dropout on.  n = 13 n_l + 5 (+ 1): 4 sqrt(n) U = 5.2e-2 for the
          10 layers of AIRL, 5.7e-2 for the reward model's 12.
    f32   per layer 512/6 (Q/K/V) + n_a + 512/6 + 2 (dense, bias, residual) + 4 (LayerNorm) + 512/6 + 3 (intermediate,
          GELU) + 1 024/6 + 2 + 4; the front 1 + 1 472/6 + 2 + 4 + 1.  AIRL: n = 5 700, 4 sqrt(n) u = 1.8e-5.
    Scores, running statistics and rewards are functions of all hidden rows through a mean over the window, a BatchNorm
    on batch statistics (which divides by the small spread of the window means), two tanh and a sigmoid, so their bound
    is PROPAGATED through the reference: the f64 hidden rows are perturbed by independent errors of the predicted rms
    (sqrt(n) U resp. sqrt(n) u of each row's norm), every later stage by its own f32 roundings (the jitter argument of
    oracle.disc_f64.score_classifier / ppo_reward; the reward model's logits also by their two bf16 roundings), 16 draws,
    and an element may miss by 4x the rms change of that element (at least the tensor's rms change).  Nothing of the
    kernels enters it.
    The losses are means over thousands of rows and take the same propagated bound (token_ce / bce / airl_losses carry
    the jitter too); the hidden-row bound times the loss, the regimes test's rule, would allow 0.2 where bf16 errs by
    2e-5.  The rounded weight copies of a bf16 model err every row by the same linear map, which a mean over rows (the
    BatchNorm's running mean above all) does not average out: the propagation gives that share, sqrt(4 n_l + 1) U, to
    one random matrix applied to all rows (weight_eps) and only the rest to independent errors.
    Gradients, every parameter, relative to the tensor's own norm in the reference: the forward count again for the
    backward path plus the heads, bf16 4 sqrt(2 n + 3) U (7.5e-2 AIRL, 8.2e-2 reward model), f32 4 sqrt(2 n + 512/6 + 3) u.
    Where a gradient is a sum of terms that cancel, the terms' errors do not cancel with them, so the denominator is at
    least the norm the sum would have without the cancellation, taken from the reference: (1) across the loss terms --
    the expert BCE and the agent BCE pull the score classifier in opposite directions, at scores near one half their
    gradients cancel to a hundredth -- sqrt(sum over terms |g_term|^2); (2) across rows, oracle.disc_f64.row_terms, as
    step_f64.row_terms and the regimes test do for the encoder: the query / key projections (the key bias gradient is
    zero in exact arithmetic: softmax does not see it); (3) inside the backward of the BatchNorm on batch statistics,
    which subtracts the batch mean of a gradient that a BCE against one label makes nearly the same for every window:
    score_classifier.0 (its bias gradient is zero in exact arithmetic too) and score_classifier.1.weight
    (oracle.disc_f64.classifier_row_terms).  The project's floor (1e-4 of the rms
    parameter-gradient norm, tests/test_model_gpu.py) is asserted to decide no tensor.  word_embeddings, the *_global
    projections, the pooler (and the reward model's eval_* heads in train_step) get no gradient at all, position rows
    outside 2 .. L + 1 and token type 1 exactly zero.

Teeth (TEETH = 5, p = 0.1): the reference rebuilt with one wrong ingredient -- window w + 1; the key mask shifted by one
position; attention keep flags with i and j exchanged; the last layer's attention-output dropout drawn with its
output-dense seed -- must miss the kernels' result, in the rms over the rows the ingredient feeds, by at least 5x the
bound.  The three attention ingredients are asked at kernel level of both dtypes and of the f32 model; the hidden-dropout
seed of the f32 model only: it moves the last hidden rows by 2 to 7 per cent, which ten layers of bf16 (5 x 5.2e-2)
cannot resolve (tests/test_oracle_disc_f64_cpu.py measures both figures).  A keep scale of 1 / (1 - p) instead of
65536 / (65536 - t) differs by 6e-6 relative and is no tooth.

Measured on an MI355X, worst figure / bound per group (every figure: profiles/disc_f64_ratios.txt; 85 tests, 13 s):
    band attention, all shapes, masks and p   f32: out 0.46, lse 0.55, dq 0.44, dk 0.44, dv 0.28
                                              mfma: out 0.61, lse 0.12, dq 0.74, dk 0.74, dv 0.33;  generic: out 0.57, lse 0.18
    hidden rows                               f32 0.06 (AIRL), 0.05 (reward model);  bf16 0.20 .. 0.22 in every case
    AIRL scores                               f32 0.24 eval, 0.28 train;  bf16 0.24 eval, 0.38 train, 0.47 in groups
    running mean / var                        f32 0.43 / 0.32;  bf16 0.22 / 0.52
    rewards                                   f32 0.42;  bf16 0.20
    AIRL losses (expert, agent, CE)           f32 0.01, 0.08, 0.01;  bf16 0.11, 0.13, 0.08;  reward model's six, bf16: 0.22
    gradients, worst tensor                   AIRL f32 0.07, bf16 0.20;  reward model bf16 0.20
    key-bias gradients                        4e-7 (f32), 7e-3 (bf16) of the uncancelled row sum
    teeth, weakest                            kernel level f32 39 913 x, bf16 19.4 x (window + 1, backward);  f32 model
                                              1 180 x (window + 1)
The f32 model bound is generous: library GEMMs do not add their 512 or 1 024 terms one after the other as the count
assumes (the torch f32 chain on the CPU measures 0.03 of it).  No kernel had to change: the first run's misses were
all in this file -- denominators that let |dO.v| itself cancel, and a propagation that took the rounded weights' error
for independent from row to row (it put the bf16 running mean at 3.7 .. 6.3 of its bound) -- and were traced on the CPU
with stand-ins for the kernels before the measure, not the multiplier, was corrected.
"""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import _lib, ops  # noqa: E402
from oracle import disc_f64, dropout  # noqa: E402

pytestmark = pytest.mark.gpu
N_CLASS = [56, 135, 18, 87, 18, 25]
U16 = 2.0 ** -9 / 3 ** 0.5
U32 = 2.0 ** -24
TEETH = 5.0
REAL_NEXT_SEED = ops.next_seed
REAL_CALL = ops._call
BF16, F32 = torch.bfloat16, torch.float32


# ----------------------------------------------------------------------------------------------------------------------
# bounds (derived in the docstring)
# ----------------------------------------------------------------------------------------------------------------------
def attn_n32(L, w):
    K = min(2 * w + 1, L)
    return 64 / 6 * max(1.0, 2 * math.log(K)) + 1 + 4 + K / 6 + 2 * ((K + 63) // 64 + 1) + 2


def fwd_bound(form, L, w):
    return {"f32": 4 * attn_n32(L, w) ** 0.5 * U32, "generic": 4 * U16, "mfma": 4 * 2 ** 0.5 * U16}[form]


def bwd_bound(form, L, w):
    if form == "f32":
        return 4 * (2 * attn_n32(L, w) + 40 + min(2 * w + 1, L) / 6) ** 0.5 * U32
    return 4 * 3 ** 0.5 * U16


def lse_bound(form, L, w):
    return 4 * (attn_n32(L, w) + (16 if form == "mfma" else 0)) ** 0.5 * U32


def n16(n_layer, dropout_on):
    return 13 * n_layer + 5 + (1 if dropout_on else 0)


def n32(n_layer, L, w):
    layer = 512 / 6 + attn_n32(L, w) + 512 / 6 + 2 + 4 + 512 / 6 + 3 + 1024 / 6 + 2 + 4
    return 1 + 1472 / 6 + 2 + 4 + 1 + n_layer * layer


def hidden_eps(dtype, n_layer, L, w, dropout_on):
    """The predicted rms error of a hidden row relative to its norm; the bound is 4x it."""
    return n16(n_layer, dropout_on) ** 0.5 * U16 if dtype == BF16 else n32(n_layer, L, w) ** 0.5 * U32


def weight_eps(dtype, n_layer):
    """The share of hidden_eps that comes from the rounded weight copies of a bf16 model (4 matrices per layer and proj):
    one error map for every row, so it does not average out over rows as the activations' roundings do."""
    return (4 * n_layer + 1) ** 0.5 * U16 if dtype == BF16 else 0.0


def grad_bound(dtype, n_layer, L, w):
    if dtype == BF16:
        return 4 * (2 * n16(n_layer, True) + 3) ** 0.5 * U16
    return 4 * (2 * n32(n_layer, L, w) + 512 / 6 + 3) ** 0.5 * U32


# ----------------------------------------------------------------------------------------------------------------------
# spies
# ----------------------------------------------------------------------------------------------------------------------
def spy_forms(monkeypatch):
    """-> a list that receives the form of every cwlt_band_attn_fwd call, read off its arguments (the C side's own
    condition: include/cwlt.h, csrc/band_attn.hip)."""
    log = []

    def call(name, *a, **kw):
        if name == "cwlt_band_attn_fwd":
            ptrs = [a[i].value for i in (0, 1, 2, 4)]
            lds, dt = a[11:15], a[19]
            ok = not any(int(ld) & 7 for ld in lds) and not any(p & 15 for p in ptrs)
            log.append("f32" if dt == _lib.CWLT_F32 else "mfma" if ok else "generic")
        return REAL_CALL(name, *a, **kw)

    monkeypatch.setattr(ops, "_call", call)
    return log


class Seeds:
    """Records the dropout seeds the model draws (ops.next_seed), or hands out `replay` in order."""

    def __init__(self, monkeypatch, replay=None):
        self.seeds = []
        it = None if replay is None else iter(replay)

        def next_seed():
            s = REAL_NEXT_SEED() if it is None else next(it)
            self.seeds.append(s)
            return s

        monkeypatch.setattr(ops, "next_seed", next_seed)


def capture_encode(monkeypatch, net):
    """-> a list that receives the last hidden state of every net._encode call."""
    outs = []
    real = type(net)._encode

    def enc(data, masks):
        h = real(net, data, masks)
        outs.append(h.detach())
        return h

    monkeypatch.setattr(net, "_encode", enc, raising=False)
    return outs


# ----------------------------------------------------------------------------------------------------------------------
# measures
# ----------------------------------------------------------------------------------------------------------------------
def row_rel(got, ref, width, unc=None):
    """Per row of `width`: |got - ref| / max(|ref|, rms |ref| / 4 [, unc]) -> (rows,)."""
    g, r = got.double().reshape(-1, width), ref.reshape(-1, width)
    nr = r.norm(dim=1)
    den = torch.maximum(nr, nr.square().mean().sqrt() / 4)
    if unc is not None:
        den = torch.maximum(den, unc.reshape(-1))
    return (g - r).norm(dim=1) / den.clamp_min(1e-300)


def rms(t):
    return t.square().mean().sqrt().item()


def note(label, value, bound):
    """Prints a figure against its bound -> their ratio."""
    print("    %-64s %.3e  bound %.3e  (%.2f)" % (label, value, bound, value / bound))
    return value / bound


# ----------------------------------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------------------------------
def combo_mask(L, seed):
    """Four windows: a padded tail; holes and a masked first token; masked entirely; a single valid key."""
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(4, L)
    if L > 1:
        m[0, L - max(1, L // 4):] = 0
        m[1, torch.rand(L, generator=g) < 0.2] = 0
        m[1, 0] = 0
        m[1, L - 1] = 1
    m[2] = 0
    m[3] = 0
    m[3, L // 2] = 1
    return m


def tile_mask(L, w):
    """Two windows, the first with keys 128 .. 191 masked.  Verified here, not trusted: that is a whole 64-key tile, it lies
    strictly inside the key tiles the unmasked query tile 64 .. 127 loops over, and tiles on both sides of it hold keys
    that queries of that tile admit."""
    m = torch.ones(2, L)
    m[0, 128:192] = 0
    q0, kt = 64, 2
    kt0, kt1 = max(0, (q0 - w) // 64), min((q0 + 63 + w) // 64, (L - 1) // 64)
    assert (m[0, 64 * kt:64 * kt + 64] == 0).all() and (m[0, q0:q0 + 64] != 0).all() and kt0 < kt < kt1
    i = torch.arange(q0, q0 + 64)[:, None]
    for t in (kt - 1, kt + 1):
        j = torch.arange(64 * t, min(L, 64 * t + 64))[None, :]
        assert (((i - j).abs() <= w) & (m[0, j] != 0)).any()
    assert (((i - torch.arange(128, 192)[None, :]).abs() <= w)).any()       # the masked tile is inside the band
    return m


def structural_zero_rows(mask, B, L, w):
    """From the mask alone: (B, L) query rows with no admissible key or masked themselves; (B, L) key rows that are masked
    or that no live query reaches."""
    valid = torch.ones(B, L, dtype=torch.bool) if mask is None else mask.cpu() != 0
    idx = torch.arange(L)
    allow = ((idx[:, None] - idx[None, :]).abs() <= w)[None] & valid[:, None, :] & valid[:, :, None]
    return ~allow.any(2), ~allow.any(1)


def make_inputs(B, L, H, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, 3, H, 64, generator=g).to(cuda), torch.randn(B, L, H * 64, generator=g).to(cuda)


def reference(qkv, dout, mask, w, p, seed, keep=dropout.keep_flags):
    """f64 on qkv's device: out, lse, dqkv and the uncancelled row norms of dq and dk."""
    x = qkv.double().requires_grad_(True)
    md = None if mask is None else mask.to(qkv.device)
    out, lse = disc_f64.band_attention(x[:, :, 0], x[:, :, 1], x[:, :, 2], md, w, p, seed, keep=keep)
    out.backward(dout.double())
    with torch.no_grad():
        xd = x.detach()
        uq, uk = disc_f64.band_attention_row_terms(xd[:, :, 0], xd[:, :, 1], xd[:, :, 2], dout.double(), md, w, p, seed)
    return {"out": out.detach(), "lse": lse.detach(), "dqkv": x.grad, "uq": uq, "uk": uk}


def run_fused(qkv, dout, mask, w, p, seed):
    """Forward with lse through ops.band_attention on the fused layout, backward through ops.BandAttentionFn."""
    B, L, _, H, _ = qkv.shape
    md = None if mask is None else mask.to(qkv.device)
    out, lse = ops.band_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], md, w, p, seed, want_lse=True)
    x = qkv.clone().requires_grad_(True)
    out2 = ops.BandAttentionFn.apply(x, md, w, p, seed)
    out2.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    return {"out": out, "lse": lse, "dqkv": x.grad}


def run_generic(qkv16, mask, w, p, seed):
    """bf16 q, k, v as column blocks of a buffer of row width 3 H 64 + 4: ops.band_attention keeps the views (stride a
    multiple of 4, base aligned) and the C side must refuse them for the MFMA kernel."""
    B, L, _, H, _ = qkv16.shape
    ld = 3 * H * 64 + 4
    buf = torch.zeros(B, L, ld, dtype=BF16, device=qkv16.device)
    buf[..., :3 * H * 64] = qkv16.reshape(B, L, -1)
    q, k, v = (buf.as_strided((B, L, H, 64), (L * ld, ld, 64, 1), i * H * 64) for i in range(3))
    assert ops._row_stride(q) == ops._row_stride(k) == ops._row_stride(v) == ld and ld % 8 == 4
    md = None if mask is None else mask.to(qkv16.device)
    out, lse = ops.band_attention(q, k, v, md, w, p, seed, want_lse=True)
    torch.cuda.synchronize()
    return {"out": out, "lse": lse}


def check_forward(label, form, got, ref, qz, L, w):
    B, H = ref["lse"].shape[:2]
    out = got["out"].view(B, L, H, 64)
    assert torch.isfinite(out.float()).all()
    assert (out[qz.to(out.device)] == 0).all(), label                     # zero by the mask alone: exactly zero
    r = row_rel(out, ref["out"], 64)
    worst = note("%s %s out rows" % (label, form), r.max().item(), fwd_bound(form, L, w))
    fin = torch.isfinite(got["lse"])
    live = (~qz).to(fin.device)[:, None, :].expand(B, H, L)
    assert torch.equal(fin, live) and torch.equal(torch.isfinite(ref["lse"]), live), label
    assert (got["lse"][~fin] == float("inf")).all()
    worst_l = 0.0
    if fin.any():
        lr = ref["lse"][fin]
        worst_l = note("%s %s lse" % (label, form), ((got["lse"][fin].double() - lr).abs() / lr.abs().clamp_min(1)).max()
                       .item(), lse_bound(form, L, w))
    assert worst <= 1 and worst_l <= 1, (label, form, worst, worst_l)


def check_backward(label, form, got, ref, qz, kz, mask, L, w):
    d, rd = got["dqkv"], ref["dqkv"]
    assert torch.isfinite(d.float()).all()
    qz, kz = qz.to(d.device), kz.to(d.device)
    assert (d[:, :, 0][qz] == 0).all() and (d[:, :, 1][kz] == 0).all() and (d[:, :, 2][kz] == 0).all(), label
    if mask is not None:
        dead = (mask == 0).all(1).to(d.device)
        assert (d[dead] == 0).all(), label                                # a fully masked window contributes exactly zero
    worst = 0.0
    for i, (name, unc) in enumerate((("dq", ref["uq"]), ("dk", ref["uk"]), ("dv", None))):
        r = row_rel(d[:, :, i], rd[:, :, i], 64, unc)
        worst = max(worst, note("%s %s %s rows" % (label, form, name), r.max().item(), bwd_bound(form, L, w)))
    assert worst <= 1, (label, form, worst)


SHAPES = [(1, 0, 1), (1, 8, 8), (50, 25, 8), (50, 0, 1), (50, 100, 8), (63, 8, 1), (64, 25, 8), (64, 64, 1), (65, 8, 8),
          (65, 100, 1), (128, 25, 8), (128, 256, 1), (300, 100, 8), (300, 8, 1), (1024, 256, 8), (1024, 25, 1),
          (1024, 0, 1)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L,w,H", SHAPES)
def test_band_attention_matches_the_f64_reference(cuda, monkeypatch, L, w, H, masked, p):
    """Every form, forward and backward, at one shape: no mask, or four windows with a padded tail / holes and a masked
    first token / no valid key / a single valid key."""
    B = 4
    forms = spy_forms(monkeypatch)
    mask = combo_mask(L, 7 * L + w) if masked else None
    qz, kz = structural_zero_rows(mask, B, L, w)
    seed = (0x5DEECE66D * (L + 3 * w + H) + 11) & ((1 << 62) - 1) if p > 0 else 0
    qkv, dout = make_inputs(B, L, H, 100 * L + w + H, cuda)
    label = "L=%d w=%d H=%d %s p=%g" % (L, w, H, "mask" if masked else "none", p)
    print(label)
    ref = reference(qkv, dout, mask, w, p, seed)
    got = run_fused(qkv, dout, mask, w, p, seed)
    assert forms == ["f32", "f32"]
    check_forward(label, "f32", got, ref, qz, L, w)
    check_backward(label, "f32", got, ref, qz, kz, mask, L, w)
    del ref, got, forms[:]
    qkv16, dout16 = qkv.bfloat16(), dout.bfloat16()
    ref = reference(qkv16, dout16, mask, w, p, seed)
    got = run_fused(qkv16, dout16, mask, w, p, seed)
    assert forms == ["mfma", "mfma"]
    check_forward(label, "mfma", got, ref, qz, L, w)
    check_backward(label, "mfma", got, ref, qz, kz, mask, L, w)
    del forms[:]
    gen = run_generic(qkv16, mask, w, p, seed)
    assert forms == ["generic"]
    check_forward(label, "generic", gen, ref, qz, L, w)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_a_masked_key_tile_inside_the_band(cuda, monkeypatch, p):
    """L = 300, w = 100, keys 128 .. 191 of window 0 masked: the query tile 64 .. 127 meets a key tile with no admissible
    key between two that have some (the running maximum stays where it was, alpha = 1)."""
    L, w, H, B = 300, 100, 8, 2
    forms = spy_forms(monkeypatch)
    mask = tile_mask(L, w)
    qz, kz = structural_zero_rows(mask, B, L, w)
    seed = 0x1234567 if p > 0 else 0
    qkv, dout = make_inputs(B, L, H, 77, cuda)
    label = "tile L=300 w=100 H=8 p=%g" % p
    print(label)
    for form, x, dy in (("f32", qkv, dout), ("mfma", qkv.bfloat16(), dout.bfloat16())):
        ref = reference(x, dy, mask, w, p, seed)
        got = run_fused(x, dy, mask, w, p, seed)
        check_forward(label, form, got, ref, qz, L, w)
        check_backward(label, form, got, ref, qz, kz, mask, L, w)
    check_forward(label, "generic", run_generic(qkv.bfloat16(), mask, w, p, seed), ref, qz, L, w)
    assert forms == ["f32", "f32", "mfma", "mfma", "generic"]


def test_generic_form_by_a_misaligned_pointer(cuda, monkeypatch):
    """The other leg of the C side's condition: row strides that are multiples of 8, q / k / v / out 8 bytes off a 16-byte
    boundary.  ops.band_attention would copy such views (ops._row_stride), so cwlt_band_attn_fwd is called directly."""
    B, L, H, w, p, seed = 4, 50, 8, 25, 0.1, 987654321
    forms = spy_forms(monkeypatch)
    mask = combo_mask(L, 5)
    qz, _ = structural_zero_rows(mask, B, L, w)
    qkv, dout = make_inputs(B, L, H, 31, cuda)
    qkv16 = qkv.bfloat16()
    ld = 3 * H * 64
    flat = torch.zeros(B * L * ld + 8, dtype=BF16, device=cuda)
    fused = flat[4:4 + B * L * ld].view(B, L, 3, H, 64)
    fused.copy_(qkv16)
    oflat = torch.zeros(B * L * H * 64 + 8, dtype=BF16, device=cuda)
    out = oflat[4:4 + B * L * H * 64].view(B, L, H * 64)
    q, k, v = fused[:, :, 0], fused[:, :, 1], fused[:, :, 2]
    assert all(t.data_ptr() % 16 == 8 for t in (q, k, v, out)) and ops._row_stride(q) is None
    lse = torch.empty(B, H, L, dtype=F32, device=cuda)
    md = mask.to(cuda)
    ops._call("cwlt_band_attn_fwd", _lib.dev(q), _lib.dev(k), _lib.dev(v), _lib.dev(md), _lib.dev(out), _lib.dev(lse), B, H,
              L, 64, w, ld, ld, ld, H * 64, 0.125, p, seed, None, _lib.CWLT_BF16, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert forms == ["generic"]
    assert (oflat[:4] == 0).all() and (oflat[-4:] == 0).all()            # nothing written outside the view
    ref = reference(qkv16, dout, mask, w, p, seed)
    check_forward("misaligned L=50 w=25 H=8 mask p=0.1", "generic", {"out": out, "lse": lse}, ref, qz, L, w)
    # the same values through the aligned fused buffer take the MFMA form
    del forms[:]
    got = run_fused(qkv16, dout.bfloat16(), mask, w, p, seed)
    assert forms == ["mfma", "mfma"]
    check_forward("misaligned L=50 w=25 H=8 mask p=0.1", "mfma", got, ref, qz, L, w)


def swapped_flags(L):
    """keep_flags with the query and the key index of ((b H + h) L + i) L + j exchanged."""
    def keep(seed, p, idx):
        j, i, bh = idx % L, (idx // L) % L, idx // (L * L)
        return dropout.keep_flags(seed, p, (bh * L + j) * L + i)
    return keep


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_band_attention_teeth(cuda, dtype):
    """The product shape (L = 50, w = 25, H = 8), p = 0.1, combo mask: a reference with a wrong window, a shifted key mask
    or exchanged keep flags misses the kernel's rows (windows 0 and 1, the ones such an ingredient feeds) by at least 5x
    the bound in the rms, forward and backward, while the right reference stays inside it."""
    B, L, H, w, p, seed = 4, 50, 8, 25, 0.1, 0x2F0E1D2C3B4A5968 & ((1 << 62) - 1)
    mask = combo_mask(L, 9)
    qkv, dout = make_inputs(B, L, H, 55, cuda)
    form = "f32"
    if dtype == BF16:
        qkv, dout, form = qkv.bfloat16(), dout.bfloat16(), "mfma"
    got = run_fused(qkv, dout, mask, w, p, seed)
    refs = {"right": reference(qkv, dout, mask, w, p, seed),
            "window + 1": reference(qkv, dout, mask, w + 1, p, seed),
            "key mask shifted by one": reference(qkv, dout, torch.roll(mask, 1, 1), w, p, seed),
            "keep flags with i and j exchanged": reference(qkv, dout, mask, w, p, seed, keep=swapped_flags(L))}
    fb, bb = fwd_bound(form, L, w), bwd_bound(form, L, w)
    print("teeth %s: bounds %.3e forward, %.3e backward" % (form, fb, bb))
    for label, ref in refs.items():
        fed = slice(0, 2)
        ro = rms(row_rel(got["out"].view(B, L, H, 64)[fed], ref["out"].view(B, L, H, 64)[fed], 64))
        rg = [rms(row_rel(got["dqkv"][fed, :, i], ref["dqkv"][fed, :, i], 64)) for i in range(3)]
        print("    %-36s out %.3e (%.1f x bound)  dq %.3e dk %.3e dv %.3e (%.1f x)" % (
            label, ro, ro / fb, rg[0], rg[1], rg[2], min(rg) / bb))
        if label == "right":
            assert ro <= fb and max(rg) <= bb
        else:
            assert ro >= TEETH * fb and min(rg) >= TEETH * bb, (label, ro, rg)


# ----------------------------------------------------------------------------------------------------------------------
# models at repo dims
# ----------------------------------------------------------------------------------------------------------------------
def tokens(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n, (B, L), generator=g) for n in N_CLASS], -1)


def window_mask(B, L, seed):
    """Padded tails in every seventh window, one window padded entirely."""
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(B, L, dtype=torch.long)
    for b in range(0, B, 7):
        m[b, int(torch.randint(1, L, (1,), generator=g)):] = 0
    m[B // 2] = 0
    return m


def set_stats(net):
    bn = net.score_classifier[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.linspace(-0.2, 0.2, 128))
        bn.running_var.copy_(torch.linspace(0.5, 1.5, 128))
    return bn.running_mean.double().clone(), bn.running_var.double().clone()


def airl_net(cuda, dtype):
    from rlmg_amd.dqn_policy import AIRL_model
    net = fill_params(AIRL_model.LongFormer(N_CLASS), seed=5).to(cuda)
    net.compute_dtype = dtype
    assert (AIRL_model.D_MODEL, AIRL_model.N_LAYER, AIRL_model.N_HEAD, net.longformer.one_sided_window) == (512, 10, 8, 25)
    return net


def reward_net(cuda, dtype):
    from rlmg_amd.ppo_policy import model as pmodel
    net = fill_params(pmodel.LongFormer(N_CLASS), seed=6).to(cuda)
    net.compute_dtype = dtype
    assert (net.N_layer, net.N_head, net.longformer.one_sided_window) == (12, 8, 256)
    return net


def params64(net):
    return {k: v.detach().double() for k, v in net.named_parameters()}


def make_jitter(gen, bf16):
    """oracle.disc_f64's jitter: relative errors of rms sqrt(n32) u (and sqrt(n16) U in a bf16 model) on every element."""
    def jitter(t, n32, n16=0):
        sd = (n32 * U32 ** 2 + (n16 * U16 ** 2 if bf16 else 0.0)) ** 0.5
        return t * (1 + sd * torch.randn(t.shape, generator=gen, device=t.device, dtype=t.dtype))
    return jitter


def propagated(fn, h, eps, eps_w, bf16, draws=16, seed=0):
    """The rms change of every element of fn(h, jitter) (a tuple of tensors) under the predicted errors: each row of h
    (.., D) perturbed by independent errors of rms sqrt(eps^2 - eps_w^2) x the row's norm plus h E with one random
    matrix E for all rows, |h_r E| = eps_w |h_r| (weight_eps), every later stage by its own roundings (make_jitter).
    An element's figure is at least its tensor's rms figure."""
    g = torch.Generator(device=h.device).manual_seed(seed)
    D = h.shape[-1]
    base = fn(h, None)
    acc = [torch.zeros_like(b) for b in base]
    scale = (eps ** 2 - eps_w ** 2) ** 0.5 * h.norm(dim=-1, keepdim=True) / D ** 0.5
    jit = make_jitter(g, bf16)

    def randn(*shape):
        return torch.randn(shape, generator=g, device=h.device, dtype=h.dtype)

    for _ in range(draws):
        hp = h + randn(*h.shape) * scale
        if eps_w:
            hp = hp + h @ (randn(D, D) * (eps_w / D ** 0.5))
        out = fn(hp, jit)
        for a, o, b in zip(acc, out, base):
            a += (o - b).square()
    return [torch.maximum((a / draws).sqrt(), (a / draws).mean().sqrt()) for a in acc]


def pooled(h, jit):
    """The window means as the product takes them (f32 sum of L rows)."""
    m = h.mean(1)
    return m if jit is None else jit(m, h.shape[1] / 6 + 1)


def check_hidden(label, got, ref, eps):
    r = row_rel(got, ref, ref.shape[-1])
    worst = note(label + " hidden rows", r.max().item(), 4 * eps)
    assert worst <= 1, (label, r.max().item(), 4 * eps)


def check_elements(label, got, ref, sigma):
    """|got - ref| <= 4 sigma, element by element (sigma from `propagated`)."""
    ratio = ((got.double() - ref).abs() / (4 * sigma)).max().item()
    worst = note(label, ratio, 1.0)
    assert worst <= 1, (label, ratio)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_airl_scoring_matches_the_f64_reference(cuda, monkeypatch, dtype, mode):
    """AIRL, 100 x 50 (one batch_size), the no-grad scoring schedule and the autograd schedule with the same seeds: eval()
    (dropout off, BatchNorm on running statistics) and train() as all_forward forces (dropout on, BatchNorm on batch
    statistics): hidden rows, scores, running statistics; the f32 train case also carries the model-level teeth."""
    B, L, nl, w = 100, 50, 10, 25
    net = airl_net(cuda, dtype)
    x, mask = tokens(B, L, 4).to(cuda), window_mask(B, L, 5).to(cuda)
    train = mode == "train"
    net.train(train)
    p = 0.1 if train else 0.0
    bn = net.score_classifier[1]
    forms = spy_forms(monkeypatch)
    hs = capture_encode(monkeypatch, net)
    runs = {}
    seeds = None
    for sched, ctx in (("scoring", torch.no_grad), ("autograd", torch.enable_grad)):
        stats0 = set_stats(net)
        spy = Seeds(monkeypatch, seeds)
        torch.manual_seed(77)
        with ctx():
            score = net(x, mask)
        torch.cuda.synchronize()
        seeds = spy.seeds
        runs[sched] = (hs.pop(), score.detach(), bn.running_mean.clone(), bn.running_var.clone())
    assert ops._seed_base() is None
    assert len(seeds) == (disc_f64.n_seeds(nl) if train else 0) and len(set(seeds)) == len(seeds)
    assert forms == ["f32" if dtype == F32 else "mfma"] * (2 * nl)       # the model's own calls take the MFMA form
    P = params64(net)
    with torch.no_grad():
        s_ref, stats_ref, h_ref = disc_f64.airl_forward(P, stats0, x, mask, nl, 8, w, train, p, p, seeds or None)
        eps = hidden_eps(dtype, nl, L, w, train)

        def classify(h, jit):
            s, st = disc_f64.score_classifier(P, pooled(h, jit), stats0, train, jitter=jit)
            return s, st[0], st[1]
        sig = propagated(classify, h_ref, eps, weight_eps(dtype, nl), dtype == BF16)
    label = "AIRL 100x50 %s %s" % ("f32" if dtype == F32 else "bf16", mode)
    print(label)
    for sched, (h, score, rm, rv) in runs.items():
        check_hidden("%s %s" % (label, sched), h, h_ref, eps)
        check_elements("%s %s scores / 4 sigma" % (label, sched), score, s_ref, sig[0])
        if train:
            check_elements("%s %s running mean / 4 sigma" % (label, sched), rm, stats_ref[0], sig[1])
            check_elements("%s %s running var / 4 sigma" % (label, sched), rv, stats_ref[1], sig[2])
        else:
            assert torch.equal(rm.double(), stats0[0]) and torch.equal(rv.double(), stats0[1])
    if not (train and dtype == F32):
        return
    bad_seeds = list(seeds)
    bad_seeds[-2] = seeds[-1]
    shifted = torch.roll(mask, 1, 1)
    part = ((mask == 0).any(1) & (mask != 0).any(1))                      # windows with a padded tail
    every = (mask != 0).any(1)
    wrong = [("window + 1", dict(attn_window=w + 1), seeds, every),
             ("key mask shifted by one", dict(attn_mask=shifted), seeds, part),
             ("keep flags with i and j exchanged", dict(keep=swapped_flags(L)), seeds, every),
             ("attention-output dropout of the last layer drawn with its output-dense seed", {}, bad_seeds, every)]
    h = runs["scoring"][0]
    for name, kw, sd, fed in wrong:
        with torch.no_grad():
            hb = disc_f64.hidden(P, x, mask, nl, 8, w, p, p, sd, **kw)
        r = rms(row_rel(h[fed], hb[fed], 512))
        print("    teeth, %s: rows of %d windows miss by %.3e = %.0f x the bound" % (name, int(fed.sum()), r, r / (4 * eps)))
        assert r >= TEETH * 4 * eps, (name, r)


def test_airl_score_in_groups_matches_the_f64_reference(cuda, monkeypatch):
    """calculate_reward's path: 300 windows, bf16, train(), p = 0.1, windows_per_pass 250 (not a multiple of 300: passes of
    200 and 100 windows, each with its own 31 seeds and its own row numbering), the classifier per group of 100: hidden
    rows per pass, scores per group, running statistics after the three groups."""
    n, L, nl, w, p = 300, 50, 10, 25, 0.1
    net = airl_net(cuda, BF16).train()
    x, mask = tokens(n, L, 14).to(cuda), window_mask(n, L, 15).to(cuda)
    stats0 = set_stats(net)
    forms = spy_forms(monkeypatch)
    hs = capture_encode(monkeypatch, net)
    spy = Seeds(monkeypatch)
    torch.manual_seed(78)
    with torch.no_grad():
        score = net.score_in_groups(x, mask, 100, windows_per_pass=250)
    torch.cuda.synchronize()
    assert [h.shape[0] for h in hs] == [200, 100] and len(spy.seeds) == 2 * disc_f64.n_seeds(nl)
    assert forms == ["mfma"] * (2 * nl) and ops._seed_base() is None
    P = params64(net)
    eps = hidden_eps(BF16, nl, L, w, True)
    bn = net.score_classifier[1]

    def classify(h, jit):
        stats, out = stats0, []
        for g0 in range(0, n, 100):
            s, stats = disc_f64.score_classifier(P, pooled(h[g0:g0 + 100], jit), stats, True, jitter=jit)
            out.append(s)
        return torch.cat(out), stats[0], stats[1]

    with torch.no_grad():
        k = disc_f64.n_seeds(nl)
        h_ref = torch.cat([disc_f64.hidden(P, x[s:e], mask[s:e], nl, 8, w, p, p, spy.seeds[i * k:(i + 1) * k])
                           for i, (s, e) in enumerate(((0, 200), (200, 300)))])
        s_ref, rm_ref, rv_ref = classify(h_ref, None)
        sig = propagated(classify, h_ref, eps, weight_eps(BF16, nl), True)
    label = "AIRL score_in_groups 300x50 bf16 train"
    print(label)
    check_hidden(label + " pass 0", hs[0], h_ref[:200], eps)
    check_hidden(label + " pass 1", hs[1], h_ref[200:], eps)
    for g0 in range(0, n, 100):
        check_elements("%s scores of group %d / 4 sigma" % (label, g0 // 100), score[g0:g0 + 100], s_ref[g0:g0 + 100],
                       sig[0][g0:g0 + 100])
    check_elements(label + " running mean / 4 sigma", bn.running_mean, rm_ref, sig[1])
    check_elements(label + " running var / 4 sigma", bn.running_var, rv_ref, sig[2])
    assert int(bn.num_batches_tracked) == 3


UNUSED = ("word_embeddings", "_global", "pooler")


def backward_terms(terms, P):
    """Back-propagates the loss terms one after the other -> (total gradients, name -> sqrt(sum over terms |g_term|^2)): the
    norm a gradient would have if the terms' contributions did not cancel (the expert and the agent BCE pull the score
    classifier in opposite directions: at a score of one half their gradients cancel to a hundredth)."""
    sq = {k: 0.0 for k in P}
    prev = {k: None for k in P}
    for i, t in enumerate(terms):
        t.backward(retain_graph=i + 1 < len(terms))
        for k, q in P.items():
            if q.grad is None:
                continue
            d = q.grad if prev[k] is None else q.grad - prev[k]
            sq[k] += d.square().sum().item()
            prev[k] = q.grad.clone()
    return {k: q.grad for k, q in P.items()}, {k: v ** 0.5 for k, v in sq.items()}


def check_grads(label, net, ref_params, ref_grads, term_unc, taps, ztaps, n_layer, bound, unused=UNUSED):
    """Every parameter gradient against the f64 one, relative to max(|ref|, what |ref| would be without cancellation, the
    project's floor); named unused parameters have no gradient; the floor decides no tensor."""
    got = {k: v.grad for k, v in net.named_parameters()}
    none = sorted(k for k in got if got[k] is None)
    assert none == sorted(k for k in ref_grads if ref_grads[k] is None), label
    assert none == sorted(k for k in got if any(u in k for u in unused)), none
    names = [k for k in got if got[k] is not None]
    assert all(got[k].dtype == F32 and torch.isfinite(got[k]).all() for k in names)
    norms = {k: ref_grads[k].norm().item() for k in names}
    floor = 1e-4 * (sum(v ** 2 for v in norms.values()) / len(names)) ** 0.5
    unc = {k: term_unc[k] for k in names}
    sums = [[0.0] * 4 for _ in range(n_layer)]
    for i, (x2, q, k) in enumerate(taps):                          # the passes' taps follow each other, layer by layer
        t = disc_f64.row_terms(x2, q) + disc_f64.row_terms(x2, k)
        sums[i % n_layer] = [a + b for a, b in zip(sums[i % n_layer], t)]
    rows = {}
    for i, sm in enumerate(sums):
        pre = "longformer.encoder.layer.%d.attention.self." % i
        rows[pre + "query.bias"], rows[pre + "query.weight"] = sm[0] ** 0.5, sm[1] ** 0.5
        rows[pre + "key.bias"], rows[pre + "key.weight"] = sm[2] ** 0.5, sm[3] ** 0.5
    if ztaps:
        zt = [disc_f64.classifier_row_terms(m, zn, sg, ref_params["score_classifier.1.weight"]) for m, zn, sg in ztaps]
        for i, k in enumerate(("score_classifier.0.bias", "score_classifier.0.weight", "score_classifier.1.weight")):
            rows[k] = sum(t[i] for t in zt) ** 0.5
    assert all(k in norms for k in rows)
    for k, v in rows.items():
        unc[k] = max(unc[k], v)
    below = sorted(k for k in names if max(norms[k], unc[k]) < floor)
    assert below == [], (below, floor)
    r = {k: (got[k].double() - ref_grads[k]).norm().item() / max(norms[k], unc[k]) for k in names}
    order = sorted(r, key=r.get, reverse=True)
    for k in order[:8]:
        print("    %-72s %.3e  |ref| %.3e uncancelled %.3e" % (k, r[k], norms[k], unc[k]))
    kb = max(r[k] for k in rows if k.endswith("key.bias"))
    print("    key biases (zero in exact arithmetic): worst %.3e of the uncancelled row sum" % kb)
    note(label + " gradients (worst tensor %s)" % order[0].replace("longformer.encoder.", ""), r[order[0]], bound)
    assert r[order[0]] <= bound, (label, order[0], r[order[0]], bound)
    return got


def check_position_rows(got, L):
    pos = got["longformer.embeddings.position_embeddings.weight"]
    assert (pos[:2] == 0).all() and (pos[L + 2:] == 0).all() and (pos[2:L + 2] != 0).any()
    assert (got["longformer.embeddings.token_type_embeddings.weight"][1] == 0).all()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_airl_training_loss_matches_the_f64_reference(cuda, monkeypatch, dtype):
    """One batch of RewardDiscri.update_disc's training branch (dqn_policy/AIRL.py:113-128) at 100 x 50, train(), p = 0.1:
    expert score, token CE, agent score -- three passes, 93 seeds, BatchNorm on batch statistics twice -- then the backward
    of e + (a + ce): the three losses, the running statistics and the gradient of every parameter."""
    from rlmg_amd.dqn_policy import AIRL
    B, L, nl, w, p = 100, 50, 10, 25, 0.1
    rd = AIRL.RewardDiscri(N_CLASS, Pretrain=False)
    net = fill_params(rd.disc_model, seed=5)
    net.compute_dtype = dtype
    st_exp, st_ag = tokens(B, L, 24).to(cuda), tokens(B, L, 25).to(cuda)
    mask = window_mask(B, L, 26).to(cuda)
    stats0 = set_stats(net)
    forms = spy_forms(monkeypatch)
    spy = Seeds(monkeypatch)
    torch.manual_seed(79)
    for q in net.parameters():
        q.grad = None
    e = rd.BCE_criterion(rd.all_forward(st_exp, None, None, mask, mask), torch.ones(B, 1, device=cuda))
    ce = net.token_forward(st_ag, st_exp, mask)
    a = rd.BCE_criterion(rd.all_forward(st_ag, None, None, mask, mask), torch.zeros(B, 1, device=cuda))
    (e + (a + ce)).backward()
    torch.cuda.synchronize()
    k = disc_f64.n_seeds(nl)
    assert net.training and len(spy.seeds) == 3 * k and len(set(spy.seeds)) == 3 * k and ops._seed_base() is None
    assert forms == ["f32" if dtype == F32 else "mfma"] * (3 * nl)
    P = disc_f64.leaves(dict(net.named_parameters()))
    taps, ztaps = [], []
    (re, ra, rc), stats = disc_f64.airl_train_loss(P, stats0, st_exp, st_ag, mask, nl, 8, w, p, p,
                                                   [spy.seeds[i * k:(i + 1) * k] for i in range(3)], taps=taps, ztap=ztaps)
    ref_grads, term_unc = backward_terms([re, ra, rc], P)
    label = "AIRL training loss 100x50 %s" % ("f32" if dtype == F32 else "bf16")
    print(label)
    eps = hidden_eps(dtype, nl, L, w, True)
    lref = torch.stack([re, ra, rc]).detach()
    lgot = torch.stack([e, a, ce]).detach().double()
    print("    losses got %s ref %s" % (lgot.tolist(), lref.tolist()))
    bn = net.score_classifier[1]
    with torch.no_grad():
        # losses and running statistics after the two scored batches, through the reference's own sensitivity to the
        # hidden rows of the three passes
        hh = torch.cat([disc_f64.hidden(P, d, mask, nl, 8, w, p, p, spy.seeds[i * k:(i + 1) * k])
                        for i, d in enumerate((st_exp, st_ag, st_ag))])

        def losses(h, jit):
            ls, st = disc_f64.airl_losses(P, stats0, h[:B], h[B:2 * B], h[2 * B:], st_exp, jitter=jit,
                                          pool=lambda t: pooled(t, jit))
            return ls[0], ls[1], ls[2], st[0], st[1]
        sig = propagated(losses, hh, eps, weight_eps(dtype, nl), dtype == BF16)
    for i, name in enumerate(("expert BCE", "agent BCE", "token CE")):
        check_elements("%s %s / 4 sigma" % (label, name), lgot[i], lref[i], sig[i])
    check_elements(label + " running mean / 4 sigma", bn.running_mean, stats[0], sig[3])
    check_elements(label + " running var / 4 sigma", bn.running_var, stats[1], sig[4])
    got = check_grads(label, net, P, ref_grads, term_unc, taps, ztaps, nl, grad_bound(dtype, nl, L, w))
    check_position_rows(got, L)


@pytest.mark.parametrize("B,L", [(4, 1024), (64, 50)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_reward_model_token_forward_matches_the_f64_reference(cuda, monkeypatch, dtype, B, L):
    """The PPO reward model (512 / 12 / 8, one-sided window 256), eval(), no-grad, at the bench's length and at the RL
    loop's: hidden rows and rewards."""
    nl, w = 12, 256
    net = reward_net(cuda, dtype).eval()
    x, mask = tokens(B, L, 34).to(cuda), window_mask(B, L, 35).to(cuda)
    forms = spy_forms(monkeypatch)
    hs = capture_encode(monkeypatch, net)
    spy = Seeds(monkeypatch)
    with torch.no_grad():
        reward = net.token_forward(x, None, mask)
    torch.cuda.synchronize()
    assert spy.seeds == [] and forms == ["f32" if dtype == F32 else "mfma"] * nl
    P = params64(net)
    eps = hidden_eps(dtype, nl, L, w, False)
    with torch.no_grad():
        r_ref, h_ref = disc_f64.ppo_token_forward(P, x, mask, nl, 8, w, slab=1 if L > 300 else None)
        sig = propagated(lambda h, jit: (disc_f64.ppo_reward(P, h, jit),), h_ref, eps, weight_eps(dtype, nl), dtype == BF16)
    label = "reward model %dx%d %s eval" % (B, L, "f32" if dtype == F32 else "bf16")
    print(label)
    check_hidden(label, hs[0], h_ref, eps)
    check_elements(label + " rewards / 4 sigma", reward, r_ref, sig[0])


def test_reward_model_train_step_matches_the_f64_reference(cuda, monkeypatch):
    """ppo_policy/model.LongFormer.train_step, 8 x 50, bf16, train(), p = 0.1, autograd: the six losses and every gradient of
    their mean."""
    B, L, nl, w, p = 8, 50, 12, 256, 0.1
    net = reward_net(cuda, BF16).train()
    x, y = tokens(B, L, 44).to(cuda), tokens(B, L, 45).to(cuda)
    mask = window_mask(B, L, 46).to(cuda)
    forms = spy_forms(monkeypatch)
    spy = Seeds(monkeypatch)
    torch.manual_seed(80)
    losses = net.train_step(x, y, mask)
    (sum(losses) / 6).backward()
    torch.cuda.synchronize()
    assert len(spy.seeds) == disc_f64.n_seeds(nl) and forms == ["mfma"] * nl and ops._seed_base() is None
    P = disc_f64.leaves(dict(net.named_parameters()))
    taps = []
    lref = disc_f64.ppo_train_step(P, x, y, mask, nl, 8, w, p, p, spy.seeds, taps=taps)
    ref_grads, term_unc = backward_terms([lref.mean()], P)
    label = "reward model train_step 8x50 bf16"
    print(label)
    eps = hidden_eps(BF16, nl, L, w, True)
    lgot = torch.stack([l.detach() for l in losses]).double()
    print("    losses got %s ref %s" % (lgot.tolist(), lref.tolist()))
    with torch.no_grad():
        h_ref = disc_f64.hidden(P, x, mask, nl, 8, w, p, p, spy.seeds)
        sig = propagated(lambda h, jit: (disc_f64.token_ce(P, h, y, jit),), h_ref, eps, weight_eps(BF16, nl), True)
    check_elements(label + " losses / 4 sigma", lgot, lref.detach(), sig[0])
    got = check_grads(label, net, P, ref_grads, term_unc, taps, None, nl, grad_bound(BF16, nl, L, w),
                      unused=UNUSED + ("eval_",))
    check_position_rows(got, L)

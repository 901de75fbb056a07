"""GPU: every f32 generation path at repo dims (d_model 512, 12 layers, 8 heads) against the f64 reference of the
recurrent form (oracle/decode_f64.py), teacher-forced with random tokens, row by row, and the decode state at the end.

Models: dqn_policy.model.LinearTransformer(is_training=False), fill_params(seed=5), as filled ("x1") and with every
layer's query and key projection weights times 10 ("x10": phi(q), phi(k) spread over both branches of elu + 1 and the
normaliser varies from row to row; as filled the features sit near phi(0) = 1 and attention is close to a running mean of
v); ppo_policy.model.Actor_Transformer(is_training=False) in the GEMV case.  The reference runs in f64 on the GPU (plain
torch ops, none of the project's kernels); test_reference_on_the_gpu_equals_the_cpu pins that against the CPU.

Cases (each spies on the entry points and asserts the path it names, so that a default flipping cannot turn two cases
into one):
    1  GEMV step (cwlt_decode_step), graph replay, one song, 4 096 steps
    2  module path (fused=False: ops.recurrent_cla_step per layer), graph on and off, 512 steps
    3  GEMM step (cwlt_decode_step_rows), graph replay, 1 / 63 / 64 / 65 / 257 songs with their own tokens, 64 steps
    4  prefill of one 4 096-token prompt, blas and gemm, every row's logits (logits="all"), the returned row, the state,
       then 8 steps from that state
    5  prefill of a ragged batch, lengths 1 31 32 33 63 64 65 1 000 1 024 (chunk 32), blas and gemm, 1 000 rows per GEMM
       call (a song straddles two calls), one-song blocks and the default; the returned rows, the state (a padding row
       must not reach it), then 8 steps on the GEMV and on the GEMM step
    6  score_songs, gemm and blas, samplers "categorical" and "dqn", 8 songs of ragged length up to 1 024

Measure.  Per row, relative to the row's own norm: |got - ref|_2 / |ref|_2 over a row's 339 logits, the same for a hidden
row; S and Z relative to the norm of that (song, layer, head).  No absolute tolerance anywhere.

Bound (oracle.decode_f64.row_bound, state_bound), derived as tests/test_model_gpu.py::BF16_GRAD_REL is, with u = 2^-24:
every f32 operation between the token and a logit rounds its result with a relative error of at most u.  One post-LN
layer puts 10 of them in a row's way: the Q/K/V projection (a dot product of 512), phi, the state update, the read-out
(dot products of 64 and the division by the normaliser), the out-projection with bias and residual (512), LayerNorm 1
(statistics, rsqrt, scale and shift), linear1 (512), GELU, linear2 with residual (2 048), LayerNorm 2.  A LayerNorm
renormalises the row, so a relative error passes through a layer with gain about one and the layers' errors add up
rather than multiply.  Around the layers: the embedding scale, in_linear (1 216), pe[0], the final norm, the heads (512):
5.  n = 10 * 12 + 5 = 125 independent errors of size u add in quadrature to sqrt(125) u = 6.7e-7 of a row's norm; the
tests allow 4x that, as the existing bounds do:
        ROW = 4 * sqrt(125) * 2^-24 = 2.67e-6      (logit rows and hidden rows; it does not depend on the row index)
State, layer l (from 0), after t tokens: S = sum phi(k_s) v_s^T is added up one token at a time.  Add number s rounds a
partial sum of s terms; for terms of random sign the partial sum is sqrt(s) terms large and the roundings (rms u / sqrt(3)
each) add to u sqrt(t / 6) of the sum's norm, for terms of one sign (Z) to u sqrt(t) / 3; the larger is taken.  k and v
carry the n_l roundings made before them, independent from token to token, so in a sum of t terms they count
sqrt(2 n_l / t) u; the product rounds once.  n_l = 14 + 10 l: the l layers before, the projection, and the front counted
as heavily as a layer.  (The count first tried, 4 + 10 l with the front as 3, under-predicts the REFERENCE's own f32
error where nothing else hides it, layer 0 after one token: the CPU f32 chain has a median error of 5.8 u (x1) and 7.2 u
(x10) over 512 (song, head) pairs, worst 8 u and 10 u, where that count predicts sqrt(2 * 4 + 1) u = 3 u.  The front is a
1 216-long dot product feeding a 512-long one with no LayerNorm between them to renormalise; counted as 10 the
prediction is sqrt(2 * 14 + 1) u = 5.4 u, which is what the reference shows.  Under the first count the hipBLASLt
prefill measured 1.12 (x10) and 0.91 (x1) of the bound in that one place -- S of layer 0 of the one-token song, 13.5 u --
while every song of more than one token stayed below 0.45 in every case; the project's own GEMM prefill has 5 u there.)
        STATE(t, l) = 4 * sqrt(t / 6 + 2 (14 + 10 l) / t + 1) * 2^-24      (9.4e-7 at t = 64, 3.1e-6 at 1 024, 6.2e-6 at 4 096)
Both are checked against a measurement of the REFERENCE, not of the kernels: tests/test_oracle_decode_cpu.py evaluates
the same chain in torch f32 on the CPU (state summed token by token) and asserts that each bound lies between that floor
and 8x it (the kernels' sum orders differ from torch's: DPP wave reductions, the MFMA k permutation, split-K partials,
32-token chunks; that changes constants, not orders of magnitude).  Floor: rows 6.0e-7 .. 7.7e-7 worst (median 5.1e-7)
for both weight sets, L = 1 .. 4 096: ROW is 3.5 .. 4.5x it.  State 1.4e-7 .. 2.3e-7 at t = 64, 5.0e-7 .. 8.0e-7 at
1 024, 1.0e-6 .. 1.4e-6 at 4 096; per layer, over t = 1 .. 1 024, STATE is 2.0 .. 6.5x it (asserted there).
Log-probs are differences of a row's logits: the model log-prob takes the absolute bound 2 * ROW * |row|_2, the sampler
log-prob that divided by the attribute's temperature.

Nucleus pairs left out of the sampler comparison ("dqn" only; the model log-prob is compared on every pair): the kept
set is a step function of the logits, so a (row, attribute) pair is skipped if and only if, in the f64 reference, some
class's rank-ahead mass is within 1e-5 of top_p in logprobs_f64's units, or the last kept and the first dropped class
tie within 1e-6 in probability and the target is one of the two (nucleus_unstable; narrower than skipping every tie).
Counted on the CPU from the f64 logits before any GPU run, token seed 21, lengths SCORE_LENS: 40 of 23 508 pairs
(0.17 %) for x1, 41 (0.17 %) for x10, most of them in the 135-class chord attribute at top_p 0.99, where the ranked
masses lie 4e-3 apart; the test asserts at most 0.5 %.

Teeth (cases 1, 3, 5): the reference built with one wrong ingredient must miss the kernels' result by at least 5x the
bound on every row that ingredient feeds: pe[t] for pe[0] (every row after the first); tanh-form GELU (every row); the
token at index 32 left out of the state (rows 33 to 1 024 of songs that long); song n reading song n + 1's state in the
last layer (all songs but the last; cases 3 and 5, case 1 has one song); Z from raw k, weight set x10 (every row).
None had to be dropped: the weakest, the GELU, is 28x the bound away.

Measured on an MI355X (worst ratio to the bound per case): profiles/decode_f64_ratios.txt, DESIGN section 5.
"""
import collections
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402
from rlmg_amd.sampling import logprobs_f64  # noqa: E402
from oracle import decode_f64  # noqa: E402

pytestmark = pytest.mark.gpu
N_CLASS = [56, 135, 18, 87, 18, 25]
OFF = np.concatenate([[0], np.cumsum(N_CLASS)])
ROW = decode_f64.row_bound(12)
TEETH = 5.0
RAGGED = [1, 31, 32, 33, 63, 64, 65, 1000, 1024]
SCORE_LENS = [1024, 1000, 777, 513, 512, 65, 33, 2]
SCORE_SEED = 21
SKIP_CAP = 0.005
_MODELS, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    """The models and the f64 references (a few GB on the GPU) are shared by the cases of this module only."""
    yield
    _MODELS.clear()
    _REFS.clear()
    torch.cuda.empty_cache()


def _net(cuda, kind="dqn", scale=1):
    """The model of a case, built once per (class, weight set): repo dims, f32, eval."""
    if (kind, scale) not in _MODELS:
        if kind == "dqn":
            from rlmg_amd.dqn_policy import model
            net = model.LinearTransformer(N_CLASS, is_training=False)
        else:
            from rlmg_amd.ppo_policy import model
            net = model.Actor_Transformer(N_CLASS, is_training=False)
        net = fill_params(net, seed=5)
        if scale != 1:
            with torch.no_grad():
                for layer in net.transformer_encoder.layers:
                    layer.attention.query_projection.weight.mul_(scale)
                    layer.attention.key_projection.weight.mul_(scale)
        net = net.to(cuda).eval()
        assert net.d_model == 512 and net.n_layer == 12 and net.n_head == 8 and net.compute_dtype == torch.float32
        _MODELS[kind, scale] = net
    return _MODELS[kind, scale]


def _tokens(n, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, c, (n, L), generator=g) for c in N_CLASS], -1)


def _ref(net, key, tok, lengths=None, wrong=None):
    """(logits, hidden, state) of the f64 reference on the GPU, kept per (model, tokens' key, lengths, wrong)."""
    key = (id(net), key, None if lengths is None else tuple(lengths), wrong)
    if key not in _REFS:
        _REFS[key] = decode_f64.decode_f64(net.state_dict(), tok, N_CLASS, 12, 8, lengths, wrong=wrong,
                                           device=next(net.parameters()).device)
    return _REFS[key]


class Spy:
    """Counts the entry points that tell the paths apart: the fused step by the library entry its plan calls, the module
    path's attention step, the scan with state (and its `segments`), the GEMM and GEMV building blocks."""

    def __init__(self, monkeypatch):
        self.calls = collections.Counter()
        self.segments = []
        real_step = generation._FusedPlan.step

        def step(plan, tok):
            self.calls[plan.entry] += 1
            return real_step(plan, tok)

        monkeypatch.setattr(generation._FusedPlan, "step", step)
        for name in ("recurrent_cla_step", "decode_gemm", "decode_gemv", "score_categorical"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        real_scan = ops.cla_fwd_state

        def scan(*a, **kw):
            self.calls["cla_fwd_state"] += 1
            self.segments.append(kw.get("segments"))
            return real_scan(*a, **kw)

        monkeypatch.setattr(ops, "cla_fwd_state", scan)

    def _wrap(self, name, real):
        def f(*a, **kw):
            self.calls[name] += 1
            return real(*a, **kw)
        return f

    def clear(self):
        self.calls.clear()
        del self.segments[:]


def _run(sess, tok):
    """Teacher-forced steps: tok (n_songs, T, 6) -> logits (n_songs, T, 339) f32, hidden (n_songs, T, 512) f32 (CPU)."""
    n, T = tok.shape[:2]
    toks = tok.numpy()
    logits = np.empty((n, T, sess.width), dtype=np.float32)
    hidden = torch.empty((T, n, sess.model.d_model), dtype=torch.float32, device=sess.dev)
    for t in range(T):
        logits[:, t] = np.asarray(sess.step(toks[:, t])).reshape(n, -1)
        hidden[t] = sess.hidden.view(n, -1)
    return torch.from_numpy(logits), hidden.permute(1, 0, 2).cpu()


def _rows(label, got, ref):
    """Worst |got - ref| / |ref| over the rows, as a ratio to ROW; printed and asserted.  got, ref: (..., width)."""
    r = decode_f64.row_rel(got, ref)
    assert torch.isfinite(r).all(), label
    worst = r.max().item()
    print("%-64s worst row %.3g = %.2f of the bound, median %.3g" % (label, worst, worst / ROW, r.median().item()))
    assert worst < ROW, (label, worst, ROW)
    return worst / ROW


def _state(label, memory, ref, lens):
    """Every layer's S and Z against the reference, each (song, head) relative to its own norm, as a ratio to
    state_bound(tokens of the song)."""
    worst, where = 0.0, ""
    for i, ((S, Z), (Sr, Zr)) in enumerate(zip(memory, ref)):
        bound = torch.tensor([decode_f64.state_bound(t, i) for t in lens], dtype=torch.float64)[:, None]
        for name, got, want in (("S", S, Sr), ("Z", Z, Zr)):
            r = decode_f64.state_rel(got, want) / bound
            assert torch.isfinite(r).all(), (label, i)
            if r.max().item() > 0.7:
                print("    %s of layer %d: ratio per song %s" % (name, i, " ".join("%.2f" % x for x in r.amax(1))))
            if r.max().item() > worst:
                worst, where = r.max().item(), "%s of layer %d, %d tokens" % (name, i, lens[int(r.amax(1).argmax())])
    print("%-64s worst state %.2f of the bound (%s)" % (label, worst, where))
    assert worst < 1.0, (label, worst)
    return worst


def _tooth(label, got, wrong_ref):
    """The kernels' rows against a reference with one wrong ingredient: every row at least TEETH x the bound away."""
    r = decode_f64.row_rel(got, wrong_ref)
    print("    tooth %-24s nearest row %.3g = %.1f x the bound" % (label, r.min().item(), r.min().item() / ROW))
    assert r.min().item() >= TEETH * ROW, (label, r.min().item())


# ---- the reference itself, where it runs ----------------------------------------------------------------------------
def test_reference_on_the_gpu_equals_the_cpu(cuda):
    net = _net(cuda, "dqn", 10)
    tok = _tokens(2, 300, 1)
    lens = [300, 77]
    P = {k: v.cpu() for k, v in net.state_dict().items()}
    a = decode_f64.decode_f64(P, tok, N_CLASS, 12, 8, lens)
    b = decode_f64.decode_f64(net.state_dict(), tok, N_CLASS, 12, 8, lens, device=cuda)
    assert b[0].is_cuda and b[0].dtype == torch.float64
    worst = max(decode_f64.row_rel(b[0], a[0]).max().item(), decode_f64.row_rel(b[1], a[1]).max().item())
    for (S, Z), (Sc, Zc) in zip(b[2], a[2]):
        worst = max(worst, decode_f64.state_rel(S, Sc).max().item(), decode_f64.state_rel(Z, Zc).max().item())
    print("f64 reference, GPU against CPU: worst relative difference %.3g" % worst)
    assert worst < 1e-12


# ---- 1. the GEMV step, full length ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,scale", [("dqn", 1), ("dqn", 10), ("ppo", 1)])
def test_gemv_step_4096(cuda, monkeypatch, kind, scale):
    spy = Spy(monkeypatch)
    net = _net(cuda, kind, scale)
    T = 4096
    tok = _tokens(1, T, 2)
    sess = generation.DecodeSession(net, graph=True)
    logits, hidden = _run(sess, tok)
    assert sess.fused and sess.use_graph and sess._graph is not None and sess.n_steps == T
    assert set(spy.calls) == {"cwlt_decode_step"}, spy.calls
    lg, h, st = _ref(net, "gemv", tok)
    label = "1 gemv step %s x%d" % (kind, scale)
    _rows(label + " logits", logits, lg)
    _rows(label + " logits, rows 3584 .. 4095", logits[:, 3584:], lg[:, 3584:])
    _rows(label + " hidden", hidden, h)
    _state(label, sess.memory, st, [T])
    if kind == "dqn":
        wrongs = ("pe_t", "gelu_tanh", "drop32") + (("z_raw",) if scale == 10 else ())
        for wrong in wrongs:
            lw = _ref(net, "gemv", tok, wrong=wrong)[0]
            sl = {"pe_t": slice(1, None), "drop32": slice(33, 1025)}.get(wrong, slice(None))
            _tooth(wrong, logits[:, sl], lw[:, sl])


# ---- 2. the module path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("scale", [1, 10])
def test_module_path_512(cuda, monkeypatch, graph, scale):
    spy = Spy(monkeypatch)
    net = _net(cuda, "dqn", scale)
    T = 512
    tok = _tokens(1, T, 3)
    sess = generation.DecodeSession(net, graph=graph, fused=False)
    logits, hidden = _run(sess, tok)
    assert not sess.fused and sess.use_graph == graph and (sess._graph is not None) == graph
    assert spy.calls["recurrent_cla_step"] >= 12 and not spy.calls["cwlt_decode_step"] \
        and not spy.calls["cwlt_decode_step_rows"], spy.calls
    if not graph:
        assert spy.calls["recurrent_cla_step"] == 12 * T
    lg, h, st = _ref(net, "module", tok)
    label = "2 module path x%d graph=%s" % (scale, graph)
    _rows(label + " logits", logits, lg)
    _rows(label + " hidden", hidden, h)
    _state(label, sess.memory, st, [T])


# ---- 3. the GEMM step across tile edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_songs", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("scale", [1, 10])
def test_gemm_step_across_tiles(cuda, monkeypatch, n_songs, scale):
    spy = Spy(monkeypatch)
    net = _net(cuda, "dqn", scale)
    T = 64
    tok = _tokens(257, T, 4)[:n_songs]                       # every song its own tokens; the first n of one draw
    sess = generation.DecodeSession(net, graph=True, n_songs=n_songs, kernel="gemm")
    logits, hidden = _run(sess, tok)
    assert sess.use_graph and sess._graph is not None and set(spy.calls) == {"cwlt_decode_step_rows"}, spy.calls
    lg, h, st = _ref(net, "gemm", _tokens(257, T, 4))
    label = "3 gemm step x%d, %d songs" % (scale, n_songs)
    _rows(label + " logits", logits, lg[:n_songs])
    _rows(label + " hidden", hidden, h[:n_songs])
    _state(label, sess.memory, [[S[:n_songs], Z[:n_songs]] for S, Z in st], [T] * n_songs)
    if n_songs == 65:
        for wrong in ("pe_t", "gelu_tanh", "drop32", "song_stride") + (("z_raw",) if scale == 10 else ()):
            lw = _ref(net, "gemm65", tok, wrong=wrong)[0]
            if wrong == "song_stride":
                _tooth(wrong, logits[:-1], lw[:-1])
            else:
                sl = {"pe_t": slice(1, None), "drop32": slice(33, None)}.get(wrong, slice(None))
                _tooth(wrong, logits[:, sl], lw[:, sl])


# ---- 4. prefill, one long prompt ----------------------------------------------------------------------------------------
def _assert_prefill_path(spy, kernel):
    assert spy.calls["cla_fwd_state"] >= 12, spy.calls
    if kernel == "gemm":
        assert spy.calls["decode_gemm"] > 0 and set(spy.segments) == {1}, (spy.calls, spy.segments)
    else:
        assert not spy.calls["decode_gemm"] and set(spy.segments) == {None}, (spy.calls, spy.segments)


@pytest.mark.parametrize("kernel", ["blas", "gemm"])
@pytest.mark.parametrize("scale", [1, 10])
def test_prefill_one_prompt_4096(cuda, monkeypatch, kernel, scale):
    spy = Spy(monkeypatch)
    net = _net(cuda, "dqn", scale)
    P, more = 4096, 8
    tok = _tokens(1, P + more, 5)
    lg, h, st = _ref(net, "prefill1", tok, [P])
    label = "4 prefill %s x%d, 4096 tokens" % (kernel, scale)
    # every row's logits, on a scratch state
    scratch = generation.DecodeSession(net, graph=False)
    every = net.prefill_hidden(tok[:, :P].to(cuda), scratch.memory, None, kernel=kernel, logits="all")
    _assert_prefill_path(spy, kernel)
    _rows(label + " logits of every row", every.cpu(), lg[:, :P])
    _state(label + " (all rows)", scratch.memory, st, [P])
    # the session's prefill: the returned row, its hidden row, the state; then 8 steps from it
    spy.clear()
    sess = generation.DecodeSession(net, graph=True)
    row = sess.prefill(tok[0, :P].numpy(), kernel=kernel)
    _assert_prefill_path(spy, kernel)
    assert not spy.calls["cwlt_decode_step"]
    _rows(label + " returned row", torch.from_numpy(row.copy())[None], lg[:, P - 1])
    _rows(label + " returned hidden", sess.hidden.cpu(), h[:, P - 1])
    _state(label, sess.memory, st, [P])
    logits, hidden = _run(sess, tok[:, P:])
    assert spy.calls["cwlt_decode_step"] > 0
    _rows(label + " + 8 steps logits", logits, lg[:, P:])
    _rows(label + " + 8 steps hidden", hidden, h[:, P:])
    _state(label + " + 8 steps", sess.memory, _ref(net, "prefill1", tok)[2], [P + more])


# ---- 5. prefill, ragged batch at the chunk edges ------------------------------------------------------------------------
def _ragged(seed):
    """Songs of RAGGED lengths + 8 continuation tokens each -> (songs (9, 1032, 6): song n is its first RAGGED[n] + 8
    rows; prompt (9, 1024, 6): the songs' prompts, rows past a song's length filled with other tokens)."""
    n, P = len(RAGGED), max(RAGGED)
    songs = _tokens(n, P + 8, seed)
    prompt = _tokens(n, P, seed + 1)
    for i, ln in enumerate(RAGGED):
        prompt[i, :ln] = songs[i, :ln]
    return songs, prompt


@pytest.mark.parametrize("step_kernel", ["gemv", "gemm"])
@pytest.mark.parametrize("kernel,how", [("blas", "default"), ("gemm", "default"), ("gemm", "rows1000"),
                                        ("gemm", "blocks1000")])
@pytest.mark.parametrize("scale", [1, 10])
def test_prefill_ragged_batch(cuda, monkeypatch, kernel, how, step_kernel, scale):
    spy = Spy(monkeypatch)
    net = _net(cuda, "dqn", scale)
    songs, prompt = _ragged(7)
    n, more = len(RAGGED), 8
    idx = torch.arange(n)
    after = [ln + more for ln in RAGGED]
    lg, h, st = _ref(net, "ragged", songs, RAGGED)
    st2 = _ref(net, "ragged", songs, after)[2]
    label = "5 prefill %s/%s x%d, %s steps" % (kernel, how, scale, step_kernel)
    sess = generation.DecodeSession(net, graph=True, n_songs=n, kernel=step_kernel)
    if how == "rows1000":           # 1 000 rows per GEMM call over the 9 216 token rows: songs straddle two calls
        hid, row = net.prefill_hidden(prompt.to(cuda), sess.memory, RAGGED, kernel="gemm", logits=True, rows=1000)
        row, hid = row.cpu(), hid.cpu()
        assert spy.calls["decode_gemm"] >= 10 * (1 + 4 * 12)
    else:
        row = sess.prefill(prompt.numpy(), lengths=RAGGED, kernel=kernel,
                           prefill_rows=1000 if how == "blocks1000" else None)
        row, hid = torch.from_numpy(row.copy()), sess.hidden.cpu()
        assert spy.calls["cla_fwd_state"] == (12 * n if how == "blocks1000" else 12), spy.calls
    _assert_prefill_path(spy, kernel)
    assert not spy.calls["cwlt_decode_step"] and not spy.calls["cwlt_decode_step_rows"]
    last = torch.tensor(RAGGED) - 1
    _rows(label + " returned rows", row, lg[idx, last])
    _rows(label + " returned hidden", hid, h[idx, last])
    _state(label, sess.memory, st, RAGGED)
    cont = torch.stack([songs[i, ln:ln + more] for i, ln in enumerate(RAGGED)])
    logits, hidden = _run(sess, cont)
    entry = "cwlt_decode_step_rows" if step_kernel == "gemm" else "cwlt_decode_step"
    assert spy.calls[entry] > 0 and not spy.calls["cwlt_decode_step" if step_kernel == "gemm" else "cwlt_decode_step_rows"]
    want = torch.stack([lg[i, ln:ln + more] for i, ln in enumerate(RAGGED)])
    _rows(label + " + 8 steps logits", logits, want)
    _rows(label + " + 8 steps hidden", hidden, torch.stack([h[i, ln:ln + more] for i, ln in enumerate(RAGGED)]))
    _state(label + " + 8 steps", sess.memory, st2, after)
    if how == "default":
        got = torch.cat([row[:, None], logits], 1)                       # song n: rows RAGGED[n] - 1 .. RAGGED[n] + 7
        for wrong in ("pe_t", "gelu_tanh", "drop32", "song_stride") + (("z_raw",) if scale == 10 else ()):
            lw = _ref(net, "ragged", songs, RAGGED, wrong=wrong)[0]
            lw = torch.stack([lw[i, ln - 1:ln + more] for i, ln in enumerate(RAGGED)])
            if wrong == "pe_t":                                          # the 1-token song's first row is row 0
                _tooth(wrong, torch.cat([got[:1, 1:], got[1:].flatten(0, 1)[None]], 1), torch.cat(
                    [lw[:1, 1:], lw[1:].flatten(0, 1)[None]], 1))
            elif wrong == "drop32":                                      # songs longer than 33: every row shown is fed
                keep = [i for i, ln in enumerate(RAGGED) if ln > 33]
                _tooth(wrong, got[keep], lw[keep])
                keep = [i for i, ln in enumerate(RAGGED) if ln <= 32]   # and a song that never had a token 32 is not
                assert decode_f64.row_rel(got[keep][:, :1], lw[keep][:, :1]).max().item() < ROW
            elif wrong == "song_stride":
                _tooth(wrong, got[:-1], lw[:-1])
            else:
                _tooth(wrong, got, lw)


# ---- 6. scoring -----------------------------------------------------------------------------------------------------------
def _word2event():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    return w2e


def nucleus_unstable(x, target, temperature, top_p):
    """x (rows, n) f64 logits of one attribute, target (rows,) classes -> (rows,) bool: the pair's sampler log-prob could
    jump under an f32-sized change.  Some class's rank-ahead mass (logprobs_f64's units: / (sum + 1e-5 sum)) within 1e-5
    of top_p (it flips in or out of the kept set, which moves every kept class's log-prob), or the last kept and the
    first dropped class within 1e-6 in probability and the target one of the two (they may swap)."""
    if top_p is None or top_p >= 1.0:
        return np.zeros(len(x), dtype=bool)
    v = x / temperature
    e = np.exp(v - v.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    order = np.argsort(-p, axis=1, kind="stable")
    r = np.arange(len(x))
    ps = p[r[:, None], order]
    ahead = (np.cumsum(ps, 1) - ps) / (1.0 + 1e-5)
    near = (np.abs(ahead - top_p) < 1e-5).any(1)
    first = (ahead <= top_p).sum(1)                         # sorted index of the first dropped class (n: none)
    j = np.minimum(first, p.shape[1] - 1)
    tie = (first < p.shape[1]) & (np.abs(ps[r, j - 1] - ps[r, j]) < 1e-6) \
        & ((order[r, j - 1] == target) | (order[r, j] == target))
    return near | tie


def _score_reference(net, songs, sampler):
    """Per song (L - 1, 6, 2) f64 [model, sampler] log-probs from the f64 logits through sampling.logprobs_f64, the
    (L - 1, 6) skip flags and each row's norm."""
    key = (id(net), "score", sampler)
    if key in _REFS:
        return _REFS[key]
    L = max(len(s) for s in songs)
    tok = torch.zeros((len(songs), L, 6), dtype=torch.int64)
    for i, s in enumerate(songs):
        tok[i, :len(s)] = torch.from_numpy(s)
    lg = _ref(net, "score", tok, [len(s) for s in songs])[0].cpu().numpy()
    temps, tops = (generation.DQN_TEMPERATURE, generation.DQN_TOP_P) if sampler == "dqn" else ((1.0,) * 6, (None,) * 6)
    out = []
    for i, s in enumerate(songs):
        x = lg[i, :len(s) - 1]
        want = np.empty((len(s) - 1, 6, 2))
        skip = np.zeros((len(s) - 1, 6), dtype=bool)
        for a in range(6):
            xa = x[:, OFF[a]:OFF[a + 1]]
            skip[:, a] = nucleus_unstable(xa, s[1:, a], temps[a], tops[a])
            for t in range(len(s) - 1):
                want[t, a] = logprobs_f64(xa[t], s[t + 1, a], temps[a], tops[a])
        out.append((want, skip, np.linalg.norm(x, axis=1)))
    _REFS[key] = out
    return out


def _score_songs():
    tok = _tokens(len(SCORE_LENS), max(SCORE_LENS), SCORE_SEED).numpy()
    return [tok[i, :ln] for i, ln in enumerate(SCORE_LENS)]


@pytest.mark.parametrize("kernel", ["gemm", "blas"])
@pytest.mark.parametrize("sampler", ["categorical", "dqn"])
@pytest.mark.parametrize("scale", [1, 10])
def test_score_songs(cuda, monkeypatch, kernel, sampler, scale):
    spy = Spy(monkeypatch)
    net = _net(cuda, "dqn", scale)
    songs = _score_songs()
    got = generation.score_songs(net, _word2event(), songs, sampler=sampler, kernel=kernel)
    _assert_prefill_path(spy, kernel)
    assert spy.calls["score_categorical"] == 1 and not spy.calls["cwlt_decode_step"]
    temps = generation.DQN_TEMPERATURE if sampler == "dqn" else (1.0,) * 6
    worst_m = worst_s = 0.0
    pairs = skipped = 0
    for g, (want, skip, norm) in zip(got, _score_reference(net, songs, sampler)):
        assert g.shape == want.shape
        g = g.astype(np.float64)
        bound = 2 * ROW * norm[:, None]
        assert np.isfinite(want[..., 0]).all() and want[..., 0].min() > np.log(1e-12)
        worst_m = max(worst_m, (np.abs(g[..., 0] - want[..., 0]) / bound).max())
        pairs += skip.size
        skipped += int(skip.sum())
        fin = np.isfinite(want[..., 1])
        assert (np.isfinite(g[..., 1]) == fin)[~skip].all(), "kept set differs away from a nucleus boundary"
        use = fin & ~skip & np.isfinite(g[..., 1])
        d = np.abs(np.where(use, g[..., 1] - want[..., 1], 0.0)) / (bound / np.asarray(temps)[None, :])
        worst_s = max(worst_s, d.max())
    print("%-64s model log-prob %.2f of the bound, sampler log-prob %.2f; %d of %d pairs skipped (%.2f %%)"
          % ("6 score_songs %s %s x%d" % (kernel, sampler, scale), worst_m, worst_s, skipped, pairs,
             100.0 * skipped / pairs))
    assert skipped <= SKIP_CAP * pairs, (skipped, pairs)
    if sampler == "categorical":
        assert skipped == 0
    assert worst_m < 1.0 and worst_s < 1.0, (worst_m, worst_s)

"""Token-by-token generation on the recurrent form of the encoder.

Surface of the reference's generation scripts (dqn_policy/testing-no-type-cp.py:126-223,
dqn_policy/agent_pretrain.py:636-706, ppo_policy/inference.py:78-160):
    res = inference_from_scratch(model, word2event, bar_cond)      # (n_tokens, 6) int64 numpy
    generate(model, word2event, ...)                               # songs + runtime_stats.json
`model` is a `LinearTransformer` / `Actor_Transformer` built with `is_training=False`.

`DecodeSession` is the device side of one song: the 12 x [S (1,H,64,64), Zs (1,H,64)] state lives in HBM
and is updated in place, the CW token is written into a static (1,1,6) buffer, and the whole per-token
step (embedding gather -> in_linear -> 12 recurrent layers -> final LN -> fused 6-head GEMV) is ONE
hipGraph replay of `cwlt_decode_step` (csrc/decode.hip: GEMVs with LayerNorm prologues and bias / GELU /
residual epilogues, 63 launches per token); the only host traffic per token is 48 B of ids in and
sum(n_token) f32 logits out.
Sampling stays on the host with numpy, in the reference's order of draws, so that a seeded
`np.random` reproduces the reference's token stream.
"""
import ctypes
import json
import math
import os
import time

import numpy as np
import torch

from . import ops
from .draw_plan import (DQN_TEMPERATURE, DQN_TOP_P, Constraint, DeviceDraw, DrawPlan, Grammar,  # noqa: F401
                        Preference, check_entry, compile_alpha, compile_constraints, compile_grammar,
                        compile_preferences)
from .metrics import METRICS, MetricReward, SongMetricSpec, song_metrics  # noqa: F401
from .sampling import logmeanexp, sample_cw

INIT_CW = np.array([[0, 0, 1, 0, 0, 0]])          # "Bar" token, testing-no-type-cp.py:135-137
PREFILL_ROWS = 32768        # default token-row budget of one gemm prefill block (prompts x the block's longest prompt)


def cut_prompt(song, word2event, prompt_bars):
    """The first `prompt_bars` bars of a CW token song (T, 6): the rows before the Bar token that opens bar
    prompt_bars + 1, by the generation bar rule (the count starts at 1 and counts the Bar tokens after the first row).
    A song with fewer bars is returned whole.  -> (P, 6) int64."""
    song = np.asarray(song, dtype=np.int64).reshape(-1, len(word2event))
    if int(prompt_bars) < 1:
        raise ValueError("prompt_bars must be >= 1, got %r" % (prompt_bars,))
    names = word2event["bar-beat"]
    cnt = 1 + np.cumsum([names[int(r[2])] == "Bar" for r in song[1:]])
    past = np.nonzero(cnt > int(prompt_bars))[0]
    return song if len(past) == 0 else song[:past[0] + 1]


def dataset_prompts(x, word2event, prompt_bars, n_songs, mask=None):
    """One prompt per song from dataset songs x (n_seq, T, 6) (mask (n_seq, T): rows > 0 are the song's own, the
    rest padding): song i continues the first `prompt_bars` bars of dataset song i % n_seq (cut_prompt)."""
    x = np.asarray(x)
    if len(x) == 0:
        raise ValueError("no dataset songs to take prompts from")
    out = []
    for i in range(int(n_songs)):
        s = x[i % len(x)]
        if mask is not None:
            s = s[:int((np.asarray(mask[i % len(x)]) > 0).sum())]
        p = cut_prompt(s, word2event, prompt_bars)
        if len(p) == 0:
            raise ValueError("dataset song %d is empty" % (i % len(x)))
        out.append(p)
    return out


def stream_bank_plan(prompt_lengths, slots, prefill_rows=None, bank=None, entry_bytes=0, free_bytes=None):
    """Block size B and bank entries of generate_stream(prompts=...) -> (B, bank).
    B = prefill_rows // the longest prompt (at least 1, at most n_songs): every block's prefill stays within the row
    budget.  bank (None): the smallest multiple of B that holds max(2 B, 2 slots) entries -- slots never wait for a
    prefill while a second batch of songs is queued -- at most the songs rounded up to whole blocks, and at most a
    quarter of free_bytes at entry_bytes per entry (never below two blocks).  A given bank must be a multiple of B (B is
    lowered to bank when bank < B)."""
    lens = [int(n) for n in prompt_lengths]
    n = len(lens)
    if n < 1 or min(lens) < 1:
        raise ValueError("stream_bank_plan needs at least one prompt, each of at least one row")
    rows = PREFILL_ROWS if prefill_rows is None else int(prefill_rows)
    if rows < 1:
        raise ValueError("prefill_rows must be >= 1, got %d" % rows)
    B = max(1, min(n, rows // max(lens)))
    blocks = -(-n // B)
    if bank is not None:
        bank = int(bank)
        if bank < 1:
            raise ValueError("bank must be >= 1, got %d" % bank)
        B = min(B, bank)
        if bank % B:
            raise ValueError("bank (%d) must be a multiple of the prefill block (%d songs)" % (bank, B))
        return B, bank
    nb = max(2, -(-2 * int(slots) // B))
    if free_bytes is not None and entry_bytes > 0:
        nb = min(nb, max(2, int(free_bytes) // 4 // (int(entry_bytes) * B)))
    return B, min(nb, blocks) * B


def packed_blocks(lengths, prefill_rows=None, max_songs=None):
    """Blocks of the packed prefill -> [(a, z), ...]: consecutive whole songs [a, z), taken greedily while the block's
    summed rows stay within prefill_rows (default PREFILL_ROWS) and it holds at most max_songs songs (None: no cap); a
    song longer than the budget is a block of its own."""
    rows = PREFILL_ROWS if prefill_rows is None else int(prefill_rows)
    if rows < 1:
        raise ValueError("prefill_rows must be >= 1, got %d" % rows)
    if max_songs is not None and int(max_songs) < 1:
        raise ValueError("max_songs must be >= 1, got %d" % max_songs)
    lens = [int(n) for n in lengths]
    out, a, used = [], 0, 0
    for i, n in enumerate(lens):
        if n < 1:
            raise ValueError("song %d is empty: a packed block holds songs of at least one row" % i)
        if i > a and (used + n > rows or (max_songs is not None and i - a >= int(max_songs))):
            out.append((a, i))
            a, used = i, 0
        used += n
    if lens:
        out.append((a, len(lens)))
    return out


def _pack_rows(arrays, dev=None):
    """Songs laid end to end: a list of (L_i, A) int64 arrays -> ((R, A) array, its ops.SeqOffsets on `dev`)."""
    cu = np.concatenate([[0], np.cumsum([len(x) for x in arrays])])
    return np.concatenate(arrays), ops.SeqOffsets(cu.tolist(), device=dev)


def bank_may_prefill(j, B, bank, assigned):
    """Reuse rule of the bank: block j (songs [j B, (j + 1) B), entries [(j % nb) B, ...) with nb = bank // B) may be
    written once the block that held those entries before it, j - nb, has all its songs assigned to slots (`assigned`:
    the device's assigned counter, as copied back one chunk behind)."""
    nb = bank // B
    return j < nb or int(assigned) >= (j - nb + 1) * B


class _FusedPlan:
    """Host description of the model for `cwlt_decode_step` (include/cwlt.h: cwlt_decode_model): stacked
    QKV / head weights, device pointers of every parameter, the per-song state and workspace.  Holds references
    to every tensor whose pointer it hands out.  Built once per song (`DecodeSession.reset` rebuilds it, so
    weights loaded between songs are picked up).  kernel="gemm": the step is `cwlt_decode_step_rows`
    (csrc/decode_gemm.hip), whose workspace also holds its GEMMs' split-K scratch."""

    def __init__(self, model, memory, n_songs, kernel="gemv"):
        from . import _lib
        lib = _lib.load()
        enc = model.transformer_encoder
        f32 = lambda t: t.detach().float().contiguous()
        self.keep = []
        self.packed = []           # (buffer, source tensors): row-stacked copies, re-filled in place by refresh()

        def P(t):
            t = f32(t)             # an f32 contiguous parameter is used in place: optimizer steps are seen directly
            self.keep.append(t)
            return _lib.dev(t).value

        def PACK(ts):
            buf = torch.cat([f32(t) for t in ts], 0)
            self.packed.append((buf, list(ts)))
            return _lib.dev(buf).value

        layers = (_lib.DecodeLayer * len(enc.layers))()
        for i, (L, (S, Z)) in enumerate(zip(enc.layers, memory)):
            at = L.attention
            d = layers[i]
            d.wqkv = PACK([at.query_projection.weight, at.key_projection.weight, at.value_projection.weight])
            d.bqkv = PACK([at.query_projection.bias, at.key_projection.bias, at.value_projection.bias])
            d.wo, d.bo = P(at.out_projection.weight), P(at.out_projection.bias)
            d.ln1_w, d.ln1_b = P(L.norm1.weight), P(L.norm1.bias)
            d.w1, d.b1 = P(L.linear1.weight), P(L.linear1.bias)
            d.w2, d.b2 = P(L.linear2.weight), P(L.linear2.bias)
            d.ln2_w, d.ln2_b = P(L.norm2.weight), P(L.norm2.bias)
            d.S, d.Z = _lib.dev(S).value, _lib.dev(Z).value
            for nrm in (L.norm1, L.norm2):
                if abs(nrm.eps - enc.layers[0].norm1.eps) > 0:
                    raise RuntimeError("decode step needs one LayerNorm eps for the whole encoder")
        tables = model._tables()
        heads = model._heads()
        m = _lib.DecodeModel()
        m.n_layer, m.n_head = len(enc.layers), enc.layers[0].attention.n_heads
        m.d_model, m.d_ff = model.d_model, enc.layers[0].linear1.out_features
        m.n_attr, m.emb_width = len(tables), sum(t.shape[1] for t in tables)
        m.n_logits = sum(h.out_features for h in heads)
        m.eps_ln, m.eps_attn = enc.layers[0].norm1.eps, ops.CLA_EPS
        self._tables = (ctypes.c_void_p * len(tables))(*[P(t) for t in tables])
        self._widths = _lib.int_array([t.shape[1] for t in tables])
        self._nrows = _lib.int_array([t.shape[0] for t in tables])
        m.tables = ctypes.cast(self._tables, ctypes.POINTER(ctypes.c_void_p))
        m.widths = ctypes.cast(self._widths, ctypes.POINTER(ctypes.c_int))
        m.nrows = ctypes.cast(self._nrows, ctypes.POINTER(ctypes.c_int))
        m.w_in, m.b_in = P(model.in_linear.weight), P(model.in_linear.bias)
        m.pe0 = P(model.pos_emb.pe[0, 0])
        self._layers = layers
        m.layers = ctypes.cast(layers, ctypes.POINTER(_lib.DecodeLayer))
        if enc.norm is not None:
            if enc.norm.eps != enc.layers[0].norm1.eps:
                raise RuntimeError("decode step needs one LayerNorm eps for the whole encoder")
            m.lnf_w, m.lnf_b = P(enc.norm.weight), P(enc.norm.bias)
        m.w_heads = PACK([h.weight for h in heads])
        m.b_heads = PACK([h.bias for h in heads])
        self.model = m
        per_song = lib.cwlt_decode_workspace_floats(ctypes.byref(m))
        if per_song <= 0:
            raise RuntimeError("cwlt_decode_step does not support this model shape (d_model %d, d_ff %d)"
                               % (m.d_model, m.d_ff))
        floats = n_songs * per_song
        if kernel == "gemm":
            floats = lib.cwlt_decode_rows_workspace_floats(ctypes.byref(m), n_songs)
            if floats <= 0:
                raise RuntimeError("cwlt_decode_step_rows does not support this model shape or batch (d_model %d, "
                                   "d_ff %d, %d songs)" % (m.d_model, m.d_ff, n_songs))
        self.entry = "cwlt_decode_step_rows" if kernel == "gemm" else "cwlt_decode_step"
        dev = memory[0][0].device
        self.work = torch.zeros(floats, dtype=torch.float32, device=dev)
        self.hidden = torch.zeros((n_songs, m.d_model), dtype=torch.float32, device=dev)
        self.logits = torch.zeros((n_songs, m.n_logits), dtype=torch.float32, device=dev)
        self.n_songs = n_songs

    def refresh(self):
        """Re-fill the row-stacked copies from the parameters, in place (pointers, and a captured graph, stay valid)."""
        with torch.no_grad():
            for buf, srcs in self.packed:
                torch.cat([t.detach().float() for t in srcs], 0, out=buf)

    def step(self, tok):
        from . import _lib
        st = getattr(_lib.load(), self.entry)(ctypes.byref(self.model), _lib.dev(tok), _lib.dev(self.work),
                                              _lib.dev(self.hidden), _lib.dev(self.logits), self.n_songs,
                                              _lib.stream_ptr())
        _lib.check(st, self.entry)
        return self.logits


class DecodeSession:
    """Decode state of `n_songs` songs + the captured one-token step.
    `step(ids) -> (sum n_token,) f32 numpy logits` (or (n_songs, sum n_token) when n_songs > 1).

    fused=True (default for f32 models): the step is `cwlt_decode_step` (csrc/decode.hip, 5 launches per layer);
    fused=False: the layer-by-layer module path (recurrent.py), the only one for bf16 activations.
    kernel="gemm" (fused f32 only): the step is `cwlt_decode_step_rows` (csrc/decode_gemm.hip), its projections f32
    MFMA GEMMs that read each weight once per 64 songs -- the step for many songs in lock-step; "gemv" (default):
    `cwlt_decode_step`, one weight stream per song."""

    def __init__(self, model, graph=None, fused=None, n_songs=1, kernel="gemv"):
        if not getattr(model, "_recurrent", False):
            raise RuntimeError("generation needs a model built with is_training=False (recurrent encoder)")
        p = next(model.parameters())
        if not p.is_cuda:
            raise RuntimeError("rlmg_amd models run on the GPU only (no CPU fallback): call .cuda() first")
        self.model, self.dev = model, p.device
        self.n_token = list(model.n_token)
        self.width = sum(self.n_token)
        self.n_songs = int(n_songs)
        if fused is None:
            fused = model.compute_dtype == torch.float32
        if fused and model.compute_dtype != torch.float32:
            raise RuntimeError("the fused decode step computes in f32; use fused=False for bf16 activations")
        if not fused and self.n_songs != 1:
            raise RuntimeError("the module-by-module decode path generates one song at a time (as the reference)")
        if kernel not in ("gemv", "gemm"):
            raise ValueError("kernel must be 'gemv' or 'gemm', got %r" % (kernel,))
        if kernel == "gemm" and not fused:
            raise RuntimeError("the GEMM decode step is the fused f32 step: it needs fused=True and f32 activations")
        self.fused = bool(fused)
        self.kernel = kernel
        enc = model.transformer_encoder
        H = enc.layers[0].attention.n_heads
        d = model.d_model // H
        n, A = self.n_songs, len(self.n_token)
        self.tok = torch.zeros((n, 1, A), dtype=torch.int64, device=self.dev)
        per = n * H * d * (d + 1)                           # all layers' [S, Zs] in ONE buffer: reset = one memset
        self._state = torch.zeros(per * len(enc.layers), dtype=torch.float32, device=self.dev)
        self.memory = [[self._state[i * per:i * per + n * H * d * d].view(n, H, d, d),
                        self._state[i * per + n * H * d * d:(i + 1) * per].view(n, H, d)]
                       for i in range(len(enc.layers))]
        # _state's layout as the refill and gather kernels take it: layers, one song's S floats (H x d x d), Z (H x d)
        self.n_layer = len(self.memory)
        self.s_floats, self.z_floats = self.memory[0][0][0].numel(), self.memory[0][1][0].numel()
        self._host_tok =torch.zeros((n, 1, A), dtype=torch.int64).pin_memory()
        self._host_logits = torch.zeros((n, self.width), dtype=torch.float32).pin_memory()
        self.use_graph = ops.GRAPHS_ENABLED if graph is None else bool(graph)
        self._graph, self._out, self._plan = None, None, None
        self.census = None                                    # node kinds of the captured step (ops.capture_hip_graph)
        self.hidden = None                                  # (n_songs, d_model) device tensor after a step
        self.n_steps = 0

    def _weights_tag(self):
        return tuple(p.data_ptr() for p in self.model.parameters())

    def reset(self):
        """Start new songs: zero the state and bring the step's weights up to date.  Unstacked f32 parameters are
        read in place; the row-stacked copies (Q/K/V, heads) are re-filled in place -- unconditionally: version
        counters do not see fused optimizers -- so the captured graph stays valid.  Only parameters that moved to
        other storage (.to(), load_state_dict(assign=True)) force a rebuild."""
        self._state.zero_()
        if self.fused and self._plan is not None:
            if self._plan.tag != self._weights_tag():
                self._plan, self._graph = None, None
            else:
                self._plan.refresh()
        self.n_steps = 0

    def _fused_plan(self):
        if self._plan is None:
            with torch.no_grad():
                self._plan = _FusedPlan(self.model, self.memory, self.n_songs, self.kernel)
            self._plan.tag = self._weights_tag()
        return self._plan

    def _device_step(self):
        """testing-no-type-cp.py:150 / :166 (`forward_hidden(input_, memory, is_training=False)`) followed by the six
        head projections of forward_output_sampling (dqn_policy/model.py:273-278) as one fused GEMV."""
        if self.fused:
            out = self._fused_plan().step(self.tok)
            self.hidden = self._plan.hidden
            return out
        h, mem = self.model.forward_hidden(self.tok, self.memory, is_training=False)
        for (S, Z), (S2, Z2) in zip(self.memory, mem):
            if S2.data_ptr() != S.data_ptr() or Z2.data_ptr() != Z.data_ptr():
                raise RuntimeError("recurrent state must be updated in place")
        self.hidden = h
        return self.model.fused_logits(h).float()[:, :self.width].contiguous()

    def _capture(self):
        saved = self._state.clone()
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                self._device_step()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        torch.cuda.synchronize(self.dev)
        # ops.capture_hip_graph: memset nodes (none in cwlt_decode_step; the module path's torch ops may add some) are
        # rewritten as kernels before the graph is instantiated; a capture that cannot be made safe is not replayed
        g, out, self.census, _ = ops.capture_hip_graph(self._device_step, torch.no_grad, "decode step")
        self._state.copy_(saved)                              # warm-up ran the step: restore
        if g is None:
            self.use_graph = False
        self._graph, self._out = g, out

    def step(self, ids):
        """Feed one CW token per song (6 ids each), advance the state, return the next-token logits (host numpy)."""
        if self.model.training:
            raise RuntimeError("generation runs in eval() mode (agent_pretrain.py:657)")
        self._host_tok.view(-1).copy_(torch.as_tensor(np.asarray(ids, dtype=np.int64).reshape(-1)))
        self.tok.copy_(self._host_tok, non_blocking=True)
        if self.use_graph:
            if self._graph is None:
                self._capture()
        if self.use_graph:
            self._graph.replay()
            out = self._out
        else:
            with torch.no_grad():
                out = self._device_step()
        self._host_logits.copy_(out, non_blocking=True)
        torch.cuda.current_stream(self.dev).synchronize()
        self.n_steps += 1
        res = self._host_logits.numpy()
        return res[0] if self.n_songs == 1 else res

    def _prefill(self, tokens, lengths=None, kernel="blas", prefill_rows=None):
        """prefill() without the host copy: -> (n_songs, sum n_token) f32 device logits."""
        if kernel not in ("blas", "gemm", "packed"):
            raise ValueError("kernel must be 'blas' or 'gemm' (or 'packed'), got %r" % (kernel,))
        if self.model.training:
            raise RuntimeError("generation runs in eval() mode (agent_pretrain.py:657)")
        if self.model.compute_dtype != torch.float32:
            raise RuntimeError("prefill computes in f32: this session's model runs %s activations (step() one token "
                               "at a time instead)" % self.model.compute_dtype)
        if kernel == "packed" and lengths is None and isinstance(tokens, (list, tuple)) and \
                len(tokens) > 0 and all(np.ndim(t) == 2 for t in tokens):
            # the packed form's own input: one (P_i, A) array per song
            arrays = [np.asarray(t, dtype=np.int64).reshape(-1, len(self.n_token)) for t in tokens]
            if any(len(t) == 0 for t in arrays):
                raise ValueError("the packed prefill takes prompts of at least one row each")
            lengths = [len(t) for t in arrays]
            tokens = np.zeros((len(arrays), max(lengths), len(self.n_token)), dtype=np.int64)
            for i, t in enumerate(arrays):
                tokens[i, :len(t)] = t
        toks = np.asarray(tokens, dtype=np.int64)
        if toks.ndim == 2:
            toks = toks[None]
        A = len(self.n_token)
        if toks.ndim != 3 or toks.shape[0] != self.n_songs or toks.shape[2] != A or toks.shape[1] == 0:
            raise ValueError("prompt tokens must be (P, %d) or (n_songs=%d, P, %d) with P >= 1, got %s"
                             % (A, self.n_songs, A, np.shape(tokens)))
        P = toks.shape[1]
        lens = np.full(self.n_songs, P) if lengths is None else np.asarray(lengths, dtype=np.int64).reshape(-1)
        if lens.shape != (self.n_songs,) or (lens < 1).any() or (lens > P).any():
            raise ValueError("prompt lengths must be %d values in [1, %d], got %s" % (self.n_songs, P, list(lens)))
        for i, n in enumerate(lens):
            bad = (toks[i, :n] < 0) | (toks[i, :n] >= np.asarray(self.n_token))
            if bad.any():
                t, a = np.argwhere(bad)[0]
                raise ValueError("prompt %d, token %d: id %d out of range for attribute %d (%d classes)"
                                 % (i, t, toks[i, t, a], a, self.n_token[a]))
        heads = self.model._heads()
        with torch.no_grad():
            if kernel == "gemm":
                # batch invariant: blocks of whole songs under the row budget give the bits of one call
                per = max(1, (PREFILL_ROWS if prefill_rows is None else int(prefill_rows)) // P)
                h = torch.empty((self.n_songs, self.model.d_model), dtype=torch.float32, device=self.dev)
                logits = torch.empty((self.n_songs, self.width), dtype=torch.float32, device=self.dev)
                for a in range(0, self.n_songs, per):
                    z = min(self.n_songs, a + per)
                    Pb = int(lens[a:z].max())
                    h[a:z], logits[a:z] = self.model.prefill_hidden(
                        torch.as_tensor(toks[a:z, :Pb]).to(self.dev), [[S[a:z], Z[a:z]] for S, Z in self.memory],
                        lens[a:z], kernel="gemm", logits=True)
            elif kernel == "packed":
                # the same bits without the padded rows: blocks of whole songs by their summed rows
                h = torch.empty((self.n_songs, self.model.d_model), dtype=torch.float32, device=self.dev)
                logits = torch.empty((self.n_songs, self.width), dtype=torch.float32, device=self.dev)
                for a, z in packed_blocks(lens, prefill_rows):
                    rows, cu = _pack_rows([toks[i, :lens[i]] for i in range(a, z)], self.dev)
                    h[a:z], logits[a:z] = self.model.prefill_hidden_packed(
                        torch.as_tensor(rows).to(self.dev), cu, [[S[a:z], Z[a:z]] for S, Z in self.memory])
            else:
                h = self.model.prefill_hidden(torch.as_tensor(toks).to(self.dev), self.memory,
                                              None if lengths is None else lens)
                # h already carries the final norm: the stacked heads are a plain GEMV (no LayerNorm prologue)
                logits = ops.decode_gemv(torch.cat([m.weight.float() for m in heads], 0),
                                         torch.cat([m.bias.float() for m in heads], 0), h)
        if self.fused:
            hid = self._fused_plan().hidden
            hid.copy_(h)
            self.hidden = hid
        elif self._graph is not None:
            self.hidden.copy_(h)            # the captured step's output buffer: every later replay refreshes it
        else:
            self.hidden = h
        self.n_steps += int(lens.max())
        return logits

    def prefill(self, tokens, lengths=None, kernel="blas", prefill_rows=None):
        """Feed a whole prompt in one parallel pass per layer: leaves the state exactly as feeding the prompt's
        tokens through step() one by one would (within f32 rounding), starting from whatever state the session holds
        (reset(), earlier steps or an earlier prefill), and returns what the last of those step() calls would: the
        next-token logits (host numpy) and `hidden`.  tokens: (P, 6) for one song, (n_songs, P, 6) for several;
        ragged prompts pass `lengths` (n_songs values in [1, P]; rows past a song's length are ignored).  The state is
        updated in the session's own buffers, so a captured step graph stays valid.  f32 sessions in eval() mode.
        n_steps advances by the longest prompt: with ragged prompts song i has then been fed
        n_steps - (max(lengths) - lengths[i]) tokens in total.

        kernel="blas" (default): the projections on hipBLASLt.  kernel="gemm": the batch-invariant prefill
        (CWTrunk.prefill_hidden(kernel="gemm"), every projection a cwlt_decode_gemm): song i's state, hidden row and
        logits are bitwise the same whatever the other prompts, their lengths and order; songs go through in blocks of
        at most prefill_rows // P (default PREFILL_ROWS) prompts, which changes no bits.  kernel="packed": the same
        bits without the padded rows (CWTrunk.prefill_hidden_packed): the prompts are laid end to end, in blocks of whole
        songs of at most prefill_rows summed rows (packed_blocks); tokens may then also be a list of n_songs (P_i, 6)
        arrays in place of a padded array with lengths."""
        out = self._prefill(tokens, lengths, kernel, prefill_rows)
        self._host_logits.copy_(out, non_blocking=True)
        torch.cuda.current_stream(self.dev).synchronize()
        res = self._host_logits.numpy()
        return res[0] if self.n_songs == 1 else res

    def shadow(self, model):
        """The second decode state of a blended loop: a GEMM-step session of `model` (the blend's reference; None: none)
        with this session's rows, stepping on the token buffer this session's sampler writes.  Takes no seed."""
        if model is None:
            return None
        ref = DecodeSession(model, n_songs=self.n_songs, kernel="gemm")
        ref.tok = self.tok
        ref.reset()
        return ref

    def split(self, logits):
        outs, o = [], 0
        for n in self.n_token:
            outs.append(logits[..., o:o + n])
            o += n
        return outs


def _draw_token(plan, logits, n_token, tok, seed, counter=None, key=None, step=None, bar=None, beat=None, logp=None,
                out_counter=None, song=None):
    """One token's draw for every row of logits into tok (rows, A), by the one rule of both loops, from `plan`
    (DeviceDraw): under a grammar (at positions `beat`) cwlt_sample_categorical_grammar, else with a log-prob ring `logp`
    (row *out_counter) ..._logp, else with a constraint table (at bar counts `bar`) ..._masked, else the plain draw.
    Keyed per row by key / step (the stream: song index, position in song), or by the row's slot at `counter` (the
    batch loop, whose plain draw also writes row *counter of `song`)."""
    kw = dict(counter=counter, key=key, step=step, **plan.keywords(bar))
    if plan.order is not None:
        ops.sample_categorical_grammar(logits, n_token, tok, seed, *plan.grammar(beat), logp=logp,
                                       out_counter=None if logp is None else out_counter, **kw)
    elif logp is not None:
        ops.sample_categorical_logp(logits, n_token, tok, seed, logp, out_counter=out_counter, **kw)
    elif plan.sched is not None:
        ops.sample_categorical_masked(logits, n_token, tok, seed, **kw)
    elif key is not None:
        ops.sample_categorical_keyed(logits, n_token, tok, seed, key, step, **plan.keywords())
    else:
        ops.sample_categorical(logits, n_token, tok, seed, counter=counter, song=song, slot_keys=True,
                               **plan.keywords())


def _prefer_token(plan, logits, n_token, seen=None, key=None, bar=None):
    """The preferred logits of one token or block of rows, written over `logits` (cwlt_prefer_logits): the
    bias rows of `plan` (DeviceDraw) at bar counts `bar`, its penalties at the states `seen`, row n of song key[n]
    (None: n).  A plan without preferences launches nothing."""
    if plan.pen is None:
        return logits
    return ops.prefer_logits(logits, n_token, sched=plan.psched, bias=plan.bias, pen=plan.pen, seen=seen, key=key,
                             bar=None if plan.bias is None else bar, out=logits)


def _enqueue_token(loop, name):
    """Enqueue one more token of `loop` (its _one; call under torch.no_grad()): eager for the first two tokens and when
    graphs are off; at the third, after a device synchronize, _one is captured as one hipGraph -- recorded, not
    executed -- and replayed from then on.  A capture that cannot be replayed leaves the loop eager."""
    if loop.use_graph and loop.enqueued >= 2 and loop._graph is None:
        torch.cuda.synchronize(loop.sess.dev)
        loop._graph = ops.capture_hip_graph(loop._one, torch.no_grad, name)[0]
        loop.use_graph = loop._graph is not None
    if loop.use_graph and loop.enqueued >= 2:
        loop._graph.replay()
    else:
        loop._one()
    loop.enqueued += 1


class _DeviceLoop:
    """Generation loop that never returns to the host: per token the decode step, ONE sampling kernel
    (csrc/sample.hip) that writes the drawn ids of every song into the step's token buffer and into row `count` of
    `song` (capacity, n_songs, 6), and the counter increment -- eager for the first two tokens, then one captured
    hipGraph replayed per token.

    ring=R: `song` holds only the last R rows (row t of the stream in slot t % R) so that many songs with a large cap
    do not need capacity x n_songs rows; read each R-row stretch before the next R tokens overwrite it.  The draws are
    the same either way (they are keyed by the counter).

    plan (DeviceDraw; None: the plain draw at temperature 1) says what the draw is (_draw_token); the loop keeps what
    moves.  With a constraint table `bar`, (n_songs,) int64 bar counts before the next row, from plan.bar0s:
    cwlt_count_bars advances them after the draw.  plan.logprobs: the draw also writes each drawn class's (model,
    sampler) log-probs into `logp` (rows, n_songs, 6, 2) f32 beside `song`, at the row `count` selects.  With a grammar
    `beat`, each song's position, from plan.beat0: cwlt_grammar_track moves it after cwlt_count_bars.  plan.ref,
    plan.alpha (the blend): `ref` (DecodeSession.shadow) steps on the same token buffer right after the
    model and cwlt_blend_logits (alpha's row n is song n) turns the model's logits into the blend's in place.
    Preferences: cwlt_prefer_logits then turns the logits into the preferred ones in place, before the
    unchanged draw; `seen` (n_songs, sum n_class) f32, each song's repetition state from plan.seen0, is moved by
    cwlt_prefer_track after the draw (only when some song has a penalty), and `bar` is kept, and cwlt_count_bars
    launched, also when only a bias schedule needs the count -- which does not select the masked sampler."""

    def __init__(self, sess, capacity, plan=None, carry_memory=True, graph=None, ring=None):
        self.sess, self.capacity, self.carry = sess, int(capacity), carry_memory
        self.plan = plan = DeviceDraw() if plan is None else plan
        self.ref, self.bar, self.bar_mask = plan.ref, None, None
        self.seen = None if plan.seen0 is None else plan.seen0.clone()
        if plan.sched is not None or plan.bias_bars:
            self.bar = torch.as_tensor(np.asarray(plan.bar0s, dtype=np.int64)).to(sess.dev)
            self.bar_mask = torch.as_tensor(plan.bar_mask).to(sess.dev)
        self.beat = None if plan.order is None else plan.beat0.clone()          # one song per row, in song order
        self.A, self.N = len(sess.n_token), sess.n_songs
        self.ring = None if ring is None or int(ring) >= self.capacity else int(ring)
        rows = self.capacity if self.ring is None else self.ring
        self.song = torch.zeros((rows, self.N, self.A), dtype=torch.int64, device=sess.dev)
        self.logp = torch.zeros((rows, self.N, self.A, 2), dtype=torch.float32, device=sess.dev) \
            if plan.logprobs else None
        self.count = torch.zeros(1, dtype=torch.int64, device=sess.dev)
        if self.ring is not None:
            self.slot = torch.zeros(1, dtype=torch.int64, device=sess.dev)       # count % ring
        self.seed = ops.next_seed()                       # keyed from torch.manual_seed, like the dropout seeds
        self.use_graph = ops.GRAPHS_ENABLED if graph is None else bool(graph)
        self._graph, self.enqueued = None, 0

    def _draw(self, logits):
        s = self.sess
        tok = s.tok.view(self.N, self.A)
        # the plain draw writes the song row itself; every other one, and a ring, takes a copy of the token buffer
        fused = self.ring is None and self.bar is None and self.logp is None and self.beat is None
        logits = _prefer_token(self.plan, logits, s.n_token, seen=self.seen, bar=self.bar)
        _draw_token(self.plan, logits, s.n_token, tok, self.seed, counter=self.count, bar=self.bar, beat=self.beat,
                    logp=self.logp, out_counter=self.count, song=self.song if fused else None)
        if self.bar is not None:
            ops.count_bars(tok, 2, self.bar_mask, self.bar)
        if self.beat is not None:
            ops.grammar_track(tok, self.plan.bar_attr, self.plan.order, self.beat)
        if self.seen is not None:
            ops.prefer_track(tok, s.n_token, self.plan.pen, self.seen)
        if not fused:
            self.song.index_copy_(0, self.count if self.ring is None else self.slot, tok.view(1, self.N, self.A))
        if self.ring is not None:
            self.slot.add_(1).remainder_(self.ring)
        self._after_draw(tok)
        self.count.add_(1)

    def _after_draw(self, tok):
        """What a loop adds to a token after the draw and its tracks, before the counter moves (none here)."""

    def _blend(self, logits, ref_logits):
        """The blended logits, written over the model's (ref_logits None: the model's own, untouched)."""
        if ref_logits is None:
            return logits
        return ops.blend_logits(logits, ref_logits, self.sess.n_token, self.plan.alpha, out=logits)

    def _one(self):
        s = self.sess
        if not self.carry:
            s._state.zero_()
            if self.ref is not None:
                self.ref._state.zero_()
        logits = s._device_step()
        self._draw(self._blend(logits, None if self.ref is None else self.ref._device_step()))

    def start(self, logits, ref_logits=None):
        """Draw the first token from logits the session already holds on the device (a prefill's; ref_logits: the
        reference session's, blended in first), as `_one` draws every later one: into the step's token buffer and row 0
        of the song, keyed by the counter."""
        if self.enqueued:
            raise RuntimeError("start() draws the loop's first token")
        with torch.no_grad():
            self._draw(self._blend(logits, ref_logits))
        self.enqueued = 1

    def run(self, n):
        """Enqueue n more tokens (no host sync)."""
        n = min(n, self.capacity - self.enqueued)
        with torch.no_grad():
            for _ in range(n):
                _enqueue_token(self, "decode loop")
        return n

    def tokens(self, start, stop):
        """Rows [start, stop) of the songs as host numpy (rows, n_songs, 6) (syncs)."""
        count = int(self.count.item())
        if count < stop:
            raise RuntimeError("device generation loop produced %d of %d tokens" % (count, stop))
        if self.ring is None:
            return self.song[start:stop].cpu().numpy()
        if count - start > self.ring:
            raise RuntimeError("rows from %d on were overwritten: the loop's ring holds the last %d" % (start, self.ring))
        idx = torch.arange(start, stop, device=self.song.device) % self.ring
        return self.song.index_select(0, idx).cpu().numpy()

    def logprobs(self, start, stop):
        """The log-probs of rows [start, stop) as host numpy (rows, n_songs, 6, 2) (logprobs=True; syncs)."""
        if self.logp is None:
            raise RuntimeError("this loop was built without logprobs=True")
        self.tokens(start, stop)                                     # the same checks (and sync)
        if self.ring is None:
            return self.logp[start:stop].cpu().numpy()
        idx = torch.arange(start, stop, device=self.logp.device) % self.ring
        return self.logp.index_select(0, idx).cpu().numpy()


def _gather_families(sessions, tensors, N):
    """The per-row buffers a resampling event of a particle loop moves, N rows each -> (families, row_bytes).  families:
    (state, scratch, row bytes, blocks, block stride in bytes) of, in launch order, the decode state of every session
    that is not None -- its S rows, then its Z rows, a block per layer -- and then every tensor that is not None, each
    with a scratch buffer of its own shape; row_bytes: what one moved row copies per phase."""
    families = []
    for s in sessions:
        if s is None:
            continue
        scratch = torch.empty_like(s._state)
        stride = 4 * N * (s.s_floats + s.z_floats)
        families.append((s._state, scratch, 4 * s.s_floats, s.n_layer, stride))
        families.append((s._state[N * s.s_floats:], scratch[N * s.s_floats:], 4 * s.z_floats, s.n_layer, stride))
    for t in tensors:
        if t is not None:
            families.append((t, torch.empty_like(t), t.numel() // N * t.element_size(), 1, 0))
    return families, sum(rb * nb for _, _, rb, nb, _ in families)


def _gather(families, anc, copy_back=False):
    """One phase of the two-phase cwlt_particle_gather over `families`, enqueued: every state's moved rows into its
    scratch, taken at the ancestors `anc`; copy_back: the same rows from the scratch back into the state."""
    for state, scratch, rb, nb, stride in families:
        dst, src = (state, scratch) if copy_back else (scratch, state)
        ops.particle_gather(dst, src, anc, rb, nb, stride, copy_back=copy_back)


def _event_ms(marks):
    """The milliseconds between the four HIP events of every timed event of a loop (None: not timed, none)."""
    return [[m[i].elapsed_time(m[i + 1]) for i in range(3)] for m in marks or []]


def _reward_buffers(loop, reward, N, A, dev, timed):
    """What both particle loops keep for a reward (`reward`: a _reward_spec or None) over N rows of A attributes, as
    _reward_event reads it off the loop: the rings `recent` (N, W, A) int64 of each row's last W drawn rows and `live`
    (N, W) int64, whether the particle was alive at each -- both gather families --, the window the callable sees (win,
    mask, any), beta_t (the device table of a beta per song, else None), the count n_rewards and, when timed, the list
    reward_timed.  Without a reward the buffers are None.  The history `h_r` is the loop's own."""
    loop.recent = loop.live = loop.win = loop.mask = loop.any = loop.beta_t = None
    loop.n_rewards = 0
    loop.reward_timed = [] if timed and reward is not None else None
    if reward is not None:
        W = reward[1]
        loop.recent = torch.zeros((N, W, A), dtype=torch.int64, device=dev)
        loop.live = torch.zeros((N, W), dtype=torch.int64, device=dev)
        loop.win, loop.mask = torch.zeros_like(loop.recent), torch.zeros_like(loop.live)
        loop.any = torch.zeros(N, dtype=torch.int64, device=dev)
        loop.beta_t = _beta_table(reward[2], dev)


def _reward_event(loop, filled, key, h_row):
    """One reward event of a particle loop (_ParticleLoop, _ParticleStreamLoop), enqueued on the current stream, no
    sync: cwlt_reward_window cuts the loop's rings into win / mask / any (filled: the ring's slots that belong to the
    window), the callable scores every row, and beta r goes into loop.lw and r into h_row -- cwlt_reward_apply, or with
    a beta per song cwlt_reward_apply_keyed, row n of song key[n] // K (key None: n // K).  A loop with a reward_timed
    list gets the four HIP events around the three steps appended."""
    fn, _, beta = loop.reward
    rows = loop.lw.numel()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if loop.reward_timed is not None else None
    mark = (lambda i: marks[i].record()) if marks else (lambda i: None)
    mark(0)
    ops.reward_window(loop.recent, loop.live, filled, loop.win, loop.mask, loop.any)
    mark(1)
    r = fn(loop.win, loop.mask)
    if not torch.is_tensor(r) or not r.is_cuda or r.dtype != torch.float32 or tuple(r.shape) != (rows,):
        raise TypeError("reward(windows, mask) must return a (%d,) float32 tensor on the GPU, got %s"
                        % (rows, "%s %s" % (tuple(r.shape), r.dtype) if torch.is_tensor(r) else type(r).__name__))
    mark(2)
    if loop.beta_t is None:
        ops.reward_apply(r.contiguous(), loop.any, beta, loop.lw, h_row)
    else:
        ops.reward_apply_keyed(r.contiguous(), loop.any, loop.beta_t, key, loop.K, loop.lw, h_row)
    mark(3)
    if marks:
        loop.reward_timed.append(marks)
    loop.n_rewards += 1


class _ParticleLoop(_DeviceLoop):
    """The lock-step loop with K particles per song: row g K + k of the pool is particle k of song g.
    Per token, inside the captured token and before the counter moves: cwlt_count_bars (into a count of the loop's own
    when the plan keeps none -- ending is decided on the device) and cwlt_particle_weigh, which adds the draw's
    lp_model - lp_sampler to `lw`, counts the row in `len` and sets `done` by the bar rule and `cap`.  After every
    `every` tokens resample(): lw is copied into row e of h_lw (E, N) f32 (the weights the event saw), then
    cwlt_particle_resample into row e of the device histories (anc (E, N) int64, u, ess (E, G) f32, resampled (E, G)
    int32), then the two-phase cwlt_particle_gather (_gather) of every per-row state the loop carries
    (_gather_families) -- the model's decode state and the reference's, the token buffer, bar, beat, seen, len, done,
    cap -- through scratch buffers of the same shapes: eager launches on the loop's stream, no sync.  lw is not
    gathered: the resampling kernel set it.  timed=True records HIP events around the resampling and each gather phase.

    reward (a _reward_spec: callable, window W, beta): two more per-row states (_reward_buffers), the
    rings `recent` and `live`, both gather families -- so a descendant inherits its ancestor's window together with its
    `done` flag, although the `song` ring is never gathered.  cwlt_reward_push fills slot count % W inside the captured
    token, ahead of cwlt_particle_weigh (it reads `done` as it was before the row).  After every W-th token, and ahead
    of a resampling event of the same token, reward_event(): cwlt_reward_window cuts the rings into win / mask / any,
    the callable scores them, cwlt_reward_apply adds beta r to lw and writes r into row j of h_r (ceil(capacity / W),
    N) f32 -- eager launches on the loop's stream, no sync.  timed=True records HIP events around the three steps too.
    A beta per song (a tuple): cwlt_reward_apply_keyed with the device table `beta_t`, row n of song
    n // K."""

    def __init__(self, sess, capacity, plan, particles, every, ess, bar_cond, caps, bar_mask, graph=None, ring=None,
                 timed=False, reward=None):
        super().__init__(sess, capacity, plan, graph=graph, ring=ring)
        dev, N = sess.dev, self.N
        self.K, self.every, self.ess_frac, self.bar_cond = int(particles), int(every), float(ess), int(bar_cond)
        self.G = N // self.K
        self.pbar, self.pbar_mask = self.bar, self.bar_mask
        if self.pbar is None:
            self.pbar = torch.as_tensor(np.asarray(self.plan.bar0s, dtype=np.int64)).to(dev)
            self.pbar_mask = torch.as_tensor(np.asarray(bar_mask, dtype=np.int32)).to(dev)
        self.lw = torch.zeros(N, dtype=torch.float32, device=dev)
        self.len = torch.zeros(N, dtype=torch.int64, device=dev)
        self.done = torch.zeros(N, dtype=torch.int64, device=dev)
        self.cap = torch.as_tensor(np.asarray(caps, dtype=np.int64)).to(dev)
        self.log_z = torch.zeros(self.G, dtype=torch.float32, device=dev)
        E = -(-self.capacity // self.every)
        self.h_anc = torch.zeros((E, N), dtype=torch.int64, device=dev)
        self.h_lw = torch.zeros((E, N), dtype=torch.float32, device=dev)
        self.h_u = torch.zeros((E, self.G), dtype=torch.float32, device=dev)
        self.h_ess = torch.zeros((E, self.G), dtype=torch.float32, device=dev)
        self.h_res = torch.zeros((E, self.G), dtype=torch.int32, device=dev)
        self.n_events = 0
        self.reward = reward
        _reward_buffers(self, reward, N, self.A, dev, timed)          # beta_t, a beta per song: row n is of song n // K
        if reward is not None:
            self.h_r = torch.zeros((-(-self.capacity // reward[1]), N), dtype=torch.float32, device=dev)
        self.families, self.row_bytes = _gather_families((sess, self.ref), (
            sess.tok, self.pbar, self.beat, self.seen, self.len, self.done, self.cap, self.recent, self.live), N)
        self.timed = [] if timed else None

    def _after_draw(self, tok):
        if self.pbar is not self.bar:
            ops.count_bars(tok, 2, self.pbar_mask, self.pbar)
        if self.reward is not None:
            ops.reward_push(tok, self.done, self.count, self.recent, self.live)
        ops.particle_weigh(self.logp, self.count, self.pbar, self.bar_cond, self.cap, self.lw, self.len, self.done)

    def reward_event(self, filled=None):
        """One reward event, enqueued: the window the callable sees, the callable, beta r into the weights.  filled:
        the ring's slots that belong to the window (default: all W, the ring has just wrapped)."""
        _reward_event(self, self.reward[1] if filled is None else filled, None, self.h_r[self.n_rewards])

    def _events(self):
        """What follows a token between replays: the reward event first, so that a resampling of the same token sees
        it."""
        if self.reward is not None and self.enqueued % self.reward[1] == 0:
            self.reward_event()
        if self.enqueued % self.every == 0:
            self.resample()

    def resample(self):
        """One resampling event, enqueued: the decision and ancestors, then every family state -> scratch -> state."""
        e = self.n_events
        anc = self.h_anc[e]
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.timed is not None else None
        mark = (lambda i: marks[i].record()) if marks else (lambda i: None)
        self.h_lw[e].copy_(self.lw)
        mark(0)
        ops.particle_resample(self.lw, self.done, self.K, self.ess_frac, self.seed, e, anc, self.h_u[e], self.h_ess[e],
                              self.h_res[e], self.log_z)
        mark(1)
        _gather(self.families, anc)
        mark(2)
        _gather(self.families, anc, copy_back=True)
        mark(3)
        if marks:
            self.timed.append(marks)
        self.n_events += 1

    def run(self, n):
        """Enqueue n more tokens, with a resampling event after every `every`-th token of the run and, under a reward, a
        reward event after every W-th (no host sync)."""
        n = min(n, self.capacity - self.enqueued)
        with torch.no_grad():
            for _ in range(n):
                _enqueue_token(self, "particle loop")
                self._events()
        return n

    def start(self, logits, ref_logits=None):
        super().start(logits, ref_logits)
        with torch.no_grad():
            self._events()                                             # only an `every` or a W of 1 has one here


class _StreamLoop:
    """Continuous batching on the device: `sess` (DecodeSession(n_songs=slots, kernel="gemm")) is a pool of decode slots
    that runs `n_songs` songs, each slot starting the next song as soon as its own one ends.  Per token, one fixed
    sequence of launches (captured as one hipGraph after two eager tokens):
      the GEMM decode step on every slot;
      the refill: slots flagged fresh get the state and logits their new song starts from;
      the draw (_draw_token), each slot's keyed by (song index, position in song): cwlt_sample_categorical_keyed, or
        the masked / log-prob / grammar entry when `plan` (DeviceDraw) has a constraint table (the song's mask row for
        the slot's bar count), log-probs or a grammar (the row grammar at the slot's position);
      the advance: (song, token, end bit) into row t % R of `ring` (R, slots, A + 2), position / bar count advanced, the
        song's end detected, finished slots handed the next song indices in slot order;
      cwlt_grammar_track (under a grammar): every slot's position after the advance.
    Preferences add cwlt_prefer_logits in front of the draw, keyed by the slots' song indices and bar
    counts, in place on the logits, and -- when some song has a penalty -- cwlt_prefer_track at the end: `seen` (slots,
    sum n_class) f32 follows the slots, a slot handed a song taking that song's seen0 through `fresh`, as `beat` does.
    The ring holds two chunks: chunk k + 1 is enqueued before chunk k is read, so the device never waits on the host.
    plan.logprobs: the sampler is cwlt_sample_categorical_logp (the same tokens), writing each slot's (model, sampler)
    log-probs into `lp_ring` (2 chunk, slots, A, 2) at the row ctl[0] selects -- the row of `ring` the advance writes --
    copied out behind the same event and filtered by the same song >= 0 mask as the token rows (`lp_parts`).

    This class holds what both forms of the stream share.  A form supplies where songs start from: _refill and _advance
    (its pair of csrc/stream.hip entries), n_ctl (the device counters {tokens, assigned, finished}, and what the form
    adds), song_cap (the most tokens one song draws: run()'s step limit) and start() (its _hand_out)."""

    n_ctl = 3

    def __init__(self, sess, n_songs, seed, bar_mask, bar_cond, chunk, plan=None, graph=None):
        self.sess, self.n_songs, self.chunk = sess, int(n_songs), int(chunk)
        self.S, self.A = sess.n_songs, len(sess.n_token)
        dev = sess.dev
        self.seed = seed
        self.plan = plan = DeviceDraw() if plan is None else plan
        self.bar_mask = torch.as_tensor(np.asarray(bar_mask, dtype=np.int32), device=dev)
        self.bar_cond = int(bar_cond)
        # the slots' song, position in it, bar count and fresh flag (1: refill me): set by start(), then the device's
        self.song, self.pos, self.bar, self.fresh = (torch.zeros(self.S, dtype=torch.int64, device=dev)
                                                     for _ in range(4))
        self.ctl = torch.zeros(self.n_ctl, dtype=torch.int64, device=dev)
        self.ring = torch.zeros((2 * self.chunk, self.S, self.A + 2), dtype=torch.int64, device=dev)
        self._host = [torch.zeros((self.chunk, self.S, self.A + 2), dtype=torch.int64).pin_memory() for _ in range(2)]
        self.beat = None if plan.order is None else torch.full((self.S,), -1, dtype=torch.int64, device=dev)
        self.seen = None if plan.seen0 is None else torch.zeros((self.S, sess.width), dtype=torch.float32, device=dev)
        self.lp_ring = torch.zeros((2 * self.chunk, self.S, self.A, 2), dtype=torch.float32, device=dev) \
            if plan.logprobs else None
        self._host_lp = [torch.zeros((self.chunk, self.S, self.A, 2), dtype=torch.float32).pin_memory()
                         for _ in range(2)] if plan.logprobs else None
        self.lp_parts = []
        self._host_ctl = [torch.zeros(self.n_ctl, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._events = [torch.cuda.Event(), torch.cuda.Event()]
        self.use_graph = ops.GRAPHS_ENABLED if graph is None else bool(graph)
        self._graph, self.enqueued = None, 0
        self.wait_s = 0.0                                          # host time spent waiting on the device

    def _hand_out(self, first, wait, ctl):
        """The hand-out before the first token: slots 0 .. first - 1 take songs 0 .. first - 1 and are fresh (under a
        grammar every slot with a song for it starts at that song's beat0; a slot handed a song later takes that song's
        in cwlt_grammar_track); a slot past them holds `wait` while there is a song for it, or idles (-1).  ctl: the
        counters to start from."""
        slot = torch.arange(self.S, dtype=torch.int64, device=self.sess.dev)
        rest = torch.where(slot < self.n_songs, torch.full_like(slot, wait), torch.full_like(slot, -1))
        self.song.copy_(torch.where(slot < first, slot, rest))
        self.fresh.copy_((slot < first).to(torch.int64))
        if self.beat is not None:
            k = min(self.S, self.n_songs)
            self.beat[:k] = self.plan.beat0[:k]
        if self.seen is not None:
            k = min(self.S, self.n_songs)
            self.seen[:k] = self.plan.seen0[:k]
        self.ctl.copy_(torch.tensor(ctl, dtype=torch.int64))

    def _one(self):
        s = self.sess
        tok = s.tok.view(self.S, self.A)
        logits = s._device_step()
        self._refill(logits)
        _prefer_token(self.plan, logits, s.n_token, seen=self.seen, key=self.song, bar=self.bar)
        _draw_token(self.plan, logits, s.n_token, tok, self.seed, key=self.song, step=self.pos, bar=self.bar,
                    beat=self.beat, logp=self.lp_ring, out_counter=self.ctl)
        self._advance(tok)
        if self.beat is not None:
            ops.grammar_track(tok, self.plan.bar_attr, self.plan.order, self.beat, fresh=self.fresh, song=self.song,
                              beat0=self.plan.beat0)
        if self.seen is not None:
            ops.prefer_track(tok, s.n_token, self.plan.pen, self.seen, fresh=self.fresh, song=self.song,
                             seen0=self.plan.seen0)

    def _read(self, h):
        """The rows of ring half h that belong to songs (waiting and idle slots write song < 0), and their log-probs
        into lp_parts by the same mask.  Boolean indexing copies: the pinned buffers are reused."""
        rows = self._host[h].numpy().reshape(-1, self.A + 2)
        keep = rows[:, 0] >= 0
        if self.lp_ring is not None:
            self.lp_parts.append(self._host_lp[h].numpy().reshape(-1, self.A, 2)[keep])
        return rows[keep]

    def _enqueue_chunk(self):
        """Enqueue `chunk` tokens and the copy of their ring half (and the counters) to pinned host memory."""
        with torch.no_grad():
            for _ in range(self.chunk):
                _enqueue_token(self, "stream step")
        k = self.enqueued // self.chunk - 1
        h = k % 2
        self._host[h].copy_(self.ring[h * self.chunk:(h + 1) * self.chunk], non_blocking=True)
        if self.lp_ring is not None:
            self._host_lp[h].copy_(self.lp_ring[h * self.chunk:(h + 1) * self.chunk], non_blocking=True)
        self._host_ctl[h].copy_(self.ctl, non_blocking=True)
        self._events[h].record()
        return h

    def _wait(self, h):
        t = time.perf_counter()
        self._events[h].synchronize()
        self.wait_s += time.perf_counter() - t

    def _step_limit(self):
        """The most steps run() enqueues before it gives up: every slot's songs, one by one."""
        return -(-self.n_songs // self.S) * (self.song_cap + 1) + 2 * self.chunk

    def _between_chunks(self, ctl, limit):
        """Between two chunks of run(), with the counters of the chunk just read: the step limit."""
        if self.enqueued > limit:
            raise RuntimeError("stream did not finish %d songs in %d steps" % (self.n_songs, self.enqueued))

    def run(self):
        """Run until the device's finished counter reaches n_songs -> (rows (n, A + 2) of every song, time-ordered)."""
        parts = []
        limit = self._step_limit()
        self.start()
        h = self._enqueue_chunk()
        while True:
            nxt = self._enqueue_chunk()
            self._wait(h)
            parts.append(self._read(h))
            ctl = self._host_ctl[h].numpy().copy()
            if ctl[2] >= self.n_songs:
                break
            self._between_chunks(ctl, limit)
            h = nxt
        self._wait(nxt)                                            # the one chunk enqueued past the end
        return np.concatenate(parts)

    def stats(self):
        """After run(): what the form adds to generate_stream's stats."""
        return {}


class _SnapshotStreamLoop(_StreamLoop):
    """The stream whose songs all start from one snapshot (snap_state, snap_logits: _stream_snapshot), with one bar0 and
    one cap: cwlt_stream_refill and cwlt_stream_advance.

    plan.ref, plan.alpha with ref_snap = (state, logits): the blend with a reference model.  `ref`
    (DecodeSession.shadow) is a second pool of the same slots on the same token buffer, with its own snapshot: per token
    it steps and is refilled right after the model's pool, by the same fresh flags, then cwlt_blend_logits (alpha: the
    (1 | n_songs, A) f32 device table, keyed by the slots' song indices -- an idle slot's row is copied)
    turns the model's logits into the blend's in place, and the draw, advance and grammar track go on as without it:
    still one stream and one linear captured graph per token."""

    def __init__(self, sess, snap_state, snap_logits, n_songs, seed, bar_mask, bar_cond, bar0, cap, chunk,
                 ref_snap=None, **kw):
        super().__init__(sess, n_songs, seed, bar_mask, bar_cond, chunk, **kw)
        self.snap_state, self.snap_logits = snap_state, snap_logits
        self.bar0, self.cap = int(bar0), int(cap)
        self.song_cap = self.cap
        self.ref_snap = ref_snap

    def start(self):
        """Slots 0, 1, ... take the first songs; slots past the last song idle."""
        first = min(self.S, self.n_songs)
        self._hand_out(first, -1, [0, first, 0])
        self.bar.fill_(self.bar0)

    def _refill(self, logits):
        s, ref = self.sess, self.plan.ref
        ops.stream_refill(s._state, self.snap_state, s.n_layer, s.s_floats, s.z_floats, logits, self.snap_logits,
                          self.fresh)
        if ref is not None:                                     # the reference's pool, then the blend over `logits`
            ref_logits = ref._device_step()
            ops.stream_refill(ref._state, self.ref_snap[0], ref.n_layer, ref.s_floats, ref.z_floats, ref_logits,
                              self.ref_snap[1], self.fresh)
            ops.blend_logits(logits, ref_logits, self.sess.n_token, self.plan.alpha, key=self.song, out=logits)

    def _advance(self, tok):
        ops.stream_advance(tok, 2, self.bar_mask, self.bar_cond, self.bar0, self.cap, self.n_songs, self.song,
                           self.pos, self.bar, self.fresh, self.ctl, self.ring)


class _ParticleStreamLoop(_StreamLoop):
    """The stream whose unit of refill is a group of K rows: `sess` (DecodeSession(S K, kernel="gemm"))
    runs S songs with K particles each, row g K + k particle k of group g's song, and a group takes the next song once
    all its K particles have ended -- at the next resampling boundary, so that every song sees its own events after its
    own rows R, 2 R, ...  `song` (rows,) holds the rows' particle ids (song K + k, the plan's rows; -1: none), `gsong`
    (S,) the groups' songs.  Per token, one captured sequence: the decode step (and the reference's), cwlt_stream_refill
    of the fresh rows from the snapshot(s), the blend, the preferences, the draw keyed by (particle id, position in
    song) with its log-probs, cwlt_count_bars, the tracks (which never see a fresh flag), cwlt_particle_weigh and
    cwlt_particle_advance.  After every R-th token, eagerly on the same stream (_event): lw into its history, the keyed
    resampling, the two-phase gather (_gather) of every family (_gather_families), cwlt_particle_release and the
    fill of the new particles' beat / seen rows.  The event histories are rings of two chunks' events, copied out with
    the token rows behind the chunk's event; rows are kept per (step, row): the lineage needs the row index.

    reward (a _reward_spec: callable, window W, beta): the rings `recent` (S K, W, A) and `live` (S K, W)
    of _reward_buffers join the gather families, and cwlt_reward_push, with the stream's step counter ctl[0] as its
    counter, sits in the captured token ahead of cwlt_particle_weigh.  A group then takes a song only at run steps that
    are multiples of B = lcm(R, W) -- the release and the fills run at those boundaries alone, a finished group waits
    for the next one -- so that every song starts at t0 = 0 (mod B) and slot ctl[0] % W is the song's own pos % W: its
    windows close after its own rows W, 2 W, ...  After every W-th token, ahead of a resampling of the same token
    (_reward_event): cwlt_reward_window (always the whole ring: it has just wrapped), the callable on all S K rows,
    cwlt_reward_apply -- or cwlt_reward_apply_keyed with a beta per song, keyed by the rows' particle ids -- into a ring
    `h_r` of two chunks' reward events, copied out with the chunk.  timed=True records HIP events around the three steps of
    every reward event.  reward=None: launch for launch the loop without this paragraph."""

    def __init__(self, sess, snap, ref_snap, n_songs, particles, every, ess, seed, bar_mask, bar_cond, bar0, cap, chunk,
                 reward=None, timed=False, **kw):
        super().__init__(sess, n_songs, seed, bar_mask, bar_cond, chunk, **kw)
        dev, N = sess.dev, self.S
        self.K, self.every, self.ess_frac = int(particles), int(every), float(ess)
        self.G = N // self.K
        self.snap, self.ref_snap, self.bar0, self.cap0 = snap, ref_snap, int(bar0), int(cap)
        self.song_cap = self.cap0
        i64 = lambda n, v=0: torch.full((n,), v, dtype=torch.int64, device=dev)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.gsong, self.len, self.done, self.cap, self.no_fresh = i64(self.G, -1), i64(N), i64(N, 1), i64(N, 1), i64(N)
        self.song.fill_(-1)
        self.lw, self.log_z = f32(N), f32(self.G)
        P = self.n_songs * self.K
        self.out_lw, self.out_len, self.out_logz = f32(P), i64(P), f32(self.n_songs)
        self.EC = self.chunk // self.every                       # events per chunk; the history rings hold two chunks'
        E2 = 2 * self.EC
        self.h_anc = torch.zeros((E2, N), dtype=torch.int64, device=dev)
        self.h_lw, self.h_u, self.h_ess = f32(E2, N), f32(E2, self.G), f32(E2, self.G)
        self.h_res = torch.zeros((E2, self.G), dtype=torch.int32, device=dev)
        self._hist = (self.h_anc, self.h_lw, self.h_ess, self.h_res)
        self._host_hist = [[torch.zeros((self.EC,) + tuple(t.shape[1:]), dtype=t.dtype).pin_memory()
                            for t in self._hist] for _ in range(2)]
        self.hist_parts = [[] for _ in self._hist]
        self.n_events = 0
        self.reward = reward
        _reward_buffers(self, reward, N, self.A, dev, timed)     # beta_t, a beta per song: keyed by particle id
        self.hand_every = self.every                             # a group takes a song at multiples of this many steps
        if reward is not None:
            W = reward[1]
            self.hand_every = _lcm(self.every, W)
            self.step = self.ctl[:1]                             # the run's step counter, cwlt_reward_push's
            self.RC = self.chunk // W                            # reward events per chunk; a ring of two chunks' again
            self.h_r = f32(2 * self.RC, N)
            self._host_r = [torch.zeros((self.RC, N), dtype=torch.float32).pin_memory() for _ in range(2)]
            self.r_parts = []
        self.families, self.row_bytes = _gather_families((sess, self.plan.ref), (
            sess.tok, self.bar, self.beat, self.seen, self.len, self.done, self.cap, self.recent, self.live), N)

    def _step_limit(self):
        """List scheduling: the songs' total over the groups plus one longest song, each rounded up to a boundary at
        which groups take songs."""
        per = -(-self.cap0 // self.hand_every) * self.hand_every + self.hand_every
        return (-(-self.n_songs // self.G) + 1) * per + 2 * self.chunk

    def _hand_out_songs(self):
        ops.particle_release(self.K, self.n_songs, self.bar0, self.cap0, self.gsong, self.song, self.pos, self.bar,
                             self.cap, self.len, self.done, self.fresh, self.lw, self.log_z, self.ctl, self.out_lw,
                             self.out_len, self.out_logz)

    def _release(self):
        """The release, then the new particles' grammar positions and repetition states by particle id."""
        self._hand_out_songs()
        if self.beat is not None:
            ops.particle_fill(self.beat, self.plan.beat0, self.fresh, self.song)
        if self.seen is not None:
            ops.particle_fill(self.seen, self.plan.seen0, self.fresh, self.song)

    def start(self):
        """Every group is without a song; the first release hands out songs 0, 1, ... in group order."""
        self.ctl.zero_()
        self._release()

    def _refill(self, sess, logits, ref=False):
        """The fresh rows of `sess` (the model's pool, or ref: the reference's) and of its logits take their start."""
        snap = self.ref_snap if ref else self.snap
        ops.stream_refill(sess._state, snap[0], sess.n_layer, sess.s_floats, sess.z_floats, logits, snap[1], self.fresh)

    def _one(self):
        s, plan = self.sess, self.plan
        tok = s.tok.view(self.S, self.A)
        logits = s._device_step()
        self._refill(s, logits)
        ref = plan.ref
        if ref is not None:
            ref_logits = ref._device_step()
            self._refill(ref, ref_logits, ref=True)
            ops.blend_logits(logits, ref_logits, s.n_token, plan.alpha, key=self.song, out=logits)
        _prefer_token(plan, logits, s.n_token, seen=self.seen, key=self.song, bar=self.bar)
        _draw_token(plan, logits, s.n_token, tok, self.seed, key=self.song, step=self.pos, bar=self.bar, beat=self.beat,
                    logp=self.lp_ring, out_counter=self.ctl)
        ops.count_bars(tok, 2, self.bar_mask, self.bar)
        if self.beat is not None:
            ops.grammar_track(tok, plan.bar_attr, plan.order, self.beat)
        if self.seen is not None:                             # keyed by the particle id; the release filled the fresh rows
            ops.prefer_track(tok, s.n_token, plan.pen, self.seen, fresh=self.no_fresh, song=self.song,
                             seen0=plan.seen0)
        if self.reward is not None:                            # slot ctl[0] % W; reads `done` as it was before the row
            ops.reward_push(tok, self.done, self.step, self.recent, self.live)
        # weigh reads the log-prob row ctl[0] selects: ahead of the advance, which moves it
        ops.particle_weigh(self.lp_ring, self.ctl, self.bar, self.bar_cond, self.cap, self.lw, self.len, self.done)
        ops.particle_advance(tok, self.song, self.done, self.pos, self.fresh, self.ctl, self.ring)

    def _reward_event(self):
        """One reward event, enqueued on the stream's own stream, no sync: the windows of all S K rows, the callable,
        beta r into the weights and r into the history ring.  Rows without a live slot -- finished, waiting, parked --
        are shown mask[n, 0] = 1 and their result is discarded."""
        _reward_event(self, self.reward[1], self.song, self.h_r[self.n_rewards % (2 * self.RC)])

    def _event(self):
        """One boundary, enqueued: the resampling of every group with a live song, the gather, then -- at a boundary at
        which groups take songs (every one without a reward) -- the release."""
        r = self.n_events % (2 * self.EC)
        anc = self.h_anc[r]
        self.h_lw[r].copy_(self.lw)
        ops.particle_resample_keyed(self.lw, self.done, self.K, self.ess_frac, self.seed, self.gsong, self.pos,
                                    self.every, anc, self.h_u[r], self.h_ess[r], self.h_res[r], self.log_z)
        _gather(self.families, anc)
        _gather(self.families, anc, copy_back=True)
        if self.enqueued % self.hand_every == 0:
            self._release()
        self.n_events += 1

    def _enqueue_chunk(self):
        with torch.no_grad():
            for _ in range(self.chunk):
                _enqueue_token(self, "particle stream step")
                if self.reward is not None and self.enqueued % self.reward[1] == 0:
                    self._reward_event()                              # ahead of a resampling of the same step
                if self.enqueued % self.every == 0:
                    self._event()
        h = (self.enqueued // self.chunk - 1) % 2
        self._host[h].copy_(self.ring[h * self.chunk:(h + 1) * self.chunk], non_blocking=True)
        self._host_lp[h].copy_(self.lp_ring[h * self.chunk:(h + 1) * self.chunk], non_blocking=True)
        for host, t in zip(self._host_hist[h], self._hist):
            host.copy_(t[h * self.EC:(h + 1) * self.EC], non_blocking=True)
        if self.reward is not None:
            self._host_r[h].copy_(self.h_r[h * self.RC:(h + 1) * self.RC], non_blocking=True)
        self._host_ctl[h].copy_(self.ctl, non_blocking=True)
        self._events[h].record()
        return h

    def _read(self, h):
        """Ring half h whole, (chunk, rows, A + 2), and its log-probs and event histories into their lists."""
        self.lp_parts.append(self._host_lp[h].numpy().copy())
        for parts, host in zip(self.hist_parts, self._host_hist[h]):
            parts.append(host.numpy().copy())
        if self.reward is not None:
            self.r_parts.append(self._host_r[h].numpy().copy())
        return self._host[h].numpy().copy()


class _PromptBank:
    """What the two streams with a prompt of its own for every song share (mixed in ahead of their _StreamLoop): the
    device bank.  Song k starts from entry k % bank of a bank laid out like a `bank`-slot DecodeSession._state (per
    layer the S rows of all entries, then their Z rows), with its next-token logits beside it.  Blocks of B consecutive
    songs are prefilled (CWTrunk._prefill_gemm, batch invariant) straight into their entries between chunks, on the
    stream's own stream, each followed by a device write of ctl[3] = songs ready, the counter these forms add; a block
    is written only once the reuse rule (bank_may_prefill) allows it.  ref (a DecodeSession, the blend's reference):
    a second bank, `ref_bank`, prefilled by the reference model in the same block step."""

    n_ctl = 4

    def _bank_buffers(self, sess):
        """(state, per-layer [S, Z] views, logits) of a bank for `sess`'s model."""
        H, d = sess.memory[0][1].shape[1:]
        sf, zf, n_layer = sess.s_floats, sess.z_floats, sess.n_layer
        per = self.bank * (sf + zf)
        state = torch.zeros(per * n_layer, dtype=torch.float32, device=sess.dev)
        mem = [[state[i * per:i * per + self.bank * sf].view(self.bank, H, d, d),
                state[i * per + self.bank * sf:(i + 1) * per].view(self.bank, H, d)] for i in range(n_layer)]
        return state, mem, torch.zeros((self.bank, sess.width), dtype=torch.float32, device=sess.dev)

    def _init_bank(self, heads, bar0s, caps, B, bank, prefill_rows=None, ref=None, packed=False):
        """heads, bar0s, caps: one entry per song.  packed: the blocks go through the packed prefill
        (CWTrunk._prefill_gemm_packed, the same bits): the prompts lie end to end on the device, without padding, and
        every block has its own offset table, all built here."""
        sess, dev = self.sess, self.sess.dev
        self.song_cap = int(max(caps))
        self.B, self.bank = int(B), int(bank)
        self.nb = self.bank // self.B
        self.n_blocks = -(-self.n_songs // self.B)
        self.bank_state, self.bank_mem, self.bank_logits = self._bank_buffers(sess)
        self.ref_bank = None if ref is None else (ref.model,) + self._bank_buffers(ref)
        # every prompt on the device once, padded to the longest: no host copy (and no sync) inside the stream
        lens = np.array([len(h) for h in heads], dtype=np.int64)
        self.lens = lens
        self.packed = bool(packed)
        if self.packed:
            # ... or end to end: block j is rows [row0[j], row0[j + 1]), its offsets (from 0) a view of one table
            self.toks = torch.as_tensor(np.concatenate(heads)).to(dev)
            cu = [np.concatenate([[0], np.cumsum(lens[j * self.B:(j + 1) * self.B])]) for j in range(self.n_blocks)]
            table = torch.as_tensor(np.concatenate(cu).astype(np.int32)).to(dev)
            at = np.concatenate([[0], np.cumsum([len(c) for c in cu])])
            self.block_cu = [ops.SeqOffsets(table[at[j]:at[j + 1]], host=c.tolist()) for j, c in enumerate(cu)]
            self.block_row0 = np.concatenate([[0], np.cumsum([c[-1] for c in cu])])
        else:
            toks = np.zeros((self.n_songs, int(lens.max()), self.A), dtype=np.int64)
            for i, h in enumerate(heads):
                toks[i, :len(h)] = h
            self.toks = torch.as_tensor(toks).to(dev)
        self.dev_len = torch.as_tensor(lens.astype(np.int32)).to(dev)
        self.bar0_all = torch.as_tensor(np.asarray(bar0s, dtype=np.int64)).to(dev)
        self.cap_all = torch.as_tensor(np.asarray(caps, dtype=np.int64)).to(dev)
        self.prefill_rows = prefill_rows
        self.next_block = 0                                        # blocks prefilled so far
        self.prefill_events = []                                   # (start, stop) CUDA events of every block
        self.gated_chunks = 0                                      # chunks that ended with every ready song assigned

    def _prefill_into(self, model, bank_mem, bank_logits, a, z, e0, e1):
        """Songs [a, z) through `model`'s batch-invariant prefill into the entries [e0, e1) of one bank."""
        mem = [[S[e0:e1], Z[e0:e1]] for S, Z in bank_mem]
        for S, Z in mem:
            S.zero_()
            Z.zero_()
        if self.packed:
            j = a // self.B
            _, logits = model._prefill_gemm_packed(self.toks[self.block_row0[j]:self.block_row0[j + 1]],
                                                   self.block_cu[j], mem)
        else:
            P = int(self.lens[a:z].max())
            dl = self.dev_len[a:z]
            _, logits = model._prefill_gemm(self.toks[a:z, :P].contiguous(), mem, dl, dl.to(torch.int64) - 1)
        bank_logits[e0:e1].copy_(logits)

    def _block_written(self, a, z, e0, e1):
        """What a form writes beside a block's entries, ahead of the ready counter (nothing here)."""

    def _prefill_block(self):
        """Enqueue block next_block's prefill into its bank entries, then ctl[3] = its last song + 1."""
        j = self.next_block
        a, z = j * self.B, min(self.n_songs, (j + 1) * self.B)
        e0 = (j % self.nb) * self.B
        e1 = e0 + (z - a)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        with torch.no_grad():
            self._prefill_into(self.sess.model, self.bank_mem, self.bank_logits, a, z, e0, e1)
            if self.ref_bank is not None:
                self._prefill_into(self.ref_bank[0], self.ref_bank[2], self.ref_bank[3], a, z, e0, e1)
            self._block_written(a, z, e0, e1)
            self.ctl[3:4].fill_(z)                                 # ordered after the block's writes: same stream
        ev[1].record()
        self.prefill_events.append(ev)
        self.next_block += 1

    def _prefill_allowed(self, assigned):
        """Prefill every block the reuse rule allows (bank_may_prefill) given the copied assigned counter."""
        while self.next_block < self.n_blocks and bank_may_prefill(self.next_block, self.B, self.bank, assigned):
            self._prefill_block()

    def _between_chunks(self, ctl, limit):
        """A chunk that ended with every ready song assigned counts as gated (slots may have waited for a prefill: a
        chunk more for the step limit); after the limit's check, prefill every block the reuse rule allows."""
        if ctl[1] < self.n_songs and ctl[1] >= ctl[3]:
            self.gated_chunks += 1
        super()._between_chunks(ctl, limit + self.gated_chunks * self.chunk)
        self._prefill_allowed(int(ctl[1]))

    def stats(self):
        """After run(): the block size, bank entries, GPU seconds of the block prefills, blocks, gated chunks."""
        return {"block": self.B, "bank": self.bank,
                "prefill_seconds": sum(a.elapsed_time(b) for a, b in self.prefill_events) / 1e3,
                "prefill_blocks": self.next_block, "gated_chunks": self.gated_chunks}


class _BankStreamLoop(_PromptBank, _StreamLoop):
    """The stream with a prompt of its own for every song (_PromptBank), each entry with its song's bar count and cap
    beside it.  cwlt_stream_refill_bank and cwlt_stream_advance_bank: a slot takes a song only below ctl[3], otherwise
    it waits (song -2), and keeps its song's cap in `cap`."""

    def __init__(self, sess, heads, n_songs, seed, bar_mask, bar_cond, bar0s, caps, B, bank, chunk, prefill_rows=None,
                 packed=False, **kw):
        super().__init__(sess, n_songs, seed, bar_mask, bar_cond, chunk, **kw)
        self.cap = torch.ones(self.S, dtype=torch.int64, device=sess.dev)
        self._init_bank(heads, bar0s, caps, B, bank, prefill_rows, packed=packed)
        self.bank_bar0 = torch.zeros(self.bank, dtype=torch.int64, device=sess.dev)
        self.bank_cap = torch.ones(self.bank, dtype=torch.int64, device=sess.dev)

    def _block_written(self, a, z, e0, e1):
        self.bank_bar0[e0:e1].copy_(self.bar0_all[a:z])
        self.bank_cap[e0:e1].copy_(self.cap_all[a:z])

    def start(self):
        """Prefill the first nb blocks and hand the ready songs to slots 0, 1, ... in order; slots past them wait while
        songs remain, or idle."""
        self._prefill_allowed(0)
        ready = min(self.n_songs, self.next_block * self.B)
        first = min(self.S, ready)
        self._hand_out(first, -2, [0, first, 0, ready])
        self.bar[:first] = self.bar0_all[:first]
        self.cap[:first] = self.cap_all[:first]

    def _refill(self, logits):
        s = self.sess
        ops.stream_refill_bank(s._state, self.bank_state, s.n_layer, s.s_floats, s.z_floats, logits, self.bank_logits,
                               self.fresh, self.song)

    def _advance(self, tok):
        ops.stream_advance_bank(tok, 2, self.bar_mask, self.bar_cond, self.bank_bar0, self.bank_cap, self.n_songs,
                                self.song, self.pos, self.bar, self.cap, self.fresh, self.ctl, self.ring)


class _ParticleBankStreamLoop(_PromptBank, _ParticleStreamLoop):
    """The particle stream with a prompt of its own for every song: _ParticleStreamLoop on _PromptBank's
    bank, one entry -- one prefill -- per song for all its K particles.  Per token cwlt_particle_refill_bank in the
    place of cwlt_stream_refill (a second one from `ref_bank` for the blend's reference, as the snapshot form does with
    ref_snap); per hand-out boundary cwlt_particle_release_bank in the place of cwlt_particle_release: a group takes a
    song only below ctl[3], else it is parked until the next boundary, and its rows start from the song's own bar count
    and cap (bar0_all, cap_all: tables of n_songs entries, not bank-sized, so no reuse hazard arises).
    The reuse rule carries over from _BankStreamLoop: a song assigned by a release at the end of chunk k is copied out
    by the refill of the first token of chunk k + 1, and that token is already on the stream when the host reads chunk
    k's counters and enqueues the next block's prefill behind it."""

    def __init__(self, sess, heads, n_songs, particles, every, ess, seed, bar_mask, bar_cond, bar0s, caps, B, bank,
                 chunk, prefill_rows=None, packed=False, **kw):
        super().__init__(sess, None, None, n_songs, particles, every, ess, seed, bar_mask, bar_cond, bar0s[0],
                         max(caps), chunk, **kw)                 # cap0, the step limit's: the largest cap
        self._init_bank(heads, bar0s, caps, B, bank, prefill_rows, ref=self.plan.ref, packed=packed)

    def _hand_out_songs(self):
        ops.particle_release_bank(self.K, self.n_songs, self.bar0_all, self.cap_all, self.gsong, self.song, self.pos,
                                  self.bar, self.cap, self.len, self.done, self.fresh, self.lw, self.log_z, self.ctl,
                                  self.out_lw, self.out_len, self.out_logz)

    def start(self):
        """Prefill the first nb blocks; then the first release hands the ready songs out in group order."""
        self.ctl.zero_()
        self._prefill_allowed(0)
        self._release()

    def _refill(self, sess, logits, ref=False):
        state, blogits = (self.ref_bank[1], self.ref_bank[3]) if ref else (self.bank_state, self.bank_logits)
        ops.particle_refill_bank(sess._state, state, sess.n_layer, sess.s_floats, sess.z_floats, logits, blogits,
                                 self.fresh, self.song, self.K)


def _stream_snapshot(model, prompt, A, kernel="blas"):
    """The state and logits every song of a stream starts from, on a one-slot GEMM session: one step of INIT_CW from
    zero state (bitwise any row of the many-slot step, by batch invariance), or a one-row prefill of the prompt with
    prefill kernel `kernel` ("gemm": batch invariant, bitwise any row of a many-song gemm prefill of the same prompt)."""
    snap = DecodeSession(model, n_songs=1, kernel="gemm", graph=False)
    snap.reset()
    with torch.no_grad():
        if prompt is None:
            snap.tok.copy_(torch.as_tensor(INIT_CW[0], dtype=torch.int64).view(1, 1, A).to(snap.dev))
            logits = snap._device_step()
        else:
            logits = snap._prefill(prompt, kernel=kernel)
    return snap._state.clone(), logits.reshape(-1).clone()


def _check_prompts(prompts, n_songs, word2event, n_token, bar_cond, max_tokens):
    """The refusals every generation entry makes for its prompts, a list of one array per song -> (heads (P_i, A) int64,
    bar0s: each song's bar count before its first drawn row, caps: the rows it may draw, 16384 without max_tokens).
    n_token: the model's classes, to refuse ids out of range as well (None: the prefill refuses them)."""
    A = len(word2event)
    if len(prompts) != n_songs:
        raise ValueError("prompts: %d arrays for %d songs" % (len(prompts), n_songs))
    names = word2event["bar-beat"]
    heads, bar0s, caps = [], [], []
    for i, p in enumerate(prompts):
        p = np.asarray(p, dtype=np.int64).reshape(-1, A)
        if len(p) == 0:
            raise ValueError("empty prompt (song %d)" % i)
        bad = False if n_token is None else (p < 0) | (p >= np.asarray(n_token))
        if np.any(bad):
            t, a = np.argwhere(bad)[0]
            raise ValueError("prompt %d, token %d: id %d out of range for attribute %d (%d classes)"
                             % (i, t, p[t, a], a, n_token[a]))
        cnt = 1 + sum(names[int(r[2])] == "Bar" for r in p[1:])
        if cnt >= bar_cond:
            raise ValueError("the prompt of song %d already reaches bar %d of bar_cond=%d" % (i, cnt, bar_cond))
        if max_tokens is not None and max_tokens <= len(p):
            raise ValueError("max_tokens (%d) leaves no room after a %d-token prompt" % (max_tokens, len(p)))
        heads.append(p)
        bar0s.append(cnt)
        caps.append(16384 if max_tokens is None else max_tokens - len(p))
    return heads, bar0s, caps


def _generate_stream(model, word2event, n_songs, slots=256, bar_cond=17, max_tokens=None, prompt=None, sampler="dqn",
                     chunk=128, log=None, prompts=None, bank=None, prefill_rows=None, constraints=None,
                     return_logprobs=False, grammar=None, reference=None, alpha=None, where="generate_stream",
                     preferences=None, packed_prefill=False):
    """generate_stream -> (songs, stats): steps run, tokens (prompts included) and drawn, slot-steps (steps x slots),
    wall seconds, host seconds spent waiting on the device, and whether the token ran as a captured graph.  With
    prompts: also the block size, bank entries, blocks prefilled, their GPU seconds and the gated chunks.
    return_logprobs=True: -> ((songs, logprobs), stats).  where: the entry the refusals name."""
    check_entry(model, "generation", sampler)
    n_songs, slots, chunk = int(n_songs), int(slots), int(chunk)
    if n_songs < 1 or chunk < 1:
        raise ValueError("n_songs and chunk must be >= 1")
    if n_songs > 1 << 20:
        raise ValueError("n_songs must be <= 2**20 (the sampler's key layout), got %d" % n_songs)
    if slots < 1:
        raise ValueError("slots must be >= 1, got %d" % slots)
    if isinstance(prompt, (list, tuple)):
        raise ValueError("generate_stream takes one shared (P, 6) prompt: ragged per-song prompts go in prompts=[...]")
    if prompt is not None and prompts is not None:
        raise ValueError("pass one shared prompt or per-song prompts, not both")
    A = len(word2event)
    start = time.perf_counter()
    if prompts is not None:
        heads, bar0s, caps = _check_prompts(prompts, n_songs, word2event, list(model.n_token), bar_cond, max_tokens)
    else:
        if bank is not None or prefill_rows is not None:
            raise ValueError("bank and prefill_rows belong to per-song prompts (prompts=[...])")
        if packed_prefill:
            raise ValueError("packed_prefill belongs to per-song prompts (prompts=[...]): a shared prompt is one "
                             "prefill with nothing to pad")
        heads, bar0s, caps = ([v[0]] * n_songs for v in _check_prompts(
            [INIT_CW[0] if prompt is None else prompt], 1, word2event, None, bar_cond, max_tokens))
    plan = DrawPlan(model, word2event, n_songs, where, sampler, constraints, grammar, reference, alpha, return_logprobs,
                    bar_cond, bar0s, max_tokens, heads, preferences=preferences)
    if plan.reference is not None and prompts is not None:
        raise ValueError("generate_stream blends songs that start from one snapshot: per-song prompts would need a "
                         "second bank and a second prefill schedule -- generate_batch(prompts=[...], reference=..., "
                         "alpha=...) is the supported form")
    if prompts is None:
        start = time.perf_counter()                           # the shared form's clock starts after the host's compiles
    sess = DecodeSession(model, n_songs=slots, kernel="gemm")
    sess.reset()
    seed = ops.next_seed()                                    # where generate_batch's _DeviceLoop takes it
    names = word2event["bar-beat"]
    bar_mask = [int(names[i] == "Bar") for i in range(sess.n_token[2])]       # every class named "Bar", not one id
    # the reference's pool is made after the seed: it takes none
    kw = dict(plan=DeviceDraw(plan, sess.dev, sess.shadow(plan.reference)), graph=sess.use_graph)
    if prompts is not None:
        per_entry = 4 * (sess._state.numel() // slots + sess.width + 2)
        B, bank = stream_bank_plan([len(h) for h in heads], slots, prefill_rows, bank, per_entry,
                                   torch.cuda.mem_get_info(sess.dev)[0])
        loop = _BankStreamLoop(sess, heads, n_songs, seed, bar_mask, bar_cond, bar0s, caps, B, bank, chunk,
                               prefill_rows=prefill_rows, packed=bool(packed_prefill), **kw)
    else:
        head = None if prompt is None else heads[0]
        snap_state, snap_logits = _stream_snapshot(model, head, A)
        ref_snap = None if plan.reference is None else _stream_snapshot(plan.reference, head, A)
        loop = _SnapshotStreamLoop(sess, snap_state, snap_logits, n_songs, seed, bar_mask, bar_cond, bar0s[0], caps[0],
                                   chunk, ref_snap=ref_snap, **kw)
    rows = loop.run()
    # rows are time-ordered and each song lives in one slot: a stable sort by song index keeps every song's order
    order = np.argsort(rows[:, 0], kind="stable")
    rows = rows[order]
    counts = np.bincount(rows[:, 0], minlength=n_songs)
    ends = np.cumsum(counts)
    if len(counts) != n_songs or (counts == 0).any() or rows[:, -1].sum() != n_songs or \
            not rows[ends - 1, -1].all():
        raise RuntimeError("stream output is inconsistent: %d rows, %d end bits for %d songs"
                           % (len(rows), int(rows[:, -1].sum()), n_songs))
    songs = [np.concatenate([h, d]) for h, d in zip(heads, np.split(rows[:, 1:1 + A], ends[:-1]))]
    seconds = time.perf_counter() - start
    stats = {"steps": loop.enqueued, "tokens": int(sum(len(x) for x in songs)), "drawn": int(len(rows)),
             "slot_steps": loop.enqueued * slots, "seconds": seconds, "wait_seconds": loop.wait_s,
             "graph": loop._graph is not None}
    stats.update(loop.stats())
    if log is not None:
        log("stream of %d songs on %d slots: %d tokens, %d steps" % (n_songs, slots, stats["tokens"], loop.enqueued))
    if return_logprobs:            # filtered by the same mask as the rows, in the same order: the same sort applies
        return (songs, np.split(np.concatenate(loop.lp_parts)[order], ends[:-1])), stats
    return songs, stats


def generate_stream(model, word2event, n_songs, slots=256, bar_cond=17, max_tokens=None, prompt=None, sampler="dqn",
                    chunk=128, log=None, prompts=None, bank=None, prefill_rows=None, constraints=None,
                    return_logprobs=False, grammar=None, reference=None, alpha=None, preferences=None,
                    packed_prefill=False):
    """Generate `n_songs` songs by continuous batching: a pool of `slots` GEMM-step decode slots (_StreamLoop) in which
    a slot starts the next song on the token after its song ends, and the device decides when a song ends.
    -> list of n_songs (L_i, 6) int64 arrays, in song order.

    Song k is bitwise the song k of generate_batch(model, word2event, n_songs, bar_cond, max_tokens, sampler=...) after
    the same torch.manual_seed, whatever `slots`: the GEMM step is batch invariant, every song starts from the same
    snapshot, and each draw is keyed by (torch seed, position in song, song index) -- generate_batch's (seed, step,
    song slot).  The bar rule is generate_batch's: the count starts at 1 and counts the Bar tokens of the prompt's rows
    after the first, a song ends WITH the token that opens bar `bar_cond`, or at `max_tokens` rows, prompt included
    (16384 drawn tokens without a cap).  prompt: None (INIT_CW) or one (P, 6) array every song continues.
    sampler: "dqn" or "categorical", as in generate_batch.  The host reads the songs every `chunk` tokens.

    prompts: a list of n_songs (P_i, 6) arrays, song k continues prompts[k] (_BankStreamLoop).  Song k is then bitwise
    song k of generate_batch(..., prompts=prompts, prefill="gemm"): each prompt is prefilled by the batch-invariant
    prefill into a device bank, in blocks of B consecutive songs, between chunks; a slot takes song k once its entry is
    written.  The bar count of song k starts from prompts[k] and its cap is max_tokens - len(prompts[k]).
    Defaults (stream_bank_plan): B = prefill_rows // the longest prompt, prefill_rows = PREFILL_ROWS (32768 token rows,
    about 0.8 GB of prefill activations at d_model 512); bank = the smallest multiple of B with max(2 B, 2 slots)
    entries, capped by the songs and a quarter of free device memory (one entry at d_model 512 / 12 layers / 8 heads
    is 12 x 8 x 64 x 65 x 4 B = 1.6 MB).  `bank` (a multiple of B) overrides the bank size.
    packed_prefill=True: the same blocks go through the packed prefill (CWTrunk.prefill_hidden_packed): a block's
    prompts lie end to end and no padded row is computed; B, the bank, the blocks and the songs are unchanged, bit for
    bit.  Refused without a prompt list.

    constraints, return_logprobs, grammar, reference / alpha: as in generate_batch, from the same plan (DrawPlan), and
    song k -- its (L_k - P_k, 6, 2) log-probs too -- is bitwise song k of generate_batch with the same options.  Each
    slot's draw is masked by its song's row for the slot's bar count and, under a grammar, made at the slot's position
    in its bar, which cwlt_grammar_track moves after the advance (a song's own prompt sets where it starts).  Under a
    blend a second pool of `slots` decode slots runs the reference on the same tokens and cwlt_blend_logits, keyed by
    each slot's song, writes the blended logits the sampler reads: with the shared-snapshot forms only (no prompt, or
    one shared prompt) -- per-song prompts are refused, generate_batch(prompts=[...], reference=, alpha=) takes them.
    preferences: as in generate_batch (Preference), with every form of the stream: each slot's logits are
    preferred by its song's bias row for the slot's bar count and its song's repetition state, which follows the slot
    and starts, for every song, from that song's own prompt rows."""
    return _generate_stream(model, word2event, n_songs, slots=slots, bar_cond=bar_cond, max_tokens=max_tokens,
                            prompt=prompt, sampler=sampler, chunk=chunk, log=log, prompts=prompts, bank=bank,
                            prefill_rows=prefill_rows, constraints=constraints, return_logprobs=return_logprobs,
                            grammar=grammar, reference=reference, alpha=alpha, preferences=preferences,
                            packed_prefill=packed_prefill)[0]


def _refuse_logprobs(return_logprobs, where):
    if return_logprobs:
        raise ValueError("%s samples one song on the host or its one-song loop: log-probs come from the device samplers "
                         "of generate_batch / generate_stream (return_logprobs=True), or score_songs()" % where)


def categorical_rollout(model, token_count, init=None, carry_memory=False, graph=None, prompt=None,
                        return_logprobs=False):
    """ppo_policy/inference.py:78-160 (`testing()`): start from the all-zero token, per step run the recurrent-form
    actor on the PREVIOUS token only -- the reference passes `memory=None` on every call (:106), so no state is
    carried; `carry_memory=True` is the evident intent -- and draw each attribute from Categorical(softmax(logits))
    (:121-133).  Everything stays on the device (`_DeviceLoop`); ONE host sync at the end.  Same distribution as the
    reference's torch.distributions draws, not the same random stream.  -> (token_count, 6) int64 numpy.

    prompt: a (P, 6) CW token array to continue (e.g. a slice of a dataset song): it is prefilled in one pass
    (DecodeSession.prefill), the first token is drawn from its logits on the device, and the result is the prompt
    followed by token_count drawn tokens.  Needs carry_memory=True: with the reference's fresh state per token the
    prompt would be thrown away after its last token.  return_logprobs=True is refused (score_songs scores a song)."""
    _refuse_logprobs(return_logprobs, "categorical_rollout")
    if prompt is not None and not carry_memory:
        raise ValueError("a prompt needs carry_memory=True: the reference's memory=None per step would discard it")
    if prompt is not None and init is not None:
        raise ValueError("pass a prompt or an initial token, not both")
    sess = DecodeSession(model, graph=False)
    if sess.model.training:
        raise RuntimeError("generation runs in eval() mode (ppo_policy/inference.py:96)")
    A = len(sess.n_token)
    if prompt is not None:
        prompt = np.asarray(prompt, dtype=np.int64).reshape(-1, A)
        logits = sess._prefill(prompt)
        loop = _DeviceLoop(sess, token_count, carry_memory=True, graph=graph)
        if token_count > 0:
            loop.start(logits)
            loop.run(token_count - 1)
        return np.concatenate([prompt, loop.tokens(0, token_count)[:, 0]])
    sess.tok.copy_(torch.as_tensor(np.zeros(A) if init is None else np.asarray(init), dtype=torch.int64)
                   .view(1, 1, A).to(sess.dev))
    loop = _DeviceLoop(sess, token_count, carry_memory=carry_memory, graph=graph)
    loop.run(token_count)
    return loop.tokens(0, token_count)[:, 0]


def _one_song(model, word2event, head, cnt_bar, bar_cond, max_tokens, log, session, device_sampling, chunk, prefill):
    """The body of inference_from_scratch / inference_from_prompt: `head`'s rows, then sampled rows until bar `bar_cond`
    begins or max_tokens rows.  prefill=True: head is a prompt, prefilled in one pass, the first draw from its logits;
    False: head's rows are fed through the step (on the device: its single row is the step's first input)."""
    classes = list(word2event.keys())
    sess = session or DecodeSession(model)
    sess.reset()
    is_bar = lambda row: word2event["bar-beat"][int(row[2])] == "Bar"

    def show(cp, prefix=""):
        if log is not None:
            log(prefix + " | ".join("{:15s}".format(str(word2event[k][int(cp[i])])) for i, k in enumerate(classes)))

    final_res = []
    for row in head:
        show(row)
        final_res.append(row[None, ...])
    if device_sampling:
        if not prefill and len(head) != 1:
            raise RuntimeError("device-side sampling starts from a single initial token")
        cap = max_tokens - len(head) if max_tokens is not None else 16384
        loop = _DeviceLoop(sess, cap, DeviceDraw(DrawPlan(model, word2event, 1, "inference", "dqn"), sess.dev),
                           graph=sess.use_graph)
        if prefill:
            loop.start(sess._prefill(head))
        else:
            sess.tok.copy_(torch.as_tensor(head[0], dtype=torch.int64).view(1, 1, -1).to(sess.dev))
        done = 0
        while done < cap:
            stop = min(cap, done + chunk)
            if prefill:
                loop.run(stop - loop.enqueued)                    # start() drew the first token
            else:
                loop.run(chunk)                                   # clamped to the loop's capacity: ends at `stop` too
            for next_arr in loop.tokens(done, stop)[:, 0]:
                final_res.append(next_arr[None, ...])
                show(next_arr, "bar: %d  ==" % cnt_bar)
                if is_bar(next_arr):
                    cnt_bar += 1
                if cnt_bar == bar_cond:
                    return np.concatenate(final_res)
            done = stop
        return np.concatenate(final_res)
    if prefill:
        logits = sess.prefill(head)
    else:
        for row in head:
            logits = sess.step(row)
    while True:
        next_arr = sample_cw(sess.split(logits))
        final_res.append(next_arr[None, ...])
        show(next_arr, "bar: %d  ==" % cnt_bar)
        logits = sess.step(next_arr)
        if is_bar(next_arr):
            cnt_bar += 1
        if cnt_bar == bar_cond:
            break
        if max_tokens is not None and len(final_res) >= max_tokens:
            break
    return np.concatenate(final_res)


def inference_from_scratch(model, word2event, bar_cond, max_tokens=None, log=None, session=None,
                           device_sampling=False, chunk=128, return_logprobs=False):
    """testing-no-type-cp.py:126-179: start from the Bar token, sample until `bar_cond` bars have begun.
    `max_tokens` (not in the reference, whose loop is unbounded) caps the song length.

    device_sampling=False: the reference's numpy samplers on the host (a seeded np.random reproduces its stream).
    device_sampling=True: the same per-attribute temperature / nucleus settings drawn on the device
    (`cwlt_sample_categorical`); the host only looks at the song every `chunk` tokens to count bars, and cuts it
    where the reference's loop would have stopped.  Same distribution, different random stream, ~1.2x faster (no host round trip per token).
    return_logprobs=True is refused (score_songs scores a song)."""
    _refuse_logprobs(return_logprobs, "inference_from_scratch")
    return _one_song(model, word2event, INIT_CW, 1, bar_cond, max_tokens, log, session, device_sampling, chunk, False)


def inference_from_prompt(model, word2event, prompt, bar_cond, max_tokens=None, log=None, session=None,
                          device_sampling=False, chunk=128, return_logprobs=False):
    """Continue a piece: `prompt` ((P, 6) CW tokens, e.g. a slice of a dataset song or an earlier song's .npy) is
    prefilled in one pass (DecodeSession.prefill) and the reference's sampling loop runs on from its logits.  The
    result is the prompt followed by the continuation.  The bar rule is the reference's, applied as if the prompt's
    tokens had been drawn by the loop: the count starts at 1 and counts the Bar tokens of prompt[1:], so a prompt that
    already reaches `bar_cond` is refused.  `max_tokens` caps the whole song, prompt included.
    prompt = INIT_CW reproduces inference_from_scratch.

    device_sampling=False: the reference's numpy samplers on the host, the first token drawn from the prefill logits.
    device_sampling=True: every token, the first included, drawn on the device (`cwlt_sample_categorical`, keyed by
    the loop's counter), with no host round trip between the prefill and the loop.
    return_logprobs=True is refused (score_songs scores a song)."""
    _refuse_logprobs(return_logprobs, "inference_from_prompt")
    (head,), (cnt_bar,), _ = _check_prompts([prompt], 1, word2event, None, bar_cond, max_tokens)
    return _one_song(model, word2event, head, cnt_bar, bar_cond, max_tokens, log, session, device_sampling, chunk, True)


def generate_batch(model, word2event, n_songs, bar_cond=17, max_tokens=None, prompts=None, sampler="dqn", chunk=128,
                   log=None, prefill="blas", constraints=None, return_logprobs=False, grammar=None, reference=None,
                   alpha=None, preferences=None):
    """Generate `n_songs` songs in lock-step: one `DecodeSession(n_songs=N, kernel="gemm")` (the token step's
    projections as f32 MFMA GEMMs, csrc/decode_gemm.hip) and one N-song device loop, so every weight is read once per
    token for all songs.  -> list of N (L_i, 6) int64 arrays.

    prompts=None: every song starts from INIT_CW (inference_from_scratch(device_sampling=True)); one (P, 6) array: every
    song continues it; a list of N arrays of any lengths: song i continues prompts[i] (prefilled in one ragged pass).
    The first token after a prompt is drawn on the device from the prefill logits.
    sampler="dqn": the per-attribute temperature / nucleus settings of forward_output_sampling; "categorical": the PPO
    side's plain draw.  Every `chunk` tokens the host cuts each song by the reference's bar rule (the count starts at 1
    and counts the Bar tokens of the prompt's rows after the first, the song ends WITH the token that opens bar
    `bar_cond`), or at `max_tokens` rows, prompt included.  Finished songs keep stepping until the batch ends; their
    extra rows are discarded.  The draws are keyed by (torch seed, step, song slot): song i of a batch from scratch
    is the same whatever the batch size.  prefill: the prompt prefill's kernel, DecodeSession.prefill's "blas"
    (default) or "gemm" (batch invariant: song i's start depends on prompts[i] alone -- generate_stream(prompts=...)
    gives the same songs).

    constraints: one Constraint for every song, or a list of n_songs Constraint / None entries (None: unconstrained).
    The loop keeps each song's bar count on the device (from its prompt's count; cwlt_count_bars after every draw) and
    masks each draw by the song's row for that count (cwlt_sample_categorical_masked).
    return_logprobs=True: -> (songs, logprobs), logprobs[i] the (L_i - P_i, 6, 2) f32 log-probs of song i's drawn rows
    (P_i its prompt's length; [..., 0] model, [..., 1] sampler, score_songs' layout), written by the
    device sampler itself (cwlt_sample_categorical_logp, into a float ring beside the token ring).  The songs are
    bitwise those drawn without the flag.
    grammar: a Grammar (the row grammar): the draw is cwlt_sample_categorical_grammar and
    cwlt_grammar_track keeps each song's position in its bar on the device, from where its prompt leaves it.  Combines
    with constraints (each mask row is intersected with the grammar's) and return_logprobs (lp_sampler is log q of the
    distribution each class was drawn from).
    reference, alpha: draw from the blend of the model with a reference model: with x the model's logits
    of one attribute and r the reference's, softmax(alpha x + (1 - alpha) r), i.e. pi^alpha pi_ref^(1 - alpha)
    renormalised (alpha's forms: compile_alpha).  A second session steps the reference on the same token buffer (and
    prefills the same prompts with the same `prefill` kernel), cwlt_blend_logits writes the blended logits and the
    samplers, constraints and grammar work on them as on a model's own; the seed is taken once, as without a reference,
    so alpha = 1 gives bitwise the model's songs and alpha = 0 the reference's.  Under a blend the log-prob pair is
    [..., 0] = log pi_alpha (the blended logits, temperature 1, no mask) and [..., 1] = log q of the sampler's
    distribution built on them; each model's own log-probs come from score_songs without a blend.  The reference: same
    classes, recurrent, eval(), f32, on the model's device, any width or depth.  One without the other is refused.
    preferences: one Preference for every song, or a list of n_songs Preference / None entries: soft
    terms on the logits, after the blend and before the unchanged draw (cwlt_prefer_logits) -- each song's bias row for
    its bar count, and a repetition penalty by the song's own `seen` state, which starts from its prompt's rows and is
    moved by cwlt_prefer_track after every draw.  Constraints, the grammar and the nucleus work on the preferred logits;
    under return_logprobs [..., 0] is the log-prob of the preferred logits at temperature 1 (the blend's convention).
    A preference with zero bias and no penalty gives bitwise the songs without it.
    All of these are compiled once, before the first token, into one plan (DrawPlan); None: nothing changes."""
    heads, caps, plan = _batch_setup("generate_batch", model, word2event, n_songs, bar_cond, max_tokens, prompts,
                                     sampler, chunk, prefill, constraints=constraints, logprobs=return_logprobs,
                                     grammar=grammar, reference=reference, alpha=alpha, preferences=preferences)
    return _run_batch(model, word2event, heads, caps, plan, bar_cond, int(chunk), log,
                      None if prompts is None else prefill)


def _batch_setup(where, model, word2event, n_songs, bar_cond, max_tokens, prompts, sampler, chunk, prefill, **draw):
    """generate_batch's refusals, in the one order of the entries (names, model, counts, prompts, then the plan's) ->
    (heads: every song's prompt rows, INIT_CW from scratch; caps: the rows each may draw; the DrawPlan)."""
    check_entry(model, "generation", sampler, prefill=prefill)
    n_songs = int(n_songs)
    if n_songs < 1 or int(chunk) < 1:
        raise ValueError("n_songs and chunk must be >= 1")
    heads = prompts if isinstance(prompts, (list, tuple)) else [INIT_CW[0] if prompts is None else prompts] * n_songs
    heads, bar0s, caps = _check_prompts(heads, n_songs, word2event, None, bar_cond, max_tokens)
    return heads, caps, DrawPlan(model, word2event, n_songs, where, sampler, bar_cond=bar_cond, bar0s=bar0s,
                                 max_tokens=max_tokens, heads=heads, **draw)


def _run_batch(model, word2event, heads, caps, plan, bar_cond, chunk, log, prefill):
    """generate_batch after its refusals: the songs of `plan` (one per entry of heads and caps), prefilled with kernel
    `prefill` (None: from scratch, heads are INIT_CW) -> songs, or (songs, logprobs) under plan.logprobs."""
    n_songs, return_logprobs, A = plan.n_songs, plan.logprobs, len(word2event)
    is_bar = lambda row: word2event["bar-beat"][int(row[2])] == "Bar"
    cnt_bar, cap = list(plan.bar0s), max(caps)
    sess = DecodeSession(model, n_songs=n_songs, kernel="gemm")
    sess.reset()
    ref = sess.shadow(plan.reference)                                 # before the loop: it takes the seed, this none
    loop = _DeviceLoop(sess, cap, DeviceDraw(plan, sess.dev, ref), graph=sess.use_graph, ring=chunk)
    if prefill is None:
        sess.tok.copy_(torch.as_tensor(np.tile(INIT_CW[0], (n_songs, 1)), dtype=torch.int64)
                       .view(n_songs, 1, A).to(sess.dev))
    else:
        P = max(len(p) for p in heads)
        toks = np.zeros((n_songs, P, A), dtype=np.int64)
        for i, p in enumerate(heads):
            toks[i, :len(p)] = p
        lengths = None if all(len(p) == P for p in heads) else [len(p) for p in heads]
        loop.start(sess._prefill(toks, lengths, kernel=prefill),
                   None if ref is None else ref._prefill(toks, lengths, kernel=prefill))
    drawn = [[] for _ in range(n_songs)]
    lp_drawn = [[] for _ in range(n_songs)] if return_logprobs else None
    live = set(range(n_songs))
    done = 0
    while done < cap and live:
        stop = min(cap, done + chunk)
        loop.run(stop - loop.enqueued)
        rows = loop.tokens(done, stop)                                # (stop - done, N, 6)
        lps = loop.logprobs(done, stop) if return_logprobs else None  # (stop - done, N, 6, 2)
        for i in sorted(live):
            for t in range(min(stop, caps[i]) - done):
                row = rows[t, i]
                drawn[i].append(row)
                if lp_drawn is not None:
                    lp_drawn[i].append(lps[t, i])
                if is_bar(row):
                    cnt_bar[i] += 1
                if cnt_bar[i] == bar_cond:
                    break
            if cnt_bar[i] == bar_cond or len(drawn[i]) >= caps[i]:
                live.discard(i)
        done = stop
    songs = [np.concatenate([p, np.asarray(d, dtype=np.int64).reshape(-1, A)]) for p, d in zip(heads, drawn)]
    if log is not None:
        log("batch of %d songs: %d tokens, %d steps" % (n_songs, sum(len(x) for x in songs), done))
    if return_logprobs:
        return songs, [np.asarray(l, dtype=np.float32).reshape(-1, A, 2) for l in lp_drawn]
    return songs


PARTICLE_ROWS = 4096        # most rows (songs x particles) of one generate_particles pool: the GEMM step's row limit


def particle_lineage(ancestors, rows=None):
    """Where each final row's song lived between the resampling events.  ancestors: (E, N) pool rows,
    event e's ancestor vector (row n continues row ancestors[e, n]'s song).  -> (E + 1, N) int64: entry [e, n] is the
    pool row that drew final row n's tokens of segment e, the rows after event e - 1 and up to event e; the last
    segment is the row itself, and segment e is ancestors[e] taken at segment e + 1's rows.  A row no final row
    descends from appears in no later segment.  rows (default N): the rows of a pool with no event."""
    anc = np.asarray(ancestors, dtype=np.int64)
    if anc.ndim != 2:
        anc = anc.reshape(0, int(rows or 0))
    E, N = anc.shape
    if E and ((anc < 0) | (anc >= N)).any():
        raise ValueError("ancestors must be rows of the pool, 0 .. %d" % (N - 1))
    out = np.empty((E + 1, N), dtype=np.int64)
    out[E] = np.arange(N)
    for e in range(E - 1, -1, -1):
        out[e] = anc[e][out[e + 1]]
    return out


class ParticleSet:
    """The K weighted particles generate_particles returns for one song.
    songs: K (L_i, 6) int64 arrays, prompt included; logprobs: K (L_i - P, 6, 2) f32 arrays, the (model, sampler) pairs
    of each song's drawn rows along its lineage (generate_batch(return_logprobs=True)'s layout); log_weights: (K,) f32,
    each particle's weight since the group was last resampled (the sum of lp_model - lp_sampler over those rows);
    log_evidence: the estimate of log P(the song obeys what the sampler enforces) under the target's unrestricted
    model, the resampling events' increments + logmeanexp(log_weights); per event that happened while the song had a
    live particle, ess (E,) f32, resampled (E,) bool, ancestors (E, K) int64 in-group indices (the identity where
    resampled is False) and event_log_weights (E, K) f32, the weights of the song's K pool rows as the event saw
    them.  Under a reward rewards: K (n_windows_i,) f32 arrays, the window rewards applied along each
    particle's lineage (n_windows_i = ceil((L_i - P) / reward_window)); log_weights then carry beta x them as well and
    log_evidence estimates the log of the constrained expectation of exp(beta sum r); event_rewards (R, K) f32 is what
    each reward event that happened while the song had a live particle recorded for the song's K pool rows (0 for a
    row without a live row in the window); beta: the song's own reward weight.  All three None without a
    reward."""

    def __init__(self, songs, logprobs, log_weights, log_evidence, ess, resampled, ancestors, event_log_weights=None,
                 rewards=None, event_rewards=None, beta=None):
        self.songs, self.logprobs = songs, logprobs
        self.log_weights, self.log_evidence = log_weights, float(log_evidence)
        self.ess, self.resampled, self.ancestors = ess, resampled, ancestors
        self.event_log_weights = event_log_weights
        self.rewards, self.event_rewards, self.beta = rewards, event_rewards, beta

    def weights(self):
        """The normalised weights, (K,) float64."""
        w = self.log_weights.astype(np.float64)
        w = np.exp(w - w.max())
        return w / w.sum()

    def draw(self, rng, return_index=False):
        """One song by final weight (rng: a numpy Generator) -> the song, or (song, its index)."""
        k = int(rng.choice(len(self.songs), p=self.weights()))
        return (self.songs[k], k) if return_index else self.songs[k]


def _repeat_per_song(value, n_songs, K):
    """A per-song list repeated K times entry by entry (row g K + k is song g); anything else passes through."""
    if isinstance(value, (list, tuple)) and len(value) == n_songs:
        return [v for v in value for _ in range(K)]
    return value


REWARD_FORMS = ("log_odds", "log", "score")


class WindowReward:
    """A reward callable for generate_particles(reward=) from an AIRL discriminator (dqn_policy.AIRL_model.LongFormer:
    forward(data (B, W, 6), masks (B, W)) -> (B, 1) scores D in (0, 1)); DESIGN §4.6n.
    form="log_odds" (default): log D - log(1 - D) with D clamped to [eps, 1 - eps], the AIRL reward; "log": log D (D
    clamped the same way); "score": D itself.  The transform is plain torch on the (N,) scores.

    The call runs under torch.no_grad() with every module of `disc` in eval() mode, and puts each module's mode back
    afterwards.  The reference scores its windows in train() mode, with live dropout and the score classifier's
    BatchNorm1d on batch statistics: there a window's score depends on the other windows of the batch -- here, on the
    other particles and songs of the pool -- and moves the running statistics.  In eval() every entry depends on its own
    window alone, which is what reward weights need, and the module is left as it was found."""

    def __init__(self, disc, form="log_odds", eps=1e-6):
        if form not in REWARD_FORMS:
            raise ValueError("form must be one of %s, got %r" % (", ".join(repr(f) for f in REWARD_FORMS), form))
        if not callable(disc):
            raise TypeError("disc must be a discriminator module: (windows, mask) -> (N, 1) scores")
        eps = float(eps)
        if not 0.0 < eps < 0.5:
            raise ValueError("eps must lie in (0, 0.5), got %r" % (eps,))
        self.disc, self.form, self.eps = disc, form, eps

    def __call__(self, windows, mask):
        modules = list(self.disc.modules()) if hasattr(self.disc, "modules") else []
        modes = [m.training for m in modules]
        try:
            if modules:
                self.disc.eval()
            with torch.no_grad():
                d = self.disc(windows, mask).reshape(-1).float()
        finally:
            for m, was in zip(modules, modes):
                m.training = was
        if self.form == "score":
            return d
        d = d.clamp(self.eps, 1.0 - self.eps)
        return torch.log(d) if self.form == "log" else torch.log(d) - torch.log(1.0 - d)


def _reward_spec(reward, reward_window, beta, n_songs=None):
    """generate_particles' reward refusals -> None without a reward, else (callable, W, beta).  beta: a float, or -- for
    a sequence of n_songs reward weights, one per song -- a tuple of floats."""
    if reward is not None and not callable(reward):
        raise TypeError("reward must be a callable (windows (N, W, A) int64, mask (N, W) int64) -> (N,) float32, got %r"
                        % (type(reward).__name__,))
    if int(reward_window) < 1:
        raise ValueError("reward_window must be >= 1, got %r" % (reward_window,))
    sequence = isinstance(beta, (list, tuple)) or (isinstance(beta, np.ndarray) and beta.ndim > 0)
    if sequence and reward is None:                                    # reward=None: nothing changes, beta is not used
        return None
    if sequence:
        table = tuple(float(b) for b in np.asarray(beta, dtype=np.float64).reshape(-1))
        if n_songs is not None and len(table) != int(n_songs):
            raise ValueError("beta: %d entries for %d songs (one reward weight per song, or one float for all)"
                             % (len(table), int(n_songs)))
        if not table:
            raise ValueError("beta: an empty sequence (one reward weight per song, or one float for all)")
        for i, b in enumerate(table):
            if not np.isfinite(b):
                raise ValueError("every entry of beta must be finite, got %r for song %d" % (b, i))
        beta = table
    else:
        if not np.isfinite(float(beta)):
            raise ValueError("beta must be finite, got %r" % (beta,))
        beta = float(beta)
    return None if reward is None else (reward, int(reward_window), beta)


def _beta_table(beta, dev):
    """A per-song beta (a tuple) as the f32 device table cwlt_reward_apply_keyed reads; None for one float."""
    return torch.tensor(beta, dtype=torch.float32, device=dev) if isinstance(beta, tuple) else None


def _song_beta(reward, s):
    """Song s's own reward weight under the _reward_spec `reward`."""
    return float(reward[2][s]) if isinstance(reward[2], tuple) else float(reward[2])


def _lcm(a, b):
    return int(a) * int(b) // math.gcd(int(a), int(b))


def _particle_setup(where, model, word2event, n_songs, particles, resample_every, ess, bar_cond, max_tokens, prompts,
                    sampler, chunk, prefill, constraints, grammar, reference, alpha, preferences, pool=None):
    """generate_particles' refusals, then generate_batch's for the n_songs x particles rows (_batch_setup), every
    per-song entry repeated `particles` times -> (heads, caps, plan) of the rows.  pool: the songs that share one
    pool (default: all)."""
    K = int(particles)
    if not 2 <= K <= 1024:
        raise ValueError("particles must be 2 .. 1024, got %r" % (particles,))
    pool = int(n_songs) if pool is None else int(pool)
    if pool * K > PARTICLE_ROWS:
        raise ValueError("n_songs x particles = %d x %d rows, the step takes at most %d" % (pool, K, PARTICLE_ROWS))
    if int(resample_every) < 1:
        raise ValueError("resample_every must be >= 1, got %r" % (resample_every,))
    if not 0.0 <= float(ess) <= 1.0:
        raise ValueError("ess must lie in [0, 1] (the fraction of `particles` below which a song is resampled), got %r"
                         % (ess,))
    n = int(n_songs)
    if alpha is not None and reference is not None and n >= 1:
        try:
            table = compile_alpha(alpha, n, len(word2event))
            alpha = np.repeat(table, K, axis=0) if len(table) > 1 else table
        except ValueError:
            pass                                                       # the plan refuses it, in its place
    return _batch_setup(where, model, word2event, n * K, bar_cond, max_tokens, _repeat_per_song(prompts, n, K),
                        sampler, chunk, prefill, constraints=_repeat_per_song(constraints, n, K), logprobs=True,
                        grammar=grammar, reference=reference, alpha=alpha,
                        preferences=_repeat_per_song(preferences, n, K))


def _shared_prefill(sess, toks, lengths, K, kernel="gemm"):
    """The lock-step pool's prefill, once a song: row g K of toks (N, P, A) -- every song's K rows hold
    the same prompt -- goes through the batch-invariant prefill on a scratch session of N / K songs, whose state is a
    bank of N / K entries, and cwlt_particle_refill_bank broadcasts entry g to rows g K .. g K + K - 1 of `sess` (ids
    arange(N), every row fresh) -> (N, width) logits, bitwise sess._prefill(toks, lengths, "gemm")'s, as is the state.
    kernel: "gemm" or "packed", the two batch-invariant prefills."""
    N = sess.n_songs
    scratch = DecodeSession(sess.model, n_songs=N // K, kernel="gemm", graph=False)
    scratch.reset()
    bank_logits = scratch._prefill(toks[::K], None if lengths is None else lengths[::K], kernel=kernel)
    logits = torch.empty((N, sess.width), dtype=torch.float32, device=sess.dev)
    ops.particle_refill_bank(sess._state, scratch._state, sess.n_layer, sess.s_floats, sess.z_floats, logits,
                             bank_logits, torch.ones(N, dtype=torch.int64, device=sess.dev),
                             torch.arange(N, dtype=torch.int64, device=sess.dev), K)
    sess.n_steps += scratch.n_steps
    return logits


def _run_particles(model, word2event, heads, caps, plan, particles, resample_every, ess, bar_cond, chunk, log, prefill,
                   stats=None, reward=None, share_prefill=False):
    """generate_particles after its refusals: the rows of `plan` (particles consecutive rows per song) -> ParticleSets.
    stats (a dict, optional): filled with steps, events, seconds, the rows every event moved and what one moved row
    copies per phase; a stats that comes with {"timed": True} also gets the HIP-event times of every event's resampling
    and two gather phases (and of every reward event's window kernel, callable and apply kernel).
    reward: a _reward_spec; a run that ends inside a window closes it with one partial reward event.
    share_prefill: every song's K rows hold one prompt and prefill is "gemm" or "packed": prefill it once
    (_shared_prefill);
    stats' prefilled_prompts is then the songs, not the rows."""
    N, K, R, A = plan.n_songs, int(particles), int(resample_every), len(word2event)
    cap = max(caps)
    start = time.perf_counter()
    sess = DecodeSession(model, n_songs=N, kernel="gemm")
    sess.reset()
    ref = sess.shadow(plan.reference)
    bar_mask = plan.bar_mask if plan.bar_mask is not None else plan._bar_classes()
    loop = _ParticleLoop(sess, cap, DeviceDraw(plan, sess.dev, ref), K, R, ess, bar_cond, caps, bar_mask,
                         graph=sess.use_graph, ring=chunk, timed=bool(stats and stats.get("timed")), reward=reward)
    if prefill is None:
        sess.tok.copy_(torch.as_tensor(np.tile(INIT_CW[0], (N, 1)), dtype=torch.int64).view(N, 1, A).to(sess.dev))
    else:
        P = max(len(p) for p in heads)
        toks = np.zeros((N, P, A), dtype=np.int64)
        for i, p in enumerate(heads):
            toks[i, :len(p)] = p
        lengths = None if all(len(p) == P for p in heads) else [len(p) for p in heads]
        if share_prefill:
            loop.start(_shared_prefill(sess, toks, lengths, K, prefill),
                       None if ref is None else _shared_prefill(ref, toks, lengths, K, prefill))
        else:
            loop.start(sess._prefill(toks, lengths, kernel=prefill),
                       None if ref is None else ref._prefill(toks, lengths, kernel=prefill))
    rows, lps = [], []
    done = 0
    while done < cap:
        stop = min(cap, done + chunk)
        loop.run(stop - loop.enqueued)
        rows.append(loop.tokens(done, stop))                           # (stop - done, N, 6)
        lps.append(loop.logprobs(done, stop))
        done = stop
        if bool(loop.done.all().item()):
            break
    rows, lps = np.concatenate(rows), np.concatenate(lps)
    W = None if reward is None else reward[1]
    if W is not None and done % W:                                     # the open window: rows already done add nothing
        with torch.no_grad():
            loop.reward_event(filled=done % W)
    lens, lw, log_z = loop.len.cpu().numpy(), loop.lw.cpu().numpy(), loop.log_z.cpu().numpy()
    E = loop.n_events
    h_anc = loop.h_anc[:E].cpu().numpy()
    h_ess, h_res = loop.h_ess[:E].cpu().numpy(), loop.h_res[:E].cpu().numpy()
    h_lw = loop.h_lw[:E].cpu().numpy()
    h_r = None if W is None else loop.h_r[:loop.n_rewards].cpu().numpy()
    out = particle_pool_sets(heads, rows, lps, lens, lw, log_z, h_anc, h_lw, h_ess, h_res, K, R, h_r=h_r, window=W)
    if W is not None:
        for g, ps in enumerate(out):
            ps.beta = _song_beta(reward, g)
    if log is not None:
        log("%d songs x %d particles: %d tokens, %d steps, %d resampling events"
            % (N // K, K, sum(len(x) for s in out for x in s.songs), done, E))
    if stats is not None:
        torch.cuda.synchronize(sess.dev)
        moved = (h_anc != np.arange(N)).sum(1)
        stats.update(steps=done, events=E, seconds=time.perf_counter() - start, graph=loop._graph is not None,
                     drawn=int(lens.sum()), row_bytes=loop.row_bytes, moved_rows=[int(m) for m in moved],
                     resampled_groups=[int(r.sum()) for r in h_res], groups=N // K,
                     prefilled_prompts=0 if prefill is None else N // K if share_prefill else N,
                     event_ms=_event_ms(loop.timed))
        if W is not None:
            stats.update(reward_events=loop.n_rewards, reward_ms=_event_ms(loop.reward_timed))
    return out


def _song_particle_set(head, toks, lps, lens, w, logz, anc, h_lw, h_ess, h_res, R, h_r=None, W=None):
    """One song's ParticleSet (beta aside) from its group's columns over the T steps it held the group: the rules the
    lock-step pool and the stream share; numpy only.  head (P, A): its prompt rows; toks (T, K, A),
    lps (T, K, A, 2): what the group's K rows drew; lens (K,), w (K,), logz: the final particles' drawn rows and weights
    and the events' evidence; the song's own events, event e after its row (e + 1) R: anc (E, K) in-group, h_lw (E, K),
    h_ess (E,), h_res (E,).  Row tau of final particle k was drawn by group row lineage[min(tau // R, E), k].  The event
    fields are cut to the events at which the song had a live particle, the first max(#{e : (e + 1) R < longest}, last
    hit + 1): up to its last resampling (which may have replaced the last live particle by copies of finished ones) and,
    after it, until the longest final particle ended; later events depend on the other songs of the run.
    h_r (n, K) f32, the reward events from the song's first window on, and W: window j < ceil(lens[k] / W) of particle k
    is read at the group row its lineage lived in at the song's row min((j + 1) W, T) - 1 (T: the event of a run that
    ended inside the window followed its last step); event_rewards spans the same steps, max(ceil(longest / W), (last
    hit + 1) R // W) events."""
    K, A, E = len(lens), toks.shape[2], len(anc)
    line = particle_lineage(anc, K)
    songs, logps, rewards = [], [], None if W is None else []
    for k in range(K):
        tau = np.arange(int(lens[k]))
        src = line[np.minimum(tau // R, E), k]
        songs.append(np.concatenate([head, toks[tau, src]]))
        logps.append(np.asarray(lps[tau, src], dtype=np.float32).reshape(-1, A, 2))
        if W is not None:
            j = np.arange(-(-int(lens[k]) // W))
            at = np.minimum((j + 1) * W, len(toks)) - 1
            rewards.append(np.asarray(h_r[j, line[np.minimum(at // R, E), k]], dtype=np.float32))
    longest = int(np.max(lens))
    hit = np.nonzero(h_res)[0]
    last = int(hit.max()) + 1 if len(hit) else 0
    live = max(int(np.count_nonzero((np.arange(E) + 1) * R < longest)), last)
    w = np.array(w, dtype=np.float32)
    ps = ParticleSet(songs, logps, w, float(logz) + logmeanexp(w), np.array(h_ess[:live]), np.asarray(h_res[:live]) != 0,
                     anc[:live], np.array(h_lw[:live]), rewards)
    if W is not None:
        ps.event_rewards = np.array(h_r[:max(-(-longest // W), last * R // W)], dtype=np.float32)
    return ps


def particle_pool_sets(heads, rows, logps, lens, lw, log_z, h_anc, h_lw, h_ess, h_res, particles, every, h_r=None,
                       window=None):
    """The ParticleSets of a lock-step particle pool from what the device wrote; numpy only.
    heads: the N pool rows' prompt rows, a song's K rows holding one prompt (row g K's is read); rows (T, N, A) int64,
    the rows of T steps, logps (T, N, A, 2) f32 beside them; lens (N,) int64, lw (N,) f32, log_z (G,) f32: the rows each
    pool row drew, the final weights, the events' evidence; the run's events e = 0, 1, ..., event e after step (e + 1) R:
    h_anc (E, N) int64 pool-row ancestors, h_lw (E, N) f32, h_ess (E, G) f32, h_res (E, G) int32.  K = particles, R =
    every.  Song g holds rows g K .. g K + K - 1 from step 0 on and every event of the run is one of its own:
    _song_particle_set on those columns.  h_r (n, N) f32, reward event i after step (i + 1) W, the last one after step
    T where the run ended inside a window, and window = W: the run carried a reward."""
    K, R = int(particles), int(every)
    W = None if window is None or h_r is None else int(window)
    out = []
    for g in range(len(heads) // K):
        own = slice(g * K, (g + 1) * K)
        out.append(_song_particle_set(heads[g * K], rows[:, own], logps[:, own], lens[own], lw[own], log_z[g],
                                      h_anc[:, own] - g * K, h_lw[:, own], h_ess[:, g], h_res[:, g], R,
                                      None if W is None else h_r[:, own], W))
    return out


def particle_stream_sets(rows, logps, h_anc, h_lw, h_ess, h_res, out_lw, out_len, out_logz, particles, every, n_songs,
                         head, stats=None, h_r=None, window=None):
    """The ParticleSets of a particle stream from what the device wrote; numpy only.
    rows (T, N, A + 2) int64, the ring rows of T steps: per pool row {particle id or -1, the A tokens, done}; logps
    (T, N, A, 2) f32 beside them; the run's events e = 0, 1, ..., event e after step (e + 1) R: h_anc (E, N) int64 pool-row
    ancestors, h_lw (E, N) f32, h_ess (E, G) f32, h_res (E, G) int32; what the release wrote: out_lw, out_len (n_songs K,)
    by particle id and out_logz (n_songs,).  K = particles, R = every, head: the (P, A) rows every song starts with, or
     a list of n_songs arrays, each song's own; stats then also gains gate_wait_group_steps, the steps
    groups spent without a song while songs were still unassigned (the bank's gate), kept out of idle_group_steps.
    The song of group g at step t is rows[t, g K, 0] // K; it held the group over the steps [t0, t1) that show it, t0 a
    multiple of R, and its own events j = 0, 1, ... are the run's events t0 / R + j, (t1 - t0) // R of them.  Its set is
    _song_particle_set's, the lock-step pool's rules, on the columns [t0:t1, g K .. g K + K - 1] and those events, once
    they are found consistent: row tau of final particle k was drawn at step t0 + tau.
    stats (a dict, optional) gains wait_group_steps -- steps groups spent with every particle done, waiting for the
    boundary --, idle_group_steps, steps of groups without a song, and start_steps, the step each song's first row was
    drawn at.
    h_r (the run's reward events, event i after step (i + 1) W: (n, N) f32) and window = W: the run carried
    a reward.  Songs then start at multiples of B = lcm(R, W) only, and ParticleSet.rewards and event_rewards are filled,
    by the same rules: the song's window j is the run's reward event t0 / W + j, and every window closes while the song
    holds the group.  A song that starts off a multiple of B, or a group released before its song's last window closed,
    is inconsistent.  stats then also gains boundary_wait_group_steps: the group-steps waited for a multiple of B beyond
    the next multiple of R."""
    rows = np.asarray(rows)
    T, N = rows.shape[:2]
    K, R, A = int(particles), int(every), rows.shape[2] - 2
    G = N // K
    W = None if window is None or h_r is None else int(window)
    B = R if W is None else _lcm(R, W)
    beyond = 0
    ids = rows[:, ::K, 0]
    gsong = np.where(ids >= 0, ids // K, -1)
    out, starts = [None] * int(n_songs), [None] * int(n_songs)
    per_song = isinstance(head, (list, tuple))
    if per_song and len(head) != int(n_songs):
        raise ValueError("head: %d arrays for %d songs" % (len(head), int(n_songs)))
    wait = idle = 0
    parked = []                                                          # the stretches groups spent without a song
    for g in range(G):
        col = gsong[:, g]
        cuts = np.nonzero(np.diff(col, prepend=np.int64(-2)))[0]
        for t0, t1 in zip(cuts, list(cuts[1:]) + [T]):
            s = int(col[t0])
            if s < 0:
                idle += int(t1 - t0)
                parked.append((int(t0), int(t1)))
                continue
            if t0 % B or out[s] is not None:
                raise RuntimeError("particle stream output is inconsistent: song %d starts at step %d (every %d)%s"
                                   % (s, t0, B, "" if out[s] is None else ", a second time"))
            e0 = int(t0) // R
            E = min(int(t1 - t0) // R, len(h_anc) - e0)
            span, own = slice(e0, e0 + E), slice(g * K, (g + 1) * K)
            lens = np.asarray(out_len[s * K:(s + 1) * K], dtype=np.int64)
            longest = int(lens.max())
            if longest < 1 or longest > t1 - t0:
                raise RuntimeError("particle stream output is inconsistent: song %d has lengths %s in %d steps"
                                   % (s, list(lens), t1 - t0))
            if W is not None:                       # its windows closed while it held the group: no partial one here
                w0, n_win = int(t0) // W, -(-longest // W)
                if n_win * W > t1 - t0 or w0 + n_win > len(h_r):
                    raise RuntimeError("particle stream output is inconsistent: song %d held its group for %d steps, "
                                       "its last window of %d rows closes after %d" % (s, t1 - t0, W, n_win * W))
                beyond += int(t1 - t0) - -(-longest // R) * R
            out[s] = _song_particle_set(head[s] if per_song else head, rows[t0:t1, own, 1:1 + A], logps[t0:t1, own], lens,
                                        out_lw[s * K:(s + 1) * K], out_logz[s],
                                        np.asarray(h_anc[span, own], dtype=np.int64) - g * K, h_lw[span, own],
                                        h_ess[span, g], h_res[span, g], R, None if W is None else h_r[w0:, own], W)
            wait += int(t1 - t0) - longest
            starts[s] = int(t0)
    missing = [s for s, ps in enumerate(out) if ps is None]
    if missing:
        raise RuntimeError("particle stream output is inconsistent: no rows of songs %s" % missing[:8])
    if stats is not None:
        if per_song:        # parked while songs were still unassigned: the bank's gate, not the idle tail
            last = max(starts)
            gate = sum(max(0, min(t1, last) - t0) for t0, t1 in parked)
            idle -= gate
            stats.update(gate_wait_group_steps=gate)
        stats.update(wait_group_steps=wait, idle_group_steps=idle, start_steps=starts)
        if W is not None:
            stats.update(boundary_wait_group_steps=beyond)
    return out


def _bank_choice(bank):
    """bank= of the particle entries -> None for "auto" (stream_bank_plan's choice), else the int."""
    if isinstance(bank, str):
        if bank != "auto":
            raise ValueError("bank must be \"auto\" or a number of entries, got %r" % (bank,))
        return None
    return int(bank)


def _particle_bank_refusals(n_songs, slots, prompts, bank, prefill_rows, word2event, bar_cond, max_tokens):
    """What bank= / prefill_rows= of the particle entries refuse, before the model is looked at: either of them without
    slots= and a prompt list; then, in the bank form, what _check_prompts and stream_bank_plan refuse.  -> whether the
    run is the bank form (slots=, a prompt list and bank=)."""
    listed = isinstance(prompts, (list, tuple))
    if (bank is not None or prefill_rows is not None) and (slots is None or not listed):
        raise ValueError("bank and prefill_rows belong to slots= with per-song prompts (prompts=[...])")
    if bank is None or not listed:
        return False
    heads = _check_prompts(prompts, int(n_songs), word2event, None, bar_cond, max_tokens)[0]
    stream_bank_plan([len(h) for h in heads], max(1, min(int(slots), int(n_songs))), prefill_rows, _bank_choice(bank))
    return True


def _particle_stream_refusals(n_songs, particles, slots, resample_every, chunk, prompts, reward, reward_window=50,
                              bank=None):
    """What generate_particles(slots=) refuses ahead of the lock-step path's own refusals.  Under a reward (DESIGN
    §4.6p) a group takes a song only at multiples of B = lcm(resample_every, reward_window) steps, and a chunk holds
    whole stretches of B.  bank: the opt-in to per-song prompt lists."""
    if reward is not None and int(resample_every) >= 1 and int(reward_window) >= 1 and int(chunk) >= 1:
        B = _lcm(resample_every, reward_window)
        if int(chunk) % B:
            raise ValueError("reward= with slots=: chunk (%d) must be a multiple of lcm(resample_every, reward_window) = "
                             "lcm(%d, %d) = %d -- windows of reward_window rows and resampling events of resample_every "
                             "rows share only every %d-th step as a boundary, a group takes a song only there, and a "
                             "chunk's ring half holds whole such stretches.  Choose a resample_every that divides "
                             "reward_window, or the other way round, and a chunk that both divide: for example "
                             "resample_every = 10 or 25 with reward_window = 50 and chunk = 100 (generate's chunk is "
                             "128: resample_every = 16 with reward_window = 32); or run the lock-step pool (slots=None)"
                             % (int(chunk), int(resample_every), int(reward_window), B, B))
    if isinstance(prompts, (list, tuple)) and bank is None:
        raise ValueError("slots= takes one shared (P, 6) prompt, prefilled once for all songs: per-song prompt lists "
                         "would need a prompt bank (generate_particles without slots takes them); bank=\"auto\" opts "
                         "into that bank")
    if int(slots) < 1:
        raise ValueError("slots must be >= 1, got %r" % (slots,))
    K = int(particles)
    if int(slots) * K > PARTICLE_ROWS:
        raise ValueError("slots x particles = %d x %d rows, the step takes at most %d" % (int(slots), K, PARTICLE_ROWS))
    if int(n_songs) * K > 1 << 20:
        raise ValueError("n_songs x particles must be <= 2**20 (the sampler's key layout), got %d x %d"
                         % (int(n_songs), K))
    if int(resample_every) >= 1 and int(chunk) >= 1 and int(chunk) % int(resample_every):
        raise ValueError("chunk (%d) must be a multiple of resample_every (%d): a chunk's ring half holds whole event "
                         "segments" % (int(chunk), int(resample_every)))


def _run_particle_stream(model, word2event, heads, caps, plan, n_songs, particles, slots, resample_every, ess, bar_cond,
                         chunk, log, prompt, stats=None, reward=None, bank=None, prefill_rows=None,
                         packed_prefill=False):
    """generate_particles(slots=) after its refusals: the rows of `plan` (particles consecutive rows per song), S =
    min(slots, n_songs) songs in flight -> n_songs ParticleSets.  stats (a dict, optional): steps, events, seconds (all
    of it) and run_seconds (up to the last chunk read, before the host rebuilds the sets), graph, drawn, the pool rows
    every event moved, the group-steps spent waiting for a boundary and idle at the tail.
    bank ("auto" or an int; None: the songs share `prompt`) and prefill_rows: every song continues its
    own heads[s K] from a device bank of prefilled prompts, one entry per song (stream_bank_plan with slots = groups);
    stats then also gets _PromptBank.stats and the group-steps parked by the bank's gate.
    reward: a _reward_spec; stats then also gets reward_events and the group-steps waited for a multiple
    of lcm(R, W) beyond the next multiple of R, and a stats that comes with {"timed": True} the HIP-event milliseconds
    of every reward event's window kernel, callable and apply kernel (reward_ms, as _run_particles')."""
    K, R, A = int(particles), int(resample_every), len(word2event)
    S = min(int(slots), int(n_songs))
    start = time.perf_counter()
    sess = DecodeSession(model, n_songs=S * K, kernel="gemm")
    sess.reset()
    seed = ops.next_seed()                                    # where _generate_stream and _DeviceLoop take it
    bar_mask = plan.bar_mask if plan.bar_mask is not None else plan._bar_classes()
    draw = DeviceDraw(plan, sess.dev, sess.shadow(plan.reference))
    kw = dict(reward=reward, timed=bool(stats and stats.get("timed")), plan=draw, graph=sess.use_graph)
    if bank is not None:
        song_heads = heads[::K]
        per_entry = 4 * (sess._state.numel() // (S * K) + sess.width) * (1 if plan.reference is None else 2)
        B, entries = stream_bank_plan([len(h) for h in song_heads], S, prefill_rows, _bank_choice(bank), per_entry,
                                      torch.cuda.mem_get_info(sess.dev)[0])
        loop = _ParticleBankStreamLoop(sess, song_heads, n_songs, K, R, ess, seed, bar_mask, bar_cond,
                                       list(plan.bar0s[::K]), caps[::K], B, entries, chunk, prefill_rows=prefill_rows,
                                       packed=packed_prefill, **kw)
    else:
        song_heads = heads[0]
        snap = _stream_snapshot(model, prompt, A, "gemm")
        ref_snap = None if plan.reference is None else _stream_snapshot(plan.reference, prompt, A, "gemm")
        loop = _ParticleStreamLoop(sess, snap, ref_snap, n_songs, K, R, ess, seed, bar_mask, bar_cond, plan.bar0s[0],
                                   caps[0], chunk, **kw)
    rows = loop.run()
    ran = time.perf_counter()
    lps = np.concatenate(loop.lp_parts)
    h_anc, h_lw, h_ess, h_res = (np.concatenate(p) for p in loop.hist_parts)
    more = {}
    h_r = None if reward is None else np.concatenate(loop.r_parts)
    sets = particle_stream_sets(rows, lps, h_anc, h_lw, h_ess, h_res, loop.out_lw.cpu().numpy(),
                                loop.out_len.cpu().numpy(), loop.out_logz.cpu().numpy(), K, R, n_songs, song_heads, more,
                                h_r=h_r, window=None if reward is None else reward[1])
    if reward is not None:
        for s, ps in enumerate(sets):
            ps.beta = _song_beta(reward, s)
    if log is not None:
        log("%d songs x %d particles on %d slots: %d tokens, %d steps, %d resampling events"
            % (n_songs, K, S, sum(len(x) for s in sets for x in s.songs), len(rows), len(h_anc)))
    if stats is not None:
        torch.cuda.synchronize(sess.dev)
        moved = (h_anc != np.arange(S * K)).sum(1)
        stats.update(steps=len(rows), events=len(h_anc), seconds=time.perf_counter() - start,
                     graph=loop._graph is not None, drawn=int(loop.out_len.sum().item()), row_bytes=loop.row_bytes,
                     moved_rows=[int(m) for m in moved], groups=S, wait_seconds=loop.wait_s,
                     run_seconds=ran - start, **more)
        if bank is not None:
            stats.update(loop.stats())
        if reward is not None:
            stats.update(reward_events=len(h_r), reward_ms=_event_ms(loop.reward_timed))
    return sets


def generate_particles(model, word2event, n_songs, particles, resample_every=16, ess=0.5, bar_cond=17, max_tokens=None,
                       prompts=None, sampler="dqn", chunk=128, log=None, prefill="blas", constraints=None,
                       grammar=None, reference=None, alpha=None, preferences=None, reward=None, reward_window=50,
                       beta=1.0, slots=None, bank=None, prefill_rows=None, share_prefill=None, packed_prefill=False):
    """Generate `n_songs` songs with `particles` = K weighted particles each, by sequential Monte Carlo with the device
    sampler as the proposal.  -> list of n_songs ParticleSet.

    Constraints, the row grammar and the nucleus act row by row: the sampler removes classes and renormalises, so a
    prefix the model rarely continues inside the allowed set is kept as readily as one it continues there with
    probability 0.9.  The pair the sampler writes for every drawn class gives the exact local error: lp_model -
    lp_sampler is, at temperature 1 without a nucleus, the log of the allowed mass of that draw -- the importance weight
    of the local proposal against the model restricted to allowed rows.  Here K particles per song run in lock-step in
    one pool (row g K + k is particle k of song g; one DecodeSession(n_songs x K, kernel="gemm") and the lock-step
    device loop), cwlt_particle_weigh accumulates the weights inside the captured token, and after every
    `resample_every` rows cwlt_particle_resample looks at each song: when its effective sample size (sum w)^2 / sum w^2
    is below ess x K, its particles are resampled systematically -- low-weight particles replaced by copies of
    high-weight ones -- and cwlt_particle_gather moves every per-row state of the loop (the decode state of the model
    and of a blend's reference, token, bar count, grammar position, repetition state, length, end flag, cap) from
    ancestor to descendant, through scratch.  A song ends by generate_batch's rule, decided on the device; a finished
    particle keeps its weight and takes part in later resamplings of its song.

    The target is the distribution of the logits the plan builds (blended, preferred), restricted to rows the mask and
    the grammar allow, and conditioned on the WHOLE song being allowed.  The weighted particles are exact for it in the
    limit of K at temperature 1 without a nucleus (sampler="categorical"); ParticleSet.log_evidence then estimates
    log P(the song obeys the constraints) under those logits.  With a temperature, the weights also carry the ratio of
    the model's distribution to the tempered one.  With a nucleus (sampler="dqn"), classes outside the kept set stay
    unreachable: the weights then correct only the renormalisation, not the cut.

    ess=0 never resamples: the run is generate_batch(n_songs x K, ..., return_logprobs=True) with every per-song entry
    repeated K times, bit for bit, plus the weights.  prompts, constraints, preferences (one for all, or a list of
    n_songs), alpha, grammar, reference, sampler, bar_cond, max_tokens, chunk, prefill: as in generate_batch.  Draws
    are keyed by (torch seed, step, row) and the resampling draw by (seed, event, song), so song g's set is the same
    whatever the other songs.
    share_prefill, for a list of per-song prompts: None (the default) shares one prefill among a song's K
    particles exactly when prefill="gemm" -- each prompt is prefilled once into a scratch bank of n_songs entries (a
    second one for a reference) and cwlt_particle_refill_bank broadcasts every entry to its song's K rows; the gemm
    prefill is batch invariant, so the sets are bitwise those of the K-fold prefill.  False: every row is prefilled, K
    times a prompt.  True with prefill="blas" is refused: that prefill is not batch invariant.  prefill="packed" (the
    gemm prefill without its padded rows, DecodeSession.prefill) is batch invariant too and is shared in the same way.

    slots=S (None, the default: the lock-step pool above, unchanged): the particle stream.  S songs are in
    flight on S K rows of one session and n_songs may be far larger than S: a group of K consecutive rows takes the next
    song once all its K particles have ended, at the next multiple of resample_every steps, from a snapshot refilled on
    the device (cwlt_stream_refill, cwlt_particle_release), so the pool never drains to its longest song.  Everything
    about a song is relative to that song: draws are keyed by (particle id = song K + k, position in song), the song's
    events follow its own rows R, 2 R, ... and their draw is keyed by (seed, the song's own event index, song)
    (cwlt_particle_resample_keyed).  A song's ParticleSet is therefore bit for bit the one the lock-step pool makes after
    the same torch.manual_seed, whatever `slots` and whatever the other songs.  Starts: from scratch, or from ONE shared
    (P, 6) `prompts` array, prefilled once -- not n_songs K times -- by the batch-invariant prefill (the lock-step twin
    is prefill="gemm"; `prefill` itself is not used); a list of per-song prompts is refused unless bank= opts into the
    prompt bank (below).  constraints, grammar, preferences, reference / alpha as above.  Refused with slots: per-song
    prompt lists without bank=, slots < 1, slots x particles > 4096, n_songs x particles > 2**20 (the sampler's key
    layout), a chunk that is no multiple of resample_every (a chunk's ring half holds whole event segments) and, with a
    reward, a chunk that is no multiple of lcm(resample_every, reward_window) (below).

    slots=S with prompts=[...] and bank=: song s continues prompts[s].  bank="auto" (stream_bank_plan's
    choice, with slots = the groups in flight) or a number of entries; prefill_rows: the token-row budget of one prefill
    block.  Each prompt is prefilled ONCE, by the batch-invariant prefill, into entry s % bank of a device bank (a
    second bank for a reference), in blocks between chunks as in generate_stream(prompts=[...]); a group takes song s
    only once its entry is written (cwlt_particle_release_bank: it is parked until the next boundary otherwise), starts
    from the song's own bar count and cap, and its K rows are filled from the one entry (cwlt_particle_refill_bank).  A
    song's ParticleSet -- rewards, event_rewards and beta included -- is bit for bit the lock-step pool's with
    prefill="gemm" after the same torch.manual_seed, whatever slots, bank, prefill_rows and the other songs.  bank or
    prefill_rows without slots= and a prompt list are refused, and what stream_bank_plan and the prompts' own checks
    refuse, before the model is looked at.  packed_prefill=True: the bank's blocks go through the packed prefill (as in
    generate_stream), same sets bit for bit; refused without a prompt bank.

    reward, reward_window = W, beta: reward terms in the weights.  Each particle's drawn rows (not its
    prompt) are cut into consecutive windows of W rows, the last one possibly partial; after the last row of each
    window the log-weight of every particle with a live row in it gains beta x r, r = reward(windows (N, W, 6) int64
    cuda, mask (N, W) int64 cuda)[n] -- the window's tokens, zero-padded, and a 0/1 mask of its live rows (the row that
    ends a song is live) -- and a resampling event of the same step sees it.  The target becomes the one above times
    exp(beta x sum of the song's window rewards): the optimum of KL-regularised RL with KL coefficient 1 / beta, sampled
    without a backward pass; log_evidence estimates the log of that expectation and ParticleSet.rewards records each
    lineage's rewards.  reward is any callable whose entry n depends on row n's window alone (WindowReward wraps the
    AIRL discriminator, whose window is the default 50; MetricReward is a rule-based one, a weighted sum of song
    measures such as in_chord, groove and h1 over the window); a row without a live row in the window is shown mask[n, 0] = 1
    over zero tokens and its result is discarded.  The windows live per pool row on the device (cwlt_reward_push per
    token, cwlt_reward_window and cwlt_reward_apply per event) and are gathered with every other per-row state.
    beta = 0 gives bitwise the run without a reward; reward=None enqueues nothing new.  The PPO reward model's
    per-attribute heads are left out.
    beta: one finite float, or a sequence of n_songs finite floats, song g's windows weighted by beta[g]
    (cwlt_reward_apply_keyed; a sweep of the KL coefficient over the songs of one run); ParticleSet.beta is the song's
    own value.  A list of equal entries gives the scalar's run bit for bit.
    reward= with slots=: with B = lcm(resample_every, reward_window), a group takes its next song only at
    run steps that are multiples of B -- a finished group waits for one -- so that every song's windows and events
    fall after its own rows W, 2 W, ... and R, 2 R, ...; resampling events stay at every R-th step and reward events
    follow every W-th, ahead of a resampling of the same step.  The sets, rewards and event_rewards included, are bit
    for bit the lock-step pool's.  The callable is given all slots x particles rows on the stream's own HIP stream.
    chunk must be a multiple of B: choose resample_every and reward_window so that one divides the other and both divide
    chunk, for example resample_every = 10 or 25 with reward_window = 50 and chunk = 100; the defaults (16, 50, 128: B =
    400) are refused.
    Refused, before anything runs: a reward that is not callable, reward_window < 1, a beta that is not finite or a beta
    sequence of another length than n_songs, particles
    outside 2 .. 1024, n_songs x particles > 4096 (the step's row limit), resample_every < 1, ess outside [0, 1], then
    everything generate_batch refuses."""
    spec = _reward_spec(reward, reward_window, beta, n_songs)
    if share_prefill and prefill not in ("gemm", "packed"):
        raise ValueError("share_prefill=True needs prefill=\"gemm\" (or \"packed\"): the %r prefill is not batch "
                         "invariant, so one prefill a song would not give the bits of one a particle" % (prefill,))
    if slots is not None:
        _particle_stream_refusals(n_songs, particles, slots, resample_every, chunk, prompts, reward, reward_window,
                                  bank=bank)
    banked = _particle_bank_refusals(n_songs, slots, prompts, bank, prefill_rows, word2event, bar_cond, max_tokens)
    if packed_prefill and not banked:
        raise ValueError("packed_prefill belongs to the prompt bank: slots= with per-song prompts (prompts=[...]) and "
                         "bank=")
    if slots is not None:
        heads, caps, plan = _particle_setup("generate_particles", model, word2event, n_songs, particles, resample_every,
                                            ess, bar_cond, max_tokens, prompts, sampler, chunk, prefill, constraints,
                                            grammar, reference, alpha, preferences,
                                            pool=min(int(slots), max(int(n_songs), 1)))
        return _run_particle_stream(model, word2event, heads, caps, plan, int(n_songs), particles, slots, resample_every,
                                    ess, bar_cond, int(chunk), log, None if prompts is None else heads[0], reward=spec,
                                    bank=bank if banked else None, prefill_rows=prefill_rows,
                                    packed_prefill=bool(packed_prefill))
    heads, caps, plan = _particle_setup("generate_particles", model, word2event, n_songs, particles, resample_every,
                                        ess, bar_cond, max_tokens, prompts, sampler, chunk, prefill, constraints,
                                        grammar, reference, alpha, preferences)
    share = isinstance(prompts, (list, tuple)) and prefill in ("gemm", "packed") and \
        (share_prefill is None or bool(share_prefill))
    return _run_particles(model, word2event, heads, caps, plan, particles, resample_every, ess, bar_cond, int(chunk),
                          log, None if prompts is None else prefill, reward=spec, share_prefill=share)


SCORE_BLOCK_SONGS = 1024    # most songs in one score_songs block: bounds its scratch decode state (1.6 MB a song at repo dims)


def song_bar_counts(song, word2event):
    """The bar count each row after the first of `song` ((L, 6) CW tokens) is drawn under, by the generation bar rule
    -> (L - 1,) int64: entry t (row t + 1) is 1 + the Bar tokens of song[1:t + 1], the count the prompt song[:t + 1]
    leaves (cut_prompt, generate_batch) -- the Bar token that opens a bar is drawn under the bar before it."""
    song = np.asarray(song, dtype=np.int64).reshape(-1, len(word2event))
    if len(song) < 2:
        return np.zeros(0, dtype=np.int64)
    names = word2event["bar-beat"]
    bars = np.array([names[int(r[2])] == "Bar" for r in song[1:-1]], dtype=np.int64)
    return 1 + np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(bars)])


def _score_inputs(songs, mask, n_token):
    """score_songs' song forms -> list of (L_i, A) int64 arrays, checked as prefill checks a prompt."""
    A = len(n_token)
    if isinstance(songs, (np.ndarray, torch.Tensor)) and np.ndim(songs) == 3:
        x = np.asarray(songs.cpu() if isinstance(songs, torch.Tensor) else songs, dtype=np.int64)
        if mask is None:
            out = list(x)
        else:
            m = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask)
            if m.shape != x.shape[:2]:
                raise ValueError("mask must be (n_seq, T) = %s, got %s" % (x.shape[:2], m.shape))
            out = [x[i][:int((m[i] > 0).sum())] for i in range(len(x))]
    else:
        if mask is not None:
            raise ValueError("mask belongs to the dataset-array form (songs (n_seq, T, 6))")
        out = [np.asarray(s, dtype=np.int64).reshape(-1, A) for s in songs]
    for i, s in enumerate(out):
        if s.ndim != 2 or s.shape[1] != A:
            raise ValueError("song %d must be (L, %d), got %s" % (i, A, s.shape))
        if len(s) == 0:
            raise ValueError("song %d is empty" % i)
        bad = (s < 0) | (s >= np.asarray(n_token))
        if bad.any():
            t, a = np.argwhere(bad)[0]
            raise ValueError("song %d, token %d: id %d out of range for attribute %d (%d classes)"
                             % (i, t, s[t, a], a, n_token[a]))
    return out


def _score_setup(where, model, word2event, songs, mask, sampler, kernel, **draw):
    """The refusals score_songs and policy_stats share, in the entries' one order (names, model, songs, the plan's) ->
    (_score_inputs' songs, their song_bar_counts, the DrawPlan: for the songs' largest bar count, and songs that end)."""
    check_entry(model, "scoring", sampler, kernel=kernel)
    songs = _score_inputs(songs, mask, list(model.n_token))
    bars = [song_bar_counts(x, word2event) for x in songs]
    top = max([int(b.max()) for b in bars if len(b)] + [1])
    return songs, bars, DrawPlan(model, word2event, len(songs), where, sampler, bar_cond=top + 1,
                                 max_tokens=max([len(x) for x in songs] + [1]), what="scoring", **draw)


def _song_blocks(model, songs, bars, plan, kernel, prefill_rows):
    """What score_songs and policy_stats share after _score_setup: the songs in blocks of whole songs under prefill_rows
    token rows (at most SCORE_BLOCK_SONGS songs), each prefilled on a fresh scratch state with the heads on every row --
    by `model`, and by plan.reference (a second model over the same tokens) when there is one.  A block is R rows: nb
    songs padded to the block's longest, Lb (R = nb * Lb, song i from row i * Lb), or with kernel="packed" laid end to
    end (packed_blocks: the SUMMED rows stay under prefill_rows; R = their sum, song i from row cu[i]) -- the two differ
    in where a song's rows lie, not in what is done with them.  Yields per block (songs of the block, the first row of
    each, [logits (R, n_logits) per model], targets (R, A) int64 on the device: row t of a song
    holds song[t + 1], -1 on its last row and on padding, the plan on the device (DeviceDraw), and what each row adds
    to it: its song index `key` (under constraints or a blend), bar count `bar` (under constraints) and position `beat`
    (under a grammar), else None).  Under plan.alpha the model's logits are replaced by the blend's, alpha x +
    (1 - alpha) r row by row (cwlt_blend_logits, keyed by `key`).  Under preferences the model's logits
    -- the blended ones under alpha -- are then replaced by the preferred ones (cwlt_prefer_logits with the per-row key
    and bar), penalised by the state cwlt_prefer_scan rebuilds from the block's own tokens: row t by the state after
    rows 0 .. t.  A reference's logits stay its own."""
    n_token, dev = plan.n_token, next(model.parameters()).device
    models = [model] if plan.reference is None else [model, plan.reference]
    A, n = len(n_token), len(songs)
    if n == 0:
        return
    rows_budget = PREFILL_ROWS if prefill_rows is None else int(prefill_rows)
    if rows_budget < 1:
        raise ValueError("prefill_rows must be >= 1, got %d" % rows_budget)
    draw = DeviceDraw(plan, dev)
    if draw.order is not None:
        beats = [plan.grammar.beat_states(x)[0] for x in songs]
    packed = kernel == "packed"
    if packed:
        blocks = packed_blocks([len(x) for x in songs], rows_budget, SCORE_BLOCK_SONGS)
    else:
        per = max(1, min(SCORE_BLOCK_SONGS, rows_budget // max(len(x) for x in songs)))
        blocks = [(a0, min(n, a0 + per)) for a0 in range(0, n, per)]
    for a0, z0 in blocks:
        blk = songs[a0:z0]
        nb, Lb = len(blk), max(len(x) for x in blk)
        lens = [len(x) for x in blk]
        span = lens if packed else [Lb] * nb                    # rows each song takes in the block
        starts = np.concatenate([[0], np.cumsum(span)])
        R = int(starts[-1])
        toks = np.zeros((R, A), dtype=np.int64)
        tgt = np.full((R, A), -1, dtype=np.int64)               # the last row of a song and padding: not scored
        bar = np.ones(R, dtype=np.int64)
        beat = np.full(R, -1, dtype=np.int64)
        for i, x in enumerate(blk):
            r = int(starts[i])
            toks[r:r + len(x)] = x
            tgt[r:r + len(x) - 1] = x[1:]
            bar[r:r + len(x) - 1] = bars[a0 + i]
            if draw.order is not None:
                beat[r:r + len(x) - 1] = beats[a0 + i][1:]
        lgs, key = [], None
        if draw.sched is not None or draw.alpha is not None or draw.pen is not None:
            key = torch.arange(a0, a0 + nb, device=dev).repeat_interleave(torch.as_tensor(span, device=dev),
                                                                          output_size=R)
        dbar = None if draw.sched is None and draw.bias is None else torch.as_tensor(bar).to(dev)
        dtoks = torch.as_tensor(toks).to(dev)
        cu = ops.SeqOffsets(starts.tolist(), device=dev) if packed else None
        with torch.no_grad():
            for net in models:
                enc = net.transformer_encoder
                H = enc.layers[0].attention.n_heads
                d = net.d_model // H
                memory = [[torch.zeros((nb, H, d, d), dtype=torch.float32, device=dev),
                           torch.zeros((nb, H, d), dtype=torch.float32, device=dev)] for _ in enc.layers]
                if packed:
                    lg = net.prefill_hidden_packed(dtoks, cu, memory, logits="all")
                else:
                    lg = net.prefill_hidden(dtoks.view(nb, Lb, A), memory, lens, kernel=kernel, logits="all")
                lgs.append(lg.reshape(R, -1))
            if draw.alpha is not None:
                lgs[0] = ops.blend_logits(lgs[0], lgs[1], n_token, draw.alpha, out=lgs[0], key=key)
            if draw.pen is not None:
                seen = None
                if draw.penalised:
                    seen = ops.prefer_scan_packed(dtoks, cu, n_token, draw.pen, key) if packed else \
                        ops.prefer_scan(dtoks, nb, n_token, draw.pen, key)
                lgs[0] = _prefer_token(draw, lgs[0], n_token, seen=seen, key=key, bar=dbar)
        dbeat = None if draw.order is None else torch.as_tensor(beat).to(dev)
        yield blk, starts, lgs, torch.as_tensor(tgt).to(dev), draw, key, dbar, dbeat


def score_songs(model, word2event, songs, sampler="categorical", constraints=None, kernel="gemm", mask=None,
                prefill_rows=None, grammar=None, reference=None, alpha=None, preferences=None):
    """Log-likelihoods of given songs under the recurrent form, as generation samples them.
    -> list of (L_i - 1, 6, 2) float32 arrays; row t is about song[t + 1] given song[:t + 1] (pe[0] on every row, as
    DecodeSession.step and prefill compute it): [..., 0] the model log-prob log_softmax(logits_t[a])[song[t + 1, a]]
    (temperature 1, no mask, no nucleus), [..., 1] the sampler log-prob log q(song[t + 1, a]) with q what the device
    sampler draws from: the tempered logits, the constraint mask, the nucleus kept set, renormalised; -inf outside the
    kept set or the mask.  A generated song with a P-row prompt has drawn rows song[P:]: their log-probs are rows
    P - 1 ... L - 2, what generate_batch / generate_stream(return_logprobs=True) return for it.

    songs: a list of (L_i, 6) arrays, or a dataset array (n_seq, T, 6) with mask (n_seq, T) (rows > 0 are the song).
    sampler: "dqn" (forward_output_sampling's temperature / nucleus settings) or "categorical", as in generate_batch.
    constraints: as in generate_batch; row t + 1 is masked by the song's entry for bar count song_bar_counts()[t].
    The table is compiled for the largest bar count among the songs; a constraint that could never end is not refused
    (the songs are given, not drawn).
    kernel="gemm": the batch-invariant prefill with the heads on every row (prefill_hidden(logits="all")) -- song k's
    scores are bitwise the same whatever the other songs, their order and lengths, and prefill_rows.  "blas": the
    hipBLASLt prefill, faster and not batch invariant.  Songs go in blocks of whole songs under prefill_rows token rows
    (default PREFILL_ROWS; at most SCORE_BLOCK_SONGS songs), each block on a fresh scratch state: no session is
    touched.  kernel="packed": the bits of "gemm" without the padded rows -- a block's songs lie end to end
    (CWTrunk.prefill_hidden_packed, cwlt_prefer_scan_packed), its SUMMED rows stay under prefill_rows (packed_blocks),
    and every per-row table is built per packed row.  The logits are scored by cwlt_score_categorical, the sampler's
    own kernel body, so the logits a draw came from, scored at the class it drew, give the sampler's pair bitwise.
    grammar: a Grammar: row t + 1 is scored under the row grammar (cwlt_score_categorical_grammar), its kind that of
    song[t + 1]'s own bar-beat class and its position Grammar.beat_states(song)[0][t + 1]; an ill-formed row gets -inf
    in the sampler column of the offending attribute and a finite model column.
    reference, alpha: score the songs under the blend of the model with a reference model (alpha's
    forms: compile_alpha, one row per song): both models prefill the same blocks, cwlt_blend_logits replaces the
    model's logits by alpha x + (1 - alpha) r, and [..., 0] is log pi_alpha (the blended logits, temperature 1, no
    mask), [..., 1] log q of the sampler's distribution built on them -- what generate_batch / generate_stream(
    reference=, alpha=, return_logprobs=True) return.  Each model's own log-probs come from a call without a blend.
    preferences: as in generate_batch: the logits -- the blended ones under alpha -- are replaced by the
    preferred ones before they are scored, row t with the song's bias row for song_bar_counts()[t] and the repetition
    state after song[:t + 1] (cwlt_prefer_scan, bitwise the state generation carries), so [..., 0] is the log-prob of
    the preferred logits at temperature 1 and both columns are what generation with the same preferences returns.
    Refused: unknown sampler or kernel, training mode, non-f32 activations, empty songs, ids out of range; reference
    without alpha or the reverse, and a reference policy_stats would refuse."""
    songs, bars, plan = _score_setup("score_songs", model, word2event, songs, mask, sampler, kernel,
                                     constraints=constraints, grammar=grammar, reference=reference, alpha=alpha,
                                     preferences=preferences)
    out = []
    for blk, starts, lgs, tgt, d, key, bar, beat in _song_blocks(model, songs, bars, plan, kernel, prefill_rows):
        kw = d.keywords(bar, key=key)
        if d.order is not None:
            lp = ops.score_categorical_grammar(lgs[0], plan.n_token, tgt, *d.grammar(beat), **kw)
        else:
            lp = ops.score_categorical(lgs[0], plan.n_token, tgt, **kw)
        lp = lp.view(len(tgt), -1, 2).cpu().numpy()
        out.extend(lp[r:r + len(x) - 1].copy() for r, x in zip(starts, blk))
    return out


def policy_stats(model, word2event, songs, reference=None, sampler="categorical", constraints=None, kernel="gemm",
                 mask=None, prefill_rows=None, grammar=None, alpha=None, preferences=None):
    """Entropy of the policy along given songs, and its KL against a reference model.
    -> list of (L_i - 1, 6, 2) float32 arrays, (L_i - 1, 6, 4) with `reference`; rows as in score_songs: row t is about
    the distribution of song[t + 1] given song[:t + 1].  In nats: [..., 0] H(p), p the model's softmax (temperature 1,
    no mask, no nucleus); [..., 1] H(q), q what the device sampler draws row t + 1 from (the sampler's temperature and
    nucleus, the song's constraint row, the row grammar with the kind of song[t + 1]'s own bar-beat class -- the q
    score_songs scores under); with `reference` [..., 2] KL(p || p') and [..., 3] KL(q || q'), p' and q' the same
    constructions on the reference model's logits for the same rows.  KL(q || q') is +inf where q keeps a class that
    q' does not (a nucleus only).  An ill-formed row still has its distributions -- the grammar removes classes, and
    compile_grammar refuses constraints that would leave a kind no class -- so no entry is NaN (the kernel's answer to an
    empty allowed set).
    songs, sampler, constraints, kernel, mask, prefill_rows, grammar: as in score_songs, on the same blocks of whole
    songs, bar counts and grammar positions; with kernel="gemm" a song's result is bitwise the same whatever the other
    songs, their order and prefill_rows.  reference: a second model over the same vocabulary (any width or depth):
    recurrent, in eval(), f32, on the model's device; its prefill runs on the same blocks and one cwlt_policy_stats call
    per block takes both logits tensors.
    alpha (with reference; compile_alpha's forms, one row per song): the stats of the BLENDED policy pi_alpha against
    the reference: cwlt_blend_logits replaces the model's logits by alpha x + (1 - alpha) r before the
    one cwlt_policy_stats call, so [..., 2] is KL(pi_alpha || pi_ref), the x-axis of the reward / KL frontier, and 0 at
    alpha = 0.  alpha = 1 gives the stats without it; a reference without alpha keeps that meaning.
    preferences: as in score_songs: p and q are built on the preferred logits of the model (of the blend
    under alpha).  The reference keeps its own logits, unpreferred: the KL columns then say how far the preferred policy
    has moved from the reference, the question a preference added on top of a tuned policy raises.
    Refused: what score_songs refuses, a reference that fails the conditions above, alpha without a reference."""
    songs, bars, plan = _score_setup("policy_stats", model, word2event, songs, mask, sampler, kernel,
                                     constraints=constraints, grammar=grammar, reference=reference, alpha=alpha,
                                     lone_reference=True, preferences=preferences)
    out = []
    for blk, starts, lgs, tgt, d, key, bar, beat in _song_blocks(model, songs, bars, plan, kernel, prefill_rows):
        st = ops.policy_stats(lgs[0], plan.n_token, None if reference is None else lgs[1], grammar=d.grammar(beat),
                              bar_class=tgt[:, d.bar_attr or 0].contiguous(),     # no grammar: only the sign is read
                              **d.keywords(bar, key=key))
        st = st.cpu().numpy()
        out.extend(st[r:r + len(x) - 1].copy() for r, x in zip(starts, blk))
    return out


def generate(model, word2event, n_songs=1, bar_cond=17, path_gendir="./gen_midis", write_midi=None,
             max_tokens=None, stats_path="runtime_stats.json", log=print, device_sampling=False, prompt=None,
             batch_size=None, slots=None, prompts=None, constraints=None, logprobs=False, grammar=None,
             reference=None, alpha=None, preferences=None, particles=None, resample_every=16, ess=0.5, reward=None,
             reward_window=50, beta=1.0, bank=None):
    """testing-no-type-cp.py:182-223 / agent_pretrain.py:663-706: generate `n_songs`, time them, write
    runtime_stats.json with the reference's keys.  `write_midi(res, path, word2event)` is the caller's MIDI writer
    (miditoolkit-based in the reference; out of scope here) -- when None the token array is saved as .npy.
    prompt: a (P, 6) CW token array every song continues (inference_from_prompt); None starts from scratch.
    batch_size: make the songs `batch_size` at a time with generate_batch (device sampling, one GEMM-step session per
    group); a song's time is then its group's wall time divided by the group's size.  None: one song at a time.
    slots: make the songs by continuous batching on that many decode slots (generate_stream); a song's time is then
    the stream's wall time divided by n_songs.  Not together with batch_size.
    prompts: a list of n_songs (P_i, 6) arrays, song i continues prompts[i] (not together with prompt): on the stream
    with slots, each batch_size group with its own slice of the list, or one song at a time.
    constraints, grammar, reference / alpha, preferences (generate_batch, generate_stream) and logprobs=True (their
    return_logprobs: each song's drawn-row log-probs are saved as get_<i>_logp.npy next to the song): with slots or
    batch_size only, the one-song path samples on the host.  Per-song entries are cut per batch_size group like prompts (DrawPlan.songs).
    particles=K (with batch_size; resample_every, ess: generate_particles'): each group is made by
    generate_particles with K particles a song, and each song kept is ParticleSet.draw -- one particle by final weight --
    with a numpy generator seeded from the torch seed.  None (the default): nothing changes.
    particles=K with slots=S: the songs are made by generate_particles(slots=S), the particle stream --
    S songs in flight, a group of K rows taking the next song when its particles have ended -- from scratch or from the
    one shared `prompt`, and each song kept is ParticleSet.draw as above; resample_every must divide 128, the chunk.
    bank ("auto" or a number of entries) with particles, slots and `prompts`: song i continues prompts[i]
    on the particle stream, from generate_particles' prompt bank; a prompt list without bank= is refused there.
    reward, reward_window, beta (with particles and batch_size or slots; generate_particles'): window
    rewards in the particles' weights; beta one float or a list of n_songs, cut per batch_size group.  With slots the
    chunk of 128 must be a multiple of lcm(resample_every, reward_window): for example resample_every = 16 with
    reward_window = 32 (the default window of 50 is refused there).  reward=None (the default): nothing changes."""
    if batch_size is not None and slots is not None:
        raise ValueError("pass batch_size or slots, not both")
    if reward is not None and particles is None:
        raise ValueError("reward terms act on the weights of generate_particles' particles: pass particles= (and "
                         "batch_size or slots); the one-song path, plain batches and the plain stream take no reward")
    spec = _reward_spec(reward, reward_window, beta, n_songs)
    if particles is not None and batch_size is None and slots is None:
        raise ValueError("particles run in generate_particles' lock-step pool or its stream: pass batch_size or slots "
                         "(the songs of one pool, or the songs in flight)")
    if bank is not None and (particles is None or slots is None or prompts is None):
        raise ValueError("bank belongs to slots= with particles= and per-song prompts (prompts=[...])")
    if particles is not None and slots is not None:
        if prompts is not None and bank is None:
            raise ValueError("slots= with particles= takes one shared prompt (prompt=), not per-song prompts; "
                             "bank=\"auto\" opts into the prompt bank")
        _particle_stream_refusals(n_songs, particles, slots, resample_every, 128, None, reward, reward_window)
        if prompts is not None:
            if prompt is not None:
                raise ValueError("pass one shared prompt or per-song prompts, not both")
            _particle_bank_refusals(n_songs, slots, list(prompts), bank, None, word2event, bar_cond, max_tokens)
    if (reference is not None or alpha is not None) and batch_size is None and slots is None:
        raise ValueError("the blend with a reference model runs in the device loops of generate_batch / generate_stream: "
                         "pass batch_size or slots (one song: generate_batch(n_songs=1, reference=..., alpha=...))")
    if logprobs and batch_size is None and slots is None:
        raise ValueError("log-probs come from the device samplers of generate_batch / generate_stream: pass batch_size "
                         "or slots (or score the songs with score_songs)")
    if grammar is not None and batch_size is None and slots is None:
        raise ValueError("the row grammar runs in the device samplers of generate_batch / generate_stream: pass "
                         "batch_size or slots (one song: generate_batch(n_songs=1, grammar=...))")
    if constraints is not None and batch_size is None and slots is None:
        raise ValueError("constraints run in the device samplers of generate_batch / generate_stream: pass "
                         "batch_size or slots (one song: generate_batch(n_songs=1, constraints=...))")
    if isinstance(constraints, (list, tuple)) and len(constraints) != n_songs:
        raise ValueError("constraints: %d entries for %d songs" % (len(constraints), n_songs))
    if preferences is not None and batch_size is None and slots is None:
        raise ValueError("preferences run in front of the device samplers of generate_batch / generate_stream: pass "
                         "batch_size or slots (one song: generate_batch(n_songs=1, preferences=...))")
    if isinstance(preferences, (list, tuple)) and len(preferences) != n_songs:
        raise ValueError("preferences: %d entries for %d songs" % (len(preferences), n_songs))
    if prompts is not None:
        if prompt is not None:
            raise ValueError("pass one shared prompt or per-song prompts, not both")
        if len(prompts) != n_songs:
            raise ValueError("prompts: %d arrays for %d songs" % (len(prompts), n_songs))
    song_prompt = (lambda i: prompt) if prompts is None else (lambda i: prompts[i])
    os.makedirs(path_gendir, exist_ok=True)
    song_time_list, words_len_list = [], []

    def save(sidx, res):
        if logprobs:
            res, lp = res
            np.save(os.path.join(path_gendir, "get_%d_logp.npy" % sidx), lp)
        if write_midi is not None:
            write_midi(res, os.path.join(path_gendir, "get_%d.mid" % sidx), word2event)
        else:
            np.save(os.path.join(path_gendir, "get_%d.npy" % sidx), res)

    def record(first, songs, wall, how):
        """Save a group's songs, each timed as its share of the group's wall time."""
        if logprobs:
            songs = list(zip(*songs))
        for j, res in enumerate(songs):
            save(first + j, res)
            res = res[0] if logprobs else res
            song_time_list.append(wall / len(songs))
            words_len_list.append(len(res))
            log("song %d: %d tokens in %.3f s (%s)" % (first + j, len(res), song_time_list[-1], how))

    if slots is not None and particles is not None:
        start = time.time()
        given = prompt if prompts is None else list(prompts)
        heads, caps, plan = _particle_setup("generate", model, word2event, n_songs, particles, resample_every, ess,
                                            bar_cond, max_tokens, given, "dqn", 128, "blas", constraints, grammar,
                                            reference, alpha, preferences, pool=min(int(slots), max(int(n_songs), 1)))
        sets = _run_particle_stream(model, word2event, heads, caps, plan, int(n_songs), particles, slots, resample_every,
                                    ess, bar_cond, 128, None, None if given is None else heads[0], reward=spec,
                                    bank=bank)
        rng = np.random.default_rng(ops.next_seed())             # after the run's seed, as the batch_size path
        picks = [s.draw(rng, return_index=True) for s in sets]
        songs = [p[0] for p in picks]
        if logprobs:
            songs = (songs, [s.logprobs[p[1]] for s, p in zip(sets, picks)])
        record(0, songs, time.time() - start, "particle stream on %d slots" % int(slots))
    elif slots is not None:
        start = time.time()
        songs = _generate_stream(model, word2event, n_songs, slots=int(slots), bar_cond=bar_cond, max_tokens=max_tokens,
                                 prompt=prompt, prompts=None if prompts is None else list(prompts),
                                 constraints=constraints, return_logprobs=logprobs, grammar=grammar,
                                 reference=reference, alpha=alpha, where="generate", preferences=preferences)[0]
        record(0, songs, time.time() - start, "stream on %d slots" % int(slots))
    elif batch_size is not None:
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        given = prompt if prompts is None else list(prompts)
        K = 1 if particles is None else int(particles)
        if particles is None:
            heads, caps, plan = _batch_setup("generate", model, word2event, n_songs, bar_cond, max_tokens, given, "dqn",
                                             128, "blas", constraints=constraints, logprobs=logprobs, grammar=grammar,
                                             reference=reference, alpha=alpha, preferences=preferences)
        else:
            heads, caps, plan = _particle_setup("generate", model, word2event, n_songs, particles, resample_every, ess,
                                                bar_cond, max_tokens, given, "dqn", 128, "blas", constraints, grammar,
                                                reference, alpha, preferences, pool=min(n_songs, int(batch_size)))
            rng = None
        for first in range(0, n_songs, int(batch_size)):
            rows = slice(first * K, (first + int(batch_size)) * K)
            count = len(heads[rows]) // K
            start = time.time()
            if particles is None:
                songs = _run_batch(model, word2event, heads[rows], caps[rows], plan.songs(first, count), bar_cond, 128,
                                   None, None if given is None else "blas")
            else:
                sets = _run_particles(model, word2event, heads[rows], caps[rows], plan.songs(first * K, count * K), K,
                                      resample_every, ess, bar_cond, 128, None, None if given is None else "blas",
                                      reward=spec if spec is None or not isinstance(spec[2], tuple) else
                                      spec[:2] + (spec[2][first:first + count],))
                if rng is None:                                        # after the first pool's seed: that pool is
                    rng = np.random.default_rng(ops.next_seed())      # generate_particles' with the same torch seed
                picks = [s.draw(rng, return_index=True) for s in sets]
                songs = [p[0] for p in picks]
                if logprobs:
                    songs = (songs, [s.logprobs[p[1]] for s, p in zip(sets, picks)])
            record(first, songs, time.time() - start, "batch of %d" % count)
    else:
        sess = DecodeSession(model)
        for sidx in range(n_songs):
            start = time.time()
            if song_prompt(sidx) is None:
                res = inference_from_scratch(model, word2event, bar_cond, max_tokens=max_tokens, session=sess,
                                             device_sampling=device_sampling)
            else:
                res = inference_from_prompt(model, word2event, song_prompt(sidx), bar_cond, max_tokens=max_tokens,
                                            session=sess, device_sampling=device_sampling)
            save(sidx, res)
            song_time_list.append(time.time() - start)
            words_len_list.append(len(res))
            log("song %d: %d tokens in %.3f s" % (sidx, len(res), song_time_list[-1]))
    result = {"song_time": song_time_list, "words_len_list": words_len_list,
              "ave token time:": sum(words_len_list) / sum(song_time_list),
              "ave song time": float(np.mean(song_time_list))}
    if stats_path:
        with open(stats_path, "w") as f:
            json.dump(result, f)
    return result

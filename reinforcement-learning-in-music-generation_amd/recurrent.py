"""Recurrent (one token per call) form of the causal-linear encoder, for generation.

Surface of fast_transformers' RecurrentEncoderBuilder product as the reference uses it
(dqn_policy/model.py:141-150,236-238; dqn_policy/testing-no-type-cp.py:126-179):
    h, memory = encoder(x (N, d_model), memory=memory)
with per-layer state [S (N, H, 64, 64), Zs (N, H, 64)].  Parameter names equal the training
encoder's, so checkpoints interchange.

The per-token attention step (state update + normalised read-out, elu+1 inside) is one libcwlt kernel
(csrc/recurrent.hip); LayerNorm / FFN activation reuse the training kernels; the projections are
GEMV-sized hipBLASLt calls.  Generation is outside the training hot path: a persistent
single-launch decode step across all 12 layers is the natural next step.
"""
import torch
import torch.nn as nn

from . import ops


class RecurrentTransformerEncoderLayer(nn.Module):
    def __init__(self, attention, d_model, d_ff, dropout):
        super().__init__()
        self.attention = attention
        self.linear1 = nn.Linear(d_model, d_ff)
        self.linear2 = nn.Linear(d_ff, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, state=None):
        at = self.attention
        N, H = x.shape[0], at.n_heads
        D = x.shape[1]
        with torch.no_grad():
            wqkv = torch.cat([at.query_projection.weight, at.key_projection.weight, at.value_projection.weight], 0)
            bqkv = torch.cat([at.query_projection.bias, at.key_projection.bias, at.value_projection.bias], 0)
            qkv = torch.addmm(bqkv.to(x.dtype), x, wqkv.to(x.dtype).t())            # (N, 3D)
            if state is None:
                S = torch.zeros((N, H, D // H, D // H), dtype=torch.float32, device=x.device)
                Zs = torch.zeros((N, H, D // H), dtype=torch.float32, device=x.device)
            else:
                S, Zs = state
                if len(S) != N:
                    raise ValueError("The batch size changed during iteration")
            a = ops.recurrent_cla_step(qkv, S, Zs, H)                                # state updated in place
            p = self.dropout.p if self.training else 0.0
            o = at.out_projection(a)
            _, x1, _, _ = ops.ln_fwd(x.contiguous(), o, ops._f32(self.norm1.weight), ops._f32(self.norm1.bias),
                                     self.norm1.eps, p, ops.next_seed() if p > 0 else 0, save_s=False)
            h = torch.mm(x1, self.linear1.weight.to(x.dtype).t())
            g = ops.gelu_fwd(h, ops._f32(self.linear1.bias), p, ops.next_seed() if p > 0 else 0)
            y = self.linear2(g)
            _, x2, _, _ = ops.ln_fwd(x1, y, ops._f32(self.norm2.weight), ops._f32(self.norm2.bias), self.norm2.eps, p,
                                     ops.next_seed() if p > 0 else 0, save_s=False)
        return x2, [S, Zs]

    def prefill(self, x, state, lengths=None):
        """A whole prompt per sequence in one pass: x (N, L, D); state [S (N, H, 64, 64), Zs (N, H, 64)] advanced IN
        PLACE as L calls of forward() would (only the first lengths[n] rows of sequence n count).  The row-wise ops are
        forward()'s own, on N*L rows; only the per-token attention step becomes ops.cla_fwd_state.  -> (N, L, D)."""
        at = self.attention
        N, L, D = x.shape
        H = at.n_heads
        if self.training:
            raise RuntimeError("prefill runs in eval() mode")
        S, Zs = state
        with torch.no_grad():
            wqkv = torch.cat([at.query_projection.weight, at.key_projection.weight, at.value_projection.weight], 0)
            bqkv = torch.cat([at.query_projection.bias, at.key_projection.bias, at.value_projection.bias], 0)
            x = x.reshape(N * L, D).contiguous()
            qkv = torch.addmm(bqkv.to(x.dtype), x, wqkv.to(x.dtype).t()).view(N, L, 3, H, D // H)
            # padded rows are never written by the scan: zero them so that everything downstream stays finite
            a = (torch.zeros if lengths is not None else torch.empty)((N, L, H, D // H), dtype=x.dtype,
                                                                      device=x.device)
            ops.cla_fwd_state(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], S, Zs, lengths, out=a)
            o = at.out_projection(a.view(N * L, D))
            _, x1, _, _ = ops.ln_fwd(x, o, ops._f32(self.norm1.weight), ops._f32(self.norm1.bias), self.norm1.eps,
                                     0.0, 0, save_s=False)
            h = torch.mm(x1, self.linear1.weight.to(x.dtype).t())
            g = ops.gelu_fwd(h, ops._f32(self.linear1.bias))
            y = self.linear2(g)
            _, x2, _, _ = ops.ln_fwd(x1, y, ops._f32(self.norm2.weight), ops._f32(self.norm2.bias), self.norm2.eps,
                                     0.0, 0, save_s=False)
        return x2.view(N, L, D)


class RecurrentTransformerEncoder(nn.Module):
    def __init__(self, layers, norm_layer=None):
        super().__init__()
        self.layers = nn.ModuleList(layers)
        self.norm = norm_layer

    def forward(self, x, state=None, memory=None):
        if not x.is_cuda:
            raise RuntimeError("rlmg_amd encoder runs on the GPU only (no CPU fallback)")
        if state is None:
            state = memory
        if state is None:
            state = [None] * len(self.layers)
        state = list(state)
        for i, layer in enumerate(self.layers):
            x, state[i] = layer(x, state[i])
        if self.norm is not None:
            with torch.no_grad():
                x = ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        return x, state

    def prefill(self, x, state, lengths=None, kernel="blas", last=None, heads=None, rows=None, all_rows=False):
        """x (N, L, D) prompt rows (embedded, positional row added) -> (N, L, D) final-norm outputs; `state` (a list of
        [S, Zs] per layer, as forward() takes it) advanced IN PLACE over each sequence's first lengths[n] rows
        (lengths: (N) int32 device tensor, None = all L).  f32 only: the result is what L calls of forward() return,
        row by row, so the projections run in full f32 (no TF32 / XF32).

        kernel="gemm": batch invariant -- sequence n's state and outputs are bitwise the same whatever the other
        sequences, their lengths, L and `rows`.  Every projection is a cwlt_decode_gemm chained as the GEMM decode step
        chains it (cwlt_decode_step_rows: a layer's norm2 is the LayerNorm prologue of the next layer's QKV, norm1 that of
        linear1; residual and GELU in the epilogue), at most `rows` (<= 4096, default 4096) rows per call, and the scan
        is one workgroup per (sequence, head) over the sequence's own chunks (segments=1).  Only row last[n] ((N) int64
        device tensor, None = all L - 1) of each sequence goes through the final norms, as the prologue of the stacked
        heads GEMM heads = (w (n_out, D), b (n_out)).  -> (hidden (N, D), logits (N, n_out)).
        all_rows=True (gemm): the heads GEMM, with the same two LayerNorms as its prologue, runs on every row of every
        sequence instead (padded rows included; `last` is ignored) -> (None, logits (N, L, n_out))."""
        if kernel not in ("blas", "gemm"):
            raise ValueError("kernel must be 'blas' or 'gemm', got %r" % (kernel,))
        if kernel == "gemm":
            self._check_prefill(x, state)
            if heads is None:
                raise ValueError("the gemm prefill ends in the heads GEMM: pass heads=(weight, bias)")
            return self._prefill_gemm(x, state, lengths, last, heads, 4096 if rows is None else int(rows), all_rows)
        if last is not None or heads is not None or rows is not None or all_rows:
            raise ValueError("last, heads, rows and all_rows belong to kernel='gemm'")
        if not x.is_cuda:
            raise RuntimeError("rlmg_amd encoder runs on the GPU only (no CPU fallback)")
        if x.dtype != torch.float32:
            raise RuntimeError("prefill computes in f32 (got %s activations)" % x.dtype)
        if state is None or len(state) != len(self.layers) or any(s is None for s in state):
            raise ValueError("prefill needs one [S, Zs] state per layer, updated in place")
        N = x.shape[0]
        for S, Zs in state:
            if len(S) != N or len(Zs) != N:
                raise ValueError("state holds %d sequences, the prompt batch %d" % (len(S), N))
        tf32 = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        try:
            for layer, st in zip(self.layers, state):
                x = layer.prefill(x, st, lengths)
            if self.norm is not None:
                with torch.no_grad():
                    x = ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        finally:
            torch.backends.cuda.matmul.allow_tf32 = tf32
        return x

    def _check_prefill(self, x, state):
        if not x.is_cuda:
            raise RuntimeError("rlmg_amd encoder runs on the GPU only (no CPU fallback)")
        if x.dtype != torch.float32:
            raise RuntimeError("prefill computes in f32 (got %s activations)" % x.dtype)
        if state is None or len(state) != len(self.layers) or any(s is None for s in state):
            raise ValueError("prefill needs one [S, Zs] state per layer, updated in place")
        for S, Zs in state:
            if len(S) != x.shape[0] or len(Zs) != x.shape[0]:
                raise ValueError("state holds %d sequences, the prompt batch %d" % (len(S), x.shape[0]))

    def prefill_packed(self, x, state, cu, heads, rows=None, all_rows=False):
        """prefill(kernel="gemm") without padded rows: x (R, D) the embedded rows of songs laid end to end, cu an
        ops.SeqOffsets (song s = rows [cu[s], cu[s + 1])), `state` one [S (n_songs, H, 64, 64), Zs (n_songs, H, 64)] per
        layer, advanced IN PLACE.  Every launch but the scan is row-wise and the scan (ops.cla_fwd_state_packed) runs
        each song from its own row 0, so a song's state, hidden row and logits are bitwise those of kernel="gemm".
        -> (hidden (n_songs, D), logits (n_songs, n_out)) of every song's last row, or with all_rows=True (None, logits
        (R, n_out)).  No host sync: the last rows are gathered at cu.dev[1:] - 1 on the device."""
        if not isinstance(cu, ops.SeqOffsets):
            raise TypeError("prefill_packed takes the songs' offsets as an ops.SeqOffsets")
        if x.dim() != 2:
            raise ValueError("prefill_packed takes packed rows (R, D), got %s" % (tuple(x.shape),))
        cu.check_rows(x.shape[0])
        if not x.is_cuda:
            raise RuntimeError("rlmg_amd encoder runs on the GPU only (no CPU fallback)")
        if x.dtype != torch.float32:
            raise RuntimeError("prefill computes in f32 (got %s activations)" % x.dtype)
        if state is None or len(state) != len(self.layers) or any(s is None for s in state):
            raise ValueError("prefill needs one [S, Zs] state per layer, updated in place")
        for S, Zs in state:
            if len(S) != cu.n_songs or len(Zs) != cu.n_songs:
                raise ValueError("state holds %d sequences, the packed rows %d songs" % (len(S), cu.n_songs))
        if heads is None:
            raise ValueError("the packed prefill ends in the heads GEMM: pass heads=(weight, bias)")
        return self._prefill_gemm(x, state, None, None, heads, 4096 if rows is None else int(rows), all_rows, cu=cu)

    def _prefill_gemm(self, x, state, lengths, last, heads, rows, all_rows=False, cu=None):
        """cu (ops.SeqOffsets): the packed form -- x is (R, D), the scan takes the offsets and `lengths`, `last` are
        unused; everything else is the same row-wise chain over M = R rows."""
        if not 1 <= rows <= 4096:
            raise ValueError("rows must be in [1, 4096] (cwlt_decode_gemm's rows per call), got %d" % rows)
        if cu is not None:
            (M, D), N, L = x.shape, cu.n_songs, None
        else:
            N, L, D = x.shape
            M = N * L
        H = self.layers[0].attention.n_heads
        d = D // H
        F = self.layers[0].linear1.out_features
        eps = self.layers[0].norm1.eps
        for layer in self.layers:
            if layer.norm1.eps != eps or layer.norm2.eps != eps or (self.norm is not None and self.norm.eps != eps):
                raise RuntimeError("the gemm prefill needs one LayerNorm eps for the whole encoder")
        f = ops._f32
        pair = lambda nrm: (f(nrm.weight), f(nrm.bias))

        def gemm(w, b, src, dst, ln=None, res=None, act=None, normed=None, ln2=None):
            for a in range(0, M, rows):
                z = min(M, a + rows)
                ops.decode_gemm(w, b, src[a:z], ln=ln, ln2=ln2, eps=eps, res=None if res is None else res[a:z],
                                act=act, out=dst[a:z], normed=None if normed is None else normed[a:z])

        dev = x.device
        new = lambda n: torch.empty((M, n), dtype=torch.float32, device=dev)
        x0 = x.reshape(M, D).contiguous()
        xn, qkv, s1, x1, hh, s2 = new(D), new(3 * D), new(D), new(D), new(F), new(D)
        if cu is not None:
            a = torch.empty((M, H, d), dtype=torch.float32, device=dev)   # every row is live
        else:
            a = torch.zeros((N, L, H, d), dtype=torch.float32, device=dev)    # padded rows stay zero: never written
        with torch.no_grad():
            for i, (layer, (S, Zs)) in enumerate(zip(self.layers, state)):
                at = layer.attention
                wqkv = torch.cat([f(at.query_projection.weight), f(at.key_projection.weight),
                                  f(at.value_projection.weight)], 0)
                bqkv = torch.cat([f(at.query_projection.bias), f(at.key_projection.bias), f(at.value_projection.bias)])
                prev = self.layers[i - 1] if i else None
                gemm(wqkv, bqkv, s2 if prev else x0, qkv, ln=pair(prev.norm2) if prev else None,
                     normed=xn if prev else None)
                q = qkv.view(a.shape[:-2] + (3, H, d))
                ops.cla_fwd_state(q.select(-3, 0), q.select(-3, 1), q.select(-3, 2), S, Zs, lengths, out=a, segments=1,
                                  cu=cu)
                gemm(f(at.out_projection.weight), f(at.out_projection.bias), a.view(M, D), s1,
                     res=xn if prev else x0)
                gemm(f(layer.linear1.weight), f(layer.linear1.bias), s1, hh, ln=pair(layer.norm1), act="gelu",
                     normed=x1)
                gemm(f(layer.linear2.weight), f(layer.linear2.bias), hh, s2, res=x1)
            if all_rows:
                w, b = f(heads[0]), f(heads[1])
                logits = torch.empty((M, w.shape[0]), dtype=torch.float32, device=dev)
                gemm(w, b, s2, logits, ln=pair(self.layers[-1].norm2),
                     ln2=pair(self.norm) if self.norm is not None else None)
                return None, logits if cu is not None else logits.view(N, L, w.shape[0])
            if cu is not None:
                top = s2[cu.dev[1:].long() - 1]                                    # every song's last row
            else:
                if last is None:
                    last = torch.full((N,), L - 1, dtype=torch.int64, device=dev)
                top = s2.view(N, L, D)[torch.arange(N, device=dev), last]      # (N, D): a gather, exact
            ln2 = pair(self.norm) if self.norm is not None else None
            w, b = f(heads[0]), f(heads[1])
            logits = torch.empty((N, w.shape[0]), dtype=torch.float32, device=dev)
            hidden = torch.empty((N, D), dtype=torch.float32, device=dev)
            for a in range(0, N, rows):
                z = min(N, a + rows)
                ops.decode_gemm(w, b, top[a:z], ln=pair(self.layers[-1].norm2), ln2=ln2, eps=eps, out=logits[a:z],
                                normed=hidden[a:z])
        return hidden, logits

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

    def prefill(self, x, state, lengths=None):
        """x (N, L, D) prompt rows (embedded, positional row added) -> (N, L, D) final-norm outputs; `state` (a list of
        [S, Zs] per layer, as forward() takes it) advanced IN PLACE over each sequence's first lengths[n] rows
        (lengths: (N) int32 device tensor, None = all L).  f32 only: the result is what L calls of forward() return,
        row by row, so the projections run in full f32 (no TF32 / XF32)."""
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

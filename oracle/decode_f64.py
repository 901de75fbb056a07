"""f64 reference of token-by-token generation: what DecodeSession.step returns after each token of a given song, all rows
at once (TEST INFRASTRUCTURE; see oracle/__init__.py).

The recurrent form of the model, teacher-forced: row t of song n is the model's output after tokens[n, :t + 1] went
through it one by one, state carried.  A causal encoder gives every row in one pass, so this is oracle/step_f64.py's
encoder (encoder_forward with p = 0: the post-LN layer, causal linear attention from oracle/cla.py, exact-erf GELU,
LayerNorm eps 1e-5) behind the recurrent path's front:

    e = in_linear(cat_f(lut_f(x_f) * sqrt(d_f))) + pe[0]      pe[0] on EVERY row: the recurrent path squeezes a
                                                               length-1 sequence, so each token sits at position 0
    h = final_norm(layers(e));  logits = cat_f(proj_f(h))      the six heads stacked in attribute order

and the state a layer holds after lengths[n] tokens, key-feature-major as the kernels keep it:

    S[n, h, d, m] = sum_{t < lengths[n]} phi(k[n, t, h, d]) v[n, t, h, m]        Z[n, h, d] = sum_t phi(k[n, t, h, d])

Parameters are taken by state-dict name (model.state_dict(): the positional table is its buffer "pos_emb.pe"), so the
same functions serve dqn_policy.model.LinearTransformer and ppo_policy.model.Actor_Transformer.  Plain torch, device
agnostic: f64 on the CPU by default, f64 on a GPU when `device` names one; `dtype=torch.float32` evaluates the same chain
in f32, which is how the tests measure the rounding floor of the chain itself.  Songs are evaluated in slabs of whole
songs, so memory does not grow with N.  Rows at or past lengths[n] are padding: their outputs mean nothing, and no
padding row reaches a state.

wrong= builds the reference with exactly ONE wrong ingredient, for tests to show that their comparison would notice:
    "pe_t"         pe[t] instead of pe[0] on row t
    "gelu_tanh"    tanh-form GELU instead of erf
    "drop32"       the token at index 32 of every song left out of the state (S and Z) of every layer
    "song_stride"  in the last layer, song n reads song n + 1's state (all songs but the last)
    "z_raw"        Z accumulated from raw k instead of phi(k)
"""
import math

import torch
import torch.nn.functional as F

from . import cla, step_f64

ATTRS = step_f64.ATTRS
WRONG = ("pe_t", "gelu_tanh", "drop32", "song_stride", "z_raw")
SLAB_ROWS = 8192
U = 2.0 ** -24                  # unit roundoff of f32


def row_bound(n_layers):
    """Bound on |got - ref|_2 / |ref|_2 of one logits or hidden row of an f32 evaluation (tests/test_decode_f64_gpu.py
    derives it): 10 roundings per layer, 5 around the layers, each of relative size u, independent, times 4."""
    return 4 * (10 * n_layers + 5) ** 0.5 * U


def state_bound(t, layer):
    """The same for S and Z of one (song, head) of layer `layer` (from 0) after t tokens, relative to its own norm:
    t / 6 for t adds in sequence, 2 (14 + 10 layer) / t for the roundings k and v carry (the front counted as a layer's
    10, the layers before, the projection and the embedding scale, pe and phi), 1 for the product."""
    return 4 * (t / 6 + 2 * (14 + 10 * layer) / t + 1) ** 0.5 * U


def _cla_parts(Q, Kn, Kd, v, eps, chunk=64):
    """Causal linear attention on given features, cla.cla_chunked's arithmetic with the numerator's keys Kn (they build
    S) apart from the normaliser's Kd (they build Z): out_t = sum_{s<=t} (Q_t . Kn_s) v_s / (sum_{s<=t} Q_t . Kd_s + eps)."""
    N, L, H, E = Q.shape
    S = Q.new_zeros((N, H, E, v.shape[-1]))
    z = Q.new_zeros((N, H, E))
    outs = []
    for c0 in range(0, L, chunk):
        sl = slice(c0, c0 + chunk)
        Qc, Knc, Kdc, Vc = Q[:, sl], Kn[:, sl], Kd[:, sl], v[:, sl]
        C = Qc.shape[1]
        tril = torch.tril(torch.ones(C, C, dtype=Q.dtype, device=Q.device))
        An = torch.einsum("nlhe,nshe->nhls", Qc, Knc) * tril
        Ad = torch.einsum("nlhe,nshe->nhls", Qc, Kdc) * tril
        num = torch.einsum("nhls,nshm->nlhm", An, Vc) + torch.einsum("nlhe,nhem->nlhm", Qc, S)
        den = Ad.sum(-1).permute(0, 2, 1) + torch.einsum("nlhe,nhe->nlh", Qc, z) + eps
        outs.append(num / den[..., None])
        S = S + torch.einsum("nshe,nshm->nhem", Knc, Vc)
        z = z + Kdc.sum(1)
    return torch.cat(outs, 1)


def _state(Kn, Kd, v, lengths, sequential):
    """[S (N, H, E, M), Z (N, H, E)] after each song's first lengths[n] tokens.  sequential: one token at a time, as the
    recurrent form adds them (the order matters only below f64)."""
    N, L = Kn.shape[:2]
    live = (torch.arange(L, device=Kn.device)[None, :] < lengths[:, None]).to(Kn.dtype)[..., None, None]
    Kn, Kd = Kn * live, Kd * live
    if not sequential:
        return [torch.einsum("nthd,nthm->nhdm", Kn, v), Kd.sum(1)]
    S = Kn.new_zeros((N,) + Kn.shape[2:] + (v.shape[-1],))
    Z = Kn.new_zeros((N,) + Kn.shape[2:])
    for t in range(L):
        S += Kn[:, t, :, :, None] * v[:, t, :, None, :]
        Z += Kd[:, t]
    return [S, Z]


def _attention(wrong, last, lengths, states, sequential):
    """attn(q, k, v, eps) of one layer (step_f64.layer_forward's hook); appends the layer's state to `states` (a list,
    None: no state wanted)."""
    def attn(q, k, v, eps):
        K = cla.feature_map(k)
        Kn, Kd, vv = K, K, v
        if wrong == "drop32" and k.shape[1] > 32:
            Kn = Kd = torch.cat([K[:, :32], torch.zeros_like(K[:, 32:33]), K[:, 33:]], 1)
        elif wrong == "z_raw":
            Kd = k
        elif wrong == "song_stride" and last and k.shape[0] > 1:
            nxt = torch.arange(1, k.shape[0] + 1, device=k.device).clamp_(max=k.shape[0] - 1)
            Kn = Kd = K[nxt]
            vv = v[nxt]
        if Kn is K and Kd is K:
            out = cla.cla_reference(q, k, v, eps)
        else:
            out = _cla_parts(cla.feature_map(q), Kn, Kd, vv, eps)
        if states is not None:
            states.append(_state(Kn, Kd, vv, lengths, sequential))
        return out
    return attn


def decode_f64(params, tokens, n_token, n_layers, n_heads, lengths=None, wrong=None, slab=None, state=True,
               dtype=torch.float64, device=None, sequential_state=False):
    """-> (logits (N, L, sum n_token), hidden (N, L, d_model), [[S (N, H, E, E), Z (N, H, E)] per layer] or None), in
    `dtype` on `device`.  params: name -> tensor (a state dict); tokens (N, L, 6) integer; lengths: N values in [1, L]
    (None: all L); slab: songs per evaluation (None: as many as fit SLAB_ROWS token rows)."""
    if wrong is not None and wrong not in WRONG:
        raise ValueError("wrong must be one of %s, got %r" % (", ".join(WRONG), wrong))
    tokens = torch.as_tensor(tokens)
    device = tokens.device if device is None else torch.device(device)
    tokens = tokens.to(device=device, dtype=torch.int64)
    N, L, A = tokens.shape
    if A != len(n_token):
        raise ValueError("tokens carry %d attributes, n_token %d" % (A, len(n_token)))
    P = {k: v.detach().to(device=device, dtype=dtype) for k, v in params.items() if torch.is_floating_point(v)}
    D = P["in_linear.weight"].shape[0]
    pe = P["pos_emb.pe"].reshape(-1, D)
    lens = torch.full((N,), L, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths, dtype=torch.int64)
    if lens.shape != (N,) or (lens < 1).any() or (lens > L).any():
        raise ValueError("lengths must be %d values in [1, %d]" % (N, L))
    lens = lens.to(device)
    slab = max(1, SLAB_ROWS // L) if slab is None else int(slab)
    if wrong == "song_stride":
        slab = N                                    # a song's neighbour must sit in its slab
    act = (lambda h: F.gelu(h, approximate="tanh")) if wrong == "gelu_tanh" else F.gelu
    tables = [P["word_emb_%s.lut.weight" % a] for a in ATTRS[:A]]
    logits, hidden, states = [], [], []
    with torch.no_grad():
        for n0 in range(0, N, slab):
            tok = tokens[n0:n0 + slab]
            embs = torch.cat([t[tok[..., i]] * math.sqrt(t.shape[1]) for i, t in enumerate(tables)], -1)
            e = F.linear(embs, P["in_linear.weight"], P["in_linear.bias"]) + (pe[:L] if wrong == "pe_t" else pe[0])
            st = [] if state else None
            h = step_f64.encoder_forward(
                e, P, n_layers, n_heads, 0.0, [0] * (3 * n_layers), pre="transformer_encoder.", act=act,
                attn=lambda i: _attention(wrong, i == n_layers - 1, lens[n0:n0 + slab], st, sequential_state))
            logits.append(torch.cat([F.linear(h, P["proj_%s.weight" % a], P["proj_%s.bias" % a]) for a in ATTRS[:A]], -1))
            hidden.append(h)
            states.append(st)
    mem = None
    if state:
        mem = [[torch.cat([s[i][j] for s in states]) for j in (0, 1)] for i in range(n_layers)]
    return torch.cat(logits), torch.cat(hidden), mem


def logits_f64(params, tokens, n_token, n_layers, n_heads, lengths=None, **kw):
    """tokens (N, L, 6) -> (logits (N, L, sum n_token), hidden rows (N, L, d_model), final norm applied)."""
    lg, h, _ = decode_f64(params, tokens, n_token, n_layers, n_heads, lengths, state=False, **kw)
    return lg, h


def state_f64(params, tokens, n_token, n_layers, n_heads, lengths=None, **kw):
    """-> per layer [S (N, H, 64, 64), Z (N, H, 64)] after lengths[n] tokens, for comparison with DecodeSession.memory."""
    return decode_f64(params, tokens, n_token, n_layers, n_heads, lengths, state=True, **kw)[2]


def row_rel(got, ref):
    """|got - ref|_2 / |ref|_2 over the last axis, in f64: the per-row measure of the generation tests."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1)


def state_rel(got, ref):
    """Per (song, head): |got - ref| / |ref| of S (N, H, E, M) or Z (N, H, E), each relative to its own norm."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = (got - ref).flatten(2).norm(dim=-1)
    return d / ref.flatten(2).norm(dim=-1)

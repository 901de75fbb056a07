"""f64 reference of the encoder stack and of the CW train step WITH the kernels' dropout (TEST INFRASTRUCTURE; see
oracle/__init__.py).

Plain, device-agnostic torch: it runs on the CPU and in f64 on the GPU.  The arithmetic is oracle/ft_encoder.py's post-LN
layer (causal linear attention from oracle/cla.py, exact-erf GELU, LayerNorm eps 1e-5) and oracle/cw_model.py's front and
heads, written as functions of a flat parameter dict keyed by the product modules' own parameter names, with the dropout
sites made explicit (oracle/dropout.py: the kernels' keep mask and scale):

    front    e = dropout(in_linear(cat_f(lut_f(x_f) * sqrt(d_f))) + pe[:T])                           seed: front
    layer i  s1 = x + dropout(out_proj(CLA(q, k, v)))                x1 = LN1(s1)                     seeds[3i]
             g  = dropout(gelu(linear1(x1)))                                                           seeds[3i + 1]
             s2 = x1 + dropout(linear2(g))                            out = LN2(s2)                    seeds[3i + 2]
    final norm, the six heads, masked CE: loss_f = sum(mask * nll_f) / sum(mask)

Each site's mask indexes the site's whole (rows, cols) tensor, rows = N * T in sequence-major order.  Every op is local to
one sequence except the parameter gradients and the loss denominator, so the batch is evaluated in SLABS of whole
sequences: forward and autograd backward per slab (each slab's rows keep their global row offset for the masks, the
global masked-token count divides every slab's loss), parameter gradients summed in f64 across slabs.  Peak memory then
does not grow with the batch.

`drop` (default oracle.dropout.dropout, signature (x, p, seed, row0)) is the dropout every site applies: tests hand in a
deliberately wrong one to show that their comparisons would notice.
"""
import math

import torch
import torch.nn.functional as F

from . import cla, dropout

LN_EPS = 1e-5
ATTRS = ("tempo", "chord", "barbeat", "pitch", "duration", "velocity")


def layer_forward(x, P, pre, n_heads, p, seeds, row0=0, drop=dropout.dropout, taps=None, attn=cla.cla_reference,
                  act=F.gelu):
    """One post-LN encoder layer: x (n, L, D) -> (n, L, D).  P[pre + name]: the layer's parameters; seeds: its 3 sites'.
    taps: a list that receives (q, k, attention output), their gradients retained (normaliser_gains).
    attn(q, k, v, eps) and act(h): the attention and the FFN activation (oracle/decode_f64.py hands in others)."""
    n, L, D = x.shape
    x2 = x.reshape(n * L, D)
    at = pre + "attention."

    def proj(name, t):
        return F.linear(t, P[at + name + ".weight"], P[at + name + ".bias"])

    q, k, v = (proj(nm, x2).view(n, L, n_heads, D // n_heads)
               for nm in ("query_projection", "key_projection", "value_projection"))
    a = attn(q, k, v, cla.EPS)
    if taps is not None:
        for t in (q, k, a):
            t.retain_grad()
        taps.append((x2, q, k, a))
    a = a.reshape(n * L, D)
    s1 = x2 + drop(proj("out_projection", a), p, seeds[0], row0)
    x1 = F.layer_norm(s1, (D,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], LN_EPS)
    g = drop(act(F.linear(x1, P[pre + "linear1.weight"], P[pre + "linear1.bias"])), p, seeds[1], row0)
    s2 = x1 + drop(F.linear(g, P[pre + "linear2.weight"], P[pre + "linear2.bias"]), p, seeds[2], row0)
    return F.layer_norm(s2, (D,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], LN_EPS).view(n, L, D)


def encoder_forward(x, P, n_layers, n_heads, p, seeds, row0=0, pre="", drop=dropout.dropout, taps=None, attn=None,
                    act=F.gelu):
    """The layers (seeds[3i:3i + 3] for layer i) and the final norm.  attn: None (cla.cla_reference) or layer index ->
    that layer's attention(q, k, v, eps); act: the FFN activation."""
    for i in range(n_layers):
        x = layer_forward(x, P, "%slayers.%d." % (pre, i), n_heads, p, seeds[3 * i:3 * i + 3], row0, drop, taps,
                          cla.cla_reference if attn is None else attn(i), act)
    D = x.shape[-1]
    return F.layer_norm(x, (D,), P[pre + "norm.weight"], P[pre + "norm.bias"], LN_EPS)


def _dphi(t):
    """Derivative of the feature map elu(t) + 1."""
    return torch.where(t > 0, torch.ones_like(t), torch.exp(t))


def normaliser_terms(q, k, out):
    """Squared norms of the attention backward's normaliser terms against the whole gradients, w.r.t. phi(q) and phi(k),
    from a tap of layer_forward after the backward.  With den_i = phi(q_i) . z_i, z_i = sum_{j<=i} phi(k_j) and c_i =
    (out_i . dout_i) / den_i, the gradients are the differences
        dphi(q_i) = (S_i dout_i) / den_i - c_i z_i,     dphi(k_j) = sum_{i>=j} phi(q_i) (v_j . dout_i) / den_i - c_i phi(q_i),
    whose second terms nearly cancel the first when the attention averages over many tokens.
    -> (|c z|^2, |dphi(q)|^2, |sum c phi(q)|^2, |dphi(k)|^2)."""
    dout = out.grad
    out = out.detach()
    qd, kd = q.detach(), k.detach()
    Q, K = cla.feature_map(qd), cla.feature_map(kd)
    z = K.cumsum(1)
    c = (out * dout).sum(-1, keepdim=True) / ((Q * z).sum(-1, keepdim=True) + cla.EPS)
    tq = c * z
    tk = (c * Q).flip(1).cumsum(1).flip(1)
    return (tq.square().sum().item(), (q.grad / _dphi(qd)).square().sum().item(), tk.square().sum().item(),
            (k.grad / _dphi(kd)).square().sum().item())


def row_terms(x2, t):
    """The row contributions to a projection's parameter gradients, from a tap: t.grad (rows, D) is the gradient of the
    projection's output, x2 (rows, D) its input.  -> (sum_r |dt_r|^2, sum_r |dt_r|^2 |x_r|^2): the squared norms a bias
    gradient (sum_r dt_r) and a weight gradient (sum_r dt_r x_r^T) would have if their rows added up without cancelling."""
    g2 = t.grad.reshape(x2.shape[0], -1).square().sum(1)
    return g2.sum().item(), (g2 * x2.detach().square().sum(1)).sum().item()


def _leaves(params, dtype, device):
    return {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in params.items()}


def encoder_vjp(params, x, dy, n_layers, n_heads, p, seeds, slab=None, dtype=torch.float64, drop=dropout.dropout,
                gains=None):
    """Output, input gradient and parameter gradients of the encoder for the upstream gradient dy, in `dtype` on x's
    device, `slab` sequences at a time.  params: name -> tensor (the encoder's named_parameters()).
    gains: a list that receives, per layer, a dict over the whole batch: "query" / "key" the normaliser gains
    |c z| / |dphi(q)| and |sum c phi(q)| / |dphi(k)| (normaliser_terms), "query_rows" / "key_rows" the uncancelled norms
    (bias, weight) of the projection gradients (row_terms).  -> (y, dx, {name: grad})."""
    dev = x.device
    P = _leaves(params, dtype, dev)
    N, L, _ = x.shape
    slab = slab or N
    ys, dxs = [], []
    sums = [[0.0] * 8 for _ in range(n_layers)]
    for n0 in range(0, N, slab):
        xs = x[n0:n0 + slab].to(dtype).requires_grad_(True)
        taps = [] if gains is not None else None
        y = encoder_forward(xs, P, n_layers, n_heads, p, seeds, n0 * L, drop=drop, taps=taps)
        y.backward(dy[n0:n0 + slab].to(dtype))
        ys.append(y.detach())
        dxs.append(xs.grad)
        for i, (x2, q, k, a) in enumerate(taps or []):
            t = normaliser_terms(q, k, a) + row_terms(x2, q) + row_terms(x2, k)
            sums[i] = [u + w for u, w in zip(sums[i], t)]
        del y, xs, taps
    if gains is not None:
        gains.extend({"query": (s[0] / s[1]) ** 0.5, "key": (s[2] / s[3]) ** 0.5,
                      "query_rows": (s[4] ** 0.5, s[5] ** 0.5), "key_rows": (s[6] ** 0.5, s[7] ** 0.5)} for s in sums)
    return torch.cat(ys), torch.cat(dxs), {k: v.grad for k, v in P.items()}


def step_losses(P, pe, tokens, target, mask, msum, n_token, emb_sizes, n_layers, n_heads, p, seeds, row0=0,
                drop=dropout.dropout):
    """The six losses' shares of one slab: tokens / target (n, T, 6) int64, mask (n, T); msum the batch's masked-token
    count; pe (max_len, D); seeds = [front] + 3 per layer -> (6,) sum(mask * nll_f) / msum over the slab."""
    n, T, _ = tokens.shape
    embs = torch.cat([P["word_emb_%s.lut.weight" % a][tokens[..., i]] * math.sqrt(d)
                      for i, (a, d) in enumerate(zip(ATTRS, emb_sizes))], -1)
    e = F.linear(embs, P["in_linear.weight"], P["in_linear.bias"]) + pe[:T].to(embs.dtype)
    e = drop(e, p, seeds[0], row0)
    h = encoder_forward(e, P, n_layers, n_heads, p, seeds[1:], row0, "transformer_encoder.", drop)
    m = mask.reshape(-1).to(h.dtype)
    losses = []
    for i, (a, nt) in enumerate(zip(ATTRS, n_token)):
        logits = F.linear(h, P["proj_%s.weight" % a], P["proj_%s.bias" % a]).reshape(-1, nt)
        nll = F.cross_entropy(logits, target[..., i].reshape(-1), reduction="none")
        losses.append((nll * m).sum() / msum)
    return torch.stack(losses)


def step_grads(params, pe, tokens, target, mask, n_token, n_layers, n_heads, p, seeds, slab=None,
               emb_sizes=(128, 256, 64, 512, 128, 128), dtype=torch.float64, drop=dropout.dropout):
    """The CW train step: the six masked-mean CE losses and the gradients of their mean (sum(losses) / 6, what the
    tests back-propagate) for every parameter the step uses, in `dtype` on tokens' device, `slab` sequences at a time.
    params: name -> tensor (the model's named_parameters(); unused ones get None).  -> (losses (6,), {name: grad})."""
    dev = tokens.device
    P = _leaves(params, dtype, dev)
    pe = pe.reshape(-1, pe.shape[-1]).to(device=dev, dtype=dtype)
    N, T, _ = tokens.shape
    slab = slab or N
    msum = mask.to(dtype).sum()
    total = torch.zeros(len(n_token), dtype=dtype, device=dev)
    for n0 in range(0, N, slab):
        sl = slice(n0, n0 + slab)
        ls = step_losses(P, pe, tokens[sl], target[sl], mask[sl], msum, n_token, emb_sizes, n_layers, n_heads, p, seeds,
                         n0 * T, drop)
        (ls.sum() / len(n_token)).backward()
        total += ls.detach()
        del ls
    return total, {k: v.grad for k, v in P.items()}

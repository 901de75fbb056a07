"""CPU: the f64 reference of token-by-token generation (oracle/decode_f64.py) checked on its own, and the bounds the GPU
tests hold the kernels to (tests/test_decode_f64_gpu.py derives them) checked against the rounding floor of the chain.

* logits, hidden rows and state equal oracle.cw_model.CWLinearTransformer(recurrent=True) in f64, fed one token per call
  with its memory, to 1e-12 relative (both are f64; only the order of the sums differs);
* the recorded generation fixture (tests/golden/dqn_generation_small.npz) lies within its own f32 precision of it;
* slabs of songs equal the whole batch, ragged lengths equal each song run alone, no padding row reaches a state;
* every wrong= variant differs from the right reference, on the rows it is meant to move;
* the floor: the same chain evaluated in torch f32 (state summed one token at a time, as the recurrent form does) against
  f64 at repo dims, for both weight sets of the GPU tests.  row_bound and state_bound must lie between that floor and 8x
  it.  Measured, 12 layers, seeds as below: rows 6.5e-7 .. 7.7e-7 worst over 1 to 1 024 tokens (median 5.1e-7), row_bound
  2.67e-6 = 3.5 .. 4.1x; state, per layer, 1.4e-7 .. 8e-7, state_bound 2.0 .. 6.5x it.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

from oracle import cw_model, decode_f64  # noqa: E402

N_CLASS = [56, 135, 18, 87, 18, 25]
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))


def _model(d_model, n_layers, n_heads, seed=5, variant="dqn"):
    return fill_params(cw_model.CWLinearTransformer(N_CLASS, d_model, n_layers, n_heads, variant=variant,
                                                    recurrent=True), seed=seed).eval()


def _tokens(n, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, c, (n, L), generator=g) for c in N_CLASS], -1)


def _scaled(params, scale):
    """The GPU tests' second weight set: every layer's query and key projection weights times `scale`."""
    return {k: v * scale if k.endswith(("query_projection.weight", "key_projection.weight")) else v
            for k, v in params.items()}


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("dims", [(128, 2, 2), (512, 2, 8)])
@pytest.mark.parametrize("variant", ["dqn", "actor"])
def test_reference_equals_the_recurrent_oracle(dims, variant):
    d_model, n_layers, n_heads = dims
    net = _model(d_model, n_layers, n_heads, variant=variant).double()
    tok = _tokens(3, 40, 1)
    lens = [40, 17, 33]
    lg, h, st = decode_f64.decode_f64(net.state_dict(), tok, N_CLASS, n_layers, n_heads, lens)
    worst = 0.0
    with torch.no_grad():
        for n, ln in enumerate(lens):                       # the recurrent oracle takes one song: (1, 1, 6) per call
            mem = None
            for t in range(ln):
                hr, mem = net.forward_hidden(tok[n:n + 1, t:t + 1], memory=mem, is_training=False)
                lr = torch.cat(net.forward_output(hr), -1)
                worst = max(worst, decode_f64.row_rel(lg[n, t], lr[0]).item(), decode_f64.row_rel(h[n, t], hr[0]).item())
            for (S, Z), (Sr, Zr) in zip(st, mem):
                worst = max(worst, _rel(S[n], Sr[0]), _rel(Z[n], Zr[0]))
    print("worst relative difference from the recurrent oracle %.3g" % worst)
    assert worst < 1e-12
    assert st[0][0].shape == (3, n_heads, 64, 64) and st[0][1].shape == (3, n_heads, 64)
    assert lg.shape == (3, 40, sum(N_CLASS)) and h.shape == (3, 40, d_model)


def test_recorded_fixture_within_its_f32_precision():
    net = _model(128, 2, 2, seed=int(FIX["fill_seed"]))
    tok = torch.from_numpy(FIX["tokens"][:len(FIX["logits"])])[None]
    lg, h = decode_f64.logits_f64(net.state_dict(), tok, [int(v) for v in FIX["n_class"]], 2, 2)
    bound = decode_f64.row_bound(2)
    rl = decode_f64.row_rel(FIX["logits"], lg[0]).max().item()
    rh = decode_f64.row_rel(FIX["h"], h[0]).max().item()
    print("fixture against f64: logits %.3g hidden %.3g of a row's norm (bound %.3g)" % (rl, rh, bound))
    assert rl < bound and rh < bound


def test_slabs_and_ragged_lengths():
    net = _model(128, 2, 2).double()
    P = net.state_dict()
    tok = _tokens(5, 70, 2)
    lens = [70, 1, 32, 33, 64]
    whole = decode_f64.decode_f64(P, tok, N_CLASS, 2, 2, lens, slab=5)
    for slab in (1, 2):
        part = decode_f64.decode_f64(P, tok, N_CLASS, 2, 2, lens, slab=slab)
        assert _rel(part[0], whole[0]) < 1e-13 and _rel(part[1], whole[1]) < 1e-13
        for (S, Z), (Sw, Zw) in zip(part[2], whole[2]):
            assert _rel(S, Sw) < 1e-13 and _rel(Z, Zw) < 1e-13
    # each song alone, cut at its length; tokens past the length replaced: a padding row reaches nothing
    other = tok.clone()
    for n, ln in enumerate(lens):
        other[n, ln:] = _tokens(1, 70, 9)[0, ln:]
    pad = decode_f64.decode_f64(P, other, N_CLASS, 2, 2, lens)
    for n, ln in enumerate(lens):
        one = decode_f64.decode_f64(P, tok[n:n + 1, :ln], N_CLASS, 2, 2)
        for w in (whole, pad):
            assert _rel(w[0][n, :ln], one[0][0]) < 1e-13 and _rel(w[1][n, :ln], one[1][0]) < 1e-13
            for (S, Z), (S1, Z1) in zip(w[2], one[2]):
                assert _rel(S[n], S1[0]) < 1e-13 and _rel(Z[n], Z1[0]) < 1e-13
    with pytest.raises(ValueError):
        decode_f64.decode_f64(P, tok, N_CLASS, 2, 2, [0, 1, 1, 1, 1])
    with pytest.raises(ValueError):
        decode_f64.decode_f64(P, tok, N_CLASS, 2, 2, wrong="nothing")


def test_every_wrong_variant_moves_the_rows_it_feeds():
    net = _model(512, 2, 8).double()
    P = _scaled(net.state_dict(), 10)
    tok = _tokens(3, 48, 3)
    lg, h, st = decode_f64.decode_f64(P, tok, N_CLASS, 2, 8)
    big = 100 * decode_f64.row_bound(12)
    for wrong in decode_f64.WRONG:
        lw, hw, sw = decode_f64.decode_f64(P, tok, N_CLASS, 2, 8, wrong=wrong)
        r = decode_f64.row_rel(lw, lg)
        print("%-12s rows moved by %.3g .. %.3g of their norm" % (wrong, r.min(), r.max()))
        if wrong == "pe_t":
            assert (r[:, 0] == 0).all() and r[:, 1:].min() > big
        elif wrong == "drop32":
            assert (r[:, :32] == 0).all() and r[:, 33:].min() > big
            assert min(_rel(a[0], b[0]) for a, b in zip(sw, st)) > big
        elif wrong == "song_stride":
            assert (r[-1] == 0).all() and r[:-1].min() > big
            assert _rel(sw[0][0], st[0][0]) == 0 and _rel(sw[-1][0][:-1], st[-1][0][:-1]) > big
        elif wrong == "z_raw":
            assert r.min() > big and min(_rel(a[1], b[1]) for a, b in zip(sw, st)) > big
        else:
            assert r.min() > 10 * decode_f64.row_bound(12)


@pytest.mark.parametrize("scale", [1, 10])
def test_bounds_lie_within_8x_of_the_f32_floor_of_the_chain(scale):
    """Repo dims, 12 layers.  The floor is the reference's own chain in f32 against f64: nothing of the kernels.  Rows:
    worst row of a song.  State: per layer and length, the worst (song, head) over S and Z of 64 songs (8 from 32 tokens on, one of 1 024)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    P = _scaled(_model(512, 12, 8).state_dict(), scale)
    ratios = []
    for lens, seed in (([1] * 64, 10), ([2] * 64, 11), ([8] * 64, 12), ([32] * 8, 13), ([64] * 8, 14), ([1024], 15)):
        L = lens[0]
        tok = _tokens(len(lens), L, seed)
        lg, h, st = decode_f64.decode_f64(P, tok, N_CLASS, 12, 8)
        lg32, h32, st32 = decode_f64.decode_f64(P, tok, N_CLASS, 12, 8, dtype=torch.float32, sequential_state=True)
        floor = max(decode_f64.row_rel(lg32, lg).max().item(), decode_f64.row_rel(h32, h).max().item())
        bound = decode_f64.row_bound(12)
        print("x%d L %d: rows floor %.3g bound %.3g (%.2fx)" % (scale, L, floor, bound, bound / floor))
        assert floor < bound < 8 * floor
        for i, ((S, Z), (S32, Z32)) in enumerate(zip(st, st32)):
            bound = decode_f64.state_bound(L, i)
            floor = max(decode_f64.state_rel(S32, S).max().item(), decode_f64.state_rel(Z32, Z).max().item())
            ratios.append(bound / floor)
            if i in (0, 11):
                print("    layer %d state floor %.3g bound %.3g (%.2fx)" % (i, floor, bound, bound / floor))
            assert floor < bound < 8 * floor, (L, i, floor, bound)
    print("x%d: state bound / floor %.2f .. %.2f" % (scale, min(ratios), max(ratios)))

"""GPU: the position-table forms of the two input-front kernels (cwlt_posenc_dropout_pos, cwlt_cw_embed_proj_fwd_pos) on
packed songs of lengths 1, 63, 64, 65, 200, f32 and bf16.

p = 0: every packed row is BITWISE the rectangular kernel's row for the same (song, position) -- the rectangular kernel run
on that song alone (T = its length, so r % T is the position).
p = 0.1: the kept set is oracle/dropout.py's for the PACKED row index and the seed, with and without the device-resident
seed offset; dropped elements are exact zeros; kept elements are the p = 0 row scaled by keep_scale.  f32: bitwise (one
f32 product either way).  bf16: the kernel rounds (x + pe) * scale once while the p = 0 row was rounded before the scale,
so the two differ by at most two bf16 roundings (8 significant bits: at most 2^-8 relative each) and one f32 product:
|got - row * scale| <= 2^-7 (1 + 2^-6) |row * scale|.
"""
import math

import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import ops
from oracle import dropout, elementwise_f64 as o

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
LENS = [1, 63, 64, 65, 200]
D = 128
SEED = 0x1234567890ABCDE
N_CLASS = [5, 7, 3, 9, 4, 6]


def layout(cuda):
    cu = [0]
    for L in LENS:
        cu.append(cu[-1] + L)
    pos = torch.cat([torch.arange(L, dtype=torch.int32) for L in LENS]).to(cuda)
    return cu, pos


def pe_table(cuda, max_len=256):
    pe = torch.zeros(max_len, D)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div = torch.exp(torch.arange(0, D, 2).float() * (-math.log(10000.0) / D))
    pe[:, 0::2], pe[:, 1::2] = torch.sin(position * div), torch.cos(position * div)
    return pe.to(cuda)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def check_dropped_and_kept(got, row0, p, base, dtype, label):
    R = got.shape[0]
    keep = o.keep(SEED, p, R, D, got.device, base=base)
    assert 0.05 < 1 - keep.double().mean().item() < 0.15
    assert torch.equal(got != 0, keep & (row0 != 0)), (label, "the kept set is the oracle's for the packed row index")
    want = row0.float() * dropout.keep_scale(p)
    if dtype == F32:
        assert same_bits(torch.where(keep, got, torch.zeros_like(got)), torch.where(keep, want, torch.zeros_like(want)))
    else:
        err = (got.float() - want).abs()
        assert bool((err[keep] <= 2.0 ** -7 * (1 + 2.0 ** -6) * want.abs()[keep]).all()), label
    assert bool((got[~keep] == 0).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_posenc_dropout_pos(cuda, dtype, monkeypatch):
    cu, pos = layout(cuda)
    R = cu[-1]
    pe = pe_table(cuda)
    x = torch.randn(R, D, generator=torch.Generator().manual_seed(1)).to(dtype).to(cuda)
    row0 = ops.posenc_dropout(x, pe, max(LENS), 0.0, 0, pos=pos)
    for s, L in enumerate(LENS):
        a, z = cu[s], cu[s + 1]
        alone = ops.posenc_dropout(x[a:z], pe, L, 0.0, 0)
        assert same_bits(row0[a:z], alone), ("song", s)
    # the rectangular kernel on the packed buffer takes other positions: the table is what places the rows
    assert not same_bits(row0, ops.posenc_dropout(x, pe, max(LENS), 0.0, 0))
    p = 0.1
    got = ops.posenc_dropout(x, pe, max(LENS), p, SEED, pos=pos)
    assert torch.equal(got != 0, ops.posenc_dropout(x, None, 7, p, SEED) != 0), "the stream cwlt_posenc_dropout draws"
    check_dropped_and_kept(got, row0, p, 0, dtype, "posenc")
    monkeypatch.setattr(ops, "_USE_SEED_BASE", True)
    base_t = ops.seed_base_tensor(cuda)
    try:
        for base in (12345, -1):
            base_t.fill_(base)
            check_dropped_and_kept(ops.posenc_dropout(x, pe, max(LENS), p, SEED, pos=pos), row0, p, base, dtype,
                                   "posenc base %d" % base)
    finally:
        base_t.fill_(0)
    with pytest.raises(RuntimeError, match="positional table"):
        ops.posenc_dropout(x, pe[:199], max(LENS), 0.0, 0, pos=pos)
    with pytest.raises(ValueError):
        ops.posenc_dropout(x, pe, max(LENS), 0.0, 0, pos=pos.long())
    with pytest.raises(ValueError):
        ops.posenc_dropout(x, pe, max(LENS), 0.0, 0, pos=pos[:-1])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_embed_proj_pos(cuda, dtype, monkeypatch):
    cu, pos = layout(cuda)
    R = cu[-1]
    pe = pe_table(cuda)
    g = torch.Generator().manual_seed(2)
    tables = [torch.randn(n, 64, generator=g).to(cuda) for n in N_CLASS]
    w_in = (torch.randn(D, 64 * len(N_CLASS), generator=g) / 20).to(cuda)
    b_in = torch.randn(D, generator=g).to(cuda)
    tok = torch.stack([torch.randint(0, n, (R,), generator=g) for n in N_CLASS], -1).to(cuda)

    def packed(p, seed):
        return ops.embed_proj(tok.unsqueeze(0), tables, w_in, b_in, pe, p, seed, dtype, pos=pos, max_len=max(LENS))[0]

    row0 = packed(0.0, 0)
    for s, L in enumerate(LENS):
        a, z = cu[s], cu[s + 1]
        alone = ops.embed_proj(tok[a:z].unsqueeze(0), tables, w_in, b_in, pe, 0.0, 0, dtype)[0]
        assert same_bits(row0[a:z], alone), ("song", s)
    p = 0.1
    check_dropped_and_kept(packed(p, SEED), row0, p, 0, dtype, "embed_proj")
    monkeypatch.setattr(ops, "_USE_SEED_BASE", True)
    base_t = ops.seed_base_tensor(cuda)
    try:
        base_t.fill_(12345)
        check_dropped_and_kept(packed(p, SEED), row0, p, 12345, dtype, "embed_proj base")
    finally:
        base_t.fill_(0)
    with pytest.raises(RuntimeError, match="positional table"):
        ops.embed_proj(tok.unsqueeze(0), tables, w_in, b_in, pe[:100], 0.0, 0, dtype, pos=pos, max_len=max(LENS))
    # the gradient reaches the tables and in_linear through the unchanged backward
    tabs = [t.clone().requires_grad_(True) for t in tables]
    w = w_in.clone().requires_grad_(True)
    out = ops.embed_proj(tok.unsqueeze(0), tabs, w, b_in, pe, 0.0, 0, dtype, pos=pos, max_len=max(LENS))
    out.float().sum().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in tabs) and torch.isfinite(w.grad).all()

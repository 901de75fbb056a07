"""The libcwlt kernels' dropout keep mask, restated in torch integer ops (TEST INFRASTRUCTURE; see oracle/__init__.py).

csrc/cwlt_common.h (hash32, rng_pair, dropout_keep, drop_thresh, drop_scale): ONE 32-bit hash per element pair, keyed
by the 62-bit seed of ops.next_seed() and the pair index idx >> 1; the even element of the pair takes the low 16 bits,
the odd one the high 16 bits, and an element is kept iff its 16 bits are >= thresh16 = round(p * 65536).  A kept
element is scaled by 65536 / (65536 - thresh16), which is 1 / (1 - p) up to the rounding of p to a multiple of 2^-16.
`idx` is the 64-bit element index in the site's (rows, cols) tensor (row * cols + col).

Device-agnostic: int64 tensors holding 32-bit values, every 32-bit product split into 16-bit halves so that no
intermediate overflows, so the same code runs on the CPU and on the GPU.
"""
import torch

M32 = 0xFFFFFFFF


def thresh16(p):
    """drop_thresh: the 16-bit drop threshold of probability p (0: keep everything)."""
    if p <= 0:
        return 0
    return min(max(int(float(p) * 65536.0 + 0.5), 1), 65535)


def keep_scale(p):
    """drop_scale: what a kept element is multiplied by."""
    t = thresh16(p)
    return 65536.0 / (65536.0 - t) if t else 1.0


def _mul32(a, c):
    """(a * c) mod 2^32 for an int64 tensor a of values in [0, 2^32) and a constant c < 2^32."""
    return (a * (c & 0xFFFF) + (((a * (c >> 16)) & 0xFFFF) << 16)) & M32


def hash32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def rng_pair(seed, pair):
    """The hash word of pair indices `pair` (int64 tensor, values >= 0) under `seed` (a Python int < 2^62)."""
    seed = int(seed)
    k0 = (seed & M32) ^ (((seed >> 32) * 0x9E3779B9) & M32)
    key = _mul32((pair >> 32) & M32, 0x85EBCA6B) ^ k0
    return hash32(_mul32(pair & M32, 0x9E3779B1) ^ key)


def keep_flags(seed, p, idx):
    """dropout_keep at element indices `idx` (int64 tensor) -> bool tensor of idx's shape."""
    t = thresh16(p)
    if t == 0:
        return torch.ones(idx.shape, dtype=torch.bool, device=idx.device)
    r = rng_pair(seed, idx >> 1)
    bits = torch.where((idx & 1) == 1, r >> 16, r & 0xFFFF)
    return bits >= t


def site_mask(seed, p, rows, cols, row0=0, device=None, offset=0):
    """(rows, cols) keep flags of rows row0 .. row0 + rows - 1 of a site's (R, cols) tensor.  `offset` is added to every
    element index (0 for the kernels' mask; tests shift a mask with it)."""
    start = int(row0) * int(cols) + int(offset)
    idx = torch.arange(start, start + rows * cols, dtype=torch.int64, device=device).view(rows, cols)
    return keep_flags(seed, p, idx)


def dropout(x, p, seed, row0=0, offset=0):
    """The kernels' dropout of x (..., cols), whose rows are rows row0 .. of the site's (R, cols) tensor."""
    if p <= 0:
        return x
    cols = x.shape[-1]
    rows = x.numel() // cols
    m = site_mask(seed, p, rows, cols, row0, x.device, offset).view(x.shape)
    return torch.where(m, x * keep_scale(p), torch.zeros((), dtype=x.dtype, device=x.device))

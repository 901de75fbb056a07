"""GPU: the un-projected CW embedding (csrc/embed.hip: cw_embed_fwd_kernel, cw_embed_bwd_kernel, cw_embed_bwd_mfma_kernel)
per element and per table row against the f64 references of oracle/elementwise_f64.py (pinned, with the bounds, by
tests/test_oracle_elementwise_f64_cpu.py).

Forward: f32 within 1 ulp of table_f[clamp(id)] sqrt(w_f), bf16 one rounding more; table sets of one 64-wide table (40 rows
at once, more than a block's 16), the repo's six (1216 columns, 2 at once), 1408 and 2048 columns (1 at once, idle lanes) and
8 attributes; rows 1, 15, 16, 17, 33; ids below 0 and >= n; a strided output whose gap keeps its sentinels; refusals.
Backward: every gradient element relative to the sum of |terms| of its table row; an id no row hits must be exactly 0.  The
kernel form (MFMA / LDS slab, raised LDS limit) is asserted by restating cwlt_cw_embed_bwd's predicate on the very arguments
passed (oracle.embed_bwd_form).  f32 slab at rows 1, 3, 4, 5, 255, 256, 257, 513; bf16 MFMA at vocabularies 1, 31, 32, 33,
160; bf16 slab through a vocabulary of 161, ldd % 8 != 0 and a dout 8 bytes off 16-byte alignment; vocabularies 257 and 640
(LDS above 64 KiB) in both dtypes, 641 refused; 131073 rows (per = 257: the last split starts past the end and must add
zeros); 2097152 rows (MFMA at exactly 4096 rows per split) and 2097153 (slab), against a chunked f64 index_add_.
Tooth: the reference without the last non-empty row split misses the kernels' result by TEETH x the bound.

Measured on an MI355X: profiles/elementwise_f64_ratios.txt.
"""
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import _lib, ops
from oracle import elementwise_f64 as o

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NAME = {F32: "f32", BF16: "bf16"}
SENT = -7777.0
WORST = {}
SETS = {"one64": ((64,), (18,)), "repo": (o.REPO_WIDTHS, o.REPO_VOCAB), "w1408": ((512, 512, 384), (7, 33, 160)),
        "w2048": ((1024, 1024), (5, 3)), "attr8": ((64,) * 8, (3, 31, 32, 33, 1, 160, 9, 2))}


def note(label, r, dtype):
    for k, v in r.items():
        WORST[(k, NAME[dtype])] = max(WORST.get((k, NAME[dtype]), 0.0), v)
    print("    %-60s %s" % (label, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert all(v <= 1 for v in r.values()), (label, r)


def guarded(n, dtype, dev, shift=0):
    """n elements inside a sentinel-filled buffer, starting 64 + shift elements in."""
    buf = torch.full((n + 128 + shift,), SENT, dtype=dtype, device=dev)
    return buf, buf[64 + shift:64 + shift + n]


def intact(buf, n, shift=0):
    return bool((buf[:64 + shift] == SENT).all()) and bool((buf[64 + shift + n:] == SENT).all())


def embed_fwd(tok, tables, dtype, ldo=None, shift=0):
    widths, nrows = [t.shape[1] for t in tables], [t.shape[0] for t in tables]
    rows, dcat = tok.shape[0], sum(widths)
    ldo = ldo or dcat
    buf, flat = guarded(rows * ldo, dtype, tok.device, shift)
    keep = tok.clone()
    ops._call("cwlt_cw_embed_fwd", _lib.dev(tok), _lib.ptr_array(tables), _lib.int_array(widths), _lib.int_array(nrows),
              len(tables), _lib.dev(flat), rows, ldo, _lib.dtype_code(dtype), _lib.stream_ptr())
    torch.cuda.synchronize()
    out = flat.view(rows, ldo)
    assert intact(buf, rows * ldo, shift) and bool((out[:, dcat:] == SENT).all()) and torch.equal(keep, tok)
    return out[:, :dcat]


def embed_bwd(tok, widths, nrows, dout):
    """dout: (rows, dcat) view with row stride ldd, any base alignment.  -> list of (n_f, w_f) f32 gradients."""
    rows = tok.shape[0]
    total = sum(w * n for w, n in zip(widths, nrows))
    ns = _lib.load().cwlt_embed_splits(rows)
    assert ns == o.embed_splits(rows)
    pbuf, part = guarded(ns * total, F32, tok.device)
    fbuf, flat = guarded(total, F32, tok.device)
    keep = dout.clone()
    ops._call("cwlt_cw_embed_bwd", _lib.dev(tok), _lib.int_array(widths), _lib.int_array(nrows), len(widths), _lib.dev(dout),
              _lib.dev(part), _lib.dev(flat), rows, dout.stride(0), _lib.dtype_code(dout.dtype), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert intact(pbuf, ns * total) and intact(fbuf, total) and torch.equal(keep, dout)
    grads, off = [], 0
    for w, n in zip(widths, nrows):
        grads.append(flat[off:off + w * n].view(n, w))
        off += w * n
    return grads


def make_dout(rows, dcat, dtype, dev, pad=0, shift=0, seed=7):
    """(rows, dcat) view: row stride dcat + pad, base `shift` elements off a 16-byte boundary."""
    ld = dcat + pad
    base = torch.randn(rows * ld + 64, generator=torch.Generator(device=dev).manual_seed(seed + rows), device=dev).to(dtype)
    return base[shift:shift + rows * ld].view(rows, ld)[:, :dcat]


def bwd_case(cuda, dtype, widths, nrows, rows, form, label, pad=0, shift=0, tok=None, tooth=False):
    tok = (o.make_tokens(rows, nrows, seed=rows, oor=True) if tok is None else tok).to(cuda)
    dout = make_dout(rows, sum(widths), dtype, cuda, pad, shift)
    assert o.embed_bwd_form(dtype, nrows, rows, dout.stride(0), dout.data_ptr()) == form, label
    got = embed_bwd(tok, widths, nrows, dout)
    again = embed_bwd(tok, widths, nrows, dout)
    ref = o.embed_backward(tok, dout, widths, nrows)
    worst = 0.0
    for f, (g, (rg, bnd)) in enumerate(zip(got, ref)):
        assert torch.equal(g, again[f]), label
        worst = max(worst, o.ratio(g, rg, bnd))
        hit = torch.zeros(nrows[f], dtype=torch.bool, device=cuda)
        hit[tok[:, f].clamp(0, nrows[f] - 1)] = True
        assert bool((g[~hit] == 0).all()), label
    note("embed_bwd %s %s %s rows %d" % (NAME[dtype], form[0] + ("+lds" if form[1] else ""), label, rows), dict(dtable=worst), dtype)
    if tooth:
        wrong = o.embed_backward(tok, dout, widths, nrows, drop_rows=o.last_split_rows(rows, o.embed_splits(rows), cuda))
        t = max(o.ratio(g, wg, bnd) for g, (wg, _), (_, bnd) in zip(got, wrong, ref))
        print("    tooth embed_bwd last split dropped %s %s: %.3g" % (NAME[dtype], form[0], t))
        assert t >= o.TEETH
    return got


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(SETS))
def test_embed_forward(cuda, dtype, name):
    widths, nrows = SETS[name]
    bf = dtype == BF16
    tables = [t.to(cuda) for t in o.make_tables(widths, nrows)]
    dcat = sum(widths)
    for rows in (1, 15, 16, 17, 33):
        tok = o.make_tokens(rows, nrows, seed=rows, oor=True).to(cuda)
        assert rows < 15 or (bool((tok < 0).any()) and bool((tok >= torch.tensor(nrows, device=cuda)).any()))
        ref = o.embed_forward(tok, tables)
        bnd = o.embed_fwd_bound(ref, bf)
        for ldo in (dcat, dcat + 8):
            out = embed_fwd(tok, tables, dtype, ldo)
            assert torch.equal(out, embed_fwd(tok, tables, dtype, ldo))
            note("embed %s %s rows %d ldo %d" % (NAME[dtype], name, rows, ldo), dict(embed=o.ratio(out, ref, bnd)), dtype)
        viaops = ops.cw_embed(tok, tables, dtype)
        assert torch.equal(viaops, embed_fwd(tok, tables, dtype))
        for mut in ("neighbour", "wrap") if name == "repo" and rows == 33 else ():
            t = o.ratio(out, o.embed_forward(tok, tables, mut=mut), bnd)
            print("    tooth embed %s %s: %.3g" % (mut, NAME[dtype], t))
            assert t >= o.TEETH


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_embed_forward_refusals(cuda, dtype):
    tok = torch.zeros(4, 1, dtype=torch.int64, device=cuda)
    for widths, nrows in (((96,), (5,)), ((1024, 1024, 64), (3, 3, 3))):          # a width of 96; 2112 columns
        tables = [torch.zeros(n, w, device=cuda) for w, n in zip(widths, nrows)]
        with pytest.raises(RuntimeError, match="1001"):
            embed_fwd(tok.expand(4, len(widths)).contiguous(), tables, dtype)
    with pytest.raises(RuntimeError, match="1001"):                                # `out` 4 (f32) / 8 (bf16) bytes off
        embed_fwd(tok, [torch.zeros(5, 64, device=cuda)], dtype, shift=1 if dtype == F32 else 4)
    with pytest.raises(RuntimeError, match="1001"):                                # ldo no multiple of the vector
        embed_fwd(tok, [torch.zeros(5, 64, device=cuda)], dtype, ldo=66)


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 255, 256, 257, 513])
def test_embed_backward_f32_slab(cuda, rows):
    bwd_case(cuda, F32, o.REPO_WIDTHS, o.REPO_VOCAB, rows, ("slab", False), "repo", tooth=rows == 513)
    bwd_case(cuda, F32, o.REPO_WIDTHS, o.REPO_VOCAB, rows, ("slab", False), "repo ldd+4", pad=4)


@pytest.mark.parametrize("vocab", [1, 31, 32, 33, 160])
def test_embed_backward_bf16_mfma(cuda, vocab):
    widths, nrows = (64, 128), (vocab, 18)
    for rows in (1, 15, 16, 17, 513):
        tok = o.make_tokens(rows, nrows, seed=rows, oor=True, every=(1, 4), never=(0, vocab // 2) if vocab > 2 else None)
        got = bwd_case(cuda, BF16, widths, nrows, rows, ("mfma", False), "vocab %d" % vocab, tok=tok, tooth=rows == 513)
        assert bool((got[1][:4] == 0).all()) and bool((got[1][5:] == 0).all()) and bool((got[1][4] != 0).any())
        assert vocab <= 2 or bool((got[0][vocab // 2] == 0).all())
    bwd_case(cuda, BF16, widths, nrows, 513, ("mfma", False), "vocab %d ldd+8" % vocab, pad=8)


def test_embed_backward_bf16_slab_triggers(cuda):
    for rows in (1, 5, 257, 513):
        bwd_case(cuda, BF16, (64, 128), (161, 18), rows, ("slab", False), "vocab 161", tooth=rows == 513)
        bwd_case(cuda, BF16, (64, 128), (33, 18), rows, ("slab", False), "ldd % 8 = 4", pad=4)
        bwd_case(cuda, BF16, (64, 128), (33, 18), rows, ("slab", False), "dout 8 bytes off", shift=4)
        bwd_case(cuda, BF16, (64, 128), (33, 18), rows, ("mfma", False), "aligned twin")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_embed_backward_large_vocabularies(cuda, dtype):
    for vocab, big in ((256, False), (257, True), (640, True)):
        for rows in (5, 513):
            bwd_case(cuda, dtype, (64,), (vocab,), rows, ("slab", big), "vocab %d" % vocab)
    assert o.embed_bwd_form(dtype, (641,), 5, 64, 0) is None
    with pytest.raises(RuntimeError, match="1001"):
        embed_bwd(torch.zeros(5, 1, dtype=torch.int64, device=cuda), (64,), (641,), torch.zeros(5, 64, dtype=dtype, device=cuda))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_embed_backward_empty_last_split(cuda, dtype):
    """131073 rows: 512 splits of 257 rows, the last one starts past the end (n < 0 in the MFMA kernel, r0 > r1 in the slab)."""
    rows = 131073
    assert o.embed_splits(rows) == 512 and -(-rows // 512) * 511 > rows
    bwd_case(cuda, dtype, (64,), (18,), rows, ("mfma", False) if dtype == BF16 else ("slab", False), "one64", tooth=True)


@pytest.mark.parametrize("rows,form", [(2097152, "mfma"), (2097153, "slab")])
def test_embed_backward_rows_per_split_limit(cuda, rows, form):
    """EB_MAXROWS = 4096 rows per split exactly (the id cache full), and one row more (the LDS-slab kernel in bf16)."""
    assert -(-rows // o.embed_splits(rows)) == (4096 if form == "mfma" else 4097)
    bwd_case(cuda, BF16, (64,), (18,), rows, (form, False), "one64")


def test_worst_ratios_summary(cuda):
    for (k, d), v in sorted(WORST.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print("    worst %-7s %-5s %.3f" % (k, d, v))
    assert all(v <= 1 for v in WORST.values())

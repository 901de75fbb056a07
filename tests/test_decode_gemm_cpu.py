"""CPU: the row-batched decode step's entry points (csrc/decode_gemm.hip) are declared, bound, exported and versioned,
and refuse arguments they cannot take before touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cwlt_decode_gemm", "cwlt_decode_gemm_scratch_floats", "cwlt_decode_step_rows",
         "cwlt_decode_rows_workspace_floats"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


def test_entries_declared_in_header():
    text = open(os.path.join(ROOT, "include", "cwlt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, text), name


def test_entries_bound_and_exported(built):
    lib = built.load()
    for name in NAMES:
        assert name in built._SIGNATURES and hasattr(lib, name), name


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 21
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_gemm_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)      # non-null, aligned dummy: every call below is refused before any launch

    def call(W=buf, x=buf, out=buf, ln_w=None, ln_b=None, ln2_w=None, ln2_b=None, n_out=512, K=512, act=0, n=8,
             ld_x=None, ld_out=None, scratch=buf):
        return lib.cwlt_decode_gemm(W, buf, x, ln_w, ln_b, ln2_w, ln2_b, 1e-5, None, out, None, n_out, K, act, n,
                                    K if ld_x is None else ld_x, 0, n_out if ld_out is None else ld_out, K, scratch,
                                    null)

    assert call(W=null) == 1001 and call(x=null) == 1001 and call(out=null) == 1001
    for K in (0, 100, 520, 4096):                   # K % 16 == 0, 16 <= K <= 2048
        assert call(K=K) == 1001, K
    assert call(n=0) == 1001 and call(n=-3) == 1001 and call(n=4097) == 1001
    assert call(n_out=0) == 1001 and call(act=2) == 1001
    assert call(ln_w=buf) == 1001                   # LayerNorm weight without bias
    assert call(ln2_w=buf, ln2_b=buf) == 1001       # second LayerNorm without a first
    assert call(ld_x=514) == 1001 and call(ld_x=256) == 1001 and call(ld_out=100) == 1001
    assert call(K=1216, n_out=512, scratch=null) == 1001             # split-K needs the caller's scratch


def test_scratch_query(built):
    lib = built.load()
    assert lib.cwlt_decode_gemm_scratch_floats(512, 100, 8) == -1
    assert lib.cwlt_decode_gemm_scratch_floats(512, 512, 0) == -1
    assert lib.cwlt_decode_gemm_scratch_floats(512, 512, 4097) == -1
    for n_out, K in [(512, 512), (1536, 512), (2048, 512), (512, 2048), (512, 1216), (339, 512), (384, 128)]:
        a = lib.cwlt_decode_gemm_scratch_floats(n_out, K, 64)
        b = lib.cwlt_decode_gemm_scratch_floats(n_out, K, 128)
        assert a >= 64 * K and b >= 128 * K
        assert b * 64 == a * 128, (n_out, K)        # the split count, hence the per-row scratch, does not depend on M


def _model(built, D=512, F=2048, E=1216, n_layer=2, heads=339):
    keep = []
    layers = (built.DecodeLayer * n_layer)()
    for L in layers:
        for f in ("wqkv", "bqkv", "wo", "bo", "ln1_w", "ln1_b", "w1", "b1", "w2", "b2", "ln2_w", "ln2_b", "S", "Z"):
            setattr(L, f, 256)
    m = built.DecodeModel()
    m.n_layer, m.n_head, m.d_model, m.d_ff, m.n_attr, m.emb_width, m.n_logits = n_layer, D // 64, D, F, 6, E, heads
    m.eps_ln, m.eps_attn = 1e-5, 1e-6
    tables = (ctypes.c_void_p * 6)(*([256] * 6))
    widths = built.int_array([128, 256, 64, 512, 128, 128])
    nrows = built.int_array([56, 135, 18, 87, 18, 25])
    keep += [tables, widths, nrows, layers]
    m.tables = ctypes.cast(tables, ctypes.POINTER(ctypes.c_void_p))
    m.widths = ctypes.cast(widths, ctypes.POINTER(ctypes.c_int))
    m.nrows = ctypes.cast(nrows, ctypes.POINTER(ctypes.c_int))
    m.layers = ctypes.cast(layers, ctypes.POINTER(built.DecodeLayer))
    m.w_in = m.b_in = m.pe0 = m.w_heads = m.b_heads = 256
    return m, keep


def test_step_workspace_and_refusals_without_gpu(built):
    lib = built.load()
    m, keep = _model(built)
    per_song = lib.cwlt_decode_workspace_floats(ctypes.byref(m))
    assert per_song > 0
    for n in (1, 64, 4096):
        assert lib.cwlt_decode_rows_workspace_floats(ctypes.byref(m), n) >= n * per_song
    assert lib.cwlt_decode_rows_workspace_floats(ctypes.byref(m), 0) == -1
    assert lib.cwlt_decode_rows_workspace_floats(ctypes.byref(m), 4097) == -1
    buf = ctypes.c_void_p(256)
    step = lambda mm, tok=buf, work=buf, logits=buf, n=4: lib.cwlt_decode_step_rows(ctypes.byref(mm), tok, work, None,
                                                                                    logits, n, None)
    assert step(m, tok=None) == 1001 and step(m, work=None) == 1001 and step(m, logits=None) == 1001
    assert step(m, n=0) == 1001 and step(m, n=-1) == 1001 and step(m, n=4097) == 1001
    bad, keep2 = _model(built, E=1210)              # embedding width not a multiple of 16
    assert lib.cwlt_decode_rows_workspace_floats(ctypes.byref(bad), 4) == -1 and step(bad) == 1001

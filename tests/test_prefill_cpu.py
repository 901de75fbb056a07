"""CPU: the prompt-prefill entry point (csrc/prefill.hip) is declared, bound, exported and versioned, and refuses
arguments it cannot take before touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cwlt_causal_linear_fwd_state"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


def test_entry_declared_in_header():
    text = open(os.path.join(ROOT, "include", "cwlt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)


def test_entry_bound_and_exported(built):
    assert NAME in built._SIGNATURES
    assert hasattr(built.load(), NAME)


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 20
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_entry_refusals_without_gpu(built):
    fn = getattr(built.load(), NAME)
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)      # non-null, aligned dummy: every call below is refused before any launch
    ok = dict(N=1, H=8, L=16, hd=64, ld=1536, seg=1, ws=null, dtype=0)

    def call(q=buf, S=buf, lengths=None, **kw):
        a = dict(ok, **kw)
        return fn(q, buf, buf, buf, S, buf, lengths, a["N"], a["H"], a["L"], a["hd"], a["ld"], a["ld"], a["ld"], 512,
                  1e-6, a["seg"], a["ws"], a["dtype"], null)

    assert call(q=null) == 1001 and call(S=null) == 1001
    assert call(hd=32) == 1001
    assert call(dtype=1) == 1002                          # bf16: f32 only
    assert call(ld=1534) == 1001                          # 16-byte row loads
    assert call(q=ctypes.c_void_p(260)) == 1001
    assert call(N=0) == 0 and call(L=0) == 0              # nothing to do, nothing launched
    assert call(seg=0) == 1001 and call(L=320, seg=4) == 1001            # segments >= 1 with a workspace
    assert call(L=320, seg=4, ws=buf, N=0) == 0
    assert call(L=288, seg=4, ws=buf, N=0) == 1001                      # 9 chunks: 3 + 3 + 3 + 0 leaves a run empty


def test_segment_choice(built):
    lib = built.load()
    # one song at the repo dims (8 streams): ~256 workgroups, every run at least one 32-token chunk
    assert lib.cwlt_prefill_segments(1, 8, 1024) == 32 and lib.cwlt_prefill_segments(1, 8, 3584) == 28
    assert lib.cwlt_prefill_segments(8, 8, 1024) == 4 and lib.cwlt_prefill_segments(1, 8, 32) == 1
    assert lib.cwlt_prefill_segments(16, 8, 4096) == 1                  # the streams fill the chip
    for N, H, L in [(1, 8, 1024), (1, 8, 3584), (3, 2, 200), (1, 2, 4096), (8, 8, 1000)]:
        P = lib.cwlt_prefill_segments(N, H, L)
        chunks = -(-L // 32)
        assert P == 1 or (P - 1) * -(-chunks // P) < chunks
        assert lib.cwlt_prefill_seg_floats(N, H, P) == (N * H * P * 4160 if P > 1 else 0)

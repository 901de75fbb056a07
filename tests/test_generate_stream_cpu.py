"""CPU: the continuous-batching entry points (csrc/stream.hip, cwlt_sample_categorical_keyed in csrc/sample.hip) are
declared, bound, exported and versioned, and refuse arguments they cannot take before touching the device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cwlt_sample_categorical_keyed", "cwlt_stream_refill", "cwlt_stream_advance"]


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
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_entries_bound_and_exported(built):
    lib = built.load()
    for name in NAMES:
        assert name in built._SIGNATURES and name in built.exported_names() and hasattr(lib, name), name
    from rlmg_amd import generation, ops
    for fn in ("sample_categorical_keyed", "stream_refill", "stream_advance"):
        assert callable(getattr(ops, fn)), fn
    assert callable(generation.generate_stream)


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 22
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_keyed_sampler_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)
    n_class = built.int_array([4, 6])

    def call(logits=buf, key=buf, step=buf, tokens=buf, n_attr=2, rows=8, ld=10, classes=n_class):
        return lib.cwlt_sample_categorical_keyed(logits, classes, None, None, n_attr, rows, ld, 7, key, step, tokens,
                                                 null)

    assert call(key=null) == 1001 and call(step=null) == 1001
    assert call(logits=null) == 1001 and call(tokens=null) == 1001
    assert call(rows=0) == 1001 and call(rows=(1 << 20) + 1) == 1001
    assert call(n_attr=0) == 1001 and call(n_attr=9) == 1001
    assert call(ld=9) == 1001                                   # ld < sum of the classes
    assert call(classes=built.int_array([4, 300])) == 1001      # more than 256 classes in one attribute


def test_refill_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)

    def call(state=buf, snap=buf, n_layer=2, s=64, z=8, logits=buf, snap_logits=buf, n_logits=10, ld=10, fresh=buf,
             slots=4):
        return lib.cwlt_stream_refill(state, snap, n_layer, s, z, logits, snap_logits, n_logits, ld, fresh, slots, null)

    for kw in ({"state": null}, {"snap": null}, {"logits": null}, {"snap_logits": null}, {"fresh": null}):
        assert call(**kw) == 1001, kw
    assert call(n_layer=0) == 1001 and call(slots=0) == 1001
    assert call(s=62) == 1001 and call(z=6) == 1001 and call(s=0) == 1001   # whole float4 pieces only
    assert call(n_logits=0) == 1001 and call(ld=9) == 1001
    assert call(state=ctypes.c_void_p(260)) == 1001                          # 16-byte alignment


def test_advance_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)

    def call(tokens=buf, n_attr=6, slots=4, bar_attr=2, mask=buf, bar_classes=18, bar_cond=17, bar0=1, cap=100,
             n_songs=10, song=buf, pos=buf, bar=buf, fresh=buf, ctl=buf, ring=buf, ring_rows=8):
        return lib.cwlt_stream_advance(tokens, n_attr, slots, bar_attr, mask, bar_classes, bar_cond, bar0, cap,
                                       n_songs, song, pos, bar, fresh, ctl, ring, ring_rows, null)

    for k in ("tokens", "mask", "song", "pos", "bar", "fresh", "ctl", "ring"):
        assert call(**{k: null}) == 1001, k
    assert call(n_attr=0) == 1001 and call(n_attr=9) == 1001
    assert call(bar_attr=-1) == 1001 and call(bar_attr=6) == 1001 and call(bar_classes=0) == 1001
    assert call(slots=0) == 1001 and call(ring_rows=0) == 1001 and call(cap=0) == 1001
    assert call(n_songs=-1) == 1001 and call(n_songs=(1 << 20) + 1) == 1001
    assert call(bar0=17) == 1001                                             # the start count already reaches bar_cond

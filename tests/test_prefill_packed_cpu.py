"""CPU: the packed prefill's two entry points (cwlt_causal_linear_fwd_state_packed, cwlt_prefer_scan_packed) are
declared, bound, exported and versioned and refuse bad arguments before any launch; generation.packed_blocks on
hand-written length lists; and the Python refusals of the packed forms that need no device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cwlt_causal_linear_fwd_state_packed", "cwlt_prefer_scan_packed")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


@pytest.mark.parametrize("name", NAMES)
def test_entries_declared_bound_exported(built, name):
    text = open(os.path.join(ROOT, "include", "cwlt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert name in built._SIGNATURES and name in built.exported_names()
    assert hasattr(built.load(), name)


def test_abi_version(built):
    assert built.ABI_VERSION >= 39
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_scan_refusals_without_gpu(built):
    fn = built.load().cwlt_causal_linear_fwd_state_packed
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)      # non-null, aligned dummy: every call below is refused before any launch
    ok = dict(n=3, H=8, hd=64, ld=1536, dtype=0)

    def call(q=buf, S=buf, cu=buf, **kw):
        a = dict(ok, **kw)
        return fn(q, buf, buf, buf, S, buf, cu, a["n"], a["H"], a["hd"], a["ld"], a["ld"], a["ld"], 512, 1e-6,
                  a["dtype"], null)

    assert call(q=null) == 1001 and call(S=null) == 1001 and call(cu=null) == 1001
    assert call(hd=32) == 1001
    assert call(dtype=1) == 1002                          # bf16: f32 only
    assert call(ld=1534) == 1001                          # 16-byte row loads
    assert call(ld=256) == 1001                           # a row stride below H * 64
    assert call(q=ctypes.c_void_p(260)) == 1001           # a misaligned base
    assert call(n=-1) == 1001 and call(H=0) == 1001
    assert call(n=0) == 0                                 # nothing to do, nothing launched


def test_prefer_scan_refusals_without_gpu(built):
    fn = built.load().cwlt_prefer_scan_packed
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(256)
    nc = (ctypes.c_int * 6)(56, 135, 18, 87, 18, 25)
    W = 339

    def call(tokens=buf, cu=buf, n_block=4, n_class=nc, n_attr=6, pen=buf, n_songs=4, out=buf, ld=W):
        return fn(tokens, cu, n_block, n_class, n_attr, pen, n_songs, null, out, ld, null)

    assert call(tokens=null) == 1001 and call(cu=null) == 1001 and call(pen=null) == 1001 and call(out=null) == 1001
    assert call(n_block=0) == 1001 and call(n_block=(1 << 20) + 1) == 1001
    assert call(n_songs=0) == 1001 and call(ld=W - 1) == 1001
    assert call(n_attr=0) == 1001 and call(n_attr=9) == 1001 and call(n_class=None) == 1001
    assert call(n_class=(ctypes.c_int * 6)(56, 135, 18, 257, 18, 25)) == 1001


def _check_blocks(lengths, blocks, budget, cap):
    assert [a for a, _ in blocks] == [0] + [z for _, z in blocks[:-1]] and blocks[-1][1] == len(lengths)
    for a, z in blocks:
        assert z > a                                                     # whole songs, every one once and in order
        assert sum(lengths[a:z]) <= budget or z - a == 1                 # only a lone oversize song breaks the budget
        assert cap is None or z - a <= cap
    # greedy: the next song did not fit
    for (a, z), (_, z2) in zip(blocks, blocks[1:]):
        assert sum(lengths[a:z]) + lengths[z] > budget or (cap is not None and z - a == cap)


def test_packed_blocks():
    import rlmg_amd  # noqa: F401
    from rlmg_amd.generation import PREFILL_ROWS, packed_blocks
    assert packed_blocks([], 10) == []
    assert packed_blocks([3], 10) == [(0, 1)]
    assert packed_blocks([2, 33, 64, 65, 7, 130], 70) == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
    assert packed_blocks([5, 48, 1, 33, 17, 40], 60) == [(0, 3), (3, 5), (5, 6)]
    assert packed_blocks([4, 4, 4, 4, 4], 8) == [(0, 2), (2, 4), (4, 5)]             # exactly the budget fits
    assert packed_blocks([100, 1, 1, 100, 1], 10) == [(0, 1), (1, 3), (3, 4), (4, 5)]   # oversize songs stand alone
    assert packed_blocks([1] * 7, 100, max_songs=3) == [(0, 3), (3, 6), (6, 7)]
    assert packed_blocks([1] * 4, 100, max_songs=1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert packed_blocks([7, 9], None) == [(0, 2)] and PREFILL_ROWS >= 16
    rng = np.random.default_rng(0)
    for budget, cap in ((1, None), (50, None), (300, 4), (10 ** 6, 5), (64, 1)):
        lengths = [int(n) for n in rng.integers(1, 200, 60)]
        _check_blocks(lengths, packed_blocks(lengths, budget, cap), budget, cap)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="prefill_rows"):
            packed_blocks([1, 2], bad)
    with pytest.raises(ValueError, match="max_songs"):
        packed_blocks([1, 2], 10, max_songs=0)
    with pytest.raises(ValueError, match="empty"):
        packed_blocks([3, 0, 2], 10)


def _stub(**kw):
    """What check_entry reads of a model."""
    d = dict(_recurrent=True, training=False, compute_dtype=torch.float32, n_token=[56, 135, 18, 87, 18, 25])
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_python_refusals_without_gpu():
    import rlmg_amd  # noqa: F401
    from rlmg_amd import generation, ops
    from rlmg_amd.draw_plan import check_entry
    # the name is known wherever a prefill kernel is named, and the model's state is still checked under it
    check_entry(_stub(), "scoring", "categorical", kernel="packed")
    check_entry(_stub(), "generation", "dqn", prefill="packed")
    with pytest.raises(ValueError, match="must be 'blas' or 'gemm'"):
        check_entry(_stub(), "scoring", "categorical", kernel="pack")
    with pytest.raises(RuntimeError, match="recurrent"):
        check_entry(_stub(_recurrent=False), "scoring", "categorical", kernel="packed")
    with pytest.raises(RuntimeError, match="eval"):
        check_entry(_stub(training=True), "scoring", "categorical", kernel="packed")
    with pytest.raises(RuntimeError, match="f32"):
        check_entry(_stub(compute_dtype=torch.bfloat16), "scoring", "categorical", kernel="packed")
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, _stub().n_token)}
    w2e["bar-beat"][1] = "Bar"
    # packed_prefill belongs to a prompt list
    with pytest.raises(ValueError, match="packed_prefill"):
        generation.generate_stream(_stub(), w2e, 4, slots=2, packed_prefill=True)
    with pytest.raises(ValueError, match="packed_prefill"):
        generation.generate_stream(_stub(), w2e, 4, slots=2, prompt=np.zeros((3, 6), np.int64), packed_prefill=True)
    with pytest.raises(ValueError, match="packed_prefill"):
        generation.generate_particles(_stub(), w2e, 4, 2, packed_prefill=True)
    with pytest.raises(ValueError, match="packed_prefill"):
        generation.generate_particles(_stub(), w2e, 4, 2, slots=2, resample_every=4, chunk=16, packed_prefill=True)
    with pytest.raises(ValueError, match="empty prompt"):              # an empty prompt, as with "gemm"
        generation.generate_stream(_stub(), w2e, 2, slots=2, prompts=[np.zeros((0, 6), np.int64)] * 2,
                                   packed_prefill=True)
    with pytest.raises(ValueError, match="share_prefill"):             # "blas" is still not batch invariant
        generation.generate_particles(_stub(), w2e, 4, 2, prefill="blas", share_prefill=True)
    # the wrappers: host checks of the offsets, and no CPU path
    q = torch.zeros(10, 2, 64)
    S, Z = torch.zeros(2, 2, 64, 64), torch.zeros(2, 2, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.cla_fwd_state_packed(q, q, q, S, Z, [0, 3, 10])
    tok = torch.zeros(10, 6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.prefer_scan_packed(tok, [0, 3, 10], _stub().n_token, torch.zeros(2, 13))
    with pytest.raises(TypeError):
        ops.prefer_scan_packed(tok.int(), [0, 3, 10], _stub().n_token, torch.zeros(2, 13))

"""CPU: per-song prompts on the stream -- the bank entry points (cwlt_stream_refill_bank, cwlt_stream_advance_bank in
csrc/stream.hip) are declared, bound, exported and versioned and refuse bad arguments without a GPU; the dataset
prompt cutter and the block / bank plan with its reuse rule are pure functions."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cwlt_stream_refill_bank", "cwlt_stream_advance_bank"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


def _w2e():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(8)} for k in keys}
    w2e["bar-beat"][1] = "Bar"
    w2e["bar-beat"][5] = "Bar"
    return w2e


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
    for fn in ("stream_refill_bank", "stream_advance_bank"):
        assert callable(getattr(ops, fn)), fn
    for fn in ("cut_prompt", "dataset_prompts", "stream_bank_plan", "bank_may_prefill"):
        assert callable(getattr(generation, fn)), fn


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 23
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_refill_bank_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)

    def call(state=buf, bank_state=buf, bank=4, n_layer=2, s=64, z=8, logits=buf, bank_logits=buf, n_logits=10,
             ld=10, ld_bank=10, fresh=buf, song=buf, slots=4):
        return lib.cwlt_stream_refill_bank(state, bank_state, bank, n_layer, s, z, logits, bank_logits, n_logits, ld,
                                           ld_bank, fresh, song, slots, null)

    for kw in ({"state": null}, {"bank_state": null}, {"logits": null}, {"bank_logits": null}, {"fresh": null},
               {"song": null}):
        assert call(**kw) == 1001, kw
    assert call(n_layer=0) == 1001 and call(slots=0) == 1001 and call(bank=0) == 1001
    assert call(s=62) == 1001 and call(z=6) == 1001 and call(s=0) == 1001
    assert call(n_logits=0) == 1001 and call(ld=9) == 1001 and call(ld_bank=9) == 1001
    assert call(bank_state=ctypes.c_void_p(264)) == 1001                       # 16-byte alignment


def test_advance_bank_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)

    def call(tokens=buf, n_attr=6, slots=4, bar_attr=2, mask=buf, bar_classes=18, bar_cond=17, bar0=buf, caps=buf,
             bank=8, n_songs=10, song=buf, pos=buf, bar=buf, cap=buf, fresh=buf, ctl=buf, ring=buf, ring_rows=8):
        return lib.cwlt_stream_advance_bank(tokens, n_attr, slots, bar_attr, mask, bar_classes, bar_cond, bar0, caps,
                                            bank, n_songs, song, pos, bar, cap, fresh, ctl, ring, ring_rows, null)

    for k in ("tokens", "mask", "bar0", "caps", "song", "pos", "bar", "cap", "fresh", "ctl", "ring"):
        assert call(**{k: null}) == 1001, k
    assert call(n_attr=0) == 1001 and call(n_attr=9) == 1001
    assert call(bar_attr=-1) == 1001 and call(bar_attr=6) == 1001 and call(bar_classes=0) == 1001
    assert call(slots=0) == 1001 and call(ring_rows=0) == 1001 and call(bank=0) == 1001
    assert call(n_songs=-1) == 1001 and call(n_songs=(1 << 20) + 1) == 1001 and call(bar_cond=0) == 1001


def test_cut_prompt():
    from rlmg_amd import generation
    w2e = _w2e()
    bb = [1, 0, 0, 5, 0, 1, 0, 0, 1, 0]                   # Bars open bars 2, 3 and 4 at rows 3, 5 and 8
    song = np.zeros((len(bb), 6), dtype=np.int64)
    song[:, 2] = bb
    song[:, 0] = np.arange(len(bb))
    assert generation.cut_prompt(song, w2e, 1)[:, 0].tolist() == [0, 1, 2]
    assert generation.cut_prompt(song, w2e, 2)[:, 0].tolist() == [0, 1, 2, 3, 4]
    assert generation.cut_prompt(song, w2e, 3)[:, 0].tolist() == list(range(8))
    assert generation.cut_prompt(song, w2e, 4).tolist() == song.tolist()           # fewer bars: the whole song
    for k in (1, 2, 3):                                    # the cut prompt's bar count is k: bar_cond k + 1 admits it
        p = generation.cut_prompt(song, w2e, k)
        assert 1 + sum(w2e["bar-beat"][int(r[2])] == "Bar" for r in p[1:]) == k
    with pytest.raises(ValueError, match="prompt_bars"):
        generation.cut_prompt(song, w2e, 0)


def test_dataset_prompts():
    from rlmg_amd import generation
    w2e = _w2e()
    x = np.zeros((2, 8, 6), dtype=np.int64)
    x[0, :, 2] = [1, 0, 1, 0, 1, 0, 0, 0]
    x[1, :, 2] = [0, 0, 0, 1, 0, 0, 0, 0]
    x[:, :, 0] = np.arange(8)
    mask = np.array([[1] * 8, [1] * 2 + [0] * 6])
    ps = generation.dataset_prompts(x, w2e, 1, 5, mask=mask)
    assert len(ps) == 5
    assert ps[0][:, 0].tolist() == [0, 1] and ps[2][:, 0].tolist() == [0, 1] and ps[4][:, 0].tolist() == [0, 1]
    assert ps[1][:, 0].tolist() == [0, 1]                  # the masked rows (a Bar at row 3) are not the song's
    assert generation.dataset_prompts(x, w2e, 2, 1)[0][:, 0].tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="no dataset"):
        generation.dataset_prompts(x[:0], w2e, 1, 1)


def test_bank_plan_defaults():
    from rlmg_amd import generation
    lens = [64, 512, 100, 300] * 512                       # 2048 songs, longest 512
    B, bank = generation.stream_bank_plan(lens, 256)
    assert B == generation.PREFILL_ROWS // 512 == 64
    assert bank % B == 0 and bank >= 2 * 256 and bank < 2 * 256 + B
    B, bank = generation.stream_bank_plan(lens, 256, prefill_rows=1024)
    assert B == 2 and bank == 512
    # memory caps the bank, never below two blocks
    B, bank = generation.stream_bank_plan(lens, 256, entry_bytes=1 << 20, free_bytes=4 * 64 * 3 * (1 << 20))
    assert (B, bank) == (64, 192)
    B, bank = generation.stream_bank_plan(lens, 256, entry_bytes=1 << 20, free_bytes=1 << 20)
    assert (B, bank) == (64, 128)
    # no more entries than the songs in whole blocks; B at most n_songs
    assert generation.stream_bank_plan([10] * 5, 256) == (5, 5)
    assert generation.stream_bank_plan([10] * 7, 256, prefill_rows=30) == (3, 9)
    # an explicit bank: a multiple of B, B lowered to it
    assert generation.stream_bank_plan([10] * 7, 4, prefill_rows=20, bank=4) == (2, 4)
    assert generation.stream_bank_plan([10] * 7, 4, prefill_rows=100, bank=2) == (2, 2)
    with pytest.raises(ValueError, match="multiple"):
        generation.stream_bank_plan([10] * 7, 4, prefill_rows=20, bank=5)
    with pytest.raises(ValueError):
        generation.stream_bank_plan([10, 0], 4)


def test_bank_reuse_rule():
    from rlmg_amd import generation
    B, bank = 3, 6                                          # two blocks of three songs
    may = generation.bank_may_prefill
    assert may(0, B, bank, 0) and may(1, B, bank, 0)        # the first nb blocks are free
    assert not may(2, B, bank, 2)                           # block 2 reuses block 0's entries: songs 0..2 assigned?
    assert may(2, B, bank, 3)
    assert not may(3, B, bank, 5) and may(3, B, bank, 6)
    # the entries a block writes wrap round the bank, and no live entry is overwritten: simulate assignment in order
    n = 17
    written, assigned, j = {}, 0, 0
    while assigned < n:
        while j < -(-n // B) and may(j, B, bank, assigned):
            for k in range(j * B, min(n, (j + 1) * B)):
                e = k % bank
                assert e == (j % (bank // B)) * B + k - j * B
                assert written.get(e) is None or written[e] < assigned, (k, e)   # the old song was handed out
                written[e] = k
            j += 1
        ready = min(n, j * B)
        assert ready > assigned                             # the gate always opens: no deadlock
        assigned = min(ready, assigned + 2)                 # two slots take songs per step
    assert j == -(-n // B)

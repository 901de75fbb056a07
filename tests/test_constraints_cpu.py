"""CPU: constrained generation -- the masked sampler and the bar counter (cwlt_sample_categorical_masked,
cwlt_count_bars in csrc/sample.hip) are declared, bound, exported and versioned and refuse bad arguments without a GPU;
generation.Constraint compiles names and ids to mask bits, schedules and shared rows, checks songs with violations(),
and every refusal of the constraints= argument that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cwlt_sample_categorical_masked", "cwlt_count_bars"]
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


def _w2e():
    """A small vocabulary: class 0 = 0, class 1 = CONTI in tempo / chord, Bar classes 1 and 5 in bar-beat."""
    n = [6, 7, 8, 9, 5, 4]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(c)} for k, c in zip(KEYS, n)}
    for k in KEYS:
        w2e[k][0] = 0
    w2e["tempo"][1] = w2e["chord"][1] = "CONTI"
    w2e["bar-beat"][1] = w2e["bar-beat"][5] = "Bar"
    return w2e


def _bits(c, bar_cond=17):
    """mask_rows() unpacked: (R, sum n_class) bool."""
    m = c.mask_rows(bar_cond)
    return np.unpackbits(m.view(np.uint8), axis=1, bitorder="little")[:, :sum(c.n_class)].astype(bool), m


def _seg(row, a, n_class):
    o = sum(n_class[:a])
    return row[o:o + n_class[a]]


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
    for fn in ("sample_categorical_masked", "count_bars"):
        assert callable(getattr(ops, fn)), fn
    assert callable(generation.Constraint) and callable(generation.compile_constraints)


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 24
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_masked_sampler_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)
    n_class = (ctypes.c_int * 6)(56, 135, 18, 87, 18, 25)           # 339 classes: 11 words

    def call(logits=buf, nc=n_class, n_attr=6, rows=4, ld=339, counter=buf, key=null, step=null, bar=buf, sched=buf,
             n_sched=4, masks=buf, mask_rows=2, words=11, tokens=buf):
        return lib.cwlt_sample_categorical_masked(logits, nc, None, None, n_attr, rows, ld, 7, counter, key, step, bar,
                                                  sched, n_sched, masks, mask_rows, words, tokens, null)

    for kw in ({"logits": null}, {"tokens": null}, {"bar": null}, {"sched": null}, {"masks": null}):
        assert call(**kw) == 1001, kw
    assert call(words=10) == 1001                                    # 320 bits < 339 classes
    assert call(rows=(1 << 20) + 1) == 1001
    assert call(counter=null) == 1001                                # neither key nor counter
    assert call(key=buf) == 1001 and call(step=buf) == 1001          # key without step, step without key
    assert call(n_sched=0) == 1001 and call(mask_rows=0) == 1001 and call(words=0) == 1001
    assert call(n_attr=9) == 1001 and call(ld=338) == 1001 and call(rows=0) == 1001


def test_count_bars_refusals_without_gpu(built):
    lib = built.load()
    null = ctypes.c_void_p(0)
    buf = ctypes.c_void_p(256)

    def call(tokens=buf, rows=4, n_attr=6, bar_attr=2, mask=buf, bar_classes=18, bar=buf):
        return lib.cwlt_count_bars(tokens, rows, n_attr, bar_attr, mask, bar_classes, bar, null)

    for kw in ({"tokens": null}, {"mask": null}, {"bar": null}):
        assert call(**kw) == 1001, kw
    assert call(rows=0) == 1001 and call(rows=(1 << 20) + 1) == 1001
    assert call(bar_attr=6) == 1001 and call(bar_attr=-1) == 1001 and call(n_attr=0) == 1001 and call(n_attr=9) == 1001
    assert call(bar_classes=0) == 1001


def test_names_and_ids_to_bits():
    from rlmg_amd import generation
    w2e = _w2e()
    c = generation.Constraint(w2e, allow={"tempo": ["tempo_3", 4], "pitch": range(2, 5), "chord": "chord_6"})
    bits, m = _bits(c)
    assert m.dtype == np.uint32 and m.shape == (1, -(-sum(c.n_class) // 32))
    row = bits[0]
    assert np.flatnonzero(_seg(row, 0, c.n_class)).tolist() == [0, 1, 3, 4]        # 0 and CONTI kept
    assert np.flatnonzero(_seg(row, 1, c.n_class)).tolist() == [0, 1, 6]
    assert np.flatnonzero(_seg(row, 3, c.n_class)).tolist() == [0, 2, 3, 4]
    for a in (2, 4, 5):                                                             # unrestricted: every class
        assert _seg(row, a, c.n_class).all()
    # bit off[a] + c of word (off[a] + c) // 32
    off = int(np.cumsum([0] + c.n_class)[3])
    assert (m[0, (off + 2) // 32] >> ((off + 2) % 32)) & 1 == 1
    assert (m[0, (off + 1) // 32] >> ((off + 1) % 32)) & 1 == 0
    strict = generation.Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": [2]}, keep_neutral=False)
    row = _bits(strict)[0][0]
    assert np.flatnonzero(_seg(row, 0, c.n_class)).tolist() == [3]
    assert np.flatnonzero(_seg(row, 3, c.n_class)).tolist() == [2]
    # every Bar class when "Bar" is named
    bb = generation.Constraint(w2e, allow={"bar-beat": ["Bar"]}, keep_neutral=False)
    assert np.flatnonzero(_seg(_bits(bb)[0][0], 2, c.n_class)).tolist() == [1, 5]


def test_schedule_cycle_and_clamp():
    from rlmg_amd import generation
    w2e = _w2e()
    prog = [["chord_2"], ["chord_3"], ["chord_4"]]
    cyc = generation.Constraint(w2e, per_bar={"chord": prog}, cycle=True)
    bits, m = _bits(cyc, bar_cond=9)
    assert m.shape[0] == 8                                           # expanded to bar_cond - 1 rows
    for i in range(8):
        assert np.flatnonzero(_seg(bits[i], 1, cyc.n_class)).tolist() == [0, 1, 2 + i % 3], i
    assert _bits(cyc, bar_cond=2)[1].shape[0] == 1
    clamp = generation.Constraint(w2e, per_bar={"chord": prog, "pitch": [[3], [4, 5]]})
    bits, m = _bits(clamp, bar_cond=17)
    assert m.shape[0] == 3                                           # the longest schedule; the device clamps past it
    assert [np.flatnonzero(_seg(b, 3, clamp.n_class)).tolist() for b in bits] == [[0, 3], [0, 4, 5], [0, 4, 5]]
    assert _bits(clamp, bar_cond=3)[1].shape[0] == 2                 # rows past bar_cond - 1 are never read
    # allowed(bar) past the end: the last entry holds, or the cycle goes on
    assert np.flatnonzero(clamp.allowed(40)[1]).tolist() == [0, 1, 4]
    assert np.flatnonzero(cyc.allowed(40)[1]).tolist() == [0, 1, 2 + 39 % 3]
    assert np.flatnonzero(clamp.allowed(0)[1]).tolist() == [0, 1, 2]


def test_compile_shares_rows():
    from rlmg_amd import generation
    w2e = _w2e()
    n_token = [len(v) for v in w2e.values()]
    a = generation.Constraint(w2e, per_bar={"chord": [["chord_2"], ["chord_3"]]}, cycle=True)
    b = generation.Constraint(w2e, allow={"pitch": [3]})
    b2 = generation.Constraint(w2e, allow={"pitch": [3]})            # equal but another object: rows of its own
    sched, masks = generation.compile_constraints([a, None, b, a, b2, b], 6, n_token, 5, [1] * 6, 200)
    assert sched.tolist() == [[0, 4], [0, 0], [4, 1], [0, 4], [5, 1], [4, 1]]
    assert masks.shape == (6, 2) and masks.dtype == np.uint32
    assert (masks[0:4] == a.mask_rows(5)).all() and (masks[4] == b.mask_rows(5)[0]).all()
    sched, masks = generation.compile_constraints(a, 3, n_token, 5, [1] * 3, 200)       # one for every song
    assert sched.tolist() == [[0, 4]] * 3 and masks.shape == (4, 2)
    assert generation.compile_constraints([None, None], 2, n_token, 5, [1, 1], 200) is None


def test_refusals():
    from rlmg_amd import generation
    w2e = _w2e()
    n_token = [len(v) for v in w2e.values()]
    with pytest.raises(ValueError, match="unknown attribute"):
        generation.Constraint(w2e, allow={"key": ["C"]})
    with pytest.raises(ValueError, match="unknown attribute"):
        generation.Constraint(w2e, per_bar={"type": [["Note"]]})
    with pytest.raises(ValueError, match="unknown event"):
        generation.Constraint(w2e, allow={"pitch": ["pitch_99"]})
    with pytest.raises(ValueError, match="unknown event"):
        generation.Constraint(w2e, per_bar={"chord": [["chord_2"], ["nope"]]})
    with pytest.raises(ValueError, match="out of range"):
        generation.Constraint(w2e, allow={"pitch": [9]})
    with pytest.raises(ValueError, match="empty"):
        generation.Constraint(w2e, allow={"pitch": []})
    with pytest.raises(ValueError, match="empty"):
        generation.Constraint(w2e, per_bar={"pitch": [[2], []]})
    with pytest.raises(ValueError, match="non-empty list"):
        generation.Constraint(w2e, per_bar={"pitch": []})
    with pytest.raises(ValueError, match="both"):
        generation.Constraint(w2e, allow={"pitch": [2]}, per_bar={"pitch": [[3]]})
    c = generation.Constraint(w2e, allow={"pitch": [2]})
    with pytest.raises(ValueError, match="3 entries for 2 songs"):
        generation.compile_constraints([c, c, None], 2, n_token, 5, [1, 1], None)
    with pytest.raises(ValueError, match="Constraint"):
        generation.compile_constraints([c, "pitch"], 2, n_token, 5, [1, 1], None)
    with pytest.raises(ValueError, match="classes"):
        generation.compile_constraints(c, 2, n_token[:5] + [9], 5, [1, 1], None)
    # a bar-beat restriction with no Bar class in a reachable bar: refused without max_tokens only
    no_bar = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar", "bar-beat_2"], ["bar-beat_3"]]})
    with pytest.raises(ValueError, match="never"):
        generation.compile_constraints(no_bar, 2, n_token, 5, [1, 1], None)
    assert generation.compile_constraints(no_bar, 2, n_token, 5, [1, 1], 100) is not None
    assert generation.compile_constraints(no_bar, 2, n_token, 2, [1, 1], None) is not None    # bar 2 never drawn
    # keep_neutral keeps class 0, never a Bar: only an explicit Bar makes the song end
    with pytest.raises(ValueError, match="never"):
        generation.compile_constraints(generation.Constraint(w2e, allow={"bar-beat": ["bar-beat_2"]}), 1, n_token,
                                       3, [1], None)
    cyc = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar"], ["bar-beat_3"]]}, cycle=True)
    with pytest.raises(ValueError, match="never"):
        generation.compile_constraints(cyc, 1, n_token, 5, [1], None)
    assert generation.compile_constraints(cyc, 1, n_token, 2, [1], None) is not None
    # the host paths refuse: the one-song GEMV path and the numpy samplers
    with pytest.raises(ValueError, match="generate_batch\\(n_songs=1, constraints"):
        generation.generate(None, w2e, n_songs=1, constraints=c, stats_path=None, log=lambda *a: None)
    with pytest.raises(ValueError, match="3 entries for 2 songs"):
        generation.generate(None, w2e, n_songs=2, constraints=[c, c, c], slots=2, stats_path=None,
                            log=lambda *a: None)


def test_violations_and_bar_boundary():
    from rlmg_amd import generation
    w2e = _w2e()
    # bar 1 allows chord_2, bar 2 chord_3; tempo fixed to tempo_4 throughout
    c = generation.Constraint(w2e, allow={"tempo": ["tempo_4"]}, per_bar={"chord": [["chord_2"], ["chord_3"]]})

    def row(tempo=0, chord=0, bb=0, pitch=0):
        return [tempo, chord, bb, pitch, 0, 0]

    song = np.array([
        row(4, 2, 2),          # 0: bar 1, ok
        row(1, 1, 3),          # 1: CONTI / CONTI, ok
        row(0, 3, 4),          # 2: chord_3 in bar 1: violation
        row(0, 2, 1),          # 3: the Bar that opens bar 2, drawn under bar 1: chord_2 ok
        row(0, 2, 2),          # 4: bar 2, chord_2: violation
        row(5, 3, 2),          # 5: tempo_5: violation
        row(0, 0, 0, 7),       # 6: note row: ok
        row(0, 3, 5),          # 7: Bar (class 5) opening bar 3, chord_3 under bar 2: ok
        row(0, 3, 2),          # 8: bar 3 clamps to bar 2's entry: ok
    ])
    assert c.violations(song) == [2, 4, 5]
    # started at bar 2 (a prompt's count): rows 0, 3 and 4 break the bar-2 entry (bar 3 clamps to it), row 2 does not
    assert c.violations(song, bar0=2) == [0, 3, 4, 5]
    assert c.violations(song[:0]) == []
    assert c.violations(np.array([row(4, 2, 9)])) == [0]            # an id out of range is a violation
    cyc = generation.Constraint(w2e, per_bar={"chord": [["chord_2"], ["chord_3"]]}, cycle=True)
    assert cyc.violations(song) == [2, 4, 8]                         # bar 3 cycles back to chord_2

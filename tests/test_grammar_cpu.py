"""CPU: the CW row grammar -- the three new entries (cwlt_sample_categorical_grammar,
cwlt_score_categorical_grammar, cwlt_grammar_track) are declared, bound, exported and versioned and refuse bad arguments
without a GPU; generation.Grammar compiles names to the order / gram tables, tracks the position in the bar, finds
ill-formed rows, and refuses constraints that would leave a draw no class; the float64 restatement of the grammar
draw's log-probs against a literal per-row walk."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cwlt_sample_categorical_grammar", "cwlt_score_categorical_grammar", "cwlt_grammar_track"]
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
N_CLASS = [56, 135, 18, 87, 18, 25]
OFF = np.concatenate([[0], np.cumsum(N_CLASS)])
NOTE, BAR, BEAT = 0, 1, 2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


def _w2e():
    """Class 0 = 0 everywhere, CONTI = class 1 of tempo / chord, bar-beat = 0, Bar, Beat_0 .. Beat_15."""
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(c)} for k, c in zip(KEYS, N_CLASS)}
    for k in KEYS:
        w2e[k][0] = 0
    w2e["tempo"][1] = w2e["chord"][1] = "CONTI"
    w2e["bar-beat"] = {0: 0, 1: "Bar", **{2 + k: "Beat_%d" % k for k in range(16)}}
    return w2e


def _grammar():
    from rlmg_amd import generation
    return generation.Grammar(_w2e())


def _row(bb, tempo=0, chord=0, pitch=0, dur=0, vel=0):
    return [tempo, chord, bb, pitch, dur, vel]


BAR_ROW = _row(1)


def _beat(k, tempo=1, chord=1):
    return _row(2 + k, tempo, chord)


def _note(pitch=40, dur=3, vel=7):
    return _row(0, 0, 0, pitch, dur, vel)


# ---- the entries -----------------------------------------------------------------------------------------------------
def test_entries_declared_in_header():
    text = open(os.path.join(ROOT, "include", "cwlt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_entries_bound_and_exported(built):
    lib = built.load()
    for name in NAMES:
        assert name in built._SIGNATURES and name in built.exported_names() and hasattr(lib, name), name
    from rlmg_amd import generation, ops, sampling
    for fn in ("sample_categorical_grammar", "score_categorical_grammar", "grammar_track"):
        assert callable(getattr(ops, fn)), fn
    assert callable(generation.Grammar) and callable(generation.compile_grammar)
    assert callable(sampling.grammar_logprobs_f64) and callable(sampling.grammar_allowed_f64)


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 26
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_grammar_sampler_refusals_without_gpu(built):
    lib = built.load()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    nc = (ctypes.c_int * 6)(*N_CLASS)                                # 339 classes: 11 words

    def draw(logits=buf, n_attr=6, rows=4, ld=339, counter=buf, key=null, step=null, bar=null, sched=null, masks=null,
             mask_words=11, beat=buf, order=buf, n_order=18, gram=buf, gram_words=11, bar_attr=2, tokens=buf,
             logp=null, out_counter=null, out_rows=1):
        return lib.cwlt_sample_categorical_grammar(logits, nc, None, None, n_attr, rows, ld, 7, counter, key, step, bar,
                                                   sched, 2, masks, 3, mask_words, beat, order, n_order, gram,
                                                   gram_words, bar_attr, tokens, logp, out_counter, out_rows, null)

    for kw in ({"logits": null}, {"tokens": null}, {"beat": null}, {"order": null}, {"gram": null}):
        assert draw(**kw) == 1001, kw
    assert draw(bar_attr=6) == 1001 and draw(bar_attr=-1) == 1001
    assert draw(n_order=17) == 1001                                  # fewer order entries than bar-beat classes
    assert draw(gram_words=10) == 1001 and draw(gram_words=0) == 1001
    assert draw(bar=buf, sched=buf, masks=buf, mask_words=10) == 1001
    assert draw(bar=buf, sched=buf) == 1001                          # a partial constraint table
    assert draw(counter=null) == 1001                                # neither key nor counter
    assert draw(key=buf) == 1001 and draw(step=buf) == 1001
    assert draw(logp=buf, out_rows=0) == 1001 and draw(logp=buf, out_rows=2) == 1001   # a ring needs its counter
    assert draw(rows=0) == 1001 and draw(rows=(1 << 20) + 1) == 1001 and draw(ld=338) == 1001 and draw(n_attr=9) == 1001

    def score(logits=buf, rows=4, ld=339, targets=buf, key=null, bar=null, sched=null, masks=null, mask_words=11,
              beat=buf, order=buf, n_order=18, gram=buf, gram_words=11, bar_attr=2, out=buf):
        return lib.cwlt_score_categorical_grammar(logits, nc, None, None, 6, rows, ld, targets, key, bar, sched, 2,
                                                  masks, 3, mask_words, beat, order, n_order, gram, gram_words,
                                                  bar_attr, out, null)

    for kw in ({"logits": null}, {"targets": null}, {"out": null}, {"beat": null}, {"order": null}, {"gram": null}):
        assert score(**kw) == 1001, kw
    assert score(bar_attr=6) == 1001 and score(bar_attr=-1) == 1001
    assert score(n_order=17) == 1001 and score(gram_words=10) == 1001
    assert score(masks=buf) == 1001 and score(bar=buf, sched=buf, masks=buf, mask_words=10) == 1001
    assert score(rows=0) == 1001 and score(rows=(1 << 20) + 1) == 1001 and score(ld=338) == 1001


def test_grammar_track_refusals_without_gpu(built):
    lib = built.load()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)

    def call(tokens=buf, rows=4, n_attr=6, bar_attr=2, order=buf, n_order=18, fresh=null, song=null, beat0=null,
             n_songs=0, beat=buf):
        return lib.cwlt_grammar_track(tokens, rows, n_attr, bar_attr, order, n_order, fresh, song, beat0, n_songs, beat,
                                      null)

    for kw in ({"tokens": null}, {"order": null}, {"beat": null}):
        assert call(**kw) == 1001, kw
    assert call(rows=0) == 1001 and call(rows=(1 << 20) + 1) == 1001
    assert call(bar_attr=6) == 1001 and call(bar_attr=-1) == 1001 and call(n_attr=0) == 1001 and call(n_attr=9) == 1001
    assert call(n_order=0) == 1001
    assert call(fresh=buf) == 1001 and call(fresh=buf, song=buf) == 1001          # fresh, song, beat0 go together
    assert call(fresh=buf, song=buf, beat0=buf, n_songs=0) == 1001


# ---- Grammar -----------------------------------------------------------------------------------------------------------
def _bits(gram):
    return np.unpackbits(gram.view(np.uint8), axis=1, bitorder="little")[:, :OFF[-1]].astype(bool)


def test_tables_bits_for_each_kind():
    g = _grammar()
    order, gram = g.tables()
    assert order.dtype == np.int32 and list(order) == [-2, -1] + list(range(16))
    assert gram.dtype == np.uint32 and gram.shape == (3, 11)
    bits = _bits(gram)
    seg = lambda kind, a: bits[kind, OFF[a]:OFF[a + 1]]
    only0 = lambda x: x[0] and not x[1:].any()
    not0 = lambda x: not x[0] and x[1:].all()
    for a in (0, 1):                                                 # tempo, chord
        assert only0(seg(NOTE, a)) and only0(seg(BAR, a)) and not0(seg(BEAT, a))
    for a in (3, 4, 5):                                              # pitch, duration, velocity
        assert not0(seg(NOTE, a)) and only0(seg(BAR, a)) and only0(seg(BEAT, a))
    assert list(np.nonzero(seg(NOTE, 2))[0]) == [0]
    assert list(np.nonzero(seg(BAR, 2))[0]) == [1]
    assert list(np.nonzero(seg(BEAT, 2))[0]) == list(range(2, 18))
    assert not np.unpackbits(gram.view(np.uint8), axis=1, bitorder="little")[:, OFF[-1]:].any()   # padding bits clear
    assert g.kind(0) == NOTE and g.kind(1) == BAR and g.kind(9) == BEAT and g.kind(18) is None


def test_vocabulary_forms_and_refusals():
    from rlmg_amd import generation
    w2e = _w2e()
    # beats= names the indices of classes whose names do not; two Bar classes
    odd = {k: dict(v) for k, v in w2e.items()}
    odd["bar-beat"][5] = "Bar"
    odd["bar-beat"][6] = "downbeat"
    g = generation.Grammar(odd, beats={6: 0})
    assert g.order[5] == -1 and g.order[6] == 0 and g.order[7] == 5 and g.bar_ids == [1, 5]
    with pytest.raises(ValueError, match="neither"):
        generation.Grammar(odd)
    with pytest.raises(ValueError, match="beats"):
        generation.Grammar(odd, beats={6: 0, 40: 1})
    with pytest.raises(ValueError, match="unknown attribute"):
        generation.Grammar(w2e, bar_attr="barbeat")
    with pytest.raises(ValueError, match="unknown attribute"):
        generation.Grammar(w2e, note=("pitch", "length"))
    with pytest.raises(ValueError, match="two roles"):
        generation.Grammar(w2e, metrical=("tempo", "pitch"))
    nobar = {k: dict(v) for k, v in w2e.items()}
    nobar["bar-beat"][1] = "Beat_16"
    with pytest.raises(ValueError, match="Bar"):
        generation.Grammar(nobar)
    # an attribute without a role is left alone by every kind
    g = generation.Grammar(w2e, metrical=("tempo",))
    assert all(g.allowed(kind)[1].all() for kind in (NOTE, BAR, BEAT))


def test_beat_states():
    g = _grammar()
    song = np.array([BAR_ROW, _beat(0), _note(), _note(), _beat(7), _note(), BAR_ROW, _beat(15), _note()])
    before, final = g.beat_states(song)
    assert list(before) == [-1, -1, 0, 0, 0, 7, 7, -1, 15] and final == 15
    assert g.beat_states(song[:1]) [1] == -1 and g.beat_states(song[:5])[1] == 7
    assert g.beat_states(np.zeros((0, 6), dtype=np.int64))[1] == -1
    assert list(g.beat_states(song[2:4], beat=3)[0]) == [3, 3]
    for b in (-1, 0, 7, 15):
        ok = g.position_allowed(b)
        assert ok[1] and ok[0] == (b >= 0) and list(ok[2:]) == [k > b for k in range(16)]


def test_violations_on_hand_written_songs():
    g = _grammar()
    good = np.array([BAR_ROW, _beat(0, 5, 9), _note(), _beat(4), _note(60, 1, 1), BAR_ROW, BAR_ROW, _beat(15), _note()])
    assert g.violations(good) == []

    def bad_at(t, row):
        s = good.copy()
        s[t] = row
        return g.violations(s)

    assert bad_at(3, _row(2 + 4, 1, 1, pitch=40)) == [3]             # a Beat with a pitch
    assert bad_at(3, _beat(0)) == [3]                                # Beat_0 after Beat_0: beats ascend strictly
    assert bad_at(6, _row(1, tempo=3)) == [6]                        # a Bar with a tempo
    assert bad_at(4, _row(0, 0, 0, 60, 0, 1)) == [4]                 # a half note: duration class 0
    assert bad_at(4, _row(0, 0, 0, 0, 0, 0)) == [4]                  # an all-zero row
    assert bad_at(1, _beat(0, 0, 1)) == [1]                          # a Beat without a tempo class
    s = np.array([BAR_ROW, _beat(9), _note(), _beat(3), _note()])    # a descending beat: Beat_3 after Beat_9
    assert g.violations(s) == [3]
    s = np.array([BAR_ROW, _note(), _beat(2), _note()])              # a note straight after Bar
    assert g.violations(s) == [1]
    # prompt rows are tracked, not checked: the same rows as a prompt leave the position for the drawn rows
    assert g.violations(s, n_prompt=2) == []
    assert g.violations(np.array([BAR_ROW, _beat(9), _beat(3)]), n_prompt=2) == [2]
    out = good.copy()
    out[2, 2] = 18                                                   # a class outside the attribute
    assert 2 in g.violations(out)


def test_compile_grammar_refusals():
    from rlmg_amd import generation
    w2e = _w2e()
    g = generation.Grammar(w2e)
    order, gram = generation.compile_grammar(g, None, 4, N_CLASS, 17)
    assert np.array_equal(order, g.tables()[0]) and np.array_equal(gram, g.tables()[1])
    ok = generation.Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(5, 12)},
                               per_bar={"bar-beat": [["Bar", "Beat_0", "Beat_8"], ["Bar", "Beat_4"]]})
    generation.compile_grammar(g, [ok, None, ok], 3, N_CLASS, 17)
    # tempo restricted without class 0: a note row could carry no tempo
    tight = generation.Constraint(w2e, allow={"tempo": ["tempo_3"]}, keep_neutral=False)
    with pytest.raises(ValueError, match="'tempo'"):
        generation.compile_grammar(g, tight, 3, N_CLASS, 17)
    # pitch restricted to class 0: a note row could carry no pitch
    with pytest.raises(ValueError, match="'pitch'"):
        generation.compile_grammar(g, generation.Constraint(w2e, allow={"pitch": [0]}), 3, N_CLASS, 17)
    # a bar-beat schedule whose second bar lacks a Bar class
    nobar = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar", "Beat_0"], ["Beat_4"]]})
    with pytest.raises(ValueError, match="no Bar class in bar 2"):
        generation.compile_grammar(g, [None, nobar], 2, N_CLASS, 17)
    with pytest.raises(ValueError, match="classes"):
        generation.compile_grammar(g, None, 2, N_CLASS[:-1] + [26], 17)
    with pytest.raises(ValueError, match="Grammar"):
        generation.compile_grammar("grammar", None, 2, N_CLASS, 17)


def test_host_paths_refuse_grammar():
    from rlmg_amd import generation
    with pytest.raises(ValueError, match="batch_size or slots"):
        generation.generate(None, _w2e(), 2, grammar=_grammar(), stats_path=None, log=lambda *a: 0)


# ---- the float64 restatement against a literal walk ---------------------------------------------------------------------
def _walk(logits, target, beat, constraint, temperature, top_p):
    """One row, literally: the allowed sets by hand from the kind table and the position rule, then per attribute a
    softmax with temperature over the allowed classes and the reference's nucleus walk."""
    bb = int(target[2])
    sets = []
    for a in range(6):
        ok = np.zeros(N_CLASS[a], dtype=bool)
        for c in range(N_CLASS[a]):
            if a == 2:                                               # bar-beat: the position rule
                yes = c == 1 or (c >= 2 and c - 2 > beat) or (c == 0 and beat >= 0)
            elif bb == 0:                                            # NOTE
                yes = (c == 0) if a in (0, 1) else (c != 0)
            elif bb == 1:                                            # BAR
                yes = c == 0
            else:                                                    # BEAT
                yes = (c != 0) if a in (0, 1) else (c == 0)
            ok[c] = yes and (constraint is None or constraint[a][c])
        sets.append(ok)
    out = np.zeros((6, 2))
    for a in range(6):
        x = np.asarray(logits[a], dtype=np.float64)
        c, ok = int(target[a]), sets[a]
        out[a, 0] = x[c] - x.max() - np.log(np.exp(x - x.max()).sum())
        if not ok[c]:
            out[a, 1] = -np.inf
            continue
        v = x / temperature[a]
        e = np.zeros(len(x))
        e[ok] = np.exp(v[ok] - v[ok].max())
        probs = e / e.sum()
        kept = [i for i in range(len(x)) if ok[i]]
        if top_p[a] is not None and top_p[a] < 1:
            p2 = probs / (probs.sum() + 1e-5)
            kept, run = [], 0.0
            for i in sorted(range(len(x)), key=lambda i: (-p2[i], -i)):
                kept.append(i)
                run += p2[i]
                if run > top_p[a]:
                    break
            kept = [i for i in kept if ok[i]]
        out[a, 1] = np.log(probs[c] / probs[kept].sum()) if c in kept else -np.inf
    return out


@pytest.mark.parametrize("seed", range(4))
def test_restatement_matches_literal_walk(seed):
    from rlmg_amd import generation
    from rlmg_amd.sampling import grammar_allowed_f64, grammar_logprobs_f64
    g = _grammar()
    order = g.tables()[0]
    gram = [g.allowed(kind) for kind in (NOTE, BAR, BEAT)]
    rng = np.random.default_rng(seed)
    settings = [(generation.DQN_TEMPERATURE, generation.DQN_TOP_P), ((1.0,) * 6, (None,) * 6)]
    inf = fin = 0
    for it in range(60):
        temperature, top_p = settings[it % 2]
        logits = [rng.normal(0, 2.5, n) for n in N_CLASS]
        if it % 3 == 0:
            logits = [np.round(x) for x in logits]                   # ties
        beat = int(rng.integers(-1, 16))
        constraint = None
        if it % 4 < 2:
            constraint = [rng.random(n) < 0.7 for n in N_CLASS]
        bb = int(rng.choice([0, 1, int(rng.integers(2, 18))]))
        target = [int(rng.integers(0, n)) for n in N_CLASS]
        target[2] = bb
        if it % 5:                                                   # mostly well-formed rows, some random ones
            kind_sets = gram[g.kind(bb)]
            for a in (0, 1, 3, 4, 5):
                target[a] = int(rng.choice(np.nonzero(kind_sets[a])[0]))
        got = grammar_logprobs_f64(logits, target, beat, order, gram, 2, temperature, top_p, constraint)
        want = _walk(logits, target, beat, constraint, temperature, top_p)
        assert got.shape == (6, 2)
        assert np.abs(got[:, 0] - want[:, 0]).max() < 1e-12
        for a in range(6):
            both_inf = np.isneginf(got[a, 1]) and np.isneginf(want[a, 1])
            assert both_inf or abs(got[a, 1] - want[a, 1]) < 1e-12, (it, a, got[a], want[a])
            inf += both_inf
            fin += not both_inf
        sets = grammar_allowed_f64(bb, beat, order, gram, 2, constraint)
        assert list(sets[2][2:]) == [k > beat and (constraint is None or constraint[2][2 + k]) for k in range(16)]
    assert inf > 20 and fin > 150                                    # both outcomes were exercised
    # a bar-beat target outside the attribute, or one the grammar never allows: no class of any other attribute
    never = order.copy()
    never[17] = -3
    for bb, o in ((18, order), (17, never)):
        sets = grammar_allowed_f64(bb, 3, o, gram, 2)
        assert all(not sets[a].any() for a in (0, 1, 3, 4, 5))

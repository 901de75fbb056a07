"""GPU: soft preferences for generation.

1. cwlt_prefer_logits, cwlt_prefer_track and cwlt_prefer_scan bitwise against their numpy float32 restatements
   (sampling.prefer_logits_f32, Preference.seen_states): three class sets, rows 1 / 2 / 257 / 8192 (the grid-stride
   loop's second pass), the scalar and the 16-byte layouts, padding columns that keep a sentinel, in place, keys absent,
   in range, -1, -2 and n_songs, bar counts 0, 1, R and R + 3, songs with 0 bias rows, no bias table, seen NULL, zero,
   integer and fractional; track row by row equals scan equals seen_states for decay 1, 0.5 and 0.9.
2. Generation on the small fixture model: a neutral preference changes no song; the stream equals the lock-step loop
   bitwise from scratch, from a shared prompt and from per-song prompts, graph or eager, with constraints + grammar +
   log-probs, and under a blend; a bias of -1e30 bans, a presence penalty of 1e30 forbids repeats; drawn log-probs agree
   with score_songs; policy_stats; batch invariance of the scorer; the per-token launch lists; the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402
from rlmg_amd.generation import Constraint, Grammar, Preference  # noqa: E402
from rlmg_amd.sampling import prefer_logits_f32  # noqa: E402
from test_blend_gpu import FIX, N_CLASS, SENTINEL, _bits, _same, _small_model, _strided, _word2event  # noqa: E402

pytestmark = pytest.mark.gpu
CLASSES = {"fixture": [56, 135, 18, 87, 18, 25], "edges": [1, 2, 7, 64, 256], "eight": [3] * 8}
ROWS = (1, 2, 257, 8192)
A = len(N_CLASS)
PEN_ROWS = 5                                                          # songs of the kernel tests' tables


def _up4(n):
    return -(-n // 4) * 4


LAYOUTS = {
    # name: (ld of logits / out, ld of seen, ld of bias as functions of W, base offset in floats, the 16-byte path)
    "width": (lambda W: W, lambda W: W, lambda W: W, 0, None),
    "width+1, base+1": (lambda W: W + 1, lambda W: W + 2, lambda W: W, 1, False),
    "width+5": (lambda W: W + 5, lambda W: W + 3, lambda W: W + 1, 0, None),
    "vector": (lambda W: _up4(W) + 8, lambda W: _up4(W) + 4, lambda W: _up4(W), 0, True),
}


def _bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def _expect(x, n_class, key, bar, sched, bias, pen, seen):
    """The restatement row by row: rows of one song go through prefer_logits_f32 together; a row without a song in the
    tables is copied."""
    W = sum(n_class)
    k = np.arange(len(x)) if key is None else key
    out = x[:, :W].copy()
    for song in np.unique(k[(k >= 0) & (k < len(pen))]):
        idx = np.nonzero(k == song)[0]
        b = None
        if bias is not None and sched[song, 1] > 0:
            j = np.clip((bar[idx] if bar is not None else np.ones(len(idx), np.int64)) - 1, 0, sched[song, 1] - 1)
            b = bias[sched[song, 0] + j][:, :W]
        out[idx] = prefer_logits_f32(x[idx], n_class, b, pen[song], None if seen is None else seen[idx])
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("classes", list(CLASSES))
def test_prefer_logits_bitwise(cuda, classes, layout):
    n_class = CLASSES[classes]
    n_attr, W = len(n_class), sum(n_class)
    f_ld, f_seen, f_bias, offset, vec = LAYOUTS[layout]
    ld, ld_seen, ld_bias = f_ld(W), f_seen(W), f_bias(W)
    if vec:                                                           # the layout is on the path it is meant for
        assert ld % 4 == 0 and ld_seen % 4 == 0 and ld_bias % 4 == 0 and offset == 0
    elif vec is False:
        assert offset % 4 != 0
    rng = np.random.default_rng(100 + 10 * list(CLASSES).index(classes) + list(LAYOUTS).index(layout))
    R = 4
    sched = np.array([[0, 3], [3, 1], [0, 0], [1, 2], [0, R]], dtype=np.int64)          # song 2: no bias rows
    bias_d, bias = _strided(cuda, rng, R, W, ld_bias, 0, fill=rng.normal(0, 4, (R, W)).astype(np.float32))
    pen = np.zeros((PEN_ROWS, 2 * n_attr + 1), dtype=np.float32)
    pen[:, :2 * n_attr] = rng.uniform(-1, 3, (PEN_ROWS, 2 * n_attr))
    pen[1, n_attr:2 * n_attr] = 1e30                                  # a presence penalty that forbids
    pen[3] = 0                                                        # a song with a bias and no penalty
    pen[:, -1] = [1.0, 0.5, 0.9, 0.0, 0.25]
    sched_d, pen_d = torch.as_tensor(sched).to(cuda), torch.as_tensor(pen).to(cuda)
    cases = 0
    for rows in ROWS:
        xd, x = _strided(cuda, rng, rows, W, ld, offset)
        keys = {"none": None, "keyed": rng.integers(0, PEN_ROWS, rows).astype(np.int64)}
        bad = rng.choice(rows, size=min(rows, 3), replace=False)
        keys["keyed"][bad] = np.array([PEN_ROWS, -1, -2], dtype=np.int64)[:len(bad)]
        bars = {"none": None, "mixed": rng.choice([0, 1, R, R + 3, 2], rows).astype(np.int64)}
        seens = {"null": None, "zero": np.zeros((rows, W), np.float32),
                 "int": rng.integers(0, 4, (rows, W)).astype(np.float32),
                 "frac": (rng.integers(0, 2, (rows, W)) * rng.uniform(0, 3, (rows, W))).astype(np.float32)}
        for key_m, bar_m, seen_m, table, inplace in (
                ("none", "none", "null", True, False), ("none", "mixed", "int", True, True),
                ("keyed", "mixed", "frac", True, False), ("keyed", "mixed", "frac", True, True),
                ("keyed", "none", "zero", True, False), ("keyed", "mixed", "null", True, True),
                ("keyed", "mixed", "frac", False, True), ("none", "none", "int", False, False)):
            key, bar, seen = keys[key_m], bars[bar_m], seens[seen_m]
            sd = None if seen is None else _strided(cuda, rng, rows, W, ld_seen, 0, fill=seen)[0]
            kw = dict(sched=sched_d if table else None, bias=bias_d if table else None, pen=pen_d, seen=sd,
                      key=None if key is None else torch.as_tensor(key).to(cuda),
                      bar=None if bar is None else torch.as_tensor(bar).to(cuda))
            if inplace:
                buf, _ = _strided(cuda, rng, rows, W, ld, offset, fill=x[:, :W])
                assert ops.prefer_logits(buf, n_class, out=buf, **kw) is buf
            else:
                buf = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=cuda)
                ops.prefer_logits(xd, n_class, out=buf, **kw)
            got = buf.cpu().numpy()
            where = (rows, key_m, bar_m, seen_m, table, inplace)
            assert (got[:, W:] == SENTINEL).all(), (where, "padding columns written")
            assert (xd.cpu().numpy() == x).all(), (where, "the input was written")
            want = _expect(x, n_class, key, bar, sched, bias if table else None, pen, seen)
            assert _bit_equal(got[:, :W], want), (where, int((got[:, :W] != want).sum()))
            k = np.arange(rows) if key is None else key
            copied = (k < 0) | (k >= PEN_ROWS)
            assert _bit_equal(got[copied][:, :W], x[copied][:, :W]), where
            cases += 1
        if rows >= PEN_ROWS:                                          # something did move
            assert not _bit_equal(got[:, :W], x[:, :W])
    # a new tensor
    got = ops.prefer_logits(xd, n_class, sched=sched_d, bias=bias_d, pen=pen_d)
    assert got.shape == (ROWS[-1], W) and _bit_equal(got.cpu().numpy(),
                                                     _expect(x, n_class, None, None, sched, bias, pen, None))
    assert cases == 8 * len(ROWS)


def _songs_of(rng, n_class, n, L):
    return np.stack([np.stack([rng.integers(0, c, L) for c in n_class], 1) for _ in range(n)]).astype(np.int64)


@pytest.mark.parametrize("classes", list(CLASSES))
def test_track_equals_scan_equals_seen_states(cuda, classes):
    n_class = CLASSES[classes]
    n_attr, W, L = len(n_class), sum(n_class), 40
    w2e = {"a%d" % a: {i: "e%d_%d" % (a, i) for i in range(n)} for a, n in enumerate(n_class)}
    rng = np.random.default_rng(7 + list(CLASSES).index(classes))
    decays = (1.0, 0.5, 0.9)
    prefs = [Preference(w2e, repeat={"a0": 1.0}, decay=d) for d in decays]
    songs = _songs_of(rng, n_class, len(decays), L)
    songs[:, :, 0] = rng.integers(0, min(3, n_class[0]), (len(decays), L))   # few classes: states above 1
    want = np.stack([p.seen_states(s) for p, s in zip(prefs, songs)])        # (3, L, W)
    pen = np.stack([p.penalties() for p in prefs] + [np.zeros(2 * n_attr + 1, np.float32)])
    pen_d = torch.as_tensor(pen).to(cuda)
    toks = torch.as_tensor(songs.reshape(-1, n_attr)).to(cuda)
    # scan: keyed (the songs' own rows of pen), keyless (song i is row i), and a permuted key
    key = torch.arange(len(decays), device=cuda).repeat_interleave(L)
    for k in (key, None):
        rows = ops.prefer_scan(toks, len(decays), n_class, pen_d, key=k)
        assert _bit_equal(rows.cpu().numpy().reshape(len(decays), L, W), want), (classes, k is None)
    perm = [2, 0, 1]
    rows = ops.prefer_scan(torch.as_tensor(songs[perm].reshape(-1, n_attr)).to(cuda), 3, n_class, pen_d,
                           key=torch.as_tensor(np.repeat(perm, L)).to(cuda))
    assert _bit_equal(rows.cpu().numpy().reshape(3, L, W), want[perm])
    out = torch.full((len(decays) * L, W + 3), SENTINEL, dtype=torch.float32, device=cuda)
    assert ops.prefer_scan(toks, len(decays), n_class, pen_d, key=key, out=out) is out
    assert (out[:, W:] == SENTINEL).all() and _bit_equal(out[:, :W].cpu().numpy().reshape(3, L, W), want)
    # track, one launch per row, on a strided state with a sentinel beside it
    seen = torch.full((len(decays), W + 3), SENTINEL, dtype=torch.float32, device=cuda)
    seen[:, :W] = 0
    for t in range(L):
        ops.prefer_track(torch.as_tensor(songs[:, t]).to(cuda).contiguous(), n_class, pen_d, seen)
        assert _bit_equal(seen[:, :W].cpu().numpy(), want[:, t]), (classes, t)
    assert (seen[:, W:] == SENTINEL).all()
    assert want[0].max() >= 3 and (want[1] != np.round(want[1])).any()


def test_track_fresh_rows_and_rows_without_a_song(cuda):
    n_class = CLASSES["fixture"]
    n_attr, W = len(n_class), sum(n_class)
    rng = np.random.default_rng(3)
    pen = np.zeros((3, 2 * n_attr + 1), dtype=np.float32)
    pen[:, -1] = [1.0, 0.5, 0.9]
    seen0 = rng.uniform(0, 3, (3, W)).astype(np.float32)
    before = rng.uniform(0, 2, (6, W)).astype(np.float32)
    tok = _songs_of(rng, n_class, 1, 6)[0]
    song = np.array([2, -1, 0, -2, 1, 3], dtype=np.int64)
    fresh = np.array([1, 1, 0, 1, 0, 0], dtype=np.int64)
    seen = torch.as_tensor(before).to(cuda)
    up = lambda v: torch.as_tensor(v).to(cuda)
    ops.prefer_track(up(tok), n_class, up(pen), seen, fresh=up(fresh), song=up(song), seen0=up(seen0))
    got = seen.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(n_class)[:-1]])
    assert _bit_equal(got[0], seen0[2])                               # fresh with a song: that song's start
    for n in (1, 3, 5):                                               # idle, waiting, past the table: left alone
        assert _bit_equal(got[n], before[n]), n
    for n, k in ((2, 0), (4, 1)):
        hit = np.zeros(W, dtype=np.float32)
        hit[off + tok[n]] = 1.0
        want = before[n] * pen[k, -1]
        assert _bit_equal(got[n], want + hit), n


# ---- 2. generation -----------------------------------------------------------------------------------------------------
N_SONGS, SLOTS, BAR_COND, CAP, SEED = 8, 3, 4, 48, 21
P0 = [[0, 0, 1, 0, 0, 0]]
P1 = P0 + [[1, 1, 2, 0, 0, 0], [0, 0, 0, 5, 3, 2]]
P2 = P1 + [[0, 0, 0, 7, 3, 2], [0, 0, 0, 5, 2, 2]]
P3 = P0 + [[1, 1, 2, 0, 0, 0], [0, 0, 0, 9, 3, 2], [0, 0, 1, 0, 0, 0], [1, 1, 2, 0, 0, 0]]
PROMPTS = [np.array((P0, P1, P2, P3)[i % 4], dtype=np.int64) for i in range(N_SONGS)]
SHARED = np.array(P2, dtype=np.int64)


@pytest.fixture(scope="module")
def world(cuda):
    seed = int(FIX["fill_seed"])
    w2e = _word2event()
    scale = Preference(w2e, bias={"pitch": {k: 2.0 for k in range(5, 12)}, "bar-beat": {"Bar": 1.0}})
    chords = Preference(w2e, per_bar={"chord": [{2: 3.0}, {5: 3.0, 6: 3.0}, {"chord_7": 3.0}]}, cycle=True,
                        bias={"bar-beat": {"Bar": 1.5}})
    forget = Preference(w2e, repeat={"pitch": (0.5, 2.0), "duration": 1.0}, decay=0.9)
    both = Preference(w2e, per_bar={"velocity": [{2: 2.0}, {3: 2.0}]}, repeat={"pitch": (0.0, 5.0)})
    outside = [c for c in range(1, N_CLASS[3]) if c not in range(5, 12)]
    return {"net": _small_model(cuda, seed), "ref": _small_model(cuda, seed + 1), "w2e": w2e,
            "mixed": [scale, chords, forget, None, both, chords, None, forget],
            "ban": Preference(w2e, bias={"pitch": {c: -1e30 for c in outside}}),
            "range": Constraint(w2e, allow={"pitch": range(5, 12)}),
            "once": Preference(w2e, repeat={"pitch": (0, 1e30)}, decay=1)}


def _batch(w, n=N_SONGS, cap=CAP, **kw):
    torch.manual_seed(SEED)
    kw.setdefault("sampler", "categorical")
    return generation.generate_batch(w["net"], w["w2e"], n, bar_cond=BAR_COND, max_tokens=cap, chunk=16,
                                     prefill="gemm", **kw)


def _stream(w, n=N_SONGS, slots=SLOTS, cap=CAP, **kw):
    torch.manual_seed(SEED)
    kw.setdefault("sampler", "categorical")
    return generation._generate_stream(w["net"], w["w2e"], n, slots=slots, bar_cond=BAR_COND, max_tokens=cap,
                                       chunk=8, **kw)


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_neutral_preference_changes_no_song(world, sampler):
    w = world
    zero = Preference(w["w2e"], bias={"pitch": {5: 0.0}}, per_bar={"chord": [{2: 0.0}, {3: 0.0}]})
    plain = _batch(w, sampler=sampler)
    assert _same(_stream(w, sampler=sampler)[0], plain)
    for neutral in (zero, Preference(w["w2e"]), [zero, None] * 4):
        assert _same(_batch(w, sampler=sampler, preferences=neutral), plain)
        assert _same(_stream(w, sampler=sampler, preferences=neutral)[0], plain)


@pytest.mark.parametrize("start", ["scratch", "shared prompt", "per-song prompts"])
def test_stream_equals_batch(world, monkeypatch, start):
    w = world
    b_kw, s_kw = {"scratch": ({}, {}), "shared prompt": ({"prompts": SHARED}, {"prompt": SHARED}),
                  "per-song prompts": ({"prompts": PROMPTS}, {"prompts": PROMPTS})}[start]
    want = _batch(w, preferences=w["mixed"], **b_kw)
    assert not _same(want, _batch(w, **b_kw))                         # the preferences do move the songs
    got, st = _stream(w, preferences=w["mixed"], **s_kw)
    assert st["graph"] and _same(got, want)
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    got, st = _stream(w, preferences=w["mixed"], **s_kw)
    assert not st["graph"] and _same(got, want)
    assert _same(_batch(w, preferences=w["mixed"], **b_kw), want)     # the eager lock-step loop too


def test_stream_equals_batch_with_constraints_grammar_logprobs(world):
    w = world
    w2e = w["w2e"]
    musical = Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(3, 40)},
                         per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7]]}, cycle=True)
    kw = dict(constraints=[musical if i % 3 else None for i in range(N_SONGS)], grammar=Grammar(w2e),
              return_logprobs=True, preferences=w["mixed"], prompts=PROMPTS)
    songs, lps = _batch(w, **kw)
    assert not any(kw["grammar"].violations(s, len(p)) for s, p in zip(songs, PROMPTS))
    (got, got_lp), _ = _stream(w, **kw)
    assert _same(got, songs) and _bits(got_lp, lps)
    assert not _same(songs, _batch(w, **dict(kw, preferences=None))[0])


def test_stream_equals_batch_under_a_blend(world):
    w = world
    kw = dict(reference=w["ref"], alpha=np.linspace(0.0, 1.5, N_SONGS), preferences=w["mixed"])
    want = _batch(w, **kw)
    assert _same(_stream(w, **kw)[0], want)
    assert not _same(want, _batch(w, **dict(kw, preferences=None)))


def test_a_ban_by_bias(world):
    w = world
    songs = _batch(w, cap=120, preferences=w["ban"])
    assert all(len(s) > 1 for s in songs) and sum(int((s[1:, 3] > 0).sum()) for s in songs) > 0
    assert [w["range"].violations(s[1:], 1) for s in songs] == [[]] * N_SONGS
    free = _batch(w, cap=120)
    assert any(w["range"].violations(s[1:], 1) for s in free)         # the same seed without it: not vacuous


def _repeats(song, n_prompt):
    """Drawn rows of `song` whose non-zero pitch class occurs in an earlier row, prompt included."""
    return [t for t in range(n_prompt, len(song)) if song[t, 3] > 0 and song[t, 3] in song[:t, 3]]


def test_no_repeats(world):
    w = world
    for kw in (dict(prompts=PROMPTS), dict()):
        heads = kw.get("prompts", [np.array(P0)] * N_SONGS)
        songs = _batch(w, cap=60, preferences=w["once"], **kw)
        assert sum(int((s[len(h):, 3] > 0).sum()) for s, h in zip(songs, heads)) >= N_SONGS   # notes are drawn
        assert [_repeats(s, len(h)) for s, h in zip(songs, heads)] == [[]] * N_SONGS
        free = _batch(w, cap=60, **kw)
        assert any(_repeats(s, len(h)) for s, h in zip(free, heads))
    got, _ = _stream(w, cap=60, preferences=w["once"], prompts=PROMPTS)
    assert [_repeats(s, len(h)) for s, h in zip(got, PROMPTS)] == [[]] * N_SONGS


def test_generated_against_scored(world):
    """The bound is test_generated_equals_scored's in test_logprobs_gpu.py, for the decode step against the prefill; the
    penalty terms themselves are bitwise (test_track_equals_scan_equals_seen_states)."""
    w = world
    songs, lps = _batch(w, preferences=w["mixed"], return_logprobs=True, prompts=PROMPTS)
    scored = generation.score_songs(w["net"], w["w2e"], songs, preferences=w["mixed"])
    plain = generation.score_songs(w["net"], w["w2e"], songs)
    worst = 0.0
    for s, p, lp, sc in zip(songs, PROMPTS, lps, scored):
        assert lp.shape == (len(s) - len(p), 6, 2) and sc.shape == (len(s) - 1, 6, 2) and np.isfinite(lp).all()
        worst = max(worst, float(np.abs(lp - sc[len(p) - 1:]).max()))
    print("prefer: generated against scored log-probs, worst |difference| = %.3g" % worst)
    assert worst <= 1e-4
    for k, pref in enumerate(w["mixed"]):                             # the scores are the preferred policy's
        d = float(np.abs(scored[k] - plain[k]).max())
        assert d == 0.0 if pref is None else d > 1e-2, (k, d)


def test_policy_stats_with_preferences(world):
    w = world
    songs = _batch(w, preferences=w["mixed"], prompts=PROMPTS)
    for kw in (dict(), dict(reference=w["ref"]), dict(reference=w["ref"], alpha=0.5)):
        st = generation.policy_stats(w["net"], w["w2e"], songs, preferences=w["mixed"], **kw)
        assert all(x.shape == (len(s) - 1, 6, 4 if "reference" in kw else 2) for x, s in zip(st, songs))
        assert not any(np.isnan(x).any() for x in st), kw
    ban = generation.policy_stats(w["net"], w["w2e"], songs, preferences=w["ban"])
    free = generation.policy_stats(w["net"], w["w2e"], songs)
    assert max(float(x[:, 3, 0].max()) for x in ban) <= np.log(8) + 1e-5      # 8 pitch classes keep mass
    assert max(float(x[:, 3, 0].max()) for x in free) > np.log(8)
    # the reference keeps its own logits: against itself the preferred policy has moved, the plain one has not
    own = generation.policy_stats(w["net"], w["w2e"], songs, reference=w["net"])
    moved = generation.policy_stats(w["net"], w["w2e"], songs, reference=w["net"], preferences=w["ban"])
    assert max(float(np.abs(x[..., 2]).max()) for x in own) <= 2e-5
    assert max(float(x[:, 3, 2].max()) for x in moved) > 1e-2


def test_score_songs_is_batch_invariant(world):
    w = world
    songs = _batch(w, preferences=w["mixed"], prompts=PROMPTS)
    whole = generation.score_songs(w["net"], w["w2e"], songs, preferences=w["mixed"], kernel="gemm")
    blocks = generation.score_songs(w["net"], w["w2e"], songs, preferences=w["mixed"], kernel="gemm", prefill_rows=64)
    assert _bits(whole, blocks)
    perm = [5, 2, 7, 0, 4, 1, 6, 3]
    shuffled = generation.score_songs(w["net"], w["w2e"], [songs[i] for i in perm],
                                      preferences=[w["mixed"][i] for i in perm])
    assert _bits(shuffled, [whole[i] for i in perm])
    for k in (1, 2, 4):
        alone = generation.score_songs(w["net"], w["w2e"], songs[k:k + 1], preferences=w["mixed"][k])
        assert _bits(alone, whole[k:k + 1]), k
    stats = generation.policy_stats(w["net"], w["w2e"], songs, preferences=w["mixed"])
    assert _bits(generation.policy_stats(w["net"], w["w2e"], songs, preferences=w["mixed"], prefill_rows=64), stats)


# ---- the per-token launch lists --------------------------------------------------------------------------------------
PER_TOKEN = ("cwlt_sample_", "cwlt_score_", "cwlt_count_bars", "cwlt_grammar_track", "cwlt_stream_", "cwlt_blend_logits",
             "cwlt_prefer_")
PRE = "cwlt_sample_categorical"


@pytest.fixture
def calls(monkeypatch):
    """Every ops._call of the test by entry name, the call itself forwarded unchanged; graphs off."""
    seen, real = [], ops._call

    def recording(name, *args, **kw):
        seen.append(name)
        return real(name, *args, **kw)

    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    monkeypatch.setattr(ops, "_call", recording)
    return seen


def _per_token(calls):
    return [name for name in calls if name.startswith(PER_TOKEN)]


@pytest.mark.parametrize("mode", ["bias", "schedule", "penalty", "penalty+constraints", "none"])
def test_launch_lists(world, calls, mode):
    w = world
    scale, chords, forget = w["mixed"][0], w["mixed"][1], w["mixed"][2]
    prefs = {"bias": [scale, None, scale], "schedule": [chords, None, scale], "penalty": [forget, None, chords],
             "penalty+constraints": [forget, None, chords], "none": None}[mode]
    cons = [w["range"], None, None] if "constraints" in mode else None
    track = ["cwlt_prefer_track"] if "penalty" in mode else []
    front = [] if prefs is None else ["cwlt_prefer_logits"]
    # the stream: the bar count is the advance's own, whatever needs it
    _, st = _stream(w, n=3, slots=2, cap=12, preferences=prefs, constraints=cons, prompts=PROMPTS[:3])
    pattern = ["cwlt_stream_refill_bank"] + front + [PRE + ("_masked" if cons else "_keyed"),
                                                     "cwlt_stream_advance_bank"] + track
    seen = _per_token(calls)
    assert not st["graph"] and seen == pattern * st["steps"], (mode, seen[:12])
    del calls[:]
    _, st = _stream(w, n=3, slots=2, cap=12, preferences=prefs, constraints=cons)
    pattern = ["cwlt_stream_refill"] + front + [PRE + ("_masked" if cons else "_keyed"), "cwlt_stream_advance"] + track
    seen = _per_token(calls)
    assert seen == pattern * st["steps"], (mode, seen[:12])
    # the lock-step loop: cwlt_count_bars under constraints, or when a bias schedule of several rows needs the count --
    # which does not select the masked sampler
    del calls[:]
    _batch(w, n=3, cap=12, preferences=prefs, constraints=cons)
    bars = ["cwlt_count_bars"] if cons or mode in ("schedule", "penalty") else []
    pattern = front + [PRE + ("_masked" if cons else "_slots")] + bars + track
    seen = _per_token(calls)
    assert len(seen) >= len(pattern) and seen == pattern * (len(seen) // len(pattern)), (mode, seen[:12])
    if prefs is None:
        assert not [name for name in calls if name.startswith("cwlt_prefer_")]
    # the scorers: the scan only under a penalty, the apply once per block
    del calls[:]
    songs = [np.array(P2), np.array(P3), np.array(P1)]
    generation.score_songs(w["net"], w["w2e"], songs, preferences=prefs, constraints=cons)
    generation.policy_stats(w["net"], w["w2e"], songs, preferences=prefs, constraints=cons)
    scan = ["cwlt_prefer_scan"] if "penalty" in mode else []
    assert _per_token(calls) == scan + front + ["cwlt_score_categorical"] + scan + front, mode


def test_refusals_on_the_device(world, tmp_path):
    w = world
    net, w2e = w["net"], w["w2e"]
    quiet = dict(stats_path=None, log=lambda *a: None, path_gendir=str(tmp_path))
    with pytest.raises(ValueError, match="generate_batch\\(n_songs=1, preferences"):
        generation.generate(net, w2e, n_songs=1, preferences=w["ban"], **quiet)
    other = Preference(dict(w2e, velocity={i: i for i in range(N_CLASS[5] + 1)}))
    songs = [np.array(P2), np.array(P3)]
    for fn, args in ((generation.generate_batch, (net, w2e, 2)), (generation.generate_stream, (net, w2e, 2)),
                     (generation.score_songs, (net, w2e, songs)), (generation.policy_stats, (net, w2e, songs))):
        with pytest.raises(ValueError, match="was built for classes"):
            fn(*args, preferences=other)
        with pytest.raises(ValueError, match="preferences: 3 entries for 2 songs"):
            fn(*args, preferences=[w["ban"], None, None])
    for kw in ({"slots": 2}, {"batch_size": 2}):
        with pytest.raises(ValueError, match="preferences: 2 entries for 3 songs"):
            generation.generate(net, w2e, n_songs=3, preferences=[w["ban"], None], **kw, **quiet)
    # the kernel's own refusal reaches Python as an error
    lg = torch.zeros(3, sum(N_CLASS), device=net.in_linear.weight.device)
    with pytest.raises(RuntimeError, match="1001"):
        ops.prefer_logits(lg, N_CLASS, pen=torch.zeros(3, 13, device=lg.device), seen=lg, out=lg)
    # generate() takes them with slots and with batch_size, cut per group, and gives generate_batch's songs
    torch.manual_seed(SEED)
    generation.generate(net, w2e, n_songs=5, bar_cond=BAR_COND, max_tokens=24, batch_size=2,
                        preferences=w["mixed"][:5], **quiet)
    torch.manual_seed(SEED)
    generation.generate(net, w2e, n_songs=5, bar_cond=BAR_COND, max_tokens=24, slots=2, preferences=w["mixed"][:5],
                        **dict(quiet, path_gendir=str(tmp_path / "stream")))
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".npy")]) == 5
    assert len([f for f in os.listdir(tmp_path / "stream") if f.endswith(".npy")]) == 5

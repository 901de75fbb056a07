"""GPU: cwlt_song_metrics against sampling.song_metrics_f32 bit for bit -- features, reward, bars, hist and
groove -- on both sides of the launcher's switch (a wave per song up to 128 rows and 64 slots, 256 threads beyond), with
carries across strides and waves; generation.song_metrics on a ragged list; generation.MetricReward end to end on the small
fixture model through generate_particles (lock-step and slots=) and generate."""
import os

import numpy as np
import pytest
import torch

import rlmg_amd  # noqa: F401
from rlmg_amd import generation, metrics, ops, sampling
from rlmg_amd.generation import Grammar

from test_blend_gpu import FIX, _small_model
from test_metrics_cpu import BAR, C_M, CHORD, bar, beat, note, random_songs, vocabulary
from test_reward_stream_gpu import _differ, _same_sets

pytestmark = pytest.mark.gpu
GUARD = 64
SENT = {torch.float32: -1234567.0, torch.int32: -77777, torch.int64: -7777777777}
WEIGHTS = np.array([0.5, -2.0, 1e30, 0.0, 3.0, -1.0, 7.0, -0.25, 0.0, 1e-3, -4e20], dtype=np.float32)


@pytest.fixture(scope="module")
def spec():
    return metrics.SongMetricSpec(vocabulary())


def _d(cuda, x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(cuda)


def _guarded(cuda, shape, dtype):
    """A sentinel-filled buffer with GUARD elements on either side of the view that is handed to the kernel."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENT[dtype], dtype=dtype, device=cuda)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def _run(cuda, spec, tok, mask=None, lengths=None, max_bars=None, weights=WEIGHTS, outputs=("bars", "hist", "groove")):
    """One launch -> (dict of numpy outputs, the restatement's dict).  Inputs must come back unchanged, the guards
    around every output untouched."""
    N, L, _ = tok.shape
    MB = int(spec.max_bars if max_bars is None else max_bars)
    lengths = None if lengths is None else np.asarray(lengths, dtype=np.int32)
    ins = [_d(cuda, tok), _d(cuda, mask), _d(cuda, lengths)]
    before = [None if t is None else t.clone() for t in ins]
    order, pitch, chord, table = spec.tables(cuda, L + 1)
    shapes = {"feat": ((N, 11), torch.float32), "reward": ((N,), torch.float32), "bars": ((N,), torch.int32),
              "hist": ((N, MB, 12), torch.int32), "groove": ((N, MB), torch.int64)}
    want = ("feat",) + (("reward",) if weights is not None else ()) + tuple(outputs)
    bufs = {k: _guarded(cuda, *shapes[k]) for k in want}
    view = lambda k: bufs[k][1] if k in bufs else None                  # noqa: E731
    ops.song_metrics(ins[0], ins[1], ins[2], spec.attrs, order, pitch, chord, spec.Q, table, MB, view("feat"),
                     weights=_d(cuda, weights), reward=view("reward"), bars=view("bars"), hist=view("hist"),
                     groove=view("groove"))
    torch.cuda.synchronize()
    for t, b in zip(ins, before):
        assert t is None or torch.equal(t, b)
    for k, (whole, v) in bufs.items():
        assert (whole[:GUARD] == SENT[v.dtype]).all() and (whole[-GUARD:] == SENT[v.dtype]).all(), k
    got = {k: v.cpu().numpy() for k, (_, v) in bufs.items()}
    ref = sampling.song_metrics_f32(tok, mask, lengths, spec, weights=weights, max_bars=MB)
    return got, ref


def _bitwise(got, ref, what=""):
    for k, g in got.items():
        r = ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.dtype, r.dtype)
        if g.dtype == np.float32:
            same = g.view(np.int32) == r.view(np.int32)
        else:
            same = g == r
        assert same.all(), (what, k, np.argwhere(~same)[:5].tolist(), g[~same][:5], r[~same][:5])


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 50, 64, 65, 257, 1025])
@pytest.mark.parametrize("N", [1, 5, 300])
def test_kernel_is_the_restatement(cuda, spec, N, L):
    """Random ill-formed rows under a mask with holes, and Grammar-shaped songs under lengths (1 and 0 among them) with
    few slots kept: features, reward, bars, hist and groove bit for bit."""
    rng = np.random.default_rng(1000 * N + L)
    tok = random_songs(rng, N, L, False)
    mask = (rng.random((N, L)) < 0.85).astype(np.int64)
    got, ref = _run(cuda, spec, tok, mask=mask, max_bars=min(L + 1, 512))
    _bitwise(got, ref, "ill-formed")
    assert ref["feat"][:, 0].any() or L == 1
    tok = random_songs(rng, N, L, True)
    lengths = rng.integers(0, L + 1, N)
    lengths[0] = 1
    lengths[-1] = L
    if N == 5:
        tok[1, ::7] = bar()                                             # more slots than the 4 that are kept
        lengths[1] = L
    got, ref = _run(cuda, spec, tok, lengths=lengths, max_bars=4 if N == 5 else min(L + 1, 512))
    _bitwise(got, ref, "well-formed")
    if N == 5 and L >= 50:
        assert ref["bars"][1] > 4                                       # slots beyond max_bars were dropped


@pytest.mark.parametrize("L", [50, 65, 257, 1025])
def test_bar_rows_everywhere(cuda, spec, L):
    """A Bar as the first, the last and every row: B = L (and B > max_bars with max_bars = 4)."""
    rng = np.random.default_rng(L)
    tok = random_songs(rng, 4, L, True)
    tok[0, :] = bar()
    tok[1, -1] = bar()
    tok[2, 0] = note(60)
    tok[2, 1:] = bar()
    tok[3, 0] = bar()
    for mb in (4, min(L + 1, 512)):
        got, ref = _run(cuda, spec, tok, max_bars=mb)
        _bitwise(got, ref, mb)
        assert ref["bars"][0] == L and ref["bars"][2] == L and ref["feat"][2, 0] == 1


def _boundary_songs(L, edges):
    """For every edge e and every way to put a Bar, a chord-setting beat and two notes on rows e-2 .. e+1 in that order
    (the rest of the song padding rows, which are nothing), one song; and the same with the beat far ahead of the
    edge, so that the carry alone brings it to the note."""
    songs = []
    for e in edges:
        for b in range(e - 2, e + 1):
            for s in range(b + 1, e + 2):
                for n in range(s + 1, min(e + 3, L)):
                    song = np.zeros((L, 6), dtype=np.int64)
                    song[b], song[s], song[n] = bar(), beat(5, C_M + 11 * (e % 12)), note(48 + e % 12)     # the chord's root
                    if n + 70 < L:
                        song[n + 70] = note(60 + e % 12)                 # a wave later: beat and chord from the carry
                    songs.append(song)
        song = np.zeros((L, 6), dtype=np.int64)
        song[0], song[1] = beat(3, C_M), note(60)                        # slot 0; set in the first stride
        if e + 1 < L:
            song[e - 1], song[e], song[e + 1] = note(64), note(61), bar()
        songs.append(song)
    return np.stack(songs)


@pytest.mark.parametrize("L,edges", [(128, (64,)), (100, (64,)), (700, (64, 128, 192, 256, 320, 512, 640))])
def test_carries_across_waves_and_strides(cuda, spec, L, edges):
    """A beat or a chord set in one stride and used in the next; the Bar, the setter and the note on either side of a wave
    boundary (row 64 k) and of a stride boundary (row 64 in the wave form, rows 256 k in the block form)."""
    tok = _boundary_songs(L, edges)
    got, ref = _run(cuda, spec, tok, max_bars=8)
    _bitwise(got, ref)
    assert (ref["feat"][:, 6] > 0).all() and (ref["groove"] != 0).any(axis=1).all()


def test_other_columns_and_no_chord(cuda):
    """A = 8 and A = 6 with the three attributes in other columns; chord_attr = -1."""
    w2e = vocabulary()
    rng = np.random.default_rng(8)
    extra = {"x": {0: 0, 1: "x_1"}, "y": {0: 0, 1: "y_1"}}
    wide = {k: (w2e[k] if k in w2e else extra[k])
            for k in ("pitch", "x", "tempo", "bar-beat", "duration", "chord", "velocity", "y")}
    moved = {k: w2e[k] for k in ("bar-beat", "velocity", "pitch", "tempo", "duration", "chord")}
    for vocab, A, cols in ((wide, 8, (5, 3, 0)), (moved, 6, (5, 0, 2))):
        sp = metrics.SongMetricSpec(vocab)
        assert sp.attrs == (cols[1], cols[2], cols[0])
        for L in (50, 300):
            tok = random_songs(rng, 9, L, True, A=A, cols=cols)
            got, ref = _run(cuda, sp, tok, max_bars=min(L + 1, 512))
            _bitwise(got, ref, (A, L))
            assert ref["feat"][:, 6].any()
    off = metrics.SongMetricSpec(w2e, chord_attr=None)
    for L in (50, 300):
        tok = random_songs(rng, 9, L, False)
        tok[:, :, CHORD] = 1 << 33                                       # not read
        got, ref = _run(cuda, off, tok, max_bars=64)
        _bitwise(got, ref, L)
        assert not ref["feat"][:, 6].any() and ref["feat"][:, 0].any()


@pytest.mark.parametrize("L", [50, 300])
def test_optional_outputs(cuda, spec, L):
    """NULL for any of reward / bars / hist / groove leaves the others as they were."""
    rng = np.random.default_rng(L)
    tok = random_songs(rng, 7, L, True)
    full, ref = _run(cuda, spec, tok, max_bars=32)
    _bitwise(full, ref)
    for outputs, weights in (((), None), (("bars",), WEIGHTS), (("hist",), None), (("groove",), WEIGHTS)):
        got, _ = _run(cuda, spec, tok, max_bars=32, weights=weights, outputs=outputs)
        assert set(got) == {"feat"} | set(outputs) | ({"reward"} if weights is not None else set())
        _bitwise(got, ref, outputs)


def test_song_metrics_on_a_ragged_list(cuda, spec):
    rng = np.random.default_rng(3)
    songs = [random_songs(rng, 1, L, True)[0] for L in (1, 37, 64, 129, 700)]
    songs.append(np.array([beat(0), note(60), note(67)]))
    out = generation.song_metrics(spec, songs, device=cuda)
    again = generation.song_metrics(vocabulary(), songs)
    mb = out["hist"].shape[1]
    assert mb == max(int((s[:, BAR] == 1).sum()) for s in songs) + 1 and out["groove_masks"].shape == (6, mb)
    for i, s in enumerate(songs):
        ref = sampling.song_metrics_f32(s[None], None, None, spec, max_bars=mb)
        for f, name in enumerate(metrics.METRICS):
            assert out[name].dtype == np.float32 and out[name][i].view(np.int32) == ref["feat"][0, f].view(np.int32), name
            assert again[name][i].view(np.int32) == out[name][i].view(np.int32)
        assert out["bars"][i] == ref["bars"][0] and np.array_equal(out["hist"][i], ref["hist"][0])
        assert np.array_equal(out["groove_masks"][i], ref["groove"][0])
    assert out["h1"][5] == 1.0 and out["n_bars"][5] == 1
    tok = random_songs(rng, 4, 90, False)
    mask = (rng.random((4, 90)) < 0.7).astype(np.int64)
    out = generation.song_metrics(spec, tok, mask=mask)
    ref = sampling.song_metrics_f32(tok, mask, None, spec, max_bars=out["hist"].shape[1])
    assert np.array_equal(np.stack([out[k] for k in metrics.METRICS], 1).view(np.int32), ref["feat"].view(np.int32))


# ---- 2. MetricReward end to end ---------------------------------------------------------------------------------------------
K4, BAR_COND, CAP, SEED, BETA = 4, 9, 120, 33, 2.0
TERMS = {"in_chord": 1.0, "groove": 0.5, "h1": 0.25, "empty_bars": -1.0, "notes_per_bar": 0.125, "pitch_range": -0.01}


@pytest.fixture(scope="module")
def world(cuda):
    w2e = vocabulary()
    sp = metrics.SongMetricSpec(w2e)
    fn = generation.MetricReward(sp, TERMS)
    return {"net": _small_model(cuda, int(FIX["fill_seed"])), "w2e": w2e, "spec": sp, "fn": fn,
            "kw": dict(bar_cond=BAR_COND, max_tokens=CAP, grammar=Grammar(w2e), sampler="categorical", beta=BETA)}


def _host_reward(sp, weights, calls=None):
    def fn(windows, mask):
        W = windows.shape[1]
        out = sampling.song_metrics_f32(windows.cpu().numpy(), mask.cpu().numpy(), None, sp, weights=weights,
                                        max_bars=min(W + 1, 512))
        if calls is not None:
            calls.append(W)
        return torch.from_numpy(out["reward"]).to(windows.device)
    return fn


def test_metric_reward_on_its_own(cuda, spec):
    """The callable against the restatement on random windows; its buffers are kept per shape; W + 1 > 512 is refused."""
    rng = np.random.default_rng(4)
    fn = generation.MetricReward(spec, TERMS)
    tok = random_songs(rng, 256, 50, True)
    mask = (rng.random((256, 50)) < 0.8).astype(np.int64)
    r = fn(_d(cuda, tok), _d(cuda, mask))
    ref = sampling.song_metrics_f32(tok, mask, None, spec, weights=fn.weights, max_bars=51)
    assert r.dtype == torch.float32 and np.array_equal(r.cpu().numpy().view(np.int32), ref["reward"].view(np.int32))
    assert len(set(ref["reward"].tolist())) > 100
    assert fn(_d(cuda, tok), _d(cuda, mask)).data_ptr() == r.data_ptr() and len(fn._buffers) == 1
    assert fn(_d(cuda, tok[:7]), _d(cuda, mask[:7])).data_ptr() != r.data_ptr() and len(fn._buffers) == 2
    fn(torch.zeros(2, 511, 6, dtype=torch.int64, device=cuda), torch.ones(2, 511, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match="512"):
        fn(torch.zeros(2, 512, 6, dtype=torch.int64, device=cuda), torch.ones(2, 512, dtype=torch.int64, device=cuda))


def test_rewards_are_the_windows_of_the_songs(world):
    """ess=0: the lineage is the identity, so reward j of particle k is the restatement on rows [P + j W, P + (j + 1) W)
    of that particle's own song (P = 1, the initial Bar row), bit for bit."""
    w, W = world, 12
    torch.manual_seed(SEED)
    sets = generation.generate_particles(w["net"], w["w2e"], 3, K4, ess=0, resample_every=6, reward=w["fn"],
                                         reward_window=W, chunk=24, **w["kw"])
    seen = set()
    for ps in sets:
        assert not ps.resampled.any()
        for k in range(K4):
            drawn = ps.songs[k][1:]
            cuts = [drawn[j:j + W] for j in range(0, len(drawn), W)]
            assert len(ps.rewards[k]) == len(cuts)
            for j, rows in enumerate(cuts):
                ref = sampling.song_metrics_f32(rows[None], None, None, w["spec"], weights=w["fn"].weights, max_bars=W + 1)
                assert ps.rewards[k][j].view(np.int32) == ref["reward"][0].view(np.int32), (k, j)
                seen.add(float(ref["reward"][0]))
    assert len(seen) > 3                                                 # the rewards tell windows apart


def test_metric_reward_is_the_host_callable(world):
    """Resampling on: the run under MetricReward is, field by field and bit for bit, the run under a host callable that
    evaluates song_metrics_f32 on the copied windows."""
    w = world
    kw = dict(ess=1.0, resample_every=4, reward_window=8, chunk=16, **w["kw"])
    torch.manual_seed(SEED)
    dev = generation.generate_particles(w["net"], w["w2e"], 3, K4, reward=w["fn"], **kw)
    calls = []
    torch.manual_seed(SEED)
    host = generation.generate_particles(w["net"], w["w2e"], 3, K4, reward=_host_reward(w["spec"], w["fn"].weights, calls),
                                         **kw)
    assert calls and _differ(dev, host) == []
    assert any(ps.resampled.any() for ps in dev) and any((ps.ancestors != np.arange(K4)).any() for ps in dev)
    assert len({float(x) for ps in dev for r in ps.rewards for x in r}) > 3


def test_stream_is_the_lock_step_pool(world):
    """slots= with MetricReward: every set is the lock-step pool's, rewards included (a window is scored from its own
    rows alone, so the score does not depend on the pool)."""
    w = world
    # bar_cond 40: the fixture model closes a bar every few rows, and a song has to outlast a window of 50
    kw = dict(ess=1.0, resample_every=10, reward_window=50, chunk=100, **dict(w["kw"], bar_cond=40, max_tokens=160))
    torch.manual_seed(SEED)
    lock = generation.generate_particles(w["net"], w["w2e"], 5, K4, reward=w["fn"], **kw)
    torch.manual_seed(SEED)
    stream = generation.generate_particles(w["net"], w["w2e"], 5, K4, reward=w["fn"], slots=2, **kw)
    assert _differ(stream, lock) == []
    assert all(_same_sets(a, b) for a, b in zip(stream, lock)) and any(len(r) > 1 for ps in lock for r in ps.rewards)
    assert any(ps.event_rewards.any() for ps in lock)


def test_generate_takes_a_metric_reward(world, tmp_path):
    w = world
    kw = dict(ess=1.0, resample_every=4, reward=w["fn"], reward_window=8,
              **{k: v for k, v in w["kw"].items() if k != "sampler"})       # generate has no sampler=: the default
    torch.manual_seed(SEED)
    first = generation.generate_particles(w["net"], w["w2e"], 3, K4, **kw)
    torch.manual_seed(SEED)
    stats = generation.generate(w["net"], w["w2e"], n_songs=5, batch_size=3, particles=K4, path_gendir=str(tmp_path),
                                stats_path=None, log=lambda s: None, **kw)
    assert len(stats["words_len_list"]) == 5
    for i, ps in enumerate(first):
        song = np.load(os.path.join(str(tmp_path), "get_%d.npy" % i))
        assert any(song.shape == s.shape and (song == s).all() for s in ps.songs) and ps.rewards is not None

"""GPU: continuous batching -- generation.generate_stream (a pool of GEMM-step decode slots refilled on the device as
songs end), its three kernels (csrc/stream.hip, cwlt_sample_categorical_keyed) and generate(slots=...)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]


def _small_model(cuda, dtype=None):
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": 2, "N_HEAD": 2})
    try:
        net = model.LinearTransformer(N_CLASS, is_training=False)
    finally:
        config.AgentConfig.update(old)
    net = fill_params(net, seed=int(FIX["fill_seed"])).to(cuda).eval()
    if dtype is not None:
        net.compute_dtype = dtype
    return net


def _word2event():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    w2e["bar-beat"][9] = "Bar"
    return w2e


def _bars(w2e, rows):
    return np.array([w2e["bar-beat"][int(r[2])] == "Bar" for r in rows])


def _check_cut(w2e, song, prompt_len, bar_cond, max_tokens):
    """The single-song bar rule: the count starts at 1 and counts Bar tokens after the first row; the song ends WITH
    the token that opens bar `bar_cond` (no earlier prefix reaches it), or it has exactly max_tokens rows."""
    cnt = 1 + np.cumsum(_bars(w2e, song[1:]))
    reached = np.nonzero(cnt >= bar_cond)[0]
    if len(song) == max_tokens and (len(reached) == 0 or reached[0] == len(song) - 2):
        return
    assert len(reached) and reached[0] == len(song) - 2, (len(song), prompt_len)
    assert len(song) > prompt_len


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_stream_equals_batch(cuda, sampler):
    net = _small_model(cuda)
    w2e = _word2event()
    torch.manual_seed(11)
    free = generation.generate_batch(net, w2e, 24, bar_cond=4, max_tokens=300, sampler=sampler, chunk=32)
    cap = int(np.median([len(s) for s in free]))            # some songs reach the cap, some end on the bar rule
    torch.manual_seed(12)
    ref = generation.generate_batch(net, w2e, 24, bar_cond=4, max_tokens=cap, sampler=sampler, chunk=32)
    lens = [len(s) for s in ref]
    assert any(n == cap for n in lens) and any(n < cap for n in lens), (cap, lens)
    for slots in (1, 5, 8, 24, 40):
        torch.manual_seed(12)
        got = generation.generate_stream(net, w2e, 24, slots=slots, bar_cond=4, max_tokens=cap, sampler=sampler,
                                         chunk=16)
        assert _same(got, ref), slots
    for s in got:
        assert s[0].tolist() == generation.INIT_CW[0].tolist()
        _check_cut(w2e, s, 1, 4, cap)


def test_stream_graph_equals_eager(cuda, monkeypatch):
    net = _small_model(cuda)
    w2e = _word2event()
    torch.manual_seed(5)
    graphed, st = generation._generate_stream(net, w2e, 12, slots=5, bar_cond=4, max_tokens=120, chunk=8)
    assert st["graph"] and st["drawn"] == sum(len(s) - 1 for s in graphed)
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    torch.manual_seed(5)
    eager, st = generation._generate_stream(net, w2e, 12, slots=5, bar_cond=4, max_tokens=120, chunk=8)
    assert not st["graph"]
    assert _same(graphed, eager)


def test_stream_repo_dims(cuda):
    from rlmg_amd.dqn_policy import model
    n_class = [56, 135, 18, 87, 18, 25]
    net = fill_params(model.LinearTransformer(n_class, is_training=False), seed=5).to(cuda).eval()
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, n_class)}
    w2e["bar-beat"][1] = "Bar"
    torch.manual_seed(7)
    ref = generation.generate_batch(net, w2e, 256, bar_cond=5, max_tokens=256)
    torch.manual_seed(7)
    got = generation.generate_stream(net, w2e, 256, slots=64, bar_cond=5, max_tokens=256, chunk=64)
    assert _same(got, ref)


def test_stream_shared_prompt(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    bars = np.cumsum(_bars(w2e, FIX["tokens"][1:]))
    p_len = int(np.argmax(bars >= 1)) + 2                  # one Bar after the first row: the count starts at 2
    prompt = FIX["tokens"][:p_len]
    outs = []
    for slots in (3, 16):
        torch.manual_seed(9)
        outs.append(generation.generate_stream(net, w2e, 10, slots=slots, bar_cond=4, max_tokens=200, prompt=prompt,
                                               chunk=16))
    assert _same(outs[0], outs[1])
    for s in outs[0]:
        assert s[:p_len].tolist() == prompt.tolist()
        _check_cut(w2e, s, p_len, 4, 200)                  # the prompt's Bar counts toward bar_cond
        if len(s) < 200:
            assert _bars(w2e, s[p_len:]).sum() == 2        # bar 2 -> bar 4: two drawn Bars, the last one ends it


def _advance_model(tokens, mask, bar_cond, bar0, cap, n_songs, song, pos, bar, ctl, ring):
    """numpy model of cwlt_stream_advance (bar attribute 2); updates its arguments, returns the fresh flags."""
    S, A = tokens.shape
    row = ctl[0] % ring.shape[0]
    ended = np.zeros(S, dtype=np.int64)
    for s in range(S):
        if song[s] >= 0:
            bar[s] += int(mask[tokens[s, 2]])
            ended[s] = int(bar[s] >= bar_cond or pos[s] + 1 >= cap)
            pos[s] += 1
    ring[row, :, 0] = song
    ring[row, :, 1:1 + A] = tokens
    ring[row, :, -1] = ended
    nxt = ctl[1]
    for s in np.nonzero(ended)[0]:
        if nxt < n_songs:
            song[s], pos[s], bar[s] = nxt, 0, bar0
        else:
            song[s] = -1
        nxt += 1
    ctl[:] = [ctl[0] + 1, min(nxt, n_songs), ctl[2] + ended.sum()]
    return ended.copy()


@pytest.mark.parametrize("slots", [7, 1500])
def test_stream_advance_kernel(cuda, slots):
    rng = np.random.default_rng(slots)
    A, R, bar_cond, bar0, cap = 6, 4, 5, 2, 9
    mask = np.zeros(18, dtype=np.int32)
    mask[[1, 9]] = 1
    n_songs = slots + slots // 2 + 1
    song = np.where(np.arange(slots) % 6 == 3, -1, np.arange(slots)).astype(np.int64)
    song[3] = -2                                            # a stray -2 is no candidate here: it stays, song-less
    pos = rng.integers(0, cap, slots).astype(np.int64)
    bar = rng.integers(bar0, bar_cond, slots).astype(np.int64)
    ctl = np.array([5, slots, 1], dtype=np.int64)
    ring = np.full((R, slots, A + 2), 7, dtype=np.int64)
    d = {k: torch.as_tensor(v).to(cuda) for k, v in dict(song=song, pos=pos, bar=bar, ctl=ctl, ring=ring).items()}
    d["fresh"] = torch.full((slots,), 5, dtype=torch.int64, device=cuda)
    ctl4 = torch.cat([d["ctl"], torch.zeros(1, dtype=torch.int64, device=cuda)])
    d["ctl"] = ctl4[:3]                                     # were ctl[3] = 0 read as songs ready, no slot took a song
    dmask = torch.as_tensor(mask).to(cuda)
    first = None
    for step in range(12):
        tokens = np.stack([rng.integers(0, n, slots) for n in N_CLASS], 1).astype(np.int64)
        if step == 0:                                       # several songs ending at once, by bar and by cap
            tokens[:, 2] = 0
            tokens[[0, 2, 4], 2] = [1, 9, 1]
            bar[[0, 2, 4]], pos[[0, 2, 4]] = bar_cond - 1, 0
            pos[[1, 3]] = 0
            pos[5 % slots] = cap - 1
            d["bar"].copy_(torch.as_tensor(bar))
            d["pos"].copy_(torch.as_tensor(pos))
        fresh = _advance_model(tokens, mask, bar_cond, bar0, cap, n_songs, song, pos, bar, ctl, ring)
        ops.stream_advance(torch.as_tensor(tokens).to(cuda), 2, dmask, bar_cond, bar0, cap, n_songs, d["song"],
                           d["pos"], d["bar"], d["fresh"], d["ctl"], d["ring"])
        for k, v in dict(song=song, pos=pos, bar=bar, ctl=ctl, ring=ring, fresh=fresh).items():
            assert (d[k].cpu().numpy() == v).all(), (step, k)
        if step == 0:
            first = song.copy()
            ended = np.nonzero(fresh)[0]
            assert len(ended) >= 4 and ended[:3].tolist() == [0, 2, 4]
            assert first[ended].tolist() == [slots + i if slots + i < n_songs else -1 for i in range(len(ended))]
    assert ctl[1] == n_songs                                # the pool ran out of songs: more idle slots
    assert (song == -1).sum() > (np.arange(slots) % 6 == 3).sum()
    assert ctl4.cpu().tolist() == ctl.tolist() + [0]        # three counters: the element after them is not written
    assert song[3] == -2 and (ring[:, 3, 0] == -2).all() and (ring[:, 3, -1] == 0).all()
    assert ring[:, :, -1].sum() > 0


def _slot_views(t, n, L, s_f, z_f):
    """Per layer the (n, s_f) S rows and (n, z_f) Z rows of a flat DecodeSession._state of n slots (views)."""
    per = s_f + z_f
    return [(t[i * n * per:i * n * per + n * s_f].view(n, s_f), t[i * n * per + n * s_f:(i + 1) * n * per].view(n, z_f))
            for i in range(L)]


# 7 slots: one wave.  300 slots, 544 float4 per slot: three blocks, fresh flags in every wave of the first 256-slot chunk
# (both edges of waves 0 / 1 and 2 / 3) and in the second chunk
REFILL_CASES = [(7, 3, 32, 8, [1, 3, 4]), (300, 2, 1024, 64, [0, 63, 64, 191, 255, 256, 299])]


def _refill_mismatch(state, want, logits, want_lg, slots, L, s_f, z_f):
    """The slots whose state in any layer, or logits row, is not exactly the expected one."""
    bad = (logits != want_lg).any(1)
    for (S, Z), (wS, wZ) in zip(_slot_views(state, slots, L, s_f, z_f), _slot_views(want, slots, L, s_f, z_f)):
        bad |= (S != wS).any(1) | (Z != wZ).any(1)
    return torch.nonzero(bad).flatten().tolist()


def test_stream_refill_kernel(cuda):
    g = torch.Generator(device=cuda).manual_seed(3)
    W = 19
    for slots, L, s_f, z_f, idx in REFILL_CASES:
        state = torch.randn(L * slots * (s_f + z_f), device=cuda, generator=g)
        snap = torch.randn(L * (s_f + z_f), device=cuda, generator=g)
        logits = torch.randn(slots, W + 5, device=cuda, generator=g)       # a row wider than n_logits
        snap_logits = torch.randn(W, device=cuda, generator=g)
        fresh = torch.zeros(slots, dtype=torch.int64, device=cuda)
        fresh[idx] = 1
        # every slot: the snapshot where fresh, untouched elsewhere, the columns past n_logits included
        want, want_lg = state.clone(), logits.clone()
        for (S, Z), (sS, sZ) in zip(_slot_views(want, slots, L, s_f, z_f), _slot_views(snap, 1, L, s_f, z_f)):
            S[idx], Z[idx] = sS[0], sZ[0]
        want_lg[idx, :W] = snap_logits
        assert _refill_mismatch(state, want, logits, want_lg, slots, L, s_f, z_f) == idx      # the check can fail
        ops.stream_refill(state, snap, L, s_f, z_f, logits, snap_logits, fresh)
        assert _refill_mismatch(state, want, logits, want_lg, slots, L, s_f, z_f) == [], slots


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_keyed_sampler_matches_slots(cuda, sampler):
    rows, W = 16, sum(N_CLASS)
    g = torch.Generator(device=cuda).manual_seed(4)
    L = torch.randn(rows, W, device=cuda, generator=g) * 2
    temp, top_p = (generation.DQN_TEMPERATURE, generation.DQN_TOP_P) if sampler == "dqn" else (None, None)
    rng = np.random.default_rng(0)
    key = rng.permutation(rows)
    step = rng.choice([0, 3, 7, 1000], rows)
    want = np.zeros((rows, len(N_CLASS)), dtype=np.int64)
    for c in np.unique(step):
        tok = torch.zeros(rows, len(N_CLASS), dtype=torch.int64, device=cuda)
        ops.sample_categorical(L, N_CLASS, tok, 123, counter=torch.tensor([int(c)], device=cuda), temperature=temp,
                               top_p=top_p, slot_keys=True)
        sel = step == c
        want[sel] = tok.cpu().numpy()[key[sel]]
    got = torch.zeros(rows, len(N_CLASS), dtype=torch.int64, device=cuda)
    ops.sample_categorical_keyed(L[torch.as_tensor(key, device=cuda)].contiguous(), N_CLASS, got, 123,
                                 torch.as_tensor(key, device=cuda), torch.as_tensor(step, device=cuda),
                                 temperature=temp, top_p=top_p)
    assert (got.cpu().numpy() == want).all()


def test_stream_refusals(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    with pytest.raises(ValueError, match="ragged"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, prompt=[FIX["tokens"][:3], FIX["tokens"][:4]])
    with pytest.raises(ValueError, match="2\\*\\*20"):
        generation.generate_stream(net, w2e, (1 << 20) + 1, bar_cond=3)
    with pytest.raises(ValueError, match="slots"):
        generation.generate_stream(net, w2e, 2, slots=0, bar_cond=3)
    with pytest.raises(ValueError, match="sampler"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, sampler="greedy")
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        generation.generate_stream(net, w2e, 2, bar_cond=3)
    net.eval()
    bf = _small_model(cuda, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="f32"):
        generation.generate_stream(bf, w2e, 2, bar_cond=3)
    with pytest.raises(ValueError, match="not both"):
        generation.generate(net, w2e, n_songs=2, bar_cond=3, batch_size=2, slots=2, log=lambda *a: None,
                            stats_path=None)


def test_generate_with_slots(cuda, tmp_path):
    net = _small_model(cuda)
    w2e = _word2event()
    stats = generation.generate(net, w2e, n_songs=5, bar_cond=3, path_gendir=str(tmp_path / "gen"), max_tokens=200,
                                stats_path=str(tmp_path / "runtime_stats.json"), log=lambda *a: None, slots=2)
    saved = json.load(open(tmp_path / "runtime_stats.json"))
    assert set(saved) == {"song_time", "words_len_list", "ave token time:", "ave song time"}
    assert len(stats["song_time"]) == 5 and len(set(stats["song_time"])) == 1       # the stream's wall time / n_songs
    for i in range(5):
        s = np.load(tmp_path / "gen" / ("get_%d.npy" % i))
        assert s.shape == (stats["words_len_list"][i], 6)
    assert not os.path.exists(tmp_path / "gen" / "get_5.npy")

"""GPU: per-song prompts on the stream -- the batch-invariant prefill (kernel="gemm"), the bank kernels
(cwlt_stream_refill_bank, cwlt_stream_advance_bank in csrc/stream.hip) against numpy models, and
generate_stream(prompts=...) against generate_batch(prompts=..., prefill="gemm")."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402
from test_generate_stream_gpu import _refill_mismatch, _slot_views  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]


def _small_model(cuda):
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": 2, "N_HEAD": 2})
    try:
        net = model.LinearTransformer(N_CLASS, is_training=False)
    finally:
        config.AgentConfig.update(old)
    return fill_params(net, seed=int(FIX["fill_seed"])).to(cuda).eval()


def _word2event(n_class=N_CLASS):
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, n_class)}
    w2e["bar-beat"][1] = "Bar"
    if n_class[2] > 9:
        w2e["bar-beat"][9] = "Bar"
    return w2e


def _prompts(lengths, seed, n_class=N_CLASS, max_bars=2):
    """Random prompts of the given lengths whose bar count (1 + Bars after the first row) stays <= max_bars."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        p = np.stack([rng.integers(0, c, n) for c in n_class], 1).astype(np.int64)
        p[:, 2] = np.where(p[:, 2] == 9, 0, p[:, 2])
        bars = np.nonzero(p[1:, 2] == 1)[0] + 1
        p[bars[max_bars - 1:], 2] = 0
        out.append(p)
    return out


def _bars(w2e, rows):
    return np.array([w2e["bar-beat"][int(r[2])] == "Bar" for r in rows])


def _check_cut(w2e, song, prompt_len, bar_cond, max_tokens):
    cnt = 1 + np.cumsum(_bars(w2e, song[1:]))
    reached = np.nonzero(cnt >= bar_cond)[0]
    if len(song) == max_tokens and (len(reached) == 0 or reached[0] == len(song) - 2):
        return
    assert len(reached) and reached[0] == len(song) - 2, (len(song), prompt_len)
    assert len(song) > prompt_len


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def _prefill_alone(net, p, kernel="gemm"):
    sess = generation.DecodeSession(net, n_songs=1, kernel="gemm", graph=False)
    sess.reset()
    logits = sess._prefill(p, kernel=kernel).clone()
    return sess._state.clone(), logits[0]


def _song_state(sess, k):
    """Song k's [S, Z] of every layer, flattened."""
    return torch.cat([torch.cat([S[k].reshape(-1), Z[k].reshape(-1)]) for S, Z in sess.memory])


def _ragged(net, prompts, pad=0, prefill_rows=None):
    n = len(prompts)
    P = max(len(p) for p in prompts) + pad
    toks = np.zeros((n, P, 6), dtype=np.int64)
    for i, p in enumerate(prompts):
        toks[i, :len(p)] = p
    sess = generation.DecodeSession(net, n_songs=n, kernel="gemm", graph=False)
    sess.reset()
    logits = sess._prefill(toks, [len(p) for p in prompts], kernel="gemm", prefill_rows=prefill_rows).clone()
    return sess, logits


def _scaled_err(a, b):
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def test_invariant_prefill(cuda):
    net = _small_model(cuda)
    prompts = _prompts([37, 5, 70, 1, 33, 64], seed=1)
    alone = [_prefill_alone(net, p) for p in prompts]
    others = _prompts([90, 2, 45], seed=2)
    layouts = [(list(range(6)), [], 0, None), (list(range(6))[::-1], others, 7, None),
               ([2, 0, 4], others[:1], 0, 1), ([5, 1, 3], others, 33, 100)]
    for order, extra, pad, rows in layouts:
        batch = [prompts[i] for i in order] + extra
        sess, logits = _ragged(net, batch, pad=pad, prefill_rows=rows)
        for j, k in enumerate(order):
            st, lg = alone[k]
            assert torch.equal(_song_state(sess, j), st), (order, k)
            assert torch.equal(logits[j], lg), (order, k)
    # GEMM row slicing inside one call changes no bits
    toks = np.zeros((3, 70, 6), dtype=np.int64)
    for i, k in enumerate([0, 2, 4]):
        toks[i, :len(prompts[k])] = prompts[k]
    outs = []
    for rows in (4096, 37, 1):
        sess = generation.DecodeSession(net, n_songs=3, kernel="gemm", graph=False)
        sess.reset()
        h, lg = net.prefill_hidden(torch.as_tensor(toks).to(cuda), sess.memory, [37, 70, 33], kernel="gemm",
                                   logits=True, rows=rows)
        outs.append((sess._state.clone(), h.clone(), lg.clone()))
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(o, outs[0]))
    # against the blas prefill and against step() one token at a time: f32 rounding
    for k in (0, 2, 3):
        st, lg = alone[k]
        st_b, lg_b = _prefill_alone(net, prompts[k], kernel="blas")
        assert float((lg - lg_b).abs().max()) < 1e-5 and _scaled_err(st, st_b) < 1e-5, k
        sess = generation.DecodeSession(net, n_songs=1, kernel="gemm", graph=False)
        sess.reset()
        for row in prompts[k]:
            out = sess.step(row)
        assert float(np.abs(out - lg.cpu().numpy()).max()) < 1e-5 and _scaled_err(st, sess._state) < 1e-5, k


# (slots, layers, s_floats, z_floats, {fresh slot: its song}); songs >= 5 wrap the bank, fresh slots with -1 / -2 stay.
# 9 slots: one wave.  300 slots, 544 float4 per slot: three blocks, fresh flags in every wave of the first 256-slot
# chunk (both edges of waves 0 / 1 and 2 / 3) and in the second chunk
REFILL_BANK_CASES = [(9, 3, 32, 8, {1: 7, 3: 11, 4: 4, 6: -1, 7: -2, 8: 5}),
                     (300, 2, 1024, 64, {0: 3, 63: -1, 64: 7, 191: 11, 255: -2, 256: 4, 299: 10})]


def test_refill_bank_kernel(cuda):
    g = torch.Generator(device=cuda).manual_seed(3)
    bank, W = 5, 19
    for slots, L, s_f, z_f, songs in REFILL_BANK_CASES:
        state = torch.randn(L * slots * (s_f + z_f), device=cuda, generator=g)
        bstate = torch.randn(L * bank * (s_f + z_f), device=cuda, generator=g)
        logits = torch.randn(slots, W + 5, device=cuda, generator=g)       # a row wider than n_logits
        blogits = torch.randn(bank, W, device=cuda, generator=g)
        fresh = torch.zeros(slots, dtype=torch.int64, device=cuda)
        fresh[list(songs)] = 1
        song = torch.arange(slots, dtype=torch.int64, device=cuda) % 13 - 2    # not fresh: any song, negative too
        song[list(songs)] = torch.tensor(list(songs.values()), device=cuda)
        idx = [s for s, k in songs.items() if k >= 0]
        e = [songs[s] % bank for s in idx]
        # every slot: its song's entry where fresh with a song, untouched elsewhere, the columns past n_logits included
        want, want_lg = state.clone(), logits.clone()
        for (S, Z), (bS, bZ) in zip(_slot_views(want, slots, L, s_f, z_f), _slot_views(bstate, bank, L, s_f, z_f)):
            S[idx], Z[idx] = bS[e], bZ[e]
        want_lg[idx, :W] = blogits[e]
        assert _refill_mismatch(state, want, logits, want_lg, slots, L, s_f, z_f) == idx      # the check can fail
        ops.stream_refill_bank(state, bstate, L, s_f, z_f, logits, blogits, fresh, song)
        assert _refill_mismatch(state, want, logits, want_lg, slots, L, s_f, z_f) == [], slots


def _advance_bank_model(tokens, mask, bar_cond, bank_bar0, bank_cap, n_songs, song, pos, bar, cap, ctl, ring):
    """numpy model of cwlt_stream_advance_bank (bar attribute 2); updates its arguments, returns the fresh flags."""
    S, A = tokens.shape
    row = ctl[0] % ring.shape[0]
    ended = np.zeros(S, dtype=np.int64)
    cand = np.zeros(S, dtype=bool)
    for s in range(S):
        if song[s] >= 0:
            bar[s] += int(mask[tokens[s, 2]])
            ended[s] = int(bar[s] >= bar_cond or pos[s] + 1 >= cap[s])
            pos[s] += 1
        cand[s] = ended[s] or song[s] == -2
    ring[row, :, 0] = np.where(song >= 0, song, -1)
    ring[row, :, 1:1 + A] = tokens
    ring[row, :, -1] = ended
    limit = min(ctl[3], n_songs)
    nxt = ctl[1]
    fresh = np.zeros(S, dtype=np.int64)
    for s in np.nonzero(cand)[0]:
        if nxt < limit:
            e = nxt % len(bank_bar0)
            song[s], pos[s], bar[s], cap[s], fresh[s] = nxt, 0, bank_bar0[e], bank_cap[e], 1
        else:
            song[s] = -2 if nxt < n_songs else -1
        nxt += 1
    ctl[:3] = [ctl[0] + 1, ctl[1] + min(int(cand.sum()), max(0, limit - ctl[1])), ctl[2] + ended.sum()]
    return fresh


@pytest.mark.parametrize("slots", [7, 1500])
def test_stream_advance_bank_kernel(cuda, slots):
    rng = np.random.default_rng(slots)
    A, R, bar_cond, bank = 6, 4, 5, 5
    mask = np.zeros(18, dtype=np.int32)
    mask[[1, 9]] = 1
    n_songs = slots + slots // 2 + 3
    bank_bar0 = rng.integers(1, bar_cond, bank).astype(np.int64)
    bank_cap = rng.integers(2, 9, bank).astype(np.int64)
    song = np.arange(slots, dtype=np.int64)
    song[np.arange(slots) % 6 == 3] = -1                   # idle from the start
    song[-2:] = -2                                         # waiting for a song
    pos = rng.integers(0, 2, slots).astype(np.int64)
    bar = rng.integers(1, bar_cond, slots).astype(np.int64)
    cap = rng.integers(3, 9, slots).astype(np.int64)
    ready = slots - 2
    ctl = np.array([5, slots - 2, 1, ready], dtype=np.int64)
    ring = np.full((R, slots, A + 2), 7, dtype=np.int64)
    d = {k: torch.as_tensor(v).to(cuda) for k, v in dict(song=song, pos=pos, bar=bar, cap=cap, ctl=ctl,
                                                          ring=ring).items()}
    d["fresh"] = torch.full((slots,), 5, dtype=torch.int64, device=cuda)
    dmask = torch.as_tensor(mask).to(cuda)
    db0, dcap = torch.as_tensor(bank_bar0).to(cuda), torch.as_tensor(bank_cap).to(cuda)
    for step in range(20):
        if step == 3:                                      # three more songs ready: the waiting slots, in slot order
            ctl[3] += 3
            d["ctl"][3] = int(ctl[3])
        if step == 8:
            ctl[3] = n_songs + 4                           # ready past n_songs: the limit is n_songs
            d["ctl"][3] = int(ctl[3])
        tokens = np.stack([rng.integers(0, n, slots) for n in N_CLASS], 1).astype(np.int64)
        if step == 0:                                      # songs ending by bar and by cap while the gate is shut
            tokens[:, 2] = 0
            tokens[[0, 2], 2] = [1, 9]
            bar[[0, 2]] = bar_cond - 1
            pos[1] = cap[1] - 1
            d["bar"].copy_(torch.as_tensor(bar))
            d["pos"].copy_(torch.as_tensor(pos))
        before = song.copy()
        fresh = _advance_bank_model(tokens, mask, bar_cond, bank_bar0, bank_cap, n_songs, song, pos, bar, cap, ctl,
                                    ring)
        ops.stream_advance_bank(torch.as_tensor(tokens).to(cuda), 2, dmask, bar_cond, db0, dcap, n_songs, d["song"],
                                d["pos"], d["bar"], d["cap"], d["fresh"], d["ctl"], d["ring"])
        for k, v in dict(song=song, pos=pos, bar=bar, cap=cap, ctl=ctl, ring=ring, fresh=fresh).items():
            assert (d[k].cpu().numpy() == v).all(), (step, k)
        if step == 0:
            assert fresh.sum() == 0 and ctl[1] == slots - 2                 # gate shut: nobody takes a song
            assert song[0] == -2 and song[1] == -2 and song[2] == -2 and (song[-2:] == -2).all()
            assert ctl[2] == 1 + 3                                          # the three ended songs are finished
        if step == 3:                                      # candidates: slots waiting before, slots ending now
            ended_now = ring[(ctl[0] - 1) % R, :, -1] == 1
            cands = np.nonzero((before == -2) | ended_now)[0]
            took = np.nonzero(fresh)[0]
            assert len(cands) > 3 and took.tolist() == cands[:3].tolist()
            assert song[took].tolist() == [slots - 2, slots - 1, slots]     # the next indices, in slot order
            assert (song[cands[3:]] == -2).all()
            assert (bar[took] == bank_bar0[song[took] % bank]).all() and (cap[took] == bank_cap[song[took] % bank]).all()
    assert ctl[1] == n_songs and (song == -2).sum() == 0
    assert (ring[:, :, 0] == -1).all()                      # every slot idle once all songs ended
    assert ctl[2] == n_songs + 1 - (np.arange(slots) % 6 == 3).sum()     # finished: all but the idle slots' indices


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_stream_prompts_equal_batch(cuda, sampler):
    net = _small_model(cuda)
    w2e = _word2event()
    lengths = [12, 1, 40, 7, 25, 3, 33, 18, 2, 9, 30, 14]
    prompts = _prompts(lengths, seed=4)
    max_tokens = 40 + 70
    torch.manual_seed(12)
    ref = generation.generate_batch(net, w2e, 12, bar_cond=4, max_tokens=max_tokens, prompts=prompts, sampler=sampler,
                                    chunk=32, prefill="gemm")
    assert any(len(s) < max_tokens for s in ref)
    runs = [dict(slots=s) for s in (1, 3, 16, 40)]
    runs += [dict(slots=3, prefill_rows=40, bank=2), dict(slots=5, prefill_rows=80, bank=4),
             dict(slots=16, prefill_rows=4096, bank=None)]
    for kw in runs:
        torch.manual_seed(12)
        got = generation.generate_stream(net, w2e, 12, bar_cond=4, max_tokens=max_tokens, prompts=prompts,
                                         sampler=sampler, chunk=16, **kw)
        assert _same(got, ref), kw
    for s, p in zip(got, prompts):
        assert s[:len(p)].tolist() == p.tolist()
        _check_cut(w2e, s, len(p), 4, max_tokens)


def test_stream_prompts_gate_pressure(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    lengths = [20, 21, 22] * 6
    prompts = _prompts(lengths, seed=5)
    max_tokens = 23                                        # one to three drawn rows per song
    torch.manual_seed(3)
    ref = generation.generate_batch(net, w2e, 18, bar_cond=6, max_tokens=max_tokens, prompts=prompts, chunk=8,
                                    prefill="gemm")
    torch.manual_seed(3)
    got, st = generation._generate_stream(net, w2e, 18, slots=8, bar_cond=6, max_tokens=max_tokens, prompts=prompts,
                                          chunk=4, prefill_rows=22, bank=2)
    assert (st["block"], st["bank"], st["prefill_blocks"]) == (1, 2, 18)
    assert st["gated_chunks"] > 0                          # slots outran the prefill
    assert _same(got, ref)
    for s, p in zip(got, prompts):
        assert s[:len(p)].tolist() == p.tolist() and 1 <= len(s) - len(p) <= 3
    assert st["drawn"] == sum(len(s) - len(p) for s, p in zip(got, prompts))


def test_stream_prompts_graph_equals_eager(cuda, monkeypatch):
    net = _small_model(cuda)
    w2e = _word2event()
    prompts = _prompts([5, 17, 2, 30, 9, 11, 4], seed=6)
    torch.manual_seed(5)
    graphed, st = generation._generate_stream(net, w2e, 7, slots=3, bar_cond=4, max_tokens=90, chunk=8,
                                              prompts=prompts, prefill_rows=34, bank=2)
    assert st["graph"]
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    torch.manual_seed(5)
    eager, st = generation._generate_stream(net, w2e, 7, slots=3, bar_cond=4, max_tokens=90, chunk=8,
                                            prompts=prompts, prefill_rows=34, bank=2)
    assert not st["graph"]
    assert _same(graphed, eager)


def test_stream_prompts_refusals(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    ps = _prompts([3, 4], seed=7)
    with pytest.raises(ValueError, match="ragged.*prompts="):
        generation.generate_stream(net, w2e, 2, bar_cond=3, prompt=ps)
    with pytest.raises(ValueError, match="not both"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, prompt=ps[0], prompts=ps)
    with pytest.raises(ValueError, match="2 arrays for 3 songs"):
        generation.generate_stream(net, w2e, 3, bar_cond=3, prompts=ps)
    with pytest.raises(ValueError, match="empty"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, prompts=[ps[0], ps[1][:0]])
    barry = ps[1].copy()
    barry[1:3, 2] = 1
    with pytest.raises(ValueError, match="already reaches"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, prompts=[ps[0], barry])
    with pytest.raises(ValueError, match="no room"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, max_tokens=4, prompts=ps)
    bad = ps[0].copy()
    bad[1, 3] = N_CLASS[3]
    with pytest.raises(ValueError, match="out of range"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, prompts=[bad, ps[1]])
    with pytest.raises(ValueError, match="multiple"):
        generation.generate_stream(net, w2e, 2, bar_cond=3, prompts=ps, prefill_rows=8, bank=3)
    with pytest.raises(ValueError, match="prefill"):
        generation.generate_batch(net, w2e, 2, bar_cond=3, prompts=ps, prefill="fast")
    with pytest.raises(ValueError, match="not both"):
        generation.generate(net, w2e, n_songs=2, bar_cond=3, prompt=ps[0], prompts=ps, log=lambda *a: None,
                            stats_path=None)


@pytest.mark.parametrize("mode", ["slots", "batch_size"])
def test_generate_with_prompts(cuda, tmp_path, mode):
    net = _small_model(cuda)
    w2e = _word2event()
    prompts = _prompts([4, 9, 2, 6, 3], seed=8)
    stats = generation.generate(net, w2e, n_songs=5, bar_cond=4, path_gendir=str(tmp_path / "gen"), max_tokens=60,
                                stats_path=str(tmp_path / "runtime_stats.json"), log=lambda *a: None, prompts=prompts,
                                **{mode: 2})
    saved = json.load(open(tmp_path / "runtime_stats.json"))
    assert set(saved) == {"song_time", "words_len_list", "ave token time:", "ave song time"}
    assert len(stats["song_time"]) == 5
    for i in range(5):
        s = np.load(tmp_path / "gen" / ("get_%d.npy" % i))
        assert s.shape == (stats["words_len_list"][i], 6)
        assert s[:len(prompts[i])].tolist() == prompts[i].tolist()
        _check_cut(w2e, s, len(prompts[i]), 4, 60)
    assert not os.path.exists(tmp_path / "gen" / "get_5.npy")


def test_stream_prompts_repo_dims(cuda):
    from rlmg_amd.dqn_policy import model
    n_class = [56, 135, 18, 87, 18, 25]
    net = fill_params(model.LinearTransformer(n_class, is_training=False), seed=5).to(cuda).eval()
    w2e = _word2event(n_class)
    rng = np.random.default_rng(9)
    lengths = [1, 700] + rng.integers(1, 701, 62).tolist()
    prompts = _prompts(lengths, seed=10, n_class=n_class, max_bars=3)
    torch.manual_seed(7)
    ref = generation.generate_batch(net, w2e, 64, bar_cond=5, max_tokens=760, prompts=prompts, prefill="gemm")
    torch.manual_seed(7)
    got = generation.generate_stream(net, w2e, 64, slots=24, bar_cond=5, max_tokens=760, prompts=prompts, chunk=64)
    assert _same(got, ref)
    for s, p in zip(got, prompts):
        assert s[:len(p)].tolist() == p.tolist()

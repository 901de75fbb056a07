"""GPU: many songs at once -- generation.generate_batch (one GEMM-step session, one N-song device loop) and
generate(batch_size=...)."""
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
from rlmg_amd import generation  # noqa: E402

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


def test_generate_batch_from_scratch(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    torch.manual_seed(3)
    a = generation.generate_batch(net, w2e, 24, bar_cond=4, max_tokens=300, chunk=32)
    torch.manual_seed(3)
    b = generation.generate_batch(net, w2e, 24, bar_cond=4, max_tokens=300, chunk=32)
    assert len(a) == 24 and all(x.tolist() == y.tolist() for x, y in zip(a, b))       # same seed, same songs
    torch.manual_seed(3)
    small = generation.generate_batch(net, w2e, 8, bar_cond=4, max_tokens=300, chunk=16)
    for i in range(8):                                                                 # batch invariant, bit for bit
        assert small[i].tolist() == a[i].tolist(), i
    for s in a:
        assert s.dtype == np.int64 and s.shape[1] == 6
        assert s[0].tolist() == generation.INIT_CW[0].tolist()
        assert all((s[:, i] >= 0).all() and (s[:, i] < n).all() for i, n in enumerate(N_CLASS))
        _check_cut(w2e, s, 1, 4, 300)
    assert len({len(s) for s in a}) > 1                                                # songs end independently
    # a cap shorter than most songs: exactly max_tokens rows unless the bar rule cut first
    capped = generation.generate_batch(net, w2e, 8, bar_cond=10 ** 6, max_tokens=40, chunk=16)
    assert [len(s) for s in capped] == [40] * 8


def test_generate_batch_prompts_and_samplers(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    bars = np.cumsum(_bars(w2e, FIX["tokens"][1:]))
    p_len = int(np.argmax(bars >= 1)) + 1                   # a prompt with one Bar after its first row: count 2
    prompts = [FIX["tokens"][:p_len], FIX["tokens"][:3], FIX["tokens"][:1], FIX["tokens"][:p_len + 2]]
    torch.manual_seed(4)
    songs = generation.generate_batch(net, w2e, 4, bar_cond=5, max_tokens=200, prompts=prompts, chunk=32)
    for s, p in zip(songs, prompts):
        assert s[:len(p)].tolist() == p.tolist()
        _check_cut(w2e, s, len(p), 5, 200)
    # one prompt for every song
    one = generation.generate_batch(net, w2e, 3, bar_cond=5, max_tokens=64, prompts=FIX["tokens"][:4], chunk=16)
    assert all(s[:4].tolist() == FIX["tokens"][:4].tolist() for s in one)
    # ragged caps: max_tokens counts the prompt
    long = generation.generate_batch(net, w2e, 2, bar_cond=10 ** 6, max_tokens=30,
                                     prompts=[FIX["tokens"][:5], FIX["tokens"][:12]], chunk=8)
    assert [len(s) for s in long] == [30, 30]
    for sampler in ("dqn", "categorical"):
        out = generation.generate_batch(net, w2e, 5, bar_cond=10 ** 6, max_tokens=50, sampler=sampler, chunk=16)
        for s in out:
            assert len(s) == 50 and all((s[:, i] >= 0).all() and (s[:, i] < n).all() for i, n in enumerate(N_CLASS))


def test_generate_batch_refusals(cuda):
    net = _small_model(cuda)
    w2e = _word2event()
    bars = np.cumsum(_bars(w2e, FIX["tokens"][1:]))
    reach = int(np.argmax(bars >= 2)) + 2                   # prompt whose rows after the first hold two Bars: count 3
    with pytest.raises(ValueError, match="already reaches"):
        generation.generate_batch(net, w2e, 2, bar_cond=3, prompts=FIX["tokens"][:reach])
    with pytest.raises(ValueError, match="leaves no room"):
        generation.generate_batch(net, w2e, 2, bar_cond=50, max_tokens=8,
                                  prompts=[FIX["tokens"][:3], FIX["tokens"][:8]])
    net.train()
    with pytest.raises(RuntimeError, match="eval"):
        generation.generate_batch(net, w2e, 2, bar_cond=3)
    net.eval()
    bf = _small_model(cuda, dtype=torch.bfloat16)
    assert bf.compute_dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="f32"):
        generation.generate_batch(bf, w2e, 2, bar_cond=3)


def test_generate_with_batch_size(cuda, tmp_path):
    net = _small_model(cuda)
    w2e = _word2event()
    stats = generation.generate(net, w2e, n_songs=5, bar_cond=3, path_gendir=str(tmp_path / "gen"), max_tokens=200,
                                stats_path=str(tmp_path / "runtime_stats.json"), log=lambda *a: None, batch_size=2)
    saved = json.load(open(tmp_path / "runtime_stats.json"))
    assert set(saved) == {"song_time", "words_len_list", "ave token time:", "ave song time"}
    assert len(stats["song_time"]) == 5 and len(stats["words_len_list"]) == 5
    assert stats["song_time"][0] == stats["song_time"][1]            # a group's wall time shared by its songs
    for i in range(5):
        s = np.load(tmp_path / "gen" / ("get_%d.npy" % i))
        assert s.shape == (stats["words_len_list"][i], 6)
    assert not os.path.exists(tmp_path / "gen" / "get_5.npy")


def test_generate_batch_repo_dims_256(cuda):
    from rlmg_amd.dqn_policy import model
    n_class = [56, 135, 18, 87, 18, 25]
    net = fill_params(model.LinearTransformer(n_class, is_training=False), seed=5).to(cuda).eval()
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, n_class)}
    w2e["bar-beat"][1] = "Bar"
    sess = generation.DecodeSession(net, n_songs=256, kernel="gemm")
    toks = np.tile(generation.INIT_CW, (256, 1))
    for _ in range(3):
        out = sess.step(toks)
        assert out.shape == (256, sum(n_class)) and np.isfinite(out).all()
    assert tuple(sess.hidden.shape) == (256, 512) and torch.isfinite(sess.hidden).all()
    torch.manual_seed(1)
    songs = generation.generate_batch(net, w2e, 256, bar_cond=17, max_tokens=64, chunk=32)
    assert len(songs) == 256 and all(s.ndim == 2 and s.shape[1] == 6 and 1 < len(s) <= 64 for s in songs)

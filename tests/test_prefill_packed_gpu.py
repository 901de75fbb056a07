"""GPU: the packed prefill -- ragged songs laid end to end, no padded rows, and every song's state,
hidden row, logits, scores and stats BIT FOR BIT those of the batch-invariant prefill (kernel="gemm").

1. cwlt_causal_linear_fwd_state_packed against ops.cla_fwd_state on each song alone (torch.equal), one case against the
   f64 token-by-token oracle.
2. cwlt_prefer_scan_packed against cwlt_prefer_scan on the padded block and against Preference.seen_states.
3. CWTrunk.prefill_hidden_packed against prefill_hidden(kernel="gemm", lengths=...).
4. DecodeSession.prefill(kernel="packed"), steps and a captured graph after it.
5. score_songs / policy_stats(kernel="packed") against kernel="gemm".
6. generate_batch / generate_particles(prefill="packed") against "gemm".
7. The bank streams with packed_prefill=True against packed_prefill=False.
Small fixture model (128 / 2 layers / 2 heads) throughout."""
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
from oracle.cla import cla_recurrent_step  # noqa: E402
from test_blend_gpu import FIX, N_CLASS, _bits, _same, _small_model, _word2event  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
A = len(N_CLASS)


def _eq(a, b):
    """Bit for bit, NaN and -inf included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _cu(lens):
    return [0] + [int(x) for x in np.cumsum(lens)]


def _random_songs(rng, lens):
    return [np.stack([rng.integers(0, n, L) for n in N_CLASS], 1).astype(np.int64) for L in lens]


@pytest.fixture(scope="module")
def world(cuda):
    seed = int(FIX["fill_seed"])
    return {"net": _small_model(cuda, seed), "ref": _small_model(cuda, seed + 1), "w2e": _word2event()}


# ---- 1. the scan ----------------------------------------------------------------------------------------------------------
SCAN_LENS = [1, 31, 32, 33, 64, 65, 200]


def _scan_inputs(cuda, H, lens, seed):
    g = torch.Generator().manual_seed(seed)
    D, R, n = H * 64, sum(lens), len(lens)
    qkv = (0.5 * torch.randn(R, 3 * D, generator=g)).to(cuda)            # the projection's own buffer: row stride 3 D
    q, k, v = (qkv[:, i * D:(i + 1) * D].view(R, H, 64) for i in range(3))
    S0 = (0.5 * torch.randn(n, H, 64, 64, generator=g)).to(cuda)         # a non-zero starting state per song
    Z0 = (0.5 + 4 * torch.rand(n, H, 64, generator=g)).to(cuda)          # key sums are sums of phi > 0
    return q, k, v, S0, Z0


@pytest.mark.parametrize("H", [2, 8])
def test_scan_is_the_rectangular_scan_of_each_song(cuda, H):
    lens = SCAN_LENS
    cu, R = _cu(lens), sum(lens)
    assert any(a % 32 for a in cu[1:-1]) and any(a % 4 for a in cu[1:-1])
    q, k, v, S0, Z0 = _scan_inputs(cuda, H, lens, 7 + H)
    big = torch.full((R + 9, H, 64), SENTINEL, device=cuda)
    S, Z = S0.clone(), Z0.clone()
    out = ops.cla_fwd_state_packed(q, k, v, S, Z, cu, out=big[:R])
    assert out.data_ptr() == big.data_ptr()
    assert (big[R:] == SENTINEL).all() and not (big[:R] == SENTINEL).any()
    for s, (a, z) in enumerate(zip(cu, cu[1:])):
        S1, Z1 = S0[s:s + 1].clone(), Z0[s:s + 1].clone()
        want = ops.cla_fwd_state(q[a:z][None], k[a:z][None], v[a:z][None], S1, Z1, segments=1)
        assert torch.equal(out[a:z], want[0]), (H, s)
        assert torch.equal(S[s], S1[0]) and torch.equal(Z[s], Z1[0]), (H, s)
        assert not torch.equal(S[s], S0[s])
    # SeqOffsets in place of the list, a fresh output, a strided out view
    S2, Z2 = S0.clone(), Z0.clone()
    got = ops.cla_fwd_state_packed(q, k, v, S2, Z2, ops.SeqOffsets(cu, device=cuda))
    assert torch.equal(got, out) and torch.equal(S2, S) and torch.equal(Z2, Z)
    wide = torch.full((R, H * 64 + 4), SENTINEL, device=cuda)
    S2, Z2 = S0.clone(), Z0.clone()
    ops.cla_fwd_state_packed(q, k, v, S2, Z2, cu, out=wide[:, :H * 64].view(R, H, 64))
    assert torch.equal(wide[:, :H * 64].reshape(R, H, 64), out) and (wide[:, H * 64:] == SENTINEL).all()


def test_scan_single_song_of_one_row(cuda):
    q, k, v, S0, Z0 = _scan_inputs(cuda, 2, [1], 3)
    S, Z, S1, Z1 = S0.clone(), Z0.clone(), S0.clone(), Z0.clone()
    big = torch.full((3, 2, 64), SENTINEL, device=cuda)
    out = ops.cla_fwd_state_packed(q, k, v, S, Z, [0, 1], out=big[:1])
    want = ops.cla_fwd_state(q[None], k[None], v[None], S1, Z1, segments=1)
    assert torch.equal(out, want[0]) and torch.equal(S, S1) and torch.equal(Z, Z1)
    assert (big[1:] == SENTINEL).all()


def test_scan_matches_oracle(cuda):
    """The tolerance of tests/test_prefill_gpu.py::test_scan_with_state_matches_oracle: 1e-4 of a row's scale for the
    outputs, 1e-5 of the largest entry for the state."""
    H, lens = 2, SCAN_LENS
    cu = _cu(lens)
    q, k, v, S0, Z0 = _scan_inputs(cuda, H, lens, 11)
    S, Z = S0.clone(), Z0.clone()
    out = ops.cla_fwd_state_packed(q, k, v, S, Z, cu).cpu()
    S, Z = S.cpu(), Z.cpu()
    qc, kc, vc = (t.double().cpu() for t in (q, k, v))
    for s, (a, z) in enumerate(zip(cu, cu[1:])):
        st = [S0[s].double().cpu()[None], Z0[s].double().cpu()[None]]
        rows = []
        for t in range(a, z):
            o, st = cla_recurrent_step(qc[t][None], kc[t][None], vc[t][None], st)
            rows.append(o[0])
        ref = torch.stack(rows)
        scale = ref.abs().amax(dim=(1, 2)).clamp_min(1.0)
        err = (out[a:z].double() - ref).abs().amax(dim=(1, 2)) / scale
        assert err.max().item() < 1e-4, (s, err.max().item())
        assert (S[s].double() - st[0][0]).abs().max().item() <= 1e-5 * st[0][0].abs().max().item(), s
        assert (Z[s].double() - st[1][0]).abs().max().item() <= 1e-5 * st[1][0].abs().max().item(), s


def test_scan_wrapper_refusals(cuda):
    q = torch.randn(10, 2, 64, device=cuda)
    S, Z = torch.zeros(2, 2, 64, 64, device=cuda), torch.zeros(2, 2, 64, device=cuda)
    with pytest.raises(RuntimeError, match="status 1002"):
        b = q.bfloat16()
        ops.cla_fwd_state_packed(b, b, b, S, Z, [0, 3, 10])
    with pytest.raises(ValueError, match="ends at row"):
        ops.cla_fwd_state_packed(q, q, q, S, Z, [0, 3, 9])
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.cla_fwd_state_packed(q, q, q, S, Z, [0, 10, 10])
    with pytest.raises(ValueError, match="state shapes"):
        ops.cla_fwd_state_packed(q, q, q, S[:1], Z[:1], [0, 3, 10])
    with pytest.raises(ValueError, match="out must be"):
        ops.cla_fwd_state_packed(q, q, q, S, Z, [0, 3, 10], out=torch.zeros(9, 2, 64, device=cuda))


# ---- 2. the repetition scan -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [True, False])
def test_prefer_scan_packed(cuda, keyed):
    lens = [1, 2, 33, 7]
    cu, n, Lb, W = _cu(lens), 4, 33, sum(N_CLASS)
    w2e = _word2event()
    rng = np.random.default_rng(5)
    songs = _random_songs(rng, lens)
    for x in songs:
        x[:, 3] = rng.integers(0, 3, len(x))                             # few pitch classes: states above 1
    prefs = [Preference(w2e, repeat={"pitch": 1.0}, decay=d) for d in (1.0, 0.5, 0.9, 0.25)]
    pen = np.stack([p.penalties() for p in prefs] + [np.zeros(2 * A + 1, np.float32)])
    order = [2, 0, 3, 1] if keyed else [0, 1, 2, 3]                      # song i of the block is song order[i] of pen
    pen_d = torch.as_tensor(pen).to(cuda)
    packed = torch.as_tensor(np.concatenate(songs)).to(cuda)
    key = torch.as_tensor(np.repeat(order, lens)).to(cuda) if keyed else None
    big = torch.full((cu[-1] + 3, W + 2), SENTINEL, dtype=torch.float32, device=cuda)
    got = ops.prefer_scan_packed(packed, cu, N_CLASS, pen_d, key=key, out=big[:cu[-1]])
    assert got.data_ptr() == big.data_ptr() and (big[cu[-1]:] == SENTINEL).all() and (big[:, W:] == SENTINEL).all()
    got = got[:, :W].cpu().numpy()
    fresh = ops.prefer_scan_packed(packed, ops.SeqOffsets(cu, device=cuda), N_CLASS, pen_d, key=key)
    assert _eq(fresh.cpu().numpy(), got)
    # the padded block through cwlt_prefer_scan
    pad = np.zeros((n, Lb, A), dtype=np.int64)
    for i, x in enumerate(songs):
        pad[i, :len(x)] = x
    pkey = torch.as_tensor(np.repeat(order, Lb)).to(cuda) if keyed else None
    rect = ops.prefer_scan(torch.as_tensor(pad.reshape(-1, A)).to(cuda), n, N_CLASS, pen_d, key=pkey)
    rect = rect.cpu().numpy().reshape(n, Lb, W)
    for i, (a, z) in enumerate(zip(cu, cu[1:])):
        assert _eq(got[a:z], rect[i, :z - a]), i
        assert _eq(got[a:z], prefs[order[i]].seen_states(songs[i])), i
    assert got.max() > 1 and (got != np.round(got)).any()                # states above one hit, and fractional ones


# ---- 3. the model layer -----------------------------------------------------------------------------------------------------
HID_LENS = [1, 31, 32, 33, 65, 100, 7]


def _memory(net, n, dev):
    enc = net.transformer_encoder
    H = enc.layers[0].attention.n_heads
    d = net.d_model // H
    return [[torch.zeros((n, H, d, d), device=dev), torch.zeros((n, H, d), device=dev)] for _ in enc.layers]


@pytest.fixture(scope="module")
def hidden_ref(world, cuda):
    """prefill_hidden(kernel="gemm") of the ragged songs, once: hidden, last-row logits, all-row logits, states."""
    net = world["net"]
    songs = _random_songs(np.random.default_rng(9), HID_LENS)
    n, L = len(songs), max(HID_LENS)
    pad = np.zeros((n, L, A), dtype=np.int64)
    for i, x in enumerate(songs):
        pad[i, :len(x)] = x
    toks = torch.as_tensor(pad).to(cuda)
    mem = _memory(net, n, cuda)
    h, lg = net.prefill_hidden(toks, mem, HID_LENS, kernel="gemm", logits=True)
    every = net.prefill_hidden(toks, _memory(net, n, cuda), HID_LENS, kernel="gemm", logits="all")
    return songs, h, lg, every, mem


@pytest.mark.parametrize("rows,perm", [(None, None), (64, None), (None, [3, 6, 0, 5, 1, 4, 2]), (64, [6, 5, 4, 3, 2, 1, 0])])
def test_prefill_hidden_packed(world, cuda, hidden_ref, rows, perm):
    net = world["net"]
    songs, h, lg, every, mem = hidden_ref
    order = list(range(len(songs))) if perm is None else perm
    mine = [songs[i] for i in order]
    cu = _cu([len(x) for x in mine])
    toks = torch.as_tensor(np.concatenate(mine)).to(cuda)
    assert rows is None or any(a // rows != (z - 1) // rows for a, z in zip(cu, cu[1:]))   # a call boundary in a song
    m1 = _memory(net, len(mine), cuda)
    h1, lg1 = net.prefill_hidden_packed(toks, cu, m1, logits=True, rows=rows)
    idx = torch.as_tensor(order, device=cuda)
    assert torch.equal(h1, h[idx]) and torch.equal(lg1, lg[idx])
    for (S1, Z1), (S, Z) in zip(m1, mem):
        assert torch.equal(S1, S[idx]) and torch.equal(Z1, Z[idx])
        assert S1.abs().max().item() > 0
    m2 = _memory(net, len(mine), cuda)
    all1 = net.prefill_hidden_packed(toks, ops.SeqOffsets(cu, device=cuda), m2, logits="all", rows=rows)
    assert all1.shape == (cu[-1], sum(N_CLASS))
    for j, i in enumerate(order):
        assert torch.equal(all1[cu[j]:cu[j + 1]], every[i, :len(songs[i])]), (j, i)
    for (S2, Z2), (S1, Z1) in zip(m2, m1):
        assert torch.equal(S2, S1) and torch.equal(Z2, Z1)


def test_prefill_hidden_packed_refusals(world, cuda):
    net = world["net"]
    toks = torch.zeros((10, A), dtype=torch.int64, device=cuda)
    mem = _memory(net, 2, cuda)
    for rows in (0, 4097):
        with pytest.raises(ValueError, match="rows must be in"):
            net.prefill_hidden_packed(toks, [0, 3, 10], mem, rows=rows)
    with pytest.raises(ValueError, match="ends at row"):
        net.prefill_hidden_packed(toks, [0, 3, 11], mem)
    with pytest.raises(ValueError, match="strictly increasing"):
        net.prefill_hidden_packed(toks, [0, 0, 10], mem)
    with pytest.raises(ValueError, match="state holds"):
        net.prefill_hidden_packed(toks, [0, 3, 10], _memory(net, 3, cuda))
    with pytest.raises(ValueError, match="logits must be"):
        net.prefill_hidden_packed(toks, [0, 3, 10], mem, logits=False)
    with pytest.raises(RuntimeError):
        net.prefill_hidden_packed(toks.cpu(), [0, 3, 10], mem)
    net.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            generation.DecodeSession(net, n_songs=2, kernel="gemm").prefill([np.zeros((3, A), np.int64)] * 2,
                                                                            kernel="packed")
    finally:
        net.eval()
    bf = _small_model(cuda, int(FIX["fill_seed"]))
    bf.compute_dtype = torch.bfloat16
    with pytest.raises(RuntimeError, match="f32"):
        bf.prefill_hidden_packed(toks, [0, 3, 10], mem)
    from rlmg_amd.dqn_policy import model
    trainer = model.LinearTransformer(N_CLASS, is_training=True).to(cuda).eval()
    with pytest.raises(RuntimeError, match="recurrent"):
        trainer.prefill_hidden_packed(toks, [0, 3, 10], mem)


# ---- 4. the session ---------------------------------------------------------------------------------------------------------
def test_session_prefill_packed(world, cuda):
    net = world["net"]
    lens = [5, 48, 1, 33, 17, 40]
    assert len(generation.packed_blocks(lens, 60)) == 3
    rng = np.random.default_rng(4)
    songs = _random_songs(rng, lens)
    pad = np.zeros((len(lens), max(lens), A), dtype=np.int64)
    for i, x in enumerate(songs):
        pad[i, :len(x)] = x
    nxt = np.stack(_random_songs(rng, [6] * len(lens)))                  # (6 songs, 6 steps, A)
    more = _random_songs(rng, [9, 2, 30, 4, 11, 1])
    sess = {k: generation.DecodeSession(net, n_songs=len(lens), kernel="gemm", graph=True) for k in ("gemm", "packed")}
    ptr = sess["packed"]._state.data_ptr()
    out = {}
    for k, s in sess.items():
        s.reset()
        first = s.prefill(pad, lengths=lens, kernel=k, prefill_rows=60).copy()
        state, hid = s._state.clone(), s.hidden.clone()
        assert s.n_steps == 48
        steps = [s.step(nxt[:, t]).copy() for t in range(3)]             # the first step captures the graph
        assert s._graph is not None
        # a second prefill, from the state the session holds, into the captured graph's buffers
        again = s.prefill(more if k == "packed" else _padded(more), lengths=None if k == "packed" else
                          [len(x) for x in more], kernel=k, prefill_rows=60).copy()
        state2 = s._state.clone()
        steps += [s.step(nxt[:, t]).copy() for t in range(3, 6)]
        out[k] = (first, state, hid, steps, again, state2, s.hidden.clone(), s.n_steps)
    assert sess["packed"]._state.data_ptr() == ptr
    g, p = out["gemm"], out["packed"]
    assert _eq(p[0], g[0]) and torch.equal(p[1], g[1]) and torch.equal(p[2].view(-1), g[2].view(-1))
    assert all(_eq(a, b) for a, b in zip(p[3], g[3]))
    assert _eq(p[4], g[4]) and torch.equal(p[5], g[5]) and torch.equal(p[6].view(-1), g[6].view(-1)) and p[7] == g[7]
    # an eager session agrees with the graphed one step by step
    eager = generation.DecodeSession(net, n_songs=len(lens), kernel="gemm", graph=False)
    eager.reset()
    assert _eq(eager.prefill(songs, kernel="packed", prefill_rows=60), p[0])      # the list form
    for t in range(3):
        assert _eq(eager.step(nxt[:, t]), p[3][t])
    with pytest.raises(ValueError, match="at least one row"):
        eager.prefill([x[:0] if i == 2 else x for i, x in enumerate(songs)], kernel="packed")
    with pytest.raises(ValueError, match="prefill_rows"):
        eager.prefill(songs, kernel="packed", prefill_rows=0)
    with pytest.raises(ValueError, match="kernel must be"):
        eager.prefill(songs, kernel="pack")


def _padded(arrays):
    out = np.zeros((len(arrays), max(len(x) for x in arrays), A), dtype=np.int64)
    for i, x in enumerate(arrays):
        out[i, :len(x)] = x
    return out


# ---- 5. the scorers ---------------------------------------------------------------------------------------------------------
SCORE_LENS = [2, 33, 64, 65, 7, 130]


def _score_options(w):
    w2e = w["w2e"]
    scale = Preference(w2e, bias={"pitch": {k: 2.0 for k in range(5, 12)}, "bar-beat": {"Bar": 1.0}})
    chords = Preference(w2e, per_bar={"chord": [{2: 3.0}, {5: 3.0, 6: 3.0}]}, cycle=True)
    forget = Preference(w2e, repeat={"pitch": (0.5, 2.0), "duration": 1.0}, decay=0.9)
    rng = Constraint(w2e, allow={"pitch": range(5, 40)})
    bars = Constraint(w2e, per_bar={"pitch": [[5, 6, 7], [20, 21, 22]]}, cycle=True)
    return dict(constraints=[rng, None, bars, rng, None, bars], grammar=Grammar(w2e),
                preferences=[forget, scale, None, chords, forget, chords], reference=w["ref"],
                alpha=np.linspace(0.2, 1.1, len(SCORE_LENS)), sampler="dqn")


@pytest.mark.parametrize("form", ["plain", "everything", "dataset"])
def test_scorers_packed_equal_gemm(world, form):
    w = world
    rng = np.random.default_rng(12)
    songs = _random_songs(rng, SCORE_LENS)
    assert len(generation.packed_blocks(SCORE_LENS, 70)) == 5
    kw, mask = {}, None
    if form == "everything":
        kw = _score_options(w)
    elif form == "dataset":
        T = max(SCORE_LENS)
        arr = np.stack(_random_songs(rng, [T] * len(SCORE_LENS)))
        mask = np.zeros((len(SCORE_LENS), T), dtype=np.float32)
        for i, L in enumerate(SCORE_LENS):
            mask[i, :L] = 1.0
        songs = arr
    out = {}
    for kernel in ("gemm", "packed"):
        sc = generation.score_songs(w["net"], w["w2e"], songs, kernel=kernel, mask=mask, prefill_rows=70, **kw)
        st = generation.policy_stats(w["net"], w["w2e"], songs, kernel=kernel, mask=mask, prefill_rows=70,
                                     **dict(kw) if form == "everything" else dict(reference=w["ref"]))
        out[kernel] = sc, st
    for which in (0, 1):
        a, b = out["packed"][which], out["gemm"][which]
        assert len(a) == len(b) == len(SCORE_LENS)
        for i, (x, y, L) in enumerate(zip(a, b, SCORE_LENS)):
            assert x.shape[0] == L - 1 and np.array_equal(x, y, equal_nan=True) and _eq(x, y), (form, which, i)
    assert np.isfinite(out["packed"][0][-1][..., 0]).all()
    if form == "everything":                                             # the options do move the scores
        plain = generation.score_songs(w["net"], w["w2e"], songs, kernel="packed", prefill_rows=70)
        assert not any(_eq(x, y) for x, y in zip(plain[1:], out["packed"][0][1:]))
    # one block for all songs: the same bits again (batch invariance carries over)
    one = generation.score_songs(w["net"], w["w2e"], songs, kernel="packed", mask=mask, **kw)
    assert all(_eq(x, y) for x, y in zip(one, out["packed"][0]))


# ---- 6. the lock-step generators --------------------------------------------------------------------------------------------
P_LENS = [3, 40, 7, 17, 1, 26]


@pytest.fixture(scope="module")
def prompts(world):
    """Six prompts of 1 .. 40 rows: prefixes of songs the model draws itself."""
    torch.manual_seed(5)
    songs = generation.generate_batch(world["net"], world["w2e"], len(P_LENS), bar_cond=100, max_tokens=48,
                                      sampler="categorical")
    return [s[:p].copy() for s, p in zip(songs, P_LENS)]


def test_generate_batch_packed(world, prompts):
    w = world
    out = {}
    for prefill in ("gemm", "packed"):
        torch.manual_seed(3)
        out[prefill] = generation.generate_batch(w["net"], w["w2e"], len(prompts), bar_cond=100, max_tokens=60, chunk=16,
                                                 prompts=prompts, prefill=prefill, sampler="categorical",
                                                 return_logprobs=True)
    assert _same(out["packed"][0], out["gemm"][0]) and _bits(out["packed"][1], out["gemm"][1])
    assert all(len(s) == 60 and (s[:len(p)] == p).all() for s, p in zip(out["packed"][0], prompts))


def test_generate_particles_packed(world, prompts):
    w = world
    K, out = 2, {}
    kw = dict(bar_cond=100, max_tokens=56, chunk=16, resample_every=4, ess=1.0, prompts=prompts, sampler="categorical",
              constraints=Constraint(w["w2e"], per_bar={"pitch": [[5, 6, 7], [20, 21, 22]]}, cycle=True))
    for name, extra in (("gemm", dict(prefill="gemm")), ("packed", dict(prefill="packed")),
                        ("rows", dict(prefill="packed", share_prefill=False))):
        torch.manual_seed(3)
        out[name] = generation.generate_particles(w["net"], w["w2e"], len(prompts), K, **kw, **extra)
    for name in ("packed", "rows"):
        for a, b in zip(out[name], out["gemm"]):
            assert _same(a.songs, b.songs) and _bits(a.logprobs, b.logprobs)
            assert _eq(a.log_weights, b.log_weights) and a.log_evidence == b.log_evidence
            assert np.array_equal(a.ancestors, b.ancestors) and np.array_equal(a.resampled, b.resampled)
    assert any(ps.resampled.any() for ps in out["gemm"])


# ---- 7. the bank streams ----------------------------------------------------------------------------------------------------
def test_stream_bank_packed(world, prompts):
    w = world
    out = {}
    for packed in (False, True):
        torch.manual_seed(3)
        out[packed] = generation._generate_stream(w["net"], w["w2e"], len(prompts), slots=2, bar_cond=100,
                                                  max_tokens=48, chunk=8, prompts=prompts, prefill_rows=80,
                                                  sampler="categorical", return_logprobs=True,
                                                  packed_prefill=packed)
    (songs, lps), st = out[True]
    (songs0, lps0), st0 = out[False]
    assert _same(songs, songs0) and _bits(lps, lps0)
    assert st["prefill_blocks"] == st0["prefill_blocks"] >= 3 and st["block"] == st0["block"] == 2
    assert st["bank"] == st0["bank"]
    torch.manual_seed(3)
    got = generation.generate_stream(w["net"], w["w2e"], len(prompts), slots=2, bar_cond=100, max_tokens=48, chunk=8,
                                     prompts=prompts, prefill_rows=80, sampler="categorical", packed_prefill=True)
    assert _same(got, songs)


def test_particle_bank_stream_packed(world, prompts):
    w = world
    N, K, R, CHUNK, CAP = len(prompts), 2, 4, 16, 56
    cons = Constraint(w["w2e"], per_bar={"pitch": [[5, 6, 7], [20, 21, 22]]}, cycle=True)
    out = {}
    for packed in (False, True):
        torch.manual_seed(3)
        heads, caps, plan = generation._particle_setup("generate_particles", w["net"], w["w2e"], N, K, R, 1.0, 100, CAP,
                                                       prompts, "categorical", CHUNK, "blas", cons, None, w["ref"], 0.7,
                                                       None, pool=2)
        stats = {}
        sets = generation._run_particle_stream(w["net"], w["w2e"], heads, caps, plan, N, K, 2, R, 1.0, 100, CHUNK, None,
                                               heads[0], stats=stats, bank="auto", prefill_rows=80,
                                               packed_prefill=packed)
        out[packed] = sets, stats
    for a, b in zip(out[True][0], out[False][0]):
        assert _same(a.songs, b.songs) and _bits(a.logprobs, b.logprobs)
        assert _eq(a.log_weights, b.log_weights) and a.log_evidence == b.log_evidence
        assert np.array_equal(a.ancestors, b.ancestors)
    assert out[True][1]["prefill_blocks"] == out[False][1]["prefill_blocks"] >= 3
    torch.manual_seed(3)
    got = generation.generate_particles(w["net"], w["w2e"], N, K, bar_cond=100, max_tokens=CAP, chunk=CHUNK,
                                        resample_every=R, ess=1.0, prompts=prompts, sampler="categorical",
                                        constraints=cons, reference=w["ref"], alpha=0.7, slots=2, bank="auto",
                                        prefill_rows=80, packed_prefill=True)
    for a, b in zip(got, out[False][0]):
        assert _same(a.songs, b.songs) and _eq(a.log_weights, b.log_weights)

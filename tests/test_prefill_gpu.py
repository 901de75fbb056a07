"""GPU: prompt prefill -- the state-carrying scan (csrc/prefill.hip, ops.cla_fwd_state) against the f64 recurrent
oracle, DecodeSession.prefill against the reference-recorded generation fixture, continuation / batching / graph
capture semantics, and the prompt-taking generation surface."""
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
from rlmg_amd.sampling import sample_cw  # noqa: E402
from oracle.cla import cla_recurrent_step  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]
SENTINEL = 12345.0


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
    return sum(w2e["bar-beat"][int(r[2])] == "Bar" for r in rows)


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the oracle
# ------------------------------------------------------------------------------------------------------------------
def _oracle(q, k, v, S, Z):
    """f64 CPU: token by token through oracle.cla.cla_recurrent_step.  q, k, v (L, H, 64) of ONE sequence."""
    outs, st = [], [S[None].clone(), Z[None].clone()]
    for t in range(q.shape[0]):
        o, st = cla_recurrent_step(q[t][None], k[t][None], v[t][None], st)
        outs.append(o[0])
    return (torch.stack(outs) if outs else q.new_zeros((0,) + q.shape[1:])), st[0][0], st[1][0]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H", [2, 8])
def test_scan_with_state_matches_oracle(cuda, N, H):
    g = torch.Generator().manual_seed(100 * N + H)
    D = H * 64
    for L in (1, 31, 32, 33, 200, 4096):
        qkv = (0.5 * torch.randn(N * L, 3 * D, generator=g)).to(cuda)              # packed (R, 3D): row stride 3D
        q, k, v = (qkv[:, i * D:(i + 1) * D].view(N, L, H, 64) for i in range(3))
        # a non-zero starting state: the oracle over a random prefix, rounded to f32 (both sides start from it)
        S0, Z0 = [], []
        for n in range(N):
            pre = 0.5 * torch.randn(3, 7, H, 64, generator=g, dtype=torch.float64)
            _, s, z = _oracle(pre[0], pre[1], pre[2], torch.zeros(H, 64, 64, dtype=torch.float64),
                              torch.zeros(H, 64, dtype=torch.float64))
            S0.append(s.float())
            Z0.append(z.float())
        S0, Z0 = torch.stack(S0), torch.stack(Z0)
        lens = [L] if N == 1 else [L, 0, (L + 1) // 2]
        qc, kc, vc = (t.double().cpu() for t in (q, k, v))
        refs = [_oracle(qc[n, :ln], kc[n, :ln], vc[n, :ln], S0[n].double(), Z0[n].double())
                for n, ln in enumerate(lens)]
        # one workgroup per (sequence, head), and the library's few-stream choice (runs of chunks, 3 passes)
        for seg in (1, None):
            S, Z = S0.clone().to(cuda), Z0.clone().to(cuda)
            out = torch.full((N, L, H, 64), SENTINEL, device=cuda)
            got = ops.cla_fwd_state(q, k, v, S, Z, torch.tensor(lens, dtype=torch.int32, device=cuda), out=out,
                                    segments=seg)
            assert got.data_ptr() == out.data_ptr()
            torch.cuda.synchronize()
            got, Sg, Zg = got.cpu(), S.cpu(), Z.cpu()
            for n, ln in enumerate(lens):
                ref, Sr, Zr = refs[n]
                if ln:
                    scale = ref.abs().amax(dim=(1, 2)).clamp_min(1.0)                    # per-row scale
                    err = (got[n, :ln].double() - ref).abs().amax(dim=(1, 2)) / scale
                    assert err.max().item() < 1e-4, (L, seg, n, err.max().item())
                assert (got[n, ln:] == SENTINEL).all(), (L, seg, n)                      # rows past the length
                assert (Sg[n].double() - Sr).abs().max().item() <= 1e-5 * Sr.abs().max().item(), (L, seg, n)
                assert (Zg[n].double() - Zr).abs().max().item() <= 1e-5 * Zr.abs().max().item(), (L, seg, n)
                if ln == 0:                                                              # bit for bit untouched
                    assert torch.equal(Sg[n], S0[n]) and torch.equal(Zg[n], Z0[n])
        # the same final state as L calls of the one-token kernel (sequences that run the whole length)
        Ss, Zs = S0.clone().to(cuda), Z0.clone().to(cuda)
        rows = qkv.view(N, L, 3 * D)
        for t in range(L):
            ops.recurrent_cla_step(rows[:, t], Ss, Zs, H)
        Ss, Zs = Ss.cpu(), Zs.cpu()
        for n, ln in enumerate(lens):
            if ln == L:
                assert (Sg[n] - Ss[n]).abs().max().item() <= 1e-5 * Ss[n].abs().max().item(), (L, n)
                assert (Zg[n] - Zs[n]).abs().max().item() <= 1e-5 * Zs[n].abs().max().item(), (L, n)
    # no lengths = all L
    S, Z = S0.clone().to(cuda), Z0.clone().to(cuda)
    S2, Z2 = S0.clone().to(cuda), Z0.clone().to(cuda)
    a = ops.cla_fwd_state(q, k, v, S, Z)
    b = ops.cla_fwd_state(q, k, v, S2, Z2, torch.full((N,), L, dtype=torch.int32, device=cuda))
    assert torch.equal(a, b) and torch.equal(S, S2) and torch.equal(Z, Z2)


def test_scan_with_state_refusals(cuda):
    q = torch.randn(1, 8, 2, 64, device=cuda)
    S, Z = torch.zeros(1, 2, 64, 64, device=cuda), torch.zeros(1, 2, 64, device=cuda)
    with pytest.raises(RuntimeError, match="status 1002"):                        # CWLT_ERR_DTYPE through _lib.check
        b = q.bfloat16()
        ops.cla_fwd_state(b, b, b, S, Z)
    with pytest.raises(ValueError):
        ops.cla_fwd_state(q, q, q, S[:, :1], Z)
    with pytest.raises(ValueError):
        ops.cla_fwd_state(q, q, q, S, Z, torch.ones(2, dtype=torch.int32, device=cuda))


# ------------------------------------------------------------------------------------------------------------------
# 2. DecodeSession.prefill against the reference-recorded fixture
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,fused", [(False, False), (True, False), (False, True), (True, True)])
def test_prefill_matches_reference_stream(cuda, graph, fused):
    net = _small_model(cuda)
    sess = generation.DecodeSession(net, graph=graph, fused=fused)
    T = len(FIX["logits"])
    for P in (1, 2, 17, 33, 48):
        sess.reset()
        got = sess.prefill(FIX["tokens"][:P])
        assert got.shape == (sum(N_CLASS),)
        assert np.abs(got - FIX["logits"][P - 1]).max() < 1e-4, P          # pe[0] on every row: fails from P = 2
        assert np.abs(sess.hidden.view(-1).cpu().numpy() - FIX["h"][P - 1]).max() < 1e-4, P
        assert sess.n_steps == P
        for t in range(P, T):                                               # the exported state is the step's own
            assert np.abs(sess.step(FIX["tokens"][t]) - FIX["logits"][t]).max() < 1e-4, (P, t)


# ------------------------------------------------------------------------------------------------------------------
# 3. continuation: prefill starts from whatever state the session holds
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_prefill_continues_the_state(cuda, fused):
    net = _small_model(cuda)
    toks = FIX["tokens"][:40]
    one = generation.DecodeSession(net, graph=False, fused=fused)
    ref = one.prefill(toks).copy()
    ref_state = one._state.clone()
    two = generation.DecodeSession(net, graph=False, fused=fused)
    two.prefill(toks[:13])
    got = two.prefill(toks[13:])
    assert np.abs(got - ref).max() < 1e-5 and two.n_steps == 40
    assert (two._state - ref_state).abs().max().item() <= 1e-5 * ref_state.abs().max().item()
    # step x3, then the rest in one prefill == stepping all of it
    stepped = generation.DecodeSession(net, graph=False, fused=fused)
    for t in range(40):
        want = stepped.step(toks[t]).copy()
    mixed = generation.DecodeSession(net, graph=False, fused=fused)
    for t in range(3):
        mixed.step(toks[t])
    got = mixed.prefill(toks[3:])
    assert np.abs(got - want).max() < 1e-5 and mixed.n_steps == 40
    assert (mixed.hidden.view(-1) - stepped.hidden.view(-1)).abs().max().item() < 1e-5


@pytest.mark.parametrize("fused", [True, False])
def test_prefilled_state_survives_graph_capture(cuda, fused):
    net = _small_model(cuda)
    eager = generation.DecodeSession(net, graph=False, fused=fused)
    sess = generation.DecodeSession(net, graph=True, fused=fused)
    ptr = sess._state.data_ptr()
    a, b = sess.prefill(FIX["tokens"][:20]), eager.prefill(FIX["tokens"][:20])
    assert sess._graph is None and np.abs(a - b).max() < 1e-5
    for t in range(20, 30):                     # the first step captures the graph (and restores the state after)
        a, b = sess.step(FIX["tokens"][t]).copy(), eager.step(FIX["tokens"][t]).copy()
        assert np.abs(a - b).max() < 1e-5, t
        assert np.abs(a - FIX["logits"][t]).max() < 1e-4, t
    assert sess._graph is not None and sess._state.data_ptr() == ptr
    # a second prefill on the captured session writes into the same buffers; hidden follows the replays
    sess.reset()
    eager.reset()
    a, b = sess.prefill(FIX["tokens"][:5]), eager.prefill(FIX["tokens"][:5])
    assert np.abs(a - b).max() < 1e-5 and sess._state.data_ptr() == ptr
    a, b = sess.step(FIX["tokens"][5]), eager.step(FIX["tokens"][5])
    assert np.abs(a - FIX["logits"][5]).max() < 1e-4
    assert (sess.hidden.view(-1) - eager.hidden.view(-1)).abs().max().item() < 1e-5


# ------------------------------------------------------------------------------------------------------------------
# 4. several songs, ragged prompts
# ------------------------------------------------------------------------------------------------------------------
def test_prefill_batch_of_ragged_prompts(cuda):
    net = _small_model(cuda)
    g = torch.Generator().manual_seed(4)
    lens = [5, 48, 1]
    toks = torch.stack([torch.randint(0, n, (3, 48), generator=g) for n in N_CLASS], -1).numpy()     # (3, 48, 6)
    toks[1] = FIX["tokens"][:48]
    nxt = torch.stack([torch.randint(0, n, (3, 6), generator=g) for n in N_CLASS], -1).numpy()       # (3, 6, 6)
    batch = generation.DecodeSession(net, n_songs=3)
    got = batch.prefill(toks, lengths=lens).copy()
    assert got.shape == (3, sum(N_CLASS)) and batch.n_steps == 48
    hid = batch.hidden.clone()
    after = np.stack([batch.step(nxt[:, t]).copy() for t in range(6)], 1)
    single = generation.DecodeSession(net)
    for i, n in enumerate(lens):
        single.reset()
        assert np.abs(single.prefill(toks[i, :n]) - got[i]).max() < 1e-4, i
        assert (single.hidden.view(-1) - hid[i]).abs().max().item() < 1e-4, i
        for t in range(6):
            assert np.abs(single.step(nxt[i, t]) - after[i, t]).max() < 1e-4, (i, t)
    assert np.abs(got[1] - FIX["logits"][47]).max() < 1e-4
    # refusals: lengths of 0 or over P, ids out of range, a wrong song count
    for bad in ([0, 48, 1], [5, 49, 1], [5, 48]):
        with pytest.raises(ValueError):
            batch.prefill(toks, lengths=bad)
    wrong = toks.copy()
    wrong[2, 0, 3] = N_CLASS[3]
    with pytest.raises(ValueError):
        batch.prefill(wrong, lengths=lens)
    with pytest.raises(ValueError):
        batch.prefill(toks[0])


# ------------------------------------------------------------------------------------------------------------------
# 5. the generation surface
# ------------------------------------------------------------------------------------------------------------------
def test_inference_from_prompt(cuda, tmp_path):
    net = _small_model(cuda)
    w2e = _word2event()
    # prompt = INIT_CW is inference_from_scratch: the fixture's stream, cut where the third bar begins
    np.random.seed(int(FIX["np_seed"]))
    res = generation.inference_from_prompt(net, w2e, generation.INIT_CW, bar_cond=3)
    bars = np.cumsum([w2e["bar-beat"][int(r[2])] == "Bar" for r in FIX["tokens"]])
    stop = int(np.argmax(bars == 3)) + 1
    assert res.tolist() == FIX["tokens"][:stop].tolist()
    # a 20-token prompt: the same ids as feeding it through step() under the same np seed
    prompt = FIX["tokens"][:20]
    np.random.seed(3)
    res = generation.inference_from_prompt(net, w2e, prompt, bar_cond=10 ** 6, max_tokens=40)
    np.random.seed(3)
    sess = generation.DecodeSession(net)
    for r in prompt:
        logits = sess.step(r)
    want = list(prompt)
    while len(want) < 40:
        want.append(sample_cw(sess.split(logits)))
        logits = sess.step(want[-1])
    assert res.shape == (40, 6) and res.tolist() == np.stack(want).tolist()
    # device sampling: graph == eager under torch.manual_seed, the song starts with the prompt, and it stops WITH the
    # token that opens bar `bar_cond` (the prompt's own bars counted from prompt[1:] on)
    cond = 1 + _bars(w2e, prompt[1:]) + 2
    songs = []
    for graph in (True, False):
        torch.manual_seed(11)
        sess = generation.DecodeSession(net, graph=graph)
        songs.append(generation.inference_from_prompt(net, w2e, prompt, bar_cond=cond, session=sess,
                                                      device_sampling=True, chunk=16))
    assert songs[0].tolist() == songs[1].tolist()
    song = songs[0]
    assert song[:20].tolist() == prompt.tolist() and len(song) > 20
    assert 1 + _bars(w2e, song[1:]) == cond and w2e["bar-beat"][int(song[-1][2])] == "Bar"
    assert all((song[:, i] < n).all() for i, n in enumerate(N_CLASS))
    res = generation.inference_from_prompt(net, w2e, prompt, bar_cond=10 ** 6, max_tokens=57, device_sampling=True,
                                           chunk=16)
    assert len(res) == 57 and res[:20].tolist() == prompt.tolist()
    # generate(prompt=...): every song continues the prompt
    generation.generate(net, w2e, n_songs=2, bar_cond=10 ** 6, max_tokens=30, path_gendir=str(tmp_path / "gen"),
                        stats_path=None, log=lambda *a: None, prompt=prompt)
    for i in range(2):
        s = np.load(tmp_path / "gen" / ("get_%d.npy" % i))
        assert s.shape == (30, 6) and s[:20].tolist() == prompt.tolist()
    # a prompt that already reaches bar_cond is refused
    with pytest.raises(ValueError):
        generation.inference_from_prompt(net, w2e, FIX["tokens"], bar_cond=1 + _bars(w2e, FIX["tokens"][1:]))


def test_categorical_rollout_and_ppo_testing_with_prompt(cuda, tmp_path, monkeypatch):
    net = _small_model(cuda)
    prompt = FIX["tokens"][:20]
    torch.manual_seed(7)
    a = generation.categorical_rollout(net, 24, carry_memory=True, graph=True, prompt=prompt)
    torch.manual_seed(7)
    b = generation.categorical_rollout(net, 24, carry_memory=True, graph=False, prompt=prompt)
    assert a.shape == (44, 6) and (a == b).all() and a[:20].tolist() == prompt.tolist()
    assert all((a[:, i] < n).all() and (a[:, i] >= 0).all() for i, n in enumerate(N_CLASS))
    with pytest.raises(ValueError):                                     # memory=None per step would drop the prompt
        generation.categorical_rollout(net, 8, prompt=prompt)
    from rlmg_amd.ppo_policy import config, inference
    monkeypatch.chdir(tmp_path)
    old = dict(config.ActorConfig)
    config.ActorConfig.update({"D_MODEL": 128, "N_LAYER": 2, "N_HEAD": 2})
    try:
        song = inference.testing(token_count=6, carry_memory=True, log=lambda *a: None,
                                 prompt=np.zeros((3, 6), dtype=np.int64))
    finally:
        config.ActorConfig.update(old)
    assert song.shape == (9, 6) and (song[:3] == 0).all()


def test_prefill_refusals(cuda):
    w2e = _word2event()
    bf = _small_model(cuda, torch.bfloat16)
    with pytest.raises(RuntimeError):
        generation.DecodeSession(bf, fused=False, graph=False).prefill(FIX["tokens"][:4])
    net = _small_model(cuda).train()
    with pytest.raises(RuntimeError):
        generation.DecodeSession(net).prefill(FIX["tokens"][:4])
    net.eval()
    sess = generation.DecodeSession(net)
    with pytest.raises(ValueError):
        sess.prefill(FIX["tokens"][:0])
    bad = FIX["tokens"][:4].copy()
    bad[1, 0] = -1
    with pytest.raises(ValueError):
        sess.prefill(bad)
    with pytest.raises(ValueError):
        generation.inference_from_prompt(net, w2e, FIX["tokens"][:20], bar_cond=10 ** 6, max_tokens=20)


# ------------------------------------------------------------------------------------------------------------------
# 6. repo dims, f32: one 1 024-token prompt against 1 024 steps
# ------------------------------------------------------------------------------------------------------------------
def test_prefill_repo_dims_1024(cuda):
    from rlmg_amd.dqn_policy import model
    n_class = [56, 135, 18, 87, 18, 25]
    net = fill_params(model.LinearTransformer(n_class, is_training=False), seed=5).to(cuda).eval()
    assert net.d_model == 512 and net.n_layer == 12 and net.compute_dtype == torch.float32
    g = torch.Generator().manual_seed(6)
    toks = torch.stack([torch.randint(0, n, (1024,), generator=g) for n in n_class], -1).numpy()
    step = generation.DecodeSession(net, graph=True)
    for t in range(1024):
        want = step.step(toks[t]).copy()
    pre = generation.DecodeSession(net, graph=True)
    # the projections run in full f32 even where the caller allows TF32 / XF32 matmuls
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = True
    try:
        got = pre.prefill(toks)
        assert torch.backends.cuda.matmul.allow_tf32
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    worst = float(np.abs(got - want).max())
    print("repo dims, 1024-token prompt: worst |prefill - step| logit difference %.3g" % worst)
    assert worst < 1e-4, worst
    assert (pre.hidden - step.hidden).abs().max().item() < 1e-4
    assert np.abs(pre.step(toks[0]) - step.step(toks[0])).max() < 1e-4

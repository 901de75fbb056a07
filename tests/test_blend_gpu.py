"""GPU: blending the policy with a reference model at sampling time.

1. cwlt_blend_logits against the float64 restatement (sampling.blend_logits_f64), element by element:
   |out - f64| <= 4 * 2^-24 * (|alpha| |x| + |1 - alpha| |r|) -- four roundings to f32: 1 - alpha, the two products and
   the sum (an fma saves one).  Rows 1, 3, 64, 257; the fixture's six classes and [1, 2, 3, 4, 5, 64, 255, 256]; row
   strides of width + 5, strides that are multiples of 4 on aligned bases (the 16-byte path), a base one float off (the
   scalar path), a ref_ld of its own, padding columns that keep a sentinel, in place; one shared alpha row, one row per
   row, and rows chosen by key with keys -1, -2 and n_alpha (copied from logits); alpha = 1 and 0 exact under ==.
2. Generation on the small fixture model (128 / 2 layers / 2 heads) with a reference of another seed, and one of one
   layer: alpha = 1 gives bitwise the model's songs, alpha = 0 the reference's, a per-song 1 / 0 pattern song i of the
   matching plain run; the blended stream equals the blended lock-step loop bitwise for every slot count, alpha form
   and sampler, with constraints + grammar + log-probs, a shared prompt, the one-layer reference, graph or eager; the
   drawn rows' log-probs agree with score_songs under the same blend; policy_stats of the blend against the reference.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from fill import fill_params  # noqa: E402

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops, sampling  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = np.load(os.path.join(HERE, "golden", "dqn_generation_small.npz"))
N_CLASS = [int(v) for v in FIX["n_class"]]
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
CLASSES = {"fixture": N_CLASS, "edges": [1, 2, 3, 4, 5, 64, 255, 256]}
ROWS = (1, 3, 64, 257)
SENTINEL = -12345.0
EPS = 2.0 ** -24


# ---- 1. the kernel against float64 -------------------------------------------------------------------------------------
def _strided(cuda, rng, rows, W, ld, offset, fill=None):
    """A (rows, ld) f32 device view with row stride ld whose base sits `offset` floats past a 16-byte aligned address,
    and its host copy: columns < W random over magnitudes 1e-3 .. 1e4 (or `fill`), the padding columns SENTINEL."""
    host = np.full((rows, ld), SENTINEL, dtype=np.float32)
    if fill is None:
        host[:, :W] = (rng.normal(0, 1, (rows, W)) * 10.0 ** rng.uniform(-3, 4, (rows, W))).astype(np.float32)
    else:
        host[:, :W] = fill
    flat = torch.full((rows * ld + 4,), SENTINEL, dtype=torch.float32, device=cuda)
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + rows * ld].view(rows, ld)
    view.copy_(torch.as_tensor(host))
    return view, host


LAYOUTS = {
    # name: (ld, ref_ld, ld_out as functions of W, base offset of logits in floats, takes the 16-byte path)
    "width+5": (lambda W: W + 5, lambda W: W + 5, lambda W: W + 5, 0, None),
    "vector": (lambda W: -(-W // 4) * 4 + 8, lambda W: -(-W // 4) * 4 + 4, lambda W: -(-W // 4) * 4, 0, True),
    "base+1": (lambda W: -(-W // 4) * 4 + 8, lambda W: -(-W // 4) * 4 + 4, lambda W: -(-W // 4) * 4, 1, False),
}


def _check(out, x, r, n_class, alpha_rows, copied, where):
    """out (rows, W) f32 host against blend_logits_f64 with the per-row f32 alpha (rows, A); rows in `copied` equal x.
    -> the worst |out - f64| / bound."""
    W = sum(n_class)
    want = sampling.blend_logits_f64(x[:, :W], r[:, :W], n_class, alpha_rows)
    w = np.repeat(alpha_rows.astype(np.float64), n_class, axis=1)
    bound = 4 * EPS * (np.abs(w) * np.abs(x[:, :W].astype(np.float64)) +
                       np.abs(1.0 - w) * np.abs(r[:, :W].astype(np.float64)))
    keep = ~copied
    assert (out[copied] == x[copied][:, :W]).all(), where
    err = np.abs(out[keep].astype(np.float64) - want[keep])
    assert (err <= bound[keep]).all(), (where, float((err / np.maximum(bound[keep], 1e-300)).max()))
    return float((err / np.maximum(bound[keep], 1e-300)).max()) if keep.any() else 0.0


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("classes", list(CLASSES))
def test_kernel_against_f64(cuda, classes, layout):
    n_class = CLASSES[classes]
    A, W = len(n_class), sum(n_class)
    f_ld, f_ref, f_out, offset, vec = LAYOUTS[layout]
    ld, ref_ld, ld_out = f_ld(W), f_ref(W), f_out(W)
    if vec is not None:                                               # the layout is on the path it is meant for
        assert (ld % 4 == 0 and ref_ld % 4 == 0 and ld_out % 4 == 0) and (offset == 0) == vec
    rng = np.random.default_rng(10 * list(CLASSES).index(classes) + list(LAYOUTS).index(layout))
    worst = 0.0
    for rows in ROWS:
        xd, x = _strided(cuda, rng, rows, W, ld, offset)
        rd, r = _strided(cuda, rng, rows, W, ref_ld, 0)
        none = np.zeros(rows, dtype=bool)

        def run(alpha, key=None, inplace=False):
            """-> the (rows, W) result, after checking that no padding column was written."""
            al = torch.as_tensor(alpha).to(cuda)
            kd = None if key is None else torch.as_tensor(key).to(cuda)
            if inplace:
                buf, _ = _strided(cuda, rng, rows, W, ld, offset, fill=x[:, :W])
                got = ops.blend_logits(buf, rd, n_class, al, key=kd, out=buf)
                assert got is buf
            else:
                buf = torch.full((rows, ld_out), SENTINEL, dtype=torch.float32, device=cuda)
                ops.blend_logits(xd, rd, n_class, al, key=kd, out=buf)
            got = buf.cpu().numpy()
            assert (got[:, W:] == SENTINEL).all(), (rows, "padding columns written")
            assert (xd.cpu().numpy() == x).all() and (rd.cpu().numpy() == r).all()          # the inputs are inputs
            return got[:, :W]

        # one shared row of alpha, also with a key (which a one-row table ignores, idle keys included)
        shared = rng.uniform(-0.7, 3.0, (1, A)).astype(np.float32)
        rep = np.repeat(shared, rows, axis=0)
        worst = max(worst, _check(run(shared), x, r, n_class, rep, none, (rows, "shared")))
        worst = max(worst, _check(run(shared, key=np.full(rows, -1, dtype=np.int64)), x, r, n_class, rep, none,
                                  (rows, "shared, keyed")))
        # one row of alpha per row, no key; rows 0 and 1 (when there) are the exact ends
        per_row = rng.uniform(-0.7, 3.0, (rows, A)).astype(np.float32)
        per_row[0] = 1.0
        per_row[min(1, rows - 1)] = 0.0
        for inplace in (False, True):
            worst = max(worst, _check(run(per_row, inplace=inplace), x, r, n_class, per_row, none,
                                      (rows, "per row", inplace)))
        # rows chosen by key from a table of another size; keys -1 (idle), -2 (waiting) and n_alpha are copied
        n_alpha = rows + 3
        table = rng.uniform(-0.7, 3.0, (n_alpha, A)).astype(np.float32)
        key = rng.integers(0, n_alpha, rows).astype(np.int64)
        bad = rng.choice(rows, size=min(rows, 3), replace=False)
        key[bad] = np.array([-1, -2, n_alpha], dtype=np.int64)[:len(bad)]
        copied = (key < 0) | (key >= n_alpha)
        for inplace in (False, True):
            worst = max(worst, _check(run(table, key=key, inplace=inplace), x, r, n_class,
                                      table[np.clip(key, 0, n_alpha - 1)], copied, (rows, "keyed", inplace)))
        # both ends are exact, element for element (== : a -0 may come back +0)
        for inplace in (False, True):
            assert (run(np.ones((1, A), dtype=np.float32), inplace=inplace) == x[:, :W]).all(), (rows, "alpha = 1")
            assert (run(np.zeros((1, A), dtype=np.float32), inplace=inplace) == r[:, :W]).all(), (rows, "alpha = 0")
    print("blend %s / %s: worst |out - f64| / bound = %.4f" % (classes, layout, worst))
    assert worst <= 1.0


def test_blend_new_tensor_and_non_contiguous_logits(cuda):
    """out=None makes a (rows, W) tensor; inputs wider than W and of different widths are read by their own strides."""
    rng = np.random.default_rng(2)
    W, A = sum(N_CLASS), len(N_CLASS)
    xd, x = _strided(cuda, rng, 7, W, W + 13, 0)
    rd, r = _strided(cuda, rng, 7, W, W + 1, 0)
    alpha = rng.uniform(-0.7, 3.0, (7, A)).astype(np.float32)
    got = ops.blend_logits(xd, rd, N_CLASS, torch.as_tensor(alpha).to(cuda))
    assert got.shape == (7, W) and got.is_contiguous()
    _check(got.cpu().numpy(), x, r, N_CLASS, alpha, np.zeros(7, dtype=bool), "new tensor")


# ---- 2. generation -----------------------------------------------------------------------------------------------------
def _small_model(cuda, seed, layers=2):
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": layers, "N_HEAD": 2})
    try:
        net = model.LinearTransformer(N_CLASS, is_training=False)
    finally:
        config.AgentConfig.update(old)
    return fill_params(net, seed=seed).to(cuda).eval()


def _word2event():
    """Two Bar classes (songs of a few dozen rows at bar_cond 4), Beat_<k> names for the grammar, CONTI for constraints."""
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(KEYS, N_CLASS)}
    for k in KEYS:
        w2e[k][0] = 0
    w2e["tempo"][1] = w2e["chord"][1] = "CONTI"
    w2e["bar-beat"] = {0: 0, 1: "Bar", **{2 + k: "Beat_%d" % k for k in range(16)}}
    w2e["bar-beat"][9] = "Bar"
    return w2e


N_SONGS, BAR_COND, SEED = 24, 4, 12


@pytest.fixture(scope="module")
def world(cuda):
    """The models, the vocabulary, the cap (the median length of a free run, as test_generate_stream_gpu chooses it) and
    the plain songs of the model and of the reference under that cap, per sampler -- computed once, never changed."""
    seed = int(FIX["fill_seed"])
    w = {"net": _small_model(cuda, seed), "ref": _small_model(cuda, seed + 1),
         "ref1": _small_model(cuda, seed + 2, layers=1), "w2e": _word2event()}
    torch.manual_seed(11)
    free = generation.generate_batch(w["net"], w["w2e"], N_SONGS, bar_cond=BAR_COND, max_tokens=300, chunk=32)
    w["cap"] = int(np.median([len(s) for s in free]))
    for sampler in ("dqn", "categorical"):
        for name in ("net", "ref"):
            torch.manual_seed(SEED)
            w[name, sampler] = generation.generate_batch(w[name], w["w2e"], N_SONGS, bar_cond=BAR_COND,
                                                         max_tokens=w["cap"], sampler=sampler, chunk=32)
    lens = [len(s) for s in w["net", "dqn"]]
    assert any(n == w["cap"] for n in lens) and any(n < w["cap"] for n in lens), (w["cap"], lens)
    print("blend generation tests: cap %d rows, the model's songs %s" % (w["cap"], lens))
    return w


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def _bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and
                                    np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _batch(w, alpha, ref="ref", sampler="dqn", **kw):
    torch.manual_seed(SEED)
    return generation.generate_batch(w["net"], w["w2e"], N_SONGS, bar_cond=BAR_COND, max_tokens=w["cap"],
                                     sampler=sampler, chunk=32, reference=w[ref], alpha=alpha, **kw)


def _stream(w, alpha, slots, ref="ref", sampler="dqn", **kw):
    torch.manual_seed(SEED)
    return generation.generate_stream(w["net"], w["w2e"], N_SONGS, slots=slots, bar_cond=BAR_COND,
                                      max_tokens=w["cap"], sampler=sampler, chunk=16, reference=w[ref], alpha=alpha,
                                      **kw)


ALPHA_FORMS = {"scalar": 0.5, "ramp": np.linspace(-0.25, 1.5, N_SONGS),
               "row": np.array([[0.0, 0.25, 0.5, 0.75, 1.0, 1.5]])}


@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_ends_are_the_two_models(world, sampler):
    """alpha = 1: bitwise the model's songs; alpha = 0: the reference's; a per-song 1 / 0 pattern: song i of the matching
    plain run -- against a blend that ignores the key, swaps its operands or takes a seed of its own."""
    w = world
    assert not _same(w["net", sampler], w["ref", sampler])
    assert _same(_batch(w, 1, sampler=sampler), w["net", sampler])
    assert _same(_batch(w, 0.0, sampler=sampler), w["ref", sampler])
    pattern = np.arange(N_SONGS) % 2 == 0                             # 1, 0, 1, 0, ...
    want = [w["net" if m else "ref", sampler][i] for i, m in enumerate(pattern)]
    assert _same(_batch(w, pattern.astype(np.float64), sampler=sampler), want)
    assert _same(_stream(w, pattern.astype(np.float64), 5, sampler=sampler), want)
    # the (n_songs, A) form: attribute by attribute the same pattern
    assert _same(_batch(w, np.repeat(pattern[:, None], 6, axis=1).astype(np.float32), sampler=sampler), want)


@pytest.mark.parametrize("form", list(ALPHA_FORMS))
@pytest.mark.parametrize("sampler", ["dqn", "categorical"])
def test_stream_equals_batch(world, sampler, form):
    w = world
    alpha = ALPHA_FORMS[form]
    want = _batch(w, alpha, sampler=sampler)
    assert not _same(want, w["net", sampler]) and not _same(want, w["ref", sampler])
    for slots in (1, 5, 24, 40):
        assert _same(_stream(w, alpha, slots, sampler=sampler), want), slots


def test_stream_equals_batch_constrained_grammar_logprobs(world):
    w = world
    w2e = w["w2e"]
    musical = generation.Constraint(w2e, allow={"tempo": ["tempo_3"], "pitch": range(5, 12)},
                                    per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7]]}, cycle=True)
    kw = dict(constraints=[musical if i % 3 else None for i in range(N_SONGS)], grammar=generation.Grammar(w2e),
              return_logprobs=True)
    alpha = ALPHA_FORMS["ramp"]
    songs, lps = _batch(w, alpha, **kw)
    assert not any(kw["grammar"].violations(s, 1) for s in songs)
    assert _same(_batch(w, alpha, **{**kw, "return_logprobs": False}), songs)          # the flag changes no song
    for slots in (5, 40):
        got, got_lp = _stream(w, alpha, slots, **kw)
        assert _same(got, songs) and _bits(got_lp, lps), slots


def test_stream_equals_batch_shared_prompt(world):
    w = world
    bars = np.cumsum([w["w2e"]["bar-beat"][int(r[2])] == "Bar" for r in FIX["tokens"][1:]])
    prompt = FIX["tokens"][:int(np.argmax(bars >= 1)) + 2]             # one Bar after the first row
    cap = len(prompt) + w["cap"]
    out = []
    for prefill in ("gemm", "blas"):
        torch.manual_seed(SEED)
        out.append(generation.generate_batch(w["net"], w["w2e"], N_SONGS, bar_cond=BAR_COND, max_tokens=cap,
                                             prompts=prompt, chunk=32, prefill=prefill, reference=w["ref"], alpha=0.5))
        assert all((s[:len(prompt)] == prompt).all() and len(s) > len(prompt) for s in out[-1])
    for slots in (5, 24):                                             # the snapshot is a one-row gemm prefill
        torch.manual_seed(SEED)
        got = generation.generate_stream(w["net"], w["w2e"], N_SONGS, slots=slots, bar_cond=BAR_COND, max_tokens=cap,
                                         prompt=prompt, chunk=16, reference=w["ref"], alpha=0.5)
        assert _same(got, out[0]), slots
    # the first draw comes from the blended prefill logits: alpha = 0 is the reference continuing the prompt
    torch.manual_seed(SEED)
    plain = generation.generate_batch(w["ref"], w["w2e"], N_SONGS, bar_cond=BAR_COND, max_tokens=cap, prompts=prompt,
                                      chunk=32, prefill="gemm")
    torch.manual_seed(SEED)
    zero = generation.generate_batch(w["net"], w["w2e"], N_SONGS, bar_cond=BAR_COND, max_tokens=cap, prompts=prompt,
                                     chunk=32, prefill="gemm", reference=w["ref"], alpha=0)
    assert _same(zero, plain)
    # a prompt of its own for every song: the lock-step form takes it
    torch.manual_seed(SEED)
    ragged = generation.generate_batch(w["net"], w["w2e"], 3, bar_cond=BAR_COND, max_tokens=cap,
                                       prompts=[prompt, prompt[:2], prompt[:1]], prefill="gemm", reference=w["ref"],
                                       alpha=[1.0, 0.5, 0.0])
    assert [len(s) > n for s, n in zip(ragged, (len(prompt), 2, 1))] == [True] * 3


def test_one_layer_reference(world):
    w = world
    alpha = ALPHA_FORMS["ramp"]
    want = _batch(w, alpha, ref="ref1")
    assert not _same(want, _batch(w, alpha))
    for slots in (5, 40):
        assert _same(_stream(w, alpha, slots, ref="ref1"), want), slots
    torch.manual_seed(SEED)
    own = generation.generate_batch(w["ref1"], w["w2e"], N_SONGS, bar_cond=BAR_COND, max_tokens=w["cap"], chunk=32)
    assert _same(_batch(w, 0, ref="ref1"), own)


def test_graph_equals_eager(world, monkeypatch):
    w = world
    alpha = ALPHA_FORMS["ramp"]
    torch.manual_seed(SEED)
    graphed, st = generation._generate_stream(w["net"], w["w2e"], N_SONGS, slots=5, bar_cond=BAR_COND,
                                              max_tokens=w["cap"], chunk=16, reference=w["ref"], alpha=alpha)
    assert st["graph"]
    batch = _batch(w, alpha)
    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    torch.manual_seed(SEED)
    eager, st = generation._generate_stream(w["net"], w["w2e"], N_SONGS, slots=5, bar_cond=BAR_COND,
                                            max_tokens=w["cap"], chunk=16, reference=w["ref"], alpha=alpha)
    assert not st["graph"]
    assert _same(graphed, eager) and _same(_batch(w, alpha), batch) and _same(batch, eager)


def test_logprobs_agree_with_score_songs(world):
    """sampler="categorical": no nucleus, so every drawn row's pair is finite and none is exempt; 1e-4 is the tolerance
    DESIGN §4.6g gives the step-against-prefill comparison."""
    w = world
    songs, lps = _batch(w, 0.5, sampler="categorical", return_logprobs=True)
    scored = generation.score_songs(w["net"], w["w2e"], songs, sampler="categorical", reference=w["ref"], alpha=0.5)
    worst = 0.0
    for s, lp, sc in zip(songs, lps, scored):
        assert lp.shape == (len(s) - 1, 6, 2) and sc.shape == lp.shape and np.isfinite(lp).all()
        worst = max(worst, float(np.abs(lp - sc).max()))
    print("blend: generated against scored log-probs, worst |difference| = %.3g" % worst)
    assert worst <= 1e-4
    # the pair is the blend's: it is neither model's own
    own = generation.score_songs(w["net"], w["w2e"], songs, sampler="categorical")
    assert max(float(np.abs(a - b).max()) for a, b in zip(own, scored)) > 1e-2
    # a per-song alpha is keyed by the song index, whatever the block a song falls in
    ramp = ALPHA_FORMS["ramp"]
    whole = generation.score_songs(w["net"], w["w2e"], songs, reference=w["ref"], alpha=ramp)
    blocks = generation.score_songs(w["net"], w["w2e"], songs, reference=w["ref"], alpha=ramp,
                                    prefill_rows=2 * max(len(s) for s in songs))
    assert _bits(whole, blocks)
    one = generation.score_songs(w["net"], w["w2e"], songs[7:8], reference=w["ref"], alpha=float(np.float32(ramp[7])))
    assert _bits(one, whole[7:8])


def _row_logprobs(net, song, cuda):
    """float64 log-softmax per attribute of every row's logits (L, W), from the model's own batch-invariant prefill."""
    enc = net.transformer_encoder
    H = enc.layers[0].attention.n_heads
    d = net.d_model // H
    memory = [[torch.zeros((1, H, d, d), device=cuda), torch.zeros((1, H, d), device=cuda)] for _ in enc.layers]
    with torch.no_grad():
        lg = net.prefill_hidden(torch.as_tensor(song[None]).to(cuda), memory, [len(song)], kernel="gemm",
                                logits="all")[0]
    return lg.cpu().numpy().astype(np.float64)[:, :sum(N_CLASS)]


def test_policy_stats_of_the_blend(cuda, world):
    """alpha = 1 is policy_stats(reference=) itself; at alpha = 0 both KL columns are <= 2e-5; along alpha column 2 never
    decreases by more than the two entries' own bounds against float64, 2e-5 + 1e-5 sum p |l - l'| each
    (test_policy_stats_gpu.py).  Songs of 2, 33 and 64 rows: one row to one row past a 32-token prefill chunk."""
    w = world
    rng = np.random.default_rng(4)
    songs = [np.stack([rng.integers(0, c, n) for c in N_CLASS], 1).astype(np.int64) for n in (2, 33, 64)]
    plain = generation.policy_stats(w["net"], w["w2e"], songs, reference=w["ref"])
    one = generation.policy_stats(w["net"], w["w2e"], songs, reference=w["ref"], alpha=1)
    assert all(a.shape == (len(s) - 1, 6, 4) for a, s in zip(one, songs))
    assert all(np.array_equal(a, b) for a, b in zip(one, plain))
    zero = generation.policy_stats(w["net"], w["w2e"], songs, reference=w["ref"], alpha=0.0)
    assert max(float(np.abs(z[..., 2:]).max()) for z in zero) <= 2e-5
    alphas = (0.0, 0.25, 0.5, 0.75, 1.0)
    kl = [generation.policy_stats(w["net"], w["w2e"], songs, reference=w["ref"], alpha=a) for a in alphas]
    segs = np.concatenate([[0], np.cumsum(N_CLASS)])
    worst = -np.inf
    for k, song in enumerate(songs):
        x, r = _row_logprobs(w["net"], song, cuda)[:-1], _row_logprobs(w["ref"], song, cuda)[:-1]
        scale = np.zeros((len(alphas), len(song) - 1, 6))              # sum p |l - l'| of each entry, in float64
        for i, a in enumerate(alphas):
            b = sampling.blend_logits_f64(x, r, N_CLASS, np.full((1, 6), a, dtype=np.float32))
            for t in range(len(song) - 1):
                for at in range(6):
                    lo, hi = segs[at], segs[at + 1]
                    l = sampling.all_logprobs_f64(b[t, lo:hi])[0]
                    lr = sampling.all_logprobs_f64(r[t, lo:hi])[0]
                    scale[i, t, at] = (np.exp(l) * np.abs(l - lr)).sum()
        col = np.stack([kl[i][k][..., 2] for i in range(len(alphas))]).astype(np.float64)
        slack = (2e-5 + 1e-5 * scale[:-1]) + (2e-5 + 1e-5 * scale[1:])
        drop = col[:-1] - col[1:]
        worst = max(worst, float((drop / slack).max()))
        assert (drop <= slack).all(), (k, float((drop / slack).max()))
        assert (col[-1] > col[0] + 1e-3).any()                         # the frontier does move
    print("blend: KL(pi_alpha || pi_ref) along alpha, worst decrease / allowed = %.3g" % worst)


def test_refusals_on_the_device(world):
    w = world
    net, ref, w2e = w["net"], w["ref"], w["w2e"]
    cpu_ref = _small_model(torch.device("cpu"), 5)
    for fn in (generation.generate_batch, generation.generate_stream):
        with pytest.raises(ValueError, match="device"):
            fn(net, w2e, 2, reference=cpu_ref, alpha=0.5)
        with pytest.raises(ValueError, match="needs alpha="):
            fn(net, w2e, 2, reference=ref)
        with pytest.raises(ValueError, match="alpha must be"):
            fn(net, w2e, 2, reference=ref, alpha=[0.5, 0.5, 0.5])
    with pytest.raises(ValueError, match="generate_batch\\(prompts="):
        generation.generate_stream(net, w2e, 2, prompts=[generation.INIT_CW] * 2, reference=ref, alpha=0.5)
    songs = [np.zeros((4, 6), dtype=np.int64)] * 2
    with pytest.raises(ValueError, match="needs alpha="):
        generation.score_songs(net, w2e, songs, reference=ref)
    with pytest.raises(ValueError, match="pass reference="):
        generation.policy_stats(net, w2e, songs, alpha=0.5)
    with pytest.raises(ValueError, match="alpha must be"):
        generation.score_songs(net, w2e, songs, reference=ref, alpha=[1, 2, 3])
    with pytest.raises(ValueError, match="device"):
        generation.policy_stats(net, w2e, songs, reference=cpu_ref, alpha=0.5)
    # the kernel's own refusal reaches Python as an error, not as a copy of the reference
    lg = torch.zeros(3, sum(N_CLASS), device=net.in_linear.weight.device)
    with pytest.raises(RuntimeError, match="1001"):
        ops.blend_logits(torch.zeros_like(lg), lg, N_CLASS, torch.ones(1, 6, device=lg.device), out=lg)
    # with reference=None nothing changes: the same call, the same songs
    torch.manual_seed(SEED)
    again = generation.generate_batch(net, w2e, N_SONGS, bar_cond=BAR_COND, max_tokens=w["cap"], chunk=32,
                                      reference=None, alpha=None)
    assert _same(again, w["net", "dqn"])

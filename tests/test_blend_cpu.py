"""CPU: blending the policy with a reference model at sampling time -- cwlt_blend_logits is declared,
bound, exported and versioned and refuses bad arguments without a GPU; ops.blend_logits refuses malformed CPU tensors
before it takes a pointer; sampling.blend_logits_f64 against the product of powers it stands for; the alpha-shape
compiler; the refusals of the generation entries that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
NAME = "cwlt_blend_logits"
N_CLASS = [56, 135, 18, 87, 18, 25]
ALPHAS = (0.0, 0.25, 0.5, 0.75, 1.0, 1.5)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


# ---- the entry -------------------------------------------------------------------------------------------------------
def test_entry_declared_bound_and_exported(built):
    text = open(os.path.join(ROOT, "include", "cwlt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)
    lib = built.load()
    assert NAME in built._SIGNATURES and NAME in built.exported_names() and hasattr(lib, NAME)
    from rlmg_amd import generation, ops, sampling
    assert callable(ops.blend_logits) and callable(sampling.blend_logits_f64) and callable(generation.compile_alpha)


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 29
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_entry_refusals_without_gpu(built):
    lib = built.load()
    null, buf, other = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    nc = (ctypes.c_int * 6)(*N_CLASS)                                # 339 classes

    def call(logits=buf, ld=339, ref=other, ref_ld=339, n_class=nc, n_attr=6, alpha=buf, n_alpha=1, key=null,
             out=buf, ld_out=339, rows=4):
        return lib.cwlt_blend_logits(logits, ld, ref, ref_ld, n_class, n_attr, alpha, n_alpha, key, out, ld_out, rows,
                                     null)

    for kw in ({"logits": null}, {"ref": null}, {"alpha": null}, {"out": null}, {"n_class": None}):
        assert call(**kw) == 1001, kw
    assert call(n_attr=0) == 1001 and call(n_attr=9) == 1001
    assert call(n_class=(ctypes.c_int * 6)(56, 135, 257, 87, 18, 25), ld=1000, ref_ld=1000, ld_out=1000) == 1001
    assert call(n_class=(ctypes.c_int * 6)(56, 0, 18, 87, 18, 25)) == 1001
    assert call(ld=338) == 1001 and call(ref_ld=338) == 1001 and call(ld_out=338) == 1001
    assert call(n_alpha=0) == 1001 and call(n_alpha=-3) == 1001
    assert call(rows=0) == 1001 and call(rows=-1) == 1001 and call(rows=(1 << 20) + 1) == 1001
    assert call(out=other) == 1001                                   # out == ref_logits: the reference would be lost


def test_wrapper_refuses_malformed_cpu_tensors(built):
    """Every refusal comes before a pointer is taken: these are CPU tensors, and none of them reaches _lib.dev."""
    import torch
    from rlmg_amd import ops
    rows, W = 5, sum(N_CLASS)
    lg, al = torch.zeros(rows, W), torch.ones(1, 6)
    for bad in (lg.double(), lg[:, :W - 1], lg[0], lg.t().contiguous().t()):
        with pytest.raises(ValueError, match="logits"):
            ops.blend_logits(bad, lg, N_CLASS, al)
    for bad in (lg.double(), lg[:4], lg[:, :W - 1]):
        with pytest.raises(ValueError, match="ref_logits"):
            ops.blend_logits(lg, bad, N_CLASS, al)
    for bad in (torch.zeros(rows, W - 1), torch.zeros(rows + 1, W), torch.zeros(rows, W, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out"):
            ops.blend_logits(lg, lg, N_CLASS, al, out=bad)
    for bad in (al.double(), torch.ones(6), torch.ones(1, 5), torch.ones(6, 2).t(), torch.ones(0, 6)):
        with pytest.raises(ValueError, match="alpha"):
            ops.blend_logits(lg, lg, N_CLASS, bad)
    with pytest.raises(ValueError, match="one per row"):
        ops.blend_logits(lg, lg, N_CLASS, torch.ones(3, 6))           # without a key: 1 or `rows` alpha rows
    for bad in (torch.zeros(rows, dtype=torch.int32), torch.zeros(rows + 1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="key"):
            ops.blend_logits(lg, lg, N_CLASS, torch.ones(3, 6), key=bad)
    # well-formed CPU tensors get as far as the pointer, and no further
    with pytest.raises(RuntimeError, match="GPU"):
        ops.blend_logits(lg, lg, N_CLASS, al)


# ---- the float64 restatement -----------------------------------------------------------------------------------------
def _softmax(z):
    e = np.exp(z - z.max())
    return e / e.sum()


def _segments(n_class):
    o = np.concatenate([[0], np.cumsum(n_class)])
    return [(int(o[a]), int(o[a + 1])) for a in range(len(n_class))]


def test_blend_f64_is_the_product_of_powers(built):
    """softmax(alpha x + (1 - alpha) r) = pi^alpha pi_ref^(1 - alpha) / Z, per row and attribute, to 1e-12."""
    from rlmg_amd import sampling
    rng = np.random.default_rng(3)
    n_class = [1, 2, 7, 64, 256]
    rows, W = 9, sum(n_class)
    x, r = rng.normal(0, 3, (rows, W + 3)), rng.normal(0, 3, (rows, W + 1))
    alpha = rng.uniform(-0.7, 3.0, (rows, len(n_class))).astype(np.float32)
    alpha[0], alpha[1] = 1.0, 0.0
    out = sampling.blend_logits_f64(x, r, n_class, alpha)
    assert out.shape == (rows, W) and out.dtype == np.float64
    assert (out[0] == x[0, :W]).all() and (out[1] == r[1, :W]).all()
    for n in range(rows):
        for a, (lo, hi) in enumerate(_segments(n_class)):
            w = float(alpha[n, a])
            want = _softmax(x[n, lo:hi]) ** w * _softmax(r[n, lo:hi]) ** (1.0 - w)
            assert np.abs(_softmax(out[n, lo:hi]) - want / want.sum()).max() <= 1e-12, (n, a)
    # one shared row of alpha is every row's
    shared = sampling.blend_logits_f64(x, r, n_class, alpha[2:3])
    assert (shared[5] == sampling.blend_logits_f64(x[5:6], r[5:6], n_class, alpha[2:3])[0]).all()
    with pytest.raises(TypeError, match="float32"):
        sampling.blend_logits_f64(x, r, n_class, alpha.astype(np.float64))
    with pytest.raises(ValueError, match="alpha"):
        sampling.blend_logits_f64(x, r, n_class, alpha[:4])
    with pytest.raises(ValueError, match="logits"):
        sampling.blend_logits_f64(x[:, :W - 1], r, n_class, alpha)


def test_kl_against_the_reference_grows_with_alpha(built):
    """Along alpha in ALPHAS, KL(pi_alpha || pi_ref) from policy_stats_f64 never decreases: its derivative is alpha times
    the variance of log(pi / pi_ref) under pi_alpha."""
    from rlmg_amd import sampling
    rng = np.random.default_rng(8)
    n_class = [5, 18, 87]
    rows, W = 200, sum(n_class)
    x = rng.normal(0, 1, (rows, W)) * rng.choice([0.1, 1.0, 4.0], (rows, 1))
    r = rng.normal(0, 1, (rows, W)) * rng.choice([0.1, 1.0, 4.0], (rows, 1))
    kl = np.zeros((len(ALPHAS), rows, len(n_class)))
    for i, w in enumerate(ALPHAS):
        b = sampling.blend_logits_f64(x, r, n_class, np.full((1, len(n_class)), w, dtype=np.float32))
        for n in range(rows):
            for a, (lo, hi) in enumerate(_segments(n_class)):
                kl[i, n, a] = sampling.policy_stats_f64(b[n, lo:hi], r[n, lo:hi])[2]
    assert (kl[0] == 0).all()
    assert (np.diff(kl, axis=0) >= 0).all(), np.diff(kl, axis=0).min()


# ---- the alpha-shape compiler ----------------------------------------------------------------------------------------
def test_compile_alpha_forms_and_refusals(built):
    from rlmg_amd import generation
    ca = generation.compile_alpha
    t = ca(0.3, 5, 6)
    assert t.dtype == np.float32 and t.shape == (1, 6) and t.flags["C_CONTIGUOUS"] and (t == np.float32(0.3)).all()
    assert ca(np.float64(-2), 1, 6).tolist() == [[-2.0] * 6] and ca(7, 3, 2).tolist() == [[7.0, 7.0]]
    per_song = ca([1, 0, 0.5, 1.5, -1], 5, 6)
    assert per_song.shape == (5, 6) and (per_song == np.float32([1, 0, 0.5, 1.5, -1])[:, None]).all()
    row = ca([[0, 1, 2, 3, 4, 5]], 4, 6)
    assert row.shape == (1, 6) and row[0].tolist() == [0, 1, 2, 3, 4, 5]
    full = np.arange(24).reshape(4, 6) / 7
    assert (ca(full, 4, 6) == full.astype(np.float32)).all() and ca(full, 4, 6).dtype == np.float32
    assert ca(np.float32(full), 4, 6).shape == (4, 6)               # its own output goes through again
    # a one-dimensional alpha is per song, also when n_songs == the attribute count
    six = ca(np.arange(6.0), 6, 6)
    assert six.shape == (6, 6) and (six[:, 0] == np.arange(6)).all() and (six[3] == 3).all()
    for bad, n in (([1, 2, 3], 4), (np.ones((2, 6)), 4), (np.ones((4, 5)), 4), (np.ones((1, 1, 6)), 1),
                   (np.ones(6), 4), ([], 4)):
        with pytest.raises(ValueError, match="alpha must be"):
            ca(bad, n, 6)
    for bad in (np.nan, np.inf, [1.0, -np.inf], 1e39):               # 1e39 is finite in f64, not in the table's f32
        with pytest.raises(ValueError, match="finite"):
            ca(bad, 2, 6)
    for bad in ("half", None, [[1, 2], [3]], {"a": 1}):
        with pytest.raises(ValueError, match="alpha must be"):
            ca(bad, 2, 6)


# ---- the refusals of the generation entries that need no device ------------------------------------------------------
def _cpu_model(seed, layers=2):
    from fill import fill_params
    from rlmg_amd.dqn_policy import config, model
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": layers, "N_HEAD": 2})
    try:
        net = model.LinearTransformer(N_CLASS, is_training=False)
    finally:
        config.AgentConfig.update(old)
    return fill_params(net, seed=seed).eval()


def _w2e():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    return w2e


def test_generation_refusals_without_gpu(built, tmp_path):
    import torch
    from rlmg_amd import generation
    net, ref, w2e = _cpu_model(1), _cpu_model(2, layers=1), _w2e()
    quiet = dict(stats_path=None, log=lambda *a: None, path_gendir=str(tmp_path))
    songs = [np.zeros((3, 6), dtype=np.int64)]
    # one without the other
    for fn, args in ((generation.generate_batch, (net, w2e, 2)), (generation.generate_stream, (net, w2e, 2)),
                     (generation.score_songs, (net, w2e, songs))):
        with pytest.raises(ValueError, match="needs alpha="):
            fn(*args, reference=ref)
        with pytest.raises(ValueError, match="pass reference="):
            fn(*args, alpha=0.5)
    with pytest.raises(ValueError, match="pass reference="):
        generation.policy_stats(net, w2e, songs, alpha=0.5)
    for kw in ({"slots": 2}, {"batch_size": 2}):
        with pytest.raises(ValueError, match="needs alpha="):
            generation.generate(net, w2e, n_songs=2, reference=ref, **kw, **quiet)
        with pytest.raises(ValueError, match="pass reference="):
            generation.generate(net, w2e, n_songs=2, alpha=1.0, **kw, **quiet)
    # the one-song host paths name the device form
    with pytest.raises(ValueError, match="generate_batch\\(n_songs=1, reference"):
        generation.generate(net, w2e, n_songs=1, reference=ref, alpha=0.5, **quiet)
    # per-song prompts on the blended stream name the lock-step form
    prompts = [generation.INIT_CW, generation.INIT_CW]
    with pytest.raises(ValueError, match="generate_batch\\(prompts="):
        generation.generate_stream(net, w2e, 2, prompts=prompts, reference=ref, alpha=0.5)
    with pytest.raises(ValueError, match="generate_batch\\(prompts="):
        generation.generate(net, w2e, n_songs=2, slots=2, prompts=prompts, reference=ref, alpha=0.5, **quiet)
    # the alpha table is compiled before any device work
    for fn in (generation.generate_batch, generation.generate_stream):
        with pytest.raises(ValueError, match="alpha must be"):
            fn(net, w2e, 2, reference=ref, alpha=[1, 2, 3])
        with pytest.raises(ValueError, match="finite"):
            fn(net, w2e, 2, reference=ref, alpha=np.nan)
    # the reference meets _song_blocks' conditions
    with pytest.raises(ValueError, match="classes"):
        other = _cpu_model(3)
        other.n_token = N_CLASS[:5] + [26]
        generation.generate_batch(net, w2e, 2, reference=other, alpha=0.5)
    with pytest.raises(RuntimeError, match="reference model.*eval"):
        generation.generate_batch(net, w2e, 2, reference=_cpu_model(3).train(), alpha=0.5)
    half = _cpu_model(3)
    half.compute_dtype = torch.bfloat16
    with pytest.raises(RuntimeError, match="reference model.*f32"):
        generation.generate_stream(net, w2e, 2, reference=half, alpha=0.5)
    with pytest.raises(RuntimeError, match="f32"):                    # a bf16 model is refused as today
        generation.generate_batch(half, w2e, 2, reference=ref, alpha=0.5)

"""CPU: policy entropy and KL against a reference model -- cwlt_policy_stats is declared, bound, exported
and versioned and refuses bad arguments without a GPU; ops.policy_stats refuses malformed CPU tensors before it takes a
pointer; sampling.policy_stats_f64 against the literal definition built class by class from logprobs_f64."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cwlt_policy_stats"
N_CLASS = [56, 135, 18, 87, 18, 25]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import rlmg_amd  # noqa: F401
    from rlmg_amd import _lib
    return _lib


# ---- the entry -------------------------------------------------------------------------------------------------------
def test_entry_declared_in_header():
    text = open(os.path.join(ROOT, "include", "cwlt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)


def test_entry_bound_and_exported(built):
    lib = built.load()
    assert NAME in built._SIGNATURES and NAME in built.exported_names() and hasattr(lib, NAME)
    from rlmg_amd import generation, ops, sampling
    assert callable(ops.policy_stats) and callable(generation.policy_stats) and callable(sampling.policy_stats_f64)


def test_abi_version_moved(built):
    assert built.ABI_VERSION > 28
    assert built.load().cwlt_abi_version() == built.ABI_VERSION


def test_entry_refusals_without_gpu(built):
    lib = built.load()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    nc = (ctypes.c_int * 6)(*N_CLASS)                                # 339 classes: 11 words

    def call(logits=buf, n_class=nc, temperature=None, top_p=None, n_attr=6, rows=4, ld=339, ref=null, ref_ld=0,
             bar_class=null, key=null, bar=null, sched=null, n_sched=2, masks=null, mask_rows=3, mask_words=11,
             beat=null, order=null, n_order=18, gram=null, gram_words=11, bar_attr=2, out=buf):
        return lib.cwlt_policy_stats(logits, n_class, temperature, top_p, n_attr, rows, ld, ref, ref_ld, bar_class, key,
                                     bar, sched, n_sched, masks, mask_rows, mask_words, beat, order, n_order, gram,
                                     gram_words, bar_attr, out, null)

    for kw in ({"logits": null}, {"n_class": None}, {"out": null}):
        assert call(**kw) == 1001, kw
    assert call(rows=0) == 1001 and call(rows=(1 << 20) + 1) == 1001 and call(ld=338) == 1001
    assert call(n_attr=0) == 1001 and call(n_attr=9) == 1001
    assert call(n_class=(ctypes.c_int * 6)(56, 135, 257, 87, 18, 25), ld=1000) == 1001
    assert call(n_class=(ctypes.c_int * 6)(56, 0, 18, 87, 18, 25)) == 1001
    six = ctypes.c_float * 6
    assert call(temperature=six(1, 1, 0, 1, 1, 1)) == 1001 and call(top_p=six(1, 1, 1, 0, 1, 1)) == 1001
    # the reference logits have their own row stride
    assert call(ref=buf, ref_ld=338) == 1001 and call(ref=buf, ref_ld=0) == 1001
    # all of the constraint table or none of it
    assert call(masks=buf) == 1001 and call(bar=buf, sched=buf) == 1001 and call(sched=buf, masks=buf) == 1001
    full = dict(bar=buf, sched=buf, masks=buf)
    assert call(mask_words=10, **full) == 1001 and call(mask_words=0, **full) == 1001
    assert call(n_sched=0, **full) == 1001 and call(mask_rows=0, **full) == 1001
    # all of the grammar or none of it; a grammar needs the row's own bar-beat class
    g = dict(beat=buf, order=buf, gram=buf, bar_class=buf)
    assert call(beat=buf) == 1001 and call(order=buf, gram=buf, bar_class=buf) == 1001
    assert call(**{**g, "bar_class": null}) == 1001
    assert call(bar_attr=6, **g) == 1001 and call(bar_attr=-1, **g) == 1001
    assert call(n_order=17, **g) == 1001 and call(gram_words=10, **g) == 1001 and call(gram_words=0, **g) == 1001


def test_wrapper_refuses_malformed_cpu_tensors(built):
    """Every refusal comes before a pointer is taken: these are CPU tensors, and none of them reaches _lib.dev."""
    import torch
    from rlmg_amd import ops
    rows, W = 5, sum(N_CLASS)
    lg = torch.zeros(rows, W)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    bc = i64(rows)
    with pytest.raises(TypeError):
        ops.policy_stats(lg.double(), N_CLASS)
    with pytest.raises(ValueError, match="logits"):
        ops.policy_stats(lg[:, :W - 1], N_CLASS)
    for ref in (lg.double(), lg[:4], lg[:, :W - 1], lg[0]):
        with pytest.raises(ValueError, match="ref_logits"):
            ops.policy_stats(lg, N_CLASS, ref)
    for bad in (bc.int(), i64(rows + 1), i64(rows, 2)[:, 0]):
        with pytest.raises(ValueError, match="bar_class"):
            ops.policy_stats(lg, N_CLASS, bar_class=bad)
    sched, masks = i64(2, 2), torch.zeros(3, 11, dtype=torch.int32)
    with pytest.raises(ValueError, match="together"):
        ops.policy_stats(lg, N_CLASS, bar=bc, sched=sched)
    with pytest.raises(ValueError, match="key"):
        ops.policy_stats(lg, N_CLASS, key=bc)
    with pytest.raises(ValueError, match="words"):
        ops.policy_stats(lg, N_CLASS, bar=bc, sched=sched, masks=masks[:, :10].contiguous())
    with pytest.raises(ValueError, match="bar and key"):
        ops.policy_stats(lg, N_CLASS, bar=i64(rows + 1), sched=sched, masks=masks)
    order, gram = torch.zeros(18, dtype=torch.int32), torch.zeros(3, 11, dtype=torch.int32)
    with pytest.raises(ValueError, match="bar_class"):
        ops.policy_stats(lg, N_CLASS, grammar=(bc, order, gram, 2))
    with pytest.raises(ValueError, match="order"):
        ops.policy_stats(lg, N_CLASS, bar_class=bc, grammar=(bc, order[:17], gram, 2))
    with pytest.raises(ValueError, match="bar_attr"):
        ops.policy_stats(lg, N_CLASS, bar_class=bc, grammar=(bc, order, gram, 6))
    with pytest.raises(ValueError, match="beat"):
        ops.policy_stats(lg, N_CLASS, bar_class=bc, grammar=(i64(rows + 1), order, gram, 2))
    for out in (torch.zeros(rows, 6, 4), torch.zeros(rows, 6, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out"):
            ops.policy_stats(lg, N_CLASS, out=out)
    with pytest.raises(ValueError, match="out"):
        ops.policy_stats(lg, N_CLASS, lg, out=torch.zeros(rows, 6, 2))
    # well-formed CPU tensors get as far as the pointer, and no further
    with pytest.raises(RuntimeError, match="GPU"):
        ops.policy_stats(lg, N_CLASS)


# ---- the float64 restatement against the literal definition ----------------------------------------------------------
def _literal(x, y, t, p, allowed):
    """H and KL from the log-probs logprobs_f64 gives class by class."""
    from rlmg_amd.sampling import logprobs_f64
    n = len(x)
    lx = np.array([logprobs_f64(x, c, t, p, allowed) for c in range(n)])
    out = []
    for col in (0, 1):
        l = lx[:, col]
        k = np.isfinite(l)
        out.append(-(np.exp(l[k]) * l[k]).sum())
    if y is not None:
        ly = np.array([logprobs_f64(y, c, t, p, allowed) for c in range(n)])
        for col in (0, 1):
            l, r = lx[:, col], ly[:, col]
            k = np.isfinite(l)
            out.append(np.inf if np.isinf(r[k]).any() else (np.exp(l[k]) * (l[k] - r[k])).sum())
    return np.array(out)


@pytest.mark.parametrize("seed", range(4))
def test_restatement_matches_literal_definition(seed):
    from rlmg_amd.sampling import policy_stats_f64
    rng = np.random.default_rng(seed)
    inf = fin = 0
    for it in range(60):
        n = int(rng.choice([1, 2, 5, 18, 87, 256]))
        x = rng.normal(0, 2.5, n)
        if it % 3 == 0:
            x = np.round(x)                                          # ties
        y = x + rng.choice([0.0, 0.3, 2.5]) * rng.normal(0, 1, n)
        t = float(rng.choice([1.0, 1.2, 2.0, 5.0]))
        p = [None, 0.9, 0.99, 0.5][it % 4]
        allowed = None
        if it % 2:
            allowed = rng.random(n) < 0.7
            allowed[rng.integers(0, n)] = True
        got = policy_stats_f64(x, y, t, p, allowed)
        want = _literal(x, y, t, p, allowed)
        assert got.shape == (4,) and got.dtype == np.float64
        for g, w in zip(got, want):
            assert (np.isposinf(g) and np.isposinf(w)) or abs(g - w) <= 1e-12, (it, got, want)
        assert np.isfinite(got[:3]).all() and (got[:3] >= -1e-12).all()
        inf += np.isposinf(got[3])
        fin += np.isfinite(got[3])
        alone = policy_stats_f64(x, None, t, p, allowed)
        assert alone.shape == (2,) and np.array_equal(alone, got[:2])
    assert inf >= 3 and fin > 30                                     # both outcomes were exercised


def test_degenerate_cases():
    from rlmg_amd.sampling import policy_stats_f64
    rng = np.random.default_rng(7)
    x = rng.normal(0, 2.5, 87)
    # identical logits: both KLs are 0, whatever the settings
    for t, p in ((1.0, None), (1.2, 0.9), (2.0, 0.5)):
        got = policy_stats_f64(x, x.copy(), t, p, rng.random(87) < 0.6)
        assert got[2] == 0.0 and got[3] == 0.0
    # a one-class allowed set: H(q) = 0 and, the class being kept on both sides, KL(q || q') = 0
    one = np.zeros(87, dtype=bool)
    one[11] = True
    got = policy_stats_f64(x, x + rng.normal(0, 1, 87), 1.2, 0.9, one)
    assert got[1] == 0.0 and got[3] == 0.0 and got[0] > 0 and got[2] > 0
    # plain categorical, unmasked: q is p
    got = policy_stats_f64(x, x + rng.normal(0, 1, 87))
    assert abs(got[1] - got[0]) < 1e-12 and abs(got[3] - got[2]) < 1e-12
    # uniform logits: H = log n
    assert abs(policy_stats_f64(np.zeros(25))[0] - np.log(25)) < 1e-12
    # K not inside K': the model's nucleus keeps two classes, the reference's one
    x = np.log(np.array([0.5, 0.45, 0.05]))
    y = np.log(np.array([0.05, 0.9, 0.05]))
    got = policy_stats_f64(x, y, 1.0, 0.6)
    assert np.isposinf(got[3]) and np.isfinite(got[2]) and abs(got[1] - np.log(2)) < 0.01
    assert np.isfinite(policy_stats_f64(y, x, 1.0, 0.6)[3])          # K' = {1} is inside K = {0, 1}
    # no allowed class: the sampler entries are NaN, the model entries finite
    got = policy_stats_f64(x, y, 1.0, 0.6, np.zeros(3, dtype=bool))
    assert np.isnan(got[1]) and np.isnan(got[3]) and np.isfinite(got[0]) and np.isfinite(got[2])

"""GPU: which libcwlt entries each generation mode launches per token, in order, and how the seven sampler wrappers of
ops.py marshal their arguments.  Graphs are off, so every token goes through Python and ops._call sees every launch
(the decode step itself is called past ops._call and is not recorded)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402
from test_grammar_gpu import _constraints, _small_model, _word2event  # noqa: E402

pytestmark = pytest.mark.gpu

PRE = "cwlt_sample_categorical"
PER_TOKEN = ("cwlt_sample_", "cwlt_score_", "cwlt_count_bars", "cwlt_grammar_track", "cwlt_stream_", "cwlt_blend_logits")
N_SONGS, SLOTS, BAR_COND, MAX_TOKENS, CHUNK = 3, 2, 3, 12, 4
PROMPTS = [np.array([[0, 0, 1, 0, 0, 0]]),
           np.array([[0, 0, 1, 0, 0, 0], [1, 1, 2, 0, 0, 0], [0, 0, 0, 5, 3, 2]]),
           np.array([[0, 0, 1, 0, 0, 0], [1, 1, 2, 0, 0, 0]])]
# mode -> (constraints, log-probs, grammar)
MODES = {"plain": (False, False, False), "constraints": (True, False, False), "logprobs": (False, True, False),
         "constraints+logprobs": (True, True, False), "grammar": (False, False, True),
         "grammar+constraints+logprobs": (True, True, True)}
# the blend with a reference model, on top of the mode it names: one more launch in front of that mode's
BLEND = {"blend": "plain", "blend+grammar+constraints+logprobs": "grammar+constraints+logprobs"}
MODES.update({mode: MODES[base] for mode, base in BLEND.items()})
ALPHA = [1.0, 0.0, 0.5]                                   # one value per song
BATCH = {"plain": [PRE + "_slots"], "constraints": [PRE + "_masked", "cwlt_count_bars"], "logprobs": [PRE + "_logp"],
         "constraints+logprobs": [PRE + "_logp", "cwlt_count_bars"],
         "grammar": [PRE + "_grammar", "cwlt_grammar_track"],
         "grammar+constraints+logprobs": [PRE + "_grammar", "cwlt_count_bars", "cwlt_grammar_track"]}
STREAM = {"plain": [PRE + "_keyed"], "constraints": [PRE + "_masked"], "logprobs": [PRE + "_logp"],
          "constraints+logprobs": [PRE + "_logp"], "grammar": [PRE + "_grammar"],
          "grammar+constraints+logprobs": [PRE + "_grammar"]}
for _mode, _base in BLEND.items():
    BATCH[_mode] = ["cwlt_blend_logits"] + BATCH[_base]
    STREAM[_mode] = STREAM[_base]


@pytest.fixture(scope="module")
def net(cuda):
    return _small_model(cuda)


@pytest.fixture(scope="module")
def ref(cuda):
    """A second small model, of another depth and fill: the blend's reference."""
    from test_blend_gpu import _small_model as other
    return other(cuda, 5, layers=1)


@pytest.fixture
def calls(monkeypatch):
    """Every ops._call of the test as (entry name, arguments), the call itself forwarded unchanged; graphs off."""
    seen, real = [], ops._call

    def recording(name, *args, **kw):
        seen.append((name, args))
        return real(name, *args, **kw)

    monkeypatch.setattr(ops, "GRAPHS_ENABLED", False)
    monkeypatch.setattr(ops, "_call", recording)
    return seen


def _mode_kw(mode, w2e, ref):
    cons, lp, gram = MODES[mode]
    musical, beats = _constraints(w2e)
    blend = dict(reference=ref, alpha=ALPHA) if mode in BLEND else {}
    return dict(constraints=[musical, beats, None] if cons else None, return_logprobs=lp,
                grammar=generation.Grammar(w2e) if gram else None, **blend)


def _per_token(calls):
    return [name for name, _ in calls if name.startswith(PER_TOKEN)]


def _check(seen, pattern, tokens):
    assert PRE not in seen                                    # the plain entry: never from generation.py
    assert len(seen) == len(pattern) * tokens and seen == pattern * tokens, (pattern, tokens, seen)


@pytest.mark.parametrize("prompted", [False, True], ids=["scratch", "prompts"])
@pytest.mark.parametrize("mode", list(MODES))
def test_generate_batch_entries(net, ref, calls, mode, prompted):
    w2e = _word2event()
    kw = _mode_kw(mode, w2e, ref)
    torch.manual_seed(7)
    out = generation.generate_batch(net, w2e, N_SONGS, bar_cond=BAR_COND, max_tokens=MAX_TOKENS, chunk=CHUNK,
                                    prompts=PROMPTS if prompted else None, prefill="gemm", **kw)
    songs = out[0] if kw["return_logprobs"] else out
    heads = PROMPTS if prompted else [generation.INIT_CW] * N_SONGS
    drawn = max(len(s) - len(h) for s, h in zip(songs, heads))
    seen = _per_token(calls)
    tokens = len(seen) // len(BATCH[mode])
    assert drawn >= 1 and drawn <= tokens <= min(MAX_TOKENS - 1, -(-drawn // CHUNK) * CHUNK)
    _check(seen, BATCH[mode], tokens)


# the blended stream starts every song from one snapshot: it refuses per-song prompts, so those cases do not exist
@pytest.mark.parametrize("mode,prompted", [pytest.param(m, p, id="%s-%s" % (m, "prompts" if p else "shared"))
                                           for p in (False, True) for m in MODES if not (p and m in BLEND)])
def test_generate_stream_entries(net, ref, calls, mode, prompted):
    w2e = _word2event()
    kw = _mode_kw(mode, w2e, ref)
    start = dict(prompts=PROMPTS) if prompted else dict(prompt=PROMPTS[1])
    torch.manual_seed(7)
    _, stats = generation._generate_stream(net, w2e, N_SONGS, slots=SLOTS, bar_cond=BAR_COND, max_tokens=MAX_TOKENS,
                                           chunk=CHUNK, **start, **kw)
    assert not stats["graph"] and stats["steps"] >= 2 * CHUNK
    bank = "_bank" if prompted else ""
    # under a blend the reference's pool is refilled right after the model's, then the logits are blended
    blend = ["cwlt_stream_refill", "cwlt_blend_logits"] if mode in BLEND else []
    pattern = ["cwlt_stream_refill" + bank] + blend + STREAM[mode] + ["cwlt_stream_advance" + bank] + \
        (["cwlt_grammar_track"] if MODES[mode][2] else [])
    seen = _per_token(calls)
    assert "cwlt_count_bars" not in seen
    _check(seen, pattern, stats["steps"])


def test_one_song_loops_use_the_slot_keyed_entry(net, calls):
    w2e = _word2event()
    torch.manual_seed(7)
    generation.categorical_rollout(net, 4, carry_memory=True)
    generation.categorical_rollout(net, 4, carry_memory=True, prompt=PROMPTS[1])
    generation.inference_from_scratch(net, w2e, BAR_COND, max_tokens=6, device_sampling=True, chunk=CHUNK)
    generation.inference_from_prompt(net, w2e, PROMPTS[1], BAR_COND, max_tokens=8, device_sampling=True, chunk=CHUNK)
    seen = _per_token(calls)
    assert len(seen) >= 8 + 2 and set(seen) == {PRE + "_slots"}


# ---- the wrappers' marshalling ---------------------------------------------------------------------------------------
N_CLASS = [3, 4, 5, 6, 7, 8]
A, ROWS, WIDTH = len(N_CLASS), 2, sum(N_CLASS)
ANY = object()                                            # an argument not compared (the stream)


def _wrapper_tensors(cuda):
    gen = torch.Generator(device=cuda).manual_seed(1)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=cuda)
    return {"logits": torch.randn(ROWS, WIDTH, device=cuda, generator=gen),
            "tokens": torch.full((ROWS, A), -1, dtype=torch.int64, device=cuda),
            "targets": i64([[1, 2, 1, 4, 5, 6], [0, 3, 2, 0, 1, 7]]), "counter": i64([3]), "key": i64([5, 2]),
            "step": i64([0, 9]), "bar": i64([1, 2]), "sched": i64([[0, 1], [0, 1], [0, 0]]),
            "masks": torch.full((1, 2), -1, dtype=torch.int32, device=cuda),
            "song": torch.zeros((4, ROWS, A), dtype=torch.int64, device=cuda),
            "logp": torch.zeros((2, ROWS, A, 2), dtype=torch.float32, device=cuda),
            "out": torch.zeros((ROWS, A, 2), dtype=torch.float32, device=cuda), "beat": i64([-1, 0]),
            "order": torch.tensor([-2, -1, 0, 1, 2], dtype=torch.int32, device=cuda),
            "gram": torch.full((3, 2), -1, dtype=torch.int32, device=cuda)}


TEMP, TOP_P = [1.5, 1.0, 0.5, 1.0, 2.0, 1.0], [0.9, None, 1.0, 0.5, None, 0.99]
HEAD = ["logits", N_CLASS, TEMP, [1.0 if p is None else p for p in TOP_P], A, ROWS, WIDTH]
SEED = (-3) & 0xFFFFFFFFFFFFFFFF
NO_TABLE = [None, None, 0, None, 0, 0]
TABLE = ["bar", "sched", 3, "masks", 1, 2]
GTABLE = ["beat", "order", 5, "gram", 2, 2]
# wrapper -> (call, entry, expected arguments: a string is that tensor's pointer, None is NULL)
WRAPPER_CALLS = {
    "sample_categorical": (
        lambda t: ops.sample_categorical(t["logits"], N_CLASS, t["tokens"], -3, counter=t["counter"], song=t["song"],
                                         temperature=TEMP, top_p=TOP_P),
        PRE, HEAD + [SEED, "counter", "tokens", "song", 4, ANY]),
    "sample_categorical(slot_keys)": (
        lambda t: ops.sample_categorical(t["logits"], N_CLASS, t["tokens"], -3, temperature=TEMP, top_p=TOP_P,
                                         slot_keys=True),
        PRE + "_slots", HEAD + [SEED, None, "tokens", None, 0, ANY]),
    "sample_categorical_keyed": (
        lambda t: ops.sample_categorical_keyed(t["logits"], N_CLASS, t["tokens"], -3, t["key"], t["step"],
                                               temperature=TEMP, top_p=TOP_P),
        PRE + "_keyed", HEAD + [SEED, "key", "step", "tokens", ANY]),
    "sample_categorical_masked": (
        lambda t: ops.sample_categorical_masked(t["logits"], N_CLASS, t["tokens"], -3, t["bar"], t["sched"],
                                                t["masks"], key=t["key"], step=t["step"], temperature=TEMP,
                                                top_p=TOP_P),
        PRE + "_masked", HEAD + [SEED, None, "key", "step"] + TABLE + ["tokens", ANY]),
    "sample_categorical_logp": (
        lambda t: ops.sample_categorical_logp(t["logits"], N_CLASS, t["tokens"], -3, t["logp"], counter=t["counter"],
                                              out_counter=t["counter"], temperature=TEMP, top_p=TOP_P),
        PRE + "_logp", HEAD + [SEED, "counter", None, None] + NO_TABLE + ["tokens", "logp", "counter", 2, ANY]),
    "sample_categorical_grammar": (
        lambda t: ops.sample_categorical_grammar(t["logits"], N_CLASS, t["tokens"], -3, t["beat"], t["order"],
                                                 t["gram"], key=t["key"], step=t["step"], bar=t["bar"],
                                                 sched=t["sched"], masks=t["masks"], temperature=TEMP, top_p=TOP_P),
        PRE + "_grammar", HEAD + [SEED, None, "key", "step"] + TABLE + GTABLE + ["tokens", None, None, 1, ANY]),
    "sample_categorical_grammar(logp)": (
        lambda t: ops.sample_categorical_grammar(t["logits"], N_CLASS, t["tokens"], -3, t["beat"], t["order"],
                                                 t["gram"], 2, counter=t["counter"], logp=t["logp"],
                                                 out_counter=t["counter"], temperature=TEMP, top_p=TOP_P),
        PRE + "_grammar", HEAD + [SEED, "counter", None, None] + NO_TABLE + GTABLE +
        ["tokens", "logp", "counter", 2, ANY]),
    "score_categorical": (
        lambda t: ops.score_categorical(t["logits"], N_CLASS, t["targets"], temperature=TEMP, top_p=TOP_P,
                                        out=t["out"]),
        "cwlt_score_categorical", HEAD + ["targets", None] + NO_TABLE + ["out", ANY]),
    "score_categorical(masked)": (
        lambda t: ops.score_categorical(t["logits"], N_CLASS, t["targets"], temperature=TEMP, top_p=TOP_P,
                                        key=t["key"], bar=t["bar"], sched=t["sched"], masks=t["masks"], out=t["out"]),
        "cwlt_score_categorical", HEAD + ["targets", "key"] + TABLE + ["out", ANY]),
    "score_categorical_grammar": (
        lambda t: ops.score_categorical_grammar(t["logits"], N_CLASS, t["targets"], t["beat"], t["order"], t["gram"],
                                                temperature=TEMP, top_p=TOP_P, key=t["key"], bar=t["bar"],
                                                sched=t["sched"], masks=t["masks"], out=t["out"]),
        "cwlt_score_categorical_grammar", HEAD + ["targets", "key"] + TABLE + GTABLE + ["out", ANY]),
}


@pytest.mark.parametrize("case", list(WRAPPER_CALLS))
def test_wrapper_marshalling(cuda, calls, case):
    call, entry, want = WRAPPER_CALLS[case]
    t = _wrapper_tensors(cuda)
    res = call(t)
    torch.cuda.synchronize()
    assert res is (t["out"] if case.startswith("score") else t["tokens"])
    assert len(calls) == 1
    name, args = calls[0]
    assert name == entry and len(args) == len(want), (name, len(args), len(want))
    for i, (got, exp) in enumerate(zip(args, want)):
        if exp is ANY:
            assert isinstance(got, ctypes.c_void_p), i
        elif exp is None:
            assert got is None, (i, got)
        elif isinstance(exp, str):
            assert isinstance(got, ctypes.c_void_p) and got.value == t[exp].data_ptr(), (i, exp)
        elif isinstance(exp, list):
            assert len(got) == len(exp) and [float(np.float32(v)) for v in exp] == list(got), (i, list(got))
        else:
            assert not isinstance(got, ctypes.c_void_p) and got == exp, (i, got, exp)
    if case.startswith("sample"):                             # the launch ran: every id was written, in range
        ids = t["tokens"].cpu().numpy()
        assert ((ids >= 0) & (ids < np.asarray(N_CLASS))).all()

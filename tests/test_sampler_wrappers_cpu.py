"""CPU: the refusals of the seven sampler wrappers of ops.py (sample_categorical, _keyed, _masked, _logp, _grammar,
score_categorical, score_categorical_grammar).  Every probe is made of CPU tensors and must be refused by the wrapper's
own checks -- the exception type, and a message that names the offending argument -- before any pointer is taken: a
call whose arguments are all well-formed gets as far as the marshalling, which refuses CPU tensors."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import rlmg_amd  # noqa: E402,F401
from rlmg_amd import ops  # noqa: E402

N_CLASS = [3, 4, 5, 6, 7, 8]
A, ROWS, WIDTH = len(N_CLASS), 2, sum(N_CLASS)            # 33 classes: a mask row needs two 32-bit words
I64 = torch.int64


def _good():
    """Well-formed CPU arguments of every kind the wrappers take."""
    return {"logits": torch.zeros(ROWS, WIDTH), "tokens": torch.zeros(ROWS, A, dtype=I64),
            "counter": torch.zeros(1, dtype=I64), "key": torch.zeros(ROWS, dtype=I64),
            "step": torch.zeros(ROWS, dtype=I64), "bar": torch.ones(ROWS, dtype=I64),
            "sched": torch.zeros(ROWS, 2, dtype=I64), "masks": torch.zeros(1, 2, dtype=torch.int32),
            "logp": torch.zeros(1, ROWS, A, 2), "beat": torch.zeros(ROWS, dtype=I64),
            "order": torch.zeros(N_CLASS[2], dtype=torch.int32), "gram": torch.zeros(3, 2, dtype=torch.int32)}


TABLE = ("bar", "sched", "masks")
# wrapper -> (positional arguments after logits and n_class, keyword arguments of a keyed / counted call)
WRAPPERS = {
    "sample_categorical": (("tokens", 7), {"counter": "counter"}),
    "sample_categorical_keyed": (("tokens", 7, "key", "step"), {}),
    "sample_categorical_masked": (("tokens", 7, "bar", "sched", "masks"), {"counter": "counter"}),
    "sample_categorical_logp": (("tokens", 7, "logp"), {"counter": "counter"}),
    "sample_categorical_grammar": (("tokens", 7, "beat", "order", "gram"), {"counter": "counter"}),
    "score_categorical": (("tokens",), {}),
    "score_categorical_grammar": (("tokens", "beat", "order", "gram"), {}),
}
SAMPLERS = [w for w in WRAPPERS if w.startswith("sample")]
SCORERS = [w for w in WRAPPERS if w.startswith("score")]
KEYED = ["sample_categorical_masked", "sample_categorical_logp", "sample_categorical_grammar"]   # key= / step= / counter=
TABLED = ["sample_categorical_logp", "sample_categorical_grammar"] + SCORERS                   # optional bar / sched / masks
RINGED = ["sample_categorical_logp", "sample_categorical_grammar"]
GRAMMAR = ["sample_categorical_grammar", "score_categorical_grammar"]


def _call(name, change=None, **kw):
    """Call wrapper `name` with the well-formed arguments, `change` ({argument: value}) replacing some of them, and the
    keyword arguments kw (a string names a well-formed argument; given keywords replace the wrapper's defaults of
    WRAPPERS)."""
    good = _good()
    good.update(change or {})
    pos, kws = WRAPPERS[name]
    kws = dict(kws)
    if any(k in kw for k in ("key", "counter")):
        kws.pop("counter", None)
    kws.update(kw)
    pick = lambda v: good[v] if isinstance(v, str) else v
    return getattr(ops, name)(good["logits"], N_CLASS, *[pick(v) for v in pos], **{k: pick(v) for k, v in kws.items()})


def _refused(exc, words, name, change=None, **kw):
    with pytest.raises(exc) as e:
        _call(name, change, **kw)
    assert type(e.value) is exc, (name, type(e.value))
    msg = str(e.value)
    for w in words:
        assert w in msg, (name, w, msg)


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_well_formed_arguments_reach_the_marshalling(name):
    _refused(RuntimeError, ["must be a GPU tensor"], name)


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_f64_logits(name):
    _refused(TypeError, [name + " takes", "logits"], name, {"logits": torch.zeros(ROWS, WIDTH, dtype=torch.float64)})


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_int32_tokens(name):
    _refused(TypeError, [name + " takes", "int64"], name, {"tokens": torch.zeros(ROWS, A, dtype=torch.int32)})


@pytest.mark.parametrize("name", list(WRAPPERS))
@pytest.mark.parametrize("bad", ["size", "strided"])
def test_tokens_buffer(name, bad):
    t = torch.zeros(ROWS + 1, A, dtype=I64) if bad == "size" else torch.zeros(ROWS, 2 * A, dtype=I64)[:, ::2]
    assert bad == "size" or (t.numel() == ROWS * A and not t.is_contiguous())
    _refused(ValueError, ["targets" if name in SCORERS else "tokens", "contiguous"], name, {"tokens": t})


@pytest.mark.parametrize("name", ["sample_categorical_keyed"] + KEYED)
@pytest.mark.parametrize("which", ["key", "step"])
def test_key_and_step_length(name, which):
    kw = {} if name == "sample_categorical_keyed" else {"key": "key", "step": "step"}
    _refused(ValueError, ["key", "step"], name, {which: torch.zeros(ROWS + 1, dtype=I64)}, **kw)


@pytest.mark.parametrize("name", ["sample_categorical_keyed"] + KEYED)
def test_key_dtype(name):
    kw = {} if name == "sample_categorical_keyed" else {"key": "key", "step": "step"}
    _refused(ValueError, ["key", "int64"], name, {"key": torch.zeros(ROWS, dtype=torch.int32)}, **kw)


@pytest.mark.parametrize("name", KEYED)
def test_key_without_step(name):
    _refused(ValueError, [name, "key and step"], name, key="key")
    _refused(ValueError, [name, "key and step"], name, key=None, step="step")


@pytest.mark.parametrize("name", KEYED)
def test_neither_key_nor_counter(name):
    _refused(ValueError, [name, "key and step", "counter"], name, counter=None)


@pytest.mark.parametrize("name", ["sample_categorical_masked"] + TABLED)
def test_masks_with_too_few_bits(name):
    kw = {} if name == "sample_categorical_masked" else {k: k for k in TABLE}
    _refused(ValueError, ["masks", "1 words", "%d classes" % WIDTH], name,
             {"masks": torch.zeros(1, 1, dtype=torch.int32)}, **kw)


@pytest.mark.parametrize("name", ["sample_categorical_masked"] + TABLED)
def test_constraint_table_shapes(name):
    kw = {} if name == "sample_categorical_masked" else {k: k for k in TABLE}
    _refused(ValueError, ["bar", "int64"], name, {"bar": torch.ones(ROWS + 1, dtype=I64)}, **kw)
    _refused(ValueError, ["sched", "(n_songs, 2)"], name, {"sched": torch.zeros(ROWS, 3, dtype=I64)}, **kw)
    _refused(ValueError, ["masks", "32-bit"], name, {"masks": torch.zeros(1, 2, dtype=I64)}, **kw)


@pytest.mark.parametrize("name", TABLED)
@pytest.mark.parametrize("given", [("bar",), ("sched",), ("masks",), ("bar", "sched"), ("bar", "masks"),
                                   ("sched", "masks")])
def test_constraint_table_given_in_part(name, given):
    _refused(ValueError, ["bar, sched and masks together"], name, **{k: k for k in given})


@pytest.mark.parametrize("name", RINGED)
def test_logp_ring(name):
    kw = {"logp": "logp"} if name == "sample_categorical_grammar" else {}
    for bad in (torch.zeros(1, ROWS, A, 3), torch.zeros(1, ROWS + 1, A, 2), torch.zeros(ROWS, A, 2),
                torch.zeros(1, ROWS, A, 2, dtype=torch.float64), torch.zeros(1, ROWS, A, 4)[..., ::2]):
        _refused(ValueError, ["logp", "(R, %d, %d, 2) f32 ring" % (ROWS, A)], name, {"logp": bad}, **kw)
    _refused(ValueError, ["logp ring of 2 rows", "out_counter"], name, {"logp": torch.zeros(2, ROWS, A, 2)}, **kw)


@pytest.mark.parametrize("name", GRAMMAR)
def test_grammar_tables(name):
    _refused(ValueError, ["order", ">= %d entries" % N_CLASS[2]], name,
             {"order": torch.zeros(N_CLASS[2] - 1, dtype=torch.int32)})
    _refused(ValueError, ["order", "int32"], name, {"order": torch.zeros(N_CLASS[2], dtype=I64)})
    _refused(ValueError, ["order", ">= %d entries" % N_CLASS[5]], name, bar_attr=5)      # 5 entries for 8 classes
    for bar_attr in (-1, A):
        _refused(ValueError, ["bar_attr %d" % bar_attr, "%d attributes" % A], name, bar_attr=bar_attr)
    _refused(ValueError, ["gram", "1 words", "%d classes" % WIDTH], name,
             {"gram": torch.zeros(3, 1, dtype=torch.int32)})
    _refused(ValueError, ["gram", "(3, words)"], name, {"gram": torch.zeros(2, 2, dtype=torch.int32)})
    _refused(ValueError, ["beat", "int64"], name, {"beat": torch.zeros(ROWS + 1, dtype=I64)})


@pytest.mark.parametrize("name", SCORERS)
def test_scorer_key_needs_a_mask_table(name):
    _refused(ValueError, ["key", "bar, sched and masks"], name, key="key")


@pytest.mark.parametrize("name", SCORERS)
def test_scorer_key_length(name):
    kw = {k: k for k in TABLE}
    _refused(ValueError, ["key", "int64"], name, {"key": torch.zeros(ROWS + 1, dtype=I64)}, key="key", **kw)


def test_scorer_out():
    for bad in (torch.zeros(ROWS, A, 3), torch.zeros(ROWS, A, 2, dtype=torch.float64)):
        _refused(ValueError, ["out", "(%d, %d, 2) f32" % (ROWS, A)], "score_categorical", out=bad)

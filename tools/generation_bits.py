#!/usr/bin/env python3
"""Bits of the public generation entries on fixed inputs, to hold two trees to each other.

    python tools/generation_bits.py dump OUT.npz          (needs the GPU)
    python tools/generation_bits.py compare A.npz B.npz   (exit 0 when both hold the same arrays, bit for bit)

`dump` drives generate_batch (from scratch, three ragged prompts), generate_stream (no prompt, one shared prompt,
per-song prompts), generate (batch_size=2 and slots=2, so a group boundary cuts the per-song arguments), score_songs and
policy_stats (with and without a reference) under the modes each accepts: plain, list constraints with a None entry,
log-probs, grammar, grammar + constraints + log-probs, and the blend with a reference model (scalar alpha, a per-song
(3, 6) alpha, and on top of grammar + constraints + log-probs), with both samplers where the entry takes one.  Only
public names of `generation` are used, after a fixed torch.manual_seed per case, so the same file runs in an export of
another commit with that commit's own build.  The model is the small model of tests/test_grammar_gpu.py, the reference
a second one of another depth; 3 songs, 2 slots, bar_cond 3, max_tokens 12, chunk 4.  Songs are stored as they are,
log-probs and stats as uint32 bit patterns, so that -inf and +inf compare."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
N_SONGS, SLOTS, BAR_COND, MAX_TOKENS, CHUNK, SEED = 3, 2, 3, 12, 4, 7
PROMPTS = [np.array([[0, 0, 1, 0, 0, 0]]),
           np.array([[0, 0, 1, 0, 0, 0], [1, 1, 2, 0, 0, 0], [0, 0, 0, 5, 3, 2]]),
           np.array([[0, 0, 1, 0, 0, 0], [1, 1, 2, 0, 0, 0]])]
ALPHA = np.array([[1.0, 0.0, 0.5, 1.5, -0.5, 0.25], [0.0, 1.0, 2.0, 0.75, 0.5, 1.0], [0.3, 0.3, 1.0, 0.0, 1.25, -1.0]])
# mode -> (constraints, log-probs, grammar, alpha)
MODES = {"plain": (False, False, False, None), "constraints": (True, False, False, None),
         "logprobs": (False, True, False, None), "grammar": (False, False, True, None),
         "grammar+constraints+logprobs": (True, True, True, None), "blend": (False, False, False, 0.5),
         "blend_per_song": (False, False, False, ALPHA), "blend+grammar+constraints+logprobs": (True, True, True, ALPHA)}


def _world(dev):
    """(model, reference, word2event): the vocabulary and small model of tests/test_grammar_gpu.py, a one-layer
    reference from another fill."""
    from fill import fill_params
    from rlmg_amd.dqn_policy import config, model
    fix = np.load(os.path.join(ROOT, "tests", "golden", "dqn_generation_small.npz"))
    n_class = [int(v) for v in fix["n_class"]]
    names = {"tempo": "Tempo_%d", "chord": "chord_%d", "pitch": "Note_Pitch_%d", "duration": "Note_Duration_%d",
             "velocity": "Note_Velocity_%d"}
    w2e = {k: {i: names.get(k, "%d") % i for i in range(n)} for k, n in zip(KEYS, n_class)}
    for k in KEYS:
        w2e[k][0] = 0
    w2e["tempo"][1] = w2e["chord"][1] = "CONTI"
    w2e["bar-beat"] = {0: 0, 1: "Bar", **{2 + k: "Beat_%d" % k for k in range(16)}}

    def net(seed, layers):
        old = dict(config.AgentConfig)
        config.AgentConfig.update({"D_MODEL": 128, "N_LAYER": layers, "N_HEAD": 2})
        try:
            m = model.LinearTransformer(n_class, is_training=False)
        finally:
            config.AgentConfig.update(old)
        return fill_params(m, seed=seed).to(dev).eval()

    return net(int(fix["fill_seed"]), 2), net(int(fix["fill_seed"]) + 2, 1), w2e


def _mode_kw(generation, mode, w2e, ref):
    cons, lp, gram, alpha = MODES[mode]
    kw = {}
    if cons:
        musical = generation.Constraint(w2e, allow={"tempo": ["Tempo_3"], "pitch": range(5, 12)},
                                        per_bar={"chord": [["chord_2"], ["chord_5", "chord_6"], [7], ["chord_4"]]},
                                        cycle=True)
        beats = generation.Constraint(w2e, per_bar={"bar-beat": [["Bar", "Beat_0", "Beat_4", "Beat_8", "Beat_12"],
                                                                 ["Bar", "Beat_0", "Beat_6", 9]],
                                                    "velocity": [[2], [3, 4], [5]]})
        kw["constraints"] = [musical, beats, None]
    if gram:
        kw["grammar"] = generation.Grammar(w2e)
    if alpha is not None:
        kw.update(reference=ref, alpha=alpha)
    return kw, lp


def dump(path):
    import torch
    import rlmg_amd  # noqa: F401
    from rlmg_amd import generation
    dev = torch.device("cuda:0")
    net, ref, w2e = _world(dev)
    out = {}
    bits = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)

    def put(tag, res, lp):
        songs, lps = res if lp else (res, None)
        for i, s in enumerate(songs):
            out["%s/song%d" % (tag, i)] = np.asarray(s)
            if lp:
                out["%s/logp%d:bits" % (tag, i)] = bits(lps[i])

    shape = dict(bar_cond=BAR_COND, max_tokens=MAX_TOKENS)
    given = None
    for mode in MODES:
        blended = MODES[mode][3] is not None
        for sampler in ("dqn", "categorical"):
            kw, lp = _mode_kw(generation, mode, w2e, ref)
            for name, start in (("batch_scratch", {}), ("batch_prompts", dict(prompts=PROMPTS))):
                torch.manual_seed(SEED)
                put("%s/%s/%s" % (name, mode, sampler),
                    generation.generate_batch(net, w2e, N_SONGS, chunk=CHUNK, prefill="gemm", sampler=sampler,
                                              return_logprobs=lp, **start, **shape, **kw), lp)
            if given is None:
                given = [out["batch_prompts/plain/dqn/song%d" % i] for i in range(N_SONGS)]
            for name, start in (("stream_scratch", {}), ("stream_shared", dict(prompt=PROMPTS[1])),
                                ("stream_prompts", dict(prompts=PROMPTS))):
                if blended and "prompts" in start:
                    continue                                   # refused: the blended stream starts from one snapshot
                torch.manual_seed(SEED)
                put("%s/%s/%s" % (name, mode, sampler),
                    generation.generate_stream(net, w2e, N_SONGS, slots=SLOTS, chunk=CHUNK, sampler=sampler,
                                               return_logprobs=lp, **start, **shape, **kw), lp)
            if not lp or MODES[mode][0]:                       # the scorers take no log-prob flag: its own mode is plain
                torch.manual_seed(SEED)
                for i, s in enumerate(generation.score_songs(net, w2e, given, sampler=sampler, **kw)):
                    out["score_songs/%s/%s/%d:bits" % (mode, sampler, i)] = bits(s)
                for rname, r in (("single", None), ("pair", ref)):
                    if blended and r is None:
                        continue
                    torch.manual_seed(SEED)
                    st = generation.policy_stats(net, w2e, given, sampler=sampler, **dict(kw, reference=r))
                    for i, s in enumerate(st):
                        out["policy_stats_%s/%s/%s/%d:bits" % (rname, mode, sampler, i)] = bits(s)
        for how in ("batch_size", "slots"):
            for pname, pr in (("scratch", {}), ("prompts", dict(prompts=PROMPTS))):
                if how == "slots" and blended and pr:
                    continue
                kw, lp = _mode_kw(generation, mode, w2e, ref)
                with tempfile.TemporaryDirectory() as d:
                    torch.manual_seed(SEED)
                    generation.generate(net, w2e, n_songs=N_SONGS, path_gendir=d, stats_path=None,
                                        log=lambda *a: None, logprobs=lp, **{how: 2}, **pr, **shape, **kw)
                    songs = [np.load(os.path.join(d, "get_%d.npy" % i)) for i in range(N_SONGS)]
                    lps = [np.load(os.path.join(d, "get_%d_logp.npy" % i)) for i in range(N_SONGS)] if lp else None
                put("generate_%s_%s/%s" % (how, pname, mode), (songs, lps) if lp else songs, lp)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print("%s: %d arrays" % (path, len(out)))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("only in one file  %s" % k)
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
        if not same:
            print("DIFFERENT %s %s" % (k, a[k].shape))
            bad.append(k)
    print("%d arrays, %d differ" % (len(set(a.files) | set(b.files)), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)

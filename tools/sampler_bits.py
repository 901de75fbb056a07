#!/usr/bin/env python3
"""Bits of the device sampler, the scorers and cwlt_policy_stats on fixed inputs, to hold two builds to each other.

    python tools/sampler_bits.py dump OUT.npz          (needs the GPU; drives the C entries of this tree through ops)
    python tools/sampler_bits.py compare A.npz B.npz   (exit 0 when both hold the same arrays, bit for bit)
    python tools/sampler_bits.py time OUT.json         (needs the GPU; us per launch of each form at 256 rows)
    python tools/sampler_bits.py table DIR             (the series DIR/time_parent_<i>.json against DIR/time_new_<i>.json)

`dump` runs all 12 instantiations of sample_categorical_kernel (plain, slots, keyed, masked, logp and score with and
without a mask table, grammar with and without mask and logp, score_grammar with and without mask) and the 8 forms of
cwlt_policy_stats (mask x grammar x reference logits), each on two attribute tables and two sampler settings, 64 rows.
Tokens are stored as they are, log-prob pairs and stats as uint32 bit patterns, so NaN and +-inf compare too.  Outputs
are pre-filled, so an entry a kernel leaves unwritten (padding rows) compares as well.  The rows reach every branch of
the support rule: song keys < 0 and outside the schedule, schedules of length 0, bars past a schedule's end, forced
targets that are padding, outside their attribute, or whose bar-beat class is ill-formed, and a 1-class attribute that
a BEAT row leaves with no allowed class.

`time` measures one launch of every grammar or masked sampler / scorer form and of the 8 stats forms at 256 rows (the
stream's slot count) on the golden dictionary with the DQN settings: HIP events around the launch, 30 warm-up launches,
the median of 300.  To hold two trees to each other, put a copy of this file into an export of the other commit (with
its own build), run `time` as a fresh process per tree, alternating, five times each in one job, and read the result
with `table`: a form passes when the new median is not above the parent's median by more than the parent's own spread,
(max - min) / median over its five runs.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = 64
KEYS = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]


def _tables():
    """name -> (word2event, DQN-style (temperature, top_p)): the golden dictionary's class counts, and 8 attributes with
    a 256-class one, a 1-class one and one whose count is no multiple of 4."""
    from rlmg_amd import generation
    fix = np.load(os.path.join(ROOT, "tests", "golden", "dqn_generation_small.npz"))
    small = dict(zip(KEYS, [int(v) for v in fix["n_class"]]))
    wide = {"tempo": 256, "chord": 1, "bar-beat": small["bar-beat"], "pitch": 87, "duration": 18, "velocity": 25,
            "extra": 5, "more": 64}
    out = {}
    for name, counts, temp, top_p in (
            ("golden6", small, generation.DQN_TEMPERATURE, generation.DQN_TOP_P),
            ("wide8", wide, generation.DQN_TEMPERATURE + (1.0, 0.7), generation.DQN_TOP_P + (None, 0.95))):
        w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in counts.items()}
        w2e["bar-beat"] = {0: 0, 1: "Bar", **{2 + k: "Beat_%d" % k for k in range(counts["bar-beat"] - 2)}}
        out[name] = (w2e, (temp, top_p))
    return out


def _inputs(w2e, seed, dev):
    """The fixed inputs of one attribute table, as device tensors."""
    import torch
    from rlmg_amd import generation
    n_class = [len(v) for v in w2e.values()]
    A, width = len(n_class), sum(n_class)
    off = np.concatenate([[0], np.cumsum(n_class)])
    W = -(-width // 32)
    rng = np.random.default_rng(seed)
    t = lambda x, dt=np.int64: torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)
    padded = lambda: t(3 * rng.standard_normal((ROWS, width + 5)), np.float32)[:, :width]    # row stride != width
    g = generation.Grammar(w2e)
    order, gram = g.tables()
    order[-1] = -3                                   # the last Beat class: never allowed, an ill-formed row's kind
    key = rng.permutation(ROWS)                      # songs 48 .. 63 lie outside the 48-song schedule
    key[::9], key[4::11] = -1, -2                    # idle and waiting stream slots
    bits = rng.random((7, W * 32)) < 0.6             # 7 mask rows, every attribute non-empty
    for r in range(7):
        for a in range(A):
            bits[r, off[a] + rng.integers(0, n_class[a])] = True
    masks = np.packbits(bits, axis=1, bitorder="little").view("<u4").reshape(7, W).view(np.int32)
    sched = np.stack([rng.integers(0, 5, 48), rng.integers(0, 3, 48)], 1)    # lengths 0: unmasked; first + len <= 7
    targets = np.stack([rng.integers(0, c, ROWS) for c in n_class], 1)
    targets[5::13] = -1                              # padding rows
    targets[7::17, 3] = n_class[3]                   # a class outside its attribute
    targets[2::19, 0] = 1 << 40
    targets[3::8, 2] = n_class[2] - 1                # the ill-formed bar-beat class
    bar_class = targets[:, 2].copy()
    bar_class[9::21] = n_class[2] + 3                # outside bar-beat: no kind
    return dict(n_class=n_class, A=A, logits=padded(), ref=padded(), key=t(key), step=t(rng.integers(0, 5000, ROWS)),
                counter=t([123]), out_counter=t([5]), bar=t(rng.integers(0, 6, ROWS)), sched=t(sched), masks=t(masks, np.int32),
                beat=t(rng.integers(-1, 16, ROWS)), order=t(order, np.int32), gram=t(gram.view(np.int32), np.int32),
                targets=t(targets), bar_class=t(bar_class))


def dump(path):
    import torch
    import rlmg_amd  # noqa: F401
    from rlmg_amd import ops
    dev = torch.device("cuda:0")
    out = {}
    for ti, (tname, (w2e, dqn)) in enumerate(_tables().items()):
        I = _inputs(w2e, 100 + ti, dev)
        nc, A, L = I["n_class"], I["A"], I["logits"]
        table = dict(bar=I["bar"], sched=I["sched"], masks=I["masks"])
        gr = (I["beat"], I["order"], I["gram"], 2)
        for sname, (temp, top_p) in (("plain", (None, None)), ("dqn", dqn)):
            kw = dict(temperature=temp, top_p=top_p)
            tag = "%s/%s/" % (tname, sname)

            def put(name, tokens=None, f32=None):
                if tokens is not None:
                    out[tag + name + ":tokens"] = tokens.cpu().numpy()
                if f32 is not None:
                    out[tag + name + ":bits"] = f32.cpu().numpy().view(np.uint32)

            toks = lambda: torch.full((ROWS, A), -7, dtype=torch.int64, device=dev)
            ring = lambda: torch.full((3, ROWS, A, 2), 7.0, dtype=torch.float32, device=dev)
            pairs = lambda c=2: torch.full((ROWS, A, c), 7.0, dtype=torch.float32, device=dev)
            song = torch.full((200, ROWS, A), -7, dtype=torch.int64, device=dev)
            put("plain", ops.sample_categorical(L, nc, toks(), 99, counter=I["counter"], song=song, **kw))
            put("plain_song", song)
            put("slots", ops.sample_categorical(L, nc, toks(), 99, counter=I["counter"], slot_keys=True, **kw))
            put("keyed", ops.sample_categorical_keyed(L, nc, toks(), 99, I["key"], I["step"], **kw))
            for hname, how in (("counter", dict(counter=I["counter"])), ("keyed", dict(key=I["key"], step=I["step"]))):
                put("masked_" + hname, ops.sample_categorical_masked(L, nc, toks(), 99, **table, **how, **kw))
                for mname, m in (("unmasked", {}), ("masked", table)):
                    r = ring()
                    put("logp_%s_%s" % (mname, hname),
                        ops.sample_categorical_logp(L, nc, toks(), 99, r, out_counter=I["out_counter"], **how, **m, **kw), r)
                    put("grammar_%s_%s" % (mname, hname),
                        ops.sample_categorical_grammar(L, nc, toks(), 99, *gr, **how, **m, **kw))
                    r = ring()
                    put("grammar_logp_%s_%s" % (mname, hname),
                        ops.sample_categorical_grammar(L, nc, toks(), 99, *gr, logp=r, out_counter=I["out_counter"],
                                                       **how, **m, **kw), r)
            for mname, m in (("unmasked", {}), ("masked", dict(key=I["key"], **table))):
                put("score_" + mname, f32=ops.score_categorical(L, nc, I["targets"], out=pairs(), **m, **kw))
                put("score_grammar_" + mname,
                    f32=ops.score_categorical_grammar(L, nc, I["targets"], *gr, out=pairs(), **m, **kw))
                for gname, g in (("free", None), ("grammar", gr)):
                    for rname, ref in (("single", None), ("pair", I["ref"])):
                        put("stats_%s_%s_%s" % (mname, gname, rname),
                            f32=ops.policy_stats(L, nc, ref, bar_class=I["bar_class"], grammar=g,
                                                 out=pairs(2 if ref is None else 4), **m, **kw))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print("%s: %d arrays" % (path, len(out)))


def time_forms(path):
    import json
    import torch
    import rlmg_amd  # noqa: F401
    from rlmg_amd import ops
    global ROWS
    ROWS = 256
    dev = torch.device("cuda:0")
    w2e, (temp, top_p) = _tables()["golden6"]
    I = _inputs(w2e, 100, dev)
    nc, A, L = I["n_class"], I["A"], I["logits"]
    kw = dict(temperature=temp, top_p=top_p)
    table = dict(bar=I["bar"], sched=I["sched"], masks=I["masks"])
    gr = (I["beat"], I["order"], I["gram"], 2)
    how = dict(key=I["key"], step=I["step"])
    mk = dict(key=I["key"], **table)
    toks = torch.zeros((ROWS, A), dtype=torch.int64, device=dev)
    ring = torch.zeros((1, ROWS, A, 2), device=dev)
    pairs, quads = torch.zeros((ROWS, A, 2), device=dev), torch.zeros((ROWS, A, 4), device=dev)
    tg = I["targets"]
    forms = {      # named by the template arguments of sample_categorical_kernel / policy_stats_kernel
        "sample<0,0,0,1> grammar": lambda: ops.sample_categorical_grammar(L, nc, toks, 9, *gr, **how, **kw),
        "sample<0,1,0,1> grammar logp": lambda: ops.sample_categorical_grammar(L, nc, toks, 9, *gr, logp=ring, **how, **kw),
        "sample<0,1,1,1> score_grammar": lambda: ops.score_categorical_grammar(L, nc, tg, *gr, out=pairs, **kw),
        "sample<1,0,0,0> masked": lambda: ops.sample_categorical_masked(L, nc, toks, 9, **table, **how, **kw),
        "sample<1,0,0,1> grammar masked": lambda: ops.sample_categorical_grammar(L, nc, toks, 9, *gr, **how, **table, **kw),
        "sample<1,1,0,0> logp masked": lambda: ops.sample_categorical_logp(L, nc, toks, 9, ring, **how, **table, **kw),
        "sample<1,1,0,1> grammar logp masked": lambda: ops.sample_categorical_grammar(L, nc, toks, 9, *gr, logp=ring, **how,
                                                                                      **table, **kw),
        "sample<1,1,1,0> score masked": lambda: ops.score_categorical(L, nc, tg, out=pairs, **mk, **kw),
        "sample<1,1,1,1> score_grammar masked": lambda: ops.score_categorical_grammar(L, nc, tg, *gr, out=pairs, **mk, **kw),
    }
    for mi, m in enumerate(({}, mk)):
        for gi, g in enumerate((None, gr)):
            for pi, ref in enumerate((None, I["ref"])):
                forms["stats<%d,%d,%d>" % (mi, gi, pi)] = (lambda m=m, g=g, ref=ref: ops.policy_stats(
                    L, nc, ref, bar_class=I["bar_class"], grammar=g, out=pairs if ref is None else quads, **m, **kw))
    res = {}
    for name, fn in forms.items():
        for _ in range(30):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(300)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        res[name] = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]) * 1e3)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1)
    print(os.path.basename(path), " ".join("%.2f" % v for v in res.values()))


def table(d, new="new"):
    import json
    load = lambda who: [json.load(open(os.path.join(d, "time_%s_%d.json" % (who, i)))) for i in range(1, 6)]
    P, N = load("parent"), load(new)
    bad = 0
    print("%-38s %-30s %-30s %7s %7s %7s %7s" % ("us per launch, 256 rows", "parent x5", new + " x5", "med par",
                                                 "med new", "new/par", "spread"))
    for k in P[0]:
        p, n = [r[k] for r in P], [r[k] for r in N]
        mp, mn = float(np.median(p)), float(np.median(n))
        sp = (max(p) - min(p)) / mp
        ok = mn <= mp * (1 + sp)
        bad += not ok
        print("%-38s %-30s %-30s %7.2f %7.2f %+6.2f%% %6.2f%%  %s" % (
            k, " ".join("%.2f" % v for v in p), " ".join("%.2f" % v for v in n), mp, mn, 100 * (mn / mp - 1), 100 * sp,
            "ok" if ok else "ABOVE"))
    return 1 if bad else 0


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("only in one file  %s" % k)
    for k in sorted(set(a.files) & set(b.files)):
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
        print("%-9s %s %s" % ("equal" if same else "DIFFERENT", k, a[k].shape))
        if not same:
            bad.append(k)
    print("%d arrays, %d differ" % (len(set(a.files) | set(b.files)), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 3 and sys.argv[1] == "time":
        time_forms(sys.argv[2])
    elif len(sys.argv) in (3, 4) and sys.argv[1] == "table":
        sys.exit(table(*sys.argv[2:]))
    else:
        sys.exit(__doc__)

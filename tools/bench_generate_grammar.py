"""The row grammar: generate_stream(grammar=...) against the unconstrained stream, on the repo dims (512/12/8, f32)
with the random-init model and seed of tools/bench_generate_stream.py and the synthetic CW vocabulary's event names.
    python tools/bench_generate_grammar.py [--songs 2048] [--slots 256] [--reps 2] [--out FILE]
Writes JSON lines to --out (default profiles/generate_grammar_bench.jsonl) and prints them:
  * kind "mode": tokens/s of generate_stream(--songs, slots=--slots) for "none" (no grammar, no constraints), "grammar"
    and "grammar+musical" (the grammar with the musical constraint of tools/bench_generate_constraints.py), alternated
    --reps times in this one call, each with its share of ill-formed drawn rows (Grammar.violations);
  * kind "check": per grammar mode, songs of the stream that differ from generate_batch(--songs) (must be 0), and the
    grammar / constraint violations of every mode's stream and batch songs (must be 0 in the grammar modes).
--only: one stream of each mode and one grammar generate_batch after a small warm-up, for a rocprofv3 kernel trace.
--stats FILE: summarise a rocprofv3 --stats kernel CSV into per-call sampler and track costs (one JSON line, appended
to --out)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rlmg_amd  # noqa: E402,F401
from rlmg_amd import data, generation  # noqa: E402

SEED = 2


def _word2event():
    return {k: v for k, v in data.synthetic_cp_vocabulary().items() if k != "type"}


def modes(w2e):
    """The three modes -> {name: (grammar, constraints)}."""
    g = generation.Grammar(w2e)
    musical = generation.Constraint(w2e, allow={"tempo": ["Tempo_110"],
                                                "pitch": ["Note_Pitch_%d" % p for p in range(48, 84)]},
                                    per_bar={"chord": [["C_M"], ["A_m"], ["F_M"], ["G_7"]]}, cycle=True)
    return {"none": (None, None), "grammar": (g, None), "grammar+musical": (g, musical)}, g


def _stats(path):
    """rocprofv3 kernel stats CSV -> per-call average microseconds of every sampler instantiation (named by its
    MASKED, LOGP, FORCED, GRAMMAR flags), the track kernel and the bar counter."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            key = None
            if "sample_categorical_kernel<" in name:
                flags = name.split("sample_categorical_kernel<")[1].split(">")[0].replace(" ", "").split(",")
                flags = [x in ("true", "1") for x in flags]
                key = ("grammar_" if flags[3] else "") + ("masked" if flags[0] else "keyed") + "_sampler"
            elif "grammar_track_kernel" in name:
                key = "grammar_track"
            elif "count_bars_kernel" in name:
                key = "count_bars"
            if key:
                out[key + "_calls"] = int(r["Calls"])
                out[key + "_avg_us"] = float(r["AverageNs"]) / 1e3
    for a, b in (("grammar_keyed", "keyed"), ("grammar_masked", "masked")):
        if a + "_sampler_avg_us" in out and b + "_sampler_avg_us" in out:
            out["%s_over_%s" % (a, b)] = out[a + "_sampler_avg_us"] / out[b + "_sampler_avg_us"]
    return out


def _ill_formed(g, songs):
    drawn = sum(len(s) - 1 for s in songs)
    return sum(len(g.violations(s, n_prompt=1)) for s in songs), drawn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_grammar_bench.jsonl"))
    a = ap.parse_args()
    if a.stats:
        d = dict(_stats(a.stats), kind="kernels", source=os.path.basename(a.stats))
        print(json.dumps(d))
        with open(a.out, "a") as f:
            f.write(json.dumps(d) + "\n")
        return
    from rlmg_amd.dqn_policy import model
    w2e = _word2event()
    n_class = [len(v) for v in w2e.values()]
    torch.manual_seed(0)
    net = model.LinearTransformer(n_class, is_training=False).cuda().eval()
    dev = torch.cuda.get_device_name(0)
    md, g = modes(w2e)
    kw = dict(bar_cond=a.bar_cond, max_tokens=a.max_tokens)
    torch.manual_seed(SEED)
    for gr, c in md.values():                              # warm-up: library load, captures of every mode
        generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64, constraints=c, grammar=gr)
    generation.generate_batch(net, w2e, 8, bar_cond=3, max_tokens=64, grammar=g)
    torch.cuda.synchronize()
    if a.only:
        for name, (gr, c) in md.items():
            torch.manual_seed(SEED)
            _, st = generation._generate_stream(net, w2e, a.songs, slots=a.slots, constraints=c, grammar=gr, **kw)
            print(json.dumps(dict(st, mode=name, songs=a.songs, slots=a.slots)))
        torch.manual_seed(SEED)
        generation.generate_batch(net, w2e, a.slots, constraints=md["grammar+musical"][1], grammar=g, **kw)
        return
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    songs = {}
    for rep in range(a.reps):
        for name, (gr, c) in md.items():
            torch.manual_seed(SEED)
            got, st = generation._generate_stream(net, w2e, a.songs, slots=a.slots, constraints=c, grammar=gr, **kw)
            songs[name] = got
            n_tok = sum(len(s) for s in got)
            bad, drawn = _ill_formed(g, got) if rep == 0 else (None, None)
            emit({"kind": "mode", "mode": name, "rep": rep, "slots": a.slots, "songs": a.songs,
                  "seconds": st["seconds"], "tokens": n_tok, "tokens_per_s": n_tok / st["seconds"],
                  "steps": st["steps"], "wait_seconds": st["wait_seconds"], "graph": st["graph"],
                  "capped": sum(len(s) == a.max_tokens for s in got), "ill_formed_rows": bad, "drawn_rows": drawn,
                  "ill_formed_share": None if bad is None else bad / max(drawn, 1)})
            torch.cuda.empty_cache()
    same = lambda x, y: x.shape == y.shape and (x == y).all()
    for name in ("grammar", "grammar+musical"):
        gr, c = md[name]
        torch.manual_seed(SEED)
        t = time.perf_counter()
        ref = generation.generate_batch(net, w2e, a.songs, constraints=c, grammar=gr, **kw)
        wall = time.perf_counter() - t
        emit({"kind": "check", "mode": name, "slots": a.slots, "songs": a.songs, "batch_seconds": wall,
              "songs_differing_stream_vs_batch": int(sum(not same(x, y) for x, y in zip(songs[name], ref))),
              "grammar_violations_stream": _ill_formed(g, songs[name])[0],
              "grammar_violations_batch": _ill_formed(g, ref)[0],
              "constraint_violations_stream": 0 if c is None else int(sum(len(c.violations(s[1:]))
                                                                          for s in songs[name])),
              "mean_song_rows": float(np.mean([len(s) for s in songs[name]]))})
        del ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

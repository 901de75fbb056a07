"""Constrained generation: generate_stream(constraints=...) against the unconstrained stream, on the repo dims
(512/12/8, f32) with the random-init model and seed of tools/bench_generate_stream.py and the synthetic CW vocabulary's
event names.
    python tools/bench_generate_constraints.py [--songs 2048] [--slots 256] [--reps 2] [--out FILE]
Writes JSON lines to --out (default profiles/generate_constraints_bench.jsonl) and prints them:
  * kind "mode": tokens/s of generate_stream(--songs, slots=--slots) for "none" (no constraints), "permissive" (a
    Constraint that allows every class) and "musical" (a fixed tempo, a pitch range and a 4-chord progression with
    cycle=True), alternated --reps times in this one call;
  * kind "check": songs of the musical stream that differ from generate_batch(constraints=musical) (must be 0), rows
    of either that violate the constraint (must be 0), and songs of the permissive stream that differ from the
    unconstrained one (must be 0).
--only: one unconstrained stream, one musical stream and one musical generate_batch after a small warm-up, for a
rocprofv3 kernel trace (the masked sampler against cwlt_sample_categorical_keyed, and cwlt_count_bars).
--stats FILE: summarise a rocprofv3 --stats kernel CSV into per-token sampler costs (one JSON line, appended to --out)."""
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


def constraints(w2e):
    """The three modes' constraints: None, every class allowed, and the musical one."""
    permissive = generation.Constraint(w2e, allow={k: list(range(len(v))) for k, v in w2e.items()})
    musical = generation.Constraint(w2e, allow={"tempo": ["Tempo_110"],
                                                "pitch": ["Note_Pitch_%d" % p for p in range(48, 84)]},
                                    per_bar={"chord": [["C_M"], ["A_m"], ["F_M"], ["G_7"]]}, cycle=True)
    return {"none": None, "permissive": permissive, "musical": musical}


def _stats(path):
    """rocprofv3 kernel stats CSV -> per-call average microseconds of the samplers and the bar counter."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            key = ("masked_sampler" if "sample_categorical_kernel<true>" in name else
                   "keyed_sampler" if "sample_categorical_kernel<false>" in name else
                   "count_bars" if "count_bars_kernel" in name else None)
            if key:
                out[key + "_calls"] = int(r["Calls"])
                out[key + "_avg_us"] = float(r["AverageNs"]) / 1e3
    if "masked_sampler_avg_us" in out and "keyed_sampler_avg_us" in out:
        out["masked_over_keyed"] = out["masked_sampler_avg_us"] / out["keyed_sampler_avg_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_constraints_bench.jsonl"))
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
    modes = constraints(w2e)
    torch.manual_seed(SEED)
    for c in modes.values():                               # warm-up: library load, captures of every mode
        generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64, constraints=c)
    generation.generate_batch(net, w2e, 8, bar_cond=3, max_tokens=64, constraints=modes["musical"])
    torch.cuda.synchronize()
    if a.only:
        for name in ("none", "musical"):
            torch.manual_seed(SEED)
            _, st = generation._generate_stream(net, w2e, a.songs, slots=a.slots, bar_cond=a.bar_cond,
                                                max_tokens=a.max_tokens, constraints=modes[name])
            print(json.dumps(dict(st, mode=name, songs=a.songs, slots=a.slots)))
        torch.manual_seed(SEED)
        generation.generate_batch(net, w2e, a.slots, bar_cond=a.bar_cond, max_tokens=a.max_tokens,
                                  constraints=modes["musical"])
        return
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    songs = {}
    for rep in range(a.reps):
        for name, c in modes.items():
            torch.manual_seed(SEED)
            got, st = generation._generate_stream(net, w2e, a.songs, slots=a.slots, bar_cond=a.bar_cond,
                                                  max_tokens=a.max_tokens, constraints=c)
            songs[name] = got
            n_tok = sum(len(s) for s in got)
            emit({"kind": "mode", "mode": name, "rep": rep, "slots": a.slots, "songs": a.songs,
                  "seconds": st["seconds"], "tokens": n_tok, "tokens_per_s": n_tok / st["seconds"],
                  "steps": st["steps"], "wait_seconds": st["wait_seconds"], "graph": st["graph"],
                  "capped": sum(len(s) == a.max_tokens for s in got)})
            torch.cuda.empty_cache()
    musical = modes["musical"]
    torch.manual_seed(SEED)
    t = time.perf_counter()
    ref = generation.generate_batch(net, w2e, a.songs, bar_cond=a.bar_cond, max_tokens=a.max_tokens,
                                    constraints=musical)
    wall = time.perf_counter() - t
    same = lambda x, y: x.shape == y.shape and (x == y).all()
    emit({"kind": "check", "slots": a.slots, "songs": a.songs, "batch_seconds": wall,
          "songs_differing_stream_vs_batch": int(sum(not same(x, y) for x, y in zip(songs["musical"], ref))),
          "violating_rows_stream": int(sum(len(musical.violations(s[1:])) for s in songs["musical"])),
          "violating_rows_batch": int(sum(len(musical.violations(s[1:])) for s in ref)),
          "songs_differing_permissive_vs_none": int(sum(not same(x, y)
                                                        for x, y in zip(songs["permissive"], songs["none"]))),
          "mean_song_rows": {k: float(np.mean([len(s) for s in v])) for k, v in songs.items()}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

"""The blended stream against the plain one: generate_stream(reference=, alpha=) beside generate_stream, alternated in
one process, on the repo dims (512/12/8, f32) with the random-init model and seed of tools/bench_generate_stream.py and
a reference of the same shape from another seed.
    python tools/bench_generate_blend.py [--songs 2048] [--slots 256] [--max-tokens 4096] [--reps 2] [--out FILE]
Writes JSON lines to --out (default profiles/generate_blend_bench.jsonl) and prints them:
  * kind "mode": songs/s, tokens/s, steps and host wait of each run, mode "stream" or "blend" (alpha: a per-song ramp
    from 0 to 1.5, so one run traces the frontier);
  * kind "ratio": the blended stream's tokens/s over the plain stream's, best of each mode;
  * kind "launch": mean milliseconds of the cwlt_blend_logits launch and of the keyed sampler's, both bracketed by
    events (ops.KernelTimer) in one eager blended run of --timed-songs songs, with the refill's and advance's beside them;
  * kind "check": how many songs of generate_batch(reference=, alpha=) differ from the blended stream's (must be 0)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402

N_CLASS = [56, 135, 18, 87, 18, 25]
SEED = 2


def _word2event():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    return w2e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timed-songs", type=int, default=256)
    ap.add_argument("--timed-tokens", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_blend_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    torch.manual_seed(0)
    net = model.LinearTransformer(N_CLASS, is_training=False).cuda().eval()
    torch.manual_seed(1)
    ref = model.LinearTransformer(N_CLASS, is_training=False).cuda().eval()
    w2e = _word2event()
    dev = torch.cuda.get_device_name(0)
    alpha = np.linspace(0.0, 1.5, a.songs)
    blend = dict(reference=ref, alpha=alpha)
    torch.manual_seed(SEED)
    generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64)     # warm-up: library load, captures
    generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64, reference=ref, alpha=0.5)
    torch.cuda.synchronize()
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    best, songs_of = {}, {}
    for rep in range(a.reps):
        for mode, kw in (("stream", {}), ("blend", blend)):
            torch.manual_seed(SEED)
            songs, st = generation._generate_stream(net, w2e, a.songs, slots=a.slots, bar_cond=a.bar_cond,
                                                    max_tokens=a.max_tokens, **kw)
            n_tok = sum(len(s) for s in songs)
            rate = n_tok / st["seconds"]
            best[mode] = max(best.get(mode, 0.0), rate)
            songs_of[mode] = songs
            emit({"kind": "mode", "mode": mode, "rep": rep, "slots": a.slots, "songs": a.songs,
                  "seconds": st["seconds"], "tokens": n_tok, "songs_per_s": a.songs / st["seconds"],
                  "tokens_per_s": rate, "steps": st["steps"], "wait_seconds": st["wait_seconds"],
                  "graph": st["graph"], "capped": sum(len(s) == a.max_tokens for s in songs)})
            torch.cuda.empty_cache()
    emit({"kind": "ratio", "slots": a.slots, "songs": a.songs, "stream_tokens_per_s": best["stream"],
          "blend_tokens_per_s": best["blend"], "blend_over_stream": best["blend"] / best["stream"]})

    # the launches of one blended token, event by event, in an eager run (a captured graph has no events inside it)
    graphs = ops.GRAPHS_ENABLED
    ops.GRAPHS_ENABLED = False
    try:
        ops.KernelTimer.reset(True)
        torch.manual_seed(SEED)
        generation.generate_stream(net, w2e, a.timed_songs, slots=a.slots, bar_cond=a.bar_cond,
                                   max_tokens=a.timed_tokens, reference=ref, alpha=alpha[:a.timed_songs])
        torch.cuda.synchronize()
        summary = ops.KernelTimer.summary()
    finally:
        ops.KernelTimer.reset(False)
        ops.GRAPHS_ENABLED = graphs
    pick = ("cwlt_blend_logits", "cwlt_sample_categorical_keyed", "cwlt_stream_refill", "cwlt_stream_advance")
    emit({"kind": "launch", "slots": a.slots, "eager": True,
          "mean_ms": {k: summary[k][1] for k in pick if k in summary},
          "calls": {k: summary[k][0] for k in pick if k in summary}})

    torch.manual_seed(SEED)
    want = generation.generate_batch(net, w2e, a.songs, bar_cond=a.bar_cond, max_tokens=a.max_tokens, **blend)
    differ = sum(not (x.shape == y.shape and (x == y).all()) for x, y in zip(songs_of["blend"], want))
    emit({"kind": "check", "slots": a.slots, "songs": a.songs, "songs_differing_from_generate_batch": int(differ)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

"""The preferred stream against the plain one: generate_stream(preferences=) beside generate_stream, alternated in one
process, on the repo dims (512/12/8, f32) with the random-init model and seed of tools/bench_generate_stream.py.
    python tools/bench_generate_prefer.py [--songs 2048] [--slots 256] [--max-tokens 4096] [--reps 2] [--out FILE]
The preference: a scale bias on pitch, a per-bar chord bias (cycled) and a pitch repetition penalty with decay 0.9, one
object for every song.  Writes JSON lines to --out (default profiles/generate_prefer_bench.jsonl) and prints them:
  * kind "mode": songs/s, tokens/s, steps and host wait of each run, mode "stream" or "prefer";
  * kind "ratio": the preferred stream's tokens/s over the plain stream's, best of each mode;
  * kind "launch": mean milliseconds of the cwlt_prefer_logits and cwlt_prefer_track launches and of the keyed
    sampler's, refill's and advance's, bracketed by events (ops.KernelTimer) in one eager preferred run of --timed-songs;
  * kind "score": seconds of score_songs over --score-songs of the preferred songs, with and without preferences, best
    of --reps, and their ratio;
  * kind "check": how many songs of generate_batch(preferences=) differ from the preferred stream's (must be 0), and
    how many drawn rows repeat a pitch of the last 8 rows of their song, with and without the preference."""
import argparse
import json
import os
import sys
import time

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


def _preference(w2e):
    scale = {c: 1.0 for c in range(1, N_CLASS[3]) if (c - 1) % 12 in (0, 2, 4, 5, 7, 9, 11)}      # a major scale
    chords = [{1 + 12 * k + r: 2.0 for k in range(11) if 1 + 12 * k + r < N_CLASS[1]} for r in (0, 5, 7, 0)]
    return generation.Preference(w2e, bias={"pitch": scale}, per_bar={"chord": chords}, cycle=True,
                                 repeat={"pitch": (0.5, 1.0)}, decay=0.9)


def _recent_repeats(songs, window=8):
    n = 0
    for s in songs:
        p = s[:, 3]
        n += sum(1 for t in range(1, len(p)) if p[t] > 0 and p[t] in p[max(0, t - window):t])
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--timed-songs", type=int, default=256)
    ap.add_argument("--timed-tokens", type=int, default=96)
    ap.add_argument("--score-songs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_prefer_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    torch.manual_seed(0)
    net = model.LinearTransformer(N_CLASS, is_training=False).cuda().eval()
    w2e = _word2event()
    pref = _preference(w2e)
    dev = torch.cuda.get_device_name(0)
    torch.manual_seed(SEED)
    generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64)     # warm-up: library load, captures
    generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64, preferences=pref)
    torch.cuda.synchronize()
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    best, songs_of = {}, {}
    for rep in range(a.reps):
        for mode, kw in (("stream", {}), ("prefer", dict(preferences=pref))):
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
          "prefer_tokens_per_s": best["prefer"], "prefer_over_stream": best["prefer"] / best["stream"]})

    # the launches of one preferred token, event by event, in an eager run (a captured graph has no events inside it)
    graphs = ops.GRAPHS_ENABLED
    ops.GRAPHS_ENABLED = False
    try:
        ops.KernelTimer.reset(True)
        torch.manual_seed(SEED)
        generation.generate_stream(net, w2e, a.timed_songs, slots=a.slots, bar_cond=a.bar_cond,
                                   max_tokens=a.timed_tokens, preferences=pref)
        torch.cuda.synchronize()
        summary = ops.KernelTimer.summary()
    finally:
        ops.KernelTimer.reset(False)
        ops.GRAPHS_ENABLED = graphs
    pick = ("cwlt_prefer_logits", "cwlt_prefer_track", "cwlt_sample_categorical_keyed", "cwlt_stream_refill",
            "cwlt_stream_advance")
    emit({"kind": "launch", "slots": a.slots, "eager": True,
          "mean_ms": {k: summary[k][1] for k in pick if k in summary},
          "calls": {k: summary[k][0] for k in pick if k in summary}})

    # score_songs over some of the preferred songs, with and without the preference
    given = songs_of["prefer"][:a.score_songs]
    seconds = {}
    for rep in range(a.reps + 1):                                     # the first pass warms up
        for mode, kw in (("plain", {}), ("prefer", dict(preferences=pref))):
            torch.cuda.synchronize()
            t = time.perf_counter()
            generation.score_songs(net, w2e, given, **kw)
            torch.cuda.synchronize()
            if rep:
                seconds[mode] = min(seconds.get(mode, np.inf), time.perf_counter() - t)
    emit({"kind": "score", "songs": len(given), "rows": int(sum(len(s) for s in given)),
          "plain_seconds": seconds["plain"], "prefer_seconds": seconds["prefer"],
          "prefer_over_plain": seconds["prefer"] / seconds["plain"]})

    torch.manual_seed(SEED)
    want = generation.generate_batch(net, w2e, a.songs, bar_cond=a.bar_cond, max_tokens=a.max_tokens, preferences=pref)
    differ = sum(not (x.shape == y.shape and (x == y).all()) for x, y in zip(songs_of["prefer"], want))
    emit({"kind": "check", "slots": a.slots, "songs": a.songs, "songs_differing_from_generate_batch": int(differ),
          "recent_pitch_repeats": {"stream": _recent_repeats(songs_of["stream"]),
                                   "prefer": _recent_repeats(songs_of["prefer"])},
          "drawn_rows": {m: int(sum(len(s) for s in songs_of[m])) for m in ("stream", "prefer")}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

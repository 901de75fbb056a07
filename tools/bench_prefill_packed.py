"""The packed prefill against the padded batch-invariant one ("gemm"), on the repo dims (512/12/8, f32) with the
random-init model of tools/bench_generate_prompts.py and a fixed seed; the two interleaved, --repeats times each.
    python tools/bench_prefill_packed.py [--songs 2048] [--repeats 3] [--cases a b c] [--out FILE]
Writes JSON lines to --out (default profiles/prefill_packed_bench.jsonl) and prints them, one per case:
  a  score_songs on --songs songs of lengths uniform in [256, 1024];
  b  the same at fill 1.0 (every song 1 024 rows);
  c  generate_stream with --songs prompts of 64-512 rows on 256 slots, packed_prefill off and on: the prefill's GPU
     seconds (stats()["prefill_seconds"]) and tokens/s.
Each line carries every repeat's seconds, the medians, packed / padded, and the fill (live rows over the rows the
padded blocks compute).  The scores and songs of the two paths are compared bit for bit ("differing" must be 0)."""
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
from rlmg_amd import generation  # noqa: E402

N_CLASS = [56, 135, 18, 87, 18, 25]
SEED = 2


def _word2event():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    return w2e


def _songs(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    out = []
    for L in rng.integers(lo, hi + 1, n):
        p = np.stack([rng.integers(0, c, L) for c in N_CLASS], 1).astype(np.int64)
        p[1:, 2] = np.where(p[1:, 2] == 1, 0, p[1:, 2])                 # no Bar after the first row: bar count 1
        out.append(p)
    return out


def _padded_rows(lengths, budget, cap):
    """The rows the padded blocks compute: blocks of budget // longest songs, each padded to its own longest."""
    per = max(1, min(cap, budget // max(lengths)))
    return sum(len(lengths[a:a + per]) * max(lengths[a:a + per]) for a in range(0, len(lengths), per))


def _same(a, b):
    return sum(not (x.shape == y.shape and np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x,
                                                          y.view(np.int32) if y.dtype == np.float32 else y))
               for x, y in zip(a, b))


def _score_case(net, w2e, songs, repeats):
    runs = {"gemm": [], "packed": []}
    last = {}
    generation.score_songs(net, w2e, songs[:8], kernel="gemm")          # warm-up: code objects
    generation.score_songs(net, w2e, songs[:8], kernel="packed")
    for _ in range(repeats):
        for kernel in ("gemm", "packed"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            last[kernel] = generation.score_songs(net, w2e, songs, kernel=kernel)
            torch.cuda.synchronize()
            runs[kernel].append(time.perf_counter() - t)
    lens = [len(s) for s in songs]
    padded = _padded_rows(lens, generation.PREFILL_ROWS, generation.SCORE_BLOCK_SONGS)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    return {"songs": len(songs), "rows": sum(lens), "padded_rows": padded, "fill": sum(lens) / padded,
            "padded_blocks": -(-len(lens) // max(1, min(generation.SCORE_BLOCK_SONGS,
                                                       generation.PREFILL_ROWS // max(lens)))),
            "packed_blocks": len(generation.packed_blocks(lens, None, generation.SCORE_BLOCK_SONGS)),
            "gemm_seconds": runs["gemm"], "packed_seconds": runs["packed"], "gemm_median": med["gemm"],
            "packed_median": med["packed"], "packed_over_padded": med["packed"] / med["gemm"],
            "differing": _same(last["gemm"], last["packed"])}


def _stream_case(net, w2e, prompts, slots, repeats, bar_cond, max_tokens):
    runs = {False: [], True: []}
    last = {}
    for packed in (False, True):                                        # warm-up
        generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=600, prompts=prompts[:8],
                                   packed_prefill=packed)
    for _ in range(repeats):
        for packed in (False, True):
            torch.manual_seed(SEED)
            songs, st = generation._generate_stream(net, w2e, len(prompts), slots=slots, bar_cond=bar_cond,
                                                    max_tokens=max_tokens, prompts=prompts, packed_prefill=packed)
            last[packed] = songs
            runs[packed].append({"prefill_seconds": st["prefill_seconds"], "seconds": st["seconds"],
                                 "tokens_per_s": sum(len(s) for s in songs) / st["seconds"],
                                 "drawn_per_s": st["drawn"] / st["seconds"], "prefill_blocks": st["prefill_blocks"],
                                 "block": st["block"]})
            torch.cuda.empty_cache()
    lens = [len(p) for p in prompts]
    B = runs[False][0]["block"]
    padded = sum(len(lens[a:a + B]) * max(lens[a:a + B]) for a in range(0, len(lens), B))
    med = lambda packed, k: float(np.median([r[k] for r in runs[packed]]))      # noqa: E731
    return {"songs": len(prompts), "slots": slots, "rows": sum(lens), "padded_rows": padded, "fill": sum(lens) / padded,
            "block": B, "prefill_blocks": runs[False][0]["prefill_blocks"], "padded_runs": runs[False],
            "packed_runs": runs[True], "padded_prefill_median": med(False, "prefill_seconds"),
            "packed_prefill_median": med(True, "prefill_seconds"),
            "packed_over_padded": med(True, "prefill_seconds") / med(False, "prefill_seconds"),
            "padded_tokens_per_s": med(False, "tokens_per_s"), "packed_tokens_per_s": med(True, "tokens_per_s"),
            "differing": _same(last[False], last[True])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_packed_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefill_packed measures on the GPU; none found")
    from rlmg_amd.dqn_policy import model
    torch.manual_seed(0)
    net = model.LinearTransformer(N_CLASS, is_training=False).cuda().eval()
    w2e = _word2event()
    head = {"device": torch.cuda.get_device_name(0), "dims": "512/12/8 f32", "seed": SEED, "repeats": a.repeats}
    lines = []

    def emit(rec):
        rec = dict(head, **rec)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    if "a" in a.cases:
        emit(dict(case="a", what="score_songs, lengths uniform in [256, 1024]",
                  **_score_case(net, w2e, _songs(a.songs, 256, 1024, 1), a.repeats)))
    if "b" in a.cases:
        emit(dict(case="b", what="score_songs, every song 1024 rows",
                  **_score_case(net, w2e, _songs(a.songs, 1024, 1024, 1), a.repeats)))
    if "c" in a.cases:
        emit(dict(case="c", what="generate_stream, prompts of 64-512 rows",
                  **_stream_case(net, w2e, _songs(a.songs, 64, 512, 0), a.slots, a.repeats, a.bar_cond, a.max_tokens)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Song log-likelihoods: score_songs throughput against the prefill of the same rows, and the cost of
return_logprobs on the stream, on the repo dims (512/12/8, f32) with a random-init model, random tokens and the
synthetic CW vocabulary (no dataset is needed).
    python tools/bench_score.py [--songs 2048] [--rows 1024] [--stream-songs 2048] [--slots 256] [--reps 2] [--out FILE]
Writes JSON lines to --out (default profiles/score_bench.jsonl) and prints them:
  * kind "score": tokens/s of score_songs(kernel=...) on --songs random songs of --rows rows, and of the prefill alone
    of the same rows (DecodeSession._prefill, last-row heads, in the same blocks of PREFILL_ROWS // rows songs), the
    modes alternated --reps times; cost = prefill tokens/s / score tokens/s (the estimate: <= 1.2);
  * kind "stream": tokens/s of generate_stream(--stream-songs, slots=--slots, bar_cond 17) without and with
    return_logprobs, alternated --reps times; ratio = with / without (the estimate: >= 0.98);
  * kind "check": songs of the two streams that differ (must be 0), non-finite log-probs, and the largest difference
    between the stream's model log-probs and score_songs(kernel="gemm") of the same songs.
--only: one stream of --stream-songs songs without and one with return_logprobs after a warm-up, for a rocprofv3 kernel
trace (the log-prob sampler against cwlt_sample_categorical_keyed).
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


def _stats(path):
    """rocprofv3 kernel stats CSV -> per-call average microseconds of the keyed sampler and the log-prob sampler."""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"].replace(" ", "")
            key = ("logp_sampler" if "sample_categorical_kernel<false,true,false>" in name else
                   "keyed_sampler" if "sample_categorical_kernel<false,false,false>" in name else
                   "scorer" if "sample_categorical_kernel<false,true,true>" in name else None)
            if key:
                out[key + "_calls"] = int(r["Calls"])
                out[key + "_avg_us"] = float(r["AverageNs"]) / 1e3
    if "logp_sampler_avg_us" in out and "keyed_sampler_avg_us" in out:
        out["logp_over_keyed"] = out["logp_sampler_avg_us"] / out["keyed_sampler_avg_us"]
    return out


def _prefill_rows(net, songs, kernel):
    """The prefill alone of the songs' rows in score_songs' blocks: DecodeSession._prefill (last-row heads)."""
    rows = len(songs[0])
    per = max(1, generation.PREFILL_ROWS // rows)
    sess = generation.DecodeSession(net, n_songs=per, kernel="gemm", graph=False)
    for a in range(0, len(songs), per):
        blk = songs[a:a + per]
        if len(blk) != per:
            sess = generation.DecodeSession(net, n_songs=len(blk), kernel="gemm", graph=False)
        sess.reset()
        sess._prefill(np.stack(blk), kernel=kernel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--stream-songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-score", action="store_true")
    ap.add_argument("--only", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.jsonl"))
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
    torch.manual_seed(SEED)
    for flag in (False, True):                              # warm-up: library load, captures of both forms
        generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64, return_logprobs=flag)
    torch.cuda.synchronize()
    if a.only:
        for flag in (False, True):
            torch.manual_seed(SEED)
            _, st = generation._generate_stream(net, w2e, a.stream_songs, slots=a.slots, bar_cond=a.bar_cond,
                                                max_tokens=a.max_tokens, return_logprobs=flag)
            print(json.dumps(dict(st, logprobs=flag, songs=a.stream_songs, slots=a.slots)))
        return
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    if not a.skip_score:
        rng = np.random.default_rng(SEED)
        songs = [np.stack([rng.integers(0, c, a.rows) for c in n_class], 1).astype(np.int64) for _ in range(a.songs)]
        generation.score_songs(net, w2e, songs[:4])                         # warm-up
        _prefill_rows(net, songs[:4], "gemm")
        tokens = a.songs * a.rows
        for rep in range(a.reps):
            for kernel in ("gemm", "blas"):
                res = {}
                for mode in ("prefill", "score"):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    if mode == "prefill":
                        _prefill_rows(net, songs, kernel)
                    else:
                        generation.score_songs(net, w2e, songs, kernel=kernel)
                    torch.cuda.synchronize()
                    res[mode] = time.perf_counter() - t
                    torch.cuda.empty_cache()
                emit({"kind": "score", "kernel": kernel, "rep": rep, "songs": a.songs, "rows": a.rows,
                      "tokens": tokens, "prefill_seconds": res["prefill"], "score_seconds": res["score"],
                      "prefill_tokens_per_s": tokens / res["prefill"], "score_tokens_per_s": tokens / res["score"],
                      "cost": res["score"] / res["prefill"]})
        del songs
    got = {}
    for rep in range(a.reps):
        for flag in (False, True):
            torch.manual_seed(SEED)
            out, st = generation._generate_stream(net, w2e, a.stream_songs, slots=a.slots, bar_cond=a.bar_cond,
                                                  max_tokens=a.max_tokens, return_logprobs=flag)
            got[flag] = out
            songs = out[0] if flag else out
            n_tok = sum(len(s) for s in songs)
            emit({"kind": "stream", "logprobs": flag, "rep": rep, "slots": a.slots, "songs": a.stream_songs,
                  "seconds": st["seconds"], "tokens": n_tok, "tokens_per_s": n_tok / st["seconds"],
                  "steps": st["steps"], "wait_seconds": st["wait_seconds"], "graph": st["graph"]})
            torch.cuda.empty_cache()
    plain, (songs, lps) = got[False], got[True]
    same = lambda x, y: x.shape == y.shape and (x == y).all()
    check = songs[:64]
    scored = generation.score_songs(net, w2e, check, sampler="dqn")
    emit({"kind": "check", "songs": a.stream_songs, "slots": a.slots,
          "songs_differing_with_vs_without": int(sum(not same(x, y) for x, y in zip(plain, songs))),
          "nonfinite_logprobs": int(sum((~np.isfinite(lp)).sum() for lp in lps)),
          "scored_songs": len(check),
          "max_model_logprob_diff_stream_vs_scored": float(max(np.abs(sc[:, :, 0] - lp[:, :, 0]).max()
                                                              for sc, lp in zip(scored, lps[:64]))),
          "mean_song_rows": float(np.mean([len(s) for s in songs]))})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

"""Policy entropy and KL: generation.policy_stats against score_songs over the same rows, on the repo
dims (512/12/8, f32) with random-init models, random tokens and the synthetic CW vocabulary (no dataset is needed).
    python tools/bench_policy_stats.py [--songs 2048] [--rows 1024] [--reps 2] [--kernel gemm] [--out FILE]
The three modes -- score_songs, policy_stats(), policy_stats(reference=...) -- are alternated --reps times in one call,
each over the same --songs random songs of --rows rows with the "dqn" sampler settings.  Writes one JSON line per rep to
--out (default profiles/policy_stats_bench.jsonl) and prints it: the seconds of each mode and the ratios stats / score
(the estimate: <= 1.05) and stats_ref / score (the estimate: <= 2.1; the reference's prefill runs on the same blocks)."""
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
from rlmg_amd import data, generation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kernel", default="gemm", choices=("gemm", "blas"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_stats_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    w2e = {k: v for k, v in data.synthetic_cp_vocabulary().items() if k != "type"}
    n_class = [len(v) for v in w2e.values()]
    nets = []
    for seed in (0, 1):                                         # the policy and a reference of the same dims
        torch.manual_seed(seed)
        nets.append(model.LinearTransformer(n_class, is_training=False).cuda().eval())
    net, ref = nets
    rng = np.random.default_rng(2)
    songs = [np.stack([rng.integers(0, c, a.rows) for c in n_class], 1).astype(np.int64) for _ in range(a.songs)]
    kw = dict(sampler="dqn", kernel=a.kernel)
    modes = {"score": lambda s: generation.score_songs(net, w2e, s, **kw),
             "stats": lambda s: generation.policy_stats(net, w2e, s, **kw),
             "stats_ref": lambda s: generation.policy_stats(net, w2e, s, reference=ref, **kw)}
    for fn in modes.values():                                   # warm-up: library load, every kernel once
        fn(songs[:4])
    lines = []
    for rep in range(a.reps):
        res = {}
        for name, fn in modes.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(songs)
            torch.cuda.synchronize()
            res[name] = time.perf_counter() - t
            torch.cuda.empty_cache()
        d = {"kind": "policy_stats", "kernel": a.kernel, "rep": rep, "songs": a.songs, "rows": a.rows,
             "tokens": a.songs * a.rows, "score_seconds": res["score"], "stats_seconds": res["stats"],
             "stats_ref_seconds": res["stats_ref"], "stats_over_score": res["stats"] / res["score"],
             "stats_ref_over_score": res["stats_ref"] / res["score"], "device": torch.cuda.get_device_name(0)}
        print(json.dumps(d), flush=True)
        lines.append(d)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

"""Reward-guided particle generation: generate_particles with a WindowReward on the AIRL discriminator
against generate_particles without a reward, on the repo dims (policy 512/12/8, discriminator 512/10/8, f32, both random
init) and README's constrained particle workload (a fixed tempo, a pitch range and a cycled 4-chord progression).
    python tools/bench_generate_reward.py [--songs 64] [--particles 4] [--every 16] [--window 50] [--beta 1.0]
                                          [--ess 0.5] [--reps 2] [--out FILE]
Writes JSON lines to --out (default profiles/generate_reward_bench.jsonl) and prints them:
  * kind "mode": tokens/s and ms per lock-step token of generate_particles(songs, particles, resample_every=--every,
    ess=--ess) without a reward -- unchanged by this feature, the yardstick -- and with reward=WindowReward(disc),
    alternated --reps times in this one process, and the rewarded run's ratio to the plain run of the same rep;
  * kind "push": the HIP-event time of one cwlt_reward_push launch on the pool's rows, launched eagerly;
  * kind "reward_events": a timed rewarded run: per reward event the HIP-event milliseconds of cwlt_reward_window, of
    the callable (the discriminator's forward over rows x window tokens and the log-odds) and of cwlt_reward_apply --
    mean and largest -- and all reward events' share of the run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation, ops  # noqa: E402
from bench_generate_constraints import SEED, _word2event, constraints  # noqa: E402


def _particles(net, w2e, a, musical, reward, timed=False):
    """One generate_particles run through its parts, so that the loop's stats come back -> (sets, stats, seconds)."""
    torch.manual_seed(SEED)
    t = time.perf_counter()
    spec = generation._reward_spec(reward, a.window, a.beta)
    heads, caps, plan = generation._particle_setup(
        "generate_particles", net, w2e, a.songs, a.particles, a.every, a.ess, a.bar_cond, a.max_tokens, None, "dqn",
        128, "blas", musical, None, None, None, None)
    stats = {"timed": timed}
    sets = generation._run_particles(net, w2e, heads, caps, plan, a.particles, a.every, a.ess, a.bar_cond, 128, None,
                                     None, stats=stats, reward=spec)
    return sets, stats, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--particles", type=int, default=4)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--ess", type=float, default=0.5)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_reward_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import AIRL_model, model
    w2e = _word2event()
    n_class = [len(v) for v in w2e.values()]
    torch.manual_seed(0)
    net = model.LinearTransformer(n_class, is_training=False).cuda().eval()
    torch.manual_seed(1)
    disc = AIRL_model.LongFormer(n_class).cuda()
    reward = generation.WindowReward(disc)
    dev = torch.cuda.get_device_name(0)
    musical = constraints(w2e)["musical"]
    rows = a.songs * a.particles
    torch.manual_seed(SEED)                                    # warm-up: library load, the capture, the discriminator
    generation.generate_particles(net, w2e, 2, 4, resample_every=4, ess=1.0, bar_cond=3, max_tokens=64,
                                  constraints=musical, reward=reward, reward_window=a.window, beta=a.beta)
    x = torch.zeros((rows, a.window, len(n_class)), dtype=torch.int64, device="cuda")
    reward(x, torch.ones((rows, a.window), dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    lines = []

    def emit(d):
        d = dict(d, device=dev, songs=a.songs, particles=a.particles, rows=rows, resample_every=a.every,
                 reward_window=a.window, beta=a.beta, ess=a.ess)
        print(json.dumps(d), flush=True)
        lines.append(d)

    for rep in range(a.reps):
        base = None
        for name, fn in (("plain", None), ("reward", reward)):
            sets, st, wall = _particles(net, w2e, a, musical, fn)
            n_tok = sum(len(s) for ps in sets for s in ps.songs)
            d = {"kind": "mode", "mode": name, "rep": rep, "seconds": wall, "tokens": n_tok, "steps": st["steps"],
                 "tokens_per_s": n_tok / wall, "step_ms": 1e3 * wall / st["steps"], "events": st["events"],
                 "graph": st["graph"], "row_bytes": st["row_bytes"],
                 "mean_log_evidence": float(np.mean([ps.log_evidence for ps in sets]))}
            if fn is None:
                base = d
            else:
                d.update(reward_events=st["reward_events"], ratio_tokens_per_s=d["tokens_per_s"] / base["tokens_per_s"],
                         ratio_step_rate=base["step_ms"] / d["step_ms"],
                         mean_reward=float(np.mean(np.concatenate([r for ps in sets for r in ps.rewards]))))
            emit(d)
            del sets
            torch.cuda.empty_cache()
    # one push launch, by HIP events around a run of launches on buffers of the pool's size
    cuda = torch.device("cuda")
    A = len(n_class)
    tok, done = torch.zeros((rows, A), dtype=torch.int64, device=cuda), torch.zeros(rows, dtype=torch.int64, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int64, device=cuda)
    recent = torch.zeros((rows, a.window, A), dtype=torch.int64, device=cuda)
    live = torch.zeros((rows, a.window), dtype=torch.int64, device=cuda)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for n in (50, 1000):                                       # the first run warms up
        ev[0].record()
        for _ in range(n):
            ops.reward_push(tok, done, cnt, recent, live)
        ev[1].record()
        torch.cuda.synchronize()
    emit({"kind": "push", "launches": n, "us_per_launch": 1e3 * ev[0].elapsed_time(ev[1]) / n,
          "note": "eager launches back to back: launch-bound; inside the captured token the kernel itself is shorter"})
    _, st, wall = _particles(net, w2e, a, musical, reward, timed=True)
    ms = np.asarray(st["reward_ms"], dtype=np.float64).reshape(-1, 3)
    emit({"kind": "reward_events", "reward_events": st["reward_events"], "steps": st["steps"], "seconds": wall,
          "window_ms_mean": float(ms[:, 0].mean()), "callable_ms_mean": float(ms[:, 1].mean()),
          "apply_ms_mean": float(ms[:, 2].mean()), "window_ms_max": float(ms[:, 0].max()),
          "callable_ms_max": float(ms[:, 1].max()), "apply_ms_max": float(ms[:, 2].max()),
          "reward_ms_total": float(ms.sum()), "share_of_run": float(ms.sum()) * 1e-3 / wall,
          "tokens_scored_per_event": rows * a.window})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

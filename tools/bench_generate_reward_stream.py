"""Reward-guided particles on the stream: generate_particles(slots=, reward=) against lock-step reward
pools of the same size on the same song indices, on the repo dims (policy 512/12/8, discriminator 512/10/8, f32, both
random init) with README's constrained workload and reward=WindowReward(disc).
    python tools/bench_generate_reward_stream.py [--songs 2048] [--particles 4] [--slots 256] [--every 10]
                                                 [--window 50] [--chunk 100] [--beta 1.0] [--ess 1.0] [--reps 2]
                                                 [--out FILE]
--chunk must be a multiple of lcm(--every, --window), the stream's rule; the lock-step pools run with the same chunk.
Both modes run in this one process, alternated --reps times; the LAST repetition is written to --out (default
profiles/generate_reward_stream_bench.jsonl) as JSON lines, and every repetition is printed:
  * kind "mode", mode "lock_step": the songs in pools of --slots songs one after the other (generate()'s batch_size
    path: _run_particles on each slice of one plan, with the reward); tokens/s, steps, ms per step, the reward events
    and the callable's HIP-event time and share of the run -- in both modes from one pair of HIP events this tool puts
    around every call of the callable, the loops' own timing switched off, so that both are instrumented alike;
  * kind "mode", mode "stream": generate_particles(slots=--slots, reward=); the same, its ratio to the lock-step run of
    the same rep, and of its group-steps the share spent waiting for a boundary (and of that, beyond the next multiple
    of --every) and idle at the tail;
  * kind "estimate": what the code predicts from the lock-step run's own song lengths (each song's longest particle):
    lock-step steps = the sum over pools of the pool's longest song rounded up to the chunk; stream steps >= the sum
    over songs of the longest particle rounded up to B = lcm(--every, --window), divided by --slots (no tail)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation  # noqa: E402
from bench_generate_constraints import SEED, _word2event, constraints  # noqa: E402


def _setup(net, w2e, a, musical):
    return generation._particle_setup("generate_particles", net, w2e, a.songs, a.particles, a.every, a.ess, a.bar_cond,
                                      a.max_tokens, None, "dqn", a.chunk, "blas", musical, None, None, None, None,
                                      pool=min(a.songs, a.slots))


class _Timed:
    """The reward callable between two HIP events per call (no sync); ms() after a synchronize -> every call's time."""

    def __init__(self, fn):
        self.fn, self.marks = fn, []

    def __call__(self, windows, mask):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        marks[0].record()
        r = self.fn(windows, mask)
        marks[1].record()
        self.marks.append(marks)
        return r

    def ms(self):
        torch.cuda.synchronize()
        return [m[0].elapsed_time(m[1]) for m in self.marks]


def _lock_step(net, w2e, a, musical, spec):
    """The songs in lock-step reward pools of a.slots songs -> (sets, steps, reward events, seconds)."""
    torch.manual_seed(SEED)
    t = time.perf_counter()
    heads, caps, plan = _setup(net, w2e, a, musical)
    K, sets, steps, events = a.particles, [], 0, 0
    for first in range(0, a.songs, a.slots):
        rows = slice(first * K, (first + a.slots) * K)
        count = len(heads[rows]) // K
        stats = {}
        sets += generation._run_particles(net, w2e, heads[rows], caps[rows], plan.songs(first * K, count * K), K,
                                          a.every, a.ess, a.bar_cond, a.chunk, None, None, stats=stats, reward=spec)
        steps += stats["steps"]
        events += stats["reward_events"]
    return sets, steps, events, time.perf_counter() - t


def _stream(net, w2e, a, musical, spec):
    torch.manual_seed(SEED)
    t = time.perf_counter()
    heads, caps, plan = _setup(net, w2e, a, musical)
    stats = {}
    sets = generation._run_particle_stream(net, w2e, heads, caps, plan, a.songs, a.particles, a.slots, a.every, a.ess,
                                           a.bar_cond, a.chunk, None, None, stats=stats, reward=spec)
    return sets, stats, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--particles", type=int, default=4)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--ess", type=float, default=1.0)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_reward_stream_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import AIRL_model, model
    w2e = _word2event()
    n_class = [len(v) for v in w2e.values()]
    torch.manual_seed(0)
    net = model.LinearTransformer(n_class, is_training=False).cuda().eval()
    torch.manual_seed(1)
    disc = AIRL_model.LongFormer(n_class).cuda()
    reward = generation.WindowReward(disc)
    spec = generation._reward_spec(reward, a.window, a.beta)
    generation._particle_stream_refusals(a.songs, a.particles, a.slots, a.every, a.chunk, None, reward, a.window)
    B = a.every * a.window // math.gcd(a.every, a.window)
    dev = torch.cuda.get_device_name(0)
    musical = constraints(w2e)["musical"]
    torch.manual_seed(SEED)                                    # warm-up: library load, both captures, the discriminator
    for slots in (None, 2):
        generation.generate_particles(net, w2e, 4, 4, resample_every=4, ess=1.0, bar_cond=3, max_tokens=64, chunk=16,
                                      constraints=musical, slots=slots, reward=reward, reward_window=8, beta=a.beta)
    rows = min(a.songs, a.slots) * a.particles
    x = torch.zeros((rows, a.window, len(n_class)), dtype=torch.int64, device="cuda")
    reward(x, torch.ones((rows, a.window), dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    lines = []
    for rep in range(a.reps):
        lines = []

        def emit(d):
            d = dict(d, device=dev, rep=rep, songs=a.songs, particles=a.particles, slots=a.slots, resample_every=a.every,
                     reward_window=a.window, chunk=a.chunk, lcm=B, beta=a.beta, ess=a.ess)
            print(json.dumps(d), flush=True)
            lines.append(d)

        timed = _Timed(reward)
        sets, steps, events, wall = _lock_step(net, w2e, a, musical, (timed,) + spec[1:])
        ms = float(sum(timed.ms()))
        n_tok = sum(len(s) for ps in sets for s in ps.songs)
        base = {"tokens_per_s": n_tok / wall, "step_ms": 1e3 * wall / steps}
        emit({"kind": "mode", "mode": "lock_step", "seconds": wall, "tokens": n_tok, "steps": steps,
              "reward_events": events, "callable_ms_mean": ms / max(events, 1), "callable_share": 1e-3 * ms / wall,
              "mean_reward": float(np.mean(np.concatenate([r for ps in sets for r in ps.rewards]))), **base})
        longest = np.array([max(len(s) for s in ps.songs) - 1 for ps in sets], dtype=np.int64)
        pools = [longest[i:i + a.slots].max() for i in range(0, a.songs, a.slots)]
        est_lock = int(sum(-(-int(p) // a.chunk) * a.chunk for p in pools))
        est_stream = float((-(-longest // B) * B).sum()) / min(a.slots, a.songs)
        emit({"kind": "estimate", "lock_step_steps": est_lock, "stream_steps_at_least": est_stream,
              "step_ratio_at_most": est_lock / est_stream, "longest_particle_mean": float(longest.mean()),
              "longest_particle_max": int(longest.max()), "rows_scored_per_event": rows})
        del sets
        torch.cuda.empty_cache()
        timed = _Timed(reward)
        sets, st, wall = _stream(net, w2e, a, musical, (timed,) + spec[1:])
        n_tok = sum(len(s) for ps in sets for s in ps.songs)
        tps, step_ms, ms = n_tok / wall, 1e3 * wall / st["steps"], float(sum(timed.ms()))
        group_steps = st["steps"] * st["groups"]
        emit({"kind": "mode", "mode": "stream", "seconds": wall, "tokens": n_tok, "steps": st["steps"],
              "tokens_per_s": tps, "step_ms": step_ms, "ratio_tokens_per_s": tps / base["tokens_per_s"],
              "ratio_step_ms": step_ms / base["step_ms"], "events": st["events"], "graph": st["graph"],
              "reward_events": st["reward_events"], "callable_ms_mean": ms / max(st["reward_events"], 1),
              "callable_share": 1e-3 * ms / wall, "group_steps": group_steps,
              "wait_share": st["wait_group_steps"] / group_steps,
              "boundary_wait_share": st["boundary_wait_group_steps"] / group_steps,
              "idle_share": st["idle_group_steps"] / group_steps, "host_wait_seconds": st["wait_seconds"],
              "run_seconds": st["run_seconds"],
              "mean_reward": float(np.mean(np.concatenate([r for ps in sets for r in ps.rewards])))})
        del sets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

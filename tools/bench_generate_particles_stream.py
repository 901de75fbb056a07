"""Particle generation on the stream: generate_particles(slots=) against lock-step pools of the same size
on the same song indices, on the repo dims (512/12/8, f32) with the random-init model of
tools/bench_generate_constraints.py and README's constrained workload.
    python tools/bench_generate_particles_stream.py [--songs 2048] [--particles 4] [--slots 256] [--every 16]
                                                    [--ess 1.0] [--reps 2] [--out FILE]
Both modes run in this one process, alternated --reps times; the LAST repetition is written to --out (default
profiles/generate_particles_stream_bench.jsonl) as JSON lines, and every repetition is printed:
  * kind "mode", mode "lock_step": the songs in pools of --slots songs one after the other (generate()'s batch_size
    path: _run_particles on each slice of one plan); tokens/s, steps, ms per step;
  * kind "mode", mode "stream": generate_particles(slots=--slots); tokens/s, steps, ms per step, events, the
    group-steps spent waiting for a boundary and idle at the tail, its ratio to the lock-step run of the same rep, and
    run_seconds / run_step_ms: the wall time up to the last chunk read, before the host rebuilds the sets;
  * kind "estimate": what the code predicts from the lock-step run's own song lengths (each song's longest particle):
    lock-step steps = the sum over pools of the pool's longest song rounded up to the host's chunk; stream steps >= the
    sum over songs of the longest particle rounded up to --every, divided by --slots (no tail); the ratio of the two,
    the per-token cost taken as equal (the stream adds cwlt_stream_refill and cwlt_particle_advance to a token and
    drops the lock-step loop's ring copy and three counter operations)."""
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
from rlmg_amd import generation  # noqa: E402
from bench_generate_constraints import SEED, _word2event, constraints  # noqa: E402

CHUNK = 128


def _setup(net, w2e, a, musical):
    return generation._particle_setup("generate_particles", net, w2e, a.songs, a.particles, a.every, a.ess, a.bar_cond,
                                      a.max_tokens, None, "dqn", CHUNK, "blas", musical, None, None, None, None,
                                      pool=min(a.songs, a.slots))


def _lock_step(net, w2e, a, musical):
    """The songs in lock-step pools of a.slots songs -> (sets, steps, seconds)."""
    torch.manual_seed(SEED)
    t = time.perf_counter()
    heads, caps, plan = _setup(net, w2e, a, musical)
    K, sets, steps = a.particles, [], 0
    for first in range(0, a.songs, a.slots):
        rows = slice(first * K, (first + a.slots) * K)
        count = len(heads[rows]) // K
        stats = {}
        sets += generation._run_particles(net, w2e, heads[rows], caps[rows], plan.songs(first * K, count * K), K,
                                          a.every, a.ess, a.bar_cond, CHUNK, None, None, stats=stats)
        steps += stats["steps"]
    return sets, steps, time.perf_counter() - t


def _stream(net, w2e, a, musical):
    torch.manual_seed(SEED)
    t = time.perf_counter()
    heads, caps, plan = _setup(net, w2e, a, musical)
    stats = {}
    sets = generation._run_particle_stream(net, w2e, heads, caps, plan, a.songs, a.particles, a.slots, a.every, a.ess,
                                           a.bar_cond, CHUNK, None, None, stats=stats)
    return sets, stats, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--particles", type=int, default=4)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--ess", type=float, default=1.0)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_particles_stream_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    w2e = _word2event()
    torch.manual_seed(0)
    net = model.LinearTransformer([len(v) for v in w2e.values()], is_training=False).cuda().eval()
    dev = torch.cuda.get_device_name(0)
    musical = constraints(w2e)["musical"]
    torch.manual_seed(SEED)                                    # warm-up: library load, the captures of both loops
    for slots in (None, 2):
        generation.generate_particles(net, w2e, 4, 4, resample_every=4, ess=1.0, bar_cond=3, max_tokens=64, chunk=16,
                                      constraints=musical, slots=slots)
    torch.cuda.synchronize()
    lines = []
    for rep in range(a.reps):
        lines = []

        def emit(d):
            d = dict(d, device=dev, rep=rep, songs=a.songs, particles=a.particles, slots=a.slots, resample_every=a.every,
                     ess=a.ess)
            print(json.dumps(d), flush=True)
            lines.append(d)

        sets, steps, wall = _lock_step(net, w2e, a, musical)
        n_tok = sum(len(s) for ps in sets for s in ps.songs)
        base = {"tokens_per_s": n_tok / wall, "step_ms": 1e3 * wall / steps}
        emit({"kind": "mode", "mode": "lock_step", "seconds": wall, "tokens": n_tok, "steps": steps, **base})
        longest = np.array([max(len(s) for s in ps.songs) - 1 for ps in sets], dtype=np.int64)
        pools = [longest[i:i + a.slots].max() for i in range(0, a.songs, a.slots)]
        est_lock = int(sum(-(-int(p) // CHUNK) * CHUNK for p in pools))
        est_stream = float((-(-longest // a.every) * a.every).sum()) / min(a.slots, a.songs)
        emit({"kind": "estimate", "lock_step_steps": est_lock, "stream_steps_at_least": est_stream,
              "ratio_at_most": est_lock / est_stream, "longest_particle_mean": float(longest.mean()),
              "longest_particle_max": int(longest.max()), "per_token_cost": "taken as equal"})
        del sets
        torch.cuda.empty_cache()
        sets, st, wall = _stream(net, w2e, a, musical)
        n_tok = sum(len(s) for ps in sets for s in ps.songs)
        tps, step_ms = n_tok / wall, 1e3 * wall / st["steps"]
        emit({"kind": "mode", "mode": "stream", "seconds": wall, "tokens": n_tok, "steps": st["steps"],
              "tokens_per_s": tps, "step_ms": step_ms, "ratio_tokens_per_s": tps / base["tokens_per_s"],
              "ratio_step_ms": step_ms / base["step_ms"], "events": st["events"], "graph": st["graph"],
              "wait_group_steps": st["wait_group_steps"], "idle_group_steps": st["idle_group_steps"],
              "group_steps": st["steps"] * st["groups"], "host_wait_seconds": st["wait_seconds"],
              "run_seconds": st["run_seconds"], "run_step_ms": 1e3 * st["run_seconds"] / st["steps"],
              "moved_rows_per_event": float(np.mean(st["moved_rows"])) if st["moved_rows"] else 0.0})
        del sets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

"""Particle generation: generate_particles against generate_batch on the same rows, on the repo dims
(512/12/8, f32) with the random-init model of tools/bench_generate_constraints.py and README's constrained workload (a
fixed tempo, a pitch range and a cycled 4-chord progression).
    python tools/bench_generate_particles.py [--songs 64] [--particles 4] [--every 16] [--reps 2] [--out FILE]
Writes JSON lines to --out (default profiles/generate_particles_bench.jsonl) and prints them:
  * kind "mode": tokens/s and ms per lock-step token of generate_batch(songs x particles, the constraints,
    return_logprobs=True) -- unchanged by particle generation, the yardstick -- and of generate_particles(songs,
    particles, resample_every=--every) at ess 0.5 and 1.0, alternated --reps times in this one process, and each
    particle run's ratio to the batch run of the same rep; the share of (event, song) pairs that resampled;
  * kind "weigh": the HIP-event time of one cwlt_particle_weigh launch on the pool's rows;
  * kind "events": a timed run at each ess: per event the HIP-event milliseconds of cwlt_particle_resample and of
    each gather phase (all families), the payload bytes a phase copied (moved rows x bytes per row; the traffic is
    twice that, a read and a write) and its GB/s -- mean and the largest event."""
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


def _particles(net, w2e, a, ess, musical, timed=False):
    """One generate_particles run through its parts, so that the loop's stats come back -> (sets, stats, seconds)."""
    torch.manual_seed(SEED)
    t = time.perf_counter()
    heads, caps, plan = generation._particle_setup(
        "generate_particles", net, w2e, a.songs, a.particles, a.every, ess, a.bar_cond, a.max_tokens, None, "dqn", 128,
        "blas", musical, None, None, None, None)
    stats = {"timed": timed}
    sets = generation._run_particles(net, w2e, heads, caps, plan, a.particles, a.every, ess, a.bar_cond, 128, None,
                                     None, stats=stats)
    return sets, stats, time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--particles", type=int, default=4)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_particles_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    w2e = _word2event()
    n_class = [len(v) for v in w2e.values()]
    torch.manual_seed(0)
    net = model.LinearTransformer(n_class, is_training=False).cuda().eval()
    dev = torch.cuda.get_device_name(0)
    musical = constraints(w2e)["musical"]
    rows = a.songs * a.particles
    torch.manual_seed(SEED)                                    # warm-up: library load, the captures of both loops
    generation.generate_batch(net, w2e, 8, bar_cond=3, max_tokens=64, constraints=musical, return_logprobs=True)
    generation.generate_particles(net, w2e, 2, 4, resample_every=4, ess=1.0, bar_cond=3, max_tokens=64,
                                  constraints=musical)
    torch.cuda.synchronize()
    lines = []

    def emit(d):
        d = dict(d, device=dev, songs=a.songs, particles=a.particles, rows=rows, resample_every=a.every)
        print(json.dumps(d), flush=True)
        lines.append(d)

    for rep in range(a.reps):
        torch.manual_seed(SEED)
        t = time.perf_counter()
        songs, _ = generation.generate_batch(net, w2e, rows, bar_cond=a.bar_cond, max_tokens=a.max_tokens,
                                             constraints=musical, return_logprobs=True)
        wall = time.perf_counter() - t
        n_tok = sum(len(s) for s in songs)
        steps = max(len(s) for s in songs) - 1
        base = {"tokens_per_s": n_tok / wall, "step_ms": 1e3 * wall / steps}
        emit({"kind": "mode", "mode": "generate_batch", "rep": rep, "seconds": wall, "tokens": n_tok, "steps": steps,
              **base})
        torch.cuda.empty_cache()
        for ess in (0.5, 1.0):
            sets, st, wall = _particles(net, w2e, a, ess, musical)
            n_tok = sum(len(s) for ps in sets for s in ps.songs)
            tps, step_ms = n_tok / wall, 1e3 * wall / st["steps"]
            emit({"kind": "mode", "mode": "generate_particles", "ess": ess, "rep": rep, "seconds": wall,
                  "tokens": n_tok, "steps": st["steps"], "tokens_per_s": tps, "step_ms": step_ms,
                  "ratio_tokens_per_s": tps / base["tokens_per_s"], "ratio_step_rate": base["step_ms"] / step_ms,
                  "events": st["events"], "graph": st["graph"],
                  "resampled_share": sum(st["resampled_groups"]) / max(1, st["events"] * st["groups"]),
                  "moved_rows_per_event": float(np.mean(st["moved_rows"])) if st["moved_rows"] else 0.0,
                  "mean_log_evidence": float(np.mean([ps.log_evidence for ps in sets]))})
            del sets
            torch.cuda.empty_cache()
    # one weigh launch, by HIP events around a run of launches on buffers of the pool's size
    cuda = torch.device("cuda")
    logp = torch.zeros((128, rows, 6, 2), dtype=torch.float32, device=cuda)
    cnt = torch.zeros(1, dtype=torch.int64, device=cuda)
    bar, cap = torch.ones(rows, dtype=torch.int64, device=cuda), torch.full((rows,), 1 << 40, device=cuda)
    lw = torch.zeros(rows, dtype=torch.float32, device=cuda)
    length, done = (torch.zeros(rows, dtype=torch.int64, device=cuda) for _ in range(2))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for n in (50, 1000):                                       # the first run warms up
        ev[0].record()
        for _ in range(n):
            ops.particle_weigh(logp, cnt, bar, a.bar_cond, cap, lw, length, done)
        ev[1].record()
        torch.cuda.synchronize()
    emit({"kind": "weigh", "launches": n, "us_per_launch": 1e3 * ev[0].elapsed_time(ev[1]) / n,
          "note": "eager launches back to back: launch-bound; inside the captured token the kernel itself is shorter"})
    for ess in (0.5, 1.0):
        _, st, _ = _particles(net, w2e, a, ess, musical, timed=True)
        ms = np.asarray(st["event_ms"], dtype=np.float64).reshape(-1, 3)
        moved = np.asarray(st["moved_rows"], dtype=np.float64)
        payload = moved * st["row_bytes"]
        hit = moved > 0
        gbs = lambda col: (payload[hit] / (ms[hit, col] * 1e-3) / 1e9) if hit.any() else np.zeros(1)
        big = int(moved.argmax()) if len(moved) else 0
        emit({"kind": "events", "ess": ess, "events": st["events"], "events_that_moved_rows": int(hit.sum()),
              "row_bytes": st["row_bytes"], "resample_ms_mean": float(ms[:, 0].mean()),
              "phase1_ms_mean_moved": float(ms[hit, 1].mean()) if hit.any() else 0.0,
              "phase2_ms_mean_moved": float(ms[hit, 2].mean()) if hit.any() else 0.0,
              "phase_ms_mean_unmoved": float(ms[~hit, 1:].mean()) if (~hit).any() else 0.0,
              "payload_bytes_mean_moved": float(payload[hit].mean()) if hit.any() else 0.0,
              "phase1_payload_gb_per_s_mean": float(gbs(1).mean()), "phase2_payload_gb_per_s_mean": float(gbs(2).mean()),
              "largest_event": {"moved_rows": int(moved[big]) if len(moved) else 0,
                                "payload_bytes": float(payload[big]) if len(moved) else 0.0,
                                "resample_ms": float(ms[big, 0]) if len(ms) else 0.0,
                                "phase1_ms": float(ms[big, 1]) if len(ms) else 0.0,
                                "phase2_ms": float(ms[big, 2]) if len(ms) else 0.0},
              "event_ms_total": float(ms.sum()), "steps": st["steps"]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

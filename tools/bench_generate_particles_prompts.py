"""Per-song prompts with particles: generate_particles(slots=, prompts=[...], bank="auto") against
lock-step pools of the same size on the same songs, on the repo dims (512/12/8, f32) with the random-init model of
tools/bench_generate_constraints.py and README's constrained workload; every song continues its own prompt of 64-512
rows (no Bar after the first row, as tools/bench_generate_prompts.py draws them) to bar 17.
    python tools/bench_generate_particles_prompts.py [--songs 2048] [--particles 4] [--slots 256] [--every 16]
                                                     [--ess 1.0] [--reps 2] [--out FILE] [--only-kernels]
The three modes run in this one process, --reps times; the LAST repetition is written to --out (default
profiles/generate_particles_prompts_bench.jsonl) as JSON lines, and every repetition is printed:
  * kind "mode", mode "lock_step": pools of --slots songs one after the other with prefill="gemm" and
    share_prefill=False, every prompt prefilled K times -- the behaviour before the shared prefill, the baseline;
  * kind "mode", mode "lock_step_shared": the same pools with share_prefill=True, each prompt prefilled once;
  * kind "mode", mode "stream": generate_particles(slots=--slots, bank="auto"); its ratios to both pools, the prefill's
    GPU seconds, the gated chunks and the group-steps parked by the gate;
  * kind "estimate": the step counts from the run's own lengths (each song's longest particle), as
    tools/bench_generate_particles_stream.py records them;
  * kind "check": how many particles' songs of the shared pools, and of the stream within the first pool's songs (a
    later pool takes a seed of its own), differ from the baseline's (must be 0).
--only-kernels: microseconds of cwlt_particle_refill_bank against cwlt_stream_refill_bank fed the per-row song array
id // K, at --slots groups of --particles rows with nothing fresh, 8 groups fresh and all groups fresh; and of
cwlt_particle_release_bank against cwlt_particle_release with 8 candidate groups (kind "kernels"; written to
profiles/generate_particles_prompts_kernels.jsonl by default)."""
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

CHUNK = 128


def _prompts(w2e, n, lo, hi, seed=0):
    """n random prompts of lo .. hi rows with no Bar after the first row: every song starts at bar count 1."""
    rng = np.random.default_rng(seed)
    n_class = [len(v) for v in w2e.values()]
    names = w2e["bar-beat"]
    plain = next(i for i in range(n_class[2]) if names[i] != "Bar")
    is_bar = np.array([names[i] == "Bar" for i in range(n_class[2])])
    out = []
    for L in rng.integers(lo, hi + 1, n):
        p = np.stack([rng.integers(0, c, L) for c in n_class], 1).astype(np.int64)
        p[1:, 2] = np.where(is_bar[p[1:, 2]], plain, p[1:, 2])
        out.append(p)
    return out


def _setup(net, w2e, a, musical, prompts):
    return generation._particle_setup("generate_particles", net, w2e, a.songs, a.particles, a.every, a.ess, a.bar_cond,
                                      a.max_tokens, prompts, "dqn", CHUNK, "gemm", musical, None, None, None, None,
                                      pool=min(a.songs, a.slots))


def _lock_step(net, w2e, a, musical, prompts, share):
    """The songs in lock-step pools of a.slots songs -> (sets, steps, prompts prefilled, seconds)."""
    torch.manual_seed(SEED)
    t = time.perf_counter()
    heads, caps, plan = _setup(net, w2e, a, musical, prompts)
    K, sets, steps, prefilled = a.particles, [], 0, 0
    for first in range(0, a.songs, a.slots):
        rows = slice(first * K, (first + a.slots) * K)
        count = len(heads[rows]) // K
        stats = {}
        sets += generation._run_particles(net, w2e, heads[rows], caps[rows], plan.songs(first * K, count * K), K,
                                          a.every, a.ess, a.bar_cond, CHUNK, None, "gemm", stats=stats,
                                          share_prefill=share)
        steps += stats["steps"]
        prefilled += stats["prefilled_prompts"]
    return sets, steps, prefilled, time.perf_counter() - t


def _stream(net, w2e, a, musical, prompts):
    torch.manual_seed(SEED)
    t = time.perf_counter()
    heads, caps, plan = _setup(net, w2e, a, musical, prompts)
    stats = {}
    sets = generation._run_particle_stream(net, w2e, heads, caps, plan, a.songs, a.particles, a.slots, a.every, a.ess,
                                           a.bar_cond, CHUNK, None, heads[0], stats=stats, bank="auto")
    return sets, stats, time.perf_counter() - t


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3


def _kernels(net, a, emit, reps=200):
    enc = net.transformer_encoder
    n_layer, H = len(enc.layers), enc.layers[0].attention.n_heads
    d = net.d_model // H
    sf, zf, W = H * d * d, H * d, sum(net.n_token)
    dev = net.in_linear.weight.device
    G, K = a.slots, a.particles
    rows, bank = G * K, 2 * G
    state = torch.zeros(n_layer * rows * (sf + zf), device=dev)
    bstate = torch.zeros(n_layer * bank * (sf + zf), device=dev)
    logits, blogits = torch.zeros(rows, W, device=dev), torch.zeros(bank, W, device=dev)
    pid = torch.arange(rows, dtype=torch.int64, device=dev)
    song = torch.div(pid, K, rounding_mode="floor")
    for name, n_fresh in (("nothing fresh", 0), ("8 groups fresh", 8), ("all groups fresh", G)):
        fresh = (song % max(1, G // max(1, n_fresh)) == 0).to(torch.int64) if 0 < n_fresh < G else \
            torch.full((rows,), int(n_fresh > 0), dtype=torch.int64, device=dev)
        groups = int(fresh.sum().item()) // K
        new = _timed(lambda: ops.particle_refill_bank(state, bstate, n_layer, sf, zf, logits, blogits, fresh, pid, K),
                     reps)
        old = _timed(lambda: ops.stream_refill_bank(state, bstate, n_layer, sf, zf, logits, blogits, fresh, song), reps)
        emit({"kind": "kernels", "pair": "refill", "pattern": name, "fresh_groups": groups, "rows": rows, "bank": bank,
              "particle_refill_bank_us": new, "stream_refill_bank_us": old, "ratio": old / new,
              "entry_bytes": 4 * n_layer * (sf + zf)})
    i64 = lambda v: torch.full((rows,), v, dtype=torch.int64, device=dev)                # noqa: E731
    n_songs = 4 * G
    gsong = torch.arange(G, dtype=torch.int64, device=dev)
    done = (song % (G // 8) == 0).to(torch.int64) if G >= 8 else i64(1)
    arrays = lambda: (gsong.clone(), pid.clone(), i64(0), i64(1), i64(9), i64(0), done.clone(), i64(0),     # noqa: E731
                      torch.zeros(rows, device=dev), torch.zeros(G, device=dev))
    outs = (torch.zeros(n_songs * K, device=dev), torch.zeros(n_songs * K, dtype=torch.int64, device=dev),
            torch.zeros(n_songs, device=dev))
    # the candidates are parked by both (no song left / none ready), so every call sees the same candidates
    plain, ctl3 = arrays(), torch.tensor([0, n_songs, 0], dtype=torch.int64, device=dev)
    old = _timed(lambda: ops.particle_release(K, n_songs, 1, 9, *plain, ctl3, *outs), reps)
    gated, ctl4 = arrays(), torch.tensor([0, G, 0, 0], dtype=torch.int64, device=dev)
    b0, cp = torch.ones(n_songs, dtype=torch.int64, device=dev), torch.full((n_songs,), 9, dtype=torch.int64, device=dev)
    new = _timed(lambda: ops.particle_release_bank(K, n_songs, b0, cp, *gated, ctl4, *outs), reps)
    emit({"kind": "kernels", "pair": "release", "groups": G, "candidates": int(done.view(G, K)[:, 0].sum().item()),
          "particle_release_bank_us": new, "particle_release_us": old, "ratio": old / new})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--particles", type=int, default=4)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--ess", type=float, default=1.0)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "generate_particles_prompts_%s.jsonl"
                             % ("kernels" if a.only_kernels else "bench"))
    from rlmg_amd.dqn_policy import model
    w2e = _word2event()
    torch.manual_seed(0)
    net = model.LinearTransformer([len(v) for v in w2e.values()], is_training=False).cuda().eval()
    dev = torch.cuda.get_device_name(0)
    lines = []

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")

    if a.only_kernels:
        def emit(d):
            d = dict(d, device=dev, particles=a.particles, slots=a.slots)
            print(json.dumps(d), flush=True)
            lines.append(d)
        _kernels(net, a, emit)
        return write()
    musical = constraints(w2e)["musical"]
    prompts = _prompts(w2e, a.songs, 64, 512)
    n_prompt = sum(len(p) for p in prompts)
    torch.manual_seed(SEED)                                    # warm-up: library load, the captures of both loops
    for kw in (dict(prefill="gemm"), dict(slots=2, bank="auto")):
        generation.generate_particles(net, w2e, 4, 4, resample_every=4, ess=1.0, bar_cond=3, max_tokens=600, chunk=16,
                                      constraints=musical, prompts=prompts[:4], **kw)
    torch.cuda.synchronize()
    K = a.particles
    for rep in range(a.reps):
        lines = []

        def emit(d):
            d = dict(d, device=dev, rep=rep, songs=a.songs, particles=K, slots=a.slots, resample_every=a.every,
                     ess=a.ess, prompt_rows=n_prompt)
            print(json.dumps(d), flush=True)
            lines.append(d)

        base, want = {}, None
        for mode, share in (("lock_step", False), ("lock_step_shared", True)):
            sets, steps, prefilled, wall = _lock_step(net, w2e, a, musical, prompts, share)
            drawn = sum(len(s) for ps in sets for s in ps.songs) - K * n_prompt
            base[mode] = {"drawn_per_s": drawn / wall, "seconds": wall}
            emit({"kind": "mode", "mode": mode, "seconds": wall, "drawn": drawn, "steps": steps,
                  "prefilled_prompts": prefilled, "drawn_per_s": drawn / wall,
                  **({} if not share else {"ratio_to_lock_step": base["lock_step"]["seconds"] / wall})})
            songs = [s for ps in sets for s in ps.songs]
            if want is None:
                want = songs
                longest = np.array([max(len(s) - len(h) for s in ps.songs) for ps, h in zip(sets, prompts)],
                                   dtype=np.int64)
                pools = [longest[i:i + a.slots].max() for i in range(0, a.songs, a.slots)]
                est_lock = int(sum(-(-int(p) // CHUNK) * CHUNK for p in pools))
                est_stream = float((-(-longest // a.every) * a.every).sum()) / min(a.slots, a.songs)
                emit({"kind": "estimate", "lock_step_steps": est_lock, "stream_steps_at_least": est_stream,
                      "ratio_at_most": est_lock / est_stream, "longest_particle_mean": float(longest.mean()),
                      "longest_particle_max": int(longest.max()), "per_token_cost": "taken as equal, prefill left out"})
            else:
                differ = sum(not (x.shape == y.shape and (x == y).all()) for x, y in zip(songs, want))
                emit({"kind": "check", "mode": mode, "songs_differing_from_lock_step": int(differ)})
            del sets, songs
            torch.cuda.empty_cache()
        sets, st, wall = _stream(net, w2e, a, musical, prompts)
        drawn = sum(len(s) for ps in sets for s in ps.songs) - K * n_prompt
        emit({"kind": "mode", "mode": "stream", "seconds": wall, "drawn": drawn, "steps": st["steps"],
              "drawn_per_s": drawn / wall, "ratio_to_lock_step": base["lock_step"]["seconds"] / wall,
              "ratio_to_lock_step_shared": base["lock_step_shared"]["seconds"] / wall, "events": st["events"],
              "graph": st["graph"], "block": st["block"], "bank": st["bank"], "prefill_blocks": st["prefill_blocks"],
              "prefill_seconds": st["prefill_seconds"], "prefill_share": st["prefill_seconds"] / wall,
              "gated_chunks": st["gated_chunks"], "gate_wait_group_steps": st["gate_wait_group_steps"],
              "wait_group_steps": st["wait_group_steps"], "idle_group_steps": st["idle_group_steps"],
              "group_steps": st["steps"] * st["groups"], "host_wait_seconds": st["wait_seconds"],
              "run_seconds": st["run_seconds"], "step_ms": 1e3 * st["run_seconds"] / st["steps"]})
        songs = [s for ps in sets for s in ps.songs]
        # a pool takes a seed of its own and keys its draws by the row in the pool: only the first pool's songs are the
        # stream's
        first = min(a.slots, a.songs) * K
        differ = sum(not (x.shape == y.shape and (x == y).all()) for x, y in zip(songs[:first], want[:first]))
        emit({"kind": "check", "mode": "stream", "first_pool_particles": first,
              "first_pool_particles_differing_from_lock_step": int(differ)})
        del sets, songs, want
        torch.cuda.empty_cache()
    write()


if __name__ == "__main__":
    main()

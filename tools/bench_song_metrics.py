"""Song metrics on the device: what they cost as an evaluation and as a reward.
    python tools/bench_song_metrics.py [--eval-songs 2048] [--eval-rows 1024] [--songs 64] [--particles 4] [--every 10]
                                       [--window 50] [--chunk 100] [--reps 5] [--out FILE]
Two measurements, written to --out (default profiles/song_metrics_bench.jsonl) as JSON lines:
  * kind "evaluation": generation.song_metrics on --eval-songs Grammar-shaped random songs of --eval-rows rows (one
    (N, L, 6) array) -- the whole call with its upload and read-back, and the cwlt_song_metrics launch alone between two
    HIP events -- against sampling.song_metrics_f32 on the host, and whether the two agree bit for bit;
  * kind "reward": README's constrained workload (the musical constraint, 512/12/8 policy, random init) as a lock-step
    pool of --songs songs x --particles particles, run three ways in this one process, alternated --reps times (the last
    repetition is kept): without a reward, with MetricReward, and with WindowReward on the repo-dims discriminator
    (512/10/8, random init); tokens/s each, the ratio to the run without a reward of the same repetition, and the
    callable's own time from a pair of HIP events around every call (no sync) with its share of the run;
  * kind "summary": per reward the median over the repetitions of tokens/s and of both ratios, and the spread
    (max / min - 1) of the tokens/s of the run without a reward -- a run lasts about a second, so single ratios move by
    that spread.

Estimates, written before the first run:
  * evaluation: 2 048 x 1 024 rows x 48 B = 101 MB of tokens; the kernel reads three of the six columns once, in 256-thread
    workgroups, four strides per song, and then sums at most a few dozen slots per song on one thread: 100-200 us, far
    from any roof and still 4-5 orders of magnitude under the host's ~10 s (numpy, a Python loop per song).  The whole
    call is the 101 MB host-to-device copy: 10-20 ms, about 500 x the host.
  * reward: per reward event the window and apply launches take 11.5 us and 6.6 us; MetricReward adds one launch of
    about 10 us (256 windows of 50 rows, a wave each, 64 workgroups) every 50 tokens of ~2 ms each, under 0.1 % of the
    run: >= 0.97 x the tokens/s of the run without a reward (expected 0.99-1.00 x; the three runs resample differently,
    so their songs differ and so does the token count).  WindowReward costs 11-14 % of a run: 0.86-0.89 x."""
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
from rlmg_amd import generation, metrics, ops, sampling  # noqa: E402
from bench_generate_constraints import SEED, _word2event, constraints  # noqa: E402

TERMS = {"in_chord": 1.0, "groove": 0.5, "h1": 0.25, "empty_bars": -1.0}


class _Timed:
    """A reward callable between two HIP events per call (no sync); ms() after a synchronize -> every call's time."""

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


def _songs(rng, N, L):
    """Grammar-shaped random songs: a Bar about every 24 rows, ascending beats (a chord on some), notes after a beat."""
    tok = np.zeros((N, L, 6), dtype=np.int64)
    u = rng.random((N, L))
    kind = np.where(u < 1 / 24, 0, np.where(u < 1 / 24 + 0.2, 1, 2))         # Bar, Beat, note
    kind[:, 0] = 0
    tok[:, :, 2] = np.where(kind == 0, 1, np.where(kind == 1, 2 + rng.integers(0, 16, (N, L)), 0))
    tok[:, :, 1] = np.where(kind == 1, np.where(rng.random((N, L)) < 0.5, 1, rng.integers(2, 135, (N, L))), 0)
    tok[:, :, 3] = np.where(kind == 2, rng.integers(1, 87, (N, L)), 0)
    return tok


def evaluation(a, spec, dev):
    rng = np.random.default_rng(SEED)
    tok = _songs(rng, a.eval_songs, a.eval_rows)
    generation.song_metrics(spec, tok[:4])                                  # library load, table upload
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = generation.song_metrics(spec, tok)
    call = time.perf_counter() - t
    mb = out["hist"].shape[1]
    N, L, _ = tok.shape
    order, pitch, chord, table = spec.tables("cuda", L + 1)
    d_tok = torch.from_numpy(tok).cuda()
    feat = torch.empty(N, 11, dtype=torch.float32, device="cuda")
    bars = torch.empty(N, dtype=torch.int32, device="cuda")
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    us = []
    for _ in range(6):
        marks[0].record()
        ops.song_metrics(d_tok, None, None, spec.attrs, order, pitch, chord, spec.Q, table, mb, feat, bars=bars)
        marks[1].record()
        torch.cuda.synchronize()
        us.append(1e3 * marks[0].elapsed_time(marks[1]))
    t = time.perf_counter()
    ref = sampling.song_metrics_f32(tok, None, None, spec, max_bars=mb)
    host = time.perf_counter() - t
    same = bool(np.array_equal(np.stack([out[k] for k in metrics.METRICS], 1).view(np.int32), ref["feat"].view(np.int32))
                and np.array_equal(out["hist"], ref["hist"]) and np.array_equal(out["groove_masks"], ref["groove"]))
    return {"kind": "evaluation", "device": dev, "songs": N, "rows": L, "max_bars": mb, "call_ms": 1e3 * call,
            "kernel_us_median": float(np.median(us[1:])), "host_f32_s": host, "host_over_call": host / call,
            "bitwise_equal": same, "mean_h1": float(out["h1"].mean()), "mean_h4": float(out["h4"].mean()),
            "mean_groove": float(out["groove"].mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval-songs", type=int, default=2048)
    ap.add_argument("--eval-rows", type=int, default=1024)
    ap.add_argument("--songs", type=int, default=64)
    ap.add_argument("--particles", type=int, default=4)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--ess", type=float, default=1.0)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "song_metrics_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import AIRL_model, model
    w2e = _word2event()
    spec = metrics.SongMetricSpec(w2e)
    dev = torch.cuda.get_device_name(0)
    lines = [evaluation(a, spec, dev)]
    print(json.dumps(lines[0]), flush=True)

    n_class = [len(v) for v in w2e.values()]
    torch.manual_seed(0)
    net = model.LinearTransformer(n_class, is_training=False).cuda().eval()
    torch.manual_seed(1)
    disc = AIRL_model.LongFormer(n_class).cuda()
    musical = constraints(w2e)["musical"]
    rewards = {"none": None, "metric": generation.MetricReward(spec, TERMS), "window": generation.WindowReward(disc)}

    def run(reward, songs, **kw):
        torch.manual_seed(SEED)
        torch.cuda.synchronize()
        t = time.perf_counter()
        sets = generation.generate_particles(net, w2e, songs, a.particles, constraints=musical, reward=reward,
                                             beta=a.beta, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        return sets, wall

    for reward in rewards.values():                                         # warm-up: captures, the discriminator
        run(reward, 4, resample_every=4, ess=1.0, bar_cond=3, max_tokens=64, chunk=16, reward_window=8)
    kw = dict(resample_every=a.every, ess=a.ess, bar_cond=a.bar_cond, max_tokens=a.max_tokens, chunk=a.chunk,
              reward_window=a.window)
    last, every = [], {name: [] for name in rewards}
    for rep in range(a.reps):
        last, base = [], None
        for name, reward in rewards.items():
            timed = None if reward is None else _Timed(reward)
            sets, wall = run(timed, a.songs, **kw)
            n_tok = sum(len(s) for ps in sets for s in ps.songs)
            steps = max(len(s) for ps in sets for s in ps.songs) - 1
            d = {"kind": "reward", "reward": name, "device": dev, "rep": rep, "songs": a.songs, "particles": a.particles,
                 "resample_every": a.every, "reward_window": a.window, "chunk": a.chunk, "ess": a.ess, "beta": a.beta,
                 "seconds": wall, "tokens": n_tok, "longest_song": steps, "tokens_per_s": n_tok / wall,
                 "step_ms": 1e3 * wall / steps}
            if reward is not None:
                d["mean_reward"] = float(np.mean(np.concatenate([r for ps in sets for r in ps.rewards])))
                d["ratio_tokens_per_s"] = d["tokens_per_s"] / base
                d["ratio_step_ms"] = d["step_ms"] / base_step
                ms = timed.ms()
                d.update(reward_events=len(ms), callable_us_median=1e3 * float(np.median(ms)),
                         callable_share=1e-3 * float(sum(ms)) / wall)
            else:
                base, base_step = d["tokens_per_s"], d["step_ms"]
            print(json.dumps(d), flush=True)
            last.append(d)
            every[name].append(d)
            del sets
            torch.cuda.empty_cache()
    med = lambda name, key: float(np.median([d[key] for d in every[name]]))                      # noqa: E731
    none = [d["tokens_per_s"] for d in every["none"]]
    summary = {"kind": "summary", "device": dev, "reps": a.reps, "none_tokens_per_s_median": med("none", "tokens_per_s"),
               "none_tokens_per_s_spread": max(none) / min(none) - 1.0}
    for name in ("metric", "window"):
        for key in ("tokens_per_s", "ratio_tokens_per_s", "ratio_step_ms", "callable_us_median", "callable_share"):
            summary["%s_%s_median" % (name, key)] = med(name, key)
        summary["%s_ratio_tokens_per_s_min" % name] = min(d["ratio_tokens_per_s"] for d in every[name])
    print(json.dumps(summary), flush=True)
    last.append(summary)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines + last:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

"""Padded against packed pretrain step at repo dims (12 layers, d_model 512, 8 heads, d_ff 2048), bf16, dropout on.

Synthetic songs with lengths uniform in [T / 4, T] at T = 1024, enough of them for about 512 k padded rows.  Two
configurations are timed interleaved, in one process:
    padded   net.train_step on the (N, T) batch with its loss mask
    packed   net.train_step_packed on the same songs laid end to end (data.pack_songs, longest first)
and then the same pair with every song at full length (fill 1.0), where the two do the same work.  A step is forward,
backward, gradient clipping and Adam, as in bench.py.  One JSON line per run is appended to --out
(profiles/pretrain_packed_bench.jsonl): ms per step (mean and every repeat), live tokens per second, the fill fraction, the
scan's share of the step (HIP events around every C-ABI call of one extra step), the longest and the mean song of the
launch.  The estimate this is measured against is in DESIGN.md section 4.1 (packed time ~ fill x padded time).

    python tools/bench_pretrain_packed.py [--songs 512] [--steps 5] [--repeats 3] [--out FILE]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_CLASS = [56, 135, 18, 87, 18, 25]
FIXED_MS = 3.0     # the part of a step the estimate takes as not shrinking with the rows


def make_songs(n, T, full, seed):
    rng = np.random.default_rng(seed)
    lengths = np.full(n, T) if full else rng.integers(T // 4, T + 1, n)
    x = np.stack([rng.integers(0, c, (n, T)) for c in N_CLASS], -1).astype(np.int64)
    y = np.stack([rng.integers(0, c, (n, T)) for c in N_CLASS], -1).astype(np.int64)
    mask = (np.arange(T)[None, :] < lengths[:, None]).astype(np.float32)
    return x, y, mask, lengths


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=512)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--pad-rows-to", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_packed_bench.jsonl"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the cwlt hot path has no CPU implementation")

    import rlmg_amd  # noqa: F401
    from rlmg_amd import data as cwdata, dist as rdist, gemm_tuning, ops
    from rlmg_amd.dqn_policy import config, model

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gemm_tuning.enable()
    torch.manual_seed(0)
    old = dict(config.AgentConfig)
    config.AgentConfig.update({"D_MODEL": 512, "N_LAYER": args.layers, "N_HEAD": 8})
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            net = model.LinearTransformer(N_CLASS)
    finally:
        config.AgentConfig.update(old)
    net = net.to(dev).train()
    net.compute_dtype = torch.bfloat16
    sync = rdist.GradSync(net.parameters())
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, fused=True)

    def finish(losses):
        loss = (losses[0] + losses[1] + losses[2] + losses[3] + losses[4] + losses[5]) / 6
        loss.backward()
        sync.finish()
        sync.clip_grad_norm_(3.0)
        opt.step()
        return loss

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps, float(loss.item())

    def scan_share(step):
        ops.KernelTimer.reset(False)
        ops.KernelTimer.reserve(1024)
        torch.cuda.synchronize()
        ops.KernelTimer.enabled = True
        step()
        ops.KernelTimer.enabled = False
        torch.cuda.synchronize()
        kt = ops.KernelTimer.summary()
        ops.KernelTimer.reset(False)
        total = sum(c * ms for c, ms, _ in kt.values())
        scan = sum(c * ms for n, (c, ms, _) in kt.items() if n.startswith("cwlt_causal_linear"))
        return scan / total, scan, total

    lines = []
    for case, full in (("ragged", False), ("full", True)):
        x, y, mask, lengths = make_songs(args.songs, args.seq, full, 1234)
        xd, yd, md = (torch.from_numpy(a).to(dev) for a in (x, y, mask))
        batch = cwdata.pack_songs(x, y, mask, range(args.songs), pad_rows_to=args.pad_rows_to, device=dev)
        live = int(lengths.sum())
        fill = live / (args.songs * args.seq)

        def padded():
            sync.zero_grad()
            return finish(net.train_step(xd, yd, md))

        def packed():
            sync.zero_grad()
            return finish(net.train_step_packed(batch))

        steps = {"padded": padded, "packed": packed}
        for name in steps:
            for _ in range(args.warmup):
                steps[name]()
        runs = {"padded": [], "packed": []}
        loss = {}
        for _ in range(args.repeats):                       # interleaved: padded, packed, padded, packed, ...
            for name in ("padded", "packed"):
                ms, loss[name] = timed(steps[name])
                runs[name].append(ms)
        for name in ("padded", "packed"):
            share, scan_ms, kernel_ms = scan_share(steps[name])
            ms = sum(runs[name]) / len(runs[name])
            rows = args.songs * args.seq if name == "padded" else batch.rows
            lines.append({"tool": "bench_pretrain_packed", "case": case, "config": name, "dtype": "bf16", "dropout": 0.1,
                          "layers": args.layers, "songs": args.songs, "T": args.seq, "rows": rows, "live_tokens": live,
                          "fill": round(fill, 4), "ms_per_step": round(ms, 3),
                          "ms_per_step_runs": [round(v, 3) for v in runs[name]], "steps_per_run": args.steps,
                          "live_tokens_per_s": round(live / (ms * 1e-3)), "scan_share": round(share, 4),
                          "scan_ms": round(scan_ms, 3), "kernel_ms": round(kernel_ms, 3),
                          "longest_song": int(lengths.max()), "mean_song": round(float(lengths.mean()), 1),
                          "loss": round(loss[name], 4),
                          "hbm_peak_gb": round(torch.cuda.max_memory_allocated() / 1e9, 1)})
        pad_ms, pack_ms = (sum(runs[k]) / len(runs[k]) for k in ("padded", "packed"))
        spread = (max(runs["padded"]) - min(runs["padded"])) / pad_ms
        # DESIGN 4.1.1's estimate, written before the first run: the step is row-proportional but for about 3 ms
        # (optimizer, clipping, weight casts), so packed / padded ~ (fill x (padded - 3 ms) + 3 ms) / padded
        estimate = (fill * (pad_ms - FIXED_MS) + FIXED_MS) / pad_ms
        lines.append({"tool": "bench_pretrain_packed", "case": case, "config": "ratio", "fill": round(fill, 4),
                      "packed_over_padded": round(pack_ms / pad_ms, 4), "estimate": round(estimate, 4),
                      "padded_run_spread": round(spread, 4)})
        del xd, yd, md, batch
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            s = json.dumps(line)
            print(s, flush=True)
            f.write(s + "\n")


if __name__ == "__main__":
    main()

"""Prompt prefill at the repo dims (512/12/8, f32): DecodeSession.prefill against feeding the same prompt through
DecodeSession.step (captured graph on), for one song and a batch of songs.
    python tools/bench_prefill.py [--lengths 64 256 1024 3584] [--songs 1 8] [--reps 5]
Prints one JSON line per (songs, prompt length): prefill ms (median of --reps), prompt tokens/s, the step loop's ms,
their ratio, the scan's share of the prefill (HIP events around every ops.cla_fwd_state call, in a separate timed
run), the scan's segment count (cwlt_prefill_segments) and the worst |logit| difference between the two paths."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rlmg_amd  # noqa: E402,F401
from rlmg_amd import _lib, generation, ops  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="*", default=[64, 256, 1024, 3584])
    ap.add_argument("--songs", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefill measures on the GPU; none found")
    from rlmg_amd.dqn_policy import model
    n_class = [56, 135, 18, 87, 18, 25]
    torch.manual_seed(0)
    net = model.LinearTransformer(n_class, is_training=False).cuda().eval()
    assert net.compute_dtype == torch.float32
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    for n in a.songs:
        pre = generation.DecodeSession(net, graph=True, n_songs=n)
        step = generation.DecodeSession(net, graph=True, n_songs=n)
        for P in a.lengths:
            toks = torch.stack([torch.randint(0, c, (n, P), generator=g) for c in n_class], -1).numpy()
            prompt = toks[0] if n == 1 else toks
            for _ in range(2):                                   # warm-up: code objects, GEMM algorithm choice
                pre.reset()
                pre.prefill(prompt)
            runs = []
            for _ in range(a.reps):
                pre.reset()
                ms, got = timed(lambda: pre.prefill(prompt))
                runs.append(ms)
            got = np.array(got, copy=True)
            pre_ms = float(np.median(runs))
            # the scan's share: HIP events around each cwlt_causal_linear_fwd_state launch (own run: events add gaps)
            pre.reset()
            ops.KernelTimer.reserve(4 * net.n_layer)
            ops.KernelTimer.reset(True)
            try:
                pre.prefill(prompt)
                torch.cuda.synchronize()
                calls, mean_ms, _ = ops.KernelTimer.summary()["cwlt_causal_linear_fwd_state"]
            finally:
                ops.KernelTimer.reset(False)
            scan_ms = calls * mean_ms
            # the same prompt token by token (graph replay per token; the first step captures, outside the timing)
            step.reset()
            step.step(toks[:, 0] if n > 1 else toks[0, 0])
            step.reset()

            def feed():
                out = None
                for t in range(P):
                    out = step.step(toks[:, t] if n > 1 else toks[0, t])
                return out
            step_ms, want = timed(feed)
            segs = int(lib.cwlt_prefill_segments(n, net.n_head, P))
            print(json.dumps({"metric": "prompt prefill (repo dims 512/12/8, f32)", "songs": n, "prompt_tokens": P,
                              "scan_segments": segs,
                              "prefill_ms": round(pre_ms, 3),
                              "prefill_tokens_per_s": round(n * P / pre_ms * 1e3, 1),
                              "step_ms": round(step_ms, 2), "step_tokens_per_s": round(n * P / step_ms * 1e3, 1),
                              "speedup": round(step_ms / pre_ms, 1), "scan_ms": round(scan_ms, 3),
                              "scan_share": round(scan_ms / pre_ms, 3),
                              "max_abs_logit_diff": float(np.abs(got - want).max())}), flush=True)


if __name__ == "__main__":
    main()

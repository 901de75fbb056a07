"""Per-song prompts on the stream against lock-step groups, on the repo dims (512/12/8, f32) with the random-init model
of tools/bench_generate_stream.py.  Every song continues its own prompt of 64-512 tokens (no Bar after the first row)
to bar 17, i.e. 16 bars past the prompt.
    python tools/bench_generate_prompts.py [--songs 2048] [--slots 256 1024] [--out FILE]
Writes JSON lines to --out (default profiles/generate_prompts_bench.jsonl) and prints them:
  * kind "step": tokens/s of the captured GEMM step at S songs (device time);
  * kind "mode": generate_stream(prompts=..., slots=S), generate_batch(prompts=...) in groups of S with each prefill
    kernel, and the shared-prompt stream (one prompt of the median length for every song) as a ceiling: drawn tokens/s,
    tokens/s with the prompts, steps, and for the stream the prefill's GPU seconds and share of the wall time;
  * kind "prefill": one block of --block prompts prefilled by kernel "blas" and "gemm": ms and GFLOP/s (projection
    FLOPs of the valid rows);
  * kind "bank_kernels": per-token device time of refill + advance against refill_bank + advance_bank at S slots;
  * kind "check": how many songs of generate_batch(prompts, prefill="gemm") differ from the stream's (must be 0).
--only-stream S: run generate_stream(prompts=..., slots=S) alone once after a warm-up (for a rocprofv3 kernel trace).
--only-bank-kernels: the "step" and "bank_kernels" records alone (an A/B of csrc/stream.hip between two trees)."""
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
from rlmg_amd import generation, ops  # noqa: E402

N_CLASS = [56, 135, 18, 87, 18, 25]
SEED = 2


def _word2event():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    return w2e


def _prompts(n, lo, hi, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for L in rng.integers(lo, hi + 1, n):
        p = np.stack([rng.integers(0, c, L) for c in N_CLASS], 1).astype(np.int64)
        p[1:, 2] = np.where(p[1:, 2] == 1, 0, p[1:, 2])                 # no Bar after the first row: bar count 1
        out.append(p)
    return out


def _replay_rate(net, S, steps):
    sess = generation.DecodeSession(net, n_songs=S, kernel="gemm", graph=True)
    ids = np.tile(generation.INIT_CW[0], (S, 1))
    for _ in range(3):
        sess.step(ids)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        sess._graph.replay()
    t1.record()
    t1.synchronize()
    return S * steps / (t0.elapsed_time(t1) * 1e-3)


def _timed(fn, reps=1):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps * 1e-3


def _prefill_flops(net, lengths):
    """2 x weights x rows of the projections (in_linear, QKV, out, FFN) over the valid rows + the heads on one row."""
    enc = net.transformer_encoder
    D, F, E = net.d_model, enc.layers[0].linear1.out_features, net.in_linear.in_features
    per_row = E * D + len(enc.layers) * (4 * D * D + 2 * D * F)
    return 2.0 * (per_row * sum(lengths) + D * sum(N_CLASS) * len(lengths))


def _bank_kernels(S, n_layer, H, W, reps, dev):
    """Device seconds per token of (refill, advance) and (refill_bank, advance_bank) at S slots, ~2 % fresh slots."""
    d = 64
    per = H * d * d + H * d
    state = torch.zeros(n_layer * S * per, device=dev)
    snap = torch.zeros(n_layer * per, device=dev)
    bank = 2 * S
    bstate = torch.zeros(n_layer * bank * per, device=dev)
    logits = torch.zeros(S, W, device=dev)
    snap_logits, blogits = torch.zeros(W, device=dev), torch.zeros(bank, W, device=dev)
    fresh = (torch.arange(S, device=dev) % 50 == 0).to(torch.int64)
    song = torch.arange(S, dtype=torch.int64, device=dev)
    tok = torch.zeros(S, 6, dtype=torch.int64, device=dev)
    mask = torch.zeros(N_CLASS[2], dtype=torch.int32, device=dev)
    mk = lambda: [torch.zeros(S, dtype=torch.int64, device=dev) for _ in range(3)]
    ring = torch.zeros(256, S, 8, dtype=torch.int64, device=dev)
    pos, bar, fr = mk()
    ctl = torch.tensor([0, S, 0], dtype=torch.int64, device=dev)
    big = 1 << 40

    def old():
        ops.stream_refill(state, snap, n_layer, H * d * d, H * d, logits, snap_logits, fresh)
        ops.stream_advance(tok, 2, mask, 17, 1, big, 1 << 20, song, pos, bar, fr, ctl, ring)

    pos2, bar2, fr2 = mk()
    cap2 = torch.full((S,), big, dtype=torch.int64, device=dev)
    ctl2 = torch.tensor([0, S, 0, 1 << 20], dtype=torch.int64, device=dev)
    b0, bc = torch.ones(bank, dtype=torch.int64, device=dev), torch.full((bank,), big, dtype=torch.int64, device=dev)

    def new():
        ops.stream_refill_bank(state, bstate, n_layer, H * d * d, H * d, logits, blogits, fresh, song)
        ops.stream_advance_bank(tok, 2, mask, 17, b0, bc, 1 << 20, song, pos2, bar2, cap2, fr2, ctl2, ring)

    return _timed(old, reps), _timed(new, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--group", type=int, default=256)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only-stream", type=int, default=0)
    ap.add_argument("--only-bank-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_prompts_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    torch.manual_seed(0)
    net = model.LinearTransformer(N_CLASS, is_training=False).cuda().eval()
    w2e = _word2event()
    dev = torch.cuda.get_device_name(0)
    prompts = _prompts(a.songs, 64, 512)
    n_prompt = sum(len(p) for p in prompts)
    torch.manual_seed(SEED)
    generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=600, prompts=prompts[:8])   # warm-up
    generation.generate_batch(net, w2e, 8, bar_cond=3, max_tokens=600, prompts=prompts[:8], prefill="gemm")
    torch.cuda.synchronize()
    if a.only_stream:
        torch.manual_seed(SEED)
        songs, st = generation._generate_stream(net, w2e, a.songs, slots=a.only_stream, bar_cond=a.bar_cond,
                                                max_tokens=a.max_tokens, prompts=prompts)
        print(json.dumps(dict(st, songs=a.songs, slots=a.only_stream)))
        return
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    enc = net.transformer_encoder

    def step_and_bank_kernels(S):
        rate = _replay_rate(net, S, a.steps)
        step_s = S / rate
        emit({"kind": "step", "slots": S, "steps": a.steps, "tokens_per_s": rate, "step_ms": step_s * 1e3})
        old, new = _bank_kernels(S, len(enc.layers), enc.layers[0].attention.n_heads, sum(N_CLASS), 200, net.in_linear.weight.device)
        emit({"kind": "bank_kernels", "slots": S, "refill_advance_us": old * 1e6, "bank_pair_us": new * 1e6,
              "step_us": step_s * 1e6, "delta_over_step": (new - old) / step_s})
        torch.cuda.empty_cache()
        return rate

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")

    if a.only_bank_kernels:
        for S in a.slots:
            step_and_bank_kernels(S)
        return write()

    # one block of prompts through each prefill kernel
    block = prompts[:a.block]
    P = max(len(p) for p in block)
    toks = np.zeros((len(block), P, 6), dtype=np.int64)
    for i, p in enumerate(block):
        toks[i, :len(p)] = p
    lens = [len(p) for p in block]
    sess = generation.DecodeSession(net, n_songs=len(block), kernel="gemm", graph=False)
    flops = _prefill_flops(net, lens)
    for kernel in ("blas", "gemm"):
        sec = _timed(lambda: (sess.reset(), sess._prefill(toks, lens, kernel=kernel)), reps=3)
        emit({"kind": "prefill", "kernel": kernel, "prompts": len(block), "rows": sum(lens), "padded_rows": len(block) * P,
              "ms": sec * 1e3, "gflops": flops / sec / 1e9})
    del sess
    torch.cuda.empty_cache()

    streams = {}
    for S in a.slots:
        rate = step_and_bank_kernels(S)
        torch.manual_seed(SEED)
        songs, st = generation._generate_stream(net, w2e, a.songs, slots=S, bar_cond=a.bar_cond,
                                                max_tokens=a.max_tokens, prompts=prompts)
        streams[S] = songs
        n_tok = sum(len(s) for s in songs)
        emit({"kind": "mode", "mode": "generate_stream_prompts", "slots": S, "songs": a.songs,
              "seconds": st["seconds"], "drawn": st["drawn"], "tokens": n_tok,
              "drawn_per_s": st["drawn"] / st["seconds"], "tokens_per_s": n_tok / st["seconds"],
              "drawn_over_step_rate": st["drawn"] / st["seconds"] / rate, "steps": st["steps"],
              "prefill_seconds": st["prefill_seconds"], "prefill_share": st["prefill_seconds"] / st["seconds"],
              "block": st["block"], "bank": st["bank"], "gated_chunks": st["gated_chunks"],
              "wait_seconds": st["wait_seconds"], "graph": st["graph"]})
        torch.cuda.empty_cache()
        if S == a.group:
            med = prompts[int(np.argsort([len(p) for p in prompts])[len(prompts) // 2])]
            torch.manual_seed(SEED)
            songs, st = generation._generate_stream(net, w2e, a.songs, slots=S, bar_cond=a.bar_cond,
                                                    max_tokens=a.max_tokens, prompt=med)
            n_tok = sum(len(s) for s in songs)
            emit({"kind": "mode", "mode": "generate_stream_shared_prompt", "slots": S, "songs": a.songs,
                  "prompt_len": len(med), "seconds": st["seconds"], "drawn": st["drawn"], "tokens": n_tok,
                  "drawn_per_s": st["drawn"] / st["seconds"], "tokens_per_s": n_tok / st["seconds"],
                  "steps": st["steps"]})
            torch.cuda.empty_cache()

    for kernel in ("blas", "gemm"):
        torch.manual_seed(SEED)
        t = time.perf_counter()
        songs = []
        for first in range(0, a.songs, a.group):
            songs += generation.generate_batch(net, w2e, min(a.group, a.songs - first), bar_cond=a.bar_cond,
                                               max_tokens=a.max_tokens, prompts=prompts[first:first + a.group],
                                               prefill=kernel)
        wall = time.perf_counter() - t
        n_tok = sum(len(s) for s in songs)
        emit({"kind": "mode", "mode": "generate_batch_groups", "prefill": kernel, "group": a.group, "songs": a.songs,
              "seconds": wall, "drawn": n_tok - n_prompt, "tokens": n_tok, "drawn_per_s": (n_tok - n_prompt) / wall,
              "tokens_per_s": n_tok / wall})
        torch.cuda.empty_cache()

    torch.manual_seed(SEED)
    t = time.perf_counter()
    ref = generation.generate_batch(net, w2e, a.songs, bar_cond=a.bar_cond, max_tokens=a.max_tokens, prompts=prompts,
                                    prefill="gemm")
    wall = time.perf_counter() - t
    for S, songs in streams.items():
        differ = sum(not (x.shape == y.shape and (x == y).all()) for x, y in zip(songs, ref))
        emit({"kind": "check", "slots": S, "songs": a.songs, "batch_seconds": wall,
              "songs_differing_from_generate_batch_gemm": int(differ)})
    write()


if __name__ == "__main__":
    main()

"""Many songs at once: the GEMV lock-step decode step against the GEMM step (csrc/decode_gemm.hip) at the repo dims
(512/12/8, f32, graph replay), and generate_batch against the serial generate end to end.
    python tools/bench_generate.py [--songs 1 8 32 64 256 1024] [--steps 20] [--rounds 3] [--out FILE]
Writes JSON lines to --out (default profiles/decode_gemm_bench.jsonl) and prints them:
  * kind "step": tokens/s (songs x steps / device time of the captured step's replays) of each kernel at each N, the
    two kernels alternated in rounds in the same process; median and best round;
  * kind "logit_diff": the worst |gemm - gemv| logit difference over teacher-forced steps on the same tokens;
  * kind "end_to_end": songs/s and tokens/s of generate_batch(N = 256, bar_cond = 17) and of the serial generate
    (device sampling) on 16 songs."""
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
from rlmg_amd import generation  # noqa: E402

N_CLASS = [56, 135, 18, 87, 18, 25]


def _word2event():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    return w2e


def _replay_rate(sess, steps):
    """tokens/s of `steps` replays of the session's captured step (device time, cuda events)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        sess._graph.replay()
    t1.record()
    t1.synchronize()
    return sess.n_songs * steps / (t0.elapsed_time(t1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, nargs="*", default=[1, 8, 32, 64, 256, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--e2e-songs", type=int, default=256)
    ap.add_argument("--serial-songs", type=int, default=16)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_gemm_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    torch.manual_seed(0)
    net = model.LinearTransformer(N_CLASS, is_training=False).cuda().eval()
    dev = torch.cuda.get_device_name(0)
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    # teacher-forced logits of the two kernels on the same tokens
    N = 64
    g = torch.Generator().manual_seed(1)
    toks = torch.stack([torch.randint(0, n, (N, 16), generator=g) for n in N_CLASS], -1).numpy()
    outs = {}
    for kernel in ("gemv", "gemm"):
        sess = generation.DecodeSession(net, n_songs=N, kernel=kernel, graph=True)
        outs[kernel] = np.stack([sess.step(toks[:, t]).copy() for t in range(16)])
        del sess
    emit({"kind": "logit_diff", "songs": N, "steps": 16,
          "worst_abs": float(np.abs(outs["gemm"] - outs["gemv"]).max()),
          "max_abs_logit": float(np.abs(outs["gemv"]).max())})

    for N in a.songs:
        sessions = {}
        for kernel in ("gemv", "gemm"):
            s = generation.DecodeSession(net, n_songs=N, kernel=kernel, graph=True)
            ids = np.tile(generation.INIT_CW[0], (N, 1))
            for _ in range(3):
                s.step(ids)                                         # captures, then replays
            assert s._graph is not None
            sessions[kernel] = s
        rates = {k: [] for k in sessions}
        for _ in range(a.rounds):
            for k, s in sessions.items():
                rates[k].append(_replay_rate(s, a.steps))
        for k, r in rates.items():
            emit({"kind": "step", "kernel": k, "songs": N, "steps": a.steps, "rounds": a.rounds,
                  "tokens_per_s_median": float(np.median(r)), "tokens_per_s_best": float(max(r))})
        gemv, gemm = np.median(rates["gemv"]), np.median(rates["gemm"])
        emit({"kind": "step_ratio", "songs": N, "gemm_over_gemv": float(gemm / gemv)})
        del sessions
        torch.cuda.empty_cache()

    w2e = _word2event()
    torch.manual_seed(2)
    generation.generate_batch(net, w2e, 8, bar_cond=3, max_tokens=64)      # warm-up (library load, first captures)
    torch.cuda.synchronize()
    t = time.time()
    songs = generation.generate_batch(net, w2e, a.e2e_songs, bar_cond=17, max_tokens=a.max_tokens)
    wall = time.time() - t
    n_tok = sum(len(s) for s in songs)
    emit({"kind": "end_to_end", "mode": "generate_batch", "songs": a.e2e_songs, "bar_cond": 17, "seconds": wall,
          "tokens": n_tok, "songs_per_s": a.e2e_songs / wall, "tokens_per_s": n_tok / wall,
          "capped": sum(len(s) == a.max_tokens for s in songs)})
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        t = time.time()
        st = generation.generate(net, w2e, n_songs=a.serial_songs, bar_cond=17, path_gendir=tmp,
                                 max_tokens=a.max_tokens, stats_path=None, log=lambda *x: None, device_sampling=True)
        wall = time.time() - t
    n_tok = sum(st["words_len_list"])
    emit({"kind": "end_to_end", "mode": "generate_serial_device_sampling", "songs": a.serial_songs, "bar_cond": 17,
          "seconds": wall, "tokens": n_tok, "songs_per_s": a.serial_songs / wall, "tokens_per_s": n_tok / wall})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

"""Continuous batching against lock-step groups: generate_stream(slots=S) vs generate(batch_size=S) vs the GEMM step's
replay rate at S, on the repo dims (512/12/8, f32) with the random-init model and seed of tools/bench_generate.py.
    python tools/bench_generate_stream.py [--songs 2048] [--slots 256 1024] [--max-tokens 4096] [--out FILE]
Writes JSON lines to --out (default profiles/generate_stream_bench.jsonl) and prints them:
  * kind "step": tokens/s of `--steps` replays of the captured GEMM step at S songs (device time);
  * kind "mode": songs/s, tokens/s, steps run, the step-time share of the wall time (steps x step time), host time
    outside waits on the device, and slot-steps that produced no kept token (a finished song still stepping in a
    lock-step group; an idle slot or a fresh slot's first step in the stream);
  * kind "check": how many songs of generate_batch(--songs) differ from the stream's (must be 0).
--only-stream S: run generate_stream(slots=S) alone once after a small warm-up (for a rocprofv3 kernel trace)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rlmg_amd  # noqa: E402,F401
from rlmg_amd import generation  # noqa: E402

N_CLASS = [56, 135, 18, 87, 18, 25]
SEED = 2


def _word2event():
    keys = ["tempo", "chord", "bar-beat", "pitch", "duration", "velocity"]
    w2e = {k: {i: "%s_%d" % (k, i) for i in range(n)} for k, n in zip(keys, N_CLASS)}
    w2e["bar-beat"][1] = "Bar"
    return w2e


def _replay_rate(net, S, steps):
    """tokens/s of `steps` replays of the captured GEMM step at S songs (device time, cuda events)."""
    sess = generation.DecodeSession(net, n_songs=S, kernel="gemm", graph=True)
    ids = np.tile(generation.INIT_CW[0], (S, 1))
    for _ in range(3):
        sess.step(ids)                                      # captures, then replays
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        sess._graph.replay()
    t1.record()
    t1.synchronize()
    return S * steps / (t0.elapsed_time(t1) * 1e-3)


class _TimedLoop(generation._DeviceLoop):
    """generate_batch's device loop, counting steps and the host time spent in the reads that wait on the device."""
    steps, wait = 0, 0.0

    def run(self, n):
        n = super().run(n)
        _TimedLoop.steps += n
        return n

    def tokens(self, start, stop):
        t = time.perf_counter()
        out = super().tokens(start, stop)
        _TimedLoop.wait += time.perf_counter() - t
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=2048)
    ap.add_argument("--slots", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--bar-cond", type=int, default=17)
    ap.add_argument("--max-tokens", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only-stream", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_stream_bench.jsonl"))
    a = ap.parse_args()
    from rlmg_amd.dqn_policy import model
    torch.manual_seed(0)
    net = model.LinearTransformer(N_CLASS, is_training=False).cuda().eval()
    w2e = _word2event()
    dev = torch.cuda.get_device_name(0)
    torch.manual_seed(SEED)
    generation.generate_stream(net, w2e, 8, slots=4, bar_cond=3, max_tokens=64)     # warm-up: library load, captures
    generation.generate_batch(net, w2e, 8, bar_cond=3, max_tokens=64)
    torch.cuda.synchronize()
    if a.only_stream:
        torch.manual_seed(SEED)
        songs, st = generation._generate_stream(net, w2e, a.songs, slots=a.only_stream, bar_cond=a.bar_cond,
                                                max_tokens=a.max_tokens)
        print(json.dumps(dict(st, songs=a.songs, slots=a.only_stream)))
        return
    lines = []

    def emit(d):
        d = dict(d, device=dev)
        print(json.dumps(d), flush=True)
        lines.append(d)

    streams = {}
    for S in a.slots:
        rate = _replay_rate(net, S, a.steps)
        step_s = S / rate
        emit({"kind": "step", "slots": S, "steps": a.steps, "tokens_per_s": rate, "step_ms": step_s * 1e3})
        torch.cuda.empty_cache()

        torch.manual_seed(SEED)
        songs, st = generation._generate_stream(net, w2e, a.songs, slots=S, bar_cond=a.bar_cond,
                                                max_tokens=a.max_tokens)
        streams[S] = songs
        n_tok = sum(len(s) for s in songs)
        emit({"kind": "mode", "mode": "generate_stream", "slots": S, "songs": a.songs, "seconds": st["seconds"],
              "tokens": n_tok, "songs_per_s": a.songs / st["seconds"], "tokens_per_s": n_tok / st["seconds"],
              "over_step_rate": n_tok / st["seconds"] / rate, "steps": st["steps"],
              "step_seconds": st["steps"] * step_s, "wait_seconds": st["wait_seconds"],
              "host_seconds": st["seconds"] - st["wait_seconds"], "slot_steps": st["slot_steps"],
              "wasted_slot_steps": st["slot_steps"] - st["drawn"], "capped": sum(len(s) == a.max_tokens for s in songs)})
        torch.cuda.empty_cache()

        _TimedLoop.steps, _TimedLoop.wait = 0, 0.0
        plain = generation._DeviceLoop
        generation._DeviceLoop = _TimedLoop
        try:
            torch.manual_seed(SEED)
            t = time.perf_counter()
            res = generation.generate(net, w2e, n_songs=a.songs, bar_cond=a.bar_cond, path_gendir=tempfile.mkdtemp(),
                                      write_midi=lambda *x: None, max_tokens=a.max_tokens, stats_path=None,
                                      log=lambda *x: None, batch_size=S)
            wall = time.perf_counter() - t
        finally:
            generation._DeviceLoop = plain
        n_tok = sum(res["words_len_list"])
        emit({"kind": "mode", "mode": "generate_batch_size", "slots": S, "songs": a.songs, "seconds": wall,
              "tokens": n_tok, "songs_per_s": a.songs / wall, "tokens_per_s": n_tok / wall,
              "over_step_rate": n_tok / wall / rate, "steps": _TimedLoop.steps,
              "step_seconds": _TimedLoop.steps * step_s, "wait_seconds": _TimedLoop.wait,
              "host_seconds": wall - _TimedLoop.wait, "slot_steps": _TimedLoop.steps * S,
              "wasted_slot_steps": _TimedLoop.steps * S - (n_tok - a.songs)})
        torch.cuda.empty_cache()

    torch.manual_seed(SEED)
    t = time.perf_counter()
    ref = generation.generate_batch(net, w2e, a.songs, bar_cond=a.bar_cond, max_tokens=a.max_tokens)
    wall = time.perf_counter() - t
    for S, songs in streams.items():
        differ = sum(not (x.shape == y.shape and (x == y).all()) for x, y in zip(songs, ref))
        emit({"kind": "check", "slots": S, "songs": a.songs, "batch_seconds": wall,
              "songs_differing_from_generate_batch": int(differ)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()

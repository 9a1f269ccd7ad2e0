"""Slot-streaming cost of the transducer recipe's encoder (the model of tools/stream_bench.py: 12 Conformer layers, d_model 512,
SummaryMixing-fast, GELU, k = 31, bf16), chunk C = 16, left context 2.

  replay  - ms per step of one captured slot step (summarymixing_amd.streaming.CapturedSlotStep, all slots fed full chunks)
            against one captured lockstep step (CapturedStreamStep) at the same (B, C); the two are timed alternately in one
            process, `--rounds` times, and the medians reported.  step() calls are timed whole: host validation, the staging of
            valid / start (slots) and the input copy are included.
  serving - a seeded simulation of B = 64 slots serving `--utts` utterances of 2-20 s with staggered (Poisson) arrivals and
            random one-step pauses: each step every free slot takes the next arrived utterance.  Reports steps, mean slot
            occupancy (slots fed a chunk / B), ms per step and the aggregate real-time factor (device time / audio time, one
            frame = 40 ms: 10 ms hop, 4x sub-sampling by the front-end).

  python tools/slot_stream_bench.py [--B 1 16 64] [--steps 40] [--rounds 5] [--utts 256] [--json out.jsonl]
"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from stream_bench import model, timed                                                        # noqa: E402
from summarymixing_amd.streaming import CapturedSlotStep, CapturedStreamStep                  # noqa: E402
from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig                # noqa: E402

C, LEFT, F_IN, FRAME_MS = 16, 2, 640, 40.0


def replay(w, B, steps, rounds, warmup, dtype):
    cfg = DynChunkTrainConfig(C, LEFT)
    x = torch.randn(B, C, F_IN, device="cuda", dtype=dtype)
    lock = CapturedStreamStep(w, w.make_streaming_context(cfg), B, C, dtype=dtype)
    slot = CapturedSlotStep(w, w.make_slot_context(cfg, B), B, C, dtype=dtype)
    full, go, no = [C] * B, [True] * B, [False] * B
    slot.step(x, full, go)
    for _ in range(warmup):
        lock.step(x)
        slot.step(x, full, no)
    tl, ts = [], []
    for _ in range(rounds):                            # (steps * rounds + warmup chunks stay within max_length)
        tl.append(timed(lambda: lock.step(x), steps))
        ts.append(timed(lambda: slot.step(x, full, no), steps))
    ml, ms = statistics.median(tl), statistics.median(ts)
    return {"B": B, "C": C, "left": LEFT, "lockstep_replay_ms": round(ml, 4), "slot_replay_ms": round(ms, 4),
            "slot_over_lockstep": round(ms / ml, 4)}


def serving(w, B, n_utts, seed, dtype):
    """One pass of the simulation through a CapturedSlotStep; device-event time over all steps."""
    rng = random.Random(seed)
    cfg = DynChunkTrainConfig(C, LEFT)
    lengths = [int(rng.uniform(2.0, 20.0) * 1000 / FRAME_MS) for _ in range(n_utts)]
    mean_steps = sum(-(-n // C) for n in lengths) / n_utts
    rate = 0.9 * B / mean_steps                        # arrivals per step for ~90 % offered load
    arrive, t = [], 0.0
    for _ in range(n_utts):
        t += rng.expovariate(rate)
        arrive.append(int(t))
    cap = CapturedSlotStep(w, w.make_slot_context(cfg, B), B, C, dtype=dtype)
    x = torch.randn(B, C, F_IN, device="cuda", dtype=dtype)
    busy = [None] * B                                  # slot -> [utterance, frames fed]
    nxt, steps, fed = 0, 0, 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    while nxt < n_utts or any(b is not None for b in busy):
        valid, start = [0] * B, [False] * B
        for b in range(B):
            if busy[b] is None and nxt < n_utts and arrive[nxt] <= steps:
                busy[b], start[b] = [nxt, 0], True
                nxt += 1
            if busy[b] is None or rng.random() < 0.02:     # idle, or a client a chunk behind
                continue
            u, f = busy[b]
            valid[b] = min(C, lengths[u] - f)
            busy[b][1] += valid[b]
            if busy[b][1] == lengths[u]:
                busy[b] = None
        cap.step(x, valid, start)
        fed += sum(1 for v in valid if v)
        steps += 1
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    audio_ms = sum(lengths) * FRAME_MS
    return {"B": B, "C": C, "left": LEFT, "utterances": n_utts, "steps": steps, "mean_occupancy": round(fed / (steps * B), 4),
            "ms_per_step": round(ms / steps, 4), "audio_s": round(audio_ms / 1000, 1), "device_s": round(ms / 1000, 3),
            "rtf": round(ms / audio_ms, 6)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--serve-B", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dtype = torch.bfloat16
    w = model(dtype)
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(json.dumps(r) + "\n")

    for B in a.B:
        r = replay(w, B, a.steps, a.rounds, a.warmup, dtype)
        rows.append(r)
        emit(r)
    s = serving(w, a.serve_B, a.utts, a.seed, dtype) if a.utts > 0 else None
    if s:
        emit(s)
    print(f"\n|  B |  C | left | lockstep replay ms/step | slot replay ms/step | slot / lockstep |")
    print("|---:|---:|-----:|------------------------:|--------------------:|----------------:|")
    for r in rows:
        print(f"| {r['B']:>2} | {r['C']:>2} | {r['left']:>4} | {r['lockstep_replay_ms']:>23.3f} | {r['slot_replay_ms']:>19.3f} | "
              f"{r['slot_over_lockstep']:>15.3f} |")
    if s:
        print(f"\nserving: {s['utterances']} utterances ({s['audio_s']} s of audio), B = {s['B']} slots: {s['steps']} steps, "
              f"mean occupancy {s['mean_occupancy']:.3f}, {s['ms_per_step']:.3f} ms/step, RTF {s['rtf']:.5f}")


if __name__ == "__main__":
    main()

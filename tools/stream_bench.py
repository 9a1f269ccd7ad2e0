"""Streaming-inference cost of the transducer recipe's encoder (conformer_summarymixing_transducer.yaml:117-146: 12 Conformer
layers, d_model 512, 4 heads, d_ffn 2048, SummaryMixing-fast with local_proj_out_dim 256, GELU, k = 31; CNN output 640 features).

For every (B streams, C frames per chunk, left context) it times, with device events after a warm-up, in one process:
  eager   - TransformerASR.encode_streaming per chunk (Python host path + launches);
  replay  - one captured chunk step (summarymixing_amd.streaming.CapturedStreamStep) per chunk;
and reports ms per chunk, library calls per chunk (each launches one kernel, the GEMM routes aside) and the real-time factor
(chunk audio = C x 40 ms: 10 ms hop, 4x sub-sampling by the front-end).  One JSON line per configuration, a table at the end.

  python tools/stream_bench.py [--B 1 16 64] [--C 8 16 32] [--left 2 none] [--chunks 50] [--warmup 5] [--json out.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import _lib as L                                                         # noqa: E402
from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR  # noqa: E402
from summarymixing_amd.streaming import CapturedStreamStep                                       # noqa: E402
from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig                   # noqa: E402

_QUERIES = ("_ok", "_workspace", "_blocks", "_rows", "plan_query", "capture_id", "last_error", "version", "get_config", "_splits",
            "_tile_rows")


class _CallCounter:
    """Counts the launching library calls made through summarymixing_amd._lib while installed."""

    def __init__(self, lib):
        self._lib, self.n = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("smx_") or any(q in name for q in _QUERIES):
            return fn

        def call(*a):
            self.n += 1
            return fn(*a)
        return call


def model(dtype):
    torch.manual_seed(0)
    net = TransformerASR(tgt_vocab=10, input_size=640, d_model=512, nhead=4, num_encoder_layers=12, num_decoder_layers=0, d_ffn=2048,
                         dropout=0.0, encoder_module="conformer", conformer_activation=torch.nn.GELU, attention_type="SummaryMixing",
                         mode="SummaryMixing-fast", local_proj_hid_dim=[512], local_proj_out_dim=256, summary_hid_dim=[512],
                         causal=False, kernel_size=31, max_length=6000)
    return EncoderWrapper(net).cuda().eval()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def one(w, B, C, left, chunks, warmup, dtype):
    cfg = DynChunkTrainConfig(C, left)
    x = torch.randn(B, C, 640, device="cuda", dtype=dtype)
    ctx = w.make_streaming_context(cfg)
    for _ in range(warmup):
        w.forward_streaming(x, ctx)
    real = L.lib()
    L._lib = counter = _CallCounter(real)
    try:
        w.forward_streaming(x, ctx)
    finally:
        L._lib = real
    eager = timed(lambda: w.forward_streaming(x, ctx), chunks)
    cctx = w.make_streaming_context(cfg)
    cap = CapturedStreamStep(w, cctx, B, C, dtype=dtype)
    for _ in range(warmup):
        cap.step(x)
    replay = timed(lambda: cap.step(x), chunks)
    audio_ms = C * 40.0
    return {"B": B, "C": C, "left": left, "dtype": str(dtype).replace("torch.", ""), "eager_ms_per_chunk": round(eager, 4),
            "replay_ms_per_chunk": round(replay, 4), "lib_calls_per_chunk": counter.n, "audio_ms_per_chunk": audio_ms,
            "rtf_eager": round(eager / audio_ms, 5), "rtf_replay": round(replay / audio_ms, 5)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--C", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--left", nargs="+", default=["2", "none"])
    ap.add_argument("--chunks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--json", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    w = model(dtype)
    rows = []
    for left in [None if v.lower() == "none" else int(v) for v in a.left]:
        for C in a.C:
            for B in a.B:
                r = one(w, B, C, left, a.chunks, a.warmup, dtype)
                rows.append(r)
                print(json.dumps(r), flush=True)
                if a.json:
                    with open(a.json, "a") as f:
                        f.write(json.dumps(r) + "\n")
    print("\n|  B |  C | left | eager ms/chunk | replay ms/chunk | lib calls/chunk | RTF eager | RTF replay |")
    print("|---:|---:|-----:|---------------:|----------------:|----------------:|----------:|-----------:|")
    for r in rows:
        print(f"| {r['B']:>2} | {r['C']:>2} | {str(r['left']):>4} | {r['eager_ms_per_chunk']:>14.3f} | {r['replay_ms_per_chunk']:>15.3f} | "
              f"{r['lib_calls_per_chunk']:>15} | {r['rtf_eager']:>9.4f} | {r['rtf_replay']:>10.4f} |")


if __name__ == "__main__":
    main()

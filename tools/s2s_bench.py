"""Tokens per second of the seq2seq greedy search at the recipes' decoder (num_decoder_layers 6, nhead 1, d_model 512, d_ffn 2048,
normalize_before, GELU; seq_lin 512 -> 5000; encoder output of S = 390 frames), three ways, in one process on the same inputs:

  prefix    what exists without the KV cache: a host loop of TransformerASR.decode(prefix) + seq_lin on the last position + argmax,
            the whole prefix again for every token;
  cached    decoders.seq2seq.greedy_search: decode_step over the caches + seq_lin + smx_s2s_select, every position on the device;
  captured  decoders.seq2seq.CapturedS2SGreedy: the same step captured once as a graph and replayed.

eos is disabled (an index no token has), so all three run exactly `steps` steps; the searches run with poll_every = 8 as shipped (the
B-byte done vector is read, and never all set).  Timing: wall clock around a whole search with a device synchronisation before and
after; `--rounds` searches per way, alternated, after one warm-up search each; the median and the spread are reported as ms per search,
ms per token and tokens per second (per row).  growth: the cached search's ms per token over the second half of the steps divided by
the first half's (two searches of steps / 2 and steps: the cost of a step as the caches fill; both searches contain the utterance's
cross-attention projections, so the first half's per-token figure carries them and the ratio is a little low).  The cross-attention
K / V projections of the utterance (make_decode_state) are inside the cached and captured times.  No GPU: the tool fails.

  python tools/s2s_bench.py [--batches 1 8] [--steps 64 128] [--dtypes f32 bf16] [--rounds 5] [--out profiles/s2s_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd.decoders import CapturedS2SGreedy, greedy_search                                # noqa: E402
from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR                  # noqa: E402
from summarymixing_amd.nnet.linear import Linear                                                      # noqa: E402

LAYERS, D, D_FFN, NHEAD, V, S, BOS = 6, 512, 2048, 1, 5000, 390, 1
NO_EOS = V + 1


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(fns, rounds):
    for fn in fns.values():
        fn()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(wall(fn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def bench_point(model, lin, B, steps, dtype, rounds, emit):
    name = "bf16" if dtype == torch.bfloat16 else "f32"
    g = torch.Generator().manual_seed(B)
    mem = torch.randn(B, S, D, generator=g).cuda().to(dtype)
    enc_len = torch.full((B,), S, device="cuda")
    cap = CapturedS2SGreedy(model, lin, B, S, steps, dtype, BOS, NO_EOS)
    state = model.make_decode_state(mem, enc_len, steps)
    half = model.make_decode_state(mem, enc_len, steps // 2)

    @torch.no_grad()
    def prefix(n=steps):
        toks = torch.full((B, 1), BOS, dtype=torch.int32, device="cuda")
        for _ in range(n):
            z = lin(model.decode(toks, mem, enc_len)[0][:, -1])
            toks = torch.cat([toks, torch.argmax(z, -1).to(torch.int32)[:, None]], 1)
        return toks[:, 1:]

    def cached():
        return greedy_search(model, lin, mem, enc_len, BOS, NO_EOS, 0, steps, state=state).tokens

    def cached_half():
        return greedy_search(model, lin, mem, enc_len, BOS, NO_EOS, 0, steps // 2, state=half).tokens

    def captured():
        return cap.search(mem, enc_len).tokens
    agree = bool(torch.equal(cached().clone(), captured())) and (dtype != torch.float32 or bool(torch.equal(prefix(), cached())))
    res = alternate({"prefix": prefix, "cached": cached, "captured": captured, "cached_half": cached_half}, rounds)
    p, c, g_, h = res["prefix"], res["cached"], res["captured"], res["cached_half"]
    growth = ((c[0] - h[0]) / (steps - steps // 2)) / (h[0] / (steps // 2))
    emit(f"B {B:2d} steps {steps:3d} {name:4s}  prefix {p[0]:8.2f} ms [{p[1]:.2f}, {p[2]:.2f}] {p[0] / steps:6.3f} ms/tok {1e3 * steps / p[0]:7.0f} tok/s | "
         f"cached {c[0]:7.2f} ms [{c[1]:.2f}, {c[2]:.2f}] {c[0] / steps:6.3f} ms/tok {1e3 * steps / c[0]:7.0f} tok/s | "
         f"captured {g_[0]:7.2f} ms [{g_[1]:.2f}, {g_[2]:.2f}] {g_[0] / steps:6.3f} ms/tok {1e3 * steps / g_[0]:7.0f} tok/s | "
         f"prefix / cached {p[0] / c[0]:5.2f}  prefix / captured {p[0] / g_[0]:5.2f}  cached 2nd-half / 1st-half ms/tok {growth:4.2f}  "
         f"same tokens {agree}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--steps", nargs="+", type=int, default=[64, 128])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file (replacing it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("s2s_bench: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tools/s2s_bench.py on {torch.cuda.get_device_name(0)}: greedy search, {LAYERS} layers d {D} H {NHEAD} d_ffn {D_FFN} V {V} S {S}, eos "
         f"disabled; ms per search = median [min, max] of {args.rounds} alternated searches, wall clock between device synchronisations")
    torch.manual_seed(0)
    model = TransformerASR(tgt_vocab=V, input_size=80, d_model=D, nhead=NHEAD, num_encoder_layers=1, num_decoder_layers=LAYERS,
                           d_ffn=D_FFN, dropout=0.0, activation=nn.GELU, normalize_before=True, encoder_module="branchformer",
                           attention_type="SummaryMixing", causal=False, csgu_linear_units=64, kernel_size=3, local_proj_hid_dim=[64],
                           local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64).cuda().eval()
    lin = Linear(n_neurons=V, input_size=D).cuda()
    for dt in args.dtypes:
        for B in args.batches:
            for steps in args.steps:
                bench_point(model, lin, B, steps, torch.bfloat16 if dt == "bf16" else torch.float32, args.rounds, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

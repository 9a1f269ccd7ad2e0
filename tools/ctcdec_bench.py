"""CTC greedy decoding from the encoder output, three ways on the same GPU in one process:
  (i)   aten     the upstream-style chain: F.linear (ATen) + F.log_softmax + torch.max, then the host collapse (.tolist() per
                 utterance and itertools.groupby, as speechbrain.decoders.ctc.ctc_greedy_decode does);
  (ii)  unfused  this package's Linear + smx_ctc_best_path over the stored logits + smx_ctc_collapse, all on the device;
  (iii) fused    smx_ctc_head_best_path (the logits are never stored) + smx_ctc_collapse, all on the device.
Points (B, T, K, V): (128, 125, 512, 5000) and (16, 125, 512, 5000) - the Branchformer recipes' ctc_lin - and (8, 94, 640, 1000) - the
transducer recipes' proj_ctc; float32 and bfloat16.  Every variant is warmed at every point, then timed in windows of at least
--window seconds between two device events that end in a synchronise (the calls per window are calibrated per variant), the variants
alternating inside one process, in both orders; the figures are the median and the extremes of --reps windows, per call.  (i) ends on
the host (its lists), (ii) and (iii) on the device (their count and token tensors); a call carries the host's enqueue cost of its
launches.  `spread` is (max - min) / median of a variant's windows: (iii) beats (ii) only where the gap exceeds both spreads.
One JSON line per point.

    python tools/ctcdec_bench.py [--reps 5 --window 0.3 --out FILE] [--points "B,T,K,V;B,T,K,V;..."]

--points replaces the three recipe points (to locate a crossover of the fused route, decoders/ctc.py::_plan_fused)."""
import argparse
import json
import math
import os
import statistics
import sys
from itertools import groupby

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd.decoders import ctc  # noqa: E402
from summarymixing_amd.nnet.linear import Linear  # noqa: E402

POINTS = [(128, 125, 512, 5000), (16, 125, 512, 5000), (8, 94, 640, 1000)]


def aten_chain(x, W, b, rel, blank):
    """upstream's ctc_greedy_decode on the ATen head"""
    lp = Fn.log_softmax(Fn.linear(x, W, b), -1)
    T = lp.shape[1]
    hyps = []
    for seq, seq_len in zip(lp, rel):
        n = int(torch.round(seq_len * T))
        _, pred = torch.max(seq.narrow(0, 0, n), dim=1)
        hyps.append([k for k in (g[0] for g in groupby(pred.tolist())) if k != blank])
    return hyps


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_point(B, T, K, V, dtype, reps, min_window):
    g = torch.Generator().manual_seed(0)
    lin = Linear(V, input_size=K).cuda()
    x = torch.randn(B, T, K, generator=g).to(dtype).cuda()
    rel = (torch.rand(B, generator=g) * 0.5 + 0.5).cuda()
    rel[0] = 1.0
    W, b = lin.w.weight.detach().to(dtype), lin.w.bias.detach().to(dtype)
    blank = 0
    fns = {"aten": lambda: aten_chain(x, W, b, rel, blank),
           "unfused": lambda: ctc.greedy_decode_from_encoder(x, lin, rel, blank=blank, fused=False),
           "fused": lambda: ctc.greedy_decode_from_encoder(x, lin, rel, blank=blank, fused=True)}
    with torch.no_grad():
        for name in fns:                                      # warm every variant at this point
            for _ in range(3):
                fns[name]()
        hyp_a = fns["aten"]()
        ru, rf = fns["unfused"](), fns["fused"]()
        torch.cuda.synchronize()

        def lists(r):
            tk, n = r.tokens.cpu(), r.counts.cpu()
            return [tk[i, :int(n[i])].tolist() for i in range(B)]
        hyp_u, hyp_f = lists(ru), lists(rf)
        inner = {name: max(2, math.ceil(min_window * 1e3 / window(fns[name], 3))) for name in fns}
        times = {name: [] for name in fns}
        for it in range(reps):
            for name in (list(fns) if it % 2 == 0 else list(fns)[::-1]):
                times[name].append(window(fns[name], inner[name]))
    ms = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / statistics.median(v)}
          for k, v in times.items()}
    return {"B": B, "T": T, "K": K, "V": V, "dtype": str(dtype).split(".")[-1], "calls_per_window": inner, "ms_per_call": ms,
            "fused_over_unfused": ms["fused"]["median"] / ms["unfused"]["median"],
            "unfused_over_aten": ms["unfused"]["median"] / ms["aten"]["median"],
            "fused_over_aten": ms["fused"]["median"] / ms["aten"]["median"],
            "fused_beats_unfused_beyond_spread": ms["fused"]["max"] < ms["unfused"]["min"],
            "same_hypotheses": {"fused_vs_unfused": sum(a == c for a, c in zip(hyp_f, hyp_u)) / B,
                                "unfused_vs_aten": sum(a == c for a, c in zip(hyp_u, hyp_a)) / B},
            "logit_bytes": B * T * V * x.element_size(), "gemm_flop": 2.0 * B * T * K * V,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", default=None, help='"B,T,K,V;..." instead of the recipe points')
    a = ap.parse_args()
    points = POINTS if a.points is None else [tuple(int(v) for v in p.split(",")) for p in a.points.split(";")]
    if not torch.cuda.is_available():
        raise SystemExit("ctcdec_bench needs the GPU: there is nothing to time without one")
    lines = []
    for (B, T, K, V) in points:
        for dt in (torch.float32, torch.bfloat16):
            lines.append(json.dumps(bench_point(B, T, K, V, dt, a.reps, a.window)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

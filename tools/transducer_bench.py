"""Transducer head at the recipe batch (B = 10 utterances x T = 375 encoder frames, U = 60 tokens, J = 640, V = 1000, bf16):
the drop-in chain Tjoint -> transducer_lin -> transducer_loss against the fused transducer_joint_loss, alternated in one process.
Prints forward and forward + backward milliseconds (median over --reps after --warmup), each path's peak memory above what was
allocated before the call, and the fused GEMMs against a plain smx_gemm of the same shape.

    python tools/transducer_bench.py [--B 10 --T 375 --U 60 --J 640 --V 1000 --reps 20 --warmup 3]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import _lib as L  # noqa: E402
from summarymixing_amd import functional as F  # noqa: E402
from summarymixing_amd import ops  # noqa: E402
from summarymixing_amd.nnet.linear import Linear  # noqa: E402
from summarymixing_amd.nnet.losses import transducer_loss  # noqa: E402
from summarymixing_amd.nnet.transducer import Transducer_joint, transducer_joint_loss  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("B", 10), ("T", 375), ("U", 60), ("J", 640), ("V", 1000), ("reps", 20), ("warmup", 3)):
        ap.add_argument(f"--{k}", type=int, default=v)
    a = ap.parse_args()
    B, T, U, J, V = a.B, a.T, a.U, a.J, a.V
    rows = B * T * (U + 1)
    dt = torch.bfloat16
    torch.manual_seed(0)
    tj = Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU)
    lin = Linear(V, input_size=J, bias=False).cuda()
    enc = (torch.randn(B, T, J, device="cuda") * 0.5).to(dt).requires_grad_(True)
    dec = (torch.randn(B, U + 1, J, device="cuda") * 0.5).to(dt).requires_grad_(True)
    targets = torch.randint(1, V, (B, U), device="cuda")
    in_rel = torch.linspace(0.8, 1.0, B, device="cuda")
    tg_rel = torch.linspace(0.7, 1.0, B, device="cuda")

    def dropin():
        return transducer_loss(lin(tj(enc.unsqueeze(2), dec.unsqueeze(1))), targets, in_rel, tg_rel, 0)

    def fused():
        return transducer_joint_loss(enc, dec, tj, lin, targets, in_rel, tg_rel, 0)

    paths = {"drop-in": dropin, "fused": fused}
    res = {k: {"fwd": [], "fwdbwd": []} for k in paths}
    peak = {}
    for it in range(a.warmup + a.reps):
        for name, fn in paths.items():
            enc.grad = dec.grad = None
            lin.zero_grad(set_to_none=True)
            with torch.no_grad():
                tf = timed(fn)
            enc.grad = dec.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            m0 = torch.cuda.memory_allocated()
            tb = timed(lambda: fn().backward())
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - m0)
            if it >= a.warmup:
                res[name]["fwd"].append(tf)
                res[name]["fwdbwd"].append(tb)
    print(f"transducer head, recipe batch: B={B} T={T} U={U} J={J} V={V} bf16, lattice rows {rows}; "
          f"fp32 logits would be {rows * V * 4 / 2**20:.0f} MiB; median of {a.reps} after {a.warmup} warm-up, paths alternated")
    for name in paths:
        print(f"  {name:8s} forward {statistics.median(res[name]['fwd']):7.3f} ms   forward+backward "
              f"{statistics.median(res[name]['fwdbwd']):7.3f} ms   peak {peak[name] / 2**20:8.1f} MiB")
    print(f"  fused / drop-in: forward+backward {statistics.median(res['fused']['fwdbwd']) / statistics.median(res['drop-in']['fwdbwd']):.3f}x, "
          f"peak memory {peak['fused'] / peak['drop-in']:.3f}x")

    # the GEMMs alone: fused forward-statistics and gradient GEMMs against a plain smx_gemm (bf16 out) of the same shape
    with torch.no_grad():
        H2 = ops.transducer_joint_fwd(enc.detach(), dec.detach(), L.ACT_GELU).view(-1, J)
        Wc = F.wcast(lin.w.weight, dt)
        tg = targets.to(torch.int32).contiguous()
        out = torch.empty((rows, V), dtype=dt, device="cuda")
        lse, lpb, lpy = ops.transducer_gemm_stats(H2, Wc, None, tg, B, T, U + 1, 0)
        gb = torch.full((rows,), -1e-3, device="cuda")
        gy = torch.full((rows,), -1e-3, device="cuda")
        jobs = {"plain smx_gemm (logits, bf16 out)": lambda: ops.gemm(L.GEMM_NT, H2, Wc, out, rows, V, J),
                "fused forward statistics": lambda: ops.transducer_gemm_stats(H2, Wc, None, tg, B, T, U + 1, 0),
                "fused gradient (dz, bf16 out)": lambda: ops.transducer_gemm_grad(H2, Wc, None, tg, lse, gb, gy, B, T, U + 1, 0, 0,
                                                                                  rows, out)}
        times = {k: [] for k in jobs}
        for it in range(a.warmup + a.reps):
            for k, fn in jobs.items():
                t = timed(fn)
                if it >= a.warmup:
                    times[k].append(t)
    flops = 2.0 * rows * J * V
    base = statistics.median(times["plain smx_gemm (logits, bf16 out)"])
    for k in jobs:
        m = statistics.median(times[k])
        print(f"  {k:36s} {m:7.3f} ms  {flops / m / 1e9:7.1f} TFLOP/s  {m / base:5.2f}x the plain GEMM")


if __name__ == "__main__":
    main()

"""MultiheadAttention (regularMHA) forward + backward per call, on the same GPU in one process:
  (a) torch   torch.nn.MultiheadAttention the way upstream's wrapper calls it: (L, B, d) layout behind two permutes, the look-ahead
              mask as an (L, L) tensor for self-attention, key_padding_mask for cross-attention, need_weights=True;
  (b) ours    summarymixing_amd.nnet.attention.MultiheadAttention with the same arguments (weights returned);
  (c) ours, training form: return_attn_weights=False and causal=True instead of the mask tensor (what a decoder layer would call).
Points (B, L, S, H, D), float32 (the recipes' precision) and bfloat16: self-attention (32, 64, 64, 1, 512) and cross-attention
(32, 64, 390, 1, 512) - the LibriSpeech Branchformer batch, 500 s at 25 encoder frames/s and about 64 tokens per utterance - their
nhead 4 forms (.., 4, 128), (128, 80, 125, 1, 512) and the decode step (10, 1, 390, 1, 512).
Every variant is warmed at every point, then timed in windows of at least --window seconds between two device events (calls per
window calibrated per variant), the variants alternating in both orders; the figures are the median and the extremes of --reps
windows, per call.  A call carries the host's enqueue cost of its launches.  The attention kernels' own times come from a separate
pass with ops' event brackets (attn_fwd / attn_bwd / attn_weights: medians of 20 calls); next to them the grid each launch fills the
256 CUs with (smx_attn_plan_query).

    python tools/attention_bench.py [--reps 5 --window 0.25 --out FILE]"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import _lib, ops  # noqa: E402
from summarymixing_amd.nnet.attention import MultiheadAttention  # noqa: E402

POINTS = [("self", 32, 64, 64, 1, 512), ("cross", 32, 64, 390, 1, 512), ("self", 32, 64, 64, 4, 128), ("cross", 32, 64, 390, 4, 128),
          ("cross", 128, 80, 125, 1, 512), ("decode", 10, 1, 390, 1, 512)]


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_point(kind, B, L, S, H, D, dtype, reps, min_window):
    d = H * D
    torch.manual_seed(0)
    tm = torch.nn.MultiheadAttention(d, H).cuda().to(dtype)
    om = MultiheadAttention(H, d)
    om.load_state_dict({"att." + k: v.float() for k, v in tm.state_dict().items()}, strict=True)
    om = om.cuda()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, L, d, generator=g).cuda().to(dtype).requires_grad_(True)
    mem = x if kind == "self" else torch.randn(B, S, d, generator=g).cuda().to(dtype).requires_grad_(True)
    r = torch.randn(B, L, d, generator=g).cuda().to(dtype)
    look = torch.triu(torch.ones(L, L, dtype=torch.bool, device="cuda"), diagonal=1) if kind == "self" else None
    pad = None
    if kind != "self":
        lens = torch.linspace(S // 2, S, B).long().cuda()
        pad = torch.arange(S, device="cuda")[None, :] >= lens[:, None]

    def torch_call():
        q, k, v = x.permute(1, 0, 2), mem.permute(1, 0, 2), mem.permute(1, 0, 2)     # (three views, as upstream's wrapper makes them)
        out, w = tm(q, k, v, attn_mask=look, key_padding_mask=pad, need_weights=True)
        return out.permute(1, 0, 2)
    fns = {"torch": torch_call,
           "ours": lambda: om(x, mem, mem, attn_mask=look, key_padding_mask=pad)[0],
           "ours_train": lambda: om(x, mem, mem, key_padding_mask=pad, causal=kind == "self", return_attn_weights=False)}

    def step(name):
        x.grad = None
        if mem is not x:
            mem.grad = None
        for p in tm.parameters():                                # (ours accumulates into persistent fp32 gradients, as under the trainer)
            p.grad = None
        (fns[name]() * r).sum().backward()
    outs = {}
    for name in fns:
        for _ in range(3):
            step(name)
        outs[name] = (fns[name]().detach().float(), x.grad.detach().float().clone())
    torch.cuda.synchronize()
    inner = {name: max(2, math.ceil(min_window * 1e3 / window(lambda: step(name), 5))) for name in fns}
    times = {name: [] for name in fns}
    for it in range(reps):
        for name in (list(fns) if it % 2 == 0 else list(fns)[::-1]):
            times[name].append(window(lambda: step(name), inner[name]))
    ker = {"attn_fwd": [], "attn_bwd": [], "attn_weights": []}
    for _ in range(20):
        ops.prof_start()
        step("ours")
        for rec in ops.prof_stop():
            fam = rec[0].split(" ")[0]
            if fam in ker:
                ker[fam].append(rec[3])
    grids = {n: ops.attention_plan(B, L, S, H, D, dtype, w)["grid"] for n, w in (("fwd", _lib.ATTN_FWD), ("dkv", _lib.ATTN_BWD_DKV))}
    dev = {k: tuple(float((outs[k][i] - outs["torch"][i]).abs().max() / outs["torch"][i].abs().max()) for i in (0, 1)) for k in ("ours", "ours_train")}
    return {"kind": kind, "shape": (B, L, S, H, D), "dtype": str(dtype).split(".")[-1], "inner": inner,
            "ms": {k: (min(v), statistics.median(v), max(v)) for k, v in times.items()},
            "kernel_us": {k: statistics.median(v) * 1e3 for k, v in ker.items() if v}, "grids": grids, "dev": dev,
            "gflop": 4.0 * B * H * L * S * D * 3.5 / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_bench needs the GPU: there is nothing to time without one")
    rows = [bench_point(*pt, dt, a.reps, a.window) for pt in POINTS for dt in (torch.float32, torch.bfloat16)]
    lines = [f"MultiheadAttention forward + backward; ms per call: median (min .. max) of {a.reps} windows of >= {a.window} s per variant, "
             "variants alternated in both orders; (a) torch.nn.MultiheadAttention as upstream calls it, (b) this module, same arguments, "
             "weights returned, (c) this module, causal flag / no weights; kernel times: medians of 20 calls of (b) between ops' event "
             "brackets; grid = workgroups of the forward / dK-dV launch on 256 CUs; attention GFLOP = 4 B H L S D x 3.5 (fwd + bwd)"]
    for r in rows:
        m, (B, L, S, H, D) = r["ms"], r["shape"]
        lines.append(f"  {r['kind']:6s} B={B:3d} L={L:2d} S={S:3d} H={H} D={D:3d} {r['dtype']:8s} {r['gflop']:6.2f} GFLOP   "
                     + "   ".join(f"({tag}) {k} {m[k][1]:7.4f} ({m[k][0]:.4f} .. {m[k][2]:.4f})" for tag, k in zip("abc", ("torch", "ours", "ours_train")))
                     + f"   b/a {m['ours'][1] / m['torch'][1]:.3f}  c/a {m['ours_train'][1] / m['torch'][1]:.3f}")
        lines.append("        kernels of (b): " + "  ".join(f"{k} {v:7.1f} us" for k, v in r["kernel_us"].items())
                     + f"   grid fwd {math.prod(r['grids']['fwd'])} dkv {math.prod(r['grids']['dkv'])} workgroups"
                     + f"   max |out - out(a)| / max, same for d query: (b) {r['dev']['ours'][0]:.2e} {r['dev']['ours'][1]:.2e}"
                     + f"  (c) {r['dev']['ours_train'][0]:.2e} {r['dev']['ours_train'][1]:.2e}   calls per window {r['inner']}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""wav_augment (SpeedPerturb at speeds 95 and 105 of 16 kHz audio: the resample 20 -> 19 and 20 -> 21): this package's one launch
(functional.resample -> smx_resample) against the chain a user would otherwise run - torchaudio's _apply_sinc_resample_kernel
restated with upstream's ATen calls on the same GPU in the same process, in float32: F.pad, a strided F.conv1d with the (n, 1, K)
kernel, transpose + reshape (a copy), slice.  Points: (B, L) = (10, 240000) (the recipe's 150 s dynamic batch), (128, 80000) and
(128, 480000).  A run is --inner calls between two device events; per point the two paths alternate, in both orders; the figures
are medians over --reps runs after --warmup, per call, with the spread (10th to 90th percentile) of each side.  `ours beats` is
set only where the chain's median exceeds ours by more than the two spreads together.  `in a graph` is our launch replayed from a
hipGraph, without the host's enqueue cost per call.  At the largest point the 4 B (L + L_out) bytes the pass has to move, over
its time, are reported as a fraction of the 8 TB/s HBM roof (the measured copy ceiling of the part is 6.3 TB/s).

    python tools/speedperturb_bench.py [--reps 30 --warmup 5 --inner 10 --out FILE]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import functional as SF  # noqa: E402

POINTS = [(10, 240000), (128, 80000), (128, 480000)]
SPEEDS = [95, 105]
ORIG = 16000
HBM_BPS = 8.0e12


def aten_chain(x, plan, kernel):
    """torchaudio.functional.resample's _apply_sinc_resample_kernel on a (B, L) batch."""
    B, L = x.shape
    y = Fn.conv1d(Fn.pad(x[:, None, :], (plan.width, plan.width + plan.o)), kernel, stride=plan.o)
    return y.transpose(1, 2).reshape(B, -1)[..., :plan.out_len(L)]


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]


def bench_point(B, L, speed, reps, warmup, inner):
    torch.manual_seed(0)
    new = ORIG * speed // 100
    plan, _ = SF.resample_plan(ORIG, new, "cuda")
    x = torch.randn(B, L, device="cuda") * 0.1
    kernel = plan_kernel(plan).cuda()
    out = torch.empty(B, plan.out_len(L), device="cuda")
    ours = SF.resample(x, ORIG, new, out=out).clone()
    theirs = aten_chain(x, plan, kernel)
    dev = float((ours - theirs).abs().max())                  # two float32 evaluations of one sum: a few 1e-7 of |x|
    del ours, theirs
    paths = {"aten": lambda: aten_chain(x, plan, kernel), "ours": lambda: SF.resample(x, ORIG, new, out=out)}
    times = {k: [] for k in paths}
    for it in range(warmup + reps):
        for name in (list(paths) if it % 2 == 0 else list(paths)[::-1]):
            t = timed(paths[name], inner)
            if it >= warmup:
                times[name].append(t)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            SF.resample(x, ORIG, new, out=out)
    times["graph"] = [timed(g.replay, 1) / inner for _ in range(warmup + reps)][warmup:]
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: pct(v, 0.9) - pct(v, 0.1) for k, v in times.items()}
    nbytes = 4 * B * (L + plan.out_len(L))
    return {"B": B, "L": L, "speed": speed, "ms": med, "spread_ms": spread, "max_abs_dev": dev, "bytes": nbytes,
            "ours_beats": med["aten"] - med["ours"] > spread["aten"] + spread["ours"],
            "frac_hbm_roof": nbytes / HBM_BPS / (med["ours"] * 1e-3), "graph_frac_hbm_roof": nbytes / HBM_BPS / (med["graph"] * 1e-3)}


def plan_kernel(plan):
    """The (n, 1, K) float32 conv kernel of a plan: its runs of taps at their places."""
    k = torch.zeros(plan.n, 1, plan.K)
    first, w = plan.first().tolist(), plan.weights()
    for p in range(plan.n):
        m = min(plan.taps, plan.K - first[p])
        k[p, 0, first[p]:first[p] + m] = w[p, :m]
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("speedperturb_bench needs the GPU: there is nothing to time without one")
    rows = [bench_point(B, L, s, a.reps, a.warmup, a.inner) for (B, L) in POINTS for s in SPEEDS]
    lines = [f"wav_augment (SpeedPerturb, 16 kHz, speeds 95 / 105: resample 20 -> 19 / 20 -> 21, float32); median ms per call of {a.reps} "
             f"runs of {a.inner} calls after {a.warmup} warm-up runs, orders alternated, (spread: 10th to 90th percentile); roof = "
             f"4 B (L + L_out) bytes at {HBM_BPS / 1e12:.0f} TB/s"]
    for r in rows:
        m, s = r["ms"], r["spread_ms"]
        line = (f"  B={r['B']:3d} L={r['L']:6d} speed {r['speed']:3d}  ATen chain {m['aten']:8.4f} ({s['aten']:.4f})  ours {m['ours']:8.4f} "
                f"({s['ours']:.4f})  ours in a graph {m['graph']:8.4f} ({s['graph']:.4f})   ours/ATen {m['ours'] / m['aten']:.3f} "
                f"{'(beyond the two spreads)' if r['ours_beats'] else '(NOT beyond the two spreads)'}   max |ours - ATen| {r['max_abs_dev']:.1e}")
        if (r["B"], r["L"]) == POINTS[-1]:
            line += (f"   {r['bytes'] / 1e6:.1f} MB: the call at {r['frac_hbm_roof']:.2f} of the roof, in a graph "
                     f"{r['graph_frac_hbm_roof']:.2f}")
        lines.append(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""fea_augment (time drops 15-25 x 5, frequency drops 25-35 x 2, bicubic time warp, window 5 - the recipes' values): this package's
Augmenter (one draw launch + one pass, draws on the device) against the chain a user would otherwise run, upstream's ATen calls on
the same GPU in the same process - per drop stage the mask arithmetic and one masked_fill_, then two F.interpolate calls on slices
whose sizes are drawn on the host, and two slice copies.  Points: (B, T, F) = (128, 2000, 80) and (10, 1500, 80), float32 and
bfloat16.  A run is --inner calls between two device events; per point the two paths alternate, in both orders; the figures are
medians over --reps runs after --warmup, per call.  `apply` is smx_specaug_apply alone on a drawn block, called from Python like the
other two (all three carry the host's enqueue cost, which is what bounds the small point); `apply in a graph` is the same launch
replayed from a hipGraph, the kernel's own time: its 2 B T F sizeof bytes over that time are reported as a fraction of the 8 TB/s
HBM roof (the measured copy ceiling of the part is 6.3 TB/s; tensors below 256 MiB can sit in the Infinity Cache).

    python tools/specaug_bench.py [--reps 30 --warmup 5 --inner 10 --out FILE]"""
import argparse
import os
import random
import statistics
import sys

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import functional as SF  # noqa: E402
from summarymixing_amd import ops  # noqa: E402
from summarymixing_amd.augment.augmenter import Augmenter  # noqa: E402
from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping  # noqa: E402

POINTS = [(128, 2000, 80), (10, 1500, 80)]
HBM_BPS = 8.0e12
WINDOW = 5


def aten_drop(x, dim, len_lo, len_hi, cnt_lo, cnt_hi):
    """Upstream's SpectrogramDrop.forward with replace="zeros", in place."""
    B, D = x.shape[0], x.shape[dim]
    n = int(torch.randint(cnt_lo, cnt_hi + 1, (1,)))
    ln = torch.randint(len_lo, len_hi, (B, n), device=x.device).unsqueeze(2)
    pos = torch.randint(0, D, (B, n), device=x.device).unsqueeze(2)
    arange = torch.arange(D, device=x.device).view(1, 1, -1)
    mask = ((pos <= arange) * (arange < (pos + ln))).any(dim=1)
    return x.masked_fill_(mask.unsqueeze(2) if dim == 1 else mask.unsqueeze(1), 0.0)


def aten_warp(x):
    """Upstream's Warping.forward (bicubic, dim=1), in place."""
    y = x.unsqueeze(1)
    T = y.shape[2]
    if T - WINDOW <= WINDOW:
        return x
    c = random.randrange(WINDOW, T - WINDOW)
    w = random.randrange(c - WINDOW, c + WINDOW) + 1
    left = Fn.interpolate(y[:, :, :c], (w, y.shape[3]), mode="bicubic", align_corners=True)
    right = Fn.interpolate(y[:, :, c:], (T - w, y.shape[3]), mode="bicubic", align_corners=True)
    y[:, :, :w] = left
    y[:, :, w:] = right
    return x


def aten_chain(x):
    aten_drop(x, 1, 15, 25, 5, 5)
    aten_drop(x, 2, 25, 35, 2, 2)
    return aten_warp(x)


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_point(B, T, F, dtype, reps, warmup, inner):
    torch.manual_seed(0)
    random.seed(0)
    x = torch.randn(B, T, F, device="cuda").to(dtype)
    xa = x.clone()                                           # the ATen chain works in place
    aug = Augmenter(min_augmentations=3, max_augmentations=3, augmentations=[
        SpectrogramDrop(drop_length_low=15, drop_length_high=25, drop_count_low=5, drop_count_high=5, dim=1),
        SpectrogramDrop(drop_length_low=25, drop_length_high=35, drop_count_low=2, drop_count_high=2, dim=2), Warping()])
    lengths = torch.ones(B, device="cuda")
    aug(x, lengths)
    blk = aug.last_params
    paths = {"aten": lambda: aten_chain(xa), "fused": lambda: aug(x, lengths), "apply": lambda: SF.spec_augment(x, blk)}
    try:                                                     # (a torch build whose bicubic kernel lacks this dtype: the row says so)
        aten_chain(xa)
        torch.cuda.synchronize()
    except RuntimeError as e:
        print(f"  ATen chain unavailable in {dtype}: {str(e).splitlines()[0]}")
        del paths["aten"]
    times = {k: [] for k in paths}
    for it in range(warmup + reps):
        for name in (list(paths) if it % 2 == 0 else list(paths)[::-1]):
            if name == "aten":
                xa.copy_(x)                                  # (outside the timed window: the chain zeroes more of xa on every call)
            t = timed(paths[name], inner)
            if it >= warmup:
                times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    med.setdefault("aten", float("nan"))
    # the same apply launches replayed from a hipGraph: the kernel's own time, without the host's enqueue cost per call
    out = torch.empty_like(x)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            ops.specaug_apply(x, blk.data, blk.n_time_cap, blk.n_freq_cap, out=out)
    med["apply_graph"] = statistics.median([timed(g.replay, 1) / inner for _ in range(warmup + reps)][warmup:])
    nbytes = 2 * B * T * F * x.element_size()
    return {"B": B, "T": T, "F": F, "dtype": str(dtype).split(".")[-1], "ms": med, "min_ms": {k: min(v) for k, v in times.items()},
            "fused_over_aten": med["fused"] / med["aten"], "bytes": nbytes,
            "apply_frac_hbm_roof": nbytes / HBM_BPS / (med["apply_graph"] * 1e-3), "fused_frac_hbm_roof": nbytes / HBM_BPS / (med["fused"] * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specaug_bench needs the GPU: there is nothing to time without one")
    rows = [bench_point(B, T, F, dt, a.reps, a.warmup, a.inner) for (B, T, F) in POINTS for dt in (torch.float32, torch.bfloat16)]
    lines = [f"fea_augment (time drops 15-25 x 5, frequency drops 25-35 x 2, bicubic warp window 5); median ms per call of {a.reps} runs "
             f"of {a.inner} calls after {a.warmup} warm-up runs, orders alternated; roof = 2 B T F sizeof bytes at {HBM_BPS / 1e12:.0f} TB/s"]
    for r in rows:
        lines.append(f"  B={r['B']:3d} T={r['T']:4d} F={r['F']:3d} {r['dtype']:8s} ATen chain {r['ms']['aten']:7.4f}  fused (draw + apply) "
                     f"{r['ms']['fused']:7.4f}  apply alone {r['ms']['apply']:7.4f}  apply in a graph {r['ms']['apply_graph']:7.4f}   fused/ATen "
                     f"{r['fused_over_aten']:.3f}   {r['bytes'] / 1e6:6.1f} MB: the kernel at {r['apply_frac_hbm_roof']:.2f} of the roof, "
                     f"the fused call at {r['fused_frac_hbm_roof']:.2f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

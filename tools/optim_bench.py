#!/usr/bin/env python3
"""Time the optimizer update kernels on the MI355X: smx_sgd_step and smx_adamw_step (both with the bf16 shadow refresh) and
torch.optim.SGD(foreach=True) followed by the bf16 cast of the same flat buffer, at the flat sizes of the benchmark's C2b and
C2a models and at 1 M elements; plus what a learning-rate schedule on the device adds to the C2b update.

    python tools/optim_bench.py [--seconds 0.5] [--out profiles/optim_bench.txt]

Per size the three are run ALTERNATED in one process (round robin, one device-event pair per call) over a warmed window of at
least --seconds each; the time per call is the median, the spread the 10th .. 90th percentile.  Bytes are the algorithm's:
22 B per element for SGD with shadows (p read + write, g, buf read + write, one bf16), 30 B for AdamW (two moments), over the
8.0 TB/s HBM peak - next to the 6.29 TB/s a plain copy reaches on this part (MI355X_MICROARCH.md).  Needs the GPU: no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, COPY_RATE = 8.0e12, 6.29e12


def flat_size(config):
    """opt.total of a benchmark model: the flat layout is a function of the parameter shapes alone, so it is built on the CPU."""
    import bench
    from summarymixing_amd.trainer import FlatAdamW
    enc = bench.build_encoder(dict(bench.CONFIGS[config]), torch.device("cpu"), 0.0)
    return FlatAdamW(enc, compute_dtype=torch.float32).total


def timed_round_robin(calls, seconds, warmup=20):
    """calls: {name: fn}.  Alternate them until every one has at least `seconds` of device time -> {name: [ms per call]}."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    while min(sum(v) for v in times.values()) < seconds * 1e3:
        evs = []
        for _ in range(50):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                evs.append((k, e0, e1))
        torch.cuda.synchronize()
        for k, e0, e1 in evs:
            times[k].append(e0.elapsed_time(e1))
    return times


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def bench_size(n, seconds, emit):
    from summarymixing_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(n, device="cuda", generator=g)
    grad = 0.1 * torch.randn(n, device="cuda", generator=g)
    buf, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    shadow = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    pt = p.clone().requires_grad_(True)
    pt.grad = grad.clone()
    tsgd = torch.optim.SGD([pt], lr=1e-5, momentum=0.99, nesterov=True, foreach=True)
    tshadow = torch.zeros(n, device="cuda", dtype=torch.bfloat16)

    def torch_sgd():
        tsgd.step()
        tshadow.copy_(pt.detach())

    calls = {
        "smx_sgd_step": lambda: ops.sgd_step(p, grad, buf, shadow, 1e-5, 0.99, 0.0, True),
        "smx_adamw_step": lambda: ops.adamw_step(p, grad, m, v, shadow, 1e-5, 0.9, 0.98, 1e-8, 0.01, 10),
        "torch SGD(foreach) + bf16 cast": torch_sgd,
    }
    nbytes = {"smx_sgd_step": 22 * n, "smx_adamw_step": 30 * n, "torch SGD(foreach) + bf16 cast": 22 * n}
    times = timed_round_robin(calls, seconds)
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        rate = nbytes[k] / (med[k] * 1e-3)
        emit(f"  {k:32s} {med[k] * 1e3:9.1f} us/call  (p10 {pct(ts, 0.1) * 1e3:8.1f}, p90 {pct(ts, 0.9) * 1e3:8.1f}, {len(ts)} calls)  "
             f"{rate / 1e12:5.2f} TB/s of {nbytes[k] // n} B/elem = {100 * rate / HBM_PEAK:4.1f}% of the 8.0 TB/s peak, "
             f"{100 * rate / COPY_RATE:4.1f}% of the 6.29 TB/s copy rate")
    return med


def bench_schedule(seconds, emit):
    """What set_lr_schedule adds to the C2b update: the one-thread launch alone, and the update with and without it."""
    import bench
    from summarymixing_amd import _lib as L
    from summarymixing_amd import ops
    from summarymixing_amd.nnet.schedulers import NoamScheduler
    from summarymixing_amd.trainer import FlatAdamW
    out = torch.zeros(1, device="cuda")
    consts = (8e-4, 25000, 0.0, 0.0)
    k = 200

    def launches():
        for _ in range(k):
            ops.lr_schedule(L.LR_NOAM, consts, 8e-4, 1000, out)
    ts = timed_round_robin({"lr": launches}, seconds / 4, warmup=3)["lr"]
    emit(f"  smx_lr_schedule, {k} back-to-back launches: {statistics.median(ts) / k * 1e3:6.2f} us per launch "
         f"(p10 {pct(ts, 0.1) / k * 1e3:.2f}, p90 {pct(ts, 0.9) / k * 1e3:.2f})")
    enc = bench.build_encoder(dict(bench.CONFIGS["c2b"]), torch.device("cuda"), 0.0)
    opt = FlatAdamW(enc, lr=8e-4, compute_dtype=torch.bfloat16)
    opt.flat_g.normal_(0, 1e-3)
    opt.step_count = 10
    sched = NoamScheduler(8e-4, 25000)

    def plain():
        opt.set_lr_schedule(None)
        opt._apply_update(1.0)

    def scheduled():
        opt.set_lr_schedule(sched)
        opt._apply_update(1.0)
    times = timed_round_robin({"constant rate": plain, "Noam on the device": scheduled}, seconds)
    for name, ts in times.items():
        emit(f"  C2b update (sumsq + clip + AdamW), {name:20s} {statistics.median(ts) * 1e3:8.1f} us  "
             f"(p10 {pct(ts, 0.1) * 1e3:8.1f}, p90 {pct(ts, 0.9) * 1e3:8.1f}, {len(ts)} calls)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5, help="device time per kernel and size in the timed window (at least)")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs the GPU (times on a CPU say nothing about it)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"optim_bench on {torch.cuda.get_device_name(0)}: device-event medians, three kernels alternated, >= {args.seconds} s each")
    sizes = [("C2b flat size", flat_size("c2b")), ("C2a flat size", flat_size("c2a")), ("1 M elements", 1 << 20)]
    for name, n in sizes:
        emit(f"{name}: {n} elements")
        med = bench_size(n, args.seconds, emit)
        verdict = "at or below" if med["smx_sgd_step"] <= med["smx_adamw_step"] else "ABOVE"
        emit(f"  smx_sgd_step is {verdict} smx_adamw_step ({med['smx_sgd_step'] / med['smx_adamw_step']:.2f}x its time)")
    emit("learning-rate schedule on the device (C2b):")
    bench_schedule(args.seconds, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The recipes' second loss head, forward + backward from the logits (label_smoothing 0.1), three ways on the same GPU in one process:
  (a) aten    F.log_softmax + upstream's loss restated with its own ATen calls (kldiv_loss: clone / fill_ / scatter_ / F.kl_div /
              masked_fill; nll_loss: F.nll_loss and the mean over the vocabulary under the length mask) and torch's autograd;
  (b) pair    this package's drop-in pair: nnet.activations.Softmax(apply_log=True) + nnet.losses.kldiv_loss / nll_loss;
  (c) fused   nnet.losses.seq_loss_from_logits: one read of the logits forward, one read and one write backward.
Points: (B, U, V) = (64, 80, 5000) with kldiv_loss / batchmean (the Branchformer recipes' seq_cost) and (40, 48, 1000), (8, 64, 1000)
with nll_loss / mean (the transducer recipes' ce_cost, the prediction-network benchmark's shapes), float32 and bfloat16.
Every variant is warmed at every point, then timed in windows of at least --window seconds between two device events (the number of
calls per window is calibrated per variant), the variants alternating inside one process, in both orders; the figures are the median
and the extremes of --reps windows, per call.  A call carries the host's enqueue cost of its launches.  The kernels' own times come
from a separate pass with ops' event brackets around smx_seqloss_fwd / smx_seqloss_bwd; their algorithmic bytes (forward: B U V
sizeof, backward: 2 B U V sizeof, plus the per-row vectors) over that time are stated as a fraction of the 8 TB/s HBM roof (tensors
of tens of MB can sit in the Infinity Cache).

    python tools/seqloss_bench.py [--reps 5 --window 0.5 --out FILE]"""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import ops  # noqa: E402
from summarymixing_amd.nnet import losses  # noqa: E402
from summarymixing_amd.nnet.activations import Softmax  # noqa: E402

POINTS = [("kldiv", 64, 80, 5000), ("nll", 40, 48, 1000), ("nll", 8, 64, 1000)]
HBM_BPS = 8.0e12
EPS = 0.1


def aten_kldiv(lp, targets, pad_idx=0):
    """upstream kldiv_loss, label_smoothing > 0, reduction batchmean."""
    bz, _, n_class = lp.shape
    lp = lp.view(-1, n_class)
    targets = targets.view(-1)
    with torch.no_grad():
        true_distribution = lp.clone()
        true_distribution.fill_(EPS / (n_class - 1))
        ignore = targets == pad_idx
        targets = targets.masked_fill(ignore, 0)
        true_distribution.scatter_(1, targets.unsqueeze(1), 1 - EPS)
    loss = Fn.kl_div(lp, true_distribution, reduction="none")
    return loss.masked_fill(ignore.unsqueeze(1), 0).sum() / bz


def aten_nll(lp, targets, length):
    """upstream nll_loss, label_smoothing > 0, reduction mean (compute_masked_loss)."""
    B, U, _ = lp.shape
    mask = (torch.arange(U, device=lp.device, dtype=length.dtype)[None, :] < (length * U)[:, None]).to(lp.dtype)
    pred = lp.transpose(1, -1)
    loss = (Fn.nll_loss(pred, targets, reduction="none") * mask).sum() / mask.sum()
    reg = (torch.mean(pred, dim=1) * mask).sum() / mask.sum()
    return -EPS * reg + (1 - EPS) * loss


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def bench_point(kind, B, U, V, dtype, reps, min_window):
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(B, U, V, generator=g) * 2).to(dtype).cuda().requires_grad_(True)
    targets = torch.randint(1, V, (B, U), generator=g)
    rel = torch.rand(B, generator=g) * 0.5 + 0.5
    rel[0] = 1.0
    abs_len = (rel * U).ceil().long()
    targets[torch.arange(U)[None, :] >= abs_len[:, None]] = 0          # the padding token behind each utterance
    targets, rel = targets.cuda(), rel.cuda()
    log_softmax = Softmax(apply_log=True)
    if kind == "kldiv":
        fns = {"aten": lambda: aten_kldiv(Fn.log_softmax(z, -1), targets),
               "pair": lambda: losses.kldiv_loss(log_softmax(z), targets, rel, label_smoothing=EPS, reduction="batchmean"),
               "fused": lambda: losses.seq_loss_from_logits(z, targets, rel, EPS, kind="kldiv", reduction="batchmean")}
    else:
        fns = {"aten": lambda: aten_nll(Fn.log_softmax(z, -1), targets, rel),
               "pair": lambda: losses.nll_loss(log_softmax(z), targets, rel, label_smoothing=EPS),
               "fused": lambda: losses.seq_loss_from_logits(z, targets, rel, EPS, kind="nll")}

    def step(name):
        z.grad = None
        fns[name]().backward()
    vals, grads = {}, {}
    for name in fns:                                          # warm every variant at this point; keep what it computes
        for _ in range(3):
            step(name)
        vals[name] = float(fns[name]().detach())
        grads[name] = z.grad.detach().float().clone()
    torch.cuda.synchronize()
    inner = {name: max(2, math.ceil(min_window * 1e3 / window(lambda: step(name), 5))) for name in fns}
    times = {name: [] for name in fns}
    for it in range(reps):
        for name in (list(fns) if it % 2 == 0 else list(fns)[::-1]):
            times[name].append(window(lambda: step(name), inner[name]))
    # the two kernels of the fused form between ops' event brackets
    ker = {"seqloss_fwd": [], "seqloss_bwd": []}
    kbytes = {}
    for _ in range(20):
        ops.prof_start()
        step("fused")
        for rec in ops.prof_stop():
            fam = rec[0].split(" ")[0]
            if fam in ker:
                ker[fam].append(rec[3])
                kbytes[fam] = rec[1]
    scale = max(float(grads["aten"].abs().max()), 1e-30)
    return {"kind": kind, "B": B, "U": U, "V": V, "dtype": str(dtype).split(".")[-1], "inner": inner,
            "ms": {k: (min(v), statistics.median(v), max(v)) for k, v in times.items()},
            "kernel_ms": {k: statistics.median(v) for k, v in ker.items()}, "kernel_bytes": kbytes,
            "loss": vals, "grad_dev": {k: float((grads[k] - grads["aten"]).abs().max()) / scale for k in ("pair", "fused")},
            "logit_bytes": B * U * V * z.element_size()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seqloss_bench needs the GPU: there is nothing to time without one")
    rows = [bench_point(kind, B, U, V, dt, a.reps, a.window) for (kind, B, U, V) in POINTS for dt in (torch.float32, torch.bfloat16)]
    lines = [f"label-smoothed sequence loss, forward + backward from the logits, label_smoothing {EPS}; ms per call: median (min .. max) of "
             f"{a.reps} windows of >= {a.window} s per variant, variants alternated in both orders; kernel times: medians of 20 calls between "
             f"ops' event brackets; roof = algorithmic bytes at {HBM_BPS / 1e12:.0f} TB/s"]
    for r in rows:
        m = r["ms"]
        lines.append(f"  {r['kind']:5s} B={r['B']:2d} U={r['U']:2d} V={r['V']:4d} {r['dtype']:8s} logits {r['logit_bytes'] / 1e6:6.1f} MB   "
                     + "   ".join(f"({tag}) {k} {m[k][1]:7.4f} ({m[k][0]:.4f} .. {m[k][2]:.4f})" for tag, k in zip("abc", ("aten", "pair", "fused")))
                     + f"   fused/aten {m['fused'][1] / m['aten'][1]:.3f}  fused/pair {m['fused'][1] / m['pair'][1]:.3f}")
        lines.append("        kernels of (c): " + "  ".join(
            f"{k} {r['kernel_ms'][k] * 1e3:7.1f} us, {r['kernel_bytes'][k] / 1e6:6.1f} MB = {r['kernel_bytes'][k] / HBM_BPS / (r['kernel_ms'][k] * 1e-3):.3f} of the roof"
            for k in ("seqloss_fwd", "seqloss_bwd"))
            + f"   loss a/b/c {r['loss']['aten']:.6f} / {r['loss']['pair']:.6f} / {r['loss']['fused']:.6f}   max |dz - dz(a)| / max |dz(a)|: "
            f"pair {r['grad_dev']['pair']:.2e}, fused {r['grad_dev']['fused']:.2e}   calls per window {r['inner']}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

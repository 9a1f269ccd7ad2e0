"""Greedy transducer decoding at the recipe's validation point (T = 375 frames, V = 1000, H = 512, J = 640; B = 1, 4, 16; float32 and
bfloat16): nnet.transducer.greedy_decode, eager and as a CapturedGreedy replay, against the loop a user of this package had to write
before it existed - per frame the 4-D Tjoint at T = U+1 = 1, transducer_lin, torch.argmax, one .item() per row, dec at U = 1 with hx
on the emitted tokens, proj_dec - built from the package's public modules only, on the same GPU in the same process.  Per point the
three paths alternate in both orders; the figures are medians over --reps calls after --warmup (host wall time around a
synchronised call: the loop's cost IS its host synchronisation).  The transducer_lin bias is set so that about half the frames emit.

    python tools/greedy_bench.py [--reps 30 --warmup 5 --out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd.nnet import LSTM, Embedding  # noqa: E402
from summarymixing_amd.nnet.linear import Linear  # noqa: E402
from summarymixing_amd.nnet.transducer import CapturedGreedy, Transducer_joint, greedy_decode  # noqa: E402

T, V, H, J, BLANK = 375, 1000, 512, 640, 0
BATCHES = [1, 4, 16]
LAUNCHES_PER_FRAME = 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def user_loop(enc, emb, dec, proj, tj, lin):
    """What the parent commit's public modules allow: one host synchronisation per row and frame."""
    B = enc.shape[0]
    blank = torch.full((B, 1), BLANK, dtype=torch.long, device=enc.device)
    out, hx = dec(emb(blank))
    pdec = proj(out)                                                           # (B, 1, J)
    hyps = [[] for _ in range(B)]
    for t in range(enc.shape[1]):
        logits = lin(tj(enc[:, t:t + 1].unsqueeze(2), pdec.unsqueeze(1)))       # (B, 1, 1, V)
        k = torch.argmax(logits.view(B, V), 1)
        emit = []
        for b in range(B):
            kb = k[b].item()
            if kb != BLANK:
                hyps[b].append(kb)
                emit.append(b)
        if emit:
            out2, hx2 = dec(emb(k.view(B, 1)), hx)
            m = (k != BLANK).view(1, B, 1)
            hx = (torch.where(m, hx2[0], hx[0]), torch.where(m, hx2[1], hx[1]))
            pdec = torch.where(m.view(B, 1, 1), proj(out2), pdec)
    return hyps


def bench_point(B, dtype, reps, warmup):
    torch.manual_seed(0)
    emb = Embedding(V, consider_as_one_hot=True, blank_id=BLANK).cuda().to(dtype)
    dec = LSTM(H, input_size=V - 1).cuda()
    proj = Linear(J, input_size=H, bias=False).cuda()
    tj = Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU)
    lin = Linear(V, input_size=J).cuda()
    enc = torch.randn(B, T, J, device="cuda").to(dtype)
    mods = (emb, dec, proj, tj, lin)
    with torch.no_grad():
        # the blank's bias: the median shortfall of the blank logit at the start state, so about half the frames emit
        z = lin(tj(enc.unsqueeze(2), proj(dec(emb(torch.full((B, 1), BLANK, device="cuda")))[0]).unsqueeze(1))).float().view(B, T, V)
        other = z.clone()
        other[..., BLANK] = -float("inf")
        lin.w.bias[BLANK] += (other.max(-1).values - z[..., BLANK]).median()
        cap = CapturedGreedy(*mods, B=B, T=T, dtype=dtype)
        res = {}
        paths = {"loop": lambda: res.__setitem__("loop", user_loop(enc, *mods)),
                 "eager": lambda: res.__setitem__("eager", greedy_decode(enc, *mods)),
                 "captured": lambda: res.__setitem__("captured", cap.decode(enc))}
        times = {k: [] for k in paths}
        for it in range(warmup + reps):
            order = list(paths) if it % 2 == 0 else list(paths)[::-1]
            for name in order:
                t = timed(paths[name])
                if it >= warmup:
                    times[name].append(t)
    n = res["eager"].counts.cpu()
    tk = res["eager"].tokens.cpu()
    agree = sum(tk[b, :n[b]].tolist() == res["loop"][b] for b in range(B))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"B": B, "T": T, "dtype": str(dtype).split(".")[-1], "ms": med, "min_ms": {k: min(v) for k, v in times.items()},
            "us_per_frame": {k: 1e3 * v / T for k, v in med.items()}, "launches_per_frame": LAUNCHES_PER_FRAME,
            "emitted": int(n.sum()), "frames": B * T, "rows_equal_to_loop": f"{agree}/{B}",
            "eager_over_loop": med["eager"] / med["loop"], "captured_over_loop": med["captured"] / med["loop"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [bench_point(B, dt, a.reps, a.warmup) for B in BATCHES for dt in (torch.float32, torch.bfloat16)]
    lines = [f"greedy decoding, T={T} V={V} H={H} J={J}; median ms of {a.reps} after {a.warmup} warm-up, orders alternated; "
             f"{LAUNCHES_PER_FRAME} launches per frame"]
    for r in rows:
        lines.append(f"  B={r['B']:3d} {r['dtype']:8s} user loop {r['ms']['loop']:8.3f} ms   eager {r['ms']['eager']:7.3f} ms "
                     f"({r['us_per_frame']['eager']:6.2f} us/frame)   captured {r['ms']['captured']:7.3f} ms "
                     f"({r['us_per_frame']['captured']:6.2f} us/frame)   eager/loop {r['eager_over_loop']:.3f}  captured/loop "
                     f"{r['captured_over_loop']:.3f}   emitted {r['emitted']}/{r['frames']}   rows equal to the loop's {r['rows_equal_to_loop']}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

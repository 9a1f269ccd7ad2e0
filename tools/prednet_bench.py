"""Prediction network (emb -> dec -> proj_dec; V = 1000, H = 512, J = 640) forward + backward: the drop-in chain and the fused
prediction_network of this package against the chain the recipe runs today, torch.nn.Embedding (frozen one-hot table) ->
torch.nn.LSTM -> torch.nn.Linear, on the same GPU in the same process.  Points: (B, U + 1) = (8, 64), the recipe's batch_size, and
(40, 48), many short utterances as dynamic batching packs them; float32 and bfloat16.  Per point the three paths alternate in both
orders; the figures are medians over --reps calls after --warmup.  Two more columns time the drop-in LSTM alone on a dense input
of I = 999 (zero-padded to 1024 on the host, every call) and of I = 1024 (no padding): their difference is what the padding costs,
apart from the recurrence.

    python tools/prednet_bench.py [--reps 30 --warmup 5 --out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd.nnet import LSTM, Embedding  # noqa: E402
from summarymixing_amd.nnet.linear import Linear  # noqa: E402
from summarymixing_amd.nnet.transducer import prediction_network  # noqa: E402

V, H, J, BLANK = 1000, 512, 640, 0
POINTS = [(8, 64), (40, 48)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench_point(B, U1, dtype, reps, warmup):
    torch.manual_seed(0)
    emb = Embedding(V, consider_as_one_hot=True, blank_id=BLANK).cuda().to(dtype)
    dec = LSTM(H, input_shape=[None, None, V - 1]).cuda()
    proj = Linear(J, input_size=H, bias=False).cuda()
    t_emb = torch.nn.Embedding(V, V - 1).cuda().to(dtype)
    t_emb.weight.data.copy_(emb.Embedding.weight)
    t_emb.weight.requires_grad = False
    t_dec = torch.nn.LSTM(V - 1, H, batch_first=True).cuda().to(dtype)
    t_proj = torch.nn.Linear(H, J, bias=False).cuda().to(dtype)
    tokens = torch.randint(0, V, (B, U1), device="cuda")
    tokens[:, 0] = BLANK
    dOut = torch.randn(B, U1, J, device="cuda").to(dtype)
    mods = (dec, proj, t_dec, t_proj)

    def torch_chain():
        return t_proj(t_dec(t_emb(tokens))[0])

    def dropin():
        return proj(dec(emb(tokens))[0])

    def fused():
        return prediction_network(tokens, emb, dec, proj)

    dec_1024 = LSTM(H, input_shape=[None, None, 1024]).cuda()
    x999 = torch.randn(B, U1, V - 1, device="cuda").to(dtype).requires_grad_(True)
    x1024 = torch.randn(B, U1, 1024, device="cuda").to(dtype).requires_grad_(True)
    dH = torch.randn(B, U1, H, device="cuda").to(dtype)
    mods += (dec_1024,)
    paths = {"torch": torch_chain, "drop-in": dropin, "fused": fused}
    lstm_only = {"lstm I=999": lambda: dec(x999)[0].backward(dH), "lstm I=1024": lambda: dec_1024(x1024)[0].backward(dH)}
    try:                                           # (a torch build whose LSTM back end lacks this dtype: the row says so)
        torch_chain().backward(dOut)
        torch.cuda.synchronize()
    except RuntimeError as e:
        print(f"  torch chain unavailable in {dtype}: {str(e).splitlines()[0]}")
        del paths["torch"]
    times = {k: [] for k in paths}
    for it in range(warmup + reps):
        order = list(paths) if it % 2 == 0 else list(paths)[::-1]
        for name in order:
            for m in mods:
                m.zero_grad(set_to_none=True)
            t = timed(lambda: paths[name]().backward(dOut))
            if it >= warmup:
                times[name].append(t)
        for name, fn in lstm_only.items():
            for m in mods:
                m.zero_grad(set_to_none=True)
            x999.grad = x1024.grad = None
            t = timed(fn)
            if it >= warmup:
                times.setdefault(name, []).append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    med.setdefault("torch", float("nan"))
    return {"B": B, "U1": U1, "dtype": str(dtype).split(".")[-1], "ms": med, "min_ms": {k: min(v) for k, v in times.items()},
            "fused_over_torch": med["fused"] / med["torch"], "dropin_over_torch": med["drop-in"] / med["torch"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [bench_point(B, U1, dt, a.reps, a.warmup) for (B, U1) in POINTS for dt in (torch.float32, torch.bfloat16)]
    print(f"prediction network forward + backward, V={V} H={H} J={J}; median ms of {a.reps} after {a.warmup} warm-up, orders alternated")
    for r in rows:
        print(f"  B={r['B']:3d} U+1={r['U1']:3d} {r['dtype']:8s} torch {r['ms']['torch']:7.3f}  drop-in {r['ms']['drop-in']:7.3f}  "
              f"fused {r['ms']['fused']:7.3f}   fused/torch {r['fused_over_torch']:.2f}  drop-in/torch {r['dropin_over_torch']:.2f}"
              f"   LSTM alone, dense I=999 (padded) {r['ms']['lstm I=999']:7.3f}  I=1024 {r['ms']['lstm I=1024']:7.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

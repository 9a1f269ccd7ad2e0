"""The RNN language model's decode step at the recipe's size (V = 1000, E = 128, H = 2048, L = 2, dnn 512; B = 1, 10, 80 rows = batch x
beam; bfloat16 and float32): lobes.models.RNNLM fed one token per row with hx fed back, against
  (a) the route a user could write from the parent's public modules: torch.nn.functional.embedding, two one-layer nnet.RNN.LSTM at
      U = 1 with hx (a GEMM launch for the input product + a recurrence launch per layer), and the same head;
  (b) torch.nn.Embedding + torch.nn.LSTM(num_layers=2) on the same device, and the same head.
All three run in one process on the same weights; per point they alternate in both orders, a sample is the device-event time of
--inner back-to-back steps (state fed back) divided by --inner, the figure the median of --reps samples after --warmup.  Back-to-back
steps are the beam search's situation: the 103 MB (bf16) of LSTM weights stay in the 256 MiB Infinity Cache between steps.  Also
timed alone, the same way: smx_lstm_step per layer, whose weight bytes over its time are reported as a fraction of the 8 TB/s HBM
roof bench.py uses.  The margin of "not slower than (a)" is (a)'s own interquartile spread in this process.

    python tools/rnnlm_bench.py [--reps 30 --warmup 5 --inner 20 --out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import ops  # noqa: E402
from summarymixing_amd.lobes.models.RNNLM import RNNLM  # noqa: E402
from summarymixing_amd.nnet import LSTM  # noqa: E402
from summarymixing_amd.nnet.RNN import lstm_weights  # noqa: E402

V, E, H, L, D = 1000, 128, 2048, 2, 512
BATCHES = [1, 10, 80]
HBM_GBPS = 8000.0


def timed_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def quart(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def bench_point(B, dtype, reps, warmup, inner):
    torch.manual_seed(0)
    lm = RNNLM(V, embedding_dim=E, rnn_layers=L, rnn_neurons=H, dnn_neurons=D, dropout=0.0, return_hidden=True).cuda().eval()
    if dtype == torch.bfloat16:
        lm.embedding.to(dtype)
    p = lm.rnn.rnn
    decs = []
    for k in range(L):
        dec = LSTM(H, input_size=E if k == 0 else H).cuda()
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            getattr(dec.rnn, f"{n}_l0").data = getattr(p, f"{n}_l{k}").data
        decs.append(dec)
    ref = torch.nn.LSTM(E, H, num_layers=L, batch_first=True).cuda()
    ref.load_state_dict({n: q for n, q in p.state_dict().items()})
    ref = ref.to(dtype)
    table = lm.embedding.Embedding.weight.detach()
    tok = torch.randint(0, V, (B,), device="cuda")
    st = {}

    def ours():
        _, st["ours"] = lm(tok, st.get("ours"))

    def user():
        x = torch.nn.functional.embedding(tok, table).unsqueeze(1)
        hx = st.get("user") or [None] * L
        new = []
        for k in range(L):
            x, hk = decs[k](x, hx[k])
            new.append(hk)
        st["user"] = new
        lm._head(x.view(B, H), dtype)

    def torch_lstm():
        x = torch.nn.functional.embedding(tok, table).unsqueeze(1)
        y, st["torch"] = ref(x, st.get("torch"))
        lm._head(y.reshape(B, H), dtype)

    Wl = [lstm_weights(p, k, dtype) for k in range(L)]
    tk32 = tok.to(torch.int32)
    bufs = [(torch.randn(B, H, device="cuda").to(dtype), torch.randn(B, H, device="cuda"), torch.empty(B, H, device="cuda", dtype=dtype),
             torch.empty(B, H, device="cuda")) for _ in range(L)]
    xin = torch.randn(B, H, device="cuda").to(dtype)

    def layer0():
        ops.lstm_step(table, *Wl[0], bufs[0][0], bufs[0][1], bufs[0][2], bufs[0][3], tokens=tk32)

    def layer1():
        ops.lstm_step(xin, *Wl[1], bufs[1][0], bufs[1][1], bufs[1][2], bufs[1][3])

    paths = {"rnnlm": ours, "user": user, "torch": torch_lstm, "layer0": layer0, "layer1": layer1}
    with torch.no_grad():
        try:                                                    # (torch's LSTM may not take this dtype on this device: then (b) is absent)
            torch_lstm()
            torch.cuda.synchronize()
        except RuntimeError as e:
            print(f"torch.nn.LSTM {dtype} B={B}: {str(e).splitlines()[0]}", file=sys.stderr)
            del paths["torch"]
            st.pop("torch", None)
    times = {k: [] for k in paths}
    with torch.no_grad():
        for it in range(warmup + reps):
            order = list(paths) if it % 2 == 0 else list(paths)[::-1]
            for name in order:
                t = timed_us(paths[name], inner)
                if it >= warmup:
                    times[name].append(t)
    med = {k: statistics.median(v) for k, v in times.items()}
    q1, q3 = quart(times["user"])
    es = 2 if dtype == torch.bfloat16 else 4
    wbytes = [4 * H * (E + H) * es, 4 * H * (H + H) * es]
    frac = [wbytes[k] / (med[f"layer{k}"] * 1e-6) / 1e9 / HBM_GBPS for k in range(L)]
    return {"B": B, "dtype": str(dtype).split(".")[-1], "us": med, "min_us": {k: min(v) for k, v in times.items()},
            "user_iqr_us": q3 - q1, "rnnlm_over_user": med["rnnlm"] / med["user"], "rnnlm_over_torch": med["rnnlm"] / med["torch"] if "torch" in med else None,
            "not_slower_than_user": bool(med["rnnlm"] <= med["user"] + (q3 - q1)), "weight_bytes": wbytes, "frac_hbm_roof": frac,
            "frac_hbm_roof_both_layers": sum(wbytes) / ((med["layer0"] + med["layer1"]) * 1e-6) / 1e9 / HBM_GBPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [bench_point(B, dt, a.reps, a.warmup, a.inner) for dt in (torch.bfloat16, torch.float32) for B in BATCHES]
    lines = [f"RNNLM decode step, V={V} E={E} H={H} L={L} dnn={D}; median us per step of {a.reps} samples ({a.inner} back-to-back steps each) "
             f"after {a.warmup} warm-ups, orders alternated; (a) = embedding + two nnet.RNN.LSTM at U = 1, (b) = torch.nn.LSTM(num_layers=2)"]
    for r in rows:
        u = dict(r["us"])
        u.setdefault("torch", float("nan"))
        r = dict(r, rnnlm_over_torch=r["rnnlm_over_torch"] if r["rnnlm_over_torch"] is not None else float("nan"))
        lines.append(f"  {r['dtype']:8s} B={r['B']:3d}  RNNLM {u['rnnlm']:8.1f} us   (a) {u['user']:8.1f} us (IQR {r['user_iqr_us']:5.1f})   (b) {u['torch']:8.1f} us   "
                     f"RNNLM/(a) {r['rnnlm_over_user']:.3f}  RNNLM/(b) {r['rnnlm_over_torch']:.3f}  not slower than (a): {r['not_slower_than_user']}   "
                     f"lstm_step layer 0 {u['layer0']:6.1f} us, layer 1 {u['layer1']:6.1f} us; weight bytes / time = "
                     f"{r['frac_hbm_roof'][0]:.2f}, {r['frac_hbm_roof'][1]:.2f} of the {HBM_GBPS / 1e3:.0f} TB/s roof (both layers {r['frac_hbm_roof_both_layers']:.2f})")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

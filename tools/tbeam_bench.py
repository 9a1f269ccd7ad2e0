"""Transducer beam search at the recipe's test point (T = 375 frames, V = 1000, H = 512, J = 640, beam 10, state_beam = expand_beam = 2.3;
the recipe's RNNLM - 2 x 2048, embedding 128, DNN 512, lm_weight 0.5 - on and off; B = 1 and 8; float32 and bfloat16):
nnet.transducer.beam_decode, eager and as CapturedTransducerBeam replays, against the loop a user of this package had to write before it
existed - upstream's search restated over the package's public modules (Embedding / LSTM at U = 1 with hx, proj_dec, Tjoint,
transducer_lin, RNNLM's decode step, torch.topk, Python lists), one hypothesis at a time - on the same GPU, inputs and result.
The transducer_lin bias of the blank is bisected, per point, until the best hypothesis emits on 25-75 % of the frames and no cap is
hit - at max_expansions 4 W, then at 16 W; a point where neither succeeds is reported as a "capped search" - and the emission rate and
the expansions per frame are reported, since the time depends on them.  Figures are medians over --reps searches after
--warmup (host wall time around a synchronised call); the user loop runs --loop-reps times.

    python tools/tbeam_bench.py [--reps 5 --warmup 1 --loop-reps 1 --out profiles/tbeam_bench.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd.lobes.models.RNNLM import RNNLM  # noqa: E402
from summarymixing_amd.nnet import LSTM, Embedding  # noqa: E402
from summarymixing_amd.nnet.linear import Linear  # noqa: E402
from summarymixing_amd.nnet.transducer import CapturedTransducerBeam, Transducer_joint, beam_decode  # noqa: E402

T, V, H, J, BLANK, W = 375, 1000, 512, 640, 0, 10
LM_WEIGHT, STATE_BEAM, EXPAND_BEAM = 0.5, 2.3, 2.3
BATCHES = [1, 8]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def user_loop(enc, emb, dec, proj, tj, lin, lm, E):
    """Upstream's search, one utterance and one hypothesis at a time, with the expansion cap the device search has."""
    out = []
    for b in range(enc.shape[0]):
        Bh = [dict(pred=[BLANK], s=0.0, dec=None, lm=None)]
        for t in range(enc.shape[1]):
            A, Bh, nexp = Bh, [], 0
            key = lambda h: h["s"] / len(h["pred"])
            while len(Bh) < W and nexp < E and A:
                a = max(A, key=key)
                if Bh and max(Bh, key=key)["s"] >= STATE_BEAM + a["s"]:
                    break
                A.remove(a)
                nexp += 1
                tok = torch.full((1, 1), a["pred"][-1], dtype=torch.long, device=enc.device)
                o, hid = dec(emb(tok), a["dec"])
                z = lin(tj(enc[b:b + 1, t:t + 1].unsqueeze(2), proj(o).unsqueeze(1))).view(-1)
                lp = torch.log_softmax(z.float(), -1)
                if lm is not None:
                    lz, lm_hid = lm(tok.view(1), a["lm"])
                    lm_lp = torch.log_softmax(lz.view(-1).float(), -1)
                v, idx = torch.topk(lp, W)
                v, idx = v.tolist(), idx.tolist()                           # the host synchronisation of every expansion
                best = v[0] if idx[0] != BLANK else v[1]
                lmv = lm_lp[idx].tolist() if lm is not None else None
                for j in range(W):
                    if idx[j] == BLANK:
                        Bh.append(dict(pred=a["pred"], s=a["s"] + v[j], dec=a["dec"], lm=a["lm"]))
                    elif v[j] >= best - EXPAND_BEAM:
                        A.append(dict(pred=a["pred"] + [idx[j]], s=a["s"] + v[j] + (LM_WEIGHT * lmv[j] if lm is not None else 0.0), dec=hid,
                                      lm=lm_hid if lm is not None else None))
            if len(Bh) < W and nexp >= E:
                Bh += sorted(A, key=key, reverse=True)[:W - len(Bh)]
        out.append(max(Bh, key=lambda h: h["s"] / len(h["pred"]))["pred"][1:])
    return out


def bench_point(B, dtype, use_lm, a):
    torch.manual_seed(0)
    emb = Embedding(V, consider_as_one_hot=True, blank_id=BLANK).cuda().to(dtype)
    dec, proj = LSTM(H, input_size=V - 1).cuda(), Linear(J, input_size=H, bias=False).cuda()
    tj, lin = Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU), Linear(V, input_size=J).cuda()
    lm = None
    if use_lm:
        lm = RNNLM(V, embedding_dim=128, rnn_layers=2, rnn_neurons=2048, dnn_neurons=512, dropout=0.0, return_hidden=True).cuda().eval()
        lm = lm.bfloat16() if dtype == torch.bfloat16 else lm
    enc = torch.randn(B, T, J, device="cuda").to(dtype)
    mods = (emb, dec, proj, tj, lin)
    with torch.no_grad():
        z = lin(tj(enc.unsqueeze(2), proj(dec(emb(torch.full((B, 1), BLANK, device="cuda")))[0]).unsqueeze(1))).float().view(B, T, V)
        other = z.clone()
        other[..., BLANK] = -float("inf")
        kw = dict(lm=lm, lm_weight=LM_WEIGHT if use_lm else 0.0, state_beam=STATE_BEAM, expand_beam=EXPAND_BEAM)
        # the blank's bias: bisected from its median shortfall at the start state until the best hypothesis emits on 25-75 % of the
        # frames and no cap is hit (the LM's share shifts every other token by about 0.5 log(1 / V))
        base = lin.w.bias[BLANK] + (other.max(-1).values - z[..., BLANK]).median()
        # at the default expansion cap (4 W) first; where no bias in the band avoids it (the random LM spreads the keys), at 16 W; a point
        # that still hits a cap is marked "capped search" in the report
        for E in (4 * W, 16 * W):
            kw["max_expansions"] = E
            lo, hi, calibrated, in_band = -12.0, 12.0, False, None
            for _ in range(12):
                mid = 0.5 * (lo + hi)
                lin.w.bias[BLANK] = base + mid
                r = beam_decode(enc, *mods, W, **kw)
                rate = float(r.lengths[:, 0].float().mean()) / T
                if 0.25 <= rate <= 0.75:
                    in_band = mid
                    if int(r.overflow.max()) == 0:
                        calibrated = True
                        break
                lo, hi = (mid, hi) if rate > 0.5 else (lo, mid)
            if calibrated:
                break
        blank_bias = mid if calibrated or in_band is None else in_band      # (not calibrated: the last bias inside the band)
        lin.w.bias[BLANK] = base + blank_bias
        cap = CapturedTransducerBeam(*mods, B, T, W, dtype=dtype, **kw)
        res = {}
        paths = {"eager": lambda: res.__setitem__("eager", beam_decode(enc, *mods, W, **kw)),
                 "captured": lambda: res.__setitem__("captured", cap.decode(enc))}
        times = {k: [] for k in paths}
        for it in range(a.warmup + a.reps):
            for name in (list(paths) if it % 2 == 0 else list(paths)[::-1]):
                t = timed(paths[name])
                if it >= a.warmup:
                    times[name].append(t)
        times["loop"] = [timed(lambda: res.__setitem__("loop", user_loop(enc, *mods, lm, E))) for _ in range(a.loop_reps)]
    r = res["eager"]
    n, tk, exp = r.lengths[:, 0].cpu(), r.tokens[:, 0].cpu(), r.expansions.cpu()
    same = torch.equal(res["captured"].tokens, r.tokens)
    agree = sum(tk[b, :n[b]].tolist() == res["loop"][b] for b in range(B))
    med = {k: statistics.median(v) for k, v in times.items()}
    steps = -(-int(exp.max()) // 32) * 32                                         # the steps issued: polled every 32
    return {"B": B, "dtype": str(dtype).split(".")[-1], "lm": use_lm, "ms": med, "min_ms": {k: min(v) for k, v in times.items()},
            "steps": steps, "ms_per_step": {k: med[k] / steps for k in ("eager", "captured")}, "ms_per_utt": {k: v / B for k, v in med.items()},
            "expansions_per_frame": float(exp.float().mean()) / T, "emission_rate": float(n.float().mean()) / T, "overflow": r.overflow.cpu().tolist(), "blank_bias": blank_bias,
            "max_expansions": E, "calibrated": calibrated,
            "captured_equals_eager": same, "best_equal_to_loop": f"{agree}/{B}", "captured_over_loop": med["captured"] / med["loop"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [bench_point(B, dt, lm, a) for lm in (False, True) for B in BATCHES for dt in (torch.float32, torch.bfloat16)]
    lines = [f"transducer beam search, T={T} V={V} H={H} J={J} beam={W}; median ms of {a.reps} searches after {a.warmup} warm-up, orders alternated; "
             f"user loop: {a.loop_reps} run(s)"]
    for r in rows:
        lines.append(f"  lm={'on ' if r['lm'] else 'off'} B={r['B']} {r['dtype']:8s} user loop {r['ms']['loop']:9.1f} ms   eager {r['ms']['eager']:8.2f} ms "
                     f"({1e3 * r['ms_per_step']['eager']:6.1f} us/step)   captured {r['ms']['captured']:8.2f} ms ({1e3 * r['ms_per_step']['captured']:6.1f} us/step, "
                     f"{r['ms_per_utt']['captured']:7.2f} ms/utterance)   captured/loop {r['captured_over_loop']:.4f}   steps {r['steps']}   expansions/frame "
                     f"{r['expansions_per_frame']:.2f}   emission rate {r['emission_rate']:.2f}   overflow {r['overflow']}   max_expansions {r['max_expansions']}{'' if r['calibrated'] else ' CAPPED SEARCH (no bias in the band avoids the caps)'}   best equal to the loop's "
                     f"{r['best_equal_to_loop']}   captured == eager {r['captured_equals_eager']}")
    for B in BATCHES:
        for dt in ("float32", "bfloat16"):
            on = next(r for r in rows if r["lm"] and r["B"] == B and r["dtype"] == dt)
            off = next(r for r in rows if not r["lm"] and r["B"] == B and r["dtype"] == dt)
            s_on, s_off = on["ms_per_step"]["captured"], off["ms_per_step"]["captured"]
            lines.append(f"  B={B} {dt}: the LM's share of a captured step {(s_on - s_off) / s_on:.2f} ({1e3 * s_off:.1f} -> {1e3 * s_on:.1f} us/step)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

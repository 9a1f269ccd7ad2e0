"""The transducer beam search carried across streaming chunks at the recipe's test point: T = 375 frames fed in chunks of
32 (the recipe's test_chunk_size; the last chunk holds 23), V = 1000, H = 512, J = 640, beam 10, state_beam = expand_beam = 2.3, the
recipe's RNNLM (2 x 2048, embedding 128, DNN 512, lm_weight 0.5) on and off, B = 1 and 8, float32 and bfloat16.

Measured, all in one process and alternated rep by rep (host wall time around work that ends in a device synchronise):
  whole    CapturedTransducerBeam.decode over the whole utterance: ms, the steps it issued, us per step;
  stream   a captured TransducerBeamStream fed the same utterance chunk by chunk, synchronised after every chunk as a user who reads the
           partial hypotheses is: ms per utterance, the steps issued over all chunks, us per step, and ms per chunk (every chunk of every
           rep: median, min, max);
  pause    B = 1 only: the selection launch that ends a chunk (result write + turnover) against the same launch on the same state with
           one more frame to come (turnover alone), device events around the one launch, the state restored before every repetition.
The blank's bias is bisected as tools/tbeam_bench.py does it, until the best hypothesis emits on 25-75 % of the frames and no cap is hit
(at max_expansions 4 W, then 16 W).  Every point also checks that the streamed result equals the whole one on every field.

    python tools/tbeam_stream_bench.py [--reps 7 --warmup 2 --out profiles/tbeam_stream_bench.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import ops  # noqa: E402
from summarymixing_amd.lobes.models.RNNLM import RNNLM  # noqa: E402
from summarymixing_amd.nnet import LSTM, Embedding  # noqa: E402
from summarymixing_amd.nnet.linear import Linear  # noqa: E402
from summarymixing_amd.nnet.transducer import CapturedTransducerBeam, TransducerBeamStream, Transducer_joint, beam_decode  # noqa: E402

T, C, V, H, J, BLANK, W = 375, 32, 1000, 512, 640, 0, 10
U = 2 * T + 8
LM_WEIGHT, STATE_BEAM, EXPAND_BEAM = 0.5, 2.3, 2.3
BATCHES = [1, 8]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def calibrate(enc, mods, lin, kw):
    """The blank's bias and max_expansions at which the search emits on 25-75 % of the frames without hitting a cap (tools/tbeam_bench.py)."""
    emb, dec, proj, tj, _ = mods
    B = enc.shape[0]
    z = lin(tj(enc.unsqueeze(2), proj(dec(emb(torch.full((B, 1), BLANK, device="cuda")))[0]).unsqueeze(1))).float().view(B, T, V)
    other = z.clone()
    other[..., BLANK] = -float("inf")
    base = lin.w.bias[BLANK] + (other.max(-1).values - z[..., BLANK]).median()
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
    lin.w.bias[BLANK] = base + (mid if calibrated or in_band is None else in_band)
    return calibrated


def chunks_of(enc):
    out = []
    for at in range(0, T, C):
        n = min(C, T - at)
        x = torch.zeros((enc.shape[0], C, J), dtype=enc.dtype, device=enc.device)
        x[:, :n] = enc[:, at:at + n]
        out.append((x, [n] * enc.shape[0]))
    return out


def pause_cost(s, chunk, reps):
    """B = 1.  Runs one chunk of C - 1 frames step by step to the step that ends it, keeps the state before that step, and times the
    selection launch alone: with lengths = C - 1 it is a pause (result write + turnover), with lengths = C an ordinary frame end."""
    st = s.state
    x, _ = chunk
    s.decode_chunk(x, [0], start=[True])                                     # a started slot with the chunk copied in
    st.lengths.fill_(C - 1)
    ops.tbeam_resume(st)
    tensors = {k: v for k, v in vars(st).items() if isinstance(v, torch.Tensor) and k not in ("WihT", "bias", "Whh", "Wproj", "Wlin", "blin", "enc")}
    for _ in range((C - 1) * st.E):
        before = {k: v.clone() for k, v in tensors.items()}
        st.step()
        if int(st.done[0]):
            break
    out = {}
    for name, length in (("pause", C - 1), ("frame_end", C)):
        us = []
        for _ in range(reps + 2):
            for k, v in tensors.items():
                v.copy_(before[k])
            st.lengths.fill_(length)
            ops.tbeam_step(st)
            logits = None if st.lm is None else st.lm.step(st.cur_tok, hx=(st.lm_h_in, st.lm_c_in), out=(st.lm_h_out, st.lm_c_out))[0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            ops.tbeam_select_stream(st, logits)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        assert int(st.done[0]) == (1 if name == "pause" else 0), "the step kept is not the one that ends the chunk"
        out[name] = spread(us[2:])
    out["extra_us"] = out["pause"]["median"] - out["frame_end"]["median"]
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
    kw = dict(lm=lm, lm_weight=LM_WEIGHT if use_lm else 0.0, state_beam=STATE_BEAM, expand_beam=EXPAND_BEAM)
    with torch.no_grad():
        calibrated = calibrate(enc, mods, lin, kw)
        whole = CapturedTransducerBeam(*mods, B, T, W, max_symbols=U, dtype=dtype, **kw)
        stream = TransducerBeamStream(*mods, B, C, W, U, dtype=dtype, captured=True, **kw)
        parts = chunks_of(enc)
        count = {"steps": 0}
        replay = stream._step

        def counted():
            count["steps"] += 1
            replay()
        stream._step = counted
        per_chunk, res = [], {}

        def run_stream(keep):
            for i, (x, n) in enumerate(parts):
                t = timed(lambda: res.__setitem__("stream", stream.decode_chunk(x, n, start=[i == 0] * B)))
                if keep:
                    per_chunk.append(t)

        times = {"whole": [], "stream": []}
        for it in range(a.warmup + a.reps):
            keep = it >= a.warmup
            for name in (("whole", "stream") if it % 2 == 0 else ("stream", "whole")):
                if name == "whole":
                    t = timed(lambda: res.__setitem__("whole", whole.decode(enc)))
                else:
                    count["steps"] = 0
                    t0 = time.perf_counter()
                    run_stream(keep)
                    t = (time.perf_counter() - t0) * 1e3
                if keep:
                    times[name].append(t)
        same = all(torch.equal(x, y) for x, y in zip(res["stream"], res["whole"]))
        r = res["whole"]
        whole_steps = -(-int(r.expansions.max()) // 32) * 32                      # the steps issued: polled every 32
        row = {"B": B, "dtype": str(dtype).split(".")[-1], "lm": use_lm, "calibrated": calibrated, "max_expansions": kw["max_expansions"],
               "expansions_per_frame": float(r.expansions.float().mean()) / T, "emission_rate": float(r.lengths[:, 0].float().mean()) / T,
               "overflow": r.overflow.cpu().tolist(), "stream_equals_whole": same, "chunks": len(parts),
               "whole_ms": spread(times["whole"]), "stream_ms": spread(times["stream"]), "chunk_ms": spread(per_chunk),
               "whole_steps": whole_steps, "stream_steps": count["steps"]}
        row["whole_us_per_step"] = 1e3 * row["whole_ms"]["median"] / whole_steps
        row["stream_us_per_step"] = 1e3 * row["stream_ms"]["median"] / count["steps"]
        if B == 1:
            row["pause"] = pause_cost(TransducerBeamStream(*mods, 1, C, W, U, dtype=dtype, **kw), parts[0], a.reps * 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tbeam_stream_bench: needs the GPU; nothing is measured without one")
    rows = [bench_point(B, dt, lm, a) for lm in (False, True) for B in BATCHES for dt in (torch.float32, torch.bfloat16)]
    fmt = lambda s: f"{s['median']:8.2f} [{s['min']:.2f} .. {s['max']:.2f}]"
    lines = [f"transducer beam search across streaming chunks, T={T} in chunks of {C} ({-(-T // C)} chunks) V={V} H={H} J={J} beam={W} max_symbols={U}; "
             f"median [min .. max] of {a.reps} utterances after {a.warmup} warm-up, whole and streamed alternated in one process; host wall time "
             "around a synchronised call, the stream synchronised after every chunk"]
    for r in rows:
        lines.append(f"  lm={'on ' if r['lm'] else 'off'} B={r['B']} {r['dtype']:8s} whole {fmt(r['whole_ms'])} ms, {r['whole_steps']} steps, {r['whole_us_per_step']:6.1f} us/step   "
                     f"streamed {fmt(r['stream_ms'])} ms, {r['stream_steps']} steps, {r['stream_us_per_step']:6.1f} us/step   per chunk {fmt(r['chunk_ms'])} ms (n={r['chunk_ms']['n']})   "
                     f"streamed/whole {r['stream_ms']['median'] / r['whole_ms']['median']:.3f}   expansions/frame {r['expansions_per_frame']:.2f}   emission rate "
                     f"{r['emission_rate']:.2f}   overflow {r['overflow']}   max_expansions {r['max_expansions']}{'' if r['calibrated'] else ' CAPPED SEARCH'}   "
                     f"streamed == whole {r['stream_equals_whole']}")
    for r in rows:
        if "pause" in r:
            p = r["pause"]
            lines.append(f"  chunk end, lm={'on ' if r['lm'] else 'off'} B=1 {r['dtype']:8s}: selection launch at a pause {fmt(p['pause'])} us, at an ordinary frame end on the same "
                         f"state {fmt(p['frame_end'])} us (n={p['pause']['n']} each, device events): the result write costs {p['extra_us']:+.1f} us")
    lines.append("  not measured: kernel times by trace, the encoder, the host copy of forward_chunk, B > 8, other chunk sizes")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

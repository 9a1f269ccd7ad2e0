"""Milliseconds per step of the seq2seq beam search at the recipes' decoder (num_decoder_layers 6, nhead 1, d_model 512, d_ffn 2048,
normalize_before, GELU; seq_lin 512 -> 5000; encoder output of S = 390 frames), in one process on the same inputs, W hypotheses per
utterance, R = B W rows:

  beam       decoders.seq2seq.beam_search: decode_step over the indexed caches + seq_lin + smx_s2s_beam_select, everything on the device;
  captured   decoders.seq2seq.CapturedS2SBeam: the same step captured once as a graph and replayed;
  select     smx_s2s_beam_select alone (its two launches: the row selection, then the merge / pool / gathers) on fixed logits;
  greedy-R   CapturedS2SGreedy at R rows (the memory replicated W times): the same rows through the greedy step, whose code this
             search leaves as it was - the difference to `captured` is the price of the beam bookkeeping;
  host       what the indexed cache replaces: a host loop of the PLAIN decode_step over R rows + seq_lin + torch.log_softmax +
             torch.topk, the self-attention caches physically reordered by index_select after every step;
  prefix     what exists without any cache: TransformerASR.decode over the R prefixes + seq_lin + torch.topk, every step.

eos is disabled (an index no token has), so every way runs exactly `steps` steps and ends every hypothesis at the cap; the searches
poll every 8 steps as shipped.  Timing: wall clock around a whole search with a device synchronisation before and after; `--rounds`
searches per way, alternated, after one warm-up each (the prefix loop: 2 rounds); the median is reported as ms per step.  The
cross-attention K / V projections of the utterance (make_decode_state) are inside every cached time.  No GPU: the tool fails.

  python tools/s2s_beam_bench.py [--batches 1 8] [--beams 1 10 66] [--steps 64] [--dtypes f32 bf16] [--rounds 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import ops                                                                      # noqa: E402
from summarymixing_amd.decoders import CapturedS2SBeam, CapturedS2SGreedy, beam_search                  # noqa: E402
from summarymixing_amd.lobes.models.transformer.Transformer import DecodeState                        # noqa: E402
from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR                  # noqa: E402
from summarymixing_amd.nnet.linear import Linear                                                      # noqa: E402

LAYERS, D, D_FFN, NHEAD, V, S, BOS = 6, 512, 2048, 1, 5000, 390, 1
NO_EOS = V + 1


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(fns, rounds):
    for fn in fns.values():
        fn()
    got = {k: [] for k in fns}
    for i in range(rounds):
        for k, fn in fns.items():
            if k != "prefix" or i < 2:
                got[k].append(wall(fn))
    return {k: statistics.median(v) for k, v in got.items()}


def bench_point(model, lin, B, W, steps, dtype, rounds, emit):
    name = "bf16" if dtype == torch.bfloat16 else "f32"
    R = B * W
    g = torch.Generator().manual_seed(B)
    mem = torch.randn(B, S, D, generator=g).cuda().to(dtype)
    enc_len = torch.full((B,), S, device="cuda")
    mem_r, len_r = mem.repeat_interleave(W, 0), enc_len.repeat_interleave(W)
    cap = CapturedS2SBeam(model, lin, B, S, steps, dtype, BOS, NO_EOS, W)
    greedy = CapturedS2SGreedy(model, lin, R, S, steps, dtype, BOS, NO_EOS)
    state = model.make_decode_state(mem, enc_len, steps, beam=W)
    plain = model.make_decode_state(mem_r, len_r, steps)
    sel = DecodeState(B, 1, steps, 1, 64, 0, torch.float32, torch.float32, "cuda", beam=W)
    z_fixed = (torch.randn(R, V, generator=g) * 3).cuda().to(dtype)
    base = (torch.arange(B, device="cuda") * W)[:, None]

    def beam():
        return beam_search(model, lin, mem, enc_len, BOS, NO_EOS, 0, steps, W, state=state).tokens

    def captured():
        return cap.search(mem, enc_len).tokens

    def select():
        sel.reset()
        for _ in range(steps):
            ops.s2s_beam_select(z_fixed, sel, NO_EOS, 0, 1.0, True)

    def greedy_r():
        return greedy.search(mem_r, len_r).tokens

    def topk(z, score):
        cs = (score[:, :, None] + torch.log_softmax(z.float(), -1).view(B, W, V)).view(B, W * V)
        top, idx = torch.topk(cs, W, dim=1)
        return top, (idx // V + base).view(-1), (idx % V).to(torch.int32).view(-1)

    def start():
        score = torch.full((B, W), float("-inf"), device="cuda")
        score[:, 0] = 0.0
        return score, torch.full((R,), BOS, dtype=torch.int32, device="cuda")

    @torch.no_grad()
    def host():
        st = model.make_decode_state(mem_r, len_r, steps, state=plain)
        score, tok = start()
        hist = tok[:, None]
        for _ in range(steps):
            score, parent, tok = topk(lin(model.decode_step(tok, st)), score)
            st.self_kv = [kv.index_select(0, parent) for kv in st.self_kv]
            hist = torch.cat([hist.index_select(0, parent), tok[:, None]], 1)
        return hist[:, 1:]

    @torch.no_grad()
    def prefix():
        score, tok = start()
        toks = tok[:, None]
        for _ in range(steps):
            score, parent, tok = topk(lin(model.decode(toks, mem_r, len_r)[0][:, -1]), score)
            toks = torch.cat([toks.index_select(0, parent), tok[:, None]], 1)
        return toks[:, 1:]
    agree = bool(torch.equal(beam().clone(), captured()))
    r = alternate({"beam": beam, "captured": captured, "select": select, "greedy_r": greedy_r, "host": host, "prefix": prefix}, rounds)
    ms = {k: v / steps for k, v in r.items()}
    emit(f"B {B:2d} W {W:2d} rows {R:3d} steps {steps:3d} {name:4s}  ms/step: beam {ms['beam']:6.3f} | captured {ms['captured']:6.3f} | "
         f"select alone {ms['select']:6.3f} | greedy at R rows, captured {ms['greedy_r']:6.3f} | host loop, reordered caches {ms['host']:7.3f} | "
         f"prefix loop {ms['prefix']:8.3f} || captured / greedy-R {ms['captured'] / ms['greedy_r']:5.2f}  host / captured "
         f"{ms['host'] / ms['captured']:5.2f}  prefix / captured {ms['prefix'] / ms['captured']:6.2f}  select / captured "
         f"{ms['select'] / ms['captured']:4.2f}  captured = eager {agree}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--beams", nargs="+", type=int, default=[1, 10, 66])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file (replacing it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("s2s_beam_bench: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tools/s2s_beam_bench.py on {torch.cuda.get_device_name(0)}: beam search, {LAYERS} layers d {D} H {NHEAD} d_ffn {D_FFN} V {V} S {S}, "
         f"eos disabled; ms per step = median of {args.rounds} alternated searches (prefix loop: 2) / steps, wall clock between device "
         "synchronisations")
    torch.manual_seed(0)
    model = TransformerASR(tgt_vocab=V, input_size=80, d_model=D, nhead=NHEAD, num_encoder_layers=1, num_decoder_layers=LAYERS,
                           d_ffn=D_FFN, dropout=0.0, activation=nn.GELU, normalize_before=True, encoder_module="branchformer",
                           attention_type="SummaryMixing", causal=False, csgu_linear_units=64, kernel_size=3, local_proj_hid_dim=[64],
                           local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64).cuda().eval()
    lin = Linear(n_neurons=V, input_size=D).cuda()
    for dt in args.dtypes:
        for B in args.batches:
            for W in args.beams:
                bench_point(model, lin, B, W, args.steps, torch.bfloat16 if dt == "bf16" else torch.float32, args.rounds, emit)
            if args.out:                                       # (after every batch size: a partial file survives a stop)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

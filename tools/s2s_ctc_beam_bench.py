"""Milliseconds per step of the seq2seq beam search with and without the recipes' CTC scorer (joint CTC / attention scoring, DESIGN.md
§I.23) at the recipes' decoder (tools/s2s_beam_bench.py: 6 layers, d_model 512, seq_lin and ctc_lin 512 -> 5000, S = 390 encoder
frames), in one process on the same inputs, W hypotheses per utterance, R = B W rows:

  plain      decoders.seq2seq.CapturedS2SBeam without a scorer: the parent commit's captured step;
  ctc        CapturedS2SBeam(scorer=ScorerBuilder([CTCScorer], {ctc: 0.4})): the same step with smx_ctc_prefix_score in front of the
             selection and smx_ctc_prefix_advance behind it (and, per search, the CTC head's log-probabilities and the empty prefix);
  scorer     the scorer's two launches alone, on a state three real steps into a search (all W slots alive), `steps` times;
  aten       the same scoring as a vectorised host-side scorer would do it: per frame one torch.logaddexp pair over (R, V) tensors,
             then the gather of the winners' states - an ATen chain in this tool, `--aten-steps` steps.

eos is disabled (an index no token has), so every search runs exactly `steps` steps.  Timing: wall clock around a whole search (or
loop) with a device synchronisation before and after; `--rounds` per way, alternated, after one warm-up each; the median is reported
as ms per step.  No GPU: the tool fails.

  python tools/s2s_ctc_beam_bench.py [--batches 1 8] [--beams 1 10 66] [--steps 64] [--dtypes f32 bf16] [--rounds 5] [--out FILE]
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
from summarymixing_amd.decoders import CapturedS2SBeam, CTCScorer, ScorerBuilder                       # noqa: E402
from summarymixing_amd.decoders import scorer as scorer_mod                                            # noqa: E402
from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR                  # noqa: E402
from summarymixing_amd.nnet.linear import Linear                                                      # noqa: E402

LAYERS, D, D_FFN, NHEAD, V, S, BOS, BLANK, WEIGHT = 6, 512, 2048, 1, 5000, 390, 1, 0, 0.4
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
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(wall(fn))
    return {k: statistics.median(v) for k, v in got.items()}


def aten_step(x, utt, rn, rb, psi, last, first, lp, blank, weight):
    """One step of the vectorised host-side scorer: x (B, T, V) log-probabilities, utt (R) the utterance of every hypothesis row
    (the W rows of an utterance share its frames: one (R, V) gather per frame, no (R, T, V) copy), rn / rb (R, T), psi (R), last (R)
    int64 -> (extra (R, V), a function (parent (R), token (R)) -> the winners' (rn, rb, psi))."""
    _, T, Vv = x.shape
    R = utt.numel()
    both = torch.logaddexp(rn, rb)
    rows = torch.arange(R, device=x.device)
    n = x[utt, 0] if first else torch.full((R, Vv), float("-inf"), dtype=x.dtype, device=x.device)
    p1 = n.clone()
    for t in range(1, T):
        xt = x[utt, t]
        phi = both[:, t - 1, None].expand(R, Vv).clone()
        if not first:
            phi[rows, last] = rb[:, t - 1]
        p1 = torch.logaddexp(p1, phi + xt)
        n = torch.logaddexp(n, phi) + xt
    p1[:, blank] = float("-inf")
    extra = weight * (p1 - psi[:, None] - lp)

    def advance(parent, tok):
        xc = x[utt[parent], :, tok]                            # (R, T)
        xb = x[utt[parent], :, blank]
        ph = torch.where((tok == last[parent])[:, None] & (not first), rb[parent], both[parent])
        n2 = torch.full((R, T), float("-inf"), dtype=x.dtype, device=x.device)
        b2 = torch.full((R, T), float("-inf"), dtype=x.dtype, device=x.device)
        if first:
            n2[:, 0] = xc[:, 0]
        for t in range(1, T):
            n2[:, t] = torch.logaddexp(n2[:, t - 1], ph[:, t - 1]) + xc[:, t]
            b2[:, t] = torch.logaddexp(n2[:, t - 1], b2[:, t - 1]) + xb[:, t]
        return n2, b2, p1[parent, tok]
    return extra, advance


def bench_point(model, lin, head, B, W, steps, aten_steps, dtype, rounds, emit):
    name = "bf16" if dtype == torch.bfloat16 else "f32"
    R = B * W
    g = torch.Generator().manual_seed(B)
    mem = torch.randn(B, S, D, generator=g).cuda().to(dtype)
    enc_len = torch.full((B,), S, device="cuda")
    sb = ScorerBuilder(full_scorers=[CTCScorer(eos_index=NO_EOS, blank_index=BLANK, ctc_fc=head)], weights={"ctc": WEIGHT})
    plain = CapturedS2SBeam(model, lin, B, S, steps, dtype, BOS, NO_EOS, W)
    ctc = CapturedS2SBeam(model, lin, B, S, steps, dtype, BOS, NO_EOS, W, scorer=sb)
    z_fixed = (torch.randn(R, V, generator=g) * 3).cuda().to(dtype)

    def run_plain():
        return plain.search(mem, enc_len).tokens

    def run_ctc():
        return ctc.search(mem, enc_len).tokens
    # the scorer's launches alone: three real steps of a search (every slot alive), then score + advance at that step, `steps` times
    st = model.make_decode_state(mem, enc_len, steps, beam=W)
    st.tok.fill_(BOS)
    cs = scorer_mod.begin(sb, st, mem, NO_EOS)
    for _ in range(3):
        ops.s2s_beam_select(z_fixed, st, NO_EOS, 0, 1.0, True, extra=ops.ctc_prefix_score(cs, st, z_fixed, 1.0))
        ops.ctc_prefix_advance(cs, st)

    def run_scorer():
        for _ in range(steps):
            ops.ctc_prefix_score(cs, st, z_fixed, 1.0)
            ops.ctc_prefix_advance(cs, st)
    x, utt = cs.x, torch.arange(R, device="cuda") // W
    lp = torch.log_softmax(z_fixed.float(), -1)
    rn0 = torch.full((R, S), float("-inf"), device="cuda")
    rb0 = torch.cumsum(x[utt, :, BLANK], 1)
    parent = torch.arange(R, device="cuda")
    tok = torch.randint(3, V, (R,), generator=g).cuda()

    @torch.no_grad()
    def run_aten():
        rn, rb, psi, last = rn0, rb0, torch.zeros(R, device="cuda"), tok
        for i in range(aten_steps):
            extra, adv = aten_step(x, utt, rn, rb, psi, last, i == 0, lp, BLANK, WEIGHT)
            rn, rb, psi = adv(parent, tok)
            last = tok
        return extra
    agree = bool(torch.equal(run_ctc().clone(), run_ctc()))
    r = alternate({"plain": run_plain, "ctc": run_ctc, "scorer": run_scorer}, rounds)
    ms = {k: v / steps for k, v in r.items()}
    ms["aten"] = alternate({"aten": run_aten}, max(2, rounds // 2))["aten"] / aten_steps
    emit(f"B {B:2d} W {W:2d} rows {R:3d} steps {steps:3d} {name:4s}  ms/step: captured plain {ms['plain']:6.3f} | captured with the CTC scorer "
         f"{ms['ctc']:6.3f} | scorer launches alone {ms['scorer']:6.3f} | ATen chain, same scoring {ms['aten']:8.3f} || with / without "
         f"{ms['ctc'] / ms['plain']:5.2f}  scorer / captured-with {ms['scorer'] / ms['ctc']:4.2f}  ATen / scorer {ms['aten'] / ms['scorer']:7.1f}  "
         f"two runs agree {agree}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--beams", nargs="+", type=int, default=[1, 10, 66])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--aten-steps", type=int, default=2)
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file (replacing it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("s2s_ctc_beam_bench: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tools/s2s_ctc_beam_bench.py on {torch.cuda.get_device_name(0)}: beam search with / without the CTC scorer (weight {WEIGHT}), "
         f"{LAYERS} layers d {D} H {NHEAD} d_ffn {D_FFN} V {V} S {S}, eos disabled; ms per step = median of {args.rounds} alternated "
         f"searches / steps (ATen chain: {args.aten_steps} steps), wall clock between device synchronisations")
    torch.manual_seed(0)
    model = TransformerASR(tgt_vocab=V, input_size=80, d_model=D, nhead=NHEAD, num_encoder_layers=1, num_decoder_layers=LAYERS,
                           d_ffn=D_FFN, dropout=0.0, activation=nn.GELU, normalize_before=True, encoder_module="branchformer",
                           attention_type="SummaryMixing", causal=False, csgu_linear_units=64, kernel_size=3, local_proj_hid_dim=[64],
                           local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64).cuda().eval()
    lin = Linear(n_neurons=V, input_size=D).cuda()
    head = Linear(n_neurons=V, input_size=D).cuda()
    with torch.no_grad():
        head.w.bias[BLANK] += 8.0                              # blank dominates, as in a trained head
    for dt in args.dtypes:
        for B in args.batches:
            for W in args.beams:
                bench_point(model, lin, head, B, W, args.steps, args.aten_steps, torch.bfloat16 if dt == "bf16" else torch.float32,
                            args.rounds, emit)
            if args.out:                                       # (after every batch size: a partial file survives a stop)
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Milliseconds per step of the seq2seq beam search with the recipes' TransformerLM scorer at the recipe's decoder
(tools/s2s_ctc_beam_bench.py: 6 layers, d_model 512, seq_lin and ctc_lin 512 -> 5000, S = 390 encoder frames) and the recipe's LM
(12 encoder layers, d_model 768, 12 heads, d_ffn 3072, GELU, V 5000), W hypotheses per utterance, R = B W rows, per grid point in one
process on the same inputs:

  joint      decoders.seq2seq.CapturedS2SBeam(scorer=ScorerBuilder([TransformerLMScorer(T 1.15), CTCScorer], {ctc 0.4, transformerlm
             0.6})): the captured step with the CTC scorer's two launches, the LM's cached step and smx_lm_score;
  ctc        CapturedS2SBeam with the CTC scorer alone;  plain: without a scorer;
  lm         the LM's launches alone - TransformerLM.step over the R rows through an ancestor table, then smx_lm_score - captured as
             a graph of their own and replayed `steps` times from position 0 (so the caches fill as in a search);
  prefix     upstream-style scoring of the same number of hypotheses: the WHOLE prefix of n tokens through a torch.nn.TransformerEncoder
             chain restating the LM (embedding, causal mask, final norm, the three-stage head), the token memory reordered with
             index_select first, log_softmax(logits / T)[:, -1] - one call, at n = 8, 32 and 64;
  weights    the bytes of the LM's weights a step reads (every Linear once, in the compute dtype) over the lm time, as a fraction of the
             HBM peak of 8 TB/s.

eos is disabled (an index no token has), so every search runs exactly `steps` steps.  Timing: wall clock around a whole search (or
loop) with a device synchronisation before and after; `--rounds` per way, alternated, after one warm-up each; the median is reported
as ms per step.  The driver (this file without --point) touches no GPU: it runs every grid point as a child process of its own under
a time limit of its own and stops at the first one that fails or runs out of time; the lines go to --out.

  python tools/s2s_lm_beam_bench.py [--batches 1 8] [--beams 10 66] [--steps 64] [--dtypes f32 bf16] [--rounds 5] [--point-timeout 240]
                                    [--out profiles/s2s_lm_beam_bench.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS, D, D_FFN, NHEAD, V, S, BOS, BLANK = 6, 512, 2048, 1, 5000, 390, 1, 0
LM_LAYERS, LM_D, LM_H, LM_FFN = 12, 768, 12, 3072
W_CTC, W_LM, T_LM = 0.4, 0.6, 1.15
NO_EOS = V + 1
PREFIX_AT = (8, 32, 64)
HBM_PEAK = 8.0e12


def wall(fn):
    import torch
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


def prefix_chain(lm, dtype):
    """The LM restated on torch.nn.TransformerEncoder (its own weights; the timing does not depend on them) -> fn(tokens (R, n)) ->
    log_softmax(logits / T)[:, -1]."""
    import torch
    from torch import nn
    layer = nn.TransformerEncoderLayer(LM_D, LM_H, LM_FFN, dropout=0.0, activation="gelu", layer_norm_eps=1e-6, batch_first=True, norm_first=False)
    enc = nn.TransformerEncoder(layer, LM_LAYERS, norm=nn.LayerNorm(LM_D, eps=1e-6), enable_nested_tensor=False).cuda().to(dtype).eval()
    head = nn.Sequential(nn.Linear(LM_D, LM_D), nn.LayerNorm(LM_D, eps=1e-6), nn.Linear(LM_D, V)).cuda().to(dtype).eval()
    table = lm.custom_src_module.emb.Embedding.weight.detach()
    pe = lm.positional_encoding.pe[0].detach()

    @torch.no_grad()
    def fn(memory, parents):
        tokens = torch.index_select(memory, 0, parents)       # the token memory follows the beams
        n = tokens.shape[1]
        x = (table[tokens] * LM_D ** 0.5 + pe[:n]).to(dtype)
        mask = torch.triu(torch.full((n, n), float("-inf"), device=x.device, dtype=dtype), diagonal=1)
        return torch.log_softmax(head(enc(x, mask=mask)).float() / T_LM, -1)[:, -1]
    return fn


def bench_point(B, W, steps, dt, rounds):
    import torch
    from torch import nn
    from summarymixing_amd import ops
    from summarymixing_amd.decoders import CapturedS2SBeam, CTCScorer, ScorerBuilder, TransformerLMScorer
    from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from summarymixing_amd.lobes.models.transformer.TransformerLM import TransformerLM
    from summarymixing_amd.nnet.linear import Linear
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    torch.manual_seed(0)
    model = TransformerASR(tgt_vocab=V, input_size=80, d_model=D, nhead=NHEAD, num_encoder_layers=1, num_decoder_layers=LAYERS,
                           d_ffn=D_FFN, dropout=0.0, activation=nn.GELU, normalize_before=True, encoder_module="branchformer",
                           attention_type="SummaryMixing", causal=False, csgu_linear_units=64, kernel_size=3, local_proj_hid_dim=[64],
                           local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64).cuda().eval()
    lin = Linear(n_neurons=V, input_size=D).cuda()
    head = Linear(n_neurons=V, input_size=D).cuda()
    with torch.no_grad():
        head.w.bias[BLANK] += 8.0                              # blank dominates, as in a trained head
    lm = TransformerLM(V, d_model=LM_D, nhead=LM_H, num_encoder_layers=LM_LAYERS, num_decoder_layers=0, d_ffn=LM_FFN, dropout=0.0,
                       activation=nn.GELU, normalize_before=False).cuda().eval()
    R = B * W
    g = torch.Generator().manual_seed(B)
    mem = torch.randn(B, S, D, generator=g).cuda().to(dtype)
    enc_len = torch.full((B,), S, device="cuda")
    ctc_scorer = CTCScorer(eos_index=NO_EOS, blank_index=BLANK, ctc_fc=head)
    lm_scorer = TransformerLMScorer(language_model=lm, temperature=T_LM)
    caps = {"plain": CapturedS2SBeam(model, lin, B, S, steps, dtype, BOS, NO_EOS, W),
            "ctc": CapturedS2SBeam(model, lin, B, S, steps, dtype, BOS, NO_EOS, W,
                                   scorer=ScorerBuilder(full_scorers=[ctc_scorer], weights={"ctc": W_CTC})),
            "joint": CapturedS2SBeam(model, lin, B, S, steps, dtype, BOS, NO_EOS, W,
                                     scorer=ScorerBuilder(full_scorers=[lm_scorer, ctc_scorer], weights={"ctc": W_CTC, "transformerlm": W_LM}))}
    fns = {k: (lambda c=c: c.search(mem, enc_len).tokens) for k, c in caps.items()}
    # the LM's launches alone, as a graph of their own: every slot alive, every key read through the table (each row its own ancestor)
    with torch.no_grad():
        st = model.make_decode_state(mem, enc_len, steps, beam=W)
        st.score.zero_()
        st.anc.copy_(torch.arange(R, dtype=torch.int32, device="cuda")[:, None].expand(R, steps))
        ls = lm.make_state(R, steps, dtype, "cuda")
        extra = torch.empty((R, V), dtype=torch.float32, device="cuda")
        tok = torch.randint(3, V, (R,), generator=g).to(torch.int32).cuda()

        def lm_launches():
            ops.lm_score(lm.step(tok, ls, anc=st.anc), extra, st, W_LM, 1.0 / T_LM)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lm_launches()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            lm_launches()

    def run_lm():
        ls.reset()
        for _ in range(steps):
            graph.replay()
    fns["lm"] = run_lm
    agree = bool(torch.equal(fns["joint"]().clone(), fns["joint"]()))
    r = alternate(fns, rounds)
    ms = {k: v / steps for k, v in r.items()}
    chain = prefix_chain(lm, dtype)
    parents = torch.randint(0, R, (R,), generator=g).cuda()
    pre = {}
    for n in PREFIX_AT:
        memory = torch.randint(3, V, (R, n), generator=g).cuda()
        pre[n] = alternate({"p": lambda: chain(memory, parents)}, max(3, rounds))["p"]
    es = 2 if dtype == torch.bfloat16 else 4
    wbytes = es * (LM_LAYERS * (4 * LM_D * LM_D + 2 * LM_D * LM_FFN) + LM_D * LM_D + LM_D * V)
    frac = wbytes / (ms["lm"] * 1e-3) / HBM_PEAK
    slower = [n for n in PREFIX_AT if ms["lm"] > pre[n]]
    print(f"B {B:2d} W {W:2d} rows {R:3d} steps {steps:3d} {dt:4s}  ms/step: captured CTC + LM {ms['joint']:6.3f} | CTC only {ms['ctc']:6.3f} | plain "
          f"{ms['plain']:6.3f} | LM launches alone {ms['lm']:6.3f} | whole-prefix torch chain at n = " +
          ", ".join(f"{n}: {pre[n]:7.3f}" for n in PREFIX_AT) + f" || joint / ctc {ms['joint'] / ms['ctc']:5.2f}  joint / plain "
          f"{ms['joint'] / ms['plain']:5.2f}  prefix(64) / LM step {pre[64] / ms['lm']:6.1f}  LM weights {wbytes / 1e6:6.1f} MB / LM step = "
          f"{frac:5.3f} of the HBM peak  cached step slower than the prefix re-run at n = {slower if slower else 'none'}  two runs agree {agree}",
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 8])
    ap.add_argument("--beams", nargs="+", type=int, default=[10, 66])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--point-timeout", type=int, default=240, help="seconds one grid point (a process of its own) may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2s_lm_beam_bench.txt"), help="write the lines to this file (replacing it)")
    ap.add_argument("--point", nargs=3, metavar=("B", "W", "DTYPE"), default=None, help="run one grid point in this process (the driver's child)")
    args = ap.parse_args()
    if args.point:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("s2s_lm_beam_bench: needs a GPU (nothing is measured without one)")
        if args.point[2] == "name":
            print(torch.cuda.get_device_name(0))
            return
        bench_point(int(args.point[0]), int(args.point[1]), args.steps, args.point[2], args.rounds)
        return
    lines = []

    def child(point, limit):
        """One GPU step: a fresh process under its own time limit -> its last line, or None (the driver then stops)."""
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--rounds", str(args.rounds), "--point", *map(str, point)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"s2s_lm_beam_bench: point {point} ran out of its {limit} s: stopping", flush=True)
            return None
        if p.returncode != 0:
            print(f"s2s_lm_beam_bench: point {point} failed with status {p.returncode}: stopping\n{p.stderr[-2000:]}", flush=True)
            return None
        return p.stdout.strip().splitlines()[-1]
    name = child((0, 0, "name"), 120)
    if name is None:
        raise SystemExit(1)
    lines.append(f"# tools/s2s_lm_beam_bench.py on {name}: beam search with the TransformerLM scorer (T {T_LM}, weight {W_LM}) and the CTC scorer "
                 f"(weight {W_CTC}); decoder {LAYERS} layers d {D} H {NHEAD} d_ffn {D_FFN}, LM {LM_LAYERS} layers d {LM_D} H {LM_H} d_ffn {LM_FFN}, "
                 f"V {V} S {S}, eos disabled; ms per step = median of {args.rounds} alternated searches / steps (whole-prefix chain: ms per "
                 "call), wall clock between device synchronisations; one process per line")
    print(lines[0], flush=True)
    ok = True
    for dt in args.dtypes:
        for B in args.batches:
            for W in args.beams:
                line = child((B, W, dt), args.point_timeout) if ok else None
                if line is None:
                    ok = False
                    break
                print(line, flush=True)
                lines.append(line)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:                    # (after every batch size: a partial file survives a stop)
                f.write("\n".join(lines) + "\n")
            if not ok:
                raise SystemExit(1)


if __name__ == "__main__":
    main()

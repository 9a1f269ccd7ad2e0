"""Forward + backward cost of the seq2seq decoder side of TransformerASR.forward - from the tokens and a fixed encoder output to
decoder_out and back to the embedding table, the decoder parameters and the encoder output - at the recipes' decoder
(num_decoder_layers 6, nhead 1, d_model 512, d_ffn 2048, normalize_before, GELU; CommonVoice / AISHELL-1 Branchformer-SummaryMixing).

Beside it, in the same process and on the same inputs, a torch.nn chain that restates upstream's decoder, written for this tool:
nn.Embedding * sqrt(d) + the sine table, tokens.eq(pad), per layer LayerNorm(eps 1e-6) -> nn.MultiheadAttention (causal float mask +
key padding, need_weights=True as speechbrain's wrapper always asks) -> dropout + residual, LayerNorm -> nn.MultiheadAttention over
the memory -> dropout + residual, LayerNorm -> Linear, GELU, Dropout, Linear -> dropout + residual; a final LayerNorm.  bf16: ours
computes in bf16 on a float32 residual stream; the torch chain runs under torch.autocast(bfloat16), the recipes' `precision: bf16`.

Timing: device events around `--steps` forward + backward steps after `--warmup` warm-up steps of the same shape; the two sides
alternate, `--rounds` times; the median and the spread of the rounds are reported (ms per step).  The embedding launch pair alone
(smx_tgt_embed_fwd + _bwd) is timed against its ATen chain the same way.  No GPU: the tool fails.

  python tools/decoder_bench.py [--shapes 64,80,125,512,6,5000 32,64,390,512,6,1000] [--dtypes f32 bf16] [--dropout 0.1]
                                [--steps 20] [--warmup 5] [--rounds 3] [--out profiles/decoder_bench.txt]
"""
import argparse
import math
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from summarymixing_amd import ops                                                                   # noqa: E402
from summarymixing_amd.lobes.models.transformer.TransformerASR import PositionalEncoding, TransformerASR  # noqa: E402

D_FFN, NHEAD, PAD = 2048, 1, 0


class TorchDecoderLayer(nn.Module):
    def __init__(self, d, f, p):
        super().__init__()
        self.sa = nn.MultiheadAttention(d, NHEAD, dropout=p, batch_first=True)
        self.ca = nn.MultiheadAttention(d, NHEAD, dropout=p, batch_first=True)
        self.n1, self.n2, self.n3 = (nn.LayerNorm(d, eps=1e-6) for _ in range(3))
        self.ffn = nn.Sequential(nn.Linear(d, f), nn.GELU(), nn.Dropout(p), nn.Linear(f, d))
        self.d1, self.d2, self.d3 = (nn.Dropout(p) for _ in range(3))

    def forward(self, x, mem, look, tpad, mpad):
        h = self.n1(x)
        x = x + self.d1(self.sa(h, h, h, attn_mask=look, key_padding_mask=tpad, need_weights=True)[0])
        h = self.n2(x)
        x = x + self.d2(self.ca(h, mem, mem, key_padding_mask=mpad, need_weights=True)[0])
        return x + self.d3(self.ffn(self.n3(x)))


class TorchDecoderSide(nn.Module):
    def __init__(self, V, d, f, layers, p, max_len):
        super().__init__()
        self.emb = nn.Embedding(V, d, padding_idx=PAD)
        self.layers = nn.ModuleList([TorchDecoderLayer(d, f, p) for _ in range(layers)])
        self.norm = nn.LayerNorm(d, eps=1e-6)
        self.register_buffer("pe", PositionalEncoding(d, max_len).pe[0].clone())
        self.scale = math.sqrt(d)

    def forward(self, tgt, mem, mpad):
        U = tgt.shape[1]
        tpad = tgt.eq(PAD)
        look = torch.triu(torch.full((U, U), float("-inf"), device=tgt.device), diagonal=1)
        x = self.emb(tgt) * self.scale + self.pe[:U]
        tpad = torch.zeros_like(x[:, :, 0]).masked_fill_(tpad, float("-inf"))           # (float, like the look-ahead mask)
        for layer in self.layers:
            x = layer(x, mem, look, tpad, mpad)
        return self.norm(x)


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(fns, steps, warmup, rounds):
    """fns: {name: callable}; -> {name: (median ms, min ms, max ms)} over `rounds` alternating windows."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(timed(fn, steps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def inputs(B, U, S, d, V, dtype):
    g = torch.Generator().manual_seed(1)
    tgt = torch.randint(1, V, (B, U), generator=g)
    lens = torch.randint(U // 2, U + 1, (B,), generator=g)
    lens[0] = U
    tgt[torch.arange(U)[None, :] >= lens[:, None]] = PAD
    slen = torch.randint(S // 2, S + 1, (B,), generator=g)
    slen[0] = S
    mpad = torch.arange(S)[None, :] >= slen[:, None]
    mem = torch.randn(B, S, d, generator=g)
    r = torch.randn(B, U, d, generator=g) / 100
    return tgt.cuda(), mem.cuda().to(dtype).requires_grad_(True), mpad.cuda(), r.cuda()


def bench_shape(shape, dtype, args, emit):
    B, U, S, d, layers, V = shape
    name = "bf16" if dtype == torch.bfloat16 else "f32"
    tgt, mem, mpad, r = inputs(B, U, S, d, V, dtype)
    torch.manual_seed(0)
    ours = TransformerASR(tgt_vocab=V, input_size=80, d_model=d, nhead=NHEAD, num_encoder_layers=1, num_decoder_layers=layers,
                          d_ffn=D_FFN, dropout=args.dropout, activation=nn.GELU, normalize_before=True, encoder_module="branchformer",
                          attention_type="SummaryMixing", causal=False, csgu_linear_units=64, kernel_size=3, local_proj_hid_dim=[64],
                          local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64, max_length=max(2500, U)).cuda().train()
    ref = TorchDecoderSide(V, d, D_FFN, layers, args.dropout, max(2500, U)).cuda().train()
    tgt32 = tgt.to(torch.int32)

    def step_ours():
        ours._decoder_side(tgt32, mem, mpad, PAD).backward(r.to(dtype))

    def step_torch():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            out = ref(tgt, mem, mpad)
        out.backward(r.to(out.dtype))
    res = alternate({"ours": step_ours, "torch": step_torch}, args.steps, args.warmup, args.rounds)
    o, t = res["ours"], res["torch"]
    emit(f"decoder fwd+bwd  (B,U,S,d,layers,V)={shape} {name} dropout {args.dropout}: ours {o[0]:.3f} ms [{o[1]:.3f}, {o[2]:.3f}]   "
         f"torch.nn chain {t[0]:.3f} ms [{t[1]:.3f}, {t[2]:.3f}]   torch / ours {t[0] / o[0]:.2f}")
    # the embedding launch pair alone against its ATen chain
    table = ours.custom_tgt_module.layers[0].emb.Embedding.weight
    pe = ours.positional_encoding.pe[0, :U]
    out_dtype = torch.float32                                         # (the residual stream both sides open)
    dy = torch.randn(B * U, d, device="cuda")
    gt = torch.zeros_like(table)
    emb = ref.emb
    scale = math.sqrt(d)

    def emb_ours():
        ops.tgt_embed_fwd(tgt32, table.detach(), pe, PAD, out_dtype)
        ops.tgt_embed_bwd(tgt32, dy, gt, PAD)

    def emb_aten():
        y = emb(tgt) * scale + pe
        tgt.eq(PAD)
        y.backward(dy.view(B, U, d))
    res = alternate({"ours": emb_ours, "aten": emb_aten}, args.steps * 5, args.warmup, args.rounds)
    o, t = res["ours"], res["aten"]
    emit(f"embedding fwd+bwd (B,U,d,V)=({B}, {U}, {d}, {V}) float32 out: ours (2 launches) {1e3 * o[0]:.1f} us [{1e3 * o[1]:.1f}, "
         f"{1e3 * o[2]:.1f}]   ATen chain {1e3 * t[0]:.1f} us [{1e3 * t[1]:.1f}, {1e3 * t[2]:.1f}]   aten / ours {t[0] / o[0]:.2f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["64,80,125,512,6,5000", "32,64,390,512,6,1000"], help="B,U,S,d,layers,V")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decoder_bench: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit(f"# tools/decoder_bench.py on {torch.cuda.get_device_name(0)}: ms per forward + backward step, median [min, max] of {args.rounds} "
         f"alternating windows of {args.steps} steps after {args.warmup} warm-up steps")
    for s in args.shapes:
        shape = tuple(int(v) for v in s.split(","))
        for dt in args.dtypes:
            bench_shape(shape, torch.bfloat16 if dt == "bf16" else torch.float32, args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

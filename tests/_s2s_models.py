"""The small seq2seq models of the KV-cached decoding tests (tests/test_decode_step_gpu.py, tests/test_s2s_search_gpu.py), built as
tests/test_decoder_gpu.py builds its own - random non-trivial biases and LayerNorm parameters, everything rounded to the dtype - plus a
`seq_lin` head, and their float64 / ATen restatements through tests/_decoder_ref.py."""
import math

import torch
from torch import nn

from tests import _decoder_ref as DR

V, B, S = 40, 3, 70
ENC_LEN = (70, 35, 65)
# name -> (d, H, d_ffn, layers, normalize_before, forced tokens / search steps)
MODELS = {"d64-pre": (64, 1, 128, 2, True, 66), "d128-h2-post": (128, 2, 128, 2, False, 66), "d512-pre": (512, 1, 256, 1, True, 20)}
TABLE = "custom_tgt_module.layers.0.emb.Embedding.weight"


def randomise(module, dtype, seed):
    """Non-trivial biases and LayerNorm parameters (the constructors leave them at 0 / 1); everything rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if name.endswith("norm.weight") else 0.0))
            p.copy_(p.to(dtype).float())
    return module


def build(name, dtype, seed):
    """-> (TransformerASR in eval mode on the GPU, seq_lin, memory (B, S, d) in dtype on the GPU, enc_len (B) on the GPU)."""
    from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from summarymixing_amd.nnet.linear import Linear
    d, H, f, layers, pre, _ = MODELS[name]
    torch.manual_seed(seed)
    m = TransformerASR(tgt_vocab=V, input_size=20, d_model=d, nhead=H, num_encoder_layers=1, num_decoder_layers=layers, d_ffn=f,
                       dropout=0.0, activation=nn.GELU, encoder_module="branchformer", normalize_before=pre, causal=False,
                       csgu_linear_units=64, kernel_size=3, local_proj_hid_dim=[64], local_proj_out_dim=64, summary_hid_dim=[64],
                       summary_out_dim=64)
    for part in (m.decoder, m.custom_tgt_module):
        randomise(part, dtype, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    lin = Linear(n_neurons=V, input_size=d)
    with torch.no_grad():
        lin.w.weight.copy_((torch.randn(V, d, generator=g) * 4 / math.sqrt(d)).to(dtype).float())
        lin.w.bias.copy_((torch.randn(V, generator=g) * 0.1).to(dtype).float())
    mem = torch.randn(B, S, d, generator=g).to(dtype)
    return m.cuda().eval(), lin.cuda(), mem.cuda(), torch.tensor(ENC_LEN).cuda()


def restated(name, m, lin, mem, impl, dtype):
    """fn(tokens (B, U) on the CPU) -> (prediction (B, U, d), logits (B, U, V)) of the whole prefix under the look-ahead mask, in
    float64 on the CPU (impl="f64") or as the ATen chain at `dtype` on the GPU (impl="aten": the table and the embedding sum stay
    float32, as in tests/test_decoder_gpu.py)."""
    d, H, f, layers, pre, _ = MODELS[name]
    dev, dt = ("cpu", torch.float64) if impl == "f64" else ("cuda", dtype)
    sd = {k: v.detach() for k, v in m.state_dict().items() if k.startswith("decoder.") or k == TABLE}
    P = {k: v.to(device=dev, dtype=torch.float64 if impl == "f64" else (torch.float32 if k == TABLE else dtype)) for k, v in sd.items()}
    pe = m.positional_encoding.pe[0].detach().to(device=dev, dtype=P[TABLE].dtype)
    W, b = lin.w.weight.detach().to(device=dev, dtype=dt), lin.w.bias.detach().to(device=dev, dtype=dt)
    memx = mem.to(device=dev, dtype=dt)
    mpad = (torch.arange(S)[None, :] >= torch.tensor(ENC_LEN)[:, None]).to(dev)

    def fn(tokens):
        with torch.no_grad():
            x = DR.embed(tokens.to(dev), P[TABLE], pe).to(dt)
            out = DR.decoder(x, memx, P, "decoder.", layers, H, "gelu", pre, impl=impl, causal=True, mem_pad=mpad)[0]
            return out, torch.nn.functional.linear(out, W, b)
    return fn

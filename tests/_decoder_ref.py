"""Restatement of the seq2seq decoder, written from the formulas of speechbrain's Transformer.py (NormalizedEmbedding + positional
rows, get_key_padding_mask, get_lookahead_mask, TransformerDecoderLayer in both normalize_before orders, TransformerDecoder), in two
arithmetic flavours over ONE parameter dict with the package's state_dict keys:

  impl="f64":  float64 on the CPU, attention through tests/_attention_ref.mha - the yardstick;
  impl="aten": the ATen chain at the tensors' own dtype and device - F.embedding, F.multi_head_attention_forward (its baddbmm / softmax
               / bmm path, need_weights=True), F.layer_norm, F.linear - whose error against float64 is the bar the package is held to.

Gradients come from torch autograd.  Dropout is not restated (the parity checks run with p = 0)."""
import math

import torch
import torch.nn.functional as TF

from tests import _attention_ref as R
from tests._util import rel_err, report

NEG = float("-inf")


def lookahead_mask(U, dtype=torch.float64, device="cpu"):
    """0 on and below the diagonal, -inf above it."""
    return torch.triu(torch.full((U, U), NEG, dtype=dtype, device=device), diagonal=1)


def key_padding_mask(tokens, pad_idx):
    return tokens == pad_idx


def embed(tokens, table, pe, impl="f64"):
    """table[tokens] * sqrt(d) + pe[u]; a token outside [0, V) reads as a zero row (the library's stated convention)."""
    V, d = table.shape
    U = tokens.shape[1]
    ok = (tokens >= 0) & (tokens < V)
    e = TF.embedding(tokens.clamp(0, V - 1), table) * ok[..., None].to(table.dtype)
    return e * math.sqrt(d) + pe[:U].to(table.dtype)


def _aten_mha(q, k, v, in_w, in_b, out_w, out_b, nhead, attn_bias, key_pad, causal):
    Lq, S, d = q.shape[1], k.shape[1], q.shape[2]
    m = None if attn_bias is None else attn_bias.to(q.dtype)
    if causal:
        cm = torch.triu(torch.full((Lq, S), NEG, dtype=q.dtype, device=q.device), diagonal=1 + S - Lq)
        m = cm if m is None else m + cm
    out, w = TF.multi_head_attention_forward(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1), d, nhead, in_w, in_b, None, None,
                                             False, 0.0, out_w, out_b, training=False, key_padding_mask=key_pad, need_weights=True,
                                             attn_mask=m)
    return out.transpose(0, 1), w


def _mha(impl, *a):
    if impl == "aten":
        return _aten_mha(*a)
    q, k, v, in_w, in_b, out_w, out_b, nhead, attn_bias, key_pad, causal = a
    return R.mha(q, k, v, in_w, in_b, out_w, out_b, nhead, attn_bias, key_pad, causal)


def _act(name, x):
    return {"gelu": TF.gelu, "relu": TF.relu}[name](x)


def decoder_layer(x, mem, P, pfx, nhead, act, pre, causal=True, tgt_bias=None, tgt_pad=None, mem_bias=None, mem_pad=None, impl="f64"):
    """One TransformerDecoderLayer (eps 1e-6).  P[pfx + key]: the parameters.  -> (out, self weights, cross weights)."""
    d = x.shape[-1]

    def ln(t, n):
        return TF.layer_norm(t, (d,), P[f"{pfx}{n}.norm.weight"], P[f"{pfx}{n}.norm.bias"], 1e-6)

    def att(name, q, kv, bias, pad, causal_):
        a = f"{pfx}{name}.att."
        return _mha(impl, q, kv, kv, P[a + "in_proj_weight"], P[a + "in_proj_bias"], P[a + "out_proj.weight"], P[a + "out_proj.bias"],
                    nhead, bias, pad, causal_)

    def ffn(t):
        h = _act(act, TF.linear(t, P[pfx + "pos_ffn.ffn.0.weight"], P[pfx + "pos_ffn.ffn.0.bias"]))
        return TF.linear(h, P[pfx + "pos_ffn.ffn.3.weight"], P[pfx + "pos_ffn.ffn.3.bias"])
    t1 = ln(x, "norm1") if pre else x
    t2, sa = att("self_attn", t1, t1, tgt_bias, tgt_pad, causal)
    x = x + t2
    if not pre:
        x = ln(x, "norm1")
    t1 = ln(x, "norm2") if pre else x
    t2, ca = att("multihead_attn", t1, mem, mem_bias, mem_pad, False)
    x = x + t2
    if not pre:
        x = ln(x, "norm2")
    t1 = ln(x, "norm3") if pre else x
    x = x + ffn(t1)
    if not pre:
        x = ln(x, "norm3")
    return x, sa, ca


def decoder(x, mem, P, pfx, n_layers, nhead, act, pre, impl="f64", **masks):
    """The layers P[pfx + "layers.i."] and the final LayerNorm P[pfx + "norm.norm."] -> (out, [self weights], [cross weights])."""
    sas, cas = [], []
    for i in range(n_layers):
        x, sa, ca = decoder_layer(x, mem, P, f"{pfx}layers.{i}.", nhead, act, pre, impl=impl, **masks)
        sas.append(sa)
        cas.append(ca)
    d = x.shape[-1]
    return TF.layer_norm(x, (d,), P[pfx + "norm.norm.weight"], P[pfx + "norm.norm.bias"], 1e-6), sas, cas


def judge(name, dtype, ours, aten, ref):
    """The project's bar (tests/test_attention_gpu.py): per key, rel_err(ours) <= 4 x rel_err(aten) against float64, with a floor of
    8 eps(dtype) where ATen's error is 0.  Prints and records every pair, then asserts all of them."""
    eps = torch.finfo(dtype).eps
    pairs = {}
    for k, r in ref.items():
        assert torch.isfinite(ours[k].float()).all(), f"{name}: non-finite values in {k}"
        eo, ea = rel_err(ours[k], r), rel_err(aten[k], r)
        pairs[k] = (eo, ea, 4.0 * ea if ea > 0.0 else 8.0 * eps)
    print(name, {k: f"{o:.2e} / {a:.2e}" for k, (o, a, _) in pairs.items()})
    report(name, {"errors": {k: {"ours": o, "aten": a, "bar": b} for k, (o, a, b) in pairs.items()}})
    bad = {k: v for k, v in pairs.items() if not v[0] <= v[2]}
    assert not bad, f"{name}: ours > 4 x ATen (8 eps where ATen is exact) (ours, aten, bar): {bad}"

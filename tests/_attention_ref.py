"""float64 restatement of multi-head scaled-dot-product attention, written from the definition in include/smx.h (smx_attn_*):
projections, scores, the three masks, softmax, an explicit dropout keep mask, P V, the out-projection and the head-averaged
weights.  Gradients come from torch autograd in float64.  A row whose keys are all masked yields zeros (the library's stated
deviation from torch's NaN) and lse = -inf."""
import math

import torch


def masked_scores(q, k, scale, attn_bias=None, key_pad=None, causal=False):
    """q (B, L, H, D), k (B, S, H, D) -> s (B, H, L, S), -inf where masked.  attn_bias (L, S) additive; key_pad bool (B, S), True =
    masked; causal: key j visible to query i iff j <= i + (S - L)."""
    L, S = q.shape[1], k.shape[1]
    s = torch.einsum("blhd,bshd->bhls", q, k) * scale
    if attn_bias is not None:
        s = s + attn_bias.to(s.dtype)
    dead = torch.zeros((q.shape[0], 1, L, S), dtype=torch.bool, device=q.device)
    if causal:
        i = torch.arange(L, device=q.device)[:, None]
        j = torch.arange(S, device=q.device)[None, :]
        dead = dead | (j > i + (S - L))
    if key_pad is not None:
        dead = dead | key_pad[:, None, None, :].bool()
    return s.masked_fill(dead, float("-inf"))


def softmax_rows(s):
    """-> (p, lse): softmax over the last axis with the row maximum subtracted; an all -inf row gives p = 0, lse = -inf."""
    m = s.amax(dim=-1, keepdim=True)
    none = torch.isinf(m) & (m < 0)
    m0 = torch.where(none, torch.zeros_like(m), m).detach()
    e = torch.exp(s - m0)
    l = e.sum(dim=-1, keepdim=True)
    p = e / torch.where(l == 0, torch.ones_like(l), l)
    with torch.no_grad():
        lse = torch.where(none, torch.full_like(m, float("-inf")), m0 + torch.log(torch.where(l == 0, torch.ones_like(l), l)))
    return p, lse.squeeze(-1)


def attention(q, k, v, scale=None, attn_bias=None, key_pad=None, causal=False, keep=None, drop_p=0.0):
    """-> (o (B, L, H, D), lse (B, H, L), p~ (B, H, L, S)).  keep: the explicit dropout keep mask, anything that reshapes to
    (B, H, L, S) with non-zero = kept (ops.dropout on ones of shape (B H L, S)), or None."""
    B, L, H, D = q.shape
    S = k.shape[1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    p, lse = softmax_rows(masked_scores(q, k, scale, attn_bias, key_pad, causal))
    if keep is not None:
        p = p * (keep.reshape(B, H, L, S) != 0).to(p.dtype) / (1.0 - drop_p)
    return torch.einsum("bhls,bshd->blhd", p, v), lse, p


def mha(query, key, value, in_w, in_b, out_w, out_b, nhead, attn_bias=None, key_pad=None, causal=False, keep=None, drop_p=0.0):
    """Batch-first multi-head attention with torch's parameter layout: in_w (3d, d) = [Wq; Wk; Wv], in_b (3d) or None, out_w (d, d),
    out_b (d) or None -> (out (B, L, d), weights (B, L, S) = mean over heads of p~)."""
    B, L, d = query.shape
    S, D = key.shape[1], d // nhead
    bq, bk, bv = (in_b[:d], in_b[d:2 * d], in_b[2 * d:]) if in_b is not None else (None, None, None)
    lin = torch.nn.functional.linear
    q = lin(query, in_w[:d], bq).view(B, L, nhead, D)
    k = lin(key, in_w[d:2 * d], bk).view(B, S, nhead, D)
    v = lin(value, in_w[2 * d:], bv).view(B, S, nhead, D)
    o, _, p = attention(q, k, v, None, attn_bias, key_pad, causal, keep, drop_p)
    return lin(o.reshape(B, L, d), out_w, out_b), p.mean(dim=1)

"""speechbrain.nnet.attention.MultiheadAttention (``attention_type: regularMHA``; the module the reference's
``TransformerDecoderLayer`` holds twice, speechbrain/lobes/models/transformer/Transformer.py:745-751, :811-840, and ``TransformerLM``
is made of): batch-first multi-head scaled-dot-product attention.  Parameters live under ``.att`` with torch's names
(``att.in_proj_weight`` (3d, d), ``att.in_proj_bias``, ``att.out_proj.weight``, ``att.out_proj.bias``), so a reference checkpoint - or a
``torch.nn.MultiheadAttention`` state dict prefixed with ``att.`` - loads with ``strict=True``.

``forward`` holds the checks and the mask conversion; the sublayer itself - projections, fused attention, out-projection and the
backward through all three - is ``functional.attention_sublayer``, the one a decoder layer runs too, here as one autograd node over
(query, key, value) (``functional.node``).  The projections run on the package's Linear route (``functional.linear_fwd`` /
``linear_bwd``): ONE d -> 3d GEMM when ``query is key is value``, d -> d plus d -> 2d when ``key is value``, three GEMMs otherwise.  The fused attention kernels
(csrc/attention.hip) read q / k / v through strides out of the packed projection outputs and write their gradients into the packed
gradient buffer; no (B, H, L, S) tensor exists in the training path.  GPU only; computes in the dtype of ``query`` (float32 or
bfloat16, like ``nnet.linear.Linear``).

Deviations, all stated: a query row whose keys are all masked yields zeros (torch: NaN); the returned attention weights are
DETACHED (no gradient flows through them; upstream's do carry one, nothing in the recipes uses it); ``forward`` takes an extra
``causal=False`` keyword that stands for the (L, L) look-ahead mask without building it."""
import torch
from torch import nn

from .. import functional as F
from .. import ops

HEAD_DIMS = (64, 128, 256, 512)


class _AttParams(nn.Module):
    """Holder with torch.nn.MultiheadAttention's parameter names and initial distributions."""

    def __init__(self, d_model, bias):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.register_parameter("in_proj_bias", nn.Parameter(torch.zeros(3 * d_model)) if bias else None)
        self.out_proj = nn.Linear(d_model, d_model, bias=bias)
        nn.init.xavier_uniform_(self.in_proj_weight)
        if bias:
            nn.init.zeros_(self.out_proj.bias)


def _rows(x):
    x2 = x.reshape(-1, x.shape[-1])
    return x2 if x2.is_contiguous() else x2.contiguous()


class MultiheadAttention(nn.Module):
    def __init__(self, nhead, d_model, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None, vdim=None):
        super().__init__()
        if add_bias_kv:
            raise NotImplementedError("MultiheadAttention: add_bias_kv is not supported (no recipe sets it)")
        if add_zero_attn:
            raise NotImplementedError("MultiheadAttention: add_zero_attn is not supported (no recipe sets it)")
        if (kdim is not None and kdim != d_model) or (vdim is not None and vdim != d_model):
            raise NotImplementedError(f"MultiheadAttention: kdim / vdim other than d_model ({d_model}) are not supported, got kdim={kdim}, vdim={vdim}")
        if d_model % nhead != 0 or d_model // nhead not in HEAD_DIMS:
            raise NotImplementedError(f"MultiheadAttention: head dimension d_model / nhead = {d_model}/{nhead} is not supported; "
                                      f"the attention kernels take {HEAD_DIMS}")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        self.nhead, self.d_model, self.head_dim, self.dropout = nhead, d_model, d_model // nhead, float(dropout)
        self.att = _AttParams(d_model, bias)
        self._bias_cache = None          # (key, fp32 bias): attn_mask converted once per tensor identity

    def _bias_of(self, attn_mask, device):
        key = (id(attn_mask), attn_mask.data_ptr(), attn_mask._version, attn_mask.dtype, tuple(attn_mask.shape), str(device))
        if self._bias_cache is None or self._bias_cache[0] != key:
            self._bias_cache = (key, F.attn_bias_of(attn_mask, device), attn_mask)    # (the mask is held: its id cannot be reused)
        return self._bias_cache[1]

    def forward(self, query, key, value, attn_mask=None, key_padding_mask=None, return_attn_weights=True, pos_embs=None, causal=False):
        """query (B, L, d), key / value (B, S, d); attn_mask: 2-D (L, S) bool (True = masked) or float (additive);
        key_padding_mask: bool (B, S), True = padded key.  Returns (out (B, L, d), weights (B, L, S) fp32 head-averaged, DETACHED),
        or ``out`` alone with return_attn_weights=False (the training path then never computes the weights)."""
        if pos_embs is not None:
            raise NotImplementedError("MultiheadAttention: pos_embs is not supported (positional embeddings added to the keys; RelPosMHAXL is not built)")
        if query.dtype == torch.float16:
            raise TypeError("MultiheadAttention: float16 is not supported (float32 or bfloat16)")
        if query.dtype not in (torch.float32, torch.bfloat16) or key.dtype != query.dtype or value.dtype != query.dtype:
            raise TypeError(f"MultiheadAttention: query / key / value must share float32 or bfloat16, got {query.dtype}, {key.dtype}, {value.dtype}")
        if query.dim() != 3 or key.dim() != 3 or value.dim() != 3 or key.shape[:2] != value.shape[:2] or key.shape[0] != query.shape[0]:
            raise ValueError(f"MultiheadAttention: need query (B, L, d), key / value (B, S, d), got {tuple(query.shape)}, {tuple(key.shape)}, {tuple(value.shape)}")
        if attn_mask is not None and attn_mask.dim() != 2:
            raise NotImplementedError(f"MultiheadAttention: a {attn_mask.dim()}-D attn_mask (per batch / per head) is not supported; pass a 2-D (L, S) mask")
        if not (query.is_cuda and key.is_cuda and value.is_cuda):
            raise RuntimeError(ops.NO_CPU)
        B, Lq, d = query.shape
        S, H = key.shape[1], self.nhead
        assert d == self.d_model and key.shape[2] == d
        if attn_mask is not None and tuple(attn_mask.shape) != (Lq, S):
            raise ValueError(f"attn_mask must be ({Lq}, {S}), got {tuple(attn_mask.shape)}")
        bias = self._bias_of(attn_mask, query.device) if attn_mask is not None else None
        pad = F.key_pad_u8(key_padding_mask, B, S, query.device)
        p = self.dropout if self.training else 0.0
        seed = ops.new_dropout_seed() if p > 0.0 else 0
        att, inputs, kept = self.att, (query, key, value), []

        def run(need):
            xq = _rows(query)
            if query is key and key is value:
                xk = xv = None
            else:
                xk = _rows(key)
                xv = None if key is value else _rows(value)
            out, bwd2, k = F.attention_sublayer(att, H, xq, xk, xv, B, Lq, S, bias, pad, causal, p, seed=seed, need=need,
                                                need_dx=[t.requires_grad for t in inputs])
            kept.append(k)
            if not need:
                return out.view(B, Lq, d), None

            def bwd(dy):
                return tuple(g.view(t.shape) if g is not None else None for g, t in zip(bwd2(_rows(dy)), inputs))
            return out.view(B, Lq, d), bwd

        out = F.node(run, inputs, (att.in_proj_weight, att.in_proj_bias, att.out_proj.weight, att.out_proj.bias))
        if not return_attn_weights:
            return out
        return out, F.attention_sublayer_weights(kept[0])

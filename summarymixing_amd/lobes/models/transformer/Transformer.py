"""The seq2seq side of speechbrain/lobes/models/transformer/Transformer.py on MI355X: NormalizedEmbedding (:991-1021),
TransformerDecoderLayer (:683-866), TransformerDecoder (:869-987), get_key_padding_mask (:1024-1060) and get_lookahead_mask
(:1063-1090), with upstream's names, arguments and ``state_dict`` keys.  (PositionalEncoding, :284-335, lives in TransformerASR.py.)

A decoder - its layers and the final LayerNorm - is ONE autograd node over (tgt, memory) (functional.node), built like
functional.encoder_stack: every sublayer is a (forward, backward-closure) pair on the package's kernels and the gradient between two
layers never visits autograd; parameter gradients are accumulated into ``param.grad`` by the kernels.  Both attention sublayers of a
layer are functional.attention_sublayer on the parameters of its two MultiheadAttention modules - the code their own ``forward``
runs.  Per layer: norm1 -> ONE d -> 3d projection GEMM -> the
fused causal self-attention (csrc/attention.hip; the look-ahead mask is the kernels' ``causal`` flag, no (U, U) tensor exists) ->
the out-projection with dropout1 and the residual in its epilogue; norm2 -> d -> d on the targets and d -> 2d on the memory -> the
fused cross-attention -> out-projection + dropout2 + residual; then functional.ffn_module_fwd with alpha = 1 and eps = 1e-6 (norm3,
both FFN dropouts and the residual in the two GEMM epilogues).  normalize_before=False runs the same kernels in upstream's other
order (:806-859): residual first, LayerNorm after.

Residual stream: functional.stream_dtype - float32 for a bf16 model with normalize_before=True, as autocast keeps it upstream; with
normalize_before=False the LayerNorm output IS the stream and stays in the compute dtype.  ``memory`` is cast to the compute dtype
once per forward.  GPU only (a CPU tensor raises ops.NO_CPU).

Decoding one position at a time (TransformerDecoder.step, TransformerDecoderLayer._step, DecodeState): the same sublayers at inference,
the two attention launches replaced by smx_attn_step over a self-attention cache and the once-projected memory.

Deviations, all stated: a query row whose keys are all masked yields zeros (torch: NaN); returned attention weights are detached;
``tgt_mask`` may be the module constant LOOKAHEAD instead of the dense matrix (what TransformerASR.forward / decode pass); the
embedding maps a token outside [0, V) to a zero row where torch raises."""
import torch
from torch import nn

from .... import _lib as L
from .... import functional as F
from .... import ops
from ....nnet.activations import act_code
from ....nnet.attention import MultiheadAttention
from .Conformer import _FFN, _LayerNorm


class _Lookahead:
    """Stands for get_lookahead_mask(tgt) as ``tgt_mask``: the attention kernels then run with causal=True."""

    def __repr__(self):
        return "LOOKAHEAD"


LOOKAHEAD = _Lookahead()


def get_key_padding_mask(padded_input, pad_idx):
    """Transformer.py:1024-1060: True where the input equals pad_idx (for a 3-D / 4-D input: where every channel does)."""
    if padded_input.dim() == 4:
        bz, time, ch1, ch2 = padded_input.shape
        padded_input = padded_input.reshape(bz, time, ch1 * ch2)
    key_padded_mask = padded_input.eq(pad_idx)
    if padded_input.dim() > 2:
        key_padded_mask = key_padded_mask.float().prod(dim=-1).bool()
    return key_padded_mask.detach()


def get_lookahead_mask(padded_input):
    """Transformer.py:1063-1090: the (U, U) float mask, 0 on and below the diagonal, -inf above it."""
    seq_len = padded_input.shape[1]
    mask = (torch.triu(torch.ones((seq_len, seq_len), device=padded_input.device)) == 1).transpose(0, 1)
    mask = mask.float().masked_fill(mask == 0, float("-inf")).masked_fill(mask == 1, float(0.0))
    return mask.detach()


class _TgtEmbedFn(torch.autograd.Function):
    """tokens -> (table[tokens] sqrt(d) + pe, tokens == pad_idx): smx_tgt_embed_fwd; the backward adds into table.grad
    (smx_tgt_embed_bwd, fixed order, no atomics) and returns nothing to autograd, like every parameter gradient of the package."""

    @staticmethod
    def forward(ctx, tokens, table, pe, pad_idx, padding_idx, out_dtype):
        y, flags = ops.tgt_embed_fwd(tokens, table.detach(), pe, pad_idx, out_dtype)
        ctx.tokens, ctx.table, ctx.padding_idx = tokens, table, padding_idx
        ctx.mark_non_differentiable(flags)
        return y, flags

    @staticmethod
    def backward(ctx, dy, _):
        g = F.gacc(ctx.table)
        if g is not None:
            dy = dy if dy.is_contiguous() else dy.contiguous()
            ops.tgt_embed_bwd(ctx.tokens, dy, g, ctx.padding_idx)
        return None, None, None, None, None, None


class _EmbeddingHolder(nn.Module):
    """Key layout of speechbrain.nnet.embedding.Embedding(consider_as_one_hot=False): ``Embedding.weight`` (V, d), a trainable
    nn.Embedding with padding_idx = blank_id.  (nnet.embedding.Embedding is the frozen one-hot table of the transducer recipe.)"""

    def __init__(self, num_embeddings, embedding_dim, blank_id=0):
        super().__init__()
        self.Embedding = nn.Embedding(num_embeddings, embedding_dim, padding_idx=blank_id)


class NormalizedEmbedding(nn.Module):
    """emb(tokens) * sqrt(d_model) (Transformer.py:991-1021).  ``embed`` is the fused form TransformerASR uses: the same launch adds
    the positional rows and writes the key-padding mask."""

    def __init__(self, d_model, vocab):
        super().__init__()
        if d_model % 8 != 0:
            raise NotImplementedError(f"NormalizedEmbedding: d_model must be a multiple of 8 (16-byte rows), got {d_model}")
        self.emb = _EmbeddingHolder(vocab, d_model, blank_id=0)
        self.d_model = d_model
        self._zero_pe = None

    def embed(self, tokens, pe, pad_idx=0, out_dtype=torch.float32):
        """tokens (B, U), pe (>= U, d) fp32 -> (y (B, U, d) in out_dtype, key_padding_mask (B, U) bool)."""
        if not tokens.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        if tokens.dim() != 2:
            raise ValueError(f"NormalizedEmbedding: tokens must be (B, U), got {tuple(tokens.shape)}")
        table = self.emb.Embedding.weight
        if torch.is_grad_enabled() and table.requires_grad:
            return _TgtEmbedFn.apply(tokens, table, pe, pad_idx, self.emb.Embedding.padding_idx, out_dtype)
        return ops.tgt_embed_fwd(tokens, table.detach(), pe, pad_idx, out_dtype)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        U = x.shape[1]
        if self._zero_pe is None or self._zero_pe.shape[0] < U or self._zero_pe.device != x.device:
            self._zero_pe = torch.zeros((U, self.d_model), dtype=torch.float32, device=x.device)
        return self.embed(x, self._zero_pe[:U])[0]


class TransformerDecoderLayer(nn.Module):
    def __init__(self, d_ffn, nhead, d_model, kdim=None, vdim=None, dropout=0.0, activation=nn.ReLU, normalize_before=False,
                 attention_type="regularMHA", causal=None):
        super().__init__()
        if attention_type == "RelPosMHAXL":
            raise NotImplementedError("TransformerDecoderLayer: attention_type='RelPosMHAXL' is not built (regularMHA only)")
        if attention_type != "regularMHA":
            raise NotImplementedError(f"TransformerDecoderLayer: attention_type={attention_type!r} is not supported (regularMHA only)")
        if (kdim is not None and kdim != d_model) or (vdim is not None and vdim != d_model):
            raise NotImplementedError(f"TransformerDecoderLayer: kdim / vdim other than d_model ({d_model}) are not supported, "
                                      f"got kdim={kdim}, vdim={vdim}")
        self.nhead, self.d_model, self.normalize_before, self.causal = nhead, d_model, bool(normalize_before), causal
        self.p_drop = float(dropout)
        self.act = act_code(activation)
        if self.act == L.ACT_NONE:
            raise NotImplementedError("TransformerDecoderLayer: the feed-forward needs an activation (ReLU, GELU, Swish, LeakyReLU)")
        self.self_attn = MultiheadAttention(nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout)
        self.multihead_attn = MultiheadAttention(nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout)
        self.pos_ffn = _FFN(d_ffn, d_model, dropout, activation)
        self.norm1 = _LayerNorm(d_model, eps=1e-6)
        self.norm2 = _LayerNorm(d_model, eps=1e-6)
        self.norm3 = _LayerNorm(d_model, eps=1e-6)
        self.dropout1 = nn.Dropout(dropout)      # (markers, as upstream names them: the dropouts run in the GEMM epilogues)
        self.dropout2 = nn.Dropout(dropout)
        self.dropout3 = nn.Dropout(dropout)

    def _run(self, B, U, S, compute, mem2, sbias, causal, tpad, mbias, mpad, need_dmem):
        """-> run(x (B U, d) stream rows, need) -> (y, bwd, kept_self, kept_cross); bwd(dy, dmem) -> (dx, dmem + this layer's)."""
        pre = self.normalize_before
        p = self.p_drop if self.training else 0.0
        n1, n2, n3 = self.norm1.norm, self.norm2.norm, self.norm3.norm
        f0, f3 = self.pos_ffn.ffn[0], self.pos_ffn.ffn[3]
        act, H = self.act, self.nhead
        sa, ca = self.self_attn.att, self.multihead_attn.att
        need_dx = (True, need_dmem)

        def site():
            return (p, ops.new_dropout_seed()) if p > 0.0 else None

        def run(x, need):
            if pre:
                h1, lb1 = F.ln_fwd(x, n1.weight, n1.bias, n1.eps, need, out_dtype=compute)
                x1, ab1, ks = F.attention_sublayer(sa, H, h1, None, None, B, U, U, sbias, tpad, causal, p, res=x, drop=site(), need=need)
                h2, lb2 = F.ln_fwd(x1, n2.weight, n2.bias, n2.eps, need, out_dtype=compute)
                x2, ab2, kc = F.attention_sublayer(ca, H, h2, mem2, None, B, U, S, mbias, mpad, False, p, res=x1, drop=site(), need=need,
                                                    need_dx=need_dx)
                P = {"ln_w": n3.weight, "ln_b": n3.bias, "W1": f0.weight, "b1": f0.bias, "W2": f3.weight, "b2": f3.bias}
                y, fb = F.ffn_module_fwd(x2, P, act, need, compute, alpha=1.0, p=p, eps=n3.eps)
                if not need:
                    return y, None, ks, kc

                def bwd(dy, dmem):
                    g2 = fb(dy)
                    dh2, dmem, _ = ab2(g2, None, dmem)
                    g1 = lb2(dh2, res=g2)
                    dh1 = ab1(g1)[0]
                    return lb1(dh1, res=g1), dmem
                return y, bwd, ks, kc
            t1, ab1, ks = F.attention_sublayer(sa, H, x, None, None, B, U, U, sbias, tpad, causal, p, res=x, drop=site(), need=need)
            x1, lb1 = F.ln_fwd(t1, n1.weight, n1.bias, n1.eps, need)
            t2, ab2, kc = F.attention_sublayer(ca, H, x1, mem2, None, B, U, S, mbias, mpad, False, p, res=x1, drop=site(), need=need,
                                                need_dx=need_dx)
            x2, lb2 = F.ln_fwd(t2, n2.weight, n2.bias, n2.eps, need)
            W1, W2 = F.wcast(f0.weight, compute), F.wcast(f3.weight, compute)
            d1, d2 = site(), site()
            a, z1 = F.linear_fwd(x2, W1, f0.bias, act, None, save_z=need, drop=d1, wparam=f0.weight)
            t3, _ = F.linear_fwd(a, W2, f3.bias, L.ACT_NONE, None, res=x2, drop=d2, wparam=f3.weight)
            y, lb3 = F.ln_fwd(t3, n3.weight, n3.bias, n3.eps, need)
            if not need:
                return y, None, ks, kc

            def bwd(dy, dmem):
                g3 = lb3(dy)
                dz1, _ = F.linear_bwd(g3, a, W2, None, L.ACT_NONE, None, 1.0, F.gacc(f3.weight), F.gacc(f3.bias), drop=d2,
                                      up=(z1, act, None, 1.0, d1, None), wparam=f3.weight)
                g2, _ = F.linear_bwd(dz1, x2, W1, z1, act, None, 1.0, F.gacc(f0.weight), F.gacc(f0.bias), dz_ready=True, res_grad=g3)
                g2 = lb2(g2)
                g1, dmem, _ = ab2(g2, g2, dmem)
                g1 = lb1(g1)
                return ab1(g1, g1)[0], dmem
            return y, bwd, ks, kc
        return run

    def _step(self, x, compute, self_kv, cross_kv, pos, mem_len, attn_out=None, attn_ws=None, anc=None, kv_div=None):
        """ONE decoding position, inference only: x (B, d) stream rows -> the layer's output rows.  _run's sublayers at need=False in
        the same order and dtypes, the two smx_attn_fwd calls replaced by smx_attn_step over the layer's caches (self_kv (B, cap, 2,
        H, D), the keys / values so far, slot pos - 1 written here; cross_kv (B, S, 2, H, D), the projected memory); no weights.
        attn_out / attn_ws: the state's attention output and workspace, shared by the launches of a step (each is consumed by its
        out-projection before the next attention writes it: one stream).  anc / kv_div (a beam state): x holds B W rows, the
        self-attention reads its keys through the ancestor table anc, the W rows of an utterance share its row of cross_kv / mem_len."""
        kw = {"out": attn_out, "workspace": attn_ws}
        skw = dict(kw, anc=anc) if anc is not None else kw
        ckw = dict(kw, kv_div=kv_div) if kv_div is not None else kw
        n1, n2, n3 = self.norm1.norm, self.norm2.norm, self.norm3.norm
        f0, f3 = self.pos_ffn.ffn[0], self.pos_ffn.ffn[3]
        sa, ca, H = self.self_attn.att, self.multihead_attn.att, self.nhead
        if self.normalize_before:
            h1, _ = F.ln_fwd(x, n1.weight, n1.bias, n1.eps, False, out_dtype=compute)
            x1 = F.attention_step_sublayer(sa, H, h1, self_kv, pos, x, True, **skw)
            h2, _ = F.ln_fwd(x1, n2.weight, n2.bias, n2.eps, False, out_dtype=compute)
            x2 = F.attention_step_sublayer(ca, H, h2, cross_kv, mem_len, x1, False, **ckw)
            P = {"ln_w": n3.weight, "ln_b": n3.bias, "W1": f0.weight, "b1": f0.bias, "W2": f3.weight, "b2": f3.bias}
            return F.ffn_module_fwd(x2, P, self.act, False, compute, alpha=1.0, p=0.0, eps=n3.eps)[0]
        t1 = F.attention_step_sublayer(sa, H, x, self_kv, pos, x, True, **skw)
        x1, _ = F.ln_fwd(t1, n1.weight, n1.bias, n1.eps, False)
        t2 = F.attention_step_sublayer(ca, H, x1, cross_kv, mem_len, x1, False, **ckw)
        x2, _ = F.ln_fwd(t2, n2.weight, n2.bias, n2.eps, False)
        a, _ = F.linear_fwd(x2, F.wcast(f0.weight, compute), f0.bias, self.act, None, wparam=f0.weight)
        t3, _ = F.linear_fwd(a, F.wcast(f3.weight, compute), f3.bias, L.ACT_NONE, None, res=x2, wparam=f3.weight)
        return F.ln_fwd(t3, n3.weight, n3.bias, n3.eps, False)[0]

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None,
                pos_embs_tgt=None, pos_embs_src=None):
        """-> (out (B, U, d) in tgt's dtype, self-attention weights (B, U, U), cross-attention weights (B, U, S)), Transformer.py:806-859."""
        out, sa, ca = _decode_stack([self], None, tgt, memory, tgt_mask, memory_mask, tgt_key_padding_mask, memory_key_padding_mask,
                                    pos_embs_tgt, pos_embs_src, "all")
        return out, sa[0], ca[0]


def _decode_stack(layers, norm, tgt, memory, tgt_mask, memory_mask, tgt_kpm, mem_kpm, pos_embs_tgt, pos_embs_src, weights):
    """The layers (+ the final LayerNorm `norm`) over (tgt, memory).  weights: "all" | "last_cross" | "none".  Output dtype: the compute
    dtype behind a final norm, tgt's dtype without one.  -> (out, [self weights], [cross weights]) (None where not computed)."""
    if pos_embs_tgt is not None or pos_embs_src is not None:
        raise NotImplementedError("TransformerDecoder: pos_embs_tgt / pos_embs_src are not supported (RelPosMHAXL is not built)")
    if not (tgt.is_cuda and memory.is_cuda):
        raise RuntimeError(ops.NO_CPU)
    if tgt.dim() != 3 or memory.dim() != 3 or tgt.shape[0] != memory.shape[0] or tgt.shape[2] != memory.shape[2]:
        raise ValueError(f"TransformerDecoder: need tgt (B, U, d) and memory (B, S, d), got {tuple(tgt.shape)}, {tuple(memory.shape)}")
    for t in (tgt, memory):
        if t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"TransformerDecoder: float32 or bfloat16 only, got {t.dtype}")
    B, U, d = tgt.shape
    S = memory.shape[1]
    compute = memory.dtype if tgt.dtype == torch.float32 else tgt.dtype
    pre = layers[0].normalize_before
    stream = F.stream_dtype(compute) if pre else compute
    dev = tgt.device
    causal = tgt_mask is LOOKAHEAD
    sbias = None if (causal or tgt_mask is None) else F.attn_bias_of(tgt_mask, dev)
    mbias = None if memory_mask is None else F.attn_bias_of(memory_mask, dev)
    if sbias is not None and tuple(sbias.shape) != (U, U):
        raise ValueError(f"tgt_mask must be ({U}, {U}), got {tuple(sbias.shape)}")
    if mbias is not None and tuple(mbias.shape) != (U, S):
        raise ValueError(f"memory_mask must be ({U}, {S}), got {tuple(mbias.shape)}")
    tpad, mpad = F.key_pad_u8(tgt_kpm, B, U, dev), F.key_pad_u8(mem_kpm, B, S, dev)
    params = [p for l in layers for p in l.parameters()] + ([norm.weight, norm.bias] if norm is not None else [])
    need_dmem = torch.is_grad_enabled() and memory.requires_grad
    kept = []

    def run(need):
        mem2 = ops.rows2d(memory)
        if mem2.dtype != compute:
            mem2 = ops.cast(mem2, compute)                    # once per forward, not once per layer
        x = ops.rows2d(tgt if tgt.is_contiguous() else tgt.contiguous())
        if x.dtype != stream:
            x = ops.cast(x, stream)
        bwds = []
        for layer in layers:
            x, b, ks, kc = layer._run(B, U, S, compute, mem2, sbias, causal, tpad, mbias, mpad, need_dmem)(x, need)
            bwds.append(b)
            kept.append((ks, kc))
        bn = None
        if norm is not None:
            x, bn = F.ln_fwd(x, norm.weight, norm.bias, norm.eps, need, out_dtype=compute)
        elif x.dtype != tgt.dtype:
            x = ops.cast(x, tgt.dtype)
        if not need:
            return x.view(B, U, d), None

        def bwd(dy3):
            dy = ops.rows2d(dy3 if dy3.is_contiguous() else dy3.contiguous())
            if dy.dtype != compute:
                dy = ops.cast(dy, compute)
            g = bn(dy) if bn is not None else dy
            F.flush_deferred()
            dmem = None
            for b in reversed(bwds):
                g, dmem = b(g, dmem)
                F.flush_deferred()
            if g.dtype != tgt.dtype:
                g = ops.cast(g, tgt.dtype)
            if dmem is not None and dmem.dtype != memory.dtype:
                dmem = ops.cast(dmem, memory.dtype)
            return g.view(B, U, d), (dmem.view(B, S, d) if dmem is not None else None)
        return x.view(B, U, d), bwd

    out = F.node(run, (tgt, memory), params)
    n = len(layers)
    sa = [F.attention_sublayer_weights(ks) if weights == "all" else None for ks, _ in kept]
    ca = [F.attention_sublayer_weights(kc) if (weights == "all" or (weights == "last_cross" and i == n - 1)) else None for i, (_, kc) in enumerate(kept)]
    return out, sa, ca


class TransformerDecoder(nn.Module):
    def __init__(self, num_layers, nhead, d_ffn, d_model, kdim=None, vdim=None, dropout=0.0, activation=nn.ReLU,
                 normalize_before=False, causal=False, attention_type="regularMHA"):
        super().__init__()
        if num_layers < 1:
            raise ValueError(f"TransformerDecoder: num_layers must be >= 1, got {num_layers}")
        self.layers = nn.ModuleList([
            TransformerDecoderLayer(d_ffn=d_ffn, nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout,
                                    activation=activation, normalize_before=normalize_before, causal=causal,
                                    attention_type=attention_type)
            for _ in range(num_layers)])
        self.norm = _LayerNorm(d_model, eps=1e-6)

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None,
                pos_embs_tgt=None, pos_embs_src=None, _weights="all"):
        """-> (out (B, U, d) in the compute dtype, [self-attention weights per layer], [cross-attention weights per layer]),
        Transformer.py:936-987.  _weights ("all" | "last_cross" | "none"): which weights to compute; the others are None
        (TransformerASR.forward asks for none, decode for the last layer's cross-attention)."""
        return _decode_stack(list(self.layers), self.norm.norm, tgt, memory, tgt_mask, memory_mask, tgt_key_padding_mask,
                             memory_key_padding_mask, pos_embs_tgt, pos_embs_src, _weights)

    @torch.no_grad()
    def step(self, x, state):
        """ONE decoding position through every layer and the final LayerNorm: x (B, d) stream rows (the embedding of the step, after
        which state.pos counts this position) -> (B, d) in the compute dtype.  Writes slot pos - 1 of every layer's self-attention
        cache; nothing synchronises with the host."""
        for layer, skv, ckv in zip(self.layers, state.self_kv, state.cross_kv):
            x = layer._step(x, state.compute, skv, ckv, state.pos, state.mem_len, state.attn_out, state.attn_ws, **state.rows_kw)
        n = self.norm.norm
        return F.ln_fwd(x, n.weight, n.bias, n.eps, False, out_dtype=state.compute)[0]


class DecodeState:
    """What KV-cached decoding carries from step to step (TransformerASR.make_decode_state), all on the device.  Per decoder layer:
    self_kv[i] (B, cap, 2, H, D), the self-attention keys / values of the positions fed so far, and cross_kv[i] (B, S, 2, H, D), the
    layer's d -> 2d projection of the encoder output, computed once.  pos (B) int32: positions fed (the self-attention key count);
    mem_len (B) int32: encoder lengths (the cross-attention key count).  The search's own vectors: tok (B) int32 the next input token,
    done (B) uint8, n_tok (B) int32, score (B) fp32, tokens (B, cap) int32, logp_tok (B, cap) fp32.  Every step reads and advances
    these in kernels; the host never needs their values to issue the next step.  attn_out (B, H, D) / attn_ws: the output and the split
    workspace of the step's attention launches, owned here so that a step's 2 x layers smx_attn_step calls allocate nothing.

    beam=W (beam search, decoders.seq2seq.beam_search): R = B W hypothesis rows, utterance b owns rows [b W, (b + 1) W).  self_kv,
    attn_out, pos, tok, score, tokens, logp_tok have R rows; cross_kv and mem_len stay per utterance (kv_div = W: nothing is
    replicated); done and n_tok stay per utterance, row_done (R) is what the embedding step reads.  anc (R, cap) int32 names, per
    row and position, the cache row that holds that position's key - the beams reorder by rewriting anc, no K / V moves
    (smx_attn_step_rows).  Then the buffers of smx_s2s_beam_select: the scratch tables of its gathers (s_*), the candidate workspace
    (cand_*), the pool of finished hypotheses (pool_*) and the sorted result (res_*).  Without beam none of these exist, row_done is
    done and every call is the plain one."""

    def __init__(self, B, S, cap, H, D, layers, compute, stream, device, beam=None):
        self.B, self.S, self.cap, self.compute, self.stream, self.beam = B, S, cap, compute, stream, beam
        R = self.rows = B if beam is None else B * beam
        self.self_kv = [torch.zeros((R, cap, 2, H, D), dtype=compute, device=device) for _ in range(layers)]
        self.cross_kv = [torch.empty((B, S, 2, H, D), dtype=compute, device=device) for _ in range(layers)]
        self.attn_out = torch.empty((R, H, D), dtype=compute, device=device)
        self.attn_ws = torch.empty((max(1, ops.attention_step_workspace(R, H, D, cap, compute), ops.attention_step_workspace(R, H, D, S, compute)),),
                                   dtype=torch.float32, device=device)
        self.pos = torch.zeros((R,), dtype=torch.int32, device=device)
        self.mem_len = torch.empty((B,), dtype=torch.int32, device=device)
        self.tok = torch.zeros((R,), dtype=torch.int32, device=device)
        self.done = torch.zeros((B,), dtype=torch.uint8, device=device)
        self.n_tok = torch.zeros((B,), dtype=torch.int32, device=device)
        self.score = torch.zeros((R,), dtype=torch.float32, device=device)
        self.tokens = torch.full((R, cap), -1, dtype=torch.int32, device=device)
        self.logp_tok = torch.zeros((R, cap), dtype=torch.float32, device=device)
        self.row_done, self.rows_kw = self.done, {}
        if beam is not None:
            W = beam

            def buf(shape, dtype):
                return torch.zeros(shape, dtype=dtype, device=device)
            i32, f32 = torch.int32, torch.float32
            self.row_done = buf((R,), torch.uint8)
            self.anc = buf((R, cap), i32)
            self.rows_kw = {"anc": self.anc, "kv_div": W}
            self.s_tokens, self.s_logp, self.s_anc = buf((R, cap), i32), buf((R, cap), f32), buf((R, cap), i32)
            self.cand_val, self.cand_lp, self.cand_idx, self.cand_n = buf((R, W), f32), buf((R, W), f32), buf((R, W), i32), buf((R,), i32)
            self.pool_tokens, self.pool_logp = buf((B, W, cap), i32), buf((B, W, cap), f32)
            self.pool_len, self.pool_final, self.pool_sum, self.pool_seq = buf((B, W), i32), buf((B, W), f32), buf((B, W), f32), buf((B, W), i32)
            self.pool_cnt, self.pool_ins = buf((B,), i32), buf((B,), i32)
            self.res_tokens, self.res_logp = buf((B, W, cap), i32), buf((B, W, cap), f32)
            self.res_len, self.res_final, self.res_sum = buf((B, W), i32), buf((B, W), f32), buf((B, W), f32)
            self._reset_beam()

    def reset(self):
        """Back to position 0 with an empty hypothesis, in place (the buffers a captured step points at stay where they are).  The
        caches need no clearing: slots at or beyond pos are never read."""
        for t in (self.pos, self.tok, self.done, self.n_tok, self.score, self.logp_tok):
            t.zero_()
        self.tokens.fill_(-1)
        if self.beam is not None:
            self._reset_beam()

    def _reset_beam(self):
        """Slot 0 of every utterance alive with score 0, the others dead; no ancestors (-1 names no row); an empty pool and result.
        The pool's rows, the scratch tables and the candidate workspace are written before they are read: no clearing."""
        self.score.fill_(float("-inf"))
        self.score.view(self.B, self.beam)[:, 0] = 0.0
        self.anc.fill_(-1)
        for t in (self.row_done, self.pool_cnt, self.pool_ins, self.res_len, self.res_sum, self.res_logp):
            t.zero_()
        self.res_tokens.fill_(-1)
        self.res_final.fill_(float("-inf"))

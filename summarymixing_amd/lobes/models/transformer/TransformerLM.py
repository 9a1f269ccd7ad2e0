"""speechbrain.lobes.models.transformer.TransformerLM.TransformerLM on MI355X, inference only: the language model the LibriSpeech
recipe decodes with (recipes/LibriSpeech/ASR/transformer/hparams/branchformer_summarymixing.yaml:182-191, ``lm_model``), a causal
Transformer encoder over token embeddings with a three-stage output head.  ``TransformerLM.py`` is not part of the reference tree:
the constructor arguments and the outer ``state_dict`` groups (``custom_src_module``, ``output_proj``, ``positional_encoding``) are
upstream's, stated from memory; the layers are the reference's TransformerEncoder / TransformerEncoderLayer with
attention_type="regularMHA" (speechbrain/lobes/models/transformer/Transformer.py:338-526, :529-690; LayerNorms with eps 1e-6, both
normalize_before orders), whose keys tests/golden/transformerlm_state_keys.json records, so upstream's ``lm.ckpt`` loads with
strict=True.

forward(src (B, U) tokens) -> logits (B, U, vocab): smx_tgt_embed_fwd (embedding * sqrt(d) + positional rows + the key-padding mask
src == pad_idx 0, one launch), per layer functional.attention_sublayer(causal=True) + LayerNorm + the feed-forward route of the decoder
layer, ``encoder.norm``, then ``output_proj`` (Linear d -> d, LayerNorm, Linear d -> vocab, no activation between them).  The
residual stream is float32 under a bf16 compute dtype with normalize_before=True, as the decoder has it.

make_state(R, cap, dtype, device) / step(tokens (R,), state, anc=None): the KV-cached form, one row per hypothesis: per layer a
self-attention cache (R, cap, 2, H, D), smx_s2s_embed_step on the state's own position counters (advanced under state.done - a beam
search hands its done_row in, so that the host issues identical launches at every step), self-attention through
functional.attention_step_sublayer(anc=anc): with the ancestor table of a beam search the LM's hypotheses are the decoder's and no
K / V moves when the beams reorder.
Padding: the step applies NO key-padding mask.  For a prefix without pad_idx it computes forward(prefix)[:, -1]; for a prefix that
holds pad_idx it keeps that token visible where forward (and upstream) masks it.  Under the recipes' joint scorer no hypothesis can
hold one: the CTC scorer gives blank == pad the score -inf.

Not built, refused by name: num_decoder_layers != 0, d_embedding, decoder_use_memory, attention types other than regularMHA,
positional encodings other than fixed_abs_sine, causal=False, head dimensions outside nnet.attention.HEAD_DIMS, training mode with
dropout > 0, and any call that needs gradients."""
import torch
from torch import nn

from .... import _lib as L
from .... import functional as F
from .... import ops
from ....nnet.activations import act_code
from ....nnet.attention import HEAD_DIMS, MultiheadAttention
from ...models.VanillaNN import Linear
from .Conformer import _FFN, _LayerNorm
from .Transformer import NormalizedEmbedding
from .TransformerASR import PositionalEncoding


class _LMEncoderLayer(nn.Module):
    """Key layout of TransformerEncoderLayer(attention_type="regularMHA"): self_att.att.*, pos_ffn.ffn.{0,3}.*, norm{1,2}.norm.*."""

    def __init__(self, d_ffn, nhead, d_model, dropout, activation, normalize_before):
        super().__init__()
        self.nhead, self.d_model, self.normalize_before = nhead, d_model, bool(normalize_before)
        self.act = act_code(activation)
        if self.act == L.ACT_NONE:
            raise NotImplementedError("TransformerLM: the feed-forward needs an activation (ReLU, GELU, Swish, LeakyReLU)")
        self.self_att = MultiheadAttention(nhead=nhead, d_model=d_model, dropout=dropout)
        self.pos_ffn = _FFN(d_ffn, d_model, dropout, activation)
        self.norm1 = _LayerNorm(d_model, eps=1e-6)
        self.norm2 = _LayerNorm(d_model, eps=1e-6)
        self.dropout1 = nn.Dropout(dropout)      # (markers, as upstream names them: inference runs no dropout)
        self.dropout2 = nn.Dropout(dropout)

    def _ffn(self, x, compute):
        """The feed-forward half on stream rows x, both orders (the decoder layer's route)."""
        n2, f0, f3 = self.norm2.norm, self.pos_ffn.ffn[0], self.pos_ffn.ffn[3]
        if self.normalize_before:
            P = {"ln_w": n2.weight, "ln_b": n2.bias, "W1": f0.weight, "b1": f0.bias, "W2": f3.weight, "b2": f3.bias}
            return F.ffn_module_fwd(x, P, self.act, False, compute, alpha=1.0, p=0.0, eps=n2.eps)[0]
        a, _ = F.linear_fwd(x, F.wcast(f0.weight, compute), f0.bias, self.act, None, wparam=f0.weight)
        t, _ = F.linear_fwd(a, F.wcast(f3.weight, compute), f3.bias, L.ACT_NONE, None, res=x, wparam=f3.weight)
        return F.ln_fwd(t, n2.weight, n2.bias, n2.eps, False)[0]

    def _full(self, x, B, U, compute, pad):
        """x (B U, d) stream rows of whole sequences -> the layer's output rows (Transformer.py:493-526), causal."""
        n1, sa, H = self.norm1.norm, self.self_att.att, self.nhead
        if self.normalize_before:
            h, _ = F.ln_fwd(x, n1.weight, n1.bias, n1.eps, False, out_dtype=compute)
            x1 = F.attention_sublayer(sa, H, h, None, None, B, U, U, None, pad, True, 0.0, res=x, need=False)[0]
        else:
            t = F.attention_sublayer(sa, H, x, None, None, B, U, U, None, pad, True, 0.0, res=x, need=False)[0]
            x1, _ = F.ln_fwd(t, n1.weight, n1.bias, n1.eps, False)
        return self._ffn(x1, compute)

    def _step(self, x, compute, self_kv, pos, attn_out, attn_ws, anc):
        """ONE position: x (R, d) stream rows; _full's sublayers with smx_attn_step over the layer's cache (slot pos - 1 written
        here), read through the ancestor table anc when there is one."""
        n1, sa, H = self.norm1.norm, self.self_att.att, self.nhead
        kw = {"out": attn_out, "workspace": attn_ws}
        if anc is not None:
            kw["anc"] = anc
        if self.normalize_before:
            h, _ = F.ln_fwd(x, n1.weight, n1.bias, n1.eps, False, out_dtype=compute)
            x1 = F.attention_step_sublayer(sa, H, h, self_kv, pos, x, True, **kw)
        else:
            t = F.attention_step_sublayer(sa, H, x, self_kv, pos, x, True, **kw)
            x1, _ = F.ln_fwd(t, n1.weight, n1.bias, n1.eps, False)
        return self._ffn(x1, compute)


class _LMEncoder(nn.Module):
    """Key layout of TransformerEncoder: layers.{i}.* and norm.norm.* (eps 1e-6)."""

    def __init__(self, num_layers, nhead, d_ffn, d_model, dropout, activation, normalize_before):
        super().__init__()
        self.layers = nn.ModuleList([_LMEncoderLayer(d_ffn, nhead, d_model, dropout, activation, normalize_before)
                                     for _ in range(num_layers)])
        self.norm = _LayerNorm(d_model, eps=1e-6)


class _OutputProj(nn.Module):
    """Key layout of upstream's output_proj, a ModuleList container: layers.0.w (d -> d), layers.1.norm (LayerNorm, eps 1e-6),
    layers.2.w (d -> vocab)."""

    def __init__(self, d_model, vocab):
        super().__init__()
        self.layers = nn.ModuleList([Linear(d_model, input_size=d_model), _LayerNorm(d_model, eps=1e-6), Linear(vocab, input_size=d_model)])


class LMState:
    """What the cached LM step carries (TransformerLM.make_state), all on the device: per layer self_kv[i] (R, cap, 2, H, D); pos (R)
    int32 the positions fed; done (R) uint8 what smx_s2s_embed_step reads (its own zeros; a beam search points it at its done_row);
    attn_out / attn_ws the attention launches' output and split workspace.  The caches need no clearing: slots at or beyond pos are
    never read."""

    def __init__(self, R, cap, H, D, layers, compute, stream, device):
        self.R = self.rows = R
        self.cap, self.compute, self.stream = cap, compute, stream
        self.self_kv = [torch.zeros((R, cap, 2, H, D), dtype=compute, device=device) for _ in range(layers)]
        self.attn_out = torch.empty((R, H, D), dtype=compute, device=device)
        self.attn_ws = torch.empty((max(1, ops.attention_step_workspace(R, H, D, cap, compute)),), dtype=torch.float32, device=device)
        self.pos = torch.zeros((R,), dtype=torch.int32, device=device)
        self.own_done = self.done = torch.zeros((R,), dtype=torch.uint8, device=device)

    def reset(self):
        """Back to position 0, in place (the buffers a captured step points at stay where they are)."""
        self.pos.zero_()
        self.own_done.zero_()


class TransformerLM(nn.Module):
    def __init__(self, vocab, d_model=512, nhead=8, num_encoder_layers=12, num_decoder_layers=0, d_ffn=2048, dropout=0.1,
                 activation=nn.ReLU, positional_encoding="fixed_abs_sine", normalize_before=False, d_embedding=None, max_length=2500,
                 causal=True, attention_type="regularMHA", decoder_use_memory=False):
        super().__init__()
        if num_decoder_layers != 0:
            raise NotImplementedError(f"TransformerLM: num_decoder_layers={num_decoder_layers} is not built (the recipes' LM is "
                                      "encoder-only: 0)")
        if d_embedding is not None:
            raise NotImplementedError(f"TransformerLM: d_embedding={d_embedding} (an embedding projection) is not built")
        if attention_type != "regularMHA":
            raise NotImplementedError(f"TransformerLM: attention_type={attention_type!r} is not built (regularMHA only)")
        if positional_encoding != "fixed_abs_sine":
            raise NotImplementedError(f"TransformerLM: positional_encoding={positional_encoding!r} is not built (fixed_abs_sine only)")
        if not causal:
            raise NotImplementedError("TransformerLM: causal=False is not built (a language model attends to its past)")
        if decoder_use_memory:
            raise NotImplementedError("TransformerLM: decoder_use_memory=True is not built (there is no decoder)")
        if num_encoder_layers < 1:
            raise ValueError(f"TransformerLM: num_encoder_layers must be >= 1, got {num_encoder_layers}")
        if d_model % nhead != 0 or d_model // nhead not in HEAD_DIMS:
            raise NotImplementedError(f"TransformerLM: the head dimension d_model / nhead = {d_model}/{nhead} is not supported; the "
                                      f"attention kernels take {HEAD_DIMS}")
        self.vocab, self.d_model, self.nhead, self.num_encoder_layers = int(vocab), d_model, nhead, num_encoder_layers
        self.causal, self.attention_type, self.positional_encoding_type = True, attention_type, positional_encoding
        self.d_embedding, self.p_drop = d_model, float(dropout)
        self.compute_dtype = torch.float32                    # forward's default; make_state takes its own
        self.positional_encoding = PositionalEncoding(d_model, max_length)
        self.encoder = _LMEncoder(num_encoder_layers, nhead, d_ffn, d_model, dropout, activation, normalize_before)
        self.custom_src_module = NormalizedEmbedding(d_model, vocab)     # emb.Embedding.weight
        self.output_proj = _OutputProj(d_model, vocab)
        for p in self.parameters():                           # upstream's _reset_params
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)

    @property
    def max_length(self):
        return self.positional_encoding.max_len

    def _check_call(self, what):
        if self.training and self.p_drop > 0.0:
            raise NotImplementedError(f"TransformerLM.{what}: training mode with dropout={self.p_drop} is not built (inference only: "
                                      "call .eval())")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(f"TransformerLM.{what}: a call that needs gradients is not built (inference only: run under "
                                      "torch.no_grad() or freeze the parameters)")

    def _streams(self, compute):
        if compute not in (torch.float32, torch.bfloat16):
            raise TypeError(f"TransformerLM: float32 or bfloat16 only, got {compute}")
        return F.stream_dtype(compute) if self.encoder.layers[0].normalize_before else compute

    def _head(self, x, compute):
        """encoder.norm, then output_proj, on stream rows -> logits rows in the compute dtype."""
        n = self.encoder.norm.norm
        x = F.ln_fwd(x, n.weight, n.bias, n.eps, False, out_dtype=compute)[0]
        l0, l1, l2 = self.output_proj.layers
        x, _ = F.linear_fwd(x, F.wcast(l0.w.weight, compute), l0.w.bias.detach(), wparam=l0.w.weight)
        x = F.ln_fwd(x, l1.norm.weight, l1.norm.bias, l1.norm.eps, False)[0]
        return F.linear_fwd(x, F.wcast(l2.w.weight, compute), l2.w.bias.detach(), wparam=l2.w.weight)[0]

    def forward(self, src, hx=None, dtype=None):
        """src (B, U) integer tokens -> logits (B, U, vocab) in the compute dtype (dtype, default self.compute_dtype); position u sees
        positions <= u that are not pad_idx 0.  hx is upstream's unused argument."""
        self._check_call("forward")
        if src.dim() != 2 or src.is_floating_point():
            raise ValueError(f"TransformerLM: src must be (B, U) integer tokens, got {src.dtype} {tuple(src.shape)}")
        B, U = src.shape
        if U > self.max_length:
            raise ValueError(f"TransformerLM: sequence length {U} exceeds max_length {self.max_length}")
        if not src.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        compute = self.compute_dtype if dtype is None else dtype
        stream = self._streams(compute)
        with torch.no_grad():
            x, pad = self.custom_src_module.embed(src, self.positional_encoding.pe[0, :U], 0, stream)
            x = ops.rows2d(x)
            pad = F.key_pad_u8(pad, B, U, src.device)
            for layer in self.encoder.layers:
                x = layer._full(x, B, U, compute, pad)
            return self._head(x, compute).view(B, U, self.vocab)

    @torch.no_grad()
    def make_state(self, R, cap, dtype=torch.float32, device="cuda"):
        """The state of the cached step for R hypothesis rows of at most cap positions (bound: max_length) in the compute dtype."""
        if R < 1 or cap < 1 or cap > self.max_length:
            raise ValueError(f"TransformerLM.make_state: need R >= 1 and 1 <= cap <= max_length {self.max_length}, got R={R}, cap={cap}")
        return LMState(int(R), int(cap), self.nhead, self.d_model // self.nhead, len(self.encoder.layers), dtype, self._streams(dtype),
                       torch.device(device))

    def step(self, tokens, state, anc=None):
        """One cached step: tokens (R,) int32 on the device, the input at position state.pos -> logits (R, vocab) in the state's
        dtype: forward(prefix)[:, -1] for the prefix fed so far when it holds no pad_idx (module docstring), at the cost of ONE row
        per hypothesis.  anc (R, cap) int32: the ancestor table of a beam search (smx_attn_step_rows); None: row r reads its own
        cache row.  A row fed beyond cap positions is marked in state.done and yields zeros from its self-attention."""
        self._check_call("step")
        if not tokens.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        if tokens.dim() != 1 or tokens.is_floating_point() or tokens.shape[0] != state.R:
            raise ValueError(f"TransformerLM.step: tokens must be ({state.R},) integer tokens, got {tokens.dtype} {tuple(tokens.shape)}")
        tok = tokens if (tokens.dtype == torch.int32 and tokens.is_contiguous()) else tokens.to(torch.int32).contiguous()
        with torch.no_grad():
            x = ops.s2s_embed_step(tok, self.custom_src_module.emb.Embedding.weight.detach(), self.positional_encoding.pe[0], state.pos,
                                   state.done, state.cap, out_dtype=state.stream)
            for layer, skv in zip(self.encoder.layers, state.self_kv):
                x = layer._step(x, state.compute, skv, state.pos, state.attn_out, state.attn_ws, anc)
            return self._head(x, state.compute)

"""The lobes-level encoder API on MI355X: TransformerASR.encode / EncoderWrapper, mask builders, abs-sine PE.

Mirrors speechbrain/lobes/models/transformer/TransformerASR.py (:50-180 masks, :281-360 ctor, :501-560 encode,
:687-741 EncoderWrapper) and Transformer.py:284-335 (PositionalEncoding), :201-259 (encoder dispatch) for
attention_type="SummaryMixing" with encoder_module in {"conformer", "branchformer"}.  The vanilla-Transformer encoder (broken for
SummaryMixing in the reference) is out of scope.

Seq2seq side (:362-499, Transformer.py:262-277): with num_decoder_layers > 0 the constructor also builds `decoder` (always regularMHA,
causal) and `custom_tgt_module` (NormalizedEmbedding); forward(src, tgt, wav_len, pad_idx) -> (encoder_out, decoder_out) and
decode(tgt, encoder_out, enc_len) -> (prediction, last cross-attention weights).  The tokens become the decoder input in ONE launch
(smx_tgt_embed_fwd: embedding * sqrt(d) + positional rows + the key-padding mask); the look-ahead mask is the attention kernels'
causal flag.  Deviation: forward with wav_len=None runs the decoder without a memory padding mask (upstream crashes on
logical_not(None) there).  make_decode_state(encoder_out, enc_len, max_steps) / decode_step(tokens, state) are decode's KV-cached form:
one new position per call over per-layer caches whose positions are device counters (csrc/attn_step.hip; the seq2seq searchers of
summarymixing_amd.decoders.seq2seq run on them).

Streaming (:562-685,731-741): make_streaming_context / encode_streaming run a Dynamic-Chunk-trained Conformer encoder one chunk at a
time, from the encoder input on (the front-end is not streamed).  Chunk c gets rows [c C, c C + C_cur) of the positional table, as
the full forward does; a fixed (C, d) buffer holds them and is advanced on device after each chunk, so a chunk step has one shape
and no host-side state, and can be captured in a hipGraph (summarymixing_amd.streaming.CapturedStreamStep).

Slot streaming: make_slot_context / encode_slots run B independent streams, one per batch slot, in one step of B x C frames; each
slot starts, pauses and ends its stream on its own (valid / start per step).  Slot b's positional rows come from its own chunk
counter: smx_slot_begin writes them into a fixed (B*C, d) buffer at the start of the step, so the step can be captured as well
(summarymixing_amd.streaming.CapturedSlotStep).
"""
import math
from dataclasses import dataclass
from typing import Any, Optional

import torch
from torch import nn

from .... import functional as F
from .... import ops
from .... import sequence_parallel as SP
from ....nnet.activations import Swish
from ....utils.dynamic_chunk_training import DynChunkTrainConfig  # noqa: F401
from ...models.VanillaNN import Linear
from .Branchformer import BranchformerEncoder
from .Conformer import ConformerEncoder, _slot_commit
from .Transformer import (LOOKAHEAD, DecodeState, NormalizedEmbedding, TransformerDecoder, get_key_padding_mask,  # noqa: F401
                          get_lookahead_mask)
from ....nnet.attention import HEAD_DIMS


@dataclass
class TransformerASRStreamingContext:
    """Streaming state of a TransformerASR (reference :36-47): the configuration and the encoder's context, which also holds the
    positional-table buffer of the current chunk."""
    dynchunktrain_config: DynChunkTrainConfig
    encoder_context: Any


def length_to_mask(length, max_len=None):
    """arange(max_len)[None] < length[:, None]  (speechbrain.dataio.dataio.length_to_mask)."""
    if max_len is None:
        max_len = int(length.max().item())
    return torch.arange(max_len, device=length.device)[None, :] < length[:, None]


def make_transformer_src_mask(src, causal=False, masked_false_or_true=True, dynchunktrain_config=None):
    """TransformerASR.py:50-110.  Returns None or a functional.DynChunkMask (closed form of the (T,T) mask; call
    .dense() for the boolean matrix).  masked_false_or_true=True inverts the dense matrix like the reference."""
    if causal:
        raise NotImplementedError("causal masks make SummaryMixing non-finite in the reference (SURVEY §8a A5)")
    if dynchunktrain_config is None:
        return None
    m = F.DynChunkMask(src.size(1), dynchunktrain_config.chunk_size, dynchunktrain_config.left_context_size)
    if masked_false_or_true:
        return ~m.dense(src.device)
    return m


def make_transformer_src_tgt_masks(src, tgt=None, wav_len=None, pad_idx=0, causal=False, masked_false_or_true=True,
                                   dynchunktrain_config=None):
    """TransformerASR.py:113-180.  With `tgt` (B, U) tokens the two target masks are upstream's tensors: tgt.eq(pad_idx) and the dense
    (U, U) look-ahead mask (TransformerASR.forward itself builds neither: the embedding launch writes the first, the attention
    kernels' causal flag stands for the second)."""
    src_key_padding_mask = None
    if wav_len is not None:
        abs_len = torch.round(wav_len * src.shape[1])
        # the reference sizes the mask by abs_len.max() (a host sync) and only works when that equals T (the longest
        # utterance of a batch has wav_len == 1); max_len = T gives the same mask without the sync (hipGraph-capturable)
        valid = length_to_mask(abs_len, src.shape[1])
        src_key_padding_mask = ~valid if masked_false_or_true else valid
    src_mask = make_transformer_src_mask(src, causal, masked_false_or_true, dynchunktrain_config)
    if tgt is not None:
        return src_key_padding_mask, get_key_padding_mask(tgt, pad_idx=pad_idx), src_mask, get_lookahead_mask(tgt)
    return src_key_padding_mask, None, src_mask, None


class PositionalEncoding(nn.Module):
    """Absolute sinusoidal table (Transformer.py:306-335); ``forward`` returns pe[:, :T]."""

    def __init__(self, input_size, max_len=2500):
        super().__init__()
        if input_size % 2 != 0:
            raise ValueError(f"Cannot use sin/cos positional encoding with odd channels (got channels={input_size})")
        self.max_len = max_len
        pe = torch.zeros(max_len, input_size)
        pos = torch.arange(0, max_len).unsqueeze(1).float()
        den = torch.exp(torch.arange(0, input_size, 2).float() * -(math.log(10000.0) / input_size))
        pe[:, 0::2] = torch.sin(pos * den)
        pe[:, 1::2] = torch.cos(pos * den)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return self.pe[:, : x.size(1)].clone().detach()


class _SrcModule(nn.Module):
    """Key layout of the reference's custom_src_module: layers.0 = Linear holder (.w), layers.1 = Dropout."""

    def __init__(self, input_size, d_model, dropout):
        super().__init__()
        self.layers = nn.ModuleList([Linear(d_model, input_size), nn.Dropout(dropout)])


class _TgtModule(nn.Module):
    """Key layout of the reference's custom_tgt_module: layers.0 = NormalizedEmbedding (emb.Embedding.weight)."""

    def __init__(self, d_model, vocab):
        super().__init__()
        self.layers = nn.ModuleList([NormalizedEmbedding(d_model, vocab)])


class TransformerASR(nn.Module):
    def __init__(self, tgt_vocab, input_size, d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6,
                 d_ffn=2048, dropout=0.1, activation=nn.ReLU, positional_encoding="fixed_abs_sine",
                 normalize_before=False, kernel_size: Optional[int] = 31, bias: Optional[bool] = True,
                 encoder_module: Optional[str] = "transformer", conformer_activation=Swish,
                 branchformer_activation=nn.GELU, attention_type: Optional[str] = "SummaryMixing",
                 max_length: Optional[int] = 2500, causal: Optional[bool] = True,
                 csgu_linear_units: Optional[int] = 3072, gate_activation=nn.Identity,
                 use_linear_after_conv: Optional[bool] = False, local_proj_hid_dim: Optional[list] = [512],
                 local_proj_out_dim: Optional[int] = 512, summary_hid_dim: Optional[list] = [1024],
                 summary_out_dim: Optional[int] = 1024, mode: Optional[str] = "SummaryMixing",
                 masked_false_or_true: Optional[bool] = True):
        super().__init__()
        if attention_type != "SummaryMixing":
            raise NotImplementedError("summarymixing_amd implements attention_type='SummaryMixing' only")
        if causal:
            raise NotImplementedError("causal=True is unsupported with SummaryMixing (non-finite in the reference)")
        self.causal, self.attention_type = causal, attention_type
        self.positional_encoding_type = positional_encoding
        self.num_encoder_layers, self.num_decoder_layers = num_encoder_layers, num_decoder_layers
        self.masked_false_or_true = False                                    # TransformerASR.py:344-347
        self.p_drop = float(dropout)
        if positional_encoding == "fixed_abs_sine":
            self.positional_encoding = PositionalEncoding(d_model, max_length)
        elif positional_encoding is not None:
            raise NotImplementedError(f"positional_encoding={positional_encoding}")
        if encoder_module == "conformer":
            self.encoder = ConformerEncoder(nhead=nhead, num_layers=num_encoder_layers, d_ffn=d_ffn, d_model=d_model,
                                            dropout=dropout, activation=conformer_activation, kernel_size=kernel_size,
                                            bias=bias, causal=causal, attention_type=attention_type,
                                            local_proj_hid_dim=local_proj_hid_dim,
                                            local_proj_out_dim=local_proj_out_dim, summary_hid_dim=summary_hid_dim,
                                            mode=mode)
        elif encoder_module == "branchformer":
            self.encoder = BranchformerEncoder(nhead=nhead, num_layers=num_encoder_layers, d_model=d_model,
                                               dropout=dropout, activation=branchformer_activation,
                                               kernel_size=kernel_size, attention_type=attention_type,
                                               csgu_linear_units=csgu_linear_units, gate_activation=gate_activation,
                                               use_linear_after_conv=use_linear_after_conv,
                                               local_proj_hid_dim=local_proj_hid_dim,
                                               local_proj_out_dim=local_proj_out_dim, summary_hid_dim=summary_hid_dim,
                                               summary_out_dim=summary_out_dim, mode=mode)
        else:
            raise NotImplementedError("encoder_module='transformer' + SummaryMixing is broken in the reference "
                                      "(SURVEY §2 row 8); use 'conformer' or 'branchformer'")
        if num_decoder_layers > 0:                                            # Transformer.py:262-277: always regularMHA, causal
            if d_model % nhead != 0 or d_model // nhead not in HEAD_DIMS:
                raise NotImplementedError(f"TransformerASR: the decoder's head dimension d_model / nhead = {d_model}/{nhead} is not "
                                          f"supported; the attention kernels take {HEAD_DIMS}")
            self.decoder = TransformerDecoder(num_layers=num_decoder_layers, nhead=nhead, d_ffn=d_ffn, d_model=d_model,
                                              dropout=dropout, activation=activation, normalize_before=normalize_before,
                                              causal=True, attention_type="regularMHA")
        self.custom_src_module = _SrcModule(input_size, d_model, dropout)
        if num_decoder_layers > 0:
            self.custom_tgt_module = _TgtModule(d_model, tgt_vocab)           # TransformerASR.py:356-358
        for p in self.parameters():                                           # _init_params, :681-684
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)

    def forward(self, src, tgt=None, wav_len=None, pad_idx=0):
        """TransformerASR.py:362-451: -> (encoder_out, decoder_out (B, U, d)), or (encoder_out, None) without `tgt`.  src as in
        encode; tgt (B, U) integer tokens.  The encoder reads its padding mask as True = valid (masked_false_or_true is False for
        SummaryMixing, :344-347); the decoder gets it inverted as the memory key-padding mask (:437-438), or none with wav_len=None
        (upstream crashes there).  The attention weights are not computed on this path."""
        if tgt is not None:
            self._check_tgt(tgt)
        encoder_out = self.encode(src, wav_len, pad_idx, masked_false_or_true=self.masked_false_or_true)
        if tgt is None:
            return encoder_out, None
        mem_pad = None
        if wav_len is not None:
            S = encoder_out.shape[1]
            mem_pad = ~length_to_mask(torch.round(wav_len * S), S)
        return encoder_out, self._decoder_side(tgt, encoder_out, mem_pad, pad_idx)

    def _decoder_side(self, tgt, encoder_out, mem_pad, pad_idx=0):
        """forward() from the tokens and the encoder output on (:425-450); what tools/decoder_bench.py times."""
        x, tgt_pad = self._embed_tgt(tgt, pad_idx, F.stream_dtype(encoder_out.dtype) if self.decoder.layers[0].normalize_before
                                     else encoder_out.dtype)
        decoder_out, _, _ = self.decoder(tgt=x, memory=encoder_out, memory_mask=None, tgt_mask=LOOKAHEAD,
                                         tgt_key_padding_mask=tgt_pad, memory_key_padding_mask=mem_pad, _weights="none")
        return decoder_out

    def _check_tgt(self, tgt):
        """Host-side refusals, before any launch."""
        if self.num_decoder_layers <= 0:
            raise RuntimeError("TransformerASR was built with num_decoder_layers=0: there is no decoder to run `tgt` through")
        if tgt.dim() != 2 or tgt.is_floating_point():
            raise ValueError(f"tgt must be (B, U) integer tokens, got {tgt.dtype} {tuple(tgt.shape)}")
        if self.positional_encoding_type == "fixed_abs_sine" and tgt.shape[1] > self.positional_encoding.max_len:
            raise ValueError(f"target length {tgt.shape[1]} exceeds max_length {self.positional_encoding.max_len}")
        if not tgt.is_cuda:
            raise RuntimeError(ops.NO_CPU)

    def _embed_tgt(self, tgt, pad_idx, out_dtype):
        """custom_tgt_module + positional_encoding + get_key_padding_mask (:425-430, :172) in one launch."""
        emb = self.custom_tgt_module.layers[0]
        U = tgt.shape[1]
        if self.positional_encoding_type == "fixed_abs_sine":
            pe = self.positional_encoding.pe[0, :U]
        else:
            pe = torch.zeros((U, emb.d_model), device=tgt.device)
        return emb.embed(tgt, pe, pad_idx, out_dtype)

    @torch.no_grad()
    def decode(self, tgt, encoder_out, enc_len=None):
        """TransformerASR.py:453-499: one decoding step over the whole prefix tgt (B, U) -> (prediction (B, U, d), the last layer's
        cross-attention weights (B, U, S)).  enc_len: the absolute encoder lengths (B).  No key-padding mask on the targets, as
        upstream; no KV cache."""
        self._check_tgt(tgt)
        if not encoder_out.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        mem_pad = None
        if enc_len is not None:
            mem_pad = ~length_to_mask(enc_len.to(encoder_out.device), encoder_out.shape[1])
        x, _ = self._embed_tgt(tgt, 0, F.stream_dtype(encoder_out.dtype) if self.decoder.layers[0].normalize_before
                               else encoder_out.dtype)
        prediction, _, multihead_attns = self.decoder(x, encoder_out, tgt_mask=LOOKAHEAD, memory_key_padding_mask=mem_pad,
                                                      _weights="last_cross")
        return prediction, multihead_attns[-1]

    @torch.no_grad()
    def make_decode_state(self, encoder_out, enc_len=None, max_steps=None, state=None, beam=None):
        """The state of KV-cached decoding over encoder_out (B, S, d) (Transformer.DecodeState): per decoder layer an empty
        self-attention cache of cap = max_steps positions (default and bound: the positional table's max_length) and the layer's
        cross-attention keys / values, computed HERE, once, by the d -> 2d Linear on rows [d, 3d) of multihead_attn's in_proj_weight
        (functional.attention_in_proj, the projection decode runs again for every prefix).  enc_len: the absolute encoder lengths (B),
        as decode takes them; None: all S.  state: a state of the same (B, S, cap, dtype) to refill in place for the next utterance -
        its buffers stay where a captured step expects them.  beam=W: the state of a beam search of W hypotheses per utterance
        (Transformer.DecodeState): self-attention caches of B W rows read through an ancestor table, the cross-attention keys /
        values still projected once per utterance; beam=None is the state it always was.  Nothing synchronises with the host."""
        if beam is not None and not 1 <= int(beam) <= 128:
            raise ValueError(f"make_decode_state: beam must be in [1, 128], got {beam}")
        if self.num_decoder_layers <= 0:
            raise RuntimeError("TransformerASR was built with num_decoder_layers=0: there is no decoder to make a decoding state for")
        if self.training:
            raise RuntimeError("TransformerASR.make_decode_state: decoding runs in eval mode only (self.training is set)")
        if not encoder_out.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        if encoder_out.dim() != 3 or encoder_out.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"encoder_out must be (B, S, d) float32 or bfloat16, got {encoder_out.dtype} {tuple(encoder_out.shape)}")
        B, S, d = encoder_out.shape
        limit = self.positional_encoding.max_len if self.positional_encoding_type == "fixed_abs_sine" else None
        if max_steps is None and limit is None:
            raise ValueError("make_decode_state: max_steps is needed without a positional table to bound it")
        cap = limit if max_steps is None else (int(max_steps) if limit is None else min(int(max_steps), limit))
        if cap < 1:
            raise ValueError(f"make_decode_state: max_steps must be >= 1, got {max_steps}")
        layers = self.decoder.layers
        H = layers[0].nhead
        compute = encoder_out.dtype
        stream = F.stream_dtype(compute) if layers[0].normalize_before else compute
        if state is None:
            state = (DecodeState(B, S, cap, H, d // H, len(layers), compute, stream, encoder_out.device) if beam is None else
                     DecodeState(B, S, cap, H, d // H, len(layers), compute, stream, encoder_out.device, beam=int(beam)))
        elif (state.B, state.S, state.cap, state.compute) != (B, S, cap, compute) or state.pos.device != encoder_out.device:
            raise ValueError(f"make_decode_state: the state holds (B, S, cap, dtype) = {(state.B, state.S, state.cap, state.compute)}, "
                             f"this call needs {(B, S, cap, compute)}")
        elif state.beam != beam:
            raise ValueError(f"make_decode_state: the state holds beam = {state.beam}, this call needs {beam}")
        else:
            state.reset()
        mem2 = ops.rows2d(encoder_out if encoder_out.is_contiguous() else encoder_out.contiguous())
        for layer, ckv in zip(layers, state.cross_kv):
            F.attention_in_proj(layer.multihead_attn.att, mem2, 1, 3, out=ckv.view(B * S, 2 * d))
        if enc_len is None:
            state.mem_len.fill_(S)
        else:
            state.mem_len.copy_(enc_len.reshape(B))           # (cast to int32 on the device; a length outside [1, S] gives a zero row)
        return state

    @torch.no_grad()
    def decode_step(self, tokens, state):
        """One KV-cached decoding step: tokens (B,) integer on the device, the input at position state.pos -> prediction (B, d), what
        decode(prefix, encoder_out, enc_len)[0][:, -1] computes for the prefix fed so far, at the cost of ONE row per utterance:
        smx_s2s_embed_step (embedding * sqrt(d) + the positional row of the DEVICE counter state.pos, which it advances), then per
        layer the sublayers of decode with smx_attn_step over the state's caches in place of smx_attn_fwd, then the final LayerNorm.
        No attention weights.  A row fed beyond the state's cap positions is marked done (state.done) and yields zeros from its
        self-attention; the host is never asked.  Eval mode only.  Over a beam state (make_decode_state(beam=W)) tokens and the
        prediction have B W rows, the self-attention reads its keys through the state's ancestor table and the W rows of an utterance
        share its projected memory (smx_attn_step_rows)."""
        if self.training:
            raise RuntimeError("TransformerASR.decode_step: decoding runs in eval mode only (self.training is set)")
        if not tokens.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        if tokens.dim() != 1 or tokens.is_floating_point() or tokens.shape[0] != state.rows:
            raise ValueError(f"tokens must be ({state.rows},) integer tokens, got {tokens.dtype} {tuple(tokens.shape)}")
        tok = tokens if (tokens.dtype == torch.int32 and tokens.is_contiguous()) else tokens.to(torch.int32).contiguous()
        emb = self.custom_tgt_module.layers[0]
        pe = self.positional_encoding.pe[0] if self.positional_encoding_type == "fixed_abs_sine" else None
        x = ops.s2s_embed_step(tok, emb.emb.Embedding.weight.detach(), pe, state.pos, state.row_done, state.cap, out_dtype=state.stream)
        return self.decoder.step(x, state)

    def encode(self, src, wav_len=None, pad_idx=0, dynchunktrain_config=None, masked_false_or_true: Optional[bool] = True):
        """TransformerASR.py:501-560.  masked_false_or_true is honoured exactly like the reference: the SummaryMixing cell
        and conv module read the padding mask as True = VALID (masked_false_or_true=False, what EncoderWrapper and the
        reference's own forward() pass, :344-347,:720-729); a direct call with the signature's default True hands them the
        inverted mask - in the reference too."""
        if SP.enabled():
            raise NotImplementedError("sequence-parallel mode enters at the ConformerEncoder stack: the positional table, "
                                      "the wav_len masks and the input dropout counters here are not offset per shard")
        if src.dim() == 4:
            bz, t, ch1, ch2 = src.shape
            src = src.reshape(bz, t, ch1 * ch2)
        B, T, _ = src.shape
        key_padding_mask, _, src_mask, _ = make_transformer_src_tgt_masks(
            src, None, wav_len, pad_idx=pad_idx, causal=self.causal, dynchunktrain_config=dynchunktrain_config,
            masked_false_or_true=masked_false_or_true)
        lin = self.custom_src_module.layers[0].w
        if self.positional_encoding_type == "fixed_abs_sine":
            if T > self.positional_encoding.max_len:
                raise ValueError(f"sequence length {T} exceeds max_length {self.positional_encoding.max_len}")
            pe = self.positional_encoding.pe[0, :T]
        else:
            pe = torch.zeros((T, lin.weight.shape[0]), device=src.device)
        x = F.input_proj_pe(src, lin.weight, lin.bias, pe, T, self.p_drop if self.training else 0.0)
        # (x is the residual stream: float32 for a bf16 model by default - the encoder is told the GEMM dtype)
        kw = {"_compute_dtype": src.dtype}
        out, _ = self.encoder(src=x, src_mask=src_mask, src_key_padding_mask=key_padding_mask, pos_embs=None,
                              dynchunktrain_config=dynchunktrain_config, **kw)
        return out


    def make_streaming_context(self, dynchunktrain_config: DynChunkTrainConfig, encoder_kwargs={}):
        """A blank streaming context (reference :562-590).  Refused (NotImplementedError): the Branchformer, the SummaryMixing-lite
        and -expdecay modes (their Dynamic Chunk Training forward is not causal) and sequence-parallel mode."""
        if not isinstance(self.encoder, ConformerEncoder):
            raise NotImplementedError("streaming inference runs the Conformer encoder only (the Branchformer refuses Dynamic "
                                      "Chunk Training)")
        enc = self.encoder.make_streaming_context(dynchunktrain_config, **encoder_kwargs)
        return TransformerASRStreamingContext(dynchunktrain_config=dynchunktrain_config, encoder_context=enc)

    def encode_streaming(self, src, context: TransformerASRStreamingContext):
        """Encode one chunk (B, C_cur, F) (or (B, C_cur, ch1, ch2), reshaped as in encode) of B equal-length streams (reference
        :592-685).  The chunks of an utterance, fed in order with one context, give encode(src, wav_len=1,
        dynchunktrain_config=cfg) of the whole utterance; a chunk shorter than chunk_size ends the stream.  Running past
        max_length raises ValueError."""
        if src.dim() == 4:
            bz, t, ch1, ch2 = src.shape
            src = src.reshape(bz, t, ch1 * ch2)
        ec = self._stream_begin(src, context)
        with torch.no_grad():
            out = self._stream_chunk(src, ec)
        ec.frames += src.shape[1]
        ec.closed = src.shape[1] < ec.dynchunktrain_config.chunk_size
        return out

    def _stream_begin(self, src, context):
        """Validate the chunk (host only) and allocate the state on the first one; -> the encoder context."""
        ec = context.encoder_context
        B, C_cur, _ = src.shape
        if self.positional_encoding_type == "fixed_abs_sine" and ec.frames + C_cur > self.positional_encoding.max_len:
            raise ValueError(f"streaming: frame {ec.frames + C_cur} exceeds max_length {self.positional_encoding.max_len}")
        first = ec.batch_size is None
        self.encoder._stream_begin(ec, B, C_cur, src.dtype, src.device)
        if first:
            self._pe_alloc(ec, ec.dynchunktrain_config.chunk_size, src.device)
            if ec.pe_table is not None:
                n = min(ec.pe.shape[0], ec.pe_table.shape[0])
                ec.pe[:n] = ec.pe_table[:n]            # chunk 0's rows; smx_stream_advance writes the later ones
        return ec

    def _pe_alloc(self, ec, rows, device):
        """ec.pe = the (rows, d) positional rows of a step, zero; with the fixed sine table, ec.pe_table = it and pe has its dtype."""
        if self.positional_encoding_type == "fixed_abs_sine":
            ec.pe_table = self.positional_encoding.pe[0]
        ec.pe = torch.zeros((rows, self.custom_src_module.layers[0].w.weight.shape[0]), device=device,
                            dtype=ec.pe_table.dtype if ec.pe_table is not None else None)

    def _stream_chunk(self, src, ec):
        """The launches of one chunk step: input projection + the chunk's PE rows, the encoder, the counter / PE advance."""
        C_cur = src.shape[1]
        lin = self.custom_src_module.layers[0].w
        x = F.input_proj_pe(src, lin.weight, lin.bias, ec.pe[:C_cur], C_cur, 0.0)
        return self.encoder._stream_chunk(x, ec, src.dtype)


    def make_slot_context(self, dynchunktrain_config: DynChunkTrainConfig, slots: int):
        """A blank slot-streaming context for `slots` independent streams (encode_slots).  Refuses what make_streaming_context
        refuses."""
        if not isinstance(self.encoder, ConformerEncoder):
            raise NotImplementedError("streaming inference runs the Conformer encoder only (the Branchformer refuses Dynamic "
                                      "Chunk Training)")
        enc = self.encoder.make_slot_context(dynchunktrain_config, slots)
        return TransformerASRStreamingContext(dynchunktrain_config=dynchunktrain_config, encoder_context=enc)

    def encode_slots(self, src, valid, start, context: TransformerASRStreamingContext):
        """Encode one step (B, C, F) (or (B, C, ch1, ch2)) of B independent streams, one per slot of the context.  valid (B host
        ints, 0 .. C): slot b's frames in this step - C a full chunk, 1 .. C-1 its stream's last chunk, 0 the slot sits out and its
        state stays as it was.  start (B host bools): slot b begins a new stream at this step.  For every stream, the rows
        [:valid[b]] of its steps concatenate to encode_streaming of that stream alone; rows at and beyond valid[b] are unspecified,
        and the input rows there are never read (they may hold anything).  ValueError, before any launch: feeding a slot with no
        open stream without start, valid outside 0 .. C, a stream running past max_length, another B, dtype or device."""
        if src.dim() == 4:
            bz, t, ch1, ch2 = src.shape
            src = src.reshape(bz, t, ch1 * ch2)
        ec, args = self._slot_begin(src, valid, start, context)
        self.encoder._slot_stage(ec, args[0], args[1])
        with torch.no_grad():
            out = self._slot_chunk(src, ec)
        _slot_commit(ec, *args)
        return out

    def _slot_begin(self, src, valid, start, context):
        """Validate the step (host only) and allocate the state on the first one; -> (encoder context, args for _slot_commit)."""
        ec = context.encoder_context
        args = self.encoder._slot_begin(ec, tuple(src.shape), src.dtype, src.device, valid, start)
        if self.positional_encoding_type == "fixed_abs_sine":
            for b, (v, f) in enumerate(zip(args[0], args[2])):
                if f + v > self.positional_encoding.max_len:
                    raise ValueError(f"slot streaming: slot {b} reaches frame {f + v}, beyond max_length "
                                     f"{self.positional_encoding.max_len}")
        if ec.pe is None:
            self._pe_alloc(ec, ec.slots * ec.dynchunktrain_config.chunk_size, src.device)
        return ec, args

    def _slot_chunk(self, src, ec):
        """The launches of one slot step: counters reset / positional rows (smx_slot_begin), input projection + those rows (the
        (B*C, d) block indexed row by row), the encoder, the counter advance."""
        B, C, _ = src.shape
        lin = self.custom_src_module.layers[0].w
        ops.slot_begin(ec.counters, ec.start, ec.pe_table, ec.pe if ec.pe_table is not None else None, B, C, ec.pe.shape[1])
        x = F.input_proj_pe(src.reshape(1, B * C, -1), lin.weight, lin.bias, ec.pe, B * C, 0.0)
        return self.encoder._slot_layers(x.view(B, C, -1), ec, src.dtype)


class EncoderWrapper(nn.Module):
    """forward() = transformer.encode() (TransformerASR.py:715-729)."""

    def __init__(self, transformer, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.transformer = transformer

    def forward(self, x, wav_lens=None, pad_idx=0, **kwargs):
        return self.transformer.encode(x, wav_lens, pad_idx, **kwargs,
                                       masked_false_or_true=self.transformer.masked_false_or_true)

    def forward_streaming(self, x, context):
        """transformer.encode_streaming (reference :731-736)."""
        return self.transformer.encode_streaming(x, context)

    def make_streaming_context(self, *args, **kwargs):
        """transformer.make_streaming_context (reference :738-741)."""
        return self.transformer.make_streaming_context(*args, **kwargs)

    def forward_slots(self, x, valid, start, context):
        """transformer.encode_slots."""
        return self.transformer.encode_slots(x, valid, start, context)

    def make_slot_context(self, *args, **kwargs):
        """transformer.make_slot_context."""
        return self.transformer.make_slot_context(*args, **kwargs)

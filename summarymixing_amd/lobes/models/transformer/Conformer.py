"""Conformer encoder with the SummaryMixing cell on MI355X.

Mirrors the constructor / forward signatures and state-dict keys of the reference
(speechbrain/lobes/models/transformer/Conformer.py: ConvolutionModule :72-331, ConformerEncoderLayer :334-537,
ConformerEncoder :623-786) for attention_type="SummaryMixing".  The torch.nn sub-modules below are parameter
HOLDERS only (same names => same keys => reference checkpoints load); all arithmetic runs in libsmx.so:

  layer(x):  x1 = x  + 1/2 FFN1(x)              LN -> GEMM(+bias,act) -> GEMM(+bias, residual, alpha=1/2)
             x2 = x1 + SummaryMixing(LN(x1))    cell with the skip fused as the merge-GEMM residual
             x3 = x2 + mask * ConvModule(x2)    LN -> GEMM -> fused GLU+dwconv -> LN+act -> GEMM(+mask,residual)
             y  = LN(x3 + 1/2 FFN2(x3))
Attention types other than SummaryMixing and causal convolution are out of scope and raise
NotImplementedError.

Streaming inference (forward_streaming / make_streaming_context, reference :539-633,788-857) runs a Dynamic-Chunk-trained
encoder one chunk at a time and equals the masked full-utterance forward.  Unlike the reference, which keeps raw input frames as
left context and recomputes them on every chunk (its own TODO), a layer here carries only what the next chunk reads: the float32
per-chunk sums of the summary branch and the last (k-1)/2 pre-GLU rows of the convolution (functional.DynChunkStream, ops.dwconv_stream).

Slot streaming (forward_slots / make_slot_context) runs B independent streams, one per batch slot, in one fixed step of B x C
frames: each slot has its own device chunk counter, its own frame count in the step (valid) and starts a new stream when told to
(start).  Counter 0 means fresh state, so starting a slot clears no buffer (functional.DynChunkSlots, ops.dwconv_slots).
"""
from dataclasses import dataclass, field
from typing import Any, List, Optional

import numpy as np
import torch
import torch.nn as nn

from .... import functional as F
from .... import ops
from .... import sequence_parallel as SP
from ....utils.dynamic_chunk_training import DynChunkTrainConfig
from ....nnet.activations import Swish, act_code
from ....nnet.summary_mixing import SummaryMixing


@dataclass
class ConformerEncoderLayerStreamingContext:
    """Streaming state of one ConformerEncoderLayer (reference :31-59).  The reference keeps `mha_left_context` (the last raw input
    frames, recomputed on every chunk) and `dcconv_left_context`; this layer keeps instead:
      summary   - functional.DynChunkStream: the float32 sums of the summary branch over the last `left_context_size` chunks
                  ((B, left, s); one (B, s) running sum for unlimited left context; none for left 0) and the device chunk counter;
      dcconv_state - (B, (k-1)/2, 2 d) in the compute dtype: the last pre-GLU rows of the pointwise convolution (zeros at the start,
                  the full forward's zero padding).
    Both are allocated on the first chunk, which fixes the batch size, dtype and device."""
    dynchunktrain_config: DynChunkTrainConfig
    summary: Optional[F.DynChunkStream] = None
    dcconv_state: Optional[torch.Tensor] = None
    counter: Optional[torch.Tensor] = None          # device chunk counter (int64 (1,)), shared with the encoder's context
    batch_size: Optional[int] = None
    dtype: Optional[torch.dtype] = None
    device: Optional[torch.device] = None
    frames: int = 0                                 # host mirror of the frames consumed (never read back from the device)
    closed: bool = False                            # a chunk shorter than chunk_size ended the stream


@dataclass
class ConformerEncoderStreamingContext:
    """Streaming state of a ConformerEncoder (reference :62-70): the configuration, one context per layer and the state shared by
    the layers (device chunk counter, host frame mirror).  pe_table / pe: set by TransformerASR on the first chunk - the
    positional table and the fixed (C, d) buffer holding the current chunk's rows of it, advanced on device after every chunk."""
    dynchunktrain_config: DynChunkTrainConfig
    layers: List[ConformerEncoderLayerStreamingContext] = field(default_factory=list)
    counter: Optional[torch.Tensor] = None
    batch_size: Optional[int] = None
    dtype: Optional[torch.dtype] = None
    device: Optional[torch.device] = None
    frames: int = 0
    closed: bool = False
    pe_table: Optional[torch.Tensor] = None
    pe: Optional[torch.Tensor] = None


def _stream_check(ctx, training, B, C_cur, dtype, device):
    """Validate one chunk against the context (host only: no device read).  -> True when the state is still to be allocated."""
    if training:
        raise RuntimeError("streaming inference: call .eval() first (forward_streaming runs no backward)")
    C = ctx.dynchunktrain_config.chunk_size
    if ctx.closed:
        raise ValueError("streaming: a chunk shorter than chunk_size ended this stream; make a new context")
    if not 1 <= C_cur <= C:
        raise ValueError(f"streaming: a chunk holds 1 .. {C} frames, got {C_cur}")
    if ctx.batch_size is None:
        return True
    if (B, dtype, torch.device(device)) != (ctx.batch_size, ctx.dtype, ctx.device):
        raise ValueError(f"streaming: the context was started with B={ctx.batch_size}, {ctx.dtype} on {ctx.device}; got B={B}, "
                         f"{dtype} on {device}")
    return False


def _stream_commit(ctx, C_cur):
    ctx.frames += C_cur
    ctx.closed = C_cur < ctx.dynchunktrain_config.chunk_size


@dataclass
class ConformerEncoderLayerSlotContext:
    """Slot-streaming state of one ConformerEncoderLayer: the ConformerEncoderLayerStreamingContext buffers with one row per slot.
      summary      - functional.DynChunkSlots: (B, left, s) / (B, s) float32 ring and the encoder's per-slot counters and valid;
      dcconv_state - (B, (k-1)/2, 2 d) in the compute dtype.
    Neither is ever cleared: a slot's counter 0 makes the kernels read its state as zero."""
    dynchunktrain_config: DynChunkTrainConfig
    summary: Optional[F.DynChunkSlots] = None
    dcconv_state: Optional[torch.Tensor] = None


@dataclass
class ConformerEncoderSlotContext:
    """Slot-streaming state of a ConformerEncoder: `slots` independent streams in one step of slots x chunk_size frames.
    Device: `counters` (B,) int64 per-slot chunk index shared by the layers; `valid` (B,) int32 and `start` (B,) uint8, the step's
    arguments, copied from the host in stream order before the step's launches (views of one byte buffer `io`).
    Host mirrors (never read back from the device): `frames` the frames each slot's stream has consumed, `open` whether it can
    take another chunk (started, and not ended by a short chunk).  pe_table / pe: set by TransformerASR - the positional table and
    the fixed (B*C, d) buffer of each slot's current rows, written by smx_slot_begin at the start of every step."""
    dynchunktrain_config: DynChunkTrainConfig
    slots: int
    layers: List[ConformerEncoderLayerSlotContext] = field(default_factory=list)
    counters: Optional[torch.Tensor] = None
    io: Optional[torch.Tensor] = None
    valid: Optional[torch.Tensor] = None
    start: Optional[torch.Tensor] = None
    dtype: Optional[torch.dtype] = None
    device: Optional[torch.device] = None
    frames: List[int] = field(default_factory=list)
    open: List[bool] = field(default_factory=list)
    pe_table: Optional[torch.Tensor] = None
    pe: Optional[torch.Tensor] = None
    staging: Any = None


class _SlotStaging:
    """Pinned host buffers for the step arguments: a ring of them, each reused only after the copy that last read it has run
    (its event), so a step never waits for the device and never races an earlier step's copy."""

    def __init__(self, B, n=4):
        self.host = [torch.empty(5 * B, dtype=torch.uint8, pin_memory=True) for _ in range(n)]
        self.events = [None] * n
        self.i, self.B = 0, B

    def copy(self, io, valid, start):
        i, B = self.i, self.B
        self.i = (i + 1) % len(self.host)
        if self.events[i] is not None:
            self.events[i].synchronize()
        h = self.host[i].numpy()
        h[:4 * B].view(np.int32)[:] = valid
        h[4 * B:] = start
        io.copy_(self.host[i], non_blocking=True)
        ev = self.events[i] = self.events[i] or torch.cuda.Event()
        ev.record()


def _slot_args(ctx, training, src_shape, dtype, device, valid, start):
    """Validate one slot step against the context (host only: no device read).  -> (valid, start) as lists of ints and the
    frames each slot's stream holds before the step (0 for a started slot)."""
    if training:
        raise RuntimeError("slot streaming: call .eval() first (forward_slots runs no backward)")
    C, B = ctx.dynchunktrain_config.chunk_size, ctx.slots
    if len(src_shape) != 3 or src_shape[0] != B or src_shape[1] != C:
        raise ValueError(f"slot streaming: expected a ({B}, {C}, F) step for {B} slots of chunk_size {C}, got {tuple(src_shape)}")
    valid, start = [int(v) for v in valid], [bool(s) for s in start]
    if len(valid) != B or len(start) != B:
        raise ValueError(f"slot streaming: valid and start need {B} entries, got {len(valid)} and {len(start)}")
    if ctx.dtype is not None and (dtype, torch.device(device)) != (ctx.dtype, ctx.device):
        raise ValueError(f"slot streaming: the context was started with {ctx.dtype} on {ctx.device}; got {dtype} on {device}")
    base = []
    for b, (v, s) in enumerate(zip(valid, start)):
        if not 0 <= v <= C:
            raise ValueError(f"slot streaming: valid[{b}] = {v} is outside 0 .. {C}")
        if v > 0 and not s and not (ctx.open and ctx.open[b]):
            raise ValueError(f"slot streaming: slot {b} holds no open stream (never started, or ended by a short chunk); "
                             "set start for it")
        base.append(0 if s else (ctx.frames[b] if ctx.frames else 0))
    return valid, start, base


def _slot_commit(ctx, valid, start, base):
    C = ctx.dynchunktrain_config.chunk_size
    for b, (v, s) in enumerate(zip(valid, start)):
        ctx.frames[b] = base[b] + v
        if s:
            ctx.open[b] = True
        if 0 < v < C:
            ctx.open[b] = False


def _stream_refuse(layer, cfg):
    if layer.mode not in ("SummaryMixing", "SummaryMixing-fast"):
        raise NotImplementedError(f"streaming: mode {layer.mode} is not causal under Dynamic Chunk Training (SummaryMixing-lite "
                                  "ignores the chunk mask; expdecay weighs every frame) - use SummaryMixing or SummaryMixing-fast")
    if SP.enabled():
        raise NotImplementedError("streaming inference does not run in sequence-parallel mode")
    if cfg is None or cfg.chunk_size < 1 or cfg.chunk_size > 64:
        raise ValueError("streaming needs a DynChunkTrainConfig with 1 <= chunk_size <= 64")
    if cfg.left_context_size is not None and not 0 <= cfg.left_context_size <= 32:
        raise ValueError("streaming: left_context_size must be None or 0 .. 32 chunks")


class _LayerNorm(nn.Module):
    """Key layout of speechbrain.nnet.normalization.LayerNorm (``.norm`` is an nn.LayerNorm)."""

    def __init__(self, d, eps=1e-5):
        super().__init__()
        self.norm = nn.LayerNorm(d, eps=eps)


class _FFN(nn.Module):
    """Key layout of PositionalwiseFeedForward: ``ffn.0`` Linear(d,f), ``ffn.3`` Linear(f,d)."""

    def __init__(self, d_ffn, input_size, dropout, activation):
        super().__init__()
        self.ffn = nn.Sequential(nn.Linear(input_size, d_ffn), nn.Identity(), nn.Dropout(dropout),
                                 nn.Linear(d_ffn, input_size))


def _ffn_params(seq):
    return {"ln_w": seq[0].weight, "ln_b": seq[0].bias, "W1": seq[1].ffn[0].weight, "b1": seq[1].ffn[0].bias,
            "W2": seq[1].ffn[3].weight, "b2": seq[1].ffn[3].bias}


class ConvolutionModule(nn.Module):
    def __init__(self, input_size, kernel_size=31, bias=True, activation=Swish, dropout=0.0, causal=False,
                 dilation=1, masked_false_or_true=True):
        super().__init__()
        if causal or dilation != 1:
            raise NotImplementedError("causal / dilated convolution is outside the SummaryMixing hot path")
        self.kernel_size, self.causal, self.dilation = kernel_size, causal, dilation
        self.masked_false_or_true = masked_false_or_true
        self.padding = (kernel_size - 1) // 2
        self.act = act_code(activation)
        self.p_drop = float(dropout)
        self.layer_norm = nn.LayerNorm(input_size)
        self.bottleneck = nn.Sequential(nn.Conv1d(input_size, 2 * input_size, kernel_size=1, bias=bias), nn.Identity())
        self.conv = nn.Conv1d(input_size, input_size, kernel_size, padding=self.padding, groups=input_size, bias=bias)
        self.after_conv = nn.Sequential(nn.LayerNorm(input_size), nn.Identity(), nn.Linear(input_size, input_size, bias=bias),
                                        nn.Dropout(dropout))

    def params(self):
        return {"ln1_w": self.layer_norm.weight, "ln1_b": self.layer_norm.bias, "Wp": self.bottleneck[0].weight,
                "bp": self.bottleneck[0].bias, "wd": self.conv.weight, "bd": self.conv.bias,
                "ln2_w": self.after_conv[0].weight, "ln2_b": self.after_conv[0].bias, "Wo": self.after_conv[2].weight,
                "bo": self.after_conv[2].bias}

    def forward(self, x, mask: Optional[torch.Tensor] = None, dynchunktrain_config=None):
        """Returns conv_module(x) (without the residual), mask (B,T,1) multiplies the output when
        masked_false_or_true is False (the SummaryMixing convention, Conformer.py:327-331)."""
        B, T, d = x.shape
        if mask is not None and self.masked_false_or_true:
            mask = ~mask.bool()
        m8 = F.mask_u8(mask.reshape(B, T) if mask is not None else None, B, T, x.device)
        P, act = self.params(), self.act
        chunk = dynchunktrain_config.chunk_size if dynchunktrain_config is not None else 0
        pd = self.p_drop if self.training else 0.0

        def run(xin, need_bwd):
            x2 = ops.rows2d(xin)
            y, bwd = F.conv_module_fwd(x2, P, act, m8, B, T, need_bwd, xin.dtype, chunk, residual=False, p=pd)
            return y.view(B, T, d), ((lambda dy: bwd(ops.rows2d(dy.contiguous())).view(B, T, d)) if need_bwd else None)
        return F.block(x, run, list(self.parameters()))


class ConformerEncoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, nhead, kernel_size=31, kdim=None, vdim=None, activation=Swish, bias=True,
                 dropout=0.0, causal=False, attention_type="RelPosMHAXL", local_proj_hid_dim=[512],
                 local_proj_out_dim=512, summary_hid_dim=[1024], mode="SummaryMixing"):
        super().__init__()
        if attention_type != "SummaryMixing":
            raise NotImplementedError("summarymixing_amd implements attention_type='SummaryMixing' only")
        self.attention_type, self.mode = attention_type, mode
        self.masked_false_or_true = False                     # Conformer.py:447
        self.act = act_code(activation)
        self.p_drop = float(dropout)
        self.mha_layer = SummaryMixing(enc_dim=d_model, nhead=nhead, local_proj_hid_dim=local_proj_hid_dim,
                                       local_proj_out_dim=local_proj_out_dim, summary_hid_dim=summary_hid_dim,
                                       summary_out_dim=d_model, activation=activation, global_dropout=dropout, mode=mode)
        self.convolution_module = ConvolutionModule(d_model, kernel_size, bias, activation, dropout, causal=causal,
                                                    masked_false_or_true=False)
        self.ffn_module1 = nn.Sequential(nn.LayerNorm(d_model), _FFN(d_ffn, d_model, dropout, activation), nn.Dropout(dropout))
        self.ffn_module2 = nn.Sequential(nn.LayerNorm(d_model), _FFN(d_ffn, d_model, dropout, activation), nn.Dropout(dropout))
        self.norm1 = _LayerNorm(d_model)
        self.norm2 = _LayerNorm(d_model)
        self.drop = nn.Dropout(dropout)

    def make_run(self, B, T, m8, src_mask, chunk, compute_dtype=None, next_layer=None, conv_state=None):
        """compute_dtype: dtype of the GEMM operands when the incoming stream x3 is the float32 residual stream of a bf16
        model (functional.RESIDUAL_F32); None = everything in x3.dtype.
        next_layer: the layer that consumes this one's output inside an encoder stack.  Its first LayerNorm (ffn_module1's) then
        runs in the same pass as this layer's norm2 where the shapes allow (ops.layernorm_fwd_pair: one read of the float32 stream
        for both); run(..., with_post=True) then returns a third value, (LN(y), stats) | None, which the stack hands to the next
        layer's run as `pre_ln`.
        Streaming inference (forward_streaming): src_mask is a functional.DynChunkStream and conv_state a functional.ConvStream over
        the layer's convolution state; T is then the frames of one chunk.  Slot streaming (forward_slots): src_mask is a
        functional.DynChunkSlots, conv_state carries the slots' valid / counters as well; B is the slot count and T the chunk size."""
        d_act = self.act
        P1, P2 = _ffn_params(self.ffn_module1), _ffn_params(self.ffn_module2)
        Pc = self.convolution_module.params()
        n1, n2 = self.norm1.norm, self.norm2.norm
        pd = self.p_drop if self.training else 0.0
        cell = F.cell_run(self.mha_layer._params(), self.mha_layer._cfg(), B, T, m8, src_mask,
                          self.mha_layer.global_dropout if self.training else 0.0)

        Pn = _ffn_params(next_layer.ffn_module1) if next_layer is not None else None

        def run(x3, need, pre_ln=None, with_post=False):
            dtype = compute_dtype or x3.dtype
            x = ops.rows2d(x3)
            post_next = None
            # every LayerNorm that follows a Linear of width d_model = 256 runs in that GEMM's epilogue (`post` = its output and
            # statistics, None when the shape does not qualify and the consumer runs the LayerNorm kernel itself)
            y1, b1, post1 = F.ffn_module_fwd(x, P1, d_act, need, dtype, p=pd, pre_ln=pre_ln, ln_next=(n1.weight, n1.bias, n1.eps))   # :507
            h, bn1 = F.ln_fwd(y1, n1.weight, n1.bias, n1.eps, need, pre=post1, out_dtype=dtype)         # :510
            y2_3, bcell, post2 = cell(h.view(B, T, -1), need, res=y1, ln_next=(Pc["ln1_w"], Pc["ln1_b"], 1e-5))   # :512-530
            y2 = ops.rows2d(y2_3)
            y3, bconv, post3 = F.conv_module_fwd(y2, Pc, d_act, m8, B, T, need, dtype, chunk, p=pd, pre_ln=post2,
                                                 ln_next=(P2["ln_w"], P2["ln_b"], 1e-5), conv_state=conv_state)   # :532-534
            # (norm2's output is the layer output = the next layer's residual stream: stream dtype, 4th element of ln_next)
            # (inside a stack: where norm2 rides in the second FFN's down-projection, the NEXT layer's first LayerNorm can ride with it)
            y4, bf2, post4, post_next = F.ffn_module_fwd(y3, P2, d_act, need, dtype, p=pd, pre_ln=post3, ln_next=(n2.weight, n2.bias, n2.eps, True),
                                                         ln_pair=(Pn["ln_w"], Pn["ln_b"], 1e-5) if Pn is not None else ())
            if (post4 is None and Pn is not None and y4.dtype != dtype and
                    ops.layernorm_pair_ok(y4, dtype, n2.weight, n2.bias, Pn["ln_w"], Pn["ln_b"])):
                # norm2 and the next layer's first LayerNorm in one pass over the float32 stream (equal to two launches to an ulp)
                y5_, st1, hn, st2 = ops.layernorm_fwd_pair(y4, n2.weight.detach(), n2.bias.detach(), n2.eps, Pn["ln_w"].detach(),
                                                           Pn["ln_b"].detach(), 1e-5, need, dtype)
                post4, post_next = (y5_, st1), (hn, st2)
            y5, bn2 = F.ln_fwd(y4, n2.weight, n2.bias, n2.eps, need, pre=post4)        # :536
            if not need:
                return (y5.view(B, T, -1), None, post_next) if with_post else (y5.view(B, T, -1), None)

            def bwd(dy3):
                dy = ops.rows2d(dy3 if dy3.is_contiguous() else dy3.contiguous())
                if dy.dtype != dtype:                      # (a float32 gradient from autograd for the float32 stream: gradients run in the compute dtype)
                    dy = ops.cast(dy, dtype)
                # each LayerNorm backward also writes what the NEXT block applies first to its gradient (`pre`: the FFN's
                # 1/2 * dropout, the conv module's dropout * padding mask) - no separate elementwise pass per module
                pre_c = getattr(bconv, "pre", None)
                d4, d4z = bn2(dy, second=bf2.pre)
                # the cell's own first step, dy * act'(zm), as the second output of the conv module's fused LayerNorm backward
                pre_cell = getattr(bcell, "pre", None) if getattr(bconv, "ln1_fused", False) else None
                d3z = None
                if pre_c is not None:
                    d3, d3z = bf2(d4, dz_in=d4z, second=pre_c)
                else:
                    d3 = bf2(d4, dz_in=d4z)
                d2z = None
                if pre_cell is not None:
                    d2, d2z = bconv(d3, dz_in=d3z, second=pre_cell)
                else:
                    d2 = bconv(d3, dz_in=d3z)
                if getattr(bcell, "can_fuse_ln", False) and F.ln_fusable(bn1.spec, d2.shape[0], d2.shape[1], dtype, bcell.ln_reduce, bcell.ln_W):
                    # norm1's backward (+ the skip gradient, + FFN1's 1/2 * dropout) in the epilogue of the cell's input dgrad
                    d1, d1z = bcell(d2.view(B, T, -1), ln=bn1.spec, ln_res=d2, ln_second=b1.pre, dz_in=d2z)
                else:
                    dh = ops.rows2d(bcell(d2.view(B, T, -1), dz_in=d2z))
                    d1, d1z = bn1(dh, res=d2, second=b1.pre)                           # skip gradient fused
                return b1(d1, dz_in=d1z).view(B, T, -1)
            return (y5.view(B, T, -1), bwd, post_next) if with_post else (y5.view(B, T, -1), bwd)
        return run

    def forward(self, x, src_mask: Optional[torch.Tensor] = None, src_key_padding_mask: Optional[torch.Tensor] = None,
                pos_embs: torch.Tensor = None, dynchunktrain_config=None):
        B, T, _ = x.shape
        m8 = F.mask_u8(src_key_padding_mask, B, T, x.device)
        chunk = dynchunktrain_config.chunk_size if dynchunktrain_config is not None else 0
        stream = F.stream_dtype(x.dtype)
        if stream == x.dtype:
            return F.block(x, self.make_run(B, T, m8, src_mask, chunk), list(self.parameters())), None
        # a bf16 layer called on its own: the same float32 residual stream as inside the encoder stack (cast in, cast out)
        inner = self.make_run(B, T, m8, src_mask, chunk, compute_dtype=x.dtype)
        d = x.shape[2]

        def run(xin, need):
            y, b = inner(ops.cast(ops.rows2d(xin), stream).view(B, T, d), need)
            return ops.cast(ops.rows2d(y), xin.dtype).view(B, T, d), b
        return F.block(x, run, list(self.parameters())), None

    def make_streaming_context(self, dynchunktrain_config: DynChunkTrainConfig):
        """A blank streaming context for this layer (reference :618-633 takes the left context in frames, because it keeps raw
        frames; this layer keeps per-chunk sums and needs the chunk size as well, hence the whole configuration)."""
        _stream_refuse(self, dynchunktrain_config)
        return ConformerEncoderLayerStreamingContext(dynchunktrain_config=dynchunktrain_config)

    def _state_alloc(self, cfg, B, compute, device, new):
        """-> (ring | None, convolution state) of B streams: the float32 per-chunk sums ((B, left, s); (B, s) running sums for an
        unlimited left context; none for left 0) and the (B, (k-1)/2, 2 d) pre-GLU rows.  new: torch.zeros (lockstep reads its state
        as stored) or torch.empty (a slot never reads state before it wrote it)."""
        d = self.norm1.norm.weight.shape[0]
        sdim = self.mha_layer.local_proj_out_dim if self.mode == "SummaryMixing-fast" else self.mha_layer.summary_out_dim
        left = cfg.left_context_size
        ring = (new((B, sdim), dtype=torch.float32, device=device) if left is None else
                new((B, left, sdim), dtype=torch.float32, device=device) if left > 0 else None)
        return ring, new((B, (self.convolution_module.kernel_size - 1) // 2, 2 * d), dtype=compute, device=device)

    def _stream_alloc(self, ctx, B, compute, device, counter):
        cfg = ctx.dynchunktrain_config
        ring, ctx.dcconv_state = self._state_alloc(cfg, B, compute, device, torch.zeros)
        ctx.summary = F.DynChunkStream(ring, counter, cfg.chunk_size, cfg.left_context_size)
        ctx.counter, ctx.batch_size, ctx.dtype, ctx.device = counter, B, compute, torch.device(device)

    def _stream_run(self, ctx, B, C_cur, compute_dtype=None, next_layer=None):
        return self.make_run(B, C_cur, None, ctx.summary, 0, compute_dtype=compute_dtype, next_layer=next_layer,
                             conv_state=F.ConvStream(ctx.dcconv_state))

    def _slot_alloc(self, lc, enc_ctx, B, compute, device):
        cfg = lc.dynchunktrain_config
        ring, lc.dcconv_state = self._state_alloc(cfg, B, compute, device, torch.empty)
        lc.summary = F.DynChunkSlots(ring, enc_ctx.counters, enc_ctx.valid, cfg.chunk_size, cfg.left_context_size)

    def _slot_run(self, lc, enc_ctx, B, C, compute_dtype=None, next_layer=None):
        return self.make_run(B, C, None, lc.summary, 0, compute_dtype=compute_dtype, next_layer=next_layer,
                             conv_state=F.ConvStream(lc.dcconv_state, enc_ctx.valid, enc_ctx.counters))

    def forward_streaming(self, x, context: ConformerEncoderLayerStreamingContext, pos_embs: torch.Tensor = None):
        """One chunk (B, C_cur, d) of a stream through this layer (reference :539-616).  Returns (output, None); the context
        carries the summary and convolution state to the next call."""
        B, C_cur, d = x.shape
        if _stream_check(context, self.training, B, C_cur, x.dtype, x.device):
            self._stream_alloc(context, B, x.dtype, x.device, torch.zeros(1, dtype=torch.int64, device=x.device))
        stream = F.stream_dtype(x.dtype)
        with torch.no_grad():
            if stream == x.dtype:
                y, _ = self._stream_run(context, B, C_cur)(x, False)
            else:                                   # (the float32 residual stream of a bf16 layer, as in forward)
                run = self._stream_run(context, B, C_cur, compute_dtype=x.dtype)
                y, _ = run(ops.cast(ops.rows2d(x), stream).view(B, C_cur, d), False)
                y = ops.cast(ops.rows2d(y), x.dtype).view(B, C_cur, d)
            ops.step_counter_add(context.counter, 1)
        _stream_commit(context, C_cur)
        return y, None


class ConformerEncoder(nn.Module):
    def __init__(self, num_layers, d_model, d_ffn, nhead, kernel_size=31, kdim=None, vdim=None, activation=Swish,
                 bias=True, dropout=0.0, causal=False, attention_type="RelPosMHAXL", local_proj_hid_dim=[512],
                 local_proj_out_dim=512, summary_hid_dim=[1024], mode="SummaryMixing"):
        super().__init__()
        self.layers = nn.ModuleList([
            ConformerEncoderLayer(d_ffn=d_ffn, nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout,
                                  activation=activation, kernel_size=kernel_size, bias=bias, causal=causal,
                                  attention_type=attention_type, local_proj_hid_dim=local_proj_hid_dim,
                                  local_proj_out_dim=local_proj_out_dim, summary_hid_dim=summary_hid_dim, mode=mode)
            for _ in range(num_layers)])
        self.norm = _LayerNorm(d_model, eps=1e-6)
        self.attention_type = attention_type

    def forward(self, src, src_mask: Optional[torch.Tensor] = None, src_key_padding_mask: Optional[torch.Tensor] = None,
                pos_embs: Optional[torch.Tensor] = None, dynchunktrain_config=None, _compute_dtype=None):
        B, T, d = src.shape
        m8 = F.mask_u8(src_key_padding_mask, B, T, src.device)
        chunk = dynchunktrain_config.chunk_size if dynchunktrain_config is not None else 0
        # compute dtype: what the caller says (TransformerASR.encode hands over the float32 stream of a bf16 model), else the input's
        out = F.encoder_stack(src, list(self.layers),
                              lambda layer, compute, nxt=None: layer.make_run(B, T, m8, src_mask, chunk, compute_dtype=compute, next_layer=nxt),
                              self.norm.norm, list(self.parameters()), _compute_dtype, pair_next=True)
        return out, [None] * len(self.layers)

    def make_streaming_context(self, dynchunktrain_config: DynChunkTrainConfig):
        """A blank streaming context for the whole stack (reference :840-857); state is allocated on the first chunk."""
        for layer in self.layers:
            _stream_refuse(layer, dynchunktrain_config)
        return ConformerEncoderStreamingContext(dynchunktrain_config=dynchunktrain_config,
                                                layers=[layer.make_streaming_context(dynchunktrain_config) for layer in self.layers])

    def _stream_begin(self, context, B, C_cur, compute, device):
        """Validate the chunk; allocate the state on the first one."""
        if _stream_check(context, self.training, B, C_cur, compute, device):
            counter = torch.zeros(1, dtype=torch.int64, device=device)
            for layer, lc in zip(self.layers, context.layers):
                layer._stream_alloc(lc, B, compute, device, counter)
            context.counter, context.batch_size, context.dtype, context.device = counter, B, compute, torch.device(device)

    def _stream_chunk(self, src, context, compute):
        """The launches of one chunk step (no validation, no host bookkeeping - what a captured step records): the layers with the
        LayerNorm pair fusion of `forward` (functional.encoder_stack), the final LayerNorm, then the counter (and PE) advance."""
        B, C_cur, _ = src.shape
        ctx_of = {id(layer): lc for layer, lc in zip(self.layers, context.layers)}
        out = F.encoder_stack(src, list(self.layers),
                              lambda layer, comp, nxt=None: layer._stream_run(ctx_of[id(layer)], B, C_cur, comp, nxt),
                              self.norm.norm, list(self.parameters()), compute, pair_next=True)
        if context.pe_table is not None:
            ops.stream_advance(context.counter, context.pe_table, context.pe, context.dynchunktrain_config.chunk_size)
        else:
            ops.step_counter_add(context.counter, 1)
        return out

    def forward_streaming(self, src, context: ConformerEncoderStreamingContext, pos_embs: Optional[torch.Tensor] = None):
        """One chunk (B, C_cur, d) of B streams through the stack (reference :788-838).  Fed the consecutive chunks of equal-length
        utterances, the outputs concatenate to forward(src, dynchunktrain_config=cfg) of the whole utterances.  A chunk shorter than
        chunk_size ends the stream.  Returns (output, [None] * layers)."""
        B, C_cur, _ = src.shape
        self._stream_begin(context, B, C_cur, src.dtype, src.device)
        with torch.no_grad():
            out = self._stream_chunk(src, context, src.dtype)
        _stream_commit(context, C_cur)
        return out, [None] * len(self.layers)

    def make_slot_context(self, dynchunktrain_config: DynChunkTrainConfig, slots: int):
        """A blank slot-streaming context for `slots` independent streams; state is allocated on the first step.  Refuses what
        make_streaming_context refuses."""
        for layer in self.layers:
            _stream_refuse(layer, dynchunktrain_config)
        if not 1 <= int(slots) <= 65535:
            raise ValueError(f"slot streaming: 1 <= slots <= 65535, got {slots}")
        return ConformerEncoderSlotContext(dynchunktrain_config=dynchunktrain_config, slots=int(slots),
                                           layers=[ConformerEncoderLayerSlotContext(dynchunktrain_config) for _ in self.layers])

    def _slot_begin(self, context, src_shape, compute, device, valid, start):
        """Validate the step (host only) and allocate the state on the first one; -> (valid, start, base) for _slot_commit."""
        args = _slot_args(context, self.training, src_shape, compute, device, valid, start)
        if context.counters is None:
            B = context.slots
            context.counters = torch.zeros(B, dtype=torch.int64, device=device)
            context.io = torch.zeros(5 * B, dtype=torch.uint8, device=device)
            context.valid, context.start = context.io[:4 * B].view(torch.int32), context.io[4 * B:]
            context.dtype, context.device = compute, torch.device(device)
            context.frames, context.open = [0] * B, [False] * B
            context.staging = _SlotStaging(B)
            for layer, lc in zip(self.layers, context.layers):
                layer._slot_alloc(lc, context, B, compute, device)
        return args

    def _slot_stage(self, context, valid, start):
        """Copy the step's valid / start into the context's device buffers (in stream order, before the step's launches)."""
        context.staging.copy(context.io, valid, start)

    def _slot_layers(self, src, context, compute):
        """The layers, the final LayerNorm and the counter advance of one slot step (what a captured step records after
        smx_slot_begin)."""
        B, C, _ = src.shape
        ctx_of = {id(layer): lc for layer, lc in zip(self.layers, context.layers)}
        out = F.encoder_stack(src, list(self.layers),
                              lambda layer, comp, nxt=None: layer._slot_run(ctx_of[id(layer)], context, B, C, comp, nxt),
                              self.norm.norm, list(self.parameters()), compute, pair_next=True)
        ops.slot_advance(context.counters, context.valid, B, C)
        return out

    def forward_slots(self, src, valid, start, context: ConformerEncoderSlotContext):
        """One step (B, C, d) of B independent streams, one per slot.  valid[b] (host ints, 0 .. C): slot b's frames in this step -
        C a full chunk, 1 .. C-1 its stream's last chunk, 0 the slot sits out (its state is untouched).  start[b] (host bools): slot b
        begins a new stream here.  Rows [:valid[b]] of slot b's outputs, over the steps of one stream, concatenate to that stream
        alone through forward_streaming; rows at and beyond valid[b] are unspecified (input rows there are never read).
        Returns (output, [None] * layers)."""
        args = self._slot_begin(context, tuple(src.shape), src.dtype, src.device, valid, start)
        self._slot_stage(context, args[0], args[1])
        with torch.no_grad():
            ops.slot_begin(context.counters, context.start, None, None, context.slots, context.dynchunktrain_config.chunk_size,
                           src.shape[2])
            out = self._slot_layers(src, context, src.dtype)
        _slot_commit(context, *args)
        return out, [None] * len(self.layers)

"""hipGraph capture of one streaming chunk step (TransformerASR.encode_streaming).

A chunk step has a fixed shape: B streams x C frames.  Every launch of it reads the chunk index from the context's device counter
(summary ring slot, window length, positional rows) and the step ends by advancing that counter on device, so ONE capture replays
correctly for every later chunk.  Capture records without running: it does not advance the context; replays and eager calls do,
on the device and in the host mirror of the frame count.

CapturedSlotStep does the same for a slot step (TransformerASR.encode_slots): the per-slot counters, the slots' frames in the step
(valid) and the new-stream flags (start) are all device buffers, staged from the host before each replay, so one capture serves
every step, a stream's short last chunk included.
"""
import torch

from .lobes.models.transformer.TransformerASR import EncoderWrapper


class _CapturedStep:
    """The capture recipe both steps share.  The static input buffer; `warm_up(x)`, a step on a scratch context on a side stream
    (allocates weight shadows and workspaces outside the capture; the real context is untouched); `begin(x)` validates and allocates
    the real context's state without a launch and returns the encoder context; then the launches of `chunk(x, ec)` are captured on
    one stream (thread_local capture mode): the graph has no parallel branches, and capture does not advance the context."""

    def __init__(self, asr, context, B, C, dtype, device, warm_up, begin, chunk):
        self.asr, self.context, self.B, self.C = asr, context, B, C
        lin = asr.custom_src_module.layers[0].w
        device = device or lin.weight.device
        self.x = torch.zeros((B, C, lin.weight.shape[1]), dtype=dtype, device=device)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            warm_up(self.x)
        torch.cuda.current_stream(device).wait_stream(side)
        self._ec = begin(self.x)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.y = chunk(self.x, self._ec)


class CapturedStreamStep(_CapturedStep):
    """step(chunk) = encode_streaming(chunk, context) as one graph replay.  chunk: (B, C, F) on the device, dtype `dtype`.  The
    returned tensor is a static buffer, overwritten by the next step.  A short final chunk runs eagerly on the same context
    (finish)."""

    def __init__(self, wrapper, context, B, C, dtype=torch.float32, device=None):
        asr, cfg = wrapper.transformer if isinstance(wrapper, EncoderWrapper) else wrapper, context.dynchunktrain_config
        if C != cfg.chunk_size:
            raise ValueError(f"CapturedStreamStep: C={C} differs from the context's chunk_size")
        super().__init__(asr, context, B, C, dtype, device, lambda x: asr.encode_streaming(x, asr.make_streaming_context(cfg)),
                         lambda x: asr._stream_begin(x, context), asr._stream_chunk)

    def step(self, chunk):
        """One full chunk (B, C, F) through the captured step."""
        if tuple(chunk.shape[:2]) != (self.B, self.C):
            raise ValueError(f"CapturedStreamStep: expected a ({self.B}, {self.C}, F) chunk, got {tuple(chunk.shape)}")
        self.asr._stream_begin(chunk, self.context)
        self.x.copy_(chunk)
        self.graph.replay()
        self._ec.frames += self.C
        return self.y

    def finish(self, chunk):
        """The final (possibly shorter) chunk, eagerly on the same context."""
        return self.asr.encode_streaming(chunk, self.context)


class CapturedSlotStep(_CapturedStep):
    """step(chunk, valid, start) = encode_slots(chunk, valid, start, context) as one graph replay.  chunk: (B, C, F) on the device,
    dtype `dtype`; valid / start: host sequences of B ints / bools, validated and staged into the context's static device buffers
    before the replay.  The returned tensor is a static buffer, overwritten by the next step; rows at and beyond valid[b] are
    unspecified.  A stream's short last chunk runs through the same graph (valid expresses it)."""

    def __init__(self, wrapper, context, B, C, dtype=torch.float32, device=None):
        asr, cfg = wrapper.transformer if isinstance(wrapper, EncoderWrapper) else wrapper, context.dynchunktrain_config
        if C != cfg.chunk_size or B != context.encoder_context.slots:
            raise ValueError(f"CapturedSlotStep: (B, C) = ({B}, {C}) differs from the context's ({context.encoder_context.slots}, "
                             f"{cfg.chunk_size})")
        super().__init__(asr, context, B, C, dtype, device,
                         lambda x: asr.encode_slots(x, [C] * B, [True] * B, asr.make_slot_context(cfg, B)),
                         lambda x: asr._slot_begin(x, [0] * B, [False] * B, context)[0], asr._slot_chunk)

    def step(self, chunk, valid, start):
        """One slot step (B, C, F) through the captured graph."""
        from .lobes.models.transformer.Conformer import _slot_commit
        if chunk.dim() != 3 or tuple(chunk.shape[:2]) != (self.B, self.C):
            raise ValueError(f"CapturedSlotStep: expected a ({self.B}, {self.C}, F) step, got {tuple(chunk.shape)}")
        ec, args = self.asr._slot_begin(chunk, valid, start, self.context)
        self.asr.encoder._slot_stage(ec, args[0], args[1])
        self.x.copy_(chunk)
        self.graph.replay()
        _slot_commit(ec, *args)
        return self.y

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


class CapturedStreamStep:
    """step(chunk) = encode_streaming(chunk, context) as one graph replay.  chunk: (B, C, F) on the device, dtype `dtype`.  The
    returned tensor is a static buffer, overwritten by the next step.  A short final chunk runs eagerly on the same context
    (finish).  The graph is captured on one stream (thread_local capture mode) and has no parallel branches."""

    def __init__(self, wrapper, context, B, C, dtype=torch.float32, device=None):
        asr = wrapper.transformer if isinstance(wrapper, EncoderWrapper) else wrapper
        self.asr, self.context, self.B, self.C = asr, context, B, C
        if C != context.dynchunktrain_config.chunk_size:
            raise ValueError(f"CapturedStreamStep: C={C} differs from the context's chunk_size")
        lin = asr.custom_src_module.layers[0].w
        device = device or lin.weight.device
        self.x = torch.zeros((B, C, lin.weight.shape[1]), dtype=dtype, device=device)
        # warm-up on a scratch context (allocates weight shadows and workspaces outside the capture; the real context is untouched)
        scratch = asr.make_streaming_context(context.dynchunktrain_config)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            asr.encode_streaming(self.x, scratch)
        torch.cuda.current_stream(device).wait_stream(side)
        ec = asr._stream_begin(self.x, context)            # validates and allocates the real context's state (no launch)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.y = asr._stream_chunk(self.x, ec)
        self._ec = ec

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


class CapturedSlotStep:
    """step(chunk, valid, start) = encode_slots(chunk, valid, start, context) as one graph replay.  chunk: (B, C, F) on the device,
    dtype `dtype`; valid / start: host sequences of B ints / bools, validated and staged into the context's static device buffers
    before the replay.  The returned tensor is a static buffer, overwritten by the next step; rows at and beyond valid[b] are
    unspecified.  A stream's short last chunk runs through the same graph (valid expresses it).  Capture runs after a warm-up on a
    scratch context and does not advance the context; the graph is captured on one stream and has no parallel branches."""

    def __init__(self, wrapper, context, B, C, dtype=torch.float32, device=None):
        asr = wrapper.transformer if isinstance(wrapper, EncoderWrapper) else wrapper
        self.asr, self.context, self.B, self.C = asr, context, B, C
        if C != context.dynchunktrain_config.chunk_size or B != context.encoder_context.slots:
            raise ValueError(f"CapturedSlotStep: (B, C) = ({B}, {C}) differs from the context's ({context.encoder_context.slots}, "
                             f"{context.dynchunktrain_config.chunk_size})")
        lin = asr.custom_src_module.layers[0].w
        device = device or lin.weight.device
        self.x = torch.zeros((B, C, lin.weight.shape[1]), dtype=dtype, device=device)
        # warm-up on a scratch context (allocates weight shadows and workspaces outside the capture; the real context is untouched)
        scratch = asr.make_slot_context(context.dynchunktrain_config, B)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            asr.encode_slots(self.x, [C] * B, [True] * B, scratch)
        torch.cuda.current_stream(device).wait_stream(side)
        ec, _ = asr._slot_begin(self.x, [0] * B, [False] * B, context)   # validates and allocates the real context (no launch)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.y = asr._slot_chunk(self.x, ec)
        self._ec = ec

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

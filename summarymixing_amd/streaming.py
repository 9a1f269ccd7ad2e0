"""hipGraph capture of one streaming chunk step (TransformerASR.encode_streaming).

A chunk step has a fixed shape: B streams x C frames.  Every launch of it reads the chunk index from the context's device counter
(summary ring slot, window length, positional rows) and the step ends by advancing that counter on device, so ONE capture replays
correctly for every later chunk.  Capture records without running: it does not advance the context; replays and eager calls do,
on the device and in the host mirror of the frame count.
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

"""Slot streaming through the whole encoder on the GPU: a staggered serving schedule (streams start on different steps, pause,
end with full or short chunks, and slots are reused) against each stream run alone through encode_streaming, lockstep
equivalence, and hipGraph capture (CapturedSlotStep)."""
import pytest
import torch

from tests._util import rel_err

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("ln_fuse_mode")]   # (both LayerNorm dispatches: tests/conftest.py)

F_IN = 80


def _wrapper(mode="SummaryMixing-fast", d=256, seed=7):
    from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    torch.manual_seed(seed)
    net = TransformerASR(tgt_vocab=10, input_size=F_IN, d_model=d, nhead=4, num_encoder_layers=2, num_decoder_layers=0, d_ffn=2 * d,
                         dropout=0.0, encoder_module="conformer", attention_type="SummaryMixing", mode=mode,
                         local_proj_hid_dim=[d], local_proj_out_dim=d, summary_hid_dim=[d], summary_out_dim=d, causal=False,
                         kernel_size=31, positional_encoding="fixed_abs_sine")
    return EncoderWrapper(net).cuda().eval()


# (utterance length in frames, step it arrives on, steps on which its stream pauses - counted from its own first step)
_UTTS = [(40, 0, ()), (19, 0, (1,)), (72, 1, (2, 3)), (8, 2, ()), (29, 3, ()), (48, 4, (0,)), (13, 5, ())]


def _schedule(B, C, utts=_UTTS):
    """A serving schedule: each free slot takes the next arrived utterance (start), feeds one chunk per step except on its
    pauses, and is free again after the utterance's last chunk.  -> steps [(valid, start, [(slot, utt, t0)])]."""
    queue = list(range(len(utts)))
    busy = [None] * B                                  # slot -> [utt, next frame, own step]
    steps, step = [], 0
    while queue or any(busy):
        valid, start, feed = [0] * B, [False] * B, []
        for b in range(B):
            if busy[b] is None and queue and utts[queue[0]][1] <= step:
                busy[b] = [queue.pop(0), 0, 0]
                start[b] = True
            if busy[b] is None:
                continue
            u, t0, own = busy[b]
            busy[b][2] += 1
            if own in utts[u][2]:
                continue                               # paused: sits this step out
            v = min(C, utts[u][0] - t0)
            valid[b] = v
            feed.append((b, u, t0))
            busy[b][1] += v
            if busy[b][1] == utts[u][0]:
                busy[b] = None
        steps.append((valid, start, feed))
        step += 1
    return steps


def _inputs(dtype, utts=_UTTS, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(T, F_IN, generator=g).cuda().to(dtype) for T, _, _ in utts]


def _run_slots(stepper, steps, xs, B, C, dtype):
    """Feed the schedule; NaN in every input row a slot does not own.  -> per utterance, its output rows concatenated."""
    outs = [[] for _ in xs]
    for valid, start, feed in steps:
        src = torch.full((B, C, F_IN), float("nan"), device="cuda", dtype=dtype)
        for b, u, t0 in feed:
            src[b, :valid[b]] = xs[u][t0:t0 + valid[b]]
        y = stepper(src, valid, start)
        for b, u, t0 in feed:
            outs[u].append(y[b, :valid[b]].clone())
    return [torch.cat(o, 0) for o in outs]


def _alone(w, cfg, x, C):
    ctx = w.make_streaming_context(cfg)
    return torch.cat([w.forward_streaming(x[None, t0:t0 + C], ctx)[0] for t0 in range(0, x.shape[0], C)], 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("left", [2, None])
@pytest.mark.parametrize("mode", ["SummaryMixing-fast", "SummaryMixing"])
def test_staggered_schedule_matches_each_stream_alone(mode, left, dtype):
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    B, C = 4, 8
    w = _wrapper(mode)
    cfg = DynChunkTrainConfig(C, left)
    steps = _schedule(B, C)
    assert any(v == 0 and not s for valid, start, _ in steps for v, s in zip(valid, start))   # (pauses and idle slots occur)
    assert sum(start.count(True) for _, start, _ in steps) == len(_UTTS) > B               # (slots are reused)
    xs = _inputs(dtype)
    ctx = w.make_slot_context(cfg, B)
    got = _run_slots(lambda s, v, st: w.forward_slots(s, v, st, ctx), steps, xs, B, C, dtype)
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    for u, x in enumerate(xs):
        ref = _alone(w, cfg, x, C)
        assert got[u].shape == ref.shape and torch.isfinite(got[u]).all(), u
        assert rel_err(got[u], ref) <= tol, (u, rel_err(got[u], ref))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("left", [2, None])
def test_lockstep_slots_equal_encode_streaming(left, dtype):
    """B slots all started on step 0 and fed full chunks: the lockstep path's bits."""
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    B, C = 3, 8
    w = _wrapper()
    cfg = DynChunkTrainConfig(C, left)
    x = torch.randn(B, 6 * C, F_IN, device="cuda").to(dtype)
    lctx, sctx = w.make_streaming_context(cfg), w.make_slot_context(cfg, B)
    for i, t0 in enumerate(range(0, 6 * C, C)):
        yl = w.forward_streaming(x[:, t0:t0 + C], lctx)
        ys = w.forward_slots(x[:, t0:t0 + C], [C] * B, [i == 0] * B, sctx)
        assert torch.equal(yl, ys), i


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_slot_step_is_bit_identical_to_eager(dtype):
    from summarymixing_amd.streaming import CapturedSlotStep
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    B, C = 4, 8
    w = _wrapper()
    cfg = DynChunkTrainConfig(C, 2)
    steps = _schedule(B, C)
    xs = _inputs(dtype, seed=1)
    ectx = w.make_slot_context(cfg, B)
    eager = _run_slots(lambda s, v, st: w.forward_slots(s, v, st, ectx), steps, xs, B, C, dtype)
    ctx = w.make_slot_context(cfg, B)
    cap = CapturedSlotStep(w, ctx, B, C, dtype=dtype)
    ec = ctx.encoder_context
    assert ec.frames == [0] * B and ec.open == [False] * B and ec.counters.cpu().tolist() == [0] * B   # capture does not advance
    got = _run_slots(cap.step, steps, xs, B, C, dtype)
    for u in range(len(xs)):
        assert torch.equal(got[u], eager[u]), u
    assert ec.frames == ectx.encoder_context.frames and ec.open == ectx.encoder_context.open
    assert torch.equal(ec.counters, ectx.encoder_context.counters)

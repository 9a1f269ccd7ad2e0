"""Chunk-by-chunk streaming through the encoder on the GPU: pinned by the reference golden, against the fp64 oracle at width,
against the product's own full-utterance DynChunk forward, batch and context isolation, refusals, and hipGraph capture."""
import pytest
import torch

from tests import _golden as G
from tests._util import rel_err, rms_rel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("ln_fuse_mode")]   # (both LayerNorm dispatches: tests/conftest.py)


def _stream(fn, src, C, ctx):
    return torch.cat([fn(src[:, t0:t0 + C], ctx) for t0 in range(0, src.shape[1], C)], 1)


def _enc_stream(enc, x, C, ctx):
    return _stream(lambda c, k: enc.forward_streaming(c, k)[0], x, C, ctx)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_golden_dynchunk_utterance_streamed(dtype):
    """g5_config1_encoder_dynchunk, utterance 0 (wav_len 1.0, T = 50): six chunks of 8 and one of 2, left context 2."""
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    from tests.test_encoder_gpu import _asr
    meta, a, sd, _ = G.load("g5_config1_encoder_dynchunk")
    if not sd:
        sd = G.load("g5_config1_encoder")[2]
    src = a["src"]
    assert float(a["wav_len"][0]) == 1.0
    enc = _asr(meta, sd, src.shape[2] * src.shape[3])
    C, left = meta["dynchunk"]
    ctx = enc.make_streaming_context(DynChunkTrainConfig(C, left))
    y = _stream(enc.forward_streaming, src[:1].cuda().to(dtype), C, ctx)
    assert ctx.encoder_context.frames == 50 and ctx.encoder_context.closed
    err, rms = rel_err(y[0], a["y"][0]), rms_rel(y[0], a["y"][0])
    tol = 1e-3 if dtype == torch.float32 else 1e-2
    assert err <= tol and rms <= tol, (err, rms)


def _encoder(d, mode, nhead, seed):
    from summarymixing_amd.lobes.models.transformer.Conformer import ConformerEncoder
    torch.manual_seed(seed)
    enc = ConformerEncoder(2, d, 2 * d, nhead, kernel_size=31, activation="swish", dropout=0.0, attention_type="SummaryMixing",
                           local_proj_hid_dim=[d], local_proj_out_dim=d, summary_hid_dim=[d], mode=mode)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)
            elif "bias" in n:
                p.normal_(0, 0.05)
    return enc.eval()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("left", [0, 2, None])
@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("d,mode,nhead", [(256, "SummaryMixing-fast", 4), (512, "SummaryMixing-fast", 4), (256, "SummaryMixing", 4)])
def test_streaming_at_width_vs_oracle(d, mode, nhead, C, left, dtype):
    from oracle import smx_oracle as O
    from summarymixing_amd import functional as F
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    B, T = 2, 200
    enc = _encoder(d, mode, nhead, C + (left or 0))
    sd = {k: v.double() for k, v in enc.state_dict().items()}
    x = torch.randn(B, T, d)
    with torch.no_grad():
        ref = O.conformer_encoder(x.double(), sd, "", "swish", mode, d, O.dynchunk_sum_mask(T, C, left), None, C)
    enc = enc.cuda()
    cfg = DynChunkTrainConfig(C, left)
    y = _enc_stream(enc, x.cuda().to(dtype), C, enc.make_streaming_context(cfg))
    assert rel_err(y, ref) <= (1e-3 if dtype == torch.float32 else 1e-2), rel_err(y, ref)
    if dtype == torch.float32:
        with torch.no_grad():
            full, _ = enc(x.cuda(), src_mask=F.DynChunkMask(T, C, left), dynchunktrain_config=cfg)
        assert rel_err(y, full) <= 1e-5, rel_err(y, full)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_of_streams_matches_each_alone(dtype):
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    enc = _encoder(256, "SummaryMixing-fast", 4, 3).cuda()
    cfg = DynChunkTrainConfig(16, 2)
    x = torch.randn(4, 72, 256, device="cuda").to(dtype)
    yb = _enc_stream(enc, x, 16, enc.make_streaming_context(cfg))
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    for b in range(4):
        ya = _enc_stream(enc, x[b:b + 1], 16, enc.make_streaming_context(cfg))
        assert rel_err(yb[b:b + 1], ya) <= tol, (b, rel_err(yb[b:b + 1], ya))


def test_contexts_fed_alternately_are_independent():
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    enc = _encoder(256, "SummaryMixing-fast", 4, 4).cuda()
    cfg = DynChunkTrainConfig(8, None)
    xa, xb = torch.randn(2, 40, 256, device="cuda"), torch.randn(2, 40, 256, device="cuda")
    ya = _enc_stream(enc, xa, 8, enc.make_streaming_context(cfg))
    yb = _enc_stream(enc, xb, 8, enc.make_streaming_context(cfg))
    ca, cb = enc.make_streaming_context(cfg), enc.make_streaming_context(cfg)
    oa, ob = [], []
    for t0 in range(0, 40, 8):
        oa.append(enc.forward_streaming(xa[:, t0:t0 + 8], ca)[0])
        ob.append(enc.forward_streaming(xb[:, t0:t0 + 8], cb)[0])
    assert torch.equal(torch.cat(oa, 1), ya) and torch.equal(torch.cat(ob, 1), yb)


def test_state_misuse_raises():
    from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    enc = _encoder(256, "SummaryMixing-fast", 4, 5).cuda()
    ctx = enc.make_streaming_context(DynChunkTrainConfig(8, 2))
    enc.forward_streaming(torch.randn(2, 8, 256, device="cuda"), ctx)
    with pytest.raises(ValueError):                              # another batch size
        enc.forward_streaming(torch.randn(3, 8, 256, device="cuda"), ctx)
    with pytest.raises(ValueError):                              # another dtype
        enc.forward_streaming(torch.randn(2, 8, 256, device="cuda").bfloat16(), ctx)
    enc.forward_streaming(torch.randn(2, 5, 256, device="cuda"), ctx)
    with pytest.raises(ValueError):                              # after a short final chunk
        enc.forward_streaming(torch.randn(2, 8, 256, device="cuda"), ctx)
    torch.manual_seed(0)
    net = TransformerASR(tgt_vocab=10, input_size=20, d_model=64, nhead=2, num_encoder_layers=1, num_decoder_layers=0, d_ffn=128,
                         dropout=0.0, encoder_module="conformer", attention_type="SummaryMixing", mode="SummaryMixing-fast",
                         local_proj_hid_dim=[64], local_proj_out_dim=64, summary_hid_dim=[64], causal=False, kernel_size=15,
                         max_length=40)
    w = EncoderWrapper(net).cuda().eval()
    ctx = w.make_streaming_context(DynChunkTrainConfig(16, None))
    w.forward_streaming(torch.randn(1, 16, 20, device="cuda"), ctx)
    w.forward_streaming(torch.randn(1, 16, 20, device="cuda"), ctx)
    with pytest.raises(ValueError):                              # frames 32 .. 48 run past max_length 40
        w.forward_streaming(torch.randn(1, 16, 20, device="cuda"), ctx)
    w.forward_streaming(torch.randn(1, 8, 20, device="cuda"), ctx)   # (exactly up to max_length is fine)


def _wrapper(d=256):
    from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    torch.manual_seed(7)
    net = TransformerASR(tgt_vocab=10, input_size=80, d_model=d, nhead=4, num_encoder_layers=2, num_decoder_layers=0, d_ffn=2 * d,
                         dropout=0.0, encoder_module="conformer", attention_type="SummaryMixing", mode="SummaryMixing-fast",
                         local_proj_hid_dim=[d], local_proj_out_dim=d, summary_hid_dim=[d], causal=False, kernel_size=31)
    return EncoderWrapper(net).cuda().eval()


@pytest.mark.parametrize("B,C", [(1, 16), (4, 8)])
def test_captured_step_is_bit_identical_to_eager(B, C):
    from summarymixing_amd.streaming import CapturedStreamStep
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    w = _wrapper()
    cfg = DynChunkTrainConfig(C, 2)
    T = 11 * C + C // 2
    src = torch.randn(B, T, 80, device="cuda")
    eager = _stream(w.forward_streaming, src, C, w.make_streaming_context(cfg))
    ctx = w.make_streaming_context(cfg)
    cap = CapturedStreamStep(w, ctx, B, C)
    assert ctx.encoder_context.frames == 0              # capture does not advance the context
    outs = [cap.step(src[:, t0:t0 + C]).clone() for t0 in range(0, 11 * C, C)]
    outs.append(cap.finish(src[:, 11 * C:]))
    assert ctx.encoder_context.frames == T and ctx.encoder_context.closed
    assert torch.equal(torch.cat(outs, 1), eager)

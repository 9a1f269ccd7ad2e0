"""Streaming inference without a GPU: the three C entry points refuse bad arguments on the host (no launch), the module surface
refuses the modes whose Dynamic Chunk Training forward is not causal, and the context dataclasses / methods carry the reference's
names and signatures."""
import dataclasses
import inspect

import pytest
import torch

_BASE = 1 << 40          # fake, never dereferenced: every case below is refused before any launch
S, OUT, RING, CNT = _BASE, _BASE + 0x100000, _BASE + 0x200000, _BASE + 0x300000


def _summary(**kw):
    from summarymixing_amd import _lib as L
    a = dict(dtype=L.BF16, S=S, lds=144, out=OUT, ldo=144, ring=RING, counter=CNT, B=2, C_cur=8, C=8, D=144, left=2)
    a.update(kw)
    return L.lib().smx_stream_summary(a["dtype"], a["S"], a["lds"], a["out"], a["ldo"], a["ring"], a["counter"], a["B"], a["C_cur"],
                                      a["C"], a["D"], a["left"], None)


def _dwconv(**kw):
    from summarymixing_amd import _lib as L
    a = dict(dtype=L.BF16, P=S, ldp=512, w=RING, bias=None, state=CNT, Y=OUT, ldy=256, B=2, C_cur=8, D=256, k=31)
    a.update(kw)
    return L.lib().smx_dwconv1d_glu_stream(a["dtype"], a["P"], a["ldp"], a["w"], a["bias"], a["state"], a["Y"], a["ldy"], a["B"],
                                           a["C_cur"], a["D"], a["k"], None)


def _advance(**kw):
    from summarymixing_amd import _lib as L
    a = dict(dtype=L.F32, counter=CNT, table=S, ldt=256, rows=2500, pe=OUT, ldpe=256, C=16, D=256)
    a.update(kw)
    return L.lib().smx_stream_advance(a["dtype"], a["counter"], a["table"], a["ldt"], a["rows"], a["pe"], a["ldpe"], a["C"], a["D"], None)


@pytest.mark.parametrize("kw", [dict(dtype=2), dict(S=None), dict(out=None), dict(counter=None), dict(ring=None), dict(B=0),
                                dict(D=0), dict(D=140), dict(C=65, C_cur=8), dict(C=0, C_cur=0), dict(C_cur=0), dict(C_cur=9),
                                dict(left=33), dict(left=-2), dict(lds=100), dict(ldo=100)])
def test_stream_summary_refusals(kw):
    assert _summary(**kw) == -1


@pytest.mark.parametrize("kw", [dict(dtype=-1), dict(P=None), dict(w=None), dict(Y=None), dict(state=None), dict(k=0), dict(k=30),
                                dict(k=65), dict(B=0), dict(D=0), dict(D=100), dict(C_cur=0), dict(C_cur=65), dict(ldp=511),
                                dict(ldy=255)])
def test_dwconv_stream_refusals(kw):
    assert _dwconv(**kw) == -1


@pytest.mark.parametrize("kw", [dict(dtype=3), dict(counter=None), dict(table=None), dict(pe=None), dict(C=0), dict(C=65), dict(D=0),
                                dict(rows=-1), dict(ldt=255), dict(ldpe=100)])
def test_stream_advance_refusals(kw):
    assert _advance(**kw) == -1


def _asr(mode="SummaryMixing-fast", encoder_module="conformer", d=32):
    from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    kw = dict(tgt_vocab=10, input_size=20, d_model=d, nhead=2, num_encoder_layers=2, num_decoder_layers=0, d_ffn=64, dropout=0.0,
              encoder_module=encoder_module, attention_type="SummaryMixing", mode=mode, local_proj_hid_dim=[d],
              local_proj_out_dim=d, summary_hid_dim=[d], summary_out_dim=d, causal=False, kernel_size=15)
    if encoder_module == "branchformer":
        kw["csgu_linear_units"] = 64
    return EncoderWrapper(TransformerASR(**kw)).eval()


@pytest.mark.parametrize("mode", ["SummaryMixing-lite", "SummaryMixing-expdecay"])
def test_non_causal_modes_are_refused(mode):
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    with pytest.raises(NotImplementedError):
        _asr(mode).make_streaming_context(DynChunkTrainConfig(8, 2))


def test_branchformer_is_refused():
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    with pytest.raises(NotImplementedError):
        _asr("SummaryMixing", "branchformer").make_streaming_context(DynChunkTrainConfig(8, 2))


def test_sequence_parallel_is_refused(monkeypatch):
    from summarymixing_amd import sequence_parallel as SP
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    enc = _asr()
    monkeypatch.setattr(SP, "enabled", lambda: True)
    with pytest.raises(NotImplementedError):
        enc.make_streaming_context(DynChunkTrainConfig(8, 2))


@pytest.mark.parametrize("cfg", [(0, 2), (65, 2), (8, 33), (8, -1)])
def test_bad_configurations_are_refused(cfg):
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    with pytest.raises(ValueError):
        _asr().make_streaming_context(DynChunkTrainConfig(*cfg))


def test_training_mode_raises_before_any_launch():
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    enc = _asr()
    ctx = enc.make_streaming_context(DynChunkTrainConfig(8, 2))
    enc.train()
    with pytest.raises(RuntimeError):
        enc.forward_streaming(torch.zeros(1, 8, 20), ctx)
    layer = enc.transformer.encoder.layers[0].train()
    with pytest.raises(RuntimeError):
        layer.forward_streaming(torch.zeros(1, 8, 32), layer.make_streaming_context(DynChunkTrainConfig(8, 2)))
    assert ctx.encoder_context.batch_size is None and ctx.encoder_context.frames == 0


def test_contexts_and_signatures():
    from summarymixing_amd.lobes.models.transformer import Conformer as Cf
    from summarymixing_amd.lobes.models.transformer import TransformerASR as T
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    for cls in (Cf.ConformerEncoderLayerStreamingContext, Cf.ConformerEncoderStreamingContext, T.TransformerASRStreamingContext):
        assert dataclasses.is_dataclass(cls)
    assert {f.name for f in dataclasses.fields(Cf.ConformerEncoderStreamingContext)} >= {"dynchunktrain_config", "layers"}
    assert {f.name for f in dataclasses.fields(T.TransformerASRStreamingContext)} == {"dynchunktrain_config", "encoder_context"}
    assert {f.name for f in dataclasses.fields(Cf.ConformerEncoderLayerStreamingContext)} >= {"summary", "dcconv_state"}
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Cf.ConformerEncoderLayer.forward_streaming) == ["self", "x", "context", "pos_embs"]
    assert sig(Cf.ConformerEncoder.forward_streaming) == ["self", "src", "context", "pos_embs"]
    assert sig(Cf.ConformerEncoder.make_streaming_context) == ["self", "dynchunktrain_config"]
    assert sig(T.TransformerASR.make_streaming_context) == ["self", "dynchunktrain_config", "encoder_kwargs"]
    assert sig(T.TransformerASR.encode_streaming) == ["self", "src", "context"]
    assert sig(T.EncoderWrapper.forward_streaming) == ["self", "x", "context"]
    ctx = _asr().make_streaming_context(DynChunkTrainConfig(16, None))
    assert isinstance(ctx, T.TransformerASRStreamingContext)
    ec = ctx.encoder_context
    assert isinstance(ec, Cf.ConformerEncoderStreamingContext) and len(ec.layers) == 2
    assert all(isinstance(lc, Cf.ConformerEncoderLayerStreamingContext) and lc.summary is None for lc in ec.layers)

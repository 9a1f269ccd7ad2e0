"""Slot streaming without a GPU: the four C entry points refuse bad arguments on the host (no launch), the module surface refuses
what lockstep streaming refuses, the context / method signatures, and every host-side ValueError of a step raised before any
launch (the library is swapped for a stub that fails the test on any call)."""
import dataclasses
import inspect

import pytest
import torch

_BASE = 1 << 40          # fake, never dereferenced: every case below is refused before any launch
S, OUT, RING, CNT, VAL = _BASE, _BASE + 0x100000, _BASE + 0x200000, _BASE + 0x300000, _BASE + 0x400000


def _summary(**kw):
    from summarymixing_amd import _lib as L
    a = dict(dtype=L.BF16, S=S, lds=144, out=OUT, ldo=144, ring=RING, counters=CNT, valid=VAL, B=2, C=8, D=144, left=2)
    a.update(kw)
    return L.lib().smx_slot_summary(a["dtype"], a["S"], a["lds"], a["out"], a["ldo"], a["ring"], a["counters"], a["valid"], a["B"],
                                    a["C"], a["D"], a["left"], None)


def _dwconv(**kw):
    from summarymixing_amd import _lib as L
    a = dict(dtype=L.BF16, P=S, ldp=512, w=RING, bias=None, state=CNT, Y=OUT, ldy=256, valid=VAL, counters=CNT + 64, B=2, C=8, D=256,
             k=31)
    a.update(kw)
    return L.lib().smx_dwconv1d_glu_slots(a["dtype"], a["P"], a["ldp"], a["w"], a["bias"], a["state"], a["Y"], a["ldy"], a["valid"],
                                          a["counters"], a["B"], a["C"], a["D"], a["k"], None)


def _begin(**kw):
    from summarymixing_amd import _lib as L
    a = dict(dtype=L.F32, counters=CNT, start=VAL, table=S, ldt=256, rows=2500, pe=OUT, ldpe=256, B=4, C=16, D=256)
    a.update(kw)
    return L.lib().smx_slot_begin(a["dtype"], a["counters"], a["start"], a["table"], a["ldt"], a["rows"], a["pe"], a["ldpe"], a["B"],
                                  a["C"], a["D"], None)


def _advance(**kw):
    from summarymixing_amd import _lib as L
    a = dict(counters=CNT, valid=VAL, B=4, C=16)
    a.update(kw)
    return L.lib().smx_slot_advance(a["counters"], a["valid"], a["B"], a["C"], None)


@pytest.mark.parametrize("kw", [dict(dtype=2), dict(S=None), dict(out=None), dict(counters=None), dict(valid=None), dict(ring=None),
                                dict(B=0), dict(B=65536), dict(D=0), dict(D=140), dict(C=65), dict(C=0), dict(left=33),
                                dict(left=-2), dict(lds=100), dict(ldo=100)])
def test_slot_summary_refusals(kw):
    assert _summary(**kw) == -1


@pytest.mark.parametrize("kw", [dict(dtype=-1), dict(P=None), dict(w=None), dict(Y=None), dict(state=None), dict(valid=None),
                                dict(counters=None), dict(k=0), dict(k=30), dict(k=65), dict(B=0), dict(D=0), dict(D=100),
                                dict(C=0), dict(C=65), dict(ldp=511), dict(ldy=255)])
def test_dwconv_slots_refusals(kw):
    assert _dwconv(**kw) == -1


@pytest.mark.parametrize("kw", [dict(dtype=3), dict(counters=None), dict(start=None), dict(table=None), dict(B=0), dict(C=0),
                                dict(C=65), dict(D=0), dict(rows=-1), dict(ldt=255), dict(ldpe=100)])
def test_slot_begin_refusals(kw):
    assert _begin(**kw) == -1


@pytest.mark.parametrize("kw", [dict(counters=None), dict(valid=None), dict(B=0), dict(C=0), dict(C=65)])
def test_slot_advance_refusals(kw):
    assert _advance(**kw) == -1


def _asr(mode="SummaryMixing-fast", encoder_module="conformer", d=32, max_length=2500):
    from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    kw = dict(tgt_vocab=10, input_size=20, d_model=d, nhead=2, num_encoder_layers=2, num_decoder_layers=0, d_ffn=64, dropout=0.0,
              encoder_module=encoder_module, attention_type="SummaryMixing", mode=mode, local_proj_hid_dim=[d],
              local_proj_out_dim=d, summary_hid_dim=[d], summary_out_dim=d, causal=False, kernel_size=15, max_length=max_length)
    if encoder_module == "branchformer":
        kw["csgu_linear_units"] = 64
    return EncoderWrapper(TransformerASR(**kw)).eval()


@pytest.mark.parametrize("mode", ["SummaryMixing-lite", "SummaryMixing-expdecay"])
def test_non_causal_modes_are_refused(mode):
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    with pytest.raises(NotImplementedError):
        _asr(mode).make_slot_context(DynChunkTrainConfig(8, 2), 4)


def test_branchformer_is_refused():
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    with pytest.raises(NotImplementedError):
        _asr("SummaryMixing", "branchformer").make_slot_context(DynChunkTrainConfig(8, 2), 4)


def test_sequence_parallel_is_refused(monkeypatch):
    from summarymixing_amd import sequence_parallel as SP
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    enc = _asr()
    monkeypatch.setattr(SP, "enabled", lambda: True)
    with pytest.raises(NotImplementedError):
        enc.make_slot_context(DynChunkTrainConfig(8, 2), 4)


@pytest.mark.parametrize("cfg,slots", [((0, 2), 4), ((65, 2), 4), ((8, 33), 4), ((8, -1), 4), ((8, 2), 0), ((8, 2), 65536)])
def test_bad_configurations_are_refused(cfg, slots):
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    with pytest.raises(ValueError):
        _asr().make_slot_context(DynChunkTrainConfig(*cfg), slots)


class _NoLaunch:
    """Stands in for libsmx: any launching call fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} called: the step should have been refused before any launch")


@pytest.fixture
def no_launch(monkeypatch):
    from summarymixing_amd import _lib as L
    monkeypatch.setattr(L, "_lib", _NoLaunch())


def _primed(slots=3, C=8, max_length=2500, frames=None, open_=None):
    """A context whose state looks allocated (CPU tensors stand in; nothing is ever launched) with the given host mirrors."""
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    w = _asr(max_length=max_length)
    ctx = w.make_slot_context(DynChunkTrainConfig(C, 2), slots)
    ec = ctx.encoder_context
    ec.counters = torch.zeros(slots, dtype=torch.int64)
    ec.dtype, ec.device = torch.float32, torch.device("cpu")
    ec.frames = list(frames or [0] * slots)
    ec.open = list(open_ or [False] * slots)
    ec.pe = torch.zeros(slots * C, 32)
    return w, ctx


@pytest.mark.parametrize("case", ["closed", "never_started", "valid_high", "valid_negative", "changed_B", "short_lists",
                                  "changed_C", "changed_dtype", "past_max_length"])
def test_step_misuse_raises_before_any_launch(case, no_launch):
    w, ctx = _primed(frames=[16, 5, 0], open_=[True, False, False], max_length=24)
    ec = ctx.encoder_context
    src, valid, start = torch.zeros(3, 8, 20), [8, 0, 0], [False, False, False]
    if case == "closed":                       # slot 1 was ended by a short chunk
        valid = [8, 8, 0]
    elif case == "never_started":
        valid = [8, 0, 3]
    elif case == "valid_high":
        valid = [9, 0, 0]
    elif case == "valid_negative":
        valid = [8, -1, 0]
    elif case == "changed_B":
        src, valid, start = torch.zeros(4, 8, 20), [8, 0, 0, 0], [False] * 4
    elif case == "short_lists":
        valid, start = [8, 0], [False, False]
    elif case == "changed_C":
        src = torch.zeros(3, 16, 20)
    elif case == "changed_dtype":
        src = src.bfloat16()
    elif case == "past_max_length":            # slot 0 holds 16 frames, max_length 24
        valid = [8, 0, 0]
        ec.frames[0] = 17
    before = (list(ec.frames), list(ec.open))
    with pytest.raises(ValueError):
        w.forward_slots(src, valid, start, ctx)
    assert (ec.frames, ec.open) == before


def test_start_makes_a_closed_slot_usable_again(no_launch):
    """The host-side checks pass for a restarted slot and report the frames each stream holds before the step."""
    w, ctx = _primed(frames=[16, 5, 0], open_=[True, False, False], max_length=24)
    ec = ctx.encoder_context
    valid, start, base = w.transformer.encoder._slot_begin(ec, (3, 8, 20), torch.float32, "cpu", [8, 8, 0], [False, True, False])
    assert (valid, start, base) == ([8, 8, 0], [False, True, False], [16, 0, 0])


def test_training_mode_raises_before_any_launch(no_launch):
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    enc = _asr()
    ctx = enc.make_slot_context(DynChunkTrainConfig(8, 2), 2)
    enc.train()
    with pytest.raises(RuntimeError):
        enc.forward_slots(torch.zeros(2, 8, 20), [8, 8], [True, True], ctx)
    assert ctx.encoder_context.counters is None and ctx.encoder_context.frames == []


def test_contexts_and_signatures():
    from summarymixing_amd import functional as F
    from summarymixing_amd.lobes.models.transformer import Conformer as Cf
    from summarymixing_amd.lobes.models.transformer import TransformerASR as T
    from summarymixing_amd.streaming import CapturedSlotStep
    from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
    for cls in (Cf.ConformerEncoderLayerSlotContext, Cf.ConformerEncoderSlotContext):
        assert dataclasses.is_dataclass(cls)
    assert {f.name for f in dataclasses.fields(Cf.ConformerEncoderSlotContext)} >= {
        "dynchunktrain_config", "slots", "layers", "counters", "valid", "start", "frames", "open"}
    assert {f.name for f in dataclasses.fields(Cf.ConformerEncoderLayerSlotContext)} >= {"summary", "dcconv_state"}
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Cf.ConformerEncoder.make_slot_context) == ["self", "dynchunktrain_config", "slots"]
    assert sig(Cf.ConformerEncoder.forward_slots) == ["self", "src", "valid", "start", "context"]
    assert sig(T.TransformerASR.make_slot_context) == ["self", "dynchunktrain_config", "slots"]
    assert sig(T.TransformerASR.encode_slots) == ["self", "src", "valid", "start", "context"]
    assert sig(T.EncoderWrapper.forward_slots) == ["self", "x", "valid", "start", "context"]
    assert sig(CapturedSlotStep.__init__) == ["self", "wrapper", "context", "B", "C", "dtype", "device"]
    assert sig(CapturedSlotStep.step) == ["self", "chunk", "valid", "start"]
    assert sig(F.DynChunkSlots.__init__) == ["self", "ring", "counters", "valid", "chunk_size", "left_context"]
    ctx = _asr().make_slot_context(DynChunkTrainConfig(16, None), 5)
    assert isinstance(ctx, T.TransformerASRStreamingContext)
    ec = ctx.encoder_context
    assert isinstance(ec, Cf.ConformerEncoderSlotContext) and ec.slots == 5 and len(ec.layers) == 2
    assert all(isinstance(lc, Cf.ConformerEncoderLayerSlotContext) and lc.summary is None for lc in ec.layers)

"""TransformerLM and its scorer without a GPU: the state_dict keys (``encoder.*`` against tests/golden/transformerlm_state_keys.json, taken
from the reference's own TransformerEncoder(attention_type="regularMHA"); the three outer groups as stated from upstream in
tests/_transformerlm_ref.py), every refusal by name, the float64 restatement of the LM (tests/_transformerlm_ref.py) against a
torch.nn.TransformerEncoder chain in float64, the arguments and refusals of TransformerLMScorer / ScorerBuilder, and what smx_lm_score
refuses on the host before any launch."""
import ctypes
import json
import os

import pytest
import torch
from torch import nn

from tests import _lm_models as LM
from tests import _transformerlm_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
_BASE = 1 << 40


def _lm(**kw):
    from summarymixing_amd.lobes.models.transformer.TransformerLM import TransformerLM
    base = dict(vocab=40, d_model=64, nhead=1, num_encoder_layers=2, d_ffn=128, dropout=0.0, activation=nn.GELU, max_length=50)
    return TransformerLM(**{**base, **kw})


def test_state_dict_keys_are_the_references_plus_upstreams_outer_groups_and_load_strict():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "transformerlm_state_keys.json")))["encoder"]
    m = _lm()
    want = {k: tuple(v) for k, v in golden.items()}
    want.update(LR.outer_keys(64, 40, 50))
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want, sorted(set(got.items()) ^ set(want.items()))
    for layer in m.encoder.layers:
        assert layer.norm1.norm.eps == layer.norm2.norm.eps == 1e-6
    assert m.encoder.norm.norm.eps == 1e-6 and m.output_proj.layers[1].norm.eps == 1e-6
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(s, generator=g) for k, s in want.items()}            # a checkpoint with exactly those keys
    assert m.load_state_dict(sd, strict=True).missing_keys == []
    assert torch.equal(m.output_proj.layers[2].w.weight, sd["output_proj.layers.2.w.weight"])
    assert list(_lm(normalize_before=True).state_dict()) == list(m.state_dict())
    # upstream's defaults and argument names
    import inspect
    from summarymixing_amd.lobes.models.transformer import TransformerLM as exported
    sig = inspect.signature(exported.__init__)
    assert list(sig.parameters)[1:] == ["vocab", "d_model", "nhead", "num_encoder_layers", "num_decoder_layers", "d_ffn", "dropout", "activation",
                                        "positional_encoding", "normalize_before", "d_embedding", "max_length", "causal", "attention_type",
                                        "decoder_use_memory"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["d_model"], d["nhead"], d["num_encoder_layers"], d["num_decoder_layers"], d["d_ffn"], d["dropout"], d["max_length"]) == (512, 8, 12, 0, 2048, 0.1, 2500)
    assert d["activation"] is nn.ReLU and d["causal"] is True and d["attention_type"] == "regularMHA" and d["normalize_before"] is False


@pytest.mark.parametrize("kw,msg", [
    (dict(num_decoder_layers=1), "num_decoder_layers=1"),
    (dict(d_embedding=32), "d_embedding=32"),
    (dict(attention_type="RelPosMHAXL"), "attention_type='RelPosMHAXL'"),
    (dict(attention_type="SummaryMixing"), "attention_type='SummaryMixing'"),
    (dict(positional_encoding=None), "positional_encoding=None"),
    (dict(positional_encoding="rope"), "positional_encoding='rope'"),
    (dict(causal=False), "causal=False"),
    (dict(decoder_use_memory=True), "decoder_use_memory=True"),
    (dict(nhead=2), "head dimension d_model / nhead = 64/2"),
    (dict(d_model=96, nhead=1), "96/1"),
])
def test_constructor_refuses_by_name(kw, msg):
    import re
    with pytest.raises(NotImplementedError, match=re.escape(msg)):
        _lm(**kw)


def test_calls_refuse_training_with_dropout_and_gradients_before_any_launch():
    tokens = torch.ones(2, 3, dtype=torch.int64)
    m = _lm(dropout=0.1)
    assert m.training
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training mode with dropout=0.1"):
        m(tokens)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training mode with dropout=0.1"):
        m.step(tokens[:, 0], None)
    m.eval()
    with pytest.raises(NotImplementedError, match="needs gradients"):
        m(tokens)
    with pytest.raises(NotImplementedError, match="needs gradients"):
        m.step(tokens[:, 0], None)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):            # past the refusals: no CPU path
        m(tokens)
    with torch.no_grad(), pytest.raises(ValueError, match="exceeds max_length 50"):
        m(torch.ones(1, 51, dtype=torch.int64))
    with pytest.raises(ValueError, match="max_length"):
        m.make_state(4, 51)


@pytest.mark.parametrize("name", ["lm-d64-post", "lm-d128-h2-pre"])
def test_float64_restatement_equals_a_torch_transformer_encoder_chain(name):
    """Both normalize_before orders, one sequence holding a pad token (masked as a key, position 0 is never one), to 1e-12."""
    d, H, f, layers, pre = LM.MODELS[name]
    m = LM.build(name, torch.float32, 11, device="cpu")
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    layer = nn.TransformerEncoderLayer(d, H, f, dropout=0.0, activation="gelu", layer_norm_eps=1e-6, batch_first=True, norm_first=pre)
    enc = nn.TransformerEncoder(layer, layers, norm=nn.LayerNorm(d, eps=1e-6), enable_nested_tensor=False).double()
    own = {}
    for i in range(layers):
        s, t = f"encoder.layers.{i}.", f"layers.{i}."
        for a, b in (("self_att.att.in_proj_weight", "self_attn.in_proj_weight"), ("self_att.att.in_proj_bias", "self_attn.in_proj_bias"),
                     ("self_att.att.out_proj.weight", "self_attn.out_proj.weight"), ("self_att.att.out_proj.bias", "self_attn.out_proj.bias"),
                     ("pos_ffn.ffn.0.weight", "linear1.weight"), ("pos_ffn.ffn.0.bias", "linear1.bias"), ("pos_ffn.ffn.3.weight", "linear2.weight"),
                     ("pos_ffn.ffn.3.bias", "linear2.bias"), ("norm1.norm.weight", "norm1.weight"), ("norm1.norm.bias", "norm1.bias"),
                     ("norm2.norm.weight", "norm2.weight"), ("norm2.norm.bias", "norm2.bias")):
            own[t + b] = sd[s + a]
    own["norm.weight"], own["norm.bias"] = sd["encoder.norm.norm.weight"], sd["encoder.norm.norm.bias"]
    enc.load_state_dict(own, strict=True)
    enc.train()                                               # (dropout 0: the same function, and never torch's fused inference path)
    tokens = torch.randint(1, LM.V, (3, 13), generator=torch.Generator().manual_seed(5))
    tokens[1, 4] = tokens[1, 9] = 0
    U = tokens.shape[1]
    x = sd[LR.TABLE][tokens] * d ** 0.5 + sd[LR.PE][0, :U]
    causal = torch.triu(torch.full((U, U), float("-inf"), dtype=torch.float64), diagonal=1)
    pad = torch.zeros(tokens.shape, dtype=torch.float64).masked_fill(tokens == 0, float("-inf"))
    h = enc(x, mask=causal, src_key_padding_mask=pad)
    h = torch.nn.functional.linear(h, sd["output_proj.layers.0.w.weight"], sd["output_proj.layers.0.w.bias"])
    h = torch.nn.functional.layer_norm(h, (d,), sd["output_proj.layers.1.norm.weight"], sd["output_proj.layers.1.norm.bias"], 1e-6)
    want = torch.nn.functional.linear(h, sd["output_proj.layers.2.w.weight"], sd["output_proj.layers.2.w.bias"]).detach()
    got = LM.restated(name, m, "f64", torch.float32)(tokens)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 13, LM.V)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    unmasked = LM.restated(name, m, "f64", torch.float32)(tokens, mask_pad=False)
    assert torch.equal(unmasked[[0, 2]], got[[0, 2]]) and torch.equal(unmasked[1, :4], got[1, :4]) and not torch.equal(unmasked[1, 4:], got[1, 4:])
    z = got[0]
    s = LR.lm_score(z, 1.15, 0.6)
    assert float((s - 0.6 * torch.log_softmax(z / 1.15, -1)).abs().max()) == 0.0
    z[2, 3] = float("nan")
    z[4] = float("-inf")
    s = LR.lm_score(z, 1.15, 0.6)
    assert bool((s[[2, 4]] == float("-inf")).all()) and bool(torch.isfinite(s[[0, 1, 3]]).all())


class _Lin:
    def __init__(self, V=5, d=4):
        self.w = torch.nn.Linear(d, V)


_RECIPE = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, using_eos_threshold=False, length_normalization=True)


def test_lm_scorer_and_builder_take_the_recipes_arguments_and_refuse_by_name():
    from summarymixing_amd import decoders
    from summarymixing_amd.decoders.scorer import CTCScorer, ScorerBuilder, TransformerLMScorer, active
    assert decoders.TransformerLMScorer is TransformerLMScorer and "TransformerLMScorer" in decoders.__all__
    lm = _lm()
    assert lm.training
    s = TransformerLMScorer(language_model=lm, temperature=1.15)
    assert s.lm is lm and s.temperature == 1.15 and not lm.training, "the scorer puts the LM in eval mode"
    assert TransformerLMScorer(lm).temperature == 1.0
    with pytest.raises(TypeError, match="got Linear"):
        TransformerLMScorer(torch.nn.Linear(2, 2))
    for t in (0.0, -1.0):
        with pytest.raises(ValueError, match="temperature must be > 0"):
            TransformerLMScorer(lm, temperature=t)
    ctc = CTCScorer(eos_index=2, blank_index=0, ctc_fc=_Lin())
    b = ScorerBuilder(full_scorers=[s, ctc], weights={"ctc": 0.40, "transformerlm": 0.60})                # LibriSpeech's scorer_test_search
    assert b.ctc is ctc and b.ctc_weight == 0.4 and b.lm is s and b.lm_weight == 0.6 and active(b) is b
    b = ScorerBuilder(full_scorers=[s], weights={"transformerlm": 0.6})
    assert b.ctc is None and b.ctc_weight == 0.0 and b.lm is s and active(b) is b
    b = ScorerBuilder(full_scorers=[ctc], weights={"ctc": 0.4})
    assert b.lm is None and b.lm_weight == 0.0 and active(b) is b
    assert active(ScorerBuilder(full_scorers=[s], weights={"transformerlm": 0.0})) is None
    assert active(ScorerBuilder(full_scorers=[s, ctc], weights={"ctc": 0.0, "transformerlm": 0.0})) is None
    b = ScorerBuilder(full_scorers=[s, ctc], weights={"ctc": 0.4, "transformerlm": 0.0})
    assert active(b) is b and b.lm_weight == 0.0
    b = ScorerBuilder(full_scorers=[s, ctc], weights={"ctc": 0.0, "transformerlm": 0.5})
    assert active(b) is b and b.ctc_weight == 0.0
    with pytest.raises(NotImplementedError, match="'transformerlm'"):
        ScorerBuilder(full_scorers=[ctc], weights={"ctc": 0.4, "transformerlm": 0.6})
    with pytest.raises(NotImplementedError, match="'rnnlm'"):
        ScorerBuilder(full_scorers=[s], weights={"transformerlm": 0.6, "rnnlm": 0.2})
    with pytest.raises(NotImplementedError, match="exactly one CTCScorer, got 0"):
        ScorerBuilder(full_scorers=[s], weights={"transformerlm": 0.6, "ctc": 0.4})
    with pytest.raises(NotImplementedError, match="at most one TransformerLMScorer, got 2"):
        ScorerBuilder(full_scorers=[s, s], weights={"transformerlm": 0.6})
    with pytest.raises(ValueError, match="under 'transformerlm'"):
        ScorerBuilder(full_scorers=[s, ctc], weights={"ctc": 0.4})
    with pytest.raises(ValueError, match="under 'ctc'"):
        ScorerBuilder(full_scorers=[s, ctc], weights={"transformerlm": 0.6})
    for w in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="transformerlm weight"):
            ScorerBuilder(full_scorers=[s], weights={"transformerlm": w})
    with pytest.raises(NotImplementedError, match="partial_scorers"):
        ScorerBuilder(full_scorers=[s], partial_scorers=[ctc], weights={"transformerlm": 0.6, "ctc": 0.4})
    with pytest.raises(NotImplementedError, match="holds no scorer"):
        ScorerBuilder()

    class RNNLMScorer:
        pass

    class CoverageScorer:
        pass

    class LengthScorer:
        pass
    for cls in (RNNLMScorer, CoverageScorer, LengthScorer):
        with pytest.raises(NotImplementedError, match=f"{cls.__name__} in full_scorers"):
            ScorerBuilder(full_scorers=[s, cls()], weights={"transformerlm": 0.6})


def test_searchers_take_the_joint_builder_and_register_nothing():
    from summarymixing_amd.decoders import CTCScorer, S2SBeamSearcher, S2STransformerBeamSearcher, ScorerBuilder, TransformerLMScorer
    model, lin = torch.nn.Linear(4, 4), torch.nn.Linear(4, 3)
    b = ScorerBuilder(full_scorers=[TransformerLMScorer(_lm(), temperature=1.15), CTCScorer(eos_index=2, blank_index=0, ctc_fc=_Lin())],
                      weights={"ctc": 0.40, "transformerlm": 0.60})
    s = S2SBeamSearcher(modules=[model, lin], beam_size=66, scorer=b, temperature=1.15, **_RECIPE)                 # the recipe's test_search
    assert s.scorer is b and len(s.state_dict()) == 0 and list(s.parameters()) == [] and list(s.children()) == []
    with pytest.raises(NotImplementedError, match="a scorer"):
        S2STransformerBeamSearcher(modules=[model, lin], beam_size=1, scorer=b, **_RECIPE)
    with pytest.raises(NotImplementedError, match="got TransformerLMScorer"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, scorer=b.lm, **_RECIPE)


def test_lm_score_descriptor_matches_header_and_the_entry_refuses_before_any_launch():
    """The pointers are fake and never dereferenced: every case is refused on the host."""
    from summarymixing_amd import _lib
    A = _lib.LmScoreArgs
    assert ctypes.sizeof(A) == 96
    assert A.logits.offset == 0 and A.ldz.offset == 8 and A.extra.offset == 16 and A.lde.offset == 24 and A.score.offset == 32
    assert A.done.offset == 40 and A.n_tok.offset == 48 and A.inv_temp.offset == 56 and A.weight.offset == 64 and A.dtype.offset == 68
    assert A.B.offset == 72 and A.W.offset == 76 and A.V.offset == 80 and A.cap.offset == 84 and A.accumulate.offset == 88
    lib = _lib.lib()
    ptrs = [n for n, t in A._fields_ if t is ctypes.c_void_p]
    assert ptrs == ["logits", "extra", "score", "done", "n_tok"]

    def call(**kw):
        a = A(ldz=40, lde=40, inv_temp=1.0 / 1.15, weight=0.6, dtype=0, B=2, W=3, V=40, cap=8, accumulate=0,
              **{n: _BASE + i * 0x100000 for i, n in enumerate(ptrs)})
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.smx_lm_score(ctypes.byref(a), None)
    assert lib.smx_lm_score(None, None) == EINVAL
    for n in ptrs:
        assert call(**{n: None}) == EINVAL, n
    for kw in (dict(B=0), dict(W=0), dict(V=0), dict(cap=0), dict(ldz=39), dict(lde=39), dict(dtype=2), dict(inv_temp=0.0), dict(inv_temp=-1.0),
               dict(inv_temp=float("inf")), dict(inv_temp=float("nan")), dict(weight=0.0), dict(weight=-0.5), dict(weight=float("inf")),
               dict(weight=float("nan")), dict(accumulate=2), dict(B=1 << 20, W=128)):
        assert call(**kw) == EINVAL, kw
    assert call(B=1 << 20, W=128) == EINVAL and b"rows exceed" in lib.smx_last_error()

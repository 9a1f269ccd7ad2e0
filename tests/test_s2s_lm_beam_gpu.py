"""Beam search with the TransformerLM scorer (decoders.seq2seq.beam_search / CapturedS2SBeam / S2SBeamSearcher with
scorer=ScorerBuilder(full_scorers=[TransformerLMScorer, CTCScorer], ...)) end to end on the GPU: the three decoder models
of tests/_s2s_models.py with the CTC heads of tests/test_s2s_ctc_beam_gpu.py, each paired with one LM of tests/_lm_models.py, B = 3,
W = 3, 12 steps, LM temperature 1.15.

a. float32: the pool - tokens, order, lengths - equals that of the float64 search (tests/_s2s_beam_ref.py) driven by the float64
   decoder, the float64 LM over whole prefixes (run with no key-padding mask: the cached step's definition, §I.24) and the float64 CTC
   scorer, LM-only with weight 0.6 and CTC 0.4 + LM 0.6.  Admission is §I.22's: every float64 gap between adjacent ranks 1 .. W + 1 at
   least 8 (n + 1) x the float32 error of the candidate scores lp + extra, measured here from the float32 ATen chains carried along
   the same hypotheses (decoder logits, LM logits, the torch.logaddexp recursion).  None may be left out: the LM seeds below were
   chosen on the CPU with the float64 reference alone - per model the first seed whose smallest gap, in both configurations, keeps
   2.5 x that margin with the error measured from the float32 chains on the CPU.  The test counts the left-out (utterance, step)
   pairs and asserts zero.  Final scores and sums within 4 x the measured error (a sum of L steps: L x).
b. a transformerlm weight of 0 next to CTC gives the CTC search's bits; a weight of 0 alone, or scorer=None, the plain search's.
c. CapturedS2SBeam with both scorers equals the eager search bit for bit, for two utterances through one capture; an utterance alone
   equals itself in the batch.
d. the LM changes the pool of at least one utterance on every model, against CTC-only (asserted in a.).
e. S2SBeamSearcher with the recipe's test_search block returns the best pool entry, from one host copy."""
import contextlib
import functools
import math

import pytest
import torch

from tests import _ctc_prefix_ref as P
from tests import _lm_models as LM
from tests import _s2s_models as M
from tests import _transformerlm_ref as LR
from tests._util import report

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
BOS, EOS, BLANK = 1, 2, 0
SEEDS = {"d64-pre": 3, "d128-h2-post": 4, "d512-pre": 5}           # the decoders, their eos push and their CTC heads are those of
PUSH = {"d64-pre": 3.0, "d128-h2-post": 3.0, "d512-pre": 4.0}       # tests/test_s2s_ctc_beam_gpu.py
CTC_SEEDS = {"d64-pre": 47, "d128-h2-post": 75, "d512-pre": 27}
BLANK_BIAS = 8.0
PAIR = {"d64-pre": "lm-d64-post", "d128-h2-post": "lm-d128-h2-pre", "d512-pre": "lm-d768-h12-post"}
LM_SEEDS = {"d64-pre": 2, "d128-h2-post": 1, "d512-pre": 0}         # chosen on the float64 reference (docstring, a.)
STEPS, MIN_STEPS, W = 12, 2, 3
W_CTC, W_LM, T_LM = 0.4, 0.6, 1.15
MODES = {"lm": (0.0, W_LM), "ctc+lm": (W_CTC, W_LM)}


def ctc_head(name, d):
    from summarymixing_amd.nnet.linear import Linear
    g = torch.Generator().manual_seed(CTC_SEEDS[name])
    head = Linear(n_neurons=M.V, input_size=d)
    with torch.no_grad():
        head.w.weight.copy_(torch.randn(M.V, d, generator=g) * 2.0 / math.sqrt(d))
        head.w.bias.copy_(torch.randn(M.V, generator=g) * 0.1)
        head.w.bias[BLANK] += BLANK_BIAS
    return head


@functools.lru_cache(maxsize=None)
def _model(name, dt):
    m, lin, mem, enc_len = M.build(name, DT[dt], SEEDS[name])
    return m, lin, mem, enc_len, ctc_head(name, M.MODELS[name][0]).cuda(), LM.build(PAIR[name], DT[dt], LM_SEEDS[name])


def _builder(head, lm, w_ctc=W_CTC, w_lm=W_LM):
    from summarymixing_amd.decoders import CTCScorer, ScorerBuilder, TransformerLMScorer
    full, weights = [], {}
    if lm is not None:
        full.append(TransformerLMScorer(lm, temperature=T_LM))
        weights["transformerlm"] = w_lm
    if head is not None:
        full.append(CTCScorer(eos_index=EOS, blank_index=BLANK, ctc_fc=head))
        weights["ctc"] = w_ctc
    return ScorerBuilder(full_scorers=full, weights=weights)


@contextlib.contextmanager
def _pushed(lin, by):
    with torch.no_grad():
        old = lin.w.bias[EOS].item()
        lin.w.bias[EOS] += by
    try:
        yield
    finally:
        with torch.no_grad():
            lin.w.bias[EOS] = old


def _snap(r):
    return tuple(t.clone() for t in r[:-1])


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def reference_search(mode, dec64, dec32, lm64, lm32, x64, x32):
    """The float64 search of one configuration with the float32 chains carried along the same hypotheses.  dec*(tokens (B, U)) ->
    (prediction, logits (B, U, V)); lm*(tokens (R, U)) -> logits (R, U, V), run without a key-padding mask; x* (B, S, V) the CTC
    log-probabilities.  -> (BeamRef, trace, the float64 extras, the shadow's (extra, lp, float64 lp) per step)."""
    w_ctc, w_lm = MODES[mode]

    def rows(fn):
        def logits_of(prefixes):
            out = torch.empty(M.B * W, M.V, dtype=torch.float64)
            for i in range(W):                                # slot i of the B utterances: the restated decoder takes B rows
                out[i::W] = fn(prefixes[i::W])[1][:, -1].double().cpu()
            return out
        return logits_of
    c64 = P.PrefixScorer(x64, M.ENC_LEN, BLANK, EOS, w_ctc, W) if w_ctc > 0.0 else None
    c32 = P.PrefixScorer(x32, M.ENC_LEN, BLANK, EOS, w_ctc, W, dtype=torch.float32) if w_ctc > 0.0 else None
    sc = LR.JointScorer(lm64, M.B, W, M.V, BOS, EOS, w_lm, T_LM, ctc=c64)
    sh = LR.JointScorer(lm32, M.B, W, M.V, BOS, EOS, w_lm, T_LM, ctc=c32, dtype=torch.float32)
    sh.logits_of = rows(dec32)
    ref, trace, extras, _ = P.search(rows(dec64), sc, M.B, W, M.V, BOS, EOS, MIN_STEPS, STEPS, shadow=sh)
    return ref, trace, extras, sh.extras


def margins(trace, extras, shadow_extras):
    """-> (the float32 error of lp + extra, of lp alone, the gaps [(utterance, step, gap)] that are no exact ties)."""
    err = err_lp = 0.0
    for ex, (sx, slp, lp) in zip(extras, shadow_extras):
        a, b = (slp + sx).double(), lp + ex
        fin = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), fin)
        err = max(err, float((a[fin] - b[fin]).abs().max()))
        err_lp = max(err_lp, float((slp.double() - lp)[torch.isfinite(lp)].abs().max()))
    gaps = [(b, n, g) for n, st in enumerate(trace) for b, o in enumerate(st) if o is not None
            for g, tw in zip(o["gaps"], o["twins"]) if not (g == 0.0 and tw)]
    return err, err_lp, gaps


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(M.MODELS))
def test_fp32_pool_equals_the_float64_search_with_the_float64_scorers(name, mode):
    from summarymixing_amd.decoders import beam_search
    m, lin, mem, enc_len, head, lm = _model(name, "f32")
    w_ctc, w_lm = MODES[mode]
    with _pushed(lin, PUSH[name]), torch.no_grad():
        r = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, scorer=_builder(head if w_ctc > 0.0 else None, lm))
        tokens, lengths, scores, sums, lps, counts = (t.cpu() for t in _snap(r))
        if w_ctc > 0.0:
            base = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, scorer=_builder(head, None))
        else:
            base = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W)
        base_tokens = base.tokens.cpu().clone()
        Wh, bh = head.w.weight.detach(), head.w.bias.detach()
        x64 = torch.log_softmax(torch.nn.functional.linear(mem.double().cpu(), Wh.double().cpu(), bh.double().cpu()), -1)
        x32 = torch.log_softmax(torch.nn.functional.linear(mem, Wh, bh), -1).cpu()
        l64, l32 = LM.restated(PAIR[name], lm, "f64", torch.float32), LM.restated(PAIR[name], lm, "aten", torch.float32)
        ref, trace, extras, shadow = reference_search(mode, M.restated(name, m, lin, mem, "f64", torch.float32),
                                                      M.restated(name, m, lin, mem, "aten", torch.float32),
                                                      lambda t: l64(t, mask_pad=False), lambda t: l32(t, mask_pad=False), x64, x32)
    err, err_lp, gaps = margins(trace, extras, shadow)
    left_out = sorted({(b, n) for b, n, g in gaps if g < 8.0 * (n + 1) * err})
    worst = min(g / (8.0 * (n + 1)) for _, n, g in gaps)
    print(f"s2s lm beam {name} {mode}: float32 error of lp + extra {err:.2e} (lp alone {err_lp:.2e}), smallest float64 gap / (8 (n + 1)) {worst:.2e}, "
          f"{len(left_out)} of {sum(o is not None for st in trace for o in st)} (utterance, step) left out")
    report(f"s2s_lm_beam margin {name} {mode}", {"f32_err": err, "f32_err_lp": err_lp, "min_gap_over_8n1": worst, "left_out": len(left_out), "steps": len(trace)})
    assert err > 0.0 and len(left_out) == 0, "an (utterance, step) falls below the margin: the comparison would leave it out"
    worst_sum = worst_final = worst_lp = 0.0
    changed = False
    for b in range(M.B):
        res = ref.result(b)
        assert int(counts[b]) == len(res) == W
        for k, e in enumerate(res):
            L = len(e["tokens"])
            assert tokens[b, k].tolist() == e["tokens"] + [-1] * (STEPS - L), (b, k, "the pool's tokens and order")
            assert int(lengths[b, k]) == L
            worst_lp = max(worst_lp, max(abs(float(lps[b, k, j]) - e["lps"][j]) for j in range(L)))
            worst_sum = max(worst_sum, abs(float(sums[b, k]) - e["sum"]) / L)
            worst_final = max(worst_final, abs(float(scores[b, k]) - e["final"]))
        changed = changed or not torch.equal(tokens[b], base_tokens[b])
    print(f"s2s lm beam {name} {mode}: sum error per step {worst_sum:.2e}, final {worst_final:.2e}, bar {4 * err:.2e}; stored lp {worst_lp:.2e}, "
          f"bar {4 * err_lp:.2e}")
    report(f"s2s_lm_beam scores {name} {mode}", {"errors": {"sum_per_step": {"ours": worst_sum, "bar": 4 * err}, "final": {"ours": worst_final, "bar": 4 * err},
                                                          "lp": {"ours": worst_lp, "bar": 4 * err_lp}}})
    assert worst_sum <= 4.0 * err and worst_final <= 4.0 * err and worst_lp <= 4.0 * err_lp
    assert changed, "the LM changes no pool on this model: the comparison shows nothing"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_weight_of_zero_drops_the_lm_scorer_bit_for_bit(dt):
    from summarymixing_amd.decoders import beam_search
    name = "d128-h2-post"
    m, lin, mem, enc_len, head, lm = _model(name, dt)
    with _pushed(lin, PUSH[name]):
        kw = dict(temperature=1.15)
        args = (m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W)
        plain = _snap(beam_search(*args, **kw))
        ctc = _snap(beam_search(*args, scorer=_builder(head, None), **kw))
        joint = _snap(beam_search(*args, scorer=_builder(head, lm), **kw))
        alone = _snap(beam_search(*args, scorer=_builder(None, lm), **kw))
        assert not _same(joint, ctc) and not _same(alone, plain) and not _same(joint, alone)
        st = m.make_decode_state(mem, enc_len, STEPS, beam=W)
        assert _same(_snap(beam_search(*args, scorer=_builder(head, lm, w_lm=0.0), state=st, **kw)), ctc)
        assert hasattr(st, "ctc") and not hasattr(st, "lm"), "a weight of 0 drops the LM scorer on its own: nothing of its is made or launched"
        st = m.make_decode_state(mem, enc_len, STEPS, beam=W)
        assert _same(_snap(beam_search(*args, scorer=_builder(None, lm, w_lm=0.0), state=st, **kw)), plain)
        assert not hasattr(st, "ctc") and not hasattr(st, "lm")
        assert _same(_snap(beam_search(*args, scorer=None, **kw)), plain)
        st = m.make_decode_state(mem, enc_len, STEPS, beam=W)
        assert _same(_snap(beam_search(*args, scorer=_builder(head, lm, w_ctc=0.0), state=st, **kw)), alone)
        assert hasattr(st, "lm") and not hasattr(st, "ctc"), "so does a ctc weight of 0 next to the LM"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_captured_search_with_both_scorers_equals_eager_and_a_batch_does_not_matter(dt):
    from summarymixing_amd.decoders import CapturedS2SBeam, beam_search
    name = "d64-pre"
    m, lin, mem, enc_len, head, lm = _model(name, dt)
    sb = _builder(head, lm)
    with _pushed(lin, PUSH[name]):
        mem2 = torch.randn(mem.shape, generator=torch.Generator().manual_seed(11)).to(DT[dt]).cuda()
        utts = [(mem, enc_len), (mem2, None)]
        kw = dict(temperature=1.15, length_normalization=True)
        eager = [_snap(beam_search(m, lin, x, n, BOS, EOS, MIN_STEPS, STEPS, W, scorer=sb, **kw)) for x, n in utts]
        assert not _same(eager[0], eager[1])
        for (x, n), e in zip(utts, eager):                    # two runs agree bit for bit
            assert _same(_snap(beam_search(m, lin, x, n, BOS, EOS, MIN_STEPS, STEPS, W, scorer=sb, poll_every=1, **kw)), e)
        cap = CapturedS2SBeam(m, lin, M.B, M.S, STEPS, DT[dt], BOS, EOS, W, min_steps=MIN_STEPS, scorer=sb, **kw)
        for poll in (8, 1):
            for (x, n), e in zip(utts, eager):                # both utterances through ONE capture, in turn
                assert _same(_snap(cap.search(x, n, poll_every=poll)), e), poll
        for b in range(M.B):                                  # an utterance alone = the utterance inside the batch
            alone = _snap(beam_search(m, lin, mem[b:b + 1], enc_len[b:b + 1], BOS, EOS, MIN_STEPS, STEPS, W, scorer=sb, **kw))
            assert _same(alone, tuple(t[b:b + 1] for t in eager[0])), b


def test_the_searcher_with_the_recipes_test_search_block_returns_the_best_pool_entry():
    from summarymixing_amd.decoders import CTCScorer, S2SBeamSearcher, ScorerBuilder, TransformerLMScorer, beam_search
    name = "d64-pre"
    m, lin, mem, enc_len, head, lm = _model(name, "f32")
    wav_len = enc_len.float() / M.S
    # the recipe's blocks: transformerlm_scorer, ctc_scorer, scorer_test_search, test_search
    transformerlm_scorer = TransformerLMScorer(language_model=lm, temperature=1.15)
    ctc_scorer = CTCScorer(eos_index=EOS, blank_index=BLANK, ctc_fc=head)
    sb = ScorerBuilder(full_scorers=[transformerlm_scorer, ctc_scorer], weights={"ctc": .4, "transformerlm": .6})
    with _pushed(lin, PUSH[name]):
        ratio, ratio_min = STEPS / M.S + 1e-6, MIN_STEPS / M.S + 1e-6
        s = S2SBeamSearcher(modules=[m, lin], bos_index=BOS, eos_index=EOS, min_decode_ratio=ratio_min, max_decode_ratio=ratio, beam_size=W,
                            scorer=sb, temperature=1.15, using_eos_threshold=False, length_normalization=True)
        assert int(M.S * ratio) == STEPS and int(M.S * ratio_min) == MIN_STEPS
        hyps, lengths, scores, log_probs = s(mem, wav_len)
        r = _snap(beam_search(m, lin, mem, torch.round(wav_len * M.S), BOS, EOS, MIN_STEPS, STEPS, W, temperature=1.15, scorer=sb))
        ctc_only = S2SBeamSearcher([m, lin], BOS, EOS, ratio_min, ratio, beam_size=W, temperature=1.15, using_eos_threshold=False, length_normalization=True,
                                   scorer=ScorerBuilder(full_scorers=[ctc_scorer], weights={"ctc": .4}))(mem, wav_len)
    assert tuple(log_probs.shape) == (M.B, STEPS) and lengths.tolist() == [len(h) for h in hyps]
    for b in range(M.B):
        row = r[0][b, 0, :int(r[1][b, 0])].tolist()
        assert hyps[b] == (row[:-1] if row[-1] == EOS else row) and EOS not in hyps[b]
    assert torch.equal(scores, r[2][:, 0].cpu()) and torch.equal(log_probs, r[4][:, 0].cpu())
    assert hyps != ctc_only[0], "the LM changes the best hypothesis of some utterance"
    assert len(s.state_dict()) == 0

"""Joint CTC / attention beam search (decoders.seq2seq.beam_search / CapturedS2SBeam / S2SBeamSearcher with scorer=ScorerBuilder(...),
DESIGN.md §I.23) end to end on the GPU, on the three models of tests/_s2s_models.py with a CTC head, B = 3, W = 3, weight 0.4.

a. float32: the pool - tokens, order, lengths - equals that of the float64 search (tests/_s2s_beam_ref.py) over the float64 decoder
   on whole prefixes with the float64 scorer (tests/_ctc_prefix_ref.py).  Admission is §I.22's: every float64 gap between adjacent
   ranks 1 .. W + 1 at least 8 (n + 1) x the float32 error of the candidate scores lp + extra, measured here from the float32 ATen
   chain's logits and the float32 torch.logaddexp recursion carried along the same hypotheses.  The CTC heads' seeds were chosen on
   the CPU, with the float64 reference alone, so that no (utterance, step) is left out; the test counts them and asserts none is.
   Final scores and sums within 4 x that float32 error (a sum of L steps: L x).
b. a ctc weight of 0 and scorer=None give today's beam_search bit for bit.
c. CapturedS2SBeam with the scorer equals the eager search bit for bit, for two utterances through one capture; an utterance alone
   equals itself in the batch.
d. the scorer changes the pool of at least one utterance on every model (else the comparison shows nothing).
e. S2SBeamSearcher(scorer=ScorerBuilder(...)).forward returns the best pool entry, from one host copy."""
import contextlib
import functools
import math

import pytest
import torch

from tests import _ctc_prefix_ref as P
from tests import _s2s_models as M
from tests._util import report

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
BOS, EOS, BLANK = 1, 2, 0
SEEDS = {"d64-pre": 3, "d128-h2-post": 4, "d512-pre": 5}
PUSH = {"d64-pre": 3.0, "d128-h2-post": 3.0, "d512-pre": 4.0}       # added to seq_lin's eos bias, as tests/test_s2s_beam_search_gpu.py does
CTC_SEEDS = {"d64-pre": 47, "d128-h2-post": 75, "d512-pre": 27}     # the CTC heads: chosen on the float64 reference (docstring, a.)
BLANK_BIAS = 8.0                                                      # blank dominates most frames, as in a trained head: eos can win
STEPS, MIN_STEPS, W, WEIGHT = 12, 2, 3, 0.4


@functools.lru_cache(maxsize=None)
def _model(name, dt):
    from summarymixing_amd.nnet.linear import Linear
    m, lin, mem, enc_len = M.build(name, DT[dt], SEEDS[name])
    d = M.MODELS[name][0]
    g = torch.Generator().manual_seed(CTC_SEEDS[name])
    head = Linear(n_neurons=M.V, input_size=d)
    with torch.no_grad():
        head.w.weight.copy_(torch.randn(M.V, d, generator=g) * 2.0 / math.sqrt(d))
        head.w.bias.copy_(torch.randn(M.V, generator=g) * 0.1)
        head.w.bias[BLANK] += BLANK_BIAS
    return m, lin, mem, enc_len, head.cuda()


def _builder(head, weight=WEIGHT):
    from summarymixing_amd.decoders import CTCScorer, ScorerBuilder
    return ScorerBuilder(full_scorers=[CTCScorer(eos_index=EOS, blank_index=BLANK, ctc_fc=head)], weights={"ctc": weight})


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


@pytest.mark.parametrize("name", list(M.MODELS))
def test_fp32_pool_equals_the_float64_search_with_the_float64_scorer(name):
    from summarymixing_amd.decoders import beam_search
    m, lin, mem, enc_len, head = _model(name, "f32")
    with _pushed(lin, PUSH[name]), torch.no_grad():
        r = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, scorer=_builder(head))
        tokens, lengths, scores, sums, lps, counts = (t.cpu() for t in _snap(r))
        plain = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W)
        plain_tokens = plain.tokens.cpu().clone()
        f64 = M.restated(name, m, lin, mem, "f64", torch.float32)
        aten = M.restated(name, m, lin, mem, "aten", torch.float32)
        Wh, bh = head.w.weight.detach(), head.w.bias.detach()
        x64 = torch.log_softmax(torch.nn.functional.linear(mem.double().cpu(), Wh.double().cpu(), bh.double().cpu()), -1)
        x32 = torch.log_softmax(torch.nn.functional.linear(mem, Wh, bh), -1).cpu()

        def rows(fn):
            def logits_of(prefixes):
                out = torch.empty(M.B * W, M.V, dtype=torch.float64)
                for i in range(W):                             # slot i of the B utterances: the restated decoder takes B rows
                    out[i::W] = fn(prefixes[i::W])[1][:, -1].double().cpu()
                return out
            return logits_of
        sc = P.PrefixScorer(x64, M.ENC_LEN, BLANK, EOS, WEIGHT, W)
        sh = P.PrefixScorer(x32, M.ENC_LEN, BLANK, EOS, WEIGHT, W, dtype=torch.float32)
        sh.logits_of = rows(aten)
        ref, trace, extras, _ = P.search(rows(f64), sc, M.B, W, M.V, BOS, EOS, MIN_STEPS, STEPS, shadow=sh)
    err = err_lp = 0.0
    for ex, (sx, slp, lp) in zip(extras, sh.extras):           # the float32 error of the candidate scores, and of lp alone
        a, b = (slp + sx).double(), lp + ex
        fin = torch.isfinite(b)
        assert torch.equal(torch.isfinite(a), fin)
        err = max(err, float((a[fin] - b[fin]).abs().max()))
        err_lp = max(err_lp, float((slp.double() - lp)[torch.isfinite(lp)].abs().max()))
    gaps = [(b, n, g) for n, st in enumerate(trace) for b, o in enumerate(st) if o is not None
            for g, tw in zip(o["gaps"], o["twins"]) if not (g == 0.0 and tw)]
    left_out = sorted({(b, n) for b, n, g in gaps if g < 8.0 * (n + 1) * err})
    worst = min(g / (8.0 * (n + 1)) for _, n, g in gaps)
    print(f"s2s ctc beam {name}: float32 error of lp + extra {err:.2e} (lp alone {err_lp:.2e}), smallest float64 gap / (8 (n + 1)) {worst:.2e}, "
          f"{len(left_out)} of {sum(o is not None for st in trace for o in st)} (utterance, step) left out")
    report(f"s2s_ctc_beam margin {name}", {"f32_err": err, "f32_err_lp": err_lp, "min_gap_over_8n1": worst, "left_out": len(left_out), "steps": len(trace)})
    assert err > 0.0 and not left_out, "an (utterance, step) falls below the margin: the comparison would leave it out"
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
        changed = changed or not torch.equal(tokens[b], plain_tokens[b])
    print(f"s2s ctc beam {name}: sum error per step {worst_sum:.2e}, final {worst_final:.2e}, bar {4 * err:.2e}; stored lp {worst_lp:.2e}, "
          f"bar {4 * err_lp:.2e}")
    report(f"s2s_ctc_beam scores {name}", {"errors": {"sum_per_step": {"ours": worst_sum, "bar": 4 * err}, "final": {"ours": worst_final, "bar": 4 * err},
                                                    "lp": {"ours": worst_lp, "bar": 4 * err_lp}}})
    assert worst_sum <= 4.0 * err and worst_final <= 4.0 * err and worst_lp <= 4.0 * err_lp
    assert changed, "the scorer changes no pool on this model: the comparison shows nothing"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_weight_zero_and_no_scorer_are_the_plain_search_bit_for_bit(dt):
    from summarymixing_amd.decoders import beam_search
    name = "d128-h2-post"
    m, lin, mem, enc_len, head = _model(name, dt)
    with _pushed(lin, PUSH[name]):
        kw = dict(temperature=1.15)
        want = _snap(beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, **kw))
        scored = _snap(beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, scorer=_builder(head), **kw))
        assert not _same(scored, want)
        assert _same(_snap(beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, scorer=None, **kw)), want)
        st = m.make_decode_state(mem, enc_len, STEPS, beam=W)
        zero = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, scorer=_builder(head, 0.0), state=st, **kw)
        assert _same(_snap(zero), want) and not hasattr(st, "ctc"), "a weight of 0 drops the scorer: nothing of its own is made or launched"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_captured_search_with_the_scorer_equals_eager_and_a_batch_does_not_matter(dt):
    from summarymixing_amd.decoders import CapturedS2SBeam, beam_search
    name = "d64-pre"
    m, lin, mem, enc_len, head = _model(name, dt)
    sb = _builder(head)
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


def test_the_searcher_with_a_builder_returns_the_best_pool_entry():
    from summarymixing_amd.decoders import S2SBeamSearcher, beam_search
    name = "d64-pre"
    m, lin, mem, enc_len, head = _model(name, "f32")
    wav_len = enc_len.float() / M.S
    sb = _builder(head)
    with _pushed(lin, PUSH[name]):
        ratio, ratio_min = STEPS / M.S + 1e-6, MIN_STEPS / M.S + 1e-6
        s = S2SBeamSearcher([m, lin], BOS, EOS, ratio_min, ratio, beam_size=W, scorer=sb, using_eos_threshold=False, length_normalization=True)
        assert int(M.S * ratio) == STEPS and int(M.S * ratio_min) == MIN_STEPS
        hyps, lengths, scores, log_probs = s(mem, wav_len)
        r = _snap(beam_search(m, lin, mem, torch.round(wav_len * M.S), BOS, EOS, MIN_STEPS, STEPS, W, scorer=sb))
        plain = S2SBeamSearcher([m, lin], BOS, EOS, ratio_min, ratio, beam_size=W, using_eos_threshold=False, length_normalization=True)(mem, wav_len)
    assert tuple(log_probs.shape) == (M.B, STEPS) and lengths.tolist() == [len(h) for h in hyps]
    for b in range(M.B):
        row = r[0][b, 0, :int(r[1][b, 0])].tolist()
        assert hyps[b] == (row[:-1] if row[-1] == EOS else row) and EOS not in hyps[b]
    assert torch.equal(scores, r[2][:, 0].cpu()) and torch.equal(log_probs, r[4][:, 0].cpu())
    assert hyps != plain[0], "the scorer changes the best hypothesis of some utterance"
    assert len(s.state_dict()) == 0

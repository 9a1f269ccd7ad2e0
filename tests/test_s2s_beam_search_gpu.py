"""The seq2seq beam search (summarymixing_amd/decoders/seq2seq.py: beam_search, CapturedS2SBeam, S2SBeamSearcher) end to end on the GPU,
on the three models of tests/_s2s_models.py.

a. W = 1 is the greedy search: the same bits in tokens, counts, log-probabilities and the raw score, both dtypes.
b. float32, W = 3, B = 3 with ENC_LEN: the pool - tokens, order, lengths - equals that of the float64 restatement of the search
   (tests/_s2s_beam_ref.py) driven by the float64 decoder over whole prefixes, no cache.  Every (utterance, step) must be admissible:
   every float64 gap between adjacent ranks 1 .. W + 1 at least 8 x the largest logit error of the float32 ATen chain on the same
   prefixes, measured here; the eos bias of each model was chosen on the CPU so that none falls below, and the test asserts that.
c. both dtypes: the same bits as a host loop that runs the PLAIN decode_step over B W rows whose caches are physically reordered
   (index_select by parent) after every step, with the memory replicated W times, then seq_lin and the selection kernel (held to the
   reference in tests/test_s2s_beam_select_gpu.py) on a state of its own: the indexed cache against the copied one.
d. CapturedS2SBeam equals the eager search bit for bit; two runs agree; an utterance alone equals itself in the batch; min_decode_ratio
   delays eos; length normalisation changes the ranking of a case chosen so that it does; S2SBeamSearcher returns the pool's best;
   decode, greedy_search and S2STransformerBeamSearcher(beam_size=1) give the same bits before and after beam searches."""
import contextlib
import functools

import pytest
import torch

from tests import _s2s_beam_ref as R
from tests import _s2s_models as M
from tests._util import report

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
BOS, EOS = 1, 2
SEEDS = {"d64-pre": 3, "d128-h2-post": 4, "d512-pre": 5}
PUSH = {"d64-pre": 3.0, "d128-h2-post": 3.0, "d512-pre": 4.0}       # added to seq_lin's eos bias: hypotheses end at different steps
STEPS, MIN_STEPS, W = 12, 2, 3


@functools.lru_cache(maxsize=None)
def _model(name, dt):
    return M.build(name, DT[dt], SEEDS[name])


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


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(M.MODELS))
def test_beam_of_one_is_the_greedy_search_bit_for_bit(name, dt):
    from summarymixing_amd.decoders import beam_search, greedy_search
    m, lin, mem, enc_len = _model(name, dt)
    for eos, push, steps in ((EOS, 3.0, 24), (M.V + 3, 0.0, 20)):      # rows that stop at different steps; rows that run to the cap
        with _pushed(lin, push):
            g = tuple(t.clone() for t in greedy_search(m, lin, mem, enc_len, BOS, eos, MIN_STEPS, steps, temperature=1.15)[:4])
            for norm in (True, False):
                b = beam_search(m, lin, mem, enc_len, BOS, eos, MIN_STEPS, steps, 1, temperature=1.15, length_normalization=norm)
                assert b.counts.tolist() == [1] * M.B
                assert _same((b.tokens[:, 0], b.lengths[:, 0], b.sums[:, 0], b.log_probs[:, 0]), g), (eos, norm)
        if eos == EOS and name == "d64-pre":
            assert len({int(c) for c in g[1]}) > 1, "the rows stop at different steps"


def _f64_search(name, m, lin, mem, norm=True, min_steps=MIN_STEPS):
    f64 = M.restated(name, m, lin, mem, "f64", torch.float32)
    fed = []

    def logits_of(prefixes):
        fed.append(prefixes)
        out = torch.empty(M.B * W, M.V, dtype=torch.float64)
        for i in range(W):                                     # slot i of the B utterances: the restated decoder takes B rows
            out[i::W] = f64(prefixes[i::W])[1][:, -1]
        return out
    ref, trace = R.search(logits_of, M.B, W, M.V, BOS, EOS, min_steps, STEPS, 1.0, norm)
    return ref, trace, fed


@pytest.mark.parametrize("name", list(M.MODELS))
def test_fp32_pool_equals_the_float64_search_over_prefixes(name):
    from summarymixing_amd.decoders import beam_search
    m, lin, mem, enc_len = _model(name, "f32")
    with _pushed(lin, PUSH[name]):
        r = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W)
        tokens, lengths, scores, sums, lps, counts = (t.cpu() for t in _snap(r))
        ref, trace, fed = _f64_search(name, m, lin, mem)
        aten = M.restated(name, m, lin, mem, "aten", torch.float32)
        f64 = M.restated(name, m, lin, mem, "f64", torch.float32)
        err = 0.0
        for prefixes in fed:                                   # the float32 ATen chain's logit error on the prefixes the search fed
            for i in range(W):
                err = max(err, float((aten(prefixes[i::W])[1][:, -1].double().cpu() - f64(prefixes[i::W])[1][:, -1]).abs().max()))
    gaps = [(b, n, g) for n, st in enumerate(trace) for b, o in enumerate(st) if o is not None
            for g, tw in zip(o["gaps"], o["twins"]) if not (g == 0.0 and tw)]
    smallest = min(g for _, _, g in gaps)
    print(f"s2s beam {name}: float32 ATen logit error {err:.2e}, smallest float64 gap over ranks 1..{W + 1} {smallest:.2e} ({len(trace)} steps)")
    report(f"s2s_beam_search margin {name}", {"aten_logit_err": err, "min_gap": smallest, "steps": len(trace)})
    assert err > 0.0 and all(g >= 8.0 * err for _, _, g in gaps), "an (utterance, step) falls below the margin: the comparison would leave it out"
    worst_lp = 0.0
    for b in range(M.B):
        res = ref.result(b)
        assert int(counts[b]) == len(res) == W
        for k, e in enumerate(res):
            L = len(e["tokens"])
            assert tokens[b, k].tolist() == e["tokens"] + [-1] * (STEPS - L), (b, k, "the pool's tokens and order")
            assert int(lengths[b, k]) == L
            worst_lp = max(worst_lp, max(abs(float(lps[b, k, j]) - e["lps"][j]) for j in range(L)))
            assert abs(float(sums[b, k]) - e["sum"]) <= 4.0 * 2.0 * err * L, "a sum of L log-probabilities, each off by two logit errors at most"
            assert abs(float(scores[b, k]) - e["final"]) <= 4.0 * 2.0 * err
    print(f"s2s beam {name}: log-probability error {worst_lp:.2e}, bar 4 x 2 x the ATen logit error {8.0 * err:.2e}")
    report(f"s2s_beam_search lp {name}", {"errors": {"lp": {"ours": worst_lp, "bar": 8.0 * err}}})
    assert worst_lp <= 8.0 * err


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(M.MODELS))
def test_same_bits_as_a_host_loop_over_physically_reordered_caches(name, dt):
    from summarymixing_amd import ops
    from summarymixing_amd.decoders import beam_search
    from summarymixing_amd.lobes.models.transformer.Transformer import DecodeState
    m, lin, mem, enc_len = _model(name, dt)
    rows = M.B * W
    with _pushed(lin, PUSH[name]), torch.no_grad():
        want = _snap(beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W))
        plain = m.make_decode_state(mem.repeat_interleave(W, 0), enc_len.repeat_interleave(W), max_steps=STEPS)     # B W independent rows
        sel = DecodeState(M.B, 1, STEPS, 1, 64, 0, torch.float32, torch.float32, "cuda", beam=W)                    # the selection's own state
        sel.tok.fill_(BOS)
        for _ in range(STEPS):
            n_before = sel.n_tok.cpu()
            was_done = sel.done.cpu()
            plain.done.copy_(sel.row_done)
            z = lin(m.decode_step(sel.tok, plain))
            ops.s2s_beam_select(z, sel, EOS, MIN_STEPS, 1.0, True)
            # the caches follow the beams PHYSICALLY: row r <- its parent's row (a dead or finished row keeps its own)
            parent = torch.arange(rows)
            anc, score = sel.anc.cpu(), sel.score.cpu()
            for r in range(rows):
                b = r // W
                if not bool(was_done[b]) and float(score[r]) > float("-inf"):
                    parent[r] = int(anc[r, int(n_before[b])])
            idx = parent.cuda()
            plain.self_kv = [kv.index_select(0, idx) for kv in plain.self_kv]
            if bool(sel.done.all()):
                break
    got = (sel.res_tokens, sel.res_len, sel.res_final, sel.res_sum, sel.res_logp, sel.pool_cnt)
    assert _same(got, want)
    assert bool((want[1] > 0).all()) and torch.isfinite(want[2]).all()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_captured_search_equals_eager_two_runs_agree_and_a_batch_does_not_matter(dt):
    from summarymixing_amd.decoders import CapturedS2SBeam, beam_search
    name = "d64-pre"
    m, lin, mem, enc_len = _model(name, dt)
    with _pushed(lin, PUSH[name]):
        mem2 = torch.randn(mem.shape, generator=torch.Generator().manual_seed(11)).to(DT[dt]).cuda()
        utts = [(mem, enc_len), (mem2, None)]
        kw = dict(temperature=1.15, length_normalization=True)
        eager = [_snap(beam_search(m, lin, x, n, BOS, EOS, MIN_STEPS, STEPS, W, **kw)) for x, n in utts]
        assert not _same(eager[0], eager[1])
        for poll in (1, 0):
            for (x, n), e in zip(utts, eager):                # two runs agree bit for bit, however often the host looks
                assert _same(_snap(beam_search(m, lin, x, n, BOS, EOS, MIN_STEPS, STEPS, W, poll_every=poll, **kw)), e), poll
        cap = CapturedS2SBeam(m, lin, M.B, M.S, STEPS, DT[dt], BOS, EOS, W, min_steps=MIN_STEPS, **kw)
        for poll in (8, 1):
            for (x, n), e in zip(utts, eager):                # both utterances through ONE capture, in turn
                assert _same(_snap(cap.search(x, n, poll_every=poll)), e), poll
        for b in range(M.B):                                  # an utterance alone = the utterance inside the batch
            alone = _snap(beam_search(m, lin, mem[b:b + 1], enc_len[b:b + 1], BOS, EOS, MIN_STEPS, STEPS, W, **kw))
            assert _same(alone, tuple(t[b:b + 1] for t in eager[0])), b


def test_length_normalisation_changes_the_ranking_and_the_searcher_returns_the_best():
    """d64-pre with its eos bias: the float64 search ranks utterance 2's pool differently with and without length normalisation (found
    on the CPU; asserted here on the reference first, then on the device)."""
    from summarymixing_amd.decoders import S2SBeamSearcher, beam_search
    name = "d64-pre"
    m, lin, mem, enc_len = _model(name, "f32")
    wav_len = enc_len.float() / M.S
    with _pushed(lin, PUSH[name]):
        best = {}
        for norm in (True, False):
            ref, _, _ = _f64_search(name, m, lin, mem, norm)
            r = beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, W, length_normalization=norm)
            best[norm] = [r.tokens[b, 0, :int(r.lengths[b, 0])].tolist() for b in range(M.B)]
            assert best[norm] == [ref.result(b)[0]["tokens"] for b in range(M.B)], norm
            L = r.lengths.float()
            want = r.sums / L if norm else r.sums
            assert torch.allclose(r.scores, want, rtol=1e-6, atol=0.0), "final = sum / length, or the sum"
            assert bool((r.scores[:, :-1] >= r.scores[:, 1:]).all()), "best first"
        assert best[True] != best[False], "the case was chosen so that the normalisation changes the best hypothesis"
        # the module: the recipes' ratios; the best hypothesis, eos excluded, from one host copy
        ratio = STEPS / M.S + 1e-6
        s = S2SBeamSearcher([m, lin], BOS, EOS, 0.0, ratio, beam_size=W, using_eos_threshold=False, length_normalization=True)
        hyps, lengths, scores, log_probs = s(mem, wav_len)
        r = _snap(beam_search(m, lin, mem, torch.round(wav_len * M.S), BOS, EOS, 0, STEPS, W))
        assert tuple(log_probs.shape) == (M.B, STEPS) and lengths.tolist() == [len(h) for h in hyps]
        for b in range(M.B):
            row = r[0][b, 0, :int(r[1][b, 0])].tolist()
            assert hyps[b] == (row[:-1] if row[-1] == EOS else row) and EOS not in hyps[b]
        assert torch.equal(scores, r[2][:, 0].cpu()) and torch.equal(log_probs, r[4][:, 0].cpu())
        assert len(s.state_dict()) == 0
        # min_decode_ratio delays eos (sums as final scores, under which utterance 2's short hypothesis is its best): no hypothesis of
        # any pool ends before min_steps
        late = int(M.S * 0.1)
        h_min = S2SBeamSearcher([m, lin], BOS, EOS, 0.1, ratio, beam_size=W, length_normalization=False)(mem, wav_len)[0]
        r_min = _snap(beam_search(m, lin, mem, torch.round(wav_len * M.S), BOS, EOS, late, STEPS, W, length_normalization=False))
        r_0 = _snap(beam_search(m, lin, mem, torch.round(wav_len * M.S), BOS, EOS, 0, STEPS, W, length_normalization=False))
        assert late == 7 and bool((r_min[1] > late).all()) and all(len(h) >= late for h in h_min)
        assert bool((r_0[1] <= late).any()), "without the ratio some hypothesis ends earlier"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_what_existed_gives_the_same_bits_before_and_after_beam_searches(dt):
    from summarymixing_amd.decoders import S2STransformerBeamSearcher, beam_search, greedy_search
    name = "d128-h2-post"
    m, lin, mem, enc_len = _model(name, dt)
    wav_len = enc_len.float() / M.S
    toks = torch.randint(0, M.V, (M.B, 9), generator=torch.Generator().manual_seed(2)).cuda()

    def existing():
        with torch.no_grad():
            pred, attn = m.decode(toks, mem, enc_len)
        g = greedy_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS)
        hyps, lengths, scores, lps = S2STransformerBeamSearcher([m, lin], BOS, EOS, 0.0, 0.2, beam_size=1, using_eos_threshold=False,
                                                                length_normalization=True)(mem, wav_len)
        return (pred.clone(), attn.clone(), *(t.clone() for t in g[:4]), lengths, scores, lps), hyps
    with _pushed(lin, PUSH[name]):
        before, hyps_before = existing()
        for width in (1, W, 5):
            beam_search(m, lin, mem, enc_len, BOS, EOS, MIN_STEPS, STEPS, width)
        after, hyps_after = existing()
    assert _same(before, after) and hyps_before == hyps_after

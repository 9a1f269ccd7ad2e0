"""The seq2seq greedy search (summarymixing_amd/decoders/seq2seq.py) end to end on the GPU.

a. float32 against float64: the searcher's tokens equal those of a float64 greedy loop over tests/_decoder_ref.decoder + seq_lin on the
   CPU at every (row, step) whose float64 top-2 logit gap exceeds 8 x the maximum absolute logit error of the float32 ATen chain,
   measured here (8 = the project's 4 x bar, doubled because two logits move) - and no (row, step) may fall below that margin.  In
   bfloat16 ATen's own logit error (6e-2 .. 1.2e-1 on these models) is of the size of the gaps, so token equality against float64 is
   not asserted there; (b) .. (d) cover bfloat16.
b. the same bits as a host loop of decode_step + seq_lin + torch.argmax on the same logits (the selection kernel then scores the
   forced arg-max): tokens, counts, scores and log-probabilities.
c. float32: the same tokens as the loop that exists without the feature, decode(prefix) + seq_lin + argmax.
d. CapturedS2SGreedy equals the eager search bit for bit over two utterances through one capture; poll_every 1, 8 and 0 agree; the
   bookkeeping around eos, min_decode_ratio and max_decode_ratio."""
import functools

import pytest
import torch

from tests import _s2s_models as M
from tests._util import report

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
BOS, NO_EOS = 1, M.V + 3          # an eos no token equals: every row runs all its steps
SEEDS = {"d64-pre": 3, "d128-h2-post": 4, "d512-pre": 5}
STEPS = 66


def _snap(r):
    return tuple(t.clone() for t in (r.tokens, r.counts, r.scores, r.log_probs))


def _argmax(z):
    """torch's arg-max with the tie rule spelled out - the LOWEST index of the row maximum (bfloat16 logits do tie; which of the tied
    columns torch.argmax returns is not specified)."""
    cols = torch.arange(z.shape[-1], device=z.device).expand_as(z)
    return torch.where(z == z.max(-1, keepdim=True).values, cols, z.shape[-1]).min(-1).values.to(torch.int32)


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _searched(name, dt):
    """(model, seq_lin, memory, enc_len, the eager search's result over STEPS steps with eos disabled): computed once per model."""
    from summarymixing_amd.decoders import greedy_search
    m, lin, mem, enc_len = M.build(name, DT[dt], SEEDS[name])
    return m, lin, mem, enc_len, _snap(greedy_search(m, lin, mem, enc_len, BOS, NO_EOS, 0, STEPS))


@pytest.mark.parametrize("name", list(M.MODELS))
def test_fp32_tokens_equal_the_float64_greedy_loop(name):
    m, lin, mem, enc_len, (tokens, counts, scores, lps) = _searched(name, "f32")
    f64 = M.restated(name, m, lin, mem, "f64", torch.float32)
    toks = torch.full((M.B, 1), BOS)
    for _ in range(STEPS):                                    # the float64 greedy loop: the whole prefix again for every token
        toks = torch.cat([toks, f64(toks)[1][:, -1].argmax(-1)[:, None]], 1)
    z64 = f64(toks[:, :-1])[1]                                # (B, STEPS, V): the logits every choice was made on
    z32 = M.restated(name, m, lin, mem, "aten", torch.float32)(toks[:, :-1])[1]
    err = float((z32.double().cpu() - z64).abs().max())
    top2 = z64.topk(2, -1).values
    gap = top2[..., 0] - top2[..., 1]
    print(f"s2s search {name}: float32 ATen logit error {err:.2e}, smallest float64 top-2 gap {float(gap.min()):.2e}")
    report(f"s2s_search margin {name}", {"aten_logit_err": err, "min_gap": float(gap.min())})
    assert err > 0.0 and bool((gap > 8.0 * err).all()), "a (row, step) falls below the margin: the comparison would leave it out"
    assert counts.tolist() == [STEPS] * M.B
    assert torch.equal(tokens.cpu().long(), toks[:, 1:]), "the searcher's tokens equal the float64 greedy loop's at every (row, step)"
    lp64 = torch.log_softmax(z64, -1).gather(2, toks[:, 1:, None])[..., 0]
    lp32 = torch.log_softmax(z32.double().cpu(), -1).gather(2, toks[:, 1:, None])[..., 0]
    bar = 4.0 * float((lp32 - lp64).abs().max())
    got = float((lps.double().cpu() - lp64).abs().max())
    print(f"s2s search {name}: log-probability error {got:.2e}, 4 x ATen chain {bar:.2e}")
    assert got <= bar


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(M.MODELS))
def test_same_bits_as_a_host_loop_over_decode_step(name, dt):
    from summarymixing_amd import ops
    m, lin, mem, enc_len, want = _searched(name, dt)
    state = m.make_decode_state(mem, enc_len, max_steps=STEPS)
    tok = torch.full((M.B,), BOS, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        for _ in range(STEPS):
            z = lin(m.decode_step(tok, state))
            tok = _argmax(z)
            ops.s2s_select(z, state.tok, state.done, state.n_tok, state.score, state.tokens, state.logp_tok, NO_EOS, forced=tok)
    assert _same((state.tokens, state.n_tok, state.score, state.logp_tok), want)
    assert torch.isfinite(want[2]).all() and bool((want[0] >= 0).all())


@pytest.mark.parametrize("name", list(M.MODELS))
def test_fp32_tokens_equal_the_prefix_loop_that_exists_without_the_cache(name):
    m, lin, mem, enc_len, (tokens, *_) = _searched(name, "f32")
    toks = torch.full((M.B, 1), BOS, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        for _ in range(STEPS):
            z = lin(m.decode(toks, mem, enc_len)[0][:, -1])
            toks = torch.cat([toks, _argmax(z)[:, None]], 1)
    assert torch.equal(tokens, toks[:, 1:])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_captured_search_equals_eager_and_polling_does_not_matter(dt):
    from summarymixing_amd.decoders import CapturedS2SGreedy, greedy_search
    name, eos, steps = "d64-pre", 2, 24
    m, lin, mem, enc_len, _ = _searched(name, dt)
    with torch.no_grad():
        old = lin.w.bias[eos].item()
        lin.w.bias[eos] += 3.0                                # pushes eos: rows stop at different steps
    try:
        mem2 = torch.randn(mem.shape, generator=torch.Generator().manual_seed(11)).to(DT[dt]).cuda()
        utts = [(mem, enc_len), (mem2, None)]
        eager = [_snap(greedy_search(m, lin, x, n, BOS, eos, 2, steps, temperature=1.15)) for x, n in utts]
        assert len({int(c) for e in eager for c in e[1]}) > 1, "the rows stop at different steps"
        for poll in (1, 0):
            for (x, n), e in zip(utts, eager):
                assert _same(_snap(greedy_search(m, lin, x, n, BOS, eos, 2, steps, temperature=1.15, poll_every=poll)), e), poll
        cap = CapturedS2SGreedy(m, lin, M.B, M.S, steps, DT[dt], BOS, eos, min_steps=2, temperature=1.15)
        for poll in (8, 1, 0):
            for (x, n), e in zip(utts, eager):                # both utterances through ONE capture, in turn
                assert _same(_snap(cap.search(x, n, poll_every=poll)), e), poll
        for tokens, counts, scores, lps in eager:
            for b in range(M.B):
                c = int(counts[b])
                row = tokens[b].tolist()
                assert all(k != eos for k in row[:min(c, 2)]), "eos cannot be chosen below min_steps"
                assert (eos in row[:c]) == (row[c - 1] == eos) and row[:c].count(eos) <= 1 and all(k == -1 for k in row[c:])
                assert c == steps or row[c - 1] == eos
                total = torch.zeros((), dtype=torch.float32)
                for lp in lps[b, :c].cpu():                   # the score is ONE float32 chain in step order
                    total = total + lp
                assert float(scores[b]) == float(total)
    finally:
        with torch.no_grad():
            lin.w.bias[eos] = old


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_searcher_modules_bookkeeping(dt):
    from summarymixing_amd.decoders import S2STransformerBeamSearcher, S2STransformerGreedySearcher, greedy_search
    name, eos = "d64-pre", 2
    m, lin, mem, enc_len, _ = _searched(name, dt)
    wav_len = (enc_len.float() / M.S)
    with torch.no_grad():
        old = lin.w.bias[eos].item()
        lin.w.bias[eos] += 3.0
    try:
        g = S2STransformerGreedySearcher([m, lin], BOS, eos, 0.0, 0.4)
        hyps, lengths, scores, log_probs = g(mem, wav_len)
        max_steps = int(M.S * 0.4)
        r = _snap(greedy_search(m, lin, mem, torch.round(wav_len * M.S), BOS, eos, 0, max_steps))
        assert len(hyps) == M.B and lengths.tolist() == [len(h) for h in hyps] and tuple(log_probs.shape) == (M.B, max_steps)
        for b in range(M.B):
            c, row = int(r[1][b]), r[0][b].tolist()
            assert eos not in hyps[b] and len(hyps[b]) <= max_steps, "hyps exclude eos; max_decode_ratio bounds the length"
            assert hyps[b] == (row[:c - 1] if row[c - 1] == eos else row[:c])
        assert torch.equal(scores, r[2].cpu()) and torch.equal(log_probs, r[3].cpu())
        assert any(len(h) < max_steps for h in hyps) and len({len(h) for h in hyps}) > 1, "rows stop at different steps"
        # a finished row keeps its tokens and score while the others go on: a row alone = the row inside the batch, bit for bit
        for b in range(M.B):
            h1, l1, s1, p1 = g(mem[b:b + 1], wav_len[b:b + 1])
            assert h1[0] == hyps[b] and torch.equal(s1[0], scores[b]) and torch.equal(p1[0], log_probs[b]), b
        # min_decode_ratio delays eos
        h_min = S2STransformerGreedySearcher([m, lin], BOS, eos, 0.3, 0.4)(mem, wav_len)[0]
        assert all(len(h) >= int(M.S * 0.3) for h in h_min) and any(len(a) > len(b_) for a, b_ in zip(h_min, hyps))
        # beam_size = 1 is the greedy search
        hb, lb, sb, pb = S2STransformerBeamSearcher([m, lin], BOS, eos, 0.0, 0.4, beam_size=1, using_eos_threshold=False,
                                                    length_normalization=True)(mem, wav_len)
        assert hb == hyps and torch.equal(lb, lengths) and torch.equal(sb, scores) and torch.equal(pb, log_probs)
        assert len(g.state_dict()) == 0
    finally:
        with torch.no_grad():
            lin.w.bias[eos] = old

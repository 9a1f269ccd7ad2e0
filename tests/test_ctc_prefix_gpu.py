"""smx_ctc_prefix_init / _score / _advance (csrc/ctc_prefix.hip) against the float64 restatement of DESIGN.md §I.23
(tests/_ctc_prefix_ref.py) along 4-step chains with GIVEN winners - no decoder, no selection: the test writes the beam state the
selection would have left (tokens, anc, score, n_tok) and checks, at every step, the (r_n, r_b, psi) state of every live row and the
whole extra = weight (ctc - lp).

The chains hold: the empty prefix, a repeated token (c == last), the eos and the blank column, logits of -inf, a dead row, slots that
share one parent, a prefix longer than T_b (psi = -inf: enc_len 1, T 1 and 2), and at the last step a done utterance whose logits and
state are NaN.  Frames at and beyond T_b and every state slot are NaN before the chain starts: what is never written must never be read.

Bar (the project's): the error against float64 is at most 4 x that of the same recursion written with torch.logaddexp in float32 on
the CPU at the same shape (tests/_ctc_prefix_ref.py in float32), on the state and on extra - the form in which ctc leaves the device:
weight (ctc - lp), so the combination is inside the bar; both go through tests/_util.report.  Measured on an MI355X: state 0 (T = 1)
.. 3.8e-4, extra 3.4e-8 .. 1.2e-4, between 0.15 and 1.0 of the float32 recursion's own error (at most 0.25 of the bar)."""
import functools

import pytest
import torch

from tests import _ctc_prefix_ref as P
from tests._util import report

pytestmark = pytest.mark.gpu
EOS, WEIGHT, CAP, TEMP = 2, 0.4, 6, 1.15
NEG_INF = float("-inf")
# (T, V, B, W, blank, enc_len)
CASES = [(1, 7, 1, 1, 0, (1,)), (2, 64, 2, 3, 3, (2, 1)), (63, 65, 2, 3, 0, (63, 17)), (64, 7, 1, 1, 3, (40,)), (64, 1003, 2, 3, 0, (64, 1)),
         (65, 1003, 2, 3, 3, (65, 64)), (130, 64, 2, 3, 0, (129, 130)), (130, 65, 1, 1, 3, (100,))]


def _plan(W, V, blank, seed):
    """Per step, per slot: (parent slot, token) or None (dead).  Step 0 has one parent; step 1 repeats step 0's tokens (c == last)
    in slot 0; with W = 3 two slots share a parent and a slot dies at step 2."""
    g = torch.Generator().manual_seed(seed)
    labels = [k for k in range(V) if k not in (blank, EOS)]

    def tok():
        return labels[int(torch.randint(0, len(labels), (1,), generator=g))]
    if W == 1:
        a = tok()
        return [[(0, a)], [(0, a)], [(0, tok())], [(0, tok())]]
    a, b = tok(), tok()
    return [[(0, a), (0, b), (0, tok())], [(0, a), (1, b), (1, tok())], [(2, tok()), (0, a), None], [(1, a), (1, tok()), (0, tok())]]


def _chain(case, seed):
    from summarymixing_amd import ops
    from summarymixing_amd.decoders.scorer import CTCPrefixState
    from summarymixing_amd.lobes.models.transformer.Transformer import DecodeState
    T, V, B, W, blank, enc_len = case
    R = B * W
    g = torch.Generator().manual_seed(seed)
    x = torch.log_softmax(torch.randn(B, T, V, generator=g) * 2.0, -1)
    x_dev = x.clone()
    for b in range(B):
        x_dev[b, enc_len[b]:] = float("nan")
    st = DecodeState(B, T, CAP, 1, 64, 0, torch.float32, torch.float32, "cuda", beam=W)
    st.mem_len.copy_(torch.tensor(enc_len))
    cs = CTCPrefixState(st, V, blank, EOS, WEIGHT)
    cs.x.copy_(x_dev)
    cs.state.fill_(float("nan"))
    cs.psi.fill_(float("nan"))
    cs.extra.fill_(float("nan"))
    ops.ctc_prefix_init(cs, st)
    refs = {dt: [[P.empty(x[b].to(dt), enc_len[b], blank) if i == 0 else None for i in range(W)] for b in range(B)]
            for dt in (torch.float64, torch.float32)}
    hist = [[[] for _ in range(W)] for _ in range(B)]
    alive = [[i == 0 for i in range(W)] for _ in range(B)]
    plans = [_plan(W, V, blank, seed + 10 * b) for b in range(B)]
    err = {"state": [0.0, 0.0], "extra": [0.0, 0.0]}          # [ours, the float32 recursion's]
    outs = []

    def check_state(n):
        dev, psi = cs.state[n & 1].cpu(), cs.psi[n & 1].cpu()
        for b in range(B):
            for i in range(W):
                if not alive[b][i]:
                    continue
                r, Tb = b * W + i, enc_len[b]
                want = refs[torch.float64][b][i]
                f32 = refs[torch.float32][b][i]
                for k, (got, lo) in enumerate(((dev[r, :Tb, 0], f32[0]), (dev[r, :Tb, 1], f32[1]), (psi[r].view(1), f32[2].view(1)))):
                    w = want[k].view(-1)
                    fin = torch.isfinite(w)
                    assert torch.equal(torch.isfinite(got), fin) and torch.equal(got[~fin].double(), w[~fin]), (n, b, i, k, "the -inf pattern")
                    assert torch.equal(torch.isfinite(lo.view(-1)), fin)
                    if fin.any():
                        err["state"][0] = max(err["state"][0], float((got[fin].double() - w[fin]).abs().max()))
                        err["state"][1] = max(err["state"][1], float((lo.view(-1)[fin].double() - w[fin]).abs().max()))
    check_state(0)
    for n in range(4):
        last_step = n == 3
        z = torch.randn(R, V, generator=g) * 3.0
        z[:, (blank + 1) % V] = NEG_INF                       # a column of probability 0: lp = -inf
        z_dev = z.clone()
        if last_step and B > 1:                               # utterance 1 is done: its logits and its state are no numbers
            st.done[1] = 1
            z_dev[W:] = float("nan")
            cs.state[:, W:].fill_(float("nan"))
            cs.psi[:, W:].fill_(float("nan"))
        z_dev = z_dev.cuda()
        got = ops.ctc_prefix_score(cs, st, z_dev, 1.0 / TEMP).cpu()
        outs.append(got.clone())
        saw_inf_prefix = False
        for b in range(B):
            done = last_step and b == 1
            for i in range(W):
                r = b * W + i
                if done or not alive[b][i]:
                    assert bool((got[r] == NEG_INF).all()), (n, r, "a dead row / a done utterance scores -inf everywhere")
                    continue
                last = hist[b][i][-1] if hist[b][i] else None
                ex = {}
                for dt in (torch.float64, torch.float32):
                    ctc = P.scores(x[b].to(dt), enc_len[b], blank, EOS, refs[dt][b][i], last)[0]
                    ex[dt] = P.combine(ctc, torch.log_softmax(z[r].to(dt) / TEMP, -1), WEIGHT)
                want = ex[torch.float64]
                fin = torch.isfinite(want)
                assert not torch.isnan(got[r]).any() and torch.equal(torch.isfinite(got[r]), fin), (n, r, "the -inf pattern of extra")
                assert bool((got[r][~fin] == NEG_INF).all()) and float(got[r, blank]) == NEG_INF
                assert torch.equal(torch.isfinite(ex[torch.float32]), fin)
                if float(refs[torch.float64][b][i][2]) == NEG_INF:
                    saw_inf_prefix = True
                    assert not fin.any()
                if fin.any():
                    err["extra"][0] = max(err["extra"][0], float((got[r][fin].double() - want[fin]).abs().max()))
                    err["extra"][1] = max(err["extra"][1], float((ex[torch.float32][fin].double() - want[fin]).abs().max()))
        if min(enc_len) == 1 and n == 2:
            assert saw_inf_prefix, "the chain was to hold a prefix longer than T_b"
        if W == 3 and n == 2:                                 # the slot that dies at this step: what advance skips stays NaN
            for b in range(B):
                cs.state[(n + 1) & 1, b * W + 2].fill_(float("nan"))
                cs.psi[(n + 1) & 1, b * W + 2] = float("nan")
        # the selection's writes, given: slot i <- (parent, token)
        tokens, anc, score = st.tokens.cpu(), st.anc.cpu(), st.score.cpu()
        new_hist, new_alive = [[None] * W for _ in range(B)], [[False] * W for _ in range(B)]
        new_refs = {dt: [[None] * W for _ in range(B)] for dt in refs}
        for b in range(B):
            if last_step and b == 1:
                new_hist[b], new_alive[b] = hist[b], alive[b]
                for dt in refs:
                    new_refs[dt][b] = refs[dt][b]
                continue
            for i, slot in enumerate(plans[b][n]):
                r = b * W + i
                if slot is None:
                    score[r] = NEG_INF
                    new_hist[b][i] = []
                    continue
                p, c = slot
                new_hist[b][i], new_alive[b][i] = hist[b][p] + [c], True
                tokens[r, :n + 1] = torch.tensor(new_hist[b][i], dtype=torch.int32)
                anc[r, :n + 1] = b * W + p
                score[r] = -1.0 - i
                for dt in refs:
                    new_refs[dt][b][i] = P.extend(x[b].to(dt), enc_len[b], blank, refs[dt][b][p], hist[b][p][-1] if hist[b][p] else None, c)
        st.tokens.copy_(tokens)
        st.anc.copy_(anc)
        st.score.copy_(score)
        st.n_tok.copy_(torch.tensor([n + (0 if (last_step and b == 1) else 1) for b in range(B)], dtype=torch.int32))
        before = (cs.state.clone(), cs.psi.clone())
        ops.ctc_prefix_advance(cs, st)
        hist, alive, refs = new_hist, new_alive, new_refs
        if last_step and B > 1:                               # the done utterance's slots: untouched, bit for bit (NaN included)
            for t, t0 in zip((cs.state, cs.psi), before):
                assert torch.equal(t[:, W:].contiguous().view(torch.uint8), t0[:, W:].contiguous().view(torch.uint8))
            for b in range(1, B):
                alive[b] = [False] * W
        check_state(n + 1)
        outs.append(cs.state.clone().cpu())
        outs.append(cs.psi.clone().cpu())
    # what was never written was never read: the slot the dead row of step 2 would have taken is still NaN at that parity
    if W == 3:
        assert bool(torch.isnan(cs.state[1, 2, :enc_len[0]]).all()) and bool(torch.isnan(cs.psi[1, 2]))
    return err, outs, (cs, st, z_dev)


@functools.lru_cache(maxsize=None)
def _run(k):
    return _chain(CASES[k], 100 + k)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"T{c[0]}-V{c[1]}-{c[2]}x{c[3]}-blank{c[4]}" for c in CASES])
def test_state_and_extra_along_a_chain_within_four_times_the_float32_recursion(k):
    err, _, _ = _run(k)
    for what, (ours, f32) in err.items():
        print(f"ctc_prefix {CASES[k]} {what}: ours {ours:.3e}, the float32 torch.logaddexp recursion {f32:.3e}, bar {4 * f32:.3e}")
        report(f"ctc_prefix {what} T{CASES[k][0]} V{CASES[k][1]} {CASES[k][2]}x{CASES[k][3]}", {"errors": {what: {"ours": ours, "ref": f32, "bar": 4 * f32}}})
    for what, (ours, f32) in err.items():
        assert ours <= 4.0 * f32, (what, ours, f32)


@pytest.mark.parametrize("k", [2, 5])
def test_two_runs_agree_bit_for_bit_and_captured_equals_eager(k):
    from summarymixing_amd import ops
    _, a, (cs, st, z) = _run(k)
    _, b, _ = _chain(CASES[k], 100 + k)
    assert len(a) == len(b) and all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b))
    # the last step's two launches again, captured: advance (writes the parity score reads), then score
    inv = 1.0 / TEMP
    ops.ctc_prefix_advance(cs, st)
    eager = (ops.ctc_prefix_score(cs, st, z, inv).clone(), cs.state.clone(), cs.psi.clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.ctc_prefix_advance(cs, st)
        ops.ctc_prefix_score(cs, st, z, inv)
    q = st.n_tok[0].item() & 1
    cs.extra.fill_(7.0)
    cs.state[q, :st.beam].fill_(7.0)                          # utterance 0's freshly written parity: the replay writes it again
    cs.psi[q, :st.beam].fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip((cs.extra, cs.state, cs.psi), eager):
        live = ~torch.isnan(want)                             # (NaN: the slots this test poisoned, which nothing writes)
        assert torch.equal(got[live].view(torch.uint8), want[live].view(torch.uint8))

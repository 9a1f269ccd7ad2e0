"""smx_s2s_beam_select (csrc/beam.hip) alone, through ops.s2s_beam_select, on GIVEN logits: single steps and 4-step chains against the
float64 restatement of the search (tests/_s2s_beam_ref.py).

Exact: the tokens, the parents (read off the ancestor table), the histories' layout, the flags, the counters, which entries the pool
holds and in what order.  A random case is compared only if every float64 gap between adjacent ranks 1 .. W + 1 of an utterance's
candidates is at least 8 x (n + 1) x the error torch.log_softmax makes at float32 on the same logits, measured here (the project's
margin: two scores move; a score at step n is a float32 sum of n + 1 log-probabilities, hence the factor) - or is an exact tie between
two columns of ONE row that hold the same logit, which every arithmetic resolves by the column order.  The seeds were checked on the
CPU beforehand and the test asserts that NO case was left out.  Scores and log-probabilities are held to 4 x the same measured error
((n + 1) x for a sum; 8 eps(float32) x the magnitude where torch is exact), recorded through tests/_util.report."""
import pytest
import torch

from tests import _s2s_beam_ref as R
from tests._util import report

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS32 = torch.finfo(torch.float32).eps
NEG_INF = float("-inf")
FIELDS = ("tok", "score", "row_done", "done", "n_tok", "tokens", "logp_tok", "anc", "pool_tokens", "pool_logp", "pool_len", "pool_final",
          "pool_sum", "pool_seq", "pool_cnt", "pool_ins", "res_tokens", "res_logp", "res_len", "res_final", "res_sum")


def _state(B, W, cap):
    """The beam part of a decoding state, without a model (no layers: no caches)."""
    from summarymixing_amd.lobes.models.transformer.Transformer import DecodeState
    return DecodeState(B, 1, cap, 1, 64, 0, torch.float32, torch.float32, "cuda", beam=W)


def _lp_err(z, T):
    """The error torch.log_softmax makes at float32 on these logits against float64, floored where it is exact."""
    ref = torch.log_softmax(z.double().cpu() / T, -1)
    fin = torch.isfinite(ref)
    err = float((torch.log_softmax(z.float() / T, -1).double().cpu() - ref)[fin].abs().max()) if bool(fin.any()) else 0.0
    return err if err > 0.0 else 2.0 * EPS32 * float(ref[fin].abs().max()) if bool(fin.any()) else EPS32


class Chain:
    """A device state and the float64 reference stepped side by side."""

    def __init__(self, name, B, W, V, cap, eos, min_steps=0, T=1.0, norm=True):
        self.name, self.B, self.W, self.V, self.cap, self.eos, self.min_steps, self.T, self.norm = name, B, W, V, cap, eos, min_steps, T, norm
        self.st = _state(B, W, cap)
        self.ref = R.BeamRef(B, W, V, cap, eos, min_steps, T, norm)
        self.err = 0.0                                         # the largest measured log_softmax error of the steps so far
        self.left_out, self.worst = [], {"lp": (0.0, 0.0), "score": (0.0, 0.0), "final": (0.0, 0.0)}

    def step(self, z, extra=None, margin=True):
        """One step on both sides, then the comparison.  margin=False: a hand-built case whose ties are exact by construction."""
        from summarymixing_amd import ops
        was_done = list(self.ref.done)
        n_before = list(self.ref.n)
        ops.s2s_beam_select(z, self.st, self.eos, self.min_steps, 1.0 / self.T, self.norm, extra=extra)
        out = self.ref.step(z, extra)
        live = [b for b in range(self.B) if not was_done[b]]
        if live:
            rows = torch.tensor([b * self.W + i for b in live for i in range(self.W)])
            rows = rows[torch.isfinite(z[rows.cuda()].float()).all(-1).cpu()]
            if rows.numel():
                self.err = max(self.err, _lp_err(z[rows.cuda()], self.T))
        if margin:
            for b in live:
                need = 8.0 * (n_before[b] + 1) * self.err
                for g, twin in zip(out[b]["gaps"], out[b]["twins"]):
                    if not (g >= need or (g == 0.0 and twin)):
                        self.left_out.append((b, n_before[b], g, need))
        self.compare(was_done)
        return out

    def _bar(self, key, got, want, terms):
        bar = 4.0 * terms * self.err if self.err > 0.0 else 8.0 * EPS32 * max(1.0, abs(want))
        e = abs(got - want)
        if e / bar >= self.worst[key][0] / max(self.worst[key][1], 1e-300):
            self.worst[key] = (e, bar)
        assert e <= bar, f"{self.name}: {key} {got} vs {want}: error {e:.3e} over the bar {bar:.3e}"

    def compare(self, was_done):
        st, ref, W, cap = self.st, self.ref, self.W, self.cap
        c = {k: getattr(st, k).cpu() for k in FIELDS}
        for b in range(self.B):
            n = ref.n[b]
            assert int(c["n_tok"][b]) == n and bool(c["done"][b]) == ref.done[b], (self.name, b, int(c["n_tok"][b]), n)
            assert c["row_done"][b * W:(b + 1) * W].tolist() == [int(ref.done[b])] * W
            assert int(c["pool_cnt"][b]) == len(ref.pool[b]) and int(c["pool_ins"][b]) == ref.ins[b], (self.name, b)
            if not was_done[b]:
                for i in range(W):
                    r = b * W + i
                    if ref.alive(b, i):
                        assert c["tokens"][r, :n].tolist() == ref.tokens[b][i] and int(c["tok"][r]) == ref.tok[b][i], (self.name, b, i)
                        assert c["anc"][r, :n].tolist() == ref.anc[b][i], (self.name, b, i, "the parents")
                        assert bool((c["tokens"][r, n:] == -1).all())
                        self._bar("score", float(c["score"][r]), float(ref.score[b, i]), n)
                        for j in range(n):
                            self._bar("lp", float(c["logp_tok"][r, j]), ref.lps[b][i][j], 1)
                    else:
                        assert float(c["score"][r]) == NEG_INF and int(c["tok"][r]) == self.eos, (self.name, b, i, "a dead slot")
            if ref.done[b]:
                res = ref.result(b)
                for k, e in enumerate(res):
                    L = len(e["tokens"])
                    assert c["res_tokens"][b, k].tolist() == e["tokens"] + [-1] * (cap - L), (self.name, b, k, "the pool's order and tokens")
                    assert int(c["res_len"][b, k]) == L and bool((c["res_logp"][b, k, L:] == 0).all())
                    self._bar("score", float(c["res_sum"][b, k]), e["sum"], L)
                    self._bar("final", float(c["res_final"][b, k]), e["final"], 1 if self.norm else L)
                    for j in range(L):
                        self._bar("lp", float(c["res_logp"][b, k, j]), e["lps"][j], 1)
                for k in range(len(res), W):
                    assert int(c["res_len"][b, k]) == 0 and float(c["res_final"][b, k]) == NEG_INF and bool((c["res_tokens"][b, k] == -1).all())

    def finish(self):
        print(f"{self.name}: log_softmax error {self.err:.2e}; worst (error, bar) {self.worst}")
        report(self.name, {"aten_lp_err": self.err, "errors": {k: {"ours": e, "bar": b} for k, (e, b) in self.worst.items()}})
        assert not self.left_out, f"{self.name}: (utterance, step, gap, needed) below the margin - the comparison would leave them out: {self.left_out}"


def _random_logits(g, R_, V, dtype, scale=3.0):
    return (torch.randn(R_, V, generator=g) * scale).to(dtype).cuda()


WV = [(W, V) for W in (1, 2, 3, 5, 16, 66) for V in (7, 64, 1000, 5003)]
# the generator seed of each (W, V, dtype) that is not 0: the first of 0, 1, 2, ... whose 4-step chain keeps every gap above 2.5 x
# the margin with the log_softmax error of the CPU (found on the CPU; the test applies the margin with the error measured on the GPU)
SEEDS = {(16, 5003, "f32"): 1, (66, 7, "f32"): 1, (66, 64, "f32"): 1, (66, 1000, "bf16"): 3, (66, 5003, "f32"): 16}


def _heavy_logits(g, R_, V, dtype, scale=3.0):
    """Exponentially distributed logits: the best W + 1 of W V candidates lie about scale / rank apart, where normal logits crowd
    (at W = 66, V = 5003 their gaps fall below the margin whatever the seed)."""
    return (torch.empty(R_, V).exponential_(generator=g) * scale).to(dtype).cuda()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("W,V", WV)
def test_four_step_chains_equal_the_float64_reference(W, V, dt):
    """B = 2, cap = 4 (the last step is n + 1 == cap), T = 1.15, eos = 2 with min_steps 1: eos wins slots along the way, the pool fills,
    V < W leaves slots without a winner.  At n = 0 the rows of the dead slots hold NaN: they are not read."""
    B, cap, eos = 2, 4, 2
    ch = Chain(f"s2s_beam chain W{W} V{V} {dt}", B, W, V, cap, eos, min_steps=1, T=1.15)
    g = torch.Generator().manual_seed(SEEDS.get((W, V, dt), 0) * 1000 + 7 * W + V)
    for n in range(cap):
        z = _heavy_logits(g, B * W, V, DT[dt])
        if n == 0 and W > 1:
            z.view(B, W, V)[:, 1:] = float("nan")
        ch.step(z)
    assert all(ch.ref.done) and all(len(p) >= 1 for p in ch.ref.pool)
    ch.finish()


def _logp(rows):
    return torch.tensor(rows, dtype=torch.float64).log().float().cuda()


def test_exact_ties_across_parents_resolve_to_the_lowest_flat_index():
    """Integer-valued logits.  Step 0 leaves two slots with the SAME score (equal logits 20, 20) and a third below; at step 1 all rows
    hold the same logits, whose maximum 9 appears twice: four candidates tie exactly, on any arithmetic, and three slots are to be
    filled - (parent 0, col 1), (parent 0, col 4), (parent 1, col 1), in that order; (parent 1, col 4) stays out."""
    W, V = 3, 8
    ch = Chain("s2s_beam ties", 1, W, V, 6, eos=7)
    z0 = torch.tensor([[20., 3., 20., 13., 1., 0., 2., 5.]] * W).cuda()
    out = ch.step(z0, margin=False)[0]
    assert [(p, v) for p, v, _, _ in out["winners"]] == [(0, 0), (0, 2), (0, 3)] and out["gaps"][0] == 0.0
    z1 = torch.tensor([[4., 9., 0., 1., 9., 2., 3., 1.]] * W).cuda()
    out = ch.step(z1, margin=False)[0]
    assert [(p, v) for p, v, _, _ in out["winners"]] == [(0, 1), (0, 4), (1, 1)] and out["gaps"] == [0.0, 0.0, 0.0]
    assert ch.st.anc[:, :2].tolist() == [[0, 0], [0, 0], [0, 1]] and ch.st.tokens[:, :2].tolist() == [[0, 1], [0, 4], [2, 1]]
    s = ch.st.score.cpu()
    assert float(s[0]) == float(s[1]) == float(s[2]), "the three winners hold one score, bit for bit"
    ch.finish()


def test_eos_is_no_candidate_below_min_steps_and_takes_several_slots_after():
    """eos holds the largest logit of every row.  Below min_steps = 2 it is never chosen; at n = 2 it is the best candidate of all three
    rows at once: three pool entries in one step, the pool is full and the utterance ends."""
    W, V, eos = 3, 65, 9
    ch = Chain("s2s_beam eos min_steps", 2, W, V, 8, eos, min_steps=2)
    g = torch.Generator().manual_seed(21)
    for n in range(3):
        z = _random_logits(g, 2 * W, V, torch.float32, 1.0)
        z[:, eos] = 12.0
        out = ch.step(z)
        for b in range(2):
            toks = [v for _, v, _, _ in out[b]["winners"]]
            assert (eos not in toks) if n < 2 else (toks == [eos] * W), (n, toks)
    assert ch.ref.events == [["append"] * W] * 2 and all(ch.ref.done) and ch.st.done.tolist() == [1, 1]
    assert ch.st.res_len.tolist() == [[3] * W] * 2 and bool((ch.st.res_tokens[:, :, 2] == eos).all())
    ch.finish()


def _peaked(V, top, rest):
    """A probability row: `top` = {column: probability}, the other columns share `rest` equally."""
    row = [rest / (V - len(top))] * V
    for k, p in top.items():
        row[k] = p
    return row


def test_full_pool_replaces_its_worst_entry_and_refuses_a_worse_one():
    """W = 3, V = 6, eos = 5, sums as final scores.  Steps 0 and 1 put two poor hypotheses in the pool (A: sum ln .006, B: ln .0049);
    step 2 has no eos winner, so three slots are alive; at step 3 eos wins all three: .4795 fills the pool, .4703 replaces B, the
    worst, and .00094 is worse than A, now the worst: refused.  The pool, best first: the two good ones, then A."""
    W, V, eos = 3, 6, 5
    ch = Chain("s2s_beam pool", 1, W, V, 8, eos, norm=False)
    u = [1 / V] * V
    steps = [[_peaked(V, {0: .49, 1: .49, eos: .006}, .014), u, u],
             [_peaked(V, {0: .98}, .02), _peaked(V, {0: .97, eos: .01}, .02), u],
             [_peaked(V, {0: .999}, .001), _peaked(V, {0: .99, 1: .0099}, .0001), u],
             [_peaked(V, {eos: .9995}, .0005), _peaked(V, {eos: .9995}, .0005), _peaked(V, {eos: .2}, .8)]]
    for rows in steps:
        ch.step(_logp(rows))
    assert ch.ref.events == [["append", "append", "append", "replace", "refuse"]]
    assert ch.st.done.tolist() == [1] and int(ch.st.pool_cnt[0]) == 3 and int(ch.st.pool_ins[0]) == 4
    assert ch.st.res_tokens[0, :, :4].tolist() == [[0, 0, 0, eos], [1, 0, 0, eos], [eos, -1, -1, -1]] and ch.st.res_len[0].tolist() == [4, 4, 1]
    ch.finish()


def test_nan_row_has_no_candidates_and_the_last_step_ends_every_slot():
    """Step 1: the row of slot 1 holds one NaN - none of its columns is a candidate, the other two rows fill the three slots.  cap = 3:
    at n = 2 every winner enters the pool as it is, no eos appended."""
    W, V = 3, 130
    ch = Chain("s2s_beam nan row", 2, W, V, 3, eos=V + 4)
    g = torch.Generator().manual_seed(5)
    ch.step(_random_logits(g, 2 * W, V, torch.float32))
    z = _random_logits(g, 2 * W, V, torch.float32)
    z[1, 77] = float("nan")
    z[W + 1] = float("nan")
    out = ch.step(z)
    assert all(p != 1 for b in range(2) for p, _, _, _ in out[b]["winners"]) and all(len(out[b]["winners"]) == W for b in range(2))
    assert bool(torch.isfinite(ch.st.score).all())
    ch.step(_random_logits(g, 2 * W, V, torch.float32))
    assert all(ch.ref.done) and ch.st.res_len.tolist() == [[3] * W] * 2 and bool((ch.st.res_tokens >= 0).all())
    ch.finish()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_extra_scores_are_added_to_the_candidates(dt):
    """The scorer hook: extra (R, V) float32 changes the ranking inside a row and across rows; the stored log-probability stays the
    token's own."""
    W, V = 5, 1000
    ch = Chain(f"s2s_beam extra {dt}", 2, W, V, 4, eos=3, min_steps=1)
    g = torch.Generator().manual_seed(12)
    changed = False
    for n in range(4):
        z = _random_logits(g, 2 * W, V, DT[dt])
        extra = (torch.randn(2 * W, V, generator=g) * 2).cuda()
        out = ch.step(z, extra)
        plain = R.BeamRef(2, W, V, 4, 3, 1)
        if n == 0 and out[0] is not None:
            changed = [v for _, v, _, _ in plain.step(z)[0]["winners"]] != [v for _, v, _, _ in out[0]["winners"]]
    assert changed, "extra changes the ranking of this case"
    ch.finish()


def test_a_finished_utterance_is_left_untouched():
    """Utterance 0 ends at step 1 (its pool fills), utterance 1 goes on: a further step with NaN in utterance 0's logits changes no
    bit of anything utterance 0 owns, and utterance 1 equals itself stepped alone."""
    W, V, eos, cap = 2, 64, 4, 6
    ch = Chain("s2s_beam done", 2, W, V, cap, eos)
    alone = Chain("s2s_beam done alone", 1, W, V, cap, eos)
    g = torch.Generator().manual_seed(31)
    z = _random_logits(g, 2 * W, V, torch.float32, 1.0)
    ch.step(z)
    alone.step(z[W:].contiguous())
    z = _random_logits(g, 2 * W, V, torch.float32, 1.0)
    z[:W, eos] = 15.0                                          # both slots of utterance 0 end
    ch.step(z)
    alone.step(z[W:].contiguous())
    assert ch.ref.done == [True, False]
    before = {k: getattr(ch.st, k).clone() for k in FIELDS}
    z = _random_logits(g, 2 * W, V, torch.float32, 1.0)
    z[:W] = float("nan")
    ch.step(z)
    alone.step(z[W:].contiguous())
    per_row = ("tok", "score", "row_done", "tokens", "logp_tok", "anc")
    for k in FIELDS:
        a, b_ = getattr(ch.st, k), before[k]
        n0 = W if k in per_row else 1
        assert torch.equal(a[:n0].view(torch.uint8), b_[:n0].view(torch.uint8)), f"{k} of the finished utterance changed"
        theirs = getattr(alone.st, k)
        if k == "anc":
            theirs = torch.where(theirs >= 0, theirs + W, theirs)
        if k not in ("pool_tokens", "pool_logp", "pool_len", "pool_final", "pool_sum", "pool_seq"):      # (the pool's unused slots hold anything)
            assert torch.equal(a[n0:].view(torch.uint8), theirs.view(torch.uint8)), f"{k}: utterance 1 depends on its batch"
    ch.finish()

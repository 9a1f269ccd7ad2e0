"""CTC prefix scoring as DESIGN.md §I.23 defines it, restated on the host with torch.logaddexp in the dtype of the log-probabilities
it is given: float64 is what tests/test_ctc_prefix_*.py and tests/test_s2s_ctc_beam_gpu.py hold the kernels of csrc/ctc_prefix.hip
to, float32 is "the same recursion written with torch.logaddexp in fp32 on the CPU" whose error sets their bar.

x (T, V): the log-softmax of the CTC head over one utterance, Tb its frames (frames at and beyond are never read).  A prefix g (the
tokens after bos, no eos) has the state (r_n (Tb), r_b (Tb), psi): the log-probabilities of its alignments over frames 0..t ending in
a non-blank / in blank, and its log prefix probability.
  empty prefix:  r_n = -inf, r_b[t] = sum_{tau <= t} x[tau, blank], psi = 0.
  g c (c not blank, not eos), last = g's final token (none: g is empty), phi[t] = r_b[t] if c == last else logaddexp(r_n[t], r_b[t]):
     r_n'[0] = x[0, c] if g is empty else -inf, r_b'[0] = -inf, psi' = r_n'[0];  for t = 1 .. Tb - 1:
     r_n'[t] = logaddexp(r_n'[t-1], phi[t-1]) + x[t, c],  r_b'[t] = logaddexp(r_n'[t-1], r_b'[t-1]) + x[t, blank],
     psi' = logaddexp(psi', phi[t-1] + x[t, c]).
  c == eos: psi' = logaddexp(r_n[Tb-1], r_b[Tb-1]) (the whole sequence);  c == blank: psi' = -inf.
  ctc[c] = psi' - psi; every entry -inf where psi = -inf (never NaN).
Rows that are dead, rows of a done utterance and rows with psi = -inf score -inf in every column: the kernels' convention.
`PrefixScorer` carries the states of the B W rows of a tests/_s2s_beam_ref.BeamRef through its steps (BeamRef.step(logits, extra=...))."""
import torch

NEG_INF = float("-inf")


def empty(x, Tb, blank):
    r_b = torch.cumsum(x[:Tb, blank], 0)
    return torch.full_like(r_b, NEG_INF), r_b, torch.zeros((), dtype=x.dtype)


def extend(x, Tb, blank, state, last, c):
    """The state of g c from the state of g (last: g's final token, None for the empty prefix)."""
    r_n, r_b, _ = state
    phi = r_b if c == last else torch.logaddexp(r_n, r_b)
    n, b = torch.full_like(r_n, NEG_INF), torch.full_like(r_n, NEG_INF)
    if last is None:
        n[0] = x[0, c]
    psi = n[0].clone()
    for t in range(1, Tb):
        n[t] = torch.logaddexp(n[t - 1], phi[t - 1]) + x[t, c]
        b[t] = torch.logaddexp(n[t - 1], b[t - 1]) + x[t, blank]
        psi = torch.logaddexp(psi, phi[t - 1] + x[t, c])
    return n, b, psi


def scores(x, Tb, blank, eos, state, last):
    """-> (ctc (V) = psi(g c) - psi(g), psi' (V)) for every column c at once (the recursion of `extend`, one vector per frame)."""
    r_n, r_b, psi = state
    V = x.shape[1]
    if float(psi) == NEG_INF:
        return torch.full((V,), NEG_INF, dtype=x.dtype), torch.full((V,), NEG_INF, dtype=x.dtype)
    both = torch.logaddexp(r_n, r_b)
    n = x[0].clone() if last is None else torch.full((V,), NEG_INF, dtype=x.dtype)
    p1 = n.clone()
    for t in range(1, Tb):
        phi = both[t - 1].expand(V).clone()
        if last is not None:
            phi[last] = r_b[t - 1]
        p1 = torch.logaddexp(p1, phi + x[t])
        n = torch.logaddexp(n, phi) + x[t]
    p1[blank] = NEG_INF
    if 0 <= eos < V:
        p1[eos] = both[Tb - 1]
    ctc = torch.where(p1 == NEG_INF, p1, p1 - psi)
    return ctc, p1


def combine(ctc, lp, weight):
    """extra = weight (ctc - lp); -inf where either is -inf (no candidate)."""
    bad = (ctc == NEG_INF) | (lp == NEG_INF)
    return torch.where(bad, torch.full_like(ctc, NEG_INF), weight * (ctc - lp))


class PrefixScorer:
    """The prefix states of the rows of a BeamRef over x (B, T, V) (any float dtype; computed in `dtype`) with enc_len (B)."""

    def __init__(self, x, enc_len, blank, eos, weight, W, dtype=torch.float64):
        self.x = x.detach().to("cpu", dtype)
        self.B, self.T, self.V = self.x.shape
        self.Tb = [max(1, min(int(n), self.T)) for n in enc_len]
        self.blank, self.eos, self.weight, self.W, self.dtype = blank, eos, weight, W, dtype
        self.state = [[empty(self.x[b], self.Tb[b], blank) if i == 0 else None for i in range(W)] for b in range(self.B)]

    def extra(self, beam, logits):
        """(B W, V) in dtype for the step `beam` (a BeamRef) is about to take over logits (B W, V): weight (ctc - lp), lp the
        log-softmax of logits / T in dtype; -inf rows where there is nothing to score."""
        z = logits.detach().to("cpu", self.dtype).view(self.B, self.W, self.V)
        lp = self.lp = torch.log_softmax(z / beam.T, -1)
        out = torch.full((self.B, self.W, self.V), NEG_INF, dtype=self.dtype)
        self.ctc = torch.full((self.B, self.W, self.V), NEG_INF, dtype=self.dtype)
        for b in range(self.B):
            if beam.done[b]:
                continue
            for i in range(self.W):
                if not beam.alive(b, i):
                    continue
                g = beam.tokens[b][i]
                self.ctc[b, i] = scores(self.x[b], self.Tb[b], self.blank, self.eos, self.state[b][i], g[-1] if g else None)[0]
                out[b, i] = combine(self.ctc[b, i], lp[b, i], self.weight)
        return out.view(self.B * self.W, self.V)

    def advance(self, beam, was_done, stepped):
        """After beam.step: slot i of every utterance that took the step and goes on <- its parent's state extended by its token.
        stepped: what beam.step returned; was_done: beam.done before it."""
        for b in range(self.B):
            if was_done[b] or stepped[b] is None or beam.done[b]:
                continue
            old = self.state[b]
            new = [None] * self.W
            for i, (p, v, _, _) in enumerate(stepped[b]["winners"]):
                if beam.alive(b, i):
                    g = beam.tokens[b][i]
                    new[i] = extend(self.x[b], self.Tb[b], self.blank, old[p], g[-2] if len(g) >= 2 else None, v)
            self.state[b] = new


def search(logits_of, scorer, B, W, V, bos, eos, min_steps, max_steps, temperature=1.0, length_norm=True, shadow=None):
    """tests/_s2s_beam_ref.search with the scorer's extra at every step.  shadow: a second PrefixScorer (float32, say) carried along
    the SAME hypotheses, scoring its own logits where it has a source of them (shadow.logits_of); per step shadow.extras gets
    (the shadow's extra, the shadow's lp, the scorer's lp), each (B W, V).  -> (BeamRef, [per-step output of BeamRef.step],
    [the extras (B W, V)], [the prefixes fed])."""
    from tests._s2s_beam_ref import BeamRef
    ref = BeamRef(B, W, V, max_steps, eos, min_steps, temperature, length_norm)
    trace, extras, fed = [], [], []
    if shadow is not None:
        shadow.extras = []
    while not all(ref.done):
        n = max(ref.n[b] for b in range(B) if not ref.done[b])
        prefixes = torch.tensor([([bos] + ref.tokens[b][i] + [eos] * n)[:n + 1] for b in range(B) for i in range(W)], dtype=torch.int64)
        prefixes[(prefixes < 0) | (prefixes >= V)] = 0
        logits = logits_of(prefixes)
        ex = scorer.extra(ref, logits) if scorer is not None else None
        if shadow is not None:                                # (its own logits where it has a source of them: shadow.logits_of)
            sx = shadow.extra(ref, shadow.logits_of(prefixes) if hasattr(shadow, "logits_of") else logits)
            shadow.extras.append((sx, shadow.lp.reshape(sx.shape), scorer.lp.reshape(sx.shape)))
        was_done = list(ref.done)
        out = ref.step(logits, extra=ex)
        for s in (scorer, shadow):
            if s is not None:
                s.advance(ref, was_done, out)
        trace.append(out)
        extras.append(ex)
        fed.append(prefixes)
    return ref, trace, extras, fed

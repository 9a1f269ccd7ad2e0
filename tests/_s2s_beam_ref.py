"""The seq2seq beam search of DESIGN.md §I.22 restated on the host in float64, with no cache and no kernel: what
tests/test_s2s_beam_*.py hold smx_s2s_beam_select and decoders.seq2seq.beam_search to.

R = B W hypothesis rows, utterance b owns rows [b W, (b + 1) W).  Per utterance and step, n tokens so far:
  1. lp[r, v] = log_softmax(z[r] / T)[v].
  2. candidates score[r] + lp[r, v] (+ extra[r, v]); none from a dead row (score -inf), none for v == eos while n < min_steps, none that
     is NaN or -inf.  At n = 0 only row b W is alive.
  3. the best W of them, by score descending, then by the flat index (r - b W) V + v ascending.
  4. the i-th winner (parent p, token v) becomes slot i: the parent's tokens / log-probabilities / ancestors plus this step's.
  5. a winner with v == eos enters the pool (eos stored and counted; final score = sum / length under length normalisation, else sum);
     the pool keeps the best W by final score, ties to the earlier insertion; the slot is dead (score -inf, next input eos).
  6. the utterance ends when the pool holds W entries or at n + 1 == cap, where every winner enters the pool as it is.
  7. the result: the pool sorted by final score (the earlier insertion first among equals).
`step` is driven by given logits; `search` by a function of the prefixes (the whole prefix again for every token)."""
import math

import torch

NEG_INF = float("-inf")


class BeamRef:
    def __init__(self, B, W, V, cap, eos, min_steps=0, temperature=1.0, length_norm=True):
        self.B, self.W, self.V, self.cap, self.eos, self.min_steps, self.T, self.norm = B, W, V, cap, eos, min_steps, float(temperature), length_norm
        self.score = torch.full((B, W), NEG_INF, dtype=torch.float64)
        self.score[:, 0] = 0.0
        self.tokens = [[[] for _ in range(W)] for _ in range(B)]       # per slot: the tokens so far (a dead slot: n x eos)
        self.lps = [[[] for _ in range(W)] for _ in range(B)]
        self.anc = [[[] for _ in range(W)] for _ in range(B)]          # per slot: the global row that held each position's key
        self.tok = [[None] * W for _ in range(B)]                      # the next input per slot (None: the caller's bos)
        self.pool = [[] for _ in range(B)]                             # dicts: final, sum, tokens, lps, seq
        self.ins = [0] * B
        self.events = [[] for _ in range(B)]                           # what became of every entry offered to the pool
        self.n = [0] * B
        self.done = [False] * B

    def step(self, logits, extra=None):
        """logits (R, V) (any float dtype; read as float64), extra (R, V) or None.  -> per utterance None (done before the step) or
        dict(winners = [(parent, token, score, lp)], gaps = the float64 differences between adjacent ranks 1 .. W + 1 of the
        candidates - inf where a rank does not exist, twins = per gap whether the two candidates are the same parent's with equal
        logits: an exact tie on any arithmetic, which the column order resolves)."""
        B, W, V = self.B, self.W, self.V
        z = logits.detach().double().cpu().view(B, W, V)
        ex = None if extra is None else extra.detach().double().cpu().view(B, W, V)
        lp_all = torch.log_softmax(z / self.T, -1)
        out = []
        for b in range(B):
            if self.done[b]:
                out.append(None)
                continue
            n = self.n[b]
            cs = self.score[b][:, None] + lp_all[b] + (ex[b] if ex is not None else 0.0)
            cs = torch.where(torch.isnan(cs), torch.full_like(cs, NEG_INF), cs)
            if n < self.min_steps and 0 <= self.eos < V:
                cs[:, self.eos] = NEG_INF
            vals, flat = torch.sort(cs.reshape(-1), descending=True, stable=True)     # stable: equal scores keep the flat order
            nwin = min(W, int((vals > NEG_INF).sum()))
            winners = [(int(flat[i]) // V, int(flat[i]) % V, float(vals[i])) for i in range(nwin)]
            gaps = [(float(vals[i]) - float(vals[i + 1])) if (i + 1 < vals.numel() and vals[i + 1] > NEG_INF) else math.inf
                    for i in range(nwin)]
            twins = [i + 1 < vals.numel() and int(flat[i]) // V == int(flat[i + 1]) // V and
                     float(z[b, int(flat[i]) // V, int(flat[i]) % V]) == float(z[b, int(flat[i + 1]) // V, int(flat[i + 1]) % V])
                     for i in range(nwin)]
            last = n + 1 >= self.cap
            new = []
            for p, v, s in winners:
                lp = float(lp_all[b, p, v])
                toks, lps = self.tokens[b][p] + [v], self.lps[b][p] + [lp]
                if v == self.eos or last:
                    self._insert(b, dict(final=s / (n + 1) if self.norm else s, sum=s, tokens=toks, lps=lps))
                    new.append(None)
                else:
                    new.append((s, toks, lps, self.anc[b][p] + [b * W + p], v))
            new += [None] * (W - len(new))
            for i, slot in enumerate(new):
                if slot is None:
                    self.score[b, i], self.tokens[b][i], self.lps[b][i], self.tok[b][i] = NEG_INF, [self.eos] * (n + 1), [0.0] * (n + 1), self.eos
                    self.anc[b][i] = [-1] * (n + 1)
                else:
                    self.score[b, i], self.tokens[b][i], self.lps[b][i], self.anc[b][i], self.tok[b][i] = slot
            self.n[b] = n + 1
            if len(self.pool[b]) >= W or last or all(s is None for s in new):
                self.done[b] = True
            out.append(dict(winners=[(p, v, s, float(lp_all[b, p, v])) for p, v, s in winners], gaps=gaps, twins=twins))
        return out

    def _insert(self, b, entry):
        pool = self.pool[b]
        entry["seq"] = self.ins[b]
        if len(pool) < self.W:
            pool.append(entry)
            self.ins[b] += 1
            self.events[b].append("append")
            return
        worst = min(range(len(pool)), key=lambda e: (pool[e]["final"], -pool[e]["seq"]))   # the lowest final, the latest of equals
        if entry["final"] > pool[worst]["final"]:
            pool[worst] = entry
            self.ins[b] += 1
            self.events[b].append("replace")
        else:
            self.events[b].append("refuse")

    def alive(self, b, i):
        return float(self.score[b, i]) > NEG_INF

    def result(self, b):
        """The pool of utterance b, best first."""
        return sorted(self.pool[b], key=lambda e: (-e["final"], e["seq"]))


def search(logits_of, B, W, V, bos, eos, min_steps, max_steps, temperature=1.0, length_norm=True):
    """The whole search driven by logits_of(prefixes (B W, n + 1) int64 on the CPU, bos first) -> (B W, V): no cache, the whole prefix
    again at every step.  -> (BeamRef, [the per-step output of BeamRef.step])."""
    ref = BeamRef(B, W, V, max_steps, eos, min_steps, temperature, length_norm)
    trace = []
    while not all(ref.done):
        n = max(ref.n[b] for b in range(B) if not ref.done[b])
        # (a finished utterance stopped earlier: its rows are padded with eos, their logits are not read)
        prefixes = torch.tensor([([bos] + ref.tokens[b][i] + [eos] * n)[:n + 1] for b in range(B) for i in range(W)], dtype=torch.int64)
        prefixes[(prefixes < 0) | (prefixes >= V)] = 0               # (an eos outside the vocabulary, in rows that are not read)
        trace.append(ref.step(logits_of(prefixes)))
    return ref, trace

"""Plain restatement of the CHUNKED transducer beam search for the tests: the search of tests/_tbeam_ref.py written as
an expansion-at-a-time state machine with an explicit pause at a chunk's last frame and an explicit resume, float64 on the CPU, one
stream at a time with Python lists.  It is its own loop - it never calls _tbeam_ref.search - and shares only the arithmetic pieces
(_greedy_ref._lstm_step, _rnnlm_ref.run) and the key.  tests/test_tbeam_stream_cpu.py holds it to search() on every prefix.

The state between two expansions is what the device keeps: the open list A and the closed list Bh in insertion order, the frame's
expansion count, the STAGED hypothesis (already removed from A), the counters.  feed(frames):
    no frames, or a dead stream: nothing.
    otherwise the chunk-local frame index goes back to 0 - nothing is picked again - and, per expansion: expand the staged hypothesis
    at frame t; then the frame ends on "count" / "cap" / "empty" / "state" exactly as in _tbeam_ref.search, or the best of A is removed
    and staged.  A frame end advances t and the stream's frame count; at the chunk's last frame the RESULT is written (Bh sorted by key,
    stable - on a copy: Bh keeps its insertion order) and then the ordinary turnover happens all the same: A = Bh, Bh = [], the best
    of A removed and staged.  An empty Bh at a frame end has nothing to go on from: the stream is dead (overflow |= 4)."""
import torch

from tests import _greedy_ref as G
from tests import _rnnlm_ref as LM
from tests import _tbeam_ref as R


def _best(hyps, dt):
    return int(torch.argmax(torch.stack([R._key(h, dt) for h in hyps])))      # (the first maximum)


class Stream:
    def __init__(self, p, blank, W, lm=None, lm_weight=R.LM_WEIGHT, state_beam=R.STATE_BEAM, expand_beam=R.EXPAND_BEAM, E=None, U=None,
                 dtype=torch.float64):
        assert U is not None, "a stream has no T to derive max_symbols from"
        self.p, self.blank, self.W, self.lm, self.dt = p, blank, W, lm, dtype
        self.lm_weight, self.state_beam, self.expand_beam = lm_weight, state_beam, expand_beam
        self.E, self.U = (4 * W if E is None else E), U
        self.start()

    def start(self):
        zero = torch.zeros(1, self.p["w_hh"].shape[1], dtype=self.dt)
        self.staged = dict(pred=[self.blank], s=torch.zeros((), dtype=self.dt), dec=(zero, zero), lm=None)
        self.A, self.Bh, self.nexp = [], [], 0
        self.overflow, self.expansions, self.frames, self.exits, self.dead = 0, 0, 0, [], False
        self.hyps = [([], 0.0, 0.0)]                                          # no frame yet: the empty hypothesis, score 0

    def result(self):
        return dict(hyps=list(self.hyps), overflow=self.overflow, expansions=self.expansions, frames=self.frames, exits=list(self.exits))

    def _expand(self, enc_t):
        """The staged hypothesis' children at one frame into A / Bh (the body of _tbeam_ref.search's loop)."""
        p, dt, W, blank, a = self.p, self.dt, self.W, self.blank, self.staged
        tok = torch.tensor([a["pred"][-1]])
        h2, c2 = G._lstm_step(p, tok, a["dec"][0], a["dec"][1], blank, dt)
        pdec = h2 @ p["w_proj"].to(dt).t()
        z = (G.gelu(enc_t.to(dt) + pdec) @ p["w_lin"].to(dt).t() + p["b_lin"].to(dt)).view(-1)
        lp = torch.log_softmax(z, -1)
        if self.lm is not None:
            r = LM.run(self.lm, tok.view(1, 1), R.LM_LAYERS, hx=a["lm"], dtype=dt)
            lm_lp = torch.log_softmax(r["logits"].view(-1).to(dt), -1)
            lm_state = (r["hn"], r["cn"])
        v, idx = torch.sort(lp, descending=True, stable=True)
        capped = len(a["pred"]) - 1 >= self.U
        if capped:
            self.overflow |= 2
        best = v[0] if int(idx[0]) != blank else v[1]
        blank_in = False
        for j in range(W):
            k = int(idx[j])
            if k == blank:
                blank_in = True
                self.Bh.append(dict(pred=a["pred"], s=a["s"] + v[j], dec=a["dec"], lm=a["lm"]))
            elif not capped and v[j] >= best - self.expand_beam:
                s = a["s"] + v[j]
                if self.lm is not None:
                    s = s + self.lm_weight * lm_lp[k]
                self.A.append(dict(pred=a["pred"] + [k], s=s, dec=(h2, c2), lm=lm_state if self.lm is not None else None))
        if capped and not blank_in:
            self.Bh.append(dict(pred=a["pred"], s=a["s"] + lp[blank], dec=a["dec"], lm=a["lm"]))

    def _frame_ends(self):
        """After an expansion: the exit that ends the frame, or None with the next hypothesis removed from A and staged."""
        dt, W = self.dt, self.W
        if len(self.Bh) >= W:
            return "count"
        if self.nexp >= self.E:
            self.overflow |= 1
            while len(self.Bh) < W and self.A:
                self.Bh.append(self.A.pop(_best(self.A, dt)))
            return "cap"
        if not self.A:
            return "empty"
        ia = _best(self.A, dt)
        if self.Bh and self.Bh[_best(self.Bh, dt)]["s"] >= self.state_beam + self.A[ia]["s"]:
            return "state"
        self.staged = self.A.pop(ia)
        return None

    def feed(self, frames):
        """frames (n, J), n >= 0: one chunk.  -> result()."""
        n = frames.shape[0]
        if self.dead or n == 0:
            return self.result()
        t = 0                                                                 # the resume: the chunk-local frame index, nothing else
        while t < n:
            self._expand(frames[t])
            self.nexp += 1
            self.expansions += 1
            why = self._frame_ends()
            if why is None:
                continue
            self.exits.append(why)
            t += 1
            self.frames += 1
            if t >= n or not self.Bh:                                         # the pause: the result, on a copy of the closed list
                rest, order = list(range(len(self.Bh))), []
                while rest:
                    order.append(rest.pop(_best([self.Bh[r] for r in rest], self.dt)))
                self.hyps = [(self.Bh[i]["pred"][1:], float(self.Bh[i]["s"]), float(R._key(self.Bh[i], self.dt))) for i in order]
                if not self.Bh:
                    self.dead = True
                    self.overflow |= 4
                    break
            self.A, self.Bh, self.nexp = self.Bh, [], 0                       # the turnover, at a pause as at any frame end
            self.staged = self.A.pop(_best(self.A, self.dt))
        return self.result()


def feed_in_chunks(stream, enc1, sizes):
    """Feed enc1 (T, J) to a stream in chunks of the given sizes -> [(frames so far, result)] after every chunk."""
    out, at = [], 0
    for n in sizes:
        out.append((at + n, stream.feed(enc1[at:at + n])))
        at += n
    return out

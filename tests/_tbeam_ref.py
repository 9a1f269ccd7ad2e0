"""Plain restatement of transducer beam search with an LM for the tests (SpeechBrain's transducer_beam_search_decode, written from
memory - DESIGN.md §I.25 - plus the two caps the device search needs), in torch on the CPU, one utterance at a time with Python lists.
Default float64 - the yardstick of tests/test_tbeam_gpu.py, itself checked against an independent loop built from torch.nn.LSTMCell /
torch.nn.LSTM in tests/test_tbeam_cpu.py.  The same loop in float32 with h, pdec and a rounded to the operand dtype (and the LM's
roundings of tests/_rnnlm_ref.py) is the EMULATION: what the number formats alone cost.  Nothing here calls the code under test; the
arithmetic pieces are those of tests/_greedy_ref.py and tests/_rnnlm_ref.py.

A hypothesis is (pred, s, dec, lm): pred starts as [blank]; dec / lm are the prediction-network / LM states BEFORE pred[-1] is consumed
(zeros at the start); key = s / len(pred).  Per frame t:  A, B = B, [];  loop:
    len(B) >= W: the frame ends ("count")
    the frame has had E expansions: B is filled up to W with the best of A by key, overflow |= 1, the frame ends ("cap")
    A is empty: the frame ends ("empty"; only the symbol cap can empty it)
    a = best of A by key (first in list order on a tie);  B not empty, b = best of B by key, and b.s >= state_beam + a.s: the frame
    ends ("state")
    remove a;  (out, dec') = prediction network on a.pred[-1] from a.dec;  lp = log_softmax(W_lin act(enc[t] + out) + b_lin);
    (lm_lp, lm') = log_softmax(LM(a.pred[-1], a.lm));  top = the W largest of lp (value descending, index ascending);
    best = top[0], or top[1] if top[0] is the blank;  for (v, k) in top:  k == blank: B += (a.pred, a.s + v, a.dec, a.lm);
    else v >= best - expand_beam: A += (a.pred + [k], a.s + v + lm_weight lm_lp[k], dec', lm').
    A hypothesis of U symbols (len(pred) - 1 >= U) gets no child but the blank's, which it always gets; overflow |= 2.
The result: B sorted by key, descending, stable; pred[1:] of each."""
import functools

import torch

from tests import _greedy_ref as G
from tests import _rnnlm_ref as LM

BLANK_BIAS = 1.5            # added to the blank's bias of _greedy_ref.make_case, so that the blank sits in the top-k of most expansions
LM_WEIGHT, STATE_BEAM, EXPAND_BEAM = 0.5, 2.3, 2.3       # the recipe's
LM_LAYERS = 2

# name -> (T, V, H, J, blank, W, seed, pool, rows without the LM, rows with it, (LM E, LM H, LM dnn)).  The utterances of a case are
# rows of ONE _greedy_ref.make_case(pool, T, ...) batch: the first rows of the pool at which the case is ADMISSIBLE
# (tests/test_tbeam_cpu.py::test_cases_are_admissible asserts it on the reference alone), found once and written down here.
CASES = {
    "small": (12, 20, 64, 64, 0, 4, 0, 48, (0, 1, 2), (0, 1, 3), (32, 32, 32)),
    "blank7": (16, 30, 32, 64, 7, 4, 0, 48, (0, 5), (3, 5), (32, 32, 32)),
    "v300": (10, 300, 64, 128, 150, 5, 0, 48, (0, 3), (0, 2), (32, 32, 32)),
    "b17": (6, 12, 32, 64, 3, 3, 0, 96, (1, 2, 3, 4, 5, 8, 11, 12, 13, 15, 16, 18, 19, 20, 21, 23, 24), (1, 2, 3, 5, 8, 11, 15, 16, 20, 21, 24, 27, 29, 30, 32, 33, 34), (32, 32, 32)),
    "w10": (8, 40, 32, 64, 0, 10, 0, 64, (3, 7), (2, 3), (32, 32, 32)),
    "recipe": (6, 1000, 512, 640, 0, 10, 0, 24, (1, 6), (1, 15), (128, 256, 32)),
    "tie": (12, 12, 32, 64, 0, 4, 0, 48, (1, 2), (1, 2), (32, 32, 32)),
}
# the tie case: W_lin rows 5 and 9 (and their biases) are identical (_greedy_ref.make_case(tie=...)), so the two columns hold bit-equal
# logits in every arithmetic: the top-k must order them by index, their children get equal sums (without the LM) and the pick of `a` sees
# equal keys, which go to the earlier insertion.  Decisions whose margin is exactly 0 are logged as ties and left out of the margin.
TIES = {"tie": (5, 9)}
N_ROWS = {"small": 3, "blank7": 2, "v300": 2, "b17": 17, "w10": 2, "recipe": 2, "tie": 2}
SMALL_LENGTHS = (12, 0, 7)  # the absolute lengths of the small case's three rows
# the cap case (B, T, V, H, J, blank, W, seed, max_expansions, max_symbols): _greedy_ref.make_case as it is - the blank at its median
# bias, a model whose frames run away - under caps small enough that both are hit
CAP = (2, 12, 20, 64, 64, 0, 4, 0, 3, 8)


@functools.lru_cache(maxsize=None)
def pool(name, dtype=torch.float32):
    """(params, enc (pool, T, J), blank, W, lm params) of a case, made once and shared; treat as read-only."""
    T, V, H, J, blank, W, seed, n, _, _, (lE, lH, lD) = CASES[name]
    p, enc = G.make_case(n, T, V, H, J, blank, seed, dtype, tie=TIES.get(name))
    p["b_lin"][blank] += BLANK_BIAS
    lm = LM.make_params(V, lE, lH, LM_LAYERS, lD, seed + 5)
    return p, enc, blank, W, lm


def case(name, use_lm, dtype=torch.float32):
    """-> (params, enc (B, T, J) the case's rows, blank, W, lm params or None, lengths (B) list)."""
    p, enc, blank, W, lm = pool(name, dtype)
    rows = CASES[name][9 if use_lm else 8]
    e = enc[list(rows)]
    lengths = list(SMALL_LENGTHS) if name == "small" else [e.shape[1]] * e.shape[0]
    return p, e, blank, W, (lm if use_lm else None), lengths


def _key(h, dt):
    return h["s"] / torch.tensor(float(len(h["pred"])), dtype=dt)


def _log_margin(log, what, margin):
    if margin == 0.0:
        log["ties"].append(what)
    else:
        log["margins"].append((what, margin))


def _best(hyps, dt, log, what):
    """The best of a list by key, the first on a tie; logs the margin to the runner-up (an exact tie: logged as a tie instead)."""
    ks = torch.stack([_key(h, dt) for h in hyps])
    i = int(torch.argmax(ks))                    # (torch.argmax returns the first maximum)
    if len(hyps) > 1:
        rest = torch.cat([ks[:i], ks[i + 1:]])
        _log_margin(log, what, float(ks[i] - rest.max()))
    log["q"].append(float(ks[i]))
    return i


def search(p, enc1, blank, W, lm=None, lm_weight=LM_WEIGHT, state_beam=STATE_BEAM, expand_beam=EXPAND_BEAM, E=None, U=None, n_frames=None,
           dtype=torch.float64):
    """One utterance: enc1 (T, J).  -> dict: hyps [(tokens, sum, key)] best first, overflow, expansions, frames, exits (per frame: "count" /
    "state" / "cap" / "empty"), pruned (children dropped by expand_beam), margins [(decision, margin)], ties [decision] (the decisions
    between exactly equal values, which list or index order settles), q (every quantity that entered a
    decision, in order), traj (per expansion: t, tok, h, c, h2, c2, pdec, z and the LM's tensors)."""
    dt = dtype
    T = enc1.shape[0] if n_frames is None else int(n_frames)
    E = 4 * W if E is None else E
    U = 2 * enc1.shape[0] + 8 if U is None else U
    H = p["w_hh"].shape[1]
    Wl, bl, Wp = p["w_lin"].to(dt), p["b_lin"].to(dt), p["w_proj"].to(dt)
    zero = torch.zeros(1, H, dtype=dt)
    log = {"margins": [], "ties": [], "q": []}
    out = {"overflow": 0, "expansions": 0, "exits": [], "pruned": 0, "traj": []}
    Bh = [dict(pred=[blank], s=torch.zeros((), dtype=dt), dec=(zero, zero), lm=None)]
    for t in range(T):
        A, Bh, nexp = Bh, [], 0
        while True:
            if len(Bh) >= W:
                out["exits"].append("count")
                break
            if nexp >= E:
                out["overflow"] |= 1
                while len(Bh) < W and A:
                    Bh.append(A.pop(_best(A, dt, log, "cap fill")))
                out["exits"].append("cap")
                break
            if not A:
                out["exits"].append("empty")
                break
            ia = _best(A, dt, log, "pick a")
            a = A[ia]
            if Bh:
                b = Bh[_best(Bh, dt, log, "pick b")]
                log["margins"].append(("state_beam", abs(float(b["s"] - (state_beam + a["s"])))))
                log["q"] += [float(b["s"]), float(a["s"])]
                if b["s"] >= state_beam + a["s"]:
                    out["exits"].append("state")
                    break
            A.pop(ia)
            nexp += 1
            out["expansions"] += 1
            tok = torch.tensor([a["pred"][-1]])
            h2, c2 = G._lstm_step(p, tok, a["dec"][0], a["dec"][1], blank, dt)
            pdec = h2 @ Wp.t()
            z = (G.gelu(enc1[t].to(dt) + pdec) @ Wl.t() + bl).view(-1)
            lp = torch.log_softmax(z, -1)
            rec = dict(t=t, tok=int(tok), h=a["dec"][0], c=a["dec"][1], h2=h2, c2=c2, pdec=pdec, z=z)
            if lm is not None:
                r = LM.run(lm, tok.view(1, 1), LM_LAYERS, hx=a["lm"], dtype=dt)
                lm_lp = torch.log_softmax(r["logits"].view(-1).to(dt), -1)
                lm_state = (r["hn"], r["cn"])
                rec.update(lm_hx=a["lm"], lm_h2=r["hn"], lm_c2=r["cn"], lm_logits=r["logits"].view(-1))
            out["traj"].append(rec)
            v, idx = torch.sort(lp, descending=True, stable=True)            # (stable: equal values keep their index order)
            v, idx = v[:W + 1], idx[:W + 1]
            for j in range(W):
                _log_margin(log, "top-k", float(v[j] - v[j + 1]))
            log["q"] += [float(x) for x in v]
            capped = len(a["pred"]) - 1 >= U
            if capped:
                out["overflow"] |= 2
            best = v[0] if int(idx[0]) != blank else v[1]
            blank_in = False
            for j in range(W):
                k = int(idx[j])
                if k == blank:
                    blank_in = True
                    Bh.append(dict(pred=a["pred"], s=a["s"] + v[j], dec=a["dec"], lm=a["lm"]))
                    log["q"].append(float(Bh[-1]["s"]))
                    continue
                if capped:
                    continue
                log["margins"].append(("expand_beam", abs(float(v[j] - (best - expand_beam)))))
                if v[j] >= best - expand_beam:
                    s = a["s"] + v[j]
                    if lm is not None:
                        s = s + lm_weight * lm_lp[k]
                    A.append(dict(pred=a["pred"] + [k], s=s, dec=(h2, c2), lm=lm_state if lm is not None else None))
                    log["q"].append(float(s))
                else:
                    out["pruned"] += 1
            if capped and not blank_in:
                Bh.append(dict(pred=a["pred"], s=a["s"] + lp[blank], dec=a["dec"], lm=a["lm"]))
    order = []
    rest = list(range(len(Bh)))
    while rest:                                                               # sorted by key, descending, stable
        i = _best([Bh[r] for r in rest], dt, log, "final sort")
        order.append(rest.pop(i))
    out["hyps"] = [(Bh[i]["pred"][1:], float(Bh[i]["s"]), float(_key(Bh[i], dt))) for i in order]
    out["frames"] = T
    out.update(log)
    return out


def ref_and_emu(p, enc1, blank, W, lm, **kw):
    """(float64 reference, float32 emulation) of one utterance's search."""
    return search(p, enc1, blank, W, lm, **kw), search(p, enc1, blank, W, lm, dtype=torch.float32, **kw)


def deviation(ref, emu):
    """The emulation's largest distance from the reference over every quantity that entered a decision (inf: another trajectory)."""
    if [h[0] for h in ref["hyps"]] != [h[0] for h in emu["hyps"]] or len(ref["q"]) != len(emu["q"]):
        return float("inf")
    return max((abs(a - b) for a, b in zip(ref["q"], emu["q"])), default=0.0)


def admissible(ref, emu):
    """-> (ok, smallest margin, deviation): the emulation returns the reference's hypotheses in its order, every decision's margin is at
    least 8 x the emulation's largest deviation (exact ties apart, which must be the same decisions in both), no cap is hit and the best
    hypothesis is not empty."""
    dev = deviation(ref, emu)
    mg = min((m for _, m in ref["margins"]), default=float("inf"))
    ok = dev < float("inf") and mg >= 8 * dev and ref["ties"] == emu["ties"] and ref["overflow"] == 0 and emu["overflow"] == 0 and len(ref["hyps"][0][0]) > 0
    return ok, mg, dev


@functools.lru_cache(maxsize=None)
def reference(name, use_lm):
    """The float64 searches of a case's rows (a list of search() dicts), made once and shared; treat as read-only."""
    p, enc, blank, W, lm, lengths = case(name, use_lm)
    return [search(p, enc[b], blank, W, lm, n_frames=lengths[b]) for b in range(enc.shape[0])]

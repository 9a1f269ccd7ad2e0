"""CPU restatement of the CTC head of csrc/ctc.hip (speechbrain.nnet.losses.ctc_loss -> torch.nn.functional.ctc_loss with
zero_infinity=True), stage by stage and each stage from GIVEN inputs, so that one stage's rounding is not another stage's tolerance:
`abs_lengths` (relative -> absolute lengths), `ctc_lattice` (log-probabilities -> forward variables, -log P and the log occupancies
alpha + beta - y, by explicit forward and backward recursions vectorised over the state), `ctc_grad` (occupancies -> the gradient
in torch's convention) and `ctc_brute_force` (the sum over every frame labelling, for tiny cases).  Plain numpy; float64 unless a
`dtype` is passed: the same recursions in float32 are the floor the kernel tests derive their bars from.  "log 0" is -inf."""
import itertools
import math

import numpy as np
import torch


def abs_lengths(T, S, input_lens, target_lens):
    """SpeechBrain's relative lengths -> absolute (round(rel * T), round(rel * S)), clamped to [0, T] / [0, S] as the kernels'
    min(...) does.  The product is rounded in fp32, as SpeechBrain, nnet.losses.ctc_loss and the oracle do: at a tie the fp32 and the
    fp64 product differ (0.1f * 25 is 2.5 in fp32 -> 2, but 2.50000004 in fp64 -> 3)."""
    tl = (input_lens.float() * T).round().long().clamp(0, T)
    sl = (target_lens.float() * S).round().long().clamp(0, S)
    return tl, sl


def _np(x, dtype):
    """Any tensor / array -> numpy `dtype` at exactly its values (a bf16 or fp32 value is exact in both float32 and float64)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=dtype)


def ext_labels(tg, Sb, blank):
    """The extended label sequence l': the blank at even s, target s >> 1 at odd s; 2 Sb + 1 states."""
    lab = np.full(2 * Sb + 1, blank, dtype=np.int64)
    lab[1::2] = np.asarray(tg, dtype=np.int64)[:Sb]
    return lab


def _lse3(a, b, c):
    """log(exp a + exp b + exp c), elementwise, -inf where all three are -inf; in the dtype of the operands."""
    m = np.maximum(a, np.maximum(b, c))
    dead = np.isneginf(m)
    ms = np.where(dead, 0, m).astype(a.dtype)
    out = ms + np.log(np.exp(a - ms) + np.exp(b - ms) + np.exp(c - ms))
    return np.where(dead, -np.inf, out).astype(a.dtype)


def _shift(x, n, fill=-np.inf):
    """y[s] = x[s - n] (n > 0) or x[s + |n|] (n < 0), `fill` where that runs off the end."""
    out = np.full_like(x, fill)
    if n > 0:
        out[n:] = x[:-n] if n < len(x) else []
    else:
        out[:n] = x[-n:] if -n < len(x) else []
    return out


def ctc_lattice(lp, tg, Tb, Sb, blank, dtype=np.float64):
    """One utterance: lp (>= Tb, V) log-probabilities (used at exactly their values; they need not be normalised), tg its targets
    (>= Sb), L = 2 Sb + 1 states.
      alpha(0, s) = y(0, s) for s < 2, alpha(t, s) = lse(alpha(t-1, s), alpha(t-1, s-1), [l'_s != l'_{s-2}] alpha(t-1, s-2)) + y(t, s)
      beta(Tb-1, s) = y(Tb-1, s) for s >= L - 2, beta(t, s) = lse(beta(t+1, s), beta(t+1, s+1), [l'_s != l'_{s+2}] beta(t+1, s+2)) + y(t, s)
      -log P = -lse(alpha(Tb-1, L-1), alpha(Tb-1, L-2)),  occ = alpha + beta - y (-inf where alpha or beta is)
    with y(t, s) = lp[t, l'_s].  -> (alpha (Tb, L), nll (float, +inf when no alignment exists), occ (Tb, L)).  Tb = 0: no frame, no
    alignment, nll = +inf as the kernel has it (torch gives 0 for Sb = 0 there: the same after zero_infinity)."""
    lp = _np(lp, dtype)
    L = 2 * Sb + 1
    lab = ext_labels(tg, Sb, blank)
    ninf = dtype(-np.inf)
    alpha = np.full((Tb, L), ninf, dtype=dtype)
    occ = np.full((Tb, L), ninf, dtype=dtype)
    if Tb == 0:
        return alpha, math.inf, occ
    skip_a = np.zeros(L, dtype=bool)
    skip_a[2:] = lab[2:] != lab[:-2]                      # (false on the blanks: l'_s = l'_{s-2} = blank)
    skip_b = np.zeros(L, dtype=bool)
    skip_b[:-2] = lab[:-2] != lab[2:]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        alpha[0, :2] = lp[0, lab[:2]]
        for t in range(1, Tb):
            p = alpha[t - 1]
            alpha[t] = _lse3(p, _shift(p, 1), np.where(skip_a, _shift(p, 2), ninf)) + lp[t, lab]
        fin = _lse3(alpha[Tb - 1, L - 1:L], alpha[Tb - 1, L - 2:L - 1] if L > 1 else np.full(1, ninf, dtype=dtype), np.full(1, ninf, dtype=dtype))
        nll = -float(fin[0])
        beta = np.full(L, ninf, dtype=dtype)
        for t in range(Tb - 1, -1, -1):
            y = lp[t, lab]
            if t == Tb - 1:
                beta[max(L - 2, 0):] = y[max(L - 2, 0):]
            else:
                beta = _lse3(beta, _shift(beta, -1), np.where(skip_b, _shift(beta, -2), ninf)) + y
            dead = np.isneginf(alpha[t]) | np.isneginf(beta)
            occ[t] = np.where(dead, ninf, alpha[t] + beta - np.where(dead, 0, y))
    return alpha, nll, occ


def ctc_grad(lp, tg, Tb, Sb, blank, occ, nll, gscale, dtype=np.float64):
    """The gradient with respect to the log-probabilities in the convention csrc/ctc.hip documents (that of torch's ctc_loss
    backward): G[t, v] = gscale (exp(lp[t, v]) - exp(logsumexp_{s: l'_s = v} occ[t, s] + nll)); 0 for t >= Tb and when nll is
    infinite.  lp (T, V), occ (Tb, L) and nll are used at exactly their values.  -> G (T, V)."""
    lp = _np(lp, dtype)
    occ = _np(occ, dtype)
    G = np.zeros(lp.shape, dtype=dtype)
    if Tb == 0 or not math.isfinite(nll):
        return G
    lab = ext_labels(tg, Sb, blank)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = occ.max(axis=1, keepdims=True)                # finite: an aligned utterance has a live state in every frame
        e = np.exp(occ - m)
        mass = np.zeros((Tb, lp.shape[1]), dtype=dtype)
        for v in np.unique(lab):
            mass[:, v] = e[:, lab == v].sum(axis=1, dtype=dtype)
        shift = (m + dtype(nll)).astype(dtype)
        lab_p = np.where(mass > 0, np.exp(np.log(mass) + shift), 0).astype(dtype)
        G[:Tb] = dtype(gscale) * (np.exp(lp[:Tb]) - lab_p)
    return G


def ctc_brute_force(lp, tg, Tb, Sb, blank):
    """-log of the sum over every labelling of the Tb frames that collapses (merge repeats, then drop blanks) to tg[:Sb]."""
    lp = _np(lp, np.float64)
    V = lp.shape[1]
    want = [int(c) for c in np.asarray(tg)[:Sb]]
    terms = []
    for path in itertools.product(range(V), repeat=Tb):
        merged = [c for i, c in enumerate(path) if i == 0 or c != path[i - 1]]
        if [c for c in merged if c != blank] == want:
            terms.append(sum(lp[t, c] for t, c in enumerate(path)))
    terms = [x for x in terms if x != -math.inf]
    if not terms or Tb == 0:
        return math.inf
    m = max(terms)
    return -(m + math.log(sum(math.exp(x - m) for x in terms)))


def adjacent_repeats(tg, Sb):
    """The number of k with tg[k] == tg[k - 1], k < Sb: an alignment needs Sb + that many frames."""
    t = np.asarray(tg)[:Sb]
    return int((t[1:] == t[:-1]).sum()) if Sb > 1 else 0


def log_softmax_bwd_ref(dy, y, dtype=np.float64):
    """dX = dY - exp(Y) sum_v dY from given upstream gradient and log-probabilities (the formula of log_softmax_bwd_kernel)."""
    dy, y = _np(dy, dtype), _np(y, dtype)
    return (dy - np.exp(y) * dy.sum(axis=1, keepdims=True, dtype=dtype)).astype(dtype)

"""fp64 CPU restatement of the RNN-T (transducer) loss of speechbrain.nnet.losses.transducer_loss (torchaudio's rnnt_loss and
SpeechBrain's own implementation compute the same function; neither is installed here).  The forward variable runs over the
anti-diagonals t + u = d of the lattice, vectorised over u; gradients come from torch autograd.  Also a brute-force sum over
every alignment, which validates the recurrence on tiny lattices.

For the stage tests of the kernels (tests/test_transducer_kernels_gpu.py) the same function is also restated stage by stage, each
from GIVEN inputs: `row_stats` (logits -> lse, lp_blank, lp_y), `lattice` (per-cell log emissions -> forward variables, -log P and
the per-cell occupancies, by explicit forward and backward recursions) and `logit_grad` (the gradient of the logits from the
per-row coefficients)."""
import itertools
import math

import numpy as np
import torch

_NEG = -1e30            # "log 0": finite, so that autograd through logaddexp stays NaN-free


def abs_lengths(T, U, input_lens, target_lens):
    """SpeechBrain's relative lengths -> absolute (round(rel * T), round(rel * U)), clamped to [1, T] / [0, U] as the kernels do.
    The product is rounded in fp32, as SpeechBrain and nnet.losses.transducer_lengths do: at a tie the fp32 and the fp64 product
    differ (0.1f * 25 is 2.5 in fp32 -> 2, but 2.50000004 in fp64 -> 3)."""
    tl = (input_lens.float() * T).round().long().clamp(1, T)
    ul = (target_lens.float() * U).round().long().clamp(0, U)
    return tl, ul


def _nll_one(lp, tg, Tb, Ub, blank):
    """lp (T, U1, V) log-probabilities of one utterance -> -log P(y | x) on its Tb x (Ub + 1) lattice."""
    u = torch.arange(Ub + 1)
    lpb = lp[:Tb, :Ub + 1, blank]                                             # (Tb, Ub + 1)
    lpy = lp[:Tb, :Ub, :].gather(2, tg[:Ub].view(1, Ub, 1).expand(Tb, Ub, 1)).squeeze(2) if Ub > 0 else None
    neg = torch.full((Ub + 1,), _NEG, dtype=lp.dtype)
    prev = None
    for d in range(Tb + Ub):
        t = d - u
        valid = (t >= 0) & (t < Tb)
        if d == 0:
            cur = torch.where(u == 0, torch.zeros_like(neg), neg)
        else:
            tc = t.clamp(0, Tb - 1)
            a1 = prev + lpb[(t - 1).clamp(0, Tb - 1), u]
            a1 = torch.where(valid & (t >= 1), a1, neg)
            if Ub > 0:
                prev_sh = torch.cat([neg[:1], prev[:-1]])
                a2 = prev_sh + lpy[tc, (u - 1).clamp(0, Ub - 1)]
                a2 = torch.where(valid & (u >= 1), a2, neg)
            else:
                a2 = neg
            cur = torch.where(valid, torch.logaddexp(a1, a2), neg)
        prev = cur
    return -(prev[Ub] + lpb[Tb - 1, Ub])


def rnnt_nll(logits, targets, in_len, tgt_len, blank):
    """logits (B, T, U + 1, V) raw scores (any float dtype; computed in fp64), targets (B, U), ABSOLUTE lengths -> nll (B) fp64."""
    lp = logits.double().log_softmax(-1)
    return torch.stack([_nll_one(lp[b], targets[b].long(), int(in_len[b]), int(tgt_len[b]), blank) for b in range(lp.shape[0])])


def rnnt_loss(logits, targets, input_lens, target_lens, blank, reduction="mean"):
    """The reference of nnet.losses.transducer_loss (relative lengths)."""
    T, U = logits.shape[1], targets.shape[1]
    tl, ul = abs_lengths(T, U, input_lens, target_lens)
    nll = rnnt_nll(logits, targets, tl, ul, blank)
    return nll.mean() if reduction == "mean" else nll.sum() if reduction == "sum" else nll


def brute_force_nll(logits, targets, Tb, Ub, blank):
    """-log of the sum over every alignment of one utterance (logits (T, U + 1, V)): Tb blanks and Ub labels, the last step a blank
    from (Tb - 1, Ub)."""
    lp = logits.double().log_softmax(-1)
    terms = []
    for pos in itertools.combinations(range(Tb - 1 + Ub), Ub):            # which of the first Tb - 1 + Ub steps emit a label
        t = u = 0
        s = lp.new_zeros(())
        for step in range(Tb - 1 + Ub):
            if step in pos:
                s = s + lp[t, u, int(targets[u])]
                u += 1
            else:
                s = s + lp[t, u, blank]
                t += 1
        terms.append(s + lp[Tb - 1, Ub, blank])
    return -torch.logsumexp(torch.stack(terms), 0)


def joint_ref(enc, dec, act):
    """fp64 joint: act(enc (B, T, J)[:, :, None] + dec (B, U1, J)[:, None]) with act a torch module."""
    return act(enc.double()[:, :, None, :] + dec.double()[:, None, :, :])


def _lae(a, b):
    """log(exp a + exp b) in fp64, -inf safe."""
    m = max(a, b)
    if m == -math.inf:
        return -math.inf
    return m + math.log1p(math.exp(-abs(a - b)))


def lattice(lpb, lpy, Tb, Ub, with_beta=False):
    """Explicit fp64 forward and backward variables of ONE utterance from given per-cell log emissions (they need not be
    normalised): lpb[t, u] the blank at cell (t, u), lpy[t, u] the label u + 1 at cell (t, u) (read for u < Ub only); both
    (>= Tb, >= Ub + 1), any float dtype, used at exactly their values.
      alpha(0,0) = 0, alpha(t,u) = lae(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpy(t,u-1))
      beta(Tb-1,Ub) = lpb(Tb-1,Ub), beta(t,u) = lae(beta(t+1,u) + lpb(t,u), beta(t,u+1) + lpy(t,u)),  log P = beta(0,0)
      occ_blank(t,u) = exp(alpha + lpb + beta(t+1,u) - log P)   (beta(Tb,Ub) = 0, beta(Tb,u < Ub) = -inf)
      occ_y(t,u)     = exp(alpha + lpy + beta(t,u+1) - log P)   (0 at u = Ub)
    -> alpha (Tb, Ub + 1), -log P (from alpha), occ_blank, occ_y (Tb, Ub + 1), fp64 numpy; with_beta appends beta."""
    b_ = np.asarray(torch.as_tensor(lpb).double())
    y_ = np.asarray(torch.as_tensor(lpy).double())
    ninf = -math.inf
    alpha = np.full((Tb, Ub + 1), ninf)
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                alpha[t, u] = 0.0
                continue
            a1 = alpha[t - 1, u] + b_[t - 1, u] if t > 0 else ninf
            a2 = alpha[t, u - 1] + y_[t, u - 1] if u > 0 else ninf
            alpha[t, u] = _lae(a1, a2)
    nll = -(alpha[Tb - 1, Ub] + b_[Tb - 1, Ub])
    beta = np.full((Tb + 1, Ub + 2), ninf)               # one row and one column of "nothing follows"
    beta[Tb, Ub] = 0.0                                    # the terminal state after the last blank
    occ_b = np.zeros((Tb, Ub + 1))
    occ_y = np.zeros((Tb, Ub + 1))
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            vb = b_[t, u] + beta[t + 1, u]
            vy = y_[t, u] + beta[t, u + 1] if u < Ub else ninf
            beta[t, u] = _lae(vb, vy)
            occ_b[t, u] = math.exp(alpha[t, u] + vb + nll) if vb != ninf and math.isfinite(nll) else 0.0
            occ_y[t, u] = math.exp(alpha[t, u] + vy + nll) if vy != ninf and math.isfinite(nll) else 0.0
    out = (alpha, float(nll), occ_b, occ_y)
    return out + (beta[:Tb, :Ub + 1],) if with_beta else out


def row_stats(z, targets, blank):
    """z (B, T, U + 1, V) logits (any float dtype, used at exactly their values), targets (B, U) -> fp64 lse, lp_blank = z_blank -
    lse, lp_y = z_y - lse with y = targets[b, u] (0 on the u = U column, which emits no label), each (B, T, U + 1)."""
    z = z.double()
    B, T, U1, V = z.shape
    lse = torch.logsumexp(z, -1)
    lpb = z[..., blank] - lse
    lpy = torch.zeros_like(lse)
    if U1 > 1:
        idx = targets.long().view(B, 1, U1 - 1, 1).expand(B, T, U1 - 1, 1)
        lpy[:, :, :U1 - 1] = z[:, :, :U1 - 1].gather(3, idx).squeeze(3) - lse[:, :, :U1 - 1]
    return lse, lpb, lpy


def logit_grad(z, targets, blank, lse, gb, gy):
    """dz_v = [v = blank] g_b + [v = y] g_y - exp(z_v - lse) (g_b + g_y) per lattice row, fp64 (the formula in the header of
    csrc/transducer.hip); lse, gb, gy (B, T, U + 1), used at exactly their values."""
    z = z.double()
    B, T, U1, V = z.shape
    gb, gy, lse = gb.double(), gy.double(), lse.double()
    dz = -torch.exp(z - lse.unsqueeze(-1)) * (gb + gy).unsqueeze(-1)
    dz[..., blank] += gb
    if U1 > 1:
        idx = targets.long().view(B, 1, U1 - 1, 1).expand(B, T, U1 - 1, 1)
        dz[:, :, :U1 - 1].scatter_add_(3, idx, gy[:, :, :U1 - 1].unsqueeze(-1))
    return dz

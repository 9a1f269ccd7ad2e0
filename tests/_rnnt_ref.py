"""fp64 CPU restatement of the RNN-T (transducer) loss of speechbrain.nnet.losses.transducer_loss (torchaudio's rnnt_loss and
SpeechBrain's own implementation compute the same function; neither is installed here).  The forward variable runs over the
anti-diagonals t + u = d of the lattice, vectorised over u; gradients come from torch autograd.  Also a brute-force sum over
every alignment, which validates the recurrence on tiny lattices."""
import itertools

import torch

_NEG = -1e30            # "log 0": finite, so that autograd through logaddexp stays NaN-free


def abs_lengths(T, U, input_lens, target_lens):
    """SpeechBrain's relative lengths -> absolute (round(rel * T), round(rel * U)), clamped to [1, T] / [0, U] as the kernels do."""
    tl = (input_lens.double() * T).round().long().clamp(1, T)
    ul = (target_lens.double() * U).round().long().clamp(0, U)
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

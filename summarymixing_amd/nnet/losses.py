"""Losses of the recipes' heads: the CTC loss of the multitask head (recipe key ``ctc_cost``: speechbrain.nnet.losses.ctc_loss, which wraps
``torch.nn.functional.ctc_loss(..., zero_infinity=True)``; SpeechBrain is not vendored in the reference tree, the call
site is …/LibriSpeech/ASR/transducer/hparams/conformer_summarymixing_transducer.yaml:297-298) and the transducer (RNN-T)
loss the recipe trains on (recipe key ``transducer_cost``: speechbrain.nnet.losses.transducer_loss).  The forward/backward
variables and the gradients run in the HIP kernels of csrc/ctc.hip and csrc/transducer.hip; no CPU fallback.

The label-smoothed sequence losses of the second head: ``nll_loss`` (recipe key ``ce_cost``, …transducer.yaml:319-320),
``kldiv_loss`` (recipe key ``seq_cost``, …/LibriSpeech/ASR/transformer/hparams/branchformer_summarymixing.yaml:278-280) and
``seq_loss_from_logits``, the same two losses computed from raw logits without storing the log-probabilities (csrc/seqloss.hip)."""
import math

import torch

from .. import ops


class _CTC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, log_probs, targets, in_len, tgt_len, blank):
        B, T, V = log_probs.shape
        lp2 = ops.rows2d(log_probs if log_probs.is_contiguous() else log_probs.contiguous())
        nll, ws = ops.ctc_fwd(lp2, targets, in_len, tgt_len, B, T, blank)
        ctx.save_for_backward(lp2, targets, in_len, tgt_len, nll, ws)
        ctx.meta = (B, T, V, blank)
        return torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)      # zero_infinity=True

    @staticmethod
    def backward(ctx, gnll):
        lp2, targets, in_len, tgt_len, nll, ws = ctx.saved_tensors
        B, T, V, blank = ctx.meta
        g = ops.ctc_bwd(lp2, targets, in_len, tgt_len, B, T, blank, nll, gnll.float().contiguous(), ws)
        return g.view(B, T, V), None, None, None, None


def ctc_loss(log_probs, targets, input_lens, target_lens, blank_index, reduction="mean"):
    """speechbrain.nnet.losses.ctc_loss.  log_probs (B, T, V) log-softmax outputs (CUDA, fp32 or bf16); targets
    (B, S) integer tokens (padded); input_lens / target_lens RELATIVE lengths in (0, 1] as everywhere in SpeechBrain.
    targets of shape (B, 0) (no label in the whole batch) are accepted: every target is empty and the loss of an utterance is
    -sum_{t < T_b} log_probs[b, t, blank], as torch has it.  An utterance without an alignment (too few frames for its labels,
    no frame at all) has loss 0 and gradient 0 (zero_infinity=True)."""
    if not log_probs.is_cuda:
        raise RuntimeError("summarymixing_amd.nnet.losses.ctc_loss runs on the GPU only (no CPU fallback)")
    B, T, V = log_probs.shape
    in_len = (input_lens.to(log_probs.device) * T).round().to(torch.int32)
    tgt_len = (target_lens.to(log_probs.device) * targets.shape[1]).round().to(torch.int32)
    tg = targets.to(device=log_probs.device, dtype=torch.int32).contiguous()
    if tg.shape[1] == 0:                             # a (B, 0) tensor has no storage to point the kernels at: one column that
        tg = tg.new_zeros((B, 1))                    # is never read (every tgt_len is round(rel * 0) = 0)
    nll = _CTC.apply(log_probs, tg, in_len, tgt_len, int(blank_index))
    if reduction == "mean":                          # torch: each loss / target length (>= 1), then the batch mean
        return (nll / tgt_len.clamp(min=1).to(nll.dtype)).mean()
    if reduction == "sum":
        return nll.sum()
    if reduction == "batchmean":
        return nll.sum() / B
    if reduction == "batch":
        return nll / tgt_len.to(nll.dtype)           # SpeechBrain: per-utterance loss over its target length
    if reduction == "none":
        return nll
    raise ValueError(f"unknown reduction {reduction!r}")


class _RNNT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, in_len, tgt_len, blank):
        B, T, U1, V = logits.shape
        z2 = logits.reshape(-1, V)
        if not z2.is_contiguous():
            z2 = z2.contiguous()
        lse, lpb, lpy = ops.transducer_row_stats(z2, targets, B, T, U1, blank)
        nll, alpha = ops.transducer_loss_fwd(lpb, lpy, in_len, tgt_len, B, T, U1)
        ctx.save_for_backward(z2, targets, in_len, tgt_len, lse, lpb, lpy, alpha)
        ctx.meta = (B, T, U1, V, blank)
        return nll

    @staticmethod
    def backward(ctx, gnll):
        z2, targets, in_len, tgt_len, lse, lpb, lpy, alpha = ctx.saved_tensors
        B, T, U1, V, blank = ctx.meta
        gb, gy = ops.transducer_loss_bwd(lpb, lpy, alpha, gnll.float().contiguous(), in_len, tgt_len, B, T, U1)
        dz = ops.transducer_logit_grad(z2, targets, lse, gb, gy, B, T, U1, blank)
        return dz.view(B, T, U1, V), None, None, None, None


TRANSDUCER_REDUCTIONS = ("mean", "sum", "none")


def transducer_lengths(T, targets, input_lens, target_lens, device):
    """SpeechBrain's relative lengths -> absolute int32 lengths on the device (round(rel * T), round(rel * U)); padded int32 targets."""
    in_len = (input_lens.to(device) * T).round().to(torch.int32)
    tgt_len = (target_lens.to(device) * targets.shape[1]).round().to(torch.int32)
    return targets.to(device=device, dtype=torch.int32).contiguous(), in_len, tgt_len


def reduce_transducer(nll, reduction):
    if reduction == "mean":                          # torchaudio's rnnt_loss and SpeechBrain's own implementation: the batch mean
        return nll.mean()
    if reduction == "sum":
        return nll.sum()
    return nll


def transducer_loss(logits, targets, input_lens, target_lens, blank_index, reduction="mean", use_torchaudio=True):
    """speechbrain.nnet.losses.transducer_loss.  logits (B, T, U+1, V) raw joint-network scores (CUDA, fp32 or bf16; the
    log-softmax over V happens inside, in fp32); targets (B, U) padded tokens; input_lens / target_lens RELATIVE lengths.
    Per utterance -log P(y | x) on the RNN-T lattice, reduced by `reduction` ('mean' | 'sum' | 'none').  use_torchaudio is
    accepted and ignored (both SpeechBrain back-ends compute the same function)."""
    if reduction not in TRANSDUCER_REDUCTIONS:
        raise ValueError(f"unknown reduction {reduction!r} (transducer_loss: 'mean', 'sum' or 'none')")
    if not logits.is_cuda:
        raise RuntimeError("summarymixing_amd.nnet.losses.transducer_loss runs on the GPU only (no CPU fallback)")
    if logits.dim() != 4:
        raise ValueError(f"transducer_loss: logits (B, T, U+1, V) expected, got {tuple(logits.shape)}")
    B, T, U1, V = logits.shape
    if targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] != U1 - 1:
        raise ValueError(f"transducer_loss: targets (B, U) = ({B}, {U1 - 1}) expected, got {tuple(targets.shape)}")
    if not 0 <= int(blank_index) < V:
        raise ValueError(f"transducer_loss: blank_index {blank_index} outside the vocabulary of {V}")
    ops.dt(logits)
    tg, in_len, tgt_len = transducer_lengths(T, targets, input_lens, target_lens, logits.device)
    nll = _RNNT.apply(logits, tg, in_len, tgt_len, int(blank_index))
    return reduce_transducer(nll, reduction)


# ---- label-smoothed sequence losses (csrc/seqloss.hip) -----------------------------------------------------------------------------
def truncate(predictions, targets, allowed_len_diff=3):
    """speechbrain.nnet.losses.truncate: when the time axes differ by at most allowed_len_diff both are cut to the shorter (views,
    the kernels take the strides); a larger difference is a ValueError."""
    diff = predictions.shape[1] - targets.shape[1]
    if diff == 0:
        return predictions, targets
    if abs(diff) > allowed_len_diff:
        raise ValueError(f"predictions and targets differ by {abs(diff)} steps along time ({predictions.shape[1]} vs {targets.shape[1]}); "
                         f"allowed_len_diff is {allowed_len_diff}")
    if diff < 0:
        return predictions, targets[:, :predictions.shape[1]]
    return predictions[:, :targets.shape[1]], targets


def mask_count(length, U):
    """Kept steps per utterance under upstream's length mask, arange(U) < (length * U)[:, None] evaluated in length's own float dtype
    (2.5 keeps three steps), as int32 (B) on length's device.  A tiny torch op, no host synchronisation."""
    if not length.is_floating_point():
        length = length.float()
    return (torch.arange(U, device=length.device, dtype=length.dtype)[None, :] < (length * U)[:, None]).sum(1).to(torch.int32)


def smoothing_terms(kind, label_smoothing, V):
    """(conf, off, cst) of the target distribution q[y] = conf, q[v != y] = off and the constant of a kept row (include/smx.h)."""
    eps = float(label_smoothing)
    if kind == "nll":
        if not 0.0 <= eps <= 1.0:
            raise ValueError(f"label_smoothing {eps} outside [0, 1]")
        return (1.0 - eps) + eps / V, eps / V, 0.0
    if not 0.0 < eps < 1.0:
        raise ValueError(f"kldiv_loss: label_smoothing {eps} outside (0, 1)")
    if V < 2:
        raise ValueError("kldiv_loss with label smoothing spreads the mass over the V - 1 other tokens: V >= 2 needed")
    conf, off = 1.0 - eps, eps / (V - 1)
    return conf, off, conf * math.log(conf) + (V - 1) * off * math.log(off)


class _SeqLoss(torch.autograd.Function):
    """-> (row loss (B, U), utterance sums (B), kept (B), hits (B)); differentiable through the first two."""

    @staticmethod
    def forward(ctx, x, targets, keep_len, pad_idx, conf, off, cst, from_logits):
        row, lse, _, utt, kept, hits = ops.seqloss_fwd(x, targets, keep_len, pad_idx, conf, off, cst, from_logits)
        ctx.save_for_backward(x, targets, keep_len, lse)     # (the log-probability form reads x's shape and strides only)
        ctx.meta = (pad_idx, conf, off, from_logits)
        ctx.mark_non_differentiable(kept, hits)
        ctx.set_materialize_grads(False)
        return row, utt, kept, hits

    @staticmethod
    def backward(ctx, g_row, g_utt, _gk, _gh):
        x, targets, keep_len, lse = ctx.saved_tensors
        pad_idx, conf, off, from_logits = ctx.meta
        if g_row is None and g_utt is None:
            return (None,) * 8
        g = torch.zeros(x.shape[:2], dtype=torch.float32, device=x.device) if g_row is None else g_row.float()
        if g_utt is not None:
            g = g + g_utt.float()[:, None]
        dx = ops.seqloss_bwd(x, targets, keep_len, pad_idx, conf, off, lse, g.contiguous(), from_logits)
        return (dx,) + (None,) * 7


def _seq_inputs(name, x, targets):
    if x.dim() != 3 or targets.dim() != 2 or targets.shape[0] != x.shape[0]:
        raise ValueError(f"{name}: (B, U, V) scores and (B, U) tokens expected, got {tuple(x.shape)} and {tuple(targets.shape)}")
    if targets.is_floating_point() or targets.dtype == torch.bool:
        raise TypeError(f"{name}: integer targets expected, got {targets.dtype}")
    ops.dt(x)


def _seq_apply(name, x, targets, keep_len, pad_idx, terms, from_logits):
    if not x.is_cuda:
        raise RuntimeError(f"summarymixing_amd.nnet.losses.{name} runs on the GPU only (no CPU fallback)")
    if x.shape[1] != targets.shape[1]:
        raise ValueError(f"{name}: scores have {x.shape[1]} steps, targets {targets.shape[1]}")
    if x.shape[2] > 1 and x.stride(2) != 1:
        x = x.contiguous()
    tg = targets.to(device=x.device, dtype=torch.int32)
    if tg.shape[1] > 1 and tg.stride(1) != 1:
        tg = tg.contiguous()
    return _SeqLoss.apply(x, tg, keep_len, int(pad_idx), *terms, bool(from_logits))


def _nll(name, x, targets, length, label_smoothing, allowed_len_diff, reduction, from_logits):
    _seq_inputs(name, x, targets)
    x, targets = truncate(x, targets, allowed_len_diff)
    terms = smoothing_terms("nll", label_smoothing, x.shape[2])
    if not x.is_cuda:
        raise RuntimeError(f"summarymixing_amd.nnet.losses.{name} runs on the GPU only (no CPU fallback)")
    keep_len = None if length is None else mask_count(length.to(x.device), x.shape[1])
    row, utt, kept, hits = _seq_apply(name, x, targets, keep_len, -1, terms, from_logits)
    if reduction == "mean":
        loss = utt.sum() / kept.sum()
    elif reduction == "batchmean":
        loss = utt.sum() / x.shape[0]
    elif reduction == "batch":
        loss = utt / kept
    else:
        loss = row
    return loss, hits, kept


KLDIV_REDUCTIONS = ("mean", "batchmean", "batch", "sum")


def _kldiv(name, x, targets, length, label_smoothing, pad_idx, reduction, from_logits):
    if reduction not in KLDIV_REDUCTIONS:
        raise NotImplementedError(f"{name}: reduction={reduction!r} returns the pointwise (B * U, V) tensor upstream, which is not "
                                  f"implemented (one of {KLDIV_REDUCTIONS})")
    if x.dim() == 2 and targets.dim() == 1:
        x, targets = x.unsqueeze(1), targets.unsqueeze(1)
    _seq_inputs(name, x, targets)
    terms = smoothing_terms("kldiv", label_smoothing, x.shape[2])
    if reduction == "batch" and length is None:
        raise ValueError(f"{name}: reduction='batch' divides by `length`, which is None")
    row, utt, kept, hits = _seq_apply(name, x, targets, None, pad_idx, terms, from_logits)
    if reduction in ("mean", "sum"):                 # upstream's 'mean' is loss.sum().mean(): the sum
        loss = utt.sum()
    elif reduction == "batchmean":
        loss = utt.sum() / x.shape[0]
    else:
        loss = utt / length.to(utt.device)           # the RELATIVE length, as upstream writes it
    return loss, hits, kept


def nll_loss(log_probabilities, targets, length=None, label_smoothing=0.0, allowed_len_diff=3, weight=None, reduction="mean"):
    """speechbrain.nnet.losses.nll_loss.  log_probabilities (B, U, V) (CUDA, fp32 or bf16), targets (B, U') integer tokens, length the
    RELATIVE lengths or None.  Per kept step (1 - e) (-lp[y]) - e mean_v lp[v]: what torch's cross_entropy(label_smoothing=e) computes.
    reduction: 'mean' (sum / kept steps), 'batchmean' (sum / B), 'batch' (per utterance, (B,)), anything else the unreduced (B, U)."""
    if weight is not None:
        raise NotImplementedError("nll_loss: weight= (per-class weights) is not implemented")
    return _nll("nll_loss", log_probabilities, targets, length, label_smoothing, allowed_len_diff, reduction, False)[0]


def kldiv_loss(log_probabilities, targets, length=None, label_smoothing=0.0, allowed_len_diff=3, pad_idx=0, reduction="mean"):
    """speechbrain.nnet.losses.kldiv_loss.  label_smoothing == 0: nll_loss(log_probabilities, targets, length, reduction=reduction).
    Otherwise KL(q || p) per step with q[y] = 1 - e and e / (V - 1) elsewhere, steps with targets == pad_idx dropped, `length` ignored,
    no truncation; reduction 'mean' and 'sum' (the sum), 'batchmean' (sum / B), 'batch' (utterance sums / the relative length)."""
    if label_smoothing == 0:
        return nll_loss(log_probabilities, targets, length, reduction=reduction)
    return _kldiv("kldiv_loss", log_probabilities, targets, length, label_smoothing, pad_idx, reduction, False)[0]


def seq_loss_from_logits(logits, targets, length=None, label_smoothing=0.0, pad_idx=None, kind="nll", reduction="mean",
                         allowed_len_diff=3, return_accuracy=False):
    """kldiv_loss(log_softmax(logits), ...) (kind='kldiv') or nll_loss(log_softmax(logits), ...) (kind='nll') - same value, same
    gradient with respect to the logits - in one read of the logits forward and one read plus one write backward: the log-softmax
    happens inside the row pass, no log-probability tensor is stored, the row's log-sum-exp is what the backward keeps.
    pad_idx is read for kind='kldiv' only (None: upstream's default 0; below 0: no pad mask).  return_accuracy=True: also
    (hits, kept), int32 (B) on the device, from the same pass (argmax == target over the kept steps)."""
    if kind not in ("nll", "kldiv"):
        raise ValueError(f"seq_loss_from_logits: kind {kind!r} ('nll' or 'kldiv')")
    if kind == "kldiv" and label_smoothing != 0:
        loss, hits, kept = _kldiv("seq_loss_from_logits", logits, targets, length, label_smoothing, 0 if pad_idx is None else pad_idx,
                                  reduction, True)
    else:
        loss, hits, kept = _nll("seq_loss_from_logits", logits, targets, length, label_smoothing if kind == "nll" else 0.0,
                                allowed_len_diff if kind == "nll" else 3, reduction, True)
    return (loss, (hits, kept)) if return_accuracy else loss

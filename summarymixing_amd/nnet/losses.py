"""Losses of the recipes' heads: the CTC loss of the multitask head (recipe key ``ctc_cost``: speechbrain.nnet.losses.ctc_loss, which wraps
``torch.nn.functional.ctc_loss(..., zero_infinity=True)``; SpeechBrain is not vendored in the reference tree, the call
site is …/LibriSpeech/ASR/transducer/hparams/conformer_summarymixing_transducer.yaml:297-298) and the transducer (RNN-T)
loss the recipe trains on (recipe key ``transducer_cost``: speechbrain.nnet.losses.transducer_loss).  The forward/backward
variables and the gradients run in the HIP kernels of csrc/ctc.hip and csrc/transducer.hip; no CPU fallback."""
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

"""The transducer head: ``Transducer_joint`` (SpeechBrain's import path) and the fused path ``transducer_joint_loss``, which goes from
the two projected streams to the RNN-T loss without ever writing the (B T (U+1)) x V logits.

Fused forward: joint -> H; the ``transducer_lin`` GEMM on H with an epilogue that keeps per row only what the loss needs (lse,
lp_blank, lp_y) -> lattice DP.  Fused backward: lattice DP -> per-row coefficients; per group of whole utterances the same GEMM is
recomputed and its epilogue stores dz once; dW += dz^T H and d bias through the ordinary wgrad (into the parameters' fp32 .grad,
as nnet.linear.Linear does); dH = dz W; the joint backward of those utterances.  dz and dH live one utterance group at a time."""
import torch

from ... import _lib as L
from ... import functional as F
from ... import ops
from ..losses import TRANSDUCER_REDUCTIONS, reduce_transducer, transducer_lengths
from .beam import CapturedTransducerBeam, TransducerBeamResult, TransducerBeamStream, beam_decode
from .greedy import CapturedGreedy, GreedyResult, GreedyState, greedy_decode
from .prediction_network import prediction_network, prediction_network_masks
from .transducer_joint import Transducer_joint, joint_inputs

__all__ = ["Transducer_joint", "transducer_joint_loss", "prediction_network", "prediction_network_masks", "greedy_decode",
           "CapturedGreedy", "GreedyState", "GreedyResult", "beam_decode", "CapturedTransducerBeam", "TransducerBeamResult",
           "TransducerBeamStream"]

# lattice rows per backward group (whole utterances; at least one): bounds the live dz / dH slices
_BWD_GROUP_ROWS = 49152
# dz is stored with its columns padded to a multiple of 64 (zeros; W gets zero rows to match): the dgrad dz W then reduces over a
# multiple of the bf16 GEMM's 64-element stage and takes its vector path (V = 1000 does not)
_V_PAD = 64


class _FusedHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, dec, targets, in_len, tgt_len, blank, act, wparam, bparam):
        B, T, J = enc.shape
        U1 = dec.shape[1]
        H = ops.transducer_joint_fwd(enc, dec, act)
        H2 = H.view(-1, J)
        Wc = F.wcast(wparam, enc.dtype)
        bias = bparam.detach() if bparam is not None else None
        lse, lpb, lpy = ops.transducer_gemm_stats(H2, Wc, bias, targets, B, T, U1, blank)
        nll, alpha = ops.transducer_loss_fwd(lpb, lpy, in_len, tgt_len, B, T, U1)
        ctx.save_for_backward(enc, dec, targets, in_len, tgt_len, lse, lpb, lpy, alpha)
        ctx.H = H
        ctx.meta = (blank, act, wparam, bparam)
        return nll

    @staticmethod
    def backward(ctx, gnll):
        enc, dec, targets, in_len, tgt_len, lse, lpb, lpy, alpha = ctx.saved_tensors
        blank, act, wparam, bparam = ctx.meta
        H, ctx.H = ctx.H, None
        B, T, J = enc.shape
        U1 = dec.shape[1]
        H2 = H.view(-1, J)
        gb, gy = ops.transducer_loss_bwd(lpb, lpy, alpha, gnll.float().contiguous(), in_len, tgt_len, B, T, U1)
        Wc = F.wcast(wparam, enc.dtype)
        V = Wc.shape[0]
        bias = bparam.detach() if bparam is not None else None
        gW, gB = F.gacc(wparam), F.gacc(bparam)
        need_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        d_enc, d_dec = (torch.empty_like(enc), torch.empty_like(dec)) if need_x else (None, None)
        per = T * U1
        ub = max(1, _BWD_GROUP_ROWS // per)              # utterances per group (from shapes only)
        rows_g = min(B, ub) * per
        Vp = (V + _V_PAD - 1) // _V_PAD * _V_PAD
        dz_buf = torch.zeros((rows_g, Vp), dtype=enc.dtype, device=enc.device)
        Wp = Wc
        if Vp != V and need_x:
            Wp = torch.zeros((Vp, J), dtype=Wc.dtype, device=Wc.device)
            Wp[:V].copy_(Wc)
        dh_buf = torch.empty((rows_g, J), dtype=enc.dtype, device=enc.device) if need_x else None
        for b0 in range(0, B, ub):
            b1 = min(B, b0 + ub)
            r0, n = b0 * per, (b1 - b0) * per
            dzp = dz_buf[:n]
            dz = ops.transducer_gemm_grad(H2, Wc, bias, targets, lse, gb, gy, B, T, U1, blank, r0, n, dzp[:, :V])
            if gW is not None or gB is not None:
                F.linear_bwd(dz, H2[r0:r0 + n], Wc, None, L.ACT_NONE, None, 1.0, gW, gB, need_dx=False)
                F.flush_deferred()                       # this group's slabs are reduced before dz_buf is reused
            if need_x:
                dH = dh_buf[:n]
                ops.gemm(L.GEMM_NN, dzp, Wp, dH, n, J, Vp)
                ops.transducer_joint_bwd(dH.view(b1 - b0, T, U1, J), enc[b0:b1], dec[b0:b1], act, d_enc[b0:b1], d_dec[b0:b1])
        return d_enc, d_dec, None, None, None, None, None, None, None


def transducer_joint_loss(enc_out, dec_out, tjoint, transducer_lin, targets, input_lens, target_lens, blank_index, reduction="mean"):
    """The recipe's ``transducer_cost(transducer_lin(Tjoint(enc_out, dec_out)), targets, ...)`` in one call that never stores the
    logits.  enc_out (B, T, J) or (B, T, 1, J); dec_out (B, U+1, J) or (B, 1, U+1, J); tjoint a Transducer_joint; transducer_lin
    an nnet.linear.Linear (J -> V, bias optional; its bf16 shadow weights apply); targets (B, U); relative lengths.  Returns the
    same value and gradients (enc_out, dec_out, weight, bias) as the drop-in chain.  Needs J % 64 == 0 and V % 4 == 0."""
    if reduction not in TRANSDUCER_REDUCTIONS:
        raise ValueError(f"unknown reduction {reduction!r} (transducer_joint_loss: 'mean', 'sum' or 'none')")
    if not isinstance(tjoint, Transducer_joint):
        raise TypeError("transducer_joint_loss: tjoint must be a summarymixing_amd Transducer_joint")
    enc4 = enc_out.unsqueeze(2) if enc_out.dim() == 3 else enc_out
    dec4 = dec_out.unsqueeze(1) if dec_out.dim() == 3 else dec_out
    if enc4.dim() != 4 or dec4.dim() != 4:
        raise NotImplementedError("transducer_joint_loss: (B, T, J) / (B, T, 1, J) and (B, U+1, J) / (B, 1, U+1, J) streams only")
    B, T, one_t, J = enc4.shape
    U1 = dec4.shape[2]
    if one_t != 1 or dec4.shape[1] != 1 or dec4.shape[0] != B or dec4.shape[3] != J:
        raise ValueError(f"transducer_joint_loss: streams {tuple(enc_out.shape)} and {tuple(dec_out.shape)} do not form a lattice")
    W, b = transducer_lin.w.weight, transducer_lin.w.bias
    V = W.shape[0]
    if W.dim() != 2 or W.shape[1] != J:
        raise ValueError(f"transducer_joint_loss: transducer_lin maps {W.shape[-1]} features, the joint width is {J}")
    if targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] != U1 - 1:
        raise ValueError(f"transducer_joint_loss: targets (B, U) = ({B}, {U1 - 1}) expected, got {tuple(targets.shape)}")
    if not 0 <= int(blank_index) < V:
        raise ValueError(f"transducer_joint_loss: blank_index {blank_index} outside the vocabulary of {V}")
    if J % 64 != 0 or V % 4 != 0:
        raise ValueError(f"transducer_joint_loss: the fused GEMM needs J % 64 == 0 and V % 4 == 0 (J {J}, V {V})")
    enc, dec = joint_inputs(tjoint, enc4, dec4)
    if not ops.transducer_fused_ok(enc.dtype, J, V):
        raise ValueError(f"transducer_joint_loss: no fused GEMM for J {J}, V {V}")
    tg, in_len, tgt_len = transducer_lengths(T, targets, input_lens, target_lens, enc.device)
    nll = _FusedHead.apply(enc, dec, tg, in_len, tgt_len, int(blank_index), tjoint.act, W, b)
    return reduce_transducer(nll, reduction)

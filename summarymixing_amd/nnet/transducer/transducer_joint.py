"""speechbrain.nnet.transducer.transducer_joint.Transducer_joint as the transducer recipe instantiates it (recipe key ``Tjoint``:
``joint: sum``, ``nonlinearity: GELU``): ``H[b,t,u,:] = act(enc[b,t,:] + dec[b,u,:])`` on the 4-D training form
``(B, T, 1, J)`` + ``(B, 1, U+1, J)`` -> ``(B, T, U+1, J)``.  Forward and backward run in csrc/transducer.hip; GPU only.
No parameters: the recipe's state_dict is unchanged."""
import torch

from ... import _lib as L
from ... import ops


def act_code(act):
    """The SMX_ACT_* code of a nonlinearity instance (exact GELU, LeakyReLU(0.01), ReLU)."""
    if isinstance(act, torch.nn.GELU):
        if getattr(act, "approximate", "none") != "none":
            raise NotImplementedError("Transducer_joint: only the exact (erf) GELU is fused in the kernels")
        return L.ACT_GELU
    if isinstance(act, torch.nn.LeakyReLU):
        if act.negative_slope != 0.01:
            raise NotImplementedError("Transducer_joint: LeakyReLU runs with the default negative_slope 0.01 only")
        return L.ACT_LEAKY_RELU
    if isinstance(act, torch.nn.ReLU):
        return L.ACT_RELU
    raise NotImplementedError(f"Transducer_joint: nonlinearity {type(act).__name__} is not fused in the kernels "
                              "(GELU, LeakyReLU and ReLU are)")


def joint_inputs(tjoint, input_TN, input_PN):
    """Validate the recipe's 4-D training form and return the contiguous (B, T, J) / (B, U1, J) views (raises before any launch)."""
    if input_TN.dim() != 4 or input_PN.dim() != 4:
        raise NotImplementedError("Transducer_joint: only the 4-D training form (B, T, 1, J) + (B, 1, U+1, J) is implemented "
                                  "(the 1-D decoding form is not called: greedy decoding runs in nnet.transducer.greedy_decode, beam search is not built)")
    B, T, one_t, J = input_TN.shape
    if one_t != 1 or input_PN.shape[1] != 1 or input_PN.shape[0] != B or input_PN.shape[3] != J:
        raise ValueError(f"Transducer_joint: expected (B, T, 1, J) and (B, 1, U+1, J), got {tuple(input_TN.shape)} and "
                         f"{tuple(input_PN.shape)}")
    if input_TN.dtype != input_PN.dtype:
        raise ValueError(f"Transducer_joint: both streams in one dtype, got {input_TN.dtype} and {input_PN.dtype}")
    if not (input_TN.is_cuda and input_PN.is_cuda):
        raise RuntimeError("summarymixing_amd kernels run on the GPU only (no CPU fallback)")
    if J % 4 != 0:
        raise ValueError(f"Transducer_joint: the joint width must be a multiple of 4, got {J}")
    ops.dt(input_TN)
    return input_TN.reshape(B, T, J).contiguous(), input_PN.reshape(B, input_PN.shape[2], J).contiguous()


class _Joint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, dec, act):
        ctx.save_for_backward(enc, dec)
        ctx.act = act
        return ops.transducer_joint_fwd(enc, dec, act)

    @staticmethod
    def backward(ctx, dH):
        enc, dec = ctx.saved_tensors
        d_enc, d_dec = ops.transducer_joint_bwd(dH.contiguous(), enc, dec, ctx.act)
        return d_enc, d_dec, None


class Transducer_joint(torch.nn.Module):
    def __init__(self, joint_network=None, joint="sum", nonlinearity=torch.nn.LeakyReLU):
        super().__init__()
        if joint_network is not None:
            raise NotImplementedError("Transducer_joint: a joint_network is not used by the SummaryMixing transducer recipe")
        if joint != "sum":
            raise NotImplementedError(f"Transducer_joint: joint={joint!r} is not implemented (the recipe uses 'sum')")
        self.joint_network = None
        self.joint = joint
        self.nonlinearity = nonlinearity()
        self.act = act_code(self.nonlinearity)

    def forward(self, input_TN, input_PN):
        enc, dec = joint_inputs(self, input_TN, input_PN)
        return _Joint.apply(enc, dec, self.act)

"""speechbrain.nnet.RNN.LSTM as the transducer recipe instantiates it for the prediction network (``dec``,
…transducer.yaml:306-310): one layer, unidirectional, batch first, torch's gate order i, f, g, o and two biases.  Parameters live
under ``.rnn`` with torch.nn.LSTM's names (``rnn.weight_ih_l0`` …), so reference checkpoints load unchanged.  The input product
runs on the MFMA GEMM of libsmx.so, the recurrence and its BPTT on csrc/lstm.hip; every parameter gradient is added into the
parameter's fp32 ``.grad`` (functional.gacc), as nnet.linear.Linear does.  GPU only."""
import math
from typing import Optional

import torch
from torch import nn

from .. import _lib as L
from .. import functional as F
from .. import ops

H_MIN, H_MAX, H_STEP = 32, 4096, 32         # what csrc/lstm.hip supports (smx_lstm_ok)
_K_PAD = 64                                 # the dense input is zero-padded to a multiple of the bf16 GEMM's 64-element K stage


def _transposed(w):
    return w.t().contiguous()


def lstm_weights(params, k, T):
    """(W_ih in T, W_hh in T contiguous, b_ih + b_hh in fp32) of layer k of an _LSTMParams.  The bias sum and the images of the two
    weights that the routes below ask for (W_ih^T, W_hh^T, the K-padded W_ih) are kept in params._derived under functional.derived's
    rules."""
    b_ih, b_hh = getattr(params, f"bias_ih_l{k}"), getattr(params, f"bias_hh_l{k}")
    bsum = F.derived(params._derived, f"bsum{k}", (b_ih, b_hh), lambda a, b: ops.axpby(
        1.0, ops.cast(a.detach(), torch.float32).view(1, -1), 1.0, ops.cast(b.detach(), torch.float32).view(1, -1)).view(-1))
    return F.wcast(getattr(params, f"weight_ih_l{k}"), T), F.wcast(getattr(params, f"weight_hh_l{k}"), T).contiguous(), bsum


def dense_gates(x2, Wih, bsum, params, k):
    """Gx (rows, 4H) fp32 = x2 W_ih^T + bsum on the MFMA GEMM -> (Gx, the x2 and the W_ih it ran on: both zero-padded along K to a
    multiple of _K_PAD when the input width is none, the padded W_ih a kept image)."""
    rows, I = x2.shape
    if I % _K_PAD != 0:
        Kp = (I + _K_PAD - 1) // _K_PAD * _K_PAD
        xp = torch.zeros((rows, Kp), dtype=x2.dtype, device=x2.device)
        xp[:, :I].copy_(x2)

        def pad(w):
            Wp = torch.zeros((w.shape[0], Kp), dtype=w.dtype, device=w.device)
            Wp[:, :I].copy_(w)
            return Wp
        x2, Wih = xp, F.derived(params._derived, f"Wih_pad{k}", (Wih,), pad)
    elif not x2.is_contiguous():
        x2 = x2.contiguous()
    Gx, _ = F.linear_fwd(x2, Wih, bsum, out_f32=x2.dtype != torch.float32)
    return Gx, x2, Wih


def _pad_grad(params, k, param, Kp):
    """Persistent fp32 (4H, Kp) gradient image of the K-padded W_ih (a stable address for the deferred wgrad workspaces)."""
    g = params._derived.get(f"gWp{k}")
    if g is None or g.shape[1] != Kp or g.device != param.device:
        g = params._derived[f"gWp{k}"] = torch.zeros((param.shape[0], Kp), dtype=torch.float32, device=param.device)
    return g


class _LSTMFn(torch.autograd.Function):
    """(Y, h_n, c_n) = LSTM(inp; h0, c0).  onehot = None: inp is the dense (B, U, I) input; onehot = (V, blank, keep, dtype): inp are
    (B, U) tokens, the input product is a row gather of W_ih^T (keep: per-token fp32 factors or None) and no one-hot row exists."""

    @staticmethod
    def forward(ctx, inp, h0, c0, w_ih, w_hh, b_ih, b_hh, onehot, holder, k):
        ctx.set_materialize_grads(False)
        B, U = inp.shape[0], inp.shape[1]
        H = w_hh.shape[1]
        T = inp.dtype if onehot is None else onehot[3]
        need_bwd = any(ctx.needs_input_grad)
        Wih, Whh, bsum = lstm_weights(holder, k, T)
        if onehot is None:
            I = inp.shape[2]
            Gx, x2, Wp = dense_gates(inp.reshape(B * U, I), Wih, bsum, holder, k)
            side = (x2, Wp, I)
        else:
            assert k == 0, "tokens are the first layer's input"
            V, blank, keep = onehot[:3]
            tk = ops._tokens_i32(inp)
            Gx = ops.onehot_gates_fwd(tk, keep, F.derived(holder._derived, "WihT", (Wih,), _transposed), bsum, V, blank)
            side = (tk, keep, V, blank)
        h0_ = ops.cast(h0.detach().reshape(B, H), T).contiguous() if h0 is not None else None
        c0_ = ops.cast(c0.detach().reshape(B, H), torch.float32).contiguous() if c0 is not None else None
        Y, hn, cn, saved = ops.lstm_fwd(Gx, Whh, h0_, c0_, B, U, need_bwd)
        if need_bwd:
            ctx.saved = (Whh, c0_, saved, side, onehot is None, (w_ih, w_hh, b_ih, b_hh), (holder, k),
                         h0.dtype if h0 is not None else None, c0.dtype if c0 is not None else None)
        return Y, hn.view(1, B, H), cn.view(1, B, H)

    @staticmethod
    def backward(ctx, dY, dhn, dcn):
        Whh, c0_, (Hprev, gates, C), side, dense, (w_ih, w_hh, b_ih, b_hh), (holder, k), h0_dt, c0_dt = ctx.saved
        ctx.saved = None
        B, U, H = Hprev.shape
        T = Whh.dtype
        if dY is None and dhn is None and dcn is None:
            return (None,) * 10
        dY_ = ops.cast(dY, T).contiguous() if dY is not None else None
        dhn_ = ops.cast(dhn.reshape(B, H), torch.float32).contiguous() if dhn is not None else None
        dcn_ = ops.cast(dcn.reshape(B, H), torch.float32).contiguous() if dcn is not None else None
        dG, dh0, dc0 = ops.lstm_bwd(dY_, dhn_, dcn_, F.derived(holder._derived, f"WhhT{k}", (Whh,), _transposed), gates, C, c0_, B, U)
        # dW_hh += dG^T H_prev over all B U rows, db_hh += colsum(dG): the ordinary wgrad route
        F.linear_bwd(dG, Hprev.view(B * U, H), Whh, None, L.ACT_NONE, None, 1.0, F.gacc(w_hh), F.gacc(b_hh), need_dx=False)
        dx = None
        if dense:
            x2, Wp, I = side
            gW, gWp = F.gacc(w_ih), None
            if gW is not None and Wp.shape[1] != I:
                gWp = _pad_grad(holder, k, w_ih, Wp.shape[1])
                gWp.zero_()
            dxp, _ = F.linear_bwd(dG, x2, Wp, None, L.ACT_NONE, None, 1.0, gWp if gWp is not None else gW, F.gacc(b_ih),
                                  need_dx=ctx.needs_input_grad[0])
            F.flush_deferred()
            if gWp is not None:
                ops.axpby(1.0, gWp[:, :I], 1.0, gW, out=gW)
            if dxp is not None:
                dx = dxp[:, :I].reshape(B, U, I)
        else:
            tk, keep, V, blank = side
            gb = F.gacc(b_ih)
            if gb is not None:
                ops.act_mask_bwd(dG, None, None, L.ACT_NONE, 1.0, None, gb, None, 0)
            gW = F.gacc(w_ih)
            if gW is not None:
                ops.onehot_gates_wgrad(tk, keep, dG, gW, V, blank)
            F.flush_deferred()
        dh0 = ops.cast(dh0, h0_dt).view(1, B, H) if (h0_dt is not None and ctx.needs_input_grad[1]) else None
        dc0 = ops.cast(dc0, c0_dt).view(1, B, H) if (c0_dt is not None and ctx.needs_input_grad[2]) else None
        return (dx, dh0, dc0) + (None,) * 7


def lstm_apply(inp, hx, rnn, onehot=None, k=0):
    """The recurrence on `inp` with the parameters of layer k of `rnn` (a module whose ``.rnn`` is an _LSTMParams: an LSTM below);
    hx = (h0, c0), each (1, B, H), (B, H) or None, or None."""
    h0, c0 = hx if hx is not None else (None, None)
    p = rnn.rnn
    return _LSTMFn.apply(inp, h0, c0, *(getattr(p, f"{n}_l{k}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")), onehot, p, k)


class _LSTMParams(nn.Module):
    """torch.nn.LSTM's parameters of a unidirectional stack: names, shapes, order and default initialisation."""

    def __init__(self, input_size, hidden_size, num_layers=1):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        for k in range(num_layers):
            setattr(self, f"weight_ih_l{k}", nn.Parameter(torch.empty(4 * hidden_size, input_size if k == 0 else hidden_size)))
            setattr(self, f"weight_hh_l{k}", nn.Parameter(torch.empty(4 * hidden_size, hidden_size)))
            setattr(self, f"bias_ih_l{k}", nn.Parameter(torch.empty(4 * hidden_size)))
            setattr(self, f"bias_hh_l{k}", nn.Parameter(torch.empty(4 * hidden_size)))
        self._derived = {}                   # images of the parameters (functional.derived); not part of the state_dict
        k = 1.0 / math.sqrt(hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -k, k)


def rnn_init(module):
    """SpeechBrain's rnn_init: the recurrent weights start orthogonal."""
    for name, param in module.named_parameters():
        if "weight_hh" in name or ".u.weight" in name:
            nn.init.orthogonal_(param)


class LSTM(nn.Module):
    def __init__(self, hidden_size, input_shape: Optional[list] = None, input_size: Optional[int] = None, num_layers=1, bias=True,
                 dropout=0.0, re_init=True, bidirectional=False):
        super().__init__()
        if num_layers != 1:
            raise NotImplementedError("LSTM: one layer only (the transducer recipe's prediction network)")
        if bidirectional:
            raise NotImplementedError("LSTM: unidirectional only")
        if not bias:
            raise NotImplementedError("LSTM: bias=False is not used by the SummaryMixing recipes")
        if dropout > 0:
            raise NotImplementedError("LSTM: inter-layer dropout needs more than one layer")
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size.")
        if hidden_size < H_MIN or hidden_size > H_MAX or hidden_size % H_STEP != 0:
            raise NotImplementedError(f"LSTM: hidden_size must be a multiple of {H_STEP} in [{H_MIN}, {H_MAX}], got {hidden_size}")
        self.reshape = False
        if input_size is None:
            if len(input_shape) > 3:
                self.reshape = True
            input_size = int(torch.prod(torch.tensor(input_shape[2:])))
        self.hidden_size, self.num_layers, self.bidirectional = hidden_size, 1, False
        self.rnn = _LSTMParams(input_size, hidden_size)
        if re_init:
            rnn_init(self.rnn)

    def forward(self, x, hx=None, lengths=None):
        """x (B, U, I) -> (output (B, U, H), (h_n, c_n)); hx = (h0, c0), h_n and c_n are (1, B, H).  h_n has x's dtype; c_n is
        float32 whatever x is (the cell state never leaves fp32), and a c0 of any float dtype is accepted."""
        if lengths is not None:
            raise NotImplementedError("LSTM: packed / length-masked sequences are not used by the SummaryMixing recipes")
        if not x.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        if x.dim() != 3 or x.shape[2] != self.rnn.input_size:
            raise ValueError(f"LSTM: input (B, U, {self.rnn.input_size}) expected, got {tuple(x.shape)}")
        ops.dt(x)
        y, hn, cn = lstm_apply(x, hx, self)
        return y, (hn, cn)

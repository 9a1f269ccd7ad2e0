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


def _derived(holder, name, src, build):
    """Images derived from a weight in its compute dtype (W_ih^T, W_hh^T, the K-padded W_ih), kept on the parameter holder and
    rebuilt when the weight changed: torch's version counter, and functional's weight epoch for the trainer-managed bf16 shadows
    that smx_adamw_step rewrites in place.  Inside a graph capture nothing is reused or kept: the captured step builds its own
    images, so a replay that follows a captured optimizer update sees the new weights."""
    if torch.cuda.is_current_stream_capturing():
        return build(src)
    stamp = (src.data_ptr(), src.dtype, src._version, F._WEPOCH[0])
    ent = holder._derived.get(name)
    if ent is None or ent[1] != stamp:
        ent = (src, stamp, build(src))                      # (src held: its storage cannot be recycled under the stamp)
        holder._derived[name] = ent
    return ent[2]


def _pad_k(W, Kp):
    Wp = torch.zeros((W.shape[0], Kp), dtype=W.dtype, device=W.device)
    Wp[:, :W.shape[1]].copy_(W)
    return Wp


def _pad_grad(holder, param, Kp):
    """Persistent fp32 (4H, Kp) gradient image of the K-padded W_ih (a stable address for the deferred wgrad workspaces)."""
    g = holder._derived.get("gWp")
    if g is None or g.shape[1] != Kp or g.device != param.device:
        g = torch.zeros((param.shape[0], Kp), dtype=torch.float32, device=param.device)
        holder._derived["gWp"] = g
    return g


class _LSTMFn(torch.autograd.Function):
    """(Y, h_n, c_n) = LSTM(inp; h0, c0).  onehot = None: inp is the dense (B, U, I) input; onehot = (V, blank, keep, dtype): inp are
    (B, U) tokens, the input product is a row gather of W_ih^T (keep: per-token fp32 factors or None) and no one-hot row exists."""

    @staticmethod
    def forward(ctx, inp, h0, c0, w_ih, w_hh, b_ih, b_hh, onehot, holder):
        ctx.set_materialize_grads(False)
        B, U = inp.shape[0], inp.shape[1]
        H = w_hh.shape[1]
        T = inp.dtype if onehot is None else onehot[3]
        need_bwd = any(ctx.needs_input_grad)
        Whh, Wih = F.wcast(w_hh, T).contiguous(), F.wcast(w_ih, T)
        bsum = ops.axpby(1.0, b_ih.detach().view(1, -1), 1.0, b_hh.detach().view(1, -1)).view(-1)
        if onehot is None:
            I = inp.shape[2]
            x2 = inp.reshape(B * U, I)
            Wp = Wih
            if I % _K_PAD != 0:
                Kp = (I + _K_PAD - 1) // _K_PAD * _K_PAD
                xp = torch.zeros((B * U, Kp), dtype=T, device=inp.device)
                xp[:, :I].copy_(x2)
                Wp = _derived(holder, "Wih_pad", Wih, lambda w: _pad_k(w, Kp))
                x2 = xp
            elif not x2.is_contiguous():
                x2 = x2.contiguous()
            Gx, _ = F.linear_fwd(x2, Wp, bsum, out_f32=T != torch.float32)
            side = (x2, Wp, I)
        else:
            V, blank, keep = onehot[:3]
            tk = ops._tokens_i32(inp)
            Gx = ops.onehot_gates_fwd(tk, keep, _derived(holder, "WihT", Wih, lambda w: w.t().contiguous()), bsum, V, blank)
            side = (tk, keep, V, blank)
        h0_ = ops.cast(h0.detach().reshape(B, H), T).contiguous() if h0 is not None else None
        c0_ = ops.cast(c0.detach().reshape(B, H), torch.float32).contiguous() if c0 is not None else None
        Y, hn, cn, saved = ops.lstm_fwd(Gx, Whh, h0_, c0_, B, U, need_bwd)
        if need_bwd:
            ctx.saved = (Whh, c0_, saved, side, onehot is None, (w_ih, w_hh, b_ih, b_hh), holder,
                         h0.dtype if h0 is not None else None, c0.dtype if c0 is not None else None)
        return Y, hn.view(1, B, H), cn.view(1, B, H)

    @staticmethod
    def backward(ctx, dY, dhn, dcn):
        Whh, c0_, (Hprev, gates, C), side, dense, (w_ih, w_hh, b_ih, b_hh), holder, h0_dt, c0_dt = ctx.saved
        ctx.saved = None
        B, U, H = Hprev.shape
        T = Whh.dtype
        none = (None,) * 9
        if dY is None and dhn is None and dcn is None:
            return none
        dY_ = ops.cast(dY, T).contiguous() if dY is not None else None
        dhn_ = ops.cast(dhn.reshape(B, H), torch.float32).contiguous() if dhn is not None else None
        dcn_ = ops.cast(dcn.reshape(B, H), torch.float32).contiguous() if dcn is not None else None
        dG, dh0, dc0 = ops.lstm_bwd(dY_, dhn_, dcn_, _derived(holder, "WhhT", Whh, lambda w: w.t().contiguous()), gates, C, c0_, B, U)
        # dW_hh += dG^T H_prev over all B U rows, db_hh += colsum(dG): the ordinary wgrad route
        F.linear_bwd(dG, Hprev.view(B * U, H), Whh, None, L.ACT_NONE, None, 1.0, F.gacc(w_hh), F.gacc(b_hh), need_dx=False)
        dx = None
        if dense:
            x2, Wp, I = side
            gW, gWp = F.gacc(w_ih), None
            if gW is not None and Wp.shape[1] != I:
                gWp = _pad_grad(holder, w_ih, Wp.shape[1])
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
        return (dx, dh0, dc0) + (None,) * 6


def lstm_apply(inp, hx, rnn, onehot=None):
    """The recurrence on `inp` with the parameters of `rnn` (an LSTM below); hx = (h0, c0), each (1, B, H) or (B, H), or None."""
    h0, c0 = hx if hx is not None else (None, None)
    p = rnn.rnn
    return _LSTMFn.apply(inp, h0, c0, p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, onehot, p)


class _LSTMParams(nn.Module):
    """torch.nn.LSTM's parameters of one unidirectional layer: names, shapes, order and default initialisation."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.weight_ih_l0 = nn.Parameter(torch.empty(4 * hidden_size, input_size))
        self.weight_hh_l0 = nn.Parameter(torch.empty(4 * hidden_size, hidden_size))
        self.bias_ih_l0 = nn.Parameter(torch.empty(4 * hidden_size))
        self.bias_hh_l0 = nn.Parameter(torch.empty(4 * hidden_size))
        self._derived = {}                   # images derived from the weights (_derived above); not part of the state_dict
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
            raise RuntimeError("summarymixing_amd kernels run on the GPU only (no CPU fallback)")
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        if x.dim() != 3 or x.shape[2] != self.rnn.input_size:
            raise ValueError(f"LSTM: input (B, U, {self.rnn.input_size}) expected, got {tuple(x.shape)}")
        ops.dt(x)
        y, hn, cn = lstm_apply(x, hx, self)
        return y, (hn, cn)

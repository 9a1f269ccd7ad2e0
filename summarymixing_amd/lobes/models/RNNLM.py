"""speechbrain.lobes.models.RNNLM.RNNLM as the transducer recipe instantiates it for its language model (``lm_model``,
…transducer.yaml:340-349: embedding_dim 128, two LSTM layers of 2048 units, one DNN block of 512, LeakyReLU, dropout 0.0,
return_hidden True): tokens -> trainable embedding table -> dropout -> L-layer unidirectional LSTM -> Linear -> LayerNorm ->
activation -> dropout -> Linear to the vocabulary.  Inference only, GPU only.

Two routes, chosen by the input's rank as in SpeechBrain:
  * tokens (B, U), the sequence form: smx_gather_rows, then per layer the dense route of nnet.RNN (the input product on the MFMA GEMM,
    the recurrence on csrc/lstm.hip), then the head;
  * tokens (B,), the decode step a beam search runs once per expansion with ``hx`` fed back: ONE launch per layer
    (csrc/lstm_step.hip: both products, the gate arithmetic and - in layer 0 - the table lookup, every LSTM weight fetched once
    whatever B is), then the same head.  Every call returns freshly allocated state tensors (successive steps ping-pong through
    the allocator; a caller may keep earlier states); ``step(..., out=(h, c))`` writes into caller-owned static buffers instead.

The compute dtype is the embedding table's (``lm.embedding.to(torch.bfloat16)`` or ``lm.bfloat16()``): float32 or bfloat16.
Logits and h_n come in it; c_n is float32 whatever the dtype (this project's convention: the cell state never leaves fp32), and an
``hx`` of any float dtype is accepted back.

SpeechBrain's RNNLM, Embedding, LSTM, DNN-block and LayerNorm sources are not part of the reference tree: the constructor signature,
the forward and the state-dict names below (``embedding.Embedding.weight``, ``rnn.rnn.weight_ih_l0`` …, ``dnn.linear.w.weight``,
``dnn.norm.norm.weight``, ``out.w.weight``) were written from memory of SpeechBrain 1.0 so that the pretrained ``lm.ckpt`` loads with
``strict=True`` - see DESIGN.md §I.12.  The names of a second DNN block are not certain, so ``dnn_blocks != 1`` is refused.  The
arithmetic yardstick is torch.nn (tests/_rnnlm_ref.py)."""
import torch
from torch import nn

from ... import functional as F
from ... import ops
from ...nnet import RNN as _RNN
from ...nnet.activations import act_code
from ...nnet.linear import Linear

_E_MIN, _E_MAX, _E_STEP = 32, 4096, 32      # the input widths csrc/lstm_step.hip supports (smx_lstm_step_ok)


class _Table(nn.Module):
    """The trainable embedding table under SpeechBrain's name ``.Embedding`` (nnet.embedding.Embedding keeps refusing one)."""

    def __init__(self, num_embeddings, embedding_dim):
        super().__init__()
        self.Embedding = nn.Embedding(num_embeddings, embedding_dim, padding_idx=0)


class _StackedLSTM(nn.Module):
    """Holder of the stack under SpeechBrain's ``.rnn`` (nnet.RNN.LSTM keeps refusing num_layers != 1)."""

    def __init__(self, input_size, hidden_size, num_layers, re_init):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.rnn = _RNN._LSTMParams(input_size, hidden_size, num_layers)
        if re_init:
            _RNN.rnn_init(self.rnn)


class _Norm(nn.Module):
    def __init__(self, size):
        super().__init__()
        self.norm = nn.LayerNorm(size, eps=1e-5)


class _DNNBlock(nn.Module):
    """Linear -> LayerNorm -> activation -> dropout, under SpeechBrain's names ``linear`` and ``norm``."""

    def __init__(self, input_size, neurons):
        super().__init__()
        self.linear = Linear(neurons, input_size=input_size, bias=True)
        self.norm = _Norm(neurons)


class RNNLM(nn.Module):
    def __init__(self, output_neurons, embedding_dim=128, activation=torch.nn.LeakyReLU, dropout=0.15, rnn_class=None, rnn_layers=2,
                 rnn_neurons=1024, rnn_re_init=False, return_hidden=False, dnn_blocks=1, dnn_neurons=512):
        super().__init__()
        if rnn_class is not None and rnn_class is not _RNN.LSTM:
            raise NotImplementedError("RNNLM: only the LSTM of this package (rnn_class=None or summarymixing_amd.nnet.RNN.LSTM)")
        if dnn_blocks != 1:
            raise NotImplementedError("RNNLM: one DNN block only (the recipe's; the checkpoint names of further blocks are not certain)")
        self.act = act_code(activation)                        # (NotImplementedError for what the kernels do not implement)
        if rnn_layers < 1:
            raise ValueError("RNNLM: rnn_layers must be at least 1")
        if not 0.0 <= dropout < 1.0:
            raise ValueError("RNNLM: dropout must be in [0, 1)")
        H, E = int(rnn_neurons), int(embedding_dim)
        if H < _RNN.H_MIN or H > _RNN.H_MAX or H % _RNN.H_STEP != 0:
            raise NotImplementedError(f"RNNLM: rnn_neurons must be a multiple of {_RNN.H_STEP} in [{_RNN.H_MIN}, {_RNN.H_MAX}], got {H}")
        if E < _E_MIN or E > _E_MAX or E % _E_STEP != 0:
            raise NotImplementedError(f"RNNLM: embedding_dim must be a multiple of {_E_STEP} in [{_E_MIN}, {_E_MAX}], got {E}")
        if dnn_neurons < 1 or dnn_neurons > 4096:
            raise NotImplementedError(f"RNNLM: dnn_neurons must be in [1, 4096] (the LayerNorm kernel's row), got {dnn_neurons}")
        self.output_neurons, self.p_drop, self.return_hidden = int(output_neurons), float(dropout), return_hidden
        self.embedding = _Table(self.output_neurons, E)
        self.rnn = _StackedLSTM(E, H, int(rnn_layers), rnn_re_init)
        self.dnn = _DNNBlock(H, int(dnn_neurons))
        self.out = Linear(self.output_neurons, input_size=int(dnn_neurons), bias=True)
        self._derived = {}                   # float32 images of the head's biases and LayerNorm vectors; not part of the state_dict

    def _f32(self, name, param):
        return F.derived(self._derived, name, (param,), lambda p: ops.cast(p.detach(), torch.float32).contiguous())

    def _check(self, x):
        if not x.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        if x.dtype.is_floating_point or x.dim() not in (1, 2):
            raise ValueError(f"RNNLM: integer tokens (B, U) or (B,) expected, got {tuple(x.shape)} {x.dtype}")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("RNNLM: inference only - call it under torch.no_grad() (the recipe takes the LM pretrained)")
        if self.training and self.p_drop > 0.0:
            raise NotImplementedError("RNNLM: dropout > 0 in training mode is not implemented (inference only; use .eval())")
        T = self.embedding.Embedding.weight.dtype
        if T not in ops._DT:
            raise TypeError(f"summarymixing_amd supports float32 and bfloat16 activations, got {T}")
        return T

    def _state(self, hx, B, T):
        L, H = self.rnn.num_layers, self.rnn.hidden_size
        if hx is None:
            return None, None
        h, c = hx
        if h is not None and (not h.is_cuda or tuple(h.shape) != (L, B, H)) or c is not None and (not c.is_cuda or tuple(c.shape) != (L, B, H)):
            raise ValueError(f"RNNLM: hx = (h, c), each ({L}, {B}, {H}) on the GPU")
        def to(t, dtype):                    # (a state of any float dtype is accepted back: what the cast kernels do not take goes through torch)
            return t if t is None else (ops.cast(t.detach(), dtype) if t.dtype in ops._DT else t.detach().to(dtype)).contiguous()
        return to(h, T), to(c, torch.float32)

    def _head(self, y2, T):
        d = self.dnn
        z, _ = F.linear_fwd(y2, F.wcast(d.linear.w.weight, T), self._f32("dnn_b", d.linear.w.bias))
        a, _ = ops.layernorm_fwd(z, self._f32("ln_w", d.norm.norm.weight), self._f32("ln_b", d.norm.norm.bias), d.norm.norm.eps, False, self.act)
        logits, _ = F.linear_fwd(a, F.wcast(self.out.w.weight, T), self._f32("out_b", self.out.w.bias))
        return logits

    # ---- the decode step ----------------------------------------------------------------------------------------------------
    def step(self, tokens, hx=None, out=None):
        """tokens (B,) -> (logits (B, V), (h_n (L, B, H), c_n (L, B, H) fp32)): one smx_lstm_step launch per layer (layer 0 reads its
        rows from the table by token) and the head.  out = (h, c): contiguous (L, B, H) buffers in the compute dtype / float32 to
        write the new state into, distinct from hx (default: freshly allocated)."""
        T = self._check(tokens)
        if tokens.dim() != 1:
            raise ValueError(f"RNNLM.step: tokens (B,) expected, got {tuple(tokens.shape)}")
        B, L, H = tokens.shape[0], self.rnn.num_layers, self.rnn.hidden_size
        h, c = self._state(hx, B, T)
        dev = tokens.device
        if out is None:
            hn, cn = torch.empty((L, B, H), dtype=T, device=dev), torch.empty((L, B, H), dtype=torch.float32, device=dev)
        else:
            hn, cn = out
            if not (hn.shape == (L, B, H) and cn.shape == (L, B, H) and hn.dtype == T and cn.dtype == torch.float32 and hn.is_contiguous() and cn.is_contiguous()):
                raise ValueError(f"RNNLM.step: out = (h ({L}, {B}, {H}) {T}, c float32), contiguous")
        tk = ops._tokens_i32(tokens)
        table = self.embedding.Embedding.weight.detach()
        for k in range(L):
            Wih, Whh, bsum = _RNN.lstm_weights(self.rnn.rnn, k, T)
            hk, ck = (h[k] if h is not None else None), (c[k] if c is not None else None)
            if k == 0:
                ops.lstm_step(table, Wih, Whh, bsum, hk, ck, hn[0], cn[0], tokens=tk)
            else:
                ops.lstm_step(hn[k - 1], Wih, Whh, bsum, hk, ck, hn[k], cn[k])
        return self._head(hn[L - 1], T), (hn, cn)

    # ---- the sequence form --------------------------------------------------------------------------------------------------
    def _sequence(self, tokens, hx):
        T = self._check(tokens)
        B, U = tokens.shape
        L, H = self.rnn.num_layers, self.rnn.hidden_size
        h, c = self._state(hx, B, T)
        x = ops.gather_rows(tokens, self.embedding.Embedding.weight.detach())                  # (B, U, E)
        hn, cn = [], []
        for k in range(L):                                                                     # (no graph: _check refused grad mode)
            x, hk, ck = _RNN.lstm_apply(x, (h[k] if h is not None else None, c[k] if c is not None else None), self.rnn, k=k)
            hn.append(hk)
            cn.append(ck)
        logits = self._head(x.view(B * U, H), T).view(B, U, -1)
        return logits, (torch.cat(hn, 0), torch.cat(cn, 0))

    def forward(self, x, hx=None):
        """x: tokens (B, U) -> logits (B, U, V), or (B,) -> (B, V); with return_hidden: (logits, (h_n, c_n))."""
        if x.dim() == 1:
            logits, hidden = self.step(x, hx)
        else:
            self._check(x)
            logits, hidden = self._sequence(x, hx)
        return (logits, hidden) if self.return_hidden else logits

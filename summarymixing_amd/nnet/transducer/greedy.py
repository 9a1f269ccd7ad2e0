"""Greedy transducer decoding on the device (recipe key ``Greedysearcher``, …transducer.yaml:375-381: SpeechBrain's
``TransducerBeamSearcher`` with ``beam_size: 1``): frames -> tokens with the whole frame loop inside one call of csrc/greedy.hip.
Three launches per frame, no host synchronisation and no copy to the host; at most one symbol per frame.  The state is per row and
is returned and accepted back, so chunks from ``encode_streaming`` decode to the same tokens as the whole utterance, bit for bit.
SpeechBrain's decoder source is not part of the reference tree: the semantics are its ``transducer_greedy_decode`` written from
memory.  GPU only."""
from typing import NamedTuple, Optional

import torch

from ... import functional as F
from ... import ops
from ..embedding import Embedding
from ..linear import Linear
from ..RNN import LSTM, _transposed, lstm_weights
from .transducer_joint import Transducer_joint


class GreedyState(NamedTuple):
    """Per row: h (B, H) in the operand dtype, c (B, H) fp32, pdec = proj_dec(h) (B, J), frames_seen (B) int32, score (B) fp32 - the
    running sum of the emitted tokens' log-probabilities."""
    h: torch.Tensor
    c: torch.Tensor
    pdec: torch.Tensor
    frames_seen: torch.Tensor
    score: torch.Tensor


class GreedyResult(NamedTuple):
    tokens: torch.Tensor        # (B, T) int32, row b's hypothesis in tokens[b, :counts[b]], padded with -1
    counts: torch.Tensor        # (B) int32
    frames: torch.Tensor        # (B, T) int32: the frame (counted over the whole stream) each token was emitted at; padded with -1
    scores: torch.Tensor        # (B) fp32: sum of log-probabilities of the stream's tokens so far
    state: GreedyState


def _weights(enc, emb, dec, proj_dec, tjoint, transducer_lin):
    """Validate the five modules against `enc` and return the weight images in enc's dtype (raises before any launch)."""
    if not (isinstance(emb, Embedding) and isinstance(dec, LSTM) and isinstance(proj_dec, Linear) and isinstance(transducer_lin, Linear)
            and isinstance(tjoint, Transducer_joint)):
        raise TypeError("greedy_decode: emb, dec, proj_dec, tjoint and transducer_lin must be this package's Embedding, LSTM, Linear, "
                        "Transducer_joint and Linear")
    if not enc.is_cuda:
        raise RuntimeError(ops.NO_CPU)
    if enc.dim() != 3:
        raise ValueError(f"greedy_decode: enc (B, T, J) expected, got {tuple(enc.shape)}")
    ops.dt(enc)
    B, T, J = enc.shape
    H, V = dec.hidden_size, emb.num_embeddings
    Wp, Wl, bl = proj_dec.w.weight, transducer_lin.w.weight, transducer_lin.w.bias
    if proj_dec.w.bias is not None:
        raise NotImplementedError("greedy_decode: proj_dec with a bias is not used by the transducer recipe")
    if dec.rnn.input_size != emb.embedding_dim or tuple(Wp.shape) != (J, H) or tuple(Wl.shape) != (V, J):
        raise ValueError(f"greedy_decode: shapes do not chain: enc J {J}, emb V {V}, dec {dec.rnn.input_size} -> {H}, proj_dec "
                         f"{tuple(Wp.shape)}, transducer_lin {tuple(Wl.shape)}")
    if B < 1:
        raise ValueError("greedy_decode: an empty batch")
    if not ops.greedy_ok(enc.dtype, H, J, V):
        raise NotImplementedError(f"greedy_decode: no kernel for H {H}, J {J}, V {V} (H a multiple of 32 in [32, 4096], J a multiple "
                                  "of 64 in [64, 832], V >= 2)")
    DT = enc.dtype
    Wih, Whh, bsum = lstm_weights(dec.rnn, 0, DT)
    return dict(WihT=F.derived(dec.rnn._derived, "WihT", (Wih,), _transposed), bias=bsum, Whh=Whh, Wproj=F.wcast(Wp, DT).contiguous(),
                Wlin=F.wcast(Wl, DT).contiguous(), blin=bl.detach().float().contiguous() if bl is not None else None,
                act=tjoint.act, blank=emb.blank_id)


def greedy_start(B, w):
    """The state before the first frame: one LSTM step from h = c = 0 on the blank (NOT h = 0), pdec = proj_dec(h)."""
    h, c, pdec, seen = ops.greedy_start(w["bias"], w["Wproj"], B)
    return GreedyState(h, c, pdec, seen, torch.zeros((B,), dtype=torch.float32, device=h.device))


def _run(enc, in_len, w, state):
    """Decode enc on a COPY of `state` (the caller's state tensors are left as they were)."""
    st = GreedyState(*(t.clone() for t in state))
    if enc.shape[1] == 0:
        B = enc.shape[0]
        none = torch.empty((B, 0), dtype=torch.int32, device=enc.device)
        return GreedyResult(none, torch.zeros((B,), dtype=torch.int32, device=enc.device), none.clone(), st.score, st)
    if enc.stride(2) != 1 or enc.stride(0) % 8 != 0 or enc.stride(1) % 8 != 0 or enc.data_ptr() % 16 != 0:
        enc = enc.contiguous()
    tokens, frames, counts = ops.greedy_decode(enc, in_len, w["WihT"], w["bias"], w["Whh"], w["Wproj"], w["Wlin"], w["blin"],
                                               (st.h, st.c, st.pdec, st.frames_seen), st.score, w["act"], w["blank"])
    return GreedyResult(tokens, counts, frames, st.score, st)


def _check_state(state, enc, H):
    B, _, J = enc.shape
    ok = (isinstance(state, GreedyState) and state.h.shape == (B, H) and state.h.dtype == enc.dtype and state.c.shape == (B, H)
          and state.pdec.shape == (B, J) and state.frames_seen.shape == (B,) and state.score.shape == (B,)
          and all(t.device == enc.device for t in state))
    if not ok:
        raise ValueError("greedy_decode: `state` must be the GreedyState a call with the same batch, dtype and modules returned")


def greedy_decode(enc, emb, dec, proj_dec, tjoint, transducer_lin, lengths: Optional[torch.Tensor] = None,
                  state: Optional[GreedyState] = None) -> GreedyResult:
    """enc (B, T, J): the encoder output AFTER proj_enc, fp32 or bf16 (the weights are used in enc's dtype).  lengths: relative
    lengths of THIS call's frames, converted as nnet.losses converts them (round(rel * T)); a row's frames at or beyond its length
    emit nothing and leave its state alone.  None: all T frames (SpeechBrain ignores lengths here).  state: None starts every row
    (one LSTM step on the blank), else the state an earlier call returned - the stream goes on.  Everything returned is on the device."""
    w = _weights(enc, emb, dec, proj_dec, tjoint, transducer_lin)
    B, T, _ = enc.shape
    in_len = None
    if lengths is not None:
        in_len = (lengths.to(enc.device) * T).round().to(torch.int32).contiguous()
        if in_len.shape != (B,):
            raise ValueError(f"greedy_decode: lengths (B,) = ({B},) expected, got {tuple(lengths.shape)}")
    if state is None:
        state = greedy_start(B, w)
    else:
        _check_state(state, enc, dec.hidden_size)
    return _run(enc, in_len, w, state)


class CapturedGreedy:
    """One captured decode of a fixed (B, T): decode(enc, lengths=None, state=None) = greedy_decode(...) as one graph replay (a plain
    chain of 3 T + a few kernels on one stream, no parallel branches).  enc is copied into the static input; the returned tensors
    are static buffers, overwritten by the next replay.  The weight images are those of the capture: capture again after the
    weights changed."""

    def __init__(self, emb, dec, proj_dec, tjoint, transducer_lin, B, T, dtype=torch.float32, device=None):
        device = device or transducer_lin.w.weight.device
        J = transducer_lin.w.weight.shape[1]
        self.B, self.T = B, T
        self.enc = torch.zeros((B, T, J), dtype=dtype, device=device)
        self.in_len = torch.full((B,), T, dtype=torch.int32, device=device)
        self._w = _weights(self.enc, emb, dec, proj_dec, tjoint, transducer_lin)
        # warm-up on a side stream (allocates the workspace and the start state outside the capture)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            self._start = greedy_start(B, self._w)
            self.state_in = GreedyState(*(t.clone() for t in self._start))
            _run(self.enc, self.in_len, self._w, self.state_in)
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.out = _run(self.enc, self.in_len, self._w, self.state_in)

    def decode(self, enc, lengths=None, state=None) -> GreedyResult:
        if tuple(enc.shape) != tuple(self.enc.shape) or enc.dtype != self.enc.dtype:
            raise ValueError(f"CapturedGreedy: captured for {tuple(self.enc.shape)} {self.enc.dtype}, got {tuple(enc.shape)} {enc.dtype}")
        if not enc.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        self.enc.copy_(enc)
        if lengths is None:
            self.in_len.fill_(self.T)
        else:
            self.in_len.copy_((lengths.to(enc.device) * self.T).round().to(torch.int32))
        for dst, src in zip(self.state_in, self._start if state is None else state):
            dst.copy_(src)
        self.graph.replay()
        return self.out

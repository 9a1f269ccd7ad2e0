"""speechbrain.decoders.ctc: greedy (best-path) decoding of the CTC head the recipes train (``ctc_lin`` / ``proj_ctc`` followed by
``Softmax(apply_log=True)``): row arg-max, collapse repeats, drop blanks - csrc/ctcdec.hip.

``ctc_greedy_decode`` / ``filter_ctc_output`` carry upstream's names, arguments and return types (lists of lists of ints, one host
copy at the very end).  ``greedy_decode`` is the device form: nothing in it synchronises with the host, the state is per row and is
returned and accepted back, so chunks from ``encode_streaming`` / ``encode_slots`` decode to the tokens, frames, counts and scores
of the whole utterance bit for bit.  ``greedy_decode_from_encoder`` starts from the encoder output and the head's ``Linear``;
``CapturedCTCGreedy`` is one graph replay per fixed (B, T).  SpeechBrain's decoder source is not part of the reference tree: the
semantics are the ones include/smx.h states (groupby, then filter).  GPU only.  Not built: CTC prefix beam search, ``CTCPrefixScore``
/ ``CTCScorer``, any language model."""
from itertools import groupby
from typing import NamedTuple, Optional, Tuple

import torch

from .. import functional as F
from .. import ops
from ..nnet.linear import Linear

NO_TOKEN = -(1 << 31)           # `prev` before a stream's first frame: equals no token (smx.h: smx_ctc_collapse)


class CTCGreedyState(NamedTuple):
    """Per row, all on the device: prev (B) int32 - the last counted frame's token, frames_seen (B) int32, n_tok (B) int32 - tokens
    emitted since the stream began, score (B) fp32 - the sum of the best path's log-probabilities over the counted frames."""
    prev: torch.Tensor
    frames_seen: torch.Tensor
    n_tok: torch.Tensor
    score: torch.Tensor


class CTCGreedyResult(NamedTuple):
    tokens: torch.Tensor        # (B, cap) int32: row b's hypothesis so far in tokens[b, :counts[b]], padded with -1
    counts: torch.Tensor        # (B) int32 (= state.n_tok); a count above cap: the buffer overflowed, the stored prefix is exact
    frames: torch.Tensor        # (B, cap) int32: the frame (counted over the whole stream) each token was emitted at; padded with -1
    scores: torch.Tensor        # (B) fp32 (= state.score)
    state: CTCGreedyState


def filter_ctc_output(string_pred, blank_id=-1):
    """Upstream's filter on a host list: merge repeats, then drop the blank.  Pure Python."""
    if not isinstance(string_pred, list):
        raise ValueError("filter_ctc_out can only filter python lists")
    return [k for k, _ in groupby(string_pred) if k != blank_id]


def start_state(B, device) -> CTCGreedyState:
    """The state before a stream's first frame."""
    return CTCGreedyState(torch.full((B,), NO_TOKEN, dtype=torch.int32, device=device), torch.zeros((B,), dtype=torch.int32, device=device),
                          torch.zeros((B,), dtype=torch.int32, device=device), torch.zeros((B,), dtype=torch.float32, device=device))


def new_output(B, cap, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Empty (tokens, frames) buffers of `cap` entries per row, to pass as `out` to every call of one stream."""
    return (torch.full((B, cap), -1, dtype=torch.int32, device=device), torch.full((B, cap), -1, dtype=torch.int32, device=device))


def _in_len(lens, B, T, device):
    """Relative lengths -> frames of this call, on the device, as nnet.losses.ctc_loss converts them (round(rel * T))."""
    if lens is None:
        return None
    if tuple(lens.shape) != (B,):
        raise ValueError(f"ctc greedy decoding: lens (B,) = ({B},) expected, got {tuple(lens.shape)}")
    return (lens.to(device) * T).round().to(torch.int32).contiguous()


def _blank(blank, V):
    blank = int(blank)
    if blank < 0:
        blank += V
    if not 0 <= blank < V:
        raise ValueError(f"ctc greedy decoding: blank {blank} outside the vocabulary of {V}")
    return blank


def _collapse(tok, lp, in_len, blank, state, start, out):
    """Collapse on a COPY of `state` (the caller's state tensors are left as they were); `out` is appended to in place."""
    B, T = tok.shape
    dev = tok.device
    if state is None:
        if out is None:
            out = new_output(B, T, dev)
        st = start_state(B, dev)
    else:
        ok = (isinstance(state, CTCGreedyState) and all(t.shape == (B,) and t.device == dev for t in state)
              and all(t.dtype == torch.int32 for t in state[:3]) and state.score.dtype == torch.float32)
        if not ok:
            raise ValueError("ctc greedy decoding: `state` must be the CTCGreedyState a call with the same batch returned")
        if out is None:
            raise ValueError("ctc greedy decoding: a stream that goes on needs its buffers: pass out=(result.tokens, result.frames)")
        st = CTCGreedyState(*(t.clone() for t in state))
    tokens, frames = out
    if start is not None:
        start = start.to(device=dev, dtype=torch.uint8).contiguous()
        if start.shape != (B,):
            raise ValueError(f"ctc greedy decoding: start (B,) = ({B},) expected, got {tuple(start.shape)}")
    ops.ctc_collapse(tok, lp, in_len, blank, start, tuple(st), tokens, frames)
    return CTCGreedyResult(tokens, st.n_tok, frames, st.score, st)


def _check_scores(x, what):
    if not x.is_cuda:
        raise RuntimeError(ops.NO_CPU)
    if x.dim() != 3:
        raise ValueError(f"{what}: (B, T, .) expected, got {tuple(x.shape)}")
    ops.dt(x)
    if x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"{what}: an empty batch or vocabulary")


def _row_pass(scores):
    B, T, V = scores.shape
    if T == 0:
        return (torch.empty((B, 0), dtype=torch.int32, device=scores.device), torch.empty((B, 0), dtype=torch.float32, device=scores.device))
    tok, lp = ops.ctc_best_path(ops.rows2d(scores))
    return tok.view(B, T), lp.view(B, T)


def greedy_decode(scores, lens: Optional[torch.Tensor] = None, blank=0, state: Optional[CTCGreedyState] = None,
                  start: Optional[torch.Tensor] = None, out=None) -> CTCGreedyResult:
    """scores (B, T, V): log-probabilities or raw logits (the arg-max is the same), fp32 or bf16.  lens: relative lengths of THIS
    call's frames; a row's frames at or beyond its length emit nothing and leave its state alone.  blank: negative counts from V.
    state: None starts every row, else the state an earlier call returned - the stream goes on, and `out` must be that stream's
    (tokens, frames) buffers (new_output(B, cap, device), or the earlier result's): tokens are appended behind the stream's count.
    start (B) bool: rows whose state is reset before this call.  Everything returned is on the device."""
    _check_scores(scores, "greedy_decode")
    B, T, V = scores.shape
    tok, lp = _row_pass(scores)
    return _collapse(tok, lp, _in_len(lens, B, T, scores.device), _blank(blank, V), state, start, out)


# Route of greedy_decode_from_encoder: True = the fused head (csrc/ctcdec.hip: ctc_head_kernel on the tile of csrc/head_tile.h), False = this package's Linear, then the
# row pass over the stored logits.  The rule: the fused route only where it beat the unfused pair by more than the run-to-run spread
# of both (its slowest window faster than the other's fastest), measured in the same session: tools/ctcdec_bench.py on one MI355X,
# profiles/ctcdec_bench.jsonl and ctcdec_bench_crossover.jsonl; fused / unfused, medians of 5 windows, N = B T rows:
#   K = 640, V = 1000   N =   752   1504   3008   6016          K = 512, V = 5000   N =  250    500   1000   2000   16000
#   bf16                     0.81 * 0.84 * 0.85 * 0.81 *                                  0.83 * 0.82 * 0.83 * 0.83 * 0.98 *
#   fp32                     0.82 * 0.81 * 0.84 * 0.93 *                                  0.87 * 0.86 * 1.06   1.32   1.03      (* = won)
# bf16: fused at every measured point.  fp32: the tile's v_mfma_f32_32x32x2_f32 loop loses to the library GEMM behind Linear once the
# GEMM is what the call costs; per head width, the largest row count at which the fused route won.  Wider heads and fp32 row counts
# beyond these are unmeasured and take the unfused pair.
_FUSED_F32_MAX_ROWS = ((1000, 6016), (5000, 500))       # (V up to, N up to)


def _plan_fused(N, K, V, dtype):
    if dtype == torch.bfloat16:
        return True
    for v_max, n_max in _FUSED_F32_MAX_ROWS:
        if V <= v_max:
            return N <= n_max
    return False


def _head_weights(x, lin):
    if not isinstance(lin, Linear):
        raise TypeError("greedy_decode_from_encoder: lin must be this package's Linear")
    W, b = lin.w.weight, lin.w.bias
    if W.shape[1] != x.shape[2]:
        raise ValueError(f"greedy_decode_from_encoder: x has {x.shape[2]} features, the head expects {W.shape[1]}")
    return F.wcast(W, x.dtype).contiguous(), (b.detach().float().contiguous() if b is not None else None)


def _head_pass(x, lin, fused):
    B, T, K = x.shape
    V = lin.w.weight.shape[0]
    if T == 0:
        return _row_pass(x.new_empty((B, 0, V)))
    if fused is None:
        fused = _plan_fused(B * T, K, V, x.dtype)
    if fused and ops.ctc_head_ok(x.dtype, K, V):
        Wc, bias = _head_weights(x, lin)
        x2 = ops.rows2d(x)
        if x2.data_ptr() % 16 != 0 or (x2.stride(0) * x2.element_size()) % 16 != 0:
            x2 = x2.contiguous()
        tok, lp = ops.ctc_head_best_path(x2, Wc, bias)
        return tok.view(B, T), lp.view(B, T)
    _head_weights(x, lin)                       # (the same checks on either route)
    with torch.no_grad():
        return _row_pass(lin(x))


def greedy_decode_from_encoder(x, lin, lens: Optional[torch.Tensor] = None, blank=0, state: Optional[CTCGreedyState] = None,
                               start: Optional[torch.Tensor] = None, out=None, fused: Optional[bool] = None) -> CTCGreedyResult:
    """x (B, T, K): the encoder output in front of the CTC head, lin: the head's Linear (K -> V).  greedy_decode of lin(x) without the
    log-softmax (it moves no arg-max, and the row pass takes the maximum's log-probability from the logits).  fused: True asks for
    the fused head, which never stores the logits (where smx_ctc_head_ok refuses the shape the unfused pair runs instead); False for
    Linear + row pass; None lets the planner above choose.  In bf16 the unfused pair reads logits rounded to bf16 and the fused head
    compares the fp32 accumulators: on near-ties the two routes can name different columns (the fused one is the closer to fp64)."""
    _check_scores(x, "greedy_decode_from_encoder")
    B, T, _ = x.shape
    tok, lp = _head_pass(x, lin, fused)
    return _collapse(tok, lp, _in_len(lens, B, T, x.device), _blank(blank, lin.w.weight.shape[0]), state, start, out)


def ctc_greedy_decode(probabilities, seq_lens, blank_id=-1):
    """Upstream's greedy decoder: probabilities (B, T, V) - the head's output (log-)probabilities, seq_lens (B) relative lengths ->
    B lists of ints.  Decoded on the device; one copy to the host at the very end."""
    if isinstance(blank_id, int) and blank_id < 0:
        blank_id = probabilities.shape[-1] + blank_id
    r = greedy_decode(probabilities, seq_lens, blank=blank_id)
    B, cap = r.tokens.shape
    packed = torch.cat([r.tokens, r.counts.view(B, 1)], 1).cpu()                 # the one host copy
    return [[int(k) for k in packed[b, :int(packed[b, cap])]] for b in range(B)]


class CapturedCTCGreedy:
    """One captured decode of a fixed (B, T): decode(x, lens=None, state=None, start=None) = greedy_decode(...) (lin None: x holds
    (B, T, V) scores) or greedy_decode_from_encoder(x, lin, ...) as one graph replay - a plain chain of kernels on one stream, no
    parallel branches.  x is copied into the static input; the returned tensors are static buffers, overwritten by the next replay
    (cap entries per row; a stream that goes on keeps appending to them, state=None starts them empty).  With a Linear the weight
    image is the capture's: capture again after the weights changed."""

    def __init__(self, B, T, width, dtype=torch.float32, blank=0, lin=None, fused=None, cap=None, device=None):
        device = torch.device(device if device is not None else (lin.w.weight.device if lin is not None else "cuda"))
        if device.type != "cuda":
            raise RuntimeError(ops.NO_CPU)
        self.B, self.T, self.lin, self.fused = B, T, lin, fused
        self.blank = _blank(blank, lin.w.weight.shape[0] if lin is not None else width)
        self.x = torch.zeros((B, T, width), dtype=dtype, device=device)
        self.in_len = torch.full((B,), T, dtype=torch.int32, device=device)
        self.start = torch.zeros((B,), dtype=torch.uint8, device=device)
        self._out = new_output(B, T if cap is None else cap, device)
        self._fresh = start_state(B, device)
        self.state_in = CTCGreedyState(*(t.clone() for t in self._fresh))
        # warm-up on a side stream (allocates the workspace and the weight image outside the capture)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            self._run()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.out = self._run()

    def _run(self):
        tok, lp = _row_pass(self.x) if self.lin is None else _head_pass(self.x, self.lin, self.fused)
        return _collapse(tok, lp, self.in_len, self.blank, self.state_in, self.start, self._out)

    def decode(self, x, lens=None, state=None, start=None) -> CTCGreedyResult:
        if tuple(x.shape) != tuple(self.x.shape) or x.dtype != self.x.dtype:
            raise ValueError(f"CapturedCTCGreedy: captured for {tuple(self.x.shape)} {self.x.dtype}, got {tuple(x.shape)} {x.dtype}")
        if not x.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        self.x.copy_(x)
        if lens is None:
            self.in_len.fill_(self.T)
        else:
            self.in_len.copy_(_in_len(lens, self.B, self.T, x.device))
        if start is None:
            self.start.zero_()
        else:
            self.start.copy_(start.to(torch.uint8))
        for dst, src in zip(self.state_in, self._fresh if state is None else state):
            dst.copy_(src)
        if state is None:
            for buf in self._out:
                buf.fill_(-1)
        self.graph.replay()
        return self.out

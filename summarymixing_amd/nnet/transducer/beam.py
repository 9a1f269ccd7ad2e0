"""Transducer beam search on the device (recipe key ``Beamsearcher``, …transducer.yaml:383-393: SpeechBrain's
``TransducerBeamSearcher`` with ``beam_size: 10``, ``lm_module: lm_model``, ``lm_weight: 0.50``, ``state_beam: 2.3``,
``expand_beam: 2.3``), csrc/tbeam.hip.  DESIGN.md §I.25 holds the definition of the search and of its two caps
(``max_expansions`` per frame, ``max_symbols`` per hypothesis), which upstream does not have.

The unit is the EXPANSION, not the frame: every utterance carries its own frame counter on the device and one step expands the
current best open hypothesis of every utterance that is not done.  One step is always the same launches -

    smx_tbeam_step (prediction-network step on the staged token and state, pdec, joint logits of the utterance's own frame)
    -> RNNLM.step on the same staged token and LM state (two smx_lstm_step launches and the head; absent without an LM)
    -> smx_tbeam_select (log-softmaxes, top-k, child inserts, frame logic, next pick, state moves)

- so ``beam_decode`` loops over them and reads the ``done`` vector (B bytes) every ``poll_every`` steps, its only synchronisation, and
``CapturedTransducerBeam`` captures ONE step as a graph - a plain chain, no parallel branches - and replays it in the same loop.  A
search takes at most T * max_expansions steps.  No atomics, fixed summation orders: two runs agree bit for bit, and an utterance's
result does not depend on B or on the other rows.  ``TransducerBeamStream`` carries the search across streaming chunks, one stream per
batch slot: smx_tbeam_resume before a chunk's steps and smx_tbeam_select_stream in place of the selection.  GPU only."""
from typing import NamedTuple, Optional

import torch

from ... import ops
from ...lobes.models.RNNLM import RNNLM
from .greedy import _weights


class TransducerBeamResult(NamedTuple):
    """All on the device, views of the search state's buffers (clone what must outlive the next search over the same state)."""
    tokens: torch.Tensor        # (B, nbest, U) int32, best first, padded with -1
    lengths: torch.Tensor       # (B, nbest) int32 symbols per hypothesis
    scores: torch.Tensor        # (B, nbest) fp32 keys = sums / (lengths + 1); -inf: no such entry
    sums: torch.Tensor          # (B, nbest) fp32 summed log-probabilities (the LM's share included)
    n_hyps: torch.Tensor        # (B) int32 hypotheses returned per utterance
    overflow: torch.Tensor      # (B) int32: bit 0 the expansion cap ended a frame, bit 1 a hypothesis reached max_symbols
    expansions: torch.Tensor    # (B) int32 steps the utterance took
    frames: torch.Tensor        # (B) int32 frames it closed


class TransducerBeamState:
    """The buffers of one search of fixed (B, T, dtype, beam_size, nbest, caps, LM or not): the weight images, the staging rows of the
    hypothesis being expanded, the opaque state block (lists, nodes, prefixes, state slots), the counters and the result."""

    def __init__(self, w, B, T, J, H, V, dtype, device, beam_size, nbest, lm, lm_weight, state_beam, expand_beam, max_expansions, max_symbols):
        self.W, self.nbest, self.H, self.V = int(beam_size), int(nbest), H, V
        self.E = int(max_expansions) if max_expansions is not None else 4 * self.W
        self.U = int(max_symbols) if max_symbols is not None else 2 * T + 8
        if self.E < 1 or self.U < 1:
            raise ValueError(f"beam_decode: max_expansions and max_symbols must be >= 1, got {self.E}, {self.U}")
        self.lm_weight, self.state_beam, self.expand_beam = float(lm_weight), float(state_beam), float(expand_beam)
        self.WihT, self.bias, self.Whh, self.Wproj, self.Wlin, self.blin = (w[k] for k in ("WihT", "bias", "Whh", "Wproj", "Wlin", "blin"))
        self.act, self.blank = w["act"], w["blank"]
        self.lm = lm
        self.lm_L, self.lm_H = (lm.rnn.num_layers, lm.rnn.hidden_size) if lm is not None else (0, 0)
        f32, i32 = torch.float32, torch.int32
        new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self.enc = new((B, T, J), dtype)
        self.lengths = torch.full((B,), T, dtype=i32, device=device)
        self.cur_tok = new((B,), i32)
        self.h_in, self.c_in, self.h_out, self.c_out = new((B, H), dtype), new((B, H), f32), new((B, H), dtype), new((B, H), f32)
        self.pdec, self.z = new((B, J), dtype), new((B, V), f32)
        if lm is not None:
            s = (self.lm_L, B, self.lm_H)
            self.lm_h_in, self.lm_c_in, self.lm_h_out, self.lm_c_out = new(s, dtype), new(s, f32), new(s, dtype), new(s, f32)
        self.state = new((ops.tbeam_state_bytes(dtype, B, H, self.W, self.E, self.U, self.lm_L, self.lm_H),), torch.uint8)
        self.done = new((B,), torch.uint8)
        self.overflow, self.expansions, self.frames, self.n_hyps = new((B,), i32), new((B,), i32), new((B,), i32), new((B,), i32)
        self.tokens, self.out_len = new((B, self.nbest, self.U), i32), new((B, self.nbest), i32)
        self.scores, self.sums = new((B, self.nbest), f32), new((B, self.nbest), f32)

    def begin(self, enc, lengths):
        """A new search over enc (B, T, J) with absolute lengths (B) or None: the inputs copied in, the search state initialised."""
        self.enc.copy_(enc)
        T = self.enc.shape[1]
        if lengths is None:
            self.lengths.fill_(T)
        else:
            self.lengths.copy_(lengths.to(self.enc.device).clamp(0, T).to(torch.int32))
        ops.tbeam_init(self)

    _select = staticmethod(ops.tbeam_select)

    def step(self):
        """The launches of one expansion on the current stream."""
        ops.tbeam_step(self)
        if self.lm is None:
            self._select(self)
        else:
            logits, _ = self.lm.step(self.cur_tok, hx=(self.lm_h_in, self.lm_c_in), out=(self.lm_h_out, self.lm_c_out))
            self._select(self, logits)

    def max_steps(self):
        return self.enc.shape[1] * self.E

    def result(self):
        return TransducerBeamResult(self.tokens, self.out_len, self.scores, self.sums, self.n_hyps, self.overflow, self.expansions, self.frames)


def _check_lm(lm, lm_weight, V, dtype):
    """-> the LM to run, or None when there is none or its weight is 0 (the search is then the plain one, launch for launch)."""
    if lm is None:
        return None
    if not isinstance(lm, RNNLM) or not lm.return_hidden:
        raise NotImplementedError("transducer beam search: lm must be this package's lobes.models.RNNLM.RNNLM with return_hidden=True "
                                  f"(the transducer recipe's lm_model), got {type(lm).__name__}")
    if lm.output_neurons != V:
        raise ValueError(f"transducer beam search: the LM has {lm.output_neurons} outputs, the transducer {V}")
    if not lm_weight > 0.0:
        return None
    if lm.embedding.Embedding.weight.dtype != dtype:
        raise ValueError(f"transducer beam search: the LM computes in {lm.embedding.Embedding.weight.dtype}, enc is {dtype}")
    return lm


def _make_state(enc_like, emb, dec, proj_dec, tjoint, transducer_lin, beam_size, nbest, lm, lm_weight, state_beam, expand_beam, max_expansions,
                max_symbols, cls=TransducerBeamState):
    w = _weights(enc_like, emb, dec, proj_dec, tjoint, transducer_lin)
    B, T, J = enc_like.shape
    H, V = dec.hidden_size, emb.num_embeddings
    if isinstance(beam_size, bool) or int(beam_size) != beam_size or int(nbest) != nbest or not 1 <= nbest <= beam_size:
        raise ValueError(f"transducer beam search: need integers 1 <= nbest <= beam_size, got nbest={nbest}, beam_size={beam_size}")
    if not ops.tbeam_ok(enc_like.dtype, H, J, V, int(beam_size)):
        raise NotImplementedError(f"transducer beam search: no kernel for H {H}, J {J}, V {V}, beam_size {beam_size} (H a multiple of 32 in "
                                  "[32, 4096], J a multiple of 64 in [64, 832], V in [3, 8192], beam_size in [2, 32] and below V)")
    if T < 1:
        raise ValueError("transducer beam search: no frames")
    lm = _check_lm(lm, lm_weight, V, enc_like.dtype)
    return cls(w, B, T, J, H, V, enc_like.dtype, enc_like.device, beam_size, nbest, lm, lm_weight if lm is not None else 0.0, state_beam,
               expand_beam, max_expansions, max_symbols)


def _poll_loop(step, st, poll_every):
    """step() until the done vector, read every poll_every steps, is all set; at most T * max_expansions steps (poll_every=0: all)."""
    n = st.max_steps()
    for i in range(n):
        step()
        if poll_every and (i + 1) % poll_every == 0 and i + 1 < n and bool(st.done.all()):
            break


@torch.no_grad()
def beam_decode(enc, emb, dec, proj_dec, tjoint, transducer_lin, beam_size, nbest=1, lm=None, lm_weight=0.0, state_beam=2.3,
                expand_beam=2.3, lengths: Optional[torch.Tensor] = None, max_expansions=None, max_symbols=None,
                poll_every=32) -> TransducerBeamResult:
    """enc (B, T, J): the encoder output AFTER proj_enc, fp32 or bf16 (the weights are used in enc's dtype).  lm: this package's RNNLM
    (return_hidden=True) in enc's dtype, or None; lm_weight 0 drops it launch for launch.  lengths: ABSOLUTE frames per utterance
    (B), None: all T, as upstream decodes.  max_expansions (default 4 * beam_size) and max_symbols (default 2 * T + 8): the two caps of
    DESIGN.md §I.25, reported per utterance in ``overflow``; on inputs that hit neither the result is upstream's."""
    st = _make_state(enc, emb, dec, proj_dec, tjoint, transducer_lin, beam_size, nbest, lm, lm_weight, state_beam, expand_beam, max_expansions,
                     max_symbols)
    if lengths is not None and tuple(lengths.shape) != (enc.shape[0],):
        raise ValueError(f"beam_decode: lengths (B,) = ({enc.shape[0]},) expected, got {tuple(lengths.shape)}")
    st.begin(enc, lengths)
    _poll_loop(st.step, st, poll_every)
    return st.result()


class CapturedTransducerBeam:
    """beam_decode with ONE step captured as a graph: every position - the frame of each utterance, the lists, the staged hypothesis -
    lives on the device, so the same graph serves every step and every utterance of its (B, T, dtype).  The captured step is a plain
    chain of launches on one stream.  decode(enc, lengths) copies the inputs into the static buffers, initialises the search eagerly and
    replays the graph in beam_decode's polling loop; its result equals beam_decode's bit for bit.  The weight images are those of the
    capture: capture again after the weights changed."""

    def __init__(self, emb, dec, proj_dec, tjoint, transducer_lin, B, T, beam_size, nbest=1, lm=None, lm_weight=0.0, state_beam=2.3,
                 expand_beam=2.3, max_expansions=None, max_symbols=None, dtype=torch.float32, device=None):
        device = device or transducer_lin.w.weight.device
        J = transducer_lin.w.weight.shape[1]
        with torch.no_grad():
            like = torch.zeros((B, T, J), dtype=dtype, device=device)
            self.state = _make_state(like, emb, dec, proj_dec, tjoint, transducer_lin, beam_size, nbest, lm, lm_weight, state_beam,
                                     expand_beam, max_expansions, max_symbols)
            self.state.begin(like, None)
            s = torch.cuda.Stream(device=device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self.state.step()                             # warm-up: weight casts exist before the capture
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=s):
                self.state.step()

    @torch.no_grad()
    def decode(self, enc, lengths=None, poll_every=32) -> TransducerBeamResult:
        st = self.state
        if tuple(enc.shape) != tuple(st.enc.shape) or enc.dtype != st.enc.dtype:
            raise ValueError(f"CapturedTransducerBeam: captured for {tuple(st.enc.shape)} {st.enc.dtype}, got {tuple(enc.shape)} {enc.dtype}")
        if not enc.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        st.begin(enc, lengths)
        _poll_loop(self.graph.replay, st, poll_every)
        return st.result()


class TransducerBeamStreamState(TransducerBeamState):
    """The buffers of B streams fed chunk by chunk: ``enc`` / ``lengths`` / ``frames`` are those of ONE chunk of T = C
    frames, ``start`` marks the slots that begin a new stream and ``stream_frames`` counts the frames of the whole stream - the result's
    ``frames``.  ``done`` means paused; a slot that was never started is paused."""

    _select = staticmethod(ops.tbeam_select_stream)

    def __init__(self, *args):
        super().__init__(*args)
        B, device = self.enc.shape[0], self.enc.device
        self.start = torch.zeros((B,), dtype=torch.uint8, device=device)
        self.stream_frames = torch.zeros((B,), dtype=torch.int32, device=device)
        self.done.fill_(1)

    def result(self):
        return TransducerBeamResult(self.tokens, self.out_len, self.scores, self.sums, self.n_hyps, self.overflow, self.expansions,
                                    self.stream_frames)


class TransducerBeamStream:
    """The beam search of B independent streams, one per batch slot, fed in chunks of at most ``chunk_frames`` frames: after every
    ``decode_chunk`` a slot's result is exactly ``beam_decode``'s over the frames it has been given so far - every field, bit for bit, with
    the same caps - so after the last chunk it is the whole utterance's.  A chunk's last frame writes the result AND
    does the ordinary frame end, so the next chunk goes on from the hypothesis staged there; nothing is recomputed.  ``max_symbols`` has
    no default: a stream has no T to derive it from.  ``captured=True`` captures ONE step as a graph (a plain chain on one stream) and
    replays it in the polling loop; the weight images are then those of the capture.  The returned tensors are views of the buffers:
    clone what must outlive the next call."""

    def __init__(self, emb, dec, proj_dec, tjoint, transducer_lin, B, chunk_frames, beam_size, max_symbols, nbest=1, lm=None, lm_weight=0.0,
                 state_beam=2.3, expand_beam=2.3, max_expansions=None, dtype=torch.float32, device=None, captured=False):
        if max_symbols is None:
            raise ValueError("TransducerBeamStream: max_symbols is required (a stream has no length to derive it from)")
        device = device or transducer_lin.w.weight.device
        J = transducer_lin.w.weight.shape[1]
        self.B, self.chunk_frames = int(B), int(chunk_frames)
        with torch.no_grad():
            like = torch.zeros((self.B, self.chunk_frames, J), dtype=dtype, device=device)
            self.state = _make_state(like, emb, dec, proj_dec, tjoint, transducer_lin, beam_size, nbest, lm, lm_weight, state_beam, expand_beam,
                                     max_expansions, max_symbols, cls=TransducerBeamStreamState)
            self._step = self.state.step
            if captured:
                # every slot is paused, so the warm-up and the captured step select nothing and leave the search state as it is
                s = torch.cuda.Stream(device=device)
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    self.state.step()                         # warm-up: weight casts exist before the capture
                torch.cuda.current_stream().wait_stream(s)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=s):
                    self.state.step()
                self._step = self.graph.replay
        self._started = [False] * self.B
        self._calls = 0

    def _check(self, enc, lengths, start):
        st, B, C = self.state, self.B, self.chunk_frames
        if tuple(enc.shape) != tuple(st.enc.shape) or enc.dtype != st.enc.dtype or enc.device != st.enc.device:
            raise ValueError(f"TransducerBeamStream: made for chunks {tuple(st.enc.shape)} {st.enc.dtype} on {st.enc.device}, got "
                             f"{tuple(enc.shape)} {enc.dtype} on {enc.device}")
        lengths = [C] * B if lengths is None else [int(n) for n in lengths]
        start = [self._calls == 0] * B if start is None else [bool(s) for s in start]
        if len(lengths) != B or len(start) != B:
            raise ValueError(f"TransducerBeamStream: lengths and start hold one entry per slot ({B}), got {len(lengths)} and {len(start)}")
        if any(n < 0 or n > C for n in lengths):
            raise ValueError(f"TransducerBeamStream: lengths {lengths} outside [0, chunk_frames = {C}]")
        never = [b for b in range(B) if lengths[b] > 0 and not (start[b] or self._started[b])]
        if never:
            raise ValueError(f"TransducerBeamStream: frames for slots {never}, which were never started (start[b] = True begins a stream)")
        return lengths, start

    @torch.no_grad()
    def decode_chunk(self, enc, lengths=None, start=None, poll_every=32) -> TransducerBeamResult:
        """enc (B, C, J): one chunk of the encoder output AFTER proj_enc; rows at and beyond lengths[b] may hold anything.  lengths: B host
        ints in [0, C], the frames of this chunk per slot, None: all C.  start: B host bools, the slots that begin a new stream with
        this chunk, None: all on the first call and none afterwards.  A slot with 0 frames that is not started is left exactly as it
        was; a slot whose search ended on a row without numbers (overflow bit 2) ignores frames until it is started again."""
        lengths, start = self._check(enc, lengths, start)
        st = self.state
        st.enc.copy_(enc)
        st.lengths.copy_(torch.tensor(lengths, dtype=torch.int32))
        st.start.copy_(torch.tensor(start, dtype=torch.uint8))
        self._started = [a or b for a, b in zip(self._started, start)]
        self._calls += 1
        ops.tbeam_resume(st)
        n = max(lengths) * st.E                               # a frame takes at most max_expansions steps
        for i in range(n):
            self._step()
            if poll_every and (i + 1) % poll_every == 0 and i + 1 < n and bool(st.done.all()):
                break
        return st.result()

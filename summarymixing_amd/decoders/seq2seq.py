"""Greedy and beam seq2seq decoding over ``[Transformer, seq_lin]``, the pair the Branchformer recipes hand to
``speechbrain.decoders.S2STransformerBeamSearcher`` (recipes/*/ASR/transformer/hparams/branchformer_summarymixing.yaml,
``valid_search`` / ``test_search``), with the whole search on the device:

  one step = TransformerASR.decode_step (KV-cached: smx_s2s_embed_step, per layer smx_attn_step over the caches, csrc/attn_step.hip)
             -> seq_lin (the package's Linear route) -> smx_s2s_select (arg-max, log-probability, append, end-of-sequence flags).

Every position - the decoder position, the hypothesis length, the done flags - is a device counter the kernels read and advance, so
the host issues the same launches at every step: ``greedy_search`` loops over them and reads the ``done`` vector (B bytes) every
``poll_every`` steps, its only synchronisation; ``CapturedS2SGreedy`` captures ONE step as a graph - a plain chain, no parallel
branches - and replays it in the same loop for every step of every utterance of its (B, S).

Beam search is the same step over R = B W hypothesis rows (``beam_search``, ``CapturedS2SBeam``, the module ``S2SBeamSearcher``):
decode_step over a beam state - the self-attention caches are read through an ancestor table (smx_attn_step_rows), so no K / V is
copied when the beams reorder, and the W rows of an utterance share its projected memory - -> seq_lin -> smx_s2s_beam_select (the W
best candidates per utterance, the pool of finished hypotheses, the gathers of the histories and of the ancestor table, in place).
The search is defined in DESIGN.md §I.22.  Still one captured chain, still polled through ``done`` (B bytes).

``S2STransformerGreedySearcher`` and ``S2STransformerBeamSearcher`` take the recipes' constructor arguments and are what they were
before beam search existed: ``S2STransformerBeamSearcher`` refuses ``beam_size > 1`` by name and ``beam_size=1`` without a scorer runs
the greedy search (``length_normalization`` is accepted: one hypothesis has nothing to rank, and the score stays the plain sum).  A
recipe that wants ``beam_size: 10`` points ``valid_search`` at ``summarymixing_amd.decoders.S2SBeamSearcher``, which takes the same
arguments - its ``scorer:`` included when that is the recipes' ``ScorerBuilder`` over a ``CTCScorer`` (decoders.scorer: joint CTC /
attention scoring, two more launches in the same captured chain) and / or a ``TransformerLMScorer`` (LibriSpeech's
``test_search``: one KV-cached ``TransformerLM`` step per hypothesis row and smx_lm_score in the same chain).  Other
scorers and the remaining beam options (eos threshold, attention shift, top-k) are not built and are refused by name.  No parameters of their own: the modules are plain
attributes, as SpeechBrain's searchers hold them outside the checkpointed ``modules``.  SpeechBrain's ``decoders/seq2seq.py`` is not
part of the reference tree: the constructor arguments are the recipes', the returned tuple ``(hyps, lengths, scores, log_probs)`` is
written from memory."""
import collections

import torch

from .. import functional as F
from .. import ops
from . import scorer as _scorer

S2SGreedyResult = collections.namedtuple("S2SGreedyResult", "tokens counts scores log_probs state")
S2SGreedyResult.__doc__ = """tokens (B, cap) int32 (entries at and beyond counts[b] are -1), counts (B) int32, scores (B) fp32 = the sum of
the row's log_probs, log_probs (B, cap) fp32 per emitted token, state: the Transformer.DecodeState - all on the device, all views of
the state's buffers (clone what must outlive the next search over the same state)."""


def _check_args(bos, eos, min_steps, max_steps, temperature):
    if max_steps < 1:
        raise ValueError(f"seq2seq search: max_steps must be >= 1, got {max_steps}")
    if min_steps < 0 or min_steps > max_steps:
        raise ValueError(f"seq2seq search: need 0 <= min_steps <= max_steps, got {min_steps}, {max_steps}")
    if not temperature > 0.0:
        raise ValueError(f"seq2seq search: temperature must be > 0, got {temperature}")
    if bos < 0 or eos < 0:
        raise ValueError(f"seq2seq search: bos / eos must be token indices, got {bos}, {eos}")


def search_step(model, seq_lin, state, eos, min_steps, inv_temp):
    """The launches of one step on the current stream: decode_step on state.tok -> seq_lin -> smx_s2s_select into the state.  -> the
    logits (B, V) the selection read."""
    pred = model.decode_step(state.tok, state)
    W, b = seq_lin.w.weight, seq_lin.w.bias
    logits, _ = F.linear_fwd(pred, F.wcast(W, pred.dtype), b.detach() if b is not None else None)
    ops.s2s_select(logits, state.tok, state.done, state.n_tok, state.score, state.tokens, state.logp_tok, eos, min_steps, inv_temp)
    return logits


def _poll_loop(step, state, max_steps, poll_every):
    """step() max_steps times, or until the done vector, read every poll_every steps, is all set (poll_every=0: never read)."""
    for i in range(max_steps):
        step()
        if poll_every and (i + 1) % poll_every == 0 and i + 1 < max_steps and bool(state.done.all()):
            break


def _begin(model, encoder_out, enc_len, bos, max_steps, state, **beam):
    if not encoder_out.is_cuda:
        raise RuntimeError(ops.NO_CPU)
    state = model.make_decode_state(encoder_out, enc_len, max_steps, state=state, **beam)
    if state.cap != max_steps:
        raise ValueError(f"seq2seq search: max_steps {max_steps} exceeds the positional table ({state.cap} positions)")
    state.tok.fill_(bos)
    return state


def _result(state):
    return S2SGreedyResult(state.tokens, state.n_tok, state.score, state.logp_tok, state)


@torch.no_grad()
def greedy_search(model, seq_lin, encoder_out, enc_len, bos, eos, min_steps, max_steps, temperature=1.0, state=None, poll_every=8):
    """Greedy search of model (a TransformerASR in eval mode) and seq_lin (nnet.linear.Linear d -> V) over encoder_out (B, S, d) with
    the absolute encoder lengths enc_len (B) or None: from bos, at most max_steps tokens per row, a row ends with its first eos (which
    is stored and counted), eos cannot be chosen before min_steps.  state: a DecodeState of this (B, S, max_steps, dtype) to reuse.
    -> S2SGreedyResult."""
    _check_args(bos, eos, min_steps, max_steps, temperature)
    state = _begin(model, encoder_out, enc_len, bos, max_steps, state)
    inv_temp = 1.0 / float(temperature)
    _poll_loop(lambda: search_step(model, seq_lin, state, eos, min_steps, inv_temp), state, max_steps, poll_every)
    return _result(state)


class CapturedS2SGreedy:
    """greedy_search with ONE step captured as a graph: every position lives on the device, so the same graph serves every step and
    every utterance of its (B, S, max_steps, dtype).  The captured step is search_step - a plain chain of launches on one stream.
    search(encoder_out, enc_len) refills the state in place (eager: the cross-attention projections of the new utterance) and replays
    the graph in greedy_search's polling loop; its result equals greedy_search's bit for bit."""

    def __init__(self, model, seq_lin, B, S, max_steps, dtype, bos, eos, min_steps=0, temperature=1.0, device="cuda"):
        _check_args(bos, eos, min_steps, max_steps, temperature)
        self.model, self.seq_lin, self.bos, self.max_steps = model, seq_lin, int(bos), int(max_steps)
        d = model.custom_tgt_module.layers[0].d_model
        eos, min_steps, inv_temp = int(eos), int(min_steps), 1.0 / float(temperature)
        with torch.no_grad():
            mem = torch.zeros((B, S, d), dtype=dtype, device=device)
            self.state = _begin(model, mem, None, self.bos, self.max_steps, None)

            def run():
                search_step(model, seq_lin, self.state, eos, min_steps, inv_temp)
            s = torch.cuda.Stream(device=device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                run()                                         # warm-up: weight casts and packed images exist before the capture
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=s):
                run()
            self.state.reset()

    @torch.no_grad()
    def search(self, encoder_out, enc_len=None, poll_every=8):
        state = _begin(self.model, encoder_out, enc_len, self.bos, self.max_steps, self.state)
        _poll_loop(self.graph.replay, state, self.max_steps, poll_every)
        return _result(state)


S2SBeamResult = collections.namedtuple("S2SBeamResult", "tokens lengths scores sums log_probs counts state")
S2SBeamResult.__doc__ = """The pool of finished hypotheses per utterance, best first: tokens (B, W, cap) int32 (-1 at and beyond lengths),
lengths (B, W) int32 (eos counted; 0: no such entry), scores (B, W) fp32 final scores (-inf: no such entry) = sums / lengths under
length_normalization, else sums; sums (B, W) fp32 the summed log-probabilities, log_probs (B, W, cap) fp32 per token, counts (B) int32
entries per utterance, state: the beam DecodeState - all on the device, all views of the state's buffers."""


def _check_beam(beam_size):
    if not 1 <= int(beam_size) <= 128:
        raise ValueError(f"seq2seq beam search: beam_size must be in [1, 128], got {beam_size}")


def beam_step(model, seq_lin, state, eos, min_steps, inv_temp, length_normalization, scorer=None):
    """The launches of one beam-search step on the current stream: decode_step over the B W rows of the beam state -> seq_lin ->
    smx_s2s_beam_select into the state.  With a scorer (an active ScorerBuilder whose scorer.begin ran on this state) the CTC prefix
    score goes in front of the selection, which reads it as its extra, and the prefix state advances behind it;
    the LM scorer's cached step on the same state.tok and smx_lm_score, which writes or adds to that extra, go between the CTC score
    and the selection.  A scorer whose weight is 0 issues nothing; without any, exactly the launches above.  Still
    one chain on one stream.  -> the logits (B W, V) the selection read."""
    pred = model.decode_step(state.tok, state)
    W, b = seq_lin.w.weight, seq_lin.w.bias
    logits, _ = F.linear_fwd(pred, F.wcast(W, pred.dtype), b.detach() if b is not None else None)
    if scorer is None:
        ops.s2s_beam_select(logits, state, eos, min_steps, inv_temp, length_normalization)
        return logits
    use_ctc = scorer.ctc is not None and scorer.ctc_weight > 0.0
    use_lm = scorer.lm is not None and scorer.lm_weight > 0.0
    extra = None
    if use_ctc:
        if logits.shape[1] != state.ctc.x.shape[2]:
            raise ValueError(f"seq2seq beam search: seq_lin has {logits.shape[1]} outputs, the CTC head {state.ctc.x.shape[2]}")
        extra = ops.ctc_prefix_score(state.ctc, state, logits, inv_temp)
    if use_lm:                                                # one cached LM row per hypothesis, read through the search's ancestors
        ls = state.lm
        if logits.shape[1] != ls.extra.shape[1]:
            raise ValueError(f"seq2seq beam search: seq_lin has {logits.shape[1]} outputs, the language model {ls.extra.shape[1]}")
        z = scorer.lm.lm.step(state.tok, ls, anc=state.anc)
        extra = ops.lm_score(z, ls.extra if extra is None else extra, state, scorer.lm_weight, 1.0 / scorer.lm.temperature, accumulate=use_ctc)
    ops.s2s_beam_select(logits, state, eos, min_steps, inv_temp, length_normalization, extra=extra)
    if use_ctc:
        ops.ctc_prefix_advance(state.ctc, state)
    return logits


def _beam_result(state):
    return S2SBeamResult(state.res_tokens, state.res_len, state.res_final, state.res_sum, state.res_logp, state.pool_cnt, state)


@torch.no_grad()
def beam_search(model, seq_lin, encoder_out, enc_len, bos, eos, min_steps, max_steps, beam_size, temperature=1.0, length_normalization=True,
                state=None, poll_every=8, scorer=None):
    """Beam search of beam_size hypotheses per utterance over encoder_out (B, S, d), greedy_search's arguments otherwise (DESIGN.md
    §I.22 defines the search): a hypothesis ends with its eos, an utterance ends when beam_size hypotheses have ended or at max_steps,
    where the ones alive end as they are.  beam_size=1 gives greedy_search's bits.  state: a beam DecodeState of this (B, S, max_steps,
    dtype, beam_size) to reuse.  scorer: a decoders.scorer.ScorerBuilder - the search then ranks (1 - w_ctc) lp + w_ctc ctc + w_lm lm
    summed over the steps (joint CTC / attention scoring; the TransformerLM scorer, §I.24; the stored log_probs stay
    lp); None or every weight 0: the plain search, launch for launch.  -> S2SBeamResult."""
    _check_args(bos, eos, min_steps, max_steps, temperature)
    _check_beam(beam_size)
    scorer = _scorer.active(scorer)
    state = _begin(model, encoder_out, enc_len, bos, max_steps, state, beam=int(beam_size))
    if scorer is not None:
        _scorer.begin(scorer, state, encoder_out, eos, seq_lin)
    inv_temp, norm = 1.0 / float(temperature), bool(length_normalization)
    _poll_loop(lambda: beam_step(model, seq_lin, state, eos, min_steps, inv_temp, norm, scorer), state, max_steps, poll_every)
    return _beam_result(state)


class CapturedS2SBeam:
    """beam_search with ONE step captured as a graph, as CapturedS2SGreedy captures the greedy step: beam_step is a plain chain of
    launches on one stream and every position is a device counter, so the same graph serves every step and every utterance of its
    (B, S, max_steps, dtype, beam_size).  search(encoder_out, enc_len) equals beam_search bit for bit.  scorer: as beam_search takes it;
    the scorers' launches (the CTC scorer's two, the LM's cached step and smx_lm_score) are part of the captured chain, their
    per-utterance start (the CTC log-probabilities into their fixed buffer, the empty prefix's state, the LM state's counters) runs
    eagerly in search, as the cross-attention projections do."""

    def __init__(self, model, seq_lin, B, S, max_steps, dtype, bos, eos, beam_size, min_steps=0, temperature=1.0, length_normalization=True,
                 device="cuda", scorer=None):
        _check_args(bos, eos, min_steps, max_steps, temperature)
        _check_beam(beam_size)
        self.model, self.seq_lin, self.bos, self.max_steps, self.beam_size = model, seq_lin, int(bos), int(max_steps), int(beam_size)
        self.scorer, self.eos = _scorer.active(scorer), int(eos)
        d = model.custom_tgt_module.layers[0].d_model
        eos, min_steps, inv_temp, norm = int(eos), int(min_steps), 1.0 / float(temperature), bool(length_normalization)
        with torch.no_grad():
            mem = torch.zeros((B, S, d), dtype=dtype, device=device)
            self.state = _begin(model, mem, None, self.bos, self.max_steps, None, beam=self.beam_size)
            if self.scorer is not None:
                _scorer.begin(self.scorer, self.state, mem, eos, seq_lin)

            def run():
                beam_step(model, seq_lin, self.state, eos, min_steps, inv_temp, norm, self.scorer)
            s = torch.cuda.Stream(device=device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                run()                                         # warm-up: weight casts and packed images exist before the capture
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=s):
                run()
            self.state.reset()

    @torch.no_grad()
    def search(self, encoder_out, enc_len=None, poll_every=8):
        state = _begin(self.model, encoder_out, enc_len, self.bos, self.max_steps, self.state, beam=self.beam_size)
        if self.scorer is not None:
            _scorer.begin(self.scorer, state, encoder_out, self.eos, self.seq_lin)
        _poll_loop(self.graph.replay, state, self.max_steps, poll_every)
        return _beam_result(state)


# beam-search options and the one value of each that leaves the greedy search what it is
_BEAM_ONLY = {"topk": 1, "using_eos_threshold": False, "eos_threshold": 1.5, "using_max_attn_shift": False, "max_attn_shift": 60,
              "minus_inf": -1e20}


class S2STransformerGreedySearcher(torch.nn.Module):
    """speechbrain.decoders.S2STransformerGreedySearcher(modules=[model, seq_lin], bos_index, eos_index, min_decode_ratio,
    max_decode_ratio, temperature): forward(enc_states (B, S, d), wav_len (B) relative) -> (hyps: B lists of ints up to and excluding
    the first eos, lengths (B) of them, scores (B) = the summed log-probabilities of the emitted tokens (eos included), log_probs
    (B, max_steps) per emitted token) - the last three tensors on the host, from the ONE copy at the end; the tuple's layout is written
    from memory (module docstring).  max_steps = int(S * max_decode_ratio), min_steps = int(S * min_decode_ratio), enc_len =
    round(S * wav_len)."""

    def __init__(self, modules, bos_index, eos_index, min_decode_ratio, max_decode_ratio, temperature=1.0):
        super().__init__()
        mods = list(modules)
        if len(mods) != 2:
            raise NotImplementedError("S2STransformerGreedySearcher: modules = [Transformer, seq_lin] (the Branchformer recipes') is what "
                                      f"the kernels cover, got {len(mods)} modules")
        if not temperature > 0.0:
            raise ValueError(f"S2STransformerGreedySearcher: temperature must be > 0, got {temperature}")
        if not 0.0 <= min_decode_ratio <= max_decode_ratio:
            raise ValueError(f"S2STransformerGreedySearcher: need 0 <= min_decode_ratio <= max_decode_ratio, got {min_decode_ratio}, "
                             f"{max_decode_ratio}")
        # plain attributes, not registered submodules: the searcher adds nothing to any state_dict
        object.__setattr__(self, "model", mods[0])
        object.__setattr__(self, "fc", mods[1])
        self.bos_index, self.eos_index = int(bos_index), int(eos_index)
        self.min_decode_ratio, self.max_decode_ratio, self.temperature = float(min_decode_ratio), float(max_decode_ratio), float(temperature)

    def forward(self, enc_states, wav_len):
        if not enc_states.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        B, S, _ = enc_states.shape
        max_steps, min_steps = int(S * self.max_decode_ratio), int(S * self.min_decode_ratio)
        enc_len = None if wav_len is None else torch.round(wav_len.to(enc_states.device) * S)
        r = greedy_search(self.model, self.fc, enc_states, enc_len, self.bos_index, self.eos_index, min_steps, max_steps, self.temperature)
        cap = r.tokens.shape[1]
        packed = torch.cat([r.tokens.double(), r.log_probs.double(), r.counts.view(B, 1).double(), r.scores.view(B, 1).double()], 1).cpu()
        tokens, log_probs = packed[:, :cap].long(), packed[:, cap:2 * cap].float()          # the one host copy, taken apart
        counts, scores = packed[:, 2 * cap].long(), packed[:, 2 * cap + 1].float()
        hyps = []
        for b in range(B):
            h = [int(k) for k in tokens[b, :int(counts[b])]]
            hyps.append(h[:h.index(self.eos_index)] if self.eos_index in h else h)
        return hyps, torch.tensor([len(h) for h in hyps]), scores, log_probs


class S2STransformerBeamSearcher(S2STransformerGreedySearcher):
    """speechbrain.decoders.S2STransformerBeamSearcher with the recipes' arguments.  beam_size=1 without a scorer is the greedy search
    above; beam search proper, a scorer (CTC / LM rescoring) and the beam options are not built and are refused by name."""

    def __init__(self, modules, bos_index, eos_index, min_decode_ratio, max_decode_ratio, beam_size, scorer=None, temperature=1.0,
                 **beam_options):
        if scorer is not None:
            raise NotImplementedError("S2STransformerBeamSearcher: a scorer (CTC / LM scoring) belongs to beam search, which is not built "
                                      "(greedy decoding, beam_size=1 without a scorer, is)")
        if beam_size != 1:
            raise NotImplementedError(f"S2STransformerBeamSearcher: beam search (beam_size={beam_size}) is not built; beam_size=1 runs "
                                      "greedy decoding")
        # length_normalization (the recipes pass True) ranks the hypotheses of a beam: with one hypothesis there is nothing to rank, and
        # the score returned stays the plain sum of the log-probabilities either way
        beam_options.pop("length_normalization", None)
        for k, v in beam_options.items():
            if k not in _BEAM_ONLY:
                raise TypeError(f"S2STransformerBeamSearcher: unknown argument {k!r}")
            if v != _BEAM_ONLY[k]:
                raise NotImplementedError(f"S2STransformerBeamSearcher: {k}={v!r} is a beam-search option, which is not built")
        super().__init__(modules, bos_index, eos_index, min_decode_ratio, max_decode_ratio, temperature)
        self.beam_size = 1


# the beam options S2SBeamSearcher does not build, and the one value of each that it takes
_BEAM_UNBUILT = {"topk": 1, "using_eos_threshold": False, "using_max_attn_shift": False}
_BEAM_IGNORED = ("eos_threshold", "max_attn_shift", "minus_inf")      # parameters of options that are off


class S2SBeamSearcher(S2STransformerGreedySearcher):
    """Beam search over modules = [Transformer, seq_lin] with the recipes' ``valid_search`` / ``test_search`` arguments (upstream's
    base-class name; here it is the Transformer searcher).  forward(enc_states (B, S, d), wav_len (B) relative) -> (hyps, lengths,
    scores, log_probs) of the BEST hypothesis per utterance, the greedy searcher's tuple: hyps exclude eos, scores are the final scores
    (the summed log-probabilities over the length, eos counted, under length_normalization), log_probs (B, max_steps) per token - from
    ONE host copy at the end.  beam_size in [1, 128]; scorer: a decoders.scorer.ScorerBuilder (a CTCScorer with its ``ctc`` weight, the
    recipes' joint CTC / attention scoring, and / or a TransformerLMScorer with its ``transformerlm`` weight, LibriSpeech's test_search)
    or None - anything else, using_eos_threshold, using_max_attn_shift and topk > 1 are not built and are refused by name."""

    def __init__(self, modules, bos_index, eos_index, min_decode_ratio, max_decode_ratio, beam_size, scorer=None, temperature=1.0,
                 length_normalization=True, **beam_options):
        if scorer is not None and not isinstance(scorer, _scorer.ScorerBuilder):
            raise NotImplementedError(f"S2SBeamSearcher: scorer must be a decoders.scorer.ScorerBuilder (a CTCScorer and / or a "
                                      f"TransformerLMScorer with their weights are what is built), got {type(scorer).__name__}")
        if isinstance(beam_size, bool) or int(beam_size) != beam_size or not 1 <= beam_size <= 128:
            raise NotImplementedError(f"S2SBeamSearcher: beam_size={beam_size} is outside [1, 128], what the selection kernel holds")
        for k, v in beam_options.items():
            if k in _BEAM_IGNORED:
                continue
            if k not in _BEAM_UNBUILT:
                raise TypeError(f"S2SBeamSearcher: unknown argument {k!r}")
            if v != _BEAM_UNBUILT[k]:
                raise NotImplementedError(f"S2SBeamSearcher: {k}={v!r} is not built")
        super().__init__(modules, bos_index, eos_index, min_decode_ratio, max_decode_ratio, temperature)
        self.beam_size, self.length_normalization = int(beam_size), bool(length_normalization)
        object.__setattr__(self, "scorer", scorer)            # a plain attribute: the CTC head and the LM are the recipe's modules, not the searcher's

    def forward(self, enc_states, wav_len):
        if not enc_states.is_cuda:
            raise RuntimeError(ops.NO_CPU)
        B, S, _ = enc_states.shape
        max_steps, min_steps = int(S * self.max_decode_ratio), int(S * self.min_decode_ratio)
        enc_len = None if wav_len is None else torch.round(wav_len.to(enc_states.device) * S)
        r = beam_search(self.model, self.fc, enc_states, enc_len, self.bos_index, self.eos_index, min_steps, max_steps, self.beam_size,
                        self.temperature, self.length_normalization, scorer=self.scorer)
        cap = r.tokens.shape[2]
        packed = torch.cat([r.tokens[:, 0].double(), r.log_probs[:, 0].double(), r.lengths[:, :1].double(), r.scores[:, :1].double()], 1).cpu()
        tokens, log_probs = packed[:, :cap].long(), packed[:, cap:2 * cap].float()          # the one host copy, taken apart
        counts, scores = packed[:, 2 * cap].long(), packed[:, 2 * cap + 1].float()
        hyps = []
        for b in range(B):
            h = [int(k) for k in tokens[b, :int(counts[b])]]
            hyps.append(h[:h.index(self.eos_index)] if self.eos_index in h else h)
        return hyps, torch.tensor([len(h) for h in hyps]), scores, log_probs

"""speechbrain.decoders.scorer as the Branchformer recipes configure it: ``ctc_scorer: CTCScorer(eos_index, blank_index, ctc_fc:
ctc_lin)`` inside ``ScorerBuilder(full_scorers: [ctc_scorer], weights: {ctc: ctc_weight_decode})``, handed as ``scorer:`` to
``valid_search`` / ``test_search`` (recipes/*/ASR/transformer/hparams/branchformer_summarymixing.yaml) - joint CTC / attention
scoring of the beam search of decoders.seq2seq, on the device inside its one captured step - and, as LibriSpeech's ``test_search``
configures it, ``transformerlm_scorer: TransformerLMScorer(language_model: lm_model, temperature: 1.15)`` beside it in
``scorer_test_search: ScorerBuilder(full_scorers: [transformerlm_scorer, ctc_scorer], weights: {ctc: 0.40, transformerlm: 0.60})``:

  decode_step -> seq_lin -> [smx_ctc_prefix_score] -> [TransformerLM.step -> smx_lm_score] -> smx_s2s_beam_select(extra)
              -> [smx_ctc_prefix_advance]                                      (csrc/ctc_prefix.hip, csrc/lm_score.hip)

The search ranks (1 - weight) lp + weight ctc, ctc[row, c] = psi(g c) - psi(g) the CTC prefix score of extending the row's prefix g
by c; DESIGN.md §I.23 defines it (SpeechBrain's ``decoders/scorer.py`` is not part of the reference tree: the constructor arguments
are the recipes', the scoring is CTC prefix scoring as published, restated in float64 in tests/_ctc_prefix_ref.py).  With the LM the
search ranks (1 - w_ctc) lp + w_ctc ctc + w_lm lm, lm[row, c] = log_softmax(LM logits of the row's prefix / temperature)[c] from one
cached LM step per row.  What runs is at most one CTCScorer (``ctc`` weight in [0, 1]) and at most one
TransformerLMScorer (``transformerlm`` weight >= 0) in ``full_scorers``; other scorers (RNNLMScorer, CoverageScorer, LengthScorer),
``partial_scorers`` (candidate pruning) and a CTC window are not built and are refused by name.  Like the searchers, nothing here
is a registered submodule: no ``state_dict`` grows."""
import torch

from .. import functional as F
from .. import ops


class CTCPrefixState:
    """What CTC prefix scoring carries through a search over a beam DecodeState of (B, S, cap, beam) and a vocabulary of V, all on the
    device at fixed addresses (a captured step points at them): x (B, S, V) fp32 the CTC log-probabilities of the utterances, computed
    once per search; enc_len (B) int32 the state's encoder lengths (frames at and beyond are never read); state (2, R, S, 2) fp32 the
    (r_n, r_b) rows and psi (2, R) the log prefix probabilities, alternated on the parity of the step; extra (R, V) fp32 what
    smx_s2s_beam_select reads.  No buffer needs clearing: what a step reads, an earlier launch of the same search wrote."""

    def __init__(self, st, V, blank, eos, weight):
        B, S, R, dev = st.B, st.S, st.B * st.beam, st.pos.device
        self.blank, self.eos, self.weight = int(blank), int(eos), float(weight)
        self.x = torch.empty((B, S, V), dtype=torch.float32, device=dev)
        self.enc_len = st.mem_len
        self.state = torch.empty((2, R, S, 2), dtype=torch.float32, device=dev)
        self.psi = torch.empty((2, R), dtype=torch.float32, device=dev)
        self.extra = torch.empty((R, V), dtype=torch.float32, device=dev)


class CTCScorer:
    """speechbrain.decoders.scorer.CTCScorer(ctc_fc, blank_index, eos_index, ctc_window_size=0): the CTC head (nnet.linear.Linear
    d -> V) whose log-softmax over the encoder output scores the prefixes.  ctc_window_size != 0 (windowed scoring) is not built."""

    def __init__(self, ctc_fc, blank_index, eos_index, ctc_window_size=0):
        if ctc_window_size != 0:
            raise NotImplementedError(f"CTCScorer: ctc_window_size={ctc_window_size!r} (windowed prefix scoring) is not built; 0 scores "
                                      "over every frame")
        if not hasattr(ctc_fc, "w") or not hasattr(ctc_fc.w, "weight"):
            raise TypeError("CTCScorer: ctc_fc must be the CTC head, an nnet.linear.Linear (the recipes' ctc_lin)")
        if int(blank_index) < 0 or int(eos_index) < 0 or int(blank_index) == int(eos_index):
            raise ValueError(f"CTCScorer: blank_index and eos_index must be distinct token indices, got {blank_index}, {eos_index}")
        self.ctc_fc, self.blank_index, self.eos_index, self.ctc_window_size = ctc_fc, int(blank_index), int(eos_index), 0

    def log_probs(self, encoder_out, out):
        """out (B, S, V) fp32 <- log_softmax(ctc_fc(encoder_out)) in float32: the Linear route, then smx_log_softmax_fwd."""
        B, S, d = encoder_out.shape
        x2 = ops.rows2d(encoder_out if encoder_out.is_contiguous() else encoder_out.contiguous())
        if x2.dtype != torch.float32:
            x2 = ops.cast(x2, torch.float32)
        W, b = self.ctc_fc.w.weight, self.ctc_fc.w.bias
        z, _ = F.linear_fwd(x2, W.detach(), b.detach() if b is not None else None)
        ops.log_softmax_fwd(z, out=out.view(B * S, -1))
        return out


class TransformerLMScorer:
    """speechbrain.decoders.scorer.TransformerLMScorer(language_model, temperature=1.0): the recipes' ``transformerlm_scorer``.  The
    language model is this package's lobes.models.transformer.TransformerLM.TransformerLM, put in eval mode here; the scorer's share of
    a candidate's score is log_softmax(LM logits / temperature) of the candidate token given the hypothesis.
    Upstream runs the LM over every whole prefix at every step; here the LM takes ONE cached step per hypothesis row, inside the
    search's captured chain."""

    def __init__(self, language_model, temperature=1.0):
        from ..lobes.models.transformer.TransformerLM import TransformerLM
        if not isinstance(language_model, TransformerLM):
            raise TypeError("TransformerLMScorer: language_model must be a summarymixing_amd lobes.models.transformer.TransformerLM."
                            f"TransformerLM, got {type(language_model).__name__}")
        if not float(temperature) > 0.0:
            raise ValueError(f"TransformerLMScorer: temperature must be > 0, got {temperature}")
        self.lm, self.temperature = language_model.eval(), float(temperature)


class ScorerBuilder:
    """speechbrain.decoders.scorer.ScorerBuilder(weights, full_scorers, partial_scorers, scorer_beam_scale) with the recipes'
    arguments: full_scorers holds at most one CTCScorer (weight ``weights["ctc"]`` in [0, 1]) and at most one TransformerLMScorer
    (weight ``weights["transformerlm"]`` >= 0); the search then ranks (1 - w_ctc) lp + w_ctc ctc + w_lm lm (upstream's attn_weight =
    1 - ctc_weight plus weights[k] * score_k; w_ctc = 0 without a CTC scorer).  Any other scorer object, a non-empty partial_scorers,
    a weight key without its scorer and two scorers of one kind are refused by name.  scorer_beam_scale only prunes the candidates of
    partial scorers: accepted (CommonVoice passes 0.3) and unused.  ctc / ctc_weight, lm / lm_weight: the scorers and their weights
    (None / 0.0 where there is none)."""

    def __init__(self, weights=None, full_scorers=None, partial_scorers=None, scorer_beam_scale=2.0):
        weights, full, partial = dict(weights or {}), list(full_scorers or []), list(partial_scorers or [])
        if partial:
            raise NotImplementedError("ScorerBuilder: partial_scorers (scoring a pruned candidate set) are not built; pass the scorers "
                                      "in full_scorers")
        for s in full:
            if not isinstance(s, (CTCScorer, TransformerLMScorer)):
                raise NotImplementedError(f"ScorerBuilder: {type(s).__name__} in full_scorers is not built; the CTCScorer and the "
                                          "TransformerLMScorer are")
        ctcs, lms = [s for s in full if isinstance(s, CTCScorer)], [s for s in full if isinstance(s, TransformerLMScorer)]
        for k in weights:
            if k not in ("ctc", "transformerlm"):
                raise NotImplementedError(f"ScorerBuilder: the weight {k!r} names a scorer that is not built; 'ctc' and 'transformerlm' are")
        if "transformerlm" in weights and not lms:
            raise NotImplementedError("ScorerBuilder: the weight 'transformerlm' needs a TransformerLMScorer in full_scorers")
        if len(lms) > 1:
            raise NotImplementedError(f"ScorerBuilder: full_scorers may hold at most one TransformerLMScorer, got {len(lms)}")
        if len(ctcs) > 1 or ("ctc" in weights and not ctcs):
            raise NotImplementedError(f"ScorerBuilder: full_scorers must hold exactly one CTCScorer, got {len(ctcs)}")
        if not full:
            raise NotImplementedError("ScorerBuilder: full_scorers holds no scorer; a CTCScorer and / or a TransformerLMScorer is what runs")
        if ctcs and "ctc" not in weights:
            raise ValueError("ScorerBuilder: weights must give the CTCScorer's weight under 'ctc'")
        if lms and "transformerlm" not in weights:
            raise ValueError("ScorerBuilder: weights must give the TransformerLMScorer's weight under 'transformerlm'")
        w = float(weights["ctc"]) if ctcs else 0.0
        if not 0.0 <= w <= 1.0:
            raise ValueError(f"ScorerBuilder: the ctc weight must lie in [0, 1], got {w}")
        wl = float(weights["transformerlm"]) if lms else 0.0
        if not 0.0 <= wl < float("inf"):
            raise ValueError(f"ScorerBuilder: the transformerlm weight must be finite and >= 0, got {wl}")
        self.ctc, self.ctc_weight, self.scorer_beam_scale = (ctcs[0] if ctcs else None), w, scorer_beam_scale
        self.lm, self.lm_weight = (lms[0] if lms else None), wl
        self.weights, self.full_scorers, self.partial_scorers = weights, full, partial


def active(scorer):
    """The builder if it scores anything: None for scorer=None and when every weight is 0, which drops the scorers - no launch of
    their own, the plain search's bits.  (A scorer whose own weight is 0 is dropped on its own: begin and the step look at
    ctc_weight / lm_weight.)  Anything that is not a ScorerBuilder is refused."""
    if scorer is None:
        return None
    if not isinstance(scorer, ScorerBuilder):
        raise NotImplementedError(f"seq2seq beam search: scorer must be a decoders.scorer.ScorerBuilder, got {type(scorer).__name__}")
    return scorer if (scorer.ctc_weight > 0.0 or scorer.lm_weight > 0.0) else None


def begin(scorer, st, encoder_out, eos, seq_lin=None):
    """The scorers' part of the start of a search over the beam state st.  CTC: the CTC log-probabilities of encoder_out into the
    state's fixed buffer (made on first use, kept on the state as st.ctc) and the prefix state of the empty hypothesis.  LM: the LM's
    cached-step state of R = B W rows and cap = max_steps positions (made on first use, kept as st.lm, reused for the same model), its
    counters reset, advanced under the search's row_done; its own extra (R, V) when there is no CTC scorer to add to.  seq_lin: the
    search's head, whose outputs the LM's vocabulary must equal."""
    cs = None
    if scorer.ctc is not None and scorer.ctc_weight > 0.0:
        cs = _begin_ctc(scorer, st, encoder_out, eos)
    if scorer.lm is not None and scorer.lm_weight > 0.0:
        lm = scorer.lm.lm
        R = st.B * st.beam
        if seq_lin is not None and seq_lin.w.weight.shape[0] != lm.vocab:
            raise ValueError(f"seq2seq beam search: seq_lin has {seq_lin.w.weight.shape[0]} outputs, the language model a vocabulary of {lm.vocab}")
        if st.cap > lm.max_length:
            raise ValueError(f"seq2seq beam search: max_steps {st.cap} exceeds the language model's max_length {lm.max_length}")
        ls = getattr(st, "lm", None)
        if ls is None or ls.model is not lm or (ls.R, ls.cap, ls.compute) != (R, st.cap, st.compute):
            ls = st.lm = lm.make_state(R, st.cap, st.compute, st.pos.device)
            ls.model = lm
            ls.extra = torch.empty((R, lm.vocab), dtype=torch.float32, device=st.pos.device)
        ls.reset()
        ls.done = st.row_done
    return cs


def _begin_ctc(scorer, st, encoder_out, eos):
    ctc = scorer.ctc
    V = ctc.ctc_fc.w.weight.shape[0]
    if ctc.eos_index != int(eos):
        raise ValueError(f"seq2seq beam search: the CTCScorer's eos_index {ctc.eos_index} is not the search's eos {eos}")
    if ctc.blank_index >= V:
        raise ValueError(f"CTCScorer: blank_index {ctc.blank_index} is outside the CTC head's {V} outputs")
    if st.S > 4096:
        raise NotImplementedError(f"CTC prefix scoring stages a row's {st.S} frames in LDS: at most 4096 are built")
    cs = getattr(st, "ctc", None)
    if cs is None or cs.x.shape[2] != V:
        cs = st.ctc = CTCPrefixState(st, V, ctc.blank_index, ctc.eos_index, scorer.ctc_weight)
    cs.blank, cs.eos, cs.weight = ctc.blank_index, ctc.eos_index, scorer.ctc_weight
    ctc.log_probs(encoder_out, cs.x)
    ops.ctc_prefix_init(cs, st)
    return cs

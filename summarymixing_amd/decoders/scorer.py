"""speechbrain.decoders.scorer as the Branchformer recipes configure it: ``ctc_scorer: CTCScorer(eos_index, blank_index, ctc_fc:
ctc_lin)`` inside ``ScorerBuilder(full_scorers: [ctc_scorer], weights: {ctc: ctc_weight_decode})``, handed as ``scorer:`` to
``valid_search`` / ``test_search`` (recipes/*/ASR/transformer/hparams/branchformer_summarymixing.yaml) - joint CTC / attention
scoring of the beam search of decoders.seq2seq, on the device inside its one captured step:

  decode_step -> seq_lin -> smx_ctc_prefix_score -> smx_s2s_beam_select(extra) -> smx_ctc_prefix_advance   (csrc/ctc_prefix.hip)

The search ranks (1 - weight) lp + weight ctc, ctc[row, c] = psi(g c) - psi(g) the CTC prefix score of extending the row's prefix g
by c; DESIGN.md §I.23 defines it (SpeechBrain's ``decoders/scorer.py`` is not part of the reference tree: the constructor arguments
are the recipes', the scoring is CTC prefix scoring as published, restated in float64 in tests/_ctc_prefix_ref.py).  What runs is
exactly one CTCScorer in ``full_scorers`` with a ``ctc`` weight in [0, 1]; LM scorers, ``partial_scorers`` (candidate pruning) and a
CTC window are not built and are refused by name.  Like the searchers, nothing here is a registered submodule: no ``state_dict``
grows."""
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


class ScorerBuilder:
    """speechbrain.decoders.scorer.ScorerBuilder(weights, full_scorers, partial_scorers, scorer_beam_scale) with the recipes'
    arguments: exactly one CTCScorer in full_scorers and its weight ``weights["ctc"]`` in [0, 1] is what runs.  Any other scorer
    object, a non-empty partial_scorers and any other weight key are refused by name.  scorer_beam_scale only prunes the candidates of
    partial scorers: accepted (CommonVoice passes 0.3) and unused."""

    def __init__(self, weights=None, full_scorers=None, partial_scorers=None, scorer_beam_scale=2.0):
        weights, full, partial = dict(weights or {}), list(full_scorers or []), list(partial_scorers or [])
        if partial:
            raise NotImplementedError("ScorerBuilder: partial_scorers (scoring a pruned candidate set) are not built; pass the CTCScorer "
                                      "in full_scorers")
        for s in full:
            if not isinstance(s, CTCScorer):
                raise NotImplementedError(f"ScorerBuilder: {type(s).__name__} in full_scorers is not built (LM scorers are not); the "
                                          "CTCScorer is")
        for k in weights:
            if k != "ctc":
                raise NotImplementedError(f"ScorerBuilder: the weight {k!r} names a scorer that is not built; 'ctc' is")
        if len(full) != 1:
            raise NotImplementedError(f"ScorerBuilder: full_scorers must hold exactly one CTCScorer, got {len(full)}")
        if "ctc" not in weights:
            raise ValueError("ScorerBuilder: weights must give the CTCScorer's weight under 'ctc'")
        w = float(weights["ctc"])
        if not 0.0 <= w <= 1.0:
            raise ValueError(f"ScorerBuilder: the ctc weight must lie in [0, 1], got {w}")
        self.ctc, self.ctc_weight, self.scorer_beam_scale = full[0], w, scorer_beam_scale
        self.weights, self.full_scorers, self.partial_scorers = weights, full, partial


def active(scorer):
    """The builder if it scores anything: None for scorer=None and for a ctc weight of 0, which drops the scorer - no launch of its
    own, the plain search's bits.  Anything that is not a ScorerBuilder is refused."""
    if scorer is None:
        return None
    if not isinstance(scorer, ScorerBuilder):
        raise NotImplementedError(f"seq2seq beam search: scorer must be a decoders.scorer.ScorerBuilder, got {type(scorer).__name__}")
    return scorer if scorer.ctc_weight > 0.0 else None


def begin(scorer, st, encoder_out, eos):
    """The scorer's part of the start of a search over the beam state st: the CTC log-probabilities of encoder_out into the state's
    fixed buffer (made on first use, kept on the state as st.ctc) and the prefix state of the empty hypothesis."""
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

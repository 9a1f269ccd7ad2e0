"""speechbrain.decoders: the searchers the SummaryMixing recipes instantiate (the transducer's greedy search, the seq2seq searchers
over [Transformer, seq_lin] as a KV-cached greedy search, and a beam search over an indexed KV cache, with the recipes' CTC scorer and
TransformerLM scorer: decoders.scorer) and greedy decoding of the CTC head every recipe trains."""
from .ctc import (CapturedCTCGreedy, CTCGreedyResult, CTCGreedyState, ctc_greedy_decode, filter_ctc_output, greedy_decode,
                  greedy_decode_from_encoder)
from .seq2seq import (CapturedS2SBeam, CapturedS2SGreedy, S2SBeamResult, S2SBeamSearcher, S2SGreedyResult, S2STransformerBeamSearcher,
                      S2STransformerGreedySearcher, beam_search, greedy_search)
from . import scorer
from .scorer import CTCScorer, ScorerBuilder, TransformerLMScorer
from . import transducer_beam
from .transducer import TransducerBeamSearcher

__all__ = ["scorer", "transducer_beam", "CTCScorer", "ScorerBuilder", "TransformerLMScorer", "TransducerBeamSearcher", "ctc_greedy_decode", "filter_ctc_output", "greedy_decode", "greedy_decode_from_encoder",
           "CapturedCTCGreedy", "CTCGreedyState", "CTCGreedyResult", "greedy_search", "CapturedS2SGreedy", "S2SGreedyResult",
           "S2STransformerGreedySearcher", "S2STransformerBeamSearcher", "beam_search", "CapturedS2SBeam", "S2SBeamResult", "S2SBeamSearcher"]

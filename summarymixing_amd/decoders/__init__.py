"""speechbrain.decoders: the searchers the SummaryMixing recipes instantiate (the transducer's greedy search) and greedy decoding
of the CTC head every recipe trains."""
from .ctc import (CapturedCTCGreedy, CTCGreedyResult, CTCGreedyState, ctc_greedy_decode, filter_ctc_output, greedy_decode,
                  greedy_decode_from_encoder)
from .transducer import TransducerBeamSearcher

__all__ = ["TransducerBeamSearcher", "ctc_greedy_decode", "filter_ctc_output", "greedy_decode", "greedy_decode_from_encoder",
           "CapturedCTCGreedy", "CTCGreedyState", "CTCGreedyResult"]

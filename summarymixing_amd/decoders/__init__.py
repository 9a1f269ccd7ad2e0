"""speechbrain.decoders: the searchers the SummaryMixing recipes instantiate (the transducer's greedy search)."""
from .transducer import TransducerBeamSearcher

__all__ = ["TransducerBeamSearcher"]

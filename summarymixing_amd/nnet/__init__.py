"""Drop-in modules under SpeechBrain's import paths (speechbrain.nnet.* -> summarymixing_amd.nnet.*)."""
from .embedding import Embedding
from .RNN import LSTM

__all__ = ["Embedding", "LSTM"]

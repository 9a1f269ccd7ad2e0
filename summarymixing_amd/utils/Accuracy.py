"""speechbrain.utils.Accuracy: the token accuracy the Branchformer recipes report at validation (recipe key ``acc_computer``,
…/LibriSpeech/ASR/transformer/hparams/branchformer_summarymixing.yaml:347).  The argmax and the comparison run in the row pass of
csrc/seqloss.hip (first index among equal entries, as torch.argmax); the counters stay on the device."""
import torch

from ..nnet import losses


def Accuracy(log_probabilities, targets, length=None):
    """-> (correct, total): 0-d int64 tensors on the device (upstream returns the same two numbers as Python floats, which costs
    a host synchronisation per batch; float() them if that is wanted).  log_probabilities (B, U, V) (any scores: only the argmax
    matters), targets (B, U), length the RELATIVE lengths or None; the kept positions are those of the losses' length mask."""
    if log_probabilities.dim() == 2 and targets.dim() == 1:
        log_probabilities, targets = log_probabilities.unsqueeze(1), targets.unsqueeze(1)
    _, hits, kept = losses._nll("Accuracy", log_probabilities, targets, length, 0.0, 0, "none", False)
    return hits.sum(), kept.sum()


class AccuracyStats:
    """speechbrain.utils.Accuracy.AccuracyStats: append() adds a batch into two device counters without a host synchronisation;
    summarize() is the one copy to the host."""

    def __init__(self):
        self.correct = None
        self.total = None

    def append(self, log_probabilities, targets, length=None):
        c, t = Accuracy(log_probabilities, targets, length)
        if self.correct is None:
            self.correct, self.total = c.clone(), t.clone()
        else:
            self.correct += c
            self.total += t

    def summarize(self):
        if self.correct is None:
            return float("nan")
        c, t = torch.stack((self.correct, self.total)).tolist()
        return c / t if t else float("nan")

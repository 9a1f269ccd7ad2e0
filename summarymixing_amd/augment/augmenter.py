"""speechbrain.augment.augmenter.Augmenter in the recipes' configuration (``fea_augment``, …/transducer/hparams/
conformer_summarymixing_transducer.yaml:240-245): the augmentations applied one after another to the whole batch, every one of
them, once, with probability 1, nothing concatenated.  Every other option raises NotImplementedError naming it."""
import torch.nn as nn

from .. import _lib as L
from .. import functional as SF
from .freq_domain import SpectrogramDrop, Warping, _features
from .time_domain import Resample, SpeedPerturb

# what the constructor accepts for the options that are not built: name -> the values that mean "off"
_FIXED = {"parallel_augment": (False,), "concat_original": (False,), "shuffle_augmentations": (False,), "repeat_augment": (1,),
          "augment_start_index": (0,), "augment_end_index": (None,), "concat_start_index": (0,), "concat_end_index": (None,),
          "augment_prob": (1.0, 1), "enable_augmentations": (None,)}


def _slot(m):
    """Position of a module in the fused chain [time drop, frequency drop, warp], or None."""
    if isinstance(m, SpectrogramDrop):
        return 0 if m.dim == 1 else 1
    return 2 if isinstance(m, Warping) else None


class Augmenter(nn.Module):
    """forward(x, lengths) -> (augmented x, lengths).  A list of one waveform stage (the recipes' wav_augment: [SpeedPerturb] with
    min_augmentations = max_augmentations = 1) resamples the batch (B, T) -> (B, T') in one launch.  A list that is a subsequence
    of [SpectrogramDrop(dim=1), SpectrogramDrop(dim=2), Warping] runs as ONE draw launch and ONE pass over x (drops first, then the warp, which interpolates
    across the zeroed stripes exactly as the module-by-module chain does); any other list runs module by module through the
    same kernel.  `seed` / `last_params`: as on the stages (freq_domain._Stage)."""

    def __init__(self, parallel_augment=False, concat_original=False, min_augmentations=None, max_augmentations=None,
                 shuffle_augmentations=False, repeat_augment=1, augment_start_index=0, augment_end_index=None,
                 concat_start_index=0, concat_end_index=None, augment_prob=1.0, augmentations=None, enable_augmentations=None):
        super().__init__()
        given = dict(parallel_augment=parallel_augment, concat_original=concat_original, shuffle_augmentations=shuffle_augmentations,
                     repeat_augment=repeat_augment, augment_start_index=augment_start_index, augment_end_index=augment_end_index,
                     concat_start_index=concat_start_index, concat_end_index=concat_end_index, augment_prob=augment_prob,
                     enable_augmentations=enable_augmentations)
        for name, value in given.items():
            if not any(type(value) is type(ok) and value == ok for ok in _FIXED[name]):
                raise NotImplementedError(f"Augmenter({name}={value!r}) is not built: only {name}={_FIXED[name][0]!r}")
        augmentations = list(augmentations or [])
        for name, value in (("min_augmentations", min_augmentations), ("max_augmentations", max_augmentations)):
            if value is not None and value != len(augmentations):
                raise NotImplementedError(f"Augmenter({name}={value!r}) is not built: every augmentation runs on every call "
                                          f"({name}=None or {len(augmentations)})")
        # the recipes' wav_augment (…transducer.yaml:181-192): one waveform stage, applied to every batch
        wave = [isinstance(m, (SpeedPerturb, Resample)) for m in augmentations]
        self.waveform = any(wave)
        if self.waveform and not all(wave):
            raise NotImplementedError("augmentations: a list that mixes waveform stages (SpeedPerturb, Resample) with spectrogram "
                                      "stages (SpectrogramDrop, Warping) is not built: wav_augment and fea_augment are two Augmenters")
        if self.waveform and len(augmentations) > 1:
            raise NotImplementedError(f"augmentations: {len(augmentations)} waveform stages are not built (one is: the recipes' "
                                      "[speed_perturb])")
        for m in augmentations:
            if _slot(m) is None and not self.waveform:
                raise NotImplementedError(f"augmentations: {type(m).__name__} is not built (SpectrogramDrop and Warping are)")
        self.augmentations = nn.ModuleList(augmentations)
        slots = [_slot(m) for m in augmentations]
        self.fused = not self.waveform and len(slots) > 0 and all(a < b for a, b in zip(slots, slots[1:]))
        self.seed = None
        self.last_params = None

    def forward(self, x, lengths):
        if self.waveform:                                    # (B, T) samples; relative lengths stay what they were
            return self.augmentations[0](x), lengths
        x = _features(x)
        if self.fused:
            B, T, F = x.shape
            kw, stages = {}, 0
            for m in self.augmentations:
                kw.update(m.draw_args())
                stages |= m.stage
            self.last_params = SF.spec_augment_draw(B, T, F, x.device, stages, seed=self.seed, **kw)
            return SF.spec_augment(x, self.last_params), lengths
        for m in self.augmentations:
            x = m(x)
        return x, lengths

    def replicate_labels(self, labels):
        """Nothing is concatenated, so labels pass through (the recipes' train.py calls this after fea_augment)."""
        return labels

    def replicate_multiple_labels(self, *args):
        return args

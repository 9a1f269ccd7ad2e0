"""summarymixing_amd.augment <-> speechbrain.augment: the feature augmentation of the recipes' ``fea_augment``
(freq_domain.SpectrogramDrop, freq_domain.Warping, augmenter.Augmenter) and the waveform augmentation of their ``wav_augment``
(time_domain.SpeedPerturb, time_domain.Resample, the same Augmenter) on the HIP path."""
from . import augmenter, freq_domain, time_domain  # noqa: F401

__all__ = ["augmenter", "freq_domain", "time_domain"]

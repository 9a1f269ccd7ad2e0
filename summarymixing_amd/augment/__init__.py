"""summarymixing_amd.augment <-> speechbrain.augment: the feature augmentation of the recipes' ``fea_augment``
(freq_domain.SpectrogramDrop, freq_domain.Warping, augmenter.Augmenter) on the HIP path."""
from . import augmenter, freq_domain  # noqa: F401

__all__ = ["augmenter", "freq_domain"]

"""speechbrain.augment.freq_domain as the recipes instantiate it (…/transducer/hparams/conformer_summarymixing_transducer.yaml:
195-238): SpectrogramDrop along time and along frequency, and the bicubic time Warping.  Upstream's package is not part of the
reference tree; the semantics built here are written down in DESIGN.md §I.15.  Every module draws on the device
(smx_specaug_draw) and applies its stage with the one kernel of the fused chain (smx_specaug_apply): no host-drawn shapes, so a
step that holds them can be captured in a hipGraph, and with a device step counter set (ops.set_step_counter) every replay
draws afresh.  There is no CPU fallback and no backward (features carry no gradient)."""
import torch
import torch.nn as nn

from .. import _lib as L
from .. import functional as SF
from .. import ops


def _features(x):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("summarymixing_amd kernels run on the GPU only (no CPU fallback)")
    if x.dim() != 3:
        raise NotImplementedError(f"(batch, time, features) input only (upstream's 4-D form is not built), got {tuple(x.shape)}")
    return x


class _Stage(nn.Module):
    """One stage of the chain.  `seed`: None draws a fresh seed per call (ops.new_dropout_seed), an int fixes it (the device step
    counter still advances the draws); `last_params` keeps the block of the last call."""
    stage = 0

    def __init__(self):
        super().__init__()
        self.seed = None
        self.last_params = None

    def draw_args(self):
        """Keyword arguments of functional.spec_augment_draw for this stage."""
        raise NotImplementedError

    def forward(self, x):
        x = _features(x)
        B, T, F = x.shape
        self.last_params = SF.spec_augment_draw(B, T, F, x.device, self.stage, seed=self.seed, **self.draw_args())
        return SF.spec_augment(x, self.last_params)


class SpectrogramDrop(_Stage):
    """Zeroes `n` stripes per utterance along time (dim=1) or frequency (dim=2): n uniform on [drop_count_low, drop_count_high]
    (one value for the batch), each stripe's length uniform on [drop_length_low, drop_length_high) and its start on [0, D), clipped
    at D.  Utterance lengths are ignored, as upstream ignores them."""

    def __init__(self, drop_length_low=5, drop_length_high=15, drop_count_low=1, drop_count_high=3, replace="zeros", dim=1):
        super().__init__()
        if replace != "zeros":
            raise NotImplementedError(f"replace={replace!r}: only 'zeros' is built")
        if dim not in (1, 2):
            raise NotImplementedError(f"dim={dim}: drops run along time (1) or frequency (2)")
        if not (0 <= drop_length_low < drop_length_high and 0 <= drop_count_low <= drop_count_high):
            raise ValueError("need 0 <= drop_length_low < drop_length_high and 0 <= drop_count_low <= drop_count_high")
        if drop_count_high > 32:
            raise NotImplementedError(f"drop_count_high={drop_count_high}: at most 32 drops per utterance")
        self.drop_length_low, self.drop_length_high = int(drop_length_low), int(drop_length_high)
        self.drop_count_low, self.drop_count_high = int(drop_count_low), int(drop_count_high)
        self.replace, self.dim = replace, dim
        self.stage = L.SPECAUG_TIME if dim == 1 else L.SPECAUG_FREQ

    def ranges(self):
        return (self.drop_length_low, self.drop_length_high, self.drop_count_low, self.drop_count_high)

    def draw_args(self):
        return {"time_drop" if self.dim == 1 else "freq_drop": self.ranges()}


class Warping(_Stage):
    """Time warp: one centre c on [warp_window, T - warp_window) and one target w on [c - warp_window + 1, c + warp_window] for the
    batch; frames [0, c) are resampled to w frames and frames [c, T) to T - w, bicubic with aligned corners.  Utterances with
    T - warp_window <= warp_window pass through unchanged."""
    stage = L.SPECAUG_WARP

    def __init__(self, warp_window=5, warp_mode="bicubic", dim=1):
        super().__init__()
        if warp_mode != "bicubic":
            raise NotImplementedError(f"warp_mode={warp_mode!r}: only 'bicubic' is built")
        if dim != 1:
            raise NotImplementedError(f"dim={dim}: the warp runs along time (1) only")
        if warp_window < 1:
            raise ValueError("warp_window must be positive")
        self.warp_window, self.warp_mode, self.dim = int(warp_window), warp_mode, dim

    def draw_args(self):
        return {"window": self.warp_window}

"""speechbrain.augment.time_domain as the recipes instantiate it (…/transducer/hparams/conformer_summarymixing_transducer.yaml:
177-179): SpeedPerturb and the Resample it is made of.  Upstream's module is not part of the reference tree; what is built here is
what speechbrain 1.0's Resample computes by wrapping torchaudio.transforms.Resample at its defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99), written down in DESIGN.md §I.16.  One launch per batch (smx_resample); no CPU fallback and
no backward (waveforms carry no gradient)."""
import torch
import torch.nn as nn

from .. import functional as SF


class Resample(nn.Module):
    """forward(waveforms): (B, T) or (B, T, 1) float32 on the GPU -> the batch at new_freq, ceil(n T / o) samples per row with
    o / n the reduced rates.  Equal rates return the input itself.  The plan of the ratio is built once and uploaded once per
    device (functional.resample_plan holds both)."""

    def __init__(self, orig_freq=16000, new_freq=16000, *args, **kwargs):
        super().__init__()
        if args:
            raise NotImplementedError(f"Resample: positional arguments after new_freq are not built (got {args!r}): torchaudio's "
                                      "defaults are (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99)")
        for name in kwargs:
            raise NotImplementedError(f"Resample({name}=...) is not built: torchaudio's defaults are (resampling_method "
                                      "'sinc_interp_hann', lowpass_filter_width 6, rolloff 0.99)")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        if self.orig_freq != self.new_freq:
            self.plan = SF.resample_plan(self.orig_freq, self.new_freq)[0]     # an unsupported ratio is refused here, by name

    def forward(self, waveforms):
        if self.orig_freq == self.new_freq:
            return waveforms
        if not torch.is_tensor(waveforms) or not waveforms.is_cuda:
            raise RuntimeError("summarymixing_amd kernels run on the GPU only (no CPU fallback)")
        if waveforms.dim() == 2:
            return SF.resample(waveforms, self.orig_freq, self.new_freq)
        if waveforms.dim() != 3:
            raise ValueError("Input must be 2 or 3 dimensions")
        if waveforms.shape[2] != 1:
            raise NotImplementedError(f"channels={waveforms.shape[2]}: (batch, time, channels) input with more than one channel is "
                                      "not built")
        return SF.resample(waveforms.squeeze(2), self.orig_freq, self.new_freq).unsqueeze(2)


class SpeedPerturb(nn.Module):
    """Resamples the whole batch to orig_freq * speed // 100 for one speed drawn per call and lets the result pass as orig_freq
    audio: speed 95 slows the batch down (more samples), 105 speeds it up.  The draw is upstream's own call on torch's global CPU
    generator, so under one torch.manual_seed the sequence of speeds is upstream's; nothing is drawn on or read from the device.
    `device` is accepted and ignored as upstream ignores it.  The resamplers sit in a plain list: state_dict() is empty."""

    def __init__(self, orig_freq, speeds=[90, 100, 110], device="cpu"):
        super().__init__()
        self.orig_freq = orig_freq
        self.speeds = speeds
        self.device = device
        self.samp_index = 0
        self.resamplers = [Resample(orig_freq=self.orig_freq, new_freq=self.orig_freq * speed // 100) for speed in self.speeds]

    def draw(self):
        """The index of this call's speed: a 0-dim int64 CPU tensor, as upstream draws it."""
        return torch.randint(len(self.speeds), (1,))[0]

    def forward(self, waveform):
        self.samp_index = self.draw()
        return self.resamplers[self.samp_index](waveform)

"""The float64 restatement of the log-mel front-end (tests/_fbank_ref.py: the yardstick of tests/test_fbank_kernels_gpu.py) checked
on the CPU against oracle.smx_oracle.fbank (torch.stft) and mel_filterbank; the constants Fbank.__init__ derives (fold,
drop_nyquist, im_off, the registered bases and filters) against the same restatement; and the proof that the stage bars of the GPU
tests have teeth: a reference that loses one end-point sample of the fold, or one tap of the widest mel band, misses them."""
import math

import pytest
import torch

from oracle import smx_oracle as O
from tests import _fbank_ref as R


def _noise(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    wav = torch.randn(B, L, generator=g) * torch.tensor([1.0, 0.03, 0.001])[:B, None]
    wav[0, L // 2:] = 0.0                                                           # trailing silence in the loudest utterance
    return wav


@pytest.mark.parametrize("n_fft,win_ms,n_mels,L", [(512, 32, 80, 4000), (400, 25, 40, 3333)])
def test_restatement_equals_the_stft_oracle(n_fft, win_ms, n_mels, L):
    wav = _noise(3, L, n_fft).double()
    fbm = R.mel_filters(n_mels, n_fft).float()
    assert torch.equal(fbm, O.mel_filterbank(n_mels, n_fft, 16000))
    j = torch.arange(n_fft, dtype=torch.float64)
    assert float((R.hamming(n_fft) - (0.54 - 0.46 * torch.cos(2 * math.pi * j / n_fft))).abs().max()) <= 1e-15
    got = R.pipeline(wav, n_fft, 160, fbm)["out"]
    ref = O.fbank(wav, n_fft=n_fft, win_length_ms=win_ms, n_mels=n_mels)
    assert got.shape == ref.shape == (3, 1 + L // 160, n_mels)
    assert float((got - ref).abs().max()) <= 1e-9                                   # dB
    # the clamp is live in this input (utterance 0 ends in silence) and the filters with f_min / f_max are the oracle's too
    assert float(ref[0].max() - ref[0].min()) == 80.0
    assert torch.equal(R.mel_filters(23, n_fft, 16000, 50.0, 7600.0).float(), O.mel_filterbank(23, n_fft, 16000, 50.0, 7600.0))


def test_frames_are_centre_padded_with_zeros():
    wav = torch.arange(1.0, 11.0)[None]                                             # L = 10, hop 4 -> T = 3
    fr = R.frames(wav, 8, 4)
    assert fr.shape == (1, 3, 8)
    assert fr[0, 0].tolist() == [0, 0, 0, 0, 1, 2, 3, 4] and fr[0, 2].tolist() == [5, 6, 7, 8, 9, 10, 0, 0]
    assert R.frames(torch.ones(2, 3), 8, 4).shape == (2, 1, 8)                      # L < hop: one frame


def test_band_limits_and_the_documented_filter_bank_shapes():
    """The shapes the GPU mel/dB test relies on: bands wider than the kernel's 48-tap LDS image, and filters without a tap."""
    assert R.widest_band(R.mel_filters(80, 512).float()) <= 48
    assert R.widest_band(R.mel_filters(20, 512).float()) == 56
    assert R.widest_band(R.mel_filters(40, 2048).float()) == 125
    lo, hi = R.band_limits(R.mel_filters(80, 256).float())
    assert int((hi <= lo).sum()) == 2 and lo[hi <= lo].tolist() == [129, 129] and hi[hi <= lo].tolist() == [0, 0]


def test_fbank_refuses_what_it_does_not_build():
    from summarymixing_amd.lobes.features import Fbank
    for kw in (dict(win_length=32), dict(n_fft=512), dict(deltas=True), dict(context=True), dict(filter_shape="gaussian"),
               dict(filter_shape="rectangular"), dict(requires_grad=True)):
        with pytest.raises(NotImplementedError):
            Fbank(**kw)
    Fbank()                                                                          # the class default itself is built


@pytest.mark.parametrize("n_fft,win_ms,n_mels,fold,drop,im_off", [(256, 16, 80, True, True, 132), (400, 25, 40, True, False, 204),
                                                                   (512, 32, 80, True, True, 260), (2048, 128, 40, True, True, 1028)])
def test_fbank_constants_equal_the_restatement(n_fft, win_ms, n_mels, fold, drop, im_off):
    from summarymixing_amd.lobes.features import Fbank
    fb = Fbank(n_fft=n_fft, n_mels=n_mels, win_length=win_ms)
    half, n_bins = n_fft // 2, n_fft // 2 + 1
    assert (fb.fold, fb.drop_nyquist, fb.im_off, fb.hop, fb.win) == (fold, drop, im_off, 160, n_fft)
    c, s = R.dft_basis(n_fft)
    cw, sw = R.windowed_basis(n_fft, torch.float32)
    assert torch.equal(fb.window, R.hamming(n_fft, torch.float32))
    # the plain and the windowed (2 im_off, n_fft) bases: cos rows at 0, -sin rows at im_off, zero rows between
    for got, (rc, rs) in ((fb.basis, (c.float(), s.float())), (fb.basis_w, (cw, sw))):
        assert got.shape == (2 * im_off, n_fft)
        assert torch.equal(got[:n_bins], rc) and torch.equal(got[im_off:im_off + n_bins], rs)
        assert not got[n_bins:im_off].any() and not got[im_off + n_bins:].any()
    # the folded halves: cos on j = 0 .. n/2 (+ 3 zero columns), -sin on j = 0 .. n/2 - 1; without the Nyquist row when dropped
    rows = half if drop else im_off
    nr = min(n_bins, rows)
    assert fb.basis_cos.shape == (rows, half + 4) and fb.basis_sin.shape == (rows, half)
    assert torch.equal(fb.basis_cos[:nr, :half + 1], cw[:nr, :half + 1]) and not fb.basis_cos[:, half + 1:].any()
    assert torch.equal(fb.basis_sin[:nr], sw[:nr, :half])
    assert not fb.basis_cos[nr:].any() and not fb.basis_sin[nr:].any()
    fbm = R.mel_filters(n_mels, n_fft).float()
    assert torch.equal(fb.fb, fbm) and torch.equal(fb.fb_nn, fbm[:, :half])
    assert not fbm[:, -1].any()                                                      # what drop_nyquist rests on


def test_fbank_keeps_the_nyquist_row_when_a_filter_weighs_it():
    from summarymixing_amd.lobes.features import Fbank
    fb = Fbank(n_fft=512, n_mels=80, win_length=32, f_max=8400)                       # (a band reaching past sample_rate / 2)
    assert fb.fold and not fb.drop_nyquist and float(fb.fb[:, -1].max()) > 0
    assert torch.equal(fb.fb, R.mel_filters(80, 512, 16000, 0, 8400).float())


@pytest.mark.parametrize("n_fft,hop", [(512, 160), (400, 160), (256, 80), (2048, 160)])
def test_spectrum_bar_catches_a_dropped_fold_end_point(n_fft, hop):
    """The bar of the GPU spectrum test is (n_fft + 4) 2^-24 sum_j |x_j| w_j per frame.  A loader that drops the j = 0 end point of
    the fold changes re by 0.08 x[0] (w[0] = 0.08), one that drops j = n/2 by x[n/2] (w = 1): both perturbed references miss
    the bar against the true one - and the float32 evaluation of the same DFT (the floor) meets it."""
    wav = _noise(3, 20 * hop + 37, n_fft)
    fr = R.frames(wav.double(), n_fft, hop)
    re, im = R.spectrum(fr, R.hamming(n_fft))
    bar = R.spectrum_bar(fr, n_fft)
    w = R.hamming(n_fft)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
    live = fr.abs().sum(-1) > 0
    for j in (0, n_fft // 2):
        tap = fr[..., j:j + 1] * w[j] * torch.cos(2 * math.pi * k * j / n_fft)        # this sample's share of re (none of im at these j)
        miss = ((re - tap) - re).abs() > bar
        assert miss.any(-1)[live & (fr[..., j] != 0)].float().mean() > (0.1 if j == 0 else 0.8), j     # (share of the live frames that miss it)
    re32, im32 = R.spectrum(fr.float(), R.hamming(n_fft, torch.float32))
    assert ((re32.double() - re).abs() <= bar).all() and ((im32.double() - im).abs() <= bar).all()
    assert not re[~live].any() and not im[~live].any()                              # (and there are frames wholly in zeros)
    assert int((~live).sum()) > 0


def test_mel_db_bar_catches_a_lost_tap_of_the_widest_band():
    """Same idea for the mel / dB stage: without the last tap of its widest band (n_fft = 512, 20 mels: 56 bins) the reference misses
    bar = (10 / ln 10) (w_max + 4) 2^-24 + 4 x float32 floor, in that filter's column; the float32 floor itself meets it."""
    g = torch.Generator().manual_seed(5)
    fbm = R.mel_filters(20, 512).float()
    re, im = torch.randn(64, 257, generator=g), torch.randn(64, 257, generator=g)
    ref, emu = R.floor_and_ref(torch.float32, fbm, top_db=1e30, re=re, im=im)
    floor = float((emu - ref).abs().max())
    bar = R.mel_db_bar(R.widest_band(fbm)) + 4 * floor
    assert floor <= bar and bar < 1e-4
    lo, hi = R.band_limits(fbm)
    m = int((hi - lo).argmax())
    cut = fbm.clone()
    cut[m, hi[m] - 1] = 0.0
    pert = R.mel_db_stage(re, im, cut, 1e-10)
    assert ((pert - ref).abs()[:, m] > bar).float().mean() > 0.9                     # (share of the frames that miss it)
    assert torch.equal(pert[:, :m], ref[:, :m])

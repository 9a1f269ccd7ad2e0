"""Plain restatement of the log-mel front-end (summarymixing_amd.lobes.features.Fbank) for the tests, stage by stage and without
torch.stft so that every stage can be judged on its own: frames -> dense DFT against an exact float64 cos / -sin basis -> power ->
mel -> dB -> per-utterance top_db clamp, plus the HTK-mel triangular filters.  Default float64: the yardstick of the GPU stage
tests, itself checked against oracle.smx_oracle.fbank (torch.stft) in tests/test_fbank_ref_cpu.py.  The same code in float32 is the
FLOOR emulation: what a plain float32 evaluation of the same stages costs (with the output rounded to bf16 where the kernel rounds).
Nothing here calls the code under test, and no bound below is derived from it."""
import functools
import math

import torch

U32 = 2.0 ** -24            # unit roundoff of float32
U16 = 2.0 ** -8             # unit roundoff of bfloat16 (8 significand bits: half an ulp is 2^-8 of the value at most)


def hamming(n, dtype=torch.float64):
    """torch.hamming_window(n) (periodic): 0.54 - 0.46 cos(2 pi j / n); w[0] = 0.08, w[j] = w[n - j]."""
    return torch.hamming_window(n, dtype=dtype)


def mel_filters(n_mels, n_fft, sample_rate=16000, f_min=0.0, f_max=None):
    """HTK-mel triangular filters (n_mels, n_fft // 2 + 1) in float64: mel = 2595 log10(1 + f / 700), n_mels + 2 points equally
    spaced in mel between f_min and f_max, filter m rising from point m to m + 1 and falling to m + 2 (slopes 1 / its left width)."""
    f_max = sample_rate / 2 if f_max is None else f_max
    to_mel = lambda hz: 2595.0 * math.log10(1.0 + hz / 700.0)
    mel = torch.linspace(to_mel(f_min), to_mel(f_max), n_mels + 2, dtype=torch.float64)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    centre, width = hz[1:-1], (hz[1:] - hz[:-1])[:-1]
    freqs = torch.linspace(0, sample_rate // 2, n_fft // 2 + 1, dtype=torch.float64)
    slope = (freqs[None, :] - centre[:, None]) / width[:, None]
    return torch.clamp(torch.minimum(slope + 1.0, 1.0 - slope), min=0.0)


def band_limits(fbm):
    """(lo, hi) per filter: first non-zero tap and one past the last; (n_bins, 0) for a filter without a tap."""
    nz = fbm != 0
    n_bins = fbm.shape[1]
    idx = torch.arange(n_bins)
    lo = torch.where(nz, idx, torch.full_like(idx, n_bins)).amin(1)
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).amax(1)
    return lo, hi


def widest_band(fbm):
    lo, hi = band_limits(fbm)
    return int((hi - lo).clamp(min=0).max())


def frames(wav, n_fft, hop):
    """wav (B, L) -> (B, T, n_fft), T = 1 + L // hop: centre-padded with n_fft / 2 zeros on both sides."""
    B, L = wav.shape
    pad = wav.new_zeros(B, n_fft // 2)
    fr = torch.cat([pad, wav, pad], 1).unfold(1, n_fft, hop)
    assert fr.shape[1] == 1 + L // hop
    return fr


@functools.lru_cache(maxsize=8)
def dft_basis(n_fft):
    """(cos, -sin) (n_bins, n_fft) in float64.  The angle is 2 pi (k j mod n) / n with the product reduced in integers, so the
    argument of cos / sin is exact to one rounding whatever k j is."""
    k = torch.arange(n_fft // 2 + 1, dtype=torch.int64)[:, None]
    j = torch.arange(n_fft, dtype=torch.int64)[None, :]
    ang = 2.0 * math.pi * ((k * j) % n_fft).double() / n_fft
    return torch.cos(ang), -torch.sin(ang)


def windowed_basis(n_fft, dtype=torch.float64):
    c, s = dft_basis(n_fft)
    w = hamming(n_fft)
    return (c * w).to(dtype), (s * w).to(dtype)


def spectrum(fr, window):
    """fr (..., n_fft), window (n_fft) -> (re, im) (..., n_bins) of the windowed frames: a dense DFT in fr's dtype (the basis is
    the float64 one rounded to it)."""
    n_fft = fr.shape[-1]
    c, s = dft_basis(n_fft)
    x = fr * window.to(fr.dtype)
    return x @ c.to(fr.dtype).t(), x @ s.to(fr.dtype).t()


def power(re, im):
    return re * re + im * im


def mel(p, fbm):
    return p @ fbm.to(p.dtype).t()


def db(m, amin):
    return 10.0 * torch.log10(torch.clamp(m, min=amin))


def clamp(d, top_db):
    """d (B, T, n_mels): per-utterance maximum - top_db."""
    return torch.maximum(d, d.amax(dim=(-2, -1), keepdim=True) - top_db)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def mel_db_stage(re, im, fbm, amin, dtype=torch.float64):
    """Unclamped dB from a given spectrum (the arithmetic of smx_mel_db with top_db = inf)."""
    return db(mel(power(re.to(dtype), im.to(dtype)), fbm), amin)


def pipeline(wav, n_fft, hop, fbm, amin=1e-10, top_db=80.0, dtype=torch.float64):
    """wav (B, L) -> dict of every stage in `dtype` (the waveform's float32 samples are the input of both precisions)."""
    fr = frames(wav.to(dtype), n_fft, hop)
    re, im = spectrum(fr, hamming(n_fft, dtype))
    d = db(mel(power(re, im), fbm), amin)
    return {"frames": fr, "re": re, "im": im, "db": d, "out": clamp(d, top_db)}


def floor_and_ref(out_dtype, fbm, amin=1e-10, top_db=80.0, wav=None, n_fft=None, hop=None, re=None, im=None):
    """(float64 reference, float32 floor emulation) of one case, both as float64 tensors: the whole pipeline from `wav`, or the
    mel / dB stage alone from a given (re, im) (top_db is then applied when the input is (B, T, n_bins)).  For out_dtype bfloat16
    the emulation's output is rounded to bf16 where the kernel rounds (after the clamp)."""
    outs = []
    for dt in (torch.float64, torch.float32):
        if wav is not None:
            o = pipeline(wav, n_fft, hop, fbm, amin, top_db, dt)["out"]
        else:
            o = mel_db_stage(re, im, fbm, amin, dt)
            if o.dim() == 3:
                o = clamp(o, top_db)
        outs.append(o)
    ref, emu = outs
    if out_dtype == torch.bfloat16:
        emu = bf16_round(emu)
    return ref, emu.double()


def spectrum_bar(fr, n_fft):
    """A-priori bound per frame (same for every bin, real or imaginary half) of ANY float32 evaluation of sum_j x_j w_j c_kj with
    |c| <= 1: each product carries the rounding of the windowed basis entry and of the multiplication (2 u), the n - 1 additions at
    most (n - 1) u in any order, the fold's x_j +- x_{n-j} one more: (n + 4) u sum_j |x_j| w_j covers all of it to first order.
    fr: the float64 frames (..., n_fft) -> (..., 1)."""
    return (n_fft + 4) * U32 * (fr.double().abs() * hamming(n_fft)).sum(-1, keepdim=True)


def mel_db_bar(w_max):
    """A-priori bound in dB of the mel sum in float32 from an exact spectrum: the terms re^2 + im^2 are non-negative (3 u each),
    times a weight (u), summed over at most w_max taps ((w_max - 1) u in any order): relative error <= (w_max + 4) u of the sum,
    and d(10 log10 s) = (10 / ln 10) ds / s.  (The logarithm itself is covered by the measured float32 floor, not by this.)"""
    return 10.0 / math.log(10.0) * (w_max + 4) * U32

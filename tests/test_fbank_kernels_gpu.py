"""The log-mel front-end's kernels stage by stage against the float64 restatement in tests/_fbank_ref.py (itself pinned to
torch.stft on the CPU by tests/test_fbank_ref_cpu.py), on every route Fbank.forward can take:

  (a) spectrum   smx_dft_frames (folded implicit GEMM, Nyquist row dropped or kept), the unfolded implicit GEMM (lda = hop) and
                 frame_window + GEMM: real and imaginary halves of `spec` against the float64 DFT of the same float32 samples;
  (b) mel / dB   smx_mel_db on a synthetic spectrum: bands wider than the 48-tap LDS image, filters without a tap, up to four
                 filters per lane, the grid-stride loop, B*T not a multiple of 4;
  (c) clamp      bit-exact against max(u, per-utterance max - top_db) of the kernel's own unclamped output, float32 and bf16;
  (d) the module end to end on each route of (a).

Every bar is an a-priori bound (written out in _fbank_ref.spectrum_bar / mel_db_bar), four times a float32 floor measured on the CPU
from the same inputs (_fbank_ref.floor_and_ref), or bit equality; none is taken from the kernels.  That the bars of (a) and (b)
catch a dropped fold end point / a lost band tap is shown on the CPU in tests/test_fbank_ref_cpu.py.  Measured errors and floors
go to tests._util.report (profiles/fbank_parity_errors.jsonl)."""
import functools
import math

import pytest
import torch

from tests import _fbank_ref as R
from tests._util import report

pytestmark = pytest.mark.gpu

GAINS = (1.0, 0.03, 0.001)                                  # per-utterance levels over three decades


def _fbank(n_fft, hop, n_mels=40, **kw):
    from summarymixing_amd.lobes.features import Fbank
    return Fbank(n_fft=n_fft, n_mels=n_mels, win_length=n_fft / 16.0, hop_length=hop / 16.0, **kw).cuda()


def _lengths(n_fft, hop):
    """T = 1 (L < hop) | L an exact multiple of hop | not one | L < n_fft / 2 | T = 131: two 128-row tiles, the second ragged."""
    return (hop - 7, 5 * hop, 7 * hop + 11, n_fft // 2 - 3, 130 * hop + 37)


@functools.lru_cache(maxsize=None)
def _wave(B, L, seed=0):
    """Broadband noise, per-utterance gains over three decades, the last utterance ending in exact zeros."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * L + B)
    wav = torch.randn(B, L, generator=g) * torch.tensor(GAINS)[:B, None]
    wav[B - 1, L // 2:] = 0.0
    return wav


@functools.lru_cache(maxsize=None)
def _spec_ref(n_fft, hop, B, L):
    """(re, im, bar, zero-frame mask) in float64 of one input: computed once, shared by every route, never modified."""
    fr = R.frames(_wave(B, L).double(), n_fft, hop)
    re, im = R.spectrum(fr, R.hamming(n_fft))
    return re, im, R.spectrum_bar(fr, n_fft), ~fr.bool().any(-1)


def _spec(fb, wav, route, fill=float("nan")):
    """The spectrum stage of Fbank.forward on one route, into a `spec` pre-filled with a sentinel."""
    from summarymixing_amd import _lib as L
    from summarymixing_amd import ops
    B, Lw = wav.shape
    T = 1 + Lw // fb.hop
    M = fb.basis.shape[0]
    spec = torch.full((B * T, M), fill, dtype=torch.float32, device="cuda")
    if route == "explicit":
        frames = ops.frame_window(wav.contiguous(), fb.window, T, fb.n_fft, fb.hop)
        ops.gemm(L.GEMM_NT, frames, fb.basis, spec, B * T, M, fb.n_fft)
        return spec, frames
    half = fb.n_fft // 2
    Lp = (Lw + fb.n_fft + 4 + 3) // 4 * 4
    wp = torch.zeros((B, Lp), dtype=torch.float32, device="cuda")
    wp[:, half:half + Lw] = wav
    if route == "folded":
        assert fb.fold
        ops.dft_frames(wp, fb.basis_cos, fb.basis_sin, spec, fb.im_off, B, T, fb.n_fft, fb.hop)
    else:
        ops.gemm(L.GEMM_NT, wp[0, :fb.n_fft].view(1, -1), fb.basis_w, spec[:T], T, M, fb.n_fft, batch=B, sa=Lp, sb=0, sc=T * M,
                 lda=fb.hop)
    return spec, None


SPEC_CASES = [(512, 160, "folded"), (400, 160, "folded"), (256, 80, "folded"), (2048, 160, "folded"),
              (512, 160, "unfolded"), (512, 162, "explicit"), (512, 160, "explicit"), (400, 160, "unfolded")]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_fft,hop,route", SPEC_CASES)
def test_spectrum_stage_matches_float64_dft(n_fft, hop, route, B):
    """Bar per frame, for every bin of both halves: (n_fft + 4) 2^-24 sum_j |x_j| w_j - the order-independent worst case of a
    float32 evaluation of that sum (basis rounding, products, n - 1 additions, the fold's extra addition); a frame wholly in zeros
    must therefore be exactly zero.  `spec` is pre-filled with NaN: every defined column must have been written (the Nyquist
    column is undefined when the route drops it, the padding columns n_bins .. im_off always), and on the dropped-Nyquist route
    nothing outside the n_fft / 2 computed columns of either half may have been.  All routes of one (n_fft, hop) meet the same bar
    against the same cached reference."""
    fb = _fbank(n_fft, hop)
    n_bins, half, im_off = n_fft // 2 + 1, n_fft // 2, fb.im_off
    dropped = route == "folded" and fb.drop_nyquist
    assert dropped == (route == "folded" and n_fft != 400)
    ncol = half if dropped else n_bins
    worst, saw_zero_frames = 0.0, False
    for Lw in _lengths(n_fft, hop):
        wav = _wave(B, Lw)
        re, im, bar, zero = _spec_ref(n_fft, hop, B, Lw)
        T = 1 + Lw // hop
        spec, frames = _spec(fb, wav.cuda(), route)
        torch.cuda.synchronize()
        spec = spec.cpu()
        assert spec.shape == (B * T, 2 * im_off)
        gre, gim = spec[:, :ncol].view(B, T, ncol).double(), spec[:, im_off:im_off + ncol].view(B, T, ncol).double()
        assert torch.isfinite(gre).all() and torch.isfinite(gim).all(), (Lw, "a defined column was not written")
        if dropped:
            assert torch.isnan(spec[:, half:im_off]).all() and torch.isnan(spec[:, im_off + half:]).all(), (Lw, "wrote past its columns")
        ere, eim = (gre - re[..., :ncol]).abs(), (gim - im[..., :ncol]).abs()
        assert (ere <= bar).all() and (eim <= bar).all(), (Lw, float((ere / bar.clamp(min=1e-300)).max()), float((eim / bar.clamp(min=1e-300)).max()))
        assert not gre[zero].any() and not gim[zero].any(), (Lw, "a frame of zeros is not exactly zero")
        saw_zero_frames |= bool(zero.any())
        live = ~zero
        worst = max(worst, float((torch.maximum(ere, eim) / bar.clamp(min=1e-300))[live].max()))
        if frames is not None:                                                    # frame_window_kernel itself: one rounding per sample
            want = R.frames(wav, n_fft, hop) * R.hamming(n_fft, torch.float32)
            assert torch.equal(frames.cpu().view(B, T, n_fft), want)
    assert saw_zero_frames
    report("fbank_spectrum", {"n_fft": n_fft, "hop": hop, "route": route, "B": B, "err_over_bar": worst})


# ---- (b) mel / dB ---------------------------------------------------------------------------------------------------------
def _hand_bank(width):
    """(5, 257): a 7-tap band | one band exactly `width` bins wide | no tap at all | 57 taps up to the last bin | a single tap at 0."""
    g = torch.Generator().manual_seed(width)
    fbm = torch.zeros(5, 257)
    for m, band in enumerate([(3, 10), (20, 20 + width), None, (200, 257), (0, 1)]):
        if band is not None:
            fbm[m, band[0]:band[1]] = torch.rand(band[1] - band[0], generator=g) * 0.9 + 0.1
    return fbm


@functools.lru_cache(maxsize=None)
def _bank(name):
    if isinstance(name, str):
        return _hand_bank(int(name[1:]))
    n_bins, n_mels = name
    return R.mel_filters(n_mels, 2 * (n_bins - 1)).float().contiguous()


@functools.lru_cache(maxsize=4)
def _synthetic_spec(N, n_bins, seed=0):
    """(N, 2 im_off) float32: re | im halves, rows scaled over five decades, every seventh row all zero."""
    g = torch.Generator().manual_seed(31 * N + n_bins + seed)
    im_off = (n_bins + 3) // 4 * 4
    spec = torch.randn(N, 2 * im_off, generator=g)
    spec *= 10.0 ** (torch.rand(N, 1, generator=g) * 5.0 - 3.0)
    spec[3::7] = 0.0
    return spec, im_off


BANKS = [(257, 80), (257, 20), (1025, 40), (201, 40), (129, 80), (257, 130), (257, 256), "w48", "w49"]
#  widest band:  16        56         125        25 (n_fft 400)  8, 2 empty  10, 3 per lane  6, 4 per lane     48 / 49 (+ a 57-tap band)
FRAMES = [(1, 1), (5, 1), (5, 1639)]                        # B*T = 1 | 5 | 4 * 2048 + 3: more frames than 2048 workgroups x 4 waves


@pytest.mark.parametrize("B,T", FRAMES)
@pytest.mark.parametrize("bank", BANKS, ids=lambda b: b if isinstance(b, str) else f"{b[0]}x{b[1]}")
def test_mel_db_matches_float64(bank, B, T):
    """smx_mel_db with top_db = 1e30 (the unclamped dB) on a synthetic spectrum.  Bar: (10 / ln 10) (w_max + 4) 2^-24, the a-priori
    bound of a float32 sum of at most w_max non-negative terms, plus four times the float32 floor of the same stage measured on
    the CPU (which stands in for log10f, whose accuracy the library does not state).  Cells at the amin clamp (zero rows, filters
    without a tap) equal 10 log10(amin) to within that floor."""
    from summarymixing_amd import ops
    fbm = _bank(bank)
    n_mels, n_bins = fbm.shape
    N = B * T
    spec, im_off = _synthetic_spec(N, n_bins)
    re, im = spec[:, :n_bins], spec[:, im_off:im_off + n_bins]
    amin = 1e-10
    ref, emu = R.floor_and_ref(torch.float32, fbm, amin=amin, top_db=1e30, re=re, im=im)
    floor = float((emu - ref).abs().max())
    w_max = R.widest_band(fbm)
    bar = R.mel_db_bar(w_max) + 4 * floor
    out = ops.mel_db(spec.cuda(), im_off, fbm.cuda(), B, T, amin, 1e30, torch.float32)
    torch.cuda.synchronize()
    out = out.cpu().view(N, n_mels).double()
    err = (out - ref).abs()
    at_amin = R.mel(R.power(re.double(), im.double()), fbm) <= amin
    report("fbank_mel_db", {"bank": str(bank), "B": B, "T": T, "w_max": w_max, "err": float(err.max()), "floor": floor, "bar": bar,
                            "err_at_amin": float(err[at_amin].max()) if at_amin.any() else 0.0, "cells_at_amin": int(at_amin.sum())})
    assert torch.isfinite(out).all()
    assert float(err.max()) <= bar, (float(err.max()), bar, floor)
    if N > 1 or bank in ((129, 80), "w48", "w49"):
        assert at_amin.any()
    assert (err[at_amin] <= floor).all(), (float(err[at_amin].max()), floor)


def test_mel_db_refuses_more_than_256_filters_before_any_launch():
    from summarymixing_amd import _lib as L
    from summarymixing_amd import ops
    B, T, n_mels, n_bins = 1, 3, 257, 257
    spec, im_off = _synthetic_spec(3, n_bins)
    fbm = torch.rand(n_mels, n_bins).cuda()
    with pytest.raises(RuntimeError, match="code -1"):                            # SMX_EINVAL
        ops.mel_db(spec.cuda(), im_off, fbm, B, T, 1e-10, 80.0, torch.float32)
    out = torch.full((B, T, n_mels), -7.0, device="cuda")
    ws = ops._workspace(L.lib().smx_fbank_workspace(B, T, n_mels), out.device, slot=5)
    s = spec.cuda()
    rc = L.lib().smx_mel_db(L.F32, ops._p(s), s.stride(0), im_off, ops._p(fbm), n_bins, n_mels, 1e-10, 80.0, ops._p(out), B, T, ops._p(ws),
                            ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == -7.0).all())


# ---- (c) clamp ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,n_mels", [(3, 7, 80), (2, 1, 20), (4, 6601, 80)])
def test_top_db_clamp_is_exact(B, T, n_mels):
    """u = the top_db = 1e30 output.  The top_db = 80 output is bit-equal to max(u, amax of u over that utterance - 80) formed in
    float32 on the host, the bf16 output to that rounded to bf16.  The utterances of one batch sit 50 dB apart and each holds
    zero frames (-100 dB): the loud ones clamp them, the quiet ones do not, so a per-batch or a per-frame maximum fails.
    (4, 6601, 80) is 4 x 66 s of audio: B T n_mels > 8192 x 256, the clamp kernel's grid-stride loop."""
    from summarymixing_amd import ops
    n_bins, im_off = 257, 260
    g = torch.Generator(device="cuda").manual_seed(B * T)
    spec = torch.randn(B * T, 2 * im_off, generator=g, device="cuda")
    spec *= 10.0 ** (torch.rand(B * T, 1, generator=g, device="cuda") * 2.0 - 2.0)
    spec.view(B, T, -1).mul_(torch.tensor([300.0, 1.0, 0.003, 30.0], device="cuda")[:B, None, None])
    if T > 1:
        spec.view(B, T, -1)[:, T // 2] = 0.0
    else:
        spec[1] = 0.0
    fbm = _bank((n_bins, n_mels)).cuda()
    u = ops.mel_db(spec, im_off, fbm, B, T, 1e-10, 1e30, torch.float32).cpu()
    v = ops.mel_db(spec, im_off, fbm, B, T, 1e-10, 80.0, torch.float32).cpu()
    vb = ops.mel_db(spec, im_off, fbm, B, T, 1e-10, 80.0, torch.bfloat16).cpu()
    assert B * T * n_mels > 8192 * 256 or T < 100
    umax = u.amax(dim=(1, 2), keepdim=True)
    want = torch.maximum(u, umax - 80.0)
    assert torch.equal(v, want)
    assert vb.dtype == torch.bfloat16 and torch.equal(vb, want.bfloat16())
    clamped = (want > u).flatten(1).any(1)
    if B >= 3:
        assert bool(clamped[0]) and not bool(clamped[2])                          # the clamp is live in the loud utterance only
        assert float(umax.max() - umax.min()) > 80.0
        assert not torch.equal(want, torch.maximum(u, u.amax() - 80.0))           # (a per-batch maximum would differ)


# ---- (d) the module, end to end, on every route ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _signal(kind, B, L):
    """Noise, or a 440 Hz sine in noise (never the pure sine: its empty channels hold cancellation residue, not signal); levels
    1 / 0.5 / 0.1, the last utterance ending in silence so that amin and the top_db clamp engage."""
    g = torch.Generator().manual_seed(L + len(kind))
    lev = torch.tensor([1.0, 0.5, 0.1])[:B, None]
    if kind == "noise":
        wav = torch.randn(B, L, generator=g) * lev
    else:
        wav = 0.3 * torch.sin(2 * math.pi * 440.0 * torch.arange(L) / 16000.0)[None] * lev + 0.01 * torch.randn(B, L, generator=g)
    wav[B - 1, L // 2:] = 0.0
    return wav


#          name              constructor arguments                                              knobs (folded, implicit)  route
MODULES = [("recipe",        dict(n_fft=512, n_mels=80, win_length=32),                          (True, True),   "folded"),
           ("class-default", dict(),                                                             (True, True),   "folded"),
           ("n256",          dict(n_fft=256, n_mels=80, win_length=16, hop_length=5),            (True, True),   "folded"),
           ("n2048",         dict(n_fft=2048, n_mels=40, win_length=128),                        (True, True),   "folded"),
           ("unfolded",      dict(n_fft=512, n_mels=80, win_length=32),                          (False, True),  "unfolded"),
           ("explicit",      dict(n_fft=512, n_mels=80, win_length=32),                          (True, False),  "explicit"),
           ("hop162",        dict(n_fft=512, n_mels=80, win_length=32, hop_length=10.125),       (True, True),   "explicit"),
           ("fmin-fmax",     dict(n_fft=512, n_mels=80, win_length=32, f_min=50.0, f_max=7600.0), (True, True),  "folded"),
           ("fmax-past-nyq", dict(n_fft=512, n_mels=80, win_length=32, f_max=8400.0),            (True, True),   "folded")]


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["noise", "sine+noise"])
@pytest.mark.parametrize("name,kw,knobs,route", MODULES, ids=[m[0] for m in MODULES])
def test_fbank_module_on_every_route(monkeypatch, name, kw, knobs, route, kind, out_dtype):
    """Fbank.forward against the float64 pipeline.  Bar per cell: four times the float32 floor of the whole pipeline (the largest
    error of the same stages run in float32 on the CPU from the same samples), but never above the 2e-2 dB of
    test_fbank_matches_cpu_spec.  The bf16 output may sit half a bf16 ulp further off (2^-8 of the value: its one rounding, after
    the clamp).  The route is the one named: the spectrum handed to smx_mel_db is bit-equal to the stage helper's on that route."""
    from summarymixing_amd import ops
    from summarymixing_amd.lobes import features
    monkeypatch.setattr(features, "_FOLDED_DFT", knobs[0])
    monkeypatch.setattr(features, "_IMPLICIT_FRAMES", knobs[1])
    fb = features.Fbank(**kw).cuda()
    B, Lw = 3, 8000 + 37
    wav = _signal(kind, B, Lw)
    seen = {}
    real = ops.mel_db

    def spy(spec, im_off, fbm, *a):
        seen["spec"], seen["fb"] = spec.clone(), fbm
        return real(spec, im_off, fbm, *a)
    monkeypatch.setattr(ops, "mel_db", spy)
    out = fb(wav.cuda(), out_dtype=out_dtype)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "mel_db", real)
    T = 1 + Lw // fb.hop
    assert out.shape == (B, T, fb.n_mels) and out.dtype == out_dtype
    # the route taken
    dropped = route == "folded" and fb.drop_nyquist
    assert dropped == (name in ("recipe", "n256", "n2048", "fmin-fmax"))
    assert seen["fb"] is (fb.fb_nn if dropped else fb.fb)
    want_spec, _ = _spec(fb, wav.cuda(), route, fill=0.0)
    ncol = fb.n_fft // 2 if dropped else fb.n_fft // 2 + 1
    for off in (0, fb.im_off):
        assert torch.equal(seen["spec"][:, off:off + ncol], want_spec[:, off:off + ncol])
    # the values
    fbm = R.mel_filters(fb.n_mels, fb.n_fft, 16000, kw.get("f_min", 0.0), kw.get("f_max")).float()
    ref, emu = R.floor_and_ref(out_dtype, fbm, wav=wav, n_fft=fb.n_fft, hop=fb.hop)
    ref32, emu32 = (ref, emu) if out_dtype == torch.float32 else R.floor_and_ref(torch.float32, fbm, wav=wav, n_fft=fb.n_fft, hop=fb.hop)
    floor = float((emu32 - ref32).abs().max())
    bar = min(4 * floor, 2e-2)
    err = (out.cpu().double() - ref).abs()
    allow = torch.full_like(ref, bar)
    if out_dtype == torch.bfloat16:
        allow = bar + R.U16 * (ref.abs() + bar)
    report("fbank_module", {"case": name, "route": route + ("-nyquist" if dropped else ""), "input": kind, "out": str(out_dtype)[6:],
                            "err": float(err.max()), "floor_f32": floor, "floor_out": float((emu - ref).abs().max()), "bar": bar,
                            "err_over_allow": float((err / allow).max())})
    assert floor > 0 and (err <= allow).all(), (float(err.max()), bar, floor)
    assert abs(float(ref[B - 1].max() - ref[B - 1].min()) - 80.0) < 1e-9                    # (the clamp is live: the last utterance ends in silence)

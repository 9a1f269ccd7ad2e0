"""summarymixing_amd.augment without a GPU: the cases the GPU tests run are admissible (the gather-form reference equals the
literal upstream chain on them), the class surface accepts the recipes' constructor calls and refuses what is not built, and the
library's block-size helper and refusal codes."""
import ctypes

import pytest
import torch

import summarymixing_amd.augment  # noqa: F401  (the package under test: without it nothing in this file runs)
from tests import _augment_ref as R

_BASE = 1 << 40          # fake, 4 KiB-aligned device pointers: every call below is refused on the host before any launch
_EINVAL, _EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("shape", list(R.CASES), ids=[str(s) for s in R.CASES])
def test_cases_are_admissible(shape):
    """For every block of every GPU case: gather form == masked_fill + two F.interpolate calls (float64, 1e-11 absolute), the
    dropped sets equal upstream's boolean expression, the warp parameters are ones the module can draw, and the masks do what the
    case list promises (row 0, row T - 1, an overlap, a straddle of c, a clip at F)."""
    B, T, F = shape
    worst = 0.0
    for label, blk, x, ref, _, zero in R.case_refs(shape):
        flags, c, w, td, fd = R.parse_block(blk, B, R.N_TIME_CAP, R.N_FREQ_CAP)
        assert R.WINDOW <= c < T - R.WINDOW and c - R.WINDOW + 1 <= w <= c + R.WINDOW and 1 <= w <= T - 1, label
        for drops, D in ((td, T), (fd, F)):
            assert torch.equal(R.dropped(drops, B, D), R.upstream_mask(drops, B, D)), label
        worst = max(worst, float((ref - R.chain_ref(x, blk, R.N_TIME_CAP, R.N_FREQ_CAP)).abs().max()))
        assert bool((ref[zero] == 0).all()), label
        if flags & R.TIME:
            tm = R.dropped(td, B, T)
            assert tm[:, 0].all() and tm[:, T - 1].all() and tm[:, c - 1].all() and tm[:, c].all() and not tm.all(dim=1).any(), label
            assert all(any(p + q > T for p, q in row) for row in td), label
        if flags & R.FREQ:
            assert all(any(p + q > F for p, q in row) for row in fd) and not R.dropped(fd, B, F).all(dim=1).any(), label
    assert worst <= 1e-11, f"{shape}: gather form vs literal chain {worst:.3e}"
    ws = {R.parse_block(b, B, R.N_TIME_CAP, R.N_FREQ_CAP)[2] for _, b in R.case_blocks(shape)}
    assert 1 in ws and T - 1 in ws                           # n_out = 1 on either side


def test_emulation_is_close_to_the_reference_and_not_equal():
    """The float32 emulation - the bar of the GPU test - sits a few float32 ulp from float64: not zero, not large."""
    for shape in R.CASES:
        floor = max(float((emu.double() - ref).abs().max()) for _, _, _, ref, emu, _ in R.case_refs(shape))
        assert 0.0 < floor < 2e-5, (shape, floor)


def test_recipe_constructor_calls_succeed():
    """The four `!new:` lines of the recipes (…/hparams/conformer_summarymixing_transducer.yaml:195-245) with their arguments."""
    from summarymixing_amd.augment.augmenter import Augmenter
    from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping
    time_drop = SpectrogramDrop(drop_length_low=15, drop_length_high=25, drop_count_low=5, drop_count_high=5, replace="zeros", dim=1)
    freq_drop = SpectrogramDrop(drop_length_low=25, drop_length_high=35, drop_count_low=2, drop_count_high=2, replace="zeros", dim=2)
    time_warp = Warping()
    aug = Augmenter(parallel_augment=False, concat_original=False, repeat_augment=1, shuffle_augmentations=False,
                    min_augmentations=3, max_augmentations=3, augment_prob=1.0, augmentations=[time_drop, freq_drop, time_warp])
    assert aug.fused and len(aug.augmentations) == 3
    assert Augmenter(augmentations=[freq_drop, time_warp]).fused and Augmenter(augmentations=[time_warp]).fused
    assert not Augmenter(augmentations=[time_warp, time_drop]).fused and not Augmenter(augmentations=[time_drop, time_drop]).fused
    labels = torch.arange(6).view(2, 3)
    assert aug.replicate_labels(labels) is labels
    a, b = aug.replicate_multiple_labels(labels, labels[:, 0])
    assert a is labels and torch.equal(b, labels[:, 0])
    import summarymixing_amd.augment as pkg
    assert pkg.freq_domain.SpectrogramDrop is SpectrogramDrop and pkg.augmenter.Augmenter is Augmenter


_UNBUILT = [("parallel_augment", True), ("concat_original", True), ("min_augmentations", 1), ("max_augmentations", 2),
            ("shuffle_augmentations", True), ("repeat_augment", 2), ("augment_start_index", 1), ("augment_end_index", 4),
            ("concat_start_index", 1), ("concat_end_index", 4), ("augment_prob", 0.5), ("enable_augmentations", [True, False, True])]


@pytest.mark.parametrize("name,value", _UNBUILT, ids=[n for n, _ in _UNBUILT])
def test_augmenter_refuses_unbuilt_options_by_name(name, value):
    from summarymixing_amd.augment.augmenter import Augmenter
    from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping
    mods = [SpectrogramDrop(dim=1), SpectrogramDrop(dim=2), Warping()]
    with pytest.raises(NotImplementedError, match=name):
        Augmenter(augmentations=mods, **{name: value})


def test_stages_refuse_unbuilt_options():
    from summarymixing_amd.augment.augmenter import Augmenter
    from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping
    for kw in (dict(replace="mean"), dict(replace="rand"), dict(dim=3), dict(dim=0), dict(drop_count_high=33)):
        with pytest.raises(NotImplementedError):
            SpectrogramDrop(**kw)
    for kw in (dict(warp_mode="bilinear"), dict(dim=2)):
        with pytest.raises(NotImplementedError):
            Warping(**kw)
    with pytest.raises(NotImplementedError, match="augmentations"):
        Augmenter(augmentations=[torch.nn.Identity()])


def test_cpu_tensors_raise():
    from summarymixing_amd import functional as SF
    from summarymixing_amd.augment.augmenter import Augmenter
    from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping
    x = torch.randn(2, 40, 80)
    for m in (SpectrogramDrop(dim=1), SpectrogramDrop(dim=2), Warping()):
        with pytest.raises(RuntimeError, match="GPU only"):
            m(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        Augmenter(augmentations=[SpectrogramDrop(), Warping()])(x, torch.ones(2))
    blk = SF.SpecAugBlock(R.make_block(2, 0, 0, 0, 0, [[], []], 0, 0, [[], []], 0), 0, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        SF.spec_augment(x, blk)


def test_block_size_helper():
    from summarymixing_amd import _lib, ops
    L = _lib.lib()
    assert L.smx_specaug_params_bytes(1, 0, 0) == 32
    assert L.smx_specaug_params_bytes(128, 5, 2) == 4 * (8 + 2 * 128 * 7)
    assert L.smx_specaug_params_bytes(3, 32, 32) == 4 * (8 + 2 * 3 * 64)
    for bad in ((0, 1, 1), (-1, 1, 1), (2, 33, 0), (2, 0, 33), (2, -1, 0)):
        assert L.smx_specaug_params_bytes(*bad) == 0, bad
    assert ops.specaug_params_words(2, R.N_TIME_CAP, R.N_FREQ_CAP) == R.case_blocks((2, 12, 80))[0][1].numel()
    with pytest.raises(ValueError):
        ops.specaug_params_words(2, 40, 0)


def _apply(**kw):
    a = dict(dtype=0, X=_BASE, ldx=80, Y=_BASE + 0x100000, ldy=80, params=_BASE + 0x200000, B=2, T=40, F=80, ntc=5, nfc=2)
    a.update(kw)
    return [a[k] for k in ("dtype", "X", "ldx", "Y", "ldy", "params", "B", "T", "F", "ntc", "nfc")] + [None]


_APPLY_REFUSED = [("no X", dict(X=None), _EINVAL), ("no Y", dict(Y=None), _EINVAL), ("no block", dict(params=None), _EINVAL),
                  ("B = 0", dict(B=0), _EINVAL), ("T = 0", dict(T=0), _EINVAL), ("F = -1", dict(F=-1), _EINVAL),
                  ("unknown dtype", dict(dtype=3), _EINVAL), ("ldx < F", dict(ldx=79), _EINVAL),
                  ("F = 1025", dict(F=1025, ldx=1025, ldy=1025), _EUNSUPPORTED), ("time cap 33", dict(ntc=33), _EUNSUPPORTED),
                  ("frequency cap 33", dict(nfc=33), _EUNSUPPORTED), ("in place", dict(Y=_BASE), _EUNSUPPORTED)]


@pytest.mark.parametrize("case,kw,code", _APPLY_REFUSED, ids=[c[0] for c in _APPLY_REFUSED])
def test_apply_refuses_what_it_cannot_run(case, kw, code):
    from summarymixing_amd import _lib
    L = _lib.lib()
    assert L.smx_specaug_apply(*_apply(**kw)) == code, case
    assert b"smx_specaug_apply" in L.smx_last_error()


def _draw(**kw):
    a = dict(params=_BASE, B=2, T=40, F=80, stages=7, t=(15, 25, 5, 5), f=(25, 35, 2, 2), window=5)
    a.update(kw)
    return [a["params"], a["B"], a["T"], a["F"], a["stages"], *a["t"], *a["f"], a["window"], 1234, None, None]


_DRAW_REFUSED = [("no block", dict(params=None), _EINVAL), ("B = 0", dict(B=0), _EINVAL), ("T = 0", dict(T=0), _EINVAL),
                 ("unknown stage", dict(stages=8), _EINVAL), ("empty length range", dict(t=(15, 15, 5, 5)), _EINVAL),
                 ("count range reversed", dict(f=(25, 35, 3, 2)), _EINVAL), ("window 0", dict(window=0), _EINVAL),
                 ("33 time drops", dict(t=(15, 25, 5, 33)), _EUNSUPPORTED), ("33 frequency drops", dict(f=(25, 35, 2, 33)), _EUNSUPPORTED)]


@pytest.mark.parametrize("case,kw,code", _DRAW_REFUSED, ids=[c[0] for c in _DRAW_REFUSED])
def test_draw_refuses_what_it_cannot_run(case, kw, code):
    from summarymixing_amd import _lib
    L = _lib.lib()
    assert L.smx_specaug_draw(*_draw(**kw)) == code, case
    assert b"smx_specaug_draw" in L.smx_last_error()


def test_draw_restatement_stays_in_range():
    """The Python statement of the draw (the GPU test checks the kernel against it): ranges, the header, determinism."""
    t, f = (15, 25, 5, 5), (25, 35, 2, 2)
    a = R.draw_block(4, 400, 80, 7, t, f, 5, 99, counter=3)
    assert a == R.draw_block(4, 400, 80, 7, t, f, 5, 99, counter=3) and a != R.draw_block(4, 400, 80, 7, t, f, 5, 99, counter=4)
    assert len(a) == 8 + 2 * 4 * 7 and a[0] == 7 and a[3] == 5 and a[4] == 2 and a[5:8] == [0, 0, 0]
    assert 5 <= a[1] < 395 and a[1] - 4 <= a[2] <= a[1] + 5
    tp, fp = a[8:8 + 40], a[48:]
    assert all(0 <= p < 400 for p in tp[0::2]) and all(15 <= q < 25 for q in tp[1::2])
    assert all(0 <= p < 80 for p in fp[0::2]) and all(25 <= q < 35 for q in fp[1::2])
    assert R.draw_block(2, 10, 80, 7, t, f, 5, 1)[:3] == [6, 0, 0]      # T - window <= window: the warp bit stays clear

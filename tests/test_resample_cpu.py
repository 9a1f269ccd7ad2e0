"""summarymixing_amd.augment.time_domain without a GPU: the cases the GPU tests run are admissible (the gather-form reference equals
the literal upstream chain on them), smx_resample_plan against the Python statement of the plan, its refusals and smx_resample's,
SpeedPerturb's draw and state, and what the Augmenter accepts and refuses around a waveform stage."""
import ctypes

import pytest
import torch

import summarymixing_amd.augment.time_domain  # noqa: F401  (the module under test: without it nothing in this file runs)
from tests import _resample_ref as R

_BASE = 1 << 40          # fake, 4 KiB-aligned device pointers: every call below is refused on the host before any launch
_EINVAL, _EUNSUPPORTED = -1, -2
PLAN_RATIOS = [(20, 19), (20, 21), (10, 9), (100, 97), (2, 1), (441, 160), (160, 441), (1, 2), (100, 101)]
# the issue's table: ratio -> (width, K, fewest and most nonzero taps of a phase)
TABLE = {(20, 19): (7, 34, 12, 13), (20, 21): (7, 34, 12, 13), (10, 9): (None, None, 13, 14), (100, 97): (None, None, 12, 13),
         (2, 1): (13, None, 25, 25), (441, 160): (17, 475, 33, 34), (160, 441): (None, None, 12, 13)}


@pytest.mark.parametrize("ratio", R.RATIOS, ids=[f"{a}to{b}" for a, b in R.RATIOS])
def test_cases_are_admissible(ratio):
    """Every GPU case of the ratio: gather form == F.pad + strided F.conv1d + transpose + reshape + slice (float64, 1e-12), the
    output length is ceil(n L / o), S bounds |y|, and the lengths sit where the case list says (edges, block and tile seams)."""
    plan = R.plan_ref(*ratio)
    span = R.tile_blocks(plan) * plan.o
    Ls = [L for a, b, L in R.CASES if (a, b) == ratio]
    assert {1, 5, plan.o, 3 * plan.o - 1, 3 * plan.o, 3 * plan.o + 1, span + 37, 2 * span - 1} <= set(Ls) and 5 < plan.width
    for L in Ls:
        x, y, S = R.case_ref(*ratio, L)
        want = -(-plan.n * L // plan.o)
        assert y.shape == (R.B_MAX, want) == S.shape and want == R.out_len(plan.o, plan.n, L)
        assert (want - 1) * plan.o < plan.n * L <= want * plan.o
        worst = float((y - R.conv_ref(x, plan)).abs().max())
        assert worst <= 1e-12, f"{ratio} L = {L}: gather form vs literal chain {worst:.3e}"
        assert bool((y.abs() <= S * (1 + 1e-12)).all()) and float(S.min()) > 0.0


def test_the_extra_case_makes_a_workgroup_take_a_second_tile():
    """441 -> 160 at nine spans + 1: more tiles than the launch has workgroups along the row (csrc/resample.hip sizes the grid for
    3968 input samples per workgroup)."""
    plan = R.plan_ref(441, 160)
    span = R.tile_blocks(plan) * plan.o
    L = 9 * span + 1
    assert (441, 160, L) in R.CASES
    tiles = -(-(-(-R.out_len(plan.o, plan.n, L) // plan.n)) // R.tile_blocks(plan))
    assert tiles == 10 and -(-L // 3968) == 9


@pytest.mark.parametrize("ratio", PLAN_RATIOS, ids=[f"{a}to{b}" for a, b in PLAN_RATIOS])
def test_plan_matches_its_python_statement(ratio):
    from summarymixing_amd import ops
    ref = R.plan_ref(*ratio)
    got = ops.resample_plan(*ratio)
    assert (got.o, got.n, got.width, got.K, got.taps) == (ref.o, ref.n, ref.width, ref.K, ref.taps)
    assert got.tile_blocks == R.tile_blocks(ref) >= 1
    assert got.image[:8].tolist() == [ref.o, ref.n, ref.width, ref.K, ref.taps, got.tile_blocks, 0, 0]
    assert got.image.numel() == 8 + ref.n * (1 + ref.taps)
    assert got.first().tolist() == ref.first
    assert R.runs_are_contiguous(ref.h)
    w = got.weights()
    lens = []
    for p in range(ref.n):
        f = ref.first[p]
        run = int(torch.nonzero(ref.h[p]).flatten()[-1]) - f + 1
        lens.append(run)
        want = ref.h[p, f:f + run]
        # within one float32 ulp of the torch evaluation (libm against torch's sin / cos), and nonzero where it is
        ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126)) * 2.0 ** -23
        assert bool(((w[p, :run].double() - want.double()).abs() <= ulp.double()).all()), (ratio, p)
        assert bool((w[p, :run] != 0).all()) and bool((w[p, run:] == 0).all()), (ratio, p)
        assert f + run <= ref.K
    assert max(lens) == ref.taps
    if ratio in TABLE:
        width, K, lo, hi = TABLE[ratio]
        assert width in (None, ref.width) and K in (None, ref.K) and (min(lens), max(lens)) == (lo, hi)
    sums = ref.h.double().sum(dim=1)
    assert 1.00003 <= float(sums.min()) and float(sums.max()) <= 1.0009


def test_plan_table_sizes():
    from summarymixing_amd import ops
    a, b = ops.resample_plan(441, 160), ops.resample_plan(160, 441)
    assert a.n * a.taps == 5440 and b.n * b.taps == 5733
    assert ops.resample_plan(16000, 15200)[:5] == ops.resample_plan(20, 19)[:5]            # the recipe's speed 95
    assert ops.resample_plan(16000, 16800)[:5] == ops.resample_plan(20, 21)[:5]            # and 105


def test_plan_refusals():
    from summarymixing_amd import _lib, ops
    L = _lib.lib()
    info = (ctypes.c_int32 * 8)()
    nbytes = ctypes.c_size_t(7)
    for bad in ((16000, 15999), (700, 699), (0, 16000), (16000, 0), (-16000, 16000), (16000, -1), (4000, 1)):
        assert L.smx_resample_plan(bad[0], bad[1], info, ctypes.byref(nbytes), None, 0) == _EUNSUPPORTED, bad
        assert b"smx_resample_plan" in L.smx_last_error() and nbytes.value == 0
        with pytest.raises(NotImplementedError, match="smx_resample_plan"):
            ops.resample_plan(*bad)
    assert L.smx_resample_plan(700, 699, info, None, None, 0) == _EUNSUPPORTED      # 699 phases x 13 taps = 9087 floats
    assert b"699 * 13 > 8192" in L.smx_last_error() and list(info[:5]) == [700, 699, 7, 714, 13]
    assert L.smx_resample_plan(20, 19, None, None, None, 0) == _EINVAL
    assert L.smx_resample_plan(20, 19, info, ctypes.byref(nbytes), None, 0) == 0 and nbytes.value == 4 * (8 + 19 * 14)
    buf = (ctypes.c_int32 * (nbytes.value // 4))()
    assert L.smx_resample_plan(20, 19, info, None, buf, nbytes.value - 4) == _EINVAL
    assert L.smx_resample_plan(20, 19, info, None, buf, nbytes.value) == 0 and list(buf[:6]) == [20, 19, 7, 34, 13, 202]


def _resample(**kw):
    a = dict(X=_BASE, ldx=4000, Y=_BASE + 0x100000, ldy=4000, plan=_BASE + 0x200000, B=2, L=4000)
    a.update(kw)
    return [a[k] for k in ("X", "ldx", "Y", "ldy", "plan", "B", "L")] + [None]


_REFUSED = [("no X", dict(X=None), _EINVAL), ("no Y", dict(Y=None), _EINVAL), ("no plan", dict(plan=None), _EINVAL),
            ("B = 0", dict(B=0), _EINVAL), ("L = 0", dict(L=0), _EINVAL), ("L = -3", dict(L=-3), _EINVAL),
            ("ldx < L", dict(ldx=3999), _EINVAL), ("ldy = 0", dict(ldy=0), _EINVAL),
            ("in place", dict(Y=_BASE), _EUNSUPPORTED), ("B = 65536", dict(B=65536), _EUNSUPPORTED)]


@pytest.mark.parametrize("case,kw,code", _REFUSED, ids=[c[0] for c in _REFUSED])
def test_resample_refuses_what_it_cannot_run(case, kw, code):
    from summarymixing_amd import _lib
    L = _lib.lib()
    assert L.smx_resample(*_resample(**kw)) == code, case
    assert b"smx_resample" in L.smx_last_error()


def test_speed_perturb_draws_as_upstream_and_holds_no_state():
    from summarymixing_amd.augment.time_domain import Resample, SpeedPerturb
    sp = SpeedPerturb(orig_freq=16000, speeds=[95, 100, 105])                      # …transducer.yaml:177-179
    assert [(r.orig_freq, r.new_freq) for r in sp.resamplers] == [(16000, 15200), (16000, 16000), (16000, 16800)]
    assert len(sp.state_dict()) == 0 and len(list(sp.parameters())) == 0 and len(list(sp.children())) == 0
    assert len(Resample(16000, 15200).state_dict()) == 0
    torch.manual_seed(1234)
    want = [int(torch.randint(3, (1,))[0]) for _ in range(50)]
    torch.manual_seed(1234)
    got = [sp.draw() for _ in range(50)]
    assert all(torch.is_tensor(d) and d.dim() == 0 and d.device.type == "cpu" and d.dtype == torch.int64 for d in got)
    assert [int(d) for d in got] == want and set(want) == {0, 1, 2}
    # forward draws once per call, through draw(): with speed 100 drawn the very input comes back (a CPU tensor too: no launch)
    calls = []
    sp.draw = lambda: (calls.append(1), torch.tensor(1))[1]
    x = torch.randn(2, 100)
    assert sp(x) is x and len(calls) == 1 and int(sp.samp_index) == 1
    sp.draw = lambda: torch.tensor(0)
    with pytest.raises(RuntimeError, match="GPU only"):
        sp(x)
    assert SpeedPerturb(16000).speeds == [90, 100, 110]
    assert [r.new_freq for r in SpeedPerturb(16000).resamplers] == [14400, 16000, 17600]


def test_resample_module_surface():
    from summarymixing_amd import functional as SF
    from summarymixing_amd.augment.time_domain import Resample
    import summarymixing_amd.augment as pkg
    assert pkg.time_domain.Resample is Resample
    r = Resample()
    x = torch.randn(2, 50)
    assert (r.orig_freq, r.new_freq) == (16000, 16000) and r(x) is x
    for kw in (dict(lowpass_filter_width=8), dict(rolloff=0.9), dict(resampling_method="sinc_interp_kaiser"), dict(beta=14.0)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            Resample(16000, 8000, **kw)
    with pytest.raises(NotImplementedError, match="positional"):
        Resample(16000, 8000, "sinc_interp_kaiser")
    with pytest.raises(NotImplementedError, match="15999"):
        Resample(16000, 15999)
    with pytest.raises(RuntimeError, match="GPU only"):
        Resample(16000, 15200)(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        SF.resample(x, 16000, 15200)
    assert SF.resample(x, 8000, 8000) is x
    with pytest.raises(ValueError):
        SF.resample(x[0], 16000, 15200)
    plan, image = SF.resample_plan(16000, 15200)
    assert image is None and SF.resample_plan(16000, 15200)[0] is plan and plan.out_len(240000) == 228000


def test_augmenter_takes_the_recipes_wav_augment_and_refuses_the_rest():
    """…transducer.yaml:181-192 verbatim, then the lists that are not built."""
    from summarymixing_amd.augment.augmenter import Augmenter
    from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping
    from summarymixing_amd.augment.time_domain import Resample, SpeedPerturb
    speed_perturb = SpeedPerturb(orig_freq=16000, speeds=[95, 100, 105])
    wav_augment = Augmenter(parallel_augment=False, concat_original=False, repeat_augment=1, shuffle_augmentations=False,
                            min_augmentations=1, max_augmentations=1, augment_prob=1.0, augmentations=[speed_perturb])
    assert wav_augment.waveform and not wav_augment.fused and len(wav_augment.state_dict()) == 0
    speed_perturb.draw = lambda: torch.tensor(1)
    x, lens = torch.randn(2, 100), torch.tensor([1.0, 0.5])
    y, out_lens = wav_augment(x, lens)                          # speed 100: the batch itself, on any device
    assert y is x and out_lens is lens
    assert wav_augment.replicate_labels(lens) is lens
    assert Augmenter(augmentations=[Resample(16000, 8000)]).waveform
    for mixed in ([speed_perturb, SpectrogramDrop(dim=1)], [Warping(), speed_perturb], [speed_perturb, torch.nn.Identity()]):
        with pytest.raises(NotImplementedError, match="augmentations.*mixes waveform"):
            Augmenter(augmentations=mixed)
    second = SpeedPerturb(orig_freq=16000, speeds=[90, 110])
    with pytest.raises(NotImplementedError, match="augmentations.*2 waveform stages"):
        Augmenter(augmentations=[speed_perturb, second])
    with pytest.raises(NotImplementedError, match="min_augmentations"):
        Augmenter(min_augmentations=1, max_augmentations=1, augmentations=[speed_perturb, second])
    with pytest.raises(NotImplementedError, match="concat_original"):
        Augmenter(concat_original=True, augmentations=[speed_perturb])
    fea = Augmenter(augmentations=[SpectrogramDrop(dim=1), Warping()])                       # the fea_augment path is what it was
    assert fea.fused and not fea.waveform

"""summarymixing_amd.augment on the GPU: smx_specaug_apply against the float64 gather-form reference on explicit parameter blocks
(tests/_augment_ref.py; the CPU suite checks that reference against the literal upstream chain on the same cases), the bit-exact
properties of the copy paths, smx_specaug_draw's ranges and determinism, the modules against the functional form, and hipGraph
replay.  Bars: float32 - 8 x the float32 emulation's own deviation from float64 on the case (the 8 covers -ffast-math
reassociating the four-term sum and the two cubics by a few ulp each); bfloat16 - that plus 2^-8 |ref| (one rounding)."""
import pytest
import torch

import summarymixing_amd.augment  # noqa: F401  (the package under test: without it nothing in this file runs)
from tests import _augment_ref as R
from tests._util import report

pytestmark = pytest.mark.gpu

TIME_DROP, FREQ_DROP = (15, 25, 5, 5), (25, 35, 2, 2)        # the recipes' (len_lo, len_hi, cnt_lo, cnt_hi)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _block(blk, ntc=R.N_TIME_CAP, nfc=R.N_FREQ_CAP):
    from summarymixing_amd import functional as SF
    return SF.SpecAugBlock(blk.cuda(), ntc, nfc)


def _recipe_modules():
    from summarymixing_amd.augment.freq_domain import SpectrogramDrop, Warping
    return [SpectrogramDrop(drop_length_low=15, drop_length_high=25, drop_count_low=5, drop_count_high=5, replace="zeros", dim=1),
            SpectrogramDrop(drop_length_low=25, drop_length_high=35, drop_count_low=2, drop_count_high=2, replace="zeros", dim=2),
            Warping()]


# ---- 1. apply against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", list(R.CASES), ids=[str(s) for s in R.CASES])
def test_apply_matches_the_float64_reference(shape, dtype):
    from summarymixing_amd import functional as SF
    bf16 = dtype == torch.bfloat16
    refs = R.case_refs(shape, bf16)
    floor = max(float((emu.double() - ref).abs().max()) for _, _, _, ref, emu, _ in refs)
    assert floor > 0.0
    xg = refs[0][2].to(dtype).cuda()
    worst, worst_excess, where = 0.0, -1.0, None
    for label, blk, _, ref, _, zero in refs:
        y = SF.spec_augment(xg, _block(blk))
        assert y.dtype == dtype and y.shape == xg.shape and y.data_ptr() != xg.data_ptr()
        yc = y.cpu()
        assert bool((_bits(yc)[zero] == 0).all()), f"{shape} {label}: a dropped element is not +0"
        err = (yc.double() - ref).abs()
        bar = 8.0 * floor + (ref.abs() * 2.0 ** -8 if bf16 else 0.0)
        excess = float((err - bar).max())
        worst = max(worst, float(err.max()))
        if excess > worst_excess:
            worst_excess, where = excess, label
    report("specaug_apply", {"shape": list(shape), "dtype": str(dtype), "blocks": len(refs), "max_abs_err": worst,
                             "emulation_floor": floor, "bar_fp32_part": 8.0 * floor, "worst_err_minus_bar": worst_excess})
    print(f"specaug_apply {shape} {dtype}: max |err| {worst:.3e}, emulation floor {floor:.3e}, bar {8 * floor:.3e}"
          f"{' + 2^-8 |ref|' if bf16 else ''}, worst err - bar {worst_excess:.3e} at {where}")
    assert worst_excess <= 0.0, f"{shape} {where}: error exceeds the bar by {worst_excess:.3e}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_apply_on_a_grid_that_takes_the_doubled_tile(dtype):
    """From 2048 workgroups up the launch doubles its tile (128 rows at this width): same reference, same bar, one block."""
    from summarymixing_amd import functional as SF
    shape = (64, 4096, 8)
    B, T, F = shape
    bf16 = dtype == torch.bfloat16
    x = R.case_input(shape).to(dtype)
    c, w = 2047, 2051                                        # both segments fractional, the seam inside a tile
    td = [[(0, 2), (T - 2, 5), (c - 2 - (b % 2), 4), (c - 1, 3), (127 + b, 3)] for b in range(B)]
    fd = [[(F - 3, 6), (b % 3, 2)] for b in range(B)]
    blk = R.make_block(B, 7, c, w, 5, td, R.N_TIME_CAP, 2, fd, R.N_FREQ_CAP)
    ref = R.gather_ref(x, blk, R.N_TIME_CAP, R.N_FREQ_CAP)
    floor = float((R.gather_ref(x, blk, R.N_TIME_CAP, R.N_FREQ_CAP, torch.float32).double() - ref).abs().max())
    y = SF.spec_augment(x.cuda(), _block(blk)).cpu()
    assert bool((_bits(y)[R.must_be_zero(shape, blk, R.N_TIME_CAP, R.N_FREQ_CAP)] == 0).all())
    err = (y.double() - ref).abs()
    excess = float((err - (8.0 * floor + (ref.abs() * 2.0 ** -8 if bf16 else 0.0))).max())
    report("specaug_apply", {"shape": list(shape), "dtype": str(dtype), "blocks": 1, "max_abs_err": float(err.max()),
                             "emulation_floor": floor, "bar_fp32_part": 8.0 * floor, "worst_err_minus_bar": excess})
    assert floor > 0.0 and excess <= 0.0, f"error exceeds the bar by {excess:.3e}"


# ---- 2. drops only: a bit-exact copy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 11, 5), (2, 37, 80), (2, 130, 7)], ids=str)
def test_drops_alone_copy_every_other_element_bit_for_bit(shape, dtype):
    from summarymixing_amd import functional as SF
    B, T, F = shape
    x = R.case_input(shape).to(dtype)
    x[0, 2, 0] = -0.0                                        # a sign bit that an arithmetic path (0 + 1 * x) would lose
    td, fd = R._drops(B, T, F, T // 2)
    for flags in (R.TIME | R.FREQ, R.TIME, R.FREQ, 0):
        blk = R.make_block(B, flags, T // 2, T // 2 + 2, 4, td, R.N_TIME_CAP, 2, fd, R.N_FREQ_CAP)   # (c, w) set, warp bit clear
        y = SF.spec_augment(x.cuda(), _block(blk)).cpu()
        gone = R.must_be_zero(shape, blk, R.N_TIME_CAP, R.N_FREQ_CAP)
        assert gone.any() == bool(flags) and not gone.all()
        assert torch.equal(_bits(y)[~gone], _bits(x)[~gone]), f"flags {flags}: an undropped element changed"
        assert bool((_bits(y)[gone] == 0).all()), f"flags {flags}: a dropped element is not +0"


# ---- 3. identity warps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_identity_warp_is_bit_exact(dtype):
    from summarymixing_amd import functional as SF
    from summarymixing_amd.augment.freq_domain import Warping
    shape = (2, 37, 80)
    x = R.case_input(shape).to(dtype).cuda()
    none = [[] for _ in range(2)]
    for c in (5, 18, 31):                                    # c == w: every position falls on a source row
        y = SF.spec_augment(x, _block(R.make_block(2, R.WARP, c, c, 0, none, 0, 0, none, 0), 0, 0))
        assert torch.equal(_bits(y), _bits(x)), f"c = w = {c}"
    short = R.case_input((3, 10, 80)).to(dtype).cuda()      # T - window <= window: the module passes its input through
    m = Warping(warp_window=5)
    out = m(short)
    assert int(m.last_params.data[0]) == 0 and out.data_ptr() != short.data_ptr()
    assert torch.equal(_bits(out), _bits(short))


# ---- 4. leading dimensions and the scalar path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_strided_and_unaligned_views_give_the_same_values(dtype):
    from summarymixing_amd import ops
    shape = (2, 37, 80)
    B, T, F = shape
    label = "c18w21f7"                                       # all three stages, a fractional warp on both sides
    blk = dict(R.case_blocks(shape))[label]
    x = R.case_input(shape).to(dtype).cuda()
    p = blk.cuda()
    base = ops.specaug_apply(x, p, R.N_TIME_CAP, R.N_FREQ_CAP)                       # contiguous: the 16-byte path
    wide_in = torch.full((B, T, 96), 7.0, dtype=dtype, device="cuda")
    wide_in[:, :, 8:88] = x
    wide_out = torch.full((B, T, 104), -3.0, dtype=dtype, device="cuda")
    got = ops.specaug_apply(wide_in[:, :, 8:88], p, R.N_TIME_CAP, R.N_FREQ_CAP, out=wide_out[:, :, 16:96])   # ld 96 / 104, vector path
    assert torch.equal(_bits(got), _bits(base)), label
    assert bool((wide_out[:, :, :16] == -3.0).all()) and bool((wide_out[:, :, 96:] == -3.0).all())
    odd_in = torch.full((B, T, 83), 7.0, dtype=dtype, device="cuda")                 # ld 83, first element off 16 bytes: scalar path
    odd_in[:, :, 1:81] = x
    odd_out = torch.full((B, T, 85), -3.0, dtype=dtype, device="cuda")
    got = ops.specaug_apply(odd_in[:, :, 1:81], p, R.N_TIME_CAP, R.N_FREQ_CAP, out=odd_out[:, :, 3:83])
    assert torch.equal(_bits(got), _bits(base)), label
    assert bool((odd_out[:, :, :3] == -3.0).all()) and bool((odd_out[:, :, 83:] == -3.0).all())


# ---- 5. the draw ------------------------------------------------------------------------------------------------------------------
def _draw(B, T, F, seed, counter=None, stages=7, t=TIME_DROP, f=FREQ_DROP):
    from summarymixing_amd import functional as SF
    from summarymixing_amd import ops
    ops.set_step_counter(None if counter is None else torch.tensor([counter], dtype=torch.int64, device="cuda"))
    try:
        return SF.spec_augment_draw(B, T, F, "cuda", stages, time_drop=t, freq_drop=f, window=5, seed=seed)
    finally:
        ops.set_step_counter(None)


def test_draw_recipe_values():
    B, T, F = 64, 400, 80
    blk = _draw(B, T, F, seed=2024)
    assert (blk.n_time_cap, blk.n_freq_cap) == (5, 2) and blk.data.numel() == 8 + 2 * B * 7
    v = blk.data.cpu()
    assert v.tolist() == R.draw_block(B, T, F, 7, TIME_DROP, FREQ_DROP, 5, 2024), "the kernel and its Python statement differ"
    flags, c, w, n_time, n_freq = v[:5].tolist()
    assert flags == 7 and n_time == 5 and n_freq == 2 and v[5:8].tolist() == [0, 0, 0]
    assert 5 <= c < T - 5 and c - 4 <= w <= c + 5
    tp = v[8:8 + 2 * B * 5].view(B, 5, 2)
    fp = v[8 + 2 * B * 5:].view(B, 2, 2)
    assert int(tp[..., 0].min()) >= 0 and int(tp[..., 0].max()) < T and int(fp[..., 0].min()) >= 0 and int(fp[..., 0].max()) < F
    assert sorted(set(tp[..., 1].flatten().tolist())) == list(range(15, 25))      # 320 draws of 10 values: P(miss) < 1e-13
    assert int(fp[..., 1].min()) >= 25 and int(fp[..., 1].max()) < 35
    assert len({tuple(r.flatten().tolist()) for r in tp}) == B and len({tuple(r.flatten().tolist()) for r in fp}) > B // 2
    # counts: uniform on [low, high] inclusive, one value for the batch
    counts = {int(_draw(2, 100, 80, seed=s, t=(5, 15, 1, 3)).data[3]) for s in range(40)}
    assert counts == {1, 2, 3}


def test_draw_warp_parameters_over_seeds():
    T = 40
    cw = [tuple(_draw(1, T, 80, seed=s).data[:3].tolist()) for s in range(200)]
    assert all(f == 7 and 5 <= c < 35 and c - 4 <= w <= c + 5 for f, c, w in cw)
    assert {w - c for _, c, w in cw} == set(range(-4, 6))    # ten values, 200 draws: P(miss) < 1e-8
    assert len({c for _, c, _ in cw}) > 15


def test_draw_is_a_function_of_seed_and_counter():
    a = _draw(4, 300, 80, seed=7, counter=11)
    assert torch.equal(a.data, _draw(4, 300, 80, seed=7, counter=11).data)
    assert not torch.equal(a.data, _draw(4, 300, 80, seed=7, counter=12).data)
    assert not torch.equal(a.data, _draw(4, 300, 80, seed=8, counter=11).data)
    assert a.data.cpu().tolist() == R.draw_block(4, 300, 80, 7, TIME_DROP, FREQ_DROP, 5, 7, counter=11)
    only_time = _draw(4, 300, 80, seed=7, counter=11, stages=R.TIME)
    assert (only_time.n_time_cap, only_time.n_freq_cap) == (5, 0) and only_time.data[:5].tolist() == [R.TIME, 0, 0, 5, 0]


# ---- 6. modules = functional ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_augmenter_equals_functional_and_the_stage_by_stage_chain(dtype):
    from summarymixing_amd import functional as SF
    from summarymixing_amd.augment.augmenter import Augmenter
    shape = (4, 200, 80)
    x = R.case_input(shape).to(dtype).cuda()
    lengths = torch.tensor([1.0, 0.9, 0.8, 0.5], device="cuda")
    aug = Augmenter(min_augmentations=3, max_augmentations=3, augmentations=_recipe_modules())
    y, lens = aug(x, lengths)
    assert lens is lengths and y.shape == x.shape and y.dtype == dtype
    blk = aug.last_params
    assert int(blk.data[0]) == 7 and (blk.n_time_cap, blk.n_freq_cap) == (5, 2)
    assert torch.equal(_bits(y), _bits(SF.spec_augment(x, blk)))
    assert not torch.equal(y, x) and bool((y == 0).any())
    # the same draws, one stage per launch: drops, then the warp over the zeroed stripes
    z = x
    for bit in (R.TIME, R.FREQ, R.WARP):
        one = blk.data.clone()
        one[0] = bit
        z = SF.spec_augment(z, SF.SpecAugBlock(one, blk.n_time_cap, blk.n_freq_cap))
    assert torch.equal(_bits(z), _bits(y))
    # against float64 on the drawn block too (the warp reads frames that the drops zeroed)
    ref = R.gather_ref(x.cpu(), blk.data.cpu(), 5, 2)
    emu = R.gather_ref(x.cpu(), blk.data.cpu(), 5, 2, torch.float32)
    bar = 8.0 * float((emu.double() - ref).abs().max()) + (ref.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    assert bool(((y.cpu().double() - ref).abs() <= bar).all())
    # a list that is not a subsequence of the chain runs module by module, each stage on its own draw
    mods = _recipe_modules()
    rev = Augmenter(augmentations=[mods[2], mods[0]])
    assert not rev.fused
    out, _ = rev(x, lengths)
    assert int(mods[2].last_params.data[0]) == R.WARP and int(mods[0].last_params.data[0]) == R.TIME
    want = SF.spec_augment(SF.spec_augment(x, mods[2].last_params), mods[0].last_params)
    assert torch.equal(_bits(out), _bits(want))


def test_four_dimensional_input_is_refused():
    from summarymixing_amd.augment.freq_domain import Warping
    with pytest.raises(NotImplementedError):
        Warping()(torch.zeros(2, 1, 40, 80, device="cuda"))


# ---- 7. hipGraph ------------------------------------------------------------------------------------------------------------------
def test_captured_augmenter_draws_afresh_on_every_replay():
    from summarymixing_amd import ops
    from summarymixing_amd.augment.augmenter import Augmenter
    B, T, F = 2, 40, 80
    # a seed whose draws at counters 5 and 6 differ in (c, w) - chosen with the Python statement of the draw, checked here
    seed = next(s for s in range(100, 200)
                if R.draw_block(B, T, F, 7, TIME_DROP, FREQ_DROP, 5, s, counter=5)[1:3] != R.draw_block(B, T, F, 7, TIME_DROP, FREQ_DROP, 5, s, counter=6)[1:3])
    x = R.case_input((B, T, F)).float().cuda()
    lengths = torch.ones(B, device="cuda")
    aug = Augmenter(augmentations=_recipe_modules())
    aug.seed = seed
    counter = torch.tensor([5], dtype=torch.int64, device="cuda")
    ops.set_step_counter(counter)
    try:
        eager = {}
        for k in (5, 6):
            counter.fill_(k)
            eager[k] = (aug(x, lengths)[0].clone(), aug.last_params.data.clone())
        counter.fill_(5)
        aug(x, lengths)                                      # (warm-up outside the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y, _ = aug(x, lengths)
            ops.step_counter_add(counter, 1)
        counter.fill_(5)
        outs = []
        for k in (5, 6):
            g.replay()
            outs.append((y.clone(), aug.last_params.data.clone()))
        torch.cuda.synchronize()
        assert int(counter) == 7
    finally:
        ops.set_step_counter(None)
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[0][1], outs[1][1])
    for (yk, pk), k in zip(outs, (5, 6)):
        assert pk.cpu().tolist() == R.draw_block(B, T, F, 7, TIME_DROP, FREQ_DROP, 5, seed, counter=k)
        assert torch.equal(pk, eager[k][1]) and torch.equal(_bits(yk), _bits(eager[k][0])), f"replay at counter {k}"

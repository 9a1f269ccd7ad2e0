"""summarymixing_amd.augment.time_domain on the GPU: smx_resample against the float64 gather-form reference (tests/_resample_ref.py;
the CPU suite checks that reference against the literal upstream chain on the same cases), impulses against the tap columns bit
for bit, strided and unaligned views, determinism, the modules against the functional form, and hipGraph replay.
Bar of the parity test: |y - ref| <= (taps + 2) 2^-24 S[i] with S[i] = sum_k |h[p][k] x[...]| - the float32 dot-product bound of a
`taps`-term fused multiply-add chain (gamma_taps), plus two units for the taps themselves (libm's evaluation may sit one float32
ulp from the reference's)."""
import pytest
import torch

import summarymixing_amd.augment.time_domain  # noqa: F401  (the module under test: without it nothing in this file runs)
from tests import _resample_ref as R
from tests._util import report

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. parity with float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", R.RATIOS, ids=[f"{a}to{b}" for a, b in R.RATIOS])
def test_resample_matches_the_float64_reference(ratio):
    from summarymixing_amd import functional as SF
    plan = R.plan_ref(*ratio)
    worst, where = 0.0, None
    for L in [L for a, b, L in R.CASES if (a, b) == ratio]:
        x, ref, S = R.case_ref(*ratio, L)
        xg = x.cuda()
        for B in (1, 3):
            y = SF.resample(xg[:B], *ratio)
            assert y.dtype == torch.float32 and y.shape == (B, R.out_len(plan.o, plan.n, L)) and y.is_contiguous()
            frac = ((y.cpu().double() - ref[:B]).abs() / ((plan.taps + 2) * 2.0 ** -24 * S[:B])).max()
            assert bool(torch.isfinite(frac)), (ratio, L, B)
            if float(frac) > worst:
                worst, where = float(frac), (L, B)
    report("resample", {"ratio": list(ratio), "taps": plan.taps, "worst_err_over_bound": worst, "at_L_B": list(where)})
    print(f"resample {ratio}: worst |err| / ((taps + 2) 2^-24 S) = {worst:.3f} at (L, B) = {where}")
    assert worst <= 1.0, f"{ratio}: an output sits {worst:.3f} of the bound from float64 at (L, B) = {where}"


# ---- 2. impulses: the taps come back bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [(20, 19), (20, 21), (2, 1), (441, 160), (160, 441)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_impulses_return_the_tap_columns(ratio):
    from summarymixing_amd import functional as SF
    plan, _ = SF.resample_plan(*ratio)
    ref = R.plan_ref(*ratio)
    h = R.dense_taps(plan.o, plan.n, plan.K, plan.first(), plan.weights())           # the library's own taps, laid out (n, K)
    span = plan.tile_blocks * plan.o
    L = 2 * span - 1
    at = [0, L - 1, span - 1, span]                          # the two edges and either side of the seam between two workgroups
    x = torch.zeros(len(at), L)
    for b, s in enumerate(at):
        x[b, s] = 1.0
    want, _ = R.gather_ref(x, ref, h=h)                      # one product h * 1 and zeros per output: exact in any precision
    y = SF.resample(x.cuda(), *ratio).cpu()
    hit = want != 0
    assert torch.equal(want.float().double(), want) and int(hit.sum(dim=1).min()) >= 3
    assert torch.equal(_bits(y)[hit], _bits(want.float())[hit]), f"{ratio}: an impulse response is not the tap column"
    assert bool((_bits(y)[~hit] == 0).all()), f"{ratio}: an output no tap reaches is not +0"


# ---- 3. leading dimensions and the element path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [(20, 19), (20, 21), (441, 160)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_strided_and_unaligned_views_give_the_same_bits(ratio):
    from summarymixing_amd import functional as SF
    plan, _ = SF.resample_plan(*ratio)
    B, L = 3, plan.tile_blocks * plan.o + 37
    Lo = plan.out_len(L)
    x = R.case_input(L).cuda()
    base = SF.resample(x, *ratio)                                                     # contiguous, aligned: 16-byte loads and stores
    ldx4, ldy4 = L + 12 + (-L) % 4, Lo + 8 + (-Lo) % 4      # multiples of four: with a 16-byte aligned base, the 16-byte path
    ldx1, ldy1 = ldx4 + 1, ldy4 + 1
    for ldx, ldy, off in ((ldx4, ldy4, 0), (ldx4, ldy1, 0), (ldx1, ldy4, 0),          # wide rows: both, loads only, stores only
                          (ldx1, ldy1, 0), (ldx4, ldy4, 1), (ldx1, ldy1, 1)):          # element path: odd rows, one element off, both
        xin = torch.full((B * ldx + 4,), 7.0, device="cuda")
        xv = xin[off:off + B * ldx].view(B, ldx)[:, :L]
        xv.copy_(x)
        yout = torch.full((B * ldy + 64,), -3.0, device="cuda")
        yv = yout[off:off + B * ldy].view(B, ldy)[:, :Lo]
        assert (xv.data_ptr() % 16 == 0) == (off == 0) and (yv.data_ptr() % 16 == 0) == (off == 0)
        got = SF.resample(xv, *ratio, out=yv)
        assert got.data_ptr() == yv.data_ptr()
        assert torch.equal(_bits(got), _bits(base)), (ratio, ldx, ldy, off)
        canary = yout[off:off + B * ldy].view(B, ldy)[:, Lo:]
        assert bool((canary == -3.0).all()) and bool((yout[:off] == -3.0).all()) and bool((yout[off + B * ldy:] == -3.0).all())
        assert bool((xin[off:off + B * ldx].view(B, ldx)[:, L:] == 7.0).all())


def test_rows_that_start_beyond_two_to_the_31_elements():
    """b * ldx and b * ldy pass 2^31 elements from row 49 942 on: the last rows give the bits the first rows give (8.6 GB per side,
    allocated and - but for L samples per row - never touched)."""
    from summarymixing_amd import functional as SF
    B, L, ld = 50000, 64, 43000
    Lo = R.out_len(20, 19, L)
    assert (B - 2) * ld > 2 ** 31
    x = R.case_input(L)[:2].cuda()
    xv = torch.empty(B * ld, device="cuda").view(B, ld)[:, :L]
    xv[:2] = x
    xv[-2:] = x
    yv = torch.empty(B * ld, device="cuda").view(B, ld)[:, :Lo]
    yv[-2:] = -3.0
    SF.resample(xv, 20, 19, out=yv)
    want = SF.resample(x, 20, 19)
    assert torch.equal(_bits(yv[:2]), _bits(want)) and torch.equal(_bits(yv[-2:]), _bits(want))


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    from summarymixing_amd import functional as SF
    plan, _ = SF.resample_plan(16000, 15200)
    x = R.case_input(2 * plan.tile_blocks * plan.o - 1).cuda()
    a, b = SF.resample(x, 16000, 15200), SF.resample(x, 16000, 15200)
    assert a.data_ptr() != b.data_ptr() and torch.equal(_bits(a), _bits(b))


# ---- 5. modules = functional ------------------------------------------------------------------------------------------------------
def test_modules_equal_the_functional_form():
    from summarymixing_amd import functional as SF
    from summarymixing_amd.augment.augmenter import Augmenter
    from summarymixing_amd.augment.time_domain import Resample, SpeedPerturb
    B, L = 3, 4077
    x = R.case_input(L).cuda()
    lens = torch.tensor([1.0, 0.7, 0.4], device="cuda")
    sp = SpeedPerturb(orig_freq=16000, speeds=[95, 100, 105])
    aug = Augmenter(parallel_augment=False, concat_original=False, repeat_augment=1, shuffle_augmentations=False,
                    min_augmentations=1, max_augmentations=1, augment_prob=1.0, augmentations=[sp])
    for index, (o, n) in ((0, (20, 19)), (2, (20, 21))):
        sp.draw = lambda index=index: torch.tensor(index)
        y = sp(x)
        want = SF.resample(x, 16000, 16000 * sp.speeds[index] // 100)
        assert int(sp.samp_index) == index and y.shape == (B, -(-n * L // o)) and torch.equal(_bits(y), _bits(want))
        z, out_lens = aug(x, lens)
        assert out_lens is lens and z.shape == (B, -(-n * L // o)) and torch.equal(_bits(z), _bits(want))
    sp.draw = lambda: torch.tensor(1)
    assert sp(x) is x and aug(x, lens)[0] is x                                       # speed 100: the very tensor
    del sp.draw                                                                       # the class's own draw again
    torch.manual_seed(7)
    drawn = [int(torch.randint(3, (1,))[0]) for _ in range(6)]
    torch.manual_seed(7)
    shapes = [aug(x, lens)[0].shape[1] for _ in range(6)]
    assert shapes == [[-(-19 * L // 20), L, -(-21 * L // 20)][i] for i in drawn]
    # (B, T, 1) as upstream takes it; more channels are refused by name
    r = Resample(16000, 15200)
    y3 = r(x.unsqueeze(2))
    assert y3.shape == (B, -(-19 * L // 20), 1) and torch.equal(_bits(y3.squeeze(2)), _bits(SF.resample(x, 16000, 15200)))
    with pytest.raises(NotImplementedError, match="channels"):
        r(torch.zeros(2, 100, 2, device="cuda"))
    with pytest.raises(ValueError):
        r(torch.zeros(2, 100, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        SF.resample(x, 16000, 15200, out=torch.empty(B, L, device="cuda"))


# ---- 6. hipGraph ------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_on_new_input():
    from summarymixing_amd import functional as SF
    plan, _ = SF.resample_plan(16000, 16800)
    B, L = 2, plan.tile_blocks * plan.o + 37
    a, b = R.case_input(L)[:B].cuda(), R.case_input(L + 1)[:B, 1:].contiguous().cuda()
    x = a.clone()
    out = torch.empty(B, plan.out_len(L), device="cuda")
    want_a = SF.resample(a, 16000, 16800)                    # (also the warm-up: the plan is on the device before the capture)
    want_b = SF.resample(b, 16000, 16800)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        SF.resample(x, 16000, 16800, out=out)
    g.replay()
    assert torch.equal(_bits(out), _bits(want_a))
    x.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(want_a, want_b) and torch.equal(_bits(out), _bits(want_b))

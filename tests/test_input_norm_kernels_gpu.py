"""InputNormalization's kernels one by one against float64: smx_utt_meanstd (per-utterance mean / unbiased std over the valid
frames), smx_stats_combine (batch average blended into the running statistics), smx_colnorm, and the module on top of them at the
lengths, flags and feature counts tests/test_frontend_gpu.py::test_input_normalization_matches_spec does not reach.

Bars: four times the floor of a plain float32 two-pass restatement against float64, measured here on the CPU per utterance
(utt_meanstd); one float32 rounding of the float64 expression (stats_combine); a written-out a-priori bound and bit equality
(colnorm).  None is taken from the kernels.  Measured errors and floors go to tests._util.report."""
import pytest
import torch

from tests._util import rel_err, report

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = 1e-10
N_VALID = (1, 2, 15, 16, 17, 63, 64, 65, 129, 130)         # around the kernel's 16-frame groups and its 64-frame unrolled stride; 130 = T


def _meanstd(x, n, dtype):
    """Two-pass mean and unbiased std (clamped at eps; NaN for one frame, like torch.std) of x[:n] (T, F) in `dtype`, both passes
    summed frame after frame: the plain restatement - float64 is the reference, float32 the floor."""
    xs = x[:n].to(dtype)
    s = torch.zeros(x.shape[1], dtype=dtype)
    for t in range(n):
        s = s + xs[t]
    m = s / n
    q = torch.zeros_like(s)
    for t in range(n):
        d = xs[t] - m
        q = q + d * d
    var = q / (n - 1) if n > 1 else torch.full_like(q, float("nan"))
    return m, torch.maximum(var.sqrt(), torch.full_like(q, EPS))


def _utterances(F, T, dtype, seed):
    """(B, T, F): by turns features of the recipe's scale (7 randn - 20) and 1000 + 0.01 randn, where a one-pass variance
    (E x^2 - (E x)^2 in float32) is wrong by orders of magnitude; feature 2 is constant in every utterance (std 0 -> eps)."""
    g = torch.Generator().manual_seed(seed)
    B = len(N_VALID)
    x = torch.randn(B, T, F, generator=g)
    x[0::2] = x[0::2] * 7.0 - 20.0
    x[1::2] = x[1::2] * 0.01 + 1000.0
    x[:, :, 2] = 0.7
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("F", [7, 40, 80, 83])
def test_utt_meanstd_matches_float64(F, dtype):
    from summarymixing_amd import ops
    T, B = 130, len(N_VALID)
    x = _utterances(F, T, dtype, F)
    lens = torch.tensor(N_VALID, dtype=torch.int32)
    mean = torch.full((B, F), -7.0, device="cuda")
    std = torch.full((B, F), -7.0, device="cuda")
    ops.utt_meanstd(x.cuda().view(B * T, F), lens.cuda(), mean, std, B, T, True, True, EPS)
    torch.cuda.synchronize()
    mean, std = mean.cpu().double(), std.cpu().double()
    for b, n in enumerate(N_VALID):
        xf = x[b].float()                                                           # (bf16 inputs are exact in float32)
        m64, s64 = _meanstd(xf, n, torch.float64)
        m32, s32 = _meanstd(xf, n, torch.float32)
        if n == 1:
            assert torch.isnan(s64).all() and torch.isnan(s32).all() and torch.isnan(std[b]).all(), "one frame: NaN std in all three"
            assert torch.equal(mean[b], m64)
            continue
        assert torch.isfinite(mean[b]).all() and torch.isfinite(std[b]).all()
        fm, fs = float((m32.double() - m64).abs().max()), float((s32.double() - s64).abs().max())
        em, es = float((mean[b] - m64).abs().max()), float((std[b] - s64).abs().max())
        report("utt_meanstd", {"F": F, "dtype": str(dtype)[6:], "n": n, "kind": "recipe" if b % 2 == 0 else "1000+0.01randn",
                               "err_mean": em, "floor_mean": fm, "err_std": es, "floor_std": fs})
        assert em <= 4 * fm and es <= 4 * fs, (n, em, fm, es, fs)
        assert float(s64[2]) == EPS                                      # the constant feature: clamped at eps in float64
    # the switches: exact zeros / exact ones, whatever the data
    for mn, sn in ((False, True), (True, False), (False, False)):
        m2, s2 = torch.full((B, F), -7.0, device="cuda"), torch.full((B, F), -7.0, device="cuda")
        ops.utt_meanstd(x.cuda().view(B * T, F), lens.cuda(), m2, s2, B, T, mn, sn, EPS)
        torch.cuda.synchronize()
        assert (torch.equal(m2.cpu().double(), mean) if mn else not m2.any())
        assert (torch.equal(s2.cpu().double()[1:], std[1:]) if sn else bool((s2 == 1.0).all()))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("weight", [1.0, 1.0 / (3 + 1), 0.05], ids=["replace", "count3", "avg_factor"])
def test_stats_combine_is_one_rounding_of_the_expression(weight, B):
    """glob <- (1 - w) glob + w mean_b(cur)  (w = 1: glob <- mean_b(cur)) over F = 300 features (a second 256-thread block): the
    result is the float64 value of that expression - with w as the float32 the C interface receives - rounded once to float32,
    i.e. within 2^-24 of it, relatively."""
    from summarymixing_amd import ops
    g = torch.Generator().manual_seed(B)
    F = 300
    cm, cs = torch.randn(B, F, generator=g) * 5 - 20, torch.rand(B, F, generator=g) * 7 + 0.01
    gm, gs = torch.randn(F, generator=g) * 5 - 20, torch.rand(F, generator=g) * 7 + 0.01
    w = float(torch.tensor(weight, dtype=torch.float32))
    want = []
    for cur, glob in ((cm, gm), (cs, gs)):
        avg = cur.double().sum(0) / B
        want.append(avg if weight >= 1.0 else (1.0 - w) * glob.double() + w * avg)
    dm, ds = gm.cuda(), gs.cuda()
    ops.stats_combine(cm.cuda(), cs.cuda(), dm, ds, weight)
    torch.cuda.synchronize()
    worst = 0.0
    for got, ref in ((dm, want[0]), (ds, want[1])):
        err = (got.cpu().double() - ref).abs()
        worst = max(worst, float((err / ref.abs()).max()))
        assert (err <= U32 * ref.abs() * (1 + 1e-9)).all()
    report("stats_combine", {"B": B, "weight": weight, "rel_err": worst, "bar": U32})


@pytest.mark.parametrize("shared", [True, False], ids=["stride0", "strideF"])
@pytest.mark.parametrize("B,T,F", [(3, 11, 83), (2, 130, 80), (1, 1, 7)])
def test_colnorm_float32_bound_and_bf16_rounding(B, T, F, shared):
    """y = (x - mean) / std with statistics shared by the batch (stride 0) or per utterance (stride F).  float32: the subtraction
    rounds once (u) and the division - a reciprocal (1 ulp) and a product under the library's -ffast-math - at most 5 u more:
    |y - y64| <= 8 u |y64| with u = 2^-24.  bf16 (input, output; the statistics stay float32): bit-equal to the float32 kernel's
    result on the same values, rounded to bf16."""
    from summarymixing_amd import ops
    g = torch.Generator().manual_seed(T * F)
    x = (torch.randn(B * T, F, generator=g) * 7 - 20).bfloat16().float()            # (representable in both dtypes)
    mean = torch.randn((1 if shared else B), F, generator=g) * 5 - 20
    std = torch.rand((1 if shared else B), F, generator=g) * 7 + 0.01
    stride = 0 if shared else F
    y32 = torch.full((B * T, F), float("nan"), device="cuda")
    ops.colnorm(x.cuda(), mean.cuda(), std.cuda(), stride, y32, B, T)
    y16 = torch.zeros((B * T, F), dtype=torch.bfloat16, device="cuda")
    ops.colnorm(x.cuda().bfloat16(), mean.cuda(), std.cuda(), stride, y16, B, T)
    torch.cuda.synchronize()
    ref = ((x.double().view(B, T, F) - mean.double()[:, None]) / std.double()[:, None]).view(B * T, F)
    err = (y32.cpu().double() - ref).abs()
    report("colnorm", {"B": B, "T": T, "F": F, "shared": shared, "err_over_u_y": float((err / (U32 * ref.abs())).max()), "bar": 8})
    assert (err <= 8 * U32 * ref.abs()).all()
    assert torch.equal(y16.cpu(), y32.cpu().bfloat16())


# ---- the module ------------------------------------------------------------------------------------------------------------
CONFIGS = [dict(), dict(mean_norm=False), dict(std_norm=False), dict(mean_norm=False, std_norm=False), dict(avg_factor=0.1)]


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1e-2)], ids=["f32", "bf16"])
@pytest.mark.parametrize("kw", CONFIGS, ids=["default", "no-mean", "no-std", "neither", "avg-factor"])
@pytest.mark.parametrize("norm_type", ["global", "batch", "sentence"])
def test_module_flags_and_degenerate_lengths(norm_type, kw, dtype, tol):
    """The module against oracle.smx_oracle.input_normalization in float64, F = 83 (not a multiple of the kernel's 16 features per
    workgroup): eval before any training batch (global: the identity), three training batches, then a batch in which one length
    rounds to ONE frame and one to ZERO frames - mean / std of those are NaN in torch, and the output's non-finite pattern must be
    the oracle's (tests._util.rel_err asserts it) - and, for "global", that the poisoned running statistics stay what the oracle's are.
    Bar: the scale-relative 1e-5 (float32) / 1e-2 (bf16 output, 2^-9 rounding) of test_input_normalization_matches_spec; a-priori the
    float32 statistics over T = 57 frames are within (T + 2) 2^-24 max|x| ~ 1.5e-4 of exact, which is 5e-6 of the output's scale."""
    from oracle import smx_oracle as O
    from summarymixing_amd.lobes.features import InputNormalization
    g = torch.Generator().manual_seed(11)
    B, T, F = 4, 57, 83
    mod = InputNormalization(norm_type=norm_type, update_until_epoch=2, **kw).cuda()
    st = O.InputNormalizationState()
    okw = dict(norm_type=norm_type, update_until_epoch=2, mean_norm=kw.get("mean_norm", True), std_norm=kw.get("std_norm", True),
               avg_factor=kw.get("avg_factor"))
    full = torch.tensor([1.0, 0.53, 0.8, 0.31])
    x = (torch.randn(B, T, F, generator=g) * 7.0 - 20.0).to(dtype)
    if norm_type == "global":
        mod.eval()
        assert torch.equal(mod(x.cuda(), full.cuda()), x.cuda()) and mod.count == 0  # zeros / ones statistics: the identity
    mod.train()
    for epoch in (0, 1, 5):
        x = (torch.randn(B, T, F, generator=g) * 7.0 - 20.0).to(dtype)
        ref = O.input_normalization(x.double(), full, st, epoch=epoch, **okw)
        e = rel_err(mod(x.cuda(), full.cuda(), epoch=epoch), ref)
        report("input_norm_module", {"norm_type": norm_type, "flags": str(kw), "dtype": str(dtype)[6:], "epoch": epoch, "rel_err": e, "bar": tol})
        assert e <= tol
    assert torch.isfinite(ref).all()
    lens = torch.tensor([1.0, 1.0 / 57, 0.8, 0.005])                                # -> 57, 1, 46 and 0 valid frames
    assert torch.round(lens * T).tolist() == [57, 1, 46, 0]
    x = (torch.randn(B, T, F, generator=g) * 7.0 - 20.0).to(dtype)
    ref = O.input_normalization(x.double(), lens, st, epoch=0, **okw)
    y = mod(x.cuda(), lens.cuda(), epoch=0)
    assert rel_err(y, ref) <= tol                                                   # (asserts the same non-finite cells first)
    if okw["std_norm"] or okw["mean_norm"]:
        assert not torch.isfinite(ref).all()
    if norm_type == "global":
        assert mod.count == st.count == 4
        assert rel_err(mod.glob_mean, st.glob_mean.expand(F)) <= 1e-5 and rel_err(mod.glob_std, st.glob_std.expand(F)) <= 1e-5


def test_module_state_dict_round_trip_after_three_batches():
    from summarymixing_amd.lobes.features import InputNormalization
    g = torch.Generator().manual_seed(3)
    B, T, F = 3, 40, 83
    mod = InputNormalization(norm_type="global").cuda().train()
    lens = torch.tensor([1.0, 0.6, 0.35]).cuda()
    for _ in range(3):
        mod(torch.randn(B, T, F, generator=g).cuda() * 3 + 5, lens)
    sd = {k: (v.clone() if torch.is_tensor(v) else dict(v)) for k, v in mod.state_dict().items()}
    new = InputNormalization(norm_type="global")
    assert new.glob_mean is None and new.count == 0
    new.load_state_dict(sd)
    new = new.cuda().eval()
    assert new.count == mod.count == 3
    assert torch.equal(new.glob_mean, mod.glob_mean) and torch.equal(new.glob_std, mod.glob_std)
    x = torch.randn(B, T, F, generator=g).cuda()
    assert torch.equal(new(x, lens), mod.eval()(x, lens)) and new.count == 3

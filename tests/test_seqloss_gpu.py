"""The label-smoothed sequence losses and the accuracy of csrc/seqloss.hip, stage by stage through summarymixing_amd.ops and end to end
through summarymixing_amd.nnet.losses / utils.Accuracy, on inputs made on the CPU from a seed and against the fp64 restatement of
upstream's operations in tests/_seqloss_ref.py evaluated on THE SAME dtype-rounded inputs.

Shapes: (B, U) in {(1, 1), (3, 5), (2, 9)} (rows are no multiple of the four waves of a block), V in {2, 63, 64, 65, 1000, 1003,
5000} (below one wave, the seam, rows that are 16-byte aligned only every fourth / eighth row and carry a tail, the recipes' sizes).

Bars (the convention of tests/test_ctc_kernels_gpu.py; nothing has a number fixed in advance).  The same definition is evaluated in
fp32 on the CPU; its worst error against fp64, in the metric asserted, is the floor, and the kernel gets _FLOOR_X x that floor plus
_MIN_ULPS fp32 ulps of the quantity's scale.  Losses, sums and lse: |got - ref| / max(1, |ref|).  Gradients: per entry, absolute,
the scale being max |ref|; a bf16 gradient adds 2^-8 |ref entry| for the rounding of the output.  Every comparison asserts how many
rows it covered; only dropped rows are left out, and those must be exact zeros.  Floors and measured errors go to report()."""
import pytest
import torch

from tests import _seqloss_ref as R
from tests._util import report

pytestmark = pytest.mark.gpu

_FLOOR_X = 4.0
_MIN_ULPS = 4.0
_EPS32 = 2.0 ** -23
_BF16_ROUND = 2.0 ** -8
_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
_SHAPES = ((1, 1), (3, 5), (2, 9))
_VS = (2, 63, 64, 65, 1000, 1003, 5000)
_COMBOS = (("nll", 0.0), ("nll", 0.1), ("kldiv", 0.1))    # (kldiv with smoothing 0 IS nll: test_reductions_and_their_gradients)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _terms(kind, eps, V):
    from summarymixing_amd.nnet import losses
    return losses.smoothing_terms(kind, eps, V)


def _keep_args(kind, length, U, pad):
    """(keep_len on the device or None, pad_idx) as the Python surface hands them to the kernels."""
    from summarymixing_amd.nnet import losses
    if kind == "kldiv":
        return None, pad
    return (None if length is None else losses.mask_count(length.cuda(), U)), -1


def _ops_run(kind, logits, x_dev, tg, length, pad, eps, g, out=None):
    """ops.seqloss_fwd + ops.seqloss_bwd on a device tensor x_dev (any strides) -> CPU tensors."""
    from summarymixing_amd import ops
    B, U, V = x_dev.shape
    keep_len, pad_idx = _keep_args(kind, length, U, pad)
    conf, off, cst = _terms(kind, eps, V)
    tgd = tg.to(torch.int32).cuda()
    row, lse, flags, utt, kept, hits = ops.seqloss_fwd(x_dev, tgd, keep_len, pad_idx, conf, off, cst, logits)
    dx = ops.seqloss_bwd(x_dev, tgd, keep_len, pad_idx, conf, off, lse, g.float().cuda().contiguous(), logits, out=out)
    torch.cuda.synchronize()
    assert dx.dtype == x_dev.dtype and dx.shape == (B, U, V) and row.shape == (B, U)
    return dict(row=row.cpu(), lse=None if lse is None else lse.cpu(), flags=flags.cpu(), utt=utt.cpu(), kept=kept.cpu(), hits=hits.cpu(),
                dx=dx.cpu())


def _rel(name, q, got, r64, r32, n_expected):
    """max |got - ref| / max(1, |ref|) against _FLOOR_X x the same of the fp32 evaluation.  -> (floor, err)."""
    assert got.numel() == r64.numel() == n_expected, (name, q, "compared", got.numel(), "expected", n_expected)
    if n_expected == 0:
        return 0.0, 0.0
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(got).all()), (name, q, "non-finite")
    den = r64.abs().clamp(min=1.0)
    floor = float(((r32.double() - r64).abs() / den).max())
    err = float(((got.double() - r64).abs() / den).max())
    bar = _FLOOR_X * floor + _MIN_ULPS * _EPS32
    print(f"{name} {q}: n {n_expected} floor {floor:.3e} err {err:.3e} bar {bar:.3e}")
    assert err <= bar, (name, q, "err", err, "fp32 floor", floor, "bar", bar)
    return floor, err


def _grad(name, q, got, r64, r32, keep, n_expected, bf16):
    """Per entry of the kept rows; dropped rows exact zeros.  -> (floor, err, worst err / bar)."""
    rows = int(keep.sum())
    assert rows == n_expected, (name, q, "compared rows", rows, "expected", n_expected)
    assert float(got[~keep].float().abs().sum()) == 0.0 and not bool(torch.isnan(got[~keep].float()).any()), (name, q, "dropped rows must be exact zeros")
    if rows == 0:
        return 0.0, 0.0, 0.0
    g, a, b = got[keep].double(), r64[keep], r32[keep].double()
    assert bool(torch.isfinite(g).all()), (name, q, "non-finite gradient on a kept row")
    scale = float(a.abs().max())
    floor = float((b - a).abs().max())
    bar = _FLOOR_X * floor + _MIN_ULPS * _EPS32 * scale + (_BF16_ROUND * a.abs() if bf16 else 0.0)
    err = (g - a).abs()
    worst = float((err / bar).max()) if scale > 0 else float(err.max())
    print(f"{name} {q}: rows {rows} floor {floor:.3e} err {float(err.max()):.3e} scale {scale:.3e} err/bar {worst:.3f}")
    assert bool((err <= bar).all()), (name, q, "worst err / bar", worst, "floor", floor, "scale", scale)
    return floor, float(err.max()), worst


def _check(name, kind, logits, x, tg, length, pad, eps, seed=0, expect_rows=None):
    """Every stage of one case: x (B, U, V) CPU tensor in its dtype (logits or log-probabilities)."""
    B, U, V = x.shape
    bf16 = x.dtype == torch.bfloat16
    g = torch.randn(B, U, generator=torch.Generator().manual_seed(1000 + seed)) * 1.5       # non-uniform, both signs
    out = _ops_run(kind, logits, x.cuda(), tg, length, pad, eps, g)
    keep = R.keep_mask(kind, tg, length, pad)
    n = int(keep.sum())
    if expect_rows is not None:
        assert n == expect_rows, (name, "the generated case keeps", n, "rows, the test means", expect_rows)
    lp64 = x.double().log_softmax(-1) if logits else x.double()
    lp32 = x.float().log_softmax(-1) if logits else x.float()
    r64 = R.row_losses(kind, lp64, tg, length, eps, pad)
    r32 = R.row_losses(kind, lp32, tg, length, eps, pad, dtype=torch.float32)
    w = {}
    # row losses: kept rows against the reference, dropped rows exact zeros
    assert float(out["row"][~keep].abs().sum()) == 0.0, (name, "row loss of a dropped row")
    w["row_floor"], w["row_err"] = _rel(name, "row", out["row"][keep], r64[keep], r32[keep], n)
    # utterance sums, counts
    w["utt_floor"], w["utt_err"] = _rel(name, "utt", out["utt"], r64.sum(1), r32.sum(1), B)
    hits, kept = R.accuracy(x.float(), tg, keep)
    assert out["kept"].tolist() == kept.tolist(), (name, "kept", out["kept"].tolist(), kept.tolist())
    assert out["hits"].tolist() == hits.tolist(), (name, "hits", out["hits"].tolist(), hits.tolist())
    assert torch.equal((out["flags"] & 1).bool(), keep)
    if logits:
        l64, l32 = x.double().logsumexp(-1), x.float().logsumexp(-1)
        w["lse_floor"], w["lse_err"] = _rel(name, "lse", out["lse"][..., 0][keep], l64[keep], l32[keep], n)
        _rel(name, "lse hi+lo", (out["lse"][..., 0].double() + out["lse"][..., 1].double())[keep], l64[keep], l32[keep], n)
        assert float(out["lse"][~keep].abs().sum()) == 0.0
        g64 = R.grad_logits(kind, x, tg, keep, g, eps)
        g32 = R.grad_logits(kind, x, tg, keep, g, eps, dtype=torch.float32)
    else:
        g64 = R.grad_log_probs(kind, tg, V, keep, g, eps)
        g32 = R.grad_log_probs(kind, tg, V, keep, g, eps, dtype=torch.float32)
    w["g_floor"], w["g_err"], w["g_err_over_bar"] = _grad(name, "grad", out["dx"], g64, g32, keep, n, bf16)
    return w


def _merge(acc, w):
    for k, v in w.items():
        acc[k] = max(acc.get(k, 0.0), v)


# ---- 1. every stage on every path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", _VS)
def test_rows_sums_lse_and_gradient_against_fp64(V, dtype):
    worst, cases = {}, 0
    for (B, U) in _SHAPES:
        for kind, eps in _COMBOS:
            for logits in (False, True):
                z, tg, length, pad = R.case(B, U, V, _DT[dtype], seed=17 * V + 3 * B + U)
                x = z if logits else z.double().log_softmax(-1).to(_DT[dtype])
                name = f"{kind} e={eps} {'logits' if logits else 'logprobs'} ({B},{U},{V}) {dtype}"
                _merge(worst, _check(name, kind, logits, x, tg, length, pad, eps, seed=cases))
                cases += 1
    assert cases == len(_SHAPES) * len(_COMBOS) * 2
    report(f"seqloss_stages[V={V},{dtype}]", dict(cases=cases, **worst))


def test_the_batch_carries_every_kind_of_row():
    """What tests/_seqloss_ref.case promises, on the (3, 5) batch: token 0, token V - 1, a pad token inside a kept span, a full, a
    fractional and an empty utterance under the length mask, an all-pad utterance for kldiv."""
    z, tg, length, pad = R.case(3, 5, 65, torch.float32, seed=1)
    km = R.keep_mask("nll", tg, length, pad)
    assert km.sum(1).tolist() == [5, 3, 0]
    assert int(tg[0, 0]) == 0 and int(tg[0, 4]) == 64 and int(tg[0, 2]) == pad and bool(km[0, 2])
    kk = R.keep_mask("kldiv", tg, length, pad)
    assert int(kk[2].sum()) == 0 and not bool(kk[0, 2]) and int(kk[0].sum()) >= 2
    _check("composition of the batch, nll", "nll", True, z, tg, length, pad, 0.1, expect_rows=8)
    _check("composition of the batch, kldiv", "kldiv", True, z, tg, length, pad, 0.1, expect_rows=int(kk.sum()))


# ---- 2. lse stability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("what", ["shift+80", "shift-80", "dominant"])
def test_large_logits_keep_the_loss_and_the_gradient(what, dtype):
    B, U, V = 3, 5, 1000
    shift = {"shift+80": 80.0, "shift-80": -80.0, "dominant": 0.0}[what]
    z, tg, length, pad = R.case(B, U, V, torch.float64, seed=5, shift=shift)
    if what == "dominant":
        z[0, 1, 7] = 60.0                                 # one entry carries the whole row: lse = 60 + ~1e-24
        z[1, 0, int(tg[1, 0])] = 45.0                     # ... and once it is the target: loss ~ 0, gradient ~ 0
    z = z.to(_DT[dtype])
    worst = {}
    for kind, eps in _COMBOS:
        _merge(worst, _check(f"{what} {kind} e={eps} {dtype}", kind, True, z, tg, length, pad, eps))
    report(f"seqloss_lse_stability[{what},{dtype}]", worst)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("logits", [False, True], ids=["logprobs", "logits"])
def test_minus_infinity_away_from_the_target_without_smoothing(logits, dtype):
    """off == 0: the row sum does not enter, so -inf log-probabilities (or logits) away from y leave the loss finite, as upstream."""
    B, U, V = 3, 5, 65
    z, tg, length, pad = R.case(B, U, V, torch.float64, seed=6)
    for b, u in ((0, 0), (0, 3), (1, 1)):
        cols = [v for v in (1, 9, 63, 64) if v != int(tg[b, u])]
        z[b, u, cols] = float("-inf")
    x = (z if logits else z.log_softmax(-1)).to(_DT[dtype])
    w = _check(f"-inf off target {dtype}", "nll", logits, x, tg, length, pad, 0.0, expect_rows=8)
    report(f"seqloss_neg_inf[{'logits' if logits else 'logprobs'},{dtype}]", w)


# ---- 3. memory: strides, the buffer the backward is handed, out-of-range targets ----------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V,extra", [(65, 3), (65, 8), (1000, 5), (1003, 13)])
def test_a_column_slice_of_a_nan_buffer_gives_the_same_bits(V, extra, dtype):
    B, U = 3, 5
    g = torch.randn(B, U, generator=torch.Generator().manual_seed(7))
    for kind, eps in _COMBOS:
        for logits in (False, True):
            z, tg, length, pad = R.case(B, U, V, _DT[dtype], seed=8)
            x = z if logits else z.double().log_softmax(-1).to(_DT[dtype])
            dense = _ops_run(kind, logits, x.cuda(), tg, length, pad, eps, g)
            wide = torch.full((B, U, V + extra), float("nan"), dtype=_DT[dtype], device="cuda")
            wide[:, :, :V] = x.cuda()
            view = wide[:, :, :V]
            assert view.stride() == (U * (V + extra), V + extra, 1)
            sliced = _ops_run(kind, logits, view, tg, length, pad, eps, g)
            for k in ("row", "utt", "dx") + (("lse",) if logits else ()):
                assert not bool(torch.isnan(sliced[k].float()).any()), (kind, logits, k, "NaN leaked from the other columns")
                assert torch.equal(_bits(sliced[k]), _bits(dense[k])), (kind, logits, k)
            assert torch.equal(sliced["kept"], dense["kept"]) and torch.equal(sliced["hits"], dense["hits"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("logits", [False, True], ids=["logprobs", "logits"])
def test_dropped_rows_of_a_nan_filled_gradient_buffer_come_back_as_zeros(logits, dtype):
    B, U, V = 3, 5, 1003
    z, tg, length, pad = R.case(B, U, V, _DT[dtype], seed=9)
    g = torch.randn(B, U, generator=torch.Generator().manual_seed(10))
    for kind, eps in _COMBOS:
        keep = R.keep_mask(kind, tg, length, pad)
        buf = torch.full((B, U, V), float("nan"), dtype=_DT[dtype], device="cuda")
        out = _ops_run(kind, logits, z.cuda(), tg, length, pad, eps, g, out=buf)
        assert int((~keep).sum()) >= 5
        assert float(out["dx"][~keep].float().abs().sum()) == 0.0 and bool(torch.isfinite(out["dx"].float()).all())
        assert bool((out["dx"][keep].float().abs().sum(-1) > 0).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("logits", [False, True], ids=["logprobs", "logits"])
@pytest.mark.parametrize("bad", ["V", "-1"])
def test_an_out_of_range_target_is_a_nan_row_and_nothing_else(bad, logits, dtype):
    """The bad target sits on an interior row, so even a kernel that indexed with it would read inside the tensor."""
    B, U, V = 3, 5, 65
    z, tg, _, pad = R.case(B, U, V, _DT[dtype], seed=11)
    tg[2, :] = torch.arange(U) + 2                        # (no all-pad utterance here: every row is kept)
    g = torch.randn(B, U, generator=torch.Generator().manual_seed(12))
    for kind, eps in (("nll", 0.1), ("nll", 0.0)):
        good = _ops_run(kind, logits, z.cuda(), tg, None, pad, eps, g)
        tb = tg.clone()
        tb[1, 2] = V if bad == "V" else -1
        out = _ops_run(kind, logits, z.cuda(), tb, None, pad, eps, g)
        other = torch.ones(B, U, dtype=torch.bool)
        other[1, 2] = False
        assert bool(torch.isnan(out["row"][1, 2])) and bool(torch.isnan(out["dx"][1, 2].float()).all())
        assert torch.equal(_bits(out["row"][other]), _bits(good["row"][other])) and torch.equal(_bits(out["dx"][other]), _bits(good["dx"][other]))
        assert bool(torch.isnan(out["utt"][1])) and torch.equal(out["utt"][[0, 2]], good["utt"][[0, 2]])
        assert out["kept"].tolist() == [U, U, U] and int(out["hits"][1]) <= int(good["hits"][1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_runs_agree_bit_for_bit(dtype):
    B, U, V = 3, 5, 5000
    z, tg, length, pad = R.case(B, U, V, _DT[dtype], seed=13)
    g = torch.randn(B, U, generator=torch.Generator().manual_seed(14))
    for kind, eps in _COMBOS:
        for logits in (False, True):
            a = _ops_run(kind, logits, z.cuda(), tg, length, pad, eps, g)
            b = _ops_run(kind, logits, z.cuda(), tg, length, pad, eps, g)
            for k in ("row", "utt", "dx", "kept", "hits") + (("lse",) if logits else ()):
                assert torch.equal(_bits(a[k]), _bits(b[k])), (kind, logits, k)


# ---- 4. accuracy ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_accuracy_ties_take_the_smallest_index(dtype):
    from summarymixing_amd.utils.Accuracy import Accuracy
    B, U, V = 1, 6, 1000
    x = torch.randn(B, U, V, generator=torch.Generator().manual_seed(15)).clamp(max=3.0)
    x[0, 0, [8, 9]] = 5.0          # inside one 16-byte group
    x[0, 1, [700, 3]] = 5.0        # different lanes, the larger index met first by no lane order that matters
    x[0, 2, [3, 515]] = 5.0        # the same lane of the bf16 path (groups 0 and 64), different lanes in fp32
    x[0, 3, :] = 1.0               # a constant row: index 0
    x[0, 4, [998, 999]] = 5.0      # the last group
    x[0, 5, [40, 41]] = 5.0
    x = x.to(_DT[dtype])
    first = R.first_argmax(x.float())
    assert first[0].tolist() == [8, 3, 3, 0, 998, 40] and torch.equal(first, x.float().argmax(-1))
    for tg, want in ((first.clone(), 6), (torch.tensor([[9, 700, 515, 1, 999, 41]]), 0), (torch.tensor([[9, 3, 3, 5, 998, 41]]), 3)):
        c, t = Accuracy(x.cuda(), tg.cuda())
        assert (int(c), int(t)) == (want, 6), (tg.tolist(), int(c), int(t))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_accuracy_counts_and_stats_over_three_appends(dtype):
    from summarymixing_amd.utils.Accuracy import Accuracy, AccuracyStats
    stats = AccuracyStats()
    pooled = [0, 0]
    for i, (B, U, V) in enumerate(((3, 5, 65), (2, 9, 1000), (3, 5, 1003))):
        z, tg, length, pad = R.case(B, U, V, _DT[dtype], seed=20 + i)
        am = R.first_argmax(z.float())
        flip = torch.rand(B, U, generator=torch.Generator().manual_seed(30 + i)) < 0.5
        tg = torch.where(flip, am, tg)                    # about half the rows hit
        keep = R.length_mask(length, B, U)
        hits, kept = R.accuracy(z.float(), tg, keep)
        c, t = Accuracy(z.cuda(), tg.cuda(), length.cuda())
        assert c.is_cuda and (int(c), int(t)) == (int(hits.sum()), int(kept.sum()))
        assert 0 < int(hits.sum()) < int(kept.sum())
        stats.append(z.cuda(), tg.cuda(), length.cuda())
        pooled[0] += int(hits.sum())
        pooled[1] += int(kept.sum())
    assert stats.correct.is_cuda and abs(stats.summarize() - pooled[0] / pooled[1]) < 1e-12
    c, t = Accuracy(z.cuda(), tg.cuda())                  # no length: every row
    assert (int(c), int(t)) == tuple(int(v.sum()) for v in R.accuracy(z.float(), tg, torch.ones(B, U, dtype=torch.bool)))


# ---- 5. the Python surface: reductions, truncation, fused against drop-in, composition ----------------------------------------------
def _surface(fn_gpu, fn_ref, x, want_grad_dtype):
    """value + gradient of a scalar-or-tensor loss through autograd on the GPU, in fp64 and in fp32 on the CPU; the upstream gradient of a
    tensor-valued loss is non-uniform with both signs."""
    outs = []
    for mode in ("gpu", "f64", "f32"):
        xi = (x.cuda() if mode == "gpu" else x.double() if mode == "f64" else x.float()).clone().requires_grad_(True)
        y = fn_gpu(xi) if mode == "gpu" else fn_ref(xi, torch.float64 if mode == "f64" else torch.float32)
        w = torch.linspace(-1.7, 1.3, y.numel()).view(y.shape).to(y) if y.dim() else torch.tensor(-1.7).to(y)
        fin = torch.isfinite(y.detach())
        (torch.where(fin, y, torch.zeros_like(y)) * w).sum().backward()
        outs.append((y.detach().cpu(), xi.grad.detach().cpu()))
    assert outs[0][1].dtype == want_grad_dtype
    return outs


def _surface_check(name, outs, keep, bf16):
    (y, gx), (y64, g64), (y32, g32) = outs
    assert y.shape == y64.shape, (name, y.shape, y64.shape)
    fin = torch.isfinite(y64)
    assert torch.equal(torch.isfinite(y), fin), (name, "non-finite pattern (0 / 0 of an empty utterance)")
    fl, er = _rel(name, "value", y[fin], y64[fin], y32[fin], int(fin.sum()))
    gfl, ger, gw = _grad(name, "grad", gx, g64, g32, keep, int(keep.sum()), bf16)
    return dict(value_floor=fl, value_err=er, g_floor=gfl, g_err=ger, g_err_over_bar=gw)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind,eps", _COMBOS + (("kldiv", 0.0),))
def test_reductions_and_their_gradients(kind, eps, dtype):
    from summarymixing_amd.nnet import losses
    B, U, V = 3, 5, 65
    z, tg, length, pad = R.case(B, U, V, _DT[dtype], seed=40)
    lp = z.double().log_softmax(-1).to(_DT[dtype])
    smooth_kl = kind == "kldiv" and eps > 0
    keep = R.keep_mask("kldiv" if smooth_kl else "nll", tg, length, pad)
    worst = {}
    for reduction in ("mean", "batchmean", "batch", "sum") if smooth_kl else ("mean", "batchmean", "batch", "none"):
        for logits in (False, True):
            if kind == "nll":
                gpu = (lambda x: losses.seq_loss_from_logits(x, tg.cuda(), length.cuda(), eps, kind="nll", reduction=reduction)) if logits else \
                      (lambda x: losses.nll_loss(x, tg.cuda(), length.cuda(), label_smoothing=eps, reduction=reduction))
                ref = lambda x, dt: R.nll_loss(x.log_softmax(-1) if logits else x, tg, length, eps, reduction=reduction, dtype=dt)   # noqa: E731
            else:
                gpu = (lambda x: losses.seq_loss_from_logits(x, tg.cuda(), length.cuda(), eps, pad_idx=pad, kind="kldiv", reduction=reduction)) if logits else \
                      (lambda x: losses.kldiv_loss(x, tg.cuda(), length.cuda(), label_smoothing=eps, pad_idx=pad, reduction=reduction))
                ref = lambda x, dt: R.kldiv_loss(x.log_softmax(-1) if logits else x, tg, length, eps, pad_idx=pad, reduction=reduction, dtype=dt)   # noqa: E731
            name = f"{kind} e={eps} {reduction} {'logits' if logits else 'logprobs'} {dtype}"
            _merge(worst, _surface_check(name, _surface(gpu, ref, z if logits else lp, _DT[dtype]), keep, dtype == "bf16"))
    report(f"seqloss_reductions[{kind},e={eps},{dtype}]", worst)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_truncated_view_is_not_copied_and_its_cut_steps_get_no_gradient(dtype):
    from summarymixing_amd.nnet import losses
    B, U, V = 3, 7, 1000
    z, tg, length, pad = R.case(B, U, V, _DT[dtype], seed=41)
    lp = z.double().log_softmax(-1).to(_DT[dtype])
    short = tg[:, :U - 2].contiguous()                     # U' = U - 2: the scores are cut to a (B, U - 2, V) view with stride U V
    keep = torch.zeros(B, U, dtype=torch.bool)
    keep[:, :U - 2] = R.length_mask(length, B, U - 2)
    for logits in (False, True):
        gpu = (lambda x: losses.seq_loss_from_logits(x, short.cuda(), length.cuda(), 0.1, reduction="batchmean")) if logits else \
              (lambda x: losses.nll_loss(x, short.cuda(), length.cuda(), label_smoothing=0.1, reduction="batchmean"))
        ref = lambda x, dt: R.nll_loss(x.log_softmax(-1) if logits else x, short, length, 0.1, reduction="batchmean", dtype=dt)   # noqa: E731
        w = _surface_check(f"truncated {'logits' if logits else 'logprobs'} {dtype}", _surface(gpu, ref, z if logits else lp, _DT[dtype]), keep,
                           dtype == "bf16")
        report(f"seqloss_truncated[{'logits' if logits else 'logprobs'},{dtype}]", w)
    with pytest.raises(ValueError):
        losses.nll_loss(lp.cuda(), tg[:, :U - 4].cuda())
    # the other way round: longer targets are cut to the scores
    longer = torch.cat([tg, tg[:, :2]], 1)
    a = losses.nll_loss(lp.cuda(), longer.cuda(), length.cuda(), label_smoothing=0.1)
    b = losses.nll_loss(lp.cuda(), tg.cuda(), length.cuda(), label_smoothing=0.1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("kind,eps", _COMBOS)
def test_fused_form_against_the_drop_in_pair(kind, eps):
    """seq_loss_from_logits(z) against kldiv_loss / nll_loss(Softmax(apply_log=True)(z)), both from this repository, in fp32: each within
    its bar of the fp64 chain, so within the sum of the two bars of each other; value and logits gradient."""
    from summarymixing_amd.nnet import losses
    from summarymixing_amd.nnet.activations import Softmax
    B, U, V = 3, 5, 1000
    z, tg, length, pad = R.case(B, U, V, torch.float32, seed=42)
    keep = R.keep_mask(kind, tg, length, pad)
    ls = Softmax(apply_log=True)
    if kind == "nll":
        fused = lambda x: losses.seq_loss_from_logits(x, tg.cuda(), length.cuda(), eps, kind="nll", reduction="mean")          # noqa: E731
        pair = lambda x: losses.nll_loss(ls(x), tg.cuda(), length.cuda(), label_smoothing=eps, reduction="mean")                # noqa: E731
        ref = lambda x, dt: R.nll_loss(x.log_softmax(-1), tg, length, eps, reduction="mean", dtype=dt)                          # noqa: E731
    else:
        fused = lambda x: losses.seq_loss_from_logits(x, tg.cuda(), None, eps, pad_idx=pad, kind="kldiv", reduction="batchmean")   # noqa: E731
        pair = lambda x: losses.kldiv_loss(ls(x), tg.cuda(), None, label_smoothing=eps, pad_idx=pad, reduction="batchmean")        # noqa: E731
        ref = lambda x, dt: R.kldiv_loss(x.log_softmax(-1), tg, None, eps, pad_idx=pad, reduction="batchmean", dtype=dt)           # noqa: E731
    of, op = _surface(fused, ref, z, torch.float32), _surface(pair, ref, z, torch.float32)
    wf = _surface_check(f"fused {kind} e={eps}", of, keep, False)
    wp = _surface_check(f"drop-in pair {kind} e={eps}", op, keep, False)
    report(f"seqloss_fused_vs_pair[{kind},e={eps}]", dict(fused=wf, pair=wp, value_diff=float((of[0][0] - op[0][0]).abs()),
                                                         grad_diff=float((of[0][1] - op[0][1]).abs().max())))
    # return_accuracy: the same pass
    loss, (hits, kept) = losses.seq_loss_from_logits(z.cuda(), tg.cuda(), length.cuda(), eps, pad_idx=pad, kind=kind, return_accuracy=True)
    h, k = R.accuracy(z, tg, keep)
    assert hits.tolist() == h.tolist() and kept.tolist() == k.tolist()


def test_linear_then_fused_loss_input_and_weight_gradients():
    """nnet.linear.Linear(64 -> 1000) + seq_loss_from_logits: dL/dx and the weight's accumulated fp32 .grad against the fp64 chain."""
    from summarymixing_amd.nnet import losses
    from summarymixing_amd.nnet.linear import Linear
    B, U, H, V = 3, 5, 64, 1000
    gen = torch.Generator().manual_seed(43)
    h = torch.randn(B, U, H, generator=gen)
    W = torch.randn(V, H, generator=gen) / 8.0
    bias = torch.randn(V, generator=gen) / 4.0
    _, tg, length, pad = R.case(B, U, V, torch.float32, seed=44)
    keep = R.length_mask(length, B, U)
    lin = Linear(V, input_size=H).cuda()
    with torch.no_grad():
        lin.w.weight.copy_(W)
        lin.w.bias.copy_(bias)
    hg = h.cuda().requires_grad_(True)
    loss = losses.seq_loss_from_logits(lin(hg), tg.cuda(), length.cuda(), 0.1, kind="nll", reduction="batchmean")
    (loss * -1.7).backward()
    res = {}
    for dt in (torch.float64, torch.float32):
        hh, WW, bb = h.to(dt).requires_grad_(True), W.to(dt).requires_grad_(True), bias.to(dt).requires_grad_(True)
        ll = R.nll_loss((hh @ WW.T + bb).log_softmax(-1), tg, length, 0.1, reduction="batchmean", dtype=dt)
        (ll * -1.7).backward()
        res[dt] = (ll.detach(), hh.grad, WW.grad, bb.grad)
    r64, r32 = res[torch.float64], res[torch.float32]
    w = {}
    w["loss_floor"], w["loss_err"] = _rel("linear+loss", "value", loss.detach().cpu().view(1), r64[0].view(1), r32[0].view(1), 1)
    assert lin.w.weight.grad.dtype == torch.float32
    allrows = torch.ones(V, dtype=torch.bool)
    w["dx_floor"], w["dx_err"], w["dx_err_over_bar"] = _grad("linear+loss", "dL/dx", hg.grad.cpu(), r64[1], r32[1], keep, 8, False)
    w["dW_floor"], w["dW_err"], w["dW_err_over_bar"] = _grad("linear+loss", "dL/dW", lin.w.weight.grad.cpu(), r64[2], r32[2], allrows, V, False)
    w["db_floor"], w["db_err"], w["db_err_over_bar"] = _grad("linear+loss", "dL/db", lin.w.bias.grad.cpu().view(V, 1), r64[3].view(V, 1), r32[3].view(V, 1), allrows, V, False)
    report("seqloss_linear_composition", w)


# ---- 6. hipGraph ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_capture_of_forward_and_backward_replays_on_new_inputs(dtype):
    from summarymixing_amd import ops
    from summarymixing_amd.nnet import losses
    B, U, V = 3, 5, 1000
    conf, off, cst = _terms("nll", 0.1, V)
    z0, tg0, length0, _ = R.case(B, U, V, _DT[dtype], seed=50)
    z1, tg1, _, _ = R.case(B, U, V, _DT[dtype], seed=51)
    tg1[2] = tg0[0]                                       # (another utterance becomes the empty one below)
    length1 = torch.tensor([0.0, 1.0, 0.7])
    g0 = torch.randn(B, U, generator=torch.Generator().manual_seed(52))
    g1 = torch.randn(B, U, generator=torch.Generator().manual_seed(53))
    z, tg, ln, g = z0.cuda(), tg0.to(torch.int32).cuda(), length0.cuda(), g0.cuda()

    def step():
        keep_len = losses.mask_count(ln, U)
        row, lse, flags, utt, kept, hits = ops.seqloss_fwd(z, tg, keep_len, -1, conf, off, cst, True)
        dx = ops.seqloss_bwd(z, tg, keep_len, -1, conf, off, lse, g, True)
        return row, lse, utt, kept, hits, dx
    eager = {}
    for k, (zz, tt, ll, gg) in enumerate(((z0, tg0, length0, g0), (z1, tg1, length1, g1))):
        z.copy_(zz), tg.copy_(tt), ln.copy_(ll), g.copy_(gg)
        eager[k] = [t.clone() for t in step()]
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][3], eager[1][3])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k, (zz, tt, ll, gg) in reversed(list(enumerate(((z0, tg0, length0, g0), (z1, tg1, length1, g1))))):
        z.copy_(zz), tg.copy_(tt), ln.copy_(ll), g.copy_(gg)      # in place: the captured addresses
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[k]):
            assert torch.equal(_bits(got), _bits(want)), f"replay on inputs {k}"

"""The CTC head of csrc/ctc.hip stage by stage (through summarymixing_amd.ops), each on inputs made on the CPU and against the fp64
restatement of THE SAME inputs in tests/_ctc_ref.py: the forward variables and -log P that smx_ctc_loss_fwd leaves in the workspace,
the log occupancies alpha + beta - y that smx_ctc_loss_bwd turns them into, the gradient per entry (from the occupancies and the nll
the kernels stored, so that the recursion's rounding is not the gradient kernel's tolerance), and log_softmax_fwd / bwd.

Which test runs which instantiation of ctc_alpha_kernel / ctc_beta_kernel<T, KS> (KS from Lmax = 2 Smax + 1):
  KS = 1   test_lattice_and_gradient_per_cell[127], the transition, edge and reduction tests
  KS = 2   test_lattice_and_gradient_per_cell[128] (Lmax = 257: one state beyond the first seam), test_transition_rules[200],
           test_backward_is_bit_reproducible_across_the_seam, test_padded_leading_dimension_gives_the_same_bits
  KS = 4   test_lattice_and_gradient_per_cell[256]
  KS = 8   test_lattice_and_gradient_per_cell[512]
  KS = 16  test_lattice_and_gradient_per_cell[1024]
  KS = 32  test_lattice_and_gradient_per_cell[2048] and [4095] (the documented maximum: Lmax = 8191, 2 Lmax floats = 64 KB - 8 B of LDS)
each in fp32 and in bf16.

Bars.  Nothing here has a number fixed in advance.  The same recursion is evaluated in fp32 on the CPU (fp32 inputs, fp32
logaddexp / exp); its worst error against fp64 over the utterance, in the metric asserted, is the floor, and the kernel gets
_FLOOR_X x that floor (another summation order, the device's expf / logf) plus _MIN_ULPS fp32 ulps of the quantity's scale, so that
a floor of exactly 0 gives no bar of 0.  With T ~ 5e3 the log-domain values reach ~1e4, where fp32 resolves 1e-3: the floor follows.
bf16 kernels are given bf16-rounded log-probabilities and so is the reference; their gradient bar adds half a bf16 ulp of the
reference entry for the rounding of the output.  Only the workspace cells with t >= T_b or s >= L_b are left out (the kernels never
write them); every test asserts that it compared sum_b T_b L_b cells.  Floors and measured errors go to report()."""
import math

import numpy as np
import pytest
import torch

from tests._ctc_ref import abs_lengths, adjacent_repeats, ctc_grad, ctc_lattice, log_softmax_bwd_ref
from tests._util import report

pytestmark = pytest.mark.gpu

_GSCALE = (0.25, -1.5, 3.0, 0.7)                          # the upstream gradient per utterance: non-uniform, both signs
_FLOOR_X = 4.0                                            # kernel bar = _FLOOR_X * (fp32-on-CPU error against fp64) + ...
_MIN_ULPS = 4.0                                           # ... + _MIN_ULPS * eps32 * (the quantity's scale)
_EPS32 = 2.0 ** -23
_HALF_ULP_BF16 = 2.0 ** -8                                # bf16 keeps 8 significant bits: round-to-nearest moves x by <= 2^-9 * 2^e < 2^-8 |x|
_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


def _draw_targets(B, Smax, V, blank, g):
    labels = torch.tensor([v for v in range(V) if v != blank])
    return labels[torch.randint(0, V - 1, (B, Smax), generator=g)]


def _case(Smax, V, blank, B, seed, dtype, slack=3):
    """Utterance 0 at full target length with T_0 = S + repeats + slack frames (= T); utterance 1 at about half the target length
    (the upper k slots of a thread lie beyond its L) and fewer frames; where B = 3, utterance 2 with an empty target.  The
    log-probabilities are the fp64 log-softmax of unit-scale logits rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    targets = _draw_targets(B, Smax, V, blank, g)
    tgt_len = [Smax, (Smax + 1) // 2, 0][:B]
    need = [s + adjacent_repeats(targets[b], s) for b, s in enumerate(tgt_len)]
    T = max(need[0] + slack, 1)
    in_len = [T] + [min(T, need[1] + slack + 2), max(1, T // 3)][:B - 1]
    lp = torch.randn(B, T, V, generator=g, dtype=torch.float64).log_softmax(-1).to(dtype)
    return lp, targets, in_len, tgt_len


def _run(lp, targets, in_len, tgt_len, blank, gs, pad=0):
    """ops.ctc_fwd, then ops.ctc_bwd on its workspace.  The first B * T * Lmax floats of the workspace are laid out (B, T, Lmax):
    the forward variables after the forward, the log occupancies after the backward.  pad > 0: the log-probabilities are a column
    slice of a (B * T, V + pad) buffer whose other columns hold junk."""
    from summarymixing_amd import ops
    B, T, V = lp.shape
    Lmax = 2 * targets.shape[1] + 1
    lp2 = lp.cuda().view(B * T, V)
    if pad:
        wide = -torch.rand(B * T, V + pad, device="cuda").to(lp.dtype) * 7.0 - 0.01
        wide[:, :V] = lp2
        lp2 = wide[:, :V]
        assert lp2.stride(0) == V + pad
    tg, il, tl = _i32(targets), _i32(in_len), _i32(tgt_len)
    nll, ws = ops.ctc_fwd(lp2, tg, il, tl, B, T, blank)
    n = 4 * B * T * Lmax
    alpha = ws[:n].view(torch.float32).view(B, T, Lmax).cpu()
    G = ops.ctc_bwd(lp2, tg, il, tl, B, T, blank, nll, torch.tensor(gs, dtype=torch.float32).cuda(), ws)
    occ = ws[:n].view(torch.float32).view(B, T, Lmax).cpu()
    torch.cuda.synchronize()
    assert G.dtype == lp.dtype and G.shape == (B * T, V)
    return nll.cpu(), alpha, occ, G.view(B, T, V).cpu()


def _log_domain(name, q, got, r64, r32):
    """|got - ref| / max(1, |ref|) over the finite cells against _FLOOR_X x the same of the fp32 evaluation; the -inf patterns are
    equal.  -> (floor, err, bar)."""
    dead = np.isneginf(r64)
    assert np.array_equal(np.isneginf(r32), dead), (name, q, "the fp32 evaluation of the reference has another -inf pattern")
    assert np.array_equal(np.isneginf(got), dead), (name, q, "-inf pattern differs", int((np.isneginf(got) != dead).sum()))
    live = ~dead
    assert bool(np.isfinite(got[live]).all()), (name, q, "non-finite where the reference is finite")
    if not live.any():
        return 0.0, 0.0, _MIN_ULPS * _EPS32
    den = np.maximum(1.0, np.abs(r64[live]))
    floor = float((np.abs(r32[live].astype(np.float64) - r64[live]) / den).max())
    err = float((np.abs(got[live].astype(np.float64) - r64[live]) / den).max())
    bar = _FLOOR_X * floor + _MIN_ULPS * _EPS32
    assert err <= bar, (name, q, "err", err, "fp32 floor", floor, "bar", bar)
    return floor, err, bar


def _check(name, lp, targets, in_len, tgt_len, blank, out, feasible=None):
    """Every live cell of alpha and of the occupancies, -log P, and the gradient per entry with its structural facts.
    feasible: which utterances must have an alignment (checked on the reference before anything is asserted of the kernels)."""
    B, T, V = lp.shape
    Smax = targets.shape[1]
    nll, alpha, occ, G = out
    bf16 = lp.dtype == torch.bfloat16
    gs = _GSCALE[:B]
    w = {k: 0.0 for k in ("alpha_floor", "alpha_err", "occ_floor", "occ_err", "nll_floor", "nll_err", "g_floor", "g_err", "g_err_over_bar",
                          "rowsum_err_over_bar")}
    cells = {"alpha": 0, "occ": 0}
    for b in range(B):
        Tb, Sb = min(max(int(in_len[b]), 0), T), min(int(tgt_len[b]), Smax)              # the kernels' clamps
        L = 2 * Sb + 1
        a64, n64, o64 = ctc_lattice(lp[b], targets[b], Tb, Sb, blank)
        if feasible is not None:
            assert math.isfinite(n64) == feasible[b], (name, b, "the generated case is not what the test means to run", n64)
        a32, n32, o32 = ctc_lattice(lp[b], targets[b], Tb, Sb, blank, dtype=np.float32)
        # (cells with t >= Tb or s >= L are never written by the kernels: uninitialised by design, not compared)
        a_got, o_got = alpha[b, :Tb, :L].numpy(), occ[b, :Tb, :L].numpy()
        fl, er, _ = _log_domain(name, f"alpha[{b}]", a_got, a64, a32)
        w["alpha_floor"], w["alpha_err"] = max(w["alpha_floor"], fl), max(w["alpha_err"], er)
        fl, er, occ_bar = _log_domain(name, f"occ[{b}]", o_got, o64, o32)
        w["occ_floor"], w["occ_err"] = max(w["occ_floor"], fl), max(w["occ_err"], er)
        cells["alpha"] += a_got.size
        cells["occ"] += o_got.size
        del a64, a32, o32
        # -log P
        nb = float(nll[b])
        if not math.isfinite(n64):
            assert nb == math.inf, (name, b, "nll of an utterance without alignment", nb)
            assert float(G[b].float().abs().sum()) == 0.0, (name, b, "gradient of an utterance without alignment")
            continue
        fl, er = abs(n32 - n64) / max(1.0, abs(n64)), abs(nb - n64) / max(1.0, abs(n64))
        w["nll_floor"], w["nll_err"] = max(w["nll_floor"], fl), max(w["nll_err"], er)
        assert er <= _FLOOR_X * fl + _MIN_ULPS * _EPS32, (name, b, "nll", nb, n64, "fp32 floor", fl)
        # gradient, per entry and absolute, from the occupancies and the nll the kernels stored (given inputs of this stage; the
        # occupancies themselves are held to fp64 above).  Entries are of magnitude <= |gscale|: that is the scale of the minimum.
        g = gs[b]
        G64 = ctc_grad(lp[b], targets[b], Tb, Sb, blank, o_got, nb, g)
        G32 = ctc_grad(lp[b], targets[b], Tb, Sb, blank, o_got, nb, g, dtype=np.float32)
        Gb = G[b].double().numpy()
        floor = float(np.abs(G32.astype(np.float64) - G64).max())
        bar = _FLOOR_X * floor + _MIN_ULPS * _EPS32 * abs(g) + (_HALF_ULP_BF16 * np.abs(G64) if bf16 else 0.0)
        err = np.abs(Gb - G64)
        w["g_floor"], w["g_err"] = max(w["g_floor"], floor), max(w["g_err"], float(err.max()))
        w["g_err_over_bar"] = max(w["g_err_over_bar"], float((err / bar).max()))
        assert bool((err <= bar).all()), (name, b, "gradient: worst err", float(err.max()), "fp32 floor", floor)
        # frames beyond the input length: exact zeros
        assert float(np.abs(Gb[Tb:]).sum()) == 0.0, (name, b, "rows t >= Tb")
        # a column that is neither the blank nor a label of this utterance: gscale * exp(lp), to the fp32 rounding of that
        # expression.  The library is built with -ffast-math: expf(x) is exp2(x log2 e) with the product rounded to fp32, which
        # moves the result by |x| eps32 / 2 relative (|lp| reaches 14 at V = 12288); the exp2 itself, the product with gscale and
        # the margin make up the 4 ulps next to it.
        lp64 = lp[b, :Tb].double().numpy()
        free = sorted(set(range(V)) - {blank} - set(int(c) for c in targets[b, :Sb]))
        if free:
            ref = g * np.exp(lp64[:, free])
            mag = np.where(np.isfinite(lp64[:, free]), np.abs(lp64[:, free]), 0.0)
            fbar = ((4.0 + mag) * _EPS32 + (_HALF_ULP_BF16 if bf16 else 0.0)) * np.abs(ref) + 1e-37
            assert bool((np.abs(Gb[:Tb, free] - ref) <= fbar).all()), (name, b, "columns without a label")
        if not bf16:
            # a live row sums to g (sum_v exp(lp_v) - sum_s exp(occ_s + nll)), and the second sum is 1 on exact occupancies.
            # (i) the first sum is s1, off 1 by the rounding of the given log-probabilities: taken from the inputs in fp64;
            # (ii) each of the V entries is a difference of two terms <= 1, either through expf (and logf) of 2 ulp at most, then
            #      one subtraction and one product: <= 4 eps32 |g| per entry, 4 V eps32 |g| over the row (the sum here is fp64);
            # (iii) the stored occupancies are within occ_bar (asserted above) of fp64 relative to max(1, |occ|); a state that
            #      carries mass has occ + nll = log p_s in [-40, 0] (the lighter ones weigh < L e^-40 together), so |occ| <=
            #      |nll| + 40 and the summed mass moves by occ_bar (|nll| + 40) at most.
            s1 = np.exp(lp64).sum(axis=1)
            rbar = abs(g) * (4.0 * V * _EPS32 + np.abs(s1 - 1.0) + occ_bar * (abs(n64) + 40.0) + L * math.exp(-40.0))
            rs = np.abs(Gb[:Tb].sum(axis=1))
            w["rowsum_err_over_bar"] = max(w["rowsum_err_over_bar"], float((rs / rbar).max()))
            assert bool((rs <= rbar).all()), (name, b, "row sums", float((rs / rbar).max()))
    want = sum(min(max(int(in_len[b]), 0), T) * (2 * min(int(tgt_len[b]), Smax) + 1) for b in range(B))
    assert cells["alpha"] == want and cells["occ"] == want, (name, cells, want)
    report(name, {**w, "cells": want, "bf16": bf16})


# ---- every KS instantiation, both sides of the first seam, the documented maximum -------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Smax,B", [(127, 3), (128, 3), (256, 3), (512, 2), (1024, 2), (2048, 2), (4095, 2)])
def test_lattice_and_gradient_per_cell(Smax, B, dt):
    """V = 8 (7 labels over up to 4095 positions: long occurrence chains, an adjacent repeat every ~7 positions); T follows from
    feasibility.  At Smax = 4095 the backward's LDS guard asks V + Lmax = 8199 <= 16368."""
    V, blank = 8, 0
    lp, targets, in_len, tgt_len = _case(Smax, V, blank, B, 9000 + Smax, _DT[dt])
    out = _run(lp, targets, in_len, tgt_len, blank, _GSCALE[:B])
    _check(f"ctc_stages Smax{Smax} B{B} T{lp.shape[1]} {dt}", lp, targets, in_len, tgt_len, blank, out, feasible=[True] * B)


def _live_bits(x, in_len, tgt_len):
    return [x[b, :in_len[b], :2 * tgt_len[b] + 1].clone() for b in range(x.shape[0])]


def test_backward_is_bit_reproducible_across_the_seam():
    """Two runs at KS = 2 (Smax = 200, the label chains and the blank sum cross s = 256): identical bits."""
    lp, targets, in_len, tgt_len = _case(200, 8, 0, 3, 77, torch.float32)
    runs = [_run(lp, targets, in_len, tgt_len, 0, _GSCALE[:3]) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][3], runs[1][3])
    for k in (1, 2):
        for x, y in zip(_live_bits(runs[0][k], in_len, tgt_len), _live_bits(runs[1][k], in_len, tgt_len)):
            assert torch.equal(x, y)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_padded_leading_dimension_gives_the_same_bits(dt):
    """ldlp > V: a column slice of a (B T, V + 24) buffer whose other columns hold junk, at KS = 2; bit-equal to contiguous rows."""
    lp, targets, in_len, tgt_len = _case(130, 8, 0, 3, 78, _DT[dt])
    a = _run(lp, targets, in_len, tgt_len, 0, _GSCALE[:3])
    b = _run(lp, targets, in_len, tgt_len, 0, _GSCALE[:3], pad=24)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    for k in (1, 2):
        for x, y in zip(_live_bits(a[k], in_len, tgt_len), _live_bits(b[k], in_len, tgt_len)):
            assert torch.equal(x, y)
    _check(f"ctc_stages ldlp V+24 Smax130 {dt}", lp, targets, in_len, tgt_len, 0, b, feasible=[True] * 3)


# ---- transition rules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Smax", [20, 200])                  # KS = 1 and KS = 2
def test_transition_rules_tight_and_one_frame_short(Smax):
    """T_0 = S + repeats: exactly one alignment, found only if alpha and beta take no skip between equal labels (and every other
    skip).  T_0 = S + repeats - 1 >= S: none; raw nll +inf, loss 0 and gradient exactly 0 through nnet.losses.ctc_loss."""
    from summarymixing_amd import ops
    from summarymixing_amd.nnet.losses import ctc_loss
    V, blank, B = 8, 0, 3
    lp, targets, in_len, tgt_len = _case(Smax, V, blank, B, 500 + Smax, torch.float32, slack=0)
    rep = adjacent_repeats(targets[0], Smax)
    assert rep >= 1 and in_len[0] == Smax + rep == lp.shape[1]
    out = _run(lp, targets, in_len, tgt_len, blank, _GSCALE[:B])
    assert math.isfinite(float(out[0][0]))
    _check(f"ctc_stages tight Smax{Smax}", lp, targets, in_len, tgt_len, blank, out, feasible=[True] * B)
    # one frame short (still >= S frames)
    short = [in_len[0] - 1] + in_len[1:]
    assert short[0] >= Smax
    out = _run(lp, targets, short, tgt_len, blank, _GSCALE[:B])
    assert float(out[0][0]) == math.inf
    _check(f"ctc_stages one frame short Smax{Smax}", lp, targets, short, tgt_len, blank, out, feasible=[False, True, True])
    T = lp.shape[1]
    x = lp.cuda().requires_grad_(True)
    in_rel, tg_rel = torch.tensor(short) / T, torch.tensor(tgt_len) / Smax
    assert abs_lengths(T, Smax, in_rel, tg_rel) == (short, tgt_len) or \
        [v.tolist() for v in abs_lengths(T, Smax, in_rel, tg_rel)] == [short, tgt_len]
    loss = ctc_loss(x, targets.cuda(), in_rel.cuda(), tg_rel.cuda(), blank, "none")
    nll_raw, _ = ops.ctc_fwd(lp.cuda().view(B * T, V), _i32(targets), _i32(short), _i32(tgt_len), B, T, blank)
    assert float(nll_raw[0]) == math.inf and float(loss[0].detach()) == 0.0 and float(loss[1].detach()) > 0.0
    loss.sum().backward()
    assert float(x.grad[0].abs().sum()) == 0.0 and float(x.grad[1].abs().sum()) > 0.0


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def _edge_case(B, T, V, Smax, blank, seed, dtype=torch.float32, minus_inf_column=None):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, V, generator=g, dtype=torch.float64)
    if minus_inf_column is not None:
        logits[..., minus_inf_column] = -math.inf
    return logits.log_softmax(-1).to(dtype), _draw_targets(B, Smax, V, blank, g)


def test_a_single_frame():
    """T = 1 with S = 1 (one alignment: the label) and with S = 0 (the blank)."""
    lp, targets = _edge_case(2, 1, 5, 1, 0, 601)
    out = _run(lp, targets, [1, 1], [1, 0], 0, _GSCALE[:2])
    _check("ctc_stages T1", lp, targets, [1, 1], [1, 0], 0, out, feasible=[True, True])
    assert abs(float(out[0][0]) + float(lp[0, 0, targets[0, 0]])) <= 1e-6 and abs(float(out[0][1]) + float(lp[1, 0, 0])) <= 1e-6


def test_an_utterance_without_frames():
    """in_len = 0: no alignment (nll +inf, every gradient row 0, no workspace cell), next to live utterances."""
    lp, targets = _edge_case(3, 9, 6, 3, 0, 602)
    in_len, tgt_len = [9, 0, 6], [3, 2, 1]
    out = _run(lp, targets, in_len, tgt_len, 0, _GSCALE[:3])
    _check("ctc_stages in_len0", lp, targets, in_len, tgt_len, 0, out, feasible=[True, False, True])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_blank_in_the_middle_of_the_vocabulary(dt):
    V = 11
    lp, targets = _edge_case(3, 24, V, 9, V // 2, 603, _DT[dt])
    assert int(targets.min()) < V // 2 < int(targets.max())                               # labels on both sides of the blank
    in_len, tgt_len = [24, 17, 8], [9, 5, 0]
    out = _run(lp, targets, in_len, tgt_len, V // 2, _GSCALE[:3])
    _check(f"ctc_stages blank{V // 2} V{V} {dt}", lp, targets, in_len, tgt_len, V // 2, out, feasible=[True] * 3)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_vocabulary_column_of_minus_infinity(dt):
    """A masked column in every frame.  Utterance 0 does not carry it: finite, and the column's gradient is 0.  Utterance 1 does:
    no alignment, zero.  Utterance 2 has an empty target."""
    V, blank, col = 9, 2, 6
    lp, targets = _edge_case(3, 20, V, 7, blank, 604, _DT[dt], minus_inf_column=col)
    targets[0][targets[0] == col] = 1
    targets[1, 3] = col
    in_len, tgt_len = [20, 18, 5], [7, 6, 0]
    out = _run(lp, targets, in_len, tgt_len, blank, _GSCALE[:3])
    _check(f"ctc_stages -inf column {dt}", lp, targets, in_len, tgt_len, blank, out, feasible=[True, False, True])
    assert float(out[3][:, :, col].float().abs().sum()) == 0.0 and not bool(out[3].isnan().any())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_the_largest_vocabulary_the_backward_accepts(dt):
    """V = 12288: the gradient kernel's V floats of LDS, 48 passes of its 256-thread column loops."""
    V = 12288
    lp, targets = _edge_case(2, 7, V, 3, 0, 605, _DT[dt])
    targets[0] = torch.tensor([V - 1, V - 1, 4097])
    in_len, tgt_len = [7, 5], [3, 2]
    out = _run(lp, targets, in_len, tgt_len, 0, _GSCALE[:2])
    _check(f"ctc_stages V{V} {dt}", lp, targets, in_len, tgt_len, 0, out, feasible=[True, True])


def test_backward_refuses_what_does_not_fit_the_lds():
    """V = 12289, and V + Lmax one float over the budget (V + Lmax <= 16368): the library's error from the host-side checks, before
    any launch.  One float under the budget runs."""
    from summarymixing_amd import ops

    def bwd(V, Smax):
        lp2 = torch.zeros(1, V, device="cuda")
        tg = torch.ones(1, Smax, dtype=torch.int32, device="cuda")
        one = _i32([1])
        nll, ws = ops.ctc_fwd(lp2, tg, one, _i32([Smax]), 1, 1, 0)
        return ops.ctc_bwd(lp2, tg, one, _i32([Smax]), 1, 1, 0, nll, torch.ones(1, device="cuda"), ws)

    with pytest.raises(RuntimeError, match="smx_ctc_loss_bwd"):
        bwd(12289, 2)
    with pytest.raises(RuntimeError, match="do not fit"):
        bwd(12288, 2040)                                  # V + Lmax = 12288 + 4081 = 16369
    g = bwd(12288, 2039)                                  # 16367: runs (one frame for 2039 labels: no alignment, zeros)
    torch.cuda.synchronize()
    assert float(g.abs().sum()) == 0.0


def test_targets_without_a_column():
    """targets of shape (B, 0): ctc_loss treats every target as empty, -sum_{t < T_b} lp[t, blank] as torch does."""
    from summarymixing_amd.nnet.losses import ctc_loss
    B, T, V, blank = 3, 9, 6, 2
    lp, _ = _edge_case(B, T, V, 1, blank, 606)
    in_rel = torch.tensor([1.0, 0.5, 0.7])
    in_len = (in_rel * T).round().long()
    x = lp.cuda().requires_grad_(True)
    loss = ctc_loss(x, torch.zeros(B, 0, dtype=torch.long).cuda(), in_rel.cuda(), torch.ones(B).cuda(), blank, "none")
    (loss * torch.tensor(_GSCALE[:B]).cuda()).sum().backward()
    for b in range(B):
        ref = -float(lp[b, :in_len[b], blank].double().sum())
        assert abs(float(loss[b]) - ref) <= _MIN_ULPS * _EPS32 * T * max(1.0, abs(ref)), (b, float(loss[b]), ref)
        # the blank carries the whole mass: G = gscale (exp(lp) - [v = blank])
        G = _GSCALE[b] * (lp[b].double().exp() - torch.nn.functional.one_hot(torch.tensor(blank), V))
        G[in_len[b]:] = 0.0
        # alpha and beta are running sums of <= T terms, each addition rounding by <= eps32 |ref|; alpha + beta - y, the shift by
        # the nll and the two expf add a few more: (T + 8) eps32 max(1, |ref|) on the log of the mass, which is 1
        assert float((x.grad[b].cpu().double() - G).abs().max()) <= (T + 8) * _EPS32 * max(1.0, abs(ref)) * abs(_GSCALE[b]), b


# ---- reductions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["sum", "batch", "none"])
def test_reductions_scale_the_gradient(reduction):
    """Loss and input gradient of nnet.losses.ctc_loss against the same reduction of the fp64 per-utterance reference; the floor is
    the whole reference in fp32.  "batch" and "none" return a vector: it is weighted by _GSCALE and summed."""
    from summarymixing_amd.nnet.losses import ctc_loss
    B, T, V, S, blank = 4, 26, 7, 6, 3
    lp, targets = _edge_case(B, T, V, S, blank, 700)
    in_rel, tg_rel = torch.tensor([1.0, 0.7, 0.9, 0.5]), torch.tensor([1.0, 0.5, 0.34, 0.17])
    in_len, tgt_len = abs_lengths(T, S, in_rel, tg_rel)
    assert int(tgt_len.min()) >= 1
    wts = torch.tensor(_GSCALE, dtype=torch.float64)
    gsc = {"sum": torch.ones(B, dtype=torch.float64), "batch": wts / tgt_len, "none": wts}[reduction]   # d loss / d nll_b
    x = lp.cuda().requires_grad_(True)
    out = ctc_loss(x, targets.cuda(), in_rel.cuda(), tg_rel.cuda(), blank, reduction)
    assert out.shape == (() if reduction == "sum" else (B,))
    loss = out if reduction == "sum" else (out * wts.float().cuda()).sum()
    loss.backward()
    tot = {np.float64: 0.0, np.float32: 0.0}
    l_scale = 0.0
    G = {np.float64: [], np.float32: []}
    for b in range(B):
        for dt_ in (np.float64, np.float32):
            _, nll, occ = ctc_lattice(lp[b], targets[b], int(in_len[b]), int(tgt_len[b]), blank, dtype=dt_)
            assert math.isfinite(nll)
            tot[dt_] += float(gsc[b]) * nll
            l_scale += abs(float(gsc[b]) * nll) / 2           # (both passes add it: the sum of |weight * nll_b|, terms of both signs)
            G[dt_].append(ctc_grad(lp[b], targets[b], int(in_len[b]), int(tgt_len[b]), blank, occ, nll, float(gsc[b]), dtype=dt_))
    G64, G32 = np.stack(G[np.float64]), np.stack(G[np.float32]).astype(np.float64)
    scale = float(gsc.abs().max())                        # an entry of utterance b is of magnitude <= |d loss / d nll_b|
    l_floor, l_err = abs(tot[np.float32] - tot[np.float64]), abs(float(loss) - tot[np.float64])
    g_floor, g_err = float(np.abs(G32 - G64).max()), float(np.abs(x.grad.cpu().double().numpy() - G64).max())
    report(f"ctc_loss reduction {reduction}", {"loss_floor": l_floor, "loss_err": l_err, "g_floor": g_floor, "g_err": g_err})
    assert l_err <= _FLOOR_X * l_floor + _MIN_ULPS * _EPS32 * l_scale, (l_err, l_floor)
    assert g_err <= _FLOOR_X * g_floor + _MIN_ULPS * _EPS32 * scale, (g_err, g_floor)


# ---- log-softmax ------------------------------------------------------------------------------------------------------------------
# no N is a multiple of the 4 rows of a block; V = 1, both sides of one 64-lane trip, 16 and 79 trips
_LSM_SHAPES = [(1, 1), (5, 63), (7, 64), (6, 65), (9, 1000), (3, 5000)]


def _strided(x, pad=24):
    wide = torch.full((x.shape[0], x.shape[1] + pad), 3.0, dtype=x.dtype, device=x.device)
    wide[:, :x.shape[1]] = x
    return wide[:, :x.shape[1]]


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("scale", ["unit", "large"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,V", _LSM_SHAPES)
def test_log_softmax_forward(N, V, dt, scale, strided):
    """Against float64 torch.log_softmax of the same (rounded) input, per entry.  Floor: torch's fp32 log_softmax on the CPU; the
    scale of an entry is max(1, |y|).  bf16 adds the rounding of the output.  Large inputs (1e4 in fp32, 30 in bf16): the maximum
    is subtracted before expf, so nothing overflows, and every row's logsumexp(y) is 0 to the bar of its entries (in bf16: to the
    mean output rounding sum_v p_v 2^-8 |y_v| on top)."""
    from summarymixing_amd import ops
    dtype = _DT[dt]
    g = torch.Generator().manual_seed(800 + N + V)
    mag = 1.0 if scale == "unit" else (1e4 if dt == "f32" else 30.0)
    x = (torch.randn(N, V, generator=g) * mag).to(dtype)
    xc = _strided(x.cuda()) if strided else x.cuda()
    y = ops.log_softmax_fwd(xc)
    torch.cuda.synchronize()
    assert y.dtype == dtype and y.shape == (N, V) and y.is_contiguous()
    y = y.cpu().double()
    ref = torch.log_softmax(x.double(), -1)
    f32 = torch.log_softmax(x.float(), -1).double()
    assert bool(torch.isfinite(y).all())
    den = ref.abs().clamp(min=1.0)
    floor = float(((f32 - ref).abs() / den).max())
    bar = (_FLOOR_X * floor + _MIN_ULPS * _EPS32) * den + (_HALF_ULP_BF16 * ref.abs() if dt == "bf16" else 0.0)
    err = (y - ref).abs()
    lse = torch.logsumexp(y, -1).abs()
    lse_bar = (_FLOOR_X * floor + _MIN_ULPS * _EPS32) * den.max(dim=1).values
    if dt == "bf16":
        lse_bar = lse_bar + _HALF_ULP_BF16 * (ref.exp() * ref.abs()).sum(-1)
    report(f"log_softmax_fwd ({N},{V}) {dt} {scale}" + (" strided" if strided else ""),
           {"floor": floor, "err": float((err / den).max()), "err_over_bar": float((err / bar).max()), "lse_err": float(lse.max()),
            "lse_bar": float(lse_bar.min())})
    assert bool((err <= bar).all()), (float((err / bar).max()), floor)
    assert bool((lse <= lse_bar).all()), (float(lse.max()), float(lse_bar.min()))


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,V", _LSM_SHAPES)
def test_log_softmax_backward(N, V, dt, strided):
    """dX = dY - exp(Y) sum dY with a dense upstream gradient, from given (rounded) Y and dY; the formula is float64 autograd's
    (tests/test_ctc_cpu.py).  Floor: the formula in fp32 on the CPU, absolute; the scale is the largest |dX| of the case."""
    from summarymixing_amd import ops
    dtype = _DT[dt]
    g = torch.Generator().manual_seed(900 + N + V)
    yv = torch.log_softmax(torch.randn(N, V, generator=g, dtype=torch.float64) * 2.0, -1).to(dtype)
    dy = torch.randn(N, V, generator=g).to(dtype)
    yc, dc = (yv.cuda(), dy.cuda()) if not strided else (_strided(yv.cuda()), _strided(dy.cuda(), pad=8))
    dx = ops.log_softmax_bwd(dc, yc)
    torch.cuda.synchronize()
    assert dx.dtype == dtype and dx.shape == (N, V)
    dx = dx.cpu().double().numpy()
    ref = log_softmax_bwd_ref(dy, yv)
    f32 = log_softmax_bwd_ref(dy, yv, dtype=np.float32).astype(np.float64)
    floor = float(np.abs(f32 - ref).max())
    bar = _FLOOR_X * floor + _MIN_ULPS * _EPS32 * float(np.abs(ref).max()) + (_HALF_ULP_BF16 * np.abs(ref) if dt == "bf16" else 0.0)
    err = np.abs(dx - ref)
    report(f"log_softmax_bwd ({N},{V}) {dt}" + (" strided" if strided else ""),
           {"floor": floor, "err": float(err.max()), "err_over_bar": float((err / np.maximum(bar, 1e-300)).max())})
    assert bool((err <= bar).all()), (float(err.max()), floor)

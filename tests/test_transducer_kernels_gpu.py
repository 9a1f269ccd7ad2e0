"""The transducer kernels of csrc/transducer.hip stage by stage (through summarymixing_amd.ops), each on inputs made on the CPU and
against the fp64 restatement of THE SAME inputs in tests/_rnnt_ref.py, so that one stage's rounding is not another stage's
tolerance: the lattice DP per cell (every KS instantiation, the U + 1 = 2048 limit, U = 0), the row statistics and the logit
gradient of the drop-in and of the fused (logit-free GEMM) path off blank 0 and across column tiles, and the joint.

Bars.  The DP and the joint have fixed bars, derived where they are asserted.  The statistics and the logit gradient are measured
against the reference: the same quantity is evaluated in fp32 on the CPU (fp32 product, fp32 logsumexp / exp) and its worst
absolute error against fp64 over the case is the floor; the kernel gets 4 x that floor (another summation order, the device
library's expf / logf).  With bf16 operands the fused path never rounds a logit to bf16, so it is held to the same
fp32-accumulation bar against the fp64 product of the bf16-rounded operands.  Floors and errors go to report()."""
import pytest
import torch

from tests._rnnt_ref import joint_ref, lattice, logit_grad, row_stats
from tests._util import report

pytestmark = pytest.mark.gpu

_GSCALE = (0.25, -1.5, 3.0, 0.7)                          # the upstream gradient per utterance: non-uniform, both signs
_FLOOR_X = 4.0                                            # kernel bar = _FLOOR_X * (fp32-on-CPU error against fp64)


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


# ---- B1: lattice DP -----------------------------------------------------------------------------------------------------------
def _dp_lengths(B, T, U):
    """A full-length utterance, then a short one; where U > 0 one utterance has U_b = 0."""
    tl, ul = [T] * B, [U] * B
    if B == 2:
        tl[1], ul[1] = max(1, (2 * T) // 3), 0
    elif B > 2:
        tl[1], ul[1] = max(1, (2 * T) // 3), (U + 1) // 2
        ul[2] = 0
        if B > 3:
            tl[3] = max(1, T // 4)
    return tl, ul


def _emissions(B, T, U, seed, kind="softmax"):
    """fp32 per-cell log emissions, drawn directly: two columns of the log-softmax of unit-scale normal logits over 32 classes,
    or uniform in [-3, 0] (not normalised)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "softmax":
        lp = torch.randn(B, T, U + 1, 32, generator=g, dtype=torch.float64).log_softmax(-1).float()
        return lp[..., 0].contiguous(), lp[..., 1].contiguous()
    return (-3.0 * torch.rand(B, T, U + 1, generator=g)).float(), (-3.0 * torch.rand(B, T, U + 1, generator=g)).float()


def _check_dp(name, lpb, lpy, in_len, tgt_len):
    from summarymixing_amd import ops
    B, T, U1 = lpb.shape
    gs = torch.tensor(_GSCALE[:B])
    nll, alpha = ops.transducer_loss_fwd(lpb.cuda().view(-1), lpy.cuda().view(-1), _i32(in_len), _i32(tgt_len), B, T, U1)
    gb, gy = ops.transducer_loss_bwd(lpb.cuda().view(-1), lpy.cuda().view(-1), alpha, gs.cuda(), _i32(in_len), _i32(tgt_len), B, T, U1)
    torch.cuda.synchronize()
    nl64 = alpha[B * T * U1:].cpu()
    alpha = alpha[:B * T * U1].view(B, T, U1).cpu()
    nll, gb, gy = nll.cpu(), gb.view(B, T, U1).cpu(), gy.view(B, T, U1).cpu()
    worst = {"alpha": 0.0, "nll": 0.0, "g": 0.0}
    cells = live = 0
    for b in range(B):
        Tb, Ub = min(max(int(in_len[b]), 1), T), min(max(int(tgt_len[b]), 0), U1 - 1)      # the kernels' clamps
        a_ref, nl_ref, ob, oy = lattice(lpb[b], lpy[b], Tb, Ub)
        a_ref, ob, oy = torch.from_numpy(a_ref), torch.from_numpy(ob), torch.from_numpy(oy)
        # alpha: both sides fp64; a cell is reached through at most T + U ~ 2e3 additions (2e3 * 1.1e-16 = 2e-13 relative drift)
        ea = (alpha[b, :Tb, :Ub + 1] - a_ref).abs() / a_ref.abs().clamp(min=1.0)
        worst["alpha"] = max(worst["alpha"], float(ea.max()))
        assert float(ea.max()) <= 1e-11, (name, b, "alpha", float(ea.max()))
        assert abs(float(nl64[b]) - nl_ref) <= 1e-11 * max(1.0, abs(nl_ref)), (name, b, "-log P (fp64)")
        # nll: the fp32 rounding of the fp64 value
        en = abs(float(nll[b]) - nl_ref) / abs(nl_ref)
        worst["nll"] = max(worst["nll"], en)
        assert en <= 2.0 ** -23, (name, b, "nll", float(nll[b]), nl_ref)
        # g = -gscale * occupancy: the exponent is formed in fp64 and rounded once to fp32
        for got, occ, q in ((gb, ob, "g_blank"), (gy, oy, "g_y")):
            ref = -float(gs[b]) * occ
            err = (got[b, :Tb, :Ub + 1].double() - ref).abs()
            bar = 1e-6 * ref.abs() + 1e-37
            assert bool((err <= bar).all()), (name, b, q, float((err / bar).max()))
            big = occ > 1e-30
            worst["g"] = max(worst["g"], float((err[big] / ref.abs()[big]).max()) if bool(big.any()) else 0.0)
        # exactly 0 outside t < T_b, u <= U_b
        for got in (gb, gy):
            assert float(got[b, Tb:].abs().sum()) == 0.0 and float(got[b, :, Ub + 1:].abs().sum()) == 0.0, (name, b, "padding")
        assert float(gy[b, :Tb, Ub].abs().sum()) == 0.0, (name, b, "g_y at u = U_b")
        # the condition that keeps the relative check from being vacuous (on the reference alone)
        cells += Tb * (2 * Ub + 1)
        live += int((ob > 1e-30).sum()) + int((oy[:, :Ub] > 1e-30).sum())
    assert live >= 0.5 * cells, (name, "reference occupancies above 1e-30", live, cells)
    report(name, {"alpha_rel": worst["alpha"], "nll_rel": worst["nll"], "g_rel": worst["g"], "live_fraction": live / cells})


@pytest.mark.parametrize("B,T,U", [(3, 50, 9), (2, 40, 300), (2, 7, 600), (2, 6, 1100), (1, 3, 2047), (3, 300, 5), (2, 1, 5), (2, 5, 0),
                                   (4, 120, 40)])
def test_lattice_dp_per_cell(B, T, U):
    """alpha, -log P, g_blank and g_y of every valid cell; KS = 1 (U + 1 <= 256), 2, 4 (U = 600), 8 (U = 1100, 2047)."""
    lpb, lpy = _emissions(B, T, U, 40 + T + U)
    tl, ul = _dp_lengths(B, T, U)
    _check_dp(f"transducer_dp B{B} T{T} U{U}", lpb, lpy, tl, ul)


def test_lattice_dp_per_cell_unnormalised_emissions():
    B, T, U = 3, 50, 9
    lpb, lpy = _emissions(B, T, U, 77, kind="uniform")
    tl, ul = _dp_lengths(B, T, U)
    _check_dp("transducer_dp uniform B3 T50 U9", lpb, lpy, tl, ul)


def test_lattice_dp_clamps_the_lengths():
    """in_len 0 -> 1 and above T -> T; tgt_len above U -> U and below 0 -> 0 (utt_lengths)."""
    B, T, U = 3, 50, 9
    lpb, lpy = _emissions(B, T, U, 78)
    _check_dp("transducer_dp clamps B3 T50 U9", lpb, lpy, [0, T + 7, 20], [U + 4, 3, -2])


def test_lattice_dp_refuses_more_than_2048_label_columns():
    from summarymixing_amd import ops
    B, T, U1 = 1, 1, 2049
    lp = torch.zeros(B * T * U1, device="cuda")
    one, zero = _i32([1]), _i32([0])
    with pytest.raises(RuntimeError):
        ops.transducer_loss_fwd(lp, lp, one, zero, B, T, U1)
    alpha = torch.zeros(B * T * U1 + B, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.transducer_loss_bwd(lp, lp, alpha, torch.ones(B, device="cuda"), one, zero, B, T, U1)


# ---- B2 - B4: row statistics and logit gradient ---------------------------------------------------------------------------------
_LATTICES = {"rows256": (2, 8, 15), "rows210": (3, 5, 13)}   # (B, T, U): two full 128-row tiles / a ragged second tile


def _targets(B, U, V, blank, tile, g):
    """Labels off the blank column; the first and the last column of every `tile`-wide column tile and column V - 1 are the label
    of some row."""
    must = [V - 1]
    for v0 in range(0, V, tile):
        must += [v0, min(v0 + tile - 1, V - 1)]
    must = sorted({c for c in must if c != blank})
    assert len(must) <= B * U
    t = torch.randint(0, V - 1, (B * U,), generator=g)
    t = t + (t >= blank)
    t[torch.randperm(B * U, generator=g)[:len(must)]] = torch.tensor(must)
    assert not bool((t == blank).any())
    return t.view(B, U)


def _blanks(V):
    return sorted({0, V // 2, V - 1})


def _stats32(z32, targets, blank):
    """row_stats in fp32 on the CPU: what fp32 arithmetic can give on these inputs (the floor)."""
    B, T, U1, V = z32.shape
    lse = torch.logsumexp(z32, -1)
    lpb = z32[..., blank] - lse
    lpy = torch.zeros_like(lse)
    idx = targets.long().view(B, 1, U1 - 1, 1).expand(B, T, U1 - 1, 1)
    lpy[:, :, :U1 - 1] = z32[:, :, :U1 - 1].gather(3, idx).squeeze(3) - lse[:, :, :U1 - 1]
    return lse, lpb, lpy


def _check_stats(name, got, ref64, ref32):
    out = {}
    for q, a, r, f in zip(("lse", "lp_blank", "lp_y"), got, ref64, ref32):
        a, r, f = a.detach().cpu().double().view(-1), r.reshape(-1), f.double().reshape(-1)
        fin = torch.isfinite(r)
        assert torch.equal(a[~fin], r[~fin]), (name, q, "non-finite entries differ")
        assert bool(torch.isfinite(a[fin]).all()), (name, q, "non-finite where the reference is finite")
        if not bool(fin.any()):                           # (a blank in the -inf column: every lp_blank is -inf, checked above)
            continue
        floor = float((f[fin] - r[fin]).abs().max())
        err = float((a[fin] - r[fin]).abs().max())
        out[q + "_floor"], out[q + "_err"] = floor, err
    report(name, out)
    for q in ("lse", "lp_blank", "lp_y"):
        if q + "_err" in out:
            assert out[q + "_err"] <= _FLOOR_X * out[q + "_floor"], (name, q, out[q + "_err"], out[q + "_floor"])


def _coefficients(lse64, lpb64, lpy64, B, T, U):
    """Per-row gradient coefficients of a real lattice from the reference statistics, cast to fp32: (lse, g_blank, g_y)."""
    tl, ul = _dp_lengths(B, T, U)
    if B == 2:
        ul[1] = (U + 1) // 2                              # (a partial target here; U_b = 0 is the DP's business)
    gb, gy = torch.zeros(B, T, U + 1, dtype=torch.float64), torch.zeros(B, T, U + 1, dtype=torch.float64)
    for b in range(B):
        _, _, ob, oy = lattice(lpb64[b], lpy64[b], tl[b], ul[b])
        gb[b, :tl[b], :ul[b] + 1] = -_GSCALE[b] * torch.from_numpy(ob)
        gy[b, :tl[b], :ul[b] + 1] = -_GSCALE[b] * torch.from_numpy(oy)
    return lse64.float(), gb.float(), gy.float()


def _grad32(z32, targets, blank, lse, gb, gy):
    """logit_grad in fp32 on the CPU (the floor)."""
    B, T, U1, V = z32.shape
    dz = -torch.exp(z32 - lse.unsqueeze(-1)) * (gb + gy).unsqueeze(-1)
    dz[..., blank] += gb
    idx = targets.long().view(B, 1, U1 - 1, 1).expand(B, T, U1 - 1, 1)
    dz[:, :, :U1 - 1].scatter_add_(3, idx, gy[:, :, :U1 - 1].unsqueeze(-1))
    return dz


def _check_grad(name, dz, dz64, dz32, gb, gy, bf16_out):
    """Elementwise, absolute, scaled by the row's |g_b| + |g_y|; rows with g_b = g_y = 0 are exact zeros."""
    V = dz64.shape[-1]
    dz, dz64, dz32 = dz.detach().cpu().double().view(-1, V), dz64.reshape(-1, V), dz32.double().reshape(-1, V)
    scale = (gb.double().abs() + gy.double().abs()).reshape(-1, 1)
    live = scale.view(-1) > 0
    assert bool(live.any()) and float(dz[~live].abs().sum()) == 0.0, (name, "rows without gradient")
    floor = float(((dz32 - dz64).abs() / scale)[live].max())
    bar = _FLOOR_X * floor * scale + (2.0 ** -8 * dz64.abs() if bf16_out else 0.0)
    err = (dz - dz64).abs()
    worst = float((err / scale)[live].max())
    report(name, {"dz_floor": floor, "dz_err": worst, "bf16_out": bf16_out})
    assert bool((err[live] <= bar[live]).all()), (name, "worst err / (|gb| + |gy|)", worst, "fp32 floor", floor)


def _logits(B, T, U, V, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, U + 1, V, generator=g) * 2.0).to(dtype), g


def _strided(z2, pad=7):
    wide = torch.full((z2.shape[0], z2.shape[1] + pad), 3.0, dtype=z2.dtype, device=z2.device)
    wide[:, :z2.shape[1]] = z2
    return wide[:, :z2.shape[1]]


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [2, 17, 64, 65, 1000])
def test_row_stats_dropin(V, dtype, strided):
    from summarymixing_amd import ops
    B, T, U = _LATTICES["rows210"]
    z, g = _logits(B, T, U, V, dtype, 500 + V)
    z2 = z.cuda().view(-1, V)
    z2 = _strided(z2) if strided else z2
    for blank in _blanks(V):
        targets = _targets(B, U, V, blank, 64, g)
        got = ops.transducer_row_stats(z2, _i32(targets), B, T, U + 1, blank)
        _check_stats(f"transducer_row_stats V{V} {'bf16' if dtype == torch.bfloat16 else 'f32'} blank{blank}"
                     + (" strided" if strided else ""), got, row_stats(z, targets, blank), _stats32(z.float(), targets, blank))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_row_stats_dropin_with_a_column_of_minus_infinity(dtype):
    """A masked-out class: lse stays finite; lp is -inf exactly where the reference has it (the blank, then a label)."""
    from summarymixing_amd import ops
    B, T, U = _LATTICES["rows210"]
    V = 65
    z, g = _logits(B, T, U, V, dtype, 601)
    z[..., 64] = float("-inf")
    for blank in (64, 0):
        targets = _targets(B, U, V, blank, 64, g)
        got = ops.transducer_row_stats(z.cuda().view(-1, V), _i32(targets), B, T, U + 1, blank)
        ref = row_stats(z, targets, blank)
        assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isinf(ref[1] if blank == 64 else ref[2]).any())
        _check_stats(f"transducer_row_stats -inf column blank{blank}", got, ref, _stats32(z.float(), targets, blank))


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [2, 17, 64, 65, 1000])
def test_logit_grad_dropin(V, dtype, strided):
    from summarymixing_amd import ops
    B, T, U = _LATTICES["rows210"]
    z, g = _logits(B, T, U, V, dtype, 700 + V)
    z2 = z.cuda().view(-1, V)
    z2 = _strided(z2) if strided else z2
    for blank in _blanks(V):
        targets = _targets(B, U, V, blank, 64, g)
        lse, gb, gy = _coefficients(*row_stats(z, targets, blank), B, T, U)
        dz = ops.transducer_logit_grad(z2, _i32(targets), lse.cuda().view(-1), gb.cuda().view(-1), gy.cuda().view(-1), B, T, U + 1, blank)
        assert dz.dtype == dtype and dz.shape == (B * T * (U + 1), V)
        _check_grad(f"transducer_logit_grad V{V} {'bf16' if dtype == torch.bfloat16 else 'f32'} blank{blank}"
                    + (" strided" if strided else ""), dz, logit_grad(z, targets, blank, lse, gb, gy),
                    _grad32(z.float(), targets, blank, lse, gb, gy), gb, gy, dtype == torch.bfloat16)


def _fused_operands(lat, J, V, dtype, seed):
    """H (rows, J), W (V, J) in `dtype`, an fp32 bias; logits of about unit scale."""
    B, T, U = _LATTICES[lat]
    g = torch.Generator().manual_seed(seed)
    H = (torch.randn(B * T * (U + 1), J, generator=g) * 0.5).to(dtype)
    W = (torch.randn(V, J, generator=g) * (3.0 / J ** 0.5)).to(dtype)
    bias = torch.rand(V, generator=g) - 0.5
    return B, T, U, H, W, bias, g


def _products(H, W, bias, B, T, U):
    """The fp64 product of the operands as they are (bf16-rounded where they are bf16; never rounded to bf16 afterwards) and the
    same in fp32 on the CPU."""
    z64, z32 = H.double() @ W.double().t(), H.float() @ W.float().t()
    if bias is not None:
        z64, z32 = z64 + bias.double(), z32 + bias
    return z64.view(B, T, U + 1, -1), z32.view(B, T, U + 1, -1)


_FUSED = dict(argnames="V,J,dtype,lat", ids=lambda v: {torch.float32: "f32", torch.bfloat16: "bf16"}.get(v, str(v)),
              argvalues=[(V, J, dt, lat) for V in (4, 36, 128, 132, 256, 1000) for J in (64, 128, 640, 1088)
                         for dt in (torch.float32, torch.bfloat16) for lat in ("rows256", "rows210")])


@pytest.mark.parametrize(**_FUSED)
def test_gemm_stats_fused(V, J, dtype, lat):
    from summarymixing_amd import ops
    B, T, U, H, W, bias, g = _fused_operands(lat, J, V, dtype, 800 + V + J)
    Hc, Wc = H.cuda(), W.cuda()
    for bv in (None, bias):
        z64, z32 = _products(H, W, bv, B, T, U)
        for blank in _blanks(V):
            targets = _targets(B, U, V, blank, 128, g)
            got = ops.transducer_gemm_stats(Hc, Wc, bv.cuda() if bv is not None else None, _i32(targets), B, T, U + 1, blank)
            _check_stats(f"transducer_gemm_stats V{V} J{J} {'bf16' if dtype == torch.bfloat16 else 'f32'} {lat} blank{blank}"
                         + (" bias" if bv is not None else ""), got, row_stats(z64, targets, blank), _stats32(z32, targets, blank))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gemm_stats_fused_merges_very_unequal_column_tiles(dtype):
    """Three column tiles, the first shifted by -60 and the last by +40 (through the bias): the (max, sum) merge meets partial sums
    that underflow against the row's maximum; the blank sits in the lowest tile, labels in all three."""
    from summarymixing_amd import ops
    V, J = 384, 64
    B, T, U, H, W, bias, g = _fused_operands("rows210", J, V, dtype, 901)
    bias[:128] -= 60.0
    bias[256:] += 40.0
    z64, z32 = _products(H, W, bias, B, T, U)
    for blank in (5, 300):
        targets = _targets(B, U, V, blank, 128, g)
        got = ops.transducer_gemm_stats(H.cuda(), W.cuda(), bias.cuda(), _i32(targets), B, T, U + 1, blank)
        _check_stats(f"transducer_gemm_stats unequal tiles {'bf16' if dtype == torch.bfloat16 else 'f32'} blank{blank}", got,
                     row_stats(z64, targets, blank), _stats32(z32, targets, blank))


_SENTINEL = 1234.5


@pytest.mark.parametrize(**_FUSED)
def test_gemm_grad_fused(V, J, dtype, lat):
    """The recomputed-tile gradient from the reference's lse, g_blank, g_y, over row ranges as the backward's utterance groups pass
    them, into a column slice of a wider buffer whose other entries must keep their bits."""
    from summarymixing_amd import ops
    B, T, U, H, W, bias, g = _fused_operands(lat, J, V, dtype, 1000 + V + J)
    Hc, Wc = H.cuda(), W.cuda()
    rows, per = B * T * (U + 1), T * (U + 1)
    ranges = [(0, rows), (per, rows - per - 5), (37, rows - 37 - 5)]      # whole; from utterance 1, short of the end; off every tile edge
    k = 0
    for bv in (None, bias):
        z64, z32 = _products(H, W, bv, B, T, U)
        for blank in _blanks(V):
            targets = _targets(B, U, V, blank, 128, g)
            lse, gb, gy = _coefficients(*row_stats(z64, targets, blank), B, T, U)
            dz64 = logit_grad(z64, targets, blank, lse, gb, gy).view(rows, V)
            dz32 = _grad32(z32, targets, blank, lse, gb, gy).view(rows, V)
            row0, n = ranges[k % 3]
            k += 1
            Vp = (V + 63) // 64 * 64 + 64
            buf = torch.full((n + 3, Vp), _SENTINEL, dtype=dtype, device="cuda")
            ops.transducer_gemm_grad(Hc, Wc, bv.cuda() if bv is not None else None, _i32(targets), lse.cuda().view(-1),
                                     gb.cuda().view(-1), gy.cuda().view(-1), B, T, U + 1, blank, row0, n, buf[:n, :V])
            name = (f"transducer_gemm_grad V{V} J{J} {'bf16' if dtype == torch.bfloat16 else 'f32'} {lat} blank{blank} row0 {row0}"
                    + (" bias" if bv is not None else ""))
            assert bool((buf[:n, V:] == _SENTINEL).all()) and bool((buf[n:] == _SENTINEL).all()), (name, "wrote outside (nrows, V)")
            _check_grad(name, buf[:n, :V], dz64[row0:row0 + n], dz32[row0:row0 + n], gb.view(-1)[row0:row0 + n],
                        gy.view(-1)[row0:row0 + n], dtype == torch.bfloat16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gemm_grad_fused_stores_exact_zeros_for_a_tile_without_gradient(dtype):
    from summarymixing_amd import ops
    V, J = 132, 128
    B, T, U, H, W, bias, g = _fused_operands("rows256", J, V, dtype, 1101)
    rows = B * T * (U + 1)
    z64, z32 = _products(H, W, bias, B, T, U)
    targets = _targets(B, U, V, 131, 128, g)
    lse, gb, gy = _coefficients(*row_stats(z64, targets, 131), B, T, U)
    gb.view(-1)[128:] = 0.0                               # the second row tile carries no gradient: zeros, the main loop skipped
    gy.view(-1)[128:] = 0.0
    buf = torch.full((rows, 192), _SENTINEL, dtype=dtype, device="cuda")
    ops.transducer_gemm_grad(H.cuda(), W.cuda(), bias.cuda(), _i32(targets), lse.cuda().view(-1), gb.cuda().view(-1),
                             gy.cuda().view(-1), B, T, U + 1, 131, 0, rows, buf[:, :V])
    assert float(buf[128:, :V].abs().sum()) == 0.0 and bool((buf[:, V:] == _SENTINEL).all())
    _check_grad(f"transducer_gemm_grad zero tile {'bf16' if dtype == torch.bfloat16 else 'f32'}", buf[:, :V],
                logit_grad(z64, targets, 131, lse, gb, gy), _grad32(z32, targets, 131, lse, gb, gy), gb, gy, dtype == torch.bfloat16)


def test_fused_gemm_entries_refuse_misaligned_widths():
    from summarymixing_amd import ops
    B, T, U = 1, 2, 1
    tg, lse = _i32([[1]]), torch.zeros(4, device="cuda")
    for J, V in ((96, 8), (64, 6)):                       # J % 64 != 0; V % 4 != 0: refused by the host code, nothing is launched
        H, W = torch.zeros(4, J, device="cuda"), torch.zeros(V, J, device="cuda")
        with pytest.raises(RuntimeError):
            ops.transducer_gemm_stats(H, W, None, tg, B, T, U + 1, 0)
        with pytest.raises(RuntimeError):
            ops.transducer_gemm_grad(H, W, None, tg, lse, lse, lse, B, T, U + 1, 0, 0, 4, torch.zeros(4, 8, device="cuda")[:, :V])


# ---- B5: joint --------------------------------------------------------------------------------------------------------------------
_ACTS = [torch.nn.GELU, torch.nn.LeakyReLU, torch.nn.ReLU]


def _act_code(act):
    from summarymixing_amd import _lib as L
    return {torch.nn.GELU: L.ACT_GELU, torch.nn.LeakyReLU: L.ACT_LEAKY_RELU, torch.nn.ReLU: L.ACT_RELU}[act]


def _joint_case(B, T, U1, J, dtype, act, seed):
    g = torch.Generator().manual_seed(seed)
    enc = (torch.randn(B, T, J, generator=g) * 1.5).to(dtype)
    dec = (torch.randn(B, U1, J, generator=g) * 1.5).to(dtype)
    enc[0, 0, :min(J, 8)] = 0.5                           # enc + dec == 0 exactly (LeakyReLU's slope there is 0.01, as torch has it)
    dec[0, 0, :min(J, 8)] = -0.5
    gH = torch.randn(B, T, U1, J, generator=g).to(dtype)
    pre = (enc.double()[:, :, None, :] + dec.double()[:, None, :, :]).requires_grad_(True)
    ref = act()(pre)
    (dact,) = torch.autograd.grad(ref.sum(), pre)
    terms = gH.double() * dact
    return enc, dec, gH, ref.detach(), terms


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("act", _ACTS, ids=lambda a: a.__name__)
@pytest.mark.parametrize("B,T,U1,J", [(2, 33, 5, 64), (2, 97, 9, 72), (1, 64, 3, 1088), (3, 1, 1, 4)])
def test_joint_elementwise(B, T, U1, J, act, dtype):
    """Forward: fp32 arithmetic on a pre-activation of magnitude <= ~8 (one rounding of the sum, then the activation): 1e-6 of
    max(1, |ref|); bf16 adds the one rounding of the output, 2^-8 |ref|.  Backward: T or U1 terms g act' summed in fp32, each
    term within a few 1e-7 of |g|: 1e-6 of sum |g|, and for bf16 the one rounding of the result on top."""
    from summarymixing_amd import ops
    enc, dec, gH, ref, terms = _joint_case(B, T, U1, J, dtype, act, 1200 + T + J)
    assert torch.equal(joint_ref(enc, dec, act()), ref)
    code = _act_code(act)
    H = ops.transducer_joint_fwd(enc.cuda(), dec.cuda(), code)
    assert H.shape == (B, T, U1, J) and H.dtype == dtype
    r8 = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    err = (H.cpu().double() - ref).abs()
    bar = 1e-6 * ref.abs().clamp(min=1.0) + r8 * ref.abs()
    assert bool((err <= bar).all()), ("forward", float((err / bar).max()))
    d_enc, d_dec = ops.transducer_joint_bwd(gH.cuda(), enc.cuda(), dec.cuda(), code)
    out = {"fwd_err_over_bar": float((err / bar).max())}
    for name, got, dim in (("d_enc", d_enc, 2), ("d_dec", d_dec, 1)):
        assert got.dtype == dtype
        r, gsum = terms.sum(dim), gH.double().abs().sum(dim)
        e = (got.cpu().double() - r).abs()
        b_ = 1e-6 * gsum + r8 * r.abs()
        out[name + "_err_over_bar"] = float((e / b_).max())
        assert bool((e <= b_).all()), (name, float((e / b_).max()))
    report(f"transducer_joint {act.__name__} {'bf16' if dtype == torch.bfloat16 else 'f32'} ({B},{T},{U1},{J})", out)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_joint_backward_into_output_slices(dtype):
    """As the fused backward calls it: utterances [b0, b1) into d_enc[b0:b1] / d_dec[b0:b1]; the same bits as the whole batch gives,
    and nothing else touched."""
    from summarymixing_amd import ops
    B, T, U1, J = 3, 33, 5, 64
    enc, dec, gH, _, _ = _joint_case(B, T, U1, J, dtype, torch.nn.GELU, 1301)
    enc, dec, gH = enc.cuda(), dec.cuda(), gH.cuda()
    code = _act_code(torch.nn.GELU)
    full_e, full_d = ops.transducer_joint_bwd(gH, enc, dec, code)
    d_enc, d_dec = torch.full_like(enc, _SENTINEL), torch.full_like(dec, _SENTINEL)
    ops.transducer_joint_bwd(gH[1:3], enc[1:3], dec[1:3], code, d_enc[1:3], d_dec[1:3])
    assert torch.equal(d_enc[1:3], full_e[1:3]) and torch.equal(d_dec[1:3], full_d[1:3])
    assert bool((d_enc[0] == _SENTINEL).all()) and bool((d_dec[0] == _SENTINEL).all())

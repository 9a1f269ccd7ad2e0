"""The two instantiations of layernorm_bwd_kernel (layernorm.hip): dense dY, and dY as the sum of split-K slabs.

Dense form, per element against float64: D in {256, 512} (one and two 4-column chunks per lane), N in {1, 7, 260} (one row; fewer rows
than a block's 4 waves x U rows, odd; several blocks with a ragged last one), float32 and bf16 X, with and without R, with and without
the second output dX2 = alpha2 * Dropout(dX) * row_mask2.  The bar is the first-order one of tests/_gemm_ref.py's LayerNorm backward
with an exact incoming gradient (e = 0): u = 2^-24, L = log2(D) + 8 the depth of a row sum,
    xhat = (x - mean) rstd from the given float32 statistics:  dxh <= u (2 |xhat| + 2 rstd (|x| + |mean|))
    gg = dy gamma: dgg <= u |gg|;  s1 = mean(gg): ds1 <= mean(dgg) + u L mean|gg|;  s2 = mean(gg xhat): ds2 <= mean(dgg |xhat| + |gg| dxh) + u L mean|gg xhat|
    dX = rstd (gg - s1 - xhat s2) + R:  ddx <= rstd (dgg + ds1 + |xhat| ds2 + dxh |s2|) + 4 u (rstd (|gg| + |s1| + |xhat s2|) + |R|)
    bar(dX) = 2 (ddx + 2^-9 |dX|);  bar(dX2) = 2 (|alpha2| ddx / (1 - p) + 2^-9 |dX2|)
    bar(dgamma) = 2 (sum_n |dy| dxh + u (N + 16) sum_n |dy xhat|),  bar(dbeta) = 2 u (N + 16) sum_n |dy|
each plus 1e-30.

Slab form: nslab in {1, 3, 16} float32 slabs, a slab_stride larger than N * D.  The slab values are small multiples of 1/8, so every
running sum is exact in float32 AND in bf16: the float32 sum taken on the host in slab order, rounded to bf16 without loss, is the dY
of the dense form, which then sees the same numbers in the same expressions - dX and dX2 must be bit-equal."""
import ctypes
import math

import pytest
import torch

from tests._util import report

pytestmark = pytest.mark.gpu
U, UT, TINY = 2.0 ** -24, 2.0 ** -9, 1e-30
BF = torch.bfloat16


def _launch(N, D, x, gamma, beta, stats, dx, dy=None, slabs=None, slab_stride=0, nslab=0, res=None, second=None, dgamma=None, dbeta=None):
    """One smx_layernorm_bwd call on bf16 gradients.  second = (dx2, alpha2, mask_u8 | None, p, seed)."""
    from summarymixing_amd import _lib as L
    from summarymixing_amd import ops
    ws = torch.empty(L.lib().smx_layernorm_bwd_workspace(N, D), dtype=torch.uint8, device="cuda")
    a = L.LnBwd(dtype=L.BF16, x_f32=int(x.dtype == torch.float32), act=L.ACT_NONE, gamma=ops._p(gamma), beta=ops._p(beta), stats=ops._p(stats),
                dX=ops._p(dx), lddx=dx.stride(0), dgamma=ops._p(dgamma), dbeta=ops._p(dbeta), workspace=ops._p(ws), alpha2=1.0, epoch=ops._epoch(),
                N=N, D=D)
    a.X, a.ldx = ops._p(x), x.stride(0)
    if slabs is not None:
        a.slabs, a.nslab, a.slab_stride = ops._p(slabs), nslab, slab_stride
    else:
        a.dY, a.lddy = ops._p(dy), dy.stride(0)
    if res is not None:
        a.R, a.ldr = ops._p(res), res.stride(0)
    if second is not None:
        dx2, alpha2, mask, p, seed = second
        a.dX2, a.lddx2, a.alpha2, a.row_mask2, a.drop_p2, a.drop_seed2 = ops._p(dx2), dx2.stride(0), alpha2, ops._p(mask), p, seed
    L.check(L.lib().smx_layernorm_bwd(ctypes.byref(a), ops._stream()), "smx_layernorm_bwd")
    torch.cuda.synchronize()
    return ws


def _inputs(N, D, xdt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    ramp = torch.linspace(-1, 1, D, device="cuda")
    x = (rn(N, D) * 2.0 + 0.3 + ramp).to(xdt)
    gamma, beta = 1.0 + 0.5 * ramp + 0.1 * rn(D), 0.7 * ramp
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    stats = torch.cat([mean, (var + 1e-5).rsqrt()], 1).float().contiguous()
    return x, gamma.contiguous(), beta.contiguous(), stats, rn


@pytest.mark.parametrize("second", [False, True], ids=["", "dx2"])
@pytest.mark.parametrize("has_r", [False, True], ids=["", "res"])
@pytest.mark.parametrize("xdt", [torch.float32, BF], ids=["x32", "x16"])
@pytest.mark.parametrize("N", [1, 7, 260])
@pytest.mark.parametrize("D", [256, 512])
def test_dense_form_per_element_vs_fp64(D, N, xdt, has_r, second):
    from summarymixing_amd import ops
    x, gamma, beta, stats, rn = _inputs(N, D, xdt, 1000 * D + 10 * N + 2 * has_r + second)
    dy = rn(N, D).to(BF)
    res = rn(N, D).to(BF) if has_r else None
    dx = torch.empty(N, D, dtype=BF, device="cuda")
    dgamma, dbeta = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    sec = None
    alpha2, p2, seed2 = 0.5, 0.15, 0x13579B
    if second:
        mask = (torch.rand(N, device="cuda") > 0.3).to(torch.uint8)
        mask[-1] = 0
        sec = (torch.empty(N, D, dtype=BF, device="cuda"), alpha2, mask, p2, seed2)
    _launch(N, D, x, gamma, beta, stats, dx, dy=dy, res=res, second=sec, dgamma=dgamma, dbeta=dbeta)
    # float64 restatement and its bar
    xd, g, gam, st = x.double(), dy.double(), gamma.double(), stats.double()
    mean, r = st[:, :1], st[:, 1:2]
    Ld = math.log2(D) + 8
    xh = (xd - mean) * r
    dxh = U * (2 * xh.abs() + 2 * r * (xd.abs() + mean.abs()))
    gg = g * gam
    s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    rd = res.double() if has_r else torch.zeros_like(g)
    ref = r * (gg - s1 - xh * s2) + rd
    dgg = U * gg.abs()
    ds1 = dgg.mean(1, keepdim=True) + U * Ld * gg.abs().mean(1, keepdim=True)
    ds2 = (dgg * xh.abs() + gg.abs() * dxh).mean(1, keepdim=True) + U * Ld * (gg * xh).abs().mean(1, keepdim=True)
    ddx = r * (dgg + ds1 + xh.abs() * ds2 + dxh * s2.abs()) + 4 * U * (r * (gg.abs() + s1.abs() + (xh * s2).abs()) + rd.abs())
    checks = {"dX": (dx.double(), ref, 2 * (ddx + UT * ref.abs()) + TINY),
              "dgamma": (dgamma.double(), (g * xh).sum(0), 2 * ((g.abs() * dxh).sum(0) + U * (N + 16) * (g * xh).abs().sum(0)) + TINY),
              "dbeta": (dbeta.double(), g.sum(0), 2 * U * (N + 16) * g.abs().sum(0) + TINY)}
    if second:
        keep = ops.dropout(torch.ones(N, D, device="cuda"), p2, seed2) != 0
        y = torch.where(keep, ref / (1.0 - p2), torch.zeros_like(ref)) * sec[2].double().reshape(-1, 1) * alpha2
        checks["dX2"] = (sec[0].double(), y, 2 * (alpha2 * ddx / (1.0 - p2) + UT * y.abs()) + TINY)
        assert not bool((sec[0][~keep] != 0).any()), "dX2 holds a non-zero value at a dropped position"
    entry = {"case": f"dense-D{D}-N{N}-{'x32' if xdt == torch.float32 else 'x16'}{'-res' if has_r else ''}{'-dx2' if second else ''}"}
    for name, (got, want, bar) in checks.items():
        ratio = (got - want).abs() / bar
        w = float(ratio.max())
        entry[name] = round(w, 4)
        print(f"{entry['case']} {name}: err / bar {w:.4f}")
        i = int(ratio.argmax())
        assert w <= 1.0, f"{name}: err / bar {w:.3f} at flat index {i}: got {float(got.reshape(-1)[i]):.9g}, ref {float(want.reshape(-1)[i]):.9g}"
    report("layernorm_bwd_forms", entry)


@pytest.mark.parametrize("xdt", [torch.float32, BF], ids=["x32", "x16"])
@pytest.mark.parametrize("nslab", [1, 3, 16])
@pytest.mark.parametrize("D", [256, 512])
def test_slab_form_bit_equal_to_host_sum_plus_dense_form(D, nslab, xdt):
    N = 261
    x, gamma, beta, stats, rn = _inputs(N, D, xdt, 7 * D + nslab)
    stride = N * D + 64                                    # (not the dense N * D; a multiple of 4 floats: 16-byte aligned slabs)
    buf = torch.full((nslab * stride + 64,), float("nan"), device="cuda")
    slabs = buf[: nslab * stride].view(nslab, stride)[:, : N * D].view(nslab, N, D)
    slabs.copy_(torch.randint(-7, 8, (nslab, N, D), device="cuda").float() / 8)
    acc = torch.zeros(N, D, device="cuda")
    for s in range(nslab):                                 # slab order, float32 (exact by construction)
        acc += slabs[s]
    dy = acc.to(BF)
    assert torch.equal(dy.float(), acc), "the test's slab values must sum exactly in bf16"
    res = rn(N, D).to(BF)
    mask = (torch.rand(N, device="cuda") > 0.3).to(torch.uint8)
    outs = []
    for form in ("slabs", "dense"):
        dx = torch.empty(N, D, dtype=BF, device="cuda")
        dx2 = torch.empty(N, D, dtype=BF, device="cuda")
        kw = dict(slabs=buf, slab_stride=stride, nslab=nslab) if form == "slabs" else dict(dy=dy)
        _launch(N, D, x, gamma, beta, stats, dx, res=res, second=(dx2, 0.5, mask, 0.15, 0xABCDE), **kw)
        outs.append((dx, dx2))
    assert not bool(torch.isnan(outs[0][0].float()).any()), "NaN in dX: the slab form read outside its slabs"
    for name, a, b in (("dX", outs[0][0], outs[1][0]), ("dX2", outs[0][1], outs[1][1])):
        diff = (a.view(torch.int16) != b.view(torch.int16)).nonzero()
        assert diff.numel() == 0, f"{name}: {diff.shape[0]} elements differ between the slab and the dense form, first at {diff[0].tolist()}"
    report("layernorm_bwd_forms", {"case": f"slabs-D{D}-S{nslab}-{'x32' if xdt == torch.float32 else 'x16'}", "bit_equal": True})

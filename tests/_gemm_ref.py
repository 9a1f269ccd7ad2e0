"""A plain float64 restatement of smx_epilogue (include/smx.h) for every epilogue family of tests/_gemm_cases.py, and the per-element
error bar the route tests hold the kernels to.  Inputs are the dtype-rounded operands, upcast to float64.

What the kernel does, restated (gemm_common.h, epilogue_phase):
    v = acc + bias[m] + C0[map(n), m]                                      (C0 here unless SMX_EPI_C0_POST)
    Z[n, m] = v                                                             (saved pre-activation, dtype T)
    a = act(v)            or, SMX_EPI_ACT_GRAD:  a = v * act'(z[n, m])
    a = dropout(a) on the first drop_cols columns, a *= row_mask[n] * alpha, a += res[n, m], a += C0 (SMX_EPI_C0_POST)
    C[n, m] = a;  colsum[m] += sum_n a                                      (the float32 values before the output rounding)
The activation sees the float32 pre-activation, not the rounded Z: the vector epilogue stores Z from `v` and then calls act_fwd_n on the
same float32 `v` (gemm_common.h:630-637), the element-guarded one likewise (:691-692), the one-pass LayerNorm phase too (:1184-1204).

THE BAR (per element; derived, not tuned)
    |got - ref| <= 2 * ( u_acc * (K + 8) * S * |alpha| * Lip  +  u_out * |ref|  +  t_act )  +  tiny
  S = sum_k |a_k| |b_k| + |bias| + |c0| bounds every partial sum of the accumulation, which is float32 in both dtypes (bf16 products are
  exact in float32), so K + 8 roundings of at most u_acc = 2^-24 relative to S cover the reduction in any order plus the bias / C0 /
  residual adds.  Lip bounds how far the activation (or the act-grad factor) can stretch that error: 1 for none / ReLU / LeakyReLU, 1.13
  for GELU and Swish (max |gelu'| = 1.129, max |swish'| = 1.0998; the derivative factors themselves are bounded by the same numbers).
  u_out is the output rounding (2^-9 bf16, 2^-24 float32), tiny = 1e-30.  t_act covers the device's fast exponential / erf polynomial
  and is MEASURED against ATen: ref_act_err = max over the case of |torch float32 act(v32) - float64 act(v)| (v32 = the float64
  pre-activation rounded to float32), t_act = 4 * ref_act_err - the margin the attention tests give ATen; 0 for the linear activations.
  The factor 2 covers the second-order terms.

LAYERNORM OUTPUTS (`ln_fwd_bound`, `_ln_bwd`): the bar on C carried through the row statistics, first order.
  Forward.  The kernel normalises the float32 row c it just computed (two passes: mean, then the centred squares; gemm_common.h:1071-1091).
  Let e_j be the error budget of c_j before the output rounding (the first and third term of the bar), E_j = e_j + 4 u |c_j| the value as
  held, L = log2(W) + 8 the depth of a row sum.  Then
      mean:   dm  <= mean(E) + u L mean|c|
      centred d_j = c_j - mean:   D_j <= E_j + dm + 2 u |d_j|
      variance = mean(d^2):  dvar <= 2 sqrt(mean d^2) sqrt(mean D^2) + u L var          (Cauchy-Schwarz on sum d_j D_j)
      rstd r = (var + eps)^-1/2:  dr <= r^3 dvar / 2 + 4 u r                              (|d r / d var| = r^3 / 2; rsqrtf to ~2 ulp)
      y0_j = d_j r gamma_j + beta_j:  dy0_j <= |gamma_j| (r D_j + |d_j| dr) + 4 u (|d_j r gamma_j| + |beta_j|)
      y = act(y0):  dy <= Lip dy0 + t_act;   bar(y) = 2 (dy + u_y |y|) + tiny;  bar(mean) = 2 (dm + u |mean|) + tiny;  bar(rstd) = 2 (dr + u r) + tiny
  The second LayerNorm of the pair form sees the unrounded y of the first (gemm_common.h:1271-1302): the same function with c = y, e = dy.
  Backward.  g = acc (times act'(LN(x)) in the extended form) has the budget e of the bar; xhat = (x - mean) rstd comes from the given
  ln_x / ln_stats with dxh <= u (2 |xhat| + 2 rstd (|x| + |mean|)).  With gg = g gamma, s1 = mean(gg), s2 = mean(gg xhat):
      dgg_j <= |gamma_j| e_j + u |gg_j|;  ds1 <= mean(dgg) + u L mean|gg|;  ds2 <= mean(dgg |xhat| + |gg| dxh) + u L mean|gg xhat|
      dX_j = rstd (gg_j - s1 - xhat_j s2) + res_j:  ddx_j <= rstd (dgg_j + ds1 + |xhat_j| ds2 + dxh_j |s2|) + 4 u (rstd (|gg_j| + |s1| + |xhat_j s2|) + |res_j|)
      dX2 = alpha2 D(dX act'(z)) mask2:  <= |alpha2| Lip ddx + t_act
      dgamma_m = sum_n g xhat:  <= sum_n (e |xhat| + |g| dxh) + u (rows per tile + 16) sum_n |g xhat|;  dbeta likewise with xhat = 1
  each doubled, plus the output rounding, as above."""
import math

import torch

from tests import _gemm_cases as G

U_ACC = 2.0 ** -24
TINY = 1e-30
LIP = {G.ACT_NONE: 1.0, G.ACT_GELU: 1.13, G.ACT_SWISH: 1.13, G.ACT_LEAKY: 1.0, G.ACT_RELU: 1.0}
_S2 = math.sqrt(2.0)
_PHI = 1.0 / math.sqrt(2.0 * math.pi)


def u_of(dtype):
    return 2.0 ** -9 if dtype == torch.bfloat16 else 2.0 ** -24


def act(a, v):
    if a == G.ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / _S2))
    if a == G.ACT_SWISH:
        return v * torch.sigmoid(v)
    if a == G.ACT_LEAKY:
        return torch.where(v >= 0, v, 0.01 * v)
    if a == G.ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    return v


def act_grad(a, z):
    if a == G.ACT_GELU:
        return 0.5 * (1.0 + torch.erf(z / _S2)) + z * _PHI * torch.exp(-0.5 * z * z)
    if a == G.ACT_SWISH:
        s = torch.sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    if a == G.ACT_LEAKY:
        return torch.where(z >= 0, torch.ones_like(z), torch.full_like(z, 0.01))
    if a == G.ACT_RELU:
        return (z > 0).to(z.dtype)
    return torch.ones_like(z)


def t_act_fwd(a, v):
    """4 x the error of ATen's own float32 activation on the float32-rounded pre-activation (0 for the linear ones)."""
    if a not in (G.ACT_GELU, G.ACT_SWISH):
        return 0.0
    v32 = v.float()
    y32 = torch.nn.functional.gelu(v32) if a == G.ACT_GELU else torch.nn.functional.silu(v32)
    return 4.0 * float((y32.double() - act(a, v)).abs().max())


def t_act_grad(a, v, z):
    """... of the act-grad product v * act'(z), evaluated by ATen in float32."""
    if a not in (G.ACT_GELU, G.ACT_SWISH):
        return 0.0
    y32 = v.float() * act_grad(a, z.float())
    return 4.0 * float((y32.double() - v * act_grad(a, z)).abs().max())


def ln_fwd_bound(c, e, gamma, beta, eps, lact, u_y):
    """LayerNorm forward of the rows c (float64, error budget e per element) -> dict(y, dy, bar_y, mean, bar_mean, rstd, bar_rstd, t_act)."""
    W = c.shape[-1]
    Ld = math.log2(W) + 8
    u = U_ACC
    mean = c.mean(-1, keepdim=True)
    d = c - mean
    var = (d * d).mean(-1, keepdim=True)
    r = (var + eps).rsqrt()
    E = e + 4 * u * c.abs()
    dm = E.mean(-1, keepdim=True) + u * Ld * c.abs().mean(-1, keepdim=True)
    D = E + dm + 2 * u * d.abs()
    dvar = 2 * var.sqrt() * (D * D).mean(-1, keepdim=True).sqrt() + u * Ld * var
    dr = 0.5 * r ** 3 * dvar + 4 * u * r
    y0 = d * r * gamma + beta
    dy0 = gamma.abs() * (r * D + d.abs() * dr) + 4 * u * ((d * r * gamma).abs() + beta.abs())
    y = act(lact, y0)
    ta = t_act_fwd(lact, y0)
    dy = LIP[lact] * dy0 + ta
    return dict(y=y, dy=dy, bar_y=2 * (dy + u_y * y.abs()) + TINY, mean=mean[..., 0], bar_mean=2 * (dm + u * mean.abs())[..., 0] + TINY,
                rstd=r[..., 0], bar_rstd=2 * (dr + u * r)[..., 0] + TINY, t_act=ta)


def reference(case, t, keep=None, keep2=None):
    """t: name -> float64 tensor of the operand's values (A, B, C as (batch, rows, cols); the others 2-D / 1-D), C / colsum holding what
    the output buffers held before the call (atomic and column-sum outputs accumulate).  keep / keep2: the boolean dropout keep masks
    (N, drop_cols) / (N, M) of smx_dropout for the case's seeds.
    -> (outs, info): outs[name] = (ref, bar, must_be_zero | None), info = dict(t_act=...)."""
    f = G.fam(case)
    T = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    u_T = u_of(T)
    A, B = t["A"], t["B"]
    if case.layout == "NT":
        acc, S = A @ B.transpose(1, 2), A.abs() @ B.abs().transpose(1, 2)
    elif case.layout == "NN":
        acc, S = A @ B, A.abs() @ B.abs()
    else:
        acc, S = A.transpose(1, 2) @ B, A.abs().transpose(1, 2) @ B.abs()
    N, M, K = case.N, case.M, case.K
    outs, t_act = {}, 0.0
    alpha = f["alpha"]
    if f["out"] == "ATOMIC":
        ref = t["C"] + alpha * acc
        outs["C"] = (ref, 2 * (U_ACC * (K + 8) * S * abs(alpha) + U_ACC * ref.abs()) + TINY, None)
        return outs, dict(t_act=0.0)
    v = acc
    if f["bias"]:
        b = t["bias"]
        b = b[:, None, :] if f["bias_batch"] else b.reshape(1, 1, M)
        v, S = v + b, S + b.abs()
    c0 = None
    if f["c0"]:
        n = torch.arange(N, device=A.device)
        rows = {"row": n, "group": n // G.C0_DIV, "mod": n % G.C0_DIV}[f["c0"]]
        c0 = t["c0"][rows][None]
        S = S + c0.abs()
        if not f["c0_post"]:
            v = v + c0
    ln = f["ln"]
    lnb = ln is not None and ln["kind"] == "bwd"
    e_acc = U_ACC * (K + 8) * S
    if lnb:
        return _ln_bwd(case, t, v[0], e_acc[0], keep2, u_T)
    a_ = f["act"]
    lip = LIP[a_]
    if f["z"] == "save":
        outs["z"] = (v, 2 * (e_acc + u_T * v.abs()) + TINY, None)
    if f["z"] == "grad":
        z = t["z"]
        x = v * act_grad(a_, z)
        t_act = t_act_grad(a_, v, z)
    else:
        x = act(a_, v)
        t_act = t_act_fwd(a_, v)
    zero = None
    if f["drop"]:
        dc = G.drop_cols(case) or M
        scale = 1.0 / (1.0 - f["drop"][0])
        kf = torch.ones(N, M, dtype=torch.bool, device=A.device)
        kf[:, :dc] = keep
        sc = torch.ones(M, dtype=torch.float64, device=A.device)
        sc[:dc] = scale
        x = torch.where(kf[None], x * sc, torch.zeros_like(x))
        zero = (~kf)[None].expand_as(x)
    mk = t["row_mask"].reshape(1, N, 1) if f["mask"] else 1.0
    x = x * mk * alpha
    if f["res"]:
        x = x + t["res"]
    if c0 is not None and f["c0_post"]:
        x = x + c0
    if zero is not None and (f["res"] or f["c0_post"]):
        zero = None                                        # (a dropped element still carries the residual / C0)
    u_out = u_T if f["out"] == "T" else 2.0 ** -24
    e_pre = e_acc * abs(alpha) * lip + t_act               # budget of the float32 value before the output rounding
    outs["C"] = (x, 2 * (e_pre + u_out * x.abs()) + TINY, zero)
    if f["colsum"]:
        ref = t["colsum"] + x[0].sum(0)
        bar = 2 * ((e_pre[0] + U_ACC * x[0].abs()).sum(0) + U_ACC * (N + 8) * (x[0].abs().sum(0) + t["colsum"].abs())) + TINY
        outs["colsum"] = (ref, bar, None)
    if ln is not None:
        e_ln = e_pre[0] + (U_ACC * t["res"][0].abs() if f["res"] else 0.0)
        r1 = ln_fwd_bound(x[0], e_ln, t["lnf_gamma"], t["lnf_beta"], 1e-5, ln.get("lnf_act", G.ACT_NONE), 2.0 ** -24 if ln.get("y32") else u_T)
        outs["lnf_y"] = (r1["y"], r1["bar_y"], None)
        outs["lnf_stats"] = (torch.stack([r1["mean"], r1["rstd"]], 1), torch.stack([r1["bar_mean"], r1["bar_rstd"]], 1), None)
        t_act = max(t_act, r1["t_act"])
        if ln.get("pair"):
            r2 = ln_fwd_bound(r1["y"], r1["dy"], t["lnf2_gamma"], t["lnf2_beta"], 1e-5, G.ACT_NONE, u_T)
            outs["lnf2_y"] = (r2["y"], r2["bar_y"], None)
            outs["lnf2_stats"] = (torch.stack([r2["mean"], r2["rstd"]], 1), torch.stack([r2["bar_mean"], r2["bar_rstd"]], 1), None)
    return outs, dict(t_act=t_act)


def _ln_bwd(case, t, g, e, keep2, u_T):
    f = G.fam(case)
    ln = f["ln"]
    u = U_ACC
    W = case.M
    Ld = math.log2(W) + 8
    x, st, gamma = t["ln_x"], t["ln_stats"], t["ln_gamma"]
    mean, r = st[:, :1], st[:, 1:2]
    xh = (x - mean) * r
    dxh = u * (2 * xh.abs() + 2 * r * (x.abs() + mean.abs()))
    t_act = 0.0
    lact = ln.get("lnf_act", G.ACT_NONE)
    if lact:
        ag = xh * gamma + t["lnf_beta"]
        t_act = t_act_grad(lact, g, ag)
        e = e * LIP[lact] + t_act + g.abs() * LIP[lact] * 8 * u      # (the float32 evaluation of LN(x) gamma + beta behind act')
        g = g * act_grad(lact, ag)
    gg = g * gamma
    s1, s2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    res = t["res"][0] if f["res"] else torch.zeros_like(g)
    dx = r * (gg - s1 - xh * s2) + res
    dgg = gamma.abs() * e + u * gg.abs()
    ds1 = dgg.mean(1, keepdim=True) + u * Ld * gg.abs().mean(1, keepdim=True)
    ds2 = (dgg * xh.abs() + gg.abs() * dxh).mean(1, keepdim=True) + u * Ld * (gg * xh).abs().mean(1, keepdim=True)
    ddx = r * (dgg + ds1 + xh.abs() * ds2 + dxh * s2.abs()) + 4 * u * (r * (gg.abs() + s1.abs() + (xh * s2).abs()) + res.abs())
    outs = {"C": (dx[None], (2 * (ddx + u_T * dx.abs()) + TINY)[None], None)}
    tr = case.plan[3]
    dgam = (g * xh).sum(0)
    bgam = 2 * ((e * xh.abs() + g.abs() * dxh).sum(0) + u * (tr + 16) * (g * xh).abs().sum(0)) + TINY
    dbet = g.sum(0)
    bbet = 2 * (e.sum(0) + u * (tr + 16) * g.abs().sum(0)) + TINY
    outs["ln_partial"] = (torch.stack([dgam, dbet]), torch.stack([bgam, bbet]), None)
    if ln.get("dx2"):
        a2 = f["act"] if ln.get("z2") else G.ACT_NONE
        y = dx
        ta2 = 0.0
        if ln.get("z2"):
            ta2 = t_act_grad(a2, dx, t["z"][0])
            y = dx * act_grad(a2, t["z"][0])
        zero = None
        if ln.get("drop2"):
            y = torch.where(keep2, y / (1.0 - ln["drop2"][0]), torch.zeros_like(y))
            zero = ~keep2
        mk = t["ln_mask2"].reshape(-1, 1) if ln.get("mask2") else 1.0
        y = y * mk * ln["alpha2"]
        outs["ln_dx2"] = (y, 2 * (abs(ln["alpha2"]) * LIP[a2] * ddx + ta2 + u_T * y.abs()) + TINY, zero)
        t_act = max(t_act, ta2)
    return outs, dict(t_act=t_act)


def worst(case, name, got, ref, bar):
    """-> (ratio, message) of the element with the largest |got - ref| / bar; tensors (batch, rows, cols) or 2-D / 1-D."""
    err = (got.double() - ref).abs()
    ratio = err / bar
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    idx = []
    for s in reversed(ratio.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    idx3 = (0,) * (3 - len(idx)) + idx
    b, n, m = idx3
    tn, tm = case.plan[3], case.plan[4]
    w = float(ratio.reshape(-1)[int(ratio.argmax())])
    msg = (f"{case.name} plan={case.plan} {name}: worst element (batch, row, col) = ({b}, {n}, {m}), tile (row // tile_n, col // tile_m, row % tile_n, "
           f"col % tile_m) = ({n // tn}, {m // tm}, {n % tn}, {m % tm}): got {float(got[idx]):.9g}, ref {float(ref[idx]):.9g}, "
           f"|err| {float(err[idx]):.3e}, bar {float(bar[idx]):.3e}, err / bar {w:.3f}")
    return w, msg

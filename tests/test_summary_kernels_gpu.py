"""The summary kernels of csrc/rowwise.hip, per element against float64, on every launch branch, inside poisoned buffers.

masked_mean / bcast_rows / bcast_rows_act_bwd / pool_bcast / chunk_mean / expdecay_mean / act_mask_bwd through their ops.* wrappers,
with the conventions of tests/test_gemm_routes_gpu.py:
  * every read operand is a view inside a larger buffer of NaNs (rows before and after the view, the ld - D padding; the operators take
    uniformly strided (B T, D) views, so there is no gap between utterances to poison); uint8 masks are views inside a buffer of 1s.  A
    NaN in an output means the kernel summed something it was not given.  Every touched byte lies inside a live allocation.
  * every written operand the caller owns is a view inside a finite sentinel bit pattern with guard rows and (off the contiguous
    alignment, where ld = D leaves none) at least 8 elements of row padding; the guard holds the sentinel BITWISE after the call.  (The
    float32 (B, D) means and (B) counts are allocated by the wrappers themselves.)
  * three alignments: "c" contiguous, "h" the second half of a (rows, 2 D) buffer (vector path, ld != D), "o" an odd column offset in
    an odd ld (the scalar twin whatever D is).  expdecay_mean refuses "o": its refusal code is asserted instead.
  * float32 and bf16; the float64 side gets the dtype-rounded inputs.
  * a second identical call reproduces every output bit for bit, except act_mask_bwd's dgroup and the scalar kernel's dbias (atomics),
    which meet their bar again.
  * every case asserts the launch-plan values it is there for: the library's queries where they exist, else the restatement of the host
    arithmetic in tests/_summary_ref.py against the hand-written case tables there.
The bars are derived in tests/_summary_ref.py, judged per element (per row where the docstring there says so); the only elements they
do not judge are those of a fully masked utterance, which has its own exact assertions (reference summary_mixing.py:264-266).
pool_bcast's act / mask backward is judged in two steps that compose to the whole: the float32 sums it returns against float64 by the
sum bar, and its broadcast against float64 computed FROM those returned sums by the act'(z) rule (the values are the same registers).
The measured (error, bar) of every case - with ATen's error where the bar is relative to it - of the first run on an MI355X are in
profiles/summary_parity_errors.jsonl."""
import zlib

import pytest
import torch

from tests import _summary_ref as R
from tests._util import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
_SENT16, _SENT32 = 0x4B4C, 0x4B4C4D4E                     # finite in bf16 and float32 (1.3e7); never a value a case computes
GUARD = 8


def _ops():
    from summarymixing_amd import _lib as L, ops
    return L, ops


def _dn(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _bits(buf):
    return buf.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[buf.element_size()])


def _geom(rows, D, align):
    """-> (ld, offset of the view, buffer elements)."""
    if align == "c":
        ld, col = D, 0
    elif align == "h":
        ld, col = 2 * D, D
    else:
        ld, col = D + 9 + (D % 2), 1                       # odd ld >= D + 9, odd column offset
    return ld, GUARD * ld + col, (rows + 2 * GUARD) * ld + 16


def rd(vals, dtype, align):
    """A read operand: vals (rows, D) as a view inside a buffer of NaNs."""
    rows, D = vals.shape
    ld, off, total = _geom(rows, D, align)
    buf = torch.full((total,), float("nan"), dtype=dtype, device=DEV)
    v = buf.as_strided((rows, D), (ld, 1), off)
    v.copy_(vals.to(DEV).to(dtype))
    return v


def rdflat(vals):
    """A dense float32 operand (g, inv_in) between NaNs."""
    buf = torch.full((vals.numel() + 128,), float("nan"), dtype=F32, device=DEV)
    v = buf[64:64 + vals.numel()].view(vals.shape)
    v.copy_(vals.to(DEV))
    return v


def rdmask(m):
    """A uint8 mask (n) as a view inside a buffer of 1s."""
    buf = torch.ones(m.numel() + 64, dtype=torch.uint8, device=DEV)
    v = buf[32:32 + m.numel()]
    v.copy_(m.reshape(-1).to(DEV).to(torch.uint8))
    return v


class Wr:
    """A written operand: a (rows, D) view inside a sentinel-filled buffer; init: values the call accumulates onto."""

    def __init__(self, rows, D, dtype, align, init=None, what="out"):
        ld, off, total = _geom(rows, D, align)
        self.what, self.buf = what, torch.empty(total, dtype=dtype, device=DEV)
        _bits(self.buf).fill_(_SENT16 if self.buf.element_size() == 2 else _SENT32)
        self.view = self.buf.as_strided((rows, D), (ld, 1), off)
        if init is not None:
            self.view.copy_(init.to(DEV).to(dtype))
        self.inside = torch.zeros(total, dtype=torch.bool, device=DEV)
        self.inside.as_strided((rows, D), (ld, 1), off).fill_(True)
        self.before = _bits(self.buf).clone()

    def reset(self):
        _bits(self.buf).copy_(self.before)

    def check(self, case):
        """The guard is intact and the view holds no NaN -> the buffer's bits."""
        after = _bits(self.buf).clone()
        bad = (after != self.before) & ~self.inside
        assert not bool(bad.any()), f"{case}: {self.what} was written OUTSIDE its view at buffer elements {bad.nonzero()[:8, 0].tolist()}"
        assert not bool(torch.isnan(self.view.float()).any()), f"{case}: NaN in {self.what}: the kernel read outside an operand it was given"
        return after


def judge(case, what, got, ref, bar, rec, live=None):
    """Every element (of the rows in `live`) within its bar -> records the worst err / bar."""
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    got = got.double()
    if live is not None:
        got, ref, bar = got[live], ref[live], bar[live]
    assert not bool(torch.isnan(got).any()), f"{case}: NaN in {what}: the kernel summed something it was not given"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    w = float(ratio.max()) if ratio.numel() else 0.0
    i = int(ratio.argmax()) if ratio.numel() else 0
    print(f"{case} {what}: err/bar {w:.4f}")
    rec[what] = {"err": float(err.reshape(-1)[i]) if ratio.numel() else 0.0, "bar": float(bar.reshape(-1)[i]) if ratio.numel() else 0.0,
                 "err_over_bar": round(w, 4)}
    assert w <= 1.0, (f"{case}: {what} err / bar = {w:.3f} at flat element {i} of {tuple(ref.shape)}: got {float(got.reshape(-1)[i])!r}, "
                      f"float64 {float(ref.reshape(-1)[i])!r}, bar {float(bar.reshape(-1)[i]):.3e}")


def judge_act(case, what, got, aten, ref, dtype, rec):
    """The act'(z) rule, per row: ours <= max(4 x ATen, 8 eps), both row-relative against float64."""
    assert not bool(torch.isnan(got.float()).any()), f"{case}: NaN in {what}: the kernel read outside an operand it was given"
    eo, ea = R.row_rel(got, ref).reshape(-1), R.row_rel(aten, ref).reshape(-1)
    bar = R.act_bar(ea, dtype)
    w = float((eo / bar).max())
    print(f"{case} {what}: ours {float(eo.max()):.3e} ATen {float(ea.max()):.3e} err/bar {w:.4f}")
    rec[what] = {"err": float(eo.max()), "aten": float(ea.max()), "bar": float(bar[(eo / bar).argmax()]), "err_over_bar": round(w, 4)}
    assert w <= 1.0, f"{case}: {what}: row {int((eo / bar).argmax())} is {float(eo.max()):.3e} off, ATen {float(ea.max()):.3e} (err / bar {w:.3f})"


def twice(case, call, outs, tensors=()):
    """call() once -> check the guards; the caller judges; then again(): the second call must reproduce every bit."""
    call()
    torch.cuda.synchronize()
    first = [o.check(case) for o in outs]
    firstt = [t().clone() for t in tensors]

    def again():
        for o in outs:
            o.reset()
        call()
        torch.cuda.synchronize()
        for o, f in zip(outs, first):
            assert torch.equal(_bits(o.buf), f), f"{case}: {o.what} differs between two identical calls"
        for t, f in zip(tensors, firstt):
            assert torch.equal(_bits(t()), _bits(f)), f"{case}: a returned tensor differs between two identical calls"
    return again


def _keep(ops, rows, D, p, seed):
    return ops.dropout(torch.ones(rows, D, device=DEV), p, seed) != 0


# ---- masked_mean ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ["c", "h", "o"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", list(R.MM_CASES), ids=lambda s: "x".join(map(str, s)))
def test_masked_mean(shape, dtype, align):
    L, ops = _ops()
    B, T, D = shape
    case = f"masked_mean-{B}x{T}x{D}-{_dn(dtype)}-{align}"
    nv = R.nvec(dtype)
    plan = R.mm_plan(B, T, D, nv)
    assert plan == R.MM_CASES[shape][dtype], f"{case}: the table names (DC, TS, TR) = {R.MM_CASES[shape][dtype]}, mm_plan gives {plan}"
    assert L.lib().smx_masked_mean_workspace(B, T, D) == R.mm_workspace(B, T, D), case
    vec = D % nv == 0 and align != "o"
    assert vec == (shape not in R.MM_SCALAR and align != "o")
    g = _gen("mm", shape)
    s = rd(R.utterances(B, T, D, g, 0.25).view(B * T, D), dtype, align)
    x = s.double().view(B, T, D)
    masks = {k: v.to(DEV) for k, v in R.mm_masks(B, T, plan[2], g).items()}
    rec = {"case": case, "plan": list(plan), "vec": vec}
    results = {}
    for mname, scale in (("none", True), ("none", False), ("holes", True), ("holes", False), ("single", True)):
        mask = masks.get(mname)
        mk = rdmask(mask) if mask is not None else None
        ref = R.masked_mean_ref(x, mask, scale)
        assert not bool(ref["dead"].any())
        res = {}

        def call():
            res["out"], res["inv"] = ops.masked_mean(s, mk, B, T, scale, True)
        again = twice(case, call, [], [lambda: res["out"], lambda: res["inv"]])
        tag = f"{mname}-{'mean' if scale else 'sum'}"
        judge(case, tag, res["out"], ref["ref"], ref["bar"], rec)
        judge(case, tag + "-inv", res["inv"], ref["inv"], ref["inv_bar"], rec)
        results[(mname, scale)] = (res["out"].clone(), res["inv"].clone(), mk)
        again()
    if B >= 2:
        # a fully masked utterance (reference summary_mixing.py:264-266): inv = +inf, scaled mean NaN, unscaled mean 0; every other
        # utterance is bitwise what the same call gives with that utterance alive
        d = B - 2
        live = torch.ones(B, dtype=torch.bool, device=DEV)
        live[d] = False
        for scale in (True, False):
            out0, inv0, mk0 = results[("holes", scale)]
            mk = rdmask(masks["holes"])
            mk[d * T:(d + 1) * T] = 0
            out, inv = ops.masked_mean(s, mk, B, T, scale, True)
            assert float(inv[d]) == float("inf"), f"{case}: inv of the fully masked utterance is {float(inv[d])}"
            if scale:
                assert bool(torch.isnan(out[d]).all()), f"{case}: the scaled mean of a fully masked utterance must be NaN (0 * inf)"
            else:
                assert bool((out[d] == 0).all()), f"{case}: the unscaled sum of a fully masked utterance must be 0"
            assert torch.equal(_bits(out[live]), _bits(out0[live])) and torch.equal(_bits(inv[live]), _bits(inv0[live])), \
                f"{case}: a fully masked utterance changed another utterance's result"
    report("summary_kernels", rec)


# ---- bcast_rows / bcast_rows_act_bwd ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ["c", "h", "o"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", list(R.BC_CASES), ids=lambda s: "x".join(map(str, s)))
def test_bcast_rows(shape, dtype, align):
    L, ops = _ops()
    B, T, D = shape
    case = f"bcast_rows-{B}x{T}x{D}-{_dn(dtype)}-{align}"
    nv, r = R.nvec(dtype), R.rnd(dtype)
    plans = (R.bcast_plan(B, T, D, nv, False), R.bcast_plan(B, T, D, nv, True))
    assert plans == R.BC_CASES[shape][dtype], f"{case}: the table names (LPR, DC, RPB) = {R.BC_CASES[shape][dtype]}, bcast_impl gives {plans}"
    gen = _gen("bc", shape)
    g = rdflat(torch.randn((B, D), generator=gen))
    inv = rdflat(torch.rand((B,), generator=gen) + 0.5)
    mask = torch.rand((B, T), generator=gen, device="cpu") > 0.3
    mask[:, -1] = False                                    # (the poison beside a mask is 1: a read one row off the end shows)
    mask = mask.to(DEV)
    mk = rdmask(mask)
    z = rd(1.5 * torch.randn((B * T, D), generator=gen), dtype, align)
    rec = {"case": case, "plan_store": list(plans[0]), "plan_read": list(plans[1]), "vec": D % nv == 0 and align != "o"}
    ds = Wr(B * T, D, dtype, align, what="dS")
    p, seed = 0.2, 1234 + T
    keep = _keep(ops, B * T, D, p, seed).view(B, T, D)
    v64, v1 = g.double() * inv.double()[:, None], g.double()
    for tag, iv, drop in (("plain", None, None), ("inv", inv, None), ("inv-drop", inv, (p, seed))):
        again = twice(case, lambda: ops.bcast_rows(g, iv, ds.view, B, T, drop=drop), [ds])
        ref, bar = R.bcast_ref(v64 if iv is not None else v1, T, r, keep=keep if drop else None, p=p)
        if drop:
            assert bool((ds.view.view(B, T, D)[~keep] == 0).all()), f"{case}: a dropped position is not zero (index row * D + col)"
            assert bool((ds.view.view(B, T, D)[keep] != 0).all()), f"{case}: a kept position is zero (index row * D + col)"
        judge(case, tag, ds.view.view(B, T, D), ref, bar, rec)
        again()
        ds.reset()
    # the act / mask backward forms
    v32 = g * inv[:, None]
    for tag, act, zz, mm in (("swish-mask", L.ACT_SWISH, z, mask), ("gelu", L.ACT_GELU, z, None), ("mask-only", L.ACT_NONE, None, mask)):
        mkk = mk if mm is not None else None
        again = twice(case, lambda: ops.bcast_rows_act_bwd(g, inv, ds.view, B, T, zz, mkk, act), [ds])
        got = ds.view.view(B, T, D)
        if mm is not None:
            assert bool((got[~mm] == 0).all()), f"{case}: {tag}: a masked row is not exactly zero"
        if zz is None:
            ref, bar = R.bcast_ref(v64, T, r, rowmask=mm)
            judge(case, tag, got, ref, bar, rec)
        else:
            m64 = mm.double()[..., None] if mm is not None else 1.0
            m32 = mm.float()[..., None] if mm is not None else 1.0
            ref = v64[:, None, :] * R.act_grad(act, zz.double().view(B, T, D)) * m64
            aten = (v32[:, None, :] * R.act_grad(act, zz.float().view(B, T, D)) * m32).to(dtype)
            judge_act(case, tag, got, aten, ref, dtype, rec)
        again()
        ds.reset()
    report("summary_kernels", rec)


# ---- pool_bcast -------------------------------------------------------------------------------------------------------------------------
def _pb_params():
    out = []
    for dtype in DTYPES:
        for B, T, D, CL, aligns in R.pb_cases(dtype):
            out += [pytest.param(B, T, D, CL, dtype, a, id=f"{B}x{T}x{D}-{_dn(dtype)}-{a}") for a in aligns]
    return out


@pytest.mark.parametrize("B,T,D,CL,dtype,align", _pb_params())
def test_pool_bcast(B, T, D, CL, dtype, align):
    L, ops = _ops()
    case = f"pool_bcast-{B}x{T}x{D}-{_dn(dtype)}-{align}"
    nv, r = R.nvec(dtype), R.rnd(dtype)
    assert ops.pool_bcast_ok(B, T, D) and R.pool_ok(B, T, D), f"{case}: smx_pool_bcast_ok refuses the shape"
    assert L.get_config()["pool_fuse_max_rows"] == 16384
    assert R.pool_cl(B, D, nv) == CL, f"{case}: the table names CL = {CL}, smx_pool_bcast picks {R.pool_cl(B, D, nv)}"
    gen = _gen("pb", B, T, D)
    xv = R.utterances(B, T, D, gen, 0.25).view(B * T, D) + 0.5
    s = rd(xv, dtype, align)
    x = s.double().view(B, T, D)
    mask = torch.rand((B, T), generator=gen) > 0.35
    mask[:, T // 2] = True
    mask = mask.to(DEV)
    mk = rdmask(mask)
    rec = {"case": case, "CL": CL, "vec": D % nv == 0 and align != "o"}
    res = {}
    # 1. mean + inv only
    ref = R.masked_mean_ref(x, mask, True)

    def call1():
        res["mean"], res["inv"] = ops.pool_bcast(s, mk, B, T, want_mean=True, want_inv=True)
    again = twice(case, call1, [], [lambda: res["mean"], lambda: res["inv"]])
    judge(case, "mean", res["mean"], ref["ref"], ref["bar"], rec)
    judge(case, "inv", res["inv"], ref["inv"], ref["inv_bar"], rec)
    again()
    # 2. forward broadcast with dropout: out of place, then in place on the operand's own view
    p, seed = 0.2, 99 + T
    keep = _keep(ops, B * T, D, p, seed).view(B, T, D)
    dscale = 1.0 / (1.0 - float(torch.tensor(p, dtype=F32)))
    refd = R.masked_mean_ref(x, mask, True, r=r, k=1)
    fref = refd["ref"][:, None, :] * keep.double() * dscale
    fbar = (refd["bar"] * dscale)[:, None, :].expand(B, T, D)
    ds = Wr(B * T, D, dtype, align, what="dS")

    def call2():
        res["inv2"] = ops.pool_bcast(s, mk, B, T, ds=ds.view, want_mean=False, want_inv=True, drop=(p, seed))[1]
    again = twice(case, call2, [ds], [lambda: res["inv2"]])
    got = ds.view.view(B, T, D)
    assert bool((got[~keep] == 0).all()) and bool((got[keep] != 0).all()), f"{case}: the dropout pattern is not that of ops.dropout (row * D + col)"
    judge(case, "fwd-drop", got, fref, fbar, rec)
    assert torch.equal(res["inv2"], res["inv"])
    again()
    s2 = rd(xv, dtype, align)
    buf2 = s2._base if s2._base is not None else s2
    before = _bits(buf2).clone()
    inside = torch.zeros(buf2.numel(), dtype=torch.bool, device=DEV)
    inside.as_strided(s2.shape, s2.stride(), s2.storage_offset()).fill_(True)
    ops.pool_bcast(s2, mk, B, T, ds=s2, want_mean=False, drop=(p, seed))
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf2)[~inside], before[~inside]), f"{case}: the in-place broadcast wrote outside its view"
    assert torch.equal(_bits(s2.contiguous()), _bits(ds.view.contiguous())), f"{case}: in place differs from out of place"
    # 3. backward with inv_in (the sum over time, times the saved 1 / count)
    inv_in = rdflat(torch.rand((B,), generator=gen) + 0.5)
    ref3 = R.masked_mean_ref(x, None, False, r=r, k=1, post=inv_in.double())
    ds.reset()
    again = twice(case, lambda: ops.pool_bcast(s, None, B, T, ds=ds.view, scale=False, want_mean=False, inv_in=inv_in), [ds])
    judge(case, "bwd-inv", ds.view.view(B, T, D), ref3["ref"][:, None, :].expand(B, T, D), ref3["bar"][:, None, :].expand(B, T, D), rec)
    again()
    # 4. backward through act(.) * mask of the producing projection: the returned sums by the sum bar, the broadcast from them
    z = rd(1.5 * torch.randn((B * T, D), generator=gen), dtype, align)
    mo = mask.clone()
    mo[:, -1] = False
    mko = rdmask(mo)
    ref4 = R.masked_mean_ref(x, None, False)
    act = L.ACT_SWISH if (B + T) % 2 else L.ACT_GELU
    for tag, zz, a in (("bwd-act", z, act), ("bwd-mask", None, L.ACT_NONE)):
        ds.reset()

        def call4():
            res["sum"] = ops.pool_bcast(s, None, B, T, ds=ds.view, scale=False, want_mean=True, inv_in=inv_in, z=zz, mask_out=mko, act=a)[0]
        again = twice(case, call4, [ds], [lambda: res["sum"]])
        judge(case, tag + "-sum", res["sum"], ref4["ref"], ref4["bar"], rec)
        got = ds.view.view(B, T, D)
        assert bool((got[~mo] == 0).all()), f"{case}: {tag}: a masked row is not exactly zero"
        v64 = res["sum"].double() * inv_in.double()[:, None]
        if zz is None:
            ref, bar = R.bcast_ref(v64, T, r, rowmask=mo)
            judge(case, tag, got, ref, bar, rec)
        else:
            ref = v64[:, None, :] * R.act_grad(a, z.double().view(B, T, D)) * mo.double()[..., None]
            aten = ((res["sum"] * inv_in[:, None])[:, None, :] * R.act_grad(a, z.float().view(B, T, D)) * mo.float()[..., None]).to(dtype)
            judge_act(case, tag, got, aten, ref, dtype, rec)
        again()
    report("summary_kernels", rec)


# ---- chunk_mean -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ["c", "h", "o"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", list(R.CM_CASES), ids=lambda s: "x".join(map(str, s)))
def test_chunk_mean(shape, dtype, align):
    L, ops = _ops()
    B, T, D, chunk = shape
    case = f"chunk_mean-{B}x{T}x{D}-chunk{chunk}-{_dn(dtype)}-{align}"
    NC = R.cdiv(T, chunk)
    assert NC == R.CM_CASES[shape], case
    assert L.lib().smx_chunk_mean_workspace(B, T, D, chunk) == B * NC * D * 4
    nv, r = R.nvec(dtype), R.rnd(dtype)
    s = rd(R.utterances(B, T, D, _gen("cm", shape), 10.0).view(B * T, D), dtype, align)
    x = s.double().view(B, T, D)
    out = Wr(B * T, D, dtype, align)
    rec = {"case": case, "NC": NC, "vec": D % nv == 0 and align != "o"}
    for left in (None, 0, 2, NC + 1):
        for reverse in (False, True):
            out.reset()
            again = twice(case, lambda: ops.chunk_mean(s, out.view, B, T, chunk, left, reverse=reverse), [out])
            ref, bar = R.chunk_mean_ref(x, chunk, left, reverse, r)
            judge(case, f"left{left}-{'bwd' if reverse else 'fwd'}", out.view.view(B, T, D), ref, bar, rec)
            again()
    report("summary_kernels", rec)


# ---- expdecay_mean ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ["c", "h"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", list(R.ED_CASES), ids=lambda s: "x".join(map(str, s)))
def test_expdecay_mean(shape, dtype, align):
    L, ops = _ops()
    B, T, D = shape
    case = f"expdecay-{B}x{T}x{D}-{_dn(dtype)}-{align}"
    assert R.cdiv(T, R.ED_CH) == R.ED_CASES[shape], case
    assert L.lib().smx_expdecay_mean_workspace(B, T, D) == B * R.ED_CASES[shape] * 2 * D * 4
    s = rd(R.utterances(B, T, D, _gen("ed", shape), 0.25).view(B * T, D) + 0.5, dtype, align)
    x = s.double().view(B, T, D)
    out = Wr(B * T, D, dtype, align)
    rec = {"case": case, "NC": R.ED_CASES[shape]}
    for decay in R.ED_DECAYS:
        for reverse in (False, True):
            out.reset()
            again = twice(case, lambda: ops.expdecay_mean(s, out.view, B, T, decay, reverse=reverse), [out])
            ref = R.expdecay_ref(x, decay, reverse)
            err = R.row_rel(out.view.view(B, T, D), ref)
            floor = R.row_rel(R.expdecay_f32(x, decay, reverse), ref)
            tag = f"decay{decay}-{'bwd' if reverse else 'fwd'}"
            w = float(err.max())
            print(f"{case} {tag}: err {w:.3e} floor {float(floor.max()):.3e} bar {R.ED_BAR[dtype]:.0e}")
            rec[tag] = {"err": w, "floor": float(floor.max()), "bar": R.ED_BAR[dtype], "err_over_bar": round(w / R.ED_BAR[dtype], 4)}
            assert w <= R.ED_BAR[dtype], f"{case} {tag}: frame {int(err.argmax())} (flat b T + t) is {w:.3e} off relative to its max |ref|"
            again()
    report("summary_kernels", rec)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
def test_expdecay_mean_refuses_unaligned_operands(dtype):
    """D % 4, an odd leading dimension and a misaligned pointer are refused with SMX_EINVAL (-1) before anything is launched."""
    L, ops = _ops()
    B, T = 2, 17
    gen = _gen("edr")
    for D, a_in, a_out in ((6, "c", "c"), (8, "o", "c"), (8, "c", "o")):
        s = rd(torch.randn((B * T, D), generator=gen), dtype, a_in)
        out = Wr(B * T, D, dtype, a_out)
        for reverse in (False, True):
            with pytest.raises(RuntimeError, match="code -1"):
                ops.expdecay_mean(s, out.view, B, T, 0.995, reverse=reverse)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.buf), out.before), "a refused call wrote to its output"
    # an odd row offset with aligned ld: the pointer alone is misaligned
    buf = torch.zeros((B * T + 2) * 8 + 16, dtype=dtype, device=DEV)
    s = buf.as_strided((B * T, 8), (8, 1), 1)
    with pytest.raises(RuntimeError, match="code -1"):
        ops.expdecay_mean(s, torch.empty(B * T, 8, dtype=dtype, device=DEV), B, T, 0.9)


# ---- act_mask_bwd -----------------------------------------------------------------------------------------------------------------------
def _am_params():
    out = []
    for name, c in R.AM_CASES.items():
        for dtype in DTYPES:
            aligns = "o" if c.get("odd") else ("c" if c["M"] % 8 else "ch")
            out += [pytest.param(name, dtype, a, id=f"{name}-{_dn(dtype)}-{a}") for a in aligns]
    return out


@pytest.mark.parametrize("name,dtype,align", _am_params())
def test_act_mask_bwd(name, dtype, align):
    L, ops = _ops()
    c = R.AM_CASES[name]
    N, M, act, alpha, gdiv, drop = c["N"], c["M"], c["act"], c["alpha"], c["gdiv"], c["drop"]
    case = f"act_mask_bwd-{name}-{_dn(dtype)}-{align}"
    nv = R.nvec(dtype)
    plan = R.act_plan(N, M, nv, align != "o")
    assert (plan["vec"], plan["LPR"], plan["gx"], plan["ny"]) == c["plan"][dtype], f"{case}: the table names {c['plan'][dtype]}, the host picks {plan}"
    assert L.lib().smx_act_mask_bwd_workspace(N, M) == R.act_workspace(N, M), case
    gen = _gen("am", name)
    dy = rd(torch.randn((N, M), generator=gen), dtype, align)
    z = rd(1.5 * torch.randn((N, M), generator=gen), dtype, align) if c["z"] else None
    mask = mk = None
    if c["mask"]:
        mask = torch.rand((N,), generator=gen) > 0.4
        mask[-1] = False
        mask = mask.to(DEV)
        mk = rdmask(mask)
    dz = Wr(N, M, dtype, align, what="dZ") if c["dz"] else None
    G = R.cdiv(N, gdiv)
    acc = c["dbias"] == "acc"
    db = Wr(1, M, F32, "c", init=torch.randn((1, M), generator=gen) if acc else torch.zeros(1, M), what="dbias")
    dg = Wr(G, M, F32, "h", init=torch.randn((G, M), generator=gen) if acc else torch.zeros(G, M), what="dgroup")
    db0, dg0 = db.view[0].double().clone(), dg.view.double().clone()
    keep = _keep(ops, N, M, drop[0], drop[1]) if drop else None
    p = drop[0] if drop else 0.0
    ref = R.act_mask_bwd_ref(dy.double(), z.double() if z is not None else None, mask, act, alpha, keep, p, gdiv, db0, dg0)
    rec = {"case": case, "plan": list(c["plan"][dtype])}
    outs = [o for o in (dz, db, dg) if o is not None]

    def call():
        ops.act_mask_bwd(dy, z, mk, act, alpha, dz.view if dz else None, db.view[0], dg.view, gdiv, drop=drop)

    def verdict(tag):
        if dz is not None:
            got = dz.view
            if keep is not None:
                assert bool((got[~keep] == 0).all()), f"{case}: a dropped position of dZ is not zero (index row * M + col)"
            if mask is not None:
                assert bool((got[~mask] == 0).all()), f"{case}: a masked row of dZ is not exactly zero"
            o32 = alpha * dy.float() * (R.act_grad(act, z.float()) if z is not None else 1.0)
            if mask is not None:
                o32 = o32 * mask.float()[:, None]
            if keep is not None:
                o32 = o32 * keep.float() / (1.0 - torch.tensor(p, dtype=F32, device=DEV))
            judge_act(case, tag + "dZ", got, o32.to(dtype), ref["o"], dtype, rec)
        judge(case, tag + "dbias", db.view[0], ref["dbias"][0], ref["dbias"][1], rec)
        judge(case, tag + "dgroup", dg.view, ref["dgroup"][0], ref["dgroup"][1], rec)

    call()
    torch.cuda.synchronize()
    first = [o.check(case) for o in outs]
    verdict("")
    for o in outs:
        o.reset()
    call()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        o.check(case)
        if o is dz or (o is db and plan["vec"]):
            assert torch.equal(_bits(o.buf), f), f"{case}: {o.what} differs between two identical calls"
    verdict("again-")                                      # (dgroup and the scalar kernel's dbias are atomic sums: the bar again)
    report("summary_kernels", rec)

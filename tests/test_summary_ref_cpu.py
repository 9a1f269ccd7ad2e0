"""tests/_summary_ref.py on the CPU: its float64 restatements equal the dense formulas, its case tables equal the restated planners, and
a float32 torch emulation of every operator (any order) passes the very bar functions the GPU module asserts, on every listed case -
the condition that keeps a bar from being unmeetable.  No element is excluded from judgement (the fully masked utterance, which the
GPU module asserts exactly, is not part of these cases).  The exp-decay floor - the float32 sequential restatement against the dense
float64 operator - is at most a quarter of the float32 bar on every case."""
import zlib

import pytest
import torch

from tests import _summary_ref as R

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def _dn(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def within(what, got, ref, bar):
    """Every element judged (none excluded), every one within its bar -> the worst err / bar."""
    got = got.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and bool(torch.isfinite(bar).all())
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    assert ratio.numel() == ref.numel()
    w = float(ratio.max())
    assert w <= 1.0, f"{what}: the float32 emulation misses the bar (err / bar {w:.3f})"
    return w


# ---- tables and restatements ------------------------------------------------------------------------------------------------------------
def test_case_tables_equal_the_restated_planners():
    for (B, T, D), plans in R.MM_CASES.items():
        for dtype in DTYPES:
            assert R.mm_plan(B, T, D, R.nvec(dtype)) == plans[dtype], (B, T, D, dtype)
    ts = {R.MM_CASES[s][F32][1] for s in R.MM_CASES}
    assert {1, 2, 3, 4, 8, 32} <= ts                       # one pass, the scalar tail of stage 2, its 4-way fold once and twice, TS 32
    for (B, T, D), plans in R.BC_CASES.items():
        for dtype in DTYPES:
            nv = R.nvec(dtype)
            assert (R.bcast_plan(B, T, D, nv, False), R.bcast_plan(B, T, D, nv, True)) == plans[dtype], (B, T, D, dtype)
    rpb = {p[dt][k][2] for p in R.BC_CASES.values() for dt in DTYPES for k in (0, 1)}
    assert {8, 32, 64, 128} <= rpb
    for dtype in DTYPES:
        for B, T, D, CL, _ in R.pb_cases(dtype):
            assert R.pool_cl(B, D, R.nvec(dtype)) == CL and R.pool_ok(B, T, D), (B, T, D, dtype)
        assert {c[3] for c in R.pb_cases(dtype)} == {2, 4, 8}
    assert 128 * 130 > 16384 and R.pool_ok(128, 130, 128) and not R.pool_ok(100, 200, 128)
    for (B, T, D, chunk), NC in R.CM_CASES.items():
        assert R.cdiv(T, chunk) == NC
    for (B, T, D), NC in R.ED_CASES.items():
        assert R.cdiv(T, R.ED_CH) == NC
    assert max(R.ED_CASES.values()) > 16                    # the carry kernel's 16-ahead fetch wraps
    seen = set()
    for name, c in R.AM_CASES.items():
        for dtype in DTYPES:
            p = R.act_plan(c["N"], c["M"], R.nvec(dtype), not c.get("odd"))
            assert (p["vec"], p["LPR"], p["gx"], p["ny"]) == c["plan"][dtype], (name, dtype)
        seen |= {("z", c["z"]), ("mask", c["mask"]), ("act", c["act"]), ("alpha1", c["alpha"] == 1.0), ("dbias", c["dbias"]),
                 ("gdiv", c["gdiv"]), ("drop", c["drop"] is not None), ("dz", c["dz"]), ("vec", c["plan"][F32][0])}
    want = {("z", True), ("z", False), ("mask", True), ("mask", False), ("alpha1", False), ("dbias", "acc"), ("gdiv", 64), ("gdiv", 20),
            ("gdiv", 7), ("drop", True), ("dz", False), ("vec", True), ("vec", False)} | {("act", a) for a in (R.ACT_NONE, R.ACT_GELU, R.ACT_SWISH, R.ACT_RELU)}
    assert want <= seen, want - seen
    assert R.AM_CASES["16417x8-relu"]["N"] > 32 * 512 and 32 % 20 and 32 % 7 and 64 % 32 == 0


@pytest.mark.parametrize("shape", list(R.CM_CASES), ids=lambda s: "x".join(map(str, s)))
def test_chunk_windows_equal_the_dense_dynchunk_mask(shape):
    from summarymixing_amd.functional import DynChunkMask
    B, T, D, chunk = shape
    NC = R.CM_CASES[shape]
    for left in (None, 0, 2, NC + 1):
        assert torch.equal(R.chunk_windows(T, chunk, left), DynChunkMask(T, chunk, left).dense().double()), (shape, left)


def test_float64_restatements_equal_the_dense_formulas():
    g = _gen("restate")
    # the Laplace matrix, element by element
    M = R.laplace(5, 0.9)
    g32 = float(torch.tensor(0.9, dtype=F32))
    for i in range(5):
        for j in range(5):
            assert abs(float(M[i, j]) - g32 ** abs(i - j)) < 1e-15
    # the sequential two-sided recurrence with the expm1 denominators, in float64, is the dense operator
    for T in (1, 2, 3, 17, 257):
        x = torch.randn((2, T, 4), generator=g, dtype=torch.float64)
        for decay in R.ED_DECAYS:
            for reverse in (False, True):
                d = (R.expdecay_f32(x, decay, reverse, torch.float64) - R.expdecay_ref(x, decay, reverse)).abs().max()
                assert float(d) < 1e-12, (T, decay, reverse, float(d))
    # a plain masked sum
    x = torch.randn((3, 7, 5), generator=g, dtype=torch.float64)
    mask = torch.rand((3, 7), generator=g) > 0.4
    mask[:, 0] = True
    ref = R.masked_mean_ref(x, mask, True)
    for b in range(3):
        rows = [x[b, t] for t in range(7) if mask[b, t]]
        assert torch.allclose(ref["ref"][b], sum(rows) / len(rows), rtol=1e-14, atol=0) and float(ref["n"][b]) == len(rows)
    assert not bool(ref["dead"].any())
    mask[1] = False
    assert R.masked_mean_ref(x, mask, True)["dead"].tolist() == [False, True, False]
    # the transposed window operator is the adjoint of the forward one
    x, y = torch.randn((2, 9, 3), generator=g, dtype=torch.float64), torch.randn((2, 9, 3), generator=g, dtype=torch.float64)
    f, _ = R.chunk_mean_ref(x, 4, 1, False, 0.0)
    b, _ = R.chunk_mean_ref(y, 4, 1, True, 0.0)
    assert abs(float((f * y).sum() - (x * b).sum())) < 1e-10


# ---- float32 emulations through the bars ------------------------------------------------------------------------------------------------
def _emu_mean(x32, mask, scale, post=None):
    m = torch.ones(x32.shape[:2]) if mask is None else mask.float()
    s = (x32 * m[..., None]).sum(1)
    inv = 1.0 / m.sum(1)
    out = s * inv[:, None] if scale else s
    return (out if post is None else out * post[:, None]), inv


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", list(R.MM_CASES), ids=lambda s: "x".join(map(str, s)))
def test_masked_mean_emulation_meets_the_bars(shape, dtype):
    B, T, D = shape
    g = _gen("mm", shape)
    x32 = R.utterances(B, T, D, g, 0.25).to(dtype).float()
    masks = R.mm_masks(B, T, R.MM_CASES[shape][dtype][2], g)
    for mname, scale in (("none", True), ("none", False), ("holes", True), ("holes", False), ("single", True)):
        mask = masks.get(mname)
        ref = R.masked_mean_ref(x32.double(), mask, scale)
        assert not bool(ref["dead"].any())
        out, inv = _emu_mean(x32, mask, scale)
        within(f"{shape} {mname}", out, ref["ref"], ref["bar"])
        within(f"{shape} {mname} inv", inv, ref["inv"], ref["inv_bar"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", list(R.BC_CASES), ids=lambda s: "x".join(map(str, s)))
def test_bcast_emulation_meets_the_bars(shape, dtype):
    B, T, D = shape
    if B * T * D > (1 << 22):
        T = 16                                             # (the rows of a broadcast are copies: 16 of them carry the same arithmetic)
    gen = _gen("bc", shape)
    g, inv = torch.randn((B, D), generator=gen), torch.rand((B,), generator=gen) + 0.5
    mask = torch.rand((B, T), generator=gen) > 0.3
    keep = torch.rand((B, T, D), generator=gen) > 0.2
    z = (1.5 * torch.randn((B, T, D), generator=gen)).to(dtype)
    r, p = R.rnd(dtype), 0.2
    v32, v64 = g * inv[:, None], g.double() * inv.double()[:, None]
    ref, bar = R.bcast_ref(v64, T, r)
    within("plain", v32[:, None, :].expand(B, T, D).to(dtype), ref, bar)
    ref, bar = R.bcast_ref(v64, T, r, keep=keep, p=p)
    within("drop", (v32[:, None, :] * keep.float() * (1.0 / (1.0 - torch.tensor(p)))).to(dtype), ref, bar)
    ref, bar = R.bcast_ref(v64, T, r, rowmask=mask)
    within("mask", (v32[:, None, :] * mask.float()[..., None]).to(dtype), ref, bar)
    for act in (R.ACT_SWISH, R.ACT_GELU):
        ref = v64[:, None, :] * R.act_grad(act, z.double()) * mask.double()[..., None]
        emu = (v32[:, None, :] * R.act_grad(act, z.float()) * mask.float()[..., None]).to(dtype)
        assert float(R.row_rel(emu, ref).max()) <= 8 * torch.finfo(dtype).eps      # the floor of the act'(z) rule is one float32 meets


def _pb_params():
    return [pytest.param(B, T, D, dtype, id=f"{B}x{T}x{D}-{_dn(dtype)}") for dtype in DTYPES for B, T, D, _, _ in R.pb_cases(dtype)]


@pytest.mark.parametrize("B,T,D,dtype", _pb_params())
def test_pool_bcast_emulation_meets_the_bars(B, T, D, dtype):
    gen = _gen("pb", B, T, D)
    x32 = (R.utterances(B, T, D, gen, 0.25) + 0.5).to(dtype).float()
    x = x32.double()
    mask = torch.rand((B, T), generator=gen) > 0.35
    mask[:, T // 2] = True
    r, p = R.rnd(dtype), 0.2
    ref = R.masked_mean_ref(x, mask, True)
    mean, inv = _emu_mean(x32, mask, True)
    within("mean", mean, ref["ref"], ref["bar"])
    within("inv", inv, ref["inv"], ref["inv_bar"])
    dscale = 1.0 / (1.0 - float(torch.tensor(p, dtype=F32)))
    refd = R.masked_mean_ref(x, mask, True, r=r, k=1)
    within("fwd-drop", (mean * dscale).to(dtype), refd["ref"] * dscale, refd["bar"] * dscale)
    inv_in = torch.rand((B,), generator=gen) + 0.5
    ref3 = R.masked_mean_ref(x, None, False, r=r, k=1, post=inv_in.double())
    within("bwd-inv", _emu_mean(x32, None, False, inv_in)[0].to(dtype), ref3["ref"], ref3["bar"])
    ref4 = R.masked_mean_ref(x, None, False)
    within("bwd-sum", _emu_mean(x32, None, False)[0], ref4["ref"], ref4["bar"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("shape", list(R.CM_CASES), ids=lambda s: "x".join(map(str, s)))
def test_chunk_mean_emulation_meets_the_bars(shape, dtype):
    B, T, D, chunk = shape
    x32 = R.utterances(B, T, D, _gen("cm", shape), 10.0).to(dtype).float()
    for left in (None, 0, 2, R.CM_CASES[shape] + 1):
        Mx = R.chunk_windows(T, chunk, left).float()
        W = Mx / Mx.sum(1, keepdim=True)
        for reverse in (False, True):
            ref, bar = R.chunk_mean_ref(x32.double(), chunk, left, reverse, R.rnd(dtype))
            emu = torch.einsum("ts,bsd->btd", W.t() if reverse else W, x32).to(dtype)
            within(f"{shape} left {left} reverse {reverse}", emu, ref, bar)
    # the per-utterance offset makes a window that crosses an utterance boundary miss the bar at the edge rows
    if B > 1 and T > chunk:
        ref, bar = R.chunk_mean_ref(x32.double(), chunk, None, False, R.rnd(dtype))
        leak = torch.einsum("ts,sd->td", R.chunk_windows(B * T, chunk, None).float() / R.chunk_windows(B * T, chunk, None).float().sum(1, keepdim=True),
                            x32.reshape(B * T, D)).view(B, T, D)
        assert float(((leak.double() - ref).abs() / bar).max()) > 1.0


@pytest.mark.parametrize("shape", list(R.ED_CASES), ids=lambda s: "x".join(map(str, s)))
def test_expdecay_floor_is_a_quarter_of_the_bar(shape):
    B, T, D = shape
    for dtype in DTYPES:
        x = (R.utterances(B, T, D, _gen("ed", shape), 0.25) + 0.5).to(dtype).double()
        for decay in R.ED_DECAYS:
            for reverse in (False, True):
                ref = R.expdecay_ref(x, decay, reverse)
                emu = R.expdecay_f32(x, decay, reverse)
                floor = float(R.row_rel(emu, ref).max())
                assert floor <= R.ED_BAR[F32] / 4, (shape, dtype, decay, reverse, floor)
                assert float(R.row_rel(emu.to(dtype), ref).max()) <= R.ED_BAR[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("name", list(R.AM_CASES))
def test_act_mask_bwd_emulation_meets_the_bars(name, dtype):
    c = R.AM_CASES[name]
    N, M, act, alpha, gdiv = c["N"], c["M"], c["act"], c["alpha"], c["gdiv"]
    gen = _gen("am", name)
    dy = torch.randn((N, M), generator=gen).to(dtype)
    z = (1.5 * torch.randn((N, M), generator=gen)).to(dtype) if c["z"] else None
    mask = (torch.rand((N,), generator=gen) > 0.4) if c["mask"] else None
    G = R.cdiv(N, gdiv)
    acc = c["dbias"] == "acc"
    db0 = torch.randn((M,), generator=gen) if acc else torch.zeros(M)
    dg0 = torch.randn((G, M), generator=gen) if acc else torch.zeros(G, M)
    keep = (torch.rand((N, M), generator=gen) > 0.15) if c["drop"] else None
    p = c["drop"][0] if c["drop"] else 0.0
    ref = R.act_mask_bwd_ref(dy.double(), z.double() if z is not None else None, mask, act, alpha, keep, p, gdiv, db0.double(), dg0.double())
    o32 = alpha * dy.float() * (R.act_grad(act, z.float()) if z is not None else 1.0)
    if mask is not None:
        o32 = o32 * mask.float()[:, None]
    if keep is not None:
        o32 = o32 * keep.float() / (1.0 - torch.tensor(p, dtype=F32))
    assert float(R.row_rel(o32.to(dtype), ref["o"]).max()) <= 8 * torch.finfo(dtype).eps
    within(f"{name} dbias", db0 + o32.sum(0), *ref["dbias"])
    within(f"{name} dgroup", dg0.index_add(0, torch.arange(N) // gdiv, o32), *ref["dgroup"])

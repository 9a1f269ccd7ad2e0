"""Float64 references, per-element bars, launch-plan restatements and case tables of the summary kernels (csrc/rowwise.hip).

Shared by tests/test_summary_kernels_gpu.py (the kernels) and tests/test_summary_ref_cpu.py (which shows on the CPU that every bar
is one float32 arithmetic can meet).  Everything here is plain torch on whatever device its inputs live on; nothing loads the library.

Bars (u = 2^-24; r = the rounding of the store: eps / 2 of the output dtype, 0 for a float32 store of a float32 sum):
  sums        a float32 sum of n terms in any order is within (n - 1) u S of exact (S = the sum of |terms|); the reciprocal and the
              products under -ffast-math add at most 5 u:   bar = 1.01 ((n + 5 + k) u S |scale| + r |ref|),  n = the rows that enter
              the sum, k = float32 products applied AFTER the scaled sum (pool_bcast: inv_in, the dropout scale; 0 elsewhere).
  broadcasts  one product, one store:   bar = 1.01 (6 u + r) |ref|;  masked rows and dropped positions are exact zeros.
  act'(z)     not derivable (fast-math expf): row_rel() of ours and of ATen's float32 evaluation against float64, ours <= max(4 x
              ATen, 8 eps(dtype)).
  exp-decay   per frame relative to the frame's max |ref|: 1e-5 float32, 1e-2 bf16 (ED_BAR), at decay 0.995 and 0.9.
"""
import math

import torch

U = 2.0 ** -24
SLACK = 1.01
ACT_NONE, ACT_GELU, ACT_SWISH, ACT_RELU = 0, 1, 2, 4      # summarymixing_amd._lib.ACT_*
ED_BAR = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
ED_CH = 16                                                 # rows per exp-decay chunk
F32, BF16 = torch.float32, torch.bfloat16


def rnd(dtype):
    return 0.0 if dtype == torch.float32 else torch.finfo(dtype).eps / 2


def nvec(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def cdiv(a, b):
    return -(-a // b)


# ---- the host planners, restated (a change of rowwise.hip's arithmetic must fail the plan assertions of the case tables) ----------------
def mm_plan(B, T, D, nv):
    """mm_plan -> (DC, TS, TR)."""
    DC = cdiv(D, 64 * nv)
    want, maxts = cdiv(512, B * DC), (T + 127) // 128
    TS = max(1, min(want, maxts))
    TR = cdiv(T, TS)
    return DC, max(1, cdiv(T, TR)), TR


def mm_workspace(B, T, D):
    return B * max(mm_plan(B, T, D, 4)[1], mm_plan(B, T, D, 8)[1]) * (D + 1) * 4


def bcast_plan(B, T, D, nv, reads):
    """bcast_impl -> (LPR, DC, RPB); reads: the act / mask backward form (Z or a mask), else store-only."""
    LPR = 1
    while LPR < 64 and LPR * nv < D:
        LPR <<= 1
    DC = cdiv(D, LPR * nv)
    RPB = 64 if reads else 128
    while RPB > 8 and DC * cdiv(T, RPB) * B < 512:
        RPB >>= 1
    return LPR, DC, RPB


def pool_cl(B, D, nv):
    CL = 8
    while CL > 2 and B * cdiv(D, CL * nv) < 128:
        CL >>= 1
    return CL


def pool_ok(B, T, D, max_rows=16384):
    return B >= 1 and 1 <= T <= 4096 and D >= 1 and (B * T <= max_rows or B * cdiv(D, 64) >= 256)


def act_plan(N, M, nv, aligned):
    """smx_act_mask_bwd -> dict(vec, LPR, gx, ny) (vector kernel) or dict(vec=False, gx, ny) (scalar kernel, atomics)."""
    if M % nv == 0 and aligned:
        chunks, LPR = M // nv, 1
        while LPR < 64 and LPR < chunks:
            LPR <<= 1
        return dict(vec=True, LPR=LPR, gx=cdiv(chunks, LPR), ny=min(cdiv(N, 32), 512))
    return dict(vec=False, LPR=0, gx=cdiv(M, 256), ny=cdiv(N, 128))


def act_workspace(N, M):
    return cdiv(N, 32) * M * 4


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
# masked_mean / bcast_rows: (B, T, D) -> {dtype: (DC, TS, TR)} and {dtype: ((LPR, DC, RPB) store-only, (LPR, DC, RPB) act / mask form)}
MM_CASES = {
    (1, 1, 8):       {F32: (1, 1, 1), BF16: (1, 1, 1)},
    (2, 129, 40):    {F32: (1, 2, 65), BF16: (1, 2, 65)},
    (3, 257, 72):    {F32: (1, 3, 86), BF16: (1, 3, 86)},
    (1, 300, 520):   {F32: (3, 3, 100), BF16: (2, 3, 100)},
    (2, 1000, 264):  {F32: (2, 8, 125), BF16: (1, 8, 125)},
    (1, 4096, 64):   {F32: (1, 32, 128), BF16: (1, 32, 128)},
    (17, 9, 1032):   {F32: (5, 1, 9), BF16: (3, 1, 9)},
    (2, 385, 43):    {F32: (1, 4, 97), BF16: (1, 4, 97)},
}
MM_SCALAR = {(2, 385, 43)}                                 # D divides neither vector width: the scalar twin in every alignment
BC_CASES = {
    (1, 1, 8):       {F32: ((2, 1, 8), (2, 1, 8)), BF16: ((1, 1, 8), (1, 1, 8))},
    (2, 129, 40):    {F32: ((16, 1, 8), (16, 1, 8)), BF16: ((8, 1, 8), (8, 1, 8))},
    (3, 257, 72):    {F32: ((32, 1, 8), (32, 1, 8)), BF16: ((16, 1, 8), (16, 1, 8))},
    (1, 300, 520):   {F32: ((64, 3, 8), (64, 3, 8)), BF16: ((64, 2, 8), (64, 2, 8))},
    (2, 1000, 264):  {F32: ((64, 2, 8), (64, 2, 8)), BF16: ((64, 1, 8), (64, 1, 8))},
    (1, 4096, 64):   {F32: ((16, 1, 8), (16, 1, 8)), BF16: ((8, 1, 8), (8, 1, 8))},
    (17, 9, 1032):   {F32: ((64, 5, 8), (64, 5, 8)), BF16: ((64, 3, 8), (64, 3, 8))},
    (2, 385, 43):    {F32: ((16, 1, 8), (16, 1, 8)), BF16: ((8, 1, 8), (8, 1, 8))},
    # the shrink loop of RPB ends at 8 on all of the above (and on (40, 130, 256): 40 x 17 workgroups reach 512 only there)
    (40, 130, 256):  {F32: ((64, 1, 8), (64, 1, 8)), BF16: ((32, 1, 8), (32, 1, 8))},
    (40, 400, 256):  {F32: ((64, 1, 32), (64, 1, 32)), BF16: ((32, 1, 32), (32, 1, 32))},
    (64, 1030, 512): {F32: ((64, 2, 128), (64, 2, 64)), BF16: ((64, 1, 128), (64, 1, 64))},
}
# pool_bcast: (B, T, D) -> CL per dtype (None: the shape is not run in that dtype)
PB_BASE = {F32: {2: (3, 17, 40), 4: (10, 33, 200), 8: (40, 130, 256)}, BF16: {2: (3, 17, 40), 4: (10, 33, 512), 8: (40, 130, 256)}}


def pb_cases(dtype):
    """[(B, T, D, CL, aligns)]: the base shapes in all alignments, the row tails around U * RS (8 rows in flight x RS = 256 / CL row
    slots), T = 4096, and the B ceil(D / 64) >= 256 admission with B T > 16384."""
    out = []
    for CL, (B, T, D) in PB_BASE[dtype].items():
        out.append((B, T, D, CL, "cho"))
        RS = 256 // CL
        out += [(B, t, D, CL, "c") for t in (1, RS - 1, RS + 1, 8 * RS + 1)]
    out.append((1, 4096, 64, 2, "ch"))
    out.append((128, 130, 128, 8, "c"))
    return out


# chunk_mean: (B, T, D, chunk) -> NC
CM_CASES = {(3, 70, 48, 8): 9, (2, 70, 43, 8): 9, (1, 9, 8, 100): 1, (2, 33, 64, 1): 33, (2, 64, 520, 16): 4, (3, 5, 8, 4): 2}
# expdecay_mean: (B, T, D) -> NC
ED_CASES = {**{(2, T, 8): cdiv(T, ED_CH) for T in (1, 2, 3, 15, 16, 17, 33, 257)}, (1, 2000, 32): 125, (3, 50, 260): 4}
ED_DECAYS = (0.995, 0.9)

# act_mask_bwd: name -> dict(N, M, odd (alignment), z, mask, act, alpha, dbias (None / "zero" / "acc"), gdiv (0: no dgroup), drop, dz,
#                            plan {dtype: (vec, LPR, gx, ny)})
# SWISH / GELU terms carry the fast-math act' error, which the sum bar's 5 u does not cover at a handful of rows: their reductions run
# over >= 20 rows (n u >= 20 u beside a few u per term); the one-row and 7-row sums use RELU / NONE / no Z, whose terms are exact products.
AM_CASES = {
    "1x8-relu":        dict(N=1, M=8, z=True, mask=False, act=ACT_RELU, alpha=1.0, dbias="acc", gdiv=7, drop=None, dz=True,
                            plan={F32: (True, 2, 1, 1), BF16: (True, 1, 1, 1)}),
    "33x136-swish":    dict(N=33, M=136, z=True, mask=True, act=ACT_SWISH, alpha=0.5, dbias="acc", gdiv=20, drop=None, dz=True,
                            plan={F32: (True, 64, 1, 2), BF16: (True, 32, 1, 2)}),
    "320x136-gelu":    dict(N=320, M=136, z=True, mask=True, act=ACT_GELU, alpha=0.5, dbias="zero", gdiv=64, drop=None, dz=True,
                            plan={F32: (True, 64, 1, 10), BF16: (True, 32, 1, 10)}),
    "320x136-none-g7": dict(N=320, M=136, z=True, mask=True, act=ACT_NONE, alpha=1.0, dbias="acc", gdiv=7, drop=(0.15, 77), dz=True,
                            plan={F32: (True, 64, 1, 10), BF16: (True, 32, 1, 10)}),
    "320x136-red":     dict(N=320, M=136, z=False, mask=True, act=ACT_NONE, alpha=0.25, dbias="zero", gdiv=20, drop=None, dz=False,
                            plan={F32: (True, 64, 1, 10), BF16: (True, 32, 1, 10)}),
    "130x67-gelu":     dict(N=130, M=67, z=True, mask=True, act=ACT_GELU, alpha=0.5, dbias="acc", gdiv=20, drop=(0.15, 5), dz=True,
                            plan={F32: (False, 0, 1, 2), BF16: (False, 0, 1, 2)}),
    "130x67-red":      dict(N=130, M=67, z=False, mask=False, act=ACT_NONE, alpha=1.0, dbias="zero", gdiv=7, drop=None, dz=False,
                            plan={F32: (False, 0, 1, 2), BF16: (False, 0, 1, 2)}),
    "200x136-odd":     dict(N=200, M=136, odd=True, z=True, mask=True, act=ACT_SWISH, alpha=2.0, dbias="zero", gdiv=64, drop=None, dz=True,
                            plan={F32: (False, 0, 1, 2), BF16: (False, 0, 1, 2)}),
    "16417x8-relu":    dict(N=32 * 512 + 33, M=8, z=True, mask=True, act=ACT_RELU, alpha=1.0, dbias="acc", gdiv=20, drop=None, dz=True,
                            plan={F32: (True, 2, 1, 512), BF16: (True, 1, 1, 512)}),
    "77x520-swish":    dict(N=77, M=520, z=True, mask=False, act=ACT_SWISH, alpha=1.0, dbias="zero", gdiv=64, drop=(0.15, 9), dz=True,
                            plan={F32: (True, 64, 3, 3), BF16: (True, 64, 2, 3)}),
}


# ---- activations ------------------------------------------------------------------------------------------------------------------------
def act_grad(act, z):
    """act'(z) in z's dtype (float64: the reference; float32 on the GPU: ATen's evaluation of the same expression)."""
    if act == ACT_GELU:                                    # exact-erf GELU
        return 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0)))) + z * torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi))
    if act == ACT_SWISH:
        s = torch.sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    return torch.ones_like(z)


def row_rel(got, ref):
    """max over the row |got - ref| / max over the row |ref|, per row; rows whose reference is all zero must be all zero (-> 0)."""
    got, ref = got.double(), ref.double()
    den = ref.abs().amax(-1)
    err = (got - ref).abs().amax(-1)
    zero = den == 0
    assert bool((err[zero] == 0).all()), "a row whose reference is all zero holds a non-zero value"
    return torch.where(zero, torch.zeros_like(err), err / torch.where(zero, torch.ones_like(den), den))


def act_bar(aten_err, dtype):
    return torch.clamp(4.0 * aten_err, min=8.0 * torch.finfo(dtype).eps)


# ---- references: every function takes float64 inputs (the dtype-rounded values) and returns (ref, bar) ----------------------------------
def sum_bar(n, sabs, scale, ref, r=0.0, k=0):
    return SLACK * ((n + 5 + k) * U * sabs * scale.abs() + r * ref.abs())


def masked_mean_ref(x, mask, scale, r=0.0, k=0, post=None):
    """x (B, T, D), mask (B, T) bool | None -> dict(ref, bar (B, D); inv, inv_bar (B); dead (B): utterances with no valid frame, which
    the bars do not judge: inv = +inf, scaled mean NaN, unscaled mean 0 (reference summary_mixing.py:264-266)).
    post (B) | None: a factor applied after the scaled sum (k counts its products)."""
    m = torch.ones(x.shape[:2], dtype=torch.float64, device=x.device) if mask is None else mask.double()
    n = m.sum(1)
    dead = n == 0
    inv = 1.0 / torch.where(dead, torch.ones_like(n), n)
    sc = (inv if scale else torch.ones_like(inv)) * (post if post is not None else 1.0)
    ref = (x * m[..., None]).sum(1) * sc[:, None]
    bar = sum_bar(n[:, None], (x.abs() * m[..., None]).sum(1), sc[:, None], ref, r, k)
    return dict(ref=ref, bar=bar, inv=inv, inv_bar=SLACK * 5 * U * inv, dead=dead, n=n)


def bcast_ref(v, T, r, rowmask=None, keep=None, p=0.0):
    """v (B, D): the float64 product g * inv of the values the kernel was given -> (ref, bar) (B, T, D); rowmask (B, T) bool: masked rows
    are exact zeros; keep (B, T, D) bool + p: inverted dropout (scale 1 / (1 - float32(p)) as the host forms it)."""
    ref = v[:, None, :].expand(v.shape[0], T, v.shape[1]).clone()
    if rowmask is not None:
        ref = ref * rowmask.double()[..., None]
    if keep is not None:
        ref = ref * keep.double() / (1.0 - float(torch.tensor(p, dtype=torch.float32)))
    return ref, SLACK * (6 * U + r) * ref.abs()


def chunk_windows(T, chunk, left):
    """(T, T) float64 0 / 1: frame t of chunk c sees the frames of chunks [c - left, c] (left None: [0, c]) - DynChunkMask.dense()."""
    t = torch.arange(T)
    c = t // chunk
    hi = torch.clamp((c + 1) * chunk, max=T)
    lo = torch.zeros_like(c) if left is None else torch.clamp((c - left) * chunk, min=0)
    return ((t[None, :] >= lo[:, None]) & (t[None, :] < hi[:, None])).double()


def chunk_mean_ref(x, chunk, left, reverse, r):
    """x (B, T, D) -> (ref, bar): the dense window operator per utterance (windows never cross an utterance); reverse: its transpose."""
    Mx = chunk_windows(x.shape[1], chunk, left).to(x.device)
    W = Mx / Mx.sum(1, keepdim=True)                       # (T, T): row t = the weights of output frame t
    if reverse:
        W, n = W.t(), Mx.sum(0)
    else:
        n = Mx.sum(1)
    ref = torch.einsum("ts,bsd->btd", W, x)
    sabs = torch.einsum("ts,bsd->btd", W, x.abs())          # (the 1 / window length is inside W: |scale| = 1 below)
    return ref, sum_bar(n[None, :, None], sabs, torch.ones((), dtype=torch.float64, device=x.device), ref, r)


def laplace(T, decay, device="cpu"):
    """The reference's dense Laplace matrix decay^|i - j| in float64 (summary_mixing.py:316-365), decay as the float32 the kernel gets."""
    g = float(torch.tensor(decay, dtype=torch.float32))
    i = torch.arange(T, device=device)
    return torch.pow(torch.tensor(g, dtype=torch.float64, device=device), (i[None] - i[:, None]).abs().double())


def expdecay_ref(x, decay, reverse):
    """x (B, T, D) float64 -> (M x) / rowsum(M); reverse: the transposed operator M (x / rowsum(M))."""
    M = laplace(x.shape[1], decay, x.device)
    Wn = M / M.sum(1, keepdim=True)
    return torch.einsum("ji,bjd->bid" if reverse else "ij,bjd->bid", Wn, x)


def expdecay_f32(x, decay, reverse, dtype=torch.float32):
    """The float32 restatement of the O(T) operator: plain sequential two-sided recurrence f_t = x_t + g f_(t-1), g_t = x_t + g g_(t+1),
    (M x)_t = f_t + g_t - x_t, rowsum(M)_t = ((1 - g^(t+1)) + (1 - g^(T-t))) / (1 - g) - 1 with 1 - g^n = -expm1(n ln g).
    (dtype = float64: the same statements, to check them against the dense operator.)"""
    x = x.to(dtype)
    B, T, D = x.shape
    g = torch.tensor(decay, dtype=torch.float32).to(dtype)
    lng = torch.log(g.double()).to(dtype)
    t = torch.arange(T, dtype=dtype)
    den = ((-torch.expm1((t + 1) * lng) - torch.expm1((T - t) * lng)) / (1.0 - g) - 1.0).to(x.device)[None, :, None]
    g = g.to(x.device)
    if reverse:
        x = x / den
    f, b = torch.empty_like(x), torch.empty_like(x)
    acc = torch.zeros_like(x[:, 0])
    for i in range(T):
        acc = x[:, i] + g * acc
        f[:, i] = acc
    acc = torch.zeros_like(x[:, 0])
    for i in range(T - 1, -1, -1):
        acc = x[:, i] + g * acc
        b[:, i] = acc
    out = f + b - x
    return out if reverse else out / den


def act_mask_bwd_ref(dy, z, mask, act, alpha, keep, p, gdiv, dbias0, dgroup0):
    """dy, z (N, M) float64, mask (N) bool | None, keep (N, M) bool | None -> dict(o: the float64 terms alpha dy mask act'(z) D;
    dbias / dgroup: (ref, bar) of the accumulated column sums, n = the rows of the column resp. of the group)."""
    o = alpha * dy * (act_grad(act, z) if z is not None else 1.0)
    if mask is not None:
        o = o * mask.double()[:, None]
    if keep is not None:
        o = o * keep.double() / (1.0 - float(torch.tensor(p, dtype=torch.float32)))
    N, M = o.shape
    out = dict(o=o)
    one = torch.ones((), dtype=torch.float64, device=o.device)
    if dbias0 is not None:
        ref = dbias0 + o.sum(0)
        out["dbias"] = (ref, sum_bar(N + 1, dbias0.abs() + o.abs().sum(0), one, ref))          # (+ 1: the value accumulated onto)
    if dgroup0 is not None:
        G = dgroup0.shape[0]
        idx = (torch.arange(N, device=o.device) // gdiv)[:, None].expand(N, M)
        s = torch.zeros((G, M), dtype=torch.float64, device=o.device).scatter_add_(0, idx, o)
        sa = torch.zeros((G, M), dtype=torch.float64, device=o.device).scatter_add_(0, idx, o.abs())
        # a group that spans several row strips arrives as several atomic adds: still one sum of its rows in some order
        cnt = torch.bincount(torch.arange(N, device=o.device) // gdiv, minlength=G).double()[:, None]
        ref = dgroup0 + s
        out["dgroup"] = (ref, sum_bar(cnt + 1, dgroup0.abs() + sa, one, ref))
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def utterances(B, T, D, gen, offset=0.0):
    """(B, T, D) float32 values: unit noise around a per-utterance mean offset * b (chunk_mean: 10 b, so a window that crosses an
    utterance boundary shows at the edge rows)."""
    x = torch.randn((B, T, D), generator=gen)
    return x + offset * torch.arange(B, dtype=torch.float32)[:, None, None]


def mm_masks(B, T, TR, gen):
    """The masks of a masked-mean case -> {name: (B, T) bool}: random holes; utterance 0 with its only valid frame on the last row of the
    first TS range and the last utterance with exactly one valid frame elsewhere (the others random)."""
    holes = torch.rand((B, T), generator=gen) > 0.35
    holes[:, T // 2] = True                                # (at least one valid frame each)
    single = holes.clone()
    single[0] = False
    single[0, min(TR, T) - 1] = True
    if B > 1:
        single[B - 1] = False
        single[B - 1, T // 3] = True
    return {"holes": holes, "single": single}

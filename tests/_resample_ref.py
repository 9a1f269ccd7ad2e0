"""A float64 restatement of the resampler behind the recipes' wav_augment (speechbrain.augment.time_domain.Resample = torchaudio's
polyphase windowed-sinc filter at its defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), for the tests of
summarymixing_amd.augment.time_domain.  Neither package is installed here; DESIGN.md §I.16 is the specification:

  g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * 0.99, width = ceil(6 o / base), K = 2 width + o
  h[p][k] = sinc(pi t) cos^2(pi t / 12) base / o,  t = clamp(((k - width) / o - p / n) base, -6, 6)   (float64, rounded to float32)
  y[q n + p] = sum_k h[p][k] x[q o + k - width],  x zero outside [0, L),  L_out = ceil(n L / o)

plan_ref states the plan, gather_ref the output in the gather form (with S[i] = sum_k |h[p][k] x[...]|, the scale of the float32
dot-product bound), conv_ref the literal chain upstream runs (F.pad, a strided F.conv1d with the (n, 1, K) kernel, transpose,
reshape, slice).  CASES: what the GPU tests run; the CPU suite checks the two forms against each other on every one of them."""
import collections
import functools
import math

import torch
import torch.nn.functional as Fn

LOWPASS_WIDTH, ROLLOFF = 6, 0.99
SPAN_FLOATS = 4096                     # input samples one workgroup stages (csrc/resample.hip: RS_XS)

PlanRef = collections.namedtuple("PlanRef", "o n width K taps first h")      # h: (n, K) float32, first: list of n ints


@functools.lru_cache(maxsize=None)
def plan_ref(orig_freq, new_freq):
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_WIDTH * o / base)
    K = 2 * width + o
    k = torch.arange(K, dtype=torch.float64)[None, :]
    p = torch.arange(n, dtype=torch.float64)[:, None]
    t = (((k - width) / o - p / n) * base).clamp(-LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = torch.cos(t * math.pi / LOWPASS_WIDTH / 2) ** 2
    a = t * math.pi
    sinc = torch.where(a == 0, torch.ones_like(a), a.sin() / a)
    h = (sinc * (window * (base / o))).float()
    first, taps = [], 1
    for row in h:
        nz = torch.nonzero(row).flatten()
        first.append(int(nz[0]) if len(nz) else 0)
        taps = max(taps, int(nz[-1]) - int(nz[0]) + 1 if len(nz) else 1)
    return PlanRef(o, n, width, K, taps, first, h)


def runs_are_contiguous(h):
    """Every row's nonzero entries form one run."""
    for row in h:
        nz = torch.nonzero(row).flatten()
        if len(nz) == 0 or int(nz[-1]) - int(nz[0]) + 1 != len(nz):
            return False
    return True


def out_len(o, n, L):
    return -((-n * L) // o)


def tile_blocks(plan):
    """n-sample output blocks per workgroup tile: (Q - 1) o + K + taps input samples, + 3 for the alignment of the span's start, fit
    the staged span."""
    return (SPAN_FLOATS - plan.K - plan.taps - 3) // plan.o


def dense_taps(o, n, K, first, weights):
    """(n, K) float32 from a plan image's first[] and (n, taps) weights."""
    h = torch.zeros(n, K, dtype=torch.float32)
    for p in range(n):
        f = int(first[p])
        m = min(weights.shape[1], K - f)
        h[p, f:f + m] = weights[p, :m]
    return h


def gather_ref(x, plan, h=None):
    """x (B, L) -> (y, S), both (B, L_out) float64: y[b][q n + p] = sum_k h[p][k] x[b][q o + k - width] and the same sum of absolute
    values.  h: other taps than plan_ref's (the library's own, for the bit-exact tests)."""
    o, n, width, K = plan.o, plan.n, plan.width, plan.K
    h = (plan.h if h is None else h).double()
    B, L = x.shape
    Lo = out_len(o, n, L)
    nblk = -(-Lo // n)
    xp = torch.zeros(B, (nblk - 1) * o + K + width, dtype=torch.float64)
    xp[:, width:width + L] = x.double()
    idx = (torch.arange(nblk)[:, None] * o + torch.arange(K)[None, :])        # sample q o + k - width sits at q o + k of xp
    win = xp[:, idx]                                                           # (B, nblk, K)
    y = torch.einsum("pk,bqk->bqp", h, win).reshape(B, nblk * n)[:, :Lo]
    S = torch.einsum("pk,bqk->bqp", h.abs(), win.abs()).reshape(B, nblk * n)[:, :Lo]
    return y.contiguous(), S.contiguous()


def conv_ref(x, plan, dtype=torch.float64):
    """The literal chain of torchaudio.functional.resample (_apply_sinc_resample_kernel) in `dtype`."""
    o, n, width = plan.o, plan.n, plan.width
    B, L = x.shape
    kernel = plan.h.to(dtype)[:, None, :]
    xp = Fn.pad(x.to(dtype)[:, None, :], (width, width + o))
    y = Fn.conv1d(xp, kernel, stride=o)                                        # (B, n, blocks)
    y = y.transpose(1, 2).reshape(B, -1)
    return y[..., :out_len(o, n, L)]


RATIOS = [(20, 19), (20, 21), (10, 9), (10, 11), (100, 97), (2, 1), (1, 2), (441, 160), (160, 441)]
B_MAX = 3


def lengths(orig_freq, new_freq):
    """The two zero-filled edges (1, 5 < width, o), the block seams (3 o and its neighbours) and the tile seams (one workgroup's input
    span + 37, two spans - 1); 441 -> 160 also at nine spans + 1, where a workgroup takes a second tile."""
    plan = plan_ref(orig_freq, new_freq)
    o, span = plan.o, tile_blocks(plan) * plan.o
    out = {1, 5, o, 3 * o, 3 * o - 1, 3 * o + 1, span + 37, 2 * span - 1}
    if (orig_freq, new_freq) == (441, 160):
        out.add(9 * span + 1)
    return sorted(out)


CASES = [(a, b, L) for a, b in RATIOS for L in lengths(a, b)]


@functools.lru_cache(maxsize=None)
def case_input(L):
    g = torch.Generator().manual_seed(1000 + L)
    return torch.randn(B_MAX, L, generator=g, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def case_ref(orig_freq, new_freq, L):
    """(x (3, L) float32, y, S) of a case; B = 1 is row 0 of all three.  Computed once per process and left unchanged."""
    x = case_input(L)
    y, S = gather_ref(x, plan_ref(orig_freq, new_freq))
    return x, y, S

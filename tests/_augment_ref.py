"""CPU statements of the feature augmentation (summarymixing_amd.augment) for the tests.

Two independent forms of what smx_specaug_apply computes from an explicit parameter block:
  gather_ref  - the gather-form specification: per output row an integer position num / den, four taps clamped into the segment,
                torch's cubic coefficients; in float64 it is the reference, in float32 the emulation whose distance from the
                reference sets the float32 bar;
  chain_ref   - the literal upstream chain in float64: two masked_fill (upstream's boolean expression) and two
                torch.nn.functional.interpolate(mode="bicubic", align_corners=True) calls on slices.
And one of what smx_specaug_draw draws: draw_block, the counter-based hash in Python integers.
The cases the GPU tests run are listed here (CASES / case_blocks), so that the CPU suite can check that they are admissible."""
import functools

import torch

HDR = 8
WARP, TIME, FREQ = 1, 2, 4


# ---- parameter blocks ---------------------------------------------------------------------------------------------------------
def make_block(B, flags, c, w, n_time, time_drops, n_time_cap, n_freq, freq_drops, n_freq_cap):
    """The int32 block of include/smx.h as a CPU tensor.  time_drops / freq_drops: per utterance a list of (pos, len), padded with
    (0, 1 << 20) - pairs at and beyond n_time / n_freq must be ignored, and this padding would wipe everything if one were read."""
    words = [flags, c, w, n_time, n_freq, 0, 0, 0]
    for drops, cap in ((time_drops, n_time_cap), (freq_drops, n_freq_cap)):
        for b in range(B):
            row = list(drops[b]) if cap else []
            assert len(row) <= cap
            row = row + [(0, 1 << 20)] * (cap - len(row))
            for pos, ln in row:
                words += [pos, ln]
    return torch.tensor(words, dtype=torch.int32)


def parse_block(blk, B, n_time_cap, n_freq_cap):
    v = [int(a) for a in blk.tolist()]
    flags, c, w, n_time, n_freq = v[:5]
    n_time, n_freq = min(n_time, n_time_cap), min(n_freq, n_freq_cap)
    o = HDR
    td = [[(v[o + 2 * (b * n_time_cap + i)], v[o + 2 * (b * n_time_cap + i) + 1]) for i in range(n_time)] for b in range(B)]
    o += 2 * B * n_time_cap
    fd = [[(v[o + 2 * (b * n_freq_cap + i)], v[o + 2 * (b * n_freq_cap + i) + 1]) for i in range(n_freq)] for b in range(B)]
    return flags, c, w, (td if flags & TIME else [[] for _ in range(B)]), (fd if flags & FREQ else [[] for _ in range(B)])


def dropped(drops, B, D):
    """(B, D) bool: element d of row b is dropped iff some pair has pos <= d < pos + len (plain loops)."""
    m = torch.zeros(B, D, dtype=torch.bool)
    for b in range(B):
        for pos, ln in drops[b]:
            for d in range(max(pos, 0), min(pos + ln, D)):
                m[b, d] = True
    return m


def upstream_mask(drops, B, D):
    """The same set as upstream's SpectrogramDrop writes it: (pos <= arange) * (arange < pos + len), any over the drops."""
    n = len(drops[0])
    if n == 0:
        return torch.zeros(B, D, dtype=torch.bool)
    pos = torch.tensor([[p for p, _ in drops[b]] for b in range(B)]).view(B, n, 1)
    ln = torch.tensor([[q for _, q in drops[b]] for b in range(B)]).view(B, n, 1)
    arange = torch.arange(D).view(1, 1, -1)
    return ((pos <= arange) * (arange < (pos + ln))).any(dim=1)


# ---- the gather form ----------------------------------------------------------------------------------------------------------
def _plan(T, flags, c, w):
    """Per output row: the four source rows (clamped into the segment), the integer fraction rem / den."""
    src, rem, den = [], [], []
    for t in range(T):
        lo, hi, i, r, d = 0, T, t, 0, 1
        if flags & WARP:
            if t < w:
                lo, hi, n_in, n_out, tt = 0, c, c, w, t
            else:
                lo, hi, n_in, n_out, tt = c, T, T - c, T - w, t - w
            if n_out > 1:
                num, d = tt * (n_in - 1), n_out - 1
                i, r = lo + num // d, num % d
            else:
                i = lo
        src.append([min(max(i - 1 + k, lo), hi - 1) for k in range(4)])
        rem.append(r)
        den.append(d)
    return torch.tensor(src), torch.tensor(rem), torch.tensor(den)


def gather_ref(x, blk, n_time_cap, n_freq_cap, dtype=torch.float64):
    """x (B, T, F) -> the augmented tensor, every operation in `dtype` (float64: the reference; float32: the emulation of the
    kernel's arithmetic - the fraction rounded once, the two cubics as written in the specification, a four-term sum in tap
    order)."""
    B, T, F = x.shape
    flags, c, w, td, fd = parse_block(blk, B, n_time_cap, n_freq_cap)
    xd = x.to(dtype).clone()
    xd[dropped(td, B, T)] = 0                                # drops first: the warp interpolates across the zeroed frames
    xd = xd.masked_fill(dropped(fd, B, F).unsqueeze(1), 0)
    src, rem, den = _plan(T, flags, c, w)
    A = -0.75
    fr = rem.to(dtype) / den.to(dtype)

    def c1(v):
        return ((A + 2) * v - (A + 3)) * v * v + 1

    def c2(v):
        return ((A * v - 5 * A) * v + 8 * A) * v - 4 * A
    wts = [c2(fr + 1), c1(fr), c1(1 - fr), c2(2 - fr)]
    out = None
    for k in range(4):
        term = wts[k].to(dtype).view(1, T, 1) * xd[:, src[:, k], :]
        out = term if out is None else out + term
    return out


def must_be_zero(shape, blk, n_time_cap, n_freq_cap):
    """(B, T, F) bool: outputs that are exact zeros whatever x holds - a dropped column, or a row all of whose taps with a non-zero
    weight are dropped frames."""
    B, T, F = shape
    flags, c, w, td, fd = parse_block(blk, B, n_time_cap, n_freq_cap)
    tm, fm = dropped(td, B, T), dropped(fd, B, F)
    src, rem, _ = _plan(T, flags, c, w)
    rows = torch.zeros(B, T, dtype=torch.bool)
    for t in range(T):
        taps = src[t].tolist() if int(rem[t]) else [int(src[t][1])]
        rows[:, t] = tm[:, taps].all(dim=1)
    return rows.unsqueeze(2) | fm.unsqueeze(1)


# ---- the literal chain --------------------------------------------------------------------------------------------------------
def chain_ref(x, blk, n_time_cap, n_freq_cap):
    """Upstream's three modules one after another in float64, on a copy."""
    import torch.nn.functional as Fn
    B, T, F = x.shape
    flags, c, w, td, fd = parse_block(blk, B, n_time_cap, n_freq_cap)
    y = x.to(torch.float64).clone()
    if flags & TIME:
        y = y.masked_fill_(upstream_mask(td, B, T).unsqueeze(2), 0.0)
    if flags & FREQ:
        y = y.masked_fill_(upstream_mask(fd, B, F).unsqueeze(1), 0.0)
    if flags & WARP:
        y = y.unsqueeze(1)
        left = Fn.interpolate(y[:, :, :c], (w, F), mode="bicubic", align_corners=True)
        right = Fn.interpolate(y[:, :, c:], (T - w, F), mode="bicubic", align_corners=True)
        y[:, :, :w] = left
        y[:, :, w:] = right
        y = y.squeeze(1)
    return y


# ---- the draw -----------------------------------------------------------------------------------------------------------------
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _mix32(v):
    v ^= v >> 16
    v = (v * 0x21F0AAAD) & _M32
    v ^= v >> 15
    v = (v * 0x735A2D97) & _M32
    v ^= v >> 15
    return v


def _hash(seed, what, idx):
    return _mix32(_mix32((idx + what * 0x9E3779B9) & _M32) ^ _mix32(((seed & _M32) + 0x5BD1E995) & _M32) ^ (seed >> 32))


def _rint(h, lo, hi_excl):
    return lo + ((h * max(hi_excl - lo, 1)) >> 32)


def draw_block(B, T, F, stages, time_drop, freq_drop, window, seed, counter=None):
    """What smx_specaug_draw writes for (seed, device step counter): the list of int32 words."""
    if counter is not None:
        seed ^= (counter * 0x9E3779B97F4A7C15) & _M64
    tcap = time_drop[3] if stages & TIME else 0
    fcap = freq_drop[3] if stages & FREQ else 0
    flags, c, w = stages & (TIME | FREQ), 0, 0
    if stages & WARP and T - window > window:
        c = _rint(_hash(seed, 2, 0), window, T - window)
        w = _rint(_hash(seed, 3, 0), c - window + 1, c + window + 1)
        flags |= WARP
    words = [flags, c, w, _rint(_hash(seed, 0, 0), time_drop[2], time_drop[3] + 1) if tcap else 0,
             _rint(_hash(seed, 1, 0), freq_drop[2], freq_drop[3] + 1) if fcap else 0, 0, 0, 0]
    for i in range(B * tcap):
        words += [_rint(_hash(seed, 4, i), 0, T), _rint(_hash(seed, 5, i), time_drop[0], time_drop[1])]
    for i in range(B * fcap):
        words += [_rint(_hash(seed, 6, i), 0, F), _rint(_hash(seed, 7, i), freq_drop[0], freq_drop[1])]
    return words


# ---- the cases of tests/test_augment_gpu.py -----------------------------------------------------------------------------------
WINDOW = 5
N_TIME_CAP, N_FREQ_CAP = 5, 3
# (B, T, F) -> exhaustive over (c, w)?   Tile boundaries (a workgroup takes 51 rows at F = 80 and 64 at F = 7: T = 130, 200, 257 end
# in a partial tile), F not a multiple of 4 (5, 7), more than one workgroup per utterance, w = 1 and T - w = 1.
CASES = {(3, 11, 5): True, (2, 12, 80): True, (2, 37, 80): False, (2, 130, 7): False, (1, 257, 80): False, (4, 200, 80): False}


def case_input(shape):
    g = torch.Generator().manual_seed(1000 * shape[0] + 10 * shape[1] + shape[2])
    return torch.randn(shape, generator=g, dtype=torch.float64) * 2.0 + 0.5


def _pairs(T, exhaustive):
    if exhaustive:
        return [(c, w) for c in range(WINDOW, T - WINDOW) for w in range(c - WINDOW + 1, c + WINDOW + 1)]
    m = T // 2
    return [(WINDOW, 1), (T - WINDOW - 1, T - 1), (m, m + 3), (m, m - 4), (31, 33), (m + 1, m + 1)]


def _drops(B, T, F, c):
    # time: a stripe on row 0, one clipped at T - 1, two overlapping ones straddling c; frequency: one clipped at F, one inside
    td = [[(0, 2), (T - 2, 5), (c - 2 - (b % 2), 4), (c - 1, 3)] for b in range(B)]
    fd = [[(F - 3, 6), (1 + b, 2)] for b in range(B)]
    return td, fd


def case_blocks(shape):
    """[(label, block)] of one case: every (c, w) with all three stages; for the first pair also the warp alone and with each drop."""
    B, T, F = shape
    out = []
    for n, (c, w) in enumerate(_pairs(T, CASES[shape])):
        td, fd = _drops(B, T, F, c)
        for flags in ((WARP | TIME | FREQ, WARP, WARP | TIME, WARP | FREQ) if n == 0 else (WARP | TIME | FREQ,)):
            out.append((f"c{c}w{w}f{flags}", make_block(B, flags, c, w, 4, td, N_TIME_CAP, 2, fd, N_FREQ_CAP)))
    return out


@functools.lru_cache(maxsize=None)
def case_refs(shape, bf16=False):
    """[(label, block, x, float64 reference, float32 emulation, must-be-zero mask)], computed once per process.  bf16: the input is
    rounded to bfloat16 first (the reference and the emulation start from the values the kernel reads)."""
    x = case_input(shape)
    x = x.to(torch.bfloat16) if bf16 else x.to(torch.float32)
    res = []
    for label, blk in case_blocks(shape):
        ref = gather_ref(x, blk, N_TIME_CAP, N_FREQ_CAP, torch.float64)
        emu = gather_ref(x, blk, N_TIME_CAP, N_FREQ_CAP, torch.float32)
        res.append((label, blk, x, ref, emu, must_be_zero(shape, blk, N_TIME_CAP, N_FREQ_CAP)))
    return res

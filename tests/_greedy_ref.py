"""Plain restatement of greedy transducer decoding for the tests (SpeechBrain's transducer_greedy_decode, at most one symbol per
frame), in torch on the CPU.  Default float64 - the yardstick of tests/test_greedy_gpu.py, itself checked against an independent
loop built from torch.nn.LSTMCell in tests/test_greedy_cpu.py.  The same loop in float32 with h, pdec and a rounded to the operand
dtype is the EMULATION: what the number formats alone cost.  Nothing here calls the code under test.

Per row and frame: a = act(enc[b,t] + pdec[b]); z = a W_lin^T + b_lin; k = argmax z (lowest index on a tie); k != blank: append k,
score += z[k] - logsumexp(z), one LSTM step on token k, pdec = h W_proj^T; blank: nothing changes.  The start state is one LSTM step
from h = c = 0 on the blank (a zero input row: the gates are the two biases alone)."""
import functools

import torch

from tests._lstm_ref import bf16_round, col_of

# (B, T, V, H, J, blank, seed): the shapes of the GPU tests; the seeds are those at which the case is ADMISSIBLE
# (tests/test_greedy_cpu.py::test_cases_are_admissible asserts it on the reference alone)
CASES = {
    "small": (3, 24, 20, 64, 64, 0, 0),
    "blank7": (5, 40, 30, 32, 64, 7, 0),
    "two_tiles": (17, 16, 12, 64, 128, 11, 0),
    "one_frame": (1, 1, 12, 32, 64, 3, 0),
    "long": (2, 200, 50, 64, 64, 25, 0),
    "recipe": (4, 48, 1000, 512, 640, 0, 0),
    "v300": (3, 20, 300, 64, 64, 150, 0),
    "t8": (2, 8, 20, 32, 64, 4, 0),
}
EXACT = ("small", "blank7", "two_tiles", "one_frame", "long", "recipe", "v300", "t8")   # the token-exact fp32 cases
MIN_FRAMES_FOR_MIX = 16     # the 25-75 % emission rule is asked of cases with at least this many frames (one_frame has one)
TIE = (2, 16, 12, 32, 64, 0, 1, 5, 9)                                        # a case whose W_lin rows 5 and 9 (and their biases) are identical


def gelu(x):
    return torch.nn.functional.gelu(x)


def rounder(dtype):
    return bf16_round if dtype == torch.bfloat16 else (lambda t: t)


def _uniform(g, shape, k):
    return (torch.rand(shape, generator=g) * 2 - 1) * k


def make_case(B, T, V, H, J, blank, seed, dtype=torch.float32, tie=None):
    """Uniform weights, an N(0, 1) enc, and a transducer_lin bias whose blank entry is the median shortfall of the blank logit (taken at
    the start state), so the blank wins about half the frames.  Weight matrices and enc are rounded to `dtype` (the biases stay fp32,
    as the kernels read them).  -> (params dict of fp32 tensors, enc (B, T, J) fp32)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * V + H + J + B)
    r = rounder(dtype)
    kh = H ** -0.5
    p = {"w_ih": r(_uniform(g, (4 * H, V - 1), kh)), "w_hh": r(_uniform(g, (4 * H, H), kh)), "b_ih": _uniform(g, (4 * H,), kh),
         "b_hh": _uniform(g, (4 * H,), kh), "w_proj": r(_uniform(g, (J, H), 2 * kh)), "w_lin": r(_uniform(g, (V, J), 4 * J ** -0.5)),
         "b_lin": _uniform(g, (V,), 0.5)}
    if tie is not None:
        p["w_lin"][tie[1]] = p["w_lin"][tie[0]]
        p["b_lin"][tie[1]] = p["b_lin"][tie[0]]
    enc = r(torch.randn((B, T, J), generator=g))
    h, c, pdec = start_state(p, B, torch.float64)
    z = gelu(enc.double() + pdec.unsqueeze(1)) @ p["w_lin"].double().t() + p["b_lin"].double()
    other = z.clone()
    other[..., blank] = -float("inf")
    short = other.max(-1).values - z[..., blank]
    # (the median of fewer than 8 frames can BE one frame's shortfall - an exact tie by construction: stay a quarter below it)
    p["b_lin"][blank] += float(short.median()) - (0.25 if B * T < 8 else 0.0)
    return p, enc


@functools.lru_cache(maxsize=None)
def case(name, dtype=torch.float32):
    """One named case: (params, enc, blank), made once and shared; treat as read-only."""
    if name == "tie":
        B, T, V, H, J, blank, seed, k1, k2 = TIE
        p, enc = make_case(B, T, V, H, J, blank, seed, dtype, tie=(k1, k2))
    else:
        B, T, V, H, J, blank, seed = CASES[name]
        p, enc = make_case(B, T, V, H, J, blank, seed, dtype)
    return p, enc, blank


def _lstm_step(p, tok, h, c, blank, dt):
    """One step of the one-layer LSTM on token `tok` (B,) from (h, c): the input product is a column gather of W_ih."""
    H = h.shape[1]
    col = col_of(tok, blank)
    gx = p["w_ih"].to(dt).t()[col.clamp(min=0)] * (col >= 0).to(dt).unsqueeze(-1) + (p["b_ih"].to(dt) + p["b_hh"].to(dt))
    z = gx + h @ p["w_hh"].to(dt).t()
    i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
    c = f * c + i * g
    return o * torch.tanh(c), c


def start_state(p, B, dt=torch.float64, rnd=None):
    H = p["w_hh"].shape[1]
    rnd = rnd or (lambda t: t)
    h, c = _lstm_step(p, torch.full((B,), 0, dtype=torch.long), torch.zeros(B, H, dtype=dt), torch.zeros(B, H, dtype=dt), 0, dt)
    h = rnd(h)
    return h, c, rnd(h @ p["w_proj"].to(dt).t())


def decode(p, enc, blank, lengths=None, state=None, dtype=torch.float64, rnd=None, forced=None, exclude=None):
    """-> dict: hyps / frames (lists of lists of ints), n (B), scores (B), state = (h, c, pdec, seen), choice (B, T) the argmax per
    frame, z (B, T, V) the logits, gap (B, T) best minus second-best logit (inf on frames beyond a row's length).
    lengths: absolute frames per row (None: all T).  rnd: applied to h, pdec and a where the kernels store them in the operand dtype.
    forced (B, T) ints: the token to take at each frame instead of the argmax (a foreign trajectory replayed on this arithmetic).
    exclude: a vocabulary column left out of `gap` (the twin of a deliberately tied column)."""
    dt = dtype
    rnd = rnd or (lambda t: t)
    B, T, J = enc.shape
    V = p["w_lin"].shape[0]
    if state is None:
        h, c, pdec = start_state(p, B, dt, rnd)
        seen, score = torch.zeros(B, dtype=torch.long), torch.zeros(B, dtype=dt)
    else:
        h, c, pdec, seen, score = (t.clone() for t in state)
        h, c, pdec, score = h.to(dt), c.to(dt), pdec.to(dt), score.to(dt)
    ln = torch.full((B,), T, dtype=torch.long) if lengths is None else lengths.long()
    Wl, bl, Wp = p["w_lin"].to(dt), p["b_lin"].to(dt), p["w_proj"].to(dt)
    hyps, frames = [[] for _ in range(B)], [[] for _ in range(B)]
    zs, gaps, choice = [], [], []
    e = enc.to(dt)
    for t in range(T):
        a = rnd(gelu(e[:, t] + pdec))
        z = a @ Wl.t() + bl
        zs.append(z)
        zg = z
        if exclude is not None:
            zg = z.clone()
            zg[:, exclude] = -float("inf")
        top = torch.topk(zg, 2, dim=1).values
        live = t < ln
        gaps.append(torch.where(live, top[:, 0] - top[:, 1], torch.full_like(top[:, 0], float("inf"))))
        k = torch.argmax(z, 1) if forced is None else forced[:, t].long()
        choice.append(k)
        emit = live & (k != blank)
        lp = z.gather(1, k.view(B, 1)).view(B) - torch.logsumexp(z, 1)
        h2, c2 = _lstm_step(p, k, h, c, blank, dt)
        h2 = rnd(h2)
        p2 = rnd(h2 @ Wp.t())
        m = emit.unsqueeze(1)
        h, c, pdec = torch.where(m, h2, h), torch.where(m, c2, c), torch.where(m, p2, pdec)
        score = score + torch.where(emit, lp, torch.zeros_like(lp))
        for b in range(B):
            if emit[b]:
                hyps[b].append(int(k[b]))
                frames[b].append(int(seen[b]))
        seen = seen + live.long()
    return {"hyps": hyps, "frames": frames, "n": torch.tensor([len(x) for x in hyps]), "scores": score, "state": (h, c, pdec, seen, score),
            "choice": torch.stack(choice, 1), "z": torch.stack(zs, 1), "gap": torch.stack(gaps, 1)}


def ref_and_emu(p, enc, blank, operand_dtype, **kw):
    """(float64 reference, float32 emulation with the operand dtype's roundings) of one decode."""
    return decode(p, enc, blank, **kw), decode(p, enc, blank, dtype=torch.float32, rnd=rounder(operand_dtype), **kw)


def deviation(ref, emu):
    """The emulation's distance from the reference on one trajectory, both relative: (largest logit deviation / max |z_ref|,
    largest score deviation / max |score_ref|)."""
    dz = float((emu["z"].double() - ref["z"]).abs().max() / ref["z"].abs().max())
    ds = float((emu["scores"].double() - ref["scores"]).abs().max() / ref["scores"].abs().max().clamp(min=1e-30))
    return dz, ds


def choice_from(tokens, frames, counts, seen0, T, blank):
    """The per-frame choice (B, T) a decode made, from its outputs: the blank except where a token was emitted.  frames count over the
    whole stream; seen0 (B) is the rows' frame count before this call (all rows decode all T frames)."""
    B = len(counts)
    ch = torch.full((B, T), blank, dtype=torch.long)
    for b in range(B):
        for i in range(int(counts[b])):
            ch[b, int(frames[b][i]) - int(seen0[b])] = int(tokens[b][i])
    return ch

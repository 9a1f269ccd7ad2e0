"""A float64 restatement of CTC greedy decoding (upstream's ctc_greedy_decode / filter_ctc_output: row arg-max, merge repeats, drop
blanks), written for the tests of csrc/ctcdec.hip, and the named cases those tests share.  CPU only, no library code.

  best_path(x)      rows of scores -> (lowest index of the row maximum, max - logsumexp); -1 / NaN for a row without a number
  collapse(...)     the merge-and-filter with the state a stream carries (previous token, frames seen, tokens emitted, score)
  head_case(name)   operands of the fused head, their float64 logits and an emulation of the kernel's arithmetic
"""
import math

import torch

NO_TOKEN = -(1 << 31)


def best_path(x):
    """x (N, V) float64.  NaNs never win; a row with any NaN has lp NaN; a row of only NaNs has token -1."""
    x = x.double()
    N, V = x.shape
    tok, lp = [], []
    for n in range(N):
        row = x[n]
        num = ~torch.isnan(row)
        if not bool(num.any()):
            tok.append(-1); lp.append(float("nan"))
            continue
        m = float(row[num].max())
        tok.append(next(i for i in range(V) if bool(num[i]) and float(row[i]) == m))        # the lowest index among equals
        lp.append(float("nan") if not bool(num.all()) else -math.log(float(torch.exp(row - m).sum())))
    return torch.tensor(tok, dtype=torch.int64), torch.tensor(lp, dtype=torch.float64)


def start_state(B):
    return dict(prev=[NO_TOKEN] * B, seen=[0] * B, n_tok=[0] * B, score=[0.0] * B)


def collapse(tok, lp, blank, in_len=None, state=None, start=None):
    """tok (B, T) ints, lp (B, T) floats -> dict(hyps, frames: B lists - this call's emissions; state: the state after the call).
    Frame t < in_len[b] emits iff tok[t] != blank and tok[t] >= 0 and tok[t] != (prev if t == 0 else tok[t - 1])."""
    B = len(tok)
    st = {k: list(v) for k, v in (state or start_state(B)).items()}
    hyps, frames = [], []
    for b in range(B):
        if start is not None and start[b]:
            st["prev"][b], st["seen"][b], st["n_tok"][b], st["score"][b] = NO_TOKEN, 0, 0, 0.0
        T = len(tok[b])
        L = T if in_len is None else max(0, min(int(in_len[b]), T))
        h, f = [], []
        prev = st["prev"][b]
        for t in range(L):
            k = int(tok[b][t])
            if k != blank and k >= 0 and k != prev:
                h.append(k); f.append(st["seen"][b] + t)
            prev = k
        st["prev"][b] = prev
        st["seen"][b] += L
        st["n_tok"][b] += len(h)
        st["score"][b] += math.fsum(float(v) for v in lp[b][:L])
        hyps.append(h); frames.append(f)
    return dict(hyps=hyps, frames=frames, state=st)


def brute_force(string, blank):
    """upstream, literally: itertools.groupby, then filter"""
    from itertools import groupby
    return [k for k in (g[0] for g in groupby(string)) if k != blank]


# ---- token strings for the collapse tests: (B, T) with runs, blanks and a repeat that straddles frames 63 | 64
def token_rows(B, T, V, blank, seed):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        row = []
        while len(row) < T:
            k = blank if float(torch.rand((), generator=g)) < 0.4 else int(torch.randint(0, V, (), generator=g))
            row += [k] * int(torch.randint(1, 4, (), generator=g))
        row = row[:T]
        if T > 64:
            k = (blank + 1) % V
            row[61] = blank
            row[62:66] = [k] * 4                       # one token over frames 62..65: emitted once, whatever the chunk boundary
        rows.append(row[:T])
    return rows


# ---- fused-head cases.  X rows point at a planted column of W (strength `a`) under noise, so the top-2 gap of every row is wide:
# what the token-exact GPU tests need (tests/test_ctcdec_cpu.py: test_head_cases_are_admissible).  name: (N, K, V, a, bias kind, seed,
# lp floor fp32, lp floor bf16); the floors are the emulation's deviation from float64 measured on the CPU, relative to
# max(1, max |lp|), rounded up - the CPU test holds them against a fresh measurement.
HEAD_CASES = {
    "k64_v2": (111, 64, 2, 6.0, "rand", 1, 1e-7, 1e-7),
    "k64_v129": (111, 64, 129, 6.0, "rand", 2, 1.4e-6, 5e-7),
    "k64_v300": (111, 64, 300, 6.0, "rand", 3, 2e-6, 7e-7),
    "k128_v2": (111, 128, 2, 6.0, "rand", 4, 1e-7, 1e-7),
    "k128_v129": (111, 128, 129, 6.0, "none", 5, 1.4e-6, 1e-6),
    "k128_v300": (111, 128, 300, 6.0, "rand", 6, 2.8e-6, 1.4e-6),
    "k640_v1000": (111, 640, 1000, 8.0, "rand", 7, 1.8e-6, 1.4e-6),
    "all_negative_v129": (111, 64, 129, 6.0, "negative", 8, 1.5e-6, 1.2e-6),      # every logit < 0: a zero pad column would win
    "max_in_ragged_tile": (111, 64, 300, 6.0, "last_tile", 9, 1.3e-6, 7e-7),    # every row's maximum in columns 256..299
}
DTYPES = (torch.float32, torch.bfloat16)


def head_case(name, dtype):
    """-> dict(X (N, K), W (V, K), bias (V) fp32 or None: the operands rounded to dtype (as fp32 tensors);
    z64: the float64 logits of those rounded operands; emu: the logits as the kernel's arithmetic gives them on the CPU (fp32
    operands / bf16 operands, fp32 accumulation); emu_stored: emu rounded to dtype, what the unfused pair reads back)."""
    N, K, V, a, kind, seed, _, _ = HEAD_CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    W = torch.randn(V, K, generator=g) / math.sqrt(K)
    if kind == "last_tile":
        col = torch.randint(256, V, (N,), generator=g)
    else:
        col = torch.randint(0, V, (N,), generator=g)
        col[1::3] = col[0::3][:len(col[1::3])]                    # repeats, as a CTC head emits them
    X = a * W[col] / (W[col] ** 2).sum(1, keepdim=True) + 0.5 * torch.randn(N, K, generator=g) / math.sqrt(K)
    if kind == "none":
        bias = None
    else:
        bias = 0.1 * torch.randn(V, generator=g)
        if kind == "negative":
            bias = bias - 40.0
    X, W = X.to(dtype).float(), W.to(dtype).float()
    z64 = X.double() @ W.double().t() + (bias.double() if bias is not None else 0.0)
    emu = X @ W.t()                                               # fp32 accumulation of the rounded operands
    if bias is not None:
        emu = emu + bias
    return dict(X=X, W=W, bias=bias, z64=z64, emu=emu, emu_stored=emu.to(dtype).float(), col=col)


def lp_rel(lp, ref):
    """max |lp - ref| / max(1, max |ref|): the metric of the lp bars"""
    ref = ref.double()
    return float((lp.double() - ref).abs().max() / max(1.0, float(ref.abs().max())))

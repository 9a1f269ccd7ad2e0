"""Plain restatement of the prediction network's LSTM for the tests: the recurrence and its explicit BPTT (no autograd), the
one-hot input as a gather / scatter with per-token keep factors, and the dense input.  Default float64 - the yardstick of the
GPU stage tests, itself checked against torch.nn.LSTM(..., batch_first=True).double() with autograd in tests/test_prednet_cpu.py.
The same code in float32 with `round_h` / `round_g` set is the FLOOR emulation: what the number formats alone cost (h rounded
to the operand dtype where it is stored and fed back, the gate gradients rounded where they are stored as GEMM operands).
Nothing here calls the code under test.  Gate order i, f, g, o (torch's)."""
import torch


def col_of(tokens, blank):
    """Column of each token in the (V - 1)-wide one-hot row: k below the blank, k - 1 above it, -1 for the blank itself."""
    t = tokens.long()
    return torch.where(t == blank, torch.full_like(t, -1), torch.where(t < blank, t, t - 1))


def onehot_rows(tokens, V, blank, dtype=torch.float64):
    """(..., V - 1) one-hot rows, the blank a zero row (SpeechBrain's Embedding(consider_as_one_hot=True))."""
    col = col_of(tokens, blank)
    out = torch.zeros(tuple(tokens.shape) + (V - 1,), dtype=dtype)
    hot = col >= 0
    out[hot] = torch.nn.functional.one_hot(col[hot], V - 1).to(dtype)
    return out


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def gates_dense(x, w_ih, b_ih, b_hh):
    """x (B, U, I) -> Gx (B, U, 4H) = x W_ih^T + b_ih + b_hh."""
    return x @ w_ih.t() + (b_ih + b_hh)


def gates_onehot(tokens, keep, w_ih, b_ih, b_hh, blank):
    """Gx[b, u] = keep[b, u] W_ih[:, col(token)] + b_ih + b_hh: a column gather, a zero contribution for the blank."""
    col = col_of(tokens, blank)
    g = w_ih.t()[col.clamp(min=0)] * (col >= 0).to(w_ih.dtype).unsqueeze(-1)
    if keep is not None:
        g = g * keep.to(w_ih.dtype).unsqueeze(-1)
    return g + (b_ih + b_hh)


def recurrence(gx, w_hh, h0=None, c0=None, round_h=None):
    """gx (B, U, 4H) -> (Y (B, U, H), h_n, c_n, saved).  round_h (a function or None) is applied to h where it is stored / fed back."""
    B, U, G = gx.shape
    H = G // 4
    dt = gx.dtype
    h = torch.zeros(B, H, dtype=dt) if h0 is None else h0.to(dt)
    c = torch.zeros(B, H, dtype=dt) if c0 is None else c0.to(dt)
    hs, cs, acts = [h], [c], []
    for u in range(U):
        z = gx[:, u] + h @ w_hh.t()
        i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        if round_h is not None:
            h = round_h(h)
        hs.append(h)
        cs.append(c)
        acts.append((i, f, g, o))
    return torch.stack(hs[1:], 1), h, c, (hs, cs, acts)


def bptt(saved, w_hh, dY=None, dhn=None, dcn=None, round_g=None):
    """Explicit backward of `recurrence`: -> (dG (B, U, 4H), dh0, dc0, dW_hh, db) with db = the column sums of dG (both biases)."""
    hs, cs, acts = saved
    U = len(acts)
    B, H = hs[0].shape
    dt = w_hh.dtype
    dh_rec = torch.zeros(B, H, dtype=dt) if dhn is None else dhn.to(dt)
    dc = torch.zeros(B, H, dtype=dt) if dcn is None else dcn.to(dt)
    dG = [None] * U
    for u in reversed(range(U)):
        i, f, g, o = acts[u]
        dh = dh_rec + (dY[:, u].to(dt) if dY is not None else 0)
        tc = torch.tanh(cs[u + 1])
        dc = dc + dh * o * (1 - tc * tc)
        d = torch.cat([dc * g * i * (1 - i), dc * cs[u] * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        if round_g is not None:
            d = round_g(d)
        dG[u] = d
        dc = dc * f
        dh_rec = d @ w_hh
    dG = torch.stack(dG, 1)
    Hprev = torch.stack(hs[:-1], 1)
    dW_hh = dG.reshape(B * U, 4 * H).t() @ Hprev.reshape(B * U, H)
    return dG, dh_rec, dc, dW_hh, dG.sum((0, 1))


def wgrad_onehot(tokens, keep, dG, V, blank):
    """dW_ih (4H, V - 1)[:, col(token[b, u])] += keep[b, u] dG[b, u]: the scatter form."""
    col = col_of(tokens, blank).reshape(-1)
    g = dG.reshape(col.numel(), -1)
    if keep is not None:
        g = g * keep.to(g.dtype).reshape(-1, 1)
    out = torch.zeros(V - 1, g.shape[1], dtype=g.dtype)
    hot = col >= 0
    out.index_add_(0, col[hot], g[hot])
    return out.t().contiguous()


def run(params, h0=None, c0=None, x=None, tokens=None, keep=None, V=None, blank=None, dY=None, dhn=None, dcn=None,
        dtype=torch.float64, round_h=None, round_g=None, hmask=None, w_proj=None, dOut=None):
    """The whole prediction network in `dtype`: dense input `x` or one-hot `tokens` (+ keep), the recurrence, and - with w_proj (J, H) -
    out = (Y * hmask) w_proj^T with upstream gradient dOut (then dY is derived from it and added to a given dY).
    params = (w_ih, w_hh, b_ih, b_hh).  -> dict of outputs and gradients."""
    w_ih, w_hh, b_ih, b_hh = (p.to(dtype) for p in params)
    c = lambda t: None if t is None else t.to(dtype)
    x, h0, c0, dY, dhn, dcn, hmask, w_proj, dOut = (c(t) for t in (x, h0, c0, dY, dhn, dcn, hmask, w_proj, dOut))
    gx = gates_dense(x, w_ih, b_ih, b_hh) if x is not None else gates_onehot(tokens, keep, w_ih, b_ih, b_hh, blank)
    Y, hn, cn, saved = recurrence(gx, w_hh, h0, c0, round_h)
    r = {"y": Y, "hn": hn, "cn": cn}
    if w_proj is not None:
        Yd = Y * hmask if hmask is not None else Y
        r["out"] = Yd @ w_proj.t()
        if dOut is not None:
            r["dw_proj"] = dOut.reshape(-1, dOut.shape[-1]).t() @ Yd.reshape(-1, Yd.shape[-1])
            dYp = dOut @ w_proj
            if hmask is not None:
                dYp = dYp * hmask
            dY = dYp if dY is None else dY + dYp
    if dY is None and dhn is None and dcn is None:
        return r
    dG, dh0, dc0, dW_hh, db = bptt(saved, w_hh, dY, dhn, dcn, round_g)
    r.update(dh0=dh0, dc0=dc0, dw_hh=dW_hh, db_ih=db, db_hh=db, dG=dG)
    B, U = dG.shape[:2]
    if x is not None:
        r["dw_ih"] = dG.reshape(B * U, -1).t() @ x.reshape(B * U, -1)
        r["dx"] = dG @ w_ih
    else:
        r["dw_ih"] = wgrad_onehot(tokens, keep, dG, V, blank)
    return r


def floor_and_ref(operand_dtype, **kw):
    """(fp64 reference, floor emulation) of one case: the emulation is `run` in float32, for bf16 operands with h and the gate
    gradients rounded to bf16 where the kernels store them."""
    ref = run(dtype=torch.float64, **kw)
    rnd = bf16_round if operand_dtype == torch.bfloat16 else None
    emu = run(dtype=torch.float32, round_h=rnd, round_g=rnd, **kw)
    return ref, emu

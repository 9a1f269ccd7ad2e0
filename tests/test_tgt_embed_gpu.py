"""smx_tgt_embed_fwd / smx_tgt_embed_bwd (csrc/tgt_embed.hip) through ops, against the float64 restatement of tests/_decoder_ref.py,
float32 and bfloat16 output / gradient, inside poisoned guard bands.

Error bar (tests/test_attention_gpu.py's): the ATen chain - F.embedding * sqrt(d) + pe, cast to the dtype, and its autograd
gradient - runs on the same GPU and inputs; ours <= 4 x ATen's error against float64, floor 8 eps(dtype) where ATen is exact.
The flags, the untouched rows and the guard bands are checked exactly."""
import math

import pytest
import torch

from tests import _decoder_ref as DR

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 3          # guard rows on either side of every buffer


def _tokens(B, U, V, pad_idx, seed):
    """Random tokens over at most 6 distinct values (many repeats), row b padded from position U - b on (never position 0)."""
    g = torch.Generator().manual_seed(seed)
    pool = torch.randperm(V, generator=g)[:6]
    tok = pool[torch.randint(0, len(pool), (B, U), generator=g)]
    tok[tok == pad_idx] = (pad_idx + 1) % V
    for b in range(B):
        if U - b >= 1 and b > 0:
            tok[b, max(1, U - b):] = pad_idx
    return tok


def _banded(rows, cols, dtype, poison):
    """A (rows, cols) view in the middle of a poisoned buffer -> (view, whole buffer)."""
    buf = torch.full((rows + 2 * GUARD, cols), poison, dtype=dtype, device="cuda")
    return buf[GUARD:GUARD + rows], buf


def _bands_intact(buf, rows, poison):
    lo, hi = buf[:GUARD], buf[GUARD + rows:]
    if isinstance(poison, float) and math.isnan(poison):
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == poison).all() and (hi == poison).all())


def _fwd(tok, table, pe, pad_idx, dtype):
    from summarymixing_amd import ops
    B, U = tok.shape
    y, ybuf = _banded(B * U, table.shape[1], dtype, float("nan"))
    f, fbuf = _banded(B * U, 1, torch.uint8, 0xAB)
    out, flags = ops.tgt_embed_fwd(tok, table, pe, pad_idx, dtype, out=y, key_pad=f.view(-1))
    return out, flags, (ybuf, fbuf)


def _case(B, U, V, d, pad_idx, seed):
    g = torch.Generator().manual_seed(100 + seed)
    tok = _tokens(B, U, V, pad_idx, seed)
    table = torch.randn(V, d, generator=g)
    pe = torch.randn(U + 2, d, generator=g)          # (a longer table: rows [0, U) are read)
    dy = torch.randn(B * U, d, generator=g)
    g0 = torch.randn(V, d, generator=g)
    return tok, table, pe, dy, g0


# (B, U, V, d, pad_idx)
_SHAPES = [(3, 17, 11, 64, 0), (3, 17, 11, 64, 4), (2, 5, 1000, 512, 0), (2, 5, 1000, 512, 7), (1, 1, 2, 64, 0), (1, 1, 2, 64, 1)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", _SHAPES, ids=["-".join(map(str, s)) for s in _SHAPES])
def test_forward_and_backward_match_float64_within_aten_bar(shape, dt):
    from summarymixing_amd import ops
    B, U, V, d, pad_idx = shape
    dtype = DT[dt]
    tok, table, pe, dy, g0 = _case(B, U, V, d, pad_idx, B * U + V)
    tk, tb, pc = tok.cuda(), table.cuda(), pe.cuda()
    y, flags, (ybuf, fbuf) = _fwd(tk, tb, pc, pad_idx, dtype)
    assert flags.dtype == torch.bool and torch.equal(flags.cpu(), tok == pad_idx)
    assert _bands_intact(ybuf, B * U, float("nan")) and _bands_intact(fbuf, B * U, 0xAB)
    # backward onto a non-zero gradient, in a poisoned buffer; dy in the compute dtype
    dyc = dy.cuda().to(dtype)
    gt, gbuf = _banded(V, d, torch.float32, float("nan"))
    gt.copy_(g0)
    ops.tgt_embed_bwd(tk, dyc, gt, pad_idx)
    assert _bands_intact(gbuf, V, float("nan"))
    assert torch.equal(gt[pad_idx].cpu(), g0[pad_idx]), "the pad_idx row must be exactly unchanged"
    unused = torch.ones(V, dtype=torch.bool)
    unused[tok.reshape(-1)] = False
    assert torch.equal(gt.cpu()[unused], g0[unused]), "rows no token names must be exactly unchanged"
    # float64 (on the dtype-rounded gradient) and the ATen chain at the dtype
    t6 = table.double().requires_grad_(True)
    y6 = DR.embed(tok, t6, pe.double())
    (y6 * dyc.cpu().double().view(B, U, d)).sum().backward()
    g6 = t6.grad.clone()
    g6[pad_idx] = 0.0                                    # nn.Embedding(padding_idx): the row receives nothing
    ta = tb.clone().requires_grad_(True)
    ya = DR.embed(tk, ta, pc).to(dtype)
    ya.backward(dyc.view(B, U, d))
    ga = ta.grad.clone()
    ga[pad_idx] = 0.0
    g0c = g0.cuda()
    DR.judge(f"tgt_embed {dt} {shape}", dtype, {"y": y, "gtable": gt}, {"y": ya.detach(), "gtable": g0c + ga},
             {"y": y6.detach(), "gtable": g0.double() + g6})


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_out_of_range_tokens_read_as_zero_rows(dt):
    """Tokens -1 and V: y = the positional rows, flag 0, no gradient, nothing outside the buffers is touched."""
    from summarymixing_amd import ops
    B, U, V, d, pad_idx = 2, 5, 11, 64, 0
    dtype = DT[dt]
    tok, table, pe, dy, g0 = _case(B, U, V, d, pad_idx, 77)
    tok[0, 1], tok[0, 3], tok[1, 0], tok[1, 4] = -1, V, V, -1
    tk, tb, pc = tok.cuda(), table.cuda(), pe.cuda()
    y, flags, (ybuf, fbuf) = _fwd(tk, tb, pc, pad_idx, dtype)
    assert _bands_intact(ybuf, B * U, float("nan")) and _bands_intact(fbuf, B * U, 0xAB)
    assert torch.equal(flags.cpu(), tok == pad_idx) and not flags[0, 1] and not flags[1, 0]
    for b, u in ((0, 1), (0, 3), (1, 0), (1, 4)):
        assert torch.equal(y[b, u], pc[u].to(dtype)), (b, u)
    y6 = DR.embed(tok, table.double(), pe.double())
    ya = DR.embed(tk, tb, pc).to(dtype)
    dyc = dy.cuda().to(dtype)
    gt, gbuf = _banded(V, d, torch.float32, float("nan"))
    gt.copy_(g0)
    ops.tgt_embed_bwd(tk, dyc, gt, pad_idx)
    assert _bands_intact(gbuf, V, float("nan"))
    # the same tokens with the out-of-range ones replaced by the padding token: the gradient must be identical, bit for bit
    tok2 = tok.clone()
    tok2[(tok < 0) | (tok >= V)] = pad_idx
    gt2 = g0.cuda().clone()
    ops.tgt_embed_bwd(tok2.cuda(), dyc, gt2, pad_idx)
    assert torch.equal(gt, gt2)
    DR.judge(f"tgt_embed out-of-range {dt}", dtype, {"y": y}, {"y": ya}, {"y": y6})


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_runs_agree_bit_for_bit_and_replay_from_a_graph(dt):
    from summarymixing_amd import ops
    B, U, V, d, pad_idx = 3, 17, 11, 64, 4
    dtype = DT[dt]
    tok, table, pe, dy, g0 = _case(B, U, V, d, pad_idx, 5)
    tk, tb, pc, dyc = tok.cuda().to(torch.int32), table.cuda(), pe.cuda(), dy.cuda().to(dtype)

    def step(gt):
        y, flags = ops.tgt_embed_fwd(tk, tb, pc, pad_idx, dtype)
        ops.tgt_embed_bwd(tk, dyc, gt, pad_idx)
        return y, flags
    ga, gb, gc = (g0.cuda().clone() for _ in range(3))
    ya, fa = step(ga)
    yb, fb = step(gb)
    assert torch.equal(ya, yb) and torch.equal(fa, fb) and torch.equal(ga, gb)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(g0.cuda().clone())                          # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yc, fc = step(gc)
    gc.copy_(g0)
    yc.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yc, ya) and torch.equal(fc, fa) and torch.equal(gc, ga)

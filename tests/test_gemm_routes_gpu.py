"""Every GEMM route of tests/_gemm_cases.py, per element against float64, inside poisoned buffers (DESIGN.md "GEMM routes").

For every case: (1) ops.gemm_symbol on the real tensors names the instantiation the table expects; (2) every operand is a view inside a
larger buffer - read operands between NaNs (rows before and after the view, the ld - width padding, the gaps between batches; uint8 masks
between 1s, with the view's own last rows 0), written operands inside a finite sentinel bit pattern with at least tile_n guard rows and 8
elements of row padding; (3) one call; (4) the guard region still holds the sentinel BITWISE, no output holds a NaN, and every element
meets the derived bar of tests/_gemm_ref.py; (5) a second call reproduces every output bit for bit (the atomic split-K cases only meet
the bar again).  A NaN in an output means the kernel read outside the operand it was given.  Nothing here provokes a fault: every byte
the kernels may touch lies inside a live allocation.

The knob cases (SMX_T256=2 / 3, SMX_LN_TILE64=0: read once per process) run the same runner in one child process per knob value."""
import json
import os
import subprocess
import sys
import zlib

import pytest
import torch

from tests import _gemm_cases as G
from tests import _gemm_ref as R
from tests._util import report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SENT16, _SENT32 = 0x4B4C, 0x4B4C4D4E                     # finite in bf16 (1.3e7) and float32 (1.3e7); never a value a case computes


def _tdtype(case, op):
    return {"T": torch.bfloat16 if case.dtype == "bf16" else torch.float32, "f32": torch.float32, "u8": torch.uint8}[op.dtype]


def _bits(buf):
    return buf.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[buf.element_size()])


def symbol_of(case):
    if case.plan[0] == 1:
        return "gemm_tn_dma_kernel"
    tb = lambda v: "true" if v else "false"
    k, a, b, tn, tm, vec, lnf, ga = case.plan
    return f"gemm_kernel<{'bf16_t' if case.dtype == 'bf16' else 'float'}, {tb(a)}, {tb(b)}, {tn}, {tm}, {tb(vec)}, {lnf}, {ga}>"


def _values(case, op, shape, dev):
    """Deliberately structured inputs: a column ramp on A and B (a transposed fragment or a shifted column changes the value), distinct
    values per column in bias / C0 / gamma / beta, distinct rows in C0."""
    nb, rows, width = shape
    ramp = torch.linspace(-1, 1, width, device=dev)
    rn = lambda s=1.0: torch.randn(shape, device=dev) * s
    n = op.name
    if n == "A":
        return rn() + 0.5 * ramp
    if n == "B":
        return (rn() + ramp) * (case.K ** -0.5)
    if n in ("bias", "lnf_beta", "lnf2_beta"):
        return 0.7 * ramp + rn(0.1)
    if n == "c0":
        return rn(0.5) + 0.5 * ramp.flip(0) + 0.01 * torch.arange(rows, device=dev).reshape(1, rows, 1)
    if n in ("ln_gamma", "lnf_gamma", "lnf2_gamma"):
        return 1.0 + 0.5 * ramp + rn(0.1)
    if n == "z":
        return rn(1.5)
    if n == "ln_x":
        return rn(2.0) + 0.3
    if n in ("row_mask", "ln_mask2"):
        m = (torch.rand(shape, device=dev) > 0.3).to(torch.uint8)
        m[..., -3:] = 0                                     # the poison beside a mask is 1: a read one row off the end shows
        return m
    if n == "colsum":
        return torch.full(shape, 0.25, device=dev) + 0.1 * ramp
    return rn()                                            # res, the initial C of the accumulating (atomic) output


class Buffers:
    def __init__(self, case, dev):
        self.case, self.buf, self.view, self.inside, self.ops = case, {}, {}, {}, {}
        for op in G.operands(case):
            g = G.geometry(case, op)
            dt = _tdtype(case, op)
            total = g.nbatch * g.bstride + 16
            buf = torch.empty(total, dtype=dt, device=dev)
            if op.role == "w":
                _bits(buf).fill_(_SENT16 if buf.element_size() == 2 else _SENT32)
            elif dt == torch.uint8:
                buf.fill_(1)
            else:
                buf.fill_(float("nan"))
            shape, strides, off = (g.nbatch, op.rows, op.width), (g.bstride, g.ld, 1), g.guard * g.ld + g.coff
            inside = torch.zeros(total, dtype=torch.bool, device=dev)
            inside.as_strided(shape, strides, off).fill_(True)
            self.buf[op.name], self.view[op.name], self.inside[op.name], self.ops[op.name] = buf, buf.as_strided(shape, strides, off), inside, op

        if "colsum" in self.ops:                           # (ops.gemm attaches its own; the plan query wants one too)
            from summarymixing_amd import _lib as L
            self.workspace = torch.empty(L.lib().smx_gemm_colsum_workspace(case.N, case.M) // 4, device=dev)

    def ptr(self, name):
        return self.workspace.data_ptr() if name == "workspace" else self.view[name].data_ptr()


def _fill(case, bufs, dev):
    """Fill every read operand (and the accumulating outputs) -> float64 values by name."""
    f = G.fam(case)
    t = {}
    for name, op in bufs.ops.items():
        accum = name == "colsum" or (name == "C" and f["out"] == "ATOMIC")
        if op.role == "w" and not accum:
            continue
        if name == "ln_stats":
            continue
        v = bufs.view[name]
        v.copy_(_values(case, op, tuple(v.shape), dev).to(v.dtype))
        t[name] = v.double()
    for name in t:
        if name in ("A", "B", "C", "res", "z"):
            continue
        t[name] = t[name][0]                               # unbatched operands: (rows, width)
        if bufs.ops[name].dense and bufs.ops[name].rows == 1:
            t[name] = t[name][0]
    if "bias" in t and not f["bias_batch"]:
        t["bias"] = t["bias"][0]
    if "ln_x" in t:                                        # the statistics the forward would have saved, as float32
        x = t["ln_x"]
        mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
        bufs.view["ln_stats"].copy_(torch.cat([mean, (var + 1e-5).rsqrt()], 1).float()[None])
        t["ln_stats"] = bufs.view["ln_stats"][0].double()
    return t


def _call(case, bufs, check_symbol):
    from summarymixing_amd import ops
    epi = G.make_epilogue(case, bufs.ptr)
    lay, _, _, lda, sa, _, ldb, sb, _, ldc, sc, N, M, K, batch, splits = G.gemm_args(case, bufs.ptr)
    a, b, c = bufs.view["A"][0], bufs.view["B"][0], bufs.view["C"][0]
    kw = dict(batch=batch, sa=sa, sb=sb, sc=sc, splits=splits, lda=lda, ldb=ldb, ldc=ldc)
    if check_symbol:
        sym = ops.gemm_symbol(lay, a, b, c, N, M, K, epi, **kw)
        assert sym == symbol_of(case), f"{case.name}: the table names {symbol_of(case)}, the dispatch takes {sym}"
    ops.gemm(lay, a, b, c, N, M, K, epi, **kw)


def run_case(case, dev="cuda"):
    """-> the report entry of the case; raises AssertionError naming the case, the plan and the worst element."""
    from summarymixing_amd import ops
    torch.manual_seed(zlib.crc32(case.name.encode()))
    f = G.fam(case)
    bufs = Buffers(case, dev)
    t = _fill(case, bufs, dev)
    written = [n for n, op in bufs.ops.items() if op.role == "w"]
    before = {n: _bits(bufs.buf[n]).clone() for n in written}
    keep = keep2 = None
    if f["drop"]:
        keep = ops.dropout(torch.ones(case.N, G.drop_cols(case) or case.M, device=dev), f["drop"][0], f["drop"][1]) != 0
    if f["ln"] and f["ln"].get("drop2"):
        keep2 = ops.dropout(torch.ones(case.N, case.M, device=dev), *f["ln"]["drop2"]) != 0
    outs, info = R.reference(case, t, keep, keep2)
    assert set(outs) == set(written), (case.name, sorted(outs), sorted(written))
    _call(case, bufs, True)
    torch.cuda.synchronize()
    worst_ratio, worst_msg = 0.0, ""
    first = {}
    for n in written:
        after = _bits(bufs.buf[n])
        out = ~bufs.inside[n]
        bad = (after != before[n]) & out
        assert not bool(bad.any()), (f"{case.name} plan={case.plan}: {n} was written OUTSIDE its view at buffer elements "
                                     f"{bad.nonzero()[:8, 0].tolist()} (view starts at {G.view_offset(case, bufs.ops[n])}, ld {G.geometry(case, bufs.ops[n]).ld})")
        first[n] = after.clone()
        got = bufs.view[n]
        assert not bool(torch.isnan(got.float()).any()), f"{case.name} plan={case.plan}: NaN in {n}: the kernel read outside an operand it was given"
        ref, bar, zero = outs[n]
        g = got
        if n == "ln_partial":
            g = got.double().reshape(-1, 2, case.M).sum(0)
        elif n not in ("C", "z"):
            g = got[0] if bufs.ops[n].rows > 1 else got[0, 0]
        if zero is not None:
            nz = zero & (g != 0)
            assert not bool(nz.any()), f"{case.name} plan={case.plan}: {n} holds a non-zero value at the dropped position {nz.nonzero()[0].tolist()}"
        w, msg = R.worst(case, n, g, ref, bar)
        if w >= worst_ratio:
            worst_ratio, worst_msg = w, msg
        assert w <= 1.0, msg
    # the second call: bit-identical outputs (atomic accumulation: the bar again)
    for n in written:
        _bits(bufs.buf[n]).copy_(before[n])
    _call(case, bufs, False)
    torch.cuda.synchronize()
    for n in written:
        if f["out"] == "ATOMIC":
            ref, bar, _ = outs[n]
            w, msg = R.worst(case, n, bufs.view[n], ref, bar)
            assert w <= 1.0, "second call: " + msg
        else:
            assert torch.equal(_bits(bufs.buf[n]), first[n]), f"{case.name} plan={case.plan}: {n} differs between two identical calls"
    entry = {"case": case.name, "err_over_bar": round(worst_ratio, 4), "t_act": info["t_act"], "worst": worst_msg.split(": worst element", 1)[-1][:160]}
    report("gemm_routes", entry)
    return entry


def run_group(key):
    for case in G.env_groups()[key]:
        run_case(case)


def _child_main():
    from summarymixing_amd import _lib as L
    key = tuple(tuple(kv) for kv in json.loads(os.environ["SMX_ROUTE_GROUP"]))
    cfg = L.get_config()
    for k, v in key:
        assert cfg[{"SMX_T256": "t256", "SMX_LN_TILE64": "ln_tile64"}[k]] == int(v), (k, v, cfg)
    run_group(key)
    print("OK")


_DEFAULT = G.env_groups()[()]
_KNOBS = [k for k in G.env_groups() if k]


@pytest.mark.parametrize("case", _DEFAULT, ids=[c.name for c in _DEFAULT])
def test_route_per_element_in_poisoned_buffers(case):
    run_case(case)


@pytest.mark.parametrize("key", _KNOBS, ids=[",".join(f"{a}={b}" for a, b in k) for k in _KNOBS])
def test_knob_routes_per_element_in_poisoned_buffers(key):
    env = dict(os.environ, SMX_ROUTE_GROUP=json.dumps(key), **dict(key))
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gemm_routes_gpu import _child_main; _child_main()" % ROOT],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "OK" in p.stdout, p.stderr[-3000:]


# ---- smx_linear_wgrad ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [40, 38], ids=["slab", "ragged_atomic"])
@pytest.mark.parametrize("rows", [40, 511, 512, 513, 1025, 2049])
def test_linear_wgrad_in_poisoned_buffers(rows, K, dtype):
    """smx_linear_wgrad has no plan query, so NO route is asserted here: the slab path (K % 4 == 0, with the bias gradient) and the ragged
    atomic path (K % 4 != 0), batch = 3, strided views, frame counts that straddle a 512-frame split and a 64-row stage.  The frames are
    the strided reduce dimension, so the NaN rows behind the operands show a missing tail guard; the gradient accumulates into values
    and sits inside sentinel guards.  Bar: 2 (2^-24 (rows + splits + 8) S + 2^-24 |ref|), S = |alpha| sum |dz| |x| + |initial value|,
    splits <= ceil(rows / 512) (wgrad_splits never makes a split shorter than 512 frames)."""
    from summarymixing_amd import ops
    dev, M, batch, alpha, g = "cuda", 72, 3, 0.5, 4
    torch.manual_seed(rows * 100 + K)
    slab = K % 4 == 0

    def operand(width):
        ld = batch * width + 8
        buf = torch.full(((rows + 2 * g) * ld,), float("nan"), device=dev, dtype=dtype)
        v = buf.as_strided((rows, batch, width), (ld, width, 1), g * ld)
        v.copy_((torch.randn(rows, batch, width, device=dev) + torch.linspace(-1, 1, width, device=dev)).to(dtype))
        return buf, v, ld
    zb, dz, lddz = operand(M)
    xb, x, ldx = operand(K)
    ldw = K + 8
    sw = (M + 2 * g) * ldw
    wbuf = torch.empty(batch * sw + 16, device=dev)
    _bits(wbuf).fill_(_SENT32)
    gw = wbuf.as_strided((batch, M, K), (sw, ldw, 1), g * ldw)
    gw.copy_(torch.randn(batch, M, K, device=dev))
    inside = torch.zeros_like(wbuf, dtype=torch.bool)
    inside.as_strided((batch, M, K), (sw, ldw, 1), g * ldw).fill_(True)
    bbuf = torch.empty(batch * M + 2 * 64, device=dev)
    _bits(bbuf).fill_(_SENT32)
    gb = bbuf[64:64 + batch * M].view(batch, M)
    gb.copy_(torch.randn(batch, M, device=dev))
    w0, b0 = gw.double().clone(), gb.double().clone()
    wbits, bbits = _bits(wbuf).clone(), _bits(bbuf).clone()
    ops.wgrad(dz[:, 0], x[:, 0], gw[0], rows, M, K, batch=batch, sz=M, sx=K, sw=sw, lddz=lddz, ldx=ldx, lddw=ldw, alpha=alpha,
              dbias=gb if slab else None)
    torch.cuda.synchronize()
    assert torch.equal(_bits(wbuf)[~inside], wbits[~inside]), "dW was written outside its view"
    assert torch.equal(_bits(bbuf)[:64], bbits[:64]) and torch.equal(_bits(bbuf)[64 + batch * M:], bbits[64 + batch * M:]), "dbias was written outside its view"
    assert not bool(torch.isnan(gw).any()) and not bool(torch.isnan(gb).any()), "NaN: the kernel read frames outside its operands"
    dzd, xd = dz.double(), x.double()
    u, splits = 2.0 ** -24, (rows + 511) // 512
    ref = w0 + alpha * torch.einsum("rbm,rbk->bmk", dzd, xd)
    S = w0.abs() + alpha * torch.einsum("rbm,rbk->bmk", dzd.abs(), xd.abs())
    bar = 2 * (u * (rows + splits + 8) * S + u * ref.abs())
    ratio = ((gw.double() - ref).abs() / bar).max().item()
    entry = {"case": f"wgrad-{'bf16' if dtype == torch.bfloat16 else 'f32'}-rows{rows}-K{K}", "err_over_bar": round(ratio, 4), "t_act": 0.0}
    i = int(((gw.double() - ref).abs() / bar).argmax())
    assert ratio <= 1.0, f"dW: err / bar {ratio:.3f} at (batch, m, k) = ({i // (M * K)}, {i // K % M}, {i % K})"
    if slab:
        refb = b0 + alpha * dzd.sum(0)
        barb = 2 * (u * (rows + splits + 8) * (b0.abs() + alpha * dzd.abs().sum(0)) + u * refb.abs())
        rb = ((gb.double() - refb).abs() / barb).max().item()
        entry["err_over_bar_dbias"] = round(rb, 4)
        assert rb <= 1.0, f"dbias: err / bar {rb:.3f}"
    else:
        assert torch.equal(_bits(bbuf), bbits)
    report("gemm_routes", entry)

"""The bits of the depthwise conv on each route of its dispatcher (tiled, window, rolling, rolling CSGU), pinned: the SHA-256 of the raw
bytes of y, dP, dgate, dw and dbias of ops.dwconv_fwd / ops.dwconv_bwd must equal tests/golden/dwconv_route_bits.json; with a
caller-owned workspace (deferred reduction) also the row count and the bytes of the partial rows [rows][D][k+1] left in it.  The
fixture was written by this module (`python tests/test_dwconv_route_bits_gpu.py --write <path>`) at the commit before the dispatcher
became one plan (smx_dwconv_plan_query), where the third value of ops.dwconv_bwd was a flag and the row count a separate query; the
host-side rewrite must launch the same kernels with the same grids and arguments, so the bits do not move.  The shapes are the
smallest of tests/test_kernels_gpu.py and tests/test_dropout_gpu.py on each (route, form).  Inputs are integer patterns (exact in
bf16), no random generator."""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dwconv_route_bits.json")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
TILED, WINDOW, ROLL, CSGU = 0, 1, 2, 3
GLU, GATED = "glu", "gated"                               # GLU + zero padding (Conformer) | gate + reflect padding (Branchformer CSGU)


def _cases():
    """name -> (form, dtype name, B, T, D, k, chunk, drop, route)"""
    c = {}
    for dn in DTYPES:
        for B, T, D, k, chunk, route in ((1, 9, 8, 5, 4, TILED), (3, 70, 40, 7, 0, TILED), (2, 150, 96, 31, 0, WINDOW), (1, 9, 64, 31, 0, ROLL),
                                         (2, 70, 64, 31, 1, ROLL), (1, 40, 64, 31, 100, ROLL), (2, 100, 64, 31, 7, ROLL)):
            c[f"glu-{dn}-{B}x{T}x{D}-k{k}-chunk{chunk}"] = (GLU, dn, B, T, D, k, chunk, None, route)
        for B, T, D, k, route in ((2, 90, 48, 7, TILED), (1, 40, 16, 31, WINDOW)):
            c[f"gated-{dn}-{B}x{T}x{D}-k{k}"] = (GATED, dn, B, T, D, k, 0, None, route)
    for B, T, D in ((3, 16, 64), (2, 31, 64), (2, 47, 192)):
        c[f"gated-bf16-{B}x{T}x{D}-k31"] = (GATED, "bf16", B, T, D, 31, 0, None, CSGU)
    c["gated-bf16-2x31x64-k31-drop"] = (GATED, "bf16", 2, 31, 64, 31, 0, (0.15, 99), CSGU)      # forward only
    return c


CASES = _cases()


def _pattern(rows, cols, mul, mod, div, dtype):
    """x[i, j] = ((mul[0] i + mul[1] j) % mod - mod // 2) / div, exact in bf16 for the values used."""
    i = torch.arange(rows, dtype=torch.int64).view(-1, 1)
    j = torch.arange(cols, dtype=torch.int64).view(1, -1)
    return (((mul[0] * i + mul[1] * j) % mod - mod // 2).double() / div).to(dtype).cuda()


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _inputs(name):
    form, dn, B, T, D, k, chunk, drop, _ = CASES[name]
    dtype = DTYPES[dn]
    p = _pattern(B * T, 2 * D if form == GLU else D, (37, 11), 61, 16, dtype)
    gate = _pattern(B * T, D, (17, 5), 47, 16, dtype) if form == GATED else None
    w = _pattern(D, k, (13, 7), 41, 32, torch.float32)
    bias = _pattern(1, D, (0, 5), 17, 8, torch.float32).view(D)
    dy = _pattern(B * T, D, (29, 3), 53, 16, dtype)
    return p, gate, w, bias, dy


def _run(name):
    from summarymixing_amd import _lib as L, ops
    form, dn, B, T, D, k, chunk, drop, _ = CASES[name]
    glu, pad = (True, L.PAD_ZERO) if form == GLU else (False, L.PAD_REFLECT)
    p, gate, w, bias, dy = _inputs(name)
    y = ops.dwconv_fwd(p, w, bias, B, T, D, k, glu, pad, chunk, gate, drop=drop)
    assert torch.isfinite(y).all()
    out = {"y": _digest(y)}
    if drop is not None:
        return out
    named = lambda dp, dg, dw, db: {"dp": _digest(dp), "dgate": _digest(dg) if dg is not None else None, "dw": _digest(dw), "dbias": _digest(db)}
    dw, db = torch.zeros(D, k, device="cuda"), torch.zeros(D, device="cuda")
    dp, dg = ops.dwconv_bwd(dy, p, w, bias, dw, db, B, T, D, k, glu, pad, chunk, gate)
    assert all(torch.isfinite(t).all() for t in (dp, dw, db)) and (dg is None or torch.isfinite(dg).all())
    out.update(named(dp, dg, dw, db))
    # the same call with a caller-owned workspace: the partial rows stay there where the route can defer its reduction
    ws = torch.full((L.lib().smx_dwconv1d_glu_bwd_workspace(B, T, D, k) // 4,), float("nan"), device="cuda")
    dw, db = torch.zeros(D, k, device="cuda"), torch.zeros(D, device="cuda")
    dp, dg, rows = ops.dwconv_bwd(dy, p, w, bias, dw, db, B, T, D, k, glu, pad, chunk, gate, ws=ws.view(torch.uint8))
    if isinstance(rows, bool):                            # (the commit that wrote the fixture: a flag, and the row count its own query)
        rows = L.lib().smx_dwconv1d_glu_bwd_partial_rows(L.BF16 if dn == "bf16" else L.F32, B, T, D, k, int(glu), pad, chunk, int(gate is not None)) if rows else 0
    left = ws[:rows * D * (k + 1)]
    assert torch.isfinite(left).all(), f"{name}: the {rows} partial rows must all be written"
    out["deferred"] = dict(named(dp, dg, dw, db), rows=rows, ws=_digest(left))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_bits_equal_the_fixture(name, golden):
    got, want = _run(name), golden[name]
    assert sorted(got) == sorted(want)
    for key in sorted(got):
        assert got[key] == want[key], f"{name}: {key} differs from the fixture"


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_names_the_expected_route(name, golden):
    """The descriptor of the same tensors, asked of the library in both directions: the route this case is here for, and the row
    count the deferred call reported."""
    from summarymixing_amd import _lib as L
    form, dn, B, T, D, k, chunk, drop, route = CASES[name]
    p, gate, w, bias, dy = _inputs(name)
    y, dp, dw, db, ws = torch.empty_like(dy), torch.empty_like(p), torch.zeros(D, k, device="cuda"), torch.zeros(D, device="cuda"), torch.empty(64, device="cuda")
    a = L.DwconvArgs(dtype=L.BF16 if dn == "bf16" else L.F32, glu=int(form == GLU), P=p.data_ptr(), ldp=p.stride(0), w=w.data_ptr(),
                     bias=bias.data_ptr(), Y=y.data_ptr(), ldy=D, B=B, T=T, D=D, k=k, pad_mode=L.PAD_ZERO if form == GLU else L.PAD_REFLECT,
                     chunk=chunk, drop_p=drop[0] if drop else 0.0)
    if gate is not None:
        dgate = torch.empty_like(gate)
        a.gate, a.ldg, a.dgate, a.lddg = gate.data_ptr(), D, dgate.data_ptr(), D
    plan = L.DwconvPlan()
    L.check(L.lib().smx_dwconv_plan_query(ctypes.byref(a), 0, ctypes.byref(plan)), "smx_dwconv_plan_query")
    assert (plan.route, plan.chunked, plan.deferrable) == (route, int(chunk > 0), 0)
    if drop is None:
        a.Y, a.dP, a.lddp, a.dw, a.dbias, a.workspace = dy.data_ptr(), dp.data_ptr(), dp.stride(0), dw.data_ptr(), db.data_ptr(), ws.data_ptr()
        L.check(L.lib().smx_dwconv_plan_query(ctypes.byref(a), 1, ctypes.byref(plan)), "smx_dwconv_plan_query")
        assert (plan.route, plan.chunked, plan.deferrable) == (route, int(chunk > 0), int(route != TILED))
        assert golden[name]["deferred"]["rows"] == (plan.partial_rows if plan.deferrable else 0)


def test_fixture_has_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_dwconv_route_bits_gpu.py --write <path>")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[2], "w") as f:
        json.dump({name: _run(name) for name in sorted(CASES)}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(CASES)} cases to {sys.argv[2]}")

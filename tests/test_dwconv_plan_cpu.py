"""The depthwise conv's route decision (smx_dwconv_plan_query, DESIGN.md "Depthwise conv routes"), checked without a GPU: the query
runs the checks and the decision of smx_dwconv_fwd / smx_dwconv_bwd and launches nothing.  Pointers are fabricated integers with a
chosen alignment, never dereferenced.

ROUTES is a literal table: descriptor -> (route, chunked, deferrable) or the refusal code, with a case on each side of every condition
of the decision, in both directions and both dtypes.  The row counts and the workspace bound are compared with
tests/golden/dwconv_plan_parent.json, which `python tests/test_dwconv_plan_cpu.py --write <libsmx.so> <path>` recorded from the library
of the commit before the plan existed (its smx_dwconv1d_glu_bwd_partial_rows and smx_dwconv1d_glu_bwd_workspace, which need no GPU)."""
import ctypes
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dwconv_plan_parent.json")
F32, BF16 = 0, 1
ZERO, REFLECT = 0, 1
TILED, WINDOW, ROLL, CSGU = 0, 1, 2, 3
EINVAL, EUNSUPPORTED = -1, -2
_BASE = 1 << 40                                           # 4 KiB aligned; operand i lives at _BASE + i * 2^32
_PTRS = ("P", "Y", "gate", "dP", "dgate", "w", "bias", "dw", "dbias", "workspace")
_AT = {n: _BASE + (i << 32) for i, n in enumerate(_PTRS)}
FWD, BWD = 0, 1


def _args(backward, dtype, B, T, D, k, glu, pad, chunk, has_gate, **kw):
    """A well-formed, fully aligned descriptor of one direction (dense rows: ldp = 2D with GLU), then the overrides."""
    from summarymixing_amd import _lib
    a = _lib.DwconvArgs(dtype=dtype, glu=glu, P=_AT["P"], ldp=(2 if glu else 1) * D, w=_AT["w"], bias=_AT["bias"], Y=_AT["Y"], ldy=D,
                        B=B, T=T, D=D, k=k, pad_mode=pad, chunk=chunk)
    if has_gate:
        a.gate, a.ldg = _AT["gate"], D
    if backward:
        a.dP, a.lddp, a.dw, a.dbias, a.workspace = _AT["dP"], a.ldp, _AT["dw"], _AT["dbias"], _AT["workspace"]
        if has_gate:
            a.dgate, a.lddg = _AT["dgate"], D
    for name, v in kw.items():
        setattr(a, name, v)
    return a


def _query(a, backward):
    from summarymixing_amd import _lib
    plan = _lib.DwconvPlan()
    return _lib.lib().smx_dwconv_plan_query(ctypes.byref(a), backward, ctypes.byref(plan)), plan


GLU = dict(B=2, T=70, D=64, k=31, glu=1, pad=ZERO, chunk=0, has_gate=0)            # the Conformer form: rolling at these sizes
GATED = dict(B=2, T=70, D=64, k=31, glu=0, pad=REFLECT, chunk=0, has_gate=1)       # the Branchformer CSGU form
SPAN = 7669592                                            # a row stride (% 8 == 0) with 70 frames * SPAN * 4 bytes >= 2^31
NODW = dict(dw=None, dbias=None)


def _table():
    """(id, direction, dtype, form, overrides, expected)"""
    t = []
    for d, dn in ((FWD, "fwd"), (BWD, "bwd")):
        df = int(d == BWD)                                # every route but the tiled one can defer its reduction
        for dt, tn, v in ((BF16, "bf16", 8), (F32, "f32", 4)):
            add = lambda name, form, kw, want: t.append((f"{dn}-{tn}-{name}", d, dt, form, kw, want))
            csgu = (CSGU if dt == BF16 else WINDOW, 0, df)            # the rolling CSGU kernels are bf16 only
            # -- which family
            add("glu", GLU, {}, (ROLL, 0, df))
            add("glu-chunk7", GLU, dict(chunk=7), (ROLL, 1, df))
            add("glu-D72", GLU, dict(D=72), (WINDOW, 0, df))                       # D % 64 != 0, D % 8 == 0
            add("glu-D68", GLU, dict(D=68), (WINDOW, 0, df) if v == 4 else (TILED, 0, 0))      # D % 4 == 0 only
            add("glu-D66", GLU, dict(D=66), (TILED, 0, 0))
            add("glu-D72-chunk7", GLU, dict(D=72, chunk=7), (TILED, 1, 0))         # the window kernels have no chunking
            add("glu-k29", GLU, dict(k=29), (TILED, 0, 0))
            add("glu-k33", GLU, dict(k=33), (TILED, 0, 0))
            add("glu-reflect", GLU, dict(pad=REFLECT), (WINDOW, 0, df))            # the rolling GLU kernels pad with zeros
            add("glu-gate", GLU, dict(has_gate=1), (WINDOW, 0, df))
            add("gated", GATED, {}, csgu)
            add("gated-T16", GATED, dict(T=16), csgu)
            add("gated-chunk4", GATED, dict(chunk=4), (TILED, 1, 0))
            add("gated-zero-pad", GATED, dict(pad=ZERO), (WINDOW, 0, df))
            add("gated-D72", GATED, dict(D=72), (WINDOW, 0, df))
            add("gated-k7", GATED, dict(k=7), (TILED, 0, 0))
            # -- reflect padding, T 15 against 16: the forward refuses (k - 1) / 2 >= T, the backward runs the tiled kernel
            add("gated-T15", GATED, dict(T=15), EINVAL if d == FWD else (TILED, 0, 0))
            add("glu-reflect-T15", GLU, dict(pad=REFLECT, T=15), EINVAL if d == FWD else (TILED, 0, 0))
            add("glu-T15", GLU, dict(T=15), (ROLL, 0, df))
            add("glu-D72-T15", GLU, dict(D=72, T=15), (WINDOW, 0, df))
            # -- alignment, each operand in turn: bf16 falls to the tiled kernel, fp32 keeps rolling (its window kernels need al(4))
            ops_ = [("P", 2 * 64), ("Y", 64)] + ([("dP", 2 * 64)] if d == BWD else [])
            for name, ld in ops_:
                ldn = {"P": "ldp", "Y": "ldy", "dP": "lddp"}[name]
                add(f"glu-{ldn}+4", GLU, {ldn: ld + 4}, (TILED, 0, 0) if dt == BF16 else (ROLL, 0, df))
                add(f"glu-{ldn}+1", GLU, {ldn: ld + 1}, (TILED, 0, 0) if dt == BF16 else (ROLL, 0, df))
                add(f"glu-{name}+8", GLU, {name: _AT[name] + 8}, (TILED, 0, 0) if dt == BF16 else (ROLL, 0, df))
                add(f"glu-D72-{ldn}+4", GLU, {"D": 72, ldn: (ld // 64) * 72 + 4}, (TILED, 0, 0) if dt == BF16 else (WINDOW, 0, df))
                add(f"glu-D72-{ldn}+2", GLU, {"D": 72, ldn: (ld // 64) * 72 + 2}, (TILED, 0, 0))
                add(f"glu-D72-{name}+8", GLU, {"D": 72, name: _AT[name] + 8}, (TILED, 0, 0))
            gops = [("gate", "ldg")] + ([("dgate", "lddg")] if d == BWD else [])
            for name, ldn in gops:
                add(f"gated-{ldn}+4", GATED, {ldn: 68}, (TILED, 0, 0) if dt == BF16 else (WINDOW, 0, df))
                add(f"gated-{name}+8", GATED, {name: _AT[name] + 8}, (TILED, 0, 0))
            # -- refusals every call is checked for
            add("no-P", GLU, dict(P=None), EINVAL)
            add("no-w", GLU, dict(w=None), EINVAL)
            add("no-Y", GLU, dict(Y=None), EINVAL)
            add("no-bias", GLU, dict(bias=None), (ROLL, 0, df))
            add("k30", GLU, dict(k=30), EINVAL)
            add("k35", GLU, dict(k=35), EINVAL)
            add("k0", GLU, dict(k=0), EINVAL)
            # -- the 2 GB span is a limit of the rolling kernels' 32-bit offsets only
            add("glu-span", GLU, dict(ldp=SPAN), EINVAL)
            add("glu-span-ldy", GLU, dict(ldy=SPAN), EINVAL)
            add("glu-span-below", GLU, dict(ldp=SPAN - 8), (ROLL, 0, df))
            add("glu-D72-span", GLU, dict(D=72, ldp=SPAN), (WINDOW, 0, df))
            add("gated-span-ldg", GATED, dict(ldg=SPAN), EINVAL if dt == BF16 else (WINDOW, 0, df))
            if d == FWD:
                add("glu-span-unused-ldg", GLU, dict(ldg=SPAN), EINVAL)           # (ldg counts even without a gate)
                add("glu-span-unused-lddp", GLU, dict(lddp=SPAN), (ROLL, 0, 0))   # (the forward has no dP)
                # -- fused output dropout: the rolling CSGU forward only
                add("gated-drop", GATED, dict(drop_p=0.15), csgu if dt == BF16 else EUNSUPPORTED)
                add("glu-drop", GLU, dict(drop_p=0.15), EUNSUPPORTED)
                add("glu-D72-drop", GLU, dict(D=72, drop_p=0.15), EUNSUPPORTED)
                add("glu-k29-drop", GLU, dict(k=29, drop_p=0.15), EUNSUPPORTED)
                add("gated-ldg+4-drop", GATED, dict(ldg=68, drop_p=0.15), EUNSUPPORTED)
                add("gated-drop-1", GATED, dict(drop_p=1.0), EINVAL)
                add("gated-drop-negative", GATED, dict(drop_p=-0.1), EINVAL)
                add("glu-span-drop", GLU, dict(ldp=SPAN, drop_p=0.15), EINVAL)    # (the span is checked first)
                add("dgate-alone-ignored", GLU, dict(dgate=_AT["dgate"]), (ROLL, 0, 0))
            else:
                add("glu-span-lddp", GLU, dict(lddp=SPAN), EINVAL)
                add("gated-span-lddg", GATED, dict(lddg=SPAN), EINVAL if dt == BF16 else (WINDOW, 0, df))
                add("glu-drop-ignored", GLU, dict(drop_p=0.15), (ROLL, 0, 1))
                add("no-dP", GLU, dict(dP=None), EINVAL)
                add("gate-without-dgate", GATED, dict(dgate=None), EINVAL)
                add("dgate-without-gate", GLU, dict(dgate=_AT["dgate"], lddg=64), EINVAL)
                # -- no workspace: the tiled kernel with atomics; no workspace and no dw: nowhere to put the tap gradients
                add("glu-no-ws", GLU, dict(workspace=None), (TILED, 0, 0))
                add("glu-D72-no-ws", GLU, dict(D=72, workspace=None), (TILED, 0, 0))
                add("gated-no-ws", GATED, dict(workspace=None), (TILED, 0, 0))
                add("glu-k29-no-ws", GLU, dict(k=29, workspace=None), (TILED, 0, 0))
                add("glu-no-ws-no-dw", GLU, dict(workspace=None, **NODW), EINVAL)
                # -- dw == NULL (deferred reduction) on each route
                add("glu-no-dw", GLU, NODW, (ROLL, 0, 1))
                add("glu-chunk7-no-dw", GLU, dict(chunk=7, **NODW), (ROLL, 1, 1))
                add("gated-no-dw", GATED, NODW, (csgu[0], 0, 1))
                add("glu-D72-no-dw", GLU, dict(D=72, **NODW), (WINDOW, 0, 1))
                add("glu-k29-no-dw", GLU, dict(k=29, **NODW), EUNSUPPORTED)
                add("glu-D66-no-dw", GLU, dict(D=66, **NODW), EUNSUPPORTED)
                # a bf16 rolling candidate that fails al(8) runs the tiled kernel, so it cannot defer
                add("glu-ldp+4-no-dw", GLU, dict(ldp=132, **NODW), EUNSUPPORTED if dt == BF16 else (ROLL, 0, 1))
                add("gated-dgate+8-no-dw", GATED, dict(dgate=_AT["dgate"] + 8, **NODW), EUNSUPPORTED)
    return t


ROUTES = _table()


@pytest.mark.parametrize("name,backward,dtype,form,kw,want", ROUTES, ids=[r[0] for r in ROUTES])
def test_route_table(name, backward, dtype, form, kw, want):
    shape = dict(form)
    shape.update({n: kw[n] for n in shape if n in kw})
    a = _args(backward, dtype, **shape, **{n: v for n, v in kw.items() if n not in shape})
    code, plan = _query(a, backward)
    if isinstance(want, int):
        assert code == want, f"{name}: code {code}, want {want}"
    else:
        assert code == 0, f"{name}: refused with {code}"
        assert (plan.route, plan.chunked, plan.deferrable) == want, name
        assert plan.grid[0] >= 1 and plan.grid[1] >= 1 and plan.grid[2] >= 1 and plan.partial_rows >= 1
        assert (plan.seg in (32, 64, 128) and plan.nseg == -(-a.T // plan.seg)) if plan.route >= ROLL else (plan.seg == 0 and plan.nseg == 0)


def test_table_has_both_sides_of_every_route_in_both_directions_and_dtypes():
    seen = {(r[1], r[2], r[5][0]) for r in ROUTES if not isinstance(r[5], int)}
    assert seen >= {(d, t, r) for d in (FWD, BWD) for t in (F32, BF16) for r in (TILED, WINDOW, ROLL)} | {(FWD, BF16, CSGU), (BWD, BF16, CSGU)}
    assert {(r[1], r[5]) for r in ROUTES if isinstance(r[5], int)} >= {(FWD, EINVAL), (FWD, EUNSUPPORTED), (BWD, EINVAL), (BWD, EUNSUPPORTED)}


@pytest.mark.parametrize("backward", [FWD, BWD])
def test_empty_shape_is_accepted_and_launches_nothing(backward):
    for kw in (dict(B=0), dict(T=0), dict(D=0)):
        code, plan = _query(_args(backward, BF16, **dict(GLU, **kw)), backward)
        assert code == 0 and list(plan.grid) == [0, 0, 0] and plan.partial_rows == 0


def test_query_needs_a_descriptor_and_a_plan():
    from summarymixing_amd import _lib
    assert _lib.lib().smx_dwconv_plan_query(None, 0, ctypes.byref(_lib.DwconvPlan())) == EINVAL
    assert _lib.lib().smx_dwconv_plan_query(ctypes.byref(_args(FWD, BF16, **GLU)), 0, None) == EINVAL


# ---- row counts and the workspace bound against the library of the commit before the plan ----
_SHAPES = [(1, 9, 8), (1, 9, 64), (1, 40, 16), (2, 31, 64), (3, 16, 64), (2, 47, 192), (3, 70, 40), (2, 70, 64), (2, 150, 96),
           (2, 100, 64), (5, 131, 192), (16, 500, 256), (64, 500, 256), (128, 500, 256), (16, 250, 1536), (40, 1000, 512), (8, 3000, 512)]
_FORMS = [(1, ZERO, 0), (0, REFLECT, 1), (1, REFLECT, 0), (0, ZERO, 1)]          # (glu, pad, gate)
GRID = [(dt, B, T, D, k, glu, pad, chunk, gate) for dt in (F32, BF16) for (B, T, D) in _SHAPES for k in (31, 7)
        for (glu, pad, gate) in _FORMS for chunk in (0, 7)]


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        doc = json.load(f)
    return {tuple(c[:9]): (c[9], c[10]) for c in doc["cases"]}


def test_fixture_covers_exactly_the_grid(parent):
    assert sorted(parent) == sorted(GRID)


def test_partial_rows_and_workspace_equal_the_parent(parent):
    """The backward plan of the aligned call with a workspace reports the row count the parent's pointer-blind query gave, the
    workspace query is unchanged, and the rows fit the workspace on every route; the grid reaches all four routes and the three
    segment lengths of roll_geometry."""
    from summarymixing_amd import _lib
    routes, segs = set(), set()
    for case in GRID:
        dt, B, T, D, k, glu, pad, chunk, gate = case
        code, plan = _query(_args(BWD, dt, B, T, D, k, glu, pad, chunk, gate), BWD)
        assert code == 0, case
        rows, nbytes = parent[case]
        assert plan.partial_rows == rows, (case, plan.partial_rows, rows)
        assert _lib.lib().smx_dwconv1d_glu_bwd_workspace(B, T, D, k) == nbytes, case
        assert plan.partial_rows * D * (k + 1) * 4 <= nbytes, case
        routes.add(plan.route)
        if plan.route >= ROLL:
            segs.add(plan.seg)
            assert plan.grid[0] == 8 * (D // 64) * -(-rows // 8)
    assert routes == {TILED, WINDOW, ROLL, CSGU} and segs == {32, 64, 128}


def test_rows_of_a_misaligned_call_fit_the_workspace_too():
    """The workspace query sees no pointers, so it bounds the route a misaligned bf16 call drops to as well."""
    from summarymixing_amd import _lib
    for (B, T, D) in _SHAPES:
        code, plan = _query(_args(BWD, BF16, B, T, D, 31, 1, ZERO, 0, 0, P=_AT["P"] + 8), BWD)
        assert code == 0 and plan.route == TILED
        assert plan.partial_rows * D * 32 * 4 <= _lib.lib().smx_dwconv1d_glu_bwd_workspace(B, T, D, 31)


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_dwconv_plan_cpu.py --write <libsmx.so of the parent commit> <path>")
    lib = ctypes.CDLL(sys.argv[2])
    lib.smx_dwconv1d_glu_bwd_workspace.restype = ctypes.c_size_t
    cases = [list(c) + [lib.smx_dwconv1d_glu_bwd_partial_rows(*c), lib.smx_dwconv1d_glu_bwd_workspace(c[1], c[2], c[3], c[4])] for c in GRID]
    how = ("python tests/test_dwconv_plan_cpu.py --write <libsmx.so> <this file>, with the library built from the commit before "
           "smx_dwconv_plan_query: its smx_dwconv1d_glu_bwd_partial_rows(dtype, B, T, D, k, glu, pad_mode, chunk, has_gate) and "
           "smx_dwconv1d_glu_bwd_workspace(B, T, D, k), both host arithmetic")
    cols = ["dtype", "B", "T", "D", "k", "glu", "pad_mode", "chunk", "has_gate", "partial_rows", "workspace_bytes"]
    with open(sys.argv[3], "w") as f:
        f.write('{"written_by": %s,\n"columns": %s,\n"cases": [\n%s\n]}\n'
                % (json.dumps(how), json.dumps(cols), ",\n".join(json.dumps(c) for c in cases)))
    print(f"wrote {len(cases)} cases to {sys.argv[3]}")

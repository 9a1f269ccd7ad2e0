"""CPU-side checks of the drop-in boundary: libsmx.so loads and exports every symbol include/smx.h declares,
the ctypes table mirrors the header, and the product path refuses to run without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "smx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(smx_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from summarymixing_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libsmx.so not built (run __graft_entry__.build())"
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/smx.h but not exported"


def test_library_exports_nothing_undeclared():
    """The product library's dynamic `smx_*` symbols are exactly the header's: no debug hooks, no undeclared entry points
    (the clock-stamp setters live in the -DSMX_DIAG build only)."""
    import subprocess
    from summarymixing_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("smx_")})
    assert exported == _declared(), sorted(set(exported) ^ set(_declared()))


def test_ctypes_table_matches_header():
    from summarymixing_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


def test_version_and_error_string_need_no_gpu():
    from summarymixing_amd import _lib
    L = _lib.lib()
    assert L.smx_version() == 100
    assert isinstance(L.smx_last_error(), bytes)


def test_epilogue_struct_layout_matches_header():
    from summarymixing_amd import _lib
    assert ctypes.sizeof(_lib.Epilogue) == 320  # 40 x 8 bytes (round 3: + io_flags, pad_, epoch; round 5: + lnf2_*), see include/smx.h smx_epilogue
    assert _lib.Epilogue.io_flags.offset == 256 and _lib.Epilogue.epoch.offset == 264 and _lib.Epilogue.lnf2_eps.offset == 312


def test_layernorm_descriptor_layouts_match_header():
    from summarymixing_amd import _lib
    F, B = _lib.LnFwd, _lib.LnBwd
    assert ctypes.sizeof(F) == 128 and ctypes.sizeof(B) == 224    # see include/smx.h smx_ln_fwd / smx_ln_bwd
    assert F.X.offset == 8 and F.eps.offset == 64 and F.N.offset == 72 and F.gamma2.offset == 80 and F.Y2.offset == 96
    assert F.eps2.offset == 120 and F.dtype2.offset == 124
    assert B.dY.offset == 8 and B.slabs.offset == 24 and B.nslab.offset == 40 and B.X.offset == 48 and B.R.offset == 88
    assert B.dgamma.offset == 120 and B.workspace.offset == 136 and B.dX2.offset == 144 and B.alpha2.offset == 168
    assert B.drop_seed2.offset == 176 and B.epoch.offset == 184 and B.Z.offset == 192 and B.zact.offset == 208 and B.D.offset == 216


def test_dwconv_descriptor_layouts_match_header():
    from summarymixing_amd import _lib
    A, P = _lib.DwconvArgs, _lib.DwconvPlan
    assert ctypes.sizeof(A) == 176 and ctypes.sizeof(P) == 40     # see include/smx.h smx_dwconv_args / smx_dwconv_plan
    assert A.glu.offset == 4 and A.P.offset == 8 and A.w.offset == 24 and A.gate.offset == 40 and A.Y.offset == 56 and A.dP.offset == 72
    assert A.dgate.offset == 88 and A.dw.offset == 104 and A.dbias.offset == 112 and A.workspace.offset == 120 and A.B.offset == 128
    assert A.k.offset == 140 and A.pad_mode.offset == 144 and A.chunk.offset == 148 and A.drop_p.offset == 152
    assert A.drop_seed.offset == 160 and A.epoch.offset == 168
    assert P.route.offset == 0 and P.chunked.offset == 4 and P.deferrable.offset == 8 and P.partial_rows.offset == 12
    assert P.grid.offset == 16 and P.seg.offset == 28 and P.nseg.offset == 32
    assert (_lib.DW_TILED, _lib.DW_WINDOW, _lib.DW_ROLL, _lib.DW_ROLL_CSGU) == (0, 1, 2, 3)


# Inputs the library refuses, with the code it returns.  The pointers are fake (never dereferenced: every case is refused on the
# host before any launch); BASE is 4 KiB aligned, BASE + 4 / + 8 are the misaligned variants.
_BASE = 1 << 40


def _ln_fwd_args(**kw):
    from summarymixing_amd import _lib
    a = _lib.LnFwd(dtype=_lib.BF16, X=_BASE, ldx=512, gamma=_BASE + 0x100000, beta=_BASE + 0x200000, Y=_BASE + 0x300000, ldy=512,
                   eps=1e-5, N=8, D=512)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _ln_bwd_args(**kw):
    from summarymixing_amd import _lib
    a = _lib.LnBwd(dtype=_lib.BF16, dY=_BASE, lddy=512, X=_BASE + 0x100000, ldx=512, gamma=_BASE + 0x200000, beta=_BASE + 0x300000,
                   stats=_BASE + 0x400000, dX=_BASE + 0x500000, lddx=512, workspace=_BASE + 0x600000, alpha2=1.0, N=8, D=512)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


_PAIR = dict(dtype=0, x_f32=1, gamma2=_BASE + 0x400000, beta2=_BASE + 0x500000, Y2=_BASE + 0x600000, ldy2=512, dtype2=1)
_SLABS = dict(dY=None, lddy=0, slabs=_BASE + 0x700000, nslab=4, slab_stride=8 * 512)
_EINVAL, _EUNSUPPORTED = -1, -2
_LN_FWD_REFUSED = [
    ("no X", dict(X=None), _EINVAL),
    ("N < 0", dict(N=-1), _EINVAL),
    ("D = 0", dict(D=0), _EINVAL),
    ("x_f32, unknown dtype", dict(x_f32=1, dtype=5), _EINVAL),
    ("x_f32, D = 2049", dict(x_f32=1, D=2049, ldx=2052, ldy=2052), _EUNSUPPORTED),
    ("x_f32, D = 2052", dict(x_f32=1, D=2052, ldx=2052, ldy=2052), _EUNSUPPORTED),
    ("x_f32, X 8-byte aligned", dict(x_f32=1, X=_BASE + 8), _EUNSUPPORTED),
    ("x_f32, Y 4-byte aligned", dict(x_f32=1, Y=_BASE + 0x300004), _EUNSUPPORTED),
    ("x_f32, ldx % 4", dict(x_f32=1, ldx=514), _EUNSUPPORTED),
    ("pair, no gamma2", dict(_PAIR, gamma2=None), _EINVAL),
    ("pair, unknown dtype2", dict(_PAIR, dtype2=7), _EINVAL),
    ("pair, bf16 first output", dict(_PAIR, dtype=1), _EINVAL),
    ("pair, activation", dict(_PAIR, act=2), _EINVAL),
    ("pair, D = 2052", dict(_PAIR, D=2052, ldx=2052, ldy=2052, ldy2=2052), _EUNSUPPORTED),
    ("pair, bf16 Y2 4-byte aligned", dict(_PAIR, Y2=_BASE + 0x600004), _EUNSUPPORTED),
    ("pair, float32 Y2 8-byte aligned", dict(_PAIR, dtype2=0, Y2=_BASE + 0x600008), _EUNSUPPORTED),
    ("pair, beta2 8-byte aligned", dict(_PAIR, beta2=_BASE + 0x500008), _EUNSUPPORTED),
]
_LN_BWD_REFUSED = [
    ("no dY and no slabs", dict(dY=None), _EINVAL),
    ("dY and slabs", dict(slabs=_BASE + 0x700000, nslab=4), _EINVAL),
    ("no workspace", dict(workspace=None), _EINVAL),
    ("dgamma without dbeta", dict(dgamma=_BASE + 0x800000), _EINVAL),
    ("drop_p2 = 1", dict(drop_p2=1.0), _EINVAL),
    ("dX2, D = 3072", dict(dX2=_BASE + 0x800000, lddx2=3072, D=3072, lddy=3072, ldx=3072, lddx=3072), _EUNSUPPORTED),
    ("D = 4100", dict(D=4100, lddy=4100, ldx=4100, lddx=4100), _EUNSUPPORTED),
    ("float32 D = 4100, unaligned", dict(dtype=0, D=4100, lddy=4101, ldx=4101, lddx=4101), _EUNSUPPORTED),
    ("x_f32, unknown dtype", dict(x_f32=1, dtype=5), _EINVAL),
    ("x_f32, D = 2049", dict(x_f32=1, D=2049, lddy=2052, ldx=2052, lddx=2052), _EUNSUPPORTED),
    ("x_f32, D = 2052", dict(x_f32=1, D=2052, lddy=2052, ldx=2052, lddx=2052), _EUNSUPPORTED),
    ("x_f32, X 8-byte aligned", dict(x_f32=1, X=_BASE + 0x100008), _EUNSUPPORTED),
    ("slabs, nslab = 17", dict(_SLABS, nslab=17), _EINVAL),
    ("slabs, nslab = 0", dict(_SLABS, nslab=0), _EINVAL),
    ("slabs, float32", dict(_SLABS, dtype=0), _EINVAL),
    ("slabs, dgamma", dict(_SLABS, dgamma=_BASE + 0x800000, dbeta=_BASE + 0x900000), _EINVAL),
    ("slabs, D = 2052", dict(_SLABS, D=2052, ldx=2052, lddx=2052), _EUNSUPPORTED),
    ("slabs, slabs 8-byte aligned", dict(_SLABS, slabs=_BASE + 0x700008), _EUNSUPPORTED),
    ("slabs, x_f32, X 8-byte aligned", dict(_SLABS, x_f32=1, X=_BASE + 0x100008), _EUNSUPPORTED),
    ("preact, activation", dict(Z=_BASE + 0x800000, ldz=512, act=2), _EUNSUPPORTED),
    ("preact, D % 8", dict(Z=_BASE + 0x800000, ldz=516, D=516, lddy=516, ldx=516, lddx=516), _EUNSUPPORTED),
    ("preact, D = 2056", dict(Z=_BASE + 0x800000, ldz=2056, D=2056, lddy=2056, ldx=2056, lddx=2056), _EUNSUPPORTED),
    ("preact, float32", dict(Z=_BASE + 0x800000, ldz=512, dtype=0), _EUNSUPPORTED),
    ("preact, Z 8-byte aligned", dict(Z=_BASE + 0x800008, ldz=512), _EUNSUPPORTED),
    ("preact, R", dict(Z=_BASE + 0x800000, ldz=512, R=_BASE + 0x900000, ldr=512), _EINVAL),
    ("preact, dX2", dict(Z=_BASE + 0x800000, ldz=512, dX2=_BASE + 0x900000, lddx2=512), _EINVAL),
]


@pytest.mark.parametrize("case,kw,code", _LN_FWD_REFUSED, ids=[c[0] for c in _LN_FWD_REFUSED])
def test_layernorm_fwd_refuses_what_it_cannot_run(case, kw, code):
    from summarymixing_amd import _lib
    assert _lib.lib().smx_layernorm_fwd(ctypes.byref(_ln_fwd_args(**kw)), None) == code, case


@pytest.mark.parametrize("case,kw,code", _LN_BWD_REFUSED, ids=[c[0] for c in _LN_BWD_REFUSED])
def test_layernorm_bwd_refuses_what_it_cannot_run(case, kw, code):
    from summarymixing_amd import _lib
    assert _lib.lib().smx_layernorm_bwd(ctypes.byref(_ln_bwd_args(**kw)), None) == code, case


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    from summarymixing_amd.nnet.summary_mixing import SummaryMixing
    m = SummaryMixing(8, 1, [8], 8, [8], 8, global_dropout=0.0)
    with pytest.raises((AssertionError, RuntimeError)):
        m(torch.randn(1, 3, 8))


def test_wgrad_item_struct_layout_matches_header():
    from summarymixing_amd import _lib
    assert ctypes.sizeof(_lib.WgradItem) == 56  # 5 x 8 + 4 x 4 bytes, see include/smx.h smx_wgrad_item
    assert ctypes.sizeof(_lib.ReduceJob) == 56


def test_config_is_read_once_and_queryable():
    """smx_get_config returns the knobs the library read from the environment (include/smx.h: smx_config); a later change
    of the environment does not reach the library (no getenv on any call path)."""
    from summarymixing_amd import _lib
    before = _lib.get_config()
    assert before["t256"] == int(os.environ.get("SMX_T256", 1)) and before["ln_tile_rows"] == 128
    assert before["diag_build"] == 0 and before["gemm_ablate"] == 0 and before["wgroup_ablate"] == 0 and before["dwroll_ablate"] == 0
    old = os.environ.get("SMX_T256")
    os.environ["SMX_T256"] = "2" if before["t256"] != 2 else "0"
    try:
        assert _lib.get_config() == before
    finally:
        if old is None:
            del os.environ["SMX_T256"]
        else:
            os.environ["SMX_T256"] = old


def test_grouped_wgrad_slice_plan_is_size_aware():
    """smx_wgrad_group_splits is host logic (no GPU): the slice count comes from a cost model - rounds x 64-frame steps + one
    written-and-re-read fp32 slab per tile and slice.  At 64 000 frames it keeps the counts tuned in round 2 (C2b layer: 11,
    C2a layer: 8); at the recipe batch (3750 frames) a slice costs a sixth of the kernel and two beat the five that 'fill the
    chip'; a ragged frame count plans like its multiple of 64."""
    from summarymixing_amd import _lib as L
    lib = L.lib()

    def plan(rows, shapes):
        items = (L.WgradItem * len(shapes))()
        for it, (M, K) in zip(items, shapes):
            it.M, it.K, it.want_bias = M, K, 1
        return lib.smx_wgrad_group_splits(rows, items, len(shapes))
    c2b = [(1024, 256), (256, 1024), (1024, 256), (256, 1024), (512, 256), (256, 512), (512, 256), (256, 256)]
    c2a = [(2048, 512), (512, 2048), (2048, 512), (512, 2048), (1024, 512), (512, 1024), (1024, 512), (512, 512)]
    assert plan(64000, c2b) == 11
    assert plan(64000, c2a) == 8
    assert plan(3750, c2a) == 2
    assert plan(3750, c2a) == plan(3712, c2a)
    assert plan(63, c2b) == 0 and plan(64, c2b) == 1          # fewer than 64 frames: not this kernel's job
    for rows in (64, 700, 3750, 16000, 64000, 240000):
        s = plan(rows, c2a)
        assert 1 <= s <= max(1, rows // 64 // 8) or s == 1    # at least 8 steps of 64 frames per slice


def test_launch_geometry_rules_need_no_gpu_and_hold_their_measured_cells():
    """The library's geometry choices are host arithmetic (no GPU): the panel height (smx_gemm_panel_rows) and the row-complete
    LayerNorm tile (smx_gemm_ln_tile_rows_for) at the sizes whose A/B tables are in tools/experiments/r06_smalln/README.md."""
    import subprocess
    import sys
    # (a fresh process with the knobs unset: the library reads SMX_PANEL_ROWS / SMX_LN_TILE64 once)
    code = ("import ctypes;from summarymixing_amd import _lib;L=_lib.lib();"
            "print([L.smx_gemm_panel_rows(n,m) for n,m in ((3750,2048),(3750,1024),(500,1024),(12000,512),(32000,1024),(36000,1024),(64000,1024),(240000,2048),(240000,512))]);"
            "print([L.smx_gemm_ln_tile_rows_for(n,m) for n,m in ((17500,256),(32000,256),(36000,256),(64000,256),(32000,512),(0,256))]);"
            "print([L.smx_pool_bcast_ok(b,t,d) for b,t,d in ((10,375,512),(1,500,256),(128,500,256),(8,30000,512),(2,4096,64),(2,4097,64))])")
    env = {k: v for k, v in os.environ.items() if k not in ("SMX_PANEL_ROWS", "SMX_LN_TILE64", "SMX_POOL_FUSE_MAX_ROWS")}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True, cwd=ROOT, env=env).stdout.splitlines()
    rows, tiles, pools = eval(out[-3]), eval(out[-2]), eval(out[-1])
    # 3750 frames: 64-row panels for the 2048-wide up-projection, 32 rows at 1024 (one round of 188-256 workgroups); one utterance: 32 rows;
    # 12 000 x 512: 64 rows; 32 000 rows = 250 panels of 128; 36 000 rows (282 panels) takes the geometry that fills its rounds; config 5's
    # 1875 panels stay on 128 rows (the round-efficiency rule stops at four rounds)
    assert rows[0] == 64 and rows[1] == 32 and rows[2] == 32 and rows[3] == 64 and rows[4] == 128 and rows[6] == 128
    assert rows[5] in (64, 128) and rows[7] == 128 and rows[8] == 128
    # the 64-row LayerNorm tile where 128-row tiles leave one workgroup per CU (<= 32 768 rows at d_model 256), never at d_model 512
    assert tiles == [64, 64, 128, 128, 128, 128]
    assert pools == [1, 1, 1, 0, 1, 0]

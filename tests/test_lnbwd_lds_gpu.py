"""The LayerNorm-backward epilogue of the 128 x 256 GEMM tile with its side rows landed in LDS (SMX_LNB_LDS, gemm_common.h lnb_lds_item).

The cases are written in the vocabulary of tests/_gemm_cases.py (families registered here under names of their own; that file is not
edited) and run through the buffers of tests/test_gemm_routes_gpu.py: every operand a view inside a poisoned buffer with ld > width,
every output checked per element against float64 within the derived bar of tests/_gemm_ref.py, a second call reproducing every bit.

Shapes: M = 256 (row-complete); K in {64, 192, 256}: the shortest reduction the tile takes (two 32-element steps), a longer one, the
flagship's; N in {137, 128, 165, 389}: a tail tile with less than one half (9 rows), exactly one tile, two tiles with a 37-row tail that
ends inside a half, four tiles with a 5-row tail that ends inside a phase.  (smx_gemm sends a LayerNorm-fused GEMM to this tile only
with N >= 128 and K % 64 == 0 - smx_gemm_ln_fused_ok, pinned by test_what_never_reaches_the_fused_tile - so a 16-row GEMM, one step
(K = 32) and an odd step count (K = 96) cannot be run: "less than one half" is a tail tile here, the step count is always even.)
Forms: LNF 1 / 3 / 5 / 7, with and without res, with and without the second output (its mask, dropout 0 and 0.15, z with
Swish), bf16 and float32 ln_x.  Every family meets every N and every K.

The knob is read once per process, so each value runs in one child process, which prints a SHA-256 of every written buffer (guards
included); the two sets must be equal: the LDS path moves the same data by another route and computes the same bits.  One more child
runs LNF 5 at N = 66 560 (520 tiles: every CU busy, where a wrong hand-placed wait would show) twice and compares the bits."""
import functools
import hashlib
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

_RES = dict(res="T")
_DX2M = dict(dx2=True, mask2=True, alpha2=0.5, drop2=(0.15, 0x2468ACE))
_DX2 = dict(dx2=True, alpha2=1.0)                          # no mask, dropout 0
# name -> (LNF, family)
FORMS = {
    "lnbl_1_res": (1, G._fam(ln=dict(kind="bwd"), **_RES)),
    "lnbl_1_nores": (1, G._fam(ln=dict(kind="bwd"))),
    "lnbl_1_dx2m": (1, G._fam(ln=dict(kind="bwd", **_DX2M), **_RES)),
    "lnbl_1_dx2": (1, G._fam(ln=dict(kind="bwd", **_DX2))),
    "lnbl_3_z": (3, G._fam(act=G.ACT_SWISH, ln=dict(kind="bwd", z2=True, lnf_act=G.ACT_NONE, **_DX2M), **_RES)),
    "lnbl_3_lact": (3, G._fam(ln=dict(kind="bwd", lnf_act=G.ACT_GELU))),
    "lnbl_5_res": (5, G._fam(ln=dict(kind="bwd", x32=True), **_RES)),
    "lnbl_5_dx2m": (5, G._fam(ln=dict(kind="bwd", x32=True, **_DX2M), **_RES)),
    "lnbl_5_dx2": (5, G._fam(ln=dict(kind="bwd", x32=True, **_DX2))),
    "lnbl_7_z": (7, G._fam(act=G.ACT_SWISH, ln=dict(kind="bwd", x32=True, z2=True, lnf_act=G.ACT_NONE, **_DX2M), **_RES)),
    "lnbl_7_z_nomask": (7, G._fam(act=G.ACT_SWISH, ln=dict(kind="bwd", x32=True, z2=True, lnf_act=G.ACT_NONE, **_DX2))),
    "lnbl_7_lact": (7, G._fam(ln=dict(kind="bwd", x32=True, lnf_act=G.ACT_SWISH, **_DX2M), **_RES)),
}
for _name, (_lnf, _f) in FORMS.items():
    assert _name not in G.FAMILIES or G.FAMILIES[_name] == _f
    G.FAMILIES[_name] = _f
NS, KS = (137, 128, 165, 389), (64, 192, 256)
ENV = {"SMX_LN_TILE64": "0"}                               # (below ~37 000 frames the default rule takes the 64-row tile)


def cases():
    out = []
    for fi, (name, (lnf, _)) in enumerate(FORMS.items()):
        for ni, N in enumerate(NS):
            lay = "NN" if (fi + ni) % 3 else "NT"          # (NN is the product's dgrad layout)
            G._mk(out, "lnbl", "bf16", lay, (N, 256, KS[(fi + ni) % 3]), "offset" if (fi, ni) == (6, 2) else "aligned", name,
                  G.plan(lay, 128, 256, 1, lnf), env=ENV)
    return out


def _sha(buf):
    from tests.test_gemm_routes_gpu import _bits
    return hashlib.sha256(_bits(buf).cpu().numpy().tobytes()).hexdigest()


def run_case(case, dev="cuda"):
    """tests/test_gemm_routes_gpu.run_case, returning the hash of every written buffer as well."""
    from summarymixing_amd import ops
    from tests import test_gemm_routes_gpu as RT
    torch.manual_seed(zlib.crc32(case.name.encode()))
    f = G.fam(case)
    bufs = RT.Buffers(case, dev)
    t = RT._fill(case, bufs, dev)
    written = [n for n, op in bufs.ops.items() if op.role == "w"]
    before = {n: RT._bits(bufs.buf[n]).clone() for n in written}
    keep2 = None
    if f["ln"].get("drop2"):
        keep2 = ops.dropout(torch.ones(case.N, case.M, device=dev), *f["ln"]["drop2"]) != 0
    outs, info = R.reference(case, t, None, keep2)
    assert set(outs) == set(written), (case.name, sorted(outs), sorted(written))
    RT._call(case, bufs, True)
    torch.cuda.synchronize()
    worst, hashes = 0.0, {}
    for n in written:
        after = RT._bits(bufs.buf[n])
        bad = (after != before[n]) & ~bufs.inside[n]
        assert not bool(bad.any()), f"{case.name}: {n} was written OUTSIDE its view at buffer elements {bad.nonzero()[:8, 0].tolist()}"
        got = bufs.view[n]
        assert not bool(torch.isnan(got.float()).any()), f"{case.name}: NaN in {n}: the kernel read outside an operand it was given"
        ref, bar, zero = outs[n]
        g = got.double().reshape(-1, 2, case.M).sum(0) if n == "ln_partial" else (got if n == "C" else got[0])
        if zero is not None:
            nz = zero & (g != 0)
            assert not bool(nz.any()), f"{case.name}: {n} holds a non-zero value at the dropped position {nz.nonzero()[0].tolist()}"
        w, msg = R.worst(case, n, g, ref, bar)
        print(f"{case.name} {n}: err / bar {w:.4f}")
        assert w <= 1.0, msg
        worst = max(worst, w)
        hashes[n] = _sha(bufs.buf[n])
    for n in written:
        RT._bits(bufs.buf[n]).copy_(before[n])
    RT._call(case, bufs, False)
    torch.cuda.synchronize()
    for n in written:
        assert _sha(bufs.buf[n]) == hashes[n], f"{case.name}: {n} differs between two identical calls"
    report("lnbwd_lds", {"case": case.name, "lnb_lds": os.environ.get("SMX_LNB_LDS", ""), "err_over_bar": round(worst, 4), "t_act": info["t_act"]})
    return hashes


def run_full_chip(dev="cuda"):
    """LNF 5 on 520 tiles, K = 256: two calls, the same bits.  (No float64 reference at this size: the small cases have it.)"""
    from tests import test_gemm_routes_gpu as RT
    out = []
    G._mk(out, "lnbl", "bf16", "NN", (66560, 256, 256), "aligned", "lnbl_5_dx2m", G.plan("NN", 128, 256, 1, 5), env=ENV)
    case = out[0]
    torch.manual_seed(5)
    bufs = RT.Buffers(case, dev)
    RT._fill(case, bufs, dev)
    written = [n for n, op in bufs.ops.items() if op.role == "w"]
    before = {n: RT._bits(bufs.buf[n]).clone() for n in written}
    RT._call(case, bufs, True)
    torch.cuda.synchronize()
    first = {}
    for n in written:
        assert torch.equal(RT._bits(bufs.buf[n])[~bufs.inside[n]], before[n][~bufs.inside[n]]), f"{n} was written outside its view"
        assert not bool(torch.isnan(bufs.view[n].float()).any()), f"NaN in {n}"
        first[n] = RT._bits(bufs.buf[n]).clone()
        RT._bits(bufs.buf[n]).copy_(before[n])
    RT._call(case, bufs, False)
    torch.cuda.synchronize()
    for n in written:
        diff = (RT._bits(bufs.buf[n]) != first[n]).nonzero()
        assert diff.numel() == 0, f"{n}: {diff.shape[0]} elements differ between two identical calls, first at buffer element {diff[0].tolist()}"


def _child_main():
    from summarymixing_amd import _lib as L
    cfg = L.get_config()
    assert cfg["lnb_lds"] == int(os.environ["SMX_LNB_LDS"]) and cfg["ln_tile64"] == 0, cfg
    if os.environ.get("SMX_LNBL_MODE") == "full_chip":
        run_full_chip()
        print("HASHES {}")
        return
    print("HASHES " + json.dumps({c.name: run_case(c) for c in cases()}))


@functools.lru_cache(maxsize=None)
def _child(lds, mode="cases"):
    env = dict(os.environ, SMX_LNB_LDS=str(lds), SMX_LNBL_MODE=mode, **ENV)
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_lnbwd_lds_gpu import _child_main; _child_main()" % ROOT],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("HASHES ")]
    return p.returncode, p.stdout[-4000:] + p.stderr[-4000:], json.loads(lines[-1][7:]) if lines else None


@pytest.mark.parametrize("lds", [1, 0], ids=["lds", "registers"])
def test_every_form_per_element_vs_fp64_in_poisoned_buffers(lds):
    rc, log, hashes = _child(lds)
    assert rc == 0 and hashes is not None, log
    assert set(hashes) == {c.name for c in cases()}


def test_lds_path_and_register_path_write_the_same_bits():
    (rc1, log1, h1), (rc0, log0, h0) = _child(1), _child(0)
    assert rc1 == 0 and h1 is not None, log1
    assert rc0 == 0 and h0 is not None, log0
    diff = [(c, n) for c in h1 for n in h1[c] if h1[c][n] != h0[c][n]]
    assert not diff, f"SMX_LNB_LDS=1 and =0 differ in {len(diff)} buffers: {diff[:12]}"


def test_full_chip_grid_is_deterministic():
    rc, log, _ = _child(1, "full_chip")
    assert rc == 0, log


def test_what_never_reaches_the_fused_tile():
    """Why the smallest cases are a 9-row tail tile and K = 64: the dispatcher refuses the fused LayerNorm below 128 rows and for a
    reduction that is no multiple of 64 (smx_gemm_ln_fused_ok is the rule launch_layout applies)."""
    from summarymixing_amd import _lib as L
    ok = L.lib().smx_gemm_ln_fused_ok
    assert ok(L.BF16, 16, 256, 256) == 0 and ok(L.BF16, 128, 256, 32) == 0 and ok(L.BF16, 128, 256, 96) == 0
    assert ok(L.BF16, 128, 256, 64) == 1 and ok(L.BF16, 137, 256, 192) == 1

"""The GEMM route table of tests/_gemm_cases.py is true (no GPU): smx_gemm_plan_query runs the checks and the dispatch of smx_gemm on
host arithmetic alone and dereferences nothing but the epilogue struct, so every case is asked with fabricated pointers of its
alignment class and the eight plan fields are compared with the route the table names.  Cases that need a knob (SMX_T256,
SMX_LN_TILE64: read once per process) are asked in one child process per knob value, which prints its plans as JSON.

Also asserted: the table reaches every launch site of smx_gemm, every vector case of a route that has an element-guarded kernel has
an `odd` sibling on the same tile, the fused LayerNorm shapes refuse N = 127, and the default 64 / 128-row rule of the d_model = 256
LayerNorm tiles sits where DESIGN.md says."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from tests import _gemm_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BASE = 1 << 40                                            # 4 KiB aligned; operand i lives at _BASE + i * 2^32
_NAMES = ("A", "B", "C", "bias", "c0", "z", "row_mask", "res", "colsum", "workspace", "ln_x", "ln_stats", "ln_gamma", "ln_partial", "ln_dx2",
          "ln_mask2", "lnf_gamma", "lnf_beta", "lnf_y", "lnf_stats", "lnf2_gamma", "lnf2_beta", "lnf2_y", "lnf2_stats")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from summarymixing_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["bash", os.path.join(ROOT, "summarymixing_amd", "csrc", "build.sh")], check=True)


def fake_ptr(case):
    ops = {o.name: o for o in G.operands(case)}

    def ptr(name):
        base = _BASE + (_NAMES.index(name) << 32)
        return base if name == "workspace" else base + G.view_offset(case, ops[name]) * G.esize(case, ops[name])
    return ptr


def query(case):
    """-> (return code, plan tuple)"""
    from summarymixing_amd import _lib as L
    ptr = fake_ptr(case)
    epi, plan = G.make_epilogue(case, ptr), L.GemmPlan()
    rc = L.lib().smx_gemm_plan_query(*G.gemm_args(case, ptr), ctypes.byref(epi), ctypes.byref(plan))
    return rc, tuple(getattr(plan, n) for n, _ in L.GemmPlan._fields_)


def _child_main():
    key = tuple(tuple(kv) for kv in json.loads(os.environ["SMX_ROUTE_GROUP"]))
    print("PLANS " + json.dumps({c.name: query(c) for c in G.env_groups()[key]}))


_GROUPS = G.env_groups()


@pytest.mark.parametrize("key", list(_GROUPS), ids=lambda k: ",".join(f"{a}={b}" for a, b in k) or "default")
def test_every_case_takes_the_route_the_table_names(key):
    cases = _GROUPS[key]
    if key:
        env = dict(os.environ, SMX_ROUTE_GROUP=json.dumps(key), **dict(key))
        p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gemm_routes_cpu import _child_main; _child_main()" % ROOT],
                           env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0 and "PLANS " in p.stdout, p.stderr[-2000:]
        got = {k: (v[0], tuple(v[1])) for k, v in json.loads(p.stdout.split("PLANS ", 1)[1]).items()}
    else:
        from summarymixing_amd import _lib as L
        cfg = L.get_config()
        assert cfg["t256"] == 1 and cfg["ln_tile64"] == 1, f"the default group needs the default knobs, got {cfg}"
        got = {c.name: query(c) for c in cases}
    wrong = [f"{c.name}: expected {c.plan}, got rc={got[c.name][0]} plan={got[c.name][1]}" for c in cases if got[c.name] != (0, c.plan)]
    assert not wrong, "\n".join(wrong)


def test_the_table_reaches_every_launch_site_of_smx_gemm():
    hit = {(c.plan[0], c.plan[3], c.plan[4], c.plan[6], c.plan[5]) for c in G.CASES}
    assert hit == G.LAUNCH_SITES, (sorted(G.LAUNCH_SITES - hit), sorted(hit - G.LAUNCH_SITES))


def test_every_vector_case_has_an_odd_sibling_on_the_same_tile():
    """... on the routes that have an element-guarded instantiation (launch_tile: 64 x 64, 128 x 128, 128 x 256 without a LayerNorm); the
    256 x 256 tile, the LDS-DMA kernel and the row-complete LayerNorm tiles exist as vector kernels only."""
    both = {(64, 64), (128, 128), (128, 256)}
    odd = {(c.dtype, c.layout) + c.plan[3:5] for c in G.CASES if c.align == "odd" and c.plan[5] == 0 and c.plan[0] == 0}
    missing = [c.name for c in G.CASES if c.plan[5] == 1 and c.plan[0] == 0 and c.plan[6] == 0 and c.plan[3:5] in both
               and (c.dtype, c.layout) + c.plan[3:5] not in odd]
    assert not missing, missing
    assert all(c.plan[5] == 0 for c in G.CASES if c.align == "odd")
    assert 150 <= len(G.CASES) <= 260


def test_fused_layernorm_refuses_fewer_than_128_rows():
    from summarymixing_amd import _lib as L
    for c in G.CASES:
        if G.fam(c)["ln"] and c.N == 128 and not c.env:
            assert query(c)[0] == 0
            rc, plan = query(c._replace(N=127))
            assert rc == -2, (c.name, rc, plan)            # SMX_EUNSUPPORTED
            assert L.lib().smx_gemm_ln_fused_ok(L.BF16, 127, c.M, c.K) == 0 and L.lib().smx_gemm_ln_fused_ok(L.BF16, 128, c.M, c.K) == 1


def test_default_rule_of_the_64_row_layernorm_tile():
    from summarymixing_amd import _lib as L
    assert L.get_config()["ln_tile64"] == 1
    assert L.lib().smx_gemm_ln_tile_rows_for(32768, 256) == 64
    assert L.lib().smx_gemm_ln_tile_rows_for(32769, 256) == 128
    assert L.lib().smx_gemm_ln_tile_rows_for(200, 512) == 128

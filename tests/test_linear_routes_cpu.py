"""The kernel route every Linear takes (functional._fwd_route / _dgrad_route), without a GPU: the library's *_ok queries are host
arithmetic, and the launch wrappers are replaced by recorders, so linear_fwd / linear_bwd run on CPU tensors and the test reads
which kernels they would have launched and how many LayerNorms rode along.  Regimes: one utterance (500 frames), the recipe batch
(3750 frames, d_model 512), the split-K edge (2048 / 2049), the LayerNorm-fusion threshold (16 000 / 17 500), C2b (64 000)."""
import pytest
import torch

from summarymixing_amd import _lib as L
from summarymixing_amd import functional as F
from summarymixing_amd import ops

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def launches(monkeypatch):
    rec = []

    def epilogue(**kw):
        return {k for k in ("ln_fwd", "ln_fwd2", "ln_bwd", "act_grad_z", "res", "c0") if kw.get(k) is not None}
    monkeypatch.setattr(ops, "epilogue", epilogue)
    monkeypatch.setattr(ops, "gemm", lambda layout, a, b, c, N, M, K, e=None, **kw: rec.append(("gemm", N, M, K, e or set())))
    monkeypatch.setattr(ops, "gemm_panel", lambda a, wp, c, N, M, K, e=None: rec.append(("panel", N, M, K, e or set())))
    monkeypatch.setattr(ops, "gemm_panel_slabs", lambda a, wp, s, N, M, ks, ns: rec.append(("slabs", N, M, ks, ns)))
    monkeypatch.setattr(ops, "slab_epilogue", lambda s, ns, out, N, M, e: rec.append(("slab_epilogue", ns, e)))
    monkeypatch.setattr(ops, "act_mask_bwd", lambda *a, **k: rec.append(("act_mask_bwd",)))
    monkeypatch.setattr(F, "wpacked", lambda *a, **k: None)
    monkeypatch.setattr(F, "_wgrad", lambda *a: rec.append(("wgrad",)))
    monkeypatch.setattr(F, "defer", lambda *a, **k: None)
    monkeypatch.setattr(F, "deferred_ws", lambda *a, **k: torch.empty(16, dtype=torch.uint8))
    monkeypatch.setattr(F, "_LN_FUSE_MIN_ROWS", 17500)       # (the shipped threshold, whatever the conftest fixtures did)
    return rec


def _ln(M, want_stats=True, stream_out=False, pair=False):
    g, b = torch.ones(M), torch.zeros(M)
    return F.LnNext(g, b, 1e-5, want_stats, stream_out, (torch.ones(M), torch.zeros(M), 1e-5) if pair else None)


def fwd(rec, N, M, K, dtype=BF, wparam=True, res=F32, ln=True, c0=False, w_off=0, act=L.ACT_NONE, **lnkw):
    """linear_fwd of x (N, K) -> (N, M); returns (kinds of the launches, LayerNorms fused)."""
    x = torch.empty((N, K), dtype=dtype)
    W = torch.empty((M, K + w_off), dtype=dtype)[:, w_off:]
    post = []
    F.linear_fwd(x, W, None, act, res=None if res is None else torch.empty((N, M), dtype=res),
                 c0=torch.empty((N, M)) if c0 else None, save_z=act != L.ACT_NONE,
                 ln_next=_ln(M, **lnkw) if ln else None, ln_post=post, wparam=torch.empty((M, K)) if wparam else None)
    launched = [r for r in rec if r[0] in ("gemm", "panel", "slabs", "slab_epilogue")]
    rec.clear()
    return [r[0] for r in launched], len(post), launched


def test_ffn_down_projection_routes(launches):
    """FFN down-projection + residual + the LayerNorm that follows it (d_model 256 unless stated)."""
    # one utterance and the split-K edge: K-slices summed by the reducer, which also runs the LayerNorm
    kinds, nln, got = fwd(launches, 500, 256, 1024)
    assert kinds == ["slabs", "slab_epilogue"] and nln == 1 and got[0][3:] == (256, 4) and "ln_fwd" in got[1][2]
    assert fwd(launches, 2048, 256, 1024)[:2] == (["slabs", "slab_epilogue"], 1)
    assert fwd(launches, 2049, 256, 1024)[:2] == (["gemm"], 0)
    # the recipe batch (d_model 512): no split-K, below the fusion threshold -> tiled, the LayerNorm runs on its own
    assert fwd(launches, 3750, 512, 2048)[:2] == (["gemm"], 0)
    # the LayerNorm-fusion threshold
    assert fwd(launches, 16000, 256, 1024)[:2] == (["gemm"], 0)
    kinds, nln, got = fwd(launches, 17500, 256, 1024)
    assert kinds == ["gemm"] and nln == 1 and "ln_fwd" in got[0][4]
    # C2b: norm2 rides in the tile, and the next layer's first LayerNorm with it (float32 stream)
    kinds, nln, got = fwd(launches, 64000, 256, 1024, stream_out=True, pair=True)
    assert kinds == ["gemm"] and nln == 2 and {"ln_fwd", "ln_fwd2"} <= got[0][4]
    # d_model 512 at 64 000 rows: fused in a training step only
    assert fwd(launches, 64000, 512, 2048)[:2] == (["gemm"], 1)
    assert fwd(launches, 64000, 512, 2048, want_stats=False)[:2] == (["gemm"], 0)


def test_layernorm_fusion_needs_an_aligned_bf16_tile(launches):
    assert fwd(launches, 17500, 256, 1024, w_off=1)[:2] == (["gemm"], 0)        # an odd-offset column slice of W: no scalar path
    assert fwd(launches, 17500, 256, 1024, dtype=F32, res=None)[:2] == (["gemm"], 0)
    # the cell's merge with the pooled side input c0 (no wparam: never split-K): tiled, the LayerNorm from the threshold on
    assert fwd(launches, 500, 256, 256, wparam=False, c0=True)[:2] == (["gemm"], 0)
    assert fwd(launches, 17500, 256, 256, wparam=False, c0=True)[:2] == (["gemm"], 1)


def test_split_k_refused_means_the_layernorm_is_not_fused(launches):
    """bf16 500 x 1024 -> 256 with wparam, c0 and a LayerNorm: split-K cannot carry c0, and 500 rows are below the tiled fusion
    threshold, so the Linear runs tiled and the LayerNorm is left to the caller.  (The parent approved the LayerNorm through
    split-K, then refused split-K in linear_fwd and fused it on the tile anyway; no caller reaches this shape.)"""
    assert L.lib().smx_gemm_ln_fused_ok(L.BF16, 500, 256, 1024) == 1
    kinds, nln, got = fwd(launches, 500, 256, 1024, c0=True)
    assert kinds == ["gemm"] and nln == 0 and "ln_fwd" not in got[0][4]


def test_layernorm_that_cannot_fuse_leaves_the_panel_route_open(launches):
    """FFN up-projection (no residual): a requested LayerNorm that cannot ride along does not block the panel-resident GEMM."""
    assert fwd(launches, 3750, 2048, 512, res=None, act=L.ACT_SWISH)[:2] == (["panel"], 0)
    assert fwd(launches, 3750, 2048, 512, res=None, act=L.ACT_SWISH, ln=False)[:2] == (["panel"], 0)
    assert fwd(launches, 500, 1024, 256, res=None, act=L.ACT_SWISH, ln=False)[:2] == (["gemm"], 0)      # below the panel rows
    # one K-slice and no LayerNorm to absorb: the reducer would be one launch more
    assert fwd(launches, 500, 256, 256, res=None, ln=False)[:2] == (["gemm"], 0)
    assert fwd(launches, 500, 256, 1024, res=None, ln=False)[:2] == (["slabs", "slab_epilogue"], 0)


class _LnBwd:
    """Stands in for ln_fwd's backward closure: records the standalone LayerNorm backward."""

    def __init__(self, rec, N, D):
        self.rec = rec
        w, b = torch.ones(D, requires_grad=True), torch.zeros(D, requires_grad=True)
        self.spec = {"x": torch.empty((N, D), dtype=BF), "w": w, "b": b, "stats": torch.empty((N, 2)), "act": L.ACT_NONE,
                     "gw_param": w, "gb_param": b}

    def __call__(self, dy, res=None, second=None):
        self.rec.append(("ln_bwd", type(dy).__name__))
        return dy


def dgrad_ln(rec, N, M, D, packed=True):
    """dgrad of a Linear (D -> M) whose input is a LayerNorm output, carried through the LayerNorm (dgrad_ln_bwd)."""
    Wp, bp = torch.empty((M, D), requires_grad=True), torch.empty(M, requires_grad=True)
    F.dgrad_ln_bwd(_LnBwd(rec, N, D), torch.empty((N, M), dtype=BF), torch.empty((N, D), dtype=BF), torch.empty((M, D), dtype=BF),
                   Wp, bp, res=torch.empty((N, D), dtype=BF), packed=packed, dz_ready=True)
    out = [r for r in rec if r[0] in ("gemm", "panel", "slabs", "ln_bwd")]
    rec.clear()
    return out


def test_dgrad_layernorm_backward_routes(launches):
    # one utterance: the dgrad as split-K slabs, summed by the standalone LayerNorm backward
    got = dgrad_ln(launches, 500, 1024, 256)
    assert [r[0] for r in got] == ["slabs", "ln_bwd"] and got[-1][1] == "Slabs"
    # the conv module's LN2: not on the packed kernels -> tiled, then the LayerNorm backward
    assert [r[0] for r in dgrad_ln(launches, 500, 256, 256, packed=False)] == ["gemm", "ln_bwd"]
    # the recipe batch (d_model 512): neither slabs nor a fused LayerNorm
    assert [r[0] for r in dgrad_ln(launches, 3750, 2048, 512)] == ["gemm", "ln_bwd"]
    # from the threshold on, the LayerNorm backward rides in the dgrad epilogue
    got = dgrad_ln(launches, 17500, 1024, 256)
    assert [r[0] for r in got] == ["gemm"] and "ln_bwd" in got[0][4]
    assert [r[0] for r in dgrad_ln(launches, 64000, 1024, 256)] == ["gemm"]


def test_dgrad_panel_routes(launches):
    """The FFN down-projection's dgrad with the up-projection's activation gradient in its epilogue, and a plain dgrad."""
    def bwd(N, M, K, up=True, wparam=True):
        F.linear_bwd(torch.empty((N, M), dtype=BF), torch.empty((N, K), dtype=BF), torch.empty((M, K), dtype=BF), None, L.ACT_NONE,
                     None, 1.0, None, None, up=(torch.empty((N, K), dtype=BF), L.ACT_SWISH, None, 1.0, None, None) if up else None,
                     wparam=torch.empty((M, K)) if wparam else None)
        out = [r for r in launches if r[0] in ("gemm", "panel")]
        launches.clear()
        return out
    got = bwd(64000, 256, 1024)
    assert [r[0] for r in got] == ["panel"] and "act_grad_z" in got[0][4]
    assert [r[0] for r in bwd(64000, 256, 1024, wparam=False)] == ["gemm"]
    assert [r[0] for r in bwd(500, 256, 1024)] == ["gemm"]                     # below the panel rows
    assert [r[0] for r in bwd(16000, 1024, 256, up=False)] == ["gemm"]         # K = 1024 reduce: not a panel shape
    assert [r[0] for r in bwd(16000, 256, 1024, up=False)] == ["panel"]

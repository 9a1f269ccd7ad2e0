"""The launch sequence of the SummaryMixing cell (functional.cell_run), without a GPU: every launch wrapper the cell reaches is replaced
by a recorder that returns correctly shaped CPU tensors, so the cell's forward and backward run on the host and the test reads which
kernels they would have launched, in which order, on which buffers (shape, leading dimension and offset tell a view of the merge input
`cat` or of the fused gradient `dg` from a buffer of its own) and with which dropout seeds (drawn 1, 2, ... in order).

The full sequences are pinned against tests/golden/cell_routes.json, recorded from the cell before it was split into summary operators
and phases; the tests below that file's comparison spell out by hand what identifies each route."""
import json
import os

import pytest
import torch

from summarymixing_amd import _lib as L
from summarymixing_amd import functional as F
from summarymixing_amd import ops
from summarymixing_amd import sequence_parallel as SP
from summarymixing_amd.nnet.summary_mixing import SummaryMixing
from tests._util import describe as _d

BF = torch.bfloat16
B, T, D = 4, 48, 64                  # 192 frames: a shape smx_pool_bcast accepts; 48 = 6 chunks of 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_routes.json")


_EPI_DEFAULTS = {"c0_mode": L.C0_NONE, "c0_div": 0, "act": L.ACT_NONE, "out_mode": L.OUT_T, "alpha": 1.0, "bias_batch_stride": 0,
                 "c0_post": False, "drop_cols": 0}


class Record(list):
    """One string per launch / seed draw / collective; `seeds` counts the dropout seeds drawn so far (drive() starts it at 0)."""
    seeds = 0


def install(monkeypatch):
    """Put the recorders in place; returns the Record they write."""
    out = Record()

    def note(name, *a, **k):
        out.append(" ".join([name] + [_d(x) for x in a] + [f"{n}={_d(x)}" for n, x in sorted(k.items())]))

    def seed():
        out.seeds += 1
        out.append(f"seed {out.seeds}")
        return out.seeds

    def epilogue(**kw):
        return {k: v for k, v in kw.items() if v is not None and _EPI_DEFAULTS.get(k, None) != v}

    def gemm(layout, a, b, c, N, M, K, e=None, **kw):
        note("gemm", ("NT", "NN", "TN")[layout], a, b, c, N, M, K, e or {}, **kw)
        return c

    def masked_mean(s, mask, B_, T_, scale=True, want_inv=False):
        note("masked_mean", s, mask, B_, T_, scale=scale, want_inv=want_inv)
        return torch.zeros((B_, s.shape[1])), (torch.ones(B_) if want_inv else None)

    def pool_bcast(s, mask_in, B_, T_, ds=None, scale=True, want_mean=True, want_inv=False, **k):
        note("pool_bcast", s, mask_in, B_, T_, ds=ds, scale=scale, want_mean=want_mean, want_inv=want_inv, **k)
        return (torch.zeros((B_, s.shape[1])) if want_mean else None), (torch.ones(B_) if want_inv else None)

    def act_mask_bwd(dy, z, mask, act, alpha=1.0, dz=None, *a, **k):
        note("act_mask_bwd", dy, z, mask, act, alpha, dz, *a, **k)
        return dz

    def dropout(x, p, s, out=None):
        note("dropout", x, p, s, out=out)
        return out if out is not None else torch.empty_like(x)

    def cast(src, dtype):
        if src.dtype != dtype:
            note("cast", src, dtype)
        return src.to(dtype)

    def axpby(a, x, b=0.0, y0=None, out=None):
        note("axpby", a, x, b, y0, out=out)
        return out if out is not None else torch.empty(x.shape, dtype=x.dtype)

    def chunk_mean(s, out, B_, T_, chunk, left, reverse=False):
        note("chunk_mean", s, out, B_, T_, chunk, left, reverse=reverse)
        return out

    def expdecay_mean(s, out, B_, T_, decay, reverse=False):
        note("expdecay_mean", s, out, B_, T_, decay, reverse=reverse)
        return out

    def writes(name, iout):
        """A wrapper whose argument number `iout` is the output it returns."""
        def f(*a, **k):
            note(name, *a, **k)
            return a[iout]
        return f

    monkeypatch.setattr(ops, "new_dropout_seed", seed)
    monkeypatch.setattr(ops, "epilogue", epilogue)
    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "gemm_panel", lambda a, wp, c, N, M, K, e=None: note("gemm_panel", a, c, N, M, K, e or {}))
    monkeypatch.setattr(ops, "gemm_panel_slabs", lambda a, wp, s, N, M, ks, ns: note("gemm_panel_slabs", a, s, N, M, ks, ns))
    monkeypatch.setattr(ops, "slab_epilogue", lambda s, ns, c, N, M, e: note("slab_epilogue", s, ns, c, N, M, e))
    monkeypatch.setattr(ops, "wgrad", lambda *a, **k: note("wgrad", *a, **k))
    monkeypatch.setattr(ops, "act_mask_bwd", act_mask_bwd)
    monkeypatch.setattr(ops, "masked_mean", masked_mean)
    monkeypatch.setattr(ops, "pool_bcast", pool_bcast)
    monkeypatch.setattr(ops, "bcast_rows", writes("bcast_rows", 2))
    monkeypatch.setattr(ops, "bcast_rows_act_bwd", writes("bcast_rows_act_bwd", 2))
    monkeypatch.setattr(ops, "chunk_mean", chunk_mean)
    monkeypatch.setattr(ops, "expdecay_mean", expdecay_mean)
    monkeypatch.setattr(ops, "stream_summary", writes("stream_summary", 1))
    monkeypatch.setattr(ops, "slot_summary", writes("slot_summary", 1))
    monkeypatch.setattr(ops, "chunk_mean_sharded", lambda *a, **k: note("chunk_mean_sharded", *a, **k))
    monkeypatch.setattr(ops, "expdecay_mean_sharded", lambda *a, **k: note("expdecay_mean_sharded", *a, **k))
    monkeypatch.setattr(ops, "dropout", dropout)
    monkeypatch.setattr(ops, "cast", cast)
    monkeypatch.setattr(ops, "axpby", axpby)
    monkeypatch.setattr(F, "wcast", lambda p, dtype: p.detach().to(dtype))       # (weight shadows are cached: not part of the sequence)
    monkeypatch.setattr(F, "wpacked", lambda *a, **k: None)
    monkeypatch.setattr(F, "_wgrad", lambda dz, x, gW, N, M, K, dbias: note("_wgrad", dz, x, gW, N, M, K, dbias))
    monkeypatch.setattr(F, "defer", lambda *a, **k: None)
    monkeypatch.setattr(F, "deferred_ws", lambda *a, **k: torch.empty(16, dtype=torch.uint8))
    monkeypatch.setattr(F, "_LN_FUSE_MIN_ROWS", 17500)
    monkeypatch.setattr(F, "_POOL_FUSE", True)
    monkeypatch.setattr(F, "_WGRAD_BIAS", True)
    monkeypatch.setattr(SP, "all_reduce_sum", lambda t: (note("all_reduce_sum", t), t)[1] if SP.enabled() else t)
    monkeypatch.setattr(SP, "all_gather", lambda t: (note("all_gather", t), [t.clone() for _ in range(SP.world())])[1])
    return out


@pytest.fixture
def rec(monkeypatch):
    return install(monkeypatch)


def enter_seqpar(monkeypatch):
    """Rank 1 of a sequence group of 3 (the collectives are the recorder's stubs)."""
    monkeypatch.setattr(SP._State, "active", True)
    monkeypatch.setattr(SP._State, "world", 3)
    monkeypatch.setattr(SP._State, "rank", 1)


@pytest.fixture
def seqpar(monkeypatch):
    enter_seqpar(monkeypatch)


def _cell(mode, nhead=1, act="gelu"):
    torch.manual_seed(0)
    return SummaryMixing(D, nhead, [D], D, [D], D, activation=act, global_dropout=0.1, mode=mode)


def _sum_mask(kind):
    if kind == "chunk":
        return F.DynChunkMask(T, 8, 2)
    if kind == "chunk_all":
        return F.DynChunkMask(T, 8, None)
    if kind == "dense":
        return F.DynChunkMask(T, 8, 1).dense()
    if kind == "stream":
        return F.DynChunkStream(torch.zeros(B, 2, D), torch.zeros(1, dtype=torch.int64), 8, 2)
    if kind == "slots":
        return F.DynChunkSlots(torch.zeros(B, 2, D), torch.zeros(B, dtype=torch.int64), torch.full((B,), 8, dtype=torch.int32), 8, 2)
    assert kind is None
    return None


def drive(rec, mode, sm=None, p=0.0, need_bwd=True, pad=True, dz_in=False, branch=False, ln_next=False, ln=False, res=False,
          pool_fuse=True, nhead=1, dtype=BF, t=T):
    """One forward (and backward) of the cell; returns (forward launches, backward launches)."""
    m = _cell(mode, nhead)
    rec.seeds = 0
    F._POOL_FUSE = pool_fuse                                        # (the rec fixture restores it)
    mask = F.mask_u8(torch.arange(t)[None] < torch.tensor([t, t // 2, t, 5])[:, None], B, t, "cpu") if pad else None
    run = F.cell_run(m._params(), m._cfg(), B, t, mask, _sum_mask(sm) if isinstance(sm, (str, type(None))) else sm, p)
    x = torch.zeros((B, t, D), dtype=dtype)
    N = B * t
    kw = {}
    if res:
        kw["res"] = torch.zeros((N, D), dtype=torch.float32)
    if ln_next:
        kw["ln_next"] = (torch.ones(D), torch.zeros(D), 1e-5)
    if branch:                                                      # the Branchformer: the output dropped into a view of ITS merge input
        kw["out"], kw["out_drop"] = torch.empty((N, 2 * D), dtype=dtype)[:, :D], (0.2, 77)
    got = run(x, need_bwd, **kw)
    assert len(got) == (3 if ln_next else 2) and got[0].shape == (B, t, D)
    fwd = list(rec)
    rec.clear()
    if not need_bwd:
        assert got[1] is None
        return fwd, []
    bwd = got[1]
    bkw = {}
    if dz_in:
        bkw["dz_in"] = torch.zeros((N, D), dtype=dtype)
    if ln:
        assert bwd.can_fuse_ln and bwd.ln_reduce == 2 * D and bwd.ln_W.shape == (2 * D, D)
        w, b = torch.ones(D, requires_grad=True), torch.zeros(D, requires_grad=True)
        bkw["ln"] = {"x": torch.empty((N, D), dtype=dtype), "w": w, "b": b, "stats": torch.empty((N, 2)), "act": L.ACT_NONE,
                     "gw_param": w, "gb_param": b}
        bkw["ln_res"] = torch.zeros((N, D), dtype=dtype)
    dx = bwd(torch.zeros((B, t, D), dtype=dtype), **bkw)
    assert dx.shape == ((N, D) if ln else (B, t, D))
    back = list(rec)
    rec.clear()
    return fwd, back


# name -> drive() keywords.  Every case runs forward and backward unless need_bwd=False.
CASES = {}
for _mode in ("SummaryMixing", "SummaryMixing-fast", "SummaryMixing-expdecay"):
    for _sm in (None, "chunk", "chunk_all", "dense"):
        for _p in (0.0, 0.1):
            CASES[f"{_mode}|{_sm}|p{_p}"] = dict(mode=_mode, sm=_sm, p=_p)
for _p in (0.0, 0.1):
    CASES[f"SummaryMixing-lite|None|p{_p}"] = dict(mode="SummaryMixing-lite", p=_p)
CASES["SummaryMixing-lite|dense|res"] = dict(mode="SummaryMixing-lite", sm="dense", res=True)          # (lite ignores sum_mask)
for _mode in ("SummaryMixing", "SummaryMixing-fast"):
    CASES[f"{_mode}|None|p0.1|nofuse"] = dict(mode=_mode, p=0.1, pool_fuse=False)
    CASES[f"{_mode}|None|p0.1|dz_in"] = dict(mode=_mode, p=0.1, dz_in=True)
    CASES[f"{_mode}|None|p0|dz_in"] = dict(mode=_mode, dz_in=True)
    CASES[f"{_mode}|chunk|p0|dz_in"] = dict(mode=_mode, sm="chunk", dz_in=True)
    CASES[f"{_mode}|None|p0.1|branch"] = dict(mode=_mode, p=0.1, branch=True, res=True)
    CASES[f"{_mode}|None|p0|branch"] = dict(mode=_mode, branch=True, res=True)
    CASES[f"{_mode}|None|p0|nopad|ln_next"] = dict(mode=_mode, pad=False, ln_next=True, res=True)
    CASES[f"{_mode}|None|p0|f32"] = dict(mode=_mode, dtype=torch.float32)
    CASES[f"{_mode}|None|p0|inference"] = dict(mode=_mode, need_bwd=False)
    for _sm in ("stream", "slots"):
        CASES[f"{_mode}|{_sm}|inference"] = dict(mode=_mode, sm=_sm, need_bwd=False, t=8)
CASES["SummaryMixing-fast|None|p0|ln"] = dict(mode="SummaryMixing-fast", ln=True)
CASES["SummaryMixing-fast|None|p0.1|ln"] = dict(mode="SummaryMixing-fast", p=0.1, ln=True)
CASES["SummaryMixing|None|p0.1|heads4"] = dict(mode="SummaryMixing", p=0.1, nhead=4)                  # ParallelLinear projections
CASES["SummaryMixing|None|p0|heads4"] = dict(mode="SummaryMixing", nhead=4)
SP_CASES = {}
for _mode, _sm in (("SummaryMixing", None), ("SummaryMixing-fast", None), ("SummaryMixing-fast", "chunk"), ("SummaryMixing", "chunk_all"),
                   ("SummaryMixing-expdecay", None), ("SummaryMixing-lite", None)):
    for _p in (0.0, 0.1):
        SP_CASES[f"seqpar|{_mode}|{_sm}|p{_p}"] = dict(mode=_mode, sm=_sm, p=_p)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cell_launch_sequence(rec, name):
    fwd, bwd = drive(rec, **CASES[name])
    want = _golden()[name]
    assert fwd == want["fwd"]
    assert bwd == want["bwd"]


@pytest.mark.parametrize("name", sorted(SP_CASES))
def test_cell_launch_sequence_sequence_parallel(rec, seqpar, name):
    fwd, bwd = drive(rec, **SP_CASES[name])
    want = _golden()[name]
    assert fwd == want["fwd"]
    assert bwd == want["bwd"]


def _names(seq):
    return [s.split()[0] for s in seq]


def _only(seq, name):
    got = [s for s in seq if s.split()[0] == name]
    assert len(got) == 1, (name, seq)
    return got[0]


def test_golden_covers_exactly_the_cases():
    assert sorted(_golden()) == sorted(list(CASES) + list(SP_CASES))


@pytest.mark.parametrize("mode", ["SummaryMixing", "SummaryMixing-fast"])
def test_dropout_seeds_are_drawn_local_first(rec, mode):
    """s1 (the local half of the merge input) before s2 (the summary half) on every path: with the pool fused s2 is drawn in the
    summary phase, else in the merge phase; without a Linear to carry the local dropout both are drawn in the merge phase."""
    for kw in (dict(), dict(pool_fuse=False), dict(sm="chunk"), dict(sm="dense")):
        fwd, bwd = drive(rec, mode, p=0.1, **kw)
        assert [s for s in fwd if s.startswith("seed")] == ["seed 1", "seed 2"] and not any(s.startswith("seed") for s in bwd)
        # the projection that writes D(local) into cat carries seed 1; whatever fills the summary half carries seed 2
        first = [s for s in fwd if "drop=(0.1,1)" in s]
        assert len(first) == 1 and first[0].startswith("gemm NT") and fwd.index(first[0]) > fwd.index("seed 1")
        assert ("drop_cols=64" if mode == "SummaryMixing-fast" else f"bf16[{B * T}x{D}]/ld{2 * D} ") in first[0]
        fill = [s for s in fwd if s.split()[0] in ("pool_bcast", "bcast_rows", "dropout")]
        assert len(fill) == 1 and f"/ld{2 * D}+{D}" in fill[0] and ("(0.1,2)" in fill[0] or " 0.1 2 " in fill[0])
        # the backward's two merge dgrads regenerate them: local half with seed 1, summary half with seed 2
        halves = [s for s in bwd if s.startswith("gemm NN") and "drop=(0.1," in s]
        assert ["drop=(0.1,1)" in halves[0], "drop=(0.1,2)" in halves[1]] == [True, True] and len(halves) == 2
    fwd, _ = drive(rec, "SummaryMixing", p=0.1, nhead=4)             # ParallelLinear local projection: a dropout launch of its own
    i1, i2 = fwd.index("seed 1"), fwd.index("seed 2")
    assert i2 == i1 + 1 and fwd[i2 + 1].startswith("dropout") and " 0.1 1 " in fwd[i2 + 1]


def test_pool_fusion_writes_the_summary_half_of_cat(rec):
    for mode in ("SummaryMixing", "SummaryMixing-fast"):
        fwd, bwd = drive(rec, mode, p=0.1)
        assert "masked_mean" not in _names(fwd) and "bcast_rows" not in _names(fwd)
        pb = _only(fwd, "pool_bcast")
        assert f"ds=bf16[{B * T}x{D}]/ld{2 * D}+{D}" in pb and "drop=(0.1,2)" in pb and "want_inv=True" in pb and "want_mean=False" in pb
        assert fwd.index("seed 2") == fwd.index(pb) - 1
        # backward: sum over time + broadcast (+ the summary projection's act / mask backward) in one launch as well
        pb = _only(bwd, "pool_bcast")
        assert "inv_in=f32[" in pb and "scale=False" in pb and "z=bf16[" in pb and "masked_mean" not in _names(bwd)
        fwd, bwd = drive(rec, mode, p=0.1, pool_fuse=False)
        assert _names(fwd).count("masked_mean") == 1 and "pool_bcast" not in _names(fwd + bwd)
        assert "drop=(0.1,2)" in _only(fwd, "bcast_rows") and fwd.index("seed 2") > fwd.index(_only(fwd, "masked_mean"))
        assert _names(bwd).count("masked_mean") == 1 and _names(bwd).count("bcast_rows_act_bwd") == 1


def test_per_utterance_mean_rides_in_the_merge_as_a_side_input(rec):
    fwd, bwd = drive(rec, "SummaryMixing")
    merge = [s for s in fwd if s.startswith("gemm NT") and "c0=" in s]
    assert len(merge) == 1 and f"c0_mode={L.C0_GROUP}" in merge[0] and f"c0_div={T}" in merge[0] and f"c0=f32[{B}x{D}]" in merge[0]
    assert "dropout" not in _names(fwd) and "bcast_rows" not in _names(fwd)
    assert _names(bwd).count("masked_mean") == 1 and _names(bwd).count("bcast_rows_act_bwd") == 1
    fwd, bwd = drive(rec, "SummaryMixing", sm="chunk")
    merge = [s for s in fwd if s.startswith("gemm NT") and "c0=" in s]
    assert len(merge) == 1 and f"c0_mode={L.C0_ROW}" in merge[0] and f"c0=f32[{B * T}x{D}]" in merge[0]


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_frame_wise_summaries_run_their_kernel_once_each_way(rec, p):
    """One pooling launch forward, the transposed operator (reverse=True, as a keyword) once in the backward."""
    for mode in ("SummaryMixing", "SummaryMixing-fast"):
        for sm, left in (("chunk", 2), ("chunk_all", None)):
            fwd, bwd = drive(rec, mode, sm=sm, p=p)
            assert f"{B} {T} 8 {left} reverse=False" in _only(fwd, "chunk_mean")
            assert f"{B} {T} 8 {left} reverse=True" in _only(bwd, "chunk_mean")
            assert "masked_mean" not in _names(fwd + bwd) and "pool_bcast" not in _names(fwd + bwd)
        fwd, bwd = drive(rec, mode, sm="dense", p=p)
        pool = [s for s in fwd if s.startswith("gemm NN") and "batch=4" in s]
        assert len(pool) == 1 and f"bf16[{T}x{T}]" in pool[0] and "sa=0" in pool[0]
        pool = [s for s in bwd if s.startswith("gemm TN") and "batch=4" in s]
        assert len(pool) == 1 and f"bf16[{T}x{T}]" in pool[0]
    fwd, bwd = drive(rec, "SummaryMixing-expdecay", p=p)
    assert f"{B} {T} 0.995 reverse=False" in _only(fwd, "expdecay_mean")
    assert f"{B} {T} 0.995 reverse=True" in _only(bwd, "expdecay_mean")
    # expdecay with a sum_mask: the dense Laplace matrix
    fwd, bwd = drive(rec, "SummaryMixing-expdecay", sm="chunk", p=p)
    assert "expdecay_mean" not in _names(fwd + bwd) and "chunk_mean" not in _names(fwd + bwd)
    assert len([s for s in fwd if s.startswith("gemm NN") and "batch=4" in s]) == 1


def test_lite_ignores_the_sum_mask(rec):
    plain, _ = drive(rec, "SummaryMixing-lite")
    masked, bwd = drive(rec, "SummaryMixing-lite", sm="dense")
    assert plain == masked and _names(plain)[-1] == "cast" and _names(plain).count("masked_mean") == 1
    assert _names(bwd)[:2] == ["masked_mean", "bcast_rows"]
    fwd, _ = drive(rec, "SummaryMixing-lite", res=True)
    assert _names(fwd)[-2:] == ["bcast_rows", "axpby"]


@pytest.mark.parametrize("mode", ["SummaryMixing", "SummaryMixing-fast"])
def test_streaming_summaries_are_inference_only(rec, mode):
    fwd, _ = drive(rec, mode, sm="stream", need_bwd=False, t=8)
    assert f" {B} 8 8 2 f32[{B}x2x{D}] i64[1]" in _only(fwd, "stream_summary")
    fwd, _ = drive(rec, mode, sm="slots", need_bwd=False, t=8)
    assert f" {B} 8 2 f32[{B}x2x{D}] i64[{B}] i32[{B}]" in _only(fwd, "slot_summary")
    with pytest.raises(NotImplementedError, match="^streaming summary: inference of the SummaryMixing / SummaryMixing-fast modes only$"):
        drive(rec, mode, sm="stream", t=8)
    with pytest.raises(NotImplementedError,
                       match="^slot streaming summary: inference of the SummaryMixing / SummaryMixing-fast modes only$"):
        drive(rec, mode, sm="slots", t=8)


def test_sequence_parallel_summaries(rec, seqpar):
    """The three kinds the sequence-parallel mode supports: one collective per direction each; the dense kind is refused."""
    fwd, bwd = drive(rec, "SummaryMixing", p=0.1)
    assert _names(fwd).count("all_reduce_sum") == 1 and "pool_bcast" not in _names(fwd + bwd)      # (no small-batch fusion on a shard)
    assert "scale=False" in _only(fwd, "masked_mean") and _names(bwd).count("all_reduce_sum") == 1
    fwd, bwd = drive(rec, "SummaryMixing-fast", sm="chunk")
    for seq, rev in ((fwd, "False"), (bwd, "True")):
        assert [s.split()[0] for s in seq if "chunk_mean" in s or "all_" in s] == ["chunk_mean_sharded", "all_gather", "chunk_mean_sharded"]
        assert all(f" 8 2 {rev} 6 " in s for s in seq if s.startswith("chunk_mean_sharded"))        # rank 1 x 6 chunks per shard
    fwd, bwd = drive(rec, "SummaryMixing-expdecay")
    for seq, rev in ((fwd, "False"), (bwd, "True")):
        assert [s.split()[0] for s in seq if "expdecay" in s or "all_" in s] == ["expdecay_mean_sharded", "all_gather", "expdecay_mean_sharded"]
        assert all(f" {rev} {T} {3 * T} " in s for s in seq if s.startswith("expdecay_mean_sharded"))
    for mode in ("SummaryMixing", "SummaryMixing-fast"):
        with pytest.raises(NotImplementedError, match="sequence-parallel mode supports the per-utterance mean, the Dynamic Chunk Training "
                                                      r"mask and the mask-free expdecay summary \(no dense sum_mask\)"):
            drive(rec, mode, sm="dense")


def test_backward_contract(rec):
    """What the callers read off the closures."""
    m = _cell("SummaryMixing-fast")
    run = F.cell_run(m._params(), m._cfg(), B, T, None, None, 0.0)
    y3, bwd = run(torch.zeros((B, T, D), dtype=BF), True)
    assert bwd.can_fuse_ln and bwd.ln_reduce == 2 * D and bwd.pre[3].shape == (B * T, D) and bwd.pre[4] == m.act
    y3, bwd, post = run(torch.zeros((B, T, D), dtype=BF), True, ln_next=(torch.ones(D), torch.zeros(D), 1e-5))
    assert post is None                                            # (192 rows: below the LayerNorm-fusion threshold)
    m = _cell("SummaryMixing")
    y3, bwd = F.cell_run(m._params(), m._cfg(), B, T, None, None, 0.0)(torch.zeros((B, T, D), dtype=BF), True)
    assert not bwd.can_fuse_ln and not hasattr(bwd, "ln_W")


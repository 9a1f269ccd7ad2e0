"""Kernel-level parity of the two sequence-parallel summaries (smx_expdecay_mean_sharded, smx_chunk_mean_sharded and the host
folds around their one all-gather: functional._expdecay_seqpar, functional._chunk_mean_seqpar) against the dense float64
operator on the WHOLE (B, W*T, D) sequence.

No process group: the arithmetic is deterministic, so a world of W ranks is emulated in one process.  The product's own
functions run once per rank with sequence_parallel._State set to (active, W, r) and sequence_parallel.all_gather replaced:
a first sweep over the ranks records what each rank contributes to the gather (phase 1 does not depend on what the gather
returns), a second sweep returns the recorded list, and only its outputs are compared.  Nothing of the fold is restated here.

The shapes are the ones tests/test_seqpar_gpu.py (48 frames x 2 ranks until this module came) never reached: frames per rank
that are not a multiple of the scan's 16-row chunk (pad 1, 8, 9, 15), worlds with middle ranks (3, 4, 8), D that is not one full
lane group, strided rows (the second half of a (N, 2D) buffer), B = 1, bf16.  Bars: the ones the unsharded kernels are held to
in test_kernels_gpu.py (relative max error 1e-5 float32, 1e-2 bfloat16)."""
import ctypes

import pytest
import torch

from tests._util import rel_err

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
DTYPES = [torch.float32, torch.bfloat16]
SENTINEL = 777.0


def _mods():
    from summarymixing_amd import _lib as L, functional as F, ops, sequence_parallel as SP
    return L, F, ops, SP


def _views(full, W, T, strided):
    """The ranks' (B*T, D) row views of a (B, W*T, D) sequence and matching output views.  strided: each is the second half of a
    (B*T, 2D) buffer (ld = 2D) whose first half holds a sentinel.  -> (xs, outs, bufs)"""
    B, _, D = full.shape
    xs, outs, bufs = [], [], []
    for r in range(W):
        rows = full[:, r * T:(r + 1) * T].reshape(B * T, D)
        if strided:
            xb = torch.full((B * T, 2 * D), SENTINEL, device=full.device, dtype=full.dtype)
            ob = torch.full((B * T, 2 * D), SENTINEL, device=full.device, dtype=full.dtype)
            xb[:, D:] = rows
            xs.append(xb[:, D:])
            outs.append(ob[:, D:])
            bufs.append(ob)
        else:
            xs.append(rows.contiguous())
            outs.append(torch.full((B * T, D), SENTINEL, device=full.device, dtype=full.dtype))
    return xs, outs, bufs


def _emulate(monkeypatch, W, call):
    """Run call(r) for every rank of an emulated world of W, twice: sweep 1 records each rank's all-gather contributions (in
    call order), sweep 2 hands every rank the recorded lists and checks that the rank contributes the same bits again."""
    _, _, _, SP = _mods()
    monkeypatch.setattr(SP._State, "active", True)
    monkeypatch.setattr(SP._State, "world", W)
    rec = [[] for _ in range(W)]                 # rec[r][k]: rank r's k-th contribution
    for r in range(W):
        monkeypatch.setattr(SP._State, "rank", r)

        def record(t, r=r):
            rec[r].append(t.detach().clone())
            return [t.detach().clone() if q == r else torch.zeros_like(t) for q in range(W)]
        monkeypatch.setattr(SP, "all_gather", record)
        call(r)
    assert len({len(c) for c in rec}) == 1, "the ranks disagree on the number of exchanges"
    for r in range(W):
        monkeypatch.setattr(SP._State, "rank", r)
        k = [0]

        def replay(t, r=r, k=k):
            assert torch.equal(t, rec[r][k[0]]), "phase 1 is not deterministic"
            got = [rec[q][k[0]].clone() for q in range(W)]
            k[0] += 1
            return got
        monkeypatch.setattr(SP, "all_gather", replay)
        call(r)


def _gather_out(outs, B, T, D):
    return torch.cat([o.reshape(B, T, D) for o in outs], dim=1)


def _check_untouched(bufs, D):
    for ob in bufs:
        assert bool((ob[:, :D] == SENTINEL).all()), "the kernel wrote outside its (rows, D) view"


def _laplace(Tg, decay):
    idx = torch.arange(Tg, device="cuda")
    M = torch.pow(torch.tensor(decay, dtype=torch.float64, device="cuda"), (idx[None] - idx[:, None]).abs().double())
    return M / M.sum(1, keepdim=True)


def _run_expdecay(monkeypatch, full, W, T, decay, reverse, strided=False):
    _, F, _, _ = _mods()
    B, _, D = full.shape
    xs, outs, bufs = _views(full, W, T, strided)
    _emulate(monkeypatch, W, lambda r: F._expdecay_seqpar(xs[r], outs[r], B, T, decay, reverse=reverse))
    _check_untouched(bufs, D)
    return _gather_out(outs, B, T, D)


def _run_chunk(monkeypatch, full, W, T, chunk, left, reverse, strided=False):
    _, F, _, _ = _mods()
    B, _, D = full.shape
    xs, outs, bufs = _views(full, W, T, strided)
    _emulate(monkeypatch, W, lambda r: F._chunk_mean_seqpar(xs[r], outs[r], B, T, chunk, left, reverse=reverse))
    _check_untouched(bufs, D)
    return _gather_out(outs, B, T, D)


# frames per rank T (pad to the 16-row scan chunk: 1 -> 15, 15 -> 1, 16 -> 0, 17 -> 15, 40 -> 8, 47 -> 1, 48 -> 0, 375 -> 9,
# 1000 -> 8), ranks W, decay, D, B, strided.  W * T <= 4096.
ED_CASES = [
    (1, 2, 0.9, 4, 1, False),
    (1, 8, 0.9, 64, 3, True),
    (15, 3, 0.9, 8, 3, False),
    (15, 4, 0.995, 260, 1, True),
    (16, 2, 0.9, 64, 3, False),
    (16, 8, 0.995, 256, 1, True),
    (17, 8, 0.9, 64, 3, False),
    (17, 3, 0.995, 512, 1, True),
    (40, 2, 0.9, 64, 3, False),
    (40, 3, 0.995, 260, 3, True),
    (40, 4, 0.9, 8, 1, False),
    (47, 3, 0.9, 64, 3, False),
    (47, 2, 0.995, 4, 3, True),
    (47, 8, 0.9, 256, 1, True),
    (48, 2, 0.9, 64, 3, False),
    (48, 4, 0.995, 512, 3, True),
    (375, 4, 0.995, 256, 3, False),
    (375, 8, 0.995, 64, 1, True),
    (375, 3, 0.9, 260, 1, False),
    (1000, 2, 0.995, 64, 3, False),
    (1000, 4, 0.995, 256, 1, True),
    (1000, 3, 0.9, 8, 3, True),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("T,W,decay,D,B,strided", ED_CASES)
def test_expdecay_sharded_matches_dense_laplace(monkeypatch, T, W, decay, D, B, strided, dtype):
    """functional._expdecay_seqpar over W emulated ranks of T frames == the dense float64 Laplace operator on the W*T frames
    (summary_mixing.py:316-365, 233-235), forward (M s)/rowsum(M) and the transposed operator M (s/rowsum(M)).
    A state entering from the right that is not compensated for the zero padding of the shard's last 16-row chunk (the arithmetic
    this test was written against) misses these bars by orders of magnitude wherever T % 16 != 0: DESIGN.md has the figures."""
    torch.manual_seed(T * 131 + W * 17 + D)
    full = torch.randn(B, W * T, D, device="cuda").to(dtype)
    Wn = _laplace(W * T, decay)
    s3 = full.double()
    fwd = _run_expdecay(monkeypatch, full, W, T, decay, False, strided)
    e_f = rel_err(fwd, torch.einsum("ij,bjd->bid", Wn, s3))
    bwd = _run_expdecay(monkeypatch, full, W, T, decay, True, strided)
    e_b = rel_err(bwd, torch.einsum("ji,bjd->bid", Wn, s3))
    print(f"expdecay sharded T={T} W={W} decay={decay} D={D} B={B} strided={strided} {dtype}: fwd {e_f:.3e} bwd {e_b:.3e}")
    assert e_f <= TOL[dtype], f"forward rel err {e_f:.3e}"
    assert e_b <= TOL[dtype], f"transposed rel err {e_b:.3e}"


# frames per rank T (a multiple of chunk), chunk, left, ranks W, D, B, strided.  W * T <= 4096.
CH_CASES = [
    (4, 4, None, 2, 8, 1, False),          # exactly one chunk per rank
    (4, 4, 1, 8, 64, 3, True),             # one chunk per rank, left == T / chunk
    (8, 8, 0, 3, 48, 3, False),
    (24, 24, None, 4, 264, 1, True),       # one chunk per rank: every window is carry + one row
    (24, 24, 1, 3, 256, 3, False),
    (16, 8, 2, 3, 48, 3, True),            # left == T / chunk
    (24, 8, 3, 4, 64, 1, False),           # left == T / chunk
    (36, 12, 3, 8, 264, 3, True),          # left == T / chunk
    (48, 8, 2, 2, 64, 3, False),           # the geometry of test_seqpar_gpu.py
    (40, 8, 2, 3, 64, 3, False),
    (40, 8, None, 3, 256, 1, True),
    (40, 4, 3, 4, 8, 3, False),
    (48, 12, 1, 3, 48, 1, True),
    (48, 24, 2, 8, 64, 3, False),          # left == T / chunk
    (96, 24, None, 8, 264, 3, True),
    (96, 12, 0, 4, 256, 1, False),
    (120, 24, 3, 2, 48, 3, True),
    (512, 8, None, 8, 64, 1, False),
    (500, 4, 1, 4, 8, 3, True),
    (360, 12, None, 2, 256, 3, False),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("T,chunk,left,W,D,B,strided", CH_CASES)
def test_chunk_mean_sharded_matches_dense_mask(monkeypatch, T, chunk, left, W, D, B, strided, dtype):
    """functional._chunk_mean_seqpar over W emulated ranks of T frames == the dense float64 DynChunk mask on the W*T frames
    (summary_mixing.py:224-235 with the mask of TransformerASR.py:85-110), forward and the transposed operator."""
    _, F, _, _ = _mods()
    torch.manual_seed(T * 131 + W * 17 + D + chunk)
    full = torch.randn(B, W * T, D, device="cuda").to(dtype)
    Mx = F.DynChunkMask(W * T, chunk, left).dense("cuda").double()
    s3 = full.double()
    fwd = _run_chunk(monkeypatch, full, W, T, chunk, left, False, strided)
    e_f = rel_err(fwd, (Mx @ s3) / Mx.sum(1)[None, :, None])
    bwd = _run_chunk(monkeypatch, full, W, T, chunk, left, True, strided)
    e_b = rel_err(bwd, (Mx / Mx.sum(1)[:, None]).t() @ s3)
    print(f"chunk sharded T={T} chunk={chunk} left={left} W={W} D={D} B={B} strided={strided} {dtype}: fwd {e_f:.3e} bwd {e_b:.3e}")
    assert e_f <= TOL[dtype], f"forward rel err {e_f:.3e}"
    assert e_b <= TOL[dtype], f"transposed rel err {e_b:.3e}"


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("W", [3, 4])
def test_expdecay_states_hop_over_middle_ranks(monkeypatch, W, reverse):
    """(a) The states are exchanged at the right place: with W >= 3, rank 0's output moves when ONLY the last rank's input
    changes, and rank W-1's when only rank 0's does, by what the dense operator says (decay 0.995, 40 frames per rank: the far
    shard arrives with weights of 0.995^40 = 0.82 and below, far above the bar).  A fold without its decay^T hop passes the
    wrong weight on and fails here."""
    torch.manual_seed(W)
    B, T, D, decay = 3, 40, 64, 0.995
    full = torch.randn(B, W * T, D, device="cuda")
    Wn = _laplace(W * T, decay)
    op = "ji,bjd->bid" if reverse else "ij,bjd->bid"
    base = _run_expdecay(monkeypatch, full, W, T, decay, reverse)
    for src, dst in ((W - 1, 0), (0, W - 1)):
        moved = full.clone()
        moved[:, src * T:(src + 1) * T] += torch.randn(B, T, D, device="cuda")
        out = _run_expdecay(monkeypatch, moved, W, T, decay, reverse)
        sl = slice(dst * T, (dst + 1) * T)
        delta = (out - base)[:, sl]
        ref0, ref1 = torch.einsum(op, Wn, full.double()), torch.einsum(op, Wn, moved.double())
        delta_ref = (ref1 - ref0)[:, sl]
        assert float(delta_ref.abs().max()) > 1e-2            # the far shard is visible at all
        assert float(delta.abs().max()) > 1e-2, f"rank {dst} does not see rank {src}"
        # the difference of two float32 results, each within the 1e-5 bar of its own maximum
        bar = 1e-5 * float(ref0.abs().max() + ref1.abs().max()) / float(delta_ref.abs().max())
        assert bar < 1e-2 and rel_err(delta, delta_ref) <= bar, f"rank {dst} sees rank {src} with the wrong weight"


def test_chunk_mean_seqpar_refusals(monkeypatch):
    """(b) Shards that do not hold whole chunks and a left context that reaches beyond the neighbouring shard stay refusals."""
    _, F, _, SP = _mods()
    monkeypatch.setattr(SP._State, "active", True)
    monkeypatch.setattr(SP._State, "world", 2)
    monkeypatch.setattr(SP._State, "rank", 0)
    monkeypatch.setattr(SP, "all_gather", lambda t: pytest.fail("a refused shape reached the exchange"))
    B, D = 2, 8
    x = torch.randn(B * 20, D, device="cuda")
    with pytest.raises(ValueError):
        F._chunk_mean_seqpar(x, torch.empty_like(x), B, 20, 8, 1)
    x = torch.randn(B * 16, D, device="cuda")
    with pytest.raises(NotImplementedError):
        F._chunk_mean_seqpar(x, torch.empty_like(x), B, 16, 8, 3)


def test_expdecay_sharded_entry_refusals():
    """(b) smx_expdecay_mean_sharded returns SMX_EINVAL (-1) and writes nothing for D % 4 != 0, decay outside (0, 1) and a
    shard that ends beyond the sequence (T_glob < t_off + T)."""
    L, _, ops, _ = _mods()
    B, T, Da = 2, 16, 8                                  # (buffers are allocated for D = 8 whatever D is passed)
    fn = L.lib().smx_expdecay_mean_sharded

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def rc(D, decay, t_off, T_glob, phase=1):
        x = torch.randn(B * T, Da, device="cuda")
        out = torch.full_like(x, SENTINEL)
        ends = torch.full((2, B, Da), SENTINEL, device="cuda")
        ws = torch.empty(L.lib().smx_expdecay_mean_workspace(B, T, Da) // 4 + 4, device="cuda")
        code = fn(ops.dt(x), p(x), Da, p(out), Da, B, T, D, decay, 0, t_off, T_glob, phase, p(ends), p(ws), None)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and (code == 0 or bool((ends == SENTINEL).all()))
        return code
    assert rc(8, 0.9, 0, 32) == 0                       # the accepted call, for contrast
    assert rc(6, 0.9, 0, 32) == -1
    assert rc(6, 0.9, 0, 32, phase=2) == -1
    assert rc(8, 0.0, 0, 32) == -1
    assert rc(8, 1.0, 0, 32) == -1
    assert rc(8, -0.5, 0, 32) == -1
    assert rc(8, 1.5, 0, 32) == -1
    assert rc(8, 0.9, 17, 32) == -1                     # T_glob < t_off + T
    assert rc(8, 0.9, 16, 32) == 0                      # the last shard, exactly to the end
    assert rc(8, 0.9, 0, 15) == -1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_sharded_summaries_are_bit_reproducible(monkeypatch, dtype):
    """(c) Fixed-order reductions: the same call twice gives the same bits (both summaries, both directions, a padded shard,
    a middle rank)."""
    torch.manual_seed(9)
    B, W, D = 3, 3, 260
    full = torch.randn(B, W * 40, D, device="cuda").to(dtype)
    for reverse in (False, True):
        a = _run_expdecay(monkeypatch, full, W, 40, 0.995, reverse, True)
        b = _run_expdecay(monkeypatch, full, W, 40, 0.995, reverse, True)
        assert torch.equal(a, b)
        for left in (None, 2):
            a = _run_chunk(monkeypatch, full[..., :256], W, 40, 8, left, reverse, False)
            b = _run_chunk(monkeypatch, full[..., :256], W, 40, 8, left, reverse, False)
            assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_expdecay_one_shard_equals_unsharded(monkeypatch, dtype):
    """The two-phase sharded entry over ONE shard that is the whole sequence (zero entering states) gives the bits of the
    unsharded smx_expdecay_mean_fwd / _bwd, padded last chunk or not: compensating the pad leaves a zero state zero."""
    _, _, ops, _ = _mods()
    torch.manual_seed(3)
    B, D = 3, 64
    for T in (40, 48):
        full = torch.randn(B, T, D, device="cuda").to(dtype)
        for reverse in (False, True):
            got = _run_expdecay(monkeypatch, full, 1, T, 0.9, reverse)
            want = torch.empty(B * T, D, device="cuda", dtype=dtype)
            ops.expdecay_mean(full.reshape(B * T, D), want, B, T, 0.9, reverse=reverse)
            assert torch.equal(got, want.view(B, T, D))

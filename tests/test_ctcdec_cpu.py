"""CPU checks of CTC greedy decoding: the float64 restatement of tests/_ctcdec_ref.py against upstream's groupby + filter, chunked
against whole through the state, the admissibility of the cases the GPU tests decode token-exactly, and what the library and the
Python surface decide without a GPU.  No GPU."""
import ctypes

import pytest
import torch

from summarymixing_amd.decoders import ctc as C
from tests import _ctcdec_ref as R


def _strings():
    g = torch.Generator().manual_seed(7)
    out = [([], 0), ([0, 0, 0, 0], 0), ([3], 0), ([3], 3), ([2, 2, 0, 2, 2], 0), ([1, 0, 0, 1, 1, 2, 0], 0), ([4, 4, 4], 4)]
    for _ in range(200):
        V = int(torch.randint(2, 6, (), generator=g))
        T = int(torch.randint(0, 40, (), generator=g))
        out.append(([int(k) for k in torch.randint(0, V, (T,), generator=g)], int(torch.randint(0, V, (), generator=g))))
    return out


def test_restatement_equals_groupby_then_filter():
    filter_ctc_output = C.filter_ctc_output
    assert C.NO_TOKEN == R.NO_TOKEN == -2 ** 31
    for s, blank in _strings():
        want = R.brute_force(s, blank)
        got = R.collapse([s], [[0.0] * len(s)], blank)
        assert got["hyps"][0] == want, (s, blank)
        assert got["state"]["n_tok"][0] == len(want) and got["state"]["seen"][0] == len(s)
        assert all(s[f] == k for k, f in zip(got["hyps"][0], got["frames"][0]))
        assert filter_ctc_output(list(s), blank_id=blank) == want
    assert R.collapse([[1, 1, 0, 1]], [[0.0] * 4], 0)["hyps"] == [[1, 1]]
    assert R.collapse([[1, -1, 1, -1, -1, 2]], [[0.0] * 6], 0)["hyps"] == [[1, 1, 2]]      # a -1 emits nothing and separates
    with pytest.raises(ValueError):
        filter_ctc_output((1, 2), blank_id=0)


def test_chunked_equals_whole_for_every_split_point():
    s = [[2, 2, 0, 2, 2, 1, 1, 0, 0, 3, 3, 3, 0, 1], [0, 0, 1, 1, 1, 0, 2, 0, 2, 2, 3, 0, 0, 0]]
    lp = [[-0.25 * (i + 1) for i in range(14)], [-0.125 * (i + 3) for i in range(14)]]
    whole = R.collapse(s, lp, 0)
    for cut in range(15):
        a = R.collapse([r[:cut] for r in s], [r[:cut] for r in lp], 0)
        b = R.collapse([r[cut:] for r in s], [r[cut:] for r in lp], 0, state=a["state"])
        assert [x + y for x, y in zip(a["hyps"], b["hyps"])] == whole["hyps"], cut
        assert [x + y for x, y in zip(a["frames"], b["frames"])] == whole["frames"], cut
        assert b["state"] == whole["state"], cut           # (the lp are dyadic: the float64 sums are exact)
    # lengths, an empty call and a restart
    cutl = R.collapse(s, lp, 0, in_len=[14, 5])
    assert cutl["hyps"][0] == whole["hyps"][0] and cutl["hyps"][1] == R.brute_force(s[1][:5], 0) and cutl["state"]["seen"] == [14, 5]
    idle = R.collapse(s, lp, 0, in_len=[0, 0], state=whole["state"])
    assert idle["state"] == whole["state"] and idle["hyps"] == [[], []]
    again = R.collapse(s, lp, 0, state=whole["state"], start=[1, 0])
    assert again["hyps"][0] == whole["hyps"][0] and again["state"]["seen"] == [14, 28]


def test_best_path_restatement():
    x = torch.tensor([[0.0, 1.0, 1.0, -2.0], [float("nan")] * 4, [float("nan"), -1.0, -3.0, -1.0], [5.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    tok, lp = R.best_path(x)
    assert tok.tolist() == [1, -1, 1, 0]
    assert torch.isnan(lp[1]) and torch.isnan(lp[2])
    want = torch.log_softmax(x[[0, 3]], -1).max(-1).values
    assert float((lp[[0, 3]] - want).abs().max()) < 1e-14
    # log-softmax input and raw logits: the same tokens, and lp of log-probabilities is the maximum itself
    z = torch.randn(50, 37, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    t1, l1 = R.best_path(z)
    t2, l2 = R.best_path(torch.log_softmax(z, -1))
    assert torch.equal(t1, t2) and float((l1 - l2).abs().max()) < 1e-12
    assert float((l2 - torch.log_softmax(z, -1).max(-1).values).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.HEAD_CASES))
def test_head_cases_are_admissible(name, dtype):
    """What the token-exact GPU tests rely on, asserted on the float64 logits and a CPU emulation alone: the top-2 gap of every row
    is >= 8 x the largest deviation of the emulated logits (fp32 operands, or bf16 operands with fp32 accumulation; and, for the
    unfused pair, the same logits stored in the operand dtype).  The lp floor of the case table is the emulation's."""
    c = R.head_case(name, dtype)
    top2 = c["z64"].topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    dev = float((c["emu"].double() - c["z64"]).abs().max())
    dev_stored = float((c["emu_stored"].double() - c["z64"]).abs().max())
    assert gap >= 8 * dev, (gap, dev)
    assert gap >= 8 * dev_stored, (gap, dev_stored)
    tok64, lp64 = R.best_path(c["z64"])
    assert torch.equal(c["emu"].argmax(1), tok64) and torch.equal(c["emu_stored"].argmax(1), tok64)
    N, K, V, _, kind, _, floor32, floor16 = R.HEAD_CASES[name]
    if kind == "negative":
        assert float(c["z64"].max()) < 0 and V % 128 != 0
    if kind == "last_tile":
        assert int(tok64.min()) >= 128 * ((V - 1) // 128) and V % 128 != 0
    if V > 2:
        assert len(set(tok64.tolist())) > 10                  # many different winners, not one column
    lp_emu = torch.log_softmax(c["emu"], -1).max(-1).values
    measured = R.lp_rel(lp_emu, lp64)
    floor = floor32 if dtype == torch.float32 else floor16
    assert measured <= floor <= max(4 * measured, 1e-6), (measured, floor)


def test_head_shape_rule_and_workspace_need_no_gpu():
    from summarymixing_amd import _lib
    L = _lib.lib()
    ok = L.smx_ctc_head_ok
    assert ok(_lib.BF16, 512, 5000) == 1 and ok(_lib.F32, 640, 1000) == 1 and ok(_lib.F32, 64, 2) == 1 and ok(_lib.BF16, 128, 129) == 1
    assert ok(_lib.F32, 96, 100) == 0 and ok(_lib.F32, 32, 100) == 0 and ok(_lib.F32, 0, 100) == 0 and ok(_lib.F32, 64, 1) == 0
    assert ok(5, 64, 100) == 0
    assert L.smx_ctc_head_workspace(111, 300) == 111 * 3 * 12 and L.smx_ctc_head_workspace(128, 128) == 128 * 12
    assert L.smx_ctc_head_workspace(1, 129) == 2 * 12 and L.smx_ctc_head_workspace(0, 300) == 0
    # refused on the host, before any launch (the pointers are fake and never dereferenced)
    base = 1 << 40
    assert L.smx_ctc_head_best_path(_lib.F32, base, 96, base, None, 8, 96, 100, base, base, base, None) == -2
    assert b"multiple of 64" in L.smx_last_error()
    assert L.smx_ctc_head_best_path(_lib.F32, base + 4, 64, base, None, 8, 64, 100, base, base, base, None) == -2
    assert L.smx_ctc_head_best_path(_lib.BF16, base, 68, base, None, 8, 64, 100, base, base, base, None) == -2   # ldx: 136 bytes


def test_route_planner_holds_its_measured_cells():
    """greedy_decode_from_encoder's route at the measured points (profiles/ctcdec_bench.jsonl, ctcdec_bench_crossover.jsonl): bf16
    fused at all of them; fp32 fused up to 6016 rows at V = 1000 and up to 500 rows at V = 5000."""
    pts = [(128 * 125, 512, 5000), (16 * 125, 512, 5000), (8 * 94, 640, 1000), (64 * 94, 640, 1000), (8 * 125, 512, 5000), (4 * 125, 512, 5000)]
    assert [C._plan_fused(*p, torch.bfloat16) for p in pts] == [True] * 6
    assert [C._plan_fused(*p, torch.float32) for p in pts] == [False, False, True, True, False, True]
    assert not C._plan_fused(100, 512, 8000, torch.float32)      # a wider head in fp32: unmeasured, the unfused pair


def test_entry_points_refuse_bad_arguments_on_the_host():
    from summarymixing_amd import _lib
    L = _lib.lib()
    base = 1 << 40
    assert L.smx_ctc_best_path(_lib.F32, None, 8, 4, 8, base, base, None) == -1
    assert L.smx_ctc_best_path(_lib.F32, base, 7, 4, 8, base, base, None) == -1          # ldx < V
    assert L.smx_ctc_best_path(3, base, 8, 4, 8, base, base, None) == -1
    assert L.smx_ctc_head_best_path(_lib.F32, base, 32, base, None, 8, 64, 100, base, base, base, None) == -1   # ldx < K
    assert ctypes.sizeof(_lib.CtcCollapse) == 104 and _lib.CtcCollapse.B.offset == 88 and _lib.CtcCollapse.cap.offset == 100
    a = _lib.CtcCollapse(tok=base, lp=base, ld=4, prev=base, seen=base, n_tok=base, score=base, tokens=base, frames=base, B=2, T=8, blank=0, cap=8)
    assert L.smx_ctc_collapse(ctypes.byref(a), None) == -1                               # ld < T
    a.ld, a.blank = 8, -1
    assert L.smx_ctc_collapse(ctypes.byref(a), None) == -1
    a.blank, a.prev = 0, None
    assert L.smx_ctc_collapse(ctypes.byref(a), None) == -1


def test_surface_needs_a_gpu_tensor_and_exports_upstream_names():
    import summarymixing_amd.decoders as D
    from summarymixing_amd.nnet.linear import Linear
    for n in ("ctc_greedy_decode", "filter_ctc_output", "greedy_decode", "greedy_decode_from_encoder", "CapturedCTCGreedy"):
        assert n in D.__all__ and hasattr(D, n)
    with pytest.raises(RuntimeError, match="GPU only"):
        D.greedy_decode(torch.randn(2, 5, 7))
    with pytest.raises(RuntimeError, match="GPU only"):
        D.ctc_greedy_decode(torch.randn(2, 5, 7), torch.ones(2))
    with pytest.raises(RuntimeError, match="GPU only"):
        D.greedy_decode_from_encoder(torch.randn(2, 5, 64), Linear(7, input_size=64))
    with pytest.raises(RuntimeError, match="GPU only"):
        D.CapturedCTCGreedy(2, 5, 7, device="cpu")

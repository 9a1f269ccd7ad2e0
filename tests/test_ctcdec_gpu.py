"""GPU tests of CTC greedy decoding (csrc/ctcdec.hip, summarymixing_amd/decoders/ctc.py) against the float64 restatement of
tests/_ctcdec_ref.py, piece by piece: the row pass on stored scores, the fused head, the collapse on token arrays built on the host,
streaming through the state, the Python surface and the captured form.  Tokens, frames and counts are exact everywhere; the fused
head's exact cases are the ones tests/test_ctcdec_cpu.py proves admissible.  lp and scores: max |x - ref| / max(1, max |ref|) against
float64 within max(TOL[dtype], 4 x the case's emulation floor)."""
import functools

import pytest
import torch

from summarymixing_amd.decoders import ctc as _ctc_module
from tests import _ctcdec_ref as R
from tests._util import TOL

pytestmark = pytest.mark.gpu

DT_IDS = ["f32", "bf16"]
B0, T0 = 3, 37                       # N = 111 rows: no multiple of 4 (rows per workgroup), 64 or 128


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ctc():
    return _ctc_module


def _bar(dtype, floor=0.0):
    return max(TOL[dtype][0], 4 * floor)


# ---------------------------------------------------------------------------------------------------------------------- row pass
@functools.lru_cache(maxsize=None)
def _scores(V, dtype):
    g = torch.Generator().manual_seed(100 + V)
    x = (3.0 * torch.randn(B0 * T0, V, generator=g)).to(dtype)
    tok, lp = R.best_path(x.double())
    return x, tok, lp


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("V", [2, 127, 128, 129, 300])
def test_row_pass_dense_and_strided(V, dtype):
    from summarymixing_amd import ops
    x, tok_ref, lp_ref = _scores(V, dtype)
    dense = x.cuda()
    wide = torch.full((B0 * T0, V + 5), 1e4, dtype=dtype, device="cuda")         # ldx = V + 5: most rows are not 16-byte aligned
    wide[:, :V] = dense
    for xin in (dense, wide[:, :V]):
        tok, lp = ops.ctc_best_path(xin)
        assert tok.dtype == torch.int32 and torch.equal(tok.cpu().long(), tok_ref)
        err = R.lp_rel(lp.cpu(), lp_ref)
        print(f"row pass V={V} {dtype}: lp err {err:.3g}")
        assert err <= _bar(dtype)
    t1, l1 = ops.ctc_best_path(dense)
    t2, l2 = ops.ctc_best_path(wide[:, :V])
    assert torch.equal(t1, t2) and _same_bits(l1, l2)                            # vector and element loads: the same bits


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
def test_row_pass_tie_nan_and_log_softmax(dtype):
    from summarymixing_amd import ops
    V = 300
    x = _scores(V, dtype)[0].clone()
    x[5, 17] = x[5, 263] = 40.0                     # a planted tie across two lanes' groups: the lower index
    x[6, 299] = x[6, 298] = 41.0                    # and inside the element tail / last group
    x[9, :] = float("nan")                          # a row of only NaNs
    x[11, 3] = float("nan")                         # a NaN beside numbers never wins; the row's lp is a NaN
    x[11, 200] = 50.0
    tok_ref, lp_ref = R.best_path(x.double())
    assert tok_ref[5] == 17 and tok_ref[6] == 298 and tok_ref[9] == -1 and tok_ref[11] == 200
    tok, lp = ops.ctc_best_path(x.cuda())
    tok, lp = tok.cpu().long(), lp.cpu()
    assert torch.equal(tok, tok_ref)
    assert torch.equal(torch.isnan(lp), torch.isnan(lp_ref)) and bool(torch.isnan(lp[9])) and bool(torch.isnan(lp[11]))
    fin = ~torch.isnan(lp_ref)
    assert R.lp_rel(lp[fin], lp_ref[fin]) <= _bar(dtype)                         # the neighbours of the NaN rows are untouched
    # raw logits and their log-softmax: the same tokens (fp32: the shift moves no comparison at these gaps)
    z = _scores(129, torch.float32)[0]
    z = z + 40.0 * torch.nn.functional.one_hot(torch.arange(z.shape[0]) % 129, 129)     # a clear winner per row
    ta, la = ops.ctc_best_path(z.cuda())
    tb, lb = ops.ctc_best_path(torch.log_softmax(z.double(), -1).float().cuda())
    assert torch.equal(ta, tb) and torch.equal(ta.cpu().long(), torch.arange(z.shape[0]) % 129)
    assert float((la - lb).abs().max()) <= 1e-5 and float((lb.cpu() - torch.log_softmax(z.double(), -1).max(-1).values).abs().max()) <= 1e-5


# -------------------------------------------------------------------------------------------------------------------- fused head
@functools.lru_cache(maxsize=None)
def _head(name, dtype):
    c = R.head_case(name, dtype)
    tok, lp = R.best_path(c["z64"])
    return c, tok, lp


def _linear(c, dtype):
    from summarymixing_amd.nnet.linear import Linear
    V, K = c["W"].shape
    lin = Linear(V, input_size=K, bias=c["bias"] is not None)
    with torch.no_grad():
        lin.w.weight.copy_(c["W"])
        if c["bias"] is not None:
            lin.w.bias.copy_(c["bias"])
    return lin.cuda()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", sorted(R.HEAD_CASES))
def test_fused_head_tokens_exact_and_lp(name, dtype):
    from summarymixing_amd import ops
    c, tok_ref, lp_ref = _head(name, dtype)
    N, K, V = R.HEAD_CASES[name][:3]
    floor = R.HEAD_CASES[name][6 if dtype == torch.float32 else 7]
    assert ops.ctc_head_ok(dtype, K, V)
    X, W = c["X"].to(dtype).cuda(), c["W"].to(dtype).cuda()
    bias = c["bias"].cuda() if c["bias"] is not None else None
    tok, lp = ops.ctc_head_best_path(X, W, bias)
    assert torch.equal(tok.cpu().long(), tok_ref)
    err = R.lp_rel(lp.cpu(), lp_ref)
    print(f"fused head {name} {dtype}: lp err {err:.3g} (floor {floor:.3g})")
    assert err <= _bar(dtype, floor)
    tok2, lp2 = ops.ctc_head_best_path(X, W, bias)
    assert torch.equal(tok, tok2) and _same_bits(lp, lp2)                        # two runs: the same bits
    # a strided X (ldx = K + 8 elements: still 16-byte aligned rows)
    wide = torch.zeros((N, K + 8), dtype=dtype, device="cuda")
    wide[:, :K] = X
    tok3, lp3 = ops.ctc_head_best_path(wide[:, :K], W, bias)
    assert torch.equal(tok, tok3) and _same_bits(lp, lp3)
    # the unfused pair (this package's Linear, then the row pass over the stored logits) agrees on the tokens
    ctc = _ctc()
    lin = _linear(c, dtype)
    x3 = X.view(B0, T0, K)
    tu, lu = ctc._head_pass(x3, lin, False)
    tf, lf = ctc._head_pass(x3, lin, True)
    assert torch.equal(tu.reshape(-1).cpu().long(), tok_ref) and torch.equal(tf.reshape(-1), tok) and _same_bits(lf.reshape(-1), lp)
    if dtype == torch.float32:                      # (bf16: the stored logits carry their own rounding; only the tokens are compared)
        assert R.lp_rel(lu.reshape(-1).cpu(), lp_ref) <= _bar(dtype, floor)


def test_from_encoder_falls_back_where_the_head_is_refused():
    from summarymixing_amd import ops
    from summarymixing_amd.nnet.linear import Linear
    ctc = _ctc()
    torch.manual_seed(5)
    K, V = 96, 50                                   # K % 64 != 0: smx_ctc_head_ok refuses, the unfused pair runs
    assert not ops.ctc_head_ok(torch.float32, K, V)
    lin = Linear(V, input_size=K).cuda()
    x = torch.randn(2, 9, K, device="cuda")
    a = ctc.greedy_decode_from_encoder(x, lin, fused=True)
    with torch.no_grad():
        b = ctc.greedy_decode(lin(x))
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.counts, b.counts) and _same_bits(a.scores, b.scores)


def test_from_encoder_default_route_is_the_planned_one():
    ctc = _ctc()
    c, tok_ref, _ = _head("k64_v129", torch.float32)
    lin = _linear(c, torch.float32)
    x = c["X"].view(B0, T0, -1).cuda()
    planned = ctc._plan_fused(B0 * T0, 64, 129, torch.float32)
    a, b = ctc.greedy_decode_from_encoder(x, lin, blank=0), ctc.greedy_decode_from_encoder(x, lin, blank=0, fused=planned)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.counts, b.counts) and _same_bits(a.scores, b.scores)
    ref = R.collapse(tok_ref.view(B0, T0).tolist(), [[0.0] * T0] * B0, 0)
    assert a.counts.cpu().tolist() == ref["state"]["n_tok"]
    assert [a.tokens[i, :n].cpu().tolist() for i, n in enumerate(ref["state"]["n_tok"])] == ref["hyps"]


# ---------------------------------------------------------------------------------------------------------------------- collapse
VC = 6


def _lp_rows(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return -torch.rand(B, T, generator=g) * 3.0


def _run_collapse(rows, lp, blank, in_len=None, state=None, start=None, out=None):
    ctc = _ctc()
    tok = torch.tensor(rows, dtype=torch.int32).reshape(len(rows), -1).cuda()
    il = torch.tensor(in_len, dtype=torch.int32).cuda() if in_len is not None else None
    st = torch.tensor(start, dtype=torch.bool).cuda() if start is not None else None
    return ctc._collapse(tok, lp.cuda(), il, blank, state, st, out)


def _check_against_ref(r, ref, cap=None):
    B = len(ref["state"]["n_tok"])
    cap = r.tokens.shape[1] if cap is None else cap
    assert r.counts.cpu().tolist() == ref["state"]["n_tok"]
    assert r.state.prev.cpu().tolist() == ref["state"]["prev"] and r.state.frames_seen.cpu().tolist() == ref["state"]["seen"]
    tokens, frames = r.tokens.cpu().tolist(), r.frames.cpu().tolist()
    for b in range(B):
        n = min(ref["state"]["n_tok"][b], cap)
        assert tokens[b][:n] == ref["all_hyps"][b][:n] and frames[b][:n] == ref["all_frames"][b][:n], b
        assert all(v == -1 for v in tokens[b][n:]) and all(v == -1 for v in frames[b][n:]), b


def _ref(rows, lp, blank, **kw):
    ref = R.collapse(rows, lp.tolist(), blank, **kw)
    ref["all_hyps"], ref["all_frames"] = ref["hyps"], ref["frames"]
    return ref


@pytest.mark.parametrize("blank_id", [0, -1, 3])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_collapse_matches_restatement(T, blank_id):
    ctc = _ctc()
    blank = ctc._blank(blank_id, VC)
    assert blank == (VC - 1 if blank_id == -1 else blank_id)
    B = 5
    rows = R.token_rows(B, T, VC, blank, seed=10 * T + blank)
    lp = _lp_rows(B, T, T)
    for in_len in (None, [0, 1, T, T // 2, max(T - 1, 0)]):
        ref = _ref(rows, lp, blank, in_len=in_len)
        r = _run_collapse(rows, lp, blank, in_len=in_len)
        _check_against_ref(r, ref)
        r2 = _run_collapse(rows, lp, blank, in_len=in_len)
        assert _same_bits(r.scores, r2.scores)
        err = R.lp_rel(r.scores.cpu(), torch.tensor(ref["state"]["score"], dtype=torch.float64))
        print(f"collapse T={T} blank={blank}: score err {err:.3g}")
        assert err <= _bar(torch.float32)
    if T > 64:      # the run over frames 62..65 is one emission at frame 62
        full = _ref(rows, lp, blank)
        assert all(f.count(62) == 1 and not any(t in f for t in (63, 64, 65)) for f in full["frames"])


def test_collapse_minus_one_emits_nothing_and_separates():
    rows = [[1, -1, 1, -1, -1, 2, 2, -1], [-1, -1, 0, 3, 3, -1, 3, 0]]
    lp = _lp_rows(2, 8, 3)
    ref = _ref(rows, lp, 0)
    assert ref["hyps"] == [[1, 1, 2], [3, 3]]
    _check_against_ref(_run_collapse(rows, lp, 0), ref)


def test_collapse_capacity_overflow_keeps_the_prefix_and_the_guard():
    ctc = _ctc()
    B, T, cap, guard = 3, 130, 5, 64
    rows = R.token_rows(B, T, VC, 0, seed=77)
    lp = _lp_rows(B, T, 9)
    ref = _ref(rows, lp, 0)
    assert min(ref["state"]["n_tok"]) > cap
    flat_t = torch.full((B * cap + guard,), 7777, dtype=torch.int32, device="cuda")
    flat_f = torch.full((B * cap + guard,), 7777, dtype=torch.int32, device="cuda")
    out = (flat_t[:B * cap].view(B, cap), flat_f[:B * cap].view(B, cap))
    r = _run_collapse(rows, lp, 0, out=out, state=ctc.start_state(B, "cuda"))
    _check_against_ref(r, ref, cap=cap)              # every row holds its own prefix: no row ran into the next
    assert r.counts.cpu().tolist() == ref["state"]["n_tok"]                      # the count goes beyond cap
    assert bool((flat_t[B * cap:] == 7777).all()) and bool((flat_f[B * cap:] == 7777).all())


# --------------------------------------------------------------------------------------------------------------------- streaming
def _stream_rows():
    B, T = 4, 130
    rows = R.token_rows(B, T, VC, 0, seed=31)
    for r in rows:
        r[40] = 0                                   # a blank at frame 40 in every row: a split at 41 falls after a blank
    return rows, _lp_rows(B, T, 4)


@pytest.mark.parametrize("cut", [1, 64, 63, 41, 129], ids=["1|T-1", "64|rest", "between equal tokens", "after a blank", "T-1|1"])
def test_chunked_equals_whole_bit_for_bit(cut):
    ctc = _ctc()
    rows, lp = _stream_rows()
    B, T = len(rows), len(rows[0])
    assert rows[0][62] == rows[0][63] and rows[0][40] == 0
    whole = _run_collapse(rows, lp, 0, state=ctc.start_state(B, "cuda"), out=ctc.new_output(B, T, "cuda"))
    _check_against_ref(whole, _ref(rows, lp, 0))
    out = ctc.new_output(B, T, "cuda")
    a = _run_collapse([r[:cut] for r in rows], lp[:, :cut].contiguous(), 0, state=ctc.start_state(B, "cuda"), out=out)
    b = _run_collapse([r[cut:] for r in rows], lp[:, cut:].contiguous(), 0, state=a.state, out=out)
    assert torch.equal(b.tokens, whole.tokens) and torch.equal(b.frames, whole.frames) and torch.equal(b.counts, whole.counts)
    assert _same_bits(b.scores, whole.scores)
    assert all(_same_bits(x, y) for x, y in zip(b.state, whole.state))


def test_streaming_with_per_row_lengths_and_start():
    ctc = _ctc()
    rows, lp = _stream_rows()
    B, cut = len(rows), 70
    r1, r2 = [r[:cut] for r in rows], [r[cut:] for r in rows]
    l1, l2 = lp[:, :cut].contiguous(), lp[:, cut:].contiguous()
    len1, len2 = [cut, 5, 0, cut], [60, 3, 7, 0]
    ref1 = R.collapse(r1, l1.tolist(), 0, in_len=len1)
    ref2 = R.collapse(r2, l2.tolist(), 0, in_len=len2, state=ref1["state"])
    ref2["all_hyps"] = [x + y for x, y in zip(ref1["hyps"], ref2["hyps"])]
    ref2["all_frames"] = [x + y for x, y in zip(ref1["frames"], ref2["frames"])]
    out = ctc.new_output(B, 130, "cuda")
    a = _run_collapse(r1, l1, 0, in_len=len1, state=ctc.start_state(B, "cuda"), out=out)
    kept = [t.clone() for t in a.state]
    b = _run_collapse(r2, l2, 0, in_len=len2, state=a.state, out=out)
    assert all(torch.equal(x, y) for x, y in zip(kept, a.state))                 # decoded on a copy: the caller's state is as it was
    _check_against_ref(b, ref2)
    assert R.lp_rel(b.scores.cpu(), torch.tensor(ref2["state"]["score"], dtype=torch.float64)) <= _bar(torch.float32)
    assert _same_bits(b.state.score[3], a.state.score[3]) and int(b.state.prev[3]) == int(a.state.prev[3])   # in_len 0: untouched
    # start resets exactly the flagged rows: they decode the second chunk as a fresh stream, the others go on
    start = [1, 0, 1, 0]
    ref3 = R.collapse(r2, l2.tolist(), 0, in_len=len2, state=ref1["state"], start=start)
    ref3["all_hyps"] = [y if s else x + y for s, x, y in zip(start, ref1["hyps"], ref3["hyps"])]
    ref3["all_frames"] = [y if s else x + y for s, x, y in zip(start, ref1["frames"], ref3["frames"])]
    out = ctc.new_output(B, 130, "cuda")
    a = _run_collapse(r1, l1, 0, in_len=len1, state=ctc.start_state(B, "cuda"), out=out)
    c = _run_collapse(r2, l2, 0, in_len=len2, state=a.state, start=start, out=out)
    _check_against_ref(c, ref3)
    fresh = _run_collapse(r2, l2, 0, in_len=len2)
    for b_ in (0, 2):
        assert _same_bits(c.scores[b_], fresh.scores[b_]) and int(c.state.frames_seen[b_]) == len2[b_]
    for b_ in (1, 3):
        assert _same_bits(c.scores[b_], b.scores[b_])


# ----------------------------------------------------------------------------------------------------------------------- surface
def _peaky(B, T, V, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    path = torch.tensor(R.token_rows(B, T, V, V - 1, seed))
    z = torch.randn(B, T, V, generator=g) + 6.0 * torch.nn.functional.one_hot(path, V)
    return torch.log_softmax(z, -1).to(dtype)


def test_ctc_greedy_decode_returns_upstreams_lists():
    ctc = _ctc()
    B, T, V = 4, 37, 11
    p = _peaky(B, T, V, 21)
    rel = torch.tensor([1.0, 0.5, 0.26, 0.0])                                    # 0.5 x 37 = 18.5 rounds to 18 (half to even)
    n = [int(torch.round(r * T)) for r in rel]
    assert n == [37, 18, 10, 0]
    path = p.argmax(-1)
    want = [R.brute_force(path[b, :n[b]].tolist(), V - 1) for b in range(B)]
    got = ctc.ctc_greedy_decode(p.cuda(), rel.cuda())                            # blank_id = -1: the last index
    assert got == want and all(isinstance(k, int) for h in got for k in h)
    assert ctc.ctc_greedy_decode(p.cuda(), rel, blank_id=V - 1) == want          # lengths on the host are moved
    want0 = [R.brute_force(path[b, :n[b]].tolist(), 0) for b in range(B)]
    assert ctc.ctc_greedy_decode(p.cuda().bfloat16(), rel.cuda(), blank_id=0) == [R.brute_force(p.bfloat16().argmax(-1)[b, :n[b]].tolist(), 0) for b in range(B)]
    assert ctc.ctc_greedy_decode(p.cuda(), rel.cuda(), blank_id=0) == want0
    assert ctc.filter_ctc_output(path[0].tolist(), blank_id=V - 1) == want[0]


def test_greedy_decode_state_is_copied_and_cpu_raises():
    ctc = _ctc()
    B, T, V = 3, 37, 11
    p = _peaky(B, T, V, 22).cuda()
    a = ctc.greedy_decode(p[:, :20], blank=-1)
    kept = [t.clone() for t in a.state]
    n_before = a.counts.clone()
    b = ctc.greedy_decode(p[:, 20:], blank=-1, state=a.state, out=(a.tokens, a.frames))
    assert all(torch.equal(x, y) for x, y in zip(kept, a.state)) and torch.equal(a.counts, n_before)
    whole = ctc.greedy_decode(p, blank=-1)
    nmax = int(whole.counts.max())
    assert nmax <= 20, "the first chunk's buffers hold the whole hypothesis in this case"
    assert torch.equal(b.counts, whole.counts) and torch.equal(b.tokens[:, :nmax], whole.tokens[:, :nmax])
    assert torch.equal(b.frames[:, :nmax], whole.frames[:, :nmax]) and _same_bits(b.scores, whole.scores)
    with pytest.raises(ValueError, match="out="):
        ctc.greedy_decode(p[:, 20:], blank=-1, state=a.state)
    with pytest.raises(RuntimeError, match="GPU only"):
        ctc.greedy_decode(p.cpu())
    with pytest.raises(ValueError):
        ctc.greedy_decode(p, blank=V)


# ----------------------------------------------------------------------------------------------------------------------- capture
def _equal_results(a, b):
    return (torch.equal(a.tokens, b.tokens) and torch.equal(a.frames, b.frames) and torch.equal(a.counts, b.counts)
            and _same_bits(a.scores, b.scores) and all(_same_bits(x, y) for x, y in zip(a.state, b.state)))


def test_captured_decode_equals_eager_on_fresh_inputs():
    ctc = _ctc()
    B, T, V = 3, 37, 129
    cap = ctc.CapturedCTCGreedy(B, T, V, dtype=torch.float32, blank=-1)
    for seed, lens in ((41, None), (42, torch.tensor([1.0, 0.5, 0.3]))):
        p = _peaky(B, T, V, seed).cuda()
        eager = ctc.greedy_decode(p, lens, blank=-1)
        assert _equal_results(cap.decode(p, lens), eager)
    # a stream through the captured graph: two replays, the second goes on from the first's state
    p = _peaky(B, 2 * T, V, 43).cuda()
    whole = ctc.greedy_decode(p, blank=-1)
    a = cap.decode(p[:, :T].contiguous())
    st = ctc.CTCGreedyState(*(t.clone() for t in a.state))
    b = cap.decode(p[:, T:].contiguous(), state=st)
    nmax = int(whole.counts.max())
    assert nmax <= T
    assert torch.equal(b.counts, whole.counts) and torch.equal(b.tokens[:, :nmax], whole.tokens[:, :nmax]) and _same_bits(b.scores, whole.scores)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_captured_decode_from_encoder_equals_eager(fused):
    ctc = _ctc()
    c, _, _ = _head("k64_v129", torch.float32)
    lin = _linear(c, torch.float32)
    K = c["X"].shape[1]
    cap = ctc.CapturedCTCGreedy(B0, T0, K, dtype=torch.float32, blank=0, lin=lin, fused=fused)
    for shift in (0, 1):
        x = c["X"].roll(shift, 0).view(B0, T0, K).cuda()
        eager = ctc.greedy_decode_from_encoder(x, lin, blank=0, fused=fused)
        assert _equal_results(cap.decode(x), eager)
        assert int(eager.counts.min()) > 0

"""The slot-streaming kernels on the GPU: smx_slot_summary and smx_dwconv1d_glu_slots driven by random per-slot counters, valid and
start against float64 references (NaN in every input row a slot does not own), slots that sit out leave their state bit-for-bit,
full equal-counter steps give the bits of the lockstep kernels, and smx_slot_begin's positional rows."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu


def _schedule(rng, B, C, steps):
    """Per step: valid (B,) and start (B,) for B slots running streams of random length, with pauses and restarts."""
    left_frames = [0] * B                              # frames still to come of each slot's stream (0: no open stream)
    out = []
    for _ in range(steps):
        valid, start = [], []
        for b in range(B):
            s = False
            if left_frames[b] == 0 and rng.random() < 0.6:
                left_frames[b], s = rng.randint(1, 6 * C), True
            if left_frames[b] > 0 and (s or rng.random() < 0.8):
                v = min(C, left_frames[b])
                left_frames[b] -= v
                if v < C:
                    left_frames[b] = 0
            else:
                v = 0
            valid.append(v)
            start.append(s)
        out.append((valid, start))
    return out


def _bits_equal(a, b):
    it = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _dev(valid, start):
    return (torch.tensor(valid, dtype=torch.int32, device="cuda"), torch.tensor(start, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("left", [0, 2, None])
@pytest.mark.parametrize("C", [1, 8, 16])
def test_slot_summary_against_float64(C, left, dtype):
    from summarymixing_amd import ops
    rng = random.Random(C * 10 + (left or 7))
    torch.manual_seed(C * 10 + (left or 7))
    B, D = 5, 144
    counters = torch.zeros(B, dtype=torch.int64, device="cuda")
    ring = torch.full((B, D) if left is None else (B, max(left, 1), D), float("nan"), device="cuda")   # (fresh state is never read)
    hist = [[] for _ in range(B)]                      # float64 chunks of each slot's current stream
    cnt = [0] * B
    for valid, start in _schedule(rng, B, C, 30):
        v_d, s_d = _dev(valid, start)
        ops.slot_begin(counters, s_d, None, None, B, C, D)
        S = torch.randn(B, C, D, device="cuda").to(dtype)
        for b in range(B):
            S[b, valid[b]:] = float("nan")
        out = torch.full((B * C, D), 7.0, device="cuda").to(dtype)
        ring_before = ring.clone()
        ops.slot_summary(S.view(B * C, D), out, B, C, left, ring, counters, v_d)
        ops.slot_advance(counters, v_d, B, C)
        o = out.view(B, C, D).double().cpu()
        for b in range(B):
            if start[b]:
                hist[b], cnt[b] = [], 0
            if valid[b] == 0:
                assert torch.equal(o[b], torch.full((C, D), 7.0, dtype=torch.float64))
                assert _bits_equal(ring[b], ring_before[b])
                continue
            c = len(hist[b])
            lo = 0 if left is None else max(0, c - left)
            rows = torch.cat([h for h in hist[b][lo:]] + [S[b, :valid[b]].double().cpu()], 0)
            ref = rows.mean(0)
            got = o[b, :valid[b]]
            if dtype == torch.float32:
                assert (got - ref).abs().max() <= 1e-5 * max(1.0, ref.abs().max()), (b, (got - ref).abs().max())
            else:
                assert ((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6).all(), (b, (got - ref).abs().max())
            assert torch.equal(o[b, valid[b]:], torch.full((C - valid[b], D), 7.0, dtype=torch.float64))
            hist[b].append(S[b, :valid[b]].double().cpu())
            cnt[b] += valid[b] == C
        assert counters.cpu().tolist() == cnt


def _conv_ref(X, w, bias, D, k, H):
    """GLU + depthwise conv of the chunk rows of X = [H rows before the chunk; the chunk] (pre-GLU, float64): tap j of frame t reads
    X-row t + j, zero at and beyond the chunk's end (Dynamic Chunk Convolution)."""
    u = X[:, :D] * torch.sigmoid(X[:, D:])
    R = u.shape[0]
    out = torch.empty(R - H, D, dtype=torch.float64)
    for t in range(R - H):
        win = u[t:min(R, t + k)]
        out[t] = (win * w[:, :win.shape[0]].T).sum(0) + bias
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,k", [(8, 31), (16, 15), (4, 31)])
def test_dwconv_slots_against_float64(C, k, dtype):
    from summarymixing_amd import ops
    rng = random.Random(C + k)
    torch.manual_seed(C + k)
    B, D = 4, 136
    H = (k - 1) // 2
    w = torch.randn(D, k, device="cuda") * 0.2
    bias = torch.randn(D, device="cuda") * 0.1
    counters = torch.zeros(B, dtype=torch.int64, device="cuda")
    state = torch.full((B, H, 2 * D), float("nan"), device="cuda").to(dtype)   # (never read at chunk 0)
    hist = [None] * B                                  # the pre-GLU rows of each slot's stream so far, float64
    w64, b64 = w.double().cpu(), bias.double().cpu()
    for valid, start in _schedule(rng, B, C, 30):
        v_d, s_d = _dev(valid, start)
        ops.slot_begin(counters, s_d, None, None, B, C, D)
        P = torch.randn(B, C, 2 * D, device="cuda").to(dtype)
        for b in range(B):
            P[b, valid[b]:] = float("nan")
        state_before = state.clone()
        y = ops.dwconv_slots(P.view(B * C, 2 * D), w, bias, state, v_d, counters, B, C, D, k).view(B, C, D)
        ops.slot_advance(counters, v_d, B, C)
        for b in range(B):
            if start[b]:
                hist[b] = torch.zeros(0, 2 * D, dtype=torch.float64)
            if valid[b] == 0:
                assert _bits_equal(state[b], state_before[b])
                continue
            rows = P[b, :valid[b]].double().cpu()
            hist[b] = torch.cat([hist[b], rows], 0)
            ctx_rows = hist[b][max(0, hist[b].shape[0] - valid[b] - H):]
            nlead = ctx_rows.shape[0] - valid[b]
            ref = _conv_ref(torch.cat([torch.zeros(H - nlead, 2 * D, dtype=torch.float64), ctx_rows], 0), w64, b64, D, k, H)
            got = y[b, :valid[b]].double().cpu()
            tol = 1e-5 if dtype == torch.float32 else 2e-2
            assert (got - ref).abs().max() <= tol * max(1.0, ref.abs().max()), (b, (got - ref).abs().max())


def test_idle_slots_leave_state_untouched_and_restart_needs_no_clear():
    """valid 0 writes nothing; a started slot reads its old state as zero (its garbage is never touched)."""
    from summarymixing_amd import ops
    B, C, D, k = 3, 8, 64, 31
    H = (k - 1) // 2
    w, bias = torch.randn(D, k, device="cuda"), torch.randn(D, device="cuda")
    state = torch.randn(B, H, 2 * D, device="cuda")
    ring = torch.randn(B, 2, D, device="cuda")
    counters = torch.tensor([3, 0, 5], dtype=torch.int64, device="cuda")
    s0, r0 = state.clone(), ring.clone()
    v_d, s_d = _dev([0, 0, 0], [False, True, False])
    P = torch.full((B * C, 2 * D), float("nan"), device="cuda")
    ops.slot_begin(counters, s_d, None, None, B, C, D)
    ops.dwconv_slots(P, w, bias, state, v_d, counters, B, C, D, k)
    ops.slot_summary(P[:, :D].contiguous(), torch.empty(B * C, D, device="cuda"), B, C, 2, ring, counters, v_d)
    ops.slot_advance(counters, v_d, B, C)
    assert torch.equal(state, s0) and torch.equal(ring, r0)
    assert counters.cpu().tolist() == [3, 0, 5]
    # slot 1 starts over a state full of garbage: equal to a slot whose state is zero
    P = torch.randn(B * C, 2 * D, device="cuda")
    v_d, s_d = _dev([8, 8, 8], [True, True, True])
    ops.slot_begin(counters, s_d, None, None, B, C, D)
    y = ops.dwconv_slots(P, w, bias, state, v_d, counters, B, C, D, k)
    z = torch.zeros(B, H, 2 * D, device="cuda")
    ref = ops.dwconv_stream(P, w, bias, z, B, C, D, k)
    assert torch.equal(y, ref) and torch.equal(state, z)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("left", [0, 2, None])
def test_full_equal_slots_are_bit_identical_to_lockstep(left, dtype):
    from summarymixing_amd import ops
    torch.manual_seed(11)
    B, C, D, k = 4, 16, 256, 31
    H = (k - 1) // 2
    w, bias = torch.randn(D, k, device="cuda") * 0.2, torch.randn(D, device="cuda")
    shape = (B, D) if left is None else (B, max(left, 1), D)
    ring_l, ring_s = torch.zeros(shape, device="cuda"), torch.full(shape, float("nan"), device="cuda")
    st_l = torch.zeros(B, H, 2 * D, device="cuda").to(dtype)
    st_s = torch.full((B, H, 2 * D), float("nan"), device="cuda").to(dtype)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    counters = torch.zeros(B, dtype=torch.int64, device="cuda")
    v_d = torch.full((B,), C, dtype=torch.int32, device="cuda")
    for step in range(6):
        s_d = torch.full((B,), 1 if step == 0 else 0, dtype=torch.uint8, device="cuda")
        S = torch.randn(B * C, D, device="cuda").to(dtype)
        P = torch.randn(B * C, 2 * D, device="cuda").to(dtype)
        out_l, out_s = torch.empty_like(S), torch.empty_like(S)
        ops.stream_summary(S, out_l, B, C, C, left, ring_l, counter)
        y_l = ops.dwconv_stream(P, w, bias, st_l, B, C, D, k)
        ops.step_counter_add(counter, 1)
        ops.slot_begin(counters, s_d, None, None, B, C, D)
        ops.slot_summary(S, out_s, B, C, left, ring_s, counters, v_d)
        y_s = ops.dwconv_slots(P, w, bias, st_s, v_d, counters, B, C, D, k)
        ops.slot_advance(counters, v_d, B, C)
        assert torch.equal(out_l, out_s) and torch.equal(y_l, y_s), step
        assert torch.equal(st_l, st_s)
    assert counters.cpu().tolist() == [6] * B and int(counter) == 6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_slot_begin_positional_rows(dtype):
    from summarymixing_amd import ops
    B, C, D, rows = 5, 16, 72, 100
    table = torch.randn(rows, D, device="cuda").to(dtype)
    counters = torch.tensor([0, 3, 6, 7, 2], dtype=torch.int64, device="cuda")   # slot 2 straddles the end, slot 3 is past it
    start = torch.tensor([0, 0, 0, 0, 1], dtype=torch.uint8, device="cuda")
    pe = torch.full((B * C, D), float("nan"), device="cuda").to(dtype)
    ops.slot_begin(counters, start, table, pe, B, C, D)
    assert counters.cpu().tolist() == [0, 3, 6, 7, 0]
    pe = pe.view(B, C, D).cpu()
    tc = table.cpu()
    for b, c in enumerate([0, 3, 6, 7, 0]):
        for r in range(C):
            row = c * C + r
            exp = tc[row] if row < rows else torch.zeros(D, dtype=dtype)
            assert torch.equal(pe[b, r], exp), (b, r)
    v_d = torch.tensor([16, 5, 0, 16, 16], dtype=torch.int32, device="cuda")
    ops.slot_advance(counters, v_d, B, C)
    assert counters.cpu().tolist() == [1, 3, 6, 8, 1]

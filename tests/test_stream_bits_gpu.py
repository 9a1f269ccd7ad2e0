"""The bits of the four streaming operators (ops.stream_summary, ops.slot_summary, ops.dwconv_stream, ops.dwconv_slots), pinned:
after every step of a short fixed schedule the SHA-256 of the raw bytes of the output and of the state (ring / conv state) must equal
tests/golden/stream_step_bits.json, case by case and step by step.  The float64 tests of these kernels allow a tolerance and would
not see a changed summation order; this one does.  Inputs are integer patterns (exact in bf16), no random generator; rows a slot does
not own are NaN.  `python tests/test_stream_bits_gpu.py --write <path>` writes the fixture (case names and hex digests only)."""
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_step_bits.json")
B, D = 3, 72                                             # two column blocks, the second 8 columns wide
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def _slot_schedule(C):
    """Six steps of (valid, start) for the 3 slots: a valid of 0, valids strictly between 0 and C, slots at different counters,
    restarts over non-zero leftover state (slot 2 at step 1, slot 0 at step 4), every slot fed at least four times."""
    return [([C, C, 2], [True, True, True]),
            ([C, 0, C], [False, False, True]),
            ([C, C, C], [False, False, False]),
            ([3, C, C], [False, False, False]),
            ([C, C, 0], [True, False, False]),
            ([C, 1, C], [False, False, False])]


def _pattern(rows, cols, row0, mul, mod, div, dtype, spread=False):
    """x[i, j] = ((mul[0] (row0 + i) + mul[1] j) % mod - mod // 2) / div, exact in bf16 for the values used.  spread: times
    2^((7 (row0 + i) + 5 j) % 29 - 14), still exact in bf16, so that a float32 sum of a column rounds and its order shows in the bits
    (the summary has no other rounding before its sum; the convolution has the sigmoid)."""
    i = torch.arange(row0, row0 + rows, dtype=torch.int64).view(-1, 1)
    j = torch.arange(cols, dtype=torch.int64).view(1, -1)
    x = ((mul[0] * i + mul[1] * j) % mod - mod // 2).double() / div
    if spread:
        x = x * torch.exp2(((7 * i + 5 * j) % 29 - 14).double())
    return x.to(dtype).cuda()


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _slot_inputs(C, cols, step, valid, dtype, spread=False):
    x = _pattern(B * C, cols, step * B * C, (37, 11), 61, 16, dtype, spread).view(B, C, cols)
    for b in range(B):
        x[b, valid[b]:] = NAN
    return x.view(B * C, cols)


def _host_counters(cnt, valid, start, C):
    """The slot protocol on the host: start -> counter 0 before the step; a full chunk advances the counter after it."""
    before = [0 if s else c for c, s in zip(cnt, start)]
    return before, [c + (v == C) for c, v in zip(before, valid)]


def _summary_lockstep(dtype, left):
    from summarymixing_amd import ops
    C = 5
    ring = torch.zeros((B, D) if left is None else (B, max(left, 1), D), device="cuda")
    row0 = 0
    for c, C_cur in enumerate([C, C, C, C, 3]):          # (left 2: the ring wraps and the window drops a chunk)
        s = _pattern(B * C_cur, D, row0, (37, 11), 61, 16, dtype, spread=True)
        row0 += B * C_cur
        out = torch.full((B * C_cur, D), 7.0, device="cuda").to(dtype)
        ops.stream_summary(s, out, B, C_cur, C, left, ring, torch.tensor([c], dtype=torch.int64, device="cuda"))
        yield out, ring


def _summary_slots(dtype, left):
    from summarymixing_amd import ops
    C = 5
    ring = torch.full((B, D) if left is None else (B, max(left, 1), D), NAN, device="cuda")   # (fresh state is never read)
    cnt = [9] * B
    for step, (valid, start) in enumerate(_slot_schedule(C)):
        before, cnt = _host_counters(cnt, valid, start, C)
        s = _slot_inputs(C, D, step, valid, dtype, spread=True)
        out = torch.full((B * C, D), 7.0, device="cuda").to(dtype)
        ops.slot_summary(s, out, B, C, left, ring, torch.tensor(before, dtype=torch.int64, device="cuda"),
                         torch.tensor(valid, dtype=torch.int32, device="cuda"))
        yield out, ring


def _taps(k):
    w = _pattern(D, k, 0, (13, 7), 41, 32, torch.float32)
    bias = _pattern(1, D, 0, (0, 5), 17, 8, torch.float32).view(D)
    return w, bias


def _dwconv_lockstep(dtype, k, C):
    from summarymixing_amd import ops
    w, bias = _taps(k)
    state = torch.zeros((B, (k - 1) // 2, 2 * D), dtype=dtype, device="cuda")
    row0 = 0
    for C_cur in [C, C, C, 3]:
        p = _pattern(B * C_cur, 2 * D, row0, (37, 11), 61, 16, dtype)
        row0 += B * C_cur
        yield ops.dwconv_stream(p, w, bias, state, B, C_cur, D, k), state


def _dwconv_slots(dtype, k, C):
    from summarymixing_amd import ops
    w, bias = _taps(k)
    state = torch.full((B, (k - 1) // 2, 2 * D), NAN, device="cuda").to(dtype)   # (never read at chunk 0)
    cnt = [9] * B
    for step, (valid, start) in enumerate(_slot_schedule(C)):
        before, cnt = _host_counters(cnt, valid, start, C)
        p = _slot_inputs(C, 2 * D, step, valid, dtype)
        y = ops.dwconv_slots(p, w, bias, state, torch.tensor(valid, dtype=torch.int32, device="cuda"),
                             torch.tensor(before, dtype=torch.int64, device="cuda"), B, C, D, k)
        # rows a slot does not own are torch.empty: only the owned rows are pinned
        yield torch.cat([y.view(B, C, D)[b, :valid[b]] for b in range(B)], 0), state


def _cases():
    cases = {}
    for dn, dtype in DTYPES.items():
        for left in (0, 2, None):
            cases[f"summary-lockstep-{dn}-left{left}"] = (_summary_lockstep, (dtype, left))
            cases[f"summary-slots-{dn}-left{left}"] = (_summary_slots, (dtype, left))
        for k, C in ((31, 4), (7, 8), (1, 4)):           # state shifts / chunk longer than the state / no state
            cases[f"dwconv-lockstep-{dn}-k{k}-C{C}"] = (_dwconv_lockstep, (dtype, k, C))
            cases[f"dwconv-slots-{dn}-k{k}-C{C}"] = (_dwconv_slots, (dtype, k, C))
    return cases


CASES = _cases()


def _run(name):
    fn, args = CASES[name]
    steps = []
    for out, state in fn(*args):
        assert torch.isfinite(out).all(), f"{name}, step {len(steps)}: the pinned output rows must be finite"
        steps.append([_digest(out), _digest(state)])
    return steps


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_bits_equal_the_fixture(name, golden):
    got, want = _run(name), golden[name]
    assert len(got) == len(want), f"{name}: {len(got)} steps, the fixture has {len(want)}"
    for step, (g, w_) in enumerate(zip(got, want)):
        assert g[0] == w_[0], f"{name}, step {step}: the output's bits differ from the fixture"
        assert g[1] == w_[1], f"{name}, step {step}: the state's bits differ from the fixture"


def test_fixture_has_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_stream_bits_gpu.py --write <path>")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(sys.argv[2], "w") as f:
        json.dump({name: _run(name) for name in sorted(CASES)}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(CASES)} cases to {sys.argv[2]}")

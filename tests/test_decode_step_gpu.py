"""TransformerASR.make_decode_state / decode_step: teacher-forced KV-cached steps against the prefix pass.

Each step's prediction is what decode(prefix)[0][:, -1] computes; it is compared with float64 (tests/_decoder_ref.decoder over the
prefix under the look-ahead mask, whose position p is the last position of the prefix of p + 1 tokens) under the project's bar: the
ATen chain (impl="aten", same dtype, whole prefix) is measured against float64 beside ours, ours <= 4 x ATen's (tests/_decoder_ref.judge),
keyed by position."""
import pytest
import torch

from tests import _s2s_models as M
from tests import _decoder_ref as DR

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
POSITIONS = (0, 1, 15, 16, 17, 63, 64, 65)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(M.MODELS))
def test_teacher_forced_steps_match_float64_within_aten_bar(name, dt):
    dtype = DT[dt]
    U = M.MODELS[name][5]
    m, lin, mem, enc_len = M.build(name, dtype, 3)
    tokens = torch.randint(1, M.V, (M.B, U), generator=torch.Generator().manual_seed(U))
    tk = tokens.cuda()
    before, w_before = m.decode(tk, mem, enc_len)
    state = m.make_decode_state(mem, enc_len, max_steps=U)
    assert state.cap == U and len(state.self_kv) == M.MODELS[name][3] and tuple(state.cross_kv[0].shape[:3]) == (M.B, M.S, 2)
    for kv in state.self_kv:
        kv.fill_(float("nan"))                                # slots at and beyond the position are never read
    steps = [m.decode_step(tk[:, u].contiguous(), state) for u in range(U)]
    assert steps[0].dtype == dtype and tuple(steps[0].shape) == (M.B, M.MODELS[name][0])
    assert state.pos.tolist() == [U] * M.B and state.done.tolist() == [0] * M.B
    ref = M.restated(name, m, lin, mem, "f64", dtype)(tokens)[0]
    aten = M.restated(name, m, lin, mem, "aten", dtype)(tokens)[0]
    pos = [p for p in POSITIONS if p < U]
    DR.judge(f"decode_step {name} {dt}", dtype, {f"pos {p}": steps[p] for p in pos}, {f"pos {p}": aten[:, p].float() for p in pos},
             {f"pos {p}": ref[:, p] for p in pos})
    # the existing prefix pass under the same bar, for the record (and it is left as it was: same bits before and after)
    DR.judge(f"decode (prefix pass) {name} {dt}", dtype, {f"pos {p}": before[:, p] for p in pos},
             {f"pos {p}": aten[:, p].float() for p in pos}, {f"pos {p}": ref[:, p] for p in pos})
    after, w_after = m.decode(tk, mem, enc_len)
    assert torch.equal(after, before) and torch.equal(w_after, w_before), "decode is untouched by decode_step"
    # one more step than the state holds: the row is marked done, not advanced, and nothing is read past the table or the caches
    m.decode_step(tk[:, 0].contiguous(), state)
    assert state.pos.tolist() == [U] * M.B and state.done.tolist() == [1] * M.B


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_two_states_step_interleaved_without_touching_each_other(dt):
    dtype = DT[dt]
    name, U = "d64-pre", 19
    m, lin, mem, enc_len = M.build(name, dtype, 4)
    g = torch.Generator().manual_seed(8)
    ta, tb = (torch.randint(1, M.V, (M.B, U), generator=g).cuda() for _ in range(2))
    mem_b = torch.randn(mem.shape, generator=g).to(dtype).cuda()
    alone_a = m.make_decode_state(mem, enc_len, max_steps=U)
    alone_b = m.make_decode_state(mem_b, None, max_steps=U)
    want_a = [m.decode_step(ta[:, u].contiguous(), alone_a) for u in range(U)]
    want_b = [m.decode_step(tb[:, u].contiguous(), alone_b) for u in range(U)]
    sa, sb = m.make_decode_state(mem, enc_len, max_steps=U), m.make_decode_state(mem_b, None, max_steps=U)
    got_a, got_b = [], []
    for u in range(U):                                        # a, b, b, a, a, b, ...
        for which in ((0, 1) if u % 2 == 0 else (1, 0)):
            if which == 0:
                got_a.append(m.decode_step(ta[:, u].contiguous(), sa))
            else:
                got_b.append(m.decode_step(tb[:, u].contiguous(), sb))
    for u in range(U):
        assert torch.equal(got_a[u], want_a[u]) and torch.equal(got_b[u], want_b[u]), u
    # a state refilled in place for the next utterance gives what a fresh one gives
    again = m.make_decode_state(mem_b, None, max_steps=U, state=sa)
    assert again is sa and sa.pos.tolist() == [0] * M.B
    for u in range(U):
        assert torch.equal(m.decode_step(tb[:, u].contiguous(), sa), want_b[u]), u
    with pytest.raises(ValueError, match="state holds"):
        m.make_decode_state(mem, enc_len, max_steps=U + 1, state=sa)
    m.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m.decode_step(ta[:, 0].contiguous(), sa)

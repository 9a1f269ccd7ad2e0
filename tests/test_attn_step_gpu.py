"""smx_attn_step (csrc/attn_step.hip) alone, through ops.attention_step: one query row per (batch row, head) over a KV cache with a
device-side key count, against the float64 softmax of tests/_attention_ref.py.

Error bar (the project's, no constant): the ATen chain - bmm / softmax / bmm at the same dtype on the same inputs and GPU - is measured
against float64 beside ours; ours <= 4 x ATen's, floor 8 eps(dtype) where ATen is exact (tests/_decoder_ref.judge; every pair goes
through tests/_util.report).  All operands are strided views of packed buffers - q / k_new / v_new of one (B, 3, H, D) projection
output, K / V of one (B, cap, 2, H, D) cache - carved out of guarded allocations; cache slots at and beyond n_keys hold NaN."""
import math

import pytest
import torch

from tests import _attention_ref as R
from tests import _decoder_ref as DR

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
HD = [(1, 64), (2, 64), (4, 128), (1, 256), (1, 512)]
B = 3
GUARD = 64          # elements on either side of every buffer
# cap 200: 4 chunks of 50 keys, two launches; cap 40: one chunk, one launch.  Per row key counts from {1, 2, 15, 16, 17, 63, 64, 65, 130, cap}
# cap 2500 (the positional table's max_length): 16 chunks of 157 keys
CASES = [(200, (1, 2, 15)), (200, (16, 17, 63)), (200, (64, 65, 130)), (200, (200, 130, 1)), (40, (1, 17, 40)), (2500, (2500, 130, 65))]


def _guarded(shape, dtype, fill):
    """-> (flat buffer with guards, the view of `shape` inside it)."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return flat, flat[GUARD:GUARD + n].view(shape)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _problem(H, D, cap, ns, dtype, seed):
    """Packed, guarded operands: the cache holds numbers in the slots a CROSS call reads ([0, n)) and NaN beyond."""
    g = torch.Generator().manual_seed(seed)
    qkv_flat, qkv = _guarded((B, 3, H, D), dtype, 7.0)
    kv_flat, kv = _guarded((B, cap, 2, H, D), dtype, float("nan"))
    o_flat, o = _guarded((B, H, D), dtype, -3.0)
    qkv.copy_(torch.randn(B, 3, H, D, generator=g).to(dtype))
    for b, n in enumerate(ns):
        if 1 <= n <= cap:
            kv[b, :n] = torch.randn(n, 2, H, D, generator=g).to(dtype)
    n_keys = torch.tensor(ns, dtype=torch.int32, device="cuda")
    return qkv_flat, qkv, kv_flat, kv, o_flat, o, n_keys


def _aten_row(q, K, V, scale):
    """q (H, D), K / V (n, H, D) -> (H, D): bmm, softmax, bmm at the tensors' dtype."""
    s = torch.bmm(q[:, None, :], K.permute(1, 2, 0)) * scale
    return torch.bmm(torch.softmax(s, -1), V.permute(1, 0, 2))[:, 0]


def _judge(name, dtype, out, qkv, kv_eff, ns, scale):
    ours, aten, ref = {}, {}, {}
    for b, n in enumerate(ns):
        q, K, V = qkv[b, 0], kv_eff[b, :n, 0], kv_eff[b, :n, 1]
        key = f"row {b} n {n}"
        ours[key] = out[b]
        aten[key] = _aten_row(q, K, V, scale).float()
        ref[key] = R.attention(q.double().cpu()[None, None], K.double().cpu()[None], V.double().cpu()[None], scale)[0][0, 0]
    DR.judge(name, dtype, ours, aten, ref)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("H,D", HD)
def test_cross_step_matches_float64_within_aten_bar(H, D, dt):
    from summarymixing_amd import ops
    dtype = DT[dt]
    scale = 1.0 / math.sqrt(D)
    for ci, (cap, ns) in enumerate(CASES):
        qkv_flat, qkv, kv_flat, kv, o_flat, o, n_keys = _problem(H, D, cap, ns, dtype, 100 * ci + H + D)
        kv_before, qkv_before = kv_flat.clone(), qkv_flat.clone()
        out = ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, scale=scale, out=o)
        assert out.data_ptr() == o.data_ptr() and torch.isfinite(o.float()).all(), "NaN slots at and beyond n_keys must not be read"
        _judge(f"attn_step cross H{H} D{D} cap{cap} n{ns} {dt}", dtype, o, qkv, kv, ns, scale)
        assert torch.equal(_bits(kv_flat), _bits(kv_before)) and torch.equal(_bits(qkv_flat), _bits(qkv_before)), "inputs untouched"
        assert bool((o_flat[:GUARD] == -3.0).all()) and bool((o_flat[-GUARD:] == -3.0).all()), "output guards untouched"
        # two runs agree bit for bit; row b equals the same row run alone
        again = ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, scale=scale)
        assert torch.equal(_bits(again), _bits(o))
        for b in range(B):
            alone = ops.attention_step(qkv[b:b + 1, 0], kv[b:b + 1, :, 0], kv[b:b + 1, :, 1], n_keys[b:b + 1].contiguous(), scale=scale)
            assert torch.equal(_bits(alone[0]), _bits(o[b])), f"row {b} depends on its batch"
    # n_keys = None: all cap keys
    cap = 40
    qkv_flat, qkv, kv_flat, kv, o_flat, o, _ = _problem(H, D, cap, (cap, cap, cap), dtype, 5)
    full = ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], None, scale=scale)
    _judge(f"attn_step cross H{H} D{D} cap{cap} all keys {dt}", dtype, full, qkv, kv, (cap,) * B, scale)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("H,D", HD)
def test_self_step_stores_the_new_row_then_attends(H, D, dt):
    """Slot n - 1 receives k_new / v_new bit for bit (it held NaN before), every other slot and every guard element is unchanged bit
    for bit, and the output is the attention over the cache WITH the new row."""
    from summarymixing_amd import ops
    dtype = DT[dt]
    scale = 1.0 / math.sqrt(D)
    for ci, (cap, ns) in enumerate(CASES):
        qkv_flat, qkv, kv_flat, kv, o_flat, o, n_keys = _problem(H, D, cap, ns, dtype, 1000 + 100 * ci + H + D)
        for b, n in enumerate(ns):
            kv[b, n - 1] = float("nan")                       # the slot the call fills
        expect_flat = kv_flat.clone()
        expect = expect_flat[GUARD:-GUARD].view(B, cap, 2, H, D)
        for b, n in enumerate(ns):
            expect[b, n - 1, 0], expect[b, n - 1, 1] = qkv[b, 1], qkv[b, 2]
        qkv_before, kv_before = qkv_flat.clone(), kv_flat.clone()
        ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], scale=scale, out=o)
        assert torch.equal(_bits(kv_flat), _bits(expect_flat)), "slot n - 1 = k_new / v_new, everything else (guards included) unchanged"
        assert torch.equal(_bits(qkv_flat), _bits(qkv_before))
        assert bool((o_flat[:GUARD] == -3.0).all()) and bool((o_flat[-GUARD:] == -3.0).all())
        assert torch.isfinite(o.float()).all()
        _judge(f"attn_step self H{H} D{D} cap{cap} n{ns} {dt}", dtype, o, qkv, expect, ns, scale)
        first = o.clone()
        ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], scale=scale, out=o)
        assert torch.equal(_bits(first), _bits(o)) and torch.equal(_bits(kv_flat), _bits(expect_flat)), "two runs agree bit for bit"
        # row b run alone, from the cache as it was before the call: the same output and the same stored slot, bit for bit
        kv1 = kv_before[GUARD:-GUARD].view(B, cap, 2, H, D)
        for b in range(B):
            alone = ops.attention_step(qkv[b:b + 1, 0], kv1[b:b + 1, :, 0], kv1[b:b + 1, :, 1], n_keys[b:b + 1].contiguous(),
                                       k_new=qkv[b:b + 1, 1], v_new=qkv[b:b + 1, 2], scale=scale)
            assert torch.equal(_bits(alone[0]), _bits(o[b])), f"row {b} depends on its batch"
            assert torch.equal(_bits(kv1[b]), _bits(expect[b])), f"row {b} alone stores what it stores in the batch"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("cap", [40, 200])
def test_key_count_out_of_range_gives_a_zero_row_and_no_store(cap, dt):
    from summarymixing_amd import ops
    dtype = DT[dt]
    H, D = 2, 64
    ns = (0, cap + 1, 5)
    qkv_flat, qkv, kv_flat, kv, o_flat, o, n_keys = _problem(H, D, cap, ns, dtype, 77)
    kv[2, 4] = float("nan")
    before = kv_flat.clone()
    ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], out=o)
    assert bool((o[:2] == 0).all()) and bool((o[2] != 0).any()) and torch.isfinite(o.float()).all()
    assert torch.equal(_bits(kv_flat[:GUARD + 2 * cap * 2 * H * D]), _bits(before[:GUARD + 2 * cap * 2 * H * D])), "rows 0 and 1: no store"
    assert torch.equal(_bits(kv[2, 4, 0]), _bits(qkv[2, 1])) and torch.equal(_bits(kv[2, 4, 1]), _bits(qkv[2, 2]))
    for n_bad in (-1, -(2 ** 31), 2 ** 31 - 1):
        n_keys[0] = n_bad
        ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, out=o)
        assert bool((o[0] == 0).all())

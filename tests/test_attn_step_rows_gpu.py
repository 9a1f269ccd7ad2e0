"""smx_attn_step_rows (csrc/attn_step.hip) alone, through ops.attention_step(anc=, kv_div=): the decoding step's attention over an
INDEXED cache - the cache row of every key is looked up (self-attention: the ancestor table of a beam search; cross-attention: the W
rows of an utterance share its memory), so no K / V is copied when the beams reorder.

Against the float64 softmax of tests/_attention_ref.py over the GATHERED keys, under the project's bar (tests/_decoder_ref.judge,
through tests/_util.report): the ATen chain at the same dtype on the same gathered keys is measured beside ours, ours <= 4 x ATen's.
R = 6 rows (B 2 x W 3).  cap 48: one launch; 70 and 130: 2 and 3 chunks (35 / 44 keys) with a ragged last chunk; key counts 1, 2, 64,
65 and cap, one per utterance.  Every cache slot at or beyond a row's count, and every (row, slot) the table does not name, holds NaN."""
import math

import pytest
import torch

from tests import _attention_ref as R
from tests import _decoder_ref as DR

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
HD = [(1, 64), (4, 64), (1, 512), (4, 512)]
B, W = 2, 3
ROWS = B * W
CAPS = (48, 70, 130)


def _counts(cap):
    """Key counts per row, one count per utterance (the rows of an utterance are at the same position, and a call must not be asked to
    read, for one row, the slot it stores for another): every count of 1, 2, 64, 65, cap that fits, paired with the next."""
    ns = [n for n in (1, 2, 64, 65, cap) if n <= cap]
    return [(ns[k],) * W + (ns[(k + 1) % len(ns)],) * W for k in range(len(ns))]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _aten_row(q, K, V, scale):
    s = torch.bmm(q[:, None, :], K.permute(1, 2, 0)) * scale
    return torch.bmm(torch.softmax(s, -1), V.permute(1, 0, 2))[:, 0]


def _problem(H, D, cap, ns, dtype, seed, rows=ROWS):
    """qkv (rows, 3, H, D), a NaN cache (rows, cap, 2, H, D), anc (rows, cap) random within the utterance's rows for j < n - 1 (garbage
    elsewhere: never read), the named (row, slot) pairs filled with numbers.  -> qkv, kv, anc, n_keys, gathered [(K_r, V_r)] with the
    step's own key last."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3, H, D, generator=g).to(dtype).cuda()
    anc = torch.full((rows, cap), 2 ** 31 - 1, dtype=torch.int32)
    named = torch.zeros((rows, cap), dtype=torch.bool)
    for r, n in enumerate(ns):
        u = r // W
        anc[r, :n - 1] = torch.randint(u * W, (u + 1) * W, (n - 1,), generator=g, dtype=torch.int32)
        named[anc[r, :n - 1].long(), torch.arange(n - 1)] = True
    kv = torch.where(named[:, :, None, None, None], torch.randn(rows, cap, 2, H, D, generator=g), torch.tensor(float("nan"))).to(dtype).cuda()
    anc = anc.cuda()
    gathered = []
    for r, n in enumerate(ns):
        idx = anc[r, :n - 1].long()
        own = torch.arange(n - 1, device="cuda")
        K = torch.cat([kv[idx, own, 0], qkv[r:r + 1, 1]], 0)
        V = torch.cat([kv[idx, own, 1], qkv[r:r + 1, 2]], 0)
        gathered.append((K, V))
    return qkv, kv, anc, torch.tensor(ns, dtype=torch.int32, device="cuda"), gathered


def _judge(name, dtype, out, qkv, gathered, scale, drop=None):
    ours, aten, ref = {}, {}, {}
    for r, (K, V) in enumerate(gathered):
        if drop is not None and drop[0] == r:
            keep = [j for j in range(K.shape[0]) if j != drop[1]]
            K, V = K[keep], V[keep]
        q = qkv[r, 0]
        key = f"row {r} n {K.shape[0]}"
        ours[key] = out[r]
        aten[key] = _aten_row(q, K, V, scale).float()
        ref[key] = R.attention(q.double().cpu()[None, None], K.double().cpu()[None], V.double().cpu()[None], scale)[0][0, 0]
    DR.judge(name, dtype, ours, aten, ref)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("H,D", HD)
def test_self_step_reads_its_keys_through_the_ancestor_table(H, D, dt):
    from summarymixing_amd import ops
    dtype, scale = DT[dt], 1.0 / math.sqrt(D)
    for ci, (cap, ns) in enumerate((cap, ns) for cap in CAPS for ns in _counts(cap)):
        qkv, kv, anc, n_keys, gathered = _problem(H, D, cap, ns, dtype, 10 * ci + H + D)
        expect = kv.clone()
        for r, n in enumerate(ns):
            expect[r, n - 1, 0], expect[r, n - 1, 1] = qkv[r, 1], qkv[r, 2]
        before = kv.clone()
        o = ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], scale=scale, anc=anc)
        assert torch.isfinite(o.float()).all(), "a slot at or beyond n, or a (row, slot) the table does not name, was read"
        assert torch.equal(_bits(kv), _bits(expect)), "row r, slot n - 1 = k_new / v_new; nothing else is written"
        _judge(f"attn_step_rows self H{H} D{D} cap{cap} n{ns} {dt}", dtype, o, qkv, gathered, scale)
        # two runs agree bit for bit (the second finds slot n - 1 already written: it is read from k_new either way)
        again = ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], scale=scale, anc=anc)
        assert torch.equal(_bits(again), _bits(o))
        # utterance 0's rows do not depend on B: the same three rows alone, from the cache as it was
        alone = ops.attention_step(qkv[:W, 0], before[:W, :, 0], before[:W, :, 1], n_keys[:W].contiguous(), k_new=qkv[:W, 1],
                                   v_new=qkv[:W, 2], scale=scale, anc=anc[:W].contiguous())
        assert torch.equal(_bits(alone), _bits(o[:W])), "utterance 0 depends on the batch"
        # an entry outside [0, R) removes its key: the float64 softmax without it, the same bits whatever the entry
        r = max(range(ROWS), key=lambda i: ns[i])
        if ns[r] >= 3:
            j = ns[r] // 2
            outs = []
            for bad in (-1, ROWS, 2 ** 31 - 1, -(2 ** 31)):
                anc2 = anc.clone()
                anc2[r, j] = bad
                outs.append(ops.attention_step(qkv[:, 0], kv[:, :, 0], kv[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], scale=scale, anc=anc2))
                assert torch.equal(_bits(outs[-1]), _bits(outs[0])), bad
            _judge(f"attn_step_rows self H{H} D{D} cap{cap} key ({r}, {j}) removed {dt}", dtype, outs[0], qkv, gathered, scale, drop=(r, j))
            others = [i for i in range(ROWS) if i != r]
            assert torch.equal(_bits(outs[0][others]), _bits(o[others])), "the other rows are what they were"
            assert not torch.equal(_bits(outs[0][r]), _bits(o[r]))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("H,D", HD)
def test_identity_table_gives_the_plain_steps_bits(H, D, dt):
    """anc[r, j] = r with kv_div = 1 is smx_attn_step: the same bits, the same stored slot."""
    from summarymixing_amd import ops
    dtype, scale = DT[dt], 1.0 / math.sqrt(D)
    for ci, (cap, ns) in enumerate((cap, ns) for cap in CAPS for ns in _counts(cap)):
        g = torch.Generator().manual_seed(500 + 10 * ci + H + D)
        qkv = torch.randn(ROWS, 3, H, D, generator=g).to(dtype).cuda()
        kv = torch.full((ROWS, cap, 2, H, D), float("nan"), dtype=dtype, device="cuda")
        for r, n in enumerate(ns):
            kv[r, :n - 1] = torch.randn(n - 1, 2, H, D, generator=g).to(dtype).cuda()
        n_keys = torch.tensor(ns, dtype=torch.int32, device="cuda")
        anc = torch.arange(ROWS, dtype=torch.int32, device="cuda")[:, None].expand(ROWS, cap).contiguous()
        kv_a, kv_b = kv.clone(), kv.clone()
        plain = ops.attention_step(qkv[:, 0], kv_a[:, :, 0], kv_a[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], scale=scale)
        rows = ops.attention_step(qkv[:, 0], kv_b[:, :, 0], kv_b[:, :, 1], n_keys, k_new=qkv[:, 1], v_new=qkv[:, 2], scale=scale, anc=anc)
        assert torch.isfinite(plain.float()).all()
        assert torch.equal(_bits(rows), _bits(plain)) and torch.equal(_bits(kv_a), _bits(kv_b)), (cap, ns)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("H,D", HD)
def test_shared_memory_gives_the_bits_of_the_replicated_memory(H, D, dt):
    """Cross-attention with kv_div = 3: the W rows of an utterance read ITS memory row and ITS length; the same bits as smx_attn_step
    over the memory replicated 3 times, and the float64 softmax under the bar."""
    from summarymixing_amd import ops
    dtype, scale = DT[dt], 1.0 / math.sqrt(D)
    for ci, cap in enumerate(CAPS):
        lens = (cap, max(1, cap - 5)) if ci != 1 else (65, cap)
        g = torch.Generator().manual_seed(900 + 10 * ci + H + D)
        q = torch.randn(ROWS, H, D, generator=g).to(dtype).cuda()
        mem = torch.full((B, cap, 2, H, D), float("nan"), dtype=dtype, device="cuda")
        for b, n in enumerate(lens):
            mem[b, :n] = torch.randn(n, 2, H, D, generator=g).to(dtype).cuda()
        mem_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
        before = mem.clone()
        o = ops.attention_step(q, mem[:, :, 0], mem[:, :, 1], mem_len, scale=scale, kv_div=W)
        assert torch.isfinite(o.float()).all() and torch.equal(_bits(mem), _bits(before))
        rep = mem.repeat_interleave(W, 0)
        plain = ops.attention_step(q, rep[:, :, 0], rep[:, :, 1], mem_len.repeat_interleave(W).contiguous(), scale=scale)
        assert torch.equal(_bits(o), _bits(plain)), (cap, lens)
        assert torch.equal(_bits(ops.attention_step(q, mem[:, :, 0], mem[:, :, 1], mem_len, scale=scale, kv_div=W)), _bits(o))
        qkv = torch.stack([q, q, q], 1)
        gathered = [(mem[r // W, :lens[r // W], 0], mem[r // W, :lens[r // W], 1]) for r in range(ROWS)]
        _judge(f"attn_step_rows cross kv_div{W} H{H} D{D} cap{cap} len{lens} {dt}", dtype, o, qkv, gathered, scale)
        one = ops.attention_step(q[:W], mem[:1, :, 0], mem[:1, :, 1], mem_len[:1].contiguous(), scale=scale, kv_div=W)
        assert torch.equal(_bits(one), _bits(o[:W])), "utterance 0 depends on the batch"

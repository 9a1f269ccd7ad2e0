"""The fused attention kernels (csrc/attention.hip) and nnet.attention.MultiheadAttention against the float64 restatement of
tests/_attention_ref.py, through the C-ABI ops and through the module, fp32 and bf16 (the float64 side gets the bf16-rounded inputs).

Error bars: no constants.  Every parity check also runs the ATen chain at the same dtype on the same GPU and inputs
(torch.nn.MultiheadAttention's multi_head_attention_forward for the module, its baddbmm / softmax / bmm restatement where the ops are
tested or dropout needs the explicit mask), measures both against float64 with tests/_util.rel_err and asserts
ours <= 4 x ATen's (different summation orders: a k-ordered fp32 chain over D up to 512 against library tiles; one bf16 rounding of
p~), with a floor of 8 eps(dtype) max|ref| where ATen's error is 0.  Every measured pair is recorded through tests/_util.report
(profiles/attention_parity_errors.jsonl holds the records of the first run)."""
import math

import pytest
import torch

from tests import _attention_ref as R
from tests._util import rel_err, report

pytestmark = pytest.mark.gpu
NEG = float("-inf")
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _eps(dtype):
    return torch.finfo(dtype).eps


def _report(name, pairs):
    report(name, {"errors": {k: {"ours": o, "aten": a, "bar": b} for k, (o, a, b) in pairs.items()}})


def _judge(name, dtype, ours, aten, ref):
    """ours / aten / ref: dicts of tensors under the same keys.  Prints and records every pair, then asserts the bar on all of them."""
    pairs = {}
    for k, r in ref.items():
        assert torch.isfinite(ours[k].float()).all() or k == "lse", f"{name}: non-finite values in {k}"
        eo, ea = rel_err(ours[k], r), rel_err(aten[k], r)
        pairs[k] = (eo, ea, 4.0 * ea if ea > 0.0 else 8.0 * _eps(dtype))    # (rel_err is relative to max|ref|: the floor is 8 eps max|ref|)
    print(name, {k: f"{o:.2e} / {a:.2e}" for k, (o, a, _) in pairs.items()})
    _report(name, pairs)
    bad = {k: v for k, v in pairs.items() if not v[0] <= v[2]}
    assert not bad, f"{name}: ours > 4 x ATen (8 eps where ATen is exact) (ours, aten, bar): {bad}"


def _aten_attention(q, k, v, scale, bias, key_pad, causal, keep, drop_p):
    """ATen at q's dtype, as multi_head_attention_forward computes it: q scaled first, the masks merged into one additive float mask,
    baddbmm, softmax, (explicit keep mask), bmm.  -> (o (B, L, H, D), p~ (B, H, L, S), lse (B, H, L))."""
    B, L, H, D = q.shape
    S = k.shape[1]
    m = torch.zeros((B, 1, L, S), dtype=q.dtype, device=q.device)
    if bias is not None:
        m = m + bias.to(q.dtype)
    if causal:
        m = m.masked_fill(torch.triu(torch.ones(L, S, dtype=torch.bool, device=q.device), diagonal=1 + S - L), NEG)
    if key_pad is not None:
        m = m.masked_fill(key_pad[:, None, None, :], NEG)
    m = m.expand(B, H, L, S).reshape(B * H, L, S)
    qh, kh, vh = (t.permute(0, 2, 1, 3).reshape(B * H, t.shape[1], D) for t in (q, k, v))
    s = torch.baddbmm(m, qh * scale, kh.transpose(1, 2))
    p = torch.softmax(s, dim=-1)
    if keep is not None:
        p = p * keep.reshape(B * H, L, S).to(p.dtype) / (1.0 - drop_p)
    o = torch.bmm(p, vh).view(B, H, L, D).permute(0, 2, 1, 3)
    return o, p.view(B, H, L, S), torch.logsumexp(s.detach(), dim=-1).view(B, H, L)


def _key_pad(B, S, lens=True):
    """Per-row key lengths 1, S / 2, S (cycled over the batch) as a bool padding mask."""
    pad = torch.zeros(B, S, dtype=torch.bool, device="cuda")
    for b, n in zip(range(B), [max(1, S // 2), 1, S] * B):
        pad[b, n:] = True
    return pad


def _inputs(B, L, S, H, D, dtype, packed, seed, qscale=1.0):
    """q, k, v as views of a packed (B, L, 3, H, D) buffer ('qkv'), q alone + a packed (B, S, 2, H, D) buffer ('kv'), or three
    separate tensors ('none'); and matching gradient destinations."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).cuda().to(dtype)
    if packed == "qkv":
        assert L == S
        buf, gbuf = rnd(B, L, 3, H, D), torch.full((B, L, 3, H, D), float("nan"), dtype=dtype, device="cuda")
        if qscale != 1.0:
            buf[:, :, 0] *= qscale
        views, gviews = [buf[:, :, i] for i in range(3)], [gbuf[:, :, i] for i in range(3)]
    elif packed == "kv":
        q, buf = rnd(B, L, H, D) * qscale, rnd(B, S, 2, H, D)
        gbuf = torch.full((B, S, 2, H, D), float("nan"), dtype=dtype, device="cuda")
        views, gviews = [q, buf[:, :, 0], buf[:, :, 1]], [torch.empty_like(q), gbuf[:, :, 0], gbuf[:, :, 1]]
    else:
        views = [rnd(B, L, H, D) * qscale, rnd(B, S, H, D), rnd(B, S, H, D)]
        gviews = [None, None, None]
    r = rnd(B, L, H, D)
    return views, gviews, r


def _run_ops_case(name, B, L, S, H, D, dtype, packed="none", pad=None, causal=False, bias=None, drop_p=0.0, seed=0, qscale=1.0,
                  dead_rows=(), want=("o", "lse", "w", "dq", "dk", "dv")):
    """One problem through ops.attention_fwd / _weights / _bwd, the ATen chain and the float64 restatement; judged by _judge.
    dead_rows: query rows whose bias row is all -inf.  torch gives NaN there, so ATen sees those rows unmasked with a zero upstream
    gradient (the same contribution to dK / dV as the specified zero row) and its O rows are set to the specified zeros."""
    from summarymixing_amd import ops
    (q, k, v), (gq, gk, gv), r = _inputs(B, L, S, H, D, dtype, packed, 1000 + seed, qscale)
    scale = 1.0 / math.sqrt(D)
    keep = None
    if drop_p > 0.0:
        keep = ops.dropout(torch.ones(B * H * L, S, device="cuda"), drop_p, seed) != 0
    bias_ours = bias
    if dead_rows:
        bias_ours = (torch.zeros(L, S, device="cuda") if bias is None else bias.clone())
        bias_ours[list(dead_rows)] = NEG
    o, lse = ops.attention_fwd(q, k, v, bias_ours, None if pad is None else pad.view(torch.uint8), causal, scale, drop_p, seed)
    w = ops.attention_weights(q, k, lse, bias_ours, None if pad is None else pad.view(torch.uint8), causal, scale, drop_p, seed)
    dq, dk, dv = ops.attention_bwd(r, q, k, v, o, lse, bias_ours, None if pad is None else pad.view(torch.uint8), causal, scale,
                                   drop_p, seed, dq=gq, dk=gk, dv=gv)
    ours = dict(o=o, lse=lse, w=w, dq=dq, dk=dk, dv=dv)
    # float64
    q6, k6, v6 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    o6, lse6, p6 = R.attention(q6, k6, v6, scale, None if bias_ours is None else bias_ours.double(), pad, causal, keep, drop_p)
    (o6 * r.double()).sum().backward()
    ref = dict(o=o6.detach(), lse=lse6, w=p6.detach().mean(dim=1), dq=q6.grad, dk=k6.grad, dv=v6.grad)
    # ATen at the same dtype
    qa, ka, va = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    ra = r.clone()
    if dead_rows:
        ra[:, list(dead_rows)] = 0
    oa, pa, lsea = _aten_attention(qa, ka, va, scale, bias, pad, causal, keep, drop_p)
    (oa * ra).sum().backward()
    oa, wa = oa.detach().clone(), pa.detach().float().mean(dim=1)
    if dead_rows:
        oa[:, list(dead_rows)] = 0
        wa[:, list(dead_rows)] = 0
        lsea[:, :, list(dead_rows)] = NEG
    aten = dict(o=oa, lse=lsea, w=wa, dq=qa.grad, dk=ka.grad, dv=va.grad)
    _judge(name, dtype, {k_: ours[k_] for k_ in want}, aten, {k_: ref[k_] for k_ in want})
    return ours, ref, pad


# (B, L, S, H, D, packed, key lengths, causal, bias kind)
_CASES = [
    (1, 1, 200, 1, 512, "none", False, False, None),           # the decode step
    (3, 7, 5, 4, 64, "none", True, False, None),
    (3, 16, 64, 2, 128, "kv", False, False, "float"),
    (3, 17, 129, 2, 128, "kv", False, False, "tile0"),         # rows that lose the whole first key tile
    (3, 17, 129, 2, 128, "none", True, False, "float"),
    (1, 33, 63, 4, 64, "none", False, False, "float"),
    (3, 65, 65, 1, 512, "qkv", False, True, None),             # causal, L == S, packed projections
    (3, 17, 17, 2, 128, "qkv", True, True, None),              # causal and key padding together
    (3, 16, 1, 1, 512, "none", False, False, None),            # S = 1: ATen's error is 0, the floor applies
    (3, 65, 200, 4, 64, "kv", True, False, None),
    (1, 7, 65, 2, 128, "none", False, False, "float"),
    (3, 17, 129, 1, 256, "kv", True, False, None),             # D = 256: two LDS chunks of D, a count no other size has
]


def _bias(kind, L, S):
    if kind is None:
        return None
    b = torch.randn(L, S, generator=torch.Generator().manual_seed(L * 1000 + S)).cuda()
    if kind == "tile0":
        b[[3, 4, L - 1], :64] = NEG                              # these rows first see a key in the second tile
        b[5, 70:] = NEG
    return b


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", _CASES, ids=["-".join(map(str, c[:6])) for c in _CASES])
def test_ops_match_float64_within_aten_bar(case, dt):
    B, L, S, H, D, packed, lens, causal, bias_kind = case
    pad = _key_pad(B, S) if lens else None
    ours, ref, _ = _run_ops_case(f"ops {case[:6]} {dt}", B, L, S, H, D, DT[dt], packed, pad, causal, _bias(bias_kind, L, S))
    if pad is not None:
        pk = pad[:, :, None, None].expand_as(ours["dk"])
        assert float(ours["dk"][pk].float().abs().max()) == 0.0 and float(ours["dv"][pk].float().abs().max()) == 0.0
    masked = ref["w"] == 0                                                            # masked weights are exact zeros
    assert float(ours["w"][masked].abs().max() if masked.any() else 0.0) == 0.0
    # rows sum to 1 within fp32 rounding: every probability carries the rounding of lse (|lse| < 8 here: half an ulp of 8 is 4 eps), of
    # s - lse and of exp (a few eps more) - 16 eps relative in all - and the fp32 sum of S terms adds at most S eps
    rows = ours["w"].sum(dim=-1)
    assert float(ours["lse"].abs().max()) < 8 and float((rows - 1).abs().max()) <= (16 + S) * _eps(torch.float32)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_fully_masked_rows_give_zeros_and_zero_gradients(dt):
    B, L, S, H, D = 3, 17, 129, 2, 128
    dead = (0, 9, 16)
    ours, ref, _ = _run_ops_case(f"dead rows {dt}", B, L, S, H, D, DT[dt], "kv", _key_pad(B, S), False, None, dead_rows=dead)
    for k_, t in ours.items():
        assert not torch.isnan(t.float()).any(), k_
    assert float(ours["o"][:, list(dead)].float().abs().max()) == 0.0 and float(ours["dq"][:, list(dead)].float().abs().max()) == 0.0
    assert (ours["lse"][:, :, list(dead)] == NEG).all() and torch.isfinite(ours["lse"][:, :, 1]).all()
    assert float(ours["w"][:, list(dead)].abs().max()) == 0.0
    assert all(torch.isfinite(ours[k_].float()).all() for k_ in ("o", "w", "dq", "dk", "dv"))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_saturated_softmax_stays_finite(dt):
    """Queries scaled by 30: scores of several hundred, the softmax is one-hot to rounding."""
    _run_ops_case(f"saturated {dt}", 3, 33, 129, 2, 128, DT[dt], "none", _key_pad(3, 129), False, None, qscale=30.0)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_matches_reference_with_the_librarys_keep_mask(p, dt):
    """The keep mask is what ops.dropout draws on ones of shape (B H L, S) with the same seed; the restatement and ATen get it
    explicitly.  Forward, weights and all gradients."""
    _run_ops_case(f"dropout p={p} kv {dt}", 3, 17, 129, 2, 128, DT[dt], "kv", _key_pad(3, 129), False, None, drop_p=p, seed=1234,
                  want=("o", "w", "dq", "dk", "dv"))
    _run_ops_case(f"dropout p={p} causal {dt}", 1, 33, 33, 4, 64, DT[dt], "qkv", None, True, None, drop_p=p, seed=77,
                  want=("o", "w", "dq", "dk", "dv"))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keep_rate_and_seeds(p):
    """N = 3 x 260 x 200 = 156 000 draws: the keep rate lies within 5 sigma of 1 - p, sigma = sqrt(p (1 - p) / N); another seed or a
    bumped step counter gives another mask, the same seed the same one."""
    from summarymixing_amd import ops
    B, L, S, H, D = 3, 260, 200, 1, 64
    q = torch.zeros(B, L, H, D, device="cuda")                 # uniform probabilities 1 / S: a weight is non-zero iff it was kept
    k = torch.randn(B, S, H, D, device="cuda")
    _, lse = ops.attention_fwd(q, k, k)

    def kept(seed):
        return ops.attention_weights(q, k, lse, drop_p=p, seed=seed) != 0
    m1 = kept(5)
    N = m1.numel()
    assert N >= 1e5
    sigma = math.sqrt(p * (1 - p) / N)
    assert abs(float(m1.float().mean()) - (1 - p)) <= 5 * sigma
    assert torch.equal(m1.view(B * L, S), ops.dropout(torch.ones(B * H * L, S, device="cuda"), p, 5) != 0)
    assert torch.equal(m1, kept(5)) and not torch.equal(m1, kept(6))
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.set_step_counter(counter)
    try:
        a = kept(5)
        ops.step_counter_add(counter, 1)
        b = kept(5)
        assert not torch.equal(a, b) and abs(float(b.float().mean()) - (1 - p)) <= 5 * sigma
    finally:
        ops.set_step_counter(None)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_forward_and_backward_are_bit_reproducible(dt):
    from summarymixing_amd import ops
    B, L, S, H, D = 3, 65, 200, 2, 128
    (q, k, v), _, r = _inputs(B, L, S, H, D, DT[dt], "kv", 3)
    pad = _key_pad(B, S).view(torch.uint8)
    outs = []
    for _ in range(2):
        o, lse = ops.attention_fwd(q, k, v, None, pad, False, None, 0.1, 9)
        outs.append((o, lse, ops.attention_weights(q, k, lse, None, pad, False, None, 0.1, 9)) + ops.attention_bwd(r, q, k, v, o, lse, None, pad, False, None, 0.1, 9))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_functional_sdpa_autograd_on_packed_views():
    """functional.scaled_dot_product_attention as an autograd Function over views of one packed projection output."""
    from summarymixing_amd import functional as F
    B, L, H, D = 3, 17, 2, 128
    buf = torch.randn(B, L, 3, H, D, generator=torch.Generator().manual_seed(4)).cuda().requires_grad_(True)
    r = torch.randn(B, L, H, D, generator=torch.Generator().manual_seed(5)).cuda()
    pad = _key_pad(B, L)
    o = F.scaled_dot_product_attention(buf[:, :, 0], buf[:, :, 1], buf[:, :, 2], key_padding_mask=pad, causal=True)
    (o * r).sum().backward()
    b6 = buf.detach().double().requires_grad_(True)
    o6, _, _ = R.attention(b6[:, :, 0], b6[:, :, 1], b6[:, :, 2], None, None, pad, True)
    (o6 * r.double()).sum().backward()
    ba = buf.detach().clone().requires_grad_(True)
    oa, _, _ = _aten_attention(ba[:, :, 0], ba[:, :, 1], ba[:, :, 2], 1.0 / math.sqrt(D), None, pad, True, None, 0.0)
    (oa * r).sum().backward()
    _judge("functional sdpa f32", torch.float32, dict(o=o.detach(), dbuf=buf.grad), dict(o=oa.detach(), dbuf=ba.grad), dict(o=o6.detach(), dbuf=b6.grad))


# ---- module level -------------------------------------------------------------------------------------------------------------------
def _modules(d, H, dtype, dropout=0.0):
    """torch's module with random (bf16-representable when dtype is bf16) parameters; ours loaded from its state dict; a float64 copy."""
    from summarymixing_amd.nnet.attention import MultiheadAttention
    torch.manual_seed(d + H)
    tm = torch.nn.MultiheadAttention(d, H, dropout=dropout, batch_first=True)
    with torch.no_grad():
        tm.in_proj_bias.normal_(0.0, 0.1)
        tm.out_proj.bias.normal_(0.0, 0.1)
        if dtype == torch.bfloat16:
            for p_ in tm.parameters():
                p_.copy_(p_.bfloat16().float())
    ours = MultiheadAttention(H, d, dropout=dropout)
    ours.load_state_dict({"att." + k_: v_ for k_, v_ in tm.state_dict().items()}, strict=True)
    t64 = torch.nn.MultiheadAttention(d, H, batch_first=True).double()
    t64.load_state_dict(tm.state_dict())
    return ours.cuda(), tm.cuda().to(dtype), t64.cuda()


_PNAMES = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


def _pgrads(m, prefix=""):
    sd = dict(m.named_parameters())
    return {n: sd[prefix + n].grad for n in _PNAMES}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("kind,B,L,S,H,d", [("self", 3, 17, 17, 4, 256), ("kv_same", 3, 16, 65, 1, 512), ("general", 3, 7, 129, 2, 256)])
def test_module_matches_torch_module_weights(kind, B, L, S, H, d, dt):
    """out, weights, d query / d key / d value and the four parameter gradients, parameters loaded out of torch's module: self-attention
    (one d -> 3d GEMM; causal + key padding), key is value (d -> d plus d -> 2d; float mask + key padding) and the general case."""
    dtype = DT[dt]
    ours, tm, t64 = _modules(d, H, dtype)
    g = torch.Generator().manual_seed(B * L + S)
    x = [torch.randn(B, n, d, generator=g).cuda().to(dtype) for n in (L, S, S)]
    r = torch.randn(B, L, d, generator=g).cuda().to(dtype)
    pad = _key_pad(B, S)
    mask = None if kind == "self" else _bias("float", L, S)
    look = torch.triu(torch.ones(L, L, dtype=torch.bool, device="cuda"), diagonal=1) if kind == "self" else None

    def leaves(cast):
        q = cast(x[0]).requires_grad_(True)
        if kind == "self":
            return q, q, q
        k = cast(x[1]).requires_grad_(True)
        return (q, k, k) if kind == "kv_same" else (q, k, cast(x[2]).requires_grad_(True))

    def collect(ins, out, w, pg):
        res = dict(out=out.detach(), w=w.detach().float(), dquery=ins[0].grad)
        if kind != "self":
            res["dkey"] = ins[1].grad
        if kind == "general":
            res["dvalue"] = ins[2].grad
        res.update(pg)
        return res
    ins = leaves(lambda t: t.detach().clone())
    out, w = ours(*ins, attn_mask=mask, key_padding_mask=pad, causal=kind == "self")
    assert not w.requires_grad and w.dtype == torch.float32
    (out * r).sum().backward()
    res_o = collect(ins, out, w, _pgrads(ours, "att."))
    ins_a = leaves(lambda t: t.detach().clone())
    mask_a = look if kind == "self" else mask.to(dtype)
    pad_a = pad if kind == "self" else torch.zeros(B, S, dtype=dtype, device="cuda").masked_fill(pad, NEG)
    out_a, w_a = tm(*ins_a, attn_mask=mask_a, key_padding_mask=pad_a, need_weights=True)
    (out_a * r).sum().backward()
    res_a = collect(ins_a, out_a, w_a, _pgrads(tm))
    ins_6 = leaves(lambda t: t.detach().double())
    sd = dict(t64.named_parameters())
    out_6, w_6 = R.mha(*ins_6, sd["in_proj_weight"], sd["in_proj_bias"], sd["out_proj.weight"], sd["out_proj.bias"], H,
                       None if mask is None else mask.double(), pad, kind == "self")
    (out_6 * r.double()).sum().backward()
    res_6 = collect(ins_6, out_6, w_6, _pgrads(t64))
    _judge(f"module {kind} ({B},{L},{S},{H},{d}) {dt}", dtype, res_o, res_a, res_6)
    out_only = ours(*leaves(lambda t: t.detach().clone()), attn_mask=mask, key_padding_mask=pad, causal=kind == "self", return_attn_weights=False)
    assert torch.is_tensor(out_only) and torch.equal(out_only, out)


def _capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def _graph_setup(dropout):
    """A decoder layer's two attentions: causal self-attention over the tokens, then cross-attention over a padded memory."""
    sa, _, _ = _modules(256, 2, torch.float32, dropout)
    ca, _, _ = _modules(256, 4, torch.float32, dropout)
    sa.train(), ca.train()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 17, 256, generator=g).cuda().requires_grad_(True)
    mem = torch.randn(3, 65, 256, generator=g).cuda()
    r = torch.randn(3, 17, 256, generator=g).cuda()
    pad = _key_pad(3, 65)
    held = {}
    params = list(sa.parameters()) + list(ca.parameters())

    def step():
        for p_ in params:
            if p_.grad is not None:
                p_.grad.zero_()
        x.grad = None
        y = sa(x, x, x, causal=True, return_attn_weights=False)
        z = ca(y, mem, mem, key_padding_mask=pad, return_attn_weights=False)
        (z * r).sum().backward()
        held["z"], held["gx"] = z.detach(), x.grad
    return params, step, held


def test_graph_capture_replay_equals_eager():
    """One forward + backward of the module (self-attention, then cross-attention) under torch.cuda.graph on a single stream."""
    params, step, held = _graph_setup(0.0)
    step()
    torch.cuda.synchronize()
    ref = [held["z"].clone(), held["gx"].clone()] + [p_.grad.clone() for p_ in params]
    graph = _capture(step)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    got = [held["z"], held["gx"]] + [p_.grad for p_ in params]
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_graph_replays_draw_fresh_attention_dropout_masks():
    from summarymixing_amd import ops
    _, step, held = _graph_setup(0.5)
    step()                                                     # (eager first, as a training loop would: workspaces and job tables exist)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.set_step_counter(counter)
    try:
        def step_and_count():
            step()
            ops.step_counter_add(counter, 1)
        graph = _capture(step_and_count)
        graph.replay(); torch.cuda.synchronize(); z1, g1 = held["z"].clone(), held["gx"].clone()
        graph.replay(); torch.cuda.synchronize(); z2, g2 = held["z"].clone(), held["gx"].clone()
        assert torch.isfinite(z1).all() and torch.isfinite(g2).all()
        assert not torch.equal(z1, z2) and not torch.equal(g1, g2)
    finally:
        ops.set_step_counter(None)

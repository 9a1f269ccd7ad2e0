"""MultiheadAttention (regularMHA) without a GPU: the float64 restatement the GPU tests compare against equals torch's module, the
drop-in surface (state_dict keys, strict load, refusals by name) and the host side of the C ABI (descriptor size, plan query)."""
import ctypes

import pytest
import torch

from tests import _attention_ref as R


def _torch_mha(d, H, seed=0):
    torch.manual_seed(seed)
    m = torch.nn.MultiheadAttention(d, H, batch_first=True).double()
    with torch.no_grad():
        m.in_proj_bias.normal_(0.0, 0.1)
        m.out_proj.bias.normal_(0.0, 0.1)
    return m


def test_restatement_equals_torch_multihead_attention():
    """(B, L, S, H, d) = (3, 7, 13, 4, 64), a float attn_mask with -inf entries and a bool key_padding_mask that leave no row fully
    masked (torch gives NaN there).  Both sides are float64 and differ at most in the order of their sums: the bar is 1e-12 of the
    largest value, four orders above float64's 1.1e-16 for the d = 64 / S = 13 term sums, eight below any formula error."""
    B, L, S, H, d = 3, 7, 13, 4, 64
    m = _torch_mha(d, H)
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, n, d, generator=g, dtype=torch.float64) for n in (L, S, S))
    am = torch.randn(L, S, generator=g, dtype=torch.float64)
    am[torch.rand(L, S, generator=g) < 0.3] = float("-inf")
    am[:, 0] = 0.0                                           # key 0 stays visible to every query ...
    kpm = torch.zeros(B, S, dtype=torch.bool)
    kpm[1, 9:] = True                                        # ... and is never padded
    kpm[2, 1:] = True                                        # per-row key length 1
    out_t, w_t = m(q, k, v, attn_mask=am, key_padding_mask=kpm, need_weights=True)
    out_r, w_r = R.mha(q, k, v, m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias, H, attn_bias=am, key_pad=kpm)
    assert torch.isfinite(out_t).all()
    eo = float((out_r - out_t).detach().abs().max() / out_t.detach().abs().max())
    ew = float((w_r - w_t).abs().max())
    print(f"restatement vs torch: out {eo:.3e}, weights {ew:.3e}")
    assert eo <= 1e-12 and ew <= 1e-12
    assert torch.equal(w_r == 0, w_t == 0)
    # the causal flag is the (L, L) look-ahead mask
    look = torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)
    out_t, w_t = m(q, q, q, attn_mask=look)
    out_r, w_r = R.mha(q, q, q, m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias, H, causal=True)
    assert float((out_r - out_t).abs().max() / out_t.abs().max()) <= 1e-12 and float((w_r - w_t).abs().max()) <= 1e-12


def test_restatement_fully_masked_row_is_zero_with_zero_gradients():
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(2, n, 2, 8, generator=g, dtype=torch.float64).requires_grad_(True) for n in (3, 5, 5))
    bias = torch.zeros(3, 5, dtype=torch.float64)
    bias[1] = float("-inf")
    o, lse, p = R.attention(q, k, v, attn_bias=bias)
    assert torch.equal(o[:, 1], torch.zeros_like(o[:, 1])) and torch.isinf(lse[:, :, 1]).all() and torch.isfinite(lse[:, :, 0]).all()
    o.sum().backward()
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v)) and torch.equal(q.grad[:, 1], torch.zeros_like(q.grad[:, 1]))


def test_state_dict_keys_and_strict_load_from_torch():
    from summarymixing_amd.nnet.attention import MultiheadAttention
    m = MultiheadAttention(4, 256, dropout=0.1)
    assert sorted(m.state_dict()) == ["att.in_proj_bias", "att.in_proj_weight", "att.out_proj.bias", "att.out_proj.weight"]
    assert m.att.in_proj_weight.shape == (768, 256) and m.att.out_proj.weight.shape == (256, 256)
    t = torch.nn.MultiheadAttention(256, 4, batch_first=True)
    m.load_state_dict({"att." + k: v for k, v in t.state_dict().items()}, strict=True)
    assert torch.equal(m.att.in_proj_weight, t.in_proj_weight) and torch.equal(m.att.out_proj.bias, t.out_proj.bias)
    nb = MultiheadAttention(1, 64, bias=False)
    assert sorted(nb.state_dict()) == ["att.in_proj_weight", "att.out_proj.weight"]
    nb.load_state_dict({"att." + k: v for k, v in torch.nn.MultiheadAttention(64, 1, bias=False).state_dict().items()}, strict=True)


def test_initial_distributions_match_torch():
    from summarymixing_amd.nnet.attention import MultiheadAttention
    m = MultiheadAttention(1, 512)
    bound = (6.0 / (512 + 3 * 512)) ** 0.5                   # xavier-uniform over the (3d, d) in-projection
    w = m.att.in_proj_weight.detach()
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.99 * bound
    assert abs(float(w.std()) - bound / 3 ** 0.5) < 0.02 * bound
    assert float(m.att.in_proj_bias.abs().max()) == 0.0 and float(m.att.out_proj.bias.abs().max()) == 0.0


@pytest.mark.parametrize("kw,word", [(dict(kdim=128), "kdim"), (dict(vdim=32), "vdim"), (dict(add_bias_kv=True), "add_bias_kv"),
                                     (dict(add_zero_attn=True), "add_zero_attn")])
def test_constructor_refuses_by_name(kw, word):
    from summarymixing_amd.nnet.attention import MultiheadAttention
    with pytest.raises(NotImplementedError, match=word):
        MultiheadAttention(4, 256, **kw)


@pytest.mark.parametrize("nhead,d_model", [(8, 256), (3, 288), (1, 1024), (5, 256)])
def test_constructor_refuses_head_dims_outside_the_set(nhead, d_model):
    from summarymixing_amd.nnet.attention import MultiheadAttention
    with pytest.raises(NotImplementedError, match="head dimension"):
        MultiheadAttention(nhead, d_model)


def test_forward_refusals_by_name():
    from summarymixing_amd.nnet.attention import MultiheadAttention
    m = MultiheadAttention(1, 64)
    x = torch.randn(2, 5, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(x, x, x)
    with pytest.raises(NotImplementedError, match="pos_embs"):
        m(x, x, x, pos_embs=torch.zeros(1, 5, 64))
    with pytest.raises(TypeError, match="float16"):
        m(x.half(), x.half(), x.half())
    with pytest.raises(NotImplementedError, match="3-D attn_mask"):
        m(x, x, x, attn_mask=torch.zeros(2, 5, 5))


def test_mask_refusals_need_no_gpu():
    from summarymixing_amd import functional as F
    with pytest.raises(NotImplementedError, match="3-D"):
        F.attn_bias_of(torch.zeros(2, 5, 5), "cpu")
    with pytest.raises(TypeError, match="bool or floating"):
        F.attn_bias_of(torch.zeros(5, 5, dtype=torch.int32), "cpu")
    b = F.attn_bias_of(torch.tensor([[False, True], [False, False]]), "cpu")
    assert b.dtype == torch.float32 and b[0, 1] == float("-inf") and b[0, 0] == 0 and b[1, 1] == 0
    with pytest.raises(ValueError, match="key_padding_mask"):
        F.key_pad_u8(torch.zeros(2, 5), 2, 5, "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        q = torch.randn(1, 2, 1, 64)
        F.scaled_dot_product_attention(q, q, q)


def test_descriptor_sizes_match_header():
    from summarymixing_amd import _lib
    A, O, P = _lib.AttnArgs, _lib.AttnOperand, _lib.AttnPlan
    assert ctypes.sizeof(O) == 40 and ctypes.sizeof(A) == 448 and ctypes.sizeof(P) == 40     # include/smx.h smx_attn_*
    assert A.q.offset == 8 and A.dv.offset == 288 and A.lse.offset == 328 and A.attn_bias.offset == 344 and A.key_pad.offset == 360
    assert A.weights.offset == 376 and A.B.offset == 400 and A.scale.offset == 420 and A.drop_seed.offset == 432 and A.epoch.offset == 440
    assert P.grid.offset == 24


_BASE = 1 << 40


def _args(D=64, dtype=0, **kw):
    from summarymixing_amd import _lib
    B, L, S, H = 2, 5, 7, 2
    a = _lib.AttnArgs(dtype=dtype, B=B, L=L, S=S, H=H, D=D, scale=0.125)
    for i, n in enumerate(("q", "k", "v", "o", "dO", "dq", "dk", "dv")):
        rows = L if n in ("q", "o", "dO", "dq") else S
        setattr(a, n, _lib.AttnOperand(_BASE + i * 0x1000000, rows * H * D, H * D, D, 1))
    a.lse, a.delta = _BASE + 0x9000000, _BASE + 0xa000000
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_library_refuses_what_it_cannot_run():
    """Refused on the host before any launch (the pointers are fake and never dereferenced)."""
    from summarymixing_amd import _lib
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -2
    for fn in (lib.smx_attn_fwd, lib.smx_attn_bwd, lib.smx_attn_weights):
        assert fn(ctypes.byref(_args(D=96)), None) == EUNSUPPORTED
        assert b"96" in lib.smx_last_error()
        assert fn(ctypes.byref(_args(dtype=2)), None) == EUNSUPPORTED
    plan = _lib.AttnPlan()
    assert lib.smx_attn_plan_query(ctypes.byref(_args(D=96)), 0, ctypes.byref(plan)) == EUNSUPPORTED
    a = _args()
    a.k = _lib.AttnOperand(_BASE + 4, 7 * 128, 128, 64, 1)                       # misaligned base
    assert lib.smx_attn_fwd(ctypes.byref(a), None) == EUNSUPPORTED
    a = _args()
    a.v = _lib.AttnOperand(_BASE, 7 * 130, 130, 65, 1)                           # rows not 16-byte aligned (fp32 stride 130)
    assert lib.smx_attn_fwd(ctypes.byref(a), None) == EUNSUPPORTED
    a = _args()
    a.q = _lib.AttnOperand(_BASE, 5 * 256, 256, 128, 2)                          # D not contiguous
    assert lib.smx_attn_fwd(ctypes.byref(a), None) == EUNSUPPORTED
    a = _args(dtype=1)
    a.q = _lib.AttnOperand(_BASE, 5 * 132, 132, 66, 1)                           # bf16 head stride 66: 132 bytes
    assert lib.smx_attn_fwd(ctypes.byref(a), None) == EUNSUPPORTED
    a = _args()
    a.q = _lib.AttnOperand(None, 0, 0, 0, 1)
    assert lib.smx_attn_fwd(ctypes.byref(a), None) == EINVAL
    assert lib.smx_attn_fwd(ctypes.byref(_args(drop_p=1.0)), None) == EINVAL
    assert lib.smx_attn_fwd(ctypes.byref(_args(S=0)), None) == EINVAL
    assert lib.smx_attn_bwd(ctypes.byref(_args(delta=None)), None) == EINVAL
    assert lib.smx_attn_weights(ctypes.byref(_args()), None) == EINVAL           # no weights buffer


# (B, L, S, H, D): the shapes of tests/test_attention_gpu.py and the recipes' attention points
_PLAN_SHAPES = [(1, 1, 200, 1, 512), (3, 7, 5, 4, 64), (3, 17, 129, 2, 128), (1, 65, 65, 1, 512), (3, 33, 63, 4, 64), (1, 16, 64, 2, 128),
                (3, 16, 1, 1, 512), (32, 64, 390, 1, 512), (32, 64, 64, 4, 128), (128, 80, 125, 1, 512), (10, 1, 390, 1, 512)]


@pytest.mark.parametrize("shape", _PLAN_SHAPES, ids=["x".join(map(str, s)) for s in _PLAN_SHAPES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_plan_query_answers_without_a_gpu(shape, dtype):
    """Tile rows, key-tile width, grid and LDS bytes per pass: 16-row tiles (one MFMA tile), 64-wide tiles walked, D staged through
    LDS in chunks of at most 128 columns; every pass stays inside the 64 KiB of static LDS a workgroup may declare."""
    from summarymixing_amd import _lib, ops
    B, L, S, H, D = shape
    es, ldt = (4, 68) if dtype == torch.float32 else (2, 72)
    img, xt = 16 * ldt * es, min(D, 128) * ldt * es
    want = {_lib.ATTN_FWD: ((-(-L // 16), H, B), 16 * 68 * 4 + img + xt + 3 * 16 * 4, 1),
            _lib.ATTN_BWD_DQ: ((-(-L // 16), H, B), img + xt + 4 * 16 * 4, 2),
            _lib.ATTN_BWD_DKV: ((-(-S // 16), H, B), 2 * img + xt, 2),
            _lib.ATTN_WEIGHTS: ((-(-L // 16), -(-S // 64), B), 0, 1)}
    for which, (grid, lds, launches) in want.items():
        p = ops.attention_plan(B, L, S, H, D, dtype, which)
        assert p["rows"] == 16 and p["key_tile"] == 64 and p["d_chunk"] == min(D, 128) and p["threads"] == 256
        assert p["grid"] == grid and p["lds_bytes"] == lds and p["launches"] == launches
        assert p["lds_bytes"] <= 65536


def test_plan_query_refuses_unsupported_head_dim_and_dtype():
    from summarymixing_amd import ops
    with pytest.raises(RuntimeError, match="head dimension 96"):
        ops.attention_plan(1, 4, 4, 1, 96)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.attention_plan(1, 4, 4, 1, 64, torch.float16)

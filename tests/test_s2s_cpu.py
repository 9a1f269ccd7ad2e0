"""The host side of KV-cached seq2seq decoding, without a GPU: the descriptors of csrc/attn_step.hip against include/smx.h, what the
three entry points refuse before any launch, the launch geometry smx_attn_step_plan_query reports, and the searchers' constructors."""
import ctypes

import pytest
import torch

EINVAL, EUNSUPPORTED = -1, -2
_BASE = 1 << 40


def test_descriptor_sizes_and_offsets_match_header():
    from summarymixing_amd import _lib
    A, P, S = _lib.AttnStepArgs, _lib.AttnStepPlan, _lib.S2SSelectArgs
    assert ctypes.sizeof(A) == 288 and ctypes.sizeof(P) == 56 and ctypes.sizeof(S) == 104          # include/smx.h
    assert A.q.offset == 8 and A.k_new.offset == 48 and A.v_new.offset == 88 and A.K.offset == 128 and A.V.offset == 168 and A.o.offset == 208
    assert A.n_keys.offset == 248 and A.workspace.offset == 256 and A.B.offset == 264 and A.cap.offset == 276 and A.scale.offset == 280
    assert P.splits.offset == 16 and P.grid.offset == 32 and P.workspace_bytes.offset == 48
    assert S.ldz.offset == 8 and S.forced.offset == 16 and S.tok.offset == 24 and S.logp_tok.offset == 64 and S.inv_temp.offset == 72
    assert S.dtype.offset == 80 and S.min_steps.offset == 100


def _step_args(D=64, dtype=0, B=2, H=2, cap=40, **kw):
    from summarymixing_amd import _lib
    a = _lib.AttnStepArgs(dtype=dtype, B=B, H=H, D=D, cap=cap, scale=0.125, n_keys=_BASE + 0x8000000, workspace=_BASE + 0x9000000)
    for i, n in enumerate(("q", "k_new", "v_new", "o")):
        setattr(a, n, _lib.AttnOperand(_BASE + i * 0x1000000, 3 * H * D, 0, D, 1))
    a.K = _lib.AttnOperand(_BASE + 0x5000000, cap * 2 * H * D, 2 * H * D, D, 1)
    a.V = _lib.AttnOperand(_BASE + 0x5000000 + H * D * 4, cap * 2 * H * D, 2 * H * D, D, 1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_attn_step_refuses_what_it_cannot_run():
    """Refused on the host before any launch (the pointers are fake and never dereferenced)."""
    from summarymixing_amd import _lib
    lib = _lib.lib()
    fn = lib.smx_attn_step
    assert fn(None, None) == EINVAL
    assert fn(ctypes.byref(_step_args(D=96)), None) == EUNSUPPORTED and b"96" in lib.smx_last_error()
    assert fn(ctypes.byref(_step_args(dtype=2)), None) == EUNSUPPORTED
    assert fn(ctypes.byref(_step_args(cap=(1 << 16) + 1)), None) == EUNSUPPORTED
    for bad in (dict(B=0), dict(H=0), dict(cap=0), dict(D=0)):
        assert fn(ctypes.byref(_step_args(**bad)), None) == EINVAL, bad
    for name in ("q", "K", "V", "o"):
        assert fn(ctypes.byref(_step_args(**{name: _lib.AttnOperand(None, 0, 0, 0, 1)})), None) == EINVAL, name
    assert fn(ctypes.byref(_step_args(v_new=_lib.AttnOperand(None, 0, 0, 0, 1))), None) == EINVAL         # k_new without v_new
    assert fn(ctypes.byref(_step_args(cap=200, workspace=None)), None) == EINVAL                          # 4 chunks need the workspace
    assert fn(ctypes.byref(_step_args(K=_lib.AttnOperand(_BASE, 40 * 32, 32, 64, 1))), None) == EINVAL    # cache row stride < D
    assert fn(ctypes.byref(_step_args(q=_lib.AttnOperand(_BASE + 4, 384, 0, 64, 1))), None) == EUNSUPPORTED   # misaligned base
    assert fn(ctypes.byref(_step_args(q=_lib.AttnOperand(_BASE, 384, 0, 128, 2))), None) == EUNSUPPORTED      # D not contiguous
    assert fn(ctypes.byref(_step_args(V=_lib.AttnOperand(_BASE, 40 * 130, 130, 65, 1))), None) == EUNSUPPORTED  # rows not 16-byte aligned
    assert fn(ctypes.byref(_step_args(dtype=1, k_new=_lib.AttnOperand(_BASE, 396, 0, 66, 1))), None) == EUNSUPPORTED   # bf16 head stride 66
    plan = _lib.AttnStepPlan()
    assert lib.smx_attn_step_plan_query(ctypes.byref(_step_args(D=96)), ctypes.byref(plan)) == EUNSUPPORTED
    assert lib.smx_attn_step_plan_query(ctypes.byref(_step_args()), None) == EINVAL


def test_embed_step_and_select_refuse_what_they_cannot_run():
    from summarymixing_amd import _lib
    lib = _lib.lib()
    p = [ctypes.c_void_p(_BASE + i * 0x100000) for i in range(6)]
    tok, table, pe, Y, pos, done = p

    def embed(dtype=0, tok=tok, table=table, ldt=64, pe=pe, ldpe=64, Y=Y, ldy=64, pos=pos, done=done, B=3, V=10, D=64, max_pos=50):
        return lib.smx_s2s_embed_step(dtype, tok, table, ldt, pe, ldpe, Y, ldy, pos, done, B, V, D, max_pos, None)
    assert embed(dtype=2) == EINVAL
    for kw in (dict(tok=None), dict(table=None), dict(Y=None), dict(pos=None), dict(done=None), dict(B=0), dict(V=0), dict(D=0),
               dict(max_pos=0), dict(ldt=32), dict(ldy=32), dict(ldpe=32)):
        assert embed(**kw) == EINVAL, kw
    for kw in (dict(D=60, ldt=60, ldy=60, ldpe=60), dict(ldt=68), dict(ldy=68), dict(ldpe=68), dict(table=ctypes.c_void_p(_BASE + 4)),
               dict(Y=ctypes.c_void_p(_BASE + 8))):
        assert embed(**kw) == EUNSUPPORTED, kw

    def select(**kw):
        a = _lib.S2SSelectArgs(logits=_BASE, ldz=40, tok=_BASE + 0x1000, done=_BASE + 0x2000, n_tok=_BASE + 0x3000, score=_BASE + 0x4000,
                               tokens=_BASE + 0x5000, logp_tok=_BASE + 0x6000, inv_temp=1.0, dtype=0, B=3, V=40, cap=8, eos=2, min_steps=0)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.smx_s2s_select(ctypes.byref(a), None)
    assert lib.smx_s2s_select(None, None) == EINVAL
    for kw in (dict(dtype=2), dict(B=0), dict(V=0), dict(cap=0), dict(ldz=39), dict(inv_temp=0.0), dict(inv_temp=-1.0),
               dict(inv_temp=float("inf")), dict(logits=None), dict(tok=None), dict(done=None), dict(n_tok=None), dict(score=None),
               dict(tokens=None), dict(logp_tok=None)):
        assert select(**kw) == EINVAL, kw


# (B, H, D, cap)
_PLAN_SHAPES = [(1, 1, 512, 390), (8, 1, 512, 64), (3, 2, 64, 40), (3, 4, 128, 200), (1, 1, 256, 2500), (2, 1, 64, 65), (1, 1, 512, 1)]


@pytest.mark.parametrize("shape", _PLAN_SHAPES, ids=["x".join(map(str, s)) for s in _PLAN_SHAPES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_plan_query_answers_without_a_gpu(shape, dtype):
    """A key is shared by min(64, D / (elements per 16 bytes)) lanes; one 4-wave workgroup per chunk of keys, one chunk per 64 keys of
    cap up to 16, a second launch and (max, sum, accumulator) triples of D + 2 floats per (row, head, chunk) when there are several."""
    from summarymixing_amd import ops
    B, H, D, cap = shape
    p = ops.attention_step_plan(B, H, D, cap, dtype)
    lpk = min(64, D // (4 if dtype == torch.float32 else 8))
    splits = min(16, -(-cap // 64))
    assert p["lanes_per_key"] == lpk and p["keys_per_wave"] == 64 // lpk and p["waves"] == 4 and p["threads"] == 256
    assert p["splits"] == splits and p["chunk"] == -(-cap // splits) and p["splits"] * p["chunk"] >= cap
    assert p["launches"] == (2 if splits > 1 else 1) and p["grid"] == (splits, H, B)
    assert p["lds_bytes"] == 4 * (D + 2) * 4 <= 65536
    assert p["workspace_bytes"] == (B * H * splits * (D + 2) * 4 if splits > 1 else 0)


def test_plan_query_refuses_by_name():
    from summarymixing_amd import ops
    with pytest.raises(RuntimeError, match="head dimension 96"):
        ops.attention_step_plan(1, 1, 96, 10)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.attention_step_plan(1, 1, 64, 10, torch.float16)
    with pytest.raises(RuntimeError, match="cap"):
        ops.attention_step_plan(1, 1, 64, 1 << 17)


_RECIPE = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, using_eos_threshold=False, length_normalization=True)


def test_searcher_constructors_accept_the_recipes_arguments_and_refuse_by_name():
    from summarymixing_amd.decoders import S2STransformerBeamSearcher, S2STransformerGreedySearcher
    model, lin = torch.nn.Linear(4, 4), torch.nn.Linear(4, 3)
    s = S2STransformerBeamSearcher(modules=[model, lin], beam_size=1, **_RECIPE)                 # valid_search with valid_beam_size 1
    assert s.beam_size == 1 and s.model is model and s.fc is lin
    assert S2STransformerBeamSearcher(modules=[model, lin], beam_size=1, temperature=1.15, **_RECIPE).temperature == 1.15
    g = S2STransformerGreedySearcher([model, lin], 1, 2, 0.0, 1.0)
    for searcher in (s, g):
        assert len(searcher.state_dict()) == 0 and list(searcher.parameters()) == [] and list(searcher.children()) == []
    with pytest.raises(NotImplementedError, match="beam_size=10"):
        S2STransformerBeamSearcher(modules=[model, lin], beam_size=10, **_RECIPE)
    with pytest.raises(NotImplementedError, match="scorer"):
        S2STransformerBeamSearcher(modules=[model, lin], beam_size=1, scorer=object(), **_RECIPE)
    with pytest.raises(NotImplementedError, match="using_eos_threshold"):
        S2STransformerBeamSearcher(modules=[model, lin], beam_size=1, **{**_RECIPE, "using_eos_threshold": True})
    with pytest.raises(NotImplementedError, match="topk"):
        S2STransformerBeamSearcher(modules=[model, lin], beam_size=1, topk=5, **_RECIPE)
    for cls, kw in ((S2STransformerBeamSearcher, dict(beam_size=1)), (S2STransformerGreedySearcher, {})):
        for t in (0.0, -1.0):
            with pytest.raises(ValueError, match="temperature"):
                cls([model, lin], 1, 2, 0.0, 1.0, temperature=t, **kw)
    with pytest.raises(ValueError, match="min_decode_ratio"):
        S2STransformerGreedySearcher([model, lin], 1, 2, 0.5, 0.1)
    with pytest.raises(NotImplementedError, match="modules"):
        S2STransformerGreedySearcher([model], 1, 2, 0.0, 1.0)


def test_cpu_tensors_are_refused():
    from summarymixing_amd import ops
    from summarymixing_amd.decoders import S2STransformerGreedySearcher, greedy_search
    from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR
    s = S2STransformerGreedySearcher([torch.nn.Linear(4, 4), torch.nn.Linear(4, 3)], 1, 2, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        s(torch.zeros(2, 5, 4), torch.ones(2))
    with pytest.raises(RuntimeError, match="GPU only"):
        greedy_search(None, None, torch.zeros(2, 5, 4), None, 1, 2, 0, 5)
    q = torch.zeros(2, 1, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attention_step(q, torch.zeros(2, 4, 1, 64), torch.zeros(2, 4, 1, 64))
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.s2s_embed_step(z, torch.zeros(5, 64), None, z, torch.zeros(2, dtype=torch.uint8), 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.s2s_select(torch.zeros(2, 5), z, torch.zeros(2, dtype=torch.uint8), z, torch.zeros(2), torch.zeros(2, 4, dtype=torch.int32),
                       torch.zeros(2, 4), 1)
    m = TransformerASR(tgt_vocab=7, input_size=20, d_model=64, nhead=1, num_encoder_layers=1, num_decoder_layers=1, d_ffn=64,
                       encoder_module="branchformer", causal=False, csgu_linear_units=64, kernel_size=3, local_proj_hid_dim=[64],
                       local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64)
    with pytest.raises(RuntimeError, match="eval mode"):
        m.make_decode_state(torch.zeros(2, 5, 64))
    with pytest.raises(RuntimeError, match="eval mode"):
        m.decode_step(z, None)
    m.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        m.make_decode_state(torch.zeros(2, 5, 64))

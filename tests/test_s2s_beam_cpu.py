"""The host side of the seq2seq beam search, without a GPU: the new descriptors against include/smx.h, what smx_attn_step_rows and
smx_s2s_beam_select refuse before any launch, the indexed entry's plan query, the S2SBeamSearcher constructor, and the float64
reference of the GPU tests (tests/_s2s_beam_ref.py) on an example worked by hand."""
import ctypes
import math

import pytest
import torch

from tests import _s2s_beam_ref as R

EINVAL, EUNSUPPORTED = -1, -2
_BASE = 1 << 40


def test_descriptor_sizes_and_offsets_match_header():
    from summarymixing_amd import _lib
    A, S, Bm = _lib.AttnStepArgs, _lib.AttnStepRowsArgs, _lib.S2SBeamArgs
    assert ctypes.sizeof(A) == 288, "smx_attn_step_args is what it was"
    assert ctypes.sizeof(S) == 312 and S.s.offset == 0 and S.anc.offset == 288 and S.ld_anc.offset == 296 and S.kv_div.offset == 304
    assert ctypes.sizeof(Bm) == 296 and Bm.extra.offset == 16 and Bm.tok.offset == 32 and Bm.done_row.offset == 48 and Bm.anc.offset == 88
    assert Bm.cand_val.offset == 120 and Bm.pool_tokens.offset == 152 and Bm.res_tokens.offset == 216 and Bm.res_sum.offset == 248
    assert Bm.inv_temp.offset == 256 and Bm.dtype.offset == 264 and Bm.W.offset == 272 and Bm.length_norm.offset == 292


def _rows_args(D=64, dtype=0, B=6, H=2, cap=40, kv_div=1, anc=_BASE + 0xA000000, ld_anc=None, k_new=True):
    from summarymixing_amd import _lib
    Bc = -(-B // max(kv_div, 1))
    a = _lib.AttnStepArgs(dtype=dtype, B=B, H=H, D=D, cap=cap, scale=0.125, n_keys=_BASE + 0x8000000, workspace=_BASE + 0x9000000)
    for i, n in enumerate(("q", "k_new", "v_new", "o")):
        if k_new or n in ("q", "o"):
            setattr(a, n, _lib.AttnOperand(_BASE + i * 0x1000000, 3 * H * D, 0, D, 1))
    a.K = _lib.AttnOperand(_BASE + 0x5000000, cap * 2 * H * D if Bc > 1 else 0, 2 * H * D, D, 1)
    a.V = _lib.AttnOperand(_BASE + 0x5000000 + H * D * 4, cap * 2 * H * D if Bc > 1 else 0, 2 * H * D, D, 1)
    return _lib.AttnStepRowsArgs(s=a, anc=anc, ld_anc=cap if ld_anc is None else ld_anc, kv_div=kv_div)


def test_attn_step_rows_refuses_what_it_cannot_run():
    """Refused on the host before any launch (the pointers are fake and never dereferenced)."""
    from summarymixing_amd import _lib
    lib = _lib.lib()
    fn = lib.smx_attn_step_rows
    assert fn(None, None) == EINVAL
    assert fn(ctypes.byref(_rows_args(D=96)), None) == EUNSUPPORTED and b"96" in lib.smx_last_error()      # smx_attn_step's own checks
    assert fn(ctypes.byref(_rows_args(B=0)), None) == EINVAL
    assert fn(ctypes.byref(_rows_args(kv_div=0, anc=None, k_new=False)), None) == EINVAL and b"kv_div" in lib.smx_last_error()
    assert fn(ctypes.byref(_rows_args(kv_div=-3, anc=None, k_new=False)), None) == EINVAL
    assert fn(ctypes.byref(_rows_args(kv_div=3, k_new=False)), None) == EINVAL and b"anc" in lib.smx_last_error()      # anc with kv_div > 1
    assert fn(ctypes.byref(_rows_args(kv_div=3, anc=None)), None) == EINVAL and b"k_new" in lib.smx_last_error()      # a store with kv_div > 1
    assert fn(ctypes.byref(_rows_args(ld_anc=39)), None) == EINVAL and b"ld_anc" in lib.smx_last_error()


# (rows, H, D, cap, kv_div)
_PLAN_SHAPES = [(6, 1, 512, 390, 3), (80, 1, 512, 64, 10), (6, 4, 64, 48, 1), (6, 4, 64, 70, 1), (6, 1, 512, 130, 1), (128, 2, 128, 1, 128)]


@pytest.mark.parametrize("shape", _PLAN_SHAPES, ids=["x".join(map(str, s)) for s in _PLAN_SHAPES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_rows_plan_query_is_the_plain_plan_over_the_query_rows(shape, dtype):
    """The indexed entry has smx_attn_step's geometry: the splits are a function of cap alone, the grid and the workspace count the
    QUERY rows (B W), not the cache rows."""
    from summarymixing_amd import ops
    rows, H, D, cap, kv_div = shape
    p = ops.attention_step_plan(rows, H, D, cap, dtype, kv_div=kv_div)
    assert p == ops.attention_step_plan(rows, H, D, cap, dtype)
    splits = min(16, -(-cap // 64))
    assert p["splits"] == splits and p["grid"] == (splits, H, rows) and p["launches"] == (2 if splits > 1 else 1)
    assert p["workspace_bytes"] == (rows * H * splits * (D + 2) * 4 if splits > 1 else 0)


def test_rows_plan_query_refuses_by_name():
    from summarymixing_amd import ops
    with pytest.raises(RuntimeError, match="kv_div 0"):
        ops.attention_step_plan(6, 1, 64, 10, kv_div=0)
    with pytest.raises(RuntimeError, match="head dimension 96"):
        ops.attention_step_plan(6, 1, 96, 10, kv_div=3)


def test_beam_select_refuses_what_it_cannot_run():
    from summarymixing_amd import _lib
    lib = _lib.lib()
    ptrs = [n for n, t in _lib.S2SBeamArgs._fields_ if t is ctypes.c_void_p and n not in ("extra",)]

    def select(**kw):
        a = _lib.S2SBeamArgs(ldz=40, inv_temp=1.0, dtype=0, B=2, W=3, V=40, cap=8, eos=2, min_steps=0, length_norm=1,
                             **{n: _BASE + i * 0x100000 for i, n in enumerate(ptrs)})
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.smx_s2s_beam_select(ctypes.byref(a), None)
    assert lib.smx_s2s_beam_select(None, None) == EINVAL
    for kw in (dict(dtype=2), dict(B=0), dict(V=0), dict(cap=0), dict(ldz=39), dict(inv_temp=0.0), dict(inv_temp=float("inf")),
               dict(W=0), dict(W=129), dict(B=1 << 20, W=128), dict(extra=_BASE, ldx=39)):
        assert select(**kw) == EINVAL, kw
    assert select(W=129) == EINVAL and b"W=129" in lib.smx_last_error()
    for n in ptrs:
        assert select(**{n: None}) == EINVAL, n


_RECIPE = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, using_eos_threshold=False, length_normalization=True)


def test_beam_searcher_constructor_accepts_the_recipes_arguments_and_refuses_by_name():
    from summarymixing_amd import decoders
    from summarymixing_amd.decoders import S2SBeamSearcher, S2STransformerBeamSearcher
    assert decoders.S2SBeamSearcher is decoders.seq2seq.S2SBeamSearcher and callable(decoders.seq2seq.beam_search)
    assert decoders.seq2seq.CapturedS2SBeam is decoders.CapturedS2SBeam
    model, lin = torch.nn.Linear(4, 4), torch.nn.Linear(4, 3)
    for W in (1, 10, 66, 128):                                 # valid_beam_size 10, test_beam_size 10 / 66 / 80
        s = S2SBeamSearcher(modules=[model, lin], beam_size=W, **_RECIPE)
        assert s.beam_size == W and s.model is model and s.fc is lin and s.length_normalization is True
        assert len(s.state_dict()) == 0 and list(s.parameters()) == [] and list(s.children()) == []
    s = S2SBeamSearcher([model, lin], 1, 2, 0.0, 1.0, beam_size=10, temperature=1.15, length_normalization=False, max_attn_shift=60,
                        using_max_attn_shift=False, eos_threshold=1.5, topk=1)
    assert s.temperature == 1.15 and s.length_normalization is False
    with pytest.raises(NotImplementedError, match="scorer"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, scorer=object(), **_RECIPE)
    with pytest.raises(NotImplementedError, match="using_eos_threshold"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, **{**_RECIPE, "using_eos_threshold": True})
    with pytest.raises(NotImplementedError, match="topk=5"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, topk=5, **_RECIPE)
    with pytest.raises(NotImplementedError, match="max_attn_shift"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, using_max_attn_shift=True, **_RECIPE)
    for W in (0, -1, 129, 2.5):
        with pytest.raises(NotImplementedError, match="beam_size="):
            S2SBeamSearcher(modules=[model, lin], beam_size=W, **_RECIPE)
    with pytest.raises(TypeError, match="nonsense"):
        S2SBeamSearcher(modules=[model, lin], beam_size=10, nonsense=1, **_RECIPE)
    with pytest.raises(ValueError, match="temperature"):
        S2SBeamSearcher([model, lin], 1, 2, 0.0, 1.0, beam_size=10, temperature=0.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        s(torch.zeros(2, 5, 4), torch.ones(2))
    # the upstream names are what they were: beam search is reached through the new name alone
    with pytest.raises(NotImplementedError, match="beam_size=10"):
        S2STransformerBeamSearcher(modules=[model, lin], beam_size=10, **_RECIPE)


def test_beam_search_checks_its_arguments_before_any_launch():
    from summarymixing_amd.decoders import beam_search
    with pytest.raises(ValueError, match="beam_size"):
        beam_search(None, None, torch.zeros(2, 5, 4), None, 1, 2, 0, 5, beam_size=0)
    with pytest.raises(ValueError, match="beam_size"):
        beam_search(None, None, torch.zeros(2, 5, 4), None, 1, 2, 0, 5, beam_size=129)
    with pytest.raises(RuntimeError, match="GPU only"):
        beam_search(None, None, torch.zeros(2, 5, 4), None, 1, 2, 0, 5, beam_size=3)


def _logits(*rows):
    return torch.tensor(rows, dtype=torch.float64).log()


def test_reference_on_a_two_beam_three_token_example_worked_by_hand():
    """V = 3 (a = 0, b = 1, eos = 2), W = 2, cap = 3, length normalisation.  Probabilities are powers of two so that every product
    below is exact and the ties are real.
      step 0  from bos: p = (a .5, b .25, eos .25).  Best two: a (.5); then b and eos tie at .25 -> b, the lower flat index.
              slots: [a] .5, [b] .25.
      step 1  after [a]: (a .25, b .125, eos .625); after [b]: (a .5, b .25, eos .25).
              candidates: a eos .3125 | a a .125 | b a .125 | a b .0625 | b b .0625 | b eos .0625.
              Best two: a eos (.3125) -> the pool, length 2, final ln(.3125) / 2; its slot 0 is dead.  Then a a and b a tie at .125 ->
              a a (flat index 0 before 3).  slots: dead, [a a] .125.  One pool entry < W: the utterance goes on.
      step 2  n + 1 == cap.  after [a a] (slot 1): (a .5, b .25, eos .25).  candidates a a a .0625 | a a b .03125 | a a eos .03125.
              Best two: a a a, then a a b (flat 1 * 3 + 1 before 1 * 3 + 2).  Both enter the pool as they are: a a a fills it
              (final ln(.0625) / 3 = -0.924); a a b (ln(.03125) / 3 = -1.155) is not better than the worst entry and is refused.
      result  [a eos] final -0.5816, [a a a] final -0.9242."""
    ref = R.BeamRef(1, 2, 3, 3, eos=2)
    out = ref.step(_logits([.5, .25, .25], [1 / 3, 1 / 3, 1 / 3]))[0]         # (slot 1 is dead at n = 0: its row is not read)
    assert [(p, v) for p, v, _, _ in out["winners"]] == [(0, 0), (0, 1)] and out["gaps"][1] == 0.0
    assert ref.tokens[0] == [[0], [1]] and ref.score[0].tolist() == [math.log(.5), math.log(.25)] and ref.anc[0] == [[0], [0]]
    out = ref.step(_logits([.25, .125, .625], [.5, .25, .25]))[0]
    assert [(p, v) for p, v, _, _ in out["winners"]] == [(0, 2), (0, 0)]
    assert not ref.alive(0, 0) and ref.alive(0, 1) and ref.tokens[0][1] == [0, 0] and ref.anc[0][1] == [0, 0] and ref.tok[0] == [2, 0]
    assert float(ref.score[0, 1]) == pytest.approx(math.log(.125), abs=1e-15) and not ref.done[0] and len(ref.pool[0]) == 1
    out = ref.step(_logits([1 / 3, 1 / 3, 1 / 3], [.5, .25, .25]))[0]
    assert [(p, v) for p, v, _, _ in out["winners"]] == [(1, 0), (1, 1)]
    assert ref.done[0] and ref.step(_logits([.5, .25, .25], [.5, .25, .25])) == [None], "a finished utterance changes nothing"
    best, second = ref.result(0)
    assert best["tokens"] == [0, 2] and best["final"] == pytest.approx(math.log(.3125) / 2, abs=1e-15) and best["sum"] == pytest.approx(math.log(.3125), abs=1e-15)
    assert second["tokens"] == [0, 0, 0] and second["final"] == pytest.approx(math.log(.0625) / 3, abs=1e-15)
    assert best["lps"] == pytest.approx([math.log(.5), math.log(.625)], abs=1e-15)
    # without length normalisation the finals are the sums
    ref = R.BeamRef(1, 2, 3, 3, eos=2, length_norm=False)
    for rows in (([.5, .25, .25], [.5, .25, .25]), ([.25, .125, .625], [.5, .25, .25]), ([.5, .25, .25], [.5, .25, .25])):
        ref.step(_logits(*rows))
    assert [e["final"] for e in ref.result(0)] == pytest.approx([math.log(.3125), math.log(.0625)], abs=1e-15)
    # eos is no candidate below min_steps: step 1's best, a eos, is out and the two .125 candidates win
    ref = R.BeamRef(1, 2, 3, 3, eos=2, min_steps=2)
    ref.step(_logits([.5, .25, .25], [.5, .25, .25]))
    out = ref.step(_logits([.25, .125, .625], [.5, .25, .25]))[0]
    assert [(p, v) for p, v, _, _ in out["winners"]] == [(0, 0), (1, 0)] and len(ref.pool[0]) == 0


def test_reference_search_driver_feeds_whole_prefixes():
    """search() hands the prefixes of every slot, bos first, to the logits function; with logits that depend on the last token alone
    the result can be read off: from bos (1) the chain 1 -> 0 -> 2 (eos) is the best path."""
    table = torch.tensor([[.1, .1, .8], [.7, .2, .1], [.3, .3, .4]], dtype=torch.float64).log()      # row: the last token
    seen = []

    def logits_of(prefixes):
        seen.append(tuple(prefixes.shape))
        assert bool((prefixes[:, 0] == 1).all())
        return table[prefixes[:, -1]]
    ref, trace = R.search(logits_of, 1, 2, 3, bos=1, eos=2, min_steps=0, max_steps=4)
    assert seen[0] == (2, 1) and seen[1] == (2, 2) and len(trace) == len(seen)
    assert ref.result(0)[0]["tokens"] == [0, 2] and ref.result(0)[0]["sum"] == pytest.approx(math.log(.7 * .8), abs=1e-15)

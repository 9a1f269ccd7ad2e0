"""The seq2seq decoder without a GPU: the drop-in surface (state_dict keys and shapes, strict load from torch.nn modules, what an
encoder-only model keeps), upstream's mask values, every refusal by name, the no-CPU error, the float64 restatement the GPU tests
compare against, and the host side of the two new C entry points."""
import ctypes
import json
import os

import pytest
import torch
from torch import nn

from tests import _decoder_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the call whose encoder-only keys / values tests/golden/decoder_state_keys.json records (seed 0, written before the decoder existed)
KW = dict(tgt_vocab=13, input_size=20, d_model=64, nhead=1, num_encoder_layers=1, d_ffn=128, dropout=0.0, activation=nn.GELU,
          encoder_module="branchformer", normalize_before=True, causal=False, csgu_linear_units=128, kernel_size=3,
          local_proj_hid_dim=[64], local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64)


def _asr(**kw):
    from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR
    return TransformerASR(**{**KW, **kw})


def _layer_keys(pfx, d, f):
    k = {}
    for a in ("self_attn", "multihead_attn"):
        k[f"{pfx}{a}.att.in_proj_weight"] = (3 * d, d)
        k[f"{pfx}{a}.att.in_proj_bias"] = (3 * d,)
        k[f"{pfx}{a}.att.out_proj.weight"] = (d, d)
        k[f"{pfx}{a}.att.out_proj.bias"] = (d,)
    k[pfx + "pos_ffn.ffn.0.weight"], k[pfx + "pos_ffn.ffn.0.bias"] = (f, d), (f,)
    k[pfx + "pos_ffn.ffn.3.weight"], k[pfx + "pos_ffn.ffn.3.bias"] = (d, f), (d,)
    for n in ("norm1", "norm2", "norm3"):
        k[f"{pfx}{n}.norm.weight"], k[f"{pfx}{n}.norm.bias"] = (d,), (d,)
    return k


def _decoder_keys(pfx, layers, d, f):
    k = {}
    for i in range(layers):
        k.update(_layer_keys(f"{pfx}layers.{i}.", d, f))
    k[pfx + "norm.norm.weight"], k[pfx + "norm.norm.bias"] = (d,), (d,)
    return k


def test_state_dict_keys_and_shapes_with_a_decoder():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "decoder_state_keys.json")))["encoder_only"]
    m = _asr(num_decoder_layers=2)
    want = {k: tuple(v[0]) for k, v in golden.items()}
    want.update(_decoder_keys("decoder.", 2, 64, 128))
    want["custom_tgt_module.layers.0.emb.Embedding.weight"] = (13, 64)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want, sorted(set(got.items()) ^ set(want.items()))
    for layer in m.decoder.layers:
        assert layer.norm1.norm.eps == layer.norm2.norm.eps == layer.norm3.norm.eps == 1e-6
    assert m.decoder.norm.norm.eps == 1e-6
    # registered where upstream registers them: the closing xavier_normal_ loop covered the decoder and the embedding table
    assert float(m.custom_tgt_module.layers[0].emb.Embedding.weight.detach()[0].abs().sum()) > 0.0
    w = m.decoder.layers[0].self_attn.att.in_proj_weight
    assert abs(float(w.std()) - (2.0 / (64 + 192)) ** 0.5) < 0.1 * (2.0 / (64 + 192)) ** 0.5


def test_encoder_only_model_is_what_it_was():
    """num_decoder_layers=0: the same keys, shapes, RNG draws and values as before the decoder existed (the fixture holds every
    tensor's shape and sum of magnitudes under seed 0; xavier_normal_ on the CPU is deterministic, the bar is float32 summation noise)."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "decoder_state_keys.json")))["encoder_only"]
    torch.manual_seed(0)
    m = _asr(num_decoder_layers=0)
    sd = m.state_dict()
    assert list(sd) == list(golden)
    assert not hasattr(m, "decoder") and not hasattr(m, "custom_tgt_module")
    for k, (shape, s) in golden.items():
        assert list(sd[k].shape) == shape, k
        assert abs(float(sd[k].double().abs().sum()) - s) <= 1e-9 * max(1.0, abs(s)), k


def test_torch_modules_load_strict_under_the_package_keys():
    d, f, V = 64, 128, 13
    m = _asr(num_decoder_layers=2)
    sd = {k: v for k, v in m.state_dict().items() if not (k.startswith("decoder.") or k.startswith("custom_tgt_module."))}
    torch.manual_seed(5)
    src = {}
    for i in range(2):
        p = f"decoder.layers.{i}."
        for a in ("self_attn", "multihead_attn"):
            src.update({f"{p}{a}.att.{k}": v for k, v in nn.MultiheadAttention(d, 1, batch_first=True).state_dict().items()})
        src.update({f"{p}pos_ffn.ffn.0.{k}": v for k, v in nn.Linear(d, f).state_dict().items()})
        src.update({f"{p}pos_ffn.ffn.3.{k}": v for k, v in nn.Linear(f, d).state_dict().items()})
        for n in ("norm1", "norm2", "norm3"):
            src.update({f"{p}{n}.norm.{k}": v + 0.5 for k, v in nn.LayerNorm(d).state_dict().items()})
    src.update({f"decoder.norm.norm.{k}": v for k, v in nn.LayerNorm(d).state_dict().items()})
    src.update({f"custom_tgt_module.layers.0.emb.Embedding.{k}": v for k, v in nn.Embedding(V, d, padding_idx=0).state_dict().items()})
    m.load_state_dict({**sd, **src}, strict=True)
    assert torch.equal(m.decoder.layers[1].multihead_attn.att.in_proj_weight, src["decoder.layers.1.multihead_attn.att.in_proj_weight"])
    assert torch.equal(m.decoder.layers[0].norm2.norm.bias, src["decoder.layers.0.norm2.norm.bias"])
    assert torch.equal(m.custom_tgt_module.layers[0].emb.Embedding.weight, src["custom_tgt_module.layers.0.emb.Embedding.weight"])


def test_stand_alone_modules_have_upstream_keys():
    from summarymixing_amd.lobes.models.transformer.Transformer import NormalizedEmbedding, TransformerDecoder, TransformerDecoderLayer
    assert {k: tuple(v.shape) for k, v in NormalizedEmbedding(512, 1000).state_dict().items()} == {"emb.Embedding.weight": (1000, 512)}
    layer = TransformerDecoderLayer(1024, 8, d_model=512)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == _layer_keys("", 512, 1024)
    dec = TransformerDecoder(1, 8, 1024, d_model=512)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == _decoder_keys("", 1, 512, 1024)
    from summarymixing_amd.lobes.models.transformer import TransformerASR as T
    assert T.PositionalEncoding(64, 10).pe.shape == (1, 10, 64)           # still importable from where it lived


def test_mask_builders_keep_upstream_values():
    """The docstring examples of Transformer.py:1024-1090 and TransformerASR.py:113-180."""
    from summarymixing_amd.lobes.models.transformer.Transformer import get_key_padding_mask, get_lookahead_mask
    from summarymixing_amd.lobes.models.transformer.TransformerASR import make_transformer_src_tgt_masks
    a = torch.LongTensor([[1, 1, 0], [2, 3, 0], [4, 5, 0]])
    want = torch.tensor([[False, False, True]] * 3)
    assert torch.equal(get_key_padding_mask(a, pad_idx=0), want)
    inf = float("inf")
    look = torch.tensor([[0.0, -inf, -inf], [0.0, 0.0, -inf], [0.0, 0.0, 0.0]])
    got = get_lookahead_mask(a)
    assert got.dtype == torch.float32 and torch.equal(got, look)
    assert torch.equal(DR.lookahead_mask(3, torch.float32), look) and torch.equal(DR.key_padding_mask(a, 0), want)
    src = torch.zeros(3, 4, 20)
    skpm, tkpm, smask, tmask = make_transformer_src_tgt_masks(src, a, wav_len=torch.tensor([1.0, 0.5, 0.75]), pad_idx=0)
    assert torch.equal(skpm, torch.tensor([[False] * 4, [False, False, True, True], [False, False, False, True]]))
    assert torch.equal(tkpm, want) and smask is None and torch.equal(tmask, look)
    skpm, tkpm, smask, tmask = make_transformer_src_tgt_masks(src, a, pad_idx=5)
    assert skpm is None and torch.equal(tkpm, a == 5)
    # a 3-D input: padded where every channel equals pad_idx
    x3 = torch.zeros(2, 3, 4)
    x3[0, 1, 2] = 1.0
    assert torch.equal(get_key_padding_mask(x3, 0), torch.tensor([[True, False, True], [True, True, True]]))
    # without targets: what it returned before
    assert make_transformer_src_tgt_masks(src, None, wav_len=None) == (None, None, None, None)


def test_refusals_by_name():
    from summarymixing_amd.lobes.models.transformer.Transformer import NormalizedEmbedding, TransformerDecoder, TransformerDecoderLayer
    from summarymixing_amd.nnet.embedding import Embedding
    with pytest.raises(NotImplementedError, match="RelPosMHAXL"):
        TransformerDecoderLayer(128, 1, 64, attention_type="RelPosMHAXL")
    with pytest.raises(NotImplementedError, match="RelPosMHAXL"):
        TransformerDecoder(1, 1, 128, 64, attention_type="RelPosMHAXL")
    with pytest.raises(NotImplementedError, match="kdim"):
        TransformerDecoderLayer(128, 1, 64, kdim=32)
    with pytest.raises(NotImplementedError, match="vdim"):
        TransformerDecoderLayer(128, 1, 64, vdim=32)
    with pytest.raises(NotImplementedError, match="head dimension"):
        TransformerDecoderLayer(128, 4, 64)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        NormalizedEmbedding(36, 10)
    with pytest.raises(NotImplementedError):                   # the trainable table lives in a private holder: this stays refused
        Embedding(10, 64, consider_as_one_hot=False)
    layer = TransformerDecoderLayer(128, 1, 64)
    x, mem = torch.randn(2, 5, 64), torch.randn(2, 7, 64)
    with pytest.raises(NotImplementedError, match="pos_embs_tgt"):
        layer(x, mem, pos_embs_tgt=torch.zeros(1, 5, 64))
    with pytest.raises(NotImplementedError, match="pos_embs"):
        TransformerDecoder(1, 1, 128, 64)(x, mem, pos_embs_src=torch.zeros(1, 7, 64))
    # the head dimension is checked only when a decoder is requested
    with pytest.raises(NotImplementedError, match=r"head dimension d_model / nhead = 64/4"):
        _asr(num_decoder_layers=1, nhead=4)
    _asr(num_decoder_layers=0, nhead=4)


def test_cpu_tensors_raise_the_no_cpu_error():
    from summarymixing_amd import ops
    from summarymixing_amd.lobes.models.transformer.Transformer import NormalizedEmbedding, TransformerDecoder, TransformerDecoderLayer
    x, mem = torch.randn(2, 5, 64), torch.randn(2, 7, 64)
    tok = torch.randint(0, 13, (2, 5))
    with pytest.raises(RuntimeError, match="GPU only"):
        TransformerDecoderLayer(128, 1, 64)(x, mem)
    with pytest.raises(RuntimeError, match="GPU only"):
        TransformerDecoder(1, 1, 128, 64)(x, mem)
    with pytest.raises(RuntimeError, match="GPU only"):
        NormalizedEmbedding(64, 13)(tok)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.tgt_embed_fwd(tok, torch.zeros(13, 64), torch.zeros(5, 64))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.tgt_embed_bwd(tok, torch.zeros(10, 64), torch.zeros(13, 64))
    m = _asr(num_decoder_layers=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(torch.randn(2, 8, 20), tok)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.decode(tok, mem)


def test_target_checks_come_before_any_launch():
    m = _asr(num_decoder_layers=1, max_length=6)
    with pytest.raises(ValueError, match="max_length 6"):
        m(torch.randn(2, 4, 20), torch.zeros(2, 7, dtype=torch.long))
    with pytest.raises(ValueError, match="max_length 6"):
        m.decode(torch.zeros(2, 7, dtype=torch.long), torch.randn(2, 4, 64))
    with pytest.raises(ValueError, match="integer tokens"):
        m(torch.randn(2, 4, 20), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="num_decoder_layers=0"):
        _asr(num_decoder_layers=0)(torch.randn(2, 4, 20), torch.zeros(2, 3, dtype=torch.long))


def test_abi_declares_and_exports_the_embedding_entry_points():
    from summarymixing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "smx.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("smx_tgt_embed_fwd", "smx_tgt_embed_bwd"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name)
    assert "Transformer.py:991-1021" in hdr and "Transformer.py:1024-1060" in hdr and "TransformerASR.py:430" in hdr


_BASE = 1 << 40


def test_entry_points_refuse_on_the_host():
    """Refused before any launch (the pointers are fake and never dereferenced): a null pointer and V <= 0 are SMX_EINVAL, d not a
    multiple of 8 elements (no 16-byte rows) SMX_EUNSUPPORTED."""
    from summarymixing_amd import _lib
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -2
    tok, table, pe, y, flags = (_BASE + i * 0x1000000 for i in range(5))

    def fwd(dtype=_lib.F32, tok=tok, table=table, pe=pe, y=y, flags=flags, rows=10, U=5, V=13, D=64, ld=None):
        ld = D if ld is None else ld
        return lib.smx_tgt_embed_fwd(dtype, tok, table, ld, pe, ld, y, ld, flags, rows, U, V, D, 0, None)

    def bwd(dtype=_lib.F32, tok=tok, dy=y, g=table, rows=10, V=13, D=64, ld=None):
        ld = D if ld is None else ld
        return lib.smx_tgt_embed_bwd(dtype, tok, dy, ld, g, ld, rows, V, D, 0, None)
    for kw in (dict(tok=None), dict(table=None), dict(pe=None), dict(y=None), dict(flags=None), dict(V=0), dict(V=-3), dict(U=0),
               dict(rows=-1), dict(D=0), dict(dtype=2), dict(ld=32)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(D=36), dict(D=68), dict(D=4), dict(table=_BASE + 8), dict(y=_BASE + 4), dict(ld=68), dict(dtype=_lib.BF16, D=60)):
        assert fwd(**kw) == EUNSUPPORTED, kw
    assert b"multiples of 8" in lib.smx_last_error()
    for kw in (dict(tok=None), dict(dy=None), dict(g=None), dict(V=0), dict(rows=-1), dict(D=0), dict(dtype=3), dict(ld=8)):
        assert bwd(**kw) == EINVAL, kw
    for kw in (dict(D=36), dict(D=12), dict(dy=_BASE + 8), dict(g=_BASE + 4), dict(ld=68), dict(dtype=_lib.BF16, D=100)):
        assert bwd(**kw) == EUNSUPPORTED, kw
    assert fwd(rows=0) == 0 and bwd(rows=0) == 0                           # nothing to do: no launch, no error


def test_ffn_module_keeps_its_default_eps():
    import inspect
    from summarymixing_amd import functional as F
    assert inspect.signature(F.ffn_module_fwd).parameters["eps"].default == 1e-5


def test_restatement_equals_a_torch_nn_chain():
    """tests/_decoder_ref.py in float64 against torch.nn modules wired by hand in upstream's two orders, causal + padded targets
    + padded memory, (B, U, S, d, H) = (2, 5, 7, 16, 2): both are float64 and differ in summation order only - 1e-12 of the largest
    value, as tests/test_attention_cpu.py argues for the attention alone.  The two flavours of the restatement agree likewise."""
    B, U, S, d, H, f = 2, 5, 7, 16, 2, 24
    torch.manual_seed(11)
    sa, ca = nn.MultiheadAttention(d, H, batch_first=True).double(), nn.MultiheadAttention(d, H, batch_first=True).double()
    l0, l3 = nn.Linear(d, f).double(), nn.Linear(f, d).double()
    norms = [nn.LayerNorm(d, eps=1e-6).double() for _ in range(3)]
    with torch.no_grad():
        for m in (sa, ca):
            m.in_proj_bias.normal_(0.0, 0.1)
        for n in norms:
            n.weight.normal_(1.0, 0.1)
            n.bias.normal_(0.0, 0.1)
    P = {}
    for name, m in (("self_attn", sa), ("multihead_attn", ca)):
        P.update({f"{name}.att.{k}": v for k, v in m.state_dict().items()})
    P.update({f"pos_ffn.ffn.0.{k}": v for k, v in l0.state_dict().items()})
    P.update({f"pos_ffn.ffn.3.{k}": v for k, v in l3.state_dict().items()})
    for i, n in enumerate(norms):
        P.update({f"norm{i + 1}.norm.{k}": v for k, v in n.state_dict().items()})
    x, mem = torch.randn(B, U, d, dtype=torch.float64), torch.randn(B, S, d, dtype=torch.float64)
    tpad = torch.tensor([[False] * 5, [False, False, False, True, True]])
    mpad = torch.tensor([[False] * 7, [False] * 4 + [True] * 3])
    look = torch.triu(torch.ones(U, U, dtype=torch.bool), diagonal=1)
    for pre in (True, False):
        t = x
        t1 = norms[0](t) if pre else t
        t = t + sa(t1, t1, t1, attn_mask=look, key_padding_mask=tpad)[0]
        t = t if pre else norms[0](t)
        t1 = norms[1](t) if pre else t
        t2, w = ca(t1, mem, mem, key_padding_mask=mpad)
        t = t + t2
        t = t if pre else norms[1](t)
        t1 = norms[2](t) if pre else t
        t = t + l3(torch.relu(l0(t1)))
        t = t if pre else norms[2](t)
        for impl in ("f64", "aten"):
            out, _, caw = DR.decoder_layer(x, mem, P, "", H, "relu", pre, causal=True, tgt_pad=tpad, mem_pad=mpad, impl=impl)
            assert float((out - t).abs().max() / t.abs().max()) <= 1e-12 and float((caw - w).abs().max()) <= 1e-12, (pre, impl)
    # embedding + positional rows, an out-of-range token reading as a zero row
    table, pe = torch.randn(6, d, dtype=torch.float64), torch.randn(9, d, dtype=torch.float64)
    tok = torch.tensor([[1, 0, 5], [6, -1, 2]])
    y = DR.embed(tok, table, pe)
    assert torch.equal(y[0, 0], table[1] * 4.0 + pe[0]) and torch.equal(y[1, 0], pe[0]) and torch.equal(y[1, 1], pe[1])

"""TransformerDecoderLayer / TransformerDecoder / TransformerASR.forward / decode on the GPU against the float64 restatement of
tests/_decoder_ref.py, float32 and bfloat16 (the parameters and inputs are rounded to the dtype first, so all three sides start from
the same numbers).

Error bar (tests/test_attention_gpu.py's, no constants): the ATen chain of tests/_decoder_ref.py (impl="aten": F.embedding,
F.multi_head_attention_forward, F.layer_norm, F.linear at the same dtype, on the same GPU and inputs) is measured against float64
beside ours; ours <= 4 x ATen's, floor 8 eps(dtype) where ATen's error is 0.  Every pair goes through tests/_util.report
(profiles/decoder_parity_errors.jsonl holds the first run)."""
import pytest
import torch
from torch import nn

from tests import _decoder_ref as DR

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ACT = {"gelu": nn.GELU, "relu": nn.ReLU}


def _randomise(module, dtype, seed):
    """Non-trivial biases and LayerNorm parameters (the constructors leave them at 0 / 1); everything rounded to `dtype`."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if name.endswith("norm.weight") else 0.0))
            p.copy_(p.to(dtype).float())
    return module


def _params(module, prefix=""):
    return {k: v.detach() for k, v in module.state_dict().items() if k.startswith(prefix)}


def _leaf(t, dtype, device):
    return t.detach().to(device=device, dtype=dtype).requires_grad_(True)


def _pads(B, U, S):
    """Targets padded at the tail (never position 0), memory key lengths S, S / 2, 1 cycled."""
    tpad = torch.zeros(B, U, dtype=torch.bool)
    mpad = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        tpad[b, max(1, U - 2 * b):] = b > 0
        mpad[b, [S, max(1, S // 2), 1][b % 3]:] = True
    return tpad, mpad


def _grads(P):
    return {"d " + k: v.grad for k, v in P.items()}


def _three_ways(name, dtype, module, fn_ref, x, mem, r, prefix=""):
    """fn_ref(x, mem, P, impl) -> out.  Runs float64 on the CPU and the ATen chain on the GPU, collects outputs and every gradient;
    -> (ref, aten) dicts with keys out, dtgt, dmem, 'd <parameter>'."""
    sd = _params(module, prefix)
    res = []
    for impl, dt, dev in (("f64", torch.float64, "cpu"), ("aten", dtype, "cuda")):
        P = {k[len(prefix):]: _leaf(v, dt, dev) for k, v in sd.items()}
        xi, mi = _leaf(x, dt, dev), _leaf(mem, dt, dev)
        out = fn_ref(xi, mi, P, impl)
        (out * r.to(device=dev, dtype=dt)).sum().backward()
        res.append({"out": out.detach(), "dtgt": xi.grad, "dmem": mi.grad, **_grads(P)})
    return res


def _ours(module, out, xg, mg, prefix=""):
    d = {"out": out.detach(), "dtgt": xg.grad, "dmem": mg.grad}
    for k, p in module.named_parameters():
        if k.startswith(prefix):
            d["d " + k[len(prefix):]] = p.grad
    return d


# (B, U, S, d, H, d_ffn)
_LAYER_SHAPES = {"small": (3, 17, 65, 64, 1, 128), "recipe-width": (2, 9, 33, 512, 1, 256)}
_LAYER_CASES = [("small", pre, act) for pre in (True, False) for act in ("gelu", "relu")] + [("recipe-width", True, "gelu")]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", _LAYER_CASES, ids=[f"{s}-{'pre' if p else 'post'}-{a}" for s, p, a in _LAYER_CASES])
def test_decoder_layer_matches_float64_within_aten_bar(case, dt):
    """Causal mask + target padding + memory padding; output, dL/dtgt, dL/dmemory and every parameter gradient.  The GELU cases hand
    the look-ahead mask over as LOOKAHEAD (the kernels' causal flag), the ReLU cases as upstream's dense float matrix (additive bias)."""
    from summarymixing_amd.lobes.models.transformer.Transformer import LOOKAHEAD, TransformerDecoderLayer, get_lookahead_mask
    shape, pre, act = case
    B, U, S, d, H, f = _LAYER_SHAPES[shape]
    dtype = DT[dt]
    torch.manual_seed(3)
    layer = _randomise(TransformerDecoderLayer(f, H, d, activation=ACT[act], normalize_before=pre), dtype, 4).cuda()
    g = torch.Generator().manual_seed(B * U + S)
    x, mem, r = (torch.randn(B, n, d, generator=g).to(dtype).float() for n in (U, S, U))
    tpad, mpad = _pads(B, U, S)
    xg, mg = _leaf(x, dtype, "cuda"), _leaf(mem, dtype, "cuda")
    mask = LOOKAHEAD if act == "gelu" else get_lookahead_mask(xg)
    out, sa, ca = layer(xg, mg, tgt_mask=mask, tgt_key_padding_mask=tpad.cuda(), memory_key_padding_mask=mpad.cuda())
    assert out.dtype == dtype and tuple(sa.shape) == (B, U, U) and tuple(ca.shape) == (B, U, S)
    (out * r.cuda().to(dtype)).sum().backward()
    kept = {}

    def fn(xi, mi, P, impl):
        o, s_, c_ = DR.decoder_layer(xi, mi, P, "", H, act, pre, causal=True, tgt_pad=tpad.to(xi.device), mem_pad=mpad.to(xi.device),
                                     impl=impl)
        kept[impl] = (s_.detach(), c_.detach())
        return o
    ref, aten = _three_ways("layer", dtype, layer, fn, x, mem, r)
    ours = _ours(layer, out, xg, mg)
    for i, k in enumerate(("self weights", "cross weights")):
        ours[k], ref[k], aten[k] = (sa, ca)[i], kept["f64"][i], kept["aten"][i].float()
    DR.judge(f"decoder_layer {shape} {'pre' if pre else 'post'} {act} {dt}", dtype, ours, aten, ref)
    assert torch.equal(ca.cpu() == 0, mpad[:, None, :].expand(B, U, S)), "masked keys carry exact zeros, visible ones do not"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_two_layer_decoder_matches_float64_within_aten_bar(dt):
    from summarymixing_amd.lobes.models.transformer.Transformer import LOOKAHEAD, TransformerDecoder
    B, U, S, d, H, f = 3, 17, 65, 256, 4, 512
    dtype = DT[dt]
    torch.manual_seed(5)
    dec = _randomise(TransformerDecoder(2, H, f, d, activation=nn.GELU, normalize_before=True, causal=True), dtype, 6).cuda()
    g = torch.Generator().manual_seed(9)
    x, mem, r = (torch.randn(B, n, d, generator=g).to(dtype).float() for n in (U, S, U))
    tpad, mpad = _pads(B, U, S)
    xg, mg = _leaf(x, dtype, "cuda"), _leaf(mem, dtype, "cuda")
    out, sas, cas = dec(xg, mg, tgt_mask=LOOKAHEAD, tgt_key_padding_mask=tpad.cuda(), memory_key_padding_mask=mpad.cuda())
    assert out.dtype == dtype and len(sas) == 2 and len(cas) == 2 and tuple(cas[1].shape) == (B, U, S)
    (out * r.cuda().to(dtype)).sum().backward()

    def fn(xi, mi, P, impl):
        return DR.decoder(xi, mi, P, "", 2, H, "gelu", True, impl=impl, causal=True, tgt_pad=tpad.to(xi.device),
                          mem_pad=mpad.to(xi.device))[0]
    ref, aten = _three_ways("decoder", dtype, dec, fn, x, mem, r)
    DR.judge(f"decoder 2 layers {dt}", dtype, _ours(dec, out, xg, mg), aten, ref)


_ASR = dict(tgt_vocab=13, input_size=20, d_model=64, nhead=1, num_encoder_layers=1, num_decoder_layers=2, d_ffn=128, activation=nn.GELU,
            encoder_module="branchformer", normalize_before=True, causal=False, csgu_linear_units=128, kernel_size=3,
            local_proj_hid_dim=[64], local_proj_out_dim=64, summary_hid_dim=[64], summary_out_dim=64)
_B, _T, _U, _V = 3, 40, 12, 13


def _asr(dtype, dropout=0.0, seed=7):
    from summarymixing_amd.lobes.models.transformer.TransformerASR import TransformerASR
    torch.manual_seed(seed)
    m = TransformerASR(dropout=dropout, **_ASR)
    for part in (m.decoder, m.custom_tgt_module):
        _randomise(part, dtype, seed + 1)
    if dropout == 0.0:
        for layer in m.encoder.layers:                       # the SummaryMixing cell keeps its own global_dropout = 0.1 whatever
            layer.mha_layer.global_dropout = 0.0             # `dropout` is, as upstream: a dropout-free model needs it cleared too
    return m.cuda()


def _asr_inputs(dtype):
    g = torch.Generator().manual_seed(21)
    src = torch.randn(_B, _T, 20, generator=g).cuda().to(dtype)
    tgt = torch.randint(1, _V, (_B, _U), generator=g)
    tgt[1, 9:] = 0
    tgt[2, 5:] = 0
    wav_len = torch.tensor([1.0, 0.6, 0.8])
    r = torch.randn(_B, _U, 64, generator=g).to(dtype).float()
    return src, tgt, wav_len, r


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_transformer_asr_forward_matches_float64_within_aten_bar(dt):
    """encoder_out is encode()'s, bit for bit; decoder_out and every decoder-side gradient - the embedding table and the gradient
    reaching encoder_out included - against float64 run on OUR encoder_out."""
    from summarymixing_amd.lobes.models.transformer.TransformerASR import length_to_mask
    dtype = DT[dt]
    m = _asr(dtype).train()
    src, tgt, wav_len, r = _asr_inputs(dtype)
    enc, dec = m(src, tgt.cuda(), wav_len.cuda())
    assert torch.equal(enc, m.encode(src, wav_len.cuda(), masked_false_or_true=False))
    assert dec.dtype == dtype and tuple(dec.shape) == (_B, _U, 64)
    assert m(src, None, wav_len.cuda())[1] is None
    enc.retain_grad()
    (dec * r.cuda().to(dtype)).sum().backward()
    tpad = tgt == 0
    mpad = ~length_to_mask(torch.round(wav_len * _T), _T)
    pe = m.positional_encoding.pe[0].detach().cpu()
    sd = {**_params(m, "decoder."), **_params(m, "custom_tgt_module.")}
    tk = "custom_tgt_module.layers.0.emb.Embedding.weight"
    res = []
    for impl, dt_, dev in (("f64", torch.float64, "cpu"), ("aten", dtype, "cuda")):
        P = {k: _leaf(v, torch.float64 if impl == "f64" else (torch.float32 if k == tk else dtype), dev) for k, v in sd.items()}
        mem = _leaf(enc, dt_, dev)
        x = DR.embed(tgt.to(dev), P[tk], pe.to(device=dev, dtype=P[tk].dtype)).to(dt_)        # (the table and the sum stay float32 in ATen)
        out = DR.decoder(x, mem, P, "decoder.", 2, 1, "gelu", True, impl=impl, causal=True, tgt_pad=tpad.to(dev), mem_pad=mpad.to(dev))[0]
        (out * r.to(device=dev, dtype=dt_)).sum().backward()
        P[tk].grad[0] = 0.0                              # nn.Embedding(padding_idx=0): the row receives nothing
        res.append({"decoder_out": out.detach(), "d encoder_out": mem.grad, **_grads(P)})
    ref, aten = res
    ours = {"decoder_out": dec.detach(), "d encoder_out": enc.grad}
    for k, p in m.named_parameters():
        if k in sd:
            ours["d " + k] = p.grad
    assert float(ours["d " + tk][0].abs().max()) == 0.0
    DR.judge(f"TransformerASR.forward {dt}", dtype, ours, aten, ref)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_decode_equals_forward_and_is_causal(dt):
    dtype = DT[dt]
    m = _asr(dtype).eval()
    src, tgt, wav_len, _ = _asr_inputs(dtype)
    tgt = tgt.cuda()
    with torch.no_grad():
        # a pad_idx no token has: forward's target padding mask is empty, like decode's (which builds none)
        enc, dec = m(src, tgt, wav_len.cuda(), pad_idx=_V + 5)
    enc_len = torch.round(wav_len * _T).cuda()
    pred, w = m.decode(tgt, enc, enc_len)
    assert torch.equal(pred, dec)
    assert not pred.requires_grad and tuple(w.shape) == (_B, _U, _T) and w.dtype == torch.float32
    valid = (torch.arange(_T, device="cuda")[None, :] < enc_len[:, None])[:, None, :].expand(_B, _U, _T)
    assert torch.equal(w != 0, valid), "exact zeros on the padded keys only"
    # rows sum to 1 over the unmasked keys: float32 softmax, at most T terms of relative error ~eps each
    assert float((w.sum(-1) - 1.0).abs().max()) <= 4 * _T * torch.finfo(torch.float32).eps
    for j in (1, 5, _U - 1):
        t2 = tgt.clone()
        t2[:, j:] = (t2[:, j:] + 3) % _V
        p2, _ = m.decode(t2, enc, enc_len)
        assert torch.equal(p2[:, :j], pred[:, :j]) and not torch.equal(p2[:, j:], pred[:, j:]), j
    # without lengths: no memory mask
    p3, w3 = m.decode(tgt, enc)
    assert bool((w3 != 0).all()) and torch.isfinite(p3.float()).all()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_training_dropout_and_reproducibility(dt):
    from summarymixing_amd import ops
    dtype = DT[dt]
    src, tgt, wav_len, r = _asr_inputs(dtype)
    tgt, wav_len, r = tgt.cuda(), wav_len.cuda(), r.cuda().to(dtype)
    m = _asr(dtype, dropout=0.1).train()
    saved = ops._drop_state["counter"]                    # the library's seed stream is global: put it back

    def run(seed):
        torch.manual_seed(seed)
        ops._drop_state["counter"] = 9000
        with torch.no_grad():
            return m(src, tgt, wav_len)[1]
    try:
        a, b, c = run(1), run(2), run(1)
    finally:
        ops._drop_state["counter"] = saved
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    assert not torch.equal(a, b) and torch.equal(a, c)
    # a dropout step backward stays finite
    m.zero_grad()
    m(src, tgt, wav_len)[1].backward(r)
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    # no dropout: forward and backward agree bit for bit between two runs
    m0 = _asr(dtype, dropout=0.0).train()
    outs = []
    for _ in range(2):
        m0.zero_grad()
        for p in m0.parameters():
            p.grad = None
        o = m0(src, tgt, wav_len)[1]
        o.backward(r)
        outs.append((o.detach().clone(), {k: p.grad.clone() for k, p in m0.named_parameters() if p.grad is not None}))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1].keys() == outs[1][1].keys()
    assert any(k.startswith("decoder.") for k in outs[0][1]) and "custom_tgt_module.layers.0.emb.Embedding.weight" in outs[0][1]
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_eval_forward_replays_from_a_graph(dt):
    dtype = DT[dt]
    m = _asr(dtype).eval()
    src, tgt, wav_len, _ = _asr_inputs(dtype)
    tgt, wav_len = tgt.cuda().to(torch.int32), wav_len.cuda()
    with torch.no_grad():
        enc, dec = m(src, tgt, wav_len)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(src, tgt, wav_len)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            enc_g, dec_g = m(src, tgt, wav_len)
        dec_g.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(enc_g, enc) and torch.equal(dec_g, dec)

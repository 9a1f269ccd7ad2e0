"""CPU-side checks of the prediction network: the fp64 yardstick of the GPU tests (tests/_lstm_ref.py) against torch.nn.LSTM with
autograd, the drop-in modules' state_dict layout, their constructor refusals, the no-CPU-fallback error and what smx_lstm_*
refuses on the host."""
import ctypes

import pytest
import torch

from tests import _lstm_ref as R


def _torch_lstm(I, H, seed):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(I, H, batch_first=True).double()
    return m, (m.weight_ih_l0.detach(), m.weight_hh_l0.detach(), m.bias_ih_l0.detach(), m.bias_hh_l0.detach())


def _close(a, b, what):
    assert torch.allclose(a, b, rtol=1e-9, atol=1e-11), f"{what}: max |diff| {float((a - b).abs().max()):.3e}"


# (B, U, V, H, blank, with hx, with keep)
_CASES = [(2, 5, 7, 4, 0, False, False), (3, 6, 9, 5, 4, True, True), (2, 4, 6, 3, 5, True, False), (1, 1, 5, 8, 2, True, True),
          (4, 7, 8, 6, 7, False, True)]


@pytest.mark.parametrize("B,U,V,H,blank,with_hx,with_keep", _CASES)
def test_reference_matches_torch_lstm_on_one_hot_rows(B, U, V, H, blank, with_hx, with_keep):
    """The gather / scatter form with keep factors == torch.nn.LSTM fed the dense (scaled) one-hot rows, values and every
    gradient, including h0 / c0 and through h_n / c_n."""
    m, params = _torch_lstm(V - 1, H, 10 * B + U)
    g = torch.Generator().manual_seed(B + U + V)
    tokens = torch.randint(0, V, (B, U), generator=g)
    tokens[0, 0] = blank                                                    # a blank and a repeated token in every case
    tokens[-1, -1] = tokens[0, -1]
    keep = (torch.rand(B, U, generator=g) > 0.3).double() / 0.7 if with_keep else None
    h0 = torch.randn(1, B, H, generator=g, dtype=torch.float64).requires_grad_(True) if with_hx else None
    c0 = torch.randn(1, B, H, generator=g, dtype=torch.float64).requires_grad_(True) if with_hx else None
    dY, dhn, dcn = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, U, H), (B, H), (B, H)))
    x = R.onehot_rows(tokens, V, blank)
    assert x.shape == (B, U, V - 1) and float(x.sum()) == float((tokens != blank).sum())
    if keep is not None:
        x = x * keep.unsqueeze(-1)
    x.requires_grad_(True)
    y, (hn, cn) = m(x, (h0, c0) if with_hx else None)
    ((y * dY).sum() + (hn[0] * dhn).sum() + (cn[0] * dcn).sum()).backward()
    kw = dict(params=params, h0=h0.detach()[0] if with_hx else None, c0=c0.detach()[0] if with_hx else None, dY=dY, dhn=dhn, dcn=dcn)
    r = R.run(tokens=tokens, keep=keep, V=V, blank=blank, **kw)
    d = R.run(x=x.detach(), **kw)
    for res, tag in ((r, "one-hot"), (d, "dense")):
        _close(res["y"], y.detach(), f"{tag} y")
        _close(res["hn"], hn.detach()[0], f"{tag} hn")
        _close(res["cn"], cn.detach()[0], f"{tag} cn")
        _close(res["dw_ih"], m.weight_ih_l0.grad, f"{tag} dW_ih")
        _close(res["dw_hh"], m.weight_hh_l0.grad, f"{tag} dW_hh")
        _close(res["db_ih"], m.bias_ih_l0.grad, f"{tag} db_ih")
        _close(res["db_hh"], m.bias_hh_l0.grad, f"{tag} db_hh")
        if with_hx:
            _close(res["dh0"], h0.grad[0], f"{tag} dh0")
            _close(res["dc0"], c0.grad[0], f"{tag} dc0")
    _close(d["dx"], x.grad, "dense dx")


def test_reference_projection_and_mask_match_autograd():
    """The proj_dec / h-mask tail of the reference against autograd."""
    B, U, V, H, J, blank = 2, 5, 6, 4, 3, 1
    m, params = _torch_lstm(V - 1, H, 3)
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, V, (B, U), generator=g)
    hmask = (torch.rand(B, U, H, generator=g) > 0.2).double() / 0.8
    wp = torch.randn(J, H, generator=g, dtype=torch.float64).requires_grad_(True)
    dOut = torch.randn(B, U, J, generator=g, dtype=torch.float64)
    y, _ = m(R.onehot_rows(tokens, V, blank))
    out = (y * hmask) @ wp.t()
    (out * dOut).sum().backward()
    r = R.run(params=params, tokens=tokens, V=V, blank=blank, hmask=hmask, w_proj=wp.detach(), dOut=dOut)
    _close(r["out"], out.detach(), "out")
    _close(r["dw_proj"], wp.grad, "dW_proj")
    _close(r["dw_hh"], m.weight_hh_l0.grad, "dW_hh")
    _close(r["dw_ih"], m.weight_ih_l0.grad, "dW_ih")


def test_floor_emulation_rounds_h_to_bf16():
    B, U, V, H = 2, 6, 8, 4
    _, params = _torch_lstm(V - 1, H, 7)
    tokens = torch.randint(0, V, (B, U), generator=torch.Generator().manual_seed(1))
    ref, emu = R.floor_and_ref(torch.bfloat16, params=params, tokens=tokens, V=V, blank=0, dY=torch.ones(B, U, H))
    assert torch.equal(emu["y"], R.bf16_round(emu["y"])) and emu["y"].dtype == torch.float32
    err = float((emu["y"].double() - ref["y"]).abs().max())
    assert 0 < err < 2e-2
    _, emu32 = R.floor_and_ref(torch.float32, params=params, tokens=tokens, V=V, blank=0, dY=torch.ones(B, U, H))
    assert float((emu32["y"].double() - ref["y"]).abs().max()) < 1e-5


def test_lstm_state_dict_is_torch_lstm_under_rnn():
    from summarymixing_amd.nnet.RNN import LSTM
    I, H = 37, 64
    t = torch.nn.LSTM(I, H, batch_first=True)
    for m in (LSTM(H, input_shape=[None, None, I]), LSTM(H, input_size=I, re_init=False)):
        sd = m.state_dict()
        assert list(sd) == ["rnn." + k for k in t.state_dict()]
        assert all(sd["rnn." + k].shape == v.shape for k, v in t.state_dict().items())
        m.load_state_dict({"rnn." + k: v for k, v in t.state_dict().items()}, strict=True)
        assert torch.equal(m.rnn.weight_hh_l0, t.weight_hh_l0)


def test_lstm_re_init_orthogonalises_the_recurrent_weight():
    from summarymixing_amd.nnet.RNN import LSTM
    torch.manual_seed(0)
    w = LSTM(32, input_size=8, re_init=True).rnn.weight_hh_l0.detach()
    assert torch.allclose(w.t() @ w, torch.eye(32), atol=1e-5)
    w2 = LSTM(32, input_size=8, re_init=False).rnn.weight_hh_l0.detach()
    assert not torch.allclose(w2.t() @ w2, torch.eye(32), atol=1e-2) and float(w2.abs().max()) <= 1 / 32 ** 0.5


@pytest.mark.parametrize("blank", ["first", "middle", "last"])
def test_embedding_state_dict_is_the_one_hot_table(blank):
    from summarymixing_amd.nnet.embedding import Embedding
    V = 9
    b = {"first": 0, "middle": V // 2, "last": V - 1}[blank]
    e = Embedding(V, consider_as_one_hot=True, blank_id=b)
    sd = e.state_dict()
    assert list(sd) == ["Embedding.weight"] and sd["Embedding.weight"].shape == (V, V - 1)
    assert torch.equal(sd["Embedding.weight"], R.onehot_rows(torch.arange(V), V, b, torch.float32))
    assert e.embedding_dim == V - 1 and not e.Embedding.weight.requires_grad
    ref = torch.nn.Embedding(V, V - 1)
    ref.load_state_dict({"weight": sd["Embedding.weight"]})
    e.load_state_dict({"Embedding.weight": ref.weight.detach()}, strict=True)


def test_constructor_refusals():
    from summarymixing_amd.nnet.embedding import Embedding
    from summarymixing_amd.nnet.RNN import LSTM
    for kw in (dict(num_layers=2), dict(bidirectional=True), dict(bias=False), dict(dropout=0.1), dict(hidden_size=48),
               dict(hidden_size=16), dict(hidden_size=8192)):
        with pytest.raises(NotImplementedError):
            LSTM(**{"hidden_size": 64, "input_size": 8, **kw})
    with pytest.raises(ValueError):
        LSTM(64)
    with pytest.raises(NotImplementedError):
        Embedding(10, embedding_dim=16)
    with pytest.raises(ValueError):
        Embedding(10, consider_as_one_hot=True, blank_id=10)


def test_lengths_are_refused_before_any_launch():
    from summarymixing_amd.nnet.RNN import LSTM
    with pytest.raises(NotImplementedError):
        LSTM(64, input_size=8)(torch.randn(2, 3, 8), lengths=torch.ones(2))


def test_no_cpu_fallback():
    from summarymixing_amd.nnet import LSTM, Embedding
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.transducer import prediction_network
    emb, dec, proj = Embedding(10, consider_as_one_hot=True), LSTM(32, input_size=9), Linear(16, input_size=32, bias=False)
    for call in (lambda: dec(torch.randn(2, 3, 9)), lambda: emb(torch.zeros(2, 3, dtype=torch.long)),
                 lambda: prediction_network(torch.zeros(2, 3, dtype=torch.long), emb, dec, proj)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


_BASE = 1 << 40


def _p(i):
    return ctypes.c_void_p(_BASE + i * 0x100000)


@pytest.mark.parametrize("H,code", [(48, -2), (16, -2), (8192, -2), (0, -1)])
def test_lstm_entry_points_refuse_unsupported_hidden_sizes_on_the_host(H, code):
    """Fake pointers, never dereferenced: the refusal comes before any launch.  Supported H: multiples of 32 in [32, 4096]."""
    from summarymixing_amd import _lib
    lib = _lib.lib()
    for dt in (_lib.F32, _lib.BF16):
        assert lib.smx_lstm_fwd(dt, _p(0), _p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), _p(8), _p(9), 4, 3, H, None) == code
        assert lib.smx_lstm_bwd(dt, _p(0), _p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), _p(8), _p(9), 4, 3, H, None) == code
        assert lib.smx_lstm_ok(dt, H) == 0
    assert b"smx_lstm" in lib.smx_last_error()
    assert lib.smx_lstm_ok(_lib.BF16, 512) == 1 and lib.smx_lstm_ok(_lib.F32, 32) == 1 and lib.smx_lstm_ok(7, 512) == 0


def test_onehot_entry_points_refuse_bad_arguments_on_the_host():
    from summarymixing_amd import _lib
    lib = _lib.lib()
    assert lib.smx_onehot_rows(_lib.F32, _p(0), _p(1), 9, 4, 10, 10, None) == -1                       # blank outside the vocabulary
    assert lib.smx_onehot_gates_fwd(_lib.BF16, _p(0), None, _p(1), 130, _p(2), _p(3), 4, 10, 0, 130, None) == -2    # G % 4
    assert lib.smx_onehot_gates_wgrad(_lib.BF16, _p(0), None, _p(1), 128, None, 9, 4, 10, 0, 128, None) == -1       # no dW_ih
    assert lib.smx_onehot_gates_wgrad(_lib.F32, _p(0), None, _p(1), 128, _p(2), 8, 4, 10, 0, 128, None) == -1       # lddw < V - 1

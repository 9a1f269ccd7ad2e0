"""CPU-side checks of the RNN language model (lobes.models.RNNLM, csrc/lstm_step.hip): the float64 restatement tests/_rnnlm_ref.py
against a torch.nn chain, the state-dict names the pretrained checkpoint needs, the refusals, and what smx_lstm_step /
smx_gather_rows refuse on the host before any launch."""
import ctypes

import pytest
import torch

from tests import _rnnlm_ref as R

F64 = torch.float64


def _torch_chain(sd, V, E, H, L, D):
    emb = torch.nn.Embedding(V, E, padding_idx=0).double()
    rnn = torch.nn.LSTM(E, H, num_layers=L, batch_first=True).double()
    lin, norm, out = torch.nn.Linear(H, D).double(), torch.nn.LayerNorm(D).double(), torch.nn.Linear(D, V).double()
    with torch.no_grad():
        emb.weight.copy_(sd["embedding.Embedding.weight"])
        for k in range(L):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(rnn, f"{n}_l{k}").copy_(sd[f"rnn.rnn.{n}_l{k}"])
        lin.weight.copy_(sd["dnn.linear.w.weight"]); lin.bias.copy_(sd["dnn.linear.w.bias"])
        norm.weight.copy_(sd["dnn.norm.norm.weight"]); norm.bias.copy_(sd["dnn.norm.norm.bias"])
        out.weight.copy_(sd["out.w.weight"]); out.bias.copy_(sd["out.w.bias"])
    act = torch.nn.LeakyReLU()

    def fwd(tokens, hx=None):
        with torch.no_grad():
            y, (hn, cn) = rnn(emb(tokens), hx)
            return out(act(norm(lin(y)))), hn, cn
    return fwd


@pytest.mark.parametrize("L", [1, 2, 3])
def test_restatement_equals_the_torch_chain(L):
    V, E, H, D, B, U = 13, 8, 12, 10, 3, 5
    sd = {k: v.double() for k, v in R.make_params(V, E, H, L, D, seed=L).items()}
    fwd = _torch_chain(sd, V, E, H, L, D)
    tokens = torch.randint(0, V, (B, U), generator=torch.Generator().manual_seed(7))
    tokens[0, 0] = 0                                            # (row 0 of the table is NOT zero here: it is read as stored)
    logits, hn, cn = fwd(tokens)
    ref = R.run(sd, tokens, L)
    for got, want in ((ref["logits"], logits), (ref["hn"], hn), (ref["cn"], cn)):
        assert got.dtype == F64 and torch.allclose(got, want, rtol=1e-11, atol=1e-12)
    # step by step with hx fed back, on both sides
    hx_t, hx_r = None, None
    for u in range(U):
        lt, h_t, c_t = fwd(tokens[:, u:u + 1], hx_t)
        r = R.run(sd, tokens[:, u:u + 1], L, hx_r)
        hx_t, hx_r = (h_t, c_t), (r["hn"], r["cn"])
        assert torch.allclose(r["logits"], lt, rtol=1e-11, atol=1e-12) and torch.allclose(r["logits"][:, 0], ref["logits"][:, u], rtol=1e-10, atol=1e-11)
    assert torch.allclose(hx_r[0], hn, rtol=1e-10, atol=1e-11) and torch.allclose(hx_r[1], cn, rtol=1e-10, atol=1e-11)


def test_lookup_reads_tokens_outside_the_table_as_zero_rows():
    table = torch.arange(12, dtype=F64).view(4, 3) + 1
    got = R.lookup(table, torch.tensor([0, -1, 4, 3]))
    assert torch.equal(got, torch.stack([table[0], torch.zeros(3, dtype=F64), torch.zeros(3, dtype=F64), table[3]]))


def test_state_dict_names_shapes_and_strict_load():
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    V, E, H, L, D = 40, 32, 64, 2, 48
    lm = RNNLM(V, embedding_dim=E, rnn_layers=L, rnn_neurons=H, dnn_neurons=D, dropout=0.0, return_hidden=True)
    sd = lm.state_dict()
    assert list(sd) == R.keys(L)
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.shapes(V, E, H, L, D)
    # a dict built under those names from the torch modules loads strictly
    emb, rnn = torch.nn.Embedding(V, E, padding_idx=0), torch.nn.LSTM(E, H, num_layers=L, batch_first=True)
    lin, norm, out = torch.nn.Linear(H, D), torch.nn.LayerNorm(D), torch.nn.Linear(D, V)
    with torch.no_grad():
        emb.weight[0].uniform_(0.5, 1.0)                        # a non-zero padding row, as a trained table may hold
    src = {"embedding.Embedding.weight": emb.weight, "dnn.linear.w.weight": lin.weight, "dnn.linear.w.bias": lin.bias,
           "dnn.norm.norm.weight": norm.weight, "dnn.norm.norm.bias": norm.bias, "out.w.weight": out.weight, "out.w.bias": out.bias}
    src.update({f"rnn.rnn.{n}": p for n, p in rnn.named_parameters()})
    res = lm.load_state_dict({k: v.detach().clone() for k, v in src.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(lm.embedding.Embedding.weight[0], emb.weight[0]) and float(lm.embedding.Embedding.weight[0].detach().abs().min()) >= 0.5
    assert torch.equal(lm.rnn.rnn.weight_hh_l1, rnn.weight_hh_l1)


def test_recipe_constructor_and_defaults():
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    from summarymixing_amd.nnet.RNN import LSTM
    lm = RNNLM(output_neurons=1000, embedding_dim=128, activation=torch.nn.LeakyReLU, dropout=0.0, rnn_layers=2, rnn_neurons=64,
               dnn_blocks=1, dnn_neurons=512, return_hidden=True, rnn_class=LSTM)
    assert lm.return_hidden and lm.rnn.num_layers == 2 and lm.embedding.Embedding.padding_idx == 0
    d = RNNLM(10, rnn_neurons=32)
    assert d.p_drop == 0.15 and not d.return_hidden and d.embedding.Embedding.weight.shape == (10, 128)


def test_refusals():
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    for kw in (dict(dnn_blocks=2), dict(dnn_blocks=0), dict(rnn_class=torch.nn.GRU), dict(rnn_class=torch.nn.LSTM), dict(activation=torch.nn.Tanh),
               dict(rnn_neurons=48), dict(rnn_neurons=4128), dict(embedding_dim=48), dict(embedding_dim=16), dict(embedding_dim=4128)):
        with pytest.raises(NotImplementedError):
            RNNLM(20, **{"rnn_neurons": 64, **kw})


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    lm = RNNLM(20, embedding_dim=32, rnn_neurons=32, dnn_neurons=32, dropout=0.0).eval()
    with torch.no_grad():
        for tokens in (torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, dtype=torch.long)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                lm(tokens)


class _OnGpu:
    """Tokens that claim to live on the GPU: the forward's argument checks come after the device check and before any kernel."""

    def __init__(self, *shape):
        self.shape, self.is_cuda, self.dtype = shape, True, torch.long

    def dim(self):
        return len(self.shape)


def test_forward_refuses_gradients_and_training_dropout():
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    lm = RNNLM(20, embedding_dim=32, rnn_neurons=32, dnn_neurons=32, dropout=0.1)
    with pytest.raises(NotImplementedError, match="inference only"):
        lm(_OnGpu(2, 3))                                        # gradients enabled, parameters require them
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="dropout"):
            lm.train()(_OnGpu(2))                               # dropout > 0 in training mode
    with torch.no_grad(), pytest.raises(ValueError):
        lm.eval()(_OnGpu(2, 3, 4))


# ---- what the library refuses on the host (fake pointers, never dereferenced; a null stream) --------------------------------------------
_BASE = 1 << 40
_EINVAL, _EUNSUPPORTED = -1, -2


def _lib():
    from summarymixing_amd import _lib
    return _lib


def test_lstm_step_ok_at_the_edges_of_its_range():
    L = _lib()
    ok = L.lib().smx_lstm_step_ok
    for dtype in (L.F32, L.BF16):
        assert [ok(dtype, I, 64) for I in (0, 16, 32, 48, 64, 96, 4064, 4096, 4128)] == [0, 0, 1, 0, 1, 1, 1, 1, 0]
        assert [ok(dtype, 128, H) for H in (0, 16, 32, 48, 2048, 4096, 4128)] == [0, 0, 1, 0, 1, 1, 0]
    assert ok(2, 128, 2048) == 0 and ok(-1, 128, 2048) == 0
    assert ok(L.BF16, 128, 2048) == 1                          # the recipe's layers
    assert ok(L.BF16, 2048, 2048) == 1


def _step(**kw):
    B, I, H = kw.pop("B", 4), kw.pop("I", 64), kw.pop("H", 64)
    a = dict(dtype=1, X=_BASE, ldx=I, tok=None, V=0, Wih=_BASE + 0x100000, Whh=_BASE + 0x200000, bias=_BASE + 0x300000, h=_BASE + 0x400000,
             c=_BASE + 0x500000, h_out=_BASE + 0x600000, c_out=_BASE + 0x700000)
    a.update(kw)
    return _lib().lib().smx_lstm_step(a["dtype"], a["X"], a["ldx"], a["tok"], a["V"], a["Wih"], a["Whh"], a["bias"], a["h"], a["c"], a["h_out"],
                                      a["c_out"], B, I, H, None)


_STEP_REFUSED = [
    ("unknown dtype", dict(dtype=3), _EINVAL),
    ("no W_hh", dict(Whh=None), _EINVAL),
    ("no bias", dict(bias=None), _EINVAL),
    ("no h'", dict(h_out=None), _EINVAL),
    ("B < 0", dict(B=-1), _EINVAL),
    ("ldx < I", dict(ldx=32), _EINVAL),
    ("tokens without a table size", dict(tok=_BASE + 0x800000, V=0), _EINVAL),
    ("h' is h", dict(h_out=_BASE + 0x400000), _EINVAL),
    ("h' overlaps h", dict(h_out=_BASE + 0x400000 + 64), _EINVAL),
    ("c' is c", dict(c_out=_BASE + 0x500000), _EINVAL),
    ("h' is the dense input", dict(h_out=_BASE), _EINVAL),
    ("H = 48", dict(H=48), _EUNSUPPORTED),
    ("H = 4128", dict(H=4128), _EUNSUPPORTED),
    ("I = 48", dict(I=48, ldx=48), _EUNSUPPORTED),
    ("I = 4128", dict(I=4128, ldx=4128), _EUNSUPPORTED),
    ("X 8-byte aligned", dict(X=_BASE + 8), _EUNSUPPORTED),
    ("W_ih 4-byte aligned", dict(Wih=_BASE + 0x100004), _EUNSUPPORTED),
    ("h 8-byte aligned", dict(h=_BASE + 0x400008), _EUNSUPPORTED),
    ("ldx % 8", dict(ldx=68), _EUNSUPPORTED),
]


@pytest.mark.parametrize("case,kw,code", _STEP_REFUSED, ids=[c[0] for c in _STEP_REFUSED])
def test_lstm_step_refuses_what_it_cannot_run(case, kw, code):
    assert _step(**kw) == code, case


def test_lstm_step_of_no_rows_and_gather_rows_argument_checks():
    assert _step(B=0) == 0                                      # nothing to do: no launch
    assert _step(B=0, h=None, c=None) == 0
    g = _lib().lib().smx_gather_rows
    T, Y = _BASE, _BASE + 0x100000
    assert g(1, _BASE + 0x200000, T, 64, Y, 64, 0, 10, 64, None) == 0
    assert g(1, None, T, 64, Y, 64, 4, 10, 64, None) == _EINVAL
    assert g(5, _BASE + 0x200000, T, 64, Y, 64, 4, 10, 64, None) == _EINVAL
    assert g(1, _BASE + 0x200000, T, 32, Y, 64, 4, 10, 64, None) == _EINVAL             # ldt < D
    assert g(1, _BASE + 0x200000, T, 64, Y, 64, 4, 10, 60, None) == _EUNSUPPORTED       # D % 8
    assert g(0, _BASE + 0x200000, T + 8, 64, Y, 64, 4, 10, 64, None) == _EUNSUPPORTED   # table 8-byte aligned

"""The RNN language model on the GPU (csrc/lstm_step.hip behind ops.lstm_step / ops.gather_rows and lobes.models.RNNLM) against the
fp64 restatement tests/_rnnlm_ref.py on the same, dtype-rounded parameters: the one-launch LSTM step in its dense and gathered forms,
row independence, bit reproducibility, the aliasing refusal, steps against the sequence kernels, the whole model in both forms, and a
captured decode step.

Bars: float32 uses tests/_util.TOL; bf16 uses max(TOL, 4 x floor), the floor being the same computation in float32 with h and the
stored activations rounded to bf16, against fp64 - measured on the CPU per case (floor_and_ref), never from the code under test."""
import functools

import pytest
import torch

from tests import _rnnlm_ref as R
from tests._lstm_ref import bf16_round
from tests._util import TOL, rel_err, report

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
_DT = [F32, BF16]
_IDS = ["f32", "bf16"]


def _judge(name, got, ref, emu, dtype):
    entries, bad = {}, []
    for k, v in got.items():
        floor = rel_err(emu[k], ref[k])
        bar = TOL[dtype][0] if dtype == F32 else max(TOL[dtype][0], 4 * floor)
        err = rel_err(v, ref[k])
        entries[k] = {"err": err, "floor": floor, "bar": bar}
        if not err <= bar:
            bad.append((k, err, bar))
    report(name, entries)
    assert not bad, f"{name}: {bad}"


# ---- smx_lstm_step on its own -------------------------------------------------------------------------------------------------
_STEP_SHAPES = [(1, 32, 32), (3, 64, 32), (17, 128, 64), (33, 96, 160), (2, 512, 512)]


@functools.lru_cache(maxsize=None)
def _step_case(B, I, H, dtype):
    """Operands (rounded to dtype where the kernel reads them in dtype) of one step; biases and W_ih from +-0.5 so every gate matters."""
    g = torch.Generator().manual_seed(1000 * B + I + H)
    u = lambda shape, a: (torch.rand(shape, generator=g) * 2 - 1) * a
    return dict(x=torch.randn(B, I, generator=g).to(dtype), w_ih=u((4 * H, I), 0.5).to(dtype), w_hh=u((4 * H, H), H ** -0.5).to(dtype),
                b_ih=u((4 * H,), 0.5), b_hh=u((4 * H,), 0.5), h=(0.5 * torch.randn(B, H, generator=g)).to(dtype), c=torch.randn(B, H, generator=g))


def _step_ref(case, with_state, dtype, x=None):
    out = []
    for dt, rnd in ((torch.float64, None), (F32, bf16_round if dtype == BF16 else None)):
        x_ = (case["x"] if x is None else x).to(dt)
        B, H = x_.shape[0], case["w_hh"].shape[1]
        h = case["h"].to(dt) if with_state else torch.zeros(B, H, dtype=dt)
        c = case["c"].to(dt) if with_state else torch.zeros(B, H, dtype=dt)
        hn, cn = R.lstm_cell(x_, h, c, case["w_ih"].to(dt), case["w_hh"].to(dt), case["b_ih"].to(dt), case["b_hh"].to(dt))
        out.append({"h": rnd(hn) if rnd else hn, "c": cn})
    return out


def _gpu_step(case, with_state, x=None, tokens=None, rows=None):
    from summarymixing_amd import ops
    sl = slice(None) if rows is None else slice(0, rows)
    bias = (case["b_ih"] + case["b_hh"]).cuda()
    x_ = (case["x"][sl] if x is None else x).cuda()
    h = case["h"][sl].cuda().contiguous() if with_state else None
    c = case["c"][sl].cuda().contiguous() if with_state else None
    hn, cn = ops.lstm_step(x_, case["w_ih"].cuda(), case["w_hh"].cuda(), bias, h, c, tokens=tokens)
    return hn, cn


@pytest.mark.parametrize("dtype", _DT, ids=_IDS)
@pytest.mark.parametrize("with_state", [True, False], ids=["hx", "nohx"])
@pytest.mark.parametrize("B,I,H", _STEP_SHAPES)
def test_lstm_step_against_fp64(B, I, H, with_state, dtype):
    case = _step_case(B, I, H, dtype)
    ref, emu = _step_ref(case, with_state, dtype)
    hn, cn = _gpu_step(case, with_state)
    assert hn.shape == (B, H) and cn.shape == (B, H) and hn.dtype == dtype and cn.dtype == F32
    _judge(f"lstm_step B{B} I{I} H{H} {'hx' if with_state else 'nohx'} {dtype}", {"h": hn, "c": cn}, ref, emu, dtype)


@pytest.mark.parametrize("dtype", _DT, ids=_IDS)
def test_gathered_form_equals_the_dense_form_on_the_gathered_rows(dtype):
    """Row 0 of the table is NOT zero and is read as stored; -1 and V read as zero rows."""
    V, B, I, H = 11, 19, 64, 64
    case = _step_case(B, I, H, dtype)
    g = torch.Generator().manual_seed(5)
    table = torch.randn(V, I, generator=g).to(dtype)
    assert float(table[0].abs().min()) > 0
    tokens = torch.randint(0, V, (B,), generator=g).to(torch.int32)
    tokens[0], tokens[1], tokens[2], tokens[3], tokens[18] = 0, -1, V, V - 1, 0
    dense = R.lookup(table.float(), tokens).to(dtype)
    assert torch.equal(dense[1], torch.zeros(I, dtype=dtype)) and torch.equal(dense[0], table[0])
    hd, cd = _gpu_step(case, True, x=dense)
    hg, cg = _gpu_step(case, True, x=table, tokens=tokens.cuda())
    assert torch.equal(hd, hg) and torch.equal(cd, cg)
    ref, emu = _step_ref(case, True, dtype, x=dense)
    _judge(f"lstm_step gathered {dtype}", {"h": hg, "c": cg}, ref, emu, dtype)
    # and the out-of-range rows equal a zero input: the same state with x = 0
    hz, cz = _gpu_step(case, True, x=torch.zeros(B, I, dtype=dtype))
    assert torch.equal(hz[1:3], hg[1:3]) and torch.equal(cz[1:3], cg[1:3])
    assert not torch.equal(hz[0], hg[0])                        # (token 0 is not a zero row)


@pytest.mark.parametrize("dtype", _DT, ids=_IDS)
def test_rows_are_independent_and_runs_are_bit_equal(dtype):
    case = _step_case(17, 128, 64, dtype)
    h17, c17 = _gpu_step(case, True)
    h3, c3 = _gpu_step(case, True, rows=3)
    assert torch.equal(h17[:3], h3) and torch.equal(c17[:3], c3)
    again = _gpu_step(case, True)
    assert torch.equal(again[0], h17) and torch.equal(again[1], c17)
    big = _step_case(33, 96, 160, dtype)                        # three batch tiles in one pass of the weights
    h33, c33 = _gpu_step(big, True)
    h20, c20 = _gpu_step(big, True, rows=20)
    assert torch.equal(h33[:20], h20) and torch.equal(c33[:20], c20)


def test_more_rows_than_one_pass_holds():
    """B = 100 > 96 rows: the workgroup makes a second pass over its weights; rows 96-99 equal their own 4-row call."""
    B, I, H = 100, 32, 32
    case = _step_case(B, I, H, BF16)
    ref, emu = _step_ref(case, True, BF16)
    hn, cn = _gpu_step(case, True)
    _judge("lstm_step B100 two passes", {"h": hn, "c": cn}, ref, emu, BF16)
    tail = {k: (v[96:].contiguous() if k in ("x", "h", "c") else v) for k, v in case.items()}
    ht, ct = _gpu_step(tail, True)
    assert torch.equal(ht, hn[96:]) and torch.equal(ct, cn[96:])


def test_aliased_state_is_refused_before_any_launch():
    from summarymixing_amd import _lib as L
    from summarymixing_amd import ops
    case = _step_case(3, 64, 32, F32)
    d = {k: v.cuda() for k, v in case.items()}
    bias = d["b_ih"] + d["b_hh"]
    h_before = d["h"].clone()
    p = lambda t: t.data_ptr()
    call = lambda h_out, c_out: L.lib().smx_lstm_step(L.F32, p(d["x"]), 64, None, 0, p(d["w_ih"]), p(d["w_hh"]), p(bias), p(d["h"]), p(d["c"]),
                                                      p(h_out), p(c_out), 3, 64, 32, ops._stream())
    assert call(d["h"], torch.empty_like(d["c"])) == -1         # SMX_EINVAL
    assert call(torch.empty_like(d["h"]), d["c"]) == -1
    torch.cuda.synchronize()
    assert torch.equal(d["h"], h_before)
    with pytest.raises(RuntimeError, match="alias"):
        ops.lstm_step(d["x"], d["w_ih"], d["w_hh"], bias, d["h"], d["c"], h_out=d["h"])


# ---- U steps through smx_lstm_step against the sequence kernels, three layers ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_case(V, E, H, L, D, B, U, dtype, seed):
    sd = R.make_params(V, E, H, L, D, seed)
    tokens = torch.randint(0, V, (B, U), generator=torch.Generator().manual_seed(seed + 1))
    tokens[0, 0] = 0
    ref, emu = R.floor_and_ref(dtype, sd, tokens, L)
    return sd, tokens, ref, emu


@pytest.mark.parametrize("dtype", _DT, ids=_IDS)
def test_steps_and_the_sequence_route_match_the_same_reference(dtype):
    from summarymixing_amd import functional as F
    from summarymixing_amd import ops
    B, U, I, H, L = 3, 6, 32, 64, 3
    sd, tokens, ref, emu = _model_case(20, I, H, L, 32, B, U, dtype, 11)
    table = sd["embedding.Embedding.weight"].to(dtype).cuda()
    W = [(sd[f"rnn.rnn.weight_ih_l{k}"].to(dtype).cuda(), sd[f"rnn.rnn.weight_hh_l{k}"].to(dtype).cuda(),
          (sd[f"rnn.rnn.bias_ih_l{k}"] + sd[f"rnn.rnn.bias_hh_l{k}"]).cuda()) for k in range(L)]
    tk = tokens.to(torch.int32).cuda()
    # (a) U steps, the state of every layer fed back through fresh buffers
    h, c, ys = [None] * L, [None] * L, []
    for u in range(U):
        tku = tk[:, u].contiguous()
        for k in range(L):
            if k == 0:
                h[k], c[k] = ops.lstm_step(table, *W[k], h[k], c[k], tokens=tku)
            else:
                h[k], c[k] = ops.lstm_step(h[k - 1], *W[k], h[k], c[k])
        ys.append(h[L - 1])
    got = {"y": torch.stack(ys, 1), "hn": torch.stack(h), "cn": torch.stack(c)}
    _judge(f"lstm_step x{U} L{L} {dtype}", got, ref, emu, dtype)
    # (b) the existing sequence kernels on the same operands
    x = ops.gather_rows(tk, table)
    assert torch.equal(x.cpu(), R.lookup(table.cpu().float(), tokens).to(dtype))
    hs, cs = [], []
    for k in range(L):
        Kin = x.shape[2]
        x2, Wih = x.reshape(B * U, Kin), W[k][0]
        if Kin % 64:
            x2 = torch.nn.functional.pad(x2, (0, 64 - Kin % 64))
            Wih = torch.nn.functional.pad(Wih, (0, 64 - Kin % 64))
        Gx, _ = F.linear_fwd(x2.contiguous(), Wih.contiguous(), W[k][2], out_f32=dtype != F32)
        x, hk, ck, _ = ops.lstm_fwd(Gx, W[k][1], None, None, B, U, False)
        hs.append(hk)
        cs.append(ck)
    _judge(f"lstm_fwd sequence L{L} {dtype}", {"y": x, "hn": torch.stack(hs), "cn": torch.stack(cs)}, ref, emu, dtype)


# ---- the model ------------------------------------------------------------------------------------------------------------
_CONFIGS = [(40, 32, 64, 2, 64), (1000, 128, 256, 2, 512)]


def _lm(sd, V, E, H, L, D, dtype, return_hidden=True):
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    lm = RNNLM(V, embedding_dim=E, rnn_layers=L, rnn_neurons=H, dnn_neurons=D, dropout=0.0, return_hidden=return_hidden)
    lm.load_state_dict(sd, strict=True)
    lm = lm.cuda().eval()
    if dtype == BF16:
        lm.embedding.to(BF16)
    return lm


@pytest.mark.parametrize("dtype", _DT, ids=_IDS)
@pytest.mark.parametrize("B,U", [(3, 5), (17, 4)])
@pytest.mark.parametrize("V,E,H,L,D", _CONFIGS)
def test_rnnlm_sequence_form(V, E, H, L, D, B, U, dtype):
    sd, tokens, ref, emu = _model_case(V, E, H, L, D, B, U, dtype, 3)
    lm = _lm(sd, V, E, H, L, D, dtype)
    with torch.no_grad():
        logits, (hn, cn) = lm(tokens.cuda())
    assert logits.shape == (B, U, V) and hn.shape == (L, B, H) and cn.shape == (L, B, H)
    assert logits.dtype == dtype and hn.dtype == dtype and cn.dtype == F32
    _judge(f"rnnlm seq V{V} H{H} B{B} U{U} {dtype}", {"logits": logits, "hn": hn, "cn": cn}, ref, emu, dtype)
    lm.return_hidden = False
    with torch.no_grad():
        only = lm(tokens.cuda())
    assert torch.is_tensor(only) and torch.equal(only, logits)


@pytest.mark.parametrize("dtype", _DT, ids=_IDS)
@pytest.mark.parametrize("V,E,H,L,D", _CONFIGS)
def test_rnnlm_step_form_fed_token_by_token(V, E, H, L, D, dtype):
    B, U = 3, 5
    sd, tokens, ref, emu = _model_case(V, E, H, L, D, B, U, dtype, 3)
    lm = _lm(sd, V, E, H, L, D, dtype)
    tk = tokens.cuda()
    hx, outs, held = None, [], []
    with torch.no_grad():
        for u in range(U):
            lg, hx = lm(tk[:, u], hx if u != 2 else (hx[0].double(), hx[1].double()))     # (hx comes back in any float dtype)
            assert lg.shape == (B, V) and lg.dtype == dtype and hx[0].shape == (L, B, H) and hx[0].dtype == dtype and hx[1].dtype == F32
            outs.append(lg)
            held.append((hx[0], hx[0].clone()))
    assert all(torch.equal(a, b) for a, b in held)              # earlier states are not overwritten by later steps
    _judge(f"rnnlm steps V{V} H{H} {dtype}", {"logits": torch.stack(outs, 1), "hn": hx[0], "cn": hx[1]}, ref, emu, dtype)
    lm.return_hidden = False
    with torch.no_grad():
        only = lm(tk[:, 0])
    assert torch.is_tensor(only) and torch.equal(only, outs[0])


def test_rnnlm_refuses_gradients_on_the_gpu():
    sd, tokens, _, _ = _model_case(40, 32, 64, 2, 64, 3, 5, F32, 3)
    lm = _lm(sd, 40, 32, 64, 2, 64, F32)
    with pytest.raises(NotImplementedError):
        lm(tokens.cuda())
    for p in lm.parameters():
        p.requires_grad_(False)
    assert lm(tokens.cuda())[0].shape == (3, 5, 40)             # frozen parameters: no torch.no_grad() needed


@pytest.mark.parametrize("dtype", _DT, ids=_IDS)
def test_captured_step_replays_the_eager_bits(dtype):
    """One step captured once (state set A -> set B, both static) and replayed three times, the new state copied back into set A
    between replays; its bits equal three eager steps.  The step launches on the capturing stream alone: a plain chain."""
    V, E, H, L, D = _CONFIGS[0]
    B, U = 3, 3
    sd, tokens, _, _ = _model_case(V, E, H, L, D, 3, 5, dtype, 3)
    lm = _lm(sd, V, E, H, L, D, dtype)
    tk = tokens[:, :U].cuda()
    g = torch.Generator().manual_seed(9)
    h0 = (0.5 * torch.randn(L, B, H, generator=g)).to(dtype).cuda()
    c0 = torch.randn(L, B, H, generator=g).cuda()
    with torch.no_grad():
        eager, hx = [], (h0, c0)
        for u in range(U):
            lg, hx = lm(tk[:, u], hx)
            eager.append(lg)
        tok_s = tk[:, 0].clone()
        hA, cA, hB, cB = h0.clone(), c0.clone(), torch.empty_like(h0), torch.empty_like(c0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            lm.step(tok_s, (hA, cA), out=(hB, cB))              # warm-up: the weight images exist before the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            lg_s, _ = lm.step(tok_s, (hA, cA), out=(hB, cB))
        for u in range(U):
            tok_s.copy_(tk[:, u])
            graph.replay()
            assert torch.equal(lg_s, eager[u]), u
            hA.copy_(hB)
            cA.copy_(cB)
    assert torch.equal(hB, hx[0]) and torch.equal(cB, hx[1])


# ---- the parameter holder is nnet.RNN's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("re_init", [False, True], ids=["uniform", "orthogonal"])
def test_one_layer_holder_has_the_lstms_state_dict(re_init):
    """A one-layer RNNLM's rnn.rnn and an LSTM's rnn: the same keys, shapes and - the seed and the draws before them being the same -
    values."""
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    from summarymixing_amd.nnet.RNN import LSTM
    V, E, H = 50, 32, 64
    torch.manual_seed(7)
    lm = RNNLM(V, embedding_dim=E, rnn_layers=1, rnn_neurons=H, rnn_re_init=re_init, dnn_neurons=32)
    torch.manual_seed(7)
    torch.nn.Embedding(V, E, padding_idx=0)                    # (the table RNNLM draws before its LSTM)
    dec = LSTM(H, input_size=E, re_init=re_init)
    a, b = lm.rnn.rnn.state_dict(), dec.rnn.state_dict()
    assert type(lm.rnn.rnn) is type(dec.rnn) and list(a) == list(b) == ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    assert all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)


def test_two_layer_holder_has_torchs_keys():
    from summarymixing_amd.lobes.models.RNNLM import RNNLM
    V, E, H = 50, 32, 64
    lm = RNNLM(V, embedding_dim=E, rnn_layers=2, rnn_neurons=H, dnn_neurons=32)
    ref = torch.nn.LSTM(E, H, num_layers=2, batch_first=True).state_dict()
    sd = lm.rnn.rnn.state_dict()
    assert list(sd) == list(ref) == [f"{n}_l{k}" for k in (0, 1) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    assert all(sd[k].shape == ref[k].shape for k in sd)

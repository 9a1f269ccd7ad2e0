"""The prediction network on the GPU (csrc/lstm.hip behind nnet.embedding.Embedding, nnet.RNN.LSTM and
nnet.transducer.prediction_network) against the fp64 restatement tests/_lstm_ref.py on the same, dtype-rounded parameters and
inputs: forward, h_n / c_n, dX, dh0 / dc0, the four parameter gradients and proj_dec's; fused path == drop-in chain; bit
reproducibility, accumulation, graph capture, dropout masks, and the whole head in one step against tests/_rnnt_ref.py.

Bars: float32 uses tests/_util.TOL.  bf16 and the long sequence compound the rounding of h over the steps: their bar per quantity
is max(TOL, 4 x floor), the floor being the same recurrence in float32 (bf16: h and the stored gate gradients rounded to bf16)
against fp64 - measured on the CPU per case by _lstm_ref.floor_and_ref, never from the code under test."""
import pytest
import torch

from tests import _lstm_ref as R
from tests._util import TOL, rel_err, report

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _rounded(t, dtype):
    return t.to(dtype).double()


def _modules(V, H, J, blank, dtype, seed, I=None):
    from summarymixing_amd.nnet import LSTM, Embedding
    from summarymixing_amd.nnet.linear import Linear
    torch.manual_seed(seed)
    emb = Embedding(V, consider_as_one_hot=True, blank_id=blank)
    dec = LSTM(H, input_shape=[None, None, I if I is not None else V - 1])
    proj = Linear(J, input_size=H, bias=False)
    with torch.no_grad():                                      # biases and input weights large enough to matter in every gate
        dec.rnn.bias_ih_l0.uniform_(-0.5, 0.5)
        dec.rnn.bias_hh_l0.uniform_(-0.5, 0.5)
        dec.rnn.weight_ih_l0.uniform_(-0.5, 0.5)
    emb, dec, proj = emb.cuda(), dec.cuda(), proj.cuda()
    if dtype == BF16:
        emb = emb.to(BF16)
    return emb, dec, proj


def _ref_params(dec, dtype):
    p = dec.rnn
    return (_rounded(p.weight_ih_l0.detach().cpu(), dtype), _rounded(p.weight_hh_l0.detach().cpu(), dtype),
            p.bias_ih_l0.detach().cpu().double(), p.bias_hh_l0.detach().cpu().double())


def _grads(dec, proj=None):
    p = dec.rnn
    g = {"dw_ih": p.weight_ih_l0.grad, "dw_hh": p.weight_hh_l0.grad, "db_ih": p.bias_ih_l0.grad, "db_hh": p.bias_hh_l0.grad}
    if proj is not None:
        g["dw_proj"] = proj.w.weight.grad
    return {k: v.detach().clone() for k, v in g.items()}


def _zero(*mods):
    for m in mods:
        m.zero_grad(set_to_none=True)


def _judge(name, got, ref, emu, dtype, careful):
    """Every quantity in `got` against ref under its bar; the errors and floors go to the report."""
    entries, bad = {}, []
    for k, v in got.items():
        fwd = k in ("y", "hn", "cn", "out")
        tol = TOL[dtype][0 if fwd else 1]
        floor = rel_err(emu[k], ref[k])
        bar = max(tol, 4 * floor) if careful else tol
        err = rel_err(v, ref[k])
        entries[k] = {"err": err, "floor": floor, "bar": bar}
        if not err <= bar:
            bad.append((k, err, bar))
    report(name, entries)
    assert not bad, f"{name}: {bad}"


# ---- the drop-in LSTM on a dense input: (B, U, I, H, with hx) ----------------------------------------------------------------
_DENSE = [(3, 1, 37, 64, True), (5, 7, 37, 32, False), (17, 5, 64, 64, True), (8, 64, 999, 512, False)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,U,I,H,with_hx", _DENSE)
def test_lstm_dense_against_fp64(B, U, I, H, with_hx, dtype):
    _, dec, _ = _modules(I + 1, H, 8, 0, dtype, seed=B + U)
    g = torch.Generator().manual_seed(100 + B)
    x = torch.randn(B, U, I, generator=g).to(dtype)
    h0 = (0.5 * torch.randn(1, B, H, generator=g)).to(dtype) if with_hx else None
    c0 = torch.randn(1, B, H, generator=g) if with_hx else None
    dY, dhn, dcn = torch.randn(B, U, H, generator=g).to(dtype), torch.randn(B, H, generator=g).to(dtype), torch.randn(B, H, generator=g)
    xg = x.cuda().requires_grad_(True)
    hx = (h0.cuda().requires_grad_(True), c0.cuda().requires_grad_(True)) if with_hx else None
    y, (hn, cn) = dec(xg, hx)
    assert y.shape == (B, U, H) and hn.shape == (1, B, H) and cn.shape == (1, B, H) and y.dtype == dtype and cn.dtype == F32
    ((y.float() * dY.cuda().float()).sum() + (hn[0].float() * dhn.cuda().float()).sum() + (cn[0] * dcn.cuda()).sum()).backward()
    kw = dict(params=_ref_params(dec, dtype), x=x, h0=h0[0] if with_hx else None, c0=c0[0] if with_hx else None, dY=dY, dhn=dhn, dcn=dcn)
    ref, emu = R.floor_and_ref(dtype, **kw)
    got = {"y": y, "hn": hn[0], "cn": cn[0], "dx": xg.grad, **_grads(dec)}
    if with_hx:
        got.update(dh0=hx[0].grad[0], dc0=hx[1].grad[0])
    _judge(f"lstm_dense B{B} U{U} I{I} H{H} {dtype}", got, ref, emu, dtype, careful=dtype == BF16)


def test_single_steps_with_hx_equal_the_whole_sequence():
    """The decoding step form: U launches of U = 1, (h_n, c_n) fed back, give the bits of one call over the sequence."""
    B, U, I, H = 3, 6, 24, 64
    _, dec, _ = _modules(I + 1, H, 8, 0, F32, seed=2)
    x = torch.randn(B, U, I, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        y, (hn, cn) = dec(x)
        hx, ys = None, []
        for u in range(U):
            yu, hx = dec(x[:, u:u + 1], hx)
            ys.append(yu)
    assert torch.equal(torch.cat(ys, 1), y) and torch.equal(hx[0], hn) and torch.equal(hx[1], cn)


def test_embedding_rows_equal_the_table():
    from summarymixing_amd.nnet import Embedding
    V = 11
    tokens = torch.randint(0, V, (4, 9), generator=torch.Generator().manual_seed(0))
    for blank in (0, V // 2, V - 1):
        for dtype in (F32, BF16):
            e = Embedding(V, consider_as_one_hot=True, blank_id=blank).cuda().to(dtype)
            out = e(tokens.cuda())
            assert out.dtype == dtype and torch.equal(out.cpu(), e.Embedding.weight.detach().cpu()[tokens])
            assert torch.equal(out.float().cpu(), R.onehot_rows(tokens, V, blank, F32))


# ---- the fused path: (B, U1, V, H, J, blank, with hx, long) --------------------------------------------------------------------
_FUSED = [(8, 64, 1000, 512, 640, 0, False, False), (3, 1, 20, 64, 64, 7, True, False), (1, 300, 50, 512, 64, 25, False, True),
          (5, 9, 12, 32, 64, 11, True, False), (17, 6, 30, 64, 128, 3, False, False)]


def _tokens(B, U1, V, blank, seed):
    t = torch.randint(0, V, (B, U1), generator=torch.Generator().manual_seed(seed))
    t[:, 0] = blank                                            # the <bos> column is the blank, as in the recipe
    if U1 > 2:
        t[-1, -1] = t[0, 1]                                    # a repeated token: the scatter has something to add up
        t[0, 2] = t[0, 1]
    return t


def _run_fused(emb, dec, proj, tokens, hx, dOut, **kw):
    from summarymixing_amd.nnet.transducer import prediction_network
    _zero(dec, proj)
    hxg = tuple(t.detach().clone().requires_grad_(True) for t in hx) if hx is not None else None
    out = prediction_network(tokens, emb, dec, proj, hx=hxg, **kw)
    (out.float() * dOut.float()).sum().backward()
    g = _grads(dec, proj)
    if hx is not None:
        g.update(dh0=hxg[0].grad[0].clone(), dc0=hxg[1].grad[0].clone())
    return out.detach(), g


def _run_chain(emb, dec, proj, tokens, hx, dOut):
    _zero(dec, proj)
    hxg = tuple(t.detach().clone().requires_grad_(True) for t in hx) if hx is not None else None
    out = proj(dec(emb(tokens), hxg)[0])
    (out.float() * dOut.float()).sum().backward()
    g = _grads(dec, proj)
    if hx is not None:
        g.update(dh0=hxg[0].grad[0].clone(), dc0=hxg[1].grad[0].clone())
    return out.detach(), g


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,U1,V,H,J,blank,with_hx,long_seq", _FUSED)
def test_prediction_network_against_fp64_and_the_dropin_chain(B, U1, V, H, J, blank, with_hx, long_seq, dtype):
    """Fused path vs fp64; and fused == drop-in chain BIT FOR BIT in the output and every gradient but dW_ih and db_ih: a one-hot
    row times W_ih^T sums one exact product and zeros in fp32, so the GEMM's Gx is fl(w + bias) like the gather's, and everything
    downstream sees the same bits.  dW_ih and db_ih add the same fp32 terms in another order (the input wgrad GEMM's tiles and
    its fused column sums vs ascending rows / the standalone column-sum kernel): each path is within (n - 1) 2^-24 sum|terms| of
    the exact sum of its n terms, so the two are within twice that - n = the rows sharing the token for dW_ih, B U for db_ih."""
    emb, dec, proj = _modules(V, H, J, blank, dtype, seed=B + U1)
    g = torch.Generator().manual_seed(200 + B)
    tokens = _tokens(B, U1, V, blank, 300 + B)
    hx = ((0.5 * torch.randn(1, B, H, generator=g)).to(dtype).cuda(), torch.randn(1, B, H, generator=g).cuda()) if with_hx else None
    dOut = torch.randn(B, U1, J, generator=g).to(dtype)
    out, gr = _run_fused(emb, dec, proj, tokens.cuda(), hx, dOut.cuda())
    assert out.shape == (B, U1, J) and out.dtype == dtype
    kw = dict(params=_ref_params(dec, dtype), tokens=tokens, V=V, blank=blank, h0=hx[0][0].cpu() if with_hx else None,
              c0=hx[1][0].cpu() if with_hx else None, w_proj=_rounded(proj.w.weight.detach().cpu(), dtype), dOut=dOut)
    ref, emu = R.floor_and_ref(dtype, **kw)
    _judge(f"prediction_network B{B} U{U1} V{V} H{H} {dtype}", {"out": out, **gr}, ref, emu, dtype, careful=dtype == BF16 or long_seq)
    out_c, gr_c = _run_chain(emb, dec, proj, tokens.cuda(), hx, dOut.cuda())
    assert torch.equal(out, out_c)
    for k in gr:
        if k not in ("dw_ih", "db_ih"):
            assert torch.equal(gr[k], gr_c[k]), k
    c = int(torch.bincount(tokens.reshape(-1)).max())
    gabs = ref["dG"].abs().reshape(B * U1, -1)
    assert float((gr["dw_ih"] - gr_c["dw_ih"]).abs().max()) <= 2 * max(c * (c - 1), 1) * 2.0 ** -24 * float(gabs.max()) * 1.01
    bound = 2 * (B * U1 - 1) * 2.0 ** -24 * gabs.sum(0) * 1.01 + 1e-30
    assert bool(((gr["db_ih"] - gr_c["db_ih"]).abs().cpu().double() <= bound).all())


def test_backward_is_bit_reproducible_and_accumulates():
    B, U1, V, H, J = 6, 12, 9, 64, 64                           # 72 tokens over 9 symbols: every column of the scatter repeats
    for dtype in (F32, BF16):
        emb, dec, proj = _modules(V, H, J, 4, dtype, seed=1)
        tokens = _tokens(B, U1, V, 4, 5).cuda()
        dOut = torch.randn(B, U1, J, generator=torch.Generator().manual_seed(6)).to(dtype).cuda()
        o1, g1 = _run_fused(emb, dec, proj, tokens, None, dOut)
        o2, g2 = _run_fused(emb, dec, proj, tokens, None, dOut)
        assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)
        from summarymixing_amd.nnet.transducer import prediction_network
        (prediction_network(tokens, emb, dec, proj).float() * dOut.float()).sum().backward()      # a second backward, grads kept
        g3 = _grads(dec, proj)
        for k in g1:
            assert torch.equal(g3[k], 2 * g1[k]), k


def test_captured_step_replays_the_eager_run():
    from summarymixing_amd.nnet.transducer import prediction_network
    B, U1, V, H, J = 4, 10, 16, 64, 64
    emb, dec, proj = _modules(V, H, J, 0, BF16, seed=8)
    tokens = _tokens(B, U1, V, 0, 9).cuda()
    dOut = torch.randn(B, U1, J, generator=torch.Generator().manual_seed(10)).to(BF16).cuda()

    def step():
        out = prediction_network(tokens, emb, dec, proj)
        (out.float() * dOut.float()).sum().backward()
        return out

    _zero(dec, proj)
    ref = step().detach().clone()
    ref_g = _grads(dec, proj)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    params = [dec.rnn.weight_ih_l0, dec.rnn.weight_hh_l0, dec.rnn.bias_ih_l0, dec.rnn.bias_hh_l0, proj.w.weight]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for p in params:
        p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    g = _grads(dec, proj)
    for k in ref_g:
        assert torch.equal(g[k], ref_g[k]), k


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_training_dropout_uses_the_exposed_masks(dtype):
    from summarymixing_amd import ops
    from summarymixing_amd.nnet.transducer import prediction_network_masks
    B, U1, V, H, J, blank = 16, 40, 50, 64, 64, 0
    p_emb, p_dec = 0.2, 0.1
    emb, dec, proj = _modules(V, H, J, blank, dtype, seed=12)
    tokens = _tokens(B, U1, V, blank, 13)
    dOut = torch.randn(B, U1, J, generator=torch.Generator().manual_seed(14)).to(dtype)
    torch.manual_seed(77)
    saved = ops._drop_state["counter"]                                          # the library's seed stream is global: put it back
    try:
        ops._drop_state["counter"] = 4000
        keep, hmask = prediction_network_masks(B, U1, H, p_emb, p_dec, "cuda")
        ops._drop_state["counter"] = 4000
        out, gr = _run_fused(emb, dec, proj, tokens.cuda(), None, dOut.cuda(), emb_dropout=p_emb, dec_dropout=p_dec, training=True)
        used = ops._drop_state["counter"]
    finally:
        ops._drop_state["counter"] = saved
    assert used == 4002                                   # one seed per site
    keep, hmask = keep.cpu(), hmask.cpu()
    assert set(keep.unique().tolist()) <= {0.0, float(torch.tensor(1 / (1 - p_emb), dtype=F32))}
    for m, p in ((keep, p_emb), (hmask, p_dec)):                                # keep rate inside a binomial 5-sigma interval
        n, rate = m.numel(), float((m != 0).double().mean())
        assert abs(rate - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, (rate, p, n)
    kw = dict(params=_ref_params(dec, dtype), tokens=tokens, V=V, blank=blank, keep=keep, hmask=hmask,
              w_proj=_rounded(proj.w.weight.detach().cpu(), dtype), dOut=dOut)
    ref, emu = R.floor_and_ref(dtype, **kw)
    _judge(f"prediction_network dropout {dtype}", {"out": out, **gr}, ref, emu, dtype, careful=dtype == BF16)
    out_eval, _ = _run_fused(emb, dec, proj, tokens.cuda(), None, dOut.cuda(), emb_dropout=p_emb, dec_dropout=p_dec, training=False)
    assert not torch.equal(out_eval, out)


def test_whole_head_in_one_step_against_fp64():
    """tokens -> prediction_network -> transducer_joint_loss with an encoder-side tensor: loss and every gradient."""
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.transducer import Transducer_joint, prediction_network, transducer_joint_loss
    from tests._rnnt_ref import joint_ref, rnnt_loss
    B, T, U, V, H, J, blank = 3, 12, 5, 16, 32, 64, 0
    emb, dec, proj = _modules(V, H, J, blank, F32, seed=20)
    torch.manual_seed(21)
    lin = Linear(V, input_size=J, bias=False).cuda()
    tj = Transducer_joint(joint="sum", nonlinearity=torch.nn.LeakyReLU)
    g = torch.Generator().manual_seed(22)
    targets = torch.randint(1, V, (B, U), generator=g)
    tokens = torch.cat([torch.full((B, 1), blank), targets], 1)
    in_rel, tg_rel = torch.tensor([1.0, 0.75, 0.5]), torch.tensor([1.0, 0.6, 0.8])
    enc = torch.randn(B, T, J, generator=g)
    e = enc.cuda().requires_grad_(True)
    _zero(dec, proj, lin)
    d = prediction_network(tokens.cuda(), emb, dec, proj)
    loss = transducer_joint_loss(e, d, tj, lin, targets.cuda(), in_rel.cuda(), tg_rel.cuda(), blank)
    loss.backward()
    # fp64: the same graph with autograd from the joint on, the prediction network by explicit BPTT
    wp, wl = proj.w.weight.detach().cpu().double(), lin.w.weight.detach().cpu().double().requires_grad_(True)
    fwd = R.run(params=_ref_params(dec, F32), tokens=tokens, V=V, blank=blank, w_proj=wp)
    d_ref = fwd["out"].clone().requires_grad_(True)
    e_ref = enc.double().requires_grad_(True)
    ref_loss = rnnt_loss(joint_ref(e_ref, d_ref, torch.nn.LeakyReLU()) @ wl.t(), targets, in_rel, tg_rel, blank)
    ref_loss.backward()
    ref = R.run(params=_ref_params(dec, F32), tokens=tokens, V=V, blank=blank, w_proj=wp, dOut=d_ref.grad)
    tol = TOL[F32][1]
    errs = {"loss": rel_err(loss, ref_loss), "d_enc": rel_err(e.grad, e_ref.grad), "dw_lin": rel_err(lin.w.weight.grad, wl.grad)}
    errs.update({k: rel_err(v, ref[k]) for k, v in _grads(dec, proj).items()})
    report("prediction_network whole head f32", errs)
    assert all(v <= tol for v in errs.values()), errs


# ---- the weight images of the parameter holder (functional.derived) ------------------------------------------------------------
@pytest.mark.parametrize("name", ["WihT", "bsum0"])
def test_a_weight_image_is_kept_until_its_source_changes(name):
    """Kept between calls; rebuilt after an in-place change of a source and after functional.weights_changed(); inside a graph
    capture nothing is stored on the holder."""
    from summarymixing_amd import functional as F
    from summarymixing_amd.nnet.RNN import lstm_apply
    V, H = 9, 32
    emb, dec, _ = _modules(V, H, 8, 0, F32, seed=11)
    p = dec.rnn
    tokens = _tokens(2, 3, V, 0, 12).cuda()
    if name == "WihT":
        src, fresh = p.weight_ih_l0, lambda: p.weight_ih_l0.detach().t().contiguous()
    else:
        src, fresh = p.bias_hh_l0, lambda: p.bias_ih_l0.detach() + p.bias_hh_l0.detach()

    def run():
        with torch.no_grad():
            lstm_apply(tokens, None, dec, onehot=(V, 0, None, F32))

    def image():
        run()
        return p._derived[name][2]

    a = image()
    assert image() is a and torch.equal(a, fresh())
    with torch.no_grad():
        src.add_(1)
    b = image()
    assert b is not a and torch.equal(b, fresh()) and not torch.equal(b, a)
    F.weights_changed()
    c = image()
    assert c is not b and torch.equal(c, fresh())
    p._derived.clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    assert not p._derived
    assert torch.equal(image(), fresh())

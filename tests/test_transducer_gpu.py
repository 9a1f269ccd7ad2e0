"""Transducer head on the GPU: the joint, the RNN-T loss on given logits and the fused joint -> transducer_lin -> loss path against
the fp64 restatement in tests/_rnnt_ref.py; fused == drop-in chain; memory, bit-reproducibility, graph capture and a multitask
step through the encoder."""
import pytest
import torch

from tests._rnnt_ref import abs_lengths, joint_ref, rnnt_loss
from tests._util import rel_err

pytestmark = pytest.mark.gpu

ACTS = [torch.nn.GELU, torch.nn.LeakyReLU, torch.nn.ReLU]


def _modules(J, V, bias, act=torch.nn.GELU, seed=0):
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.transducer import Transducer_joint
    torch.manual_seed(seed)
    lin = Linear(V, input_size=J, bias=bias)
    with torch.no_grad():
        lin.w.weight.mul_(2.0)
        if bias:
            lin.w.bias.uniform_(-0.5, 0.5)
    return Transducer_joint(joint="sum", nonlinearity=act), lin.cuda()


def _lattice(B, T, U, V, seed, ub0=False, blank=0):
    g = torch.Generator().manual_seed(seed)
    targets = torch.randint(0, V - 1, (B, U), generator=g)
    targets = targets + (targets >= blank)                # every column but the blank (blank 0: the same draws as randint(1, V))
    in_rel = 0.5 + 0.5 * torch.rand(B, generator=g)
    tg_rel = 0.3 + 0.7 * torch.rand(B, generator=g)
    in_rel[0], tg_rel[0] = 1.0, 1.0
    if ub0:
        tg_rel[-1] = 0.0                                  # an utterance with no label: U_b = 0
    return targets, in_rel, tg_rel


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.bfloat16, 1e-2)])
@pytest.mark.parametrize("act", ACTS, ids=lambda a: a.__name__)
def test_joint_forward_and_backward_match_fp64(act, dtype, tol):
    from summarymixing_amd.nnet.transducer import Transducer_joint
    g = torch.Generator().manual_seed(7)
    B, T, U1, J = 3, 23, 9, 72
    enc = (torch.randn(B, T, J, generator=g) * 1.5).to(dtype)
    dec = (torch.randn(B, U1, J, generator=g) * 1.5).to(dtype)
    gH = torch.randn(B, T, U1, J, generator=g).to(dtype)
    er, dr = enc.double().requires_grad_(True), dec.double().requires_grad_(True)
    ref = joint_ref(er, dr, act())
    ref.backward(gH.double())
    e = enc.cuda().unsqueeze(2).requires_grad_(True)
    d = dec.cuda().unsqueeze(1).requires_grad_(True)
    H = Transducer_joint(nonlinearity=act)(e, d)
    assert H.shape == (B, T, U1, J) and H.dtype == dtype
    H.backward(gH.cuda())
    assert rel_err(H, ref) <= tol
    assert rel_err(e.grad.squeeze(2), er.grad) <= tol and rel_err(d.grad.squeeze(1), dr.grad) <= tol
    assert e.grad.dtype == dtype


_SHAPES = [(3, 50, 9, 32), (4, 120, 40, 1000), (2, 40, 300, 64), (2, 1, 5, 16)]


def _loss_case(B, T, U, V, dtype, reduction, seed, blank=0, w=None):
    """w: per-utterance weights of a 'none' loss (a non-uniform upstream gradient); None: the plain sum."""
    from summarymixing_amd.nnet.losses import transducer_loss
    targets, in_rel, tg_rel = _lattice(B, T, U, V, seed, ub0=B > 2, blank=blank)
    logits = (torch.randn(B, T, U + 1, V, generator=torch.Generator().manual_seed(seed + 1)) * 2.0).to(dtype)
    xr = logits.double().requires_grad_(True)
    ref = rnnt_loss(xr, targets, in_rel, tg_rel, blank, reduction)
    ((ref if w is None else ref * w.double()).sum() if reduction == "none" else ref).backward()
    x = logits.cuda().requires_grad_(True)
    loss = transducer_loss(x, targets.cuda(), in_rel.cuda(), tg_rel.cuda(), blank, reduction=reduction, use_torchaudio=False)
    ((loss if w is None else loss * w.cuda()).sum() if reduction == "none" else loss).backward()
    return loss, ref, x, xr, in_rel, tg_rel


def _loss_matches_fp64(B, T, U, V, dtype, tl, tg, blank):
    loss, ref, x, xr, in_rel, tg_rel = _loss_case(B, T, U, V, dtype, "mean", 300 + T + U, blank=blank)
    assert loss.dtype == torch.float32 and loss.shape == ()
    assert abs(loss.item() - ref.item()) <= tl * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    assert x.grad.dtype == dtype
    assert rel_err(x.grad, xr.grad) <= tg
    tl_, ul_ = abs_lengths(T, U, in_rel, tg_rel)
    for b in range(B):                                    # padding rows: exactly zero
        assert float(x.grad[b, tl_[b]:].abs().sum()) == 0.0 and float(x.grad[b, :, ul_[b] + 1:].abs().sum()) == 0.0


@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-5, 1e-4), (torch.bfloat16, 2e-2, 3e-2)])
@pytest.mark.parametrize("B,T,U,V", _SHAPES)
def test_transducer_loss_matches_fp64(B, T, U, V, dtype, tl, tg):
    _loss_matches_fp64(B, T, U, V, dtype, tl, tg, 0)


@pytest.mark.parametrize("dtype,tl,tg", [(torch.float32, 1e-5, 1e-4), (torch.bfloat16, 2e-2, 3e-2)])
@pytest.mark.parametrize("B,T,U,V", _SHAPES)
def test_transducer_loss_matches_fp64_blank_in_the_last_column(B, T, U, V, dtype, tl, tg):
    _loss_matches_fp64(B, T, U, V, dtype, tl, tg, V - 1)


@pytest.mark.parametrize("reduction", ["sum", "none"])
def test_transducer_loss_reductions(reduction):
    loss, ref, x, xr, _, _ = _loss_case(3, 50, 9, 32, torch.float32, reduction, 11)
    assert loss.shape == ref.shape
    assert rel_err(loss, ref) <= 1e-5 and rel_err(x.grad, xr.grad) <= 1e-4


_W = torch.tensor([0.25, -1.5, 3.0])                     # a non-uniform upstream gradient: gscale[b] of the wrong utterance shows


@pytest.mark.parametrize("blank", [0, 31])
def test_transducer_loss_non_uniform_upstream_gradient(blank):
    loss, ref, x, xr, _, _ = _loss_case(3, 50, 9, 32, torch.float32, "none", 11, blank=blank, w=_W)
    assert rel_err(loss, ref) <= 1e-5 and rel_err(x.grad, xr.grad) <= 1e-4
    for b in range(3):                                    # per utterance: the smallest weight is not hidden behind the largest
        assert rel_err(x.grad[b], xr.grad[b]) <= 1e-4, b


def _streams(B, T, U, J, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    enc = (torch.randn(B, T, J, generator=g) * 0.5).to(dtype)
    dec = (torch.randn(B, U + 1, J, generator=g) * 0.5).to(dtype)
    return enc, dec


def _backward(loss, w):
    (loss if w is None else (loss * w.to(loss.device, loss.dtype)).sum()).backward()


def _dropin(tj, lin, enc, dec, targets, in_rel, tg_rel, reduction="mean", blank=0, w=None):
    from summarymixing_amd.nnet.losses import transducer_loss
    e = enc.cuda().requires_grad_(True)
    d = dec.cuda().requires_grad_(True)
    lin.zero_grad(set_to_none=True)
    loss = transducer_loss(lin(tj(e.unsqueeze(2), d.unsqueeze(1))), targets.cuda(), in_rel.cuda(), tg_rel.cuda(), blank, reduction)
    _backward(loss, w)
    return loss.detach(), e.grad, d.grad, lin.w.weight.grad.clone(), (lin.w.bias.grad.clone() if lin.w.bias is not None else None)


def _fused(tj, lin, enc, dec, targets, in_rel, tg_rel, reduction="mean", four_d=False, blank=0, w=None):
    from summarymixing_amd.nnet.transducer import transducer_joint_loss
    e = enc.cuda().requires_grad_(True)
    d = dec.cuda().requires_grad_(True)
    lin.zero_grad(set_to_none=True)
    loss = transducer_joint_loss(e.unsqueeze(2) if four_d else e, d.unsqueeze(1) if four_d else d, tj, lin, targets.cuda(),
                                 in_rel.cuda(), tg_rel.cuda(), blank, reduction)
    _backward(loss, w)
    return loss.detach(), e.grad, d.grad, lin.w.weight.grad.clone(), (lin.w.bias.grad.clone() if lin.w.bias is not None else None)


def _ref_chain(tj, lin, enc, dec, targets, in_rel, tg_rel, reduction="mean", blank=0, w=None):
    e = enc.double().requires_grad_(True)
    d = dec.double().requires_grad_(True)
    W = lin.w.weight.detach().to(enc.dtype).double().cpu().requires_grad_(True)
    b = lin.w.bias.detach().double().cpu().requires_grad_(True) if lin.w.bias is not None else None
    z = joint_ref(e, d, type(tj.nonlinearity)()) @ W.t()
    if b is not None:
        z = z + b
    loss = rnnt_loss(z, targets, in_rel, tg_rel, blank, reduction)
    _backward(loss, w)
    return loss.detach(), e.grad, d.grad, W.grad, (b.grad if b is not None else None)


def _fused_equals_dropin_fp32(bias, act, blank, J=128, V=36, reduction="mean", w=None):
    B, T, U = 3, 20, 6                                   # 420 rows
    tj, lin = _modules(J, V, bias, act)
    enc, dec = _streams(B, T, U, J, torch.float32, 5)
    targets, in_rel, tg_rel = _lattice(B, T, U, V, 6, ub0=True, blank=blank)
    a = _dropin(tj, lin, enc, dec, targets, in_rel, tg_rel, reduction, blank=blank, w=w)
    f = _fused(tj, lin, enc, dec, targets, in_rel, tg_rel, reduction, four_d=True, blank=blank, w=w)
    r = _ref_chain(tj, lin, enc, dec, targets, in_rel, tg_rel, reduction, blank=blank, w=w)
    if w is None:
        assert abs(f[0].item() - a[0].item()) <= 1e-5 * abs(a[0].item())
    for i, name in enumerate(("loss", "enc", "dec", "weight", "bias")):
        if a[i] is None:
            assert f[i] is None and not bias
            continue
        assert rel_err(f[i], a[i]) <= 1e-5, name
        assert rel_err(f[i], r[i]) <= 1e-4, name
    return f, r


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", ACTS, ids=lambda a: a.__name__)
def test_fused_path_equals_dropin_chain_fp32(bias, act):
    _fused_equals_dropin_fp32(bias, act, 0)              # V = 36: not a multiple of the 128-column tile


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("act", ACTS, ids=lambda a: a.__name__)
def test_fused_path_equals_dropin_chain_fp32_blank_in_the_last_column(bias, act):
    _fused_equals_dropin_fp32(bias, act, 35)


@pytest.mark.parametrize("blank", [0, 999])
def test_fused_path_equals_dropin_chain_fp32_at_the_recipe_width(blank):
    """V = 1000, J = 640 in fp32: eight column tiles, the last ragged (the only fp32 run of the cross-tile combine end to end)."""
    _fused_equals_dropin_fp32(True, torch.nn.GELU, blank, J=640, V=1000)


@pytest.mark.parametrize("blank", [0, 35])
def test_fused_path_non_uniform_upstream_gradient(blank):
    f, r = _fused_equals_dropin_fp32(True, torch.nn.GELU, blank, reduction="none", w=_W)
    for b in range(3):                                    # the stream gradients per utterance
        assert rel_err(f[1][b], r[1][b]) <= 1e-4 and rel_err(f[2][b], r[2][b]) <= 1e-4, b


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 2e-2)], ids=["f32", "bf16"])
def test_fused_backward_utterance_groups(monkeypatch, dtype, tol):
    """B = 5 with one utterance per backward group, two per group (the last group short) and all in one: groups are whole
    utterances and every reduction has a fixed order, so the stream gradients are bit-identical; the weight and bias gradients add
    the groups in another order (fp32: within 1e-5 of each other); everything within the path's bar of fp64."""
    import summarymixing_amd.nnet.transducer as TR
    B, T, U, J, V = 5, 20, 6, 128, 132
    per = T * (U + 1)
    tj, lin = _modules(J, V, True, seed=5)
    enc, dec = _streams(B, T, U, J, dtype, 31)
    targets, in_rel, tg_rel = _lattice(B, T, U, V, 32, ub0=True, blank=V - 1)
    w = torch.tensor([0.25, -1.5, 3.0, 1.0, 0.5])
    r = _ref_chain(tj, lin, enc, dec, targets, in_rel, tg_rel, "none", blank=V - 1, w=w)
    runs = []
    for group_rows in (per, 2 * per + 1, 1 << 30):       # 1 + 1 + 1 + 1 + 1, 2 + 2 + 1, 5
        monkeypatch.setattr(TR, "_BWD_GROUP_ROWS", group_rows)
        runs.append(_fused(tj, lin, enc, dec, targets, in_rel, tg_rel, "none", blank=V - 1, w=w))
    for f in runs:
        for i in range(5):
            assert rel_err(f[i], r[i]) <= tol, i
    for f in runs[:2]:
        assert torch.equal(f[0], runs[2][0])
        assert torch.equal(f[1], runs[2][1]), "d_enc differs between group sizes"
        assert torch.equal(f[2], runs[2][2]), "d_dec differs between group sizes"
        if dtype == torch.float32:
            assert rel_err(f[3], runs[2][3]) <= 1e-5 and rel_err(f[4], runs[2][4]) <= 1e-5


def test_fused_path_and_dropin_chain_bf16_against_fp64():
    B, T, U, J, V = 3, 20, 6, 128, 36
    tj, lin = _modules(J, V, True)
    enc, dec = _streams(B, T, U, J, torch.bfloat16, 8)
    targets, in_rel, tg_rel = _lattice(B, T, U, V, 9, ub0=True)
    r = _ref_chain(tj, lin, enc, dec, targets, in_rel, tg_rel)
    for run in (_dropin, _fused):
        out = run(tj, lin, enc, dec, targets, in_rel, tg_rel)
        assert out[1].dtype == torch.bfloat16
        assert abs(out[0].item() - r[0].item()) <= 2e-2 * abs(r[0].item()), run.__name__
        for i in range(1, 5):
            assert rel_err(out[i], r[i]) <= 2e-2, (run.__name__, i)


def test_fused_path_at_the_recipe_width_bf16():
    B, T, U, J, V = 2, 375, 60, 640, 1000
    tj, lin = _modules(J, V, False, seed=1)
    with torch.no_grad():
        lin.w.weight.mul_(0.5)
    enc, dec = _streams(B, T, U, J, torch.bfloat16, 12)
    targets, in_rel, tg_rel = _lattice(B, T, U, V, 13)
    f = _fused(tj, lin, enc, dec, targets, in_rel, tg_rel)
    r = _ref_chain(tj, lin, enc, dec, targets, in_rel, tg_rel)
    assert abs(f[0].item() - r[0].item()) <= 2e-2 * abs(r[0].item())
    for i in range(1, 4):
        assert rel_err(f[i], r[i]) <= 3e-2, i


def test_fused_path_memory():
    """fp32 logits of this lattice: 73 200 x 1000 x 4 B = 293 MB.  The fused forward keeps H and 16 B per row; forward + backward
    stay below the fp32 logits."""
    from summarymixing_amd.nnet.transducer import transducer_joint_loss
    B, T, U, J, V = 4, 300, 60, 640, 1000
    rows = B * T * (U + 1)
    tj, lin = _modules(J, V, False, seed=2)
    enc, dec = _streams(B, T, U, J, torch.bfloat16, 14)
    targets, in_rel, tg_rel = _lattice(B, T, U, V, 15)
    e, d = enc.cuda().requires_grad_(True), dec.cuda().requires_grad_(True)
    tgc, irc, trc = targets.cuda(), in_rel.cuda(), tg_rel.cuda()
    transducer_joint_loss(e, d, tj, lin, tgc, irc, trc, 0).backward()     # warm-up: shadow weights, .grad tensors, workspaces
    e.grad = d.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    loss = transducer_joint_loss(e, d, tj, lin, tgc, irc, trc, 0)
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - m0
    assert kept <= rows * J * 2 + rows * 16 + (16 << 20), kept
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - m0
    assert peak < rows * V * 4, (peak, rows * V * 4)
    assert torch.isfinite(e.grad.float()).all() and torch.isfinite(lin.w.weight.grad).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_path_is_bit_reproducible(dtype):
    B, T, U, J, V = 3, 60, 12, 128, 100
    tj, lin = _modules(J, V, True, seed=3)
    enc, dec = _streams(B, T, U, J, dtype, 16)
    targets, in_rel, tg_rel = _lattice(B, T, U, V, 17)
    a = _fused(tj, lin, enc, dec, targets, in_rel, tg_rel)
    b = _fused(tj, lin, enc, dec, targets, in_rel, tg_rel)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_fused_path_replays_in_a_graph_bit_for_bit():
    from summarymixing_amd.nnet.transducer import transducer_joint_loss
    B, T, U, J, V = 2, 40, 8, 128, 64
    tj, lin = _modules(J, V, True, seed=4)
    enc, dec = _streams(B, T, U, J, torch.float32, 18)
    targets, in_rel, tg_rel = _lattice(B, T, U, V, 19)
    e, d = enc.cuda().requires_grad_(True), dec.cuda().requires_grad_(True)
    tgc, irc, trc = targets.cuda(), in_rel.cuda(), tg_rel.cuda()

    def step():
        loss = transducer_joint_loss(e, d, tj, lin, tgc, irc, trc, 0)
        loss.backward()
        return loss

    lin.zero_grad(set_to_none=True)
    ref = step().detach().clone()
    ref_g = [e.grad.clone(), d.grad.clone(), lin.w.weight.grad.clone(), lin.w.bias.grad.clone()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        e.grad = d.grad = None
        step()
    torch.cuda.current_stream().wait_stream(s)
    e.grad = d.grad = None
    lin.w.weight.grad.zero_()
    lin.w.bias.grad.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    lin.w.weight.grad.zero_()
    lin.w.bias.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    for x, y in zip([e.grad, d.grad, lin.w.weight.grad, lin.w.bias.grad], ref_g):
        assert torch.equal(x, y)


def test_multitask_ctc_plus_transducer_step_through_the_encoder():
    """0.3 ctc + 0.7 transducer back through EncoderWrapper (the CTC test's small Conformer): finite gradients, and the fused and
    drop-in transducer heads give the same encoder gradients."""
    from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    from summarymixing_amd.nnet.activations import Softmax
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.losses import ctc_loss, transducer_loss
    from summarymixing_amd.nnet.transducer import Transducer_joint, transducer_joint_loss
    torch.manual_seed(21)
    B, T, Fin, d, J, V, U = 3, 60, 80, 64, 64, 40, 8
    net = TransformerASR(tgt_vocab=V, input_size=Fin, d_model=d, nhead=4, num_encoder_layers=2, num_decoder_layers=0,
                         d_ffn=128, dropout=0.0, encoder_module="conformer", conformer_activation="swish",
                         attention_type="SummaryMixing", mode="SummaryMixing-fast", local_proj_out_dim=d,
                         local_proj_hid_dim=[d], summary_hid_dim=[d], summary_out_dim=d, causal=False, kernel_size=15)
    enc = EncoderWrapper(net).cuda()
    proj_enc, proj_ctc = Linear(J, input_size=d).cuda(), Linear(V, input_size=d).cuda()
    tj, lin = Transducer_joint(nonlinearity=torch.nn.GELU), Linear(V, input_size=J, bias=False).cuda()
    src = torch.randn(B, T, Fin).cuda()
    wav_len = torch.tensor([1.0, 0.7, 0.85]).cuda()
    targets = torch.randint(1, V, (B, U)).cuda()
    tg_rel = torch.tensor([1.0, 0.5, 0.75]).cuda()
    dec_src = torch.randn(B, U + 1, J).cuda()
    mods = [net, proj_enc, proj_ctc, lin]

    def run(fused):
        for m in mods:
            m.zero_grad(set_to_none=True)
        dec_out = dec_src.clone().requires_grad_(True)
        x = enc(src, wav_len)
        ctc = ctc_loss(Softmax(apply_log=True)(proj_ctc(x)), targets, wav_len, tg_rel, 0)
        h = proj_enc(x)
        if fused:
            tr = transducer_joint_loss(h, dec_out, tj, lin, targets, wav_len, tg_rel, 0)
        else:
            tr = transducer_loss(lin(tj(h.unsqueeze(2), dec_out.unsqueeze(1))), targets, wav_len, tg_rel, 0)
        loss = 0.3 * ctc + 0.7 * tr
        loss.backward()
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
        grads["proj_enc"] = proj_enc.w.weight.grad.clone()
        grads["lin"] = lin.w.weight.grad.clone()
        grads["dec_out"] = dec_out.grad.clone()
        return loss.detach(), grads

    la, ga = run(False)
    lf, gf = run(True)
    assert torch.isfinite(la) and abs(lf.item() - la.item()) <= 1e-5 * abs(la.item())
    assert len(ga) > 10 and ga.keys() == gf.keys()
    for k in ga:
        assert torch.isfinite(ga[k]).all() and torch.isfinite(gf[k]).all(), k
        assert rel_err(gf[k], ga[k]) <= 1e-5, k

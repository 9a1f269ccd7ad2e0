"""Transducer head, CPU side: the fp64 RNN-T reference against brute-force enumeration of alignments (the yardstick of the GPU
tests), and the module / loss / fused-entry surface with its refusals (no GPU needed: every case is refused before a launch)."""
import pytest
import torch

from tests._rnnt_ref import _nll_one, abs_lengths, brute_force_nll, lattice, logit_grad, rnnt_nll, row_stats


def _brute_force_case(T, U, Tb, Ub, blank):
    g = torch.Generator().manual_seed(10 * T + U + Tb + Ub)
    V = 5
    logits = (torch.randn(1, T, U + 1, V, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    targets = torch.randint(0, V - 1, (1, U), generator=g)
    targets = targets + (targets >= blank)                # every column but the blank (blank 0: the labels 1 .. V - 1 as before)
    nll = rnnt_nll(logits, targets, torch.tensor([Tb]), torch.tensor([Ub]), blank)[0]
    (g_ref,) = torch.autograd.grad(nll, logits)
    x = logits.detach().clone().requires_grad_(True)
    bf = brute_force_nll(x[0], targets[0], Tb, Ub, blank)
    (g_bf,) = torch.autograd.grad(bf, x)
    assert abs(nll.item() - bf.item()) <= 1e-12 * max(1.0, abs(bf.item()))
    assert float((g_ref - g_bf).abs().max()) <= 1e-12
    # rows outside t < Tb, u <= Ub take no part
    assert float(g_ref[0, Tb:].abs().sum() + g_ref[0, :, Ub + 1:].abs().sum()) == 0.0


_TINY = [(4, 3, 4, 3), (4, 3, 3, 2), (3, 2, 1, 2), (4, 3, 2, 0), (1, 1, 1, 1), (2, 0, 2, 0)]


@pytest.mark.parametrize("T,U,Tb,Ub", _TINY)
def test_reference_equals_brute_force_enumeration(T, U, Tb, Ub):
    _brute_force_case(T, U, Tb, Ub, 0)


@pytest.mark.parametrize("blank", [2, 4])                 # a middle column and V - 1 (V = 5)
@pytest.mark.parametrize("T,U,Tb,Ub", _TINY)
def test_reference_equals_brute_force_enumeration_off_blank_0(T, U, Tb, Ub, blank):
    _brute_force_case(T, U, Tb, Ub, blank)


_STAGE = [(6, 4, 6, 4, 0), (6, 4, 4, 2, 3), (5, 7, 5, 7, 6), (9, 3, 1, 3, 2), (4, 5, 3, 0, 6), (3, 0, 3, 0, 0), (30, 12, 27, 9, 6)]


@pytest.mark.parametrize("T,U,Tb,Ub,blank", _STAGE)
def test_lattice_occupancies_are_minus_the_gradient_of_the_reference(T, U, Tb, Ub, blank):
    """The explicit forward / backward recursions of `lattice` against autograd through the anti-diagonal recurrence of rnnt_nll:
    the occupancies are minus the gradient of -log P with respect to the gathered log-probabilities; -log P from alpha equals
    -beta(0, 0)."""
    g = torch.Generator().manual_seed(1000 + 10 * T + U + blank)
    V = 7
    targets = torch.randint(0, V - 1, (U,), generator=g)
    targets = targets + (targets >= blank)
    lp = (torch.randn(T, U + 1, V, generator=g, dtype=torch.float64) * 1.5).log_softmax(-1).requires_grad_(True)
    nll = _nll_one(lp, targets, Tb, Ub, blank)            # the body of rnnt_nll, on the log-probabilities themselves
    (glp,) = torch.autograd.grad(nll, lp)
    lpb = lp.detach()[:, :, blank]
    lpy = torch.zeros(T, U + 1, dtype=torch.float64)
    if U > 0:
        lpy[:, :U] = lp.detach()[:, :U].gather(2, targets.view(1, U, 1).expand(T, U, 1)).squeeze(2)
    alpha, nl, occ_b, occ_y, beta = lattice(lpb, lpy, Tb, Ub, with_beta=True)
    assert abs(nl - nll.item()) <= 1e-12 * max(1.0, abs(nll.item()))
    assert abs(nl + beta[0, 0]) <= 1e-12 * max(1.0, abs(nl))
    assert alpha.shape == (Tb, Ub + 1) and alpha[0, 0] == 0.0
    ref_b = -glp[:Tb, :Ub + 1, blank]
    assert float((torch.from_numpy(occ_b) - ref_b).abs().max()) <= 1e-12
    if Ub > 0:
        ref_y = -glp[:Tb, :Ub].gather(2, targets[:Ub].view(1, Ub, 1).expand(Tb, Ub, 1)).squeeze(2)
        assert float((torch.from_numpy(occ_y[:, :Ub]) - ref_y).abs().max()) <= 1e-12
    assert float(abs(occ_y[:, Ub]).max()) == 0.0
    # flow conservation: what enters the lattice leaves through the last blank
    assert abs(occ_b[Tb - 1, Ub] - 1.0) <= 1e-12


@pytest.mark.parametrize("T,U,Tb,Ub,blank", _STAGE)
def test_stage_functions_compose_to_the_gradient_of_the_reference(T, U, Tb, Ub, blank):
    """row_stats -> lattice -> logit_grad on raw logits equals torch.autograd.grad of rnnt_nll (two utterances, the second one at
    the given lengths, a non-uniform upstream gradient)."""
    g = torch.Generator().manual_seed(2000 + 10 * T + U + blank)
    V, B = 7, 2
    targets = torch.randint(0, V - 1, (B, U), generator=g)
    targets = targets + (targets >= blank)
    z = (torch.randn(B, T, U + 1, V, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    tl, ul = torch.tensor([T, Tb]), torch.tensor([U, Ub])
    w = torch.tensor([-1.5, 0.25], dtype=torch.float64)
    nll = rnnt_nll(z, targets, tl, ul, blank)
    (gz,) = torch.autograd.grad((nll * w).sum(), z)
    lse, lpb, lpy = row_stats(z.detach(), targets, blank)
    gb, gy = torch.zeros_like(lse), torch.zeros_like(lse)
    for b in range(B):
        _, nl, ob, oy = lattice(lpb[b], lpy[b], int(tl[b]), int(ul[b]))
        assert abs(nl - nll[b].item()) <= 1e-12 * max(1.0, abs(nl))
        gb[b, :tl[b], :ul[b] + 1] = -w[b] * torch.from_numpy(ob)               # g = -gscale * occupancy, as the kernels define it
        gy[b, :tl[b], :ul[b] + 1] = -w[b] * torch.from_numpy(oy)
    dz = logit_grad(z.detach(), targets, blank, lse, gb, gy)
    assert float((dz - gz).abs().max()) <= 1e-12


def test_abs_lengths_round_the_fp32_product_like_the_library():
    from summarymixing_amd.nnet.losses import transducer_lengths
    rel = torch.tensor([0.1, 0.3, 0.5, 0.7, 0.9, 1.0, 0.02])
    for T, U in [(25, 5), (15, 35), (45, 25), (50, 9)]:
        tl, ul = abs_lengths(T, U, rel, rel)
        _, il, gl = transducer_lengths(T, torch.zeros(len(rel), U, dtype=torch.long), rel, rel, "cpu")
        assert torch.equal(tl, il.long().clamp(1, T)) and torch.equal(ul, gl.long().clamp(0, U))
    assert int(abs_lengths(25, 25, torch.tensor([0.1]), torch.tensor([0.1]))[0]) == 2      # 0.1f * 25 == 2.5f -> 2 (half to even)


def test_transducer_joint_constructs_with_the_recipe_arguments():
    from summarymixing_amd import _lib as L
    from summarymixing_amd.nnet.transducer.transducer_joint import Transducer_joint
    j = Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU)
    assert j.act == L.ACT_GELU and isinstance(j.nonlinearity, torch.nn.GELU)
    assert len(j.state_dict()) == 0 and len(list(j.parameters())) == 0
    assert Transducer_joint().act == L.ACT_LEAKY_RELU                     # SpeechBrain's default
    assert Transducer_joint(nonlinearity=torch.nn.ReLU).act == L.ACT_RELU
    from summarymixing_amd.nnet.transducer import Transducer_joint as T2
    assert T2 is Transducer_joint


def test_transducer_joint_refuses_what_it_does_not_implement():
    from summarymixing_amd.nnet.transducer.transducer_joint import Transducer_joint
    with pytest.raises(NotImplementedError):
        Transducer_joint(joint="concat", nonlinearity=torch.nn.GELU)
    with pytest.raises(NotImplementedError):
        Transducer_joint(joint_network=torch.nn.Linear(4, 4))
    with pytest.raises(NotImplementedError):
        Transducer_joint(nonlinearity=torch.nn.Tanh)
    with pytest.raises(NotImplementedError):
        Transducer_joint(nonlinearity=lambda: torch.nn.GELU(approximate="tanh"))
    j = Transducer_joint(nonlinearity=torch.nn.GELU)
    with pytest.raises(NotImplementedError):                              # the 1-D decoding form
        j(torch.randn(8), torch.randn(8))
    with pytest.raises(NotImplementedError):
        j(torch.randn(2, 8), torch.randn(2, 8))
    with pytest.raises(RuntimeError):                                     # no CPU fallback
        j(torch.randn(2, 5, 1, 8), torch.randn(2, 1, 4, 8))
    with pytest.raises(ValueError):
        j(torch.randn(2, 5, 1, 8), torch.randn(2, 1, 4, 12))


def test_transducer_loss_refuses_cpu_tensors_and_unknown_reductions():
    from summarymixing_amd.nnet.losses import transducer_loss
    logits = torch.randn(2, 5, 4, 7)
    targets = torch.randint(1, 7, (2, 3))
    lens = torch.tensor([1.0, 0.6])
    with pytest.raises(RuntimeError):
        transducer_loss(logits, targets, lens, lens, 0)
    with pytest.raises(RuntimeError):
        transducer_loss(logits, targets, lens, lens, 0, reduction="sum", use_torchaudio=False)
    for bad in ("batchmean", "batch", "avg"):
        with pytest.raises(ValueError):
            transducer_loss(logits, targets, lens, lens, 0, reduction=bad)


def _head(J=64, V=32, bias=False):
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.transducer.transducer_joint import Transducer_joint
    return Transducer_joint(nonlinearity=torch.nn.GELU), Linear(V, input_size=J, bias=bias)


@pytest.mark.parametrize("case", ["B", "J", "V_vs_J", "targets_U", "targets_B", "blank", "J_align", "V_align", "reduction", "T_form"])
def test_fused_entry_refuses_mismatched_shapes_before_any_launch(case):
    from summarymixing_amd.nnet.transducer import transducer_joint_loss
    B, T, U, J, V = 2, 6, 3, 64, 32
    enc, dec = torch.randn(B, T, J), torch.randn(B, U + 1, J)
    targets = torch.randint(1, V, (B, U))
    lens = torch.ones(B)
    tj, lin = _head(J, V)
    kw = dict(blank_index=0, reduction="mean")
    if case == "B":
        dec = torch.randn(B + 1, U + 1, J)
    elif case == "J":
        dec = torch.randn(B, U + 1, J + 64)
    elif case == "V_vs_J":
        tj, lin = _head(J, V)
        lin.w = torch.nn.Linear(J + 64, V, bias=False)
    elif case == "targets_U":
        targets = torch.randint(1, V, (B, U + 1))
    elif case == "targets_B":
        targets = torch.randint(1, V, (B + 1, U))
    elif case == "blank":
        kw["blank_index"] = V
    elif case == "J_align":
        enc, dec = torch.randn(B, T, 96), torch.randn(B, U + 1, 96)
        tj, lin = _head(96, V)
    elif case == "V_align":
        tj, lin = _head(J, 30)
    elif case == "reduction":
        kw["reduction"] = "batchmean"
    elif case == "T_form":
        enc = torch.randn(B, T, 2, J)
    with pytest.raises(ValueError):
        transducer_joint_loss(enc, dec, tj, lin, targets, lens, lens, **kw)


def test_fused_entry_refuses_cpu_tensors():
    from summarymixing_amd.nnet.transducer import transducer_joint_loss
    tj, lin = _head()
    with pytest.raises(RuntimeError):
        transducer_joint_loss(torch.randn(2, 6, 1, 64), torch.randn(2, 1, 4, 64), tj, lin, torch.randint(1, 32, (2, 3)),
                              torch.ones(2), torch.ones(2), 0)

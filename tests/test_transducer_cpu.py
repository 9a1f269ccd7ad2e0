"""Transducer head, CPU side: the fp64 RNN-T reference against brute-force enumeration of alignments (the yardstick of the GPU
tests), and the module / loss / fused-entry surface with its refusals (no GPU needed: every case is refused before a launch)."""
import pytest
import torch

from tests._rnnt_ref import brute_force_nll, rnnt_nll


@pytest.mark.parametrize("T,U,Tb,Ub", [(4, 3, 4, 3), (4, 3, 3, 2), (3, 2, 1, 2), (4, 3, 2, 0), (1, 1, 1, 1), (2, 0, 2, 0)])
def test_reference_equals_brute_force_enumeration(T, U, Tb, Ub):
    g = torch.Generator().manual_seed(10 * T + U + Tb + Ub)
    V, blank = 5, 0
    logits = (torch.randn(1, T, U + 1, V, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    targets = torch.randint(1, V, (1, U), generator=g)
    nll = rnnt_nll(logits, targets, torch.tensor([Tb]), torch.tensor([Ub]), blank)[0]
    (g_ref,) = torch.autograd.grad(nll, logits)
    x = logits.detach().clone().requires_grad_(True)
    bf = brute_force_nll(x[0], targets[0], Tb, Ub, blank)
    (g_bf,) = torch.autograd.grad(bf, x)
    assert abs(nll.item() - bf.item()) <= 1e-12 * max(1.0, abs(bf.item()))
    assert float((g_ref - g_bf).abs().max()) <= 1e-12
    # rows outside t < Tb, u <= Ub take no part
    assert float(g_ref[0, Tb:].abs().sum() + g_ref[0, :, Ub + 1:].abs().sum()) == 0.0


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

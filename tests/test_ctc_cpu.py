"""CTC head, CPU side: the fp64 restatement of tests/_ctc_ref.py (the yardstick of tests/test_ctc_kernels_gpu.py) is itself checked,
against brute-force enumeration of the frame labellings and against torch's float64 ctc_loss and its autograd gradient."""
import math

import numpy as np
import pytest
import torch

from tests._ctc_ref import abs_lengths, adjacent_repeats, ctc_brute_force, ctc_grad, ctc_lattice, log_softmax_bwd_ref

_V = 4

# (T, targets, blank): a repeated label, S = 0, a tight repeat case (T == S + repeats: one alignment), an infeasible one
# (S <= T < S + repeats) and plain ones; T <= 6, S <= 3
_TINY = [(5, [1, 2], 0), (6, [1, 1, 2], 0), (4, [], 0), (1, [], 2), (4, [1, 1, 2], 0), (3, [1, 1, 2], 0), (5, [3, 3, 3], 0),
         (4, [3, 3, 3], 0), (6, [0, 3, 0], 1), (5, [2, 2], 3), (3, [2, 2], 3), (2, [2, 2], 3), (1, [1], 0), (6, [0, 1, 1], 3)]


@pytest.mark.parametrize("T,tg,blank", _TINY)
def test_lattice_equals_brute_force_enumeration(T, tg, blank):
    g = torch.Generator().manual_seed(100 * T + len(tg) + blank)
    lp = (torch.randn(T + 2, _V, generator=g, dtype=torch.float64) * 1.5).log_softmax(-1)     # (two frames beyond Tb: not read)
    S = len(tg)
    alpha, nll, occ = ctc_lattice(lp, tg, T, S, blank)
    bf = ctc_brute_force(lp, tg, T, S, blank)
    need = S + adjacent_repeats(tg, S)
    assert math.isfinite(bf) == (T >= need)
    if T < need:
        assert nll == math.inf and bool(np.isneginf(occ).all())
        return
    assert abs(nll - bf) <= 1e-12 * max(1.0, abs(bf)), (nll, bf)
    # every frame is in exactly one state: the occupancies alpha beta / y of a frame sum to P
    mass = np.exp(occ + nll).sum(axis=1)
    assert float(np.abs(mass - 1.0).max()) <= 1e-12
    if T == need:                                         # the single alignment: every live state carries the whole mass
        assert int(np.isfinite(occ).sum()) == T and float(np.abs(occ[np.isfinite(occ)] + nll).max()) <= 1e-12


def _torch_case(B, T, V, S, blank, seed, minus_inf_column=None):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, V, generator=g, dtype=torch.float64) * 1.5
    if minus_inf_column is not None:
        logits[..., minus_inf_column] = -math.inf
    labels = torch.tensor([v for v in range(V) if v != blank])
    targets = labels[torch.randint(0, V - 1, (B, S), generator=g)]
    targets[0, 1] = targets[0, 0]                         # a repeated label
    return logits.log_softmax(-1), targets


@pytest.mark.parametrize("blank", [0, 3, 5])              # first column, a middle one, V - 1
def test_lattice_and_grad_equal_torch_float64(blank):
    B, T, V, S = 4, 12, 6, 4
    lp, targets = _torch_case(B, T, V, S, blank, 7 + blank)
    in_len, tgt_len = torch.tensor([12, 9, 5, 7]), torch.tensor([4, 2, 0, 3])                 # mixed lengths, one empty target
    gs = torch.tensor([0.25, -1.5, 3.0, 0.7], dtype=torch.float64)
    leaf = lp.clone().requires_grad_(True)
    ref = torch.nn.functional.ctc_loss(leaf.transpose(0, 1), targets, in_len, tgt_len, blank=blank, reduction="none")
    (g_ref,) = torch.autograd.grad((ref * gs).sum(), leaf)
    for b in range(B):
        Tb, Sb = int(in_len[b]), int(tgt_len[b])
        _, nll, occ = ctc_lattice(lp[b], targets[b], Tb, Sb, blank)
        assert abs(nll - ref[b].item()) <= 1e-10, (b, nll, ref[b].item())
        G = ctc_grad(lp[b], targets[b], Tb, Sb, blank, occ, nll, float(gs[b]))
        assert float(np.abs(G - g_ref[b].numpy()).max()) <= 1e-10, b
        assert float(np.abs(G[Tb:]).sum()) == 0.0


def test_lattice_and_grad_equal_torch_float64_with_a_column_of_minus_infinity():
    """A masked vocabulary column: the utterance without it in its target keeps a finite loss, the one with it has no alignment
    (loss 0 and gradient 0 under zero_infinity=True)."""
    B, T, V, S, blank, col = 2, 10, 6, 3, 2, 4
    lp, targets = _torch_case(B, T, V, S, blank, 31, minus_inf_column=col)
    targets[0] = torch.tensor([1, 1, 5])
    targets[1] = torch.tensor([3, col, 0])
    in_len, tgt_len = torch.tensor([10, 8]), torch.tensor([3, 3])
    leaf = lp.clone().requires_grad_(True)
    ref = torch.nn.functional.ctc_loss(leaf.transpose(0, 1), targets, in_len, tgt_len, blank=blank, reduction="none", zero_infinity=True)
    (g_ref,) = torch.autograd.grad(ref.sum(), leaf)
    _, nll0, occ0 = ctc_lattice(lp[0], targets[0], 10, 3, blank)
    _, nll1, occ1 = ctc_lattice(lp[1], targets[1], 8, 3, blank)
    assert math.isfinite(nll0) and abs(nll0 - ref[0].item()) <= 1e-10
    assert nll1 == math.inf and ref[1].item() == 0.0
    G0 = ctc_grad(lp[0], targets[0], 10, 3, blank, occ0, nll0, 1.0)
    G1 = ctc_grad(lp[1], targets[1], 8, 3, blank, occ1, nll1, 1.0)
    # torch's own backward is NaN in the masked column of the aligned utterance (exp(-inf) - exp(-inf - -inf)); the convention
    # of csrc/ctc.hip gives exp(-inf) - 0 = 0 there.  Every other column agrees.
    keep = [v for v in range(V) if v != col]
    assert bool(g_ref[0, :, col].isnan().all())
    assert not np.isnan(G0).any() and float(np.abs(G0[:, keep] - g_ref[0].numpy()[:, keep]).max()) <= 1e-10
    assert float(np.abs(G0[:, col]).sum()) == 0.0
    assert float(np.abs(G1).sum()) == 0.0 and float(g_ref[1].abs().sum()) == 0.0


def test_lattice_in_float32_stays_close_to_float64():
    """The float32 evaluation that the GPU tests take their floors from is the same recursion, not another one."""
    lp, targets = _torch_case(1, 40, 6, 9, 0, 5)
    a64, n64, o64 = ctc_lattice(lp[0].float(), targets[0], 40, 9, 0)
    a32, n32, o32 = ctc_lattice(lp[0].float(), targets[0], 40, 9, 0, dtype=np.float32)
    assert a32.dtype == np.float32 and o32.dtype == np.float32
    assert np.array_equal(np.isneginf(a32), np.isneginf(a64)) and np.array_equal(np.isneginf(o32), np.isneginf(o64))
    fin = np.isfinite(o64)
    assert 0.0 < float(np.abs(o32[fin] - o64[fin]).max()) <= 1e-3 and abs(n32 - n64) <= 1e-4
    G64 = ctc_grad(lp[0].float(), targets[0], 40, 9, 0, o64, n64, -1.5)
    G32 = ctc_grad(lp[0].float(), targets[0], 40, 9, 0, o64, n64, -1.5, dtype=np.float32)
    assert G32.dtype == np.float32 and float(np.abs(G32 - G64).max()) <= 1e-5


def test_absolute_lengths_round_the_fp32_product():
    tl, sl = abs_lengths(25, 25, torch.tensor([0.1, 1.0, 0.0, 1.2]), torch.tensor([0.1, 0.5, 1.0, -0.2]))
    assert tl.tolist() == [2, 25, 0, 25]                  # 0.1f * 25 == 2.5f exactly: round-half-even -> 2; clamped to [0, T]
    assert sl.tolist() == [2, 12, 25, 0]
    assert round(float(torch.tensor(0.1).double()) * 25) == 3                                 # the fp64 product of the same fp32 0.1


def test_log_softmax_backward_formula_equals_autograd():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(5, 63, generator=g, dtype=torch.float64) * 2.0).requires_grad_(True)
    dy = torch.randn(5, 63, generator=g, dtype=torch.float64)
    y = torch.log_softmax(x, -1)
    (dx,) = torch.autograd.grad((y * dy).sum(), x)
    assert float(np.abs(log_softmax_bwd_ref(dy, y) - dx.numpy()).max()) <= 1e-13

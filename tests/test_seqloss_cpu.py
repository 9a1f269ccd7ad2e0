"""CPU checks around the label-smoothed sequence losses: the float64 reference of tests/_seqloss_ref.py against independent statements
(torch's cross_entropy(label_smoothing=e), a closed-form double loop for the KL row), its analytic gradients against autograd, the
truncate rule, the reduction table with upstream's quirks, the mask count at fractional lengths, and what
summarymixing_amd.nnet.losses refuses before it looks for a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _seqloss_ref as R


def _lp(B, U, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, U, V, generator=g, dtype=torch.float64).log_softmax(-1), torch.randint(0, V, (B, U), generator=g)


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.35])
def test_nll_reference_is_cross_entropy_with_label_smoothing_under_the_mask(eps):
    B, U, V = 3, 5, 17
    g = torch.Generator().manual_seed(1)
    z = torch.randn(B, U, V, generator=g, dtype=torch.float64)
    tg = torch.randint(0, V, (B, U), generator=g)
    length = R.rel_lengths(B)
    mask = R.length_mask(length, B, U)
    assert mask.sum(1).tolist() == [5, 3, 0]
    ce = F.cross_entropy(z.reshape(-1, V), tg.reshape(-1), label_smoothing=eps, reduction="none").view(B, U)
    rows = R.row_losses("nll", z.log_softmax(-1), tg, length, eps)
    assert torch.allclose(rows[mask], ce[mask], rtol=1e-12, atol=1e-12) and float(rows[~mask].abs().sum()) == 0.0
    got = R.nll_loss(z.log_softmax(-1), tg, length, label_smoothing=eps, reduction="mean")
    assert math.isclose(float(got), float(ce[mask].sum() / mask.sum()), rel_tol=1e-12)


def test_kldiv_reference_is_the_closed_form_double_loop():
    B, U, V, eps, pad = 2, 4, 7, 0.1, 3
    lp, tg = _lp(B, U, V, 2)
    tg[0, 1] = pad
    tg[1, :] = pad
    rows = R.row_losses("kldiv", lp, tg, None, eps, pad)
    for b in range(B):
        for u in range(U):
            y = int(tg[b, u])
            want = 0.0
            if y != pad:
                for v in range(V):
                    q = 1 - eps if v == y else eps / (V - 1)
                    want += q * (math.log(q) - float(lp[b, u, v]))
            assert math.isclose(float(rows[b, u]), want, rel_tol=1e-12, abs_tol=1e-15), (b, u)
    assert float(rows[1].abs().sum()) == 0.0
    assert math.isclose(float(R.kldiv_loss(lp, tg, None, eps, pad_idx=pad, reduction="batchmean")), float(rows.sum()) / B, rel_tol=1e-12)


@pytest.mark.parametrize("kind,eps", [("nll", 0.0), ("nll", 0.1), ("kldiv", 0.1)])
def test_analytic_gradients_are_autograd_of_the_reference(kind, eps):
    B, U, V, pad = 3, 5, 11, 1
    g = torch.Generator().manual_seed(3)
    z = torch.randn(B, U, V, generator=g, dtype=torch.float64, requires_grad=True)
    tg = torch.randint(0, V, (B, U), generator=g)
    tg[2, :] = pad
    length = R.rel_lengths(B)
    w = torch.randn(B, U, generator=g, dtype=torch.float64)
    keep = R.keep_mask(kind, tg, length, pad)
    lp = z.log_softmax(-1)
    lp.retain_grad()
    (R.row_losses(kind, lp, tg, length, eps, pad) * w).sum().backward()
    assert torch.allclose(lp.grad, R.grad_log_probs(kind, tg, V, keep, w, eps), rtol=1e-12, atol=1e-14)
    assert torch.allclose(z.grad, R.grad_logits(kind, z.detach(), tg, keep, w, eps), rtol=1e-10, atol=1e-13)
    assert float(z.grad[~keep].abs().sum()) == 0.0


def test_truncate_rule():
    from summarymixing_amd.nnet import losses
    lp, tg = _lp(2, 7, 5, 4)
    for fn in (R.truncate, losses.truncate):
        a, b = fn(lp, tg[:, :5])
        assert a.shape == (2, 5, 5) and b.shape == (2, 5) and a.data_ptr() == lp.data_ptr() and a.stride() == lp.stride()   # a view
        a, b = fn(lp[:, :4], tg)
        assert a.shape == (2, 4, 5) and b.shape == (2, 4) and torch.equal(b, tg[:, :4])
        a, b = fn(lp, tg)
        assert a is lp and b is tg
        with pytest.raises(ValueError):
            fn(lp, tg[:, :3])
        a, b = fn(lp, tg[:, :3], allowed_len_diff=4)
        assert a.shape[1] == 3


def test_reduction_table_with_upstreams_quirks():
    B, U, V, eps, pad = 3, 5, 9, 0.1, 1
    lp, tg = _lp(B, U, V, 5)
    tg[0, 2] = pad
    length = R.rel_lengths(B)
    # nll: mean = sum / kept steps, batchmean = sum / B, batch = per utterance over its kept steps (0 / 0 for an empty one), else (B, U)
    rows = R.row_losses("nll", lp, tg, length, eps)
    kept = R.length_mask(length, B, U).sum(1)
    assert math.isclose(float(R.nll_loss(lp, tg, length, eps, reduction="mean")), float(rows.sum() / kept.sum()), rel_tol=1e-12)
    assert math.isclose(float(R.nll_loss(lp, tg, length, eps, reduction="batchmean")), float(rows.sum() / B), rel_tol=1e-12)
    per = R.nll_loss(lp, tg, length, eps, reduction="batch")
    assert per.shape == (B,) and torch.allclose(per[:2], rows.sum(1)[:2] / kept[:2], rtol=1e-12) and bool(torch.isnan(per[2]))
    assert torch.allclose(R.nll_loss(lp, tg, length, eps, reduction="none"), rows, rtol=1e-12, atol=1e-15)
    # kldiv: 'mean' is loss.sum().mean() = the SUM; batchmean = sum / B; batch = utterance sums / the RELATIVE length; length is ignored otherwise
    krows = R.row_losses("kldiv", lp, tg, None, eps, pad)
    S = float(krows.sum())
    assert math.isclose(float(R.kldiv_loss(lp, tg, length, eps, pad_idx=pad, reduction="mean")), S, rel_tol=1e-12)
    assert math.isclose(float(R.kldiv_loss(lp, tg, None, eps, pad_idx=pad, reduction="sum")), S, rel_tol=1e-12)
    assert math.isclose(float(R.kldiv_loss(lp, tg, length, eps, pad_idx=pad, reduction="batchmean")), S / B, rel_tol=1e-12)
    ln = torch.tensor([1.0, 0.5, 0.25])
    assert torch.allclose(R.kldiv_loss(lp, tg, ln, eps, pad_idx=pad, reduction="batch"), krows.sum(1) / ln.double(), rtol=1e-12)
    assert R.kldiv_loss(lp, tg, None, eps, pad_idx=pad, reduction="none").shape == (B * U, V)
    # smoothing 0: kldiv IS nll (pad_idx unused, length used)
    assert torch.equal(R.kldiv_loss(lp, tg, length, 0.0, pad_idx=pad, reduction="batch")[:2], R.nll_loss(lp, tg, length, reduction="batch")[:2])


def test_mask_count_at_fractional_lengths():
    from summarymixing_amd.nnet import losses
    length = torch.tensor([1.0, 0.5, 0.0, 0.4, 0.41, 0.2])
    U = 5                                                 # length * U = 5, 2.5, 0, 2, 2.05, 1: keeps 5, 3, 0, 2, 3, 1
    got = losses.mask_count(length, U)
    assert got.dtype == torch.int32 and got.tolist() == [5, 3, 0, 2, 3, 1]
    assert got.tolist() == R.length_mask(length, len(length), U).sum(1).tolist()
    for U in (1, 7, 48, 80):
        ln = torch.rand(64, generator=torch.Generator().manual_seed(U))
        assert losses.mask_count(ln, U).tolist() == R.length_mask(ln, 64, U).sum(1).tolist()


def test_smoothing_terms_are_the_two_distributions():
    from summarymixing_amd.nnet import losses
    V, eps = 13, 0.1
    tg = torch.tensor([[4]])
    for kind in ("nll", "kldiv"):
        conf, off, cst = losses.smoothing_terms(kind, eps, V)
        q = R.target_distribution(kind, tg, V, eps)[0, 0]
        assert math.isclose(conf, float(q[4]), rel_tol=1e-14) and math.isclose(off, float(q[0]), rel_tol=1e-14)
        assert math.isclose(float(q.sum()), 1.0, rel_tol=1e-14)
        assert math.isclose(cst, float((q * q.log()).sum()) if kind == "kldiv" else 0.0, rel_tol=1e-13, abs_tol=0.0)
    assert losses.smoothing_terms("nll", 0.0, V) == (1.0, 0.0, 0.0)


def test_refusals_come_before_the_gpu_check():
    from summarymixing_amd.nnet import losses
    from summarymixing_amd.utils.Accuracy import Accuracy, AccuracyStats
    lp, tg = _lp(2, 6, 5, 6)
    lp = lp.float()
    with pytest.raises(NotImplementedError, match="weight"):
        losses.nll_loss(lp, tg, weight=torch.ones(5))
    with pytest.raises(NotImplementedError, match="reduction"):
        losses.kldiv_loss(lp, tg, label_smoothing=0.1, reduction="none")
    with pytest.raises(NotImplementedError, match="reduction"):
        losses.seq_loss_from_logits(lp, tg, label_smoothing=0.1, kind="kldiv", reduction="none")
    with pytest.raises(ValueError, match="V >= 2"):
        losses.kldiv_loss(lp[:, :, :1], tg * 0, label_smoothing=0.1)
    with pytest.raises(ValueError, match="allowed_len_diff"):
        losses.nll_loss(lp, tg[:, :2])
    with pytest.raises(ValueError, match="batch"):
        losses.seq_loss_from_logits(lp, tg, label_smoothing=0.1, kind="kldiv", reduction="batch")
    with pytest.raises(ValueError, match="kind"):
        losses.seq_loss_from_logits(lp, tg, kind="ce")
    with pytest.raises(TypeError):
        losses.nll_loss(lp.double(), tg)
    # a valid call on CPU tensors: no fallback
    for call in (lambda: losses.nll_loss(lp, tg, label_smoothing=0.1), lambda: losses.kldiv_loss(lp, tg, label_smoothing=0.1),
                 lambda: losses.kldiv_loss(lp, tg), lambda: losses.seq_loss_from_logits(lp, tg, kind="kldiv", label_smoothing=0.1),
                 lambda: Accuracy(lp, tg), lambda: AccuracyStats().append(lp, tg, torch.ones(2))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_library_refuses_bad_arguments_on_the_host():
    """SMX_EINVAL / SMX_EUNSUPPORTED before any launch: the pointers are fake and never dereferenced."""
    from summarymixing_amd import _lib
    L = _lib.lib()
    P = 1 << 40
    fwd = dict(dtype=_lib.F32, from_logits=1, X=P, ldx=1000, bsx=5000, targets=P + 0x100000, ldt=5, len=None, B=3, U=5, V=1000, pad_idx=-1,
               conf=0.9, off=1e-4, cst=0.0, row_loss=P + 0x200000, lse=P + 0x300000, row_flags=P + 0x400000, utt_loss=P + 0x500000,
               utt_kept=P + 0x600000, utt_hits=None, stream=None)
    bwd = dict(dtype=_lib.BF16, from_logits=1, X=P, ldx=1000, bsx=5000, targets=P + 0x100000, ldt=5, len=None, B=3, U=5, V=1000, pad_idx=0,
               conf=0.9, off=1e-4, lse=P + 0x300000, g=P + 0x700000, dX=P + 0x800000, lddx=1000, stream=None)
    cases = [(L.smx_seqloss_fwd, fwd, dict(X=None), -1), (L.smx_seqloss_fwd, fwd, dict(lse=None), -1), (L.smx_seqloss_fwd, fwd, dict(V=0), -1),
             (L.smx_seqloss_fwd, fwd, dict(ldx=999), -1), (L.smx_seqloss_fwd, fwd, dict(ldt=4), -1), (L.smx_seqloss_fwd, fwd, dict(dtype=7), -1),
             (L.smx_seqloss_fwd, fwd, dict(off=float("nan")), -1), (L.smx_seqloss_fwd, fwd, dict(off=-0.1), -1),
             (L.smx_seqloss_fwd, fwd, dict(pad_idx=1000), -2), (L.smx_seqloss_fwd, fwd, dict(B=1 << 16, U=1 << 15, ldt=1 << 15), -2),
             (L.smx_seqloss_bwd, bwd, dict(g=None), -1), (L.smx_seqloss_bwd, bwd, dict(X=None), -1), (L.smx_seqloss_bwd, bwd, dict(lddx=999), -1),
             (L.smx_seqloss_bwd, bwd, dict(dX=P), -2), (L.smx_seqloss_bwd, bwd, dict(pad_idx=1000), -2)]
    for fn, base, change, code in cases:
        assert fn(*{**base, **change}.values()) == code, (fn.__name__, change)
    # the log-probability form needs neither X nor lse in the backward; empty batches are not an error
    assert L.smx_seqloss_bwd(*{**bwd, "from_logits": 0, "X": None, "lse": None, "B": 0}.values()) == 0

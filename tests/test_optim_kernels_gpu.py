"""smx_sgd_step, smx_adamw_step_lr and smx_lr_schedule against float64 restatements (tests/_optim_ref.py).

SGD: three consecutive updates of a range that sits inside poisoned buffers, 0 / 1 / 2 elements past a 16-byte boundary, at
sizes around the float4 body, the block and one full sweep of the capped grid.  Bar per tensor (the package's usual one):
max|err| against float64 at most 4x the max|err| of torch.optim.SGD(foreach=False) in fp32 on the same inputs, with a floor of
2^-23 * max|tensor| (one fused-versus-unfused rounding where ATen happens to be exact)."""
import numpy as np
import pytest
import torch

from tests import _optim_ref as R

pytestmark = pytest.mark.gpu

LR = 1e-2
GUARD = 8                                   # poisoned words in front of and behind every range
P_POISON, B_POISON, S_POISON = 1234.5, -4321.25, 777.0


def _sizes():
    from summarymixing_amd import ops
    return [1, 3, 4, 5, 63, 64, 257, 4097, ops.SGD_GRID_SWEEP + 7]


def _inputs(n, off, seed):
    """p ~ N(0,1), three gradients ~ 0.1 N(0,1); every tensor a view [GUARD + off, GUARD + off + n) of a poisoned buffer whose
    base is 16-byte aligned (the caching allocator's blocks are 512-byte aligned)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo = GUARD + off
    size = lo + n + GUARD
    P = torch.full((size,), P_POISON, device="cuda")
    B = torch.full((size,), B_POISON, device="cuda")
    S = torch.full((size,), S_POISON, device="cuda", dtype=torch.bfloat16)
    G = [torch.full((size,), 55.0, device="cuda") for _ in range(3)]
    assert P.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0 and S.data_ptr() % 16 == 0 and all(x.data_ptr() % 16 == 0 for x in G)
    P[lo:lo + n] = torch.randn(n, device="cuda", generator=g)
    B[lo:lo + n] = 0.0
    for x in G:
        x[lo:lo + n] = 0.1 * torch.randn(n, device="cuda", generator=g)
    return P, B, S, G, lo


def _run_kernel(P, B, S, G, lo, n, mu, nesterov, wd, shadows, gdev, lr_dev):
    from summarymixing_amd import ops
    P, B, S = P.clone(), B.clone(), S.clone()
    p, b, s = P[lo:lo + n], B[lo:lo + n], S[lo:lo + n]
    for k in range(3):
        ops.sgd_step(p, G[k][lo:lo + n], b if mu > 0 else None, s if shadows else None,
                     123.0 if lr_dev is not None else LR, mu, wd, nesterov,
                     0.5 if gdev is not None else 1.0, gdev, lr_dev=lr_dev)
    return P, B, S


def _bar(got, aten, ref64):
    err = (got.double() - ref64).abs().max().item()
    err_aten = (aten.double() - ref64).abs().max().item()
    return err, max(4.0 * err_aten, 2.0 ** -23 * ref64.abs().max().item())


@pytest.mark.parametrize("lr_mode", ["lr_value", "lr_dev"])
@pytest.mark.parametrize("gscale", ["host_scale", "gscale_dev"])
@pytest.mark.parametrize("shadows", [False, True], ids=["no_shadow", "shadow"])
@pytest.mark.parametrize("mu,nesterov,wd", [(0.0, False, 0.0), (0.9, False, 1e-2), (0.99, True, 0.0), (0.99, True, 1e-2)])
def test_sgd_step_matches_float64(mu, nesterov, wd, shadows, gscale, lr_mode):
    lr32, mu32, wd32 = float(np.float32(LR)), float(np.float32(mu)), float(np.float32(wd))    # what the kernel is handed
    lr_dev = torch.tensor([LR], device="cuda") if lr_mode == "lr_dev" else None
    gdev = torch.tensor([0.37], device="cuda") if gscale == "gscale_dev" else None
    gs32 = torch.tensor(0.5) * torch.tensor(0.37) if gdev is not None else torch.tensor(1.0)    # the kernel's fp32 product
    gs = float(gs32)
    for n in _sizes():
        for off in (0, 1, 2):
            P, B, S, G, lo = _inputs(n, off, seed=1000 * off + n % 997)
            P1, B1, S1 = _run_kernel(P, B, S, G, lo, n, mu, nesterov, wd, shadows, gdev, lr_dev)
            P2, B2, S2 = _run_kernel(P, B, S, G, lo, n, mu, nesterov, wd, shadows, gdev, lr_dev)
            tag = (n, off)
            assert torch.equal(P1, P2) and torch.equal(B1, B2) and torch.equal(S1.view(torch.int16), S2.view(torch.int16)), tag
            # the words around [lo, lo + n) are untouched, and so are a buffer / shadows that were not passed
            for new, old in ((P1, P), (B1, B), (S1, S)):
                assert torch.equal(new[:lo].view(torch.uint8), old[:lo].view(torch.uint8)), tag
                assert torch.equal(new[lo + n:].view(torch.uint8), old[lo + n:].view(torch.uint8)), tag
            if mu == 0:
                assert torch.equal(B1, B), tag
            if shadows:
                assert torch.equal(S1[lo:lo + n].view(torch.int16), P1[lo:lo + n].to(torch.bfloat16).view(torch.int16)), tag
            else:
                assert torch.equal(S1.view(torch.int16), S.view(torch.int16)), tag
            # float64 and ATen (fp32, foreach=False) on the same inputs
            p64, b64 = P[lo:lo + n].double(), torch.zeros(n, dtype=torch.float64, device="cuda")
            pa = P[lo:lo + n].clone().requires_grad_(True)
            sgd = torch.optim.SGD([pa], lr=LR, momentum=mu, nesterov=nesterov, weight_decay=wd, foreach=False)
            for k in range(3):
                gk = G[k][lo:lo + n]
                R.sgd_step(p64, gk.double(), b64, lr32, mu32, wd32, nesterov, gs)
                pa.grad = gk * gs
                sgd.step()
            err, bound = _bar(P1[lo:lo + n], pa.detach(), p64)
            print(f"sgd n={n} off={off} p: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (tag, "p", err, bound)
            if mu > 0:
                err, bound = _bar(B1[lo:lo + n], sgd.state[pa]["momentum_buffer"], b64)
                print(f"sgd n={n} off={off} buf: err {err:.3e} bound {bound:.3e}")
                assert err <= bound, (tag, "buf", err, bound)


@pytest.mark.parametrize("n", [5, 4097])
def test_sgd_step_clip_factor_zero_skips_everything(n):
    from summarymixing_amd import ops
    P, B, S, G, lo = _inputs(n, 1, seed=7)
    B[lo:lo + n] = 0.25
    P0, B0, S0 = P.clone(), B.clone(), S.clone()
    clip = torch.zeros(2, device="cuda")                  # smx_clip_factor's verdict on a non-finite norm
    G[0][lo + n // 2] = float("nan")
    ops.sgd_step(P[lo:lo + n], G[0][lo:lo + n], B[lo:lo + n], S[lo:lo + n], LR, 0.99, 1e-2, True, 1.0, clip)
    assert torch.equal(P, P0) and torch.equal(B, B0) and torch.equal(S.view(torch.int16), S0.view(torch.int16))


def test_sgd_step_unaligned_relative_offsets_run_scalar():
    """Buffers at different offsets from a 16-byte boundary (no common float4 grid) take the scalar path: same results."""
    from summarymixing_amd import ops
    n = 1029
    P, B, S, G, lo = _inputs(n, 0, seed=11)
    want = _run_kernel(P, B, S, G, lo, n, 0.9, False, 1e-2, True, None, None)
    g_shift = [torch.cat([x.new_zeros(1), x]) for x in G]          # the gradients one element off the others' alignment
    P1, B1, S1 = P.clone(), B.clone(), S.clone()
    for k in range(3):
        ops.sgd_step(P1[lo:lo + n], g_shift[k][lo + 1:lo + 1 + n], B1[lo:lo + n], S1[lo:lo + n], LR, 0.9, 1e-2, False)
    assert torch.equal(P1, want[0]) and torch.equal(B1, want[1]) and torch.equal(S1.view(torch.int16), want[2].view(torch.int16))


def test_adamw_step_lr_equals_adamw_step_bit_for_bit():
    from summarymixing_amd import ops
    n, lr = 4097, 8e-4
    g = torch.Generator(device="cuda").manual_seed(3)
    p = torch.randn(n, device="cuda", generator=g)
    grad = 0.1 * torch.randn(n, device="cuda", generator=g)
    m = 0.05 * torch.randn(n, device="cuda", generator=g)
    v = (0.01 * torch.randn(n, device="cuda", generator=g)) ** 2
    outs = []
    for lr_dev in (None, torch.tensor([lr], device="cuda")):
        pp, mm, vv, sh = p.clone(), m.clone(), v.clone(), torch.zeros(n, device="cuda", dtype=torch.bfloat16)
        ops.adamw_step(pp, grad, mm, vv, sh, lr if lr_dev is None else 99.0, 0.9, 0.98, 1e-8, 0.01, 3, 0.5, None, lr_dev=lr_dev)
        outs.append((pp, mm, vv, sh.view(torch.int16)))
    assert not torch.equal(outs[0][0], p)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _ulp_close(got, want64):
    want = np.float32(want64)
    return abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(np.abs(want)))


_SCHEDULES = [
    ("noam", dict(lr_initial=1e-3)),
    ("noam_model_size", dict(lr_initial=1.0, model_size=256)),
    ("warm_exp", dict(base=1e-3, total_steps=1000, decay_factor=0.1)),
    ("warm_exp_long", dict(base=2e-3, total_steps=300000, decay_factor=0.5)),
]


@pytest.mark.parametrize("warmup", [1, 3, 25000])
@pytest.mark.parametrize("name,kw", _SCHEDULES, ids=[s[0] for s in _SCHEDULES])
def test_lr_schedule_matches_float64_definition(name, kw, warmup):
    from summarymixing_amd import _lib as L
    from summarymixing_amd import ops
    lr0 = 5e-4
    if name.startswith("noam"):
        kind, consts = L.LR_NOAM, (kw["lr_initial"], warmup, kw.get("model_size", 0.0), 0.0)
        ref = lambda t: R.noam_lr(t, lr0, kw["lr_initial"], warmup, kw.get("model_size"))
    else:
        kind, consts = L.LR_WARM_EXP_DECAY, (kw["base"], warmup, kw["total_steps"], kw["decay_factor"])
        ref = lambda t: R.warm_exp_decay_lr(t, lr0, kw["base"], warmup, kw["total_steps"], kw["decay_factor"])
    out = torch.full((1,), -1.0, device="cuda")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.set_step_counter(counter)
    try:
        for t in sorted({1, 2, 3, warmup, warmup + 1, warmup + 2, 10 ** 6, 2 ** 31 + 5}):
            want = ref(t)
            ops.lr_schedule(kind, consts, lr0, t, out)                       # t by value (the counter holds something else)
            by_value = out.item()
            counter.fill_(t)
            out.fill_(-1.0)
            ops.lr_schedule(kind, consts, lr0, 0, out)                       # t from the device counter
            by_counter = out.item()
            counter.zero_()
            print(f"{name} warmup={warmup} t={t}: want {want:.9e} value {by_value:.9e} counter {by_counter:.9e}")
            assert _ulp_close(by_value, want), (t, by_value, want)
            assert _ulp_close(by_counter, want), (t, by_counter, want)
    finally:
        ops.set_step_counter(None)
    if name == "warm_exp":
        assert ref(2) == 0.0                                                 # update 2 runs at rate 0, as upstream's does

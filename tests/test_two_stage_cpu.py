"""CPU-side checks of the two-stage training surface: the schedulers' host form, FlatSGD's refusals, FlatSGD.adopt's hand-over,
and FlatSGD under world-size-2 gloo in both gradient exchange modes with CPU restatements of the _k_* hooks (the style and the
tolerances of tests/test_trainer_dist.py)."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_trainer_dist import _free_port, _model, _oracle_grads_into


class _CpuKernels:
    """CPU restatements of the device primitives behind FlatOptimizer._apply_update and of smx_sgd_step."""

    def _k_cast(self, src, dst):
        dst.copy_(src)

    def _k_sumsq(self, g):
        self._sumsq += (g.double() ** 2).sum().float()

    def _k_clip(self, gscale):
        nrm = float(self._sumsq.sqrt()) * gscale
        self._clip[0] = min(1.0, self.max_grad_norm / (nrm + 1e-6))

    def _k_sgd(self, a, b, g, gscale, clip):
        p = self.flat_p[a:b]
        g = g * gscale * (float(clip[0]) if clip is not None else 1.0) + self.wd * p
        if self.momentum > 0:
            buf = self.momentum_buffer[a:b]
            buf.mul_(self.momentum).add_(g)
            g = g + self.momentum * buf if self.nesterov else buf
        p.sub_(g, alpha=self.lr)

    def _k_adamw(self, a, b, g, gscale, clip):
        g = g * gscale * (float(clip[0]) if clip is not None else 1.0)
        b1, b2 = self.betas
        p, m, v = self.flat_p[a:b], self.exp_avg[a:b], self.exp_avg_sq[a:b]
        p.mul_(1 - self.lr * self.wd)
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = 1 - b1 ** self.step_count, 1 - b2 ** self.step_count
        p.addcdiv_(m, v.sqrt() / bc2 ** 0.5 + self.eps, value=-self.lr / bc1)


def _cpu_sgd(enc, **kw):
    from summarymixing_amd.trainer import FlatSGD

    class Opt(_CpuKernels, FlatSGD):
        pass
    kw = dict(dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-3, max_grad_norm=0.5, compute_dtype=torch.float32), **kw)
    return Opt(enc, **kw)


def _cpu_adamw(enc, **kw):
    from summarymixing_amd.trainer import FlatAdamW

    class Opt(_CpuKernels, FlatAdamW):
        pass
    return Opt(enc, compute_dtype=torch.float32, **kw)


# ---- schedulers, host form ------------------------------------------------------------------------------------------------
def _noam_expected():        # NoamScheduler(1e-3, 4): after call k the rate is 1e-3 * 4^0.5 * min(k^-0.5, k * 4^-1.5)
    return [1e-3 * 2.0 * min(k ** -0.5, k / 8.0) for k in range(1, 11)]


def _warm_exp_expected():    # WarmAndExpDecayLRSchedule(1e-3, 3, 5, 0.1): after call k, c = k - 1
    return [1e-3 * c / 3.0 if c < 3 else min(1e-3, 1e-3 * 0.1 ** ((c - 3) / 5.0)) for c in range(10)]


def test_noam_host_calls_set_torch_and_flat_optimizers():
    from summarymixing_amd.nnet.schedulers import NoamScheduler
    want = _noam_expected()
    assert want[0] == pytest.approx(2.5e-4) and want[3] == pytest.approx(1e-3) and want[8] == pytest.approx(2e-3 / 3)
    assert max(want) == want[3]                                  # the peak sits at the end of the warm-up
    w = torch.nn.Parameter(torch.zeros(3))
    sgd = torch.optim.SGD([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "lr": 7.0}], lr=0.5)
    flat = _cpu_adamw(_model(layers=1), lr=0.5)
    for opt, read in ((sgd, lambda: [g["lr"] for g in sgd.param_groups]), (flat, lambda: [flat.lr])):
        sched, prev = NoamScheduler(lr_initial=1e-3, n_warmup_steps=4), 0.5
        for k in range(10):
            old, new = sched(opt)
            assert old == prev and new == pytest.approx(want[k], rel=1e-15)
            assert all(x == new for x in read())
            assert new == sched.lr_for_update(k + 2)
            prev = new
        assert sched.n_steps == 10
        again = NoamScheduler(lr_initial=1e-3, n_warmup_steps=4)
        again.load_state_dict(sched.state_dict())
        assert again.n_steps == 10 and again(opt)[1] == sched(opt)[1] == sched.lr_for_update(12)
    assert NoamScheduler(1.0, 25000, model_size=256).lr_for_update(2) == pytest.approx(256 ** -0.5 * 25000 ** -1.5, rel=1e-15)
    assert sched.lr_for_update(1, lr0=0.125) == 0.125
    with pytest.raises(ValueError, match="lr0"):
        sched.lr_for_update(1)


def test_warm_and_exp_decay_host_calls_set_torch_and_flat_optimizers():
    from summarymixing_amd.nnet.schedulers import WarmAndExpDecayLRSchedule
    want = _warm_exp_expected()
    assert want[0] == 0.0 and want[3] == 1e-3 and want[8] == pytest.approx(1e-4)     # update 2 at rate 0; a decade per total_steps
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.5)
    flat = _cpu_sgd(_model(layers=1), lr=0.5)
    for opt, read in ((sgd, lambda: sgd.param_groups[0]["lr"]), (flat, lambda: flat.lr)):
        sched = WarmAndExpDecayLRSchedule(1e-3, 3, 5)
        for k in range(10):
            sched(opt)
            assert read() == pytest.approx(want[k], rel=1e-15) and read() == sched.lr_for_update(k + 2)
        assert sched.state_dict() == {"n_steps": 10}


def test_scheduler_attached_to_a_flat_optimizer_only_counts():
    """On the optimizer it is attached to, the call changes nothing on the optimizer and returns the host-computed pair."""
    from summarymixing_amd.nnet.schedulers import NoamScheduler
    flat = _cpu_sgd(_model(layers=1), lr=0.5)
    sched = NoamScheduler(1e-3, 4)
    flat.set_lr_schedule(sched)
    want = _noam_expected()
    assert sched(flat) == (0.5, want[0]) and sched(flat) == (want[0], want[1])
    assert flat.lr == 0.5 and sched.n_steps == 2


# ---- FlatSGD refusals and the hand-over ---------------------------------------------------------------------------------------
def test_flat_sgd_refuses_by_name():
    enc = _model(layers=1)
    with pytest.raises(ValueError, match="dampening"):
        _cpu_sgd(enc, dampening=0.1)
    with pytest.raises(ValueError, match="nesterov"):
        _cpu_sgd(enc, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="maximize"):
        _cpu_sgd(enc, maximize=True)
    with pytest.raises(TypeError, match="foreach"):
        _cpu_sgd(enc, foreach=True)
    with pytest.raises(ValueError, match="reduce"):
        _cpu_sgd(enc, reduce="ring")
    from summarymixing_amd.trainer import FlatSGD
    with pytest.raises(ValueError, match="dampening"):
        FlatSGD.adopt(_cpu_adamw(_model(layers=1)), lr=1e-2, momentum=0.9, dampening=0.5)
    plain = _cpu_sgd(_model(layers=1), momentum=0.0, nesterov=False)
    assert plain.momentum_buffer is None and plain.state_dict()["momentum_buffer"] is None


def test_adopt_hands_the_buffers_over_and_retires_the_old_optimizer():
    from summarymixing_amd.trainer import FlatSGD

    class Sgd(_CpuKernels, FlatSGD):
        pass
    enc = _model(layers=1)
    old = _cpu_adamw(enc, lr=1e-2)
    for p in enc.parameters():
        p.grad.fill_(0.01)
    old.step()
    ptrs = (old.flat_p.data_ptr(), old.flat_g.data_ptr())
    new = Sgd.adopt(old, lr=1e-2, momentum=0.99, nesterov=True)
    assert isinstance(new, Sgd) and (new.flat_p.data_ptr(), new.flat_g.data_ptr()) == ptrs
    assert all(p.data_ptr() == ptrs[0] + 4 * o and p.grad.data_ptr() == ptrs[1] + 4 * o for p, o in zip(new.params, new.offs))
    assert new.step_count == 1 and new.max_grad_norm == old.max_grad_norm and new.buckets == old.buckets
    assert not hasattr(new, "exp_avg") and old.exp_avg is None and old.flat_p is None
    assert new.momentum_buffer.shape == new.flat_p.shape and not new.momentum_buffer.any()
    with pytest.raises(RuntimeError, match="adopt"):
        old.step()
    before = new.flat_p.clone()
    new.step()
    assert new.step_count == 2 and not torch.equal(new.flat_p, before) and new.momentum_buffer.any()
    sd = new.state_dict()
    assert set(sd) >= {"momentum_buffer", "step", "skipped_steps", "total", "complete"} and "exp_avg" not in sd
    with pytest.raises(ValueError, match="momentum_buffer"):
        new.load_state_dict({"total": new.total, "step": 1, "exp_avg": before})


# ---- world size 2 over gloo -------------------------------------------------------------------------------------------------
def _batch():
    g = torch.Generator().manual_seed(5)
    X = torch.randn(4, 9, 16, generator=g)
    R = torch.randn(4, 9, 16, generator=g)
    lens = torch.tensor([9, 5, 7, 9])
    return X, R, torch.arange(9)[None] < lens[:, None]


def _worker(rank, world, port, out, reduce, phase):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        enc = _model()
        opt = _cpu_sgd(enc, reduce=reduce)
        ranges = [opt.param_range(list(l.parameters())) for l in enc.layers]
        X, R, pad = _batch()
        sl = slice(rank * 2, rank * 2 + 2)

        def one_step():
            opt.zero_grad()
            _oracle_grads_into(enc, X[sl], pad[sl], R[sl])
            for a, b in reversed(ranges):
                opt.reduce_bucket_async(a, b)
            opt.reduce_bucket_async(ranges[-1][1], opt.total)
            opt.step()

        if phase in ("two", "straight"):
            for _ in range(2 if phase == "two" else 3):
                one_step()
        elif phase in ("save", "save_local"):
            for _ in range(2):
                one_step()
            sd = opt.state_dict(gather=phase == "save")          # (gather=True is a collective: both ranks call it)
            if phase == "save_local":
                assert not sd["complete"] and sd["rank"] == rank and sum(b - a for a, b in sd["owned"]) == opt.total // world
                torch.save({"opt": sd, "model": enc.state_dict()}, out + f".ckpt{rank}")
            elif rank == 0:
                assert sd["complete"] and sd["step"] == 2
                torch.save({"opt": sd, "model": enc.state_dict()}, out + ".ckpt")
        else:
            ck = torch.load(out + (f".ckpt{rank}" if phase == "resume_local" else ".ckpt"))
            if phase == "resume_local":
                with pytest.raises(ValueError, match="only resumes on that rank"):
                    opt.load_state_dict(torch.load(out + f".ckpt{1 - rank}")["opt"])
            enc.load_state_dict(ck["model"])
            opt.load_state_dict(ck["opt"])
            one_step()
        torch.save({"params": opt.flat_p.clone(), "clip": opt._clip.clone(), "momentum_buffer": opt.state_dict()["momentum_buffer"]},
                   out + f".{phase}.{rank}")
    finally:
        dist.destroy_process_group()


def _single_process(steps=2):
    enc = _model()
    opt = _cpu_sgd(enc)
    X, R, pad = _batch()
    for _ in range(steps):
        opt.zero_grad()
        _oracle_grads_into(enc, X, pad, R)
        opt.flat_g.mul_(0.5)                                     # the DP step averages over the 2 ranks
        opt.step()
    return opt


@pytest.mark.timeout(300)
@pytest.mark.parametrize("reduce", ["allreduce", "rs_ag"])
def test_dp2_flat_sgd_matches_single_process(tmp_path, reduce):
    out = str(tmp_path / "r")
    mp.spawn(_worker, args=(2, _free_port(), out, reduce, "two"), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".two.0"), torch.load(out + ".two.1")
    assert torch.equal(r0["params"], r1["params"])               # ranks never drift apart
    assert float(r0["clip"][0]) < 1.0                            # the clip was active
    ref = _single_process()
    if reduce == "allreduce":
        torch.testing.assert_close(r0["params"], ref.flat_p, rtol=1e-4, atol=5e-5)
    base = _cpu_sgd(_model()).flat_p.clone()
    du, dr = r0["params"] - base, ref.flat_p - base
    err = (du - dr).abs().max().item() / dr.abs().max().item()
    assert err <= 1e-3, err
    torch.testing.assert_close(r0["momentum_buffer"], ref.momentum_buffer, rtol=1e-4, atol=5e-5)


@pytest.mark.timeout(600)
def test_dp2_flat_sgd_rs_ag_checkpoint_round_trip(tmp_path):
    """Under reduce='rs_ag' each rank updates its shard of the momentum buffer only: state_dict(gather=True) saves it complete
    from any rank, state_dict(gather=False) per rank; either resumes bit-identically to uninterrupted steps."""
    out = str(tmp_path / "r")
    for phase in ("straight", "save", "resume", "save_local", "resume_local"):
        mp.spawn(_worker, args=(2, _free_port(), out, "rs_ag", phase), nprocs=2, join=True)
    want = torch.load(out + ".straight.0")
    assert want["momentum_buffer"].any()
    for phase in ("resume", "resume_local"):
        got0, got1 = torch.load(out + f".{phase}.0"), torch.load(out + f".{phase}.1")
        assert torch.equal(got0["params"], got1["params"])
        for k in ("params", "momentum_buffer"):
            assert torch.equal(want[k], got0[k]), (phase, k)
    ck = torch.load(out + ".ckpt")["opt"]
    nz, full = (ck["momentum_buffer"] != 0).float().mean().item(), (want["momentum_buffer"] != 0).float().mean().item()
    assert nz > 0.9 * full, (nz, full)                           # complete: no half of any bucket is still zero

"""The recipes' per-step learning-rate schedules (upstream speechbrain.nnet.schedulers: NoamScheduler for the three
transformer recipes, WarmAndExpDecayLRSchedule for the two transducer ones), with upstream's constructor arguments.

Both define the rate of optimizer update t (counted from 1) - ``lr_for_update(t)``, float64 - as what a recipe gets by calling
the scheduler once behind every optimizer step:

  t == 1   the optimizer's own constructor rate (the first call comes after the first update);
  Noam, t >= 2, n = t - 1:                 lr_initial * norm * min(n^-0.5, n * warmup^-1.5),
                                            norm = warmup^0.5, or model_size^-0.5 when model_size is given;
  WarmAndExpDecay, t >= 2, c = t - 2:      lr * c / warmup while c < warmup (update 2 runs at rate 0, as upstream's does),
                                            else min(lr, lr * decay_factor^((c - warmup) / total_steps)).

Two ways to use one:
  host    ``sched(opt)`` behind ``opt.step()``, as in the recipes: advances the count and sets ``opt.lr`` of a flat optimizer
          (summarymixing_amd.trainer) or every ``param_groups[i]["lr"]`` of a torch.optim optimizer;
  device  ``opt.set_lr_schedule(sched)``: every update launches smx_lr_schedule in front of its update kernel, the rate lives in
          ``opt.lr_dev`` and follows the device step counter through a captured step.  ``sched(opt)`` may stay in the loop: on the
          optimizer it is attached to it only advances the count and returns the host-computed values."""
from .. import _lib as L


class _Schedule:
    def __init__(self):
        self.n_steps = 0              # calls so far = optimizer updates already taken

    # -- to be provided: _rate(t) for t >= 2 (float64) and device_args() -> (kind, constants) --------------------------------
    def lr_for_update(self, t, lr0=None):
        """The rate of update t >= 1 in float64.  t == 1 is the optimizer's own rate: pass it as lr0."""
        t = int(t)
        if t < 1:
            raise ValueError(f"{type(self).__name__}.lr_for_update: updates count from 1, got {t}")
        if t == 1:
            if lr0 is None:
                raise ValueError(f"{type(self).__name__}.lr_for_update: update 1 runs at the optimizer's own rate (pass lr0)")
            return float(lr0)
        return self._rate(t)

    def _advance(self, opt):
        """One call behind an optimizer step -> (rate of the update just taken, rate of the next one)."""
        attached = getattr(opt, "_sched", None) is self
        groups = getattr(opt, "param_groups", None)
        if attached:                  # the device evaluates the schedule; opt.lr stays the constructor rate
            old = self.lr_for_update(self.n_steps + 1, opt.lr)
        else:
            old = groups[0]["lr"] if groups is not None else opt.lr
        self.n_steps += 1
        new = self.lr_for_update(self.n_steps + 1)
        if not attached:
            if groups is not None:
                for g in groups:
                    g["lr"] = new
            else:
                opt.lr = new
        return old, new

    def state_dict(self):
        return {"n_steps": self.n_steps}

    def load_state_dict(self, sd):
        self.n_steps = int(sd["n_steps"])


class NoamScheduler(_Schedule):
    """``NoamScheduler(lr_initial, n_warmup_steps, model_size=None)``; ``sched(opt)`` returns (old_lr, new_lr)."""

    def __init__(self, lr_initial, n_warmup_steps, model_size=None):
        super().__init__()
        if n_warmup_steps <= 0:
            raise ValueError("NoamScheduler: n_warmup_steps must be positive")
        self.lr_initial, self.n_warmup_steps, self.model_size = lr_initial, n_warmup_steps, model_size
        self.normalize = n_warmup_steps ** 0.5 if model_size is None else model_size ** -0.5

    def _rate(self, t):
        n = float(t - 1)
        return float(self.lr_initial) * self.normalize * min(n ** -0.5, n * float(self.n_warmup_steps) ** -1.5)

    def device_args(self):
        return L.LR_NOAM, (self.lr_initial, self.n_warmup_steps, self.model_size or 0.0, 0.0)

    def __call__(self, opt):
        return self._advance(opt)


class WarmAndExpDecayLRSchedule(_Schedule):
    """``WarmAndExpDecayLRSchedule(lr, n_warmup_steps, total_steps, decay_factor=0.1)``: linear warm-up to lr, then an
    exponential decay that reaches lr * decay_factor after total_steps more updates."""

    def __init__(self, lr, n_warmup_steps, total_steps, decay_factor=0.1):
        super().__init__()
        if n_warmup_steps <= 0 or total_steps <= 0 or decay_factor <= 0:
            raise ValueError("WarmAndExpDecayLRSchedule: n_warmup_steps, total_steps and decay_factor must be positive")
        self.base_lr, self.n_warmup_steps, self.total_steps, self.decay_factor = lr, n_warmup_steps, total_steps, decay_factor

    def _rate(self, t):
        c, w, base = float(t - 2), float(self.n_warmup_steps), float(self.base_lr)
        if c < w:
            return base * c / w
        return min(base, base * float(self.decay_factor) ** ((c - w) / float(self.total_steps)))

    def device_args(self):
        return L.LR_WARM_EXP_DECAY, (self.base_lr, self.n_warmup_steps, self.total_steps, self.decay_factor)

    def __call__(self, opt):
        self._advance(opt)

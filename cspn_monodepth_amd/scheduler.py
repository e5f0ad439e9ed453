"""The reference's learning-rate schedules — the drop-in for `libs.scheduler`:

    from cspn_monodepth_amd.scheduler import get_schedular, do_schedule     # was: from libs.scheduler import ...

`get_schedular(optimizer, args)` offers what the reference's does (libs/scheduler/__init__.py): `args.scheduler` "poly_lr" ->
PolynomialLR(max_iter, decay_iter, gamma), "reduce_lr" -> ReduceLROnPlateau(mode "min", factor, patience lr_patience);
`do_schedule(args, scheduler, it, len, metrics)` steps the first on every call and the second when `it % len == 0`, with epoch
`it // len`.  PolynomialLR and WarmUpLR keep the reference's formulas and branches (libs/scheduler/scheduler.py):

  * PolynomialLR leaves every group's rate as it is on an iteration that is no multiple of decay_iter, or past max_iter; otherwise
    the rate is base * (1 - it / max_iter) ** gamma;
  * WarmUpLR asks the scheduler it wraps for its rates WITHOUT stepping it, scales them by gamma * (1 - a) + a (a = it /
    warmup_iters; "constant": by gamma) during warm-up and returns them unscaled afterwards.  One difference: an unknown `mode`
    raises ValueError when the scheduler is constructed, where the reference raises KeyError from its first step.

On float rates they compute what the reference computes, double for double (tests/golden/make_golden_g24.py).  On tensor rates
(cspn_monodepth_amd.optim.SGD.lr_to_device) all arithmetic stays on the host, in the same doubles, and a new rate is written with
`fill_` and nothing else: no `.item()`, no synchronisation, nothing that a captured graph's replay would miss.  The float last
written stands in `group["lr_host"]`; the "keep" branch does not touch a tensor rate at all.  Only a rate tensor that nothing of
this package has written yet (no `lr_host`) is read, once, when a scheduler of this module is constructed on it."""
import torch
from torch.optim import lr_scheduler as _torch_sched

__all__ = ["PolynomialLR", "WarmUpLR", "ReduceLROnPlateau", "get_schedular", "do_schedule"]


def _is_tensor_rate(group):
    return isinstance(group["lr"], torch.Tensor)


def _host_rate(group):
    """The group's rate as a float: the float itself, or the mirror of a tensor rate."""
    if not _is_tensor_rate(group):
        return group["lr"]
    if "lr_host" not in group:
        group["lr_host"] = float(group["lr"])          # the one read, at construction (see the module docstring)
    return group["lr_host"]


def _write_rate(group, lr):
    """lr None: keep.  A tensor rate is written in place, a float rate replaced."""
    if lr is None:
        return
    if _is_tensor_rate(group):
        lr = float(lr)
        group["lr"].fill_(lr)
        group["lr_host"] = lr
    else:
        group["lr"] = lr


class _HostScheduler(_torch_sched.LRScheduler):
    """torch's scheduler protocol (state_dict, get_last_lr, last_epoch) with a step() that never reads a device value.
    get_lr() returns one entry per group: the new rate, or None for "keep" on a tensor rate."""

    def __init__(self, optimizer, last_epoch=-1):
        for group in optimizer.param_groups:
            if _is_tensor_rate(group):                   # a float base rate: torch would clone the tensor instead
                group.setdefault("initial_lr", _host_rate(group))
        super().__init__(optimizer, last_epoch)

    def step(self, epoch=None):
        self._step_count += 1
        self.last_epoch = self.last_epoch + 1 if epoch is None else epoch
        for group, lr in zip(self.optimizer.param_groups, self.get_lr()):
            _write_rate(group, lr)
        self._last_lr = [_host_rate(group) for group in self.optimizer.param_groups]


class PolynomialLR(_HostScheduler):
    """base * (1 - it / max_iter) ** gamma on the iterations that are multiples of decay_iter, up to and including max_iter; on
    every other iteration the rate stays what it is (a float rate is handed back, a tensor rate is not touched)."""

    def __init__(self, optimizer, max_iter, decay_iter=1, gamma=0.9, last_epoch=-1):
        self.max_iter, self.decay_iter, self.gamma = max_iter, decay_iter, gamma
        super().__init__(optimizer, last_epoch)

    def _decays_now(self):
        on_grid = self.last_epoch % self.decay_iter == 0
        return on_grid and self.last_epoch <= self.max_iter

    def get_lr(self):
        if self._decays_now():
            scale = (1 - self.last_epoch / float(self.max_iter)) ** self.gamma
            return [base * scale for base in self.base_lrs]
        return [None if _is_tensor_rate(group) else group["lr"] for group in self.optimizer.param_groups]


class WarmUpLR(_HostScheduler):
    """The rates of `scheduler` — asked through its get_lr(), never stepped — scaled during the first warmup_iters iterations:
    "constant" by gamma, "linear" by a ramp from gamma at iteration 0 to 1 at warmup_iters.  Afterwards they pass through."""

    MODES = ("linear", "constant")

    def __init__(self, optimizer, scheduler, mode="linear", warmup_iters=100, gamma=0.2, last_epoch=-1):
        if mode not in self.MODES:
            raise ValueError("WarmUpLR: mode %r is not one of %s" % (mode, ", ".join(self.MODES)))
        self.scheduler, self.mode, self.warmup_iters, self.gamma = scheduler, mode, warmup_iters, gamma
        super().__init__(optimizer, last_epoch)

    def _scale(self):
        if self.mode == "constant":
            return self.gamma
        done = self.last_epoch / float(self.warmup_iters)
        return self.gamma * (1 - done) + done

    def get_lr(self):
        rates = self.scheduler.get_lr()
        if self.last_epoch >= self.warmup_iters:
            return rates
        scale = self._scale()
        # a tensor rate that the wrapped scheduler keeps is scaled from the float last written to it
        return [scale * (_host_rate(group) if rate is None else rate) for group, rate in zip(self.optimizer.param_groups, rates)]


class ReduceLROnPlateau(_torch_sched.ReduceLROnPlateau):
    """torch's scheduler, whose decisions are host arithmetic on the metric; only its write differs: a tensor rate is reduced from
    its float mirror and written with fill_, where torch reads the tensor back."""

    def __init__(self, optimizer, *args, **kwargs):
        for group in optimizer.param_groups:             # the mirror of a tensor rate is taken here, not during a step
            _host_rate(group)
        super().__init__(optimizer, *args, **kwargs)

    def _reduce_lr(self, epoch):
        groups = self.optimizer.param_groups
        if not any(_is_tensor_rate(group) for group in groups) or len(groups) != len(self.min_lrs):
            return super()._reduce_lr(epoch)
        for i, group in enumerate(groups):
            old_lr = float(_host_rate(group))
            new_lr = max(old_lr * self.factor, self.min_lrs[i])
            if old_lr - new_lr > self.eps:
                _write_rate(group, new_lr)


def get_schedular(optimizer, args):
    name = args.scheduler.lower()
    if name == "poly_lr":
        return PolynomialLR(optimizer, max_iter=args.max_iter, decay_iter=args.decay_iter, gamma=args.gamma)
    if name == "reduce_lr":
        return ReduceLROnPlateau(optimizer, mode="min", factor=args.factor, patience=args.lr_patience)
    raise NotImplementedError("get_schedular: no scheduler named %r (poly_lr, reduce_lr)" % (name,))


def do_schedule(args, scheduler, it=None, len=None, metrics=None):
    name = args.scheduler.lower()
    if name == "poly_lr":
        scheduler.step()
    elif name == "reduce_lr":
        missing = [k for k, v in (("it", it), ("len", len), ("metrics", metrics)) if v is None]
        if missing:
            raise RuntimeError("do_schedule: reduce_lr needs %s" % ", ".join(missing))
        epoch, within = divmod(it, len)
        if within == 0:                                  # the first iteration of an epoch
            scheduler.step(epoch=epoch, metrics=metrics)
    else:
        raise NotImplementedError("do_schedule: no scheduler named %r (poly_lr, reduce_lr)" % (name,))

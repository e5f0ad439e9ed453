"""The reference's optimiser on the device — the drop-in for `torch.optim.SGD(lr, momentum=0.9, weight_decay=1e-4)` of
main.py:72-74, whose `step()` is a line of `train_iter` (libs/trainers/single_gpu_trainer.py):

    from cspn_monodepth_amd.optim import SGD                     # was: torch.optim.SGD

One `step()` is one call of include/cspn_optim.h per parameter group: a multi-tensor kernel that carries its tensor descriptors
by value, ceil(tensors / 109) launches for the group, on the current stream, without a host synchronisation and without reading
a device value.  Its arithmetic is the bits of torch's single-tensor form (`foreach=False, fused=False`), which is what the
reference runs; torch's `fused` form multiplies by a double rate and rounds differently.

The state is `state[p]["momentum_buffer"]` and the options are torch's, so `state_dict()` / `load_state_dict()` interchange with
`torch.optim.SGD` in both directions, and the object pickles (the reference's checkpoint stores the optimiser itself).

`group["lr"]` is a Python float — passed by value and frozen into a captured graph, as in torch — or a 0-dim fp32 tensor on the
parameters' device, which the kernel reads when it RUNS: a captured step follows a schedule from replay to replay.
`lr_to_device()` converts every group's rate; the schedulers of cspn_monodepth_amd.scheduler then write it with `fill_`.  Next to
a tensor rate the group holds `lr_host`, the float last written, so that no scheduler ever has to read the tensor back.

Refused, as everywhere in this package, instead of falling back: CPU parameters, any dtype but fp32, sparse gradients,
non-contiguous parameters, parameters on more than one device, a rate tensor that is not 0-dim fp32 on that device, and a
`step()` under stream capture while a momentum buffer is still missing (the captured first step, buf = g, would replay for
ever: run one step before capturing, as torch requires too)."""
import ctypes

import torch
from torch.optim.optimizer import Optimizer

from . import _lib
from ._host import launch

__all__ = ["SGD", "sgd_step"]


def _check_hyper(lr, momentum, dampening, weight_decay, nesterov):
    if isinstance(lr, torch.Tensor):
        if lr.dim() != 0 or lr.dtype != torch.float32:
            raise ValueError("SGD: a tensor lr must be a 0-dim fp32 tensor, got shape %s %s" % (tuple(lr.shape), lr.dtype))
    elif lr < 0.0:
        raise ValueError("Invalid learning rate: %s" % (lr,))
    if momentum < 0.0:
        raise ValueError("Invalid momentum value: %s" % (momentum,))
    if weight_decay < 0.0:
        raise ValueError("Invalid weight_decay value: %s" % (weight_decay,))
    if nesterov and (momentum <= 0 or dampening != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")


def _check_tensors(params, grads, lr):
    """The per-tensor refusals of the module's docstring and the rate tensor's form -> the one device of these tensors."""
    devices = set()
    for p, g in zip(params, grads):
        if p.dtype != torch.float32 or g.dtype != torch.float32:
            raise RuntimeError("SGD: fp32 only, got a %s parameter with a %s gradient (no other dtype is built)" % (p.dtype, g.dtype))
        if g.is_sparse or g.layout != torch.strided:
            raise RuntimeError("SGD does not support sparse gradients")
        if p.is_sparse or not p.is_contiguous():
            raise RuntimeError("SGD: a parameter of shape %s is not contiguous" % (tuple(p.shape),))
        if g.shape != p.shape:
            raise RuntimeError("SGD: gradient of shape %s for a parameter of shape %s" % (tuple(g.shape), tuple(p.shape)))
        devices.add(p.device)
        devices.add(g.device)
    if len(devices) > 1:
        raise RuntimeError("SGD: parameters on more than one device (%s)" % ", ".join(sorted(str(d) for d in devices)))
    device = next(iter(devices))
    if isinstance(lr, torch.Tensor):
        if lr.dim() != 0 or lr.dtype != torch.float32 or lr.device != device:
            raise ValueError("SGD: a tensor lr must be a 0-dim fp32 tensor on %s, got shape %s %s on %s"
                             % (device, tuple(lr.shape), lr.dtype, lr.device))
    return device


def _require_one_rocm_device(devices):
    devices = sorted({str(d) for d in devices})
    if len(devices) > 1:
        raise RuntimeError("SGD: parameters on more than one device (%s)" % ", ".join(devices))
    if devices and not devices[0].startswith("cuda"):
        raise RuntimeError("SGD: parameters must live on a ROCm device, got %s (no CPU implementation here)" % devices[0])


def _prepare(params, grads, lr, momentum, dampening, weight_decay, nesterov):
    """Every check of one group that needs no launch -> the group's device (the caller holds it against the other groups')."""
    _check_hyper(lr, momentum, dampening, weight_decay, nesterov)
    return _check_tensors(params, grads, lr)


def _refuse_captured_first_step(momentum, momentum_buffers):
    missing = sum(b is None for b in momentum_buffers) if momentum != 0 else 0
    if missing and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("SGD: step() under stream capture while %d momentum buffers are missing — the captured first step "
                           "(buf = g) would be replayed for ever; run one step before capturing" % missing)


def sgd_step(params, grads, momentum_buffers, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False,
             max_workgroups=0):
    """One step over explicit lists, in place: params[i] and momentum_buffers[i] from grads[i].  With momentum, an entry of
    momentum_buffers that is None marks the tensor's first step: the buffer is created (uninitialised), written with buf = g and
    put into the list.  Without momentum the list is not looked at.  max_workgroups: the grid's cap (0 = the library's 2048)."""
    if not (len(params) == len(grads) and (momentum == 0 or len(momentum_buffers) == len(params))):
        raise ValueError("sgd_step: params, grads and momentum_buffers must have the same length")
    if not params:
        _check_hyper(lr, momentum, dampening, weight_decay, nesterov)
        return
    device = _prepare(params, grads, lr, momentum, dampening, weight_decay, nesterov)
    _require_one_rocm_device([device])
    _refuse_captured_first_step(momentum, momentum_buffers)
    _launch(device, params, grads, momentum_buffers, lr, momentum, dampening, weight_decay, nesterov, maximize, max_workgroups)


def _launch(device, params, grads, momentum_buffers, lr, momentum, dampening, weight_decay, nesterov, maximize, max_workgroups=0):
    """The step of one checked group: buffers, descriptors, one call of cspn_sgd_step on the current stream."""
    dense = [g if g.is_contiguous() else g.contiguous() for g in grads]
    first = [False] * len(params)
    if momentum != 0:
        for i in [i for i, b in enumerate(momentum_buffers) if b is None]:
            momentum_buffers[i] = torch.empty_like(params[i], memory_format=torch.contiguous_format)
            first[i] = True
        for p, b in zip(params, momentum_buffers):
            if b.dtype != torch.float32 or b.device != device or b.shape != p.shape or not b.is_contiguous():
                raise RuntimeError("SGD: a momentum buffer must be a contiguous fp32 tensor of its parameter's shape and device")
    n = len(params)
    tensors = (_lib.cspn_sgd_tensor * n)()
    for i in range(n):
        t = tensors[i]
        t.param, t.grad, t.n, t.first = params[i].data_ptr(), dense[i].data_ptr(), params[i].numel(), int(first[i])
        t.momentum_buffer = momentum_buffers[i].data_ptr() if momentum != 0 else None
    by_pointer = isinstance(lr, torch.Tensor)
    hyper = _lib.cspn_sgd_hyper(lr=0.0 if by_pointer else float(lr), lr_device=lr.data_ptr() if by_pointer else None,
                                momentum=float(momentum), dampening=float(dampening), weight_decay=float(weight_decay),
                                nesterov=int(bool(nesterov)), maximize=int(bool(maximize)))
    launch(device, "cspn_sgd_step", tensors, n, ctypes.byref(hyper), _lib.CSPN_F32, int(max_workgroups))


class SGD(Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False):
        _check_hyper(lr, momentum, dampening, weight_decay, nesterov)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:          # a state from before an option existed, or from torch.optim.SGD
            group.setdefault("nesterov", False)
            group.setdefault("maximize", False)

    def lr_to_device(self):
        """Every group's rate -> a 0-dim fp32 tensor on the group's device (the float stays in group["lr_host"]); returns self."""
        for group in self.param_groups:
            if isinstance(group["lr"], torch.Tensor):
                continue
            if not group["params"]:
                raise ValueError("SGD.lr_to_device: a group without parameters has no device")
            value = float(group["lr"])
            group["lr"] = torch.tensor(value, dtype=torch.float32, device=group["params"][0].device)
            group["lr_host"] = value
        return self

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            grads = [p.grad for p in params]
            hyper = [group[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")]
            buffers = [self.state[p].get("momentum_buffer") for p in params] if group["momentum"] != 0 else []
            work.append((_prepare(params, grads, *hyper), params, grads, buffers, hyper + [group["maximize"]]))
        _require_one_rocm_device([w[0] for w in work])                      # across the groups, before anything is launched
        for _, _, _, buffers, hyper in work:
            _refuse_captured_first_step(hyper[1], buffers)
        for device, params, grads, buffers, hyper in work:
            _launch(device, params, grads, buffers, *hyper)
            for p, b in zip(params, buffers):
                self.state[p]["momentum_buffer"] = b
        return loss

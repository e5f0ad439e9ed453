"""In-Place Activated BatchNorm on the device — the drop-in for the reference's only native component:

    from cspn_monodepth_amd.network.inplace_abn import InPlaceABN, InPlaceABNSync      # was: from network.libs.inplace_abn import ...

One module normalises, scales and activates its input IN PLACE and keeps only the output for the backward, which inverts the
activation and the affine map to recover what it needs (network/libs/inplace_abn/bn.py, functions.py, src/bn.cu).  The kernels are
include/cspn_abn.h: wave64 reductions, one read of x for the statistics, no atomics (equal bits run after run), the activation and
its inverse fused into the apply / gradient passes, one launch for a small layer and a partial / finalise / apply split for a big
one, the running statistics updated on the device — a step has no host arithmetic and no synchronisation, so it can be captured in
a graph.

What is as in the reference: y = (x - mean) / sqrt(var + eps), z = act(y * (|weight| + eps) + bias) with act one of "leaky_relu"
(slope), "elu", "none"; biased batch variance, running variance unbiased by n / (n - 1); parameter and buffer names (`weight`,
`bias`, `running_mean`, `running_var`, no `num_batches_tracked`: its checkpoints load); the modules' `__repr__`; eval-mode
backward with edz = eydz = 0 (functions.py:144-147); ValueError("Non-contiguous input").

What differs, on purpose:
  * the backward reads the saved output and the incoming gradient and modifies NEITHER (the reference overwrites the saved output
    with the pre-activation and scales the incoming gradient in place, functions.py:54-60: a second use of either is wrong there);
  * a training call with one value per channel (N * S == 1) raises ValueError before any launch, as stock BatchNorm2d does (the
    reference divides by n - 1 = 0);
  * InPlaceABNSync is one process per GPU over torch.distributed instead of one thread per GPU with queues: one all_gather of
    [2, C] per direction, merged as functions.py:196-197 / :271-272 merge them — mean = mean_r(means),
    var = mean_r(vars + (mean - means)^2), edz and eydz averaged.  Like the reference it ASSUMES THE SAME N * S ON EVERY RANK
    (the merge weighs the ranks equally).  dweight / dbias of a rank are the global edz / eydz times the rank's own N * S, as in
    the reference: summed over the ranks (DataParallel's reduce) they are the whole batch's gradients, averaged (DDP) they are
    those divided by the world size, the convention of nn.SyncBatchNorm under DDP.

fp32 and ROCm tensors only; there is no CPU implementation and no fallback."""
from collections import OrderedDict

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib
from .._host import _p, launch

ACT_LEAKY_RELU = "leaky_relu"
ACT_ELU = "elu"
ACT_NONE = "none"
_ACTIVATIONS = {ACT_LEAKY_RELU: _lib.ABN_ACT_LEAKY_RELU, ACT_ELU: _lib.ABN_ACT_ELU, ACT_NONE: _lib.ABN_ACT_NONE}

__all__ = ["ABN", "InPlaceABN", "InPlaceABNSync", "InPlaceABNWrapper", "InPlaceABNSyncWrapper", "inplace_abn", "inplace_abn_sync",
           "convert_batchnorm", "abn_plan", "ACT_LEAKY_RELU", "ACT_ELU", "ACT_NONE"]


def _ncs(x):
    n, c = x.shape[0], x.shape[1]
    s = 1
    for d in x.shape[2:]:
        s *= d
    return int(n), int(c), int(s)


def abn_plan(N, C, S):
    """cspn_abn_plan as a dict: regime ("small" / "split"), channels_per_workgroup, workgroups_per_channel, threads,
    elements_per_workgroup, small_limit.  Needs no device."""
    plan = _lib.cspn_abn_plan()
    _lib.check(_lib.lib().cspn_abn_plan(int(N), int(C), int(S), plan), "cspn_abn_plan")
    out = {name: int(getattr(plan, name)) for name, _ in plan._fields_}
    out["regime"] = "small" if plan.regime == _lib.ABN_SMALL else "split"
    return out


def _validate(x, weight, bias, running_mean, running_var, training, activation, world=1):
    """Everything that can be refused is refused here, before any launch."""
    if not all(t is None or t.is_contiguous() for t in (x, weight, bias, running_mean, running_var)):
        raise ValueError("Non-contiguous input")                          # functions.py:65-67
    for t in (x, weight, bias, running_mean, running_var):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("inplace_abn: fp32 only, got %s" % (t.dtype,))
    if activation not in _ACTIVATIONS:
        raise ValueError("inplace_abn: unknown activation %r (leaky_relu, elu, none)" % (activation,))
    if x.dim() < 2 or x.numel() < 1:
        raise ValueError("inplace_abn: expected a non-empty (N, C, ...) input, got %s" % (tuple(x.shape),))
    n, c, s = _ncs(x)
    if running_mean is None or running_var is None:
        raise ValueError("inplace_abn: running_mean / running_var are required")
    for t in (weight, bias, running_mean, running_var):
        if t is not None and tuple(t.shape) != (c,):
            raise ValueError("inplace_abn: per-channel vectors must have shape (%d,), got %s" % (c, tuple(t.shape)))
    if training and n * s * world <= 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    for t in (x, weight, bias, running_mean, running_var):
        if t is not None and not t.is_cuda:
            raise RuntimeError("inplace_abn: tensors must live on a ROCm device (no CPU implementation here)")
        if t is not None and t.device != x.device:
            raise RuntimeError("inplace_abn: all tensors must be on the input's device")


def _workspace(x, n, c, s):
    nbytes = _lib.lib().cspn_abn_workspace_bytes(n, c, s)
    return None if nbytes == 0 else torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=x.device)


def _native_forward(x, weight, bias, running_mean, running_var, mean, var, training, phase, momentum, eps, activation, slope):
    n, c, s = _ncs(x)
    work = _workspace(x, n, c, s)
    launch(x.device, "cspn_abn_forward", x.data_ptr(), _p(weight), _p(bias), _p(running_mean), _p(running_var), _p(mean),
           _p(var), n, c, s, int(bool(training)), phase, float(momentum), float(eps), _ACTIVATIONS[activation], float(slope), _p(work))


def _native_backward_reduce(z, dz, weight, bias, edz, eydz, eps, activation, slope):
    n, c, s = _ncs(z)
    work = _workspace(z, n, c, s)
    launch(z.device, "cspn_abn_backward_reduce", z.data_ptr(), dz.data_ptr(), _p(weight), _p(bias), edz.data_ptr(), eydz.data_ptr(),
           n, c, s, float(eps), _ACTIVATIONS[activation], float(slope), _p(work))


def _native_backward(z, dz, var, weight, bias, edz, eydz, dx, dweight, dbias, training, eps, activation, slope):
    n, c, s = _ncs(z)
    work = _workspace(z, n, c, s)
    launch(z.device, "cspn_abn_backward", z.data_ptr(), dz.data_ptr(), var.data_ptr(), _p(weight), _p(bias), _p(edz), _p(eydz),
           dx.data_ptr(), _p(dweight), _p(dbias), n, c, s, int(bool(training)), float(eps), _ACTIVATIONS[activation], float(slope), _p(work))


def _cotangent(dz, z):
    if dz.dtype != torch.float32 or dz.device != z.device:
        dz = dz.to(device=z.device, dtype=torch.float32)
    return dz.contiguous()                      # never written: a copy is made only where the layout asks for one


def _grad_buffers(ctx, z, weight, bias):
    dx = torch.empty_like(z)
    dweight = torch.empty_like(weight) if weight is not None and ctx.needs_input_grad[1] else None
    dbias = torch.empty_like(bias) if bias is not None and ctx.needs_input_grad[2] else None
    return dx, dweight, dbias


class _InPlaceABN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training=True, momentum=0.1, eps=1e-05,
                activation=ACT_LEAKY_RELU, slope=0.01):
        ctx.training, ctx.eps, ctx.activation, ctx.slope = training, eps, activation, slope
        mean = var = None
        if training:
            mean, var = x.new_empty((2, x.shape[1])).unbind(0)
        _native_forward(x, weight, bias, running_mean, running_var, mean, var, training, _lib.ABN_FULL, momentum, eps, activation, slope)
        ctx.var = var if training else running_var
        ctx.save_for_backward(x, weight, bias)
        ctx.mark_dirty(x)
        return x

    @staticmethod
    @once_differentiable                         # double backward raises
    def backward(ctx, dz):
        z, weight, bias = ctx.saved_tensors
        dz = _cotangent(dz, z)
        dx, dweight, dbias = _grad_buffers(ctx, z, weight, bias)
        _native_backward(z, dz, ctx.var, weight, bias, None, None, dx, dweight, dbias, ctx.training, ctx.eps, ctx.activation, ctx.slope)
        return (dx if ctx.needs_input_grad[0] else None), dweight, dbias, None, None, None, None, None, None, None


def _all_gather(t, group):
    import torch.distributed as dist
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size(group))]
    dist.all_gather(parts, t, group=group)
    return torch.stack(parts)                    # [world, 2, C], the same on every rank


class _InPlaceABNSync(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, group, training=True, momentum=0.1, eps=1e-05,
                activation=ACT_LEAKY_RELU, slope=0.01):
        import torch.distributed as dist
        ctx.training, ctx.eps, ctx.activation, ctx.slope, ctx.group = training, eps, activation, slope, group
        if training:
            n, c, s = _ncs(x)
            local = x.new_empty((2, c))
            _native_forward(x, None, None, None, None, local[0], local[1], True, _lib.ABN_STATS_ONLY, momentum, eps, activation, slope)
            both = _all_gather(local, group)
            means, variances = both[:, 0], both[:, 1]
            mean = means.mean(0)
            var = (variances + (mean - means) ** 2).mean(0)
            count = n * s * dist.get_world_size(group)
            running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
            running_var.mul_(1 - momentum).add_(var, alpha=momentum * count / (count - 1))
            _native_forward(x, weight, bias, None, None, mean, var, True, _lib.ABN_APPLY_ONLY, momentum, eps, activation, slope)
        else:
            var = running_var
            _native_forward(x, weight, bias, running_mean, running_var, None, None, False, _lib.ABN_FULL, momentum, eps, activation, slope)
        ctx.var = var
        ctx.save_for_backward(x, weight, bias)
        ctx.mark_dirty(x)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        z, weight, bias = ctx.saved_tensors
        dz = _cotangent(dz, z)
        dx, dweight, dbias = _grad_buffers(ctx, z, weight, bias)
        edz = eydz = None
        if ctx.training:
            local = z.new_empty((2, z.shape[1]))
            _native_backward_reduce(z, dz, weight, bias, local[0], local[1], ctx.eps, ctx.activation, ctx.slope)
            edz, eydz = _all_gather(local, ctx.group).mean(0).unbind(0)
        _native_backward(z, dz, ctx.var, weight, bias, edz, eydz, dx, dweight, dbias, ctx.training, ctx.eps, ctx.activation, ctx.slope)
        return (dx if ctx.needs_input_grad[0] else None), dweight, dbias, None, None, None, None, None, None, None, None


def inplace_abn(x, weight, bias, running_mean, running_var, training=True, momentum=0.1, eps=1e-05, activation=ACT_LEAKY_RELU,
                slope=0.01):
    """The functional form (functions.py:70-109): x is overwritten and returned (the result shares x's storage)."""
    _validate(x, weight, bias, running_mean, running_var, training, activation)
    return _InPlaceABN.apply(x, weight, bias, running_mean, running_var, training, momentum, eps, activation, slope)


def _world_size(group):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def inplace_abn_sync(x, weight, bias, running_mean, running_var, process_group=None, training=True, momentum=0.1, eps=1e-05,
                     activation=ACT_LEAKY_RELU, slope=0.01):
    """inplace_abn with the batch statistics (and the backward's two reductions) taken over every rank of `process_group` (None:
    the default group).  The reference's sixth argument was its dictionary of queues; here it is the group.  Without an
    initialised torch.distributed, or with a world size of 1, this IS inplace_abn."""
    world = _world_size(process_group)
    _validate(x, weight, bias, running_mean, running_var, training, activation, world)
    if world == 1:
        return _InPlaceABN.apply(x, weight, bias, running_mean, running_var, training, momentum, eps, activation, slope)
    return _InPlaceABNSync.apply(x, weight, bias, running_mean, running_var, process_group, training, momentum, eps, activation, slope)


class ABN(nn.Sequential):
    """Activated Batch Normalization out of stock ops: a `BatchNorm2d` and an activation module (bn.py:24-45)."""

    def __init__(self, num_features, activation=None, **kwargs):
        super(ABN, self).__init__(OrderedDict([
            ("bn", nn.BatchNorm2d(num_features, **kwargs)),
            ("act", nn.ReLU(inplace=True) if activation is None else activation)
        ]))


class InPlaceABN(nn.Module):
    """InPlace Activated Batch Normalization (bn.py:48-105)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, activation="leaky_relu", slope=0.01):
        super(InPlaceABN, self).__init__()
        if activation not in _ACTIVATIONS:
            raise ValueError("InPlaceABN: unknown activation %r (leaky_relu, elu, none)" % (activation,))
        self.num_features = num_features
        self.affine = affine
        self.eps = eps
        self.momentum = momentum
        self.activation = activation
        self.slope = slope
        if self.affine:
            self.weight = nn.Parameter(torch.empty(num_features))
            self.bias = nn.Parameter(torch.empty(num_features))
        else:
            self.register_parameter('weight', None)
            self.register_parameter('bias', None)
        self.register_buffer('running_mean', torch.zeros(num_features))
        self.register_buffer('running_var', torch.ones(num_features))
        self.reset_parameters()

    def reset_parameters(self):
        self.running_mean.zero_()
        self.running_var.fill_(1)
        if self.affine:
            self.weight.data.fill_(1)
            self.bias.data.zero_()

    def forward(self, x):
        return inplace_abn(x, self.weight, self.bias, self.running_mean, self.running_var, self.training, self.momentum, self.eps,
                           self.activation, self.slope)

    def __repr__(self):
        rep = '{name}({num_features}, eps={eps}, momentum={momentum},' \
              ' affine={affine}, activation={activation}'
        if self.activation == "leaky_relu":
            rep += ' slope={slope})'
        else:
            rep += ')'
        return rep.format(name=self.__class__.__name__, **self.__dict__)


class InPlaceABNSync(InPlaceABN):
    """InPlaceABN with statistics over every rank of `process_group` (bn.py:108-193, re-hosted on torch.distributed: one process
    per GPU).  `devices` is accepted for source compatibility and ignored, apart from being shown by `__repr__`."""

    def __init__(self, num_features, devices=None, eps=1e-5, momentum=0.1, affine=True, activation="leaky_relu", slope=0.01,
                 process_group=None):
        super(InPlaceABNSync, self).__init__(num_features, eps, momentum, affine, activation, slope)
        self.devices = devices
        self.process_group = process_group

    def forward(self, x):
        return inplace_abn_sync(x, self.weight, self.bias, self.running_mean, self.running_var, self.process_group, self.training,
                                self.momentum, self.eps, self.activation, self.slope)

    def __repr__(self):
        rep = '{name}({num_features}, eps={eps}, momentum={momentum},' \
              ' affine={affine}, devices={devices}, activation={activation}'
        if self.activation == "leaky_relu":
            rep += ' slope={slope})'
        else:
            rep += ')'
        return rep.format(name=self.__class__.__name__, **self.__dict__)


class InPlaceABNWrapper(nn.Module):
    """Wrapper module to make `InPlaceABN` compatible with `ABN` (bn.py:196-204)."""

    def __init__(self, *args, **kwargs):
        super(InPlaceABNWrapper, self).__init__()
        self.bn = InPlaceABN(*args, **kwargs)

    def forward(self, input):
        return self.bn(input)


class InPlaceABNSyncWrapper(nn.Module):
    """Wrapper module to make `InPlaceABNSync` compatible with `ABN` (bn.py:207-215)."""

    def __init__(self, *args, **kwargs):
        super(InPlaceABNSyncWrapper, self).__init__()
        self.bn = InPlaceABNSync(*args, **kwargs)

    def forward(self, input):
        return self.bn(input)


def convert_batchnorm(module, activation="none", sync=False, process_group=None):
    """Every nn.BatchNorm2d of a module tree replaced by InPlaceABN (sync=True: InPlaceABNSync on `process_group`) with the given
    activation, parameters and running statistics carried over — as nn.SyncBatchNorm.convert_sync_batchnorm does for its class.
    `convert_batchnorm(unet_ours.resnet50(), sync=True)` is the reference's multi-GPU model (its unet_ours.py:23-28:
    every normalisation layer an InPlaceABNSync(activation='none')), and a checkpoint of that configuration loads into it.

    Mind the one difference in meaning: the scale of an InPlaceABN is |weight| + eps, that of a BatchNorm2d is weight."""
    out = module
    if isinstance(module, nn.BatchNorm2d):
        if not module.track_running_stats or module.momentum is None:
            raise ValueError("convert_batchnorm: InPlaceABN keeps running statistics with a fixed momentum; got %r" % (module,))
        if sync:
            out = InPlaceABNSync(module.num_features, None, module.eps, module.momentum, module.affine, activation,
                                 process_group=process_group)
        else:
            out = InPlaceABN(module.num_features, module.eps, module.momentum, module.affine, activation)
        out.to(module.running_mean.device)
        with torch.no_grad():
            if module.affine:
                out.weight.copy_(module.weight)
                out.bias.copy_(module.bias)
                out.weight.requires_grad_(module.weight.requires_grad)
                out.bias.requires_grad_(module.bias.requires_grad)
            out.running_mean.copy_(module.running_mean)
            out.running_var.copy_(module.running_var)
        out.training = module.training
    for name, child in module.named_children():
        out.add_module(name, convert_batchnorm(child, activation, sync, process_group))
    return out

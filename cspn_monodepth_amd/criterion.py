"""The reference's training criteria on the device — the drop-in for `libs.criterion`:

    from cspn_monodepth_amd.criterion import get_criteria        # was: from libs.criterion import get_criteria

`get_criteria(args)` offers what the reference's does (libs/criterion/__init__.py:11-30): `args.criterion` in l1 / l2 / l1_log
-> MaskedL1Loss / MaskedMSELoss / L1_log (criteria.py:14-39, 91-107), wrapped by `args.loss_wrapper`: "dsn" -> CriterionDSN
(loss1 + 0.4 * loss2), anything else -> Criterion_No_DSN (criteria.py:170-219).

The reference's other working criteria are modules to construct directly, as get_criteria does not offer them there either:
berHuLoss (criteria.py:42-64; works inside both wrappers), RMSE, RMSE_log, L1 and GradLoss (:67-88, :133-152), on the kernels
of include/cspn_losses.h — berHu's threshold 0.2 * max(pred - target) is a dependent pass on the device, three launches
forward, and never reaches the host.  BerHu(threshold) and NormalLoss are not built: the reference's BerHu raises IndexError
(`.numpy()[0]` on a 0-dim array) and its NormalLoss divides [B,C,H,W] by a [B,C,H] norm, which raises for almost every shape.

The reference selects the valid pixels with `diff[valid_mask]`: boolean indexing calls nonzero, a device-to-host copy on every
step that no graph can capture.  Here a loss is three launches of include/cspn_criterion.h on the current stream — per-slice
sums and their combination forward, one streaming kernel backward — with no atomics, no `.item()`, no nonzero and no host
synchronisation; the loss is a 0-dim fp32 device tensor, deterministic to the bit (a function of the values, the kind and the
element count only), and the whole step can sit inside a `torch.cuda.graph` capture.

fp32 only, on purpose: the criterion is a mean, so a valid pixel's gradient is g / count — about 1e-6 for a 24 x 228 x 304
batch, below what fp16 can hold.  A half prediction raises TypeError; cast it with `.float()` in front of the criterion (the
cast's backward rounds the gradient once, where the caller can see it)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._host import launch

KINDS = {"l1": _lib.LOSS_L1, "l2": _lib.LOSS_L2, "l1_log": _lib.LOSS_L1_LOG}
MEAN_KINDS = {"l1": _lib.MEAN_L1, "grad": _lib.MEAN_GRAD, "rmse": _lib.MEAN_RMSE, "rmse_log": _lib.MEAN_RMSE_LOG}
STATE_BYTES = 32     # CSPN_CRITERION_STATE_BYTES: float loss, float 1 / count, double sum, double count, 8 reserved

_FP32_ONLY = ("%s: fp32 only, got %s — the gradient of a mean over ~1e6 pixels (g / count) is below the smallest fp16 "
              "subnormal; cast the prediction with .float() first")


def criterion_workspace(n, device):
    """(work, state) of one forward over n elements.  Fresh from torch's caching allocator on every call — which hands back the
    same blocks step after step without a synchronisation, also inside a graph capture — because a state belongs to ONE
    forward until its backward has run: CriterionDSN has two forwards of the same size alive at once."""
    nbytes = _lib.lib().cspn_criterion_workspace_bytes(int(n))
    return (torch.empty((nbytes // 8,), dtype=torch.float64, device=device),
            torch.empty((STATE_BYTES // 4,), dtype=torch.float32, device=device))


def losses_workspace(n, device):
    """(work, state) of one forward of include/cspn_losses.h over n elements; fresh on every call, as criterion_workspace."""
    nbytes = _lib.lib().cspn_losses_workspace_bytes(int(n))
    return (torch.empty((nbytes // 8,), dtype=torch.float64, device=device),
            torch.empty((_lib.LOSSES_STATE_BYTES // 4,), dtype=torch.float32, device=device))


# family -> (forward entry, backward entry, workspace function, whether the entries take a `kind`)
_FAMILIES = {"masked": ("cspn_criterion_forward", "cspn_criterion_backward", criterion_workspace, True),
             "berhu": ("cspn_berhu_forward", "cspn_berhu_backward", losses_workspace, False),
             "mean": ("cspn_mean_loss_forward", "cspn_mean_loss_backward", losses_workspace, True)}


class _Loss(torch.autograd.Function):
    """One loss of a family of _FAMILIES over (a, b) = (pred, target) / (fake, real), with a gradient for `a` only."""

    @staticmethod
    def forward(ctx, a, b, family, kind):
        entry, _, workspace, has_kind = _FAMILIES[family]
        n = a.numel()
        work, state = workspace(n, a.device)
        launch(a.device, entry, a.data_ptr(), b.data_ptr(), _lib.CSPN_F32, *((kind,) if has_kind else ()), n, work.data_ptr(), state.data_ptr())
        ctx.save_for_backward(a, b)
        ctx.state, ctx.family, ctx.kind = state, family, kind
        return state[0]                                  # 0-dim view of the state's first word: no copy, no launch

    @staticmethod
    @torch.autograd.function.once_differentiable         # double backward raises
    def backward(ctx, grad_loss):
        a, b = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        _, entry, _, has_kind = _FAMILIES[ctx.family]
        g = grad_loss
        if g.dtype != torch.float32 or g.device != a.device:
            g = g.to(device=a.device, dtype=torch.float32)
        g = g.contiguous()
        grad = torch.empty_like(a, memory_format=torch.contiguous_format)
        launch(a.device, entry, a.data_ptr(), b.data_ptr(), _lib.CSPN_F32, *((ctx.kind,) if has_kind else ()), a.numel(),
               ctx.state.data_ptr(), g.data_ptr(), grad.data_ptr())
        return grad, None, None, None


def _apply(who, family, a, b, kind=None):
    """The one validation of every loss here, then the launches: fp32 `a`, equal shapes and devices, at least one element, a ROCm
    device; `b` is detached and cast to fp32, both are made contiguous."""
    if a.dtype != torch.float32:
        raise TypeError(_FP32_ONLY % (who, a.dtype))
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("%s: both tensors must have the same shape and device, got %s and %s" % (who, tuple(a.shape), tuple(b.shape)))
    if a.numel() < 1:
        raise ValueError("%s: empty tensors" % who)
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError("%s: tensors must live on a ROCm device (no CPU implementation here)" % who)
    b = b.detach()
    if b.dtype != torch.float32:
        b = b.float()
    return _Loss.apply(a.contiguous(), b.contiguous(), family, kind)


def masked_loss(pred, target, kind):
    """mean over target > 0 of |t - p| ("l1"), (t - p)^2 ("l2") or |log t - log p| ("l1_log"): a 0-dim fp32 device tensor with
    a gradient for `pred` only.  No valid pixel: NaN, and a zero gradient, as the reference gives."""
    if kind not in KINDS:
        raise NotImplementedError("masked_loss: no criterion named %r (l1, l2, l1_log)" % (kind,))
    return _apply("masked_loss", "masked", pred, target, KINDS[kind])


def _resized(pred, target):
    """pred at the target's spatial size: a stock bilinear resize with align_corners=True when the sizes differ."""
    if tuple(pred.shape[-2:]) == tuple(target.shape[-2:]):
        return pred
    return F.interpolate(pred, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)


class _Masked(nn.Module):
    """One kind of masked_loss as a module; the result is also kept in self.loss."""
    kind = None

    def forward(self, pred, target):
        if pred.dim() != target.dim():
            raise AssertionError("inconsistent dimensions")
        self.loss = masked_loss(pred, target, self.kind)
        return self.loss


class MaskedL1Loss(_Masked):
    kind = "l1"


class MaskedMSELoss(_Masked):
    kind = "l2"


class L1_log(nn.Module):
    """(fake, real), as the reference names them; a prediction of another size is resized to the target's first."""

    def forward(self, fake, real):
        if fake.dim() != real.dim():
            raise AssertionError("inconsistent dimensions")
        return masked_loss(_resized(fake, real), real, "l1_log")


class _Wrapper(nn.Module):
    def __init__(self, criterion=None):
        super().__init__()
        self.criterion = criterion

    def _one(self, pred, target):
        return self.criterion(_resized(pred, target), target)


class Criterion_No_DSN(_Wrapper):
    """One output: criterion(preds[0], target), preds[0] resized to the target's size when it differs (criteria.py:170-188)."""

    def forward(self, preds, target):
        return self._one(preds[0], target)


class CriterionDSN(_Wrapper):
    """Deep supervision: criterion(preds[0], target) + 0.4 * criterion(preds[1], target), each prediction resized to the
    target's size when it differs (criteria.py:191-219).  The second backward receives 0.4 as its incoming gradient."""

    def forward(self, preds, target):
        return self._one(preds[0], target) + 0.4 * self._one(preds[1], target)


def berhu_loss(pred, target):
    """The reverse Huber loss of criteria.py:42-64: c = 0.2 * max(pred - target) over ALL pixels, d = |target - pred| over
    target > 0, mean of the d and of the d^2 of those with d > c — a 0-dim fp32 device tensor with a gradient for `pred` only
    (c enters a comparison only).  No valid pixel: NaN, and a zero gradient.  Inputs as masked_loss takes them."""
    return _apply("berhu_loss", "berhu", pred, target)


def unmasked_loss(fake, real, kind):
    """A mean over all elements: "l1" mean |10 r - 10 f|, "grad" mean |r - f|, "rmse" sqrt(mean (10 r - 10 f)^2), "rmse_log"
    sqrt(mean (log r - log f)^2) — a 0-dim fp32 device tensor with a gradient for `fake` only."""
    if kind not in MEAN_KINDS:
        raise NotImplementedError("unmasked_loss: no criterion named %r (%s)" % (kind, ", ".join(MEAN_KINDS)))
    return _apply("unmasked_loss", "mean", fake, real, MEAN_KINDS[kind])


class berHuLoss(nn.Module):
    """criteria.py:42-64; the result is also kept in self.loss."""

    def forward(self, pred, target):
        if pred.dim() != target.dim():
            raise AssertionError("inconsistent dimensions")
        self.loss = berhu_loss(pred, target)
        return self.loss


class GradLoss(nn.Module):
    """criteria.py:145-152: mean |target - pred|."""

    def forward(self, pred, target):
        if pred.dim() != target.dim():
            raise AssertionError("inconsistent dimensions")
        return unmasked_loss(pred, target, "grad")


class _Unmasked(nn.Module):
    """(fake, real); a fake of another shape is resized as the reference's F.upsample does: bilinear, align_corners=False."""
    kind = None

    def forward(self, fake, real):
        if fake.shape != real.shape and fake.dim() == 4 and real.dim() == 4:
            fake = F.interpolate(fake, size=tuple(real.shape[-2:]), mode="bilinear", align_corners=False)
        return unmasked_loss(fake, real, self.kind)


class RMSE(_Unmasked):
    kind = "rmse"


class RMSE_log(_Unmasked):
    kind = "rmse_log"


class L1(_Unmasked):
    kind = "l1"


key_to_criteria = {"l1": MaskedL1Loss, "l2": MaskedMSELoss, "l1_log": L1_log}


def get_criteria(args):
    """args.criterion: a key of key_to_criteria; anything else raises NotImplementedError (the reference prints args.arch and
    raises it bare; here the message names the key, and args.arch is not read).  args.loss_wrapper: "dsn" in any letter case ->
    CriterionDSN, anything else -> Criterion_No_DSN."""
    if args.criterion not in key_to_criteria:
        raise NotImplementedError("no available criterion method named %r (%s)" % (args.criterion, ", ".join(key_to_criteria)))
    wrapper = CriterionDSN if args.loss_wrapper.lower() == "dsn" else Criterion_No_DSN
    return wrapper(criterion=key_to_criteria[args.criterion]())

"""Depth metrics on device + the batch-shard / metrics all-gather used for multi-GPU inference.

Reference formulas: libs/metrics.py:49-83 (Result.evaluate) and the on-device twin
network/libs/base/base_model.py:28-73, whose 10-vector order (irmse, imae, mse, rmse, mae, absrel,
lg10, delta1, delta2, delta3) is kept.  The reference averages the per-GPU vectors with an
in-process Reduce (network/libs/base/encoding.py:264-276), which is only right for equal valid-pixel
counts; here every rank contributes additive masked *sums* + the count, gathered with one
torch.distributed all_gather (RCCL over xGMI when the backend is "nccl"), then finalised.

Three meters, three different figures (they agree for mse / mae / absrel / lg10 / delta only when every unit has the same
valid-pixel count, and never exactly for rmse / irmse — a mean of square roots is not the square root of the mean):

* pixel-weighted sums — `metric_sums` (+ `all_gather_metric_sums`) -> `finalize_metrics`: every valid pixel of everything
  accumulated counts once, one square root at the end.  The multi-GPU figure; NOT what the reference prints.
* per batch — `BatchAverageMeter`: Result.evaluate on each BATCH, weighted by the batch size (libs/metrics.py:49-127 as the
  trainers call it).  Host-side: one `.cpu()` (a stream synchronisation) per update.  Equals the reference's printed
  averages only when the caller really runs batch size 1, as the reference's evaluation loader does
  (dataloaders/nyu_dataloader/__init__.py:59-60).
* per frame — `metric_sums_per_frame` / `FrameAverageMeter` (+ `all_gather_frame_meter`): Result.evaluate on each FRAME and
  AverageMeter.update(n = 1) over frames, both on the device (cspn_metrics_per_frame, cspn_meter_update).  This is what
  `trainer.eval` prints (libs/trainers/single_gpu_trainer.py:114-206) — at ANY batch size, without a host synchronisation
  per batch, and capturable in a graph: frame i's sums do not depend on the batch it arrived in.
"""
import math

import torch
import torch.distributed as dist

from . import _lib
from . import functional as _F
from ._host import launch

METRIC_NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")
N_SUMS = 10   # {inv^2, inv, diff^2, diff, diff/t, |dlog10|, #<1.25, #<1.25^2, #<1.25^3, n}
N_SLOTS = 1024  # accumulator rows: >= workgroups per launch, so no two blocks contend on one fp64 atomic address


def new_accumulator(device):
    """Zeroed [N_SLOTS, 10] float64 accumulator for metric_sums(..., out=acc) in a loop over batches."""
    return torch.zeros((N_SLOTS, N_SUMS), dtype=torch.float64, device=device)


def shard_bounds(n_items, rank, world_size):
    """Contiguous batch chunks: rank r gets [lo, hi); remainders go to the low ranks."""
    base, rem = divmod(int(n_items), int(world_size))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def metric_sums(pred, target, out=None):
    """Masked sums over target > 0 (one fused HIP reduction kernel).

    Without `out`: returns the float64[10] sums.  With `out` (from new_accumulator): accumulates into its
    rows and returns it, so a loop over batches needs neither a host sync nor an extra reduction launch."""
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("metric_sums: tensors must live on a ROCm device (no CPU implementation here)")
    if pred.shape != target.shape or pred.dtype != target.dtype:
        raise ValueError("pred / target must have the same shape and dtype")
    p, t = pred.contiguous(), target.contiguous()
    acc = new_accumulator(p.device) if out is None else out
    if acc.dtype != torch.float64 or acc.dim() != 2 or acc.shape[1] != N_SUMS or not acc.is_contiguous():
        raise ValueError("out must be a contiguous float64 [nslots, 10] tensor (evaluation.new_accumulator)")
    dt = _lib.CSPN_F32 if p.dtype == torch.float32 else _lib.CSPN_F16 if p.dtype == torch.float16 else None
    if dt is None:
        raise TypeError("metric_sums supports float32 / float16")
    launch(p.device, "cspn_metrics_accumulate", p.data_ptr(), t.data_ptr(), dt, p.numel(), acc.data_ptr(), int(acc.shape[0]))
    return acc.sum(0) if out is None else acc


def finalize_metrics(sums):
    """float64[10] sums -> dict of the reference's 10 metrics + 'count'."""
    # the numbers are about to be used on the host: a weight-resident launch that timed out is repaired here (or raised, when it
    # cannot be), not averaged in (a device tensor is waited for first; a host tensor has been through a synchronising copy already)
    if getattr(sums, "is_cuda", False):
        _F.ensure_resident_ok(sums.device)
    else:
        _F.check_resident_errors()
    if hasattr(sums, "dim") and sums.dim() == 2:
        sums = sums.sum(0)
    s = [float(v) for v in sums]
    n = s[9]
    if n <= 0:
        return dict({k: float("nan") for k in METRIC_NAMES}, count=0)
    mse = s[2] / n
    return dict(irmse=math.sqrt(s[0] / n), imae=s[1] / n, mse=mse, rmse=math.sqrt(mse), mae=s[3] / n,
                absrel=s[4] / n, lg10=s[5] / n, delta1=s[6] / n, delta2=s[7] / n, delta3=s[8] / n,
                count=int(round(n)))


class BatchAverageMeter(object):
    """The reference's averaging, for numbers comparable with its logs: `Result.evaluate` finalises the metrics PER BATCH
    (libs/metrics.py:49-83: rmse = sqrt of that batch's mse, irmse likewise) and `AverageMeter` averages those per-batch
    values weighted by the batch size n (libs/metrics.py:101-127, called with n = input.size(0) by the trainers).

    `finalize_metrics` over accumulated sums is the pixel-weighted GLOBAL figure instead (one sqrt over all pixels):
    the two agree for mse / mae / absrel / lg10 / delta only when every batch has the same valid-pixel count, and
    never exactly for rmse / irmse (mean of square roots != square root of the mean).  Use this class to reproduce the
    reference's printed averages; use the sums for the all-gathered multi-GPU figure.

        meter = BatchAverageMeter()
        for batch: meter.update(metric_sums(pred, target), n=pred.shape[0])      # one float64[10] per batch
        meter.average()  ->  dict of the 10 metrics (+ 'count' = number of samples, as AverageMeter.count)"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.count = 0.0
        self.sums = {k: 0.0 for k in METRIC_NAMES}

    def update(self, batch_sums, n=1):
        # (a batch without valid pixels records NaN, as the reference's Result.evaluate would)
        fin = finalize_metrics(batch_sums.cpu() if hasattr(batch_sums, "cpu") else batch_sums)
        self.count += n
        for k in METRIC_NAMES:
            self.sums[k] += n * fin[k]
        return fin

    def average(self):
        if self.count <= 0:
            return dict({k: float("nan") for k in METRIC_NAMES}, count=0)
        return dict({k: self.sums[k] / self.count for k in METRIC_NAMES}, count=self.count)


def all_gather_metric_sums(sums, group=None, force_collective=False):
    """All-gather the per-rank sums (world x 10 float64) and add them.  Works with gloo (CPU) and nccl/RCCL.

    This is where an evaluation loop hands its numbers on, so it first waits for the weight-resident launches that
    produced them; one that timed out is re-run on the multi-launch schedule and its metric sums are corrected
    (functional.ensure_resident_ok) — also for the last batch of the loop, which no later launch would check.  Returns (total [10], per_rank [world, 10]), independent tensors."""
    initialised = dist.is_available() and dist.is_initialized()
    if not initialised or (dist.get_world_size(group) == 1 and not force_collective):
        # one rank: nothing to gather (force_collective: run the collective anyway — the world-size-1 RCCL test and bench.py's
        # forced group).  The copies are enqueued BEHIND the launches first and the wait + check comes after: the same
        # guarantee (nothing is returned from a timed-out launch), without two kernel launches into an idle queue
        n0 = _F.resident_fallbacks()
        total = sums.sum(0) if sums.dim() == 2 else sums.clone()
        per_rank = total.clone().unsqueeze(0)
        if sums.is_cuda:
            _F.ensure_resident_ok(sums.device)
            if _F.resident_fallbacks() != n0:          # a timed-out launch was repaired (its sums corrected) after the copies
                total = sums.sum(0) if sums.dim() == 2 else sums.clone()
                per_rank = total.clone().unsqueeze(0)
        return total, per_rank
    if sums.is_cuda:
        _F.ensure_resident_ok(sums.device)
    if sums.dim() == 2:
        sums = sums.sum(0)
    world = dist.get_world_size(group)
    src = sums.contiguous()
    if sums.is_cuda and dist.get_backend(group) == "gloo":
        src = src.cpu()                                   # gloo dry runs: gather through host memory
    parts = [torch.empty_like(src) for _ in range(world)]
    dist.all_gather(parts, src, group=group)
    stacked = torch.stack(parts, 0).to(sums.device)
    return stacked.sum(0), stacked


# ---------------------------------------------------------------------------------------------------------------------
# per-frame sums and the reference's per-frame meter, on the device
# ---------------------------------------------------------------------------------------------------------------------
N_METER = 12   # meter state: sum over frames of the 10 metrics, frames, valid pixels


def _frames(pred, target, who):
    """-> (pred, target) contiguous, B, pixels per frame, dtype code."""
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("%s: tensors must live on a ROCm device (no CPU implementation here)" % who)
    if pred.shape != target.shape or pred.dtype != target.dtype or pred.device != target.device:
        raise ValueError("pred / target must have the same shape, dtype and device")
    if pred.dim() == 4 and pred.shape[1] != 1 or pred.dim() not in (3, 4):
        raise ValueError("pred / target must be [B,1,H,W] or [B,H,W], got %s" % (tuple(pred.shape),))
    dt = _lib.CSPN_F32 if pred.dtype == torch.float32 else _lib.CSPN_F16 if pred.dtype == torch.float16 else None
    if dt is None:
        raise TypeError("%s supports float32 / float16" % who)
    B, n = int(pred.shape[0]), int(pred.shape[-2]) * int(pred.shape[-1])
    if B < 1 or n < 1:
        raise ValueError("empty batch")
    return pred.contiguous(), target.contiguous(), B, n, dt


def per_frame_workspace(B, pixels_per_frame, device):
    """The scratch tensor one cspn_metrics_per_frame launch pair needs for B frames of that size."""
    nbytes = _lib.lib().cspn_metrics_per_frame_workspace_bytes(int(B), int(pixels_per_frame))
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=device)


def _per_frame_launch(p, t, dt, B, n, work, sums):
    launch(p.device, "cspn_metrics_per_frame", p.data_ptr(), t.data_ptr(), dt, B, n, work.data_ptr(), sums.data_ptr())


def metric_sums_per_frame(pred, target, out=None):
    """The ten masked sums of `metric_sums`, for every frame: float64 [B, 10] on the device (row i: frame i; `out`, when given,
    is overwritten).  pred / target [B,1,H,W] or [B,H,W], float32 / float16.  One launch pair whatever B is, no atomics, and
    frame i's row is bit-identical wherever that frame sits — alone, at another position of another batch, at an unaligned
    address (include/cspn_hip.h: cspn_metrics_per_frame).  finalize_metrics(row) is that frame's Result.evaluate."""
    p, t, B, n, dt = _frames(pred, target, "metric_sums_per_frame")
    if out is None:
        out = torch.empty((B, N_SUMS), dtype=torch.float64, device=p.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (B, N_SUMS) or not out.is_contiguous() or out.device != p.device:
        raise ValueError("out must be a contiguous float64 [B, 10] tensor on the inputs' device")
    _per_frame_launch(p, t, dt, B, n, per_frame_workspace(B, n, p.device), out)
    return out


def average_from_state(state):
    """The 12 doubles of a FrameAverageMeter (host or device tensor) -> dict of the ten averages + 'count' (frames)."""
    m = [float(v) for v in state]
    frames = m[10]
    if frames <= 0:
        return dict({k: float("nan") for k in METRIC_NAMES}, count=0)
    return dict({k: m[i] / frames for i, k in enumerate(METRIC_NAMES)}, count=int(round(frames)))


class FrameAverageMeter(object):
    """The reference's evaluation protocol (`trainer.eval`, libs/trainers/single_gpu_trainer.py:114-206: batch size 1,
    Result.evaluate per frame, AverageMeter over frames) for batches of any size, entirely on the device:

        meter = FrameAverageMeter(device)
        for batch: meter.update(pred, target)        # two launches; no host synchronisation, no allocation (see below)
        meter.average()  ->  dict of the ten metrics + 'count' (frames)   -- the one place that synchronises

    `update` enqueues cspn_metrics_per_frame (per-frame sums) and cspn_meter_update (finalise every frame, add to the 12-double
    state) on the current stream.  After the first call with a given (B, H, W, dtype) it allocates nothing, so it can sit inside
    a `torch.cuda.graph` capture / `GraphedForward` (warm it up once with that shape first); every replay adds the batch again.
    The state after N frames is bit-identical however the frames were cut into batches.  If the spatial sizes differ, `pred`
    is resized to the target's as libs/metrics.py:52-55 does (a stock bilinear interpolation, which does allocate).

    Which producers may feed a sync-free loop: `average()` calls functional.ensure_resident_ok first, so a weight-resident
    launch that timed out is dealt with before numbers are reported — but the frames were scored when `update` ran.  The
    modules' plain forward is safe (it is device-guarded: a timed-out launch is re-computed on the stream before anything
    downstream reads it).  The output of `forward_scored` is repaired on the HOST, i.e. after this meter has already read it:
    do not feed it here unless functional.set_resident_guard("all") covers that launch."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FrameAverageMeter: needs a ROCm device (no CPU implementation here)")
        self._meter = None      # allocated with the first use: constructing a meter touches no device
        self._buffers = {}      # (B, pixels per frame) -> (workspace, sums [B,10])

    @property
    def meter(self):
        if self._meter is None:
            self._meter = torch.zeros((N_METER,), dtype=torch.float64, device=self.device)
        return self._meter

    def reset(self):
        self.meter.zero_()

    def _buf(self, B, n):
        buf = self._buffers.get((B, n))
        if buf is None:
            buf = self._buffers[(B, n)] = (per_frame_workspace(B, n, self.device),
                                           torch.empty((B, N_SUMS), dtype=torch.float64, device=self.device))
        return buf

    def update(self, pred, target):
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("FrameAverageMeter.update: tensors must live on a ROCm device (no CPU implementation here)")
        if pred.shape[-2:] != target.shape[-2:]:
            if pred.dim() == 3:
                pred = pred.unsqueeze(1)
            pred = torch.nn.functional.interpolate(pred, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=True)
            if target.dim() == 3:
                pred = pred[:, 0]
        p, t, B, n, dt = _frames(pred, target, "FrameAverageMeter.update")
        if self.device.index is None:       # built for "cuda": the device of the first batch
            self.device = p.device
        if p.device != self.device:
            raise RuntimeError("FrameAverageMeter on %s fed tensors on %s" % (self.device, p.device))
        work, sums = self._buf(B, n)
        _per_frame_launch(p, t, dt, B, n, work, sums)
        return self.update_from_sums(sums)

    def update_from_sums(self, sums):
        """Add frames already reduced to their ten sums (float64 [B, 10] on this meter's device, e.g. metric_sums_per_frame)."""
        if not sums.is_cuda or sums.device != self.device or sums.dtype != torch.float64 or sums.dim() != 2 \
                or sums.shape[1] != N_SUMS or not sums.is_contiguous():
            raise ValueError("sums must be a contiguous float64 [B, 10] tensor on %s" % (self.device,))
        launch(self.device, "cspn_meter_update", sums.data_ptr(), int(sums.shape[0]), self.meter.data_ptr())
        return self

    def state(self):
        """The 12 doubles on the device: sum over frames of the ten metrics, frames, valid pixels (no synchronisation)."""
        return self.meter

    def average(self):
        _F.ensure_resident_ok(self.device)
        return average_from_state(self.meter.cpu())


def all_gather_frame_meter(state, group=None):
    """Multi-GPU form of the per-frame protocol (batch shards per rank): one all-gather of every rank's 12
    doubles (FrameAverageMeter.state()), added.  Sums of per-frame metrics and frame counts are additive, so
    average_from_state(total) is the average over all frames of all ranks for any shard sizes.  Works over gloo (host tensors;
    device tensors go through host memory) and nccl / RCCL; without a process group the local state is returned (a copy)."""
    if state.dim() != 1 or state.shape[0] != N_METER or state.dtype != torch.float64:
        raise ValueError("state must be the float64 [12] tensor of FrameAverageMeter.state()")
    if state.is_cuda:
        _F.ensure_resident_ok(state.device)
    if not (dist.is_available() and dist.is_initialized()):
        return state.clone()
    src = state.contiguous()
    if state.is_cuda and dist.get_backend(group) == "gloo":
        src = src.cpu()
    parts = [torch.empty_like(src) for _ in range(dist.get_world_size(group))]
    dist.all_gather(parts, src, group=group)
    return torch.stack(parts, 0).sum(0).to(state.device)

"""The reference's sparse-depth sampler on the device — the drop-in for `dataloaders.nyu_dataloader.dense_to_sparse`:

    from cspn_monodepth_amd.dataloaders.nyu_dataloader.dense_to_sparse import UniformSampling, create_rgbd

`UniformSampling(num_samples, max_depth)` is the reference's "uar" sparsifier (dense_to_sparse.py:27-52) for a BATCH that already
sits on the GPU, with the reference's per-frame semantics: frame b keeps `depth > 0 [and depth <= max_depth]`, counts its own
n_keep, and samples a kept pixel where `u < num_samples / n_keep` (fp64).  `create_sparse_depth` / `create_rgbd` are
MyDataloader's methods of those names (dataloader.py:85-97) as module-level functions that take the sparsifier first.

The reference samples in a loader worker, per frame, with numpy's global generator.  Here a call is the two launches of
include/cspn_sparsify.h on the current stream — a count pass and an apply pass that writes the sparse plane straight into channel
3 of the [B,4,H,W] input and copies the RGB planes next to it — with no atomics, no host synchronisation and nothing read back, so
a training or evaluation step can draw a fresh sample inside a `torch.cuda.graph` capture.

Where `u` comes from:
  * `uniform=` a [B,1,H,W] fp32 or fp64 tensor: the caller's numbers (torch's generator, or the plane a reference run consumed —
    the outputs then equal the reference's bit for bit);
  * otherwise Philox4x32-10 in the kernel, counter (pixel index, 0, frame id low, frame id high), key `seed`: the mask of a frame
    depends on (seed, frame id, depth) only, not on the batch the frame sits in.  `frame_ids` is a device int64 [B] tensor
    (default: 0 .. B-1); a captured loop advances it on the device (`frame_ids += B`) between replays.

fp32 depth on a ROCm device only; there is no CPU implementation here and no fallback to one."""
import numpy as np
import torch

from ... import _lib
from ..._host import _p, launch


def _check_plane(name, t, B, H, W, channels, dtypes):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype not in dtypes:
        raise TypeError("%s: dtype %s is not supported (%s)" % (name, t.dtype, ", ".join(str(d) for d in dtypes)))
    if tuple(t.shape) != (B, channels, H, W):
        raise ValueError("%s must have the shape %s, got %s" % (name, (B, channels, H, W), tuple(t.shape)))


def _check(depth, rgb, uniform, frame_ids, seed):
    """Every argument rule, dtype before shape before device (so that each can be met on its own).  -> (B, H, W)"""
    if not isinstance(depth, torch.Tensor):
        raise TypeError("depth must be a torch.Tensor, got %s" % type(depth).__name__)
    if depth.dtype != torch.float32:
        raise TypeError("depth: fp32 only, got %s — a sparse sample is a copy of the measured depth; cast with .float() first" % (depth.dtype,))
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError("depth must be [B,1,H,W], got %s" % (tuple(depth.shape),))
    B, _, H, W = depth.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("depth: empty tensor %s" % (tuple(depth.shape),))
    if B > 65535:
        raise ValueError("depth: at most 65535 frames per call, got %d" % B)
    if rgb is not None:
        _check_plane("rgb", rgb, B, H, W, 3, (torch.float32, torch.uint8))
    if uniform is not None:
        _check_plane("uniform", uniform, B, H, W, 1, (torch.float32, torch.float64))
    if frame_ids is not None:
        if not isinstance(frame_ids, torch.Tensor):
            raise TypeError("frame_ids must be a device int64 tensor, got %s" % type(frame_ids).__name__)
        if frame_ids.dtype != torch.int64:
            raise TypeError("frame_ids: int64 only, got %s" % (frame_ids.dtype,))
        if tuple(frame_ids.shape) != (B,):
            raise ValueError("frame_ids must have the shape (%d,), got %s" % (B, tuple(frame_ids.shape)))
    if not isinstance(seed, int) or isinstance(seed, bool):
        raise TypeError("seed must be an int, got %s" % type(seed).__name__)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64), got %d" % seed)
    for name, t in (("depth", depth), ("rgb", rgb), ("uniform", uniform), ("frame_ids", frame_ids)):
        if t is not None and not t.is_cuda:
            raise RuntimeError("%s must live on a ROCm device (no CPU implementation here)" % name)
        if t is not None and t.device != depth.device:
            raise ValueError("%s is on %s, depth on %s" % (name, t.device, depth.device))
    return B, H, W


def _launch(sparsifier, depth, rgb, uniform, frame_ids, seed, want_mask=False, want_rgbd=False):
    """One cspn_sparsify call.  -> (sparse or None, rgbd or None, mask or None)"""
    if sparsifier is not None and (sparsifier.num_samples != int(sparsifier.num_samples) or abs(int(sparsifier.num_samples)) >= 1 << 63):
        raise ValueError("num_samples must be a whole number that fits 64 bits, got %r" % (sparsifier.num_samples,))
    B, H, W = _check(depth, rgb, uniform, frame_ids, seed)
    dev, HW = depth.device, H * W
    depth = depth.detach().contiguous()
    L = _lib.lib()
    dense = sparsifier is None
    kind, u_ptr, ids_ptr = _lib.UNIFORM_PHILOX, None, None
    if not dense:
        if uniform is not None:
            uniform = uniform.detach().contiguous()
            kind, u_ptr = (_lib.UNIFORM_F32 if uniform.dtype == torch.float32 else _lib.UNIFORM_F64), uniform.data_ptr()
        else:
            if frame_ids is None:
                frame_ids = torch.arange(B, dtype=torch.int64, device=dev)
            frame_ids = frame_ids.contiguous()
            ids_ptr = frame_ids.data_ptr()
    rgb_kind, rgb_ptr, rgb_out_ptr, rgbd, mask, sparse = _lib.RGB_NONE, None, None, None, None, None
    if want_rgbd:
        rgb = rgb.detach().contiguous()
        rgb_kind, rgb_ptr = (_lib.RGB_F32 if rgb.dtype == torch.float32 else _lib.RGB_U8), rgb.data_ptr()
        rgbd = torch.empty((B, 4, H, W), dtype=torch.float32, device=dev)
        sparse = rgbd[:, 3:4]
        rgb_out_ptr = rgbd.data_ptr()
        sparse_bs = 4 * HW
    elif not want_mask:
        sparse = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        sparse_bs = HW
    else:
        sparse_bs = HW
    if want_mask:
        mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
    work = None
    if not dense:
        work = torch.empty((L.cspn_sparsify_workspace_bytes(B, HW) // 4,), dtype=torch.int32, device=dev)
    launch(dev, "cspn_sparsify", depth.data_ptr(), _lib.CSPN_F32, B, H, W, _lib.SPARSIFY_DENSE if dense else _lib.SPARSIFY_UAR,
           0 if dense else int(sparsifier.num_samples), float("inf") if dense else float(np.float32(sparsifier.max_depth)),
           u_ptr, kind, ids_ptr, seed, _p(sparse), sparse_bs, rgb_ptr, rgb_kind, rgb_out_ptr, 4 * HW, HW, _p(mask), _p(work))
    return sparse, rgbd, None if mask is None else mask.view(torch.bool)


class DenseToSparse:
    """The base of the sparsifiers, as in the reference: `name`, `dense_to_sparse(rgb, depth, ...)` -> bool mask, `__repr__`."""
    name = None

    def dense_to_sparse(self, rgb, depth, uniform=None, frame_ids=None, seed=0):
        raise NotImplementedError("%s has no dense_to_sparse" % type(self).__name__)


class UniformSampling(DenseToSparse):
    name = "uar"

    def __init__(self, num_samples, max_depth=np.inf):
        self.num_samples = num_samples
        self.max_depth = max_depth

    def __repr__(self):
        return "%s{ns=%d,md=%f}" % (self.name, self.num_samples, self.max_depth)

    def dense_to_sparse(self, rgb, depth, uniform=None, frame_ids=None, seed=0):
        """The bool mask [B,1,H,W] of the sampled pixels of depth [B,1,H,W] (fp32, on the device): per frame, a pixel with
        `depth > 0 [and depth <= max_depth]` is sampled with probability num_samples / n_keep of its frame.  `rgb` is not read (the
        reference's does not read it either) and may be None.  max_depth is compared in fp32, as numpy compares the reference's fp32
        depth with a Python scalar."""
        return _launch(self, depth, rgb, uniform, frame_ids, seed, want_mask=True)[2]


class SimulatedStereo(DenseToSparse):
    name = "sim_stereo"

    def __init__(self, num_samples, max_depth=np.inf, dilate_kernel=3, dilate_iterations=1):
        self.num_samples = num_samples
        self.max_depth = max_depth
        self.dilate_kernel = dilate_kernel
        self.dilate_iterations = dilate_iterations

    def __repr__(self):
        return "%s{ns=%d,md=%f,dil=%d.%d}" % \
               (self.name, self.num_samples, self.max_depth, self.dilate_kernel, self.dilate_iterations)

    def dense_to_sparse(self, rgb, depth, uniform=None, frame_ids=None, seed=0):
        raise NotImplementedError(
            "SimulatedStereo.dense_to_sparse is not built: its arithmetic is OpenCV's (cv2.GaussianBlur, cv2.Sobel with ksize=5, "
            "cv2.magnitude: border handling, kernel coefficients and accumulation order are OpenCV's own), and without OpenCV no "
            "reference output exists to hold device kernels to.  Use UniformSampling (\"uar\", the reference's default).")


def create_sparse_depth(sparsifier, rgb, depth, uniform=None, frame_ids=None, seed=0):
    """MyDataloader.create_sparse_depth (dataloader.py:85-92): `depth` itself when sparsifier is None, else a new [B,1,H,W] fp32
    tensor holding depth at the sampled pixels and +0 elsewhere."""
    if sparsifier is None:
        return depth
    if not isinstance(sparsifier, UniformSampling):
        return _by_mask(sparsifier, rgb, depth, uniform, frame_ids, seed)
    return _launch(sparsifier, depth, rgb, uniform, frame_ids, seed)[0]


def create_rgbd(sparsifier, rgb, depth, uniform=None, frame_ids=None, seed=0):
    """MyDataloader.create_rgbd (dataloader.py:94-97) + ToTensor's .float(): -> (rgbd [B,4,H,W] fp32, sparse), where `sparse` is the
    view rgbd[:, 3:4] — the kernel writes the sparse plane in place, there is no `cat`.  rgb [B,3,H,W]: fp32 planes are copied bit
    for bit, uint8 planes become (float)(v / 255.0) with the division in fp64, as the reference's loader computes them.  With
    sparsifier None the dense depth goes into channel 3 unchanged."""
    if rgb is None:
        raise TypeError("create_rgbd needs rgb")
    if sparsifier is not None and not isinstance(sparsifier, UniformSampling):
        _by_mask(sparsifier, rgb, depth, uniform, frame_ids, seed)
    _, rgbd, _ = _launch(sparsifier, depth, rgb, uniform, frame_ids, seed, want_rgbd=True)
    return rgbd, rgbd[:, 3:4]


def _by_mask(sparsifier, rgb, depth, uniform, frame_ids, seed):
    """Any other sparsifier has no kernel here: its dense_to_sparse says so (SimulatedStereo raises NotImplementedError)."""
    sparsifier.dense_to_sparse(rgb, depth, uniform=uniform, frame_ids=frame_ids, seed=seed)
    raise NotImplementedError("no device kernel for the sparsifier %r" % (sparsifier,))

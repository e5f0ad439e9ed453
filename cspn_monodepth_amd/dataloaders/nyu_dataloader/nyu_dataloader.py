"""The reference's NYU train / val transforms on the device — the step in front of the sparse-depth sampler, the drop-in for
`NYUDataset.train_transform` / `val_transform` of `dataloaders.nyu_dataloader.nyu_dataloader` (nyu_dataloader.py:13-44, with
transforms.py and ColorJitter(0.4, 0.4, 0.4) of dataloader.py:54):

    from cspn_monodepth_amd.dataloaders.nyu_dataloader.nyu_dataloader import train_transform, val_transform, draw_train_params

A BATCH of raw frames that already sits on the GPU — rgb uint8 [B,3,H,W], the layout the h5 files hold and `create_rgbd` takes, and
depth fp32 [B,1,H,W] — becomes the (rgb fp32 [B,3,oh,ow], depth fp32 [B,1,oh,ow]) pair the reference's loader workers produce frame by
frame with Pillow and scipy:

    val     Resize(first) -> CenterCrop(output_size)                                              rgb / 255
    train   depth / s;  Resize(first) -> Rotate(angle) -> Resize(s) -> CenterCrop -> HorizontalFlip;  ColorJitter on rgb;  rgb / 255

The reference's geometry is nearest-neighbour throughout, so an output pixel is a copy of one raw pixel, and for the same parameters
the outputs equal the reference's bit for bit (tests/test_transforms.py, golden G22; include/cspn_transform.h says what has to be
reproduced for that).  One difference from a plain copy is the reference's own: a train frame's depth goes through scipy's order-0 sum,
which turns a -0 into +0; val copies the word.

A call is the two (val) or three (train) launches of include/cspn_transform.h on the current stream, with no atomics, no host
synchronisation and nothing read back, so the chain raw frame -> transform -> sparse sample -> RGB-D -> model can sit inside one
`torch.cuda.graph` capture and draw a fresh augmentation per replay.

Where a train frame's parameters come from:
  * `params=` a device fp64 [B,8] tensor, a row per frame: s, angle in degrees, flip (!= 0), the brightness, contrast and saturation
    factors, an order code 0..5 for the lexicographic permutations of (brightness, contrast, saturation) — -1: no jitter — and one
    reserved slot.  Precondition: finite values, int(h1 * s) >= oh and int(w1 * s) >= ow, (h1, w1) the size after the first resize.
    The parameters live on the device, so the host cannot check them: a row outside the precondition gives a meaningless frame, never
    an out-of-range access (the kernels clamp every index), and leaves the other frames alone;
  * otherwise `draw_train_params`: Philox4x32-10 in a small kernel, counter (slot, 1, frame id low, frame id high), key `seed`, with
    s = 1 + 0.5u, angle = -5 + 10u, flip = u < 0.5, each factor 0.6 + 0.8u, order = floor(6u).  These are the reference's
    DISTRIBUTIONS (np.random.uniform(1, 1.5), (-5, 5), (0, 1) < 0.5, (0.6, 1.4), a shuffle), not numpy's stream: a seed here does not
    reproduce a numpy seed.  A row depends on (seed, frame id) only.  `frame_ids` is a device int64 [B] tensor (default 0 .. B-1) as
    in dense_to_sparse; a captured loop advances it on the device between replays.

`out=(rgb_out, depth_out)` writes into the caller's fp32 tensors of the output shapes; each [oh,ow] plane must be contiguous, batch and
channel strides are free, so rgb_out can be channels 0..2 of a [B,4,oh,ow] buffer.

The defaults are the reference's geometry: raw 480 x 640, first = 250/480 (train) or 240/480 (val), output (228, 304); `first=` and
`output_size=` override them for any raw size.  ROCm device only; there is no CPU implementation here and no fallback to one."""
import ctypes

import torch

from ... import _lib
from ..._host import _p, launch

iheight, iwidth = 480, 640      # raw image size (nyu_dataloader.py:5)
OUTPUT_SIZE = (228, 304)        # nyu_dataloader.py:11
TRAIN_FIRST = 250.0 / iheight   # nyu_dataloader.py:21
VAL_FIRST = 240.0 / iheight     # nyu_dataloader.py:37


def _check_seed(seed):
    if not isinstance(seed, int) or isinstance(seed, bool):
        raise TypeError("seed must be an int, got %s" % type(seed).__name__)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must be in [0, 2^64), got %d" % seed)


def _check_ids(frame_ids, B):
    if not isinstance(frame_ids, torch.Tensor):
        raise TypeError("frame_ids must be a device int64 tensor, got %s" % type(frame_ids).__name__)
    if frame_ids.dtype != torch.int64:
        raise TypeError("frame_ids: int64 only, got %s" % (frame_ids.dtype,))
    if tuple(frame_ids.shape) != (B,):
        raise ValueError("frame_ids must have the shape (%d,), got %s" % (B, tuple(frame_ids.shape)))


def _check(rgb, depth, params, frame_ids, seed, out, first, output_size, train):
    """Every argument rule, dtype before shape before device (so that each can be met on its own).  -> (B, H, W, oh, ow)"""
    if not isinstance(rgb, torch.Tensor):
        raise TypeError("rgb must be a torch.Tensor, got %s" % type(rgb).__name__)
    if rgb.dtype != torch.uint8:
        raise TypeError("rgb: uint8 only, got %s — the transform works on the raw frame the h5 file holds" % (rgb.dtype,))
    if not isinstance(depth, torch.Tensor):
        raise TypeError("depth must be a torch.Tensor, got %s" % type(depth).__name__)
    if depth.dtype != torch.float32:
        raise TypeError("depth: fp32 only, got %s — an output depth is a copy of the measured depth; cast with .float() first" % (depth.dtype,))
    if params is not None:
        if not isinstance(params, torch.Tensor):
            raise TypeError("params must be a device fp64 tensor, got %s" % type(params).__name__)
        if params.dtype != torch.float64:
            raise TypeError("params: fp64 only, got %s" % (params.dtype,))
        if frame_ids is not None:
            raise TypeError("give params or frame_ids, not both: frame_ids only feed the draw")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(isinstance(t, torch.Tensor) for t in out):
            raise TypeError("out must be a pair (rgb_out, depth_out) of tensors")
        for name, t in zip(("out[0]", "out[1]"), out):
            if t.dtype != torch.float32:
                raise TypeError("%s: fp32 only, got %s" % (name, t.dtype))
    if isinstance(first, bool) or not isinstance(first, (int, float)):
        raise TypeError("first must be a float, got %s" % type(first).__name__)
    if (not isinstance(output_size, (tuple, list)) or len(output_size) != 2
            or not all(isinstance(v, int) and not isinstance(v, bool) for v in output_size)):
        raise TypeError("output_size must be a pair of ints (oh, ow), got %r" % (output_size,))
    if train:
        _check_seed(seed)

    if rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError("rgb must be [B,3,H,W], got %s" % (tuple(rgb.shape),))
    B, _, H, W = rgb.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("rgb: empty tensor %s" % (tuple(rgb.shape),))
    if B > 65535:
        raise ValueError("rgb: at most 65535 frames per call, got %d" % B)
    if H * W >= 1 << 31:
        raise ValueError("rgb: H * W must be below 2^31, got %d x %d" % (H, W))
    if tuple(depth.shape) != (B, 1, H, W):
        raise ValueError("depth must have the shape %s, got %s" % ((B, 1, H, W), tuple(depth.shape)))
    oh, ow = output_size
    if oh < 1 or ow < 1 or oh * ow >= 1 << 31:
        raise ValueError("output_size must be positive and oh * ow below 2^31, got %r" % (output_size,))
    h1, w1 = ctypes.c_int(0), ctypes.c_int(0)
    if not first > 0 or not _lib.lib().cspn_transform_first_size(H, W, float(first), ctypes.byref(h1), ctypes.byref(w1)):
        raise ValueError("first = %r leaves nothing of a %d x %d frame" % (first, H, W))
    h1, w1 = h1.value, w1.value
    if not train and (oh > h1 or ow > w1):
        raise ValueError("output_size %r is larger than the resized frame %r" % (tuple(output_size), (h1, w1)))
    if params is not None and tuple(params.shape) != (B, _lib.TRANSFORM_PARAMS):
        raise ValueError("params must have the shape %s, got %s" % ((B, _lib.TRANSFORM_PARAMS), tuple(params.shape)))
    if frame_ids is not None:
        _check_ids(frame_ids, B)
    if out is not None:
        for name, t, c in (("out[0]", out[0], 3), ("out[1]", out[1], 1)):
            if tuple(t.shape) != (B, c, oh, ow):
                raise ValueError("%s must have the shape %s, got %s" % (name, (B, c, oh, ow), tuple(t.shape)))
            if t.stride(3) != 1 or t.stride(2) != ow or (c > 1 and t.stride(1) < oh * ow) or (B > 1 and t.stride(0) < oh * ow):
                raise ValueError("%s: every [oh,ow] plane must be contiguous and planes must not overlap, got strides %s" % (name, t.stride()))

    named = [("rgb", rgb), ("depth", depth), ("params", params), ("frame_ids", frame_ids)]
    if out is not None:
        named += [("out[0]", out[0]), ("out[1]", out[1])]
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise RuntimeError("%s must live on a ROCm device (no CPU implementation here)" % name)
        if t is not None and t.device != rgb.device:
            raise ValueError("%s is on %s, rgb on %s" % (name, t.device, rgb.device))
    return B, H, W, oh, ow


def _launch(rgb, depth, params, out, first, output_size, mode):
    B, _, H, W = rgb.shape
    oh, ow = output_size
    dev = rgb.device
    L = _lib.lib()
    rgb, depth = rgb.detach().contiguous(), depth.detach().contiguous()
    if params is not None:
        params = params.detach().contiguous()
    if out is None:
        rgb_out = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=dev)
        depth_out = torch.empty((B, 1, oh, ow), dtype=torch.float32, device=dev)
    else:
        rgb_out, depth_out = out
    nbytes = L.cspn_transform_workspace_bytes(mode, B, H, W, float(first), oh, ow)
    work = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
    launch(dev, "cspn_transform", rgb.data_ptr(), depth.data_ptr(), B, H, W, float(first), oh, ow, mode, _p(params), rgb_out.data_ptr(),
           rgb_out.stride(0), rgb_out.stride(1), depth_out.data_ptr(), depth_out.stride(0), work.data_ptr())
    return rgb_out, depth_out


def draw_train_params(B, frame_ids=None, seed=0, device=None):
    """The parameter rows of B train frames, a device fp64 [B,8] tensor: s = 1 + 0.5u, angle = -5 + 10u, flip = u < 0.5, the three
    factors 0.6 + 0.8u, the order code floor(6u), 0 — u from Philox4x32-10 on the counter (slot, 1, frame id low, frame id high) with
    the key `seed`, u = (x0 >> 8) * 2^-24.  The reference's distributions, not numpy's stream.  frame_ids: device int64 [B] (default
    0 .. B-1 on `device`, default the current ROCm device)."""
    if not isinstance(B, int) or isinstance(B, bool):
        raise TypeError("B must be an int, got %s" % type(B).__name__)
    if not 1 <= B <= 65535:
        raise ValueError("B must be in [1, 65535], got %d" % B)
    _check_seed(seed)
    if frame_ids is not None:
        _check_ids(frame_ids, B)
        if not frame_ids.is_cuda:
            raise RuntimeError("frame_ids must live on a ROCm device (no CPU implementation here)")
        if device is not None and torch.device(device).type == "cuda" and torch.device(device).index not in (None, frame_ids.device.index):
            raise ValueError("frame_ids is on %s, device is %s" % (frame_ids.device, device))
        dev = frame_ids.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("device must be a ROCm device (no CPU implementation here), got %s" % dev)
        frame_ids = torch.arange(B, dtype=torch.int64, device=dev)
    frame_ids = frame_ids.contiguous()
    dev = frame_ids.device                  # a tensor's device has an index; a caller's "cuda" has none
    params = torch.empty((B, _lib.TRANSFORM_PARAMS), dtype=torch.float64, device=dev)
    launch(dev, "cspn_transform_draw_params", frame_ids.data_ptr(), B, seed, params.data_ptr())
    return params


def val_transform(rgb, depth, out=None, first=VAL_FIRST, output_size=OUTPUT_SIZE):
    """NYUDataset.val_transform (nyu_dataloader.py:34-44) + ToTensor for rgb uint8 [B,3,H,W] and depth fp32 [B,1,H,W] on the device
    -> (rgb fp32 [B,3,oh,ow] = (float)(v / 255.0), depth fp32 [B,1,oh,ow], every word a copy)."""
    _check(rgb, depth, None, None, 0, out, first, output_size, train=False)
    return _launch(rgb, depth, None, out, first, output_size, _lib.TRANSFORM_VAL)


def train_transform(rgb, depth, params=None, frame_ids=None, seed=0, out=None, first=TRAIN_FIRST, output_size=OUTPUT_SIZE):
    """NYUDataset.train_transform (nyu_dataloader.py:13-32) + ToTensor for rgb uint8 [B,3,H,W] and depth fp32 [B,1,H,W] on the device
    -> (rgb fp32 [B,3,oh,ow], depth fp32 [B,1,oh,ow]).  `params`: the frames' rows (see the module text); None: drawn by
    draw_train_params(B, frame_ids, seed)."""
    B = _check(rgb, depth, params, frame_ids, seed, out, first, output_size, train=True)[0]
    if params is None:
        params = draw_train_params(B, frame_ids, seed, device=rgb.device)
    return _launch(rgb, depth, params, out, first, output_size, _lib.TRANSFORM_TRAIN)

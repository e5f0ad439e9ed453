"""Zero-insertion un-pooling of the UNet decoders on the HIP engine (cspn_unpool2d in include/cspn_hip.h).

``MyBlock`` mirrors network/unet_ours.py:131-157 (constructor ``(oheight=0, owidth=0)``, method
``_up_pooling(x, scale)``), so the decoder blocks that subclass it (UpProj_Block, Simple_Gudi_UpConv_Block, ...,
unet_ours.py:160-250) and the five copies of ``_up_pooling`` in network/unet_cspn_nyu.py:138-284 can take it unchanged:

    y[n, c, s*h, s*w] = x[n, c, h, w], zero elsewhere, cropped to (oheight, owidth)

The reference builds this with a grouped conv_transpose2d against a freshly allocated one-hot weight
(unet_ours.py:141-145) or with nearest upsampling times a checkerboard mask filled by an O(H*W) Python double loop
(unet_cspn_nyu.py:208-212, ~17 k iterations at the last decoder stage).  Here it is one streaming
kernel that also writes the zeros, and a strided-gather backward.

Non-finite inputs behave as in the reference (the inserted positions are ``x * 0``, so NaN/inf fill their s x s block);
the backward is a plain strided gather and ignores non-finite gradients at the dropped positions.

Loud difference: ``oheight == 0`` or ``owidth == 0`` (the constructor defaults) raise — the reference returns an
empty tensor (unet_ours.py:147-148) or an all-zero one (the mask loop never runs, unet_cspn_nyu.py:209) there.

``up_pooling_conv3x3`` is the un-pooling by 2 fused with the bias-free 3x3 convolutions that follow it in the two output heads
(``Simple_Gudi_UpConv_Block_Last_Layer``, unet_ours.py:194-202): the un-pooled map is never written (include/cspn_heads.h).  It is
opt-in — ``fused_heads=True`` of the models — and differs from the two-block path in one stated way, see its docstring.
"""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import Function, once_differentiable

from .. import _lib
from .._host import _dt, _p, _require_device, launch

__all__ = ["up_pooling", "up_pooling_conv3x3", "MyBlock"]


def _forward(x, scale, oh, ow):
    dev = _require_device(x)
    N, C, H, W = x.shape
    xc = x.contiguous()
    out = torch.empty((N, C, oh, ow), dtype=x.dtype, device=dev)
    launch(dev, "cspn_unpool2d", _p(xc), _p(out), _dt(xc), N * C, H, W, scale, oh, ow)
    return out


class _UpPooling(Function):
    @staticmethod
    def forward(ctx, x, scale, oh, ow):
        ctx.geom = (tuple(x.shape), scale, oh, ow)
        return _forward(x, scale, oh, ow)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (N, C, H, W), scale, oh, ow = ctx.geom
        dev = _require_device(grad_out)
        go = grad_out.contiguous()
        gx = torch.empty((N, C, H, W), dtype=go.dtype, device=dev)
        launch(dev, "cspn_unpool2d_backward", _p(go), _p(gx), _dt(go), N * C, H, W, scale, oh, ow)
        return gx, None, None, None


def up_pooling(x, scale, oheight, owidth):
    """[N,C,H,W] -> [N,C,oheight,owidth] (unet_ours.py:138-150)."""
    if x.dim() != 4:
        raise ValueError("up_pooling: x must be [N,C,H,W], got %s" % (tuple(x.shape),))
    scale, oheight, owidth = int(scale), int(oheight), int(owidth)
    H, W = x.shape[-2:]
    if not (1 <= oheight <= scale * H and 1 <= owidth <= scale * W):
        raise ValueError("up_pooling: output %dx%d must lie within [1, %d] x [1, %d] (scale %d of a %dx%d input); the "
                         "reference's oheight/owidth = 0 defaults give an empty or all-zero tensor and are not supported"
                         % (oheight, owidth, scale * H, scale * W, scale, H, W))
    if torch.is_grad_enabled() and x.requires_grad:
        return _UpPooling.apply(x, scale, oheight, owidth)
    return _forward(x, scale, oheight, owidth)


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _channels(tensors):
    return (ctypes.c_int * len(tensors))(*[t.shape[0] for t in tensors])


def _heads_work(which, weights, x, oh, ow):
    nbytes = _lib.lib().cspn_heads_workspace_bytes(which, sum(w.shape[0] for w in weights), *x.shape, oh, ow)
    if not nbytes:
        raise RuntimeError("cspn_heads_workspace_bytes: no workspace for x %s -> %dx%d" % (tuple(x.shape), oh, ow))
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device)


def _heads_forward(x, weights, oh, ow):
    """x, weights: contiguous fp32 on one device."""
    dev = x.device
    N, C, H, W = x.shape
    outs = tuple(torch.empty((N, w.shape[0], oh, ow), dtype=x.dtype, device=dev) for w in weights)
    work = _heads_work(_lib.HEADS_FORWARD, weights, x, oh, ow)
    launch(dev, "cspn_heads_forward", _p(x), _ptrs(weights), _ptrs(outs), _channels(weights), len(weights), _p(work), N, C, H, W, oh, ow)
    return outs


class _UpPoolingConv3x3(Function):
    @staticmethod
    def forward(ctx, x, oh, ow, *weights):
        xc, wc = x.contiguous(), tuple(w.contiguous() for w in weights)
        ctx.geom = (oh, ow)
        ctx.set_materialize_grads(False)                  # an output nobody used arrives as None and costs nothing
        ctx.save_for_backward(xc, *wc)
        return _heads_forward(xc, wc, oh, ow)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grad_outs):
        x, weights = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        oh, ow = ctx.geom
        dev = x.device
        N, C, H, W = x.shape
        live = [h for h, g in enumerate(grad_outs) if g is not None]
        gys = {h: grad_outs[h].contiguous() for h in live}
        gx = None
        if ctx.needs_input_grad[0]:
            if live:
                gx, ws = torch.empty_like(x), [weights[h] for h in live]
                work = _heads_work(_lib.HEADS_BACKWARD_INPUT, ws, x, oh, ow)
                launch(dev, "cspn_heads_backward_input", _ptrs([gys[h] for h in live]), _ptrs(ws), _channels(ws), len(live), _p(gx),
                       _p(work), N, C, H, W, oh, ow)
            else:
                gx = torch.zeros_like(x)
        gws = [None] * len(weights)
        want = [h for h in live if ctx.needs_input_grad[3 + h]]
        for h in range(len(weights)):
            if ctx.needs_input_grad[3 + h]:
                gws[h] = torch.empty_like(weights[h]) if h in want else torch.zeros_like(weights[h])
        if want:
            work = _heads_work(_lib.HEADS_BACKWARD_WEIGHTS, [weights[h] for h in want], x, oh, ow)
            launch(dev, "cspn_heads_backward_weights", _p(x), _ptrs([gys[h] for h in want]), _ptrs([gws[h] for h in want]),
                   _channels([weights[h] for h in want]), len(want), _p(work), N, C, H, W, oh, ow)
        return (gx, None, None) + tuple(gws)


def up_pooling_conv3x3(x, weights, oheight, owidth):
    """Un-pooling by 2 to (oheight, owidth) and the bias-free 3x3 convolutions (padding 1) of several heads over it, in one kernel:

        x [N,C,H,W], weights (w_0 [O_0,C,3,3], ...)  ->  (y_0 [N,O_0,oheight,owidth], ...)
        y_h == conv2d(up_pooling(x, 2, oheight, owidth), w_h, padding=1)

    as ``Simple_Gudi_UpConv_Block_Last_Layer`` computes it per head (unet_ours.py:194-202), without the un-pooled map: an output
    pixel reads the 1, 2, 2 or 4 pixels of ``x`` its window covers (include/cspn_heads.h).  fp32 on a ROCm device; at most 4 heads
    with at most 16 output channels together; 1 <= oheight <= 2H, 1 <= owidth <= 2W as ``up_pooling`` at scale 2.  One autograd
    node with gradients to ``x`` (one gather over all heads) and to every weight (split-K with a fixed summation order: the same bits
    run after run); each is computed only if it is asked for, an output without a gradient counts as zero, and nothing is saved
    under ``no_grad``.  A non-contiguous ``x`` or weight view (``w[:8]``) is made contiguous.

    One difference from the two-block path: a NaN or Inf in ``x[n,c,i,j]`` reaches only the outputs whose 3x3 window covers
    (2i, 2j).  The reference's un-pooling holds ``x * 0`` at the inserted positions (see above), so there it also reaches the
    windows that cover the other three positions of the 2 x 2 block."""
    if not isinstance(weights, (tuple, list)):
        raise ValueError("up_pooling_conv3x3: weights must be a tuple of [O,C,3,3] tensors")
    weights = tuple(weights)
    if x.dim() != 4:
        raise ValueError("up_pooling_conv3x3: x must be [N,C,H,W], got %s" % (tuple(x.shape),))
    if not 1 <= len(weights) <= _lib.HEADS_MAX_HEADS:
        raise ValueError("up_pooling_conv3x3: between 1 and %d heads, got %d" % (_lib.HEADS_MAX_HEADS, len(weights)))
    N, C, H, W = x.shape
    for h, w in enumerate(weights):
        if w.dim() != 4 or w.shape[0] < 1 or tuple(w.shape[1:]) != (C, 3, 3):
            raise ValueError("up_pooling_conv3x3: weight %d must be [O,%d,3,3], got %s" % (h, C, tuple(w.shape)))
    total = sum(w.shape[0] for w in weights)
    if total > _lib.HEADS_MAX_OUT_CHANNELS:
        raise ValueError("up_pooling_conv3x3: %d output channels over all heads, at most %d" % (total, _lib.HEADS_MAX_OUT_CHANNELS))
    for t in (x,) + weights:
        if t.dtype != torch.float32:
            raise ValueError("up_pooling_conv3x3: fp32 only, got %s" % t.dtype)
    oheight, owidth = int(oheight), int(owidth)
    if not (1 <= oheight <= 2 * H and 1 <= owidth <= 2 * W):
        raise ValueError("up_pooling_conv3x3: output %dx%d must lie within [1, %d] x [1, %d] (scale 2 of a %dx%d input)"
                         % (oheight, owidth, 2 * H, 2 * W, H, W))
    if N < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError("up_pooling_conv3x3: empty input %s" % (tuple(x.shape),))
    _require_device(x, *weights)
    if torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in weights)):
        return _UpPoolingConv3x3.apply(x, oheight, owidth, *weights)
    return _heads_forward(x.contiguous(), tuple(w.contiguous() for w in weights), oheight, owidth)


class MyBlock(nn.Module):
    """network/unet_ours.py:131-157: base of the decoder blocks; holds the target size of the un-pooled map."""

    def __init__(self, oheight=0, owidth=0):
        super(MyBlock, self).__init__()
        self.oheight = oheight
        self.owidth = owidth

    def _up_pooling(self, x, scale):
        return up_pooling(x, scale, self.oheight, self.owidth)

    def init_weights(self):                               # unet_ours.py:152-157
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(m.weight.data)
                if m.bias is not None:
                    nn.init.constant_(m.bias.data, 0)

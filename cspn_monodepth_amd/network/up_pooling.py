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
``up_pooling_conv3x3_half`` is its forward for a half ``x`` (``torch.autocast``, ``model.half()``) on the fp16 matrix cores
(include/cspn_head16.h), and ``fused_heads_forward`` is how the models choose between the two and the stock blocks.

``up_pooling_conv5x5`` is the same for the head of a decoder block (``Gudi_UpProj_Block``, ``Gudi_UpProj_Block_Cat``, ``UpProj_Block``,
``Simple_Gudi_UpConv_Block``, unet_ours.py:160-248): un-pooling by 2, the one or two bias-free 5x5 convolutions over it, their batch
norms in eval mode and the ReLU of the first, as one implicit GEMM per output phase on the fp32 matrix cores
(include/cspn_upconv.h).  Forward only and opt-in — ``fused_decoder`` of the models; the filters are reordered once by
``pack_upconv5x5``.  A half ``x`` (``torch.autocast``, ``model.half()``) takes a pack of ``dtype=torch.float16`` and runs on the fp16
matrix cores with fp32 accumulation and one rounding of the result (include/cspn_uphalf.h).  ``precision="bf16x3"`` — the models'
``fused_decoder_precision`` — keeps fp32 tensors and the fp32 pack and runs the products on the bf16 matrix cores, every operand split
into three bf16 terms: fp32-class, other bits, measured slower than the exact path and so selected by nothing but the keyword.

``conv3x3_bn_act`` is the rest of such a block — the 3x3 convolutions ``conv1_1`` (over the head's output and the encoder skip, without
the ``cat``) and ``conv2``, their eval-mode batch norms, the shortcut add and the ReLUs — one call per convolution on the same matrix
cores (include/cspn_uptail.h).  Forward only and opt-in — ``fused_tail`` of the models; ``pack_conv3x3`` makes its pack.
"""
import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import Function, once_differentiable

from .. import _lib
from .._host import _dt, _p, _require_device, launch

__all__ = ["up_pooling", "up_pooling_conv3x3", "up_pooling_conv3x3_half", "fused_heads_forward", "up_pooling_conv5x5", "pack_upconv5x5", "UpconvPack", "pack_conv3x3", "conv3x3_bn_act", "MyBlock"]
_UPCONV_KERNELS = {torch.float32: ("cspn_upconv_workspace_bytes", "cspn_upconv_pack", "cspn_upconv_forward", True, 4),      # by pack dtype: bytes, pack, forward,
                   torch.float16: ("cspn_uphalf_packed_bytes", "cspn_uphalf_pack", "cspn_uphalf_forward", False, 2)}       # forward takes a dtype, element size

_DT = {torch.float32: _lib.CSPN_F32, torch.float16: _lib.CSPN_F16}


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


def up_pooling_conv3x3_half(x, weights, oheight, owidth):
    """``up_pooling_conv3x3`` for a half ``x``, forward only, on the fp16 matrix cores (include/cspn_head16.h):

        x [N,C,H,W] fp16, weights (w_0 [O_0,C,3,3], ...)  ->  (y_0 [N,O_0,oheight,owidth], ...) fp16
        y_h == conv2d(up_pooling(x, 2, oheight, owidth), w_h, padding=1)

    without the un-pooled map.  The weights are all fp32 (autocast: rounded to fp16 once, to nearest even) or all fp16
    (``model.half()``: taken as they are); fp16 products accumulated in fp32, one rounding of the result to fp16, beyond the fp16
    range +-Inf.  At most 4 heads with at most 16 output channels together; 1 <= oheight <= 2H, 1 <= owidth <= 2W; every tensor
    below 2^31 elements.  Every output element is one fixed chain (the header says which), so a frame's bits do not depend on the
    batch, runs repeat, and the call can be captured in a graph.  Non-contiguous inputs are made contiguous.

    Forward only.  With grad mode on and ``x`` or a weight requiring a gradient it raises: training runs the stock blocks
    (``up_pooling`` and the 3x3 convolutions, as the models do by default).

    The difference from the two-block path is ``up_pooling_conv3x3``'s: a NaN or Inf in ``x[n,c,i,j]`` reaches only the outputs whose
    3x3 window covers (2i, 2j)."""
    who = "up_pooling_conv3x3_half"
    if not isinstance(weights, (tuple, list)):
        raise ValueError("%s: weights must be a tuple of [O,C,3,3] tensors" % who)
    weights = tuple(weights)
    if x.dim() != 4:
        raise ValueError("%s: x must be [N,C,H,W], got %s" % (who, tuple(x.shape)))
    if not 1 <= len(weights) <= _lib.HEAD16_MAX_HEADS:
        raise ValueError("%s: between 1 and %d heads, got %d" % (who, _lib.HEAD16_MAX_HEADS, len(weights)))
    N, C, H, W = x.shape
    for h, w in enumerate(weights):
        if w.dim() != 4 or w.shape[0] < 1 or tuple(w.shape[1:]) != (C, 3, 3):
            raise ValueError("%s: weight %d must be [O,%d,3,3], got %s" % (who, h, C, tuple(w.shape)))
    total = sum(w.shape[0] for w in weights)
    if total > _lib.HEAD16_MAX_OUT_CHANNELS:
        raise ValueError("%s: %d output channels over all heads, at most %d" % (who, total, _lib.HEAD16_MAX_OUT_CHANNELS))
    if x.dtype != torch.float16:
        raise ValueError("%s: x must be fp16 (a fp32 x takes up_pooling_conv3x3), got %s" % (who, x.dtype))
    for w in weights:
        if w.dtype not in (torch.float32, torch.float16):
            raise ValueError("%s: the weights are fp32 or fp16, got %s" % (who, w.dtype))
        if w.dtype != weights[0].dtype:
            raise ValueError("%s: the weights of one call have one dtype, got %s and %s" % (who, weights[0].dtype, w.dtype))
    oheight, owidth = int(oheight), int(owidth)
    if not (1 <= oheight <= 2 * H and 1 <= owidth <= 2 * W):
        raise ValueError("%s: output %dx%d must lie within [1, %d] x [1, %d] (scale 2 of a %dx%d input)"
                         % (who, oheight, owidth, 2 * H, 2 * W, H, W))
    if N < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError("%s: empty input %s" % (who, tuple(x.shape)))
    if x.numel() >= 2 ** 31 or N * max(w.shape[0] for w in weights) * oheight * owidth >= 2 ** 31:
        raise ValueError("%s: a tensor of 2^31 elements or more; split the batch" % who)
    if torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in weights)):
        raise RuntimeError("%s is forward-only: with grad mode on, run the stock blocks (up_pooling and the 3x3 convolutions, the "
                           "models' default and their training path), or call it under torch.no_grad()" % who)
    dev = _require_device(x, *weights)
    xc, wc = x.contiguous(), tuple(w.detach().contiguous() for w in weights)
    nbytes = _lib.lib().cspn_head16_workspace_bytes(total, C)
    if not nbytes:
        raise RuntimeError("cspn_head16_workspace_bytes: no workspace for %d output channels over %d channels" % (total, C))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    outs = tuple(torch.empty((N, w.shape[0], oheight, owidth), dtype=torch.float16, device=dev) for w in wc)
    launch(dev, "cspn_head16_forward", _p(xc), _ptrs(wc), _dt(wc[0]), _ptrs(outs), _channels(wc), len(wc), _p(work), N, C, H, W, oheight, owidth)
    return outs


def fused_heads_forward(x, weights, oheight, owidth):
    """What the models' `fused_heads` runs on the decoder's last map: a fp16 ``x`` with no gradient needed — grad mode off, or neither
    ``x`` nor a weight requiring one — takes ``up_pooling_conv3x3_half``; everything else ``up_pooling_conv3x3`` (fp32: its
    kernels and its autograd node; any other dtype: its refusal).  None: a fp16 ``x`` that needs a gradient — the caller runs the two
    stock blocks, the training path in half."""
    if x.dtype == torch.float16:
        if torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w in weights)):
            return None
        return up_pooling_conv3x3_half(x, weights, oheight, owidth)
    return up_pooling_conv3x3(x, weights, oheight, owidth)


class UpconvPack(object):
    """What ``up_pooling_conv5x5`` runs on: the filters of one block head in the order the kernel walks them (``packed``), the folded
    batch norms (``scale``, ``shift``: fp32 [sum of out_channels], or None), how many leading flat channels get a ReLU, the ``dtype``
    of the packed filters and so of the ``x`` it takes and the outputs it gives (fp32: include/cspn_upconv.h, fp16: cspn_uphalf.h), and the
    ``_version`` and ``data_ptr`` of every tensor it was made from — ``stale()`` says whether one of them has changed since.  A pack of
    ``pack_conv3x3`` for ``conv3x3_bn_act`` is the same thing with one filter and a ``split``: how many of its ``in_channels`` come from
    the first of two maps (None: one map)."""

    def __init__(self, packed, scale, shift, out_channels, in_channels, relu_channels, sources, dtype=torch.float32, split=None):
        self.packed, self.scale, self.shift, self.dtype, self.split = packed, scale, shift, dtype, split
        self.out_channels, self.in_channels, self.relu_channels = tuple(out_channels), int(in_channels), int(relu_channels)
        self.sources = tuple(sources)
        self._seen = tuple((t._version, t.data_ptr()) for t in self.sources)

    def stale(self):
        """True once a source tensor was written in place (an optimizer step, ``load_state_dict``) or moved."""
        return any((t._version, t.data_ptr()) != seen for t, seen in zip(self.sources, self._seen))

    def made_from(self, sources):
        """Are these the very tensors the pack was made from (a parameter that was replaced, not written, is another object)?"""
        sources = tuple(sources)
        return len(sources) == len(self.sources) and all(a is b for a, b in zip(sources, self.sources))


def _check_filters(who, weights, dtype=torch.float32):
    """The filters as a tuple.  They are fp32, or — for a pack of ``dtype`` fp16 only — fp16 (the parameters of ``model.half()``)."""
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("%s: a pack is fp32 or fp16, got dtype=%s" % (who, dtype))
    if not isinstance(weights, (tuple, list)):
        raise ValueError("%s: weights must be a tuple of [O,C,5,5] tensors" % who)
    weights = tuple(weights)
    if not 1 <= len(weights) <= _lib.UPCONV_MAX_FILTERS:
        raise ValueError("%s: one or two filters, got %d" % (who, len(weights)))
    for k, w in enumerate(weights):
        if w.dim() != 4 or w.shape[0] < 1 or w.shape[1] < 1 or tuple(w.shape[2:]) != (5, 5) or w.shape[1] != weights[0].shape[1]:
            raise ValueError("%s: filter %d must be [O,%d,5,5], got %s" % (who, k, weights[0].shape[1] if weights[0].dim() == 4 else 0, tuple(w.shape)))
        if w.dtype != torch.float32 and not (dtype == torch.float16 and w.dtype == torch.float16):
            raise ValueError("%s: fp32 only (fp16 filters go into a pack of dtype=torch.float16 alone), got %s" % (who, w.dtype))
        if w.dtype != weights[0].dtype:
            raise ValueError("%s: the filters of one pack have one dtype, got %s and %s" % (who, weights[0].dtype, w.dtype))
        if w.numel() >= 2 ** 31:
            raise ValueError("%s: filter %d has 2^31 elements or more" % (who, k))
    return weights


def _bn_sources(bn):
    return [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var) if t is not None]


def _fold(bn):
    """(scale, shift) of a batch norm as eval mode applies it, in fp32 by device tensor ops; call under no_grad."""
    s = 1.0 / torch.sqrt(bn.running_var.float() + bn.eps)
    if bn.weight is not None:
        s = bn.weight.detach().float() * s
    b = -bn.running_mean.float() * s
    if bn.bias is not None:
        b = bn.bias.detach().float() + b
    return s, b


def pack_upconv5x5(weights, batchnorms=None, relu=(True, False), dtype=torch.float32):
    """The pack of one block head: ``weights`` — one or two [O_k, C, 5, 5] fp32 filters on a ROCm device (``conv1.weight``,
    ``sc_conv1.weight``) — reordered for the kernel, and ``batchnorms`` — None, or one ``nn.BatchNorm2d`` per filter —
    folded as eval mode applies them: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, by device
    tensor ops (nothing is read back).  ``relu``: per filter, whether a ReLU follows; the filters with one come first.  Made once
    per version of the weights: ``stale()`` of the result says when to make it again.

    ``dtype``: torch.float32, or torch.float16 for the half-precision kernel (include/cspn_uphalf.h) — fp32 filters are then rounded
    to fp16 once (autocast: fp32 parameters, half activations), fp16 filters (``model.half()``) are taken as they are; the batch
    norms are folded in fp32 either way.  The pack takes an ``x`` of its dtype."""
    who = "pack_upconv5x5"
    weights = _check_filters(who, weights, dtype)
    relu = tuple(bool(r) for r in relu)[:len(weights)]
    if len(relu) != len(weights):
        raise ValueError("%s: relu needs one entry per filter" % who)
    if any(b and not a for a, b in zip(relu, relu[1:])):
        raise ValueError("%s: the filters with a ReLU come first, got relu=%s" % (who, relu))
    if batchnorms is not None:
        batchnorms = tuple(batchnorms)
        if len(batchnorms) != len(weights):
            raise ValueError("%s: batchnorms needs one entry per filter" % who)
        for w, bn in zip(weights, batchnorms):
            if bn.num_features != w.shape[0] or bn.running_mean is None:
                raise ValueError("%s: a batch norm over %d channels with running statistics per filter" % (who, w.shape[0]))
    dev = _require_device(*weights)
    out_channels, C = [w.shape[0] for w in weights], weights[0].shape[1]
    total = sum(out_channels)
    bytes_fn, pack_fn, _, _, esize = _UPCONV_KERNELS[dtype]
    nbytes = getattr(_lib.lib(), bytes_fn)(total, C)
    if not nbytes:
        raise ValueError("%s: the packed form of %d x %d channels has 2^31 elements or more" % (who, total, C))
    sources = list(weights)
    with torch.no_grad():
        wc = [w.detach().contiguous() for w in weights]
        packed = torch.empty(nbytes // esize, dtype=dtype, device=dev)
        launch(dev, pack_fn, _ptrs(wc), _channels(wc), len(wc), C, 5, 5, _dt(wc[0]), _p(packed))
        scale = shift = None
        if batchnorms is not None:
            scales, shifts = [], []
            for w, bn in zip(weights, batchnorms):
                _require_device(w, *_bn_sources(bn))
                sources += _bn_sources(bn)
                s, b = _fold(bn)
                scales.append(s)
                shifts.append(b)
            scale, shift = torch.cat(scales).contiguous(), torch.cat(shifts).contiguous()
    return UpconvPack(packed, scale, shift, out_channels, C, sum(o for o, r in zip(out_channels, relu) if r), sources, dtype)


UPCONV_PRECISIONS = (None, "exact", "bf16x3")


def up_pooling_conv5x5(x, pack_or_weights, oheight, owidth, scale=None, shift=None, relu_channels=0, precision=None):
    """Un-pooling by 2 to (oheight, owidth), the one or two bias-free 5x5 convolutions (padding 2) of a decoder block over it, a
    per-channel affine map and a ReLU on the leading channels, in one kernel:

        x [N,C,H,W], filters (w_0 [O_0,C,5,5][, w_1 [O_1,C,5,5]])  ->  (y_0 [N,O_0,oheight,owidth][, y_1 [N,O_1,oheight,owidth]])
        (y_0 | y_1)[:, q] == act_q(conv2d(up_pooling(x, 2, oheight, owidth), w, padding=2)[:, q] * scale[q] + shift[q])

    over the flat channels q of both filters, act_q the ReLU for q < relu_channels — with a pack of ``pack_upconv5x5(weights,
    (bn1, sc_bn1))`` that is ``relu(bn1(conv1(u)))`` and ``sc_bn1(sc_conv1(u))`` of ``Gudi_UpProj_Block`` in eval mode
    (unet_ours.py:205-223).  The un-pooled map u is never written: each of the four output phases is an implicit GEMM over the 9, 6, 6
    or 4 taps that meet the compact map (include/cspn_upconv.h), on the fp32 matrix cores — exact fp32 products, every output one
    chain over (tap, channel), so a frame's bits do not depend on the batch and runs repeat.  fp32 on a ROCm device; 1 <= oheight
    <= 2H, 1 <= owidth <= 2W as ``up_pooling`` at scale 2; every tensor below 2^31 elements.

    Half precision: a fp16 ``x`` goes with an ``UpconvPack`` of ``dtype`` fp16 (``pack_upconv5x5(..., dtype=torch.float16)``) and
    gives fp16 outputs — fp16 products accumulated in fp32 on the fp16 matrix cores, the affine map and the ReLU in fp32, one
    rounding to fp16 at the end (include/cspn_uphalf.h); the same contract otherwise.  The filters themselves are taken in fp32 only.

    ``precision``: None or ``"exact"`` — the above — or ``"bf16x3"``: fp32 ``x``, fp32 outputs and the same fp32 pack (switching costs
    no repack), but every value of ``x`` and of the filters is split into three bf16 terms that sum to it exactly, and the six
    leading cross products of a product run on the bf16 matrix cores with fp32 accumulation (include/cspn_upconv.h: the order, the
    bound (2^-23 + 2^-32) |x w| on what a product drops, and what an Inf or a value outside bf16's range does).  fp32-class results
    with other bits than the exact path — hence never a default — and the same contract otherwise: bits independent of the batch,
    runs repeat, capturable.  Refused with a half ``x`` or a fp16 pack.

    ``pack_or_weights``: an ``UpconvPack`` (its scale, shift and ReLU count apply; the arguments of that name must be left alone),
    or the filters themselves — packed for this one call — with ``scale`` / ``shift`` (fp32 [O_0 + O_1], both or neither) and
    ``relu_channels`` as given.

    Forward only.  With grad mode on and ``x`` or a source of the pack requiring a gradient it raises: training runs the stock
    blocks (``up_pooling`` and the convolutions, as the models do by default).

    One difference from the stock blocks: a NaN or Inf in ``x[n,c,i,j]`` reaches only the outputs whose 5x5 window covers (2i, 2j).
    The reference's un-pooling holds ``x * 0`` at the inserted positions, so there it also reaches the rest of the windows over its
    2 x 2 block."""
    who = "up_pooling_conv5x5"
    if x.dim() != 4:
        raise ValueError("%s: x must be [N,C,H,W], got %s" % (who, tuple(x.shape)))
    pack = pack_or_weights if isinstance(pack_or_weights, UpconvPack) else None
    if precision not in UPCONV_PRECISIONS:
        raise ValueError("%s: precision must be None, \"exact\" or \"bf16x3\", got %r" % (who, precision))
    if precision == "bf16x3" and (x.dtype == torch.float16 or (pack is not None and pack.dtype == torch.float16)):
        raise ValueError("%s: precision=\"bf16x3\" splits fp32 values: it takes a fp32 x and a fp32 pack, got x %s%s (a half x runs on the "
                         "fp16 matrix cores as it is)" % (who, x.dtype, "" if pack is None else " and a pack of %s" % pack.dtype))
    if pack is not None:
        if scale is not None or shift is not None or relu_channels:
            raise ValueError("%s: scale, shift and relu_channels come with the pack" % who)
        out_channels, C_w, sources = pack.out_channels, pack.in_channels, pack.sources
        scale, shift, relu_channels = pack.scale, pack.shift, pack.relu_channels
    else:
        weights = _check_filters(who, pack_or_weights)
        out_channels, C_w, sources = tuple(w.shape[0] for w in weights), weights[0].shape[1], weights
    N, C, H, W = x.shape
    if C != C_w:
        raise ValueError("%s: x has %d channels, the filters take %d" % (who, C, C_w))
    if pack is None:
        if x.dtype != torch.float32:
            raise ValueError("%s: fp32 only with the filters themselves (a half x takes pack_upconv5x5(..., dtype=torch.float16)), got %s"
                             % (who, x.dtype))
    elif x.dtype != pack.dtype:
        raise ValueError("%s: x is %s, the pack was made for %s (pack_upconv5x5(..., dtype=...); fp32 and fp16 packs exist)"
                         % (who, x.dtype, pack.dtype))
    total = sum(out_channels)
    if (scale is None) != (shift is None):
        raise ValueError("%s: scale and shift come together" % who)
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (total,)):
            raise ValueError("%s: %s must be fp32 [%d], got %s %s" % (who, name, total, t.dtype, tuple(t.shape)))
    relu_channels = int(relu_channels)
    if not 0 <= relu_channels <= total:
        raise ValueError("%s: relu_channels %d outside [0, %d]" % (who, relu_channels, total))
    oheight, owidth = int(oheight), int(owidth)
    if N < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError("%s: empty input %s" % (who, tuple(x.shape)))
    if not (1 <= oheight <= 2 * H and 1 <= owidth <= 2 * W):
        raise ValueError("%s: output %dx%d must lie within [1, %d] x [1, %d] (scale 2 of a %dx%d input)"
                         % (who, oheight, owidth, 2 * H, 2 * W, H, W))
    if x.numel() >= 2 ** 31 or N * max(out_channels) * oheight * owidth >= 2 ** 31:
        raise ValueError("%s: a tensor of 2^31 elements or more; split the batch" % who)
    if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in sources)):
        raise RuntimeError("%s is forward-only: with grad mode on, run the stock blocks (up_pooling and the 5x5 convolutions, the "
                           "models' default and their training path), or call it under torch.no_grad()" % who)
    dev = _require_device(x, scale, shift, *sources)
    if pack is None:
        pack = pack_upconv5x5(weights, None, (False,) * len(weights))
    xc = x.contiguous()
    outs = tuple(torch.empty((N, o, oheight, owidth), dtype=pack.dtype, device=dev) for o in out_channels)
    tail = (_p(pack.packed), _p(None if scale is None else scale.contiguous()), _p(None if shift is None else shift.contiguous()),
            relu_channels, _ptrs(outs), (ctypes.c_int * len(outs))(*out_channels), len(outs), N, C, H, W, oheight, owidth)
    _, _, forward_fn, takes_dtype, _ = _UPCONV_KERNELS[pack.dtype]
    dtype = _lib.UPCONV_F32_BF16X3 if precision == "bf16x3" else _dt(xc)       # the arithmetic; the tensors are fp32 either way
    launch(dev, forward_fn, _p(xc), *((dtype,) if takes_dtype else ()), *tail)
    return outs


def pack_conv3x3(weight, batchnorm=None, split=None, dtype=torch.float32):
    """The pack ``conv3x3_bn_act`` runs on: ``weight`` — one bias-free [O, C, 3, 3] filter on a ROCm device (``conv1_1.weight``,
    ``conv2.weight``) — reordered for the kernel, and ``batchnorm`` — None or its ``nn.BatchNorm2d`` — folded in fp32 by device tensor
    ops exactly as ``pack_upconv5x5`` folds one.  ``split``: Ca, when the convolution reads the concatenation of a [N, Ca, H, W] and a
    [N, C - Ca, H, W] map (``conv3x3_bn_act`` then takes the second as ``side``); the default is all of C, one map.  ``dtype``: fp32, or
    fp16 for the half kernel — fp32 weights are rounded once, fp16 weights (``model.half()``) go into a fp16 pack alone.  An
    ``UpconvPack``: ``stale()`` and ``made_from()`` as there."""
    who = "pack_conv3x3"
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("%s: a pack is fp32 or fp16, got dtype=%s" % (who, dtype))
    if not torch.is_tensor(weight) or weight.dim() != 4 or weight.shape[0] < 1 or weight.shape[1] < 1 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("%s: weight must be [O,C,3,3], got %s" % (who, tuple(weight.shape) if torch.is_tensor(weight) else type(weight)))
    if weight.dtype != torch.float32 and not (dtype == torch.float16 and weight.dtype == torch.float16):
        raise ValueError("%s: fp32 only (a fp16 weight goes into a pack of dtype=torch.float16 alone), got %s" % (who, weight.dtype))
    O, C = weight.shape[:2]
    if split is not None and not 1 <= int(split) <= C:
        raise ValueError("%s: split %s outside [1, %d], the weight's input channels" % (who, split, C))
    Ca = C if split is None else int(split)
    if batchnorm is not None and (batchnorm.num_features != O or batchnorm.running_mean is None):
        raise ValueError("%s: batchnorm must be over %d channels with running statistics" % (who, O))
    if weight.numel() >= 2 ** 31:
        raise ValueError("%s: weight has 2^31 elements or more" % who)
    sources = [weight] + ([] if batchnorm is None else _bn_sources(batchnorm))
    dev = _require_device(*sources)
    nbytes = _lib.lib().cspn_uptail_packed_bytes(O, Ca, C - Ca, _DT[dtype])
    if not nbytes:
        raise ValueError("%s: the packed form of %d x %d channels has 2^31 elements or more" % (who, O, C))
    with torch.no_grad():
        wc = weight.detach().contiguous()
        packed = torch.empty(nbytes // (4 if dtype == torch.float32 else 2), dtype=dtype, device=dev)
        launch(dev, "cspn_uptail_pack", _p(wc), O, Ca, C - Ca, 3, 3, _dt(wc), _DT[dtype], _p(packed))
        scale, shift = (None, None) if batchnorm is None else (t.contiguous() for t in _fold(batchnorm))
    return UpconvPack(packed, scale, shift, (O,), C, 0, sources, dtype, Ca if Ca < C else None)


def conv3x3_bn_act(a, pack, side=None, residual=None, relu=True):
    """The 3x3 tail step of a decoder block in one kernel (include/cspn_uptail.h):

        out [N,O,H,W] = act( conv2d(cat(a, side), w, padding=1) * scale + shift  [+ residual] )

    for the filter, scale and shift of ``pack`` (``pack_conv3x3``); ``cat`` is never formed — ``a`` [N,Ca,H,W] and ``side``
    [N,C - Ca,H,W] (a pack made with ``split=Ca``; None otherwise) are read where they are.  ``residual``: [N,O,H,W] or None.
    ``relu``: whether act is the ReLU (NaN stays NaN).  ``conv1_1`` of ``Gudi_UpProj_Block_Cat`` is ``conv3x3_bn_act(out, pack(conv1_1,
    bn1_1, split), side_input)``, ``conv2`` of every block ``conv3x3_bn_act(out, pack(conv2, bn2), residual=shortcut)``.

    Everything is of the pack's dtype, the result too.  fp32: exact products, one fused multiply-add chain over (tap, channel: a before
    side) per output, then fmaf(acc, scale, shift), the residual added with a rounding of its own, the ReLU — the roundings of the
    stock eval path.  fp16: fp16 products accumulated in fp32, the whole epilogue in fp32, ONE rounding to fp16; the stock half path
    rounds after the convolution, after the batch norm and after the add.  A frame's bits do not depend on the batch, runs repeat, and
    the call can be captured in a graph.  Non-contiguous inputs are made contiguous; every tensor stays below 2^31 elements.

    Forward only.  With grad mode on and an input or a source of the pack requiring a gradient it raises: training runs the stock
    block (``cat``, the convolutions and batch norms, as the models do by default)."""
    who = "conv3x3_bn_act"
    if not isinstance(pack, UpconvPack) or len(pack.out_channels) != 1:
        raise ValueError("%s: pack must come from pack_conv3x3" % who)
    if a.dim() != 4:
        raise ValueError("%s: a must be [N,C,H,W], got %s" % (who, tuple(a.shape)))
    N, Ca, H, W = a.shape
    O, C = pack.out_channels[0], pack.in_channels
    if side is None and pack.split is not None:
        raise ValueError("%s: the pack was made with split=%d and needs a side of %d channels" % (who, pack.split, C - pack.split))
    if side is not None and pack.split is None:
        raise ValueError("%s: side given, but the pack was made without a split" % who)
    Cb = 0 if side is None else C - pack.split
    for name, t, want in (("a", a, (N, C - Cb, H, W)), ("side", side, (N, Cb, H, W)), ("residual", residual, (N, O, H, W))):
        if t is None:
            continue
        if t.dtype != pack.dtype:
            raise ValueError("%s: %s is %s, the pack was made for %s" % (who, name, t.dtype, pack.dtype))
        if t.dim() != 4 or t.shape[1] != want[1]:
            raise ValueError("%s: %s has %s channels, the pack takes %d there" % (who, name, t.shape[1] if t.dim() == 4 else "no", want[1]))
        if tuple(t.shape) != want:
            raise ValueError("%s: %s must be %s, got %s" % (who, name, want, tuple(t.shape)))
        if t.numel() >= 2 ** 31:
            raise ValueError("%s: %s has 2^31 elements or more; split the batch" % (who, name))
    if N < 1 or H < 1 or W < 1:
        raise ValueError("%s: empty input %s" % (who, tuple(a.shape)))
    if N * O * H * W >= 2 ** 31:
        raise ValueError("%s: the output has 2^31 elements or more; split the batch" % who)
    inputs = [t for t in (a, side, residual) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in inputs + list(pack.sources)):
        raise RuntimeError("%s is forward-only: with grad mode on, run the stock block (cat, the 3x3 convolutions and batch norms, the "
                           "models' default and their training path), or call it under torch.no_grad()" % who)
    dev = _require_device(*inputs, pack.scale, pack.shift, *pack.sources)
    ac, sc, rc = (None if t is None else t.contiguous() for t in (a, side, residual))
    out = torch.empty((N, O, H, W), dtype=pack.dtype, device=dev)
    launch(dev, "cspn_uptail_forward", _p(ac), _p(sc), _p(pack.packed), _p(pack.scale), _p(pack.shift), _p(rc), int(bool(relu)), _p(out),
           _DT[pack.dtype], N, Ca, Cb, O, H, W)
    return out


DECODER_BLOCKS = ("gud_up_proj_layer1", "gud_up_proj_layer2", "gud_up_proj_layer3", "gud_up_proj_layer4")
# What `fused_decoder=True` selects: the blocks at which `tools/decoder_bench.py upconv` measured the fused head ahead of the stock one by
# more than the spread of the two measurements — its 90th percentile below the stock 10th, warm and cache-cold
# (profiles/r18_upconv_bench.json, RESULTS.md row 33: all four, 3.3 to 5.3 times).
FUSED_DECODER_DEFAULT = ("gud_up_proj_layer1", "gud_up_proj_layer2", "gud_up_proj_layer3", "gud_up_proj_layer4")
# The same rule for half inputs, from `tools/decoder_bench.py uphalf`: the half kernel's 90th percentile below the 10th of the stock half head
# (un-pool, MIOpen convolutions, batch norms and ReLU on half tensors), warm and cache-cold (profiles/r19_uphalf_bench.json,
# RESULTS.md row 34: all four, 3.8 to 9.5 times).
FUSED_DECODER_HALF_DEFAULT = ("gud_up_proj_layer1", "gud_up_proj_layer2", "gud_up_proj_layer3", "gud_up_proj_layer4")


# What `fused_tail=True` selects, by the same rule from `tools/decoder_bench.py uptail` against the stock tail (cat, MIOpen 3x3 convolutions,
# eval batch norms, add, ReLUs) measured in the same process: the fused tail's 90th percentile below the stock 10th, warm and
# cache-cold (profiles/r21_uptail_bench.json, RESULTS.md row 36).  fp32: none — the fused tail was 4 to 67 % SLOWER than the stock tail
# at every stage (11.2 against 9.6 ms per forward), so True selects nothing for fp32 inputs; names still force the path.  fp16: layers 2
# and 3 (1.7 and 1.9 times); at layers 1 and 4 the two paths were within 4 % of each other.
FUSED_TAIL_DEFAULT = ()
FUSED_TAIL_HALF_DEFAULT = ("gud_up_proj_layer2", "gud_up_proj_layer3")


def _select(model, switch, value, default, half_default, attr):
    """One switch of the models over DECODER_BLOCKS: False / None, True (`default`; for half inputs `half_default`) or a collection of
    block names (for inputs of either precision).  Marks the blocks (`attr`, `attr`_half) and returns the fp32 names in decoder order."""
    if value is True:
        names = default
    elif not value:
        names = ()
    elif isinstance(value, str):
        names = (value,)
    else:
        names = tuple(value)
    unknown = [n for n in names if n not in DECODER_BLOCKS]
    if unknown:
        raise ValueError("%s: %s not among %s" % (switch, unknown, list(DECODER_BLOCKS)))
    for n in DECODER_BLOCKS:
        setattr(getattr(model, n), attr, n in names)
        setattr(getattr(model, n), attr + "_half", n in (half_default if value is True else names))
    return tuple(n for n in DECODER_BLOCKS if n in names)


def select_fused_decoder(model, fused_decoder):
    """The `fused_decoder` switch of the models: False / None, True (FUSED_DECODER_DEFAULT; for half inputs
    FUSED_DECODER_HALF_DEFAULT) or a collection of block names out of DECODER_BLOCKS (for inputs of either precision).  Marks the named
    blocks and returns their names in decoder order (what the model keeps as `fused_decoder`)."""
    return _select(model, "fused_decoder", fused_decoder, FUSED_DECODER_DEFAULT, FUSED_DECODER_HALF_DEFAULT, "fused_head")


def select_fused_precision(model, precision):
    """The `fused_decoder_precision` keyword of the models: None, "exact" or "bf16x3" (``up_pooling_conv5x5``'s ``precision``), set
    on every decoder block as `fused_precision`.  It selects no block — `fused_decoder` does — and is never a default: "bf16x3"
    changes bits.  What the model keeps as `fused_decoder_precision`."""
    if precision not in UPCONV_PRECISIONS:
        raise ValueError("fused_decoder_precision: must be None, \"exact\" or \"bf16x3\", got %r" % (precision,))
    for n in DECODER_BLOCKS:
        getattr(model, n).fused_precision = precision
    return precision


def select_fused_tail(model, fused_tail):
    """The `fused_tail` switch of the models, as `select_fused_decoder`: True selects FUSED_TAIL_DEFAULT (half inputs:
    FUSED_TAIL_HALF_DEFAULT), names select those blocks for both precisions.  What the model keeps as `fused_tail`."""
    return _select(model, "fused_tail", fused_tail, FUSED_TAIL_DEFAULT, FUSED_TAIL_HALF_DEFAULT, "fused_tail")


class FusedHead(object):
    """Mixed into the decoder blocks: the block's head — un-pool, conv1 -> bn1 -> ReLU and, where the block has one, sc_conv1 -> sc_bn1 —
    as one ``up_pooling_conv5x5`` call when the block is marked (`fused_head`, set by the model's `fused_decoder`), in eval mode and
    with grad mode off.  The pack is made at the first such call, made again when a source changed (``load_state_dict``, an
    in-place update, a parameter replaced by ``.to()``) and dropped by ``train()``; it is no parameter, buffer or module.  It is made
    for the dtype of the block's input, fp32 or fp16, and made again when that changes (one pack at a time: a model run in both
    precisions in turn repacks at every change).  `fused_precision` (the models' `fused_decoder_precision`) is handed to
    ``up_pooling_conv5x5`` as its ``precision`` for fp32 inputs; half inputs ignore it, and the fp32 pack is the same for every value."""
    fused_head = False
    fused_head_half = None               # None: as fused_head (a block marked by hand)
    fused_precision = None               # the `precision` of up_pooling_conv5x5 for fp32 inputs (the models' fused_decoder_precision)
    _upconv_pack = None

    def _fuse_head(self, x=None):
        """Does this call run the fused head?  ``x``: the block's input — fp32 goes by `fused_head`, fp16 (autocast, ``model.half()``)
        by `fused_head_half`, any other dtype runs the stock block."""
        if self.training or torch.is_grad_enabled():
            return False
        if x is None or x.dtype == torch.float32:
            return self.fused_head
        if x.dtype == torch.float16:
            return self.fused_head if self.fused_head_half is None else self.fused_head_half
        return False

    def _head(self, x):
        """(relu(bn1(conv1(u))), sc_bn1(sc_conv1(u)) or None) for u = the un-pooled x, without u."""
        convs, bns = [self.conv1], [self.bn1]
        if hasattr(self, "sc_conv1"):
            convs.append(self.sc_conv1)
            bns.append(self.sc_bn1)
        weights = [c.weight for c in convs]
        pack = self._upconv_pack
        if pack is None or pack.dtype != x.dtype or pack.stale() or not pack.made_from(weights + [t for bn in bns for t in _bn_sources(bn)]):
            pack = self._upconv_pack = pack_upconv5x5(weights, bns, (True, False)[:len(convs)], dtype=x.dtype)
        if self.fused_precision is not None and x.dtype == torch.float32:       # half inputs run the fp16 kernel whatever it says
            outs = up_pooling_conv5x5(x, pack, self.oheight, self.owidth, precision=self.fused_precision)
        else:
            outs = up_pooling_conv5x5(x, pack, self.oheight, self.owidth)
        return outs[0], (outs[1] if len(outs) > 1 else None)

    # The tail of the block — conv1_1 -> bn1_1 -> ReLU over (out, side_input) where the block has them, then conv2 -> bn2, + shortcut,
    # ReLU — as one ``conv3x3_bn_act`` call per convolution when the block is marked (`fused_tail`, set by the model's `fused_tail`),
    # under the conditions of the head and whether or not the head of the same block is fused.  Its packs are kept as the head's is.
    fused_tail = False
    fused_tail_half = None               # None: as fused_tail
    _tail_packs = None

    def _fuse_tail(self, *operands):
        """Does this call run the fused tail?  ``operands``: the tensors the tail reads (out, shortcut, side_input) — all fp32 goes
        by `fused_tail`, all fp16 by `fused_tail_half`, anything else runs the stock lines.  Without operands: could any call?"""
        if self.training or torch.is_grad_enabled():
            return False
        half = self.fused_tail if self.fused_tail_half is None else self.fused_tail_half
        if not operands:
            return self.fused_tail or half
        dtype = operands[0].dtype
        if any(t.dtype != dtype for t in operands):
            return False
        return self.fused_tail if dtype == torch.float32 else half if dtype == torch.float16 else False

    def _stock_head(self, x):
        """What `_head` returns, on stock ops."""
        x = self._up_pooling(x, 2)
        return self.relu(self.bn1(self.conv1(x))), (self.sc_bn1(self.sc_conv1(x)) if hasattr(self, "sc_conv1") else None)

    def _tail_pack(self, conv, bn, dtype, split=None):
        """The pack of the convolution named `conv` and the batch norm named `bn`, made or made again as the head's."""
        packs = self._tail_packs = self._tail_packs or {}
        pack, weight, bn = packs.get(conv), getattr(self, conv).weight, getattr(self, bn)
        if pack is None or pack.dtype != dtype or pack.stale() or not pack.made_from([weight] + _bn_sources(bn)):
            pack = packs[conv] = pack_conv3x3(weight, bn, split, dtype)
        return pack

    def _tail(self, out, shortcut, side_input=None):
        """relu(bn2(conv2(out')) + shortcut), out' = relu(bn1_1(conv1_1(cat(out, side_input)))) with a side_input and out without."""
        operands = (out, shortcut) if side_input is None else (out, shortcut, side_input)
        if self._fuse_tail(*operands):
            if side_input is not None:
                out = conv3x3_bn_act(out, self._tail_pack("conv1_1", "bn1_1", out.dtype, out.shape[1]), side_input)
            return conv3x3_bn_act(out, self._tail_pack("conv2", "bn2", out.dtype), residual=shortcut)
        if side_input is not None:
            out = self.relu(self.bn1_1(self.conv1_1(torch.cat((out, side_input), 1))))
        return self.relu(self.bn2(self.conv2(out)) + shortcut)

    def train(self, mode=True):
        self._upconv_pack = self._tail_packs = None
        return super(FusedHead, self).train(mode)


class MyBlock(FusedHead, nn.Module):
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

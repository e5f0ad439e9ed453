"""The encoder's convolutions on the HIP engine (include/cspn_convbn.h): a bias-free k x k convolution (k = 1 or 3, padding k // 2,
stride 1 or 2), its eval-mode batch norm, an optional residual and an optional ReLU in one kernel.

``pack_conv_bn`` reorders a filter once and folds its batch norm; ``conv_bn_act`` runs one convolution on such a pack.  Forward only,
fp32 or fp16, and opt-in: ``fused_encoder`` of the two models routes the residual blocks of ``layer1`` .. ``layer4`` and the bridge
``bn2(conv2(x))`` between encoder and decoder through it in eval mode with grad mode off (``FusedResidual``, ``FusedBridge``), and is
off by default.  The kernel is the implicit GEMM of the decoder's 3x3 tail (``up_pooling.conv3x3_bn_act``) with a window and a stride;
for k = 3 at stride 1 the two give the same bits.

Not built: a kernel instance with a 64-row tile for the 64-channel convolutions of ``layer1`` (half of every 128-row tile is padding
there), the 7x7 stem (its 4 input channels would be padded to 32) and the max-pool, which stay on stock ops.
"""
import torch

from .. import _lib
from .._host import _dt, _p, _require_device, launch
from .up_pooling import UpconvPack, _bn_sources, _fold

__all__ = ["ConvBnPack", "pack_conv_bn", "conv_bn_act", "select_fused_encoder", "FusedResidual", "FusedBridge", "ENCODER_STAGES",
           "FUSED_ENCODER_DEFAULT", "FUSED_ENCODER_HALF_DEFAULT"]

_DT = {torch.float32: _lib.CSPN_F32, torch.float16: _lib.CSPN_F16}


class ConvBnPack(UpconvPack):
    """What ``conv_bn_act`` runs on: an ``UpconvPack`` of one filter — ``packed``, the folded ``scale`` / ``shift`` (or None), the
    ``dtype``, the sources with ``stale()`` and ``made_from()`` — that also remembers the window ``k`` and the ``stride``."""

    def __init__(self, packed, scale, shift, out_channels, in_channels, k, stride, sources, dtype=torch.float32):
        super(ConvBnPack, self).__init__(packed, scale, shift, (out_channels,), in_channels, 0, sources, dtype)
        self.k, self.stride = int(k), int(stride)


def pack_conv_bn(weight, batchnorm=None, stride=1, dtype=torch.float32):
    """The pack ``conv_bn_act`` runs on: ``weight`` — one bias-free [O, C, k, k] filter on a ROCm device, k = 1 or 3 — reordered for
    the kernel, and ``batchnorm`` — None or its ``nn.BatchNorm2d`` — folded in fp32 by device tensor ops exactly as ``pack_conv3x3``
    folds one: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale.  ``stride``: 1 or 2, the convolution's
    (its padding is k // 2).  ``dtype``: fp32, or fp16 for the half kernel — fp32 weights are rounded once, fp16 weights
    (``model.half()``) go into a fp16 pack alone.  A ``ConvBnPack``: ``stale()`` and ``made_from()`` as ``UpconvPack``."""
    who = "pack_conv_bn"
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("%s: a pack is fp32 or fp16, got dtype=%s" % (who, dtype))
    if not torch.is_tensor(weight) or weight.dim() != 4 or weight.shape[0] < 1 or weight.shape[1] < 1 or \
            tuple(weight.shape[2:]) not in ((1, 1), (3, 3)):
        raise ValueError("%s: weight must be [O,C,k,k] with k = 1 or 3, got %s" % (who, tuple(weight.shape) if torch.is_tensor(weight) else type(weight)))
    if weight.dtype != torch.float32 and not (dtype == torch.float16 and weight.dtype == torch.float16):
        raise ValueError("%s: fp32 only (a fp16 weight goes into a pack of dtype=torch.float16 alone), got %s" % (who, weight.dtype))
    if stride not in (1, 2):
        raise ValueError("%s: stride must be 1 or 2, got %r" % (who, stride))
    O, C, k = weight.shape[:3]
    if batchnorm is not None and (batchnorm.num_features != O or batchnorm.running_mean is None):
        raise ValueError("%s: batchnorm must be over %d channels with running statistics" % (who, O))
    if weight.numel() >= 2 ** 31:
        raise ValueError("%s: weight has 2^31 elements or more" % who)
    sources = [weight] + ([] if batchnorm is None else _bn_sources(batchnorm))
    dev = _require_device(*sources)
    nbytes = _lib.lib().cspn_convbn_packed_bytes(O, C, k, _DT[dtype])
    if not nbytes:
        raise ValueError("%s: the packed form of %d x %d channels has 2^31 elements or more" % (who, O, C))
    with torch.no_grad():
        wc = weight.detach().contiguous()
        packed = torch.empty(nbytes // (4 if dtype == torch.float32 else 2), dtype=dtype, device=dev)
        launch(dev, "cspn_convbn_pack", _p(wc), O, C, k, k, _dt(wc), _DT[dtype], _p(packed))
        scale, shift = (None, None) if batchnorm is None else (t.contiguous() for t in _fold(batchnorm))
    return ConvBnPack(packed, scale, shift, O, C, k, int(stride), sources, dtype)


def conv_bn_act(x, pack, residual=None, relu=True):
    """One convolution of the encoder in one kernel (include/cspn_convbn.h):

        out [N,O,Ho,Wo] = act( conv2d(x, w, stride=s, padding=k // 2) * scale + shift  [+ residual] )

    for the filter, scale, shift, k and s of ``pack`` (``pack_conv_bn``); Ho = (H - 1) // s + 1, Wo = (W - 1) // s + 1.  ``residual``:
    [N,O,Ho,Wo] or None.  ``relu``: whether act is the ReLU (NaN stays NaN).

    Everything is of the pack's dtype, the result too.  fp32: exact products, one fused multiply-add chain over (tap, channel) per
    output, then fmaf(acc, scale, shift), the residual added with a rounding of its own, the ReLU — the roundings of the stock eval
    path.  fp16: fp16 products accumulated in fp32, the whole epilogue in fp32, ONE rounding to fp16; the stock half path rounds after
    the convolution, after the batch norm and after the add.  A frame's bits do not depend on the batch, runs repeat, and the call
    can be captured in a graph.  Non-contiguous inputs are made contiguous; every tensor stays below 2^31 elements.

    Forward only.  With grad mode on and an input or a source of the pack requiring a gradient it raises: training runs the stock
    block (the convolutions and batch norms, as the models do by default)."""
    who = "conv_bn_act"
    if not isinstance(pack, ConvBnPack):
        raise ValueError("%s: pack must come from pack_conv_bn" % who)
    if x.dim() != 4:
        raise ValueError("%s: x must be [N,C,H,W], got %s" % (who, tuple(x.shape)))
    N, _, H, W = x.shape
    O, C, s = pack.out_channels[0], pack.in_channels, pack.stride
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    for name, t, want in (("x", x, (N, C, H, W)), ("residual", residual, (N, O, Ho, Wo))):
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
        raise ValueError("%s: empty input %s" % (who, tuple(x.shape)))
    if N * O * Ho * Wo >= 2 ** 31:
        raise ValueError("%s: the output has 2^31 elements or more; split the batch" % who)
    inputs = [t for t in (x, residual) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in inputs + list(pack.sources)):
        raise RuntimeError("%s is forward-only: with grad mode on, run the stock block (the convolutions and batch norms, the models' "
                           "default and their training path), or call it under torch.no_grad()" % who)
    dev = _require_device(*inputs, pack.scale, pack.shift, *pack.sources)
    xc, rc = (None if t is None else t.contiguous() for t in (x, residual))
    out = torch.empty((N, O, Ho, Wo), dtype=pack.dtype, device=dev)
    launch(dev, "cspn_convbn_forward", _p(xc), _p(pack.packed), _p(pack.scale), _p(pack.shift), _p(rc), int(bool(relu)), _p(out),
           _DT[pack.dtype], N, C, O, H, W, pack.k, s)
    return out


ENCODER_STAGES = ("layer1", "layer2", "layer3", "layer4", "conv2")         # "conv2": the bridge bn2(conv2(x))
# What `fused_encoder=True` selects, by the rule of the decoder's switches from `tools/decoder_bench.py encoder` against the stock stage
# (MIOpen convolutions, eval batch norms, adds, ReLUs) measured in the same process: the fused stage's 90th percentile below the stock
# 10th, warm and cache-cold (profiles/r23_encoder_bench.json, RESULTS.md row 38).  Both lists are empty: at B = 24 the fused stages were
# SLOWER than the stock ones in both precisions — fp32 10.1 against 6.3 ms over the five stages (1.2 to 2.6 times per stage), fp16 6.6
# against 3.8 ms (level at layer1 and layer2, 1.7 to 4.4 times at layer3, layer4 and the bridge) — so True selects nothing and only
# names force the path (NEGATIVE_RESULTS.md row 64; DESIGN.md §8 f-16 says what bounds the kernel there).
FUSED_ENCODER_DEFAULT = ()
FUSED_ENCODER_HALF_DEFAULT = ()


def select_fused_encoder(model, fused_encoder):
    """The `fused_encoder` switch of the models: False / None, True (FUSED_ENCODER_DEFAULT; for half inputs
    FUSED_ENCODER_HALF_DEFAULT) or a collection of names out of ENCODER_STAGES (for inputs of either precision).  Marks the residual
    blocks of the named stages and the model's bridge, and returns the names in encoder order (what the model keeps as
    `fused_encoder`)."""
    if fused_encoder is True:
        names, half = FUSED_ENCODER_DEFAULT, FUSED_ENCODER_HALF_DEFAULT
    elif not fused_encoder:
        names = half = ()
    elif isinstance(fused_encoder, str):
        names = half = (fused_encoder,)
    else:
        names = half = tuple(fused_encoder)
    unknown = [n for n in names if n not in ENCODER_STAGES]
    if unknown:
        raise ValueError("fused_encoder: %s not among %s" % (unknown, list(ENCODER_STAGES)))
    for n in ENCODER_STAGES[:4]:
        for block in getattr(model, n):
            block.fused_encoder, block.fused_encoder_half = n in names, n in half
    model.fused_bridge, model.fused_bridge_half = "conv2" in names, "conv2" in half
    return tuple(n for n in ENCODER_STAGES if n in names)


class _FusedConvs(object):
    """What the residual blocks and the bridge share: whether a call runs fused, and the packs — made at the first fused call for the
    dtype of the input, made again when a source changed (``load_state_dict``, an in-place update, a parameter replaced by ``.to()``) or
    the dtype did, and dropped by ``train()``; they are no parameter, buffer or module."""
    _convbn_packs = None

    def _fuses(self, x, mark, half_mark):
        if self.training or torch.is_grad_enabled():
            return False
        half = mark if half_mark is None else half_mark
        if x is None:
            return mark or half
        return mark if x.dtype == torch.float32 else half if x.dtype == torch.float16 else False

    def _convbn_pack(self, key, conv, bn, dtype):
        packs = self._convbn_packs = self._convbn_packs or {}
        pack = packs.get(key)
        if pack is None or pack.dtype != dtype or pack.stale() or not pack.made_from([conv.weight] + _bn_sources(bn)):
            pack = packs[key] = pack_conv_bn(conv.weight, bn, conv.stride[0], dtype)
        return pack

    def train(self, mode=True):
        self._convbn_packs = None
        return super(_FusedConvs, self).train(mode)


class FusedResidual(_FusedConvs):
    """Mixed into BasicBlock and Bottleneck: when the block is marked (`fused_encoder`, set by the model's `fused_encoder`), in eval
    mode, with grad mode off and on a fp32 or fp16 input, every convolution of the block is one ``conv_bn_act`` call — conv1 + bn1 +
    ReLU, (Bottleneck: conv2 + bn2 + ReLU,) the downsample convolution + its batch norm where the block has one (no ReLU), and the last
    convolution + its batch norm + the shortcut + ReLU.  Anything else runs the block's own lines."""
    fused_encoder = False
    fused_encoder_half = None            # None: as fused_encoder (a block marked by hand)

    def _fuse_encoder(self, x=None):
        return self._fuses(x, self.fused_encoder, self.fused_encoder_half)

    def _fused_forward(self, x):
        names = [n for n in ("conv1", "conv2", "conv3") if hasattr(self, n)]
        out = x
        for n in names[:-1]:
            out = conv_bn_act(out, self._convbn_pack(n, getattr(self, n), getattr(self, "bn" + n[4:]), x.dtype))
        shortcut = x
        if self.downsample is not None:
            shortcut = conv_bn_act(x, self._convbn_pack("downsample", self.downsample[0], self.downsample[1], x.dtype), relu=False)
        last = names[-1]
        return conv_bn_act(out, self._convbn_pack(last, getattr(self, last), getattr(self, "bn" + last[4:]), x.dtype), residual=shortcut)


class FusedBridge(_FusedConvs):
    """Mixed into the two ResNets: the bridge bn2(conv2(x)) between encoder and decoder as one ``conv_bn_act`` call without a ReLU when
    the model is marked (`fused_bridge`, set by `fused_encoder` naming "conv2"), under the conditions of ``FusedResidual``."""
    fused_bridge = False
    fused_bridge_half = None

    def _bridge(self, x):
        if self._fuses(x, self.fused_bridge, self.fused_bridge_half):
            return conv_bn_act(x, self._convbn_pack("conv2", self.conv2, self.bn2, x.dtype), relu=False)
        return self.bn2(self.conv2(x))

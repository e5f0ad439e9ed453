"""Host model the reference's ``get_model`` returns (network/__init__.py:19-20): the topology of its
network/unet_ours.py:251-335 — ResNet encoder on a 4-channel RGB-D input, ``MyBlock`` decoder with encoder skips, a
1-channel coarse-depth head and a bias-free 8-channel affinity head, ``CSPN_ours.AffinityPropagate(prop_time=24)`` (the
K x K pixel-adaptive recurrence, K = 3 for 8 channels) on top; output ``[x, guidance]``.

As network/unet_cspn_nyu.py here, this file is the CALLER of the hot path: convolutions and batch-norms are stock
``torch.nn`` ops; the two pieces of this package it uses are ``network.up_pooling.MyBlock`` (the zero-insertion un-pooling
of every decoder block as one HIP kernel, instead of a grouped conv_transpose2d against a freshly allocated one-hot
weight, unet_ours.py:138-150) and ``post_process.CSPN_ours.AffinityPropagate`` (the HIP recurrence, forward and backward).

Attribute names are the reference's — they are the checkpoint format: ``resnet50().state_dict()`` has the reference's 417
keys / 218 123 072 parameters (``conv3``, which the reference builds at :270 and never calls, included) and loads one of
its checkpoints with ``strict=True``.  Modules are constructed in the reference's order, so the same ``torch.manual_seed``
gives the same weights.  The encoder blocks are the ones of unet_cspn_nyu.py here (the reference's two files define the
same BasicBlock / Bottleneck, unet_ours.py:59-128); the decoder blocks subclass ``MyBlock`` as unet_ours.py:160-248 do.
The import this replaces at unet_ours.py:16 is ``from cspn_monodepth_amd.post_process import CSPN_ours as post_process``.
"""
import torch
import torch.nn as nn

from ..post_process import CSPN_ours as post_process
from .unet_cspn_nyu import DECODER_SIZES_NYU, BasicBlock, Bottleneck, _conv
from .conv_bn import FusedBridge, select_fused_encoder
from . import up_pooling as _up
from .up_pooling import MyBlock, select_fused_decoder, select_fused_precision, select_fused_tail

__all__ = ["ResNet", "resnet50", "resnet18", "Bottleneck", "BasicBlock", "UpProj_Block", "Gudi_UpProj_Block",
           "Gudi_UpProj_Block_Cat", "Simple_Gudi_UpConv_Block", "Simple_Gudi_UpConv_Block_Last_Layer", "DECODER_SIZES_NYU", "decoder_sizes_for"]


def decoder_sizes_for(height, width):
    """The five (oheight, owidth) pairs for an input of that size: every stride-2 stage of the encoder maps n to ceil(n / 2)
    (7x7 / 3x3 windows with padding 3 / 1), and decoder stage i un-pools back to the size of the matching encoder stage.
    decoder_sizes_for(228, 304) == DECODER_SIZES_NYU."""
    sizes = [(int(height), int(width))]
    for _ in range(4):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return tuple(reversed(sizes))


class Gudi_UpProj_Block(MyBlock):                              # unet_ours.py:205-223
    """un-pool -> [5x5 conv, BN, ReLU, 3x3 conv, BN] + [5x5 conv, BN] shortcut -> ReLU."""

    def __init__(self, in_channels, out_channels, oheight=0, owidth=0):
        super(Gudi_UpProj_Block, self).__init__(oheight, owidth)
        self.conv1, self.bn1 = _conv(in_channels, out_channels, 5), nn.BatchNorm2d(out_channels)
        self.conv2, self.bn2 = _conv(out_channels, out_channels, 3), nn.BatchNorm2d(out_channels)
        self.sc_conv1, self.sc_bn1 = _conv(in_channels, out_channels, 5), nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=False)

    def forward(self, x):
        if self._fuse_head(x) or self._fuse_tail():
            return self._tail(*(self._head(x) if self._fuse_head(x) else self._stock_head(x)))
        x = self._up_pooling(x, 2)
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + self.sc_bn1(self.sc_conv1(x)))


class UpProj_Block(Gudi_UpProj_Block):                           # unet_ours.py:160-178: the same block under its other name
    pass


class Simple_Gudi_UpConv_Block(MyBlock):                         # unet_ours.py:181-191: un-pool -> 5x5 conv, BN, ReLU
    def __init__(self, in_channels, out_channels, oheight=0, owidth=0):
        super(Simple_Gudi_UpConv_Block, self).__init__(oheight, owidth)
        self.conv1, self.bn1 = _conv(in_channels, out_channels, 5), nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=False)

    def forward(self, x):
        if self._fuse_head(x):
            return self._head(x)[0]
        return self.relu(self.bn1(self.conv1(self._up_pooling(x, 2))))


class Simple_Gudi_UpConv_Block_Last_Layer(MyBlock):              # unet_ours.py:194-202: un-pool -> one bias-free 3x3 conv
    def __init__(self, in_channels, out_channels, oheight=0, owidth=0):
        super(Simple_Gudi_UpConv_Block_Last_Layer, self).__init__(oheight, owidth)
        self.conv1 = _conv(in_channels, out_channels, 3)

    def forward(self, x):
        return self.conv1(self._up_pooling(x, 2))


class Gudi_UpProj_Block_Cat(MyBlock):                            # unet_ours.py:226-248
    """As Gudi_UpProj_Block, with the encoder skip concatenated after the first conv and fused by a 3x3 conv."""

    def __init__(self, in_channels, out_channels, oheight=0, owidth=0):
        super(Gudi_UpProj_Block_Cat, self).__init__(oheight, owidth)
        self.conv1, self.bn1 = _conv(in_channels, out_channels, 5), nn.BatchNorm2d(out_channels)
        self.conv1_1, self.bn1_1 = _conv(out_channels * 2, out_channels, 3), nn.BatchNorm2d(out_channels)
        self.conv2, self.bn2 = _conv(out_channels, out_channels, 3), nn.BatchNorm2d(out_channels)
        self.sc_conv1, self.sc_bn1 = _conv(in_channels, out_channels, 5), nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=False)

    def forward(self, x, side_input):
        if self._fuse_head(x) or self._fuse_tail():
            return self._tail(*(self._head(x) if self._fuse_head(x) else self._stock_head(x)), side_input)
        x = self._up_pooling(x, 2)
        out = torch.cat((self.relu(self.bn1(self.conv1(x))), side_input), 1)
        out = self.bn2(self.conv2(self.relu(self.bn1_1(self.conv1_1(out)))))
        return self.relu(out + self.sc_bn1(self.sc_conv1(x)))


class ResNet(FusedBridge, nn.Module):
    """unet_ours.py:251-335.  input [B,4,H,W] (RGB + sparse depth) -> [refined depth [B,1,H,W], guidance [B,8,H,W]].

    `up_proj_block` is accepted and ignored, as in the reference (:253; it builds no up_proj_layer).  decoder_sizes: the five
    (oheight, owidth) pairs of the decoder stages; the default is the reference's hard-coded 228 x 304 pyramid (:274-279).
    prop_time: the reference hard-codes 24 (:305).  cspn_plan: handed to the CSPN module.  `return_cspn_io = True` makes
    forward return ([x, guidance], (blur_depth, guidance, sparse_depth)) — the tensors handed to the CSPN module.
    fused_heads (off by default): the two output heads run as one ``up_pooling_conv3x3`` call on the weights of
    gud_up_proj_layer5 / 6 instead of the two blocks — the [B,64,H,W] un-pooled map is neither written nor saved for the backward.
    The blocks and their parameters stay where they are (the same state_dict either way); the sums are the same terms in another
    order, and a NaN in the decoder's last map spreads less far (up_pooling_conv3x3's docstring).  A half map (autocast,
    ``half()``) runs ``up_pooling_conv3x3_half`` on the same weights — forward only, on the fp16 matrix cores (include/cspn_head16.h) —
    when no gradient is needed (grad mode off, or nothing involved requires one), and the two stock blocks when one is.
    fused_decoder (off by default; independent of fused_heads): True, or a collection of block names out of "gud_up_proj_layer1" ..
    "gud_up_proj_layer4".  In eval mode with grad mode off a named block computes relu(bn1(conv1(up(x)))) and sc_bn1(sc_conv1(up(x)))
    with one ``up_pooling_conv5x5`` call on the compact map and runs the rest of itself on stock ops; in train mode or with grad mode
    on it runs exactly the default code.  True selects the blocks where that was measured to be faster
    (up_pooling.FUSED_DECODER_DEFAULT; for a half input — autocast, ``half()`` — FUSED_DECODER_HALF_DEFAULT, on the fp16 kernel of
    include/cspn_uphalf.h; any other dtype runs the default code).  Modules, parameters and the state_dict are the same either way.
    fused_tail (off by default; independent of the other two): True, or block names as for fused_decoder.  Under the same conditions
    a named block runs the rest of itself — conv1_1 -> bn1_1 -> ReLU over (out, side_input) without the ``cat``, then conv2 -> bn2,
    + shortcut, ReLU — as one ``conv3x3_bn_act`` call per convolution (include/cspn_uptail.h), whether its head is fused or not.  True
    selects up_pooling.FUSED_TAIL_DEFAULT (half inputs: FUSED_TAIL_HALF_DEFAULT), the blocks where that was measured to be faster —
    lists that may be empty; names select those blocks in both precisions.
    fused_decoder_precision (None; never a default): the ``precision`` of ``up_pooling_conv5x5`` for the blocks fused_decoder names, on
    fp32 inputs — None / "exact", or "bf16x3": the products split into bf16 terms on the bf16 matrix cores, fp32-class results with
    other bits (include/cspn_upconv.h).  It selects no block, half inputs ignore it, and train or grad mode run the stock blocks.
    fused_encoder (off by default; independent of the other three): True, or a collection of names out of "layer1" .. "layer4" and
    "conv2" (the bridge bn2(conv2(x)) between encoder and decoder).  In eval mode with grad mode off and on a fp32 or fp16 input, every
    residual block of a named stage runs each of its convolutions with its batch norm, and where they follow the shortcut add and the
    ReLU, as one ``conv_bn_act`` call (network/conv_bn.py, include/cspn_convbn.h), and the bridge runs as one call without a ReLU;
    anything else runs exactly the default code.  True selects conv_bn.FUSED_ENCODER_DEFAULT (half inputs:
    FUSED_ENCODER_HALF_DEFAULT), the stages where that was measured to be faster — lists that may be empty; names select those stages
    in both precisions.  The 7x7 stem and the max-pool stay on stock ops.
    The four switches together: fused_heads covers gud_up_proj_layer5 / 6, fused_decoder the head and fused_tail the tail of
    gud_up_proj_layer1 .. 4, fused_encoder layer1 .. 4 and the bridge; each is forward-only, changes no module, parameter or state_dict
    key, and none changes what another does."""

    def __init__(self, block, layers, up_proj_block=None, decoder_sizes=DECODER_SIZES_NYU, prop_time=24, cspn_plan=None,
                 fused_heads=False, fused_decoder=False, fused_tail=False, fused_encoder=False,
                 fused_decoder_precision=None):
        super(ResNet, self).__init__()
        self.inplanes = 64
        e = block.expansion
        self.conv1_1 = nn.Conv2d(4, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=False)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.mid_channel = 256 * e
        self.conv2, self.bn2 = _conv(512 * e, 512 * e, 3), nn.BatchNorm2d(512 * e)
        self.conv3 = _conv(128, 1, 3)                                  # built and never called (:270): a checkpoint key only
        self.post_process_layer = post_process.AffinityPropagate(prop_time=prop_time, plan=cspn_plan)
        s = decoder_sizes
        self.gud_up_proj_layer1 = Gudi_UpProj_Block(512 * e, 256 * e, *s[0])
        self.gud_up_proj_layer2 = Gudi_UpProj_Block_Cat(256 * e, 128 * e, *s[1])
        self.gud_up_proj_layer3 = Gudi_UpProj_Block_Cat(128 * e, 64 * e, *s[2])
        self.gud_up_proj_layer4 = Gudi_UpProj_Block_Cat(64 * e, 64, *s[3])
        self.gud_up_proj_layer5 = Simple_Gudi_UpConv_Block_Last_Layer(64, 1, *s[4])       # coarse ("blur") depth head
        self.gud_up_proj_layer6 = Simple_Gudi_UpConv_Block_Last_Layer(64, 8, *s[4])       # affinity head: K*K - 1 = 8, K = 3
        self.return_cspn_io = False
        self.fused_heads = bool(fused_heads)
        self.fused_decoder = select_fused_decoder(self, fused_decoder)
        self.fused_tail = select_fused_tail(self, fused_tail)
        self.fused_encoder = select_fused_encoder(self, fused_encoder)
        self.fused_decoder_precision = select_fused_precision(self, fused_decoder_precision)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(_conv(self.inplanes, planes * block.expansion, 1, stride),
                                       nn.BatchNorm2d(planes * block.expansion))
        stack = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        stack += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*stack)

    def unused_parameters(self):
        """Parameters the forward never touches (freeze them before wrapping in DistributedDataParallel)."""
        return list(self.conv3.parameters())

    def features(self, x):
        """Everything below the CSPN module: (blur_depth [B,1,H,W], guidance [B,8,H,W], sparse_depth [B,1,H,W])."""
        sparse_depth = x.narrow(1, 3, 1).clone()                       # :308
        x = self.conv1_1(x)
        skip4 = x                                                      # pre-BN stem output, 64 ch at H/2 (:310)
        x = self.layer1(self.maxpool(self.relu(self.bn1(x))))
        skip3 = x                                                      # 64e ch at H/4 (:316)
        x = self.layer2(x)
        skip2 = x                                                      # 128e ch at H/8 (:319)
        x = self._bridge(self.layer4(self.layer3(x)))
        x = self.gud_up_proj_layer1(x)
        x = self.gud_up_proj_layer2(x, skip2)
        x = self.gud_up_proj_layer3(x, skip3)
        x = self.gud_up_proj_layer4(x, skip4)
        if self.fused_heads:
            l5, l6 = self.gud_up_proj_layer5, self.gud_up_proj_layer6
            outs = _up.fused_heads_forward(x, (l5.conv1.weight, l6.conv1.weight), l5.oheight, l5.owidth)
            if outs is not None:                                       # None: a half x that needs a gradient, the stock blocks below
                return outs[0], outs[1], sparse_depth
        return self.gud_up_proj_layer5(x), self.gud_up_proj_layer6(x), sparse_depth

    def forward(self, x):
        blur_depth, guidance, sparse_depth = self.features(x)
        x = self.post_process_layer(blur_depth, guidance, sparse_depth=sparse_depth)      # :333
        if self.return_cspn_io:
            return [x, guidance], (blur_depth, guidance, sparse_depth)
        return [x, guidance]


def resnet50(pretrained=False, **kwargs):
    """unet_ours.py:352-363.  `pretrained` would read pretrained/resnet50.pth there; no checkpoint ships with this package."""
    if pretrained:
        raise RuntimeError("no pretrained checkpoint is available here; load one with model.load_state_dict(...)")
    return ResNet(Bottleneck, [3, 4, 6, 3], UpProj_Block, **kwargs)


def resnet18(pretrained=False, **kwargs):
    """unet_ours.py:338-349.  Deviation: the reference hard-codes the decoder widths of the ResNet-50 plan (2048 / 1024 / 512 /
    256, :274-277), so its own resnet18 cannot run a forward (channel mismatch at the first decoder block); here the widths
    follow the block expansion (512 e, 256 e, ...), the same numbers for ResNet-50 and a working model for ResNet-18.
    Checkpoints of the reference exist for ResNet-50 only (state_dict parity: tests, golden G17)."""
    if pretrained:
        raise RuntimeError("no pretrained checkpoint is available here; load one with model.load_state_dict(...)")
    return ResNet(BasicBlock, [2, 2, 2, 2], UpProj_Block, **kwargs)

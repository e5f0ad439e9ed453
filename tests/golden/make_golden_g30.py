#!/usr/bin/env python3
"""Golden G30 (convbn): the reference's encoder blocks and its bridge in eval mode, made by IMPORTING the reference.

    python tests/golden/make_golden_g30.py        (needs the reference: CSPN_REFERENCE, default the directory `reference` beside this repository)

For every case of tests/convbn_cases.GOLDEN_CASES: one ``Bottleneck`` or ``BasicBlock`` (network/unet_ours.py:59-128), without a
downsample branch (stride 1, inplanes = planes * expansion) and with the stride-2 one ``_make_layer`` builds (:281-288: a bias-free 1x1
convolution at the block's stride and a batch norm), or the bridge ``bn2(conv2(x))`` of ``ResNet.forward`` (:324) from the reference's
``conv3x3`` and ``BatchNorm2d`` — on the CPU in fp64, eval mode, with running statistics and affine parameters that are not the initial
ones.  Writes g30_convbn_<case>.npz with

    x                               the block's input, fp64
    w_<conv>, bn_<bn>               the parameters; bn_*: [4, O] gamma, beta, running_mean, running_var (fp32 values);
                                    <conv> / <bn> are conv1 / bn1 .. conv3 / bn3 and downsample / downsample
    eps                             0.5 for the integer-valued cases (gamma in {0.5, 1, 2, -4}, variance in {0.5, 3.5, 15.5}: every
                                    folded scale and shift is a power of two times a small integer, and every sum is exact), the
                                    default 1e-5 for the others
    out1, out2, shortcut, y         the reference in fp64: after bn1 + ReLU, after bn2 + ReLU (Bottleneck), the downsample branch,
                                    and the block's forward
    kind, geom                      the block's class name or "bridge"; stride, planes, inplanes

Nothing is written unless tests/convbn_cases.restate, composed per block, agrees with the reference (exactly / to 1e-12 of the
largest element).
"""
import json
import os
import sys
import types
from collections import defaultdict

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CSPN_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
_stub = types.ModuleType("torch._thnn")          # pac.py:20 imports torch._thnn (removed in torch>=1.0)
_stub.type2backend = defaultdict(lambda: None)
sys.modules.setdefault("torch._thnn", _stub)

from network import unet_ours as ref_net                    # noqa: E402  (reference)
import convbn_cases as cc                                   # noqa: E402
from make_golden_g27 import make_bn                         # noqa: E402

torch.set_num_threads(4)
MAX_BYTES = 131072


def main():
    manifest = {"torch": torch.__version__, "files": {}}
    torch.set_default_dtype(torch.float64)
    for idx, (name, (kind, planes, inplanes, stride, down, (N, H, W), integer)) in enumerate(cc.GOLDEN_CASES.items()):
        rng = np.random.RandomState(3000 + idx)
        draw = (lambda *s: rng.randint(-3, 4, size=s).astype(np.float64)) if integer else (lambda *s: rng.standard_normal(s))
        x = draw(N, inplanes, H, W)
        eps = 0.5 if integer else 1e-5
        if kind == "bridge":
            block = nn.Module()
            block.conv2, block.bn2 = ref_net.conv3x3(inplanes, planes), ref_net.BatchNorm2d(planes)      # unet_ours.py:267-269
            pairs = {"conv2": (block.conv2, block.bn2, "bn2")}
        else:
            cls = getattr(ref_net, kind)
            downsample = None
            if down:                                             # unet_ours.py:283-288
                downsample = nn.Sequential(nn.Conv2d(inplanes, planes * cls.expansion, kernel_size=1, stride=stride, bias=False),
                                           ref_net.BatchNorm2d(planes * cls.expansion))
            block = cls(inplanes, planes, stride, downsample)
            pairs = {n: (getattr(block, n), getattr(block, "bn" + n[4:]), "bn" + n[4:]) for n in ("conv1", "conv2", "conv3") if hasattr(block, n)}
            if down:
                pairs["downsample"] = (downsample[0], downsample[1], "downsample")
        block.eval()
        arrs = dict(x=x, eps=np.float64(eps), kind=np.array(kind), geom=np.array([stride, planes, inplanes], np.int32))
        for cname, (conv, bn, bname) in pairs.items():
            w, p = draw(*conv.weight.shape).astype(np.float32), make_bn(rng, conv.weight.shape[0], integer)
            conv.weight.data = torch.from_numpy(w).double()
            bn.weight.data, bn.bias.data = torch.from_numpy(p[0]).double(), torch.from_numpy(p[1]).double()
            bn.running_mean.copy_(torch.from_numpy(p[2]).double())
            bn.running_var.copy_(torch.from_numpy(p[3]).double())
            bn.eps = eps
            arrs["w_" + cname], arrs["bn_" + bname] = w, p
        with torch.no_grad():
            xt = torch.from_numpy(x)
            if kind == "bridge":
                y = block.bn2(block.conv2(xt))
            else:
                arrs["out1"] = block.relu(block.bn1(block.conv1(xt))).numpy().copy()
                if kind == "Bottleneck":
                    arrs["out2"] = block.relu(block.bn2(block.conv2(torch.from_numpy(arrs["out1"])))).numpy().copy()
                if down:
                    arrs["shortcut"] = block.downsample(xt).numpy().copy()
                y = block(xt.clone())                             # BasicBlock adds in place
        assert not block.training, name
        arrs["y"] = y.numpy()
        assert arrs["y"].shape == (N, planes * (1 if kind != "Bottleneck" else 4), cc.out_size(H, stride), cc.out_size(W, stride)), name

        def agree(got, want):
            return np.array_equal(got, want) if integer else np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())

        steps = cc.block_steps(arrs)
        assert len(steps) == len(pairs), name
        for src, w, s, scale, shift, res, relu, dst in steps:
            got = cc.restate(arrs[src], w, s, scale, shift, None if res is None else arrs[res], relu)
            assert agree(got, arrs[dst]), (name, dst)
        if kind != "bridge":
            assert (arrs["y"] == 0).any() and (arrs["y"] > 0).any(), name      # the ReLU cut something and kept something
        path = os.path.join(HERE, "g30_convbn_" + name + ".npz")
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (name, size)
        manifest["files"]["g30_convbn_" + name] = {"bytes": size, "block": kind, "x": list(x.shape), "y": list(arrs["y"].shape), "stride": stride,
                                                   "downsample": bool(down), "integer": integer}
    with open(os.path.join(HERE, "g30_convbn_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("total bytes", sum(v["bytes"] for v in manifest["files"].values()))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden G29 (uptail): the tail of the reference's decoder blocks in eval mode, made by IMPORTING the reference.

    python tests/golden/make_golden_g29.py        (needs the reference: CSPN_REFERENCE, default /root/reference)

For every case of tests/uptail_cases.GOLDEN_CASES: one ``Gudi_UpProj_Block`` or ``Gudi_UpProj_Block_Cat`` (network/unet_ours.py:205-248)
on the CPU in fp64, eval mode, with running statistics and affine parameters that are not the initial ones.  The block's own modules
give the head's two outputs

    u = block._up_pooling(x, 2);  out = block.relu(block.bn1(block.conv1(u)));  shortcut = block.sc_bn1(block.sc_conv1(u))

the intermediate ``mid = block.relu(block.bn1_1(block.conv1_1(cat(out, side))))`` of the ``_Cat`` block, and the block's forward gives
``y``.  Writes g29_uptail_<case>.npz with

    out, shortcut, side             the tail's inputs (side: the ``_Cat`` block only), fp64
    w1_1, bn1_1, w2, bn2            the tail's parameters; bn*: [4, O] gamma, beta, running_mean, running_var (fp32 values)
    eps                             0.5 for the integer-valued cases (gamma in {0.5, 1, 2, -4}, variance in {0.5, 3.5, 15.5}: every
                                    folded scale and shift is a power of two times a small integer, and every sum is exact), the
                                    default 1e-5 for the others
    mid, y                          the reference in fp64
    geom                            H, W, O, 1 for the ``_Cat`` block

Nothing is written unless tests/uptail_cases.restate agrees with the reference (exactly / to 1e-12 of the largest element).
"""
import json
import os
import sys
import types
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CSPN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
_stub = types.ModuleType("torch._thnn")          # pac.py:20 imports torch._thnn (removed in torch>=1.0)
_stub.type2backend = defaultdict(lambda: None)
sys.modules.setdefault("torch._thnn", _stub)

from network import unet_ours as ref_net                    # noqa: E402  (reference)
import uptail_cases as tc                                   # noqa: E402
from make_golden_g27 import make_bn                         # noqa: E402

torch.set_num_threads(4)
MAX_BYTES = 131072


def main():
    manifest = {"torch": torch.__version__, "files": {}}
    torch.set_default_dtype(torch.float64)      # the reference's un-pooling allocates its one-hot weight in the default dtype
    for idx, (name, (kind, N, O, (H, W), integer)) in enumerate(tc.GOLDEN_CASES.items()):
        cat = kind.endswith("_Cat")
        rng = np.random.RandomState(2900 + idx)
        C, hc, wc = 3, (H + 1) // 2, (W + 1) // 2
        draw = (lambda *s: rng.randint(-3, 4, size=s).astype(np.float64)) if integer else (lambda *s: rng.standard_normal(s))
        x, side = draw(N, C, hc, wc), draw(N, O, H, W)
        block = getattr(ref_net, kind)(C, O, H, W).eval()
        eps = 0.5 if integer else 1e-5
        params = {}
        for conv, bn in (("conv1", "bn1"), ("sc_conv1", "sc_bn1"), ("conv1_1", "bn1_1"), ("conv2", "bn2")):
            if not hasattr(block, conv):
                continue
            c, b = getattr(block, conv), getattr(block, bn)
            w, p = draw(*c.weight.shape).astype(np.float32), make_bn(rng, O, integer)
            c.weight.data = torch.from_numpy(w).double()
            b.weight.data, b.bias.data = torch.from_numpy(p[0]).double(), torch.from_numpy(p[1]).double()
            b.running_mean.copy_(torch.from_numpy(p[2]).double())
            b.running_var.copy_(torch.from_numpy(p[3]).double())
            b.eps = eps
            params[conv], params[bn] = w, p
        with torch.no_grad():
            xt, st = torch.from_numpy(x), torch.from_numpy(side)
            u = block._up_pooling(xt, 2)
            out, shortcut = block.relu(block.bn1(block.conv1(u))), block.sc_bn1(block.sc_conv1(u))
            mid = block.relu(block.bn1_1(block.conv1_1(torch.cat((out, st), 1)))) if cat else out
            y = block(xt, st) if cat else block(xt)
        assert not block.training and tuple(y.shape) == (N, O, H, W) == tuple(out.shape), name
        out, shortcut, mid, y = (t.numpy() for t in (out, shortcut, mid, y))

        def agree(got, want):
            return np.array_equal(got, want) if integer else np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())

        if cat:
            assert agree(tc.restate(out, side, params["conv1_1"], *tc.fold(*params["bn1_1"], eps), None, True), mid), name
        assert agree(tc.restate(mid, None, params["conv2"], *tc.fold(*params["bn2"], eps), shortcut, True), y), name
        assert y.size < 20 or ((y == 0).any() and (y > 0).any()), name      # the ReLU cut something and kept something
        arrs = dict(out=out, shortcut=shortcut, w2=params["conv2"], bn2=params["bn2"], y=y, eps=np.float64(eps),
                    geom=np.array([H, W, O, int(cat)], np.int32))
        if cat:
            arrs.update(side=side, w1_1=params["conv1_1"], bn1_1=params["bn1_1"], mid=mid)
        path = os.path.join(HERE, "g29_uptail_" + name + ".npz")
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (name, size)
        manifest["files"]["g29_uptail_" + name] = {"bytes": size, "block": kind, "shape": [N, O, H, W], "integer": integer}
    with open(os.path.join(HERE, "g29_uptail_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("total bytes", sum(v["bytes"] for v in manifest["files"].values()))


if __name__ == "__main__":
    main()

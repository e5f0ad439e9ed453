#!/usr/bin/env python3
"""Golden G27 (upconv): the head of the reference's decoder blocks in eval mode, made by IMPORTING the reference.

    python tests/golden/make_golden_g27.py        (needs the reference: CSPN_REFERENCE, default /root/reference)

For every case of tests/upconv_cases.GOLDEN_CASES: one ``Gudi_UpProj_Block``, ``Gudi_UpProj_Block_Cat`` or
``Simple_Gudi_UpConv_Block`` (network/unet_ours.py:181-248) on the CPU in fp64, eval mode, with running statistics and affine
parameters that are not the initial ones, and the first lines of its forward:

    u = block._up_pooling(x, 2);  y0 = block.relu(block.bn1(block.conv1(u)));  y1 = block.sc_bn1(block.sc_conv1(u))

(the ``Simple_`` block has no shortcut and gives y0 only).  Writes g27_upconv_<case>.npz with

    x, w<k>                         the inputs (fp32 values)
    bn<k>                           [4, O]: gamma, beta, running_mean, running_var of the batch norm behind filter k (fp32 values)
    eps                             the batch norms' eps: 0.5 for the integer-valued cases (gamma in {0.5, 1, 2, -4}, variance in
                                    {0.5, 3.5, 15.5}, so variance + eps is 1, 4 or 16 and every folded scale and shift is exact in
                                    fp32), the default 1e-5 for the others
    y<k>                            the reference in fp64 (stored as fp32 for the integer-valued cases: every value is exact there)
    geom                            oh, ow, O, number of filters

Nothing is written unless tests/upconv_cases.restate agrees with the reference (exactly / to 1e-12).
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
import upconv_cases as uc                                   # noqa: E402

torch.set_num_threads(4)
MAX_BYTES = 131072


def make_bn(rng, O, integer):
    if integer:
        return np.stack([rng.choice([0.5, 1, 2, -4], size=O), rng.randint(-5, 6, size=O), rng.randint(-3, 4, size=O),
                         rng.choice([0.5, 3.5, 15.5], size=O)]).astype(np.float32)
    return np.stack([rng.standard_normal(O) + 1.5, rng.standard_normal(O), rng.standard_normal(O), rng.uniform(0.5, 2.0, size=O)]).astype(np.float32)


def reference(kind, x, ws, bns, eps, oh, ow):
    """The reference's block in fp64 (its un-pooling allocates its one-hot weight in the default dtype)."""
    torch.set_default_dtype(torch.float64)
    try:
        block = getattr(ref_net, kind)(x.shape[1], ws[0].shape[0], oh, ow).eval()
        pairs = [(block.conv1, block.bn1)] + ([(block.sc_conv1, block.sc_bn1)] if len(ws) > 1 else [])
        assert len(pairs) == len(ws) and hasattr(block, "sc_conv1") == (len(ws) > 1)
        for (conv, bn), w, p in zip(pairs, ws, bns):
            conv.weight.data = torch.from_numpy(w).double()
            bn.weight.data, bn.bias.data = torch.from_numpy(p[0]).double(), torch.from_numpy(p[1]).double()
            bn.running_mean.copy_(torch.from_numpy(p[2]).double())
            bn.running_var.copy_(torch.from_numpy(p[3]).double())
            bn.eps = eps
        with torch.no_grad():
            u = block._up_pooling(torch.from_numpy(x).double(), 2)
            ys = [block.relu(block.bn1(block.conv1(u)))]
            if len(ws) > 1:
                ys.append(block.sc_bn1(block.sc_conv1(u)))
        assert not block.training and tuple(u.shape[2:]) == (oh, ow)
        return [y.numpy() for y in ys]
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    manifest = {"torch": torch.__version__, "files": {}}
    for idx, (name, (kind, shape, (oh, ow), O, integer)) in enumerate(uc.GOLDEN_CASES.items()):
        nf = 1 if kind == "Simple_Gudi_UpConv_Block" else 2
        rng = np.random.RandomState(2700 + idx)
        x, ws, _, _ = uc.make_inputs(2700 + idx, shape, (O,) * nf, integer)
        bns = [make_bn(rng, O, integer) for _ in range(nf)]
        eps = 0.5 if integer else 1e-5
        ys = reference(kind, x, ws, bns, eps, oh, ow)
        folded = [uc.fold(*p, eps) for p in bns]
        scale, shift = np.concatenate([f[0] for f in folded]), np.concatenate([f[1] for f in folded])
        got = uc.restate(x, ws, oh, ow, scale, shift, O)
        for g, want in zip(got, ys):
            assert g.shape == want.shape == (shape[0], O, oh, ow), name
            if integer:
                assert np.array_equal(g, want) and np.array_equal(want, want.astype(np.float32)), name
            else:
                assert np.abs(g - want).max() <= 1e-12, name
        assert ys[0].size < 20 or ((ys[0] == 0).any() and (ys[0] > 0).any()), name      # the ReLU cut something and kept something
        keep = np.float32 if integer else np.float64
        arrs = dict(x=x, eps=np.float64(eps), geom=np.array([oh, ow, O, nf], np.int32))
        for k in range(nf):
            arrs.update({"w%d" % k: ws[k], "bn%d" % k: bns[k], "y%d" % k: ys[k].astype(keep)})
        path = os.path.join(HERE, "g27_upconv_" + name + ".npz")
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (name, size)
        manifest["files"]["g27_upconv_" + name] = {"bytes": size, "block": kind, "shape": list(shape), "out": [oh, ow], "out_channels": O,
                                                   "integer": integer}
    with open(os.path.join(HERE, "g27_upconv_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("total bytes", sum(v["bytes"] for v in manifest["files"].values()))


if __name__ == "__main__":
    main()

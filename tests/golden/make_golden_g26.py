#!/usr/bin/env python3
"""Golden G26 (heads): the reference's output-head block on several heads over one map, made by IMPORTING the reference.

    python tests/golden/make_golden_g26.py        (needs the reference: CSPN_REFERENCE, default /root/reference)

For every case of tests/heads_cases.GOLDEN_CASES: one ``Simple_Gudi_UpConv_Block_Last_Layer`` (network/unet_ours.py:194-202) per
head in fp64 on the same ``x``, its autograd for ``sum_h <y_h, gy_h>`` — and writes g26_heads_<case>.npz with

    x, w<h>, gy<h>                 the inputs (fp32 values)
    y<h>, gx, gw<h>                the reference in fp64 (stored as fp32 for the integer-valued cases: every value is an integer)
    y32_<h>, gx32, gw32_<h>        real-valued cases: the reference's own fp32 run
    ay<h>, agx, agw<h>             real-valued cases: the "absolute run", the same operations on |x|, |w|, |gy| in fp64

Nothing is written unless tests/heads_cases.restate agrees with the reference (exactly / to 1e-12 relative).
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
import heads_cases as hc                                    # noqa: E402

torch.set_num_threads(4)
MAX_BYTES = 550851                                          # the largest fixture committed before this one


def reference(x, ws, gys, oh, ow, dtype):
    """The reference's blocks and autograd in `dtype` (its un-pooling allocates its one-hot weight in the default dtype)."""
    torch.set_default_dtype(dtype)
    try:
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        blocks = []
        for w in ws:
            b = ref_net.Simple_Gudi_UpConv_Block_Last_Layer(x.shape[1], w.shape[0], oh, ow)
            b.conv1.weight.data = torch.from_numpy(w).to(dtype)
            blocks.append(b)
        ys = [b(xt) for b in blocks]
        sum((y * torch.from_numpy(g).to(dtype)).sum() for y, g in zip(ys, gys)).backward()
        return [y.detach().numpy() for y in ys], xt.grad.numpy(), [b.conv1.weight.grad.numpy() for b in blocks]
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    manifest = {"torch": torch.__version__, "files": {}}
    for idx, (name, (shape, (oh, ow), heads, integer)) in enumerate(hc.GOLDEN_CASES.items()):
        x, ws, gys = hc.make_inputs(2600 + idx, shape, (oh, ow), heads, integer)
        ys, gx, gws = reference(x, ws, gys, oh, ow, torch.float64)
        rys, rgx, rgws = hc.restate(x, ws, gys, oh, ow)
        for got, want in zip(rys + [rgx] + rgws, ys + [gx] + gws):
            if integer:
                assert np.array_equal(got, want), name
            else:
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name
        keep = np.float32 if integer else np.float64
        arrs = dict(x=x, gx=gx.astype(keep), geom=np.array([oh, ow] + list(heads), np.int32))
        for h in range(len(heads)):
            arrs.update({"w%d" % h: ws[h], "gy%d" % h: gys[h], "y%d" % h: ys[h].astype(keep), "gw%d" % h: gws[h].astype(keep)})
        if integer:
            assert all(np.array_equal(v, np.rint(v)) and np.abs(v).max() < 2 ** 24 for v in ys + [gx] + gws), name
        else:
            ys32, gx32, gws32 = reference(x, ws, gys, oh, ow, torch.float32)
            ays, agx, agws = reference(np.abs(x), [np.abs(w) for w in ws], [np.abs(g) for g in gys], oh, ow, torch.float64)
            arrs.update(gx32=gx32, agx=agx)
            for h in range(len(heads)):
                arrs.update({"y32_%d" % h: ys32[h], "gw32_%d" % h: gws32[h], "ay%d" % h: ays[h], "agw%d" % h: agws[h]})
        path = os.path.join(HERE, "g26_heads_" + name + ".npz")
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size <= MAX_BYTES, (name, size)
        manifest["files"]["g26_heads_" + name] = {"bytes": size, "shape": list(shape), "out": [oh, ow], "heads": list(heads),
                                                  "integer": integer}
    with open(os.path.join(HERE, "g26_heads_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("total bytes", sum(v["bytes"] for v in manifest["files"].values()))


if __name__ == "__main__":
    main()

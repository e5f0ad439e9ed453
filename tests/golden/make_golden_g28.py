#!/usr/bin/env python3
"""Golden G28 (upgrad): the gradients of the head of the reference's decoder blocks in train() mode, made by IMPORTING the reference.

    python tests/golden/make_golden_g28.py        (needs the reference: CSPN_REFERENCE, default /root/reference)

For every case of tests/upconv_cases.GOLDEN_CASES: one ``Gudi_UpProj_Block``, ``Gudi_UpProj_Block_Cat`` or
``Simple_Gudi_UpConv_Block`` (network/unet_ours.py:181-248) on the CPU in fp64, train() mode, the first lines of its forward

    u = block._up_pooling(x, 2);  a0 = block.conv1(u);  a1 = block.sc_conv1(u)

(the ``Simple_`` block has no shortcut and gives a0 only) and torch.autograd.grad of sum(a0 g0) + sum(a1 g1).  Writes
g28_upgrad_<case>.npz with

    x, w<k>, g<k>                   the inputs and the given cotangents (fp32 values)
    gx, gw<k>                       the reference's gradients in fp64 (stored as fp32 for the integer-valued cases: exact there)
    geom                            oh, ow, O, number of filters

and, for the cases of BLOCK_CASES, g28_upgrad_block_<case>.npz: the whole block in train() mode on that x with conv1 / sc_conv1
holding w0 / w1 and every other parameter drawn here,

    p_<name>                        every parameter of the block (fp32 values), <name> as in its state_dict
    side, cot                       the encoder skip (``_Cat`` only) and the cotangent of the block's output (fp32 values)
    out                             the block's output (fp64)
    rm_<bn>, rv_<bn>                running_mean / running_var of every batch norm after that one forward (fp64)
    gx, g_<name>                    the gradients of x and of every parameter (fp64)

Nothing is written unless tests/upgrad_cases.restate agrees with the reference (exactly / to 1e-12).
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
import upgrad_cases as ug                                   # noqa: E402

torch.set_num_threads(4)
MAX_BYTES = 131072
BLOCK_CASES = ("real_5x7", "real_deep_crop", "real_simple")      # one per block class


def head_reference(kind, x, ws, gys, oh, ow):
    torch.set_default_dtype(torch.float64)
    try:
        block = getattr(ref_net, kind)(x.shape[1], ws[0].shape[0], oh, ow).train()
        convs = [block.conv1] + ([block.sc_conv1] if len(ws) > 1 else [])
        assert hasattr(block, "sc_conv1") == (len(ws) > 1) and block.training
        for conv, w in zip(convs, ws):
            conv.weight.data = torch.from_numpy(w).double()
        xt = torch.from_numpy(x).double().requires_grad_(True)
        u = block._up_pooling(xt, 2)
        assert tuple(u.shape[2:]) == (oh, ow)
        loss = sum((conv(u) * torch.from_numpy(g).double()).sum() for conv, g in zip(convs, gys))
        grads = torch.autograd.grad(loss, [xt] + [c.weight for c in convs])
        return grads[0].numpy(), [g.numpy() for g in grads[1:]]
    finally:
        torch.set_default_dtype(torch.float32)


def block_reference(kind, x, ws, oh, ow, seed):
    """The whole block in train() mode, fp64: what it was given, what it returned and every gradient."""
    rng = np.random.RandomState(seed)
    torch.set_default_dtype(torch.float64)
    try:
        O = ws[0].shape[0]
        block = getattr(ref_net, kind)(x.shape[1], O, oh, ow).train()
        params = {}
        for name, p in block.named_parameters():
            if name == "conv1.weight":
                v = ws[0]
            elif name == "sc_conv1.weight":
                v = ws[1]
            elif p.dim() == 4:
                v = (rng.standard_normal(tuple(p.shape)) * 0.3).astype(np.float32)
            elif name.endswith("weight"):
                v = (1.0 + 0.2 * rng.standard_normal(tuple(p.shape))).astype(np.float32)
            else:
                v = (0.1 * rng.standard_normal(tuple(p.shape))).astype(np.float32)
            params[name] = v
            p.data = torch.from_numpy(v).double()
        arrs = {"p_" + n: v for n, v in params.items()}
        xt = torch.from_numpy(x).double().requires_grad_(True)
        args = [xt]
        if kind == "Gudi_UpProj_Block_Cat":
            arrs["side"] = rng.standard_normal((x.shape[0], O, oh, ow)).astype(np.float32)
            args.append(torch.from_numpy(arrs["side"]).double())
        out = block(*args)
        arrs["cot"] = rng.standard_normal(tuple(out.shape)).astype(np.float32)
        named = list(block.named_parameters())
        grads = torch.autograd.grad((out * torch.from_numpy(arrs["cot"]).double()).sum(), [xt] + [p for _, p in named])
        arrs["out"], arrs["gx"] = out.detach().numpy(), grads[0].numpy()
        for (n, _), g in zip(named, grads[1:]):
            arrs["g_" + n] = g.numpy()
        for n, m in block.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                assert m.momentum == 0.1 and m.eps == 1e-5 and int(m.num_batches_tracked) == 1
                arrs["rm_" + n], arrs["rv_" + n] = m.running_mean.numpy().copy(), m.running_var.numpy().copy()
        assert (arrs["out"] == 0).any() and (arrs["out"] > 0).any()
        return arrs
    finally:
        torch.set_default_dtype(torch.float32)


def save(manifest, stem, arrs, **facts):
    path = os.path.join(HERE, stem + ".npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (stem, size)
    manifest["files"][stem] = dict(bytes=size, **facts)


def main():
    manifest = {"torch": torch.__version__, "files": {}}
    for idx, (name, (kind, shape, (oh, ow), O, integer)) in enumerate(uc.GOLDEN_CASES.items()):
        nf = 1 if kind == "Simple_Gudi_UpConv_Block" else 2
        x, ws, _, _ = uc.make_inputs(2800 + idx, shape, (O,) * nf, integer)
        gys = ug.make_cotangents(2800 + idx, shape, (O,) * nf, (oh, ow), integer)
        gx, gws = head_reference(kind, x, ws, gys, oh, ow)
        rx, rws = ug.restate(x, ws, gys, (oh, ow))
        for got, want in zip([rx] + rws, [gx] + gws):
            assert got.shape == want.shape, name
            if integer:
                assert np.array_equal(got, want) and np.array_equal(want, want.astype(np.float32)), name
            else:
                assert np.abs(got - want).max() <= 1e-12, name
        keep = np.float32 if integer else np.float64
        arrs = dict(x=x, gx=gx.astype(keep), geom=np.array([oh, ow, O, nf], np.int32))
        for k in range(nf):
            arrs.update({"w%d" % k: ws[k], "g%d" % k: gys[k], "gw%d" % k: gws[k].astype(keep)})
        save(manifest, "g28_upgrad_" + name, arrs, block=kind, shape=list(shape), out=[oh, ow], out_channels=O, integer=integer)
        if name in BLOCK_CASES:
            save(manifest, "g28_upgrad_block_" + name, block_reference(kind, x, ws, oh, ow, 2850 + idx), block=kind, shape=list(shape),
                 out=[oh, ow], out_channels=O, whole_block=True)
    assert {uc.GOLDEN_CASES[n][0] for n in BLOCK_CASES} == {"Gudi_UpProj_Block", "Gudi_UpProj_Block_Cat", "Simple_Gudi_UpConv_Block"}
    with open(os.path.join(HERE, "g28_upgrad_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("total bytes", sum(v["bytes"] for v in manifest["files"].values()))


if __name__ == "__main__":
    main()

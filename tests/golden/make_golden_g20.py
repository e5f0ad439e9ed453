"""Golden G20: In-Place Activated BatchNorm (network/libs/inplace_abn of the reference), forward and backward.

The reference's native extension cannot be built (nvcc, THC, torch.utils.ffi), its Python can run.  This maker imports the
reference's own `bn.InPlaceABN` module and `functions.InPlaceABN` autograd function (CSPN_REFERENCE, default /root/reference —
nothing of it is copied) with three arrangements:
  * empty `network`, `network.libs` and `network.libs.inplace_abn` packages whose `__path__` points into the reference, so that
    their `__init__` files (which import the whole model zoo) do not run;
  * `collections.Iterable = collections.abc.Iterable` (bn.py:1 predates Python 3.10);
  * a stub `network.libs.inplace_abn._ext` in sys.modules whose entry points are fp32 torch statements of the C signatures in
    src/bn.h — same operand order, same in-place outputs, the arithmetic of src/bn.cu:125-232, :302-377 in fp32 tensors.
The module then runs forward and backward on the CPU in fp32 for every case of tests/abn_cases.CASES and the maker writes
g20_abn_<case>.npz: the case's parameters, the reference's out / dx / dweight / dbias / running statistics (out and dx of the
three big cases as every 97th element — the test regenerates the inputs from the seed).

Asserted before anything is written, following the G18 maker:
  1. the reference's fp32 run sits within 2e-6 of tests/abn_cases.restate (fp64, independent: it never inverts anything), every
     field measured against its largest magnitude (dx of a zero-weight channel: abn_cases.zero_channel_dx_bar, dweight there
     exactly 0).  The distances go into the manifest.  The device is held to 1e-5 against these numbers;
  2. an elu case has no pre-activation below -4;
  3. no pre-activation of a leaky_relu case is within 1e-6 of 0 relative to the largest: the slope jumps there, and an fp32
     pre-activation is a few 2^-24 of the largest away from the fp64 one (elu and its slope are continuous at 0).
The OFFSET: the channel means of the `offset` cases sit `offset` standard deviations from 0.  The maker tries the powers of two
from 2^12 down and keeps the largest at which condition 1 still holds for the reference's own fp32 arithmetic in both; it is recorded
in the manifest and in the cases' files.

`backward` is given a COPY of the cotangent and the output is copied before it: the reference scales the one and overwrites the
other in place (functions.py:54-60)."""
import collections
import collections.abc
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CSPN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import abn_cases as ac                                       # noqa: E402


# ------------------------------------------------------------------------------------------------ the stub extension
def _ncs(x):
    return x.size(0), x.size(1), int(x.numel() // (x.size(0) * x.size(1)))


def _opt(t, c, fill):
    return t.view(1, c, 1) if t.numel() else torch.full((1, c, 1), fill, dtype=torch.float32)


def _gamma_beta(weight, bias, c, eps):
    return (weight.abs().view(1, c, 1) + eps) if weight.numel() else torch.ones(1, c, 1), _opt(bias, c, 0.0)


def _invstd(var, eps):
    return torch.where((var != 0) | torch.tensor(eps != 0), 1 / torch.sqrt(var + eps), torch.zeros_like(var))


def bn_mean_var_cuda(x, mean, var):
    n, c, s = _ncs(x)
    x3 = x.view(n, c, s)
    m = x3.sum(2).sum(0) * (1.0 / (n * s))
    v = ((x3 - m.view(1, c, 1)) ** 2).sum(2).sum(0) * (1.0 / (n * s))
    mean.view(-1).copy_(m)
    var.view(-1).copy_(v)
    return True


def bn_forward_cuda(x, mean, var, weight, bias, y, z, eps):
    n, c, s = _ncs(x)
    gamma, beta = _gamma_beta(weight, bias, c, eps)
    yy = (x.view(n, c, s) - mean.view(1, c, 1)) * _invstd(var.view(1, c, 1), eps)
    zz = yy * gamma + beta
    y.view(n, c, s).copy_(yy)
    z.view(n, c, s).copy_(zz)
    return True


def bn_edz_eydz_cuda(z, dz, weight, bias, edz, eydz, eps):
    n, c, s = _ncs(z)
    gamma, beta = _gamma_beta(weight, bias, c, eps)
    y = (z.view(n, c, s) - beta) / gamma
    d = dz.view(n, c, s)
    edz.view(-1).copy_(d.sum(2).sum(0) * (1.0 / (n * s)))
    eydz.view(-1).copy_((y * d).sum(2).sum(0) * (1.0 / (n * s)))
    return True


def bn_backard_cuda(dz, z, var, weight, bias, edz, eydz, dx, dweight, dbias, eps):
    n, c, s = _ncs(z)
    gamma, beta = _gamma_beta(weight, bias, c, eps)
    if dx.numel():
        y = (z.view(n, c, s) - beta) / gamma
        mul = gamma * _invstd(var.view(1, c, 1), eps)
        dx.view(n, c, s).copy_((dz.view(n, c, s) - edz.view(1, c, 1) - y * eydz.view(1, c, 1)) * mul)
    norm = float(n * s)
    if dweight.numel():
        dweight.add_(torch.sign(weight) * (eydz.view(-1) * norm))
    if dbias.numel():
        dbias.add_(edz.view(-1) * norm)
    return True


def leaky_relu_cuda(x, slope):
    x.copy_(torch.where(x < 0, x * slope, x))
    return True


def leaky_relu_backward_cuda(x, dx, slope):
    dx.copy_(torch.where(x < 0, dx * slope, dx))
    return True


def elu_cuda(x):
    x.copy_(torch.where(x < 0, torch.exp(x) - 1.0, x))
    return True


def elu_backward_cuda(x, dx):
    dx.copy_(torch.where(x < 0, dx * (x + 1.0), dx))
    return True


def elu_inv_cuda(x):
    x.copy_(torch.where(x < 0, torch.log1p(x), x))
    return True


def import_reference():
    collections.Iterable = collections.abc.Iterable
    for name, rel in (("network", "network"), ("network.libs", "network/libs"), ("network.libs.inplace_abn", "network/libs/inplace_abn")):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, rel)]
        sys.modules[name] = pkg
    ext = types.ModuleType("network.libs.inplace_abn._ext")
    for fn in (bn_mean_var_cuda, bn_forward_cuda, bn_edz_eydz_cuda, bn_backard_cuda, leaky_relu_cuda, leaky_relu_backward_cuda,
               elu_cuda, elu_backward_cuda, elu_inv_cuda):
        setattr(ext, fn.__name__, fn)
    ext.bn_backward_cuda = bn_backard_cuda                  # the name the C header spells correctly
    sys.modules[ext.__name__] = ext
    sys.modules["network.libs.inplace_abn"]._ext = ext
    import importlib
    return importlib.import_module("network.libs.inplace_abn.bn")


# ------------------------------------------------------------------------------------------------ the runs
torch.set_num_threads(4)
manifest = {"files": {}, "cases": {}}


def reference(bn, case, inp):
    """The reference's module on the CPU in fp32: dict of abn_cases.FIELDS."""
    c = case["shape"][1]
    mod = bn.InPlaceABN(c, eps=case["eps"], momentum=case["momentum"], affine=case["affine"], activation=case["activation"],
                        slope=case["slope"])
    with torch.no_grad():
        if case["affine"]:
            mod.weight.copy_(torch.from_numpy(inp["weight"]))
            mod.bias.copy_(torch.from_numpy(inp["bias"]))
        mod.running_mean.copy_(torch.from_numpy(inp["running_mean"]))
        mod.running_var.copy_(torch.from_numpy(inp["running_var"]))
    mod.train(case["training"])
    leaf = torch.from_numpy(inp["x"].copy()).requires_grad_(True)
    out = mod(leaf * 1.0)                                   # the module writes in place: not on the leaf
    res = dict(out=out.detach().clone().numpy())            # before backward overwrites it
    out.backward(torch.from_numpy(inp["cot"]).clone())      # ... and scales its cotangent
    res.update(dx=leaf.grad.numpy(), dweight=mod.weight.grad.numpy() if case["affine"] else None,
               dbias=mod.bias.grad.numpy() if case["affine"] else None, running_mean=mod.running_mean.numpy().copy(),
               running_var=mod.running_var.numpy().copy())
    return res


def measure(bn, case, offset):
    inp = ac.make_inputs(case, offset)
    got, want = reference(bn, case, inp), ac.restate_case(case, inp)
    errs = ac.compare(got, want, inp["weight"], ac.ORACLE_BAR, case["eps"])
    return inp, got, want, errs


def check_inputs(name, case, want):
    pre = want["pre"]
    if case["activation"] == "elu":
        assert pre.min() >= -4.0, (name, float(pre.min()))
    if case["activation"] == "leaky_relu":
        assert np.abs(pre).min() >= 1e-6 * np.abs(pre).max(), (name, float(np.abs(pre).min()))


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: v for k, v in arrs.items() if v is not None})
    manifest["files"][name] = {"bytes": os.path.getsize(path), "arrays": {k: list(np.shape(v)) for k, v in arrs.items() if v is not None}}
    assert os.path.getsize(path) <= ac.MAX_FILE_BYTES, (name, os.path.getsize(path))


def find_offset(bn):
    """The largest power of two at which the reference's fp32 run of EVERY offset case (the small one and the one with 17 328
    values per channel, whose fp32 mean has more additions behind it) still passes condition 1."""
    tried = {}
    for k in range(12, -1, -1):
        off = float(2 ** k)
        worst = max(max(measure(bn, case, off)[3].values()) for name, case in ac.CASES.items() if "offset" in name)
        tried[str(off)] = worst * ac.ORACLE_BAR
        if worst <= 1.0:
            manifest["offset"] = {"chosen": off, "worst_reference_vs_fp64_by_offset": tried}
            return off
    raise AssertionError(tried)


if __name__ == "__main__":
    bn = import_reference()
    offset = find_offset(bn)
    for name, case in ac.CASES.items():
        off = offset if "offset" in name else 0.0
        inp, got, want, errs = measure(bn, case, off)
        check_inputs(name, case, want)
        assert max(errs.values()) <= 1.0, (name, {k: v * ac.ORACLE_BAR for k, v in errs.items()})
        for ch in ac.zero_channels(inp["weight"]):
            assert got["dweight"][ch] == 0.0
        manifest["cases"][name] = {"reference_vs_fp64": {k: v * ac.ORACLE_BAR for k, v in errs.items()}, "offset": off,
                                   "shape": list(case["shape"]), "min_pre_activation": float(want["pre"].min()),
                                   "channel_mean_over_std_max": float(np.abs(inp["x"].astype(np.float64).reshape(ac.ncs(case["shape"])).mean(axis=(0, 2))
                                                                             * want["invstd"]).max()) if case["training"] else None}
        meta = dict(shape=np.array(case["shape"], np.int64), seed=np.int64(case["seed"]), offset=np.float64(off),
                    activation=np.array(case["activation"]), training=np.bool_(case["training"]), affine=np.bool_(case["affine"]),
                    momentum=np.float64(case["momentum"]), eps=np.float64(case["eps"]), slope=np.float64(case["slope"]))
        if case["full"]:
            save("g20_abn_" + name, out_sub=got["out"].reshape(-1)[::ac.FULL_STRIDE].copy(), dx_sub=got["dx"].reshape(-1)[::ac.FULL_STRIDE].copy(),
                 stride=np.int64(ac.FULL_STRIDE), out_absmax=np.float64(np.abs(got["out"]).max()), dx_absmax=np.float64(np.abs(got["dx"]).max()),
                 dweight=got["dweight"], dbias=got["dbias"], running_mean=got["running_mean"], running_var=got["running_var"], **meta)
        else:
            save("g20_abn_" + name, x=inp["x"], cot=inp["cot"], weight=inp["weight"], bias=inp["bias"], running_mean_in=inp["running_mean"],
                 running_var_in=inp["running_var"], out=got["out"], dx=got["dx"], dweight=got["dweight"], dbias=got["dbias"],
                 running_mean=got["running_mean"], running_var=got["running_var"], **meta)
    manifest["torch"] = torch.__version__
    manifest["numpy"] = np.__version__
    with open(os.path.join(HERE, "golden_g20_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest["cases"], indent=1, sort_keys=True))
    print(json.dumps(manifest["offset"], indent=1, sort_keys=True))

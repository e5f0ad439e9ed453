#!/usr/bin/env python3
"""Golden vectors G16, made by IMPORTING the reference.  Build container only (needs the reference tree):

    CSPN_REFERENCE=/path/to/reference python tests/golden/make_golden_g16.py

G16 extends G15 (make_golden_r06.py: one frame) to an external anchor for config 3's fp16 paths PER FRAME, per input regime and for
the gradients.  Every input comes from the hash generators of oracle/cspn_oracle.py; every seed, scale and shape is stored, so the
tests rebuild the inputs themselves.  Each case goes through the reference's CSPN_ours.AffinityPropagate (CSPN_ours.py:24-54) twice,
as G15 does:
  * `taps16`: half inputs under the default dtype float32 (fp16 softmax taps, fp32 state: CSPN_ours.py:37's zeros are fp32), and
  * `half`:   the same call under torch.set_default_dtype(float16) (taps, state and every step's sums in half),
and the fixture records each run's distance from the fp32 oracle on the same fp16-rounded inputs as (max / scale, rmse / scale),
scale = max |oracle| (per frame where the record is per frame).

G16a  config 3's full batch: B = 24 distinct 228 x 304 frames, K = 5, T = 12, without / with sparse depth; distances per frame, and
      the `half` output of frames 0 and 13 (one from each 12-frame round of the one-launch kernel) in fp16.
G16b  input regimes on shapes the dot-product kernel (cspnk_d2) runs, i.e. kres_plan(...)["quads_per_thread"] == 1: guidance x 8
      (peaky softmax, small taps reach fp16 subnormals), guidance x 0.05 (near-uniform taps), a KITTI depth range (0-85), and one
      guidance channel at +30 on a tenth of the pixels (saturated softmax); full outputs of both runs.
G16c  gradients: the reference's half autograd through its differentiable branch (pac.conv2d(native_impl=True), pac.py:130-140,
      forced on here only: Conv2dFn.backward needs the THNN backend torch removed) with a fixed fp16 cotangent; the distances of
      dL/dx and dL/dguided from oracle.pac_backward(..., np.float64) for both runs.  Statistics only.  Under native_impl the
      in-place `im_cols *= kernel` (pac.py:137) keeps the dtype of the half input columns, so the `taps16` run's state stays half
      as well there; its gradients still differ from the `half` run's (fp32 taps through the softmax backward).
"""
import functools
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
sys.path.insert(0, REF)
_stub = types.ModuleType("torch._thnn")          # pac.py:20 imports torch._thnn (removed in torch>=1.0)
_stub.type2backend = defaultdict(lambda: None)
sys.modules.setdefault("torch._thnn", _stub)

from network.libs.base import pac as ref_pac                # noqa: E402  (reference)
from network.libs.post_process import CSPN_ours             # noqa: E402  (reference)
from oracle import cspn_oracle as orc                       # noqa: E402

torch.set_num_threads(4)
K = 5
RUNS = (("taps16", torch.float32), ("half", torch.float16))


def make_inputs(seed, B, H, W, g_scale=1.0, x_hi=10.0, sparse_rate=0.0, hot=None):
    """fp16-rounded (guidance, x, sparse or None): oracle.cspn_oracle.fp16_case_inputs, which the tests call with the stored values."""
    return orc.fp16_case_inputs(seed, B, H, W, K, g_scale, x_hi, sparse_rate, hot)


def f32(a):
    return None if a is None else a.astype(np.float32)


def dist(o, want, axes=None):
    """(max |o - want| / scale, rmse / scale); per frame when axes are given."""
    o, want = np.asarray(o, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(axis=axes)
    return np.abs(o - want).max(axis=axes) / scale, np.sqrt(((o - want) ** 2).mean(axis=axes)) / scale


def ref_forward(gd, x, sp, T):
    m = CSPN_ours.AffinityPropagate(T)
    outs = {}
    for name, dd in RUNS:
        torch.set_default_dtype(dd)
        try:
            with torch.no_grad():
                outs[name] = m(torch.from_numpy(x), torch.from_numpy(gd), None if sp is None else torch.from_numpy(sp))
        finally:
            torch.set_default_dtype(torch.float32)
    assert outs["taps16"].dtype == torch.float32 and outs["half"].dtype == torch.float16
    return {k: v.numpy() for k, v in outs.items()}


def case_meta(seed, B, H, W, T, g_scale, x_hi, sparse_rate, hot):
    return dict(seed=np.int32(seed), T=np.int32(T), K=np.int32(K), shape=np.array([B, H, W], np.int32), g_scale=np.float64(g_scale),
                x_hi=np.float64(x_hi), sparse_rate=np.float64(sparse_rate),
                hot=np.array([-1, 0.0, 0.0] if hot is None else list(hot), np.float64))


manifest = {"torch": torch.__version__, "g16a": {}, "g16b": {}, "g16c": {}}

# ------------------------------------------------------------------------------------------------ G16a: config 3, 24 frames
B, H, W, T, SEED = 24, 228, 304, 12, 46
FRAMES = np.array([0, 13], np.int32)
for tag, rate in (("nosp", 0.0), ("sp", 500.0 / (H * W))):
    gd, x, sp = make_inputs(SEED, B, H, W, sparse_rate=rate)
    outs = ref_forward(gd, x, sp, T)
    want = orc.pac_forward(f32(x), f32(gd), f32(sp), T)
    err = {name: np.stack(dist(outs[name], want, axes=(1, 2, 3)), axis=1) for name, _ in RUNS}
    name = "g16a_k5_t12_fp16_b24_%s" % tag
    np.savez_compressed(os.path.join(HERE, name + ".npz"), frames=FRAMES, out_half_frames=outs["half"][FRAMES],
                        ref_err_taps16=err["taps16"], ref_err_half=err["half"], **case_meta(SEED, B, H, W, T, 1.0, 10.0, rate, None))
    manifest["g16a"][name] = {r: {"max_over_scale_worst": float(err[r][:, 0].max()), "rmse_over_scale_worst": float(err[r][:, 1].max())}
                              for r, _ in RUNS}

# ------------------------------------------------------------------------------------------------ G16b: input regimes
REGIMES = [  # name, seed, (B, H, W), T, guidance scale, x range, hot channel
    ("peaky", 47, (2, 40, 64), 12, 8.0, 10.0, None),
    ("flat", 48, (2, 40, 64), 12, 0.05, 10.0, None),
    ("kitti", 49, (5, 60, 72), 12, 1.0, 85.0, None),
    ("saturated", 50, (5, 60, 72), 12, 1.0, 10.0, (7, 30.0, 0.1)),
]
for reg, seed, (b, h, w), t, gs, xhi, hot in REGIMES:
    for tag, rate in (("nosp", 0.0), ("sp", max(500.0 / (h * w), 0.02))):
        gd, x, sp = make_inputs(seed, b, h, w, gs, xhi, rate, hot)
        outs = ref_forward(gd, x, sp, t)
        want = orc.pac_forward(f32(x), f32(gd), f32(sp), t)
        err = {name: np.array(dist(outs[name], want)) for name, _ in RUNS}
        name = "g16b_%s_%s" % (reg, tag)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), out_taps16=outs["taps16"].astype(np.float32), out_half=outs["half"],
                            ref_err_taps16=err["taps16"], ref_err_half=err["half"], **case_meta(seed, b, h, w, t, gs, xhi, rate, hot))
        manifest["g16b"][name] = {r: {"max_over_scale": float(err[r][0]), "rmse_over_scale": float(err[r][1])} for r, _ in RUNS}

# ------------------------------------------------------------------------------------------------ G16c: gradients
GRADS = [(52, (3, 228, 304), 12), (53, (2, 40, 64), 6)]
orig_conv2d = ref_pac.conv2d
ref_pac.conv2d = functools.partial(orig_conv2d, native_impl=True)      # CSPN_ours imports conv2d from the module at every step
try:
    for seed, (b, h, w), t in GRADS:
        for tag, rate in (("nosp", 0.0), ("sp", max(500.0 / (h * w), 0.02))):
            gd, x, sp = make_inputs(seed, b, h, w, sparse_rate=rate)
            cot = orc.hash_normal(seed, 9, (b, 1, h, w)).astype(np.float16)
            wx, wg = orc.pac_backward(f32(x), f32(gd), f32(sp), f32(cot), t, np.float64)
            m = CSPN_ours.AffinityPropagate(t)
            errs = {}
            for name, dd in RUNS:
                torch.set_default_dtype(dd)
                try:
                    xt = torch.from_numpy(x).requires_grad_(True)
                    gt = torch.from_numpy(gd).requires_grad_(True)
                    out = m(xt, gt, None if sp is None else torch.from_numpy(sp))
                    out.backward(torch.from_numpy(cot).to(out.dtype))
                finally:
                    torch.set_default_dtype(torch.float32)
                assert xt.grad.dtype == gt.grad.dtype == torch.float16
                errs[name] = np.array([dist(xt.grad.float().numpy(), wx), dist(gt.grad.float().numpy(), wg)])   # [dx | dguided][max | rmse]
            name = "g16c_grad_%dx%dx%d_t%d_%s" % (b, h, w, t, tag)
            np.savez_compressed(os.path.join(HERE, name + ".npz"), ref_grad_err_taps16=errs["taps16"], ref_grad_err_half=errs["half"],
                                **case_meta(seed, b, h, w, t, 1.0, 10.0, rate, None))
            manifest["g16c"][name] = {r: {"dx": errs[r][0].tolist(), "dguided": errs[r][1].tolist()} for r, _ in RUNS}
finally:
    ref_pac.conv2d = orig_conv2d

json.dump(manifest, open(os.path.join(HERE, "golden_g16_manifest.json"), "w"), indent=1)
print(json.dumps(manifest, indent=1))

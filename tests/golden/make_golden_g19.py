"""Golden G19: the original CSPN release's module, network/libs/post_process/CSPN.py — AffinityPropagate (sparse blend) and
AffinityPropagate_prediction (none) — forward and, for the small cases, autograd.

Imports the reference's CSPN.py from its file (CSPN_REFERENCE names the reference checkout) — nothing of it is copied — and runs
every case of tests/max8_cases.golden_cases() through it on the CPU in fp32.  The file calls `.cuda()` on its ones-kernels, so
this process makes torch.Tensor.cuda the identity; its loop count is the literal 16, so the prop_time cases give the module a
`range` of their own length.  Writes g19_max8_<case>.npz with OUTPUTS only (out, and grad_guidance / grad_blur / gap for the
autograd cases) plus the seed: the tests regenerate the inputs with tests/max8_cases.

Asserted before anything is written:
  1. the reference's fp32 result agrees with the fp64 restatement (tests/max8_cases.restate) to 2e-6, NaN position for position;
     gradients measured against their largest magnitude;
  2. autograd cases: the seed is searched until the fp64 run's smallest top-two relative gap over all pixel-steps is >= 1e-5 —
     the fp32 reference then selects as fp64 does (about one seed in fifty qualifies at these sizes); the gap is stored;
  3. the seeds of the device tests' large shapes (max8_cases.BIG_SEEDS) exclude at most 1 % of their pixel-steps at that gap.
"""
import builtins
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["CSPN_REFERENCE"]
sys.path.insert(0, os.path.join(ROOT, "tests"))

import max8_cases as mc                                      # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self               # the reference's ones-kernels stay on the CPU
spec = importlib.util.spec_from_file_location("ref_cspn", os.path.join(REF, "network", "libs", "post_process", "CSPN.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

torch.set_num_threads(4)
LIMIT = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and not f.startswith("g19_"))
manifest = {}


def run_reference(g, d, s, T, cot):
    ref.range = lambda n: builtins.range(T)                  # CSPN.py:36, :146 loop over the literal 16
    gt, dt = torch.from_numpy(g).requires_grad_(cot is not None), torch.from_numpy(d).requires_grad_(cot is not None)
    if s is not None:
        out = ref.AffinityPropagate()(gt, dt, torch.from_numpy(s))
    else:
        out = ref.AffinityPropagate_prediction()(gt, dt)
    res = dict(out=out.detach().numpy())
    if cot is not None:
        out.backward(torch.from_numpy(cot))
        res.update(grad_guidance=gt.grad.numpy(), grad_blur=dt.grad.numpy())
    return res


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    fin = np.isfinite(got) & np.isfinite(want)
    return float((np.abs(got - want)[fin] / np.maximum(np.abs(want[fin]), 1e-6)).max()) if fin.any() else 0.0


def main():
    seed = 1910
    for name, (kind, shape, sp, T, with_grad) in mc.golden_cases().items():
        while True:
            seed += 1
            g, d, s = mc.special_inputs(kind, seed, shape, sp)
            cot = mc.make_cotangent(seed, shape) if with_grad else None
            want = mc.restate(g, d, s, T, cot)
            gap = float(np.nanmin(want["gap"])) if np.isfinite(want["gap"]).any() else float("inf")
            if not with_grad or gap >= mc.GAP_BAR:
                break
        got = run_reference(g, d, s, T, cot)
        errs = dict(out=rel_err(got["out"], want["out"]))
        arrs = dict(out=got["out"], seed=np.int64(seed), T=np.int64(T))
        if with_grad:
            for k in ("grad_guidance", "grad_blur"):
                errs[k] = mc.grad_err(got[k], want[k])
                arrs[k] = got[k]
            arrs["gap"] = np.float64(gap)
        print("%-28s seed %d  %s" % (name, seed, "  ".join("%s %.2e" % kv for kv in errs.items())), flush=True)
        assert max(errs.values()) <= mc.ORACLE_BAR, (name, errs)
        path = os.path.join(HERE, "g19_max8_%s.npz" % name)
        np.savez_compressed(path, **arrs)
        assert os.path.getsize(path) <= LIMIT, (name, os.path.getsize(path))
        manifest[name] = dict(seed=seed, bytes=os.path.getsize(path), nan=int(np.isnan(got["out"]).sum()), **errs)
    for shape, bseed in mc.BIG_SEEDS.items():
        for sp in (True, False):
            g, d, s = mc.make_inputs(bseed, shape, sp)
            for T in (16, 5):
                share = mc.excluded_share(mc.restate(g, d, s, T)["gap"])
                print("big %s sparse=%d T=%d: %.3f %% of the pixel-steps excluded" % (mc.shape_tag(shape), sp, T, 100 * share))
                assert share <= mc.EXCLUDED_CAP
                manifest["big_%s_%s_t%d" % (mc.shape_tag(shape), "sp" if sp else "nosp", T)] = dict(seed=bseed, excluded=share)
    print(json.dumps(manifest, indent=1))


if __name__ == "__main__":
    main()

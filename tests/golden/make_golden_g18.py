"""Golden G18: the training criteria get_criteria offers (libs/criterion: l1 -> MaskedL1Loss, l2 -> MaskedMSELoss,
l1_log -> L1_log, wrapped by Criterion_No_DSN / CriterionDSN), forward and backward.

Imports the reference (CSPN_REFERENCE, default /root/reference) — nothing of it is copied — runs every case through it on the
CPU in fp32 with autograd and writes g18_criterion_<case>.npz:

  <kind>_<shape>_g10 / _g04   shapes 1 (1,1,1,1), 3x5 (1,1,3,5), 3x57x77 (3,1,57,77: 13 167 elements, odd), the incoming gradient
                              of the loss 1 or 0.4 (the reference run is (0.4 * loss).backward()): pred, target, loss, grad
  <kind>_ties                 10 % of the pixels have pred == target bit for bit (term 0, gradient 0)
  <kind>_empty                no pixel has target > 0: loss NaN, gradient all 0
  l1_log_pred_zero / _neg     a valid pixel with pred == 0 (loss Inf, gradient -inf there) / pred < 0 (loss NaN, gradient 0 there)
  dsn_l1                      CriterionDSN(MaskedL1Loss): target 2x1x8x12, predictions 8x12 and 4x6 -> loss, both gradients
  <kind>_full                 24x1x228x304: the seed, the loss and every 997th gradient element (the test regenerates the inputs)

Inputs: tests/criterion_cases.make_inputs (the oracle's hash generator; every seed and shape is stored).  Three conditions are
asserted before anything is written:
  1. the reference's fp32 loss and gradient agree with the fp64 numpy restatement (tests/criterion_cases.restate) to 2e-6 — the
     gradient measured against its largest magnitude, NaN / +-Inf position for position.  The tests hold the device to 1e-5
     against these numbers; that bar means something only if the reference's own arithmetic sits well inside it;
  2. for every l1_log case with a finite loss, the worst rounding of the logarithms to fp32 moves the loss by less than 2e-6
     (a single pixel with pred within a few percent of target would not do: |log t - log p| cancels).  The seeds of the three
     shapes (182, 181, 180) were picked so that the 1-pixel case is a valid pixel and passes this: another seed may not;
  3. for every case, each valid pixel has pred == target exactly or |pred / target - 1| >= 1e-3: at a near-tie the sign of
     log t - log p can differ between fp32 and fp64, and the gradient of that pixel with it (one such pixel in unconstrained
     random inputs at full size: 6e-3 of the largest gradient).  With the constraint no pixel needs excluding.
"""
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
sys.path.insert(0, REF)

_stub = types.ModuleType("libs.image_processor")     # criteria.py:11 imports a module the reference does not ship
_stub.sobel_filter = None
sys.modules.setdefault("libs.image_processor", _stub)

from libs import criterion as ref_criterion                 # noqa: E402  (reference)
import criterion_cases as cc                                # noqa: E402

torch.set_num_threads(4)
manifest = {"files": {}, "cases": {}}
SHAPES = (("1", (1, 1, 1, 1)), ("3x5", (1, 1, 3, 5)), ("3x57x77", (3, 1, 57, 77)))


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    manifest["files"][name] = {"bytes": os.path.getsize(path), "arrays": {k: list(np.shape(v)) for k, v in arrs.items()}}
    assert os.path.getsize(path) <= 580000, (name, os.path.getsize(path))


def args(kind, wrapper):
    return types.SimpleNamespace(criterion=kind, loss_wrapper=wrapper, arch="g18")


def reference(kind, pred, target, g):
    """The reference on the CPU in fp32: loss and d (g * loss) / d pred."""
    p = torch.from_numpy(pred).requires_grad_(True)
    loss = ref_criterion.get_criteria(args(kind, "no_dsn"))([p], torch.from_numpy(target))
    (loss if g == 1.0 else loss * g).backward()
    return float(loss.detach()), p.grad.numpy()


def check(case, kind, pred, target, g, loss, grad):
    assert cc.no_tie_ok(pred, target), case
    if kind == "l1_log" and np.isfinite(loss):
        # conditioning: were both logarithms of every valid pixel rounded to fp32 the worst way (half an ulp each), the loss would
        # still move by less than the bar — a case of one pixel with pred within a few percent of target would not pass this
        v = target > 0
        lt, lp = np.abs(np.log(target[v].astype(np.float64))), np.abs(np.log(pred[v].astype(np.float64)))
        cond = 2.0 ** -24 * float((lt + lp).sum()) / float(np.abs(np.log(target[v].astype(np.float64)) - np.log(pred[v].astype(np.float64))).sum())
        assert cond <= cc.ORACLE_BAR, (case, cond)
    want_loss, want_grad = cc.restate(pred, target, kind, g)
    el, eg = cc.loss_err(loss, want_loss), cc.grad_err(grad, want_grad)
    assert el <= cc.ORACLE_BAR and eg <= cc.ORACLE_BAR, (case, el, eg)
    manifest["cases"][case] = {"reference_vs_fp64_loss_rel": el, "reference_vs_fp64_grad_rel": eg, "loss": repr(loss),
                               "valid_pixels": int((target > 0).sum()), "elements": int(target.size)}


def small(case, kind, seed, shape, g=1.0, **kw):
    pred, target = cc.make_inputs(seed, shape, **kw)
    loss, grad = reference(kind, pred, target, g)
    check(case, kind, pred, target, g, loss, grad)
    save("g18_criterion_" + case, kind=np.array(kind), seed=np.int64(seed), shape=np.array(shape, np.int64), g=np.float64(g),
         pred=pred, target=target, loss=np.float64(loss), grad=grad)
    return pred, target, loss, grad


def full(kind, seed):
    case = kind + "_full"
    pred, target = cc.make_inputs(seed, cc.FULL_SHAPE)
    loss, grad = reference(kind, pred, target, 1.0)
    check(case, kind, pred, target, 1.0, loss, grad)
    save("g18_criterion_" + case, kind=np.array(kind), seed=np.int64(seed), shape=np.array(cc.FULL_SHAPE, np.int64), g=np.float64(1.0),
         loss=np.float64(loss), grad_sub=grad.reshape(-1)[::cc.FULL_STRIDE].copy(), stride=np.int64(cc.FULL_STRIDE),
         grad_absmax=np.float64(np.abs(grad).max()))


def dsn(seed):
    case, kind = "dsn_l1", "l1"
    pred0, target = cc.make_inputs(seed, (2, 1, 8, 12))
    from oracle import cspn_oracle as orc
    pred1 = orc.hash_uniform(seed, 5, (2, 1, 4, 6), 0.5, 10.0)
    p0, p1 = torch.from_numpy(pred0).requires_grad_(True), torch.from_numpy(pred1).requires_grad_(True)
    loss = ref_criterion.get_criteria(args(kind, "DSN"))([p0, p1], torch.from_numpy(target))
    loss.backward()
    loss, g0, g1 = float(loss.detach()), p0.grad.numpy(), p1.grad.numpy()
    want_loss, w0, w1 = cc.restate_dsn(pred0, pred1, target, kind)
    errs = (cc.loss_err(loss, want_loss), cc.grad_err(g0, w0), cc.grad_err(g1, w1))
    assert max(errs) <= cc.ORACLE_BAR, (case, errs)
    manifest["cases"][case] = {"reference_vs_fp64_loss_rel": errs[0], "reference_vs_fp64_grad_rel": max(errs[1:]), "loss": repr(loss)}
    save("g18_criterion_" + case, kind=np.array(kind), seed=np.int64(seed), pred0=pred0, pred1=pred1, target=target,
         loss=np.float64(loss), grad0=g0, grad1=g1)


if __name__ == "__main__":
    for ki, kind in enumerate(cc.KINDS):
        for si, (tag, shape) in enumerate(SHAPES):
            for g, gt in ((1.0, "g10"), (0.4, "g04")):
                pred, target, loss, grad = small("%s_%s_%s" % (kind, tag, gt), kind, 182 - si, shape, g)
                assert (target > 0).any() and np.isfinite(loss), (kind, tag)
        pred, target, loss, grad = small(kind + "_ties", kind, 184, (2, 1, 19, 23), tie_frac=0.10)
        tie = (target > 0) & (pred == target)
        assert 0.05 * (target > 0).sum() < tie.sum() < 0.2 * (target > 0).sum() and not grad[tie].any()
        pred, target, loss, grad = small(kind + "_empty", kind, 185, (1, 1, 3, 5), all_invalid=True)
        assert np.isnan(loss) and not grad.any() and (target < 0).any()
        full(kind, 190)                                             # one input pair for the three kinds
    pred, target, loss, grad = small("l1_log_pred_zero", "l1_log", 186, (1, 1, 3, 5), hostile="zero")
    hit = (target > 0) & (pred == 0)
    assert hit.any() and loss == float("inf") and np.all(grad[hit] == -np.inf) and np.isfinite(grad[~hit]).all()
    pred, target, loss, grad = small("l1_log_pred_neg", "l1_log", 186, (1, 1, 3, 5), hostile="neg")
    hit = (target > 0) & (pred < 0)
    assert hit.any() and np.isnan(loss) and not grad[hit].any() and np.isfinite(grad).all()
    dsn(187)
    manifest["torch"] = torch.__version__
    manifest["numpy"] = np.__version__
    with open(os.path.join(HERE, "golden_g18_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest["cases"], indent=1, sort_keys=True))

"""Golden G23: the reference's berHuLoss and its unmasked criteria L1, GradLoss, RMSE and RMSE_log (libs/criterion/criteria.py:
42-88, 133-152), forward and backward.  BerHu(threshold) and NormalLoss are not covered: both raise before they compute anything.

Imports the reference (CSPN_REFERENCE, default /root/reference) — nothing of it is copied — runs every case of
tests/losses_cases.CASES through it on the CPU in fp32 with autograd and writes g23_losses_<case>.npz:

  <loss>_<shape>_g10 / _g04   loss in berhu, l1, grad, rmse, rmse_log; shapes 1, 3x5, 3x57x77 (13 167 elements: odd, 13 slices); the
                              incoming gradient 1 or 0.4: a, b (pred, target / fake, real), loss, grad
  <loss>_full                 24x1x228x304: the seed, the loss, every 997th gradient element (the test regenerates the inputs)
  berhu_*                     + c (fp32), n_valid, n_huber, max_at_valid.  ties; c_negative (c < 0, n_huber == n_valid);
                              c_from_invalid / c_from_valid; nan_invalid (c NaN, n_huber 0, the loss is masked L1); nan_valid (loss NaN,
                              no n_huber stored: the reference's own count is of a NaN comparison); empty (loss NaN, gradient 0)
  <kind>_equal                fake == real: loss 0; gradient 0 (l1, grad) or all NaN (rmse, rmse_log)
  rmse_log_real_nonpositive / _fake_zero
  rmse_resize                 fake 2x1x4x6 resized to real 2x1x8x12 (F.upsample: bilinear, align_corners=False)
  dsn_berhu                   CriterionDSN(berHuLoss()): target 2x1x8x12, predictions 8x12 and 4x6 -> loss, both gradients

Asserted before anything is written:
  1. the reference's fp32 loss and gradient agree with the fp64 restatement (tests/losses_cases.py) to 2e-6 — the loss relative,
     the gradient against its largest magnitude, NaN / +-Inf position for position;
  2. berHu: the restatement's c equals the reference's 0.2 * max(pred - target) bit for bit, and its Huber set has the size the
     reference's has (read from the sizes of the reference's own selections);
  3. every berHu main case of at least 15 pixels has between 10 % and 90 % of its valid pixels in the Huber set (a case of one
     pixel cannot: that pixel is in its own set whenever pred != target);
  4. l1 / grad: every pixel has fake == real exactly or |fake - real| >= 1e-4, so that the sign is the same in fp32 and fp64.
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

from libs.criterion import criteria as ref            # noqa: E402  (reference)
import losses_cases as lc                             # noqa: E402

torch.set_num_threads(4)
manifest = {"files": {}, "cases": {}}
MODULES = {"berhu": ref.berHuLoss, "l1": ref.L1, "grad": ref.GradLoss, "rmse": ref.RMSE, "rmse_log": ref.RMSE_log}


def save(name, **arrs):
    path = os.path.join(HERE, "g23_losses_" + name + ".npz")
    np.savez_compressed(path, **arrs)
    manifest["files"][name] = {"bytes": os.path.getsize(path), "arrays": {k: list(np.shape(v)) for k, v in arrs.items()}}
    assert os.path.getsize(path) <= 580000, (name, os.path.getsize(path))


def reference(loss_name, a, b, g):
    """The reference on the CPU in fp32: loss and d (g * loss) / d a."""
    x = torch.from_numpy(a).requires_grad_(True)
    loss = MODULES[loss_name]()(x, torch.from_numpy(b))
    (loss if g == 1.0 else loss * g).backward()
    return float(loss.detach()), x.grad.numpy()


def reference_berhu_sets(pred, target):
    """c and the sizes of the two selections, from the reference's own expressions (criteria.py:49-59)."""
    p, t = torch.from_numpy(pred), torch.from_numpy(target)
    c = 0.2 * torch.max(p - t)
    diff = (t - p)[t > 0].abs()
    return c.numpy().astype(np.float32), int(diff.numel()), int((diff > c).sum())


def case(name):
    s = lc.CASES[name]
    a, b = lc.make_inputs(name)
    loss, grad = reference(s["loss"], a, b, s["g"])
    want_loss, want_grad, extra = lc.restate(name, a, b)
    el, eg = lc.loss_err(loss, want_loss), lc.grad_err(grad, want_grad)
    assert el <= lc.ORACLE_BAR and eg <= lc.ORACLE_BAR, (name, el, eg)
    info = {"reference_vs_fp64_loss_rel": el, "reference_vs_fp64_grad_rel": eg, "loss": repr(loss), "elements": int(a.size)}
    arrs = dict(loss_name=np.array(s["loss"]), seed=np.int64(s["seed"]), shape=np.array(s["shape"], np.int64), g=np.float64(s["g"]),
                variant=np.array(s["variant"]), loss=np.float64(loss))
    if s["loss"] == "berhu":
        c, nv, nh = reference_berhu_sets(a, b)
        assert c.tobytes() == np.float32(extra["c"]).tobytes() or (np.isnan(c) and np.isnan(extra["c"])), (name, c, extra["c"])
        assert nv == extra["n_valid"] and nh == extra["n_huber"], (name, nv, nh, extra["n_valid"], extra["n_huber"])
        arrs.update(c=np.float32(c), n_valid=np.int64(nv), max_at_valid=np.bool_(extra["max_at_valid"]))
        if s["variant"] != "nan_valid":
            arrs.update(n_huber=np.int64(nh))
        info.update(c=repr(float(c)), n_valid=nv, n_huber=nh, max_at_valid=extra["max_at_valid"])
        if s["variant"] == "main" and a.size >= 15:
            assert 0.10 * nv <= nh <= 0.90 * nv, (name, nv, nh)
    elif s["loss"] in ("l1", "grad"):
        assert np.all((a == b) | (np.abs(a.astype(np.float64) - b.astype(np.float64)) >= 1e-4)), name
    if tuple(s["shape"]) == lc.FULL_SHAPE:
        arrs.update(grad_sub=grad.reshape(-1)[::lc.FULL_STRIDE].copy(), stride=np.int64(lc.FULL_STRIDE),
                    grad_absmax=np.float64(np.abs(grad).max()))
    else:
        arrs.update(a=a, b=b, grad=grad)
    manifest["cases"][name] = info
    save(name, **arrs)
    return a, b, loss, grad, extra


def dsn():
    pred0, pred1, target = lc.dsn_inputs()
    p0, p1 = torch.from_numpy(pred0).requires_grad_(True), torch.from_numpy(pred1).requires_grad_(True)
    loss = ref.CriterionDSN(criterion=ref.berHuLoss())([p0, p1], torch.from_numpy(target))
    loss.backward()
    loss, g0, g1 = float(loss.detach()), p0.grad.numpy(), p1.grad.numpy()
    want_loss, w0, w1 = lc.restate_dsn_berhu(pred0, pred1, target)
    errs = (lc.loss_err(loss, want_loss), lc.grad_err(g0, w0), lc.grad_err(g1, w1))
    assert max(errs) <= lc.ORACLE_BAR, ("dsn_berhu", errs)
    manifest["cases"]["dsn_berhu"] = {"reference_vs_fp64_loss_rel": errs[0], "reference_vs_fp64_grad_rel": max(errs[1:]), "loss": repr(loss)}
    save("dsn_berhu", pred0=pred0, pred1=pred1, target=target, loss=np.float64(loss), grad0=g0, grad1=g1)


def resize():
    fake, real = lc.resize_inputs()
    loss, grad = reference("rmse", fake, real, 1.0)
    want_loss, want_grad = lc.restate_resize(fake, real, "rmse")
    errs = (lc.loss_err(loss, want_loss), lc.grad_err(grad, want_grad))
    assert max(errs) <= lc.ORACLE_BAR, ("rmse_resize", errs)
    manifest["cases"]["rmse_resize"] = {"reference_vs_fp64_loss_rel": errs[0], "reference_vs_fp64_grad_rel": errs[1], "loss": repr(loss)}
    save("rmse_resize", fake=fake, real=real, loss=np.float64(loss), grad=grad)


if __name__ == "__main__":
    import warnings
    warnings.filterwarnings("ignore", message=".*upsample.*")
    for name in lc.CASES:
        a, b, loss, grad, extra = case(name)
        s = lc.CASES[name]
        v = s["variant"]
        if v == "main":
            assert np.isfinite(loss) and np.isfinite(grad).all(), name
        if s["loss"] == "berhu":
            valid = b > 0
            assert not grad[~valid].any(), name
            if v == "ties":
                tie = valid & (a == b)
                assert 0.05 * valid.sum() < tie.sum() < 0.2 * valid.sum() and not grad[tie].any() and extra["c"] > 0
            if v == "c_negative":
                assert extra["c"] < 0 and extra["n_huber"] == extra["n_valid"] > 0 and (a < b).all()
                assert ((a - b) == (a - b).max()).sum() == 4
            if v == "c_from_invalid":
                assert not extra["max_at_valid"] and 0 < extra["n_huber"] < extra["n_valid"]
            if v == "c_from_valid":
                assert extra["max_at_valid"] and 0 < extra["n_huber"] < extra["n_valid"]
            if v == "nan_invalid":
                assert np.isnan(extra["c"]) and extra["n_huber"] == 0 and np.isfinite(loss)
                masked_l1 = np.abs(b.astype(np.float64) - a.astype(np.float64))[valid].mean()
                assert abs(loss - masked_l1) <= lc.ORACLE_BAR * masked_l1
            if v == "nan_valid":
                hit = np.isnan(a)
                assert hit.sum() == 1 and valid[hit].all() and np.isnan(loss) and not grad[hit].any()
                assert np.isfinite(grad).all() and grad[valid & ~hit].all()
            if v == "empty":
                assert np.isnan(loss) and not grad.any() and (b < 0).any() and not valid.any()
        else:
            if v == "equal":
                assert loss == 0.0
                assert np.isnan(grad).all() if s["loss"] in ("rmse", "rmse_log") else not grad.any()
            if v == "real_nonpositive":
                assert (b <= 0).any() and np.isnan(loss) and np.isnan(grad).all()
            if v == "fake_zero":
                assert (a == 0).sum() == 3 and loss == float("inf") and np.isnan(grad[a == 0]).all() and not grad[a != 0].any()
            if s["loss"] == "rmse_log" and v == "main":
                assert (b > 0).all()
    dsn()
    resize()
    manifest["torch"] = torch.__version__
    manifest["numpy"] = np.__version__
    with open(os.path.join(HERE, "golden_g23_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest["cases"], indent=1, sort_keys=True))

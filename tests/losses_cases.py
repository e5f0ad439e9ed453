"""Golden G23 (berHuLoss and the unmasked criteria L1, GradLoss, RMSE, RMSE_log): the case table, the seeded inputs and the fp64
numpy restatement of libs/criterion/criteria.py:42-88, 133-152 that both tests/golden/make_golden_g23.py (which holds the
reference to it before writing a fixture) and tests/test_losses.py use.  No torch, no reference, no package code: numpy, the
oracle's hash generator and tests/criterion_cases.py only."""
import numpy as np

import criterion_cases as cc
from oracle import cspn_oracle as orc

ORACLE_BAR = cc.ORACLE_BAR     # 2e-6: the reference's fp32 result against fp64
TEST_RTOL = cc.TEST_RTOL       # 1e-5: README "Parity", fp32
FULL_SHAPE = cc.FULL_SHAPE
FULL_STRIDE = cc.FULL_STRIDE
MEAN_KINDS = ("l1", "grad", "rmse", "rmse_log")
SHAPES = (("1", (1, 1, 1, 1)), ("3x5", (1, 1, 3, 5)), ("3x57x77", (3, 1, 57, 77)))
SMALL_SHAPE = (2, 1, 19, 23)
BERHU_RATIO = np.float32(0.2)
loss_err, grad_err = cc.loss_err, cc.grad_err


def _cases():
    c = {}
    for si, (tag, shape) in enumerate(SHAPES):
        for g, gt in ((1.0, "g10"), (0.4, "g04")):
            # the seeds of G18: 182 makes the one-pixel case a valid pixel (which is then its own Huber set: |e| > 0.2 e)
            c["berhu_%s_%s" % (tag, gt)] = dict(loss="berhu", seed=182 - si, shape=shape, g=g, variant="main")
            for kind in MEAN_KINDS:
                c["%s_%s_%s" % (kind, tag, gt)] = dict(loss=kind, seed=182 - si, shape=shape, g=g, variant="main")
    c["berhu_ties"] = dict(loss="berhu", seed=184, shape=SMALL_SHAPE, g=1.0, variant="ties")
    c["berhu_full"] = dict(loss="berhu", seed=190, shape=FULL_SHAPE, g=1.0, variant="main")
    for v, seed in (("c_negative", 193), ("c_from_invalid", 194), ("c_from_valid", 194), ("nan_invalid", 195), ("nan_valid", 195),
                    ("empty", 185)):
        c["berhu_" + v] = dict(loss="berhu", seed=seed, shape=(1, 1, 3, 5) if v == "empty" else SMALL_SHAPE, g=1.0, variant=v)
    for kind in MEAN_KINDS:
        c[kind + "_full"] = dict(loss=kind, seed=190, shape=FULL_SHAPE, g=1.0, variant="main")
        c[kind + "_equal"] = dict(loss=kind, seed=196, shape=SMALL_SHAPE, g=1.0, variant="equal")
    c["rmse_log_real_nonpositive"] = dict(loss="rmse_log", seed=197, shape=SMALL_SHAPE, g=1.0, variant="real_nonpositive")
    c["rmse_log_fake_zero"] = dict(loss="rmse_log", seed=197, shape=SMALL_SHAPE, g=1.0, variant="fake_zero")
    return c


CASES = _cases()                                   # name -> what make_inputs needs; the fixture of a case is g23_losses_<name>.npz
EXTRA = ("dsn_berhu", "rmse_resize")               # fixtures with a layout of their own
DSN_SEED, RESIZE_SEED = 187, 198


def _uniform(seed, tid, shape):
    return (orc.hash_u24(seed, tid, int(np.prod(shape))).astype(np.float64) / 16777216.0).reshape(shape)


def berhu_inputs(seed, shape, variant="main"):
    """(pred, target) fp32.  target: criterion_cases' (U(0.5, 10), ~30 % zeros, ~5 % negatives) with the negatives scaled by
    0.01 — as they stand max(pred - target) is ~20, c ~4 and no pixel is in the Huber set; pred = max(|target| + N(0, 1), 0.05).
      ties             10 % of the pixels have pred == target bit for bit
      c_negative       pred < target at EVERY pixel, so c < 0 and every valid pixel is in the set; the pixel that holds the
                       maximum is copied to three more places (the maximum is attained four times)
      c_from_invalid / c_from_valid   pred = target + 8 at one invalid / valid pixel, which then holds the maximum
      nan_invalid / nan_valid         pred = NaN at one invalid / valid pixel
      empty            no pixel has target > 0"""
    _, target = cc.make_inputs(seed, shape)
    target = np.where(target < 0, target * np.float32(0.01), target).astype(np.float32)
    if variant == "empty":
        target = np.where(target > 0, np.float32(0), target).astype(np.float32)
    noise = orc.hash_normal(seed, 6, shape).astype(np.float32)
    pred = np.maximum(np.abs(target) + noise, np.float32(0.05)).astype(np.float32)
    flat_p, flat_t = pred.reshape(-1).copy(), target.reshape(-1).copy()
    n = flat_p.size
    if variant == "ties":
        sel = _uniform(seed, 4, (n,)) < 0.10
        flat_p = np.where(sel, flat_t, flat_p).astype(np.float32)
    elif variant == "c_negative":
        flat_p = (flat_t - np.float32(0.1) - np.abs(noise.reshape(-1))).astype(np.float32)
        i = int(np.argmax(flat_p - flat_t))
        for j in ((i + 7) % n, (i + 300) % n, (i + 601) % n):
            flat_p[j], flat_t[j] = flat_p[i], flat_t[i]
    elif variant in ("c_from_invalid", "c_from_valid", "nan_invalid", "nan_valid"):
        where = np.flatnonzero((flat_t > 0) == variant.endswith("_valid"))
        i = int(where[len(where) // 2])
        flat_p[i] = np.float32("nan") if variant.startswith("nan") else flat_t[i] + np.float32(8)
    return flat_p.reshape(shape), flat_t.reshape(shape)


def mean_inputs(kind, seed, shape, variant="main"):
    """(fake, real) fp32: criterion_cases.make_inputs' (pred, target) — zeros and negatives in `real` included, and every
    pixel either an exact tie or well apart, so that sign(10 r - 10 f) is the same in fp32 and fp64.  rmse_log:
    real = |target| + 0.5 > 0.  equal: fake == real.  real_nonpositive: three negative `real`.  fake_zero: three zeros in `fake`."""
    fake, real = cc.make_inputs(seed, shape)
    if kind == "rmse_log":
        real = (np.abs(real) + np.float32(0.5)).astype(np.float32)
    if variant == "equal":
        fake = real.copy()
    elif variant in ("real_nonpositive", "fake_zero"):
        flat = (real if variant == "real_nonpositive" else fake).reshape(-1).copy()
        flat[[5, flat.size // 2, flat.size - 1]] = np.float32(-1.5 if variant == "real_nonpositive" else 0.0)
        if variant == "real_nonpositive":
            real = flat.reshape(shape)
        else:
            fake = flat.reshape(shape)
    return fake, real


def make_inputs(name):
    s = CASES[name]
    if s["loss"] == "berhu":
        return berhu_inputs(s["seed"], s["shape"], s["variant"])
    return mean_inputs(s["loss"], s["seed"], s["shape"], s["variant"])


def dsn_inputs():
    """(pred0 2x1x8x12, pred1 2x1x4x6, target 2x1x8x12) of the CriterionDSN(berHuLoss()) case."""
    pred0, target = berhu_inputs(DSN_SEED, (2, 1, 8, 12))
    return pred0, orc.hash_uniform(DSN_SEED, 5, (2, 1, 4, 6), 0.5, 10.0), target


def resize_inputs():
    """(fake 2x1x4x6, real 2x1x8x12) of the RMSE case whose prediction is resized first."""
    _, real = cc.make_inputs(RESIZE_SEED, (2, 1, 8, 12))
    return orc.hash_uniform(RESIZE_SEED, 5, (2, 1, 4, 6), 0.5, 10.0), real


def _sign(x):
    return np.where(np.isnan(x), 0.0, np.sign(x))          # the backward of abs: sgn(NaN) = 0


def restate_berhu(pred, target, g=1.0):
    """berHuLoss: the threshold and the Huber set from the fp32 operations the reference performs (pred - target, its maximum,
    one multiply by fp32 0.2, |target - pred|, the comparison), the sums and the gradient in fp64.
    -> dict(loss, grad, c (np.float32), n_valid, n_huber, max_at_valid)."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = pred - target
        m = np.float32("nan") if np.isnan(e).any() else e.max()
        c = np.float32(BERHU_RATIO * m)
        valid = target > 0
        huber = valid & (np.abs(target - pred) > c)
        x = target.astype(np.float64) - pred.astype(np.float64)
        d = np.abs(x)
        nv, nh = int(valid.sum()), int(huber.sum())
        loss = (d[valid].sum() + (d[huber] ** 2).sum()) / (nv + nh) if nv else float("nan")
        grad = np.where(valid, -_sign(x) * np.where(huber, 1.0 + 2.0 * d, 1.0) * (g / (nv + nh)), 0.0) if nv else np.zeros_like(x)
        at_valid = bool(valid.reshape(-1)[int(np.argmax(e))]) if not np.isnan(m) else False
    return dict(loss=float(loss), grad=grad, c=c, n_valid=nv, n_huber=nh, max_at_valid=at_valid)


def restate_mean(fake, real, kind, g=1.0):
    """The unmasked means in fp64: (loss, d (g * loss) / d fake)."""
    f, r = np.asarray(fake, np.float64), np.asarray(real, np.float64)
    n = f.size
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "l1":
            x = 10.0 * r - 10.0 * f
            return float(np.abs(x).sum() / n), -10.0 * _sign(x) * (g / n)
        if kind == "grad":
            x = r - f
            return float(np.abs(x).sum() / n), -_sign(x) * (g / n)
        if kind == "rmse":
            x = 10.0 * r - 10.0 * f
            loss = np.sqrt((x * x).sum() / n)
            return float(loss), -10.0 * x * (g / (n * loss))
        if kind == "rmse_log":
            x = np.log(r) - np.log(f)
            loss = np.sqrt((x * x).sum() / n)
            return float(loss), -x * (g / (n * loss)) / f
    raise NotImplementedError(kind)


def restate(name_or_spec, a, b):
    """The restatement of a case of CASES on the inputs (a, b) -> (loss, grad, extras or None)."""
    s = CASES[name_or_spec] if isinstance(name_or_spec, str) else name_or_spec
    if s["loss"] == "berhu":
        r = restate_berhu(a, b, s["g"])
        return r["loss"], r["grad"], r
    loss, grad = restate_mean(a, b, s["loss"], s["g"])
    return loss, grad, None


def half_pixel_matrix(n_out, n_in):
    """[n_out, n_in] weights of a 1-D bilinear resize with align_corners=False (what F.upsample(mode='bilinear') does)."""
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        x = max((i + 0.5) * n_in / n_out - 0.5, 0.0)
        lo = min(int(np.floor(x)), n_in - 1)
        hi = min(lo + 1, n_in - 1)
        m[i, lo] += 1.0 - (x - lo)
        m[i, hi] += x - lo
    return m


def restate_resize(fake, real, kind):
    """RMSE / RMSE_log / L1 on a fake of another size -> (loss, grad wrt the small fake)."""
    ah, aw = half_pixel_matrix(real.shape[-2], fake.shape[-2]), half_pixel_matrix(real.shape[-1], fake.shape[-1])
    loss, gu = restate_mean(ah @ fake.astype(np.float64) @ aw.T, real, kind)
    return loss, ah.T @ gu @ aw


def restate_dsn_berhu(pred0, pred1, target):
    """CriterionDSN(berHuLoss()) in fp64: loss1 + 0.4 * loss2, predictions resized (align_corners=True) to the target's size.
    The Huber set of the resized prediction is taken from its fp32 rounding."""
    H, W = target.shape[-2:]
    total, grads = 0.0, []
    for pred, g in ((pred0, 1.0), (pred1, 0.4)):
        ah, aw = cc.bilinear_matrix(H, pred.shape[-2]), cc.bilinear_matrix(W, pred.shape[-1])
        up = ah @ pred.astype(np.float64) @ aw.T
        r = restate_berhu_fp64(up, target, g)
        total += g * r[0]
        grads.append(ah.T @ r[1] @ aw)
    return total, grads[0], grads[1]


def restate_berhu_fp64(pred64, target, g):
    """berHu on an fp64 prediction (the resized one of the DSN case): the Huber set from its fp32 rounding, and — asserted —
    no valid pixel within 1e-4 of the threshold, so that the set does not depend on how the resize was rounded."""
    p32 = pred64.astype(np.float32)
    r = restate_berhu(p32, target, g)
    t = target.astype(np.float64)
    valid = t > 0
    x = t - pred64
    d = np.abs(x)
    assert not (valid & (np.abs(d - float(r["c"])) < 1e-4)).any(), "a pixel of the DSN case sits on the threshold"
    huber = valid & (d > float(r["c"]))
    count = int(valid.sum()) + int(huber.sum())
    loss = (d[valid].sum() + (d[huber] ** 2).sum()) / count
    grad = np.where(valid, -_sign(x) * np.where(huber, 1.0 + 2.0 * d, 1.0) * (g / count), 0.0)
    return float(loss), grad

"""Golden G18 (the training criteria): the seeded inputs and the fp64 numpy restatement of libs/criterion/criteria.py that both
tests/golden/make_golden_g18.py (which holds the reference to it before writing a fixture) and tests/test_criterion.py use.
No torch, no reference, no package code: numpy and the oracle's hash generator only."""
import numpy as np

from oracle import cspn_oracle as orc

KINDS = ("l1", "l2", "l1_log")
ORACLE_BAR = 2e-6          # the reference's fp32 result against fp64: a fifth of the bar the device is held to
TEST_RTOL = 1e-5           # README "Parity", fp32
TIE_BAND = 1e-3            # l1_log: a valid pixel has pred == target exactly or |pred / target - 1| >= TIE_BAND
FULL_SHAPE = (24, 1, 228, 304)
FULL_STRIDE = 997          # the full-size fixtures keep every 997th gradient element


def make_inputs(seed, shape, tie_frac=0.0, all_invalid=False, hostile=None):
    """(pred, target) fp32.  target: U(0.5, 10) with ~30 % zeros and ~5 % negatives; pred = |target| + N(0, 1), floored at
    0.05 (noise of that size keeps l1_log well conditioned in fp32 down to a single pixel: the two logarithms are rounded to
    ~1e-7 absolute each, which must stay far below 2e-6 of their difference).  tie_frac: that share of the pixels gets pred = target bit for bit.  Every other valid pixel is moved out of the band
    |pred / target - 1| < TIE_BAND (to target * 1.002), so that the sign of log t - log p is the same in fp32 and fp64.
    all_invalid: no pixel has target > 0.  hostile "zero" / "neg": every 5th valid pixel has pred = 0 / pred = -1.5."""
    n = int(np.prod(shape))
    mag = orc.hash_uniform(seed, 1, shape, 0.5, 10.0)
    u = (orc.hash_u24(seed, 2, n).astype(np.float64) / 16777216.0).reshape(shape)
    target = np.where(u < 0.30, np.float32(0), np.where(u < 0.35, -mag, mag)).astype(np.float32)
    if all_invalid:
        target = np.where(target > 0, np.float32(0), target).astype(np.float32)
    noise = orc.hash_normal(seed, 3, shape)
    pred = np.maximum(np.abs(target) + noise, np.float32(0.05)).astype(np.float32)
    valid = target > 0
    if tie_frac > 0:
        sel = (orc.hash_u24(seed, 4, n).astype(np.float64) / 16777216.0).reshape(shape) < tie_frac
        pred = np.where(sel & valid, target, pred).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        near = valid & (pred != target) & (np.abs(pred.astype(np.float64) / target.astype(np.float64) - 1.0) < TIE_BAND)
    pred = np.where(near, (target.astype(np.float64) * 1.002).astype(np.float32), pred).astype(np.float32)
    if hostile is not None:
        idx = np.flatnonzero(valid.reshape(-1))[::5]
        flat = pred.reshape(-1).copy()
        flat[idx] = np.float32({"zero": 0.0, "neg": -1.5}[hostile])
        pred = flat.reshape(shape)
    return pred, target


def no_tie_ok(pred, target):
    """The l1_log condition: every valid pixel has pred == target or |pred / target - 1| >= TIE_BAND (a pred <= 0 is far away)."""
    p, t = pred.astype(np.float64), target.astype(np.float64)
    valid = t > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(p / t - 1.0)
    return bool(np.all(~valid | (p == t) | (r >= TIE_BAND)))


def restate(pred, target, kind, g=1.0):
    """fp64 restatement: (loss, d (g * loss) / d pred).  loss is NaN without a valid pixel, the gradient is 0 then."""
    p, t = pred.astype(np.float64), target.astype(np.float64)
    valid = t > 0
    cnt = float(valid.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "l1":
            d = t - p
            term, core = np.abs(d), -np.where(np.isnan(d), 0.0, np.sign(d))   # the backward of abs: sgn(NaN) = 0
        elif kind == "l2":
            d = t - p
            term, core = d * d, 2.0 * (p - t)
        elif kind == "l1_log":
            d = np.log(t) - np.log(p)
            s = np.where(np.isnan(d), 0.0, np.sign(d))
            term, core = np.abs(d), -s / p                             # p == 0: -inf; p < 0: -0 / p = 0
        else:
            raise NotImplementedError(kind)
        loss = term[valid].sum() / cnt if cnt else float("nan")
        grad = np.where(valid, core * (g / cnt), 0.0) if cnt else np.zeros_like(p)
    return float(loss), grad


def bilinear_matrix(n_out, n_in):
    """[n_out, n_in] weights of a 1-D bilinear resize with align_corners=True."""
    m = np.zeros((n_out, n_in))
    for i in range(n_out):
        x = i * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        lo = min(int(np.floor(x)), n_in - 1)
        hi = min(lo + 1, n_in - 1)
        m[i, lo] += 1.0 - (x - lo)
        m[i, hi] += x - lo
    return m


def restate_dsn(pred0, pred1, target, kind):
    """CriterionDSN in fp64: loss1 + 0.4 * loss2, predictions resized to the target's size -> (loss, grad_pred0, grad_pred1)."""
    H, W = target.shape[-2:]
    total, grads = 0.0, []
    for pred, g in ((pred0, 1.0), (pred1, 0.4)):
        ah, aw = bilinear_matrix(H, pred.shape[-2]), bilinear_matrix(W, pred.shape[-1])
        up = ah @ pred.astype(np.float64) @ aw.T
        loss, gu = restate(up, target, kind, g)
        total += g * loss
        grads.append(ah.T @ gu @ aw)
    return total, grads[0], grads[1]


def loss_err(got, want):
    """Relative error of a loss; a non-finite `want` must be matched in kind (NaN, +Inf, -Inf): 0 or inf."""
    got, want = float(got), float(want)
    if not np.isfinite(want) or not np.isfinite(got):
        same = (np.isnan(got) and np.isnan(want)) or got == want
        return 0.0 if same else float("inf")
    return abs(got - want) / max(abs(want), 1e-30)


def grad_err(got, want):
    """max |got - want| over the finite entries, over max |want|; NaN and +-Inf must sit at the same places: else inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return float("inf")
    fin = np.isfinite(want)
    if not np.array_equal(fin, np.isfinite(got)):
        return float("inf")
    bad = ~fin
    if bad.any() and not np.array_equal(np.nan_to_num(got[bad], nan=7.0, posinf=1.0, neginf=-1.0),
                                        np.nan_to_num(want[bad], nan=7.0, posinf=1.0, neginf=-1.0)):
        return float("inf")
    if not fin.any():
        return 0.0
    scale = np.abs(want[fin]).max()
    diff = np.abs(got[fin] - want[fin]).max()
    return float(diff / scale) if scale > 0 else (0.0 if diff == 0 else float("inf"))

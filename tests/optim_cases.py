"""What tests/test_optim.py and tests/golden/make_golden_g24.py share: the numpy restatement of the SGD arithmetic of
include/cspn_optim.h, the hyper-parameter combinations, the comparison rule, and the drivers of the scheduler golden G24.

The restatement (every scalar rounded to fp32 first; 1 - dampening formed in double, then rounded):
    g   = maximize ? -grad : grad
    g   = fma(wd, p, g)                                 if wd != 0
    buf = g                                             on a tensor's first step
    buf = fma(1 - dampening, g, fl(momentum * buf))     otherwise: the product is rounded on its own
    d   = nesterov ? fma(momentum, buf, g) : buf        (momentum == 0: d = g)
    p   = fma(-lr, d, p)
"""
import itertools
import types

import numpy as np

CHUNK = 4096                  # CSPN_SGD_CHUNK
TENSORS_PER_LAUNCH = 109      # CSPN_SGD_TENSORS_PER_LAUNCH
CPU_SIZES = (1, 3, 5, 7, 9, 17, 33, 70, 1000, 40000)


def _combos():
    out = []
    for momentum, dampening, nesterov, wd, maximize in itertools.product((0.0, 0.9), (0.0, 0.3), (False, True), (0.0, 1e-4), (False, True)):
        if nesterov and (momentum <= 0 or dampening != 0):
            continue                                   # torch refuses it
        out.append(dict(momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd, maximize=maximize))
    return out


COMBOS = _combos()


def combo_id(c):
    return "m%g_d%g_%s_wd%g_%s" % (c["momentum"], c["dampening"], "nesterov" if c["nesterov"] else "plain", c["weight_decay"],
                                   "max" if c["maximize"] else "min")


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 operands.  The product of two fp32 values is exact in fp64; the sum is made
    exact by TwoSum and the fp64 result rounded to odd, after which the rounding to fp32 (29 bits fewer) is the correct one."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        x = a * b
        s = x + c
        bb = s - x
        err = (x - (s - bb)) + (c - bb)
        bits = s.view(np.int64).copy() if s.ndim else np.array(s).view(np.int64).copy()
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        grow = (err > 0) == (s > 0)                    # the exact sum lies further from zero than s
        bits = np.where(fix, np.where(grow, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(np.float32)


def sgd_restated(p, g, buf, first, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    """One step on fp32 arrays -> (p, buf); buf is returned as given (None included) when momentum == 0."""
    p = np.asarray(p, np.float32)
    g = np.asarray(g, np.float32)
    lr32, mom32, wd32 = np.float32(lr), np.float32(momentum), np.float32(weight_decay)
    omd32 = np.float32(1.0 - dampening)
    if maximize:
        g = -g
    if weight_decay != 0:
        g = fma32(wd32, p, g)
    d = g
    if momentum != 0:
        if first:
            buf = g.copy()
        else:
            with np.errstate(all="ignore"):
                prod = (mom32 * np.asarray(buf, np.float32)).astype(np.float32)
            buf = fma32(omd32, g, prod)
        d = fma32(mom32, buf, g) if nesterov else buf
    return fma32(-lr32, d, p), buf


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same(got, want):
    """The comparison rule: bit for bit on every finite value, +-Inf and +-0; NaN position for position (a NaN's sign and
    payload are not compared)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn]))


def n_differing(got, want):
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    gn, wn = np.isnan(got), np.isnan(want)
    return int(((bits(got) != bits(want)) & ~(gn & wn)).sum())


def values(seed, n):
    return np.random.RandomState(seed).standard_normal(n).astype(np.float32)


SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.4028234663852886e38, -3.4028234663852886e38, 1.0, -1.5, 2.5e38],
                    dtype=np.float32)
DENORMALS = np.array([1e-40, -1e-40, 1.401298464324817e-45, -1.401298464324817e-45, 1.1754942106924411e-38, -1.1754942106924411e-38,
                      1.1754943508222875e-38, -1.1754943508222875e-38, 3e-38, -2.3e-38, 0.0, 7e-39], dtype=np.float32)


def cross3(vals):
    """p, g, buf running over vals x vals x vals, plus three elements so that the 16-byte path leaves a tail."""
    k = len(vals)
    i = np.arange(k ** 3)
    p, g, b = vals[i // (k * k)], vals[(i // k) % k], vals[i % k]
    tail = vals[:3]
    return np.concatenate([p, tail]), np.concatenate([g, tail[::-1]]), np.concatenate([b, tail])


# ------------------------------------------------------------------------------------------------ golden G24
G24_BASE_RATES = (0.01, 0.003)
POLY_CASES = ((40, 1), (40, 10), (25, 4))
PLATEAU_METRICS = (1.0, 0.9, 0.8, 0.8, 0.8, 0.8, 0.7, 0.6, 0.6, 0.6, 0.6, 0.6, 0.5, 0.5)      # per epoch: plateaus twice
PLATEAU_LEN = 5


def _optimizer():
    import torch
    ps = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3))]
    return torch.optim.SGD([dict(params=[ps[0]], lr=G24_BASE_RATES[0]), dict(params=[ps[1]], lr=G24_BASE_RATES[1])], lr=0.1, momentum=0.9)


def _rates(opt):
    return [float(g["lr"]).hex() for g in opt.param_groups]


def g24_run(sched):
    """Every G24 case through the scheduler module `sched` (the reference's libs.scheduler, or cspn_monodepth_amd.scheduler) on a
    plain torch optimiser with float rates -> {case: [[rate of every group as a hex double] per iteration]}; entry 0 is the rate
    after construction."""
    out = {}
    for max_iter, decay_iter in POLY_CASES:
        args = types.SimpleNamespace(scheduler="poly_lr", max_iter=max_iter, decay_iter=decay_iter, gamma=0.9)
        opt = _optimizer()
        s = sched.get_schedular(opt, args)
        rows = [_rates(opt)]
        for it in range(max_iter + 7):                 # past max_iter
            opt.step()
            sched.do_schedule(args, s, it, 5, None)
            rows.append(_rates(opt))
        out["poly_%d_%d" % (max_iter, decay_iter)] = rows
    for mode in ("linear", "constant"):
        opt = _optimizer()
        inner = sched.PolynomialLR(opt, max_iter=40, decay_iter=1, gamma=0.9)
        s = sched.WarmUpLR(opt, inner, mode=mode, warmup_iters=5, gamma=0.2)
        rows = [_rates(opt)]
        for it in range(12):
            opt.step()
            s.step()
            rows.append(_rates(opt))
        out["warmup_" + mode] = rows
    args = types.SimpleNamespace(scheduler="reduce_lr", factor=0.2, lr_patience=2)
    opt = _optimizer()
    s = sched.get_schedular(opt, args)
    rows = [_rates(opt)]
    for it in range(PLATEAU_LEN * len(PLATEAU_METRICS)):
        opt.step()
        sched.do_schedule(args, s, it, PLATEAU_LEN, PLATEAU_METRICS[it // PLATEAU_LEN])
        rows.append(_rates(opt))
    out["reduce_lr"] = rows
    return out

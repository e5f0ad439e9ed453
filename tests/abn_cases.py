"""Cases, inputs and the fp64 restatement of In-Place Activated BatchNorm (cspn_monodepth_amd/network/inplace_abn.py,
include/cspn_abn.h) shared by tests/golden/make_golden_g20.py and tests/test_abn.py.

`restate` is the INDEPENDENT statement: batch normalisation with the scale |weight| + eps, then the activation, and the gradient
of that composition by the chain rule from the PRE-activation — it never inverts the activation or the affine map, which is what
the module under test (and the reference) do.  Training-mode parameter gradients are the true ones; eval mode restates what the
reference leaves (functions.py:144-147: edz = eydz = 0, so dx = dz' gamma invstd and dweight = dbias = 0).

Inputs (oracle.cspn_oracle's hash generator, every seed in CASES):
  x       per channel: offset_c + scale_c * U(-1, 1), scale_c in [0.5, 2] (times the case's `spread`), offset_c in [-scale_c, scale_c] (+ the case's `offset`, in units of
          the channel's standard deviation scale_c / sqrt(3)).  Uniform, so |y| < 2 or so and, with bias >= -0.5 and |w| <= 2, an
          elu pre-activation stays above -4: near z = -1 the inversion log1p(z) is ill-conditioned in ANY fp32 implementation
          (the maker asserts the bound);
  cot     ~ N(0, 1);  |weight| in [0.25, 2], signs alternating by channel ("mixed"), weight[1] = 0 exactly ("zero");
  bias in [-0.5, 0.5];  running_mean in [-0.5, 0.5], running_var in [0.5, 1.5] (not the initial 0 / 1: the update is then visible);
          eval cases: the channel's own centre and variance, perturbed.
"""
from collections import OrderedDict

import numpy as np

from oracle import cspn_oracle as orc

EPS = 1e-5
SLOPE = 0.01
ORACLE_BAR = 2e-6        # the reference's fp32 run against `restate`, asserted by the maker
DEVICE_BAR = 1e-5        # the project's fp32 bar: max |got - want| <= 1e-5 max |want|
ACTIVATIONS = ("leaky_relu", "elu", "none")
FIELDS = ("out", "dx", "dweight", "dbias", "running_mean", "running_var")
FULL_STRIDE = 97         # the big cases store every 97th element of out and dx (the test regenerates the inputs)
MAX_FILE_BYTES = 580000


def _case(shape, activation, seed, affine=True, weights="mixed", training=True, momentum=0.1, offset=0.0, full=False, spread=1.0):
    return dict(shape=tuple(shape), activation=activation, seed=seed, affine=affine, weights=weights if affine else None,
                training=training, momentum=momentum, offset=float(offset), full=full, eps=EPS, slope=SLOPE, spread=float(spread))


def ncs_of(shape):
    return int(shape[0]) * int(np.prod(shape[2:], dtype=np.int64))


SHAPES = OrderedDict([("1x2x1x2", (1, 2, 1, 2)), ("3x4x1x1", (3, 4, 1, 1)), ("6x5", (6, 5)), ("2x3x5x7", (2, 3, 5, 7)),
                      ("3x5x9x11", (3, 5, 9, 11))])
CASES = OrderedDict()
for _si, (_tag, _shape) in enumerate(SHAPES.items()):
    for _ai, _act in enumerate(ACTIVATIONS):
        # N * S = 2: y = +-a with 1 - a^2 = eps / (var + eps), and dx = gamma invstd (dz_1 - dz_2) / 2 * (1 - a^2) exactly — with a
        # variance of order 1 that factor is 1e-5, formed by cancellation of terms of order 1: NO fp32 implementation has five
        # digits of it (the reference's own run is 1e-3 from fp64 there).  A spread of 0.01 makes the variance ~1e-4 and the factor
        # ~0.1: the case then tests what it is there for (two values per channel, eps inside invstd), well-conditioned
        CASES["%s_%s" % (_act, _tag)] = _case(_shape, _act, 200 + 10 * _si + _ai, spread=0.01 if ncs_of(_shape) == 2 else 1.0)
CASES["affine_false"] = _case((2, 3, 5, 7), "leaky_relu", 260, affine=False)
for _ai, _act in enumerate(ACTIVATIONS):
    CASES["zero_weight_" + _act] = _case((3, 5, 9, 11), _act, 270 + _ai, weights="zero")
    CASES["eval_" + _act] = _case((2, 3, 5, 7), _act, 280 + _ai, training=False)
CASES["momentum_1"] = _case((2, 3, 5, 7), "none", 290, momentum=1.0)
# the offset case: `offset` is filled in from the golden's manifest (the largest power of two at which the reference's own fp32
# run still sits within ORACLE_BAR of the restatement: tests/golden/make_golden_g20.py)
CASES["offset"] = _case((3, 5, 9, 11), "none", 291)
CASES["full_small_regime"] = _case((2, 2048, 8, 10), "leaky_relu", 292, full=True)       # many channels, tiny planes
CASES["full_split_regime"] = _case((1, 64, 114, 152), "elu", 293, full=True)             # one big plane per channel
CASES["full_split_offset"] = _case((1, 64, 114, 152), "none", 294, full=True)            # ... with `offset` as the offset case


def ncs(shape):
    return int(shape[0]), int(shape[1]), int(np.prod(shape[2:], dtype=np.int64))


def make_inputs(case, offset=None):
    """x, cot, weight, bias, running_mean, running_var (fp32; weight / bias None when not affine)."""
    shape, seed = case["shape"], case["seed"]
    offset = case["offset"] if offset is None else offset
    n, c, s = ncs(shape)
    bshape = (1, c) + (1,) * (len(shape) - 2)
    scale = orc.hash_uniform(seed, 2, (c,), 0.5, 2.0).astype(np.float64) * case["spread"]
    centre = scale * (orc.hash_uniform(seed, 3, (c,), -1.0, 1.0).astype(np.float64) + offset / np.sqrt(3.0))
    u = orc.hash_uniform(seed, 1, shape, -1.0, 1.0).astype(np.float64)
    x = (centre.reshape(bshape) + scale.reshape(bshape) * u).astype(np.float32)
    cot = orc.hash_normal(seed, 4, shape)
    weight = bias = None
    if case["affine"]:
        weight = orc.hash_uniform(seed, 5, (c,), 0.25, 2.0) * np.where(np.arange(c) % 2 == 0, 1.0, -1.0).astype(np.float32)
        if case["weights"] == "zero":
            weight[1] = 0.0
        bias = orc.hash_uniform(seed, 6, (c,), -0.5, 0.5)
    running_mean, running_var = orc.hash_uniform(seed, 7, (c,), -0.5, 0.5), orc.hash_uniform(seed, 8, (c,), 0.5, 1.5)
    if not case["training"]:       # eval mode normalises with these: keep them near the data's, so that |y| stays near 2
        running_mean = (centre + 0.2 * running_mean).astype(np.float32)
        running_var = (scale * scale / 3.0 * (0.3 + running_var)).astype(np.float32)
    return dict(x=x, cot=cot, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var)


def restate(x, cot, weight, bias, running_mean, running_var, training=True, momentum=0.1, eps=EPS, activation="leaky_relu",
            slope=SLOPE):
    """fp64: dict of FIELDS (dweight / dbias None when weight / bias are) + "pre" (the pre-activation) and "invstd"."""
    f8 = np.float64
    shape = x.shape
    n, c, s = ncs(shape)
    x3, g3 = np.asarray(x, f8).reshape(n, c, s), np.asarray(cot, f8).reshape(n, c, s)
    rm, rv = np.asarray(running_mean, f8), np.asarray(running_var, f8)
    count = n * s
    if training:
        mean, var = x3.mean(axis=(0, 2)), x3.var(axis=(0, 2))
        new_rm = (1.0 - momentum) * rm + momentum * mean
        new_rv = (1.0 - momentum) * rv + momentum * var * count / (count - 1)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    invstd = np.where((var != 0) | (eps != 0), 1.0 / np.sqrt(var + eps), 0.0)
    gamma = np.abs(np.asarray(weight, f8)) + eps if weight is not None else np.ones(c)
    beta = np.asarray(bias, f8) if bias is not None else np.zeros(c)
    col = lambda v: v.reshape(1, c, 1)        # noqa: E731
    y = (x3 - col(mean)) * col(invstd)
    pre = y * col(gamma) + col(beta)
    if activation == "leaky_relu":
        out, slope_at = np.where(pre < 0, pre * slope, pre), np.where(pre < 0, slope, 1.0)
    elif activation == "elu":
        out, slope_at = np.where(pre < 0, np.expm1(pre), pre), np.where(pre < 0, np.exp(pre), 1.0)
    else:
        out, slope_at = pre, np.ones_like(pre)
    du = g3 * slope_at
    if training:
        sum_du, sum_ydu = du.sum(axis=(0, 2)), (y * du).sum(axis=(0, 2))
        dx = col(gamma * invstd) * (du - col(sum_du / count) - y * col(sum_ydu / count))
    else:
        sum_du, sum_ydu = np.zeros(c), np.zeros(c)
        dx = col(gamma * invstd) * du
    res = dict(out=out.reshape(shape), dx=dx.reshape(shape), running_mean=new_rm, running_var=new_rv, pre=pre.reshape(shape),
               invstd=invstd, eydz=sum_ydu / count,
               dweight=None if weight is None else np.sign(np.asarray(weight, f8)) * sum_ydu,
               dbias=None if bias is None else sum_du)
    return res


def restate_case(case, inputs=None, offset=None):
    inp = make_inputs(case, offset) if inputs is None else inputs
    return restate(inp["x"], inp["cot"], inp["weight"], inp["bias"], inp["running_mean"], inp["running_var"], case["training"],
                   case["momentum"], case["eps"], case["activation"], case["slope"])


def max_err(got, want):
    """max |got - want| / max |want| (an all-zero `want` asks for exact zeros: any difference is infinite)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.isfinite(got).all():
        return float("inf")
    d, m = float(np.abs(got - want).max()), float(np.abs(want).max())
    return 0.0 if d == 0.0 else (float("inf") if m == 0.0 else d / m)


def zero_channels(weight):
    return [] if weight is None else [int(i) for i in np.nonzero(np.asarray(weight) == 0)[0]]


def zero_channel_dx_bar(want, ch, eps, bar):
    """The absolute bar on dx of a channel whose weight is exactly 0 (gamma = eps).  The backward recovers y = (z' - beta) / eps
    from the stored output, z' the activation undone.  Half an ulp of the stored z is 2^-24 max|z|; undoing elu multiplies it by
    1 / (1 + z) <= 2 (pre-activations of such a channel are beta >= -0.5) and adds log1p's own ulp or two, the subtraction of
    beta one more: 4 x 2^-24 max(|z|, |pre|) on z' - beta, so 4 x 2^-24 max(|z|, |pre|) / eps on y.  dx picks that up as
    err(y) |eydz| gamma invstd, gamma = eps: the eps cancels, which is why the bar is in terms of eps invstd times the channel's
    own quantities.  eydz is a mean of those same y, so as much again: 8 x 2^-24 max(|z|, |pre|) |eydz| invstd — plus the ordinary
    relative bar on the channel's own largest dx.  Everything is taken from the restatement, nothing from the code under test;
    the channel's dx itself is of order eps invstd max|dz|, 1e-5 of its neighbours'."""
    zmax = max(float(np.abs(want["out"][:, ch]).max()), float(np.abs(want["pre"][:, ch]).max()))
    return 8.0 * 2.0 ** -24 * zmax * abs(float(want["eydz"][ch])) * float(want["invstd"][ch]) + bar * float(np.abs(want["dx"][:, ch]).max())


def compare(got, want, weight, bar, eps=EPS, index=None):
    """{field: error / bar} for every field present in `got` — a value <= 1 passes.  dx of a zero-weight channel is taken out of
    the relative measure and held to zero_channel_dx_bar; dweight there must be exactly 0.  index: flat indices into out / dx when
    `got` holds a sub-sample of them."""
    res = {}
    zc = zero_channels(weight)
    for f in FIELDS:
        if f not in got or got[f] is None:
            continue
        g, w = np.asarray(got[f], np.float64), np.asarray(want[f], np.float64)
        if f in ("out", "dx") and index is not None:
            res[f] = max_err(g, w.reshape(-1)[index]) / bar
            continue
        if f == "dx" and zc:
            keep = [i for i in range(w.shape[1]) if i not in zc]
            res[f] = max_err(g[:, keep], w[:, keep]) / bar
            for ch in zc:
                res["dx_zero_channel_%d" % ch] = float(np.abs(g[:, ch] - w[:, ch]).max()) / zero_channel_dx_bar(want, ch, eps, bar)
            continue
        if f == "dweight" and zc:
            res["dweight_zero_exact"] = 0.0 if all(g[ch] == 0.0 for ch in zc) else float("inf")
        res[f] = max_err(g, w) / bar
    return res

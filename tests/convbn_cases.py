"""The encoder's convolutions (include/cspn_convbn.h) restated in numpy, the a-priori bounds, and the cases tests/test_convbn.py and
tests/golden/make_golden_g30.py run.

    acc[n,q,y,x] = sum_{ky,kx} sum_c w[q,c,ky,kx] x[n, c, s y + ky - k//2, s x + kx - k//2]      (outside the frame: nothing)
    out = act( acc * scale[q] + shift[q]  [+ r[n,q,y,x]] )

for k = 1 or 3 and stride s = 1 or 2, written tap by tap on strided slices of x: torch's conv2d(stride=s, padding=k // 2) checks the
restatement (tests/test_convbn.py), golden G30 (the reference's encoder blocks in fp64) checks it composed per block, and it checks
the kernel.

The bounds are uptail_cases' with the term count of this convolution.  fp32: an fp32 sum of n terms in any order, fused or not, is
within gamma_n sum |terms| of the exact one, gamma_n = n u / (1 - n u), u = 2^-24.  An output is k k C products summed (k k C
roundings of the chain), one fused multiply-add with scale and shift (one) and one add of r (one): n = k k C + 3 covers them,
    |got - exact| <= gamma_n (|scale| sum |w x| + |shift| + |r|),
and n + 4 where scale and shift were themselves folded on the device.  The ReLU does not enlarge a difference.
fp16: inputs are fp16 values, products exact, every fp32 addition only assumed faithful (u' = 2^-23), the epilogue in fp32 and one
conversion:
    E = gamma'_n (|scale| sum |w x| + |shift| + |r|),     |got - y| <= E + 2^-11 (|y| + E) + 2^-25.
"""
import functools

import numpy as np

from uphalf_cases import HALF_MAX, gamma_faithful, to_half
from upconv_cases import fold, gamma

__all__ = ["restate", "restate_half", "bound", "bound_half", "fold", "to_half", "HALF_MAX", "out_size"]

# what the issue lists
CHANNELS = (1, 3, 32, 33, 67)
OUTS = (1, 3, 33, 64, 129)
SHAPES = ((1, 1, 1), (1, 1, 2), (1, 2, 1), (3, 3, 4), (2, 5, 7), (3, 7, 9), (1, 15, 19))
KS = ((1, 1), (1, 2), (3, 1), (3, 2))                       # (k, stride)
BIG = dict(C=40, O=40, shape=(2, 18, 22))                   # several pixel tiles, two chunks per tap
WIDE = dict(C=3, O=257, shape=(2, 5, 7))                    # three M tiles
RAGGED = dict(C=33, O=129, shape=(3, 7, 9), k=3, s=2)       # partly filled last chunk, a second M tile with one live row, odd H and W
# real-valued (C, O, shape): the ragged case, the widest map on the largest frame, a padding-dominated chunk, and BIG
REAL_CASES = ((33, 129, (3, 7, 9)), (67, 33, (1, 15, 19)), (3, 3, (2, 5, 7)), (BIG["C"], BIG["O"], BIG["shape"]))
# every combination of residual, ReLU and affine map
EPILOGUES = tuple((res, relu, affine) for res in (True, False) for relu in (True, False) for affine in (True, False))

# golden G30: name -> (what, planes, inplanes, stride, with a downsample branch, (N, H, W), integer-valued)
GOLDEN_CASES = {}
for _kind in ("Bottleneck", "BasicBlock"):
    _e = 4 if _kind == "Bottleneck" else 1
    for _tag, _integer, _n, _hw, _planes in (("int", True, 2, (5, 7), 2), ("real", False, 2, (9, 13), 3)):
        GOLDEN_CASES["%s_%s_plain" % (_tag, _kind.lower())] = (_kind, _planes, _planes * _e, 1, False, (_n,) + _hw, _integer)
        GOLDEN_CASES["%s_%s_down" % (_tag, _kind.lower())] = (_kind, _planes, 5, 2, True, (_n,) + _hw, _integer)
GOLDEN_CASES["int_bridge"] = ("bridge", 6, 6, 1, False, (2, 4, 5), True)
GOLDEN_CASES["real_bridge"] = ("bridge", 7, 7, 1, False, (2, 8, 10), False)


def out_size(n, s):
    return (n - 1) // s + 1


def accumulate(x, w, s=1):
    """acc [N, O, Ho, Wo] in the dtype of `x`: tap by tap, row-major."""
    N, C, H, W = x.shape
    O, Cw, k, kw = w.shape
    assert Cw == C and k == kw and k in (1, 3) and s in (1, 2)
    Ho, Wo = out_size(H, s), out_size(W, s)
    acc = np.zeros((N, O, Ho, Wo), x.dtype)
    for ky in range(k):
        for kx in range(k):
            dy, dx = ky - k // 2, kx - k // 2
            # outputs whose neighbour exists: 0 <= s y + dy < H
            y0, y1 = (max(0, -dy) + s - 1) // s, min(Ho, (H - 1 - dy) // s + 1)
            x0, x1 = (max(0, -dx) + s - 1) // s, min(Wo, (W - 1 - dx) // s + 1)
            if y0 >= y1 or x0 >= x1:
                continue
            src = x[:, :, s * y0 + dy:s * (y1 - 1) + dy + 1:s, s * x0 + dx:s * (x1 - 1) + dx + 1:s]
            acc[:, :, y0:y1, x0:x1] += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], src, optimize=True)      # a matrix product per tap
    return acc


def epilogue(acc, scale, shift, r, relu):
    y = acc if scale is None else acc * np.asarray(scale, acc.dtype)[None, :, None, None] + np.asarray(shift, acc.dtype)[None, :, None, None]
    if r is not None:
        y = y + r.astype(acc.dtype)
    return np.where(y < 0, 0, y) if relu else y                     # a NaN stays a NaN


def restate(x, w, s=1, scale=None, shift=None, r=None, relu=True, dtype=np.float64):
    """out [N, O, Ho, Wo] in `dtype`."""
    return epilogue(accumulate(x.astype(dtype), w.astype(dtype), s), scale, shift, r, relu)


def restate_half(x, w, s=1, scale=None, shift=None, r=None, relu=True):
    """(out rounded once to fp16, the fp64 values it was rounded from) on x, w and r rounded to fp16."""
    exact = restate(to_half(x), to_half(w), s, scale, shift, None if r is None else to_half(r), relu)
    with np.errstate(over="ignore"):
        return exact.astype(np.float16), exact


def _terms(x, w, s, scale, shift, r):
    A = accumulate(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), s)
    O = w.shape[0]
    scale = np.ones(O) if scale is None else np.abs(np.asarray(scale, np.float64))
    shift = np.zeros(O) if shift is None else np.abs(np.asarray(shift, np.float64))
    return scale[None, :, None, None] * A + shift[None, :, None, None] + (0 if r is None else np.abs(r.astype(np.float64)))


def terms_count(w):
    return w.shape[2] * w.shape[3] * w.shape[1] + 3


def bound(x, w, s, scale, shift, r, extra=0):
    """Per-element fp32 bound [N, O, Ho, Wo] for restate(x, w, s, scale, shift, r, ...); extra = 4 with the fold on the device."""
    return gamma(terms_count(w) + extra) * _terms(x, w, s, scale, shift, r)


def bound_half(x, w, s, scale, shift, r, relu=True, extra=0):
    """Per-element bound [N, O, Ho, Wo] on |kernel - y|, y the fp64 restatement of the fp16-rounded inputs."""
    x, w, r = to_half(x), to_half(w), None if r is None else to_half(r)
    y = np.abs(restate(x, w, s, scale, shift, r, relu))
    E = gamma_faithful(terms_count(w) + extra) * _terms(x, w, s, scale, shift, r)
    return E + 2.0 ** -11 * (y + E) + 2.0 ** -25


@functools.lru_cache(maxsize=None)
def make_inputs(C, O, shape, k, s, integer):
    """x, w, scale, shift, r as fp32 arrays; a fixed function of its arguments.  Integer-valued: x and w in -2 .. 2, so |acc| <=
    9 * 67 * 4 < 2^24 and every fp32 partial sum, the affine map (scale a power of two, shift and r small integers) and the add are
    exact; tests/test_convbn.py asserts for every row that the results are fp16 values too.  scale[0] < 0 with shift[0] = -0.0 makes
    -0 of an exact zero sum."""
    N, H, W = shape
    rng = np.random.RandomState((C * 131 + O * 17 + N * 7 + H * 5 + W * 3 + k * 1009 + s * 2003 + integer) % (2 ** 31))
    Ho, Wo = out_size(H, s), out_size(W, s)
    if integer:
        x = rng.randint(-2, 3, size=(N, C, H, W)).astype(np.float32)
        w = rng.randint(-2, 3, size=(O, C, k, k)).astype(np.float32)
        scale = rng.choice(np.array([0.5, 1, 2, -4], np.float32), size=O)
        shift = rng.randint(-5, 6, size=O).astype(np.float32)
        scale[0], shift[0] = -4.0, -0.0
        r = rng.randint(-8, 9, size=(N, O, Ho, Wo)).astype(np.float32)
    else:
        x = rng.standard_normal((N, C, H, W)).astype(np.float32)
        w = rng.standard_normal((O, C, k, k)).astype(np.float32)
        scale = (rng.standard_normal(O) + 1.5).astype(np.float32)
        shift = rng.standard_normal(O).astype(np.float32)
        r = rng.standard_normal((N, O, Ho, Wo)).astype(np.float32)
    return x, w, scale, shift, r


def integer_cases(shape, k, s):
    """Every integer-valued case of one (N, H, W) and one (k, s): the issue's product of input and output channels."""
    return [(C, O, shape, k, s) for C in CHANNELS for O in OUTS]


EXTRA_INTEGER_CASES = tuple((d["C"], d["O"], d["shape"], k, s) for d in (BIG, WIDE) for k, s in KS)


def block_steps(z):
    """A golden of G30 as conv_bn_act steps in the order the fused block runs them: (input key, w, stride, scale, shift, residual
    key or None, relu, result key), over the arrays of the golden; "x" is the block's input."""
    eps = float(z["eps"])
    kind = str(z["kind"])
    stride = int(z["geom"][0])

    def step(src, conv, bn, s, res, relu, dst):
        return (src, z["w_" + conv], s, *fold(*z["bn_" + bn], eps), res, relu, dst)

    if kind == "bridge":
        return [step("x", "conv2", "bn2", 1, None, False, "y")]
    down = "w_downsample" in z
    steps = []
    if kind == "Bottleneck":
        steps += [step("x", "conv1", "bn1", 1, None, True, "out1"), step("out1", "conv2", "bn2", stride, None, True, "out2")]
        last = ("out2", "conv3", "bn3", 1)
    else:
        steps += [step("x", "conv1", "bn1", stride, None, True, "out1")]
        last = ("out1", "conv2", "bn2", 1)
    if down:
        steps.append(step("x", "downsample", "downsample", stride, None, False, "shortcut"))
    steps.append(step(*last, "shortcut" if down else "x", True, "y"))
    return steps

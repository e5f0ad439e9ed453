"""The 3x3 tail of the decoder blocks (include/cspn_uptail.h) restated in numpy, the a-priori bounds, and the cases
tests/test_uptail.py and tests/golden/make_golden_g29.py run.

    acc[n,q,y,x] = sum_{ky,kx} ( sum_{c<Ca} w[q,c,ky,kx] a[n,c,y+ky-1,x+kx-1] + sum_{c<Cb} w[q,Ca+c,ky,kx] b[n,c,y+ky-1,x+kx-1] )
    out = act( acc * scale[q] + shift[q]  [+ r[n,q,y,x]] )

written tap by tap on the two maps — the concatenation is never formed, so torch's conv2d on the concatenated input checks the
restatement (tests/test_uptail.py), golden G29 (the reference's blocks in fp64) checks it too, and it checks the kernel.

The bounds.  fp32 (upconv_cases.bound's reasoning): an fp32 sum of n terms in any order, fused or not, is within gamma_n sum |terms|
of the exact one, gamma_n = n u / (1 - n u), u = 2^-24.  An output is 9 (Ca + Cb) products summed, one product with scale, one sum
with shift and one with r: n = 9 (Ca + Cb) + 4 covers them,
    |got - exact| <= gamma_n (|scale| sum |w x| + |shift| + |r|),
and n + 4 where scale and shift were themselves folded on the device.  The ReLU does not enlarge a difference.
fp16 (uphalf_cases.bound_half's reasoning): inputs are fp16 values, products exact, every fp32 addition only assumed faithful
(u' = 2^-23), the epilogue in fp32 and one conversion:
    E = gamma'_n (|scale| sum |w x| + |shift| + |r|),     |got - y| <= E + 2^-11 (|y| + E) + 2^-25.
"""
import functools

import numpy as np

from uphalf_cases import HALF_MAX, gamma_faithful, to_half
from upconv_cases import fold, gamma

__all__ = ["restate", "restate_half", "bound", "bound_half", "fold", "to_half", "HALF_MAX"]

# what the issue lists
CHANNELS = ((1, 0), (3, 0), (32, 0), (33, 0), (67, 0), (1, 1), (3, 5), (32, 32), (33, 40), (67, 1))
OUTS = (1, 3, 33, 64, 129)
SHAPES = ((1, 1, 1), (1, 1, 2), (1, 2, 1), (3, 3, 4), (2, 5, 7), (3, 7, 9), (1, 15, 19))
BIG = dict(channels=(40, 40), O=40, shape=(2, 18, 22))
# real-valued: both maps with partly filled last chunks over two M tiles and the tile that ends inside a frame; the widest single
# map beside one channel; a single padding-dominated chunk per map; and BIG
REAL_CASES = (((33, 40), 129, (3, 7, 9)), ((67, 1), 33, (1, 15, 19)), ((3, 5), 3, (2, 5, 7)), (BIG["channels"], BIG["O"], BIG["shape"]))
# every combination of residual, ReLU and affine map
EPILOGUES = tuple((res, relu, affine) for res in (True, False) for relu in (True, False) for affine in (True, False))

# golden G29: name -> (block, N, O (= the channels of every map), (H, W), integer-valued)
GOLDEN_CASES = {}
for _hw, _n, _o in (((1, 1), 1, 2), ((2, 3), 3, 3), ((6, 8), 2, 4), ((4, 5), 2, 3)):
    for _kind in ("Gudi_UpProj_Block", "Gudi_UpProj_Block_Cat"):
        GOLDEN_CASES["int_%s_%dx%d" % ("cat" if _kind.endswith("Cat") else "plain", _hw[0], _hw[1])] = (_kind, _n, _o, _hw, True)
for _hw, _n, _o in (((9, 13), 2, 5), ((15, 19), 1, 6)):
    for _kind in ("Gudi_UpProj_Block", "Gudi_UpProj_Block_Cat"):
        GOLDEN_CASES["real_%s_%dx%d" % ("cat" if _kind.endswith("Cat") else "plain", _hw[0], _hw[1])] = (_kind, _n, _o, _hw, False)


def accumulate(a, b, w):
    """acc [N, O, H, W] in the dtype of `a`: tap by tap, map a then map b (None: one map)."""
    N, Ca, H, W = a.shape
    assert w.shape[1] == Ca + (0 if b is None else b.shape[1]) and w.shape[2:] == (3, 3)
    acc = np.zeros((N, w.shape[0], H, W), a.dtype)
    for ky in range(3):
        for kx in range(3):
            dy, dx = ky - 1, kx - 1
            y0, y1, x0, x1 = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)      # outputs whose neighbour exists
            if y0 >= y1 or x0 >= x1:
                continue
            for src, c0 in ((a, 0), (b, Ca)):
                if src is not None:
                    acc[:, :, y0:y1, x0:x1] += np.einsum("oc,nchw->nohw", w[:, c0:c0 + src.shape[1], ky, kx],
                                                         src[:, :, y0 + dy:y1 + dy, x0 + dx:x1 + dx])
    return acc


def epilogue(acc, scale, shift, r, relu):
    y = acc if scale is None else acc * np.asarray(scale, acc.dtype)[None, :, None, None] + np.asarray(shift, acc.dtype)[None, :, None, None]
    if r is not None:
        y = y + r.astype(acc.dtype)
    return np.where(y < 0, 0, y) if relu else y                     # a NaN stays a NaN


def restate(a, b, w, scale=None, shift=None, r=None, relu=True, dtype=np.float64):
    """out [N, O, H, W] in `dtype`."""
    return epilogue(accumulate(a.astype(dtype), None if b is None else b.astype(dtype), w.astype(dtype)), scale, shift, r, relu)


def restate_half(a, b, w, scale=None, shift=None, r=None, relu=True):
    """(out rounded once to fp16, the fp64 values it was rounded from) on a, b, w and r rounded to fp16."""
    exact = restate(to_half(a), None if b is None else to_half(b), to_half(w), scale, shift, None if r is None else to_half(r), relu)
    with np.errstate(over="ignore"):
        return exact.astype(np.float16), exact


def _terms(a, b, w, scale, shift, r):
    A = accumulate(np.abs(a.astype(np.float64)), None if b is None else np.abs(b.astype(np.float64)), np.abs(w.astype(np.float64)))
    O = w.shape[0]
    scale = np.ones(O) if scale is None else np.abs(np.asarray(scale, np.float64))
    shift = np.zeros(O) if shift is None else np.abs(np.asarray(shift, np.float64))
    return scale[None, :, None, None] * A + shift[None, :, None, None] + (0 if r is None else np.abs(r.astype(np.float64)))


def bound(a, b, w, scale, shift, r, extra=0):
    """Per-element fp32 bound [N, O, H, W] for restate(a, b, w, scale, shift, r, ...); extra = 4 with the fold on the device."""
    return gamma(9 * w.shape[1] + 4 + extra) * _terms(a, b, w, scale, shift, r)


def bound_half(a, b, w, scale, shift, r, relu=True, extra=0):
    """Per-element bound [N, O, H, W] on |kernel - y|, y the fp64 restatement of the fp16-rounded inputs."""
    a, b, w, r = to_half(a), None if b is None else to_half(b), to_half(w), None if r is None else to_half(r)
    y = np.abs(restate(a, b, w, scale, shift, r, relu))
    E = gamma_faithful(9 * w.shape[1] + 4 + extra) * _terms(a, b, w, scale, shift, r)
    return E + 2.0 ** -11 * (y + E) + 2.0 ** -25


@functools.lru_cache(maxsize=None)
def make_inputs(channels, O, shape, integer):
    """a, b (None with Cb = 0), w, scale, shift, r as fp32 arrays; a fixed function of its arguments.  Integer-valued: |acc| <=
    9 * 107 * 9 < 2^24 and |4 acc| + 5 + 8 < 65504, so every fp32 partial sum, the affine map and the add are exact and the result
    lies in the fp16 range; scale[0] < 0 with shift[0] = -0.0 makes -0 of an exact zero sum."""
    Ca, Cb = channels
    N, H, W = shape
    rng = np.random.RandomState((Ca * 131 + Cb * 31 + O * 17 + N * 7 + H * 5 + W * 3 + integer) % (2 ** 31))
    if integer:
        a, b = (rng.randint(-3, 4, size=(N, c, H, W)).astype(np.float32) for c in channels)
        w = rng.randint(-3, 4, size=(O, Ca + Cb, 3, 3)).astype(np.float32)
        scale = rng.choice(np.array([0.5, 1, 2, -4], np.float32), size=O)
        shift = rng.randint(-5, 6, size=O).astype(np.float32)
        scale[0], shift[0] = -4.0, -0.0
        r = rng.randint(-8, 9, size=(N, O, H, W)).astype(np.float32)
    else:
        a, b = (rng.standard_normal((N, c, H, W)).astype(np.float32) for c in channels)
        w = rng.standard_normal((O, Ca + Cb, 3, 3)).astype(np.float32)
        scale = (rng.standard_normal(O) + 1.5).astype(np.float32)
        shift = rng.standard_normal(O).astype(np.float32)
        r = rng.standard_normal((N, O, H, W)).astype(np.float32)
    return a, (b if Cb else None), w, scale, shift, r


def integer_cases(shape):
    """Every integer-valued case of one (N, H, W): the issue's product of channel pairs and output channels."""
    return [(channels, O, shape) for channels in CHANNELS for O in OUTS]

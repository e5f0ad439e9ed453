"""The split products of the fused decoder-block head (include/cspn_upconv.h, dtype CSPN_UPCONV_F32_BF16X3) restated in numpy, and
the cases tests/test_upsplit.py runs.

bf16 is taken by bit masking: the upper 16 bits of an fp32 word after adding 0x7FFF + (bit 16), which rounds to nearest even.  The
split of a value v, as the header states it:

    v1 = bf16(v),   v2 = bf16(v - v1),   v3 = bf16(v - v1 - v2)        both subtractions in fp32, where they are exact

and a product x w becomes the six terms w_i x_j with i + j <= 4.  Geometry, phases and the epilogue are upconv_cases'.
"""
import numpy as np

import upconv_cases as uc

TERMS = ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 1))      # (filter term, pixel term), the kernel's order within a block
DROPPED = 2.0 ** -23 + 2.0 ** -32                             # |x2 w3 + x3 w2 + x3 w3| <= DROPPED |x w|
U_FAITHFUL = 2.0 ** -23                                       # the order inside a matrix instruction is not documented (uphalf_cases)

CHANNELS = (1, 3, 5, 33, 67)                                  # one, two and three chunks of 32, ragged ends
FILTER_SETS = uc.FILTER_SETS
REAL_CASES = uc.REAL_CASES


def bf16(v):
    """fp32 -> the nearest bf16 (ties to even), as fp32.  Finite values below bf16's overflow threshold."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def split(v):
    """(v1, v2, v3) as fp32 arrays."""
    v = np.ascontiguousarray(v, np.float32)
    v1 = bf16(v)
    r1 = v - v1
    v2 = bf16(r1)
    return v1, v2, bf16(r1 - v2)


def six_terms(x, ws, oh, ow, absolute=False):
    """The six partial accumulations [6][N, sum O, oh, ow] in fp64, in the order of TERMS (of absolute values: their sizes)."""
    xs = [t.astype(np.float64) for t in split(x)]
    wss = [[t.astype(np.float64) for t in split(w)] for w in ws]
    if absolute:
        xs, wss = [np.abs(t) for t in xs], [[np.abs(t) for t in w] for w in wss]
    return [uc.accumulate(xs[j - 1], [w[i - 1] for w in wss], oh, ow) for i, j in TERMS]


def gamma_faithful(n):
    return n * U_FAITHFUL / (1 - n * U_FAITHFUL)


def bound(x, ws, oh, ow, scale, shift, extra=0):
    """|got - fp64| <= gamma'_n (|scale| A + |shift|) + (2^-23 + 2^-32) |scale| A per element, A = sum |w x|, n = 6 taps C + 3
    (+ extra: 4 where the batch norms were folded on the device).  Six fp32-exact products per (tap, channel) summed in fp32 by
    faithful additions, one product with scale and one sum with shift (upconv_cases.bound says where the + 3 comes from); the
    second term is what the three dropped products of every x w add up to at most."""
    C = x.shape[1]
    A = uc.accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], oh, ow)
    total = A.shape[1]
    scale = np.ones(total) if scale is None else np.abs(np.asarray(scale, np.float64))
    shift = np.zeros(total) if shift is None else np.abs(np.asarray(shift, np.float64))
    g = np.zeros((oh, ow))
    for a, b in uc.PHASES:
        g[a::2, b::2] = gamma_faithful(6 * uc.PHASE_TAPS[(a, b)] * C + 3 + extra)
    sA = scale[None, :, None, None] * A
    return g[None, None] * (sA + shift[None, :, None, None]) + DROPPED * sA


# The dyadic-exact cases: values whose split has few non-zero terms, so that every kept product class is pinned by bits.
#   a   x = s (1 + k 2^-9 + l 2^-17), w an integer in [-2, 2]          x has three terms, w one: classes (1,1) (1,2) (1,3)
#   b   the roles swapped                                                                       (1,1) (2,1) (3,1)
#   c   x and w both s (1 + k 2^-9)                                                             (1,1) (1,2) (2,1) (2,2)
# s in {-1, 0, 1}; k, l in {1, 2, 3}.  The dropped classes (2,3) (3,2) (3,3) are zero, so the six-term sum is the exact product sum;
# every term is a multiple of 2^-18, and with sum |terms| < 2^6 every partial sum in any order has at most 24 significant bits.
DYADIC_KINDS = ("a", "b", "c")
DYADIC_GEOMETRIES = (((5, 7), (9, 13)), ((6, 7), (4, 5)), ((8, 10), (15, 19)))
DYADIC_DENSE_CHANNELS = (1, 2, 3)
DYADIC_SPARSE = (67, (0, 33, 66))                              # C, the non-zero channels: one per chunk of 32


def _fine(rng, size, third):
    s = rng.randint(-1, 2, size=size).astype(np.float64)
    v = 1 + rng.randint(1, 4, size=size) * 2.0 ** -9
    if third:
        v = v + rng.randint(1, 4, size=size) * 2.0 ** -17
    return (s * v).astype(np.float32)


def dyadic_inputs(kind, seed, shape, filters, live=None):
    """x and the filters (fp32).  live: the channels that are not zero (None: all)."""
    rng = np.random.RandomState(seed)
    C = shape[1]
    wshapes = [(o, C, 5, 5) for o in filters]
    if kind == "a":
        x, ws = _fine(rng, shape, True), [rng.randint(-2, 3, size=s).astype(np.float32) for s in wshapes]
    elif kind == "b":
        x, ws = rng.randint(-2, 3, size=shape).astype(np.float32), [_fine(rng, s, True) for s in wshapes]
    else:
        x, ws = _fine(rng, shape, False), [_fine(rng, s, False) for s in wshapes]
    if live is not None:
        dead = np.setdiff1d(np.arange(C), live)
        x[:, dead] = 0
        for w in ws:
            w[:, dead] = 0
    return x, ws


def grain(a):
    """The smallest g with a 2^g integer-valued (0 for an all-zero array)."""
    a = np.asarray(a, np.float64)
    for g in range(64):
        if np.array_equal(np.floor(a * 2.0 ** g), a * 2.0 ** g):
            return g
    raise AssertionError("not dyadic")

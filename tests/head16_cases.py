"""The half-precision fused output heads (include/cspn_head16.h): the cases tests/test_head16.py runs, the reference and the a-priori
bound it holds the kernel to.

The reference is heads_cases.forward — the formula on the compact map, held to golden G26 by tests/test_heads.py — in fp64 on inputs
rounded to fp16 (what the kernel is given), rounded ONCE to fp16: numpy's float64 -> float16 conversion rounds to nearest even
directly, with overflow to +-Inf, as the kernel's fp32 -> fp16 conversion does.  On integer-valued inputs with |y| < 2048 over the
absolute values every product and partial sum is exact in fp32 and the result is a fp16 value, so the kernel gives the reference's
bits.

The bound of the real-valued checks, derived as uphalf_cases.bound_half.  The products of fp16 values are exact in fp32; what is
rounded is the fp32 additions and the final conversion.  How v_mfma_f32_16x16x32_f16 rounds the additions inside one instruction is
not documented, so every fp32 addition is only assumed to be a faithful rounding: u' = 2^-23 in place of 2^-24 (Higham, Accuracy
and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1 holds for any |delta| <= u').  With
    n = taps C + 3, taps the phase's 1, 2, 2 or 4,   gamma'_n = n u' / (1 - n u'),   A = the formula on the absolute values,
    E = gamma'_n A
the fp32 value before the conversion is within E of the exact y, and the conversion adds half an ulp of fp16 of that value:
    |got - y| <= E + 2^-11 (|y| + E) + 2^-25
(2^-11 (|y| + E): a normal result; 2^-25: half the spacing of the fp16 subnormals).
"""
import numpy as np

import heads_cases as hc
from cspn_monodepth_amd import _lib

TH, TW, KC = _lib.HEAD16_TILE_H, _lib.HEAD16_TILE_W, _lib.HEAD16_CHANNEL_BLOCK      # the kernel's tile of compact pixels, its channel block
MAX_OUT = _lib.HEAD16_MAX_OUT_CHANNELS
U_FAITHFUL = 2.0 ** -23
HALF_MAX = 65504.0
PHASE_TAPS = {(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4}

CHANNELS = (1, 3, 5, 64, 67)              # below, at and above two channel blocks
BATCHES = (1, 3)
HEAD_SETS = hc.HEAD_SETS + tuple((o,) for o in range(1, MAX_OUT + 1))      # and every flat total as a single head


def _geometries():
    """name -> (H, W, oh, ow), named from the tile: Hc = ceil(oh / 2) x Wc = ceil(ow / 2) compact pixels take part."""
    g = {
        "one_tile_exact_even": (TH, TW, 2 * TH, 2 * TW),
        "one_tile_exact_odd": (TH, TW, 2 * TH - 1, 2 * TW - 1),
        "one_below_the_edge_even": (TH - 1, TW - 1, 2 * TH - 2, 2 * TW - 2),
        "one_below_the_edge_odd": (TH - 1, TW - 1, 2 * TH - 3, 2 * TW - 3),
        "one_above_the_edge_even": (TH + 1, TW + 1, 2 * TH + 2, 2 * TW + 2),      # 2 x 2 tiles, the last of one pixel
        "one_above_the_edge_odd": (TH + 1, TW + 1, 2 * TH + 1, 2 * TW + 1),
        "neighbour_cropped_away": (TH + 1, TW + 1, 2 * TH, 2 * TW),               # x goes on past the tile, the crop does not
        "neighbour_cropped_in_x_only": (TH + 1, TW + 8, 2 * TH + 1, 2 * TW + 2),
        # two and three tiles in each direction, one direction at a time (the table is a product over 210 rows per geometry)
        "two_tiles_down_exact": (2 * TH, 5, 4 * TH, 10),
        "two_tiles_across_exact": (3, 2 * TW, 6, 4 * TW),
        "three_tiles_down_last_of_one": (2 * TH + 1, 5, 4 * TH + 1, 9),
        "three_tiles_across_last_of_one": (3, 2 * TW + 1, 5, 4 * TW + 1),
        "three_tiles_down_exact": (3 * TH, 4, 6 * TH, 8),
        "three_tiles_across_exact": (2, 3 * TW, 4, 6 * TW),
        "three_tiles_down_ragged": (2 * TH + 5, 6, 4 * TH + 8, 11),                # a row of x past the crop
        "three_tiles_across_ragged": (3, 2 * TW + 9, 6, 4 * TW + 15),             # a column of x past the crop
        "deep_crop": (6, 7, 4, 5),
        "one_px_1x1": (1, 1, 1, 1),
        "one_px_2x2": (1, 1, 2, 2),
    }
    return g


GEOMETRIES = _geometries()
# 3 x 3 tiles, the last ragged in both directions, a row and a column of x past the crop, even oh and odd ow: the case of the
# guard-band, poisoned-LDS and determinism tests, and — with hc.HEAD_SETS — one more row of the integer table
RAGGED = (2 * TH + 5, 2 * TW + 9, 4 * TH + 8, 4 * TW + 15)


def to_half(a):
    """Rounded to fp16 (to nearest even) and back to the array's own dtype: the values the kernel is given."""
    a = np.asarray(a)
    return a.astype(np.float16).astype(a.dtype)


def gamma_faithful(n):
    return n * U_FAITHFUL / (1 - n * U_FAITHFUL)


def make_inputs(shape, heads, integer, seed=0):
    """x and the filters as fp32 arrays of fp16 values; a fixed function of its arguments.  Integer-valued: {-1, 0, 1} from 64
    channels on and {-3 .. 3} below, so that 4 C max|x| max|w| — the largest |y| over absolute values — stays below 2048."""
    N, C, H, W = shape
    rng = np.random.RandomState((seed * 7919 + sum(shape) * 131 + H * 17 + W * 7 + sum(heads) * 3 + len(heads)) % (2 ** 31))
    lim = 1 if C >= 64 else 3

    def draw(*s):
        if integer:
            return rng.randint(-lim, lim + 1, size=s).astype(np.float32)
        return to_half(rng.standard_normal(s).astype(np.float32))

    return draw(N, C, H, W), [draw(o, C, 3, 3) for o in heads]


def reference(x, ws, oh, ow):
    """(the outputs in fp16, one per head; the fp64 values they were rounded from).  x and ws are rounded to fp16 first."""
    exact = hc.forward(to_half(x).astype(np.float64), [to_half(w).astype(np.float64) for w in ws], oh, ow)
    with np.errstate(over="ignore"):
        return [y.astype(np.float16) for y in exact], exact


def absolute_run(x, ws, oh, ow):
    """The formula on the absolute values of the fp16-rounded inputs: every partial sum of every output lies below it."""
    return hc.forward(np.abs(to_half(x).astype(np.float64)), [np.abs(to_half(w).astype(np.float64)) for w in ws], oh, ow)


def bound_half(x, ws, oh, ow):
    """Per head, the per-element bound on |kernel - y|, y the fp64 reference on the fp16-rounded inputs (the docstring)."""
    C = x.shape[1]
    g = np.zeros((oh, ow))
    for (a, b), taps in PHASE_TAPS.items():
        g[a::2, b::2] = gamma_faithful(taps * C + 3)
    exact = reference(x, ws, oh, ow)[1]
    return [g[None, None] * A + 2.0 ** -11 * (np.abs(y) + g[None, None] * A) + 2.0 ** -25 for y, A in zip(exact, absolute_run(x, ws, oh, ow))]


def integer_case(shape, out_hw, heads):
    """(x, ws, the reference's fp16 outputs, the largest |y| over absolute values) of an integer-valued case."""
    x, ws = make_inputs(shape, heads, True)
    want, _ = reference(x, ws, *out_hw)
    worst = max(float(a.max()) for a in absolute_run(x, ws, *out_hw))
    return x, ws, want, worst


def table_cases(name):
    """The integer table at one geometry: every head set x CHANNELS x BATCHES."""
    H, W, oh, ow = GEOMETRIES[name]
    return [((B, C, H, W), (oh, ow), heads) for heads in HEAD_SETS for C in CHANNELS for B in BATCHES]

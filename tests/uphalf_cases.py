"""The half-precision fused decoder-block head (include/cspn_uphalf.h) restated in numpy, on top of tests/upconv_cases.py, and the
a-priori bound tests/test_uphalf.py holds the kernel to.

The restatement: x and the filters rounded to fp16 (what the kernel is given), the four-phase formula of upconv_cases.restate on
those values in fp64, and ONE rounding of the result to fp16 — numpy's float64 -> float16 conversion rounds to nearest even directly,
with overflow to +-Inf, as the kernel's fp32 -> fp16 conversion does.  On integer-valued inputs every product and every partial sum
is exact in fp32 (|acc| <= 9 * 67 * 9 < 2^24), so is the affine map (|y| <= 4 * 5427 + 5), and the kernel has to give the
restatement's bits.

The bound of the real-valued checks.  The products of fp16 values are exact in fp32; what is rounded is the fp32 additions, the
fused multiply-add of the epilogue and the final conversion.  How v_mfma_f32_32x32x16_f16 rounds the 16 additions inside one
instruction is not documented, so every fp32 addition is only assumed to be a faithful rounding: u' = 2^-23 in place of the 2^-24 of
round-to-nearest (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Lemma 3.1 holds for any |delta| <= u').  With
    n  = taps C + 3 (+ 4 where the batch norms were folded on the device), taps the phase's 9, 6, 6 or 4, as upconv_cases.bound
    E  = gamma'_n (|scale| A + |shift|),   gamma'_n = n u' / (1 - n u'),   A = the restatement on the absolute values
the fp32 value before the conversion is within E of the exact y, and the conversion adds half an ulp of fp16 of that value:
    |got - y| <= E + 2^-11 (|y| + E) + 2^-25
(2^-11 (|y| + E): a normal result; 2^-25: half the spacing of the fp16 subnormals).  The ReLU does not enlarge a difference.
"""
import functools

import numpy as np

import upconv_cases as uc

U_FAITHFUL = 2.0 ** -23
HALF_MAX = 65504.0


def to_half(a):
    """Rounded to fp16 (to nearest even) and back to the array's own dtype: the values the kernel is given."""
    a = np.asarray(a)
    return a.astype(np.float16).astype(a.dtype)


def gamma_faithful(n):
    return n * U_FAITHFUL / (1 - n * U_FAITHFUL)


def restate_half(x, ws, oh, ow, scale=None, shift=None, relu_channels=0):
    """(the outputs in fp16, one per filter; the fp64 values they were rounded from).  x and ws are rounded to fp16 first."""
    exact = uc.restate(to_half(x), [to_half(w) for w in ws], oh, ow, scale, shift, relu_channels)
    with np.errstate(over="ignore"):
        return [y.astype(np.float16) for y in exact], exact


def bound_half(x, ws, oh, ow, scale, shift, relu_channels=0, extra=0):
    """Per-element bound [N, sum O, oh, ow] on |kernel - y|, y the fp64 restatement of the fp16-rounded inputs (the docstring)."""
    x, ws = to_half(x), [to_half(w) for w in ws]
    C = x.shape[1]
    y = np.abs(np.concatenate(uc.restate(x, ws, oh, ow, scale, shift, relu_channels), 1))
    A = uc.accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], oh, ow)
    total = A.shape[1]
    scale = np.ones(total) if scale is None else np.abs(np.asarray(scale, np.float64))
    shift = np.zeros(total) if shift is None else np.abs(np.asarray(shift, np.float64))
    g = np.zeros((oh, ow))
    for a, b in uc.PHASES:
        g[a::2, b::2] = gamma_faithful(uc.PHASE_TAPS[(a, b)] * C + 3 + extra)
    E = g[None, None] * (scale[None, :, None, None] * A + shift[None, :, None, None])
    return E + 2.0 ** -11 * (y + E) + 2.0 ** -25


def relu_boundaries(filters):
    return sorted({0, filters[0], sum(filters)})


def integer_shapes():
    """Every integer-valued case the GPU test runs: the issue's product, and BIG."""
    for (hw, out_hw) in uc.GEOMETRIES:
        for C in uc.CHANNELS:
            for both in uc.FILTER_SETS:
                for B in uc.BATCHES:
                    yield (B, C) + hw, out_hw, uc.filters_of(both)
    yield uc.BIG["shape"], uc.BIG["out_hw"], uc.BIG["filters"]


@functools.lru_cache(maxsize=None)
def integer_case(shape, out_hw, filters):
    """The inputs of an integer-valued case (upconv_cases.make_inputs: all of them fp16 values already) and the largest |acc|."""
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters), shape, filters, True)
    assert np.array_equal(to_half(x), x) and all(np.array_equal(to_half(w), w) for w in ws)
    acc = uc.accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], *out_hw)
    return x, ws, scale, shift, float(acc.max())


@functools.lru_cache(maxsize=None)
def real_case(shape, out_hw, both):
    """The inputs of a real-valued case of upconv_cases.REAL_CASES, x and the filters rounded to fp16."""
    filters = uc.filters_of(both)
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters) + 1, shape, filters, False)
    return to_half(x), [to_half(w) for w in ws], scale, shift, filters

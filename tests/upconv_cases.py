"""The fused decoder-block head (include/cspn_upconv.h) restated in numpy, and the cases tests/test_upconv.py and
tests/golden/make_golden_g27.py run.

The formula is written on the COMPACT map, phase by phase, as the header states it — not through the un-pooled map the reference
builds — so that golden G27 (the reference's blocks in fp64, eval mode) checks the restatement and the restatement checks the kernel
on the shapes no golden covers.  Output pixel (2i + a, 2j + b) of a pad-2 5x5 window over the un-pooled map meets the compact map
through the taps (ky, kx) with a + ky and b + kx even, at compact pixel (i + (a + ky - 2) / 2, j + (b + kx - 2) / 2):

    phase (0,0): 3 x 3 taps   (0,1): 3 x 2   (1,0): 2 x 3   (1,1): 2 x 2          25 products per compact pixel and channel pair

A compact pixel takes part iff 2i < oh and 2j < ow; a neighbour that does not exist contributes nothing.  Then, per flat output
channel q over both filters, y = acc * scale[q] + shift[q] and max(y, 0) for q < relu_channels.

Every function keeps the dtype it is given (fp64 for the references; integer-valued inputs are exact in any float type).
"""
import numpy as np

PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))
PHASE_TAPS = {(0, 0): 9, (0, 1): 6, (1, 0): 6, (1, 1): 4}

# what the issue lists: C, (O1, O2), compact H x W -> oh x ow, B
CHANNELS = (1, 3, 5, 67)
FILTER_SETS = ((1, 0), (3, 3), (17, 16), (33, 0))
GEOMETRIES = (((1, 1), (1, 1)), ((1, 1), (2, 2)), ((1, 2), (2, 3)), ((2, 1), (3, 2)), ((3, 4), (6, 8)), ((5, 7), (9, 13)),
              ((6, 7), (4, 5)), ((8, 10), (15, 19)))
BATCHES = (1, 3)
# K spans several LDS chunks of 32 channels per tap, and the pixels of every phase span several tiles of 128
BIG = dict(shape=(2, 40, 9, 11), out_hw=(18, 22), filters=(40, 40))

# More than one 128-row tile of flat output channels (mt > 0 in fwd<P>; every case above has at most 80): a second tile with one live
# row; the filter boundary and the ReLU boundary inside tile 1; the boundary on the tile edge, and three tiles; the boundary in tile 0
# with live rows in tile 1.  Run at C = 3 and 33 (one chunk, and a second one partly filled), B = 2, bit for bit, by the three
# precisions' test_integer_cases_over_several_m_tiles.
M_TILE_FILTER_SETS = ((129, 0), (130, 31), (128, 129), (100, 60))
M_TILE_GEOMETRIES = (((3, 4), (6, 8)), ((5, 7), (9, 13)))
M_TILE_CHANNELS = (3, 33)
M_TILE_BATCH = 2


def m_tile_shapes():
    """shape, out_hw, filters of every case over several M tiles."""
    for hw, out_hw in M_TILE_GEOMETRIES:
        for C in M_TILE_CHANNELS:
            for both in M_TILE_FILTER_SETS:
                yield (M_TILE_BATCH, C) + hw, out_hw, filters_of(both)


# the case the poisoned-LDS runs take: ragged in M (130 + 31 = 161 = 128 + 33), in K (33 = 32 + 1) and in the pixels of every phase
M_TILE_POISON_CASE = ((M_TILE_BATCH, 33, 5, 7), (9, 13), (130, 31))

# The integer-valued test runs the whole product of the four lists (a test per geometry), and BIG.
# The real-valued cases that are no golden: the odd crop at C = 67 (three 32-channel chunks per tap, the last one partly filled)
# with two filters, the widest single filter, and the big one.
REAL_CASES = (((3, 67, 8, 10), (15, 19), (17, 16)), ((1, 5, 5, 7), (9, 13), (33, 0)), (BIG["shape"], BIG["out_hw"], BIG["filters"]))

# golden G27: name -> (block, (N, C, H, W), (oh, ow), out_channels, integer-valued)
GOLDEN_CASES = {
    "int_one_px_1x1": ("Simple_Gudi_UpConv_Block", (1, 1, 1, 1), (1, 1), 1, True),
    "int_one_px_2x2": ("Gudi_UpProj_Block", (1, 1, 1, 1), (2, 2), 3, True),
    "int_1x2": ("Gudi_UpProj_Block_Cat", (3, 3, 1, 2), (2, 3), 3, True),
    "int_2x1": ("Gudi_UpProj_Block", (1, 5, 2, 1), (3, 2), 2, True),
    "int_3x4": ("Gudi_UpProj_Block_Cat", (3, 5, 3, 4), (6, 8), 4, True),
    "int_deep_crop": ("Gudi_UpProj_Block", (2, 3, 6, 7), (4, 5), 3, True),
    "int_odd_crop_c3": ("Gudi_UpProj_Block_Cat", (1, 3, 8, 10), (15, 19), 2, True),
    "real_5x7": ("Gudi_UpProj_Block", (3, 5, 5, 7), (9, 13), 6, False),
    "real_deep_crop": ("Gudi_UpProj_Block_Cat", (2, 3, 6, 7), (4, 5), 5, False),
    "real_odd_crop_c3": ("Gudi_UpProj_Block_Cat", (1, 3, 8, 10), (15, 19), 17, False),
    "real_simple": ("Simple_Gudi_UpConv_Block", (2, 7, 3, 4), (6, 7), 9, False),
}


def filters_of(out_channels):
    """(O1, O2) -> the out_channels of the filters that exist."""
    return tuple(o for o in out_channels if o)


def make_inputs(seed, shape, filters, integer):
    """x, filters, scale, shift as fp32 arrays (what the device gets); a fixed function of its arguments."""
    rng = np.random.RandomState(seed)
    N, C, H, W = shape
    total = sum(filters)
    if integer:
        x = rng.randint(-3, 4, size=shape).astype(np.float32)
        ws = [rng.randint(-3, 4, size=(o, C, 5, 5)).astype(np.float32) for o in filters]
        scale = rng.choice(np.array([0.5, 1, 2, -4], np.float32), size=total)
        shift = rng.randint(-5, 6, size=total).astype(np.float32)
    else:
        x = rng.standard_normal(shape).astype(np.float32)
        ws = [rng.standard_normal((o, C, 5, 5)).astype(np.float32) for o in filters]
        scale = (rng.standard_normal(total) + 1.5).astype(np.float32)
        shift = rng.standard_normal(total).astype(np.float32)
    return x, ws, scale, shift


def case_seed(shape, out_hw, filters):
    return (sum(shape) * 131 + out_hw[0] * 17 + out_hw[1] * 7 + sum(filters) * 3 + len(filters)) % (2 ** 31)


def _phase_axis(a, n_out, n_compact):
    """For one axis of phase a: the output positions 2i + a < n_out, and per tap k (a + k even) the pair (positions of i that have
    the neighbour i + d, d = (a + k - 2) / 2, among the n_compact compact pixels that take part; those neighbours)."""
    i = np.arange((n_out + 1 - a) // 2)
    taps = []
    for k in range(5):
        if (a + k) % 2 == 0:
            d = (a + k - 2) // 2
            ok = (i + d >= 0) & (i + d < n_compact)
            taps.append((k, i[ok], i[ok] + d))
    return i, taps


def accumulate(x, ws, oh, ow):
    """acc [N, sum O, oh, ow]: the un-pooled 5x5 convolutions of all filters, from the compact map."""
    w = np.concatenate(ws, 0)
    N = x.shape[0]
    acc = np.zeros((N, w.shape[0], oh, ow), x.dtype)
    Hc, Wc = (oh + 1) // 2, (ow + 1) // 2
    for a, b in PHASES:
        i, rows = _phase_axis(a, oh, Hc)
        j, cols = _phase_axis(b, ow, Wc)
        assert len(rows) * len(cols) == PHASE_TAPS[(a, b)]
        if not (i.size and j.size):
            continue
        part = np.zeros((N, w.shape[0], i.size, j.size), x.dtype)
        for ky, ii, si in rows:
            for kx, jj, sj in cols:
                if ii.size and jj.size:
                    part[np.ix_(range(N), range(w.shape[0]), ii, jj)] += np.einsum("oc,ncij->noij", w[:, :, ky, kx], x[np.ix_(range(N), range(x.shape[1]), si, sj)])
        acc[:, :, a::2, b::2] = part
    return acc


def restate(x, ws, oh, ow, scale=None, shift=None, relu_channels=0, dtype=np.float64):
    """The outputs, one per filter, in `dtype`."""
    x, ws = x.astype(dtype), [w.astype(dtype) for w in ws]
    y = accumulate(x, ws, oh, ow)
    if scale is not None:
        y = y * np.asarray(scale, dtype)[None, :, None, None] + np.asarray(shift, dtype)[None, :, None, None]
    y[:, :relu_channels] = np.where(y[:, :relu_channels] < 0, 0, y[:, :relu_channels])
    cuts = np.cumsum([w.shape[0] for w in ws])[:-1]
    return np.split(y, cuts, axis=1)


def fold(gamma, beta, mean, var, eps):
    """The eval-mode batch norm as scale, shift (fp64)."""
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return scale, np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale


# The a-priori bound of the real-valued checks.  An fp32 sum of n products in any order, with or without fused multiply-adds, differs
# from the exact one by at most gamma_n * sum |terms|, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of
# Numerical Algorithms, 2nd ed., Lemma 3.1 and eq. 3.5).  Here an output is acc * scale + shift: at most 9 C products summed, one
# product with scale and one sum with shift — n = taps C + 3 covers them with room for fused or unfused forms — so
#     |got - exact| <= gamma_n * (|scale| * sum |w x| + |shift|),     n = taps * C + 3, taps the phase's 9, 6, 6 or 4;
# the ReLU does not enlarge a difference.  With the batch norms folded on the device scale and shift are themselves rounded results
# of a handful of fp32 operations (sqrt, divide, multiply, subtract): n + 4.
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def bound(x, ws, oh, ow, scale, shift, extra=0):
    """Per-element bound [N, sum O, oh, ow] for restate(x, ws, oh, ow, scale, shift, ...)."""
    C = x.shape[1]
    A = accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], oh, ow)
    total = A.shape[1]
    scale = np.ones(total) if scale is None else np.abs(np.asarray(scale, np.float64))
    shift = np.zeros(total) if shift is None else np.abs(np.asarray(shift, np.float64))
    g = np.zeros((oh, ow))
    for a, b in PHASES:
        g[a::2, b::2] = gamma(PHASE_TAPS[(a, b)] * C + 3 + extra)
    return g[None, None] * (scale[None, :, None, None] * A + shift[None, :, None, None])

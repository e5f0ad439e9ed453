"""The fused output heads (include/cspn_heads.h) restated in numpy, and the cases tests/test_heads.py and
tests/golden/make_golden_g26.py run.

The three formulas are written on the COMPACT map, as the header states them — not through the un-pooled map the reference builds
— so that golden G26 (the reference's un-pool + conv2d and its autograd, in fp64) checks the restatement and the restatement
checks the kernels on the shapes no golden covers:

    y_h[n,o,2i+1-ky,2j+1-kx] += w_h[o,c,ky,kx] x[n,c,i,j]            over 2i < oh, 2j < ow and the target inside oh x ow
    gx[n,c,i,j]               = sum w_h[o,c,ky,kx] gy_h[n,o,2i+1-ky,2j+1-kx]      (0 where the crop removed (2i, 2j))
    gw_h[o,c,ky,kx]           = sum gy_h[n,o,2i+1-ky,2j+1-kx] x[n,c,i,j]

Every function keeps the dtype it is given (fp64 for the references; integer-valued inputs are exact in any float type).
"""
import numpy as np

# (N, C, H, W), (oh, ow) of the integer-valued cases
INT_SHAPES = (
    ((1, 1, 1, 1), (1, 1)), ((1, 1, 1, 1), (2, 2)),
    ((2, 3, 3, 5), (5, 9)), ((2, 3, 3, 5), (6, 10)), ((2, 3, 3, 5), (6, 9)),
    ((1, 64, 9, 11), (17, 22)),
    ((3, 5, 19, 37), (37, 74)), ((3, 5, 19, 37), (38, 73)),      # more than one block of 256 compact pixels, odd crops
    ((1, 64, 114, 152), (228, 304)),
    ((2, 3, 6, 7), (4, 5)),                                      # a deep crop: most of x takes no part
)
HEAD_SETS = ((1,), (8,), (1, 8), (1, 12), (4, 4, 4, 4))

# golden G26: name -> ((N, C, H, W), (oh, ow), heads, integer-valued)
GOLDEN_CASES = {
    "int_one_px_1x1": ((1, 1, 1, 1), (1, 1), (1,), True),
    "int_one_px_2x2": ((1, 1, 1, 1), (2, 2), (8,), True),
    "int_5x9": ((2, 3, 3, 5), (5, 9), (1, 8), True),
    "int_6x10": ((2, 3, 3, 5), (6, 10), (1, 12), True),
    "int_6x9": ((2, 3, 3, 5), (6, 9), (4, 4, 4, 4), True),
    "int_deep_crop": ((2, 3, 6, 7), (4, 5), (1, 8), True),
    "real_6x9": ((2, 3, 3, 5), (6, 9), (1, 8), False),
    "real_deep_crop": ((2, 3, 6, 7), (4, 5), (1, 12), False),
    "real_c64": ((1, 64, 9, 11), (17, 22), (1, 8), False),
    "real_blocks": ((1, 5, 19, 37), (37, 73), (1, 4), False),   # three blocks of compact pixels, odd crop
}


# The tiling constants of csrc/cspn_heads.hip, restated: a weight-gradient workgroup takes one 64-pixel segment of a compact row at a
# time and 64 channels (its grid is capped at 1024 workgroups, each walking segments s, s + 1024, ...), the input gradient holds 32
# channels per pass, and the kernels exist for 1 .. 16 flat output channels.
GW_PX, GW_CB, GX_CB, GW_MAX_GROUPS, MAX_OUT = 64, 64, 32, 1024, 16


def segments(N, oh, ow):
    """Row segments of the weight gradient: frames x compact rows that take part x 64-pixel pieces of such a row."""
    return N * ((oh + 1) // 2) * -(-((ow + 1) // 2) // GW_PX)


def _coverage_cases():
    """name -> ((N, C, H, W), (oh, ow), heads): integer-valued cases named for the branch of the kernels each is there for."""
    rows = {}
    # every instantiation of heads_fwd / heads_gx / heads_gw (a workgroup of 16 OT threads): two width segments (64 + 6), two channel
    # blocks (64 + 1), three 32-channel passes of gx with one channel in the last, odd ow
    for ot in range(1, MAX_OUT + 1):
        rows["ot%d" % ot] = ((1, 65, 2, 70), (3, 139), (ot,))
    # several heads flattened to OT = 3, 10, 11, 14, 15: the frame strides of the heads differ
    for heads in ((2, 1), (3, 4, 3), (5, 6), (2, 3, 5, 4), (7, 8)):
        rows["split_" + "x".join(map(str, heads))] = ((2, 5, 4, 6), (7, 11), heads)
    # ragged and exact ends of the 32- and 64-channel blocks
    for C in (31, 32, 33, 63, 65, 97, 128, 130):
        rows["c%d" % C] = ((2, C, 3, 5), (5, 9), (1, 8))
    # a last segment of 63, 64 and 1 pixels, `left` of a later segment from real data, even and odd ow
    for Wc in (63, 64, 65, 128, 129):
        rows["w%d_even" % Wc] = ((1, 3, 2, Wc), (4, 2 * Wc), (1, 4))
        rows["w%d_odd" % Wc] = ((1, 3, 2, Wc), (3, 2 * Wc - 1), (1, 4))
    # more segments than workgroups: workgroups with 3 and with 2 trips, crossing frames; and with two segments per row, where only
    # workgroups 0 .. 15 take a second trip
    rows["segs_2560"] = ((5, 3, 512, 2), (1023, 3), (1, 8))
    rows["segs_1040_w65"] = ((2, 3, 260, 65), (519, 130), (3,))
    return rows


COVERAGE_CASES = _coverage_cases()
SPLIT_TOTALS = (3, 10, 11, 14, 15)


def make_inputs(seed, shape, out_hw, heads, integer):
    """x, weights, output gradients as fp32 arrays (what the device gets); a fixed function of its arguments."""
    rng = np.random.RandomState(seed)
    N, C, H, W = shape

    def draw(*s):
        if integer:
            return rng.randint(-3, 4, size=s).astype(np.float32)
        return rng.standard_normal(s).astype(np.float32)

    x = draw(N, C, H, W)
    ws = [draw(o, C, 3, 3) for o in heads]
    gys = [draw(N, o, out_hw[0], out_hw[1]) for o in heads]
    return x, ws, gys


def case_seed(shape, out_hw, heads):
    return (sum(shape) * 131 + out_hw[0] * 17 + out_hw[1] * 7 + sum(heads) * 3 + len(heads)) % (2 ** 31)


def _tap(k, o):
    """Compact indices i with 2i < o whose tap k lands inside [0, o), and where it lands: 2i + 1 - k."""
    i = np.arange((o + 1) // 2)
    t = 2 * i + 1 - k
    ok = (t >= 0) & (t < o)
    return i[ok], t[ok]


def _taps(oh, ow):
    for ky in range(3):
        i, Y = _tap(ky, oh)
        for kx in range(3):
            j, X = _tap(kx, ow)
            if i.size and j.size:
                yield ky, kx, np.ix_(i, j), np.ix_(Y, X)


def forward(x, ws, oh, ow):
    outs = []
    for w in ws:
        y = np.zeros((x.shape[0], w.shape[0], oh, ow), x.dtype)
        for ky, kx, (i, j), (Y, X) in _taps(oh, ow):
            y[:, :, Y, X] += np.einsum("oc,ncij->noij", w[:, :, ky, kx], x[:, :, i, j])
        outs.append(y)
    return outs


def grad_x(x_shape, ws, gys, oh, ow):
    gx = np.zeros(x_shape, ws[0].dtype)
    for w, gy in zip(ws, gys):
        for ky, kx, (i, j), (Y, X) in _taps(oh, ow):
            gx[:, :, i, j] += np.einsum("oc,noij->ncij", w[:, :, ky, kx], gy[:, :, Y, X])
    return gx


def grad_w(x, gys, oh, ow):
    gws = []
    for gy in gys:
        gw = np.zeros((gy.shape[1], x.shape[1], 3, 3), x.dtype)
        for ky, kx, (i, j), (Y, X) in _taps(oh, ow):
            gw[:, :, ky, kx] = np.einsum("noij,ncij->oc", gy[:, :, Y, X], x[:, :, i, j])
        gws.append(gw)
    return gws


def restate(x, ws, gys, oh, ow, dtype=np.float64):
    """(outputs, gx, gws) in `dtype`."""
    x, ws, gys = x.astype(dtype), [w.astype(dtype) for w in ws], [g.astype(dtype) for g in gys]
    return forward(x, ws, oh, ow), grad_x(x.shape, ws, gys, oh, ow), grad_w(x, gys, oh, ow)


# The a-priori bound of the real-valued checks.  A sum of n products formed in fp32 in any order, with or without fused multiply-adds,
# differs from the exact sum by at most gamma_n * sum |terms| with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and
# Stability of Numerical Algorithms, 2nd ed., eq. 3.5 with Lemma 3.1); rounding the fp64 reference's own result adds 2^-53 per term
# and is far below it.  The tests use n * 2^-24 * A, A = the same sum over absolute values (the golden's "absolute run"), with
#   n = 4 C for an output (a 2 x 2 block position reads at most 4 compact pixels per channel),
#   n = 9 * (output channels over all heads) for gx,   n = N H W for gw.
U = 2.0 ** -24


def terms_forward(C):
    return 4 * C


def terms_grad_x(heads):
    return 9 * sum(heads)


def terms_grad_w(shape):
    return shape[0] * shape[2] * shape[3]

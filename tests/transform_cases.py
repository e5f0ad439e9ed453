"""Cases, seeded inputs and the numpy restatement of the NYU train / val transforms (cspn_monodepth_amd/dataloaders/nyu_dataloader/
nyu_dataloader.py, include/cspn_transform.h), shared by tests/golden/make_golden_g22.py and tests/test_transforms.py.

The restatement is written from the semantics, not from the reference's file: Pillow's nearest resize is a running-sum index table,
scipy's order-0 rotation a rounded affine map with the validity range [0, n-1], the crop Python's round, the jitter Pillow's blend in
C float.  Every step is a gather or integer / single-rounded arithmetic, so the G22 fixtures — the reference's own outputs — must equal
it bit for bit, and so must the device.  numpy rounds every elementwise operation on its own (no fused multiply-add): the device code has
to switch contraction off to do the same.  One step is not a plain copy: a train frame's depth goes through scipy's order-0 sum
`t = 0; t += v`, which turns a -0 into +0.

A frame's parameters are one row of 8 fp64: s, angle (degrees), flip, brightness, contrast, saturation factor, order code, reserved.
The order code numbers the permutations of (brightness, contrast, saturation) lexicographically; -1: no jitter."""
import hashlib
import itertools

import numpy as np

from sparsify_cases import philox4x32_10

MAX_FILE_BYTES = 89617          # the largest G20 fixture: no G21 / G22 file is larger
P_S, P_ANGLE, P_FLIP, P_BRIGHTNESS, P_CONTRAST, P_SATURATION, P_ORDER, P_RESERVED = range(8)
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION = 0, 1, 2
ORDERS = list(itertools.permutations((OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION)))      # code 0..5, lexicographic
GATHER_THREADS = 256            # pixels of a frame one workgroup of the gather pass covers (one integer partial of L each)


def P(s, angle, flip, fb=1.0, fc=1.0, fs=1.0, order=-1):
    return [float(s), float(angle), float(flip), float(fb), float(fc), float(fs), float(order), 0.0]


# name -> raw (H, W), first (the first resize factor), out (oh, ow), mode, params (a row per frame; val: the number of frames),
# seed, depth kind ("plain" / "hostile"), rgb kind ("random" / "half": mean L of the cropped frame is exactly k + 0.5)
CASES = {
    # 8 x 12 -> 6 x 9 -> crop 4 x 6: identity without jitter; up-scaled, rotated, flipped, jittered; a third with another order
    "tiny_8x12": dict(raw=(8, 12), first=0.75, out=(4, 6), mode="train", seed=2201, depth="plain", rgb="random", params=[
        P(1.0, 0.0, 0), P(1.25, 3.0, 1, 0.8, 1.3, 0.7, 2), P(1.5, -4.0, 0, 1.4, 0.6, 1.2, 5)]),
    # 48 x 64 -> 25 x 33 (the 64 -> 33 column table differs from the closed form) -> crop 22 x 30; all six op orders
    "orders_48x64": dict(raw=(48, 64), first=25.0 / 48, out=(22, 30), mode="train", seed=2202, depth="plain", rgb="random", params=[
        P(1.07, 2.1, 0, 0.7, 1.3, 0.8, 0), P(1.31, -3.3, 1, 1.2, 0.7, 1.35, 1), P(1.18, 4.4, 1, 0.9, 1.25, 1.1, 2),
        P(1.45, -1.2, 0, 1.38, 1.39, 0.61, 3), P(1.0, 0.7, 1, 0.62, 0.65, 1.4, 4), P(1.26, -4.9, 0, 1.1, 0.9, 0.75, 5)]),
    # factors exactly 1 (Pillow copies), all below 1 (no clipping possible), all above 1 (the clipping branch), jitter off
    "factors_48x64": dict(raw=(48, 64), first=25.0 / 48, out=(22, 30), mode="train", seed=2203, depth="plain", rgb="random", params=[
        P(1.1, 1.5, 0, 1.0, 1.0, 1.0, 3), P(1.2, -2.5, 1, 0.6, 0.6, 0.6, 4), P(1.3, 3.5, 0, 1.4, 1.4, 1.4, 1), P(1.4, -0.5, 1)]),
    # s = 1: the crop reaches the corners the rotation fills with zeros
    "rot5_48x64": dict(raw=(48, 64), first=25.0 / 48, out=(22, 30), mode="train", seed=2204, depth="hostile", rgb="random", params=[
        P(1.0, 5.0, 0, 1.2, 0.8, 1.1, 2), P(1.0, -5.0, 1)]),
    "identity_48x64": dict(raw=(48, 64), first=25.0 / 48, out=(22, 30), mode="train", seed=2205, depth="hostile", rgb="random", params=[
        P(1.0, 0.0, 0), P(1.0, 0.0, 1, 1.1, 1.2, 0.9, 0)]),
    # 120 x 160 -> 63 x 84 -> crop 57 x 76 = 4332 pixels: 17 workgroups of the gather pass, 17 partial sums of L per frame
    "mid_120x160": dict(raw=(120, 160), first=63.0 / 120, out=(57, 76), mode="train", seed=2206, depth="plain", rgb="random", params=[
        P(1.13, -2.7, 1, 1.3, 1.2, 0.7, 3), P(1.41, 3.9, 0, 0.7, 0.8, 1.3, 4)]),
    # grey frame, half the cropped pixels 100 and half 101: mean L = 100.5, the contrast constant is int(100.5 + 0.5) = 101
    "half_mean_8x12": dict(raw=(8, 12), first=0.75, out=(4, 6), mode="train", seed=2207, depth="plain", rgb="half", params=[
        P(1.0, 0.0, 0, 1.0, 1.37, 1.0, 2), P(1.0, 0.0, 1, 1.0, 0.63, 1.0, 3)]),
    "val_48x64": dict(raw=(48, 64), first=24.0 / 48, out=(22, 30), mode="val", seed=2208, depth="hostile", rgb="random", params=2),
    # the reference's own geometry, stored as digests
    "full_train_480x640": dict(raw=(480, 640), first=250.0 / 480, out=(228, 304), mode="train", seed=2209, depth="plain", rgb="random",
                               params=[P(1.23, 3.1, 1, 0.75, 1.33, 1.21, 2), P(1.0, -5.0, 0, 1.3, 0.7, 0.8, 4)]),
    "full_val_480x640": dict(raw=(480, 640), first=240.0 / 480, out=(228, 304), mode="val", seed=2210, depth="plain", rgb="random", params=1),
}
DIGEST_ONLY = ("full_train_480x640", "full_val_480x640")


def n_frames(case):
    return case["params"] if case["mode"] == "val" else len(case["params"])


def params_of(case):
    """fp64 [B,8], or None for a val case"""
    return None if case["mode"] == "val" else np.array(case["params"], np.float64).reshape(-1, 8)


# ------------------------------------------------------------------------------------------------ geometry
def out_len(n, f):
    """the size a float factor gives: the fp64 product, truncated"""
    return int(np.float64(n) * np.float64(f))


def resize_table(n_in, n_out):
    """Pillow's nearest resize: the source index of every output index, a RUNNING SUM in fp64"""
    a = np.float64(n_in) / np.float64(n_out)
    o = a * np.float64(0.5)
    tab = np.empty(n_out, np.int64)
    for i in range(n_out):
        tab[i] = int(o)
        o = o + a
    return tab


def closed_form_table(n_in, n_out):
    """what the running sum is NOT: floor((i + 0.5) * n_in / n_out)"""
    a = np.float64(n_in) / np.float64(n_out)
    return np.floor((np.arange(n_out, dtype=np.float64) + 0.5) * a).astype(np.int64)


def crop_offset(n, o):
    return int(round((n - o) / 2.))             # Python 3: ties to even


def geometry(raw, first, out, s=None):
    """-> h1, w1, h2, w2, i0, j0 (s None: val, no second resize)"""
    h1, w1 = out_len(raw[0], first), out_len(raw[1], first)
    h2, w2 = (h1, w1) if s is None else (out_len(h1, s), out_len(w1, s))
    return h1, w1, h2, w2, crop_offset(h2, out[0]), crop_offset(w2, out[1])


def rotation(angle, h1, w1):
    """-> M00, M01, M10, M11, off0, off1 in fp64, every operation rounded on its own"""
    th = np.deg2rad(np.float64(angle))
    c, sn = np.cos(th), np.sin(th)
    c0, c1 = np.float64(h1) / 2 - 0.5, np.float64(w1) / 2 - 0.5
    off0 = c0 - (c * c0 + sn * c1)
    off1 = c1 - (-sn * c0 + c * c1)
    return c, sn, -sn, c, off0, off1


def rotated_coordinates(p, raw, first, out):
    """-> cy, cx fp64 [oh,ow]: where output pixel (y, x) of a train frame looks in the h1 x w1 image, and h1, w1"""
    h1, w1, h2, w2, i0, j0 = geometry(raw, first, out, p[P_S])
    assert h2 >= out[0] and w2 >= out[1], "the precondition int(h1*s) >= oh, int(w1*s) >= ow"
    rows = resize_table(h1, h2)[i0:i0 + out[0]]
    cols = resize_table(w1, w2)[j0:j0 + out[1]]
    if p[P_FLIP] != 0:
        cols = cols[::-1]
    m00, m01, m10, m11, off0, off1 = rotation(p[P_ANGLE], h1, w1)
    Y, X = rows[:, None].astype(np.float64), cols[None, :].astype(np.float64)
    cy = off0 + Y * m00
    cy = cy + X * m01
    cx = off1 + Y * m10
    cx = cx + X * m11
    return cy, cx, h1, w1


def source_map(p, raw, first, out):
    """-> valid bool [oh,ow], r0, c0 int [oh,ow]: the raw pixel every output pixel copies (p None: val)"""
    if p is None:
        h1, w1, _, _, i0, j0 = geometry(raw, first, out)
        r = resize_table(raw[0], h1)[i0:i0 + out[0]]
        c = resize_table(raw[1], w1)[j0:j0 + out[1]]
        assert r.size == out[0] and c.size == out[1]
        return np.ones(out, bool), np.broadcast_to(r[:, None], out), np.broadcast_to(c[None, :], out)
    cy, cx, h1, w1 = rotated_coordinates(p, raw, first, out)
    valid = (cy >= 0) & (cy <= h1 - 1) & (cx >= 0) & (cx <= w1 - 1)
    sy = np.clip(np.floor(cy + 0.5), 0, h1 - 1).astype(np.int64)
    sx = np.clip(np.floor(cx + 0.5), 0, w1 - 1).astype(np.int64)
    return valid, resize_table(raw[0], h1)[sy], resize_table(raw[1], w1)[sx]


# ------------------------------------------------------------------------------------------------ colour jitter
def luma(img):
    """Pillow's RGB -> L on int [3,h,w]"""
    return (img[0] * 19595 + img[1] * 38470 + img[2] * 7471 + 0x8000) >> 16


def blend(deg, img, f):
    """Pillow's blend(degenerate, img, f), f a C float: int arrays in, int array out"""
    f = np.float32(f)
    t = deg.astype(np.float32) + f * (img - deg).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.int64)


def contrast_constant(img):
    lum = luma(img)
    return int(np.float64(int(lum.sum())) / np.float64(lum.size) + 0.5)


def jitter(img, p):
    """uint8 [3,h,w] -> uint8 [3,h,w]"""
    code = int(p[P_ORDER])
    if code < 0:
        return img
    v = img.astype(np.int64)
    for op in ORDERS[code]:
        if op == OP_BRIGHTNESS:
            v = blend(np.zeros_like(v), v, p[P_BRIGHTNESS])
        elif op == OP_CONTRAST:
            v = blend(np.full_like(v, contrast_constant(v)), v, p[P_CONTRAST])
        else:
            v = blend(np.broadcast_to(luma(v), v.shape), v, p[P_SATURATION])
    return v.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the transform
def restate_frame(rgb, depth, p, raw, first, out):
    """rgb uint8 [3,H,W], depth fp32 [H,W], p a parameter row or None (val) -> rgb fp32 [3,oh,ow], depth fp32 [oh,ow]"""
    assert rgb.dtype == np.uint8 and depth.dtype == np.float32 and rgb.shape == (3,) + tuple(raw) and depth.shape == tuple(raw)
    valid, r0, c0 = source_map(p, raw, first, out)
    if p is not None:
        with np.errstate(all="ignore"):
            depth = depth / np.float32(p[P_S])                                  # fp32 / fp32, before the gather
    picked = depth[r0, c0]
    if p is not None:
        with np.errstate(all="ignore"):
            picked = np.float32(0.0) + picked                                   # scipy's order-0 sum `t = 0; t += v`: a -0 leaves as +0
    words = np.where(valid, picked.view(np.uint32), np.uint32(0))               # otherwise depth moves as 32-bit words
    img = np.where(valid[None], rgb[:, r0, c0], np.uint8(0))
    if p is not None:
        img = jitter(img, p)
    return (img.astype(np.float64) / 255.0).astype(np.float32), words.astype(np.uint32).view(np.float32)


def restate(rgb, depth, params, first, out):
    """rgb uint8 [B,3,H,W], depth fp32 [B,1,H,W], params fp64 [B,8] or None -> rgb fp32 [B,3,oh,ow], depth fp32 [B,1,oh,ow]"""
    raw = tuple(rgb.shape[2:])
    frames = [restate_frame(rgb[b], depth[b, 0], None if params is None else params[b], raw, first, out) for b in range(rgb.shape[0])]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])[:, None]


def restate_case(case):
    rgb, depth = make_inputs(case)
    return restate(rgb, depth, params_of(case), case["first"], case["out"])


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(case):
    """-> rgb uint8 [B,3,H,W], depth fp32 [B,1,H,W] from the case's seed"""
    B, (H, W) = n_frames(case), case["raw"]
    r = np.random.RandomState(case["seed"])
    rgb = r.randint(0, 256, size=(B, 3, H, W)).astype(np.uint8)
    depth = r.uniform(0.5, 10.0, (B, 1, H, W)).astype(np.float32)
    depth[r.uniform(size=depth.shape) < 0.15] = 0.0
    if case["depth"] == "hostile":              # a quarter of the pixels, so that the few a crop keeps hold every kind
        kinds = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 1e-45, 3.4e38, 0.0], np.float32)
        pick = r.uniform(size=depth.shape) < 0.25
        depth[pick] = kinds[r.randint(0, kinds.size, size=int(pick.sum()))]
    if case["rgb"] == "half":
        params = params_of(case)
        for b in range(B):
            valid, r0, c0 = source_map(params[b], case["raw"], case["first"], case["out"])
            assert valid.all() and np.unique(r0 * W + c0).size == valid.size and valid.size % 2 == 0
            rgb[b] = 100
            half = r.permutation(valid.size)[:valid.size // 2]
            rgb[b][:, r0.reshape(-1)[half], c0.reshape(-1)[half]] = 101
    return rgb, depth


# ------------------------------------------------------------------------------------------------ comparison
def words(a):
    """fp32 -> its 32-bit words with every NaN mapped to one word (a NaN may match any NaN)"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(words(a), words(b))


def digest(rgb, depth):
    return hashlib.sha256(words(rgb).tobytes() + words(depth).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ drawn parameters
def restate_draw(frame_ids, seed):
    """fp64 [B,8]: Philox4x32-10 on the counter (slot, 1, frame id low, frame id high) with the key `seed`; u = (x0 >> 8) * 2^-24"""
    seed = int(seed) & (2 ** 64 - 1)
    rows = []
    for fid in frame_ids:
        fid = int(fid) & (2 ** 64 - 1)
        k = np.arange(7, dtype=np.uint64)
        x0 = philox4x32_10(k, np.ones_like(k), np.full_like(k, fid & 0xFFFFFFFF), np.full_like(k, fid >> 32), seed & 0xFFFFFFFF, seed >> 32)[0]
        u = (x0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        rows.append([1.0 + 0.5 * u[0], -5.0 + 10.0 * u[1], 1.0 if u[2] < 0.5 else 0.0, 0.6 + 0.8 * u[3], 0.6 + 0.8 * u[4], 0.6 + 0.8 * u[5],
                     np.floor(6.0 * u[6]), 0.0])
    return np.array(rows, np.float64).reshape(-1, 8)

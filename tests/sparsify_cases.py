"""Cases, inputs and the numpy restatement of the sparse-depth sampler (cspn_monodepth_amd/dataloaders/nyu_dataloader/
dense_to_sparse.py, include/cspn_sparsify.h), shared by tests/golden/make_golden_g21.py and tests/test_sparsify.py.

The restatement is written from the semantics (keep, per-frame n_keep, prob in fp64, `u < prob`, copy or +0), not from the
reference's file; the G21 fixtures — the reference's own outputs — must equal it bit for bit, and so must the device.

philox4x32_10 is a pure-numpy Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) on uint64 lanes; philox_uniform is the uniform the
kernels derive from it: counter (pixel, 0, frame id low, frame id high), key (seed low, seed high), u = (x0 >> 8) * 2^-24."""
import numpy as np

MAX_FILE_BYTES = 89617          # the largest G20 fixture: no G21 file is larger
SLICE_PIXELS, MAX_SLICES = 1024, 64

# name -> shape (B, H, W), num_samples, max_depth, seed, depth (the kind make_depth builds), u ("seeded": what np.random gives the
# reference, fp64 with 53 random bits; "f32": the same rounded to fp32 before the reference sees it; "hand": written out below),
# rgb (None, "f32", "u8")
CASES = {
    "valid_1x1":          dict(shape=(1, 1, 1), num_samples=1, max_depth=np.inf, seed=2101, depth="one_valid", u="seeded", rgb="f32"),
    "invalid_1x1":        dict(shape=(1, 1, 1), num_samples=1, max_depth=np.inf, seed=2102, depth="one_invalid", u="seeded", rgb="u8"),
    "odd_3x5x7":          dict(shape=(3, 5, 7), num_samples=10, max_depth=np.inf, seed=2103, depth="plain", u="seeded", rgb="f32"),
    "odd_3x5x7_f32u":     dict(shape=(3, 5, 7), num_samples=10, max_depth=np.inf, seed=2104, depth="plain", u="f32", rgb="u8"),
    "empty_middle_3x5x7": dict(shape=(3, 5, 7), num_samples=10, max_depth=np.inf, seed=2105, depth="empty_middle", u="seeded", rgb=None),
    "all_sampled_2x4x6":  dict(shape=(2, 4, 6), num_samples=100, max_depth=np.inf, seed=2106, depth="plain", u="seeded", rgb=None),
    "none_sampled_2x4x6": dict(shape=(2, 4, 6), num_samples=0, max_depth=np.inf, seed=2107, depth="plain", u="seeded", rgb=None),
    "max_depth_2x6x9":    dict(shape=(2, 6, 9), num_samples=5, max_depth=2.7, seed=2108, depth="around_max_depth", u="f32", rgb=None),
    "hostile_2x5x7":      dict(shape=(2, 5, 7), num_samples=12, max_depth=np.inf, seed=2109, depth="hostile", u="seeded", rgb=None),
    "hostile_cut_2x5x7":  dict(shape=(2, 5, 7), num_samples=6, max_depth=6.0, seed=2110, depth="hostile", u="f32", rgb=None),
    "boundary_quarter":   dict(shape=(1, 2, 3), num_samples=1, max_depth=np.inf, seed=2111, depth="four_valid", u="hand", rgb=None),
    # 37 x 41 = 1517 pixels = 380 units of 4: more than the 256 units (1024 pixels) of one count slice, so a frame's n_keep is the
    # sum of TWO partial counts; 1517 is odd, so frame 1 starts 4 bytes off 16-byte alignment and goes element by element
    "two_slices_2x37x41": dict(shape=(2, 37, 41), num_samples=100, max_depth=np.inf, seed=2112, depth="plain", u="seeded", rgb=None),
    # 57 x 76 = 4332 pixels: 5 count slices, 5 workgroups of the apply pass; the quarter-size NYU frame at the reference's 500 samples
    "frame_57x76":        dict(shape=(1, 57, 76), num_samples=500, max_depth=np.inf, seed=2113, depth="plain", u="f32", rgb="u8"),
}
SPANS_SLICES = {"two_slices_2x37x41": 2, "frame_57x76": 5}


def slices(hw):
    return max(1, min(MAX_SLICES, -(-hw // SLICE_PIXELS)))


def make_depth(case):
    """[B,1,H,W] fp32 from the case's seed (a generator of its own: np.random's global state belongs to the reference's draw)."""
    B, H, W = case["shape"]
    r = np.random.RandomState(case["seed"])
    kind = case["depth"]
    d = (r.uniform(0.5, 10.0, (B, 1, H, W))).astype(np.float32)
    d[r.uniform(size=d.shape) < 0.15] = 0.0
    if kind == "one_valid":
        d[...] = 2.5
    elif kind == "one_invalid":
        d[...] = 0.0
    elif kind == "empty_middle":
        d[1] = np.where(r.uniform(size=d[1].shape) < 0.5, 0.0, -1.5).astype(np.float32)
    elif kind == "four_valid":
        d = np.array([1.0, 1.5, 2.0, 2.5, 0.0, -1.0], np.float32).reshape(1, 1, 2, 3)
    elif kind == "around_max_depth":
        md = np.float32(case["max_depth"])
        flat = d.reshape(B, -1)
        for b in range(B):                 # the fp32 neighbours of max_depth, where an fp64 comparison would decide differently
            flat[b, 1], flat[b, 4], flat[b, 8] = md, np.nextafter(md, np.float32(np.inf)), np.nextafter(md, np.float32(0))
    elif kind == "hostile":
        flat = d.reshape(B, -1)
        for b in range(B):
            flat[b, 0:8] = [np.nan, np.inf, -np.inf, -3.0, -0.0, 1e-45, 3.4e38, -np.nan]
            flat[b, 20 + b] = np.inf
    return d


def make_rgb(case):
    """[B,3,H,W] fp32 in [0,1) or uint8 (every value 0..255 present once the planes hold 256 elements), or None."""
    if case["rgb"] is None:
        return None
    B, H, W = case["shape"]
    r = np.random.RandomState(case["seed"] + 5000)
    if case["rgb"] == "f32":
        return r.uniform(size=(B, 3, H, W)).astype(np.float32)
    v = r.randint(0, 256, size=(B, 3, H, W)).astype(np.uint8)
    flat = v.reshape(-1)
    if flat.size >= 256:
        flat[r.permutation(flat.size)[:256]] = np.arange(256, dtype=np.uint8)
    return v


def hand_uniform(case):
    """boundary_quarter: n_keep = 4, num_samples = 1, prob = 0.25 exactly; u == prob is NOT sampled, the double below it is."""
    below = np.nextafter(0.25, 0.0)
    return np.array([0.25, below, 0.25, below, 0.1, 0.1], np.float64).reshape(1, 1, 2, 3)


def restate(depth, u, num_samples, max_depth=np.inf):
    """-> (mask bool [B,1,H,W], sparse fp32 [B,1,H,W]) of depth fp32 [B,1,H,W] and u fp64 [B,1,H,W]."""
    assert depth.dtype == np.float32 and u.dtype == np.float64 and depth.shape == u.shape
    mask = np.zeros(depth.shape, bool)
    with np.errstate(invalid="ignore"):
        for b in range(depth.shape[0]):
            d = depth[b]
            keep = d > 0
            if not np.isposinf(max_depth):
                keep = keep & (d <= np.float32(max_depth))
            n_keep = int(keep.sum())
            if n_keep:
                mask[b] = keep & (u[b] < float(num_samples) / n_keep)
    return mask, np.where(mask, depth, np.float32(0.0)).astype(np.float32)


def restate_rgbd(rgb, plane):
    """[B,4,H,W] fp32: the RGB planes (uint8: (float)(v / 255.0), the division in fp64) and `plane` as channel 3."""
    if rgb.dtype == np.uint8:
        rgb = (rgb.astype(np.float64) / 255).astype(np.float32)
    assert rgb.dtype == np.float32
    return np.concatenate([rgb, plane], axis=1)


def bits(a):
    """the bit pattern of an fp32 / bool / uint8 array, for exact comparison (NaN payloads and -0.0 included)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def fp32_exact(u):
    with np.errstate(invalid="ignore"):
        return np.array_equal(u.astype(np.float32).astype(np.float64), u)


# ------------------------------------------------------------------------------------------------ Philox4x32-10
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays of 32-bit words held in uint64 (the products need 64 bits) -> the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _LO for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _LO, np.uint64(k1) & _LO
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + PHILOX_W0) & _LO, (k1 + PHILOX_W1) & _LO
    return c0, c1, c2, c3


def philox_uniform(hw, frame_id, seed):
    """fp64 [hw]: the uniform of every pixel of the frame with this id under this seed (24 bits, in [0, 1))."""
    fid, seed = int(frame_id) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    p = np.arange(hw, dtype=np.uint64)
    x0 = philox4x32_10(p, np.zeros_like(p), np.full_like(p, fid & 0xFFFFFFFF), np.full_like(p, fid >> 32), seed & 0xFFFFFFFF, seed >> 32)[0]
    return (x0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def philox_plane(shape, frame_ids, seed):
    """fp64 [B,1,H,W] for the frames with these ids."""
    B, H, W = shape
    return np.stack([philox_uniform(H * W, f, seed).reshape(1, H, W) for f in frame_ids])

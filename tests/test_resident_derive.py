"""The weight derive of the resident forward (csrc/cspn_resident.hip, div8_quad_shared_reciprocal / div8_shared_reciprocal of
csrc/cspn_common.hpp) on guidance that drives BOTH sides of the normalisation — the shared refined reciprocal and the true division
behind the wave-uniform test — within one wavefront and within one quad: patches whose normaliser S is below 2^-100, denormal or
above 2^100 among ordinary N(0,1) pixels (the finite inputs), plus S = 0 and +-inf / NaN gates (the hostile inputs), at image
corners, inside tiles, across tile borders and in the halo of the neighbouring tiles.

Every case compares the resident launch (explicit 768-thread plans of 2 x 3 and 3 x 3 tiles of about 32 x 20 pixels, and the
512-thread default) with the multi-launch schedule bit for bit, plain and scored, and with the C oracle at the project's bar of 1e-5
(which also supplies the NaN pattern); the training forward's published weights and S are the bits of cspn3_prepare.  T = 9 and 17:
two and three phases.  The oracle is checked on the CPU first to be defined on these inputs.

Reference: network/libs/post_process/CSPN_new.py:26-92, :124-127."""
import numpy as np
import pytest
import torch

import cspn_monodepth_amd as pkg
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import functional as F
from conftest import bits_equal, lds_poison, golden_names, load_golden, rel_err

DEV = "cuda:0"
B, H = 2, 60
SMALL, DENORMAL, LARGE = 2.0 ** -105, 2.0 ** -131, 2.0 ** 101
# tap j = (dy, dx) row-major without the centre reads channel 7 - j at p + off_j (csrc/cspn_resident.hip)
OFFS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
TILINGS = [(64, 2), (96, 3)]                 # (W, tile columns): 3 tile rows 24 / 17 / 19 high, tile columns 32 wide
TS = [9, 17]


def patches(W):
    """Top-left corners of the 5 x 5 patches: both image corners (clipped to 4 x 4), a tile interior, the corner where four tiles meet
    (rows 22..26 across y = 24, columns 30..34 across x = 32: border pixels of four tiles, halo of all of them), a tile's halo-only
    neighbourhood, the last tile column's interior, the left image edge.  5 wide and not quad-aligned: every patch shares quads
    and wavefronts with ordinary pixels."""
    return [(-1, -1), (H - 4, W - 4), (9, 13), (22, 30), (30, 37), (44, W - 9), (50, -2)]


def make_guidance(c_oracle, W, hostile):
    g = c_oracle.hash_normal(700 + W, 1, (B, 12, H, W))
    scales = (SMALL, DENORMAL, LARGE)
    for b in range(B):
        for k, (y, x) in enumerate(patches(W)):
            ys, xs = slice(max(y, 0), min(y + 5, H)), slice(max(x, 0), min(x + 5, W))
            g[b, :, ys, xs] *= np.float32(scales[(k + b) % 3])
    if hostile:
        g[:, :, 44:47, 9:12] = 0.0                       # S = 0 at (45, 10): all eight gates zero (a tile interior) ...
        g[:, :, 0:2, W - 2:W] = 0.0                      # ... and at the top right image corner
        # single gates: image corners, the point where four tiles meet (border + halo), a tile interior
        for (y, x, c, v) in [(0, 0, 3, np.nan), (H - 1, W - 1, 5, -np.inf), (24, 32, 0, np.inf), (23, 31, 7, -np.inf), (12, 50, 6, np.nan),
                             (13, 50, 1, np.inf)]:
            g[:, c, y, x] = v
    return g


def normaliser(g):
    """S per pixel as the kernels sum it (numpy, any order: for classification only)."""
    S = np.zeros((g.shape[0], H, g.shape[-1]), np.float64)
    pad = np.pad(np.abs(g[:, :8].astype(np.float64)), ((0, 0), (0, 0), (1, 1), (1, 1)))
    for j, (dy, dx) in enumerate(OFFS):
        S += pad[:, 7 - j, 1 + dy:1 + dy + H, 1 + dx:1 + dx + g.shape[-1]]
    return S


_CASES = {}


def case(c_oracle, W, T, sparse, hostile):
    """Host inputs and the oracle's result of a case: computed once, shared, never written."""
    key = (W, T, sparse, hostile)
    if key not in _CASES:
        g = make_guidance(c_oracle, W, hostile)
        d = c_oracle.hash_uniform(710 + W, 2, (B, 1, H, W), 0.0, 10.0)
        s = c_oracle.hash_sparse(720 + W, 3, d, 1.0 / 60.0) if sparse else None
        _CASES[key] = (g, d, s, c_oracle.cspn3_forward(g, d, s, T))
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ CPU: the inputs and the oracle
@pytest.mark.parametrize("W,nx", TILINGS)
def test_inputs_reach_both_sides_of_the_normalisation_in_one_quad(W, nx, c_oracle):
    for hostile in (False, True):
        S = normaliser(make_guidance(c_oracle, W, hostile))
        with np.errstate(invalid="ignore"):
            in_range = ((S >= 2.0 ** -100) & (S <= 2.0 ** 100)) | (S == 0)
            kinds = {"small": (S >= 2.0 ** -126) & (S < 2.0 ** -100), "denormal": (S > 0) & (S < 2.0 ** -126), "large": (S > 2.0 ** 100) & np.isfinite(S)}
            if hostile:
                kinds.update(zero=S == 0, inf=np.isinf(S), nan=np.isnan(S))
        for name, m in kinds.items():
            assert m.any(), (name, hostile)
        quads = in_range.reshape(B, H, W // 4, 4)
        mixed = quads.any(-1) & ~quads.all(-1)               # a quad with pixels on both sides
        assert mixed.sum() >= 8, hostile
        for b in range(B):                                   # ... at the image corners, and across the tile border at x = 32
            assert not in_range[b, 0, 0] and not in_range[b, H - 1, W - 1]
            assert (~in_range[b, 22:27, 28:32]).any() and (~in_range[b, 22:27, 32:36]).any()
            assert (~in_range[b, 22:24, 28:36]).any() and (~in_range[b, 24:27, 28:36]).any()
        if not hostile:
            assert np.isfinite(S).all() and (S > 0).all()


@pytest.mark.parametrize("W,nx", TILINGS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
def test_oracle_is_defined_on_these_inputs(W, nx, T, sparse, c_oracle):
    g, d, s, want = case(c_oracle, W, T, sparse, False)
    assert np.isfinite(want).all()
    # the fp32 oracle is a reference at the bar of 1e-5 here: it stays well inside it against its own fp64 form
    w64 = c_oracle.cspn3_forward(g, d, s, T, dtype=np.float64)
    err = rel_err(want, w64)
    print("fp32 oracle against fp64 oracle: %.2e" % err)
    assert err <= 3e-6
    g, d, s, want = case(c_oracle, W, T, sparse, True)
    nan = np.isnan(want)
    assert nan.any() and not np.isinf(want).any()
    assert np.array_equal(nan, np.isnan(c_oracle.cspn3_forward(g, d, s, T, dtype=np.float64)))
    if T == 9:
        assert (~nan).sum() >= 200                           # the NaNs have not swallowed the image: finite pixels are still compared


# ------------------------------------------------------------------------------------------------ GPU
def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def plan768(nx):
    rp = _lib.cspn_resident_plan()
    rp.steps_per_phase, rp.tiles_x, rp.tiles_y, rp.tile_w, rp.tile_h = 8, nx, 3, 32, 24
    rp.threads, rp.images_per_launch = 768, B
    return rp


def same_bits(a, b, **ctx):
    """bits_equal with NaNs equal to NaNs at the same places (the hostile inputs spread NaNs by design)."""
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return bits_equal(a, b, **ctx)
    z = torch.zeros_like(a)
    return bits_equal(torch.where(na, z, a), torch.where(nb, z, b), **ctx)


_DEVICE = {}


def device_case(c_oracle, W, T, sparse, hostile):
    """Device inputs, the multi-launch result, the scoring target and the metric sums of the multi-launch result."""
    key = (W, T, sparse, hostile)
    if key not in _DEVICE:
        g, d, s, want = case(c_oracle, W, T, sparse, hostile)
        gt, dt, st = dev(g), dev(d), dev(s)
        tgt = np.maximum(d[:, 0] + 0.1 * c_oracle.hash_normal(730 + W, 9, (B, H, W)), 0.0).astype(np.float32)
        tgt[c_oracle.hash_uniform(731 + W, 9, (B, H, W)) < 0.05] = 0.0
        tt = dev(tgt)
        prev = F._RESIDENT_MODE
        F.set_resident("off")
        try:
            with torch.no_grad():
                ref = pkg.CSPN_new.AffinityPropagate(T, 3)(gt, dt, st)[:, 0].contiguous()
        finally:
            F.set_resident(prev)
        sums = pkg.evaluation.new_accumulator(DEV)
        pkg.evaluation.metric_sums(ref, tt, out=sums)
        _DEVICE[key] = (gt, dt[:, 0].contiguous(), None if st is None else st[:, 0].contiguous(), ref, tt, sums.sum(0).cpu().numpy(), want)
    return _DEVICE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("W,nx", TILINGS, ids=["2x3", "3x3"])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
@pytest.mark.parametrize("hostile", [False, True], ids=["finite", "hostile"])
def test_resident_derive_equals_multi_launch_and_oracle(W, nx, T, sparse, hostile, c_oracle):
    gt, d0, sp, ref, tt, ref_sums, want = device_case(c_oracle, W, T, sparse, hostile)
    ctx = dict(T=T, sparse=sparse)
    err = rel_err(ref.cpu().numpy(), want[:, 0])
    print("multi-launch against the oracle: %.2e" % err)
    assert err <= 1e-5                                       # finite: the project's bar; hostile: + the oracle's NaN pattern
    for which, kw in (("768", dict(_plan=plan768(nx))), ("512", dict(threads=512))):
        with torch.no_grad():
            out = F.forward_resident(gt, d0, sp, T, int(sparse), guard=0, **kw)
            acc = pkg.evaluation.new_accumulator(DEV)
            if which == "768":
                kw = dict(_plan=plan768(nx))
            outs = F.forward_resident(gt, d0, sp, T, int(sparse), score=(tt, acc), guard=0, **kw)
        torch.cuda.synchronize()
        F.check_resident_errors()
        assert same_bits(out, ref, which=which, **ctx)
        assert same_bits(outs, ref, which=which + " scored", **ctx)
        err = rel_err(out.cpu().numpy(), want[:, 0])
        print("%s against the oracle: %.2e" % (which, err))
        assert err <= 1e-5
        got = acc.sum(0).cpu().numpy()
        print("scored sums", which, got, ref_sums)
        assert np.allclose(got, ref_sums, rtol=2e-5, equal_nan=True)     # other order of the atomic additions


@pytest.mark.gpu
@pytest.mark.parametrize("W,nx", TILINGS, ids=["2x3", "3x3"])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
@pytest.mark.parametrize("hostile", [False, True], ids=["finite", "hostile"])
def test_training_forward_publishes_the_bits_of_prepare(W, nx, T, sparse, hostile, c_oracle):
    gt, d0, sp, ref, _, _, _ = device_case(c_oracle, W, T, sparse, hostile)
    with torch.no_grad():
        w8p, Sp, _ = F.cspn3_prepare(gt, want_s=True)
        d_T, hist, w8, S = F.forward_resident(gt, d0, sp, T, int(sparse), keep_history=True, guard=0)
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert same_bits(w8, w8p, which="w8") and same_bits(S, Sp, which="S")
    assert same_bits(d_T, ref, T=T, sparse=sparse, which="training forward")


@pytest.mark.gpu
@pytest.mark.parametrize("hostile", [False, True], ids=["finite", "hostile"])
def test_derive_under_poisoned_lds(hostile, c_oracle):
    W, nx, T, sparse = 96, 3, 17, True
    gt, d0, sp, ref, _, _, _ = device_case(c_oracle, W, T, sparse, hostile)
    with torch.no_grad(), lds_poison():
        o768 = F.forward_resident(gt, d0, sp, T, 1, _plan=plan768(nx), guard=0)
        o512 = F.forward_resident(gt, d0, sp, T, 1, threads=512, guard=0)
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert same_bits(o768, ref, T=T, sparse=sparse, which="768 under poisoned LDS")
    assert same_bits(o512, ref, T=T, sparse=sparse, which="512 under poisoned LDS")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in golden_names("g1_") + golden_names("g2_") if load_golden(n)["guidance"].shape[-1] % 4 == 0])
def test_reference_goldens_through_both_workgroup_sizes(name):
    """What the reference recorded (degenerate sizes, NaN-spreading zero gates, negative sparse depth), through the 512-thread
    instances and, where the shape has a clipped plan, the 768-thread ones."""
    z = load_golden(name)
    g, d, s, T = z["guidance"], z["blur"], z.get("sparse"), int(z["T"])
    gt, d0, sp = dev(g), dev(d)[:, 0].contiguous(), None if s is None else dev(s)[:, 0].contiguous()
    Bg, _, Hg, Wg = g.shape
    sizes = [512] + ([768] if F.resident_plan(Bg, Hg, Wg, T, int(s is not None), 0, threads=768) is not None else [])
    for threads in sizes:
        with torch.no_grad():
            out = F.forward_resident(gt, d0, sp, T, int(s is not None), threads=threads, guard=0)
        torch.cuda.synchronize()
        F.check_resident_errors()
        assert rel_err(out.cpu().numpy(), z["out"][:, 0]) <= 1e-5, (name, threads)

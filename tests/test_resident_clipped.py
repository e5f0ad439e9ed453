"""The clipped 768-thread plans of the weight-resident forward (csrc/cspn_resident.hip: clipped_geometry, the <3, 768, ...> instances of
cspn3_resident): regions as large as (tile +- halo) cut to the image, uneven tile rows, three quads per thread, three wavefronts per
SIMD.  The host part is checked without a device; on the GPU the instance must give the bits of the multi-launch schedule and of the
512-thread resident plan.  Explicit plans on small images, as tests/test_hip_resident.py drives them: 2 x 3 and 3 x 3 tiles of about
32 x 20 pixels are the smallest tilings with edge-only columns, an inner column and all three kinds of tile row.

Reference: network/libs/post_process/CSPN_new.py:26-92."""
import numpy as np
import pytest
import torch

import cspn_monodepth_amd as pkg
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import functional as F
from conftest import bits_equal, lds_poison

DEV = "cuda:0"


def round_up4(v):
    return (v + 3) & ~3


# ------------------------------------------------------------------------------------------------ host (no device)
@pytest.mark.parametrize("blend", [0, 1])
def test_config2_plan_is_one_launch_of_768_threads(blend):
    p = F.resident_plan(24, 228, 304, 24, blend, 256, threads=768)
    assert p is not None
    assert (p["steps_per_phase"], p["tiles_x"], p["tiles_y"], p["tile_w"], p["quads_per_thread"], p["threads"], p["images_per_launch"],
            p["launches"]) == (8, 2, 5, 152, 3, 768, 24, 1)
    assert p["tile_h"] == 50                                  # the first row; then 43 / 43 / 43 and 49 for the last
    assert 0 < p["lds_bytes"] <= 160 * 1024
    assert abs(p["region_over_tile"] - 160 * 57 * 10 / (228.0 * 304.0)) < 1e-5
    d = F.resident_plan(24, 228, 304, 24, blend, 256, threads=0)
    assert (d["steps_per_phase"], d["tiles_x"], d["tiles_y"], d["tile_w"], d["tile_h"], d["quads_per_thread"], d["images_per_launch"],
            d["launches"], d["threads"]) == (8, 2, 5, 152, 46, 5, 24, 1, 512)
    assert d == F.resident_plan(24, 228, 304, 24, blend, 256, threads=512)


def clipped_regions(p, H, W, T):
    """Tiles and regions of a threads = 768 plan, from the rule include/cspn_hip.h documents (tile_h = the first row) and the
    kernel's origin rule: [(x0, x1, rx0, rx1)] per tile column, [(y0, y1, ry0, ry1)] per tile row, wq, wr."""
    S = min(p["steps_per_phase"], T)
    hyw, hxw, exch = S - 1, round_up4(S - 1), T > S
    nx, ny, tw, th0 = p["tiles_x"], p["tiles_y"], p["tile_w"], p["tile_h"]
    xs = [(tx * tw, min(W, (tx + 1) * tw)) for tx in range(nx)]
    if ny == 1:
        ys = [(0, H)]
    else:
        th = th0 - hyw
        org = [0] + [th0 + k * th for k in range(ny - 1)]
        ys = [(org[k], org[k + 1] if k + 1 < ny else H) for k in range(ny)]
    wq4 = max(min(W, x1 + hxw) - max(0, x0 - hxw) for x0, x1 in xs)
    wr = max(min(H, y1 + hyw) - max(0, y0 - hyw) for y0, y1 in ys)
    cols, rows = [], []
    for k, (x0, x1) in enumerate(xs):
        lo = max(0, xs[k - 1][0]) if (exch and k > 0) else 0
        r = max(lo, min(x0 - hxw, W - wq4))
        cols.append((x0, x1, r, r + wq4))
    for k, (y0, y1) in enumerate(ys):
        lo = ys[k - 1][0] if (exch and k > 0) else 0
        r = max(lo, min(y0 - hyw, H - wr))
        rows.append((y0, y1, r, r + wr))
    return cols, rows, wq4 // 4, wr, hxw, hyw


def test_clipped_regions_cover_the_halo_inside_the_image_from_adjacent_tiles():
    seen = 0
    for S in (4, 6, 8, 12):
        for H in list(range(24, 240, 11)) + [228, 352]:
            for W in list(range(16, 330, 28)) + [304, 1216]:
                for B, T in ((1, 24), (6, 24), (24, 24), (3, 17), (2, S - 1)):
                    p = F.resident_plan(B, H, W, T, 0, 256, steps_per_phase=S, threads=768)
                    if p is None:
                        continue
                    seen += 1
                    assert p["threads"] == 768 and p["quads_per_thread"] == 3
                    assert p["tiles_x"] * p["tiles_y"] * p["images_per_launch"] <= 256 and p["lds_bytes"] <= 160 * 1024
                    cols, rows, wq, wr, hxw, hyw = clipped_regions(p, H, W, T)
                    ctx = (B, H, W, T, S, p)
                    assert -(-wr // 3) * wq <= 768, ctx
                    assert abs(p["region_over_tile"] - 4.0 * wq * wr * len(cols) * len(rows) / (H * W)) < 1e-4 * p["region_over_tile"], ctx
                    for axis, n, halo in ((cols, W, hxw), (rows, H, hyw)):
                        assert axis[0][0] == 0 and axis[-1][1] == n and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(axis, axis[1:])), ctx
                        for k, (t0, t1, r0, r1) in enumerate(axis):
                            assert r0 >= 0 and r1 <= n, ctx                                             # inside the image
                            assert r0 <= max(0, t0 - halo) and r1 >= min(n, t1 + halo), ctx             # covers tile +- halo
                            if T > min(S, T):            # a launch that exchanges borders waits for the adjacent tiles only
                                assert r0 >= (axis[k - 1][0] if k > 0 else 0), ctx
                                assert r1 <= (axis[k + 1][1] if k + 1 < len(axis) else n), ctx
    assert seen > 200


def test_inner_tiles_keep_two_sided_halos():
    """Three or more tile columns: the inner columns need both halos, the region is as wide as in the 512-thread plans."""
    p = F.resident_plan(2, 60, 96, 24, 0, 256, steps_per_phase=8, threads=768)
    assert p is not None
    cols, rows, wq, wr, hxw, hyw = clipped_regions(p, 60, 96, 24)
    if p["tiles_x"] >= 3:
        assert 4 * wq == p["tile_w"] + 2 * hxw
    if p["tiles_y"] >= 3:
        assert wr == (rows[1][1] - rows[1][0]) + 2 * hyw


# ------------------------------------------------------------------------------------------------ GPU
def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def plan768(B, tiles_x, tiles_y, tile_w, tile_h, S=8, spin=0):
    rp = _lib.cspn_resident_plan()
    rp.steps_per_phase, rp.tiles_x, rp.tiles_y, rp.tile_w, rp.tile_h = S, tiles_x, tiles_y, tile_w, tile_h
    rp.threads, rp.images_per_launch, rp.spin_limit = 768, B, spin
    return rp


_INPUTS = {}


def inputs(c_oracle, B, H, W, T, sparse):
    """Device inputs and the multi-launch result of a case: computed once, shared, never written."""
    key = (B, H, W, T, sparse)
    if key not in _INPUTS:
        g, d, s = c_oracle.synthetic_inputs(400 + H + W + T, B, H, W, 12, max(2, H * W // 60) if sparse else None)
        gt, dt, st = dev(g), dev(d), dev(s)
        prev = F._RESIDENT_MODE
        F.set_resident("off")
        try:
            with torch.no_grad():
                ref = pkg.CSPN_new.AffinityPropagate(T, 3)(gt, dt, st)[:, 0].contiguous()
        finally:
            F.set_resident(prev)
        _INPUTS[key] = (gt, dt[:, 0].contiguous(), None if st is None else st[:, 0].contiguous(), ref)
    return _INPUTS[key]


# (H, W, tiles_x, tiles_y, tile_w, first row, T): rows follow from the first one (S = 8: halo 7): 23 -> 23 / 16 / 21, region 30 rows;
# 24 -> 24 / 17 / 19, region 31 rows (31 % 3 != 0: the last strip of a thread column is partly past the region); 26 -> 26 / 19 / 15
# (the last row shorter than the inner one).  T = 24: three phases, both exchange planes used twice; T = 17: a last phase of one step;
# T = 7: a single phase without any exchange (halo 6: 24 / 18 / 18, region 30).
CASES = [(60, 64, 2, 3, 32, 23, 24), (60, 64, 2, 3, 32, 24, 24), (60, 64, 2, 3, 32, 26, 24), (60, 96, 3, 3, 32, 24, 24),
         (60, 96, 3, 3, 32, 23, 17), (60, 64, 2, 3, 32, 24, 17), (60, 64, 2, 3, 32, 24, 7), (60, 96, 3, 3, 32, 24, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,nx,ny,tw,th0,T", CASES, ids=["%dx%d-%dx%d-h%d-T%d" % (c[0], c[1], c[2], c[3], c[5], c[6]) for c in CASES])
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
def test_clipped_plan_equals_multi_launch_and_512_bit_for_bit(H, W, nx, ny, tw, th0, T, sparse, c_oracle):
    B = 2
    gt, d0, sp, ref = inputs(c_oracle, B, H, W, T, sparse)
    with torch.no_grad():
        out = F.forward_resident(gt, d0, sp, T, int(sparse), _plan=plan768(B, nx, ny, tw, th0), guard=0)
        r512 = F.forward_resident(gt, d0, sp, T, int(sparse), threads=512, guard=0)
        with lds_poison():
            outp = F.forward_resident(gt, d0, sp, T, int(sparse), _plan=plan768(B, nx, ny, tw, th0), guard=0)
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert bits_equal(out, ref, T=T, sparse=sparse, which="768 vs multi-launch")
    assert bits_equal(out, r512, T=T, sparse=sparse, which="768 vs 512")
    assert bits_equal(outp, ref, T=T, sparse=sparse, which="768 under poisoned LDS")


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
def test_searched_clipped_plan_and_scored_sums(sparse, c_oracle):
    """The plan the engine's own search finds (threads = 768 without tile fields), plain and scored: the refined depth is the
    multi-launch bits, the fused sums are those of the metric kernel on it (other order of the atomic additions: rtol 2e-5)."""
    ev = pkg.evaluation
    B, H, W, T = 2, 60, 96, 24
    gt, d0, sp, ref = inputs(c_oracle, B, H, W, T, sparse)
    tgt = np.maximum(d0.cpu().numpy() + 0.1 * c_oracle.hash_normal(92, 9, (B, H, W)), 0.0).astype(np.float32)
    tgt[c_oracle.hash_uniform(93, 9, (B, H, W)) < 0.05] = 0.0
    tt = dev(tgt)
    p = F.resident_plan(B, H, W, T, int(sparse), 0, threads=768)
    assert p is not None and p["threads"] == 768 and p["launches"] == 1
    with torch.no_grad():
        out = F.forward_resident(gt, d0, sp, T, int(sparse), threads=768, guard=0)
        acc = ev.new_accumulator(DEV)
        outs = F.forward_resident(gt, d0, sp, T, int(sparse), score=(tt, acc), _plan=plan768(B, 3, 3, 32, 24), guard=0)
        want = ev.new_accumulator(DEV)
        ev.metric_sums(ref, tt, out=want)
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert bits_equal(out, ref, T=T, sparse=sparse) and bits_equal(outs, ref, T=T, sparse=sparse)
    got, exp = acc.sum(0).cpu().numpy(), want.sum(0).cpu().numpy()
    print("scored sums", got, exp)
    assert np.allclose(got, exp, rtol=2e-5)


@pytest.mark.gpu
def test_padded_rows_fall_back_to_the_512_thread_instance(c_oracle):
    """W_valid < W is the 512-thread instances' business: a call that brings a clipped plan runs their plan instead."""
    B, H, W, T = 2, 60, 64, 24
    gt, d0, sp, _ = inputs(c_oracle, B, H, W, T, True)
    with torch.no_grad():
        ref, _ = F.propagate_from_guidance(gt, d0, sp, T, 1, valid_w=W - 3)
        out = F.forward_resident(gt, d0, sp, T, 1, valid_w=W - 3, _plan=plan768(B, 2, 3, 32, 24), guard=0)
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert bits_equal(out[..., :W - 3], ref[..., :W - 3], T=T, sparse=True)


@pytest.mark.gpu
def test_clipped_plan_give_up_path_is_repaired(c_oracle):
    """spin_limit = 1: the first neighbour wait gives up at once, the launch ends normally with its tiles NaN-filled, and the next
    call repairs the result into the same tensor (tests/test_hip_resident.py: test_resident_timeout_is_repaired_not_a_hang)."""
    B, H, W, T = 2, 60, 96, 24
    gt, d0, _, ref = inputs(c_oracle, B, H, W, T, False)
    F.ensure_resident_ok()
    with torch.no_grad():
        broken = F.forward_resident(gt, d0, None, T, 0, _plan=plan768(B, 3, 3, 32, 24, spin=1), guard=0)
        torch.cuda.synchronize()
        if F.resident_fallbacks() == 0:
            assert bool(torch.isnan(broken).any()) and F._holds_poison(broken)
        clean = F.forward_resident(gt, d0, None, T, 0, _plan=plan768(B, 3, 3, 32, 24), guard=0)
        torch.cuda.synchronize()
    assert F.resident_fallbacks() == 1
    assert bits_equal(broken, ref, T=T) and bits_equal(clean, ref, T=T) and bits_equal(broken, clean)
    F.ensure_resident_ok()

"""The NYU train / val transforms on raw batches (cspn_monodepth_amd/dataloaders/nyu_dataloader/nyu_dataloader.py,
include/cspn_transform.h) against golden G22: the reference's transforms.py per frame on the CPU (tests/golden/make_golden_g22.py),
which equals the numpy restatement of tests/transform_cases.py bit for bit.

An output pixel is a copy of a raw pixel, a zero, or integer / singly-rounded arithmetic on one, so EVERY comparison here is bit
equality: no tolerance appears anywhere.  Depth is compared as 32-bit words, a NaN may match any NaN (transform_cases.words).

  * CPU: the restatement against every fixture and digest, the fixture set and its size cap, the header / library / loader contract,
    the host-side argument checks of the C ABI and of the module;
  * GPU: every G22 case through the C ABI (RGB into channels 0..2 of a [B,4,oh,ow] buffer) and through the module; what a frame's
    place in the batch may not change; drawn parameters against the numpy Philox; a captured chain transform -> create_rgbd ->
    AffinityPropagate; parameters outside the precondition."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import cspn_monodepth_amd as pkg
import transform_cases as tc
from conftest import ROOT, golden_names, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd.dataloaders.nyu_dataloader import dense_to_sparse as d2s
from cspn_monodepth_amd.dataloaders.nyu_dataloader import nyu_dataloader as nyu

DEV = "cuda:0"
STORED = [n for n in tc.CASES if n not in tc.DIGEST_ONLY]
NAMES = list(tc.CASES)


@functools.lru_cache(maxsize=None)
def golden(name):
    return load_golden("g22_transform_" + name)      # shared among the tests: nobody writes into it


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(ROOT, "tests", "golden", "golden_g22_manifest.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def inputs(name):
    return tc.make_inputs(tc.CASES[name])


def equals_reference(name, rgb, depth):
    """the reference's output of the case: the stored arrays, or their digest for the full-size cases"""
    if name in tc.DIGEST_ONLY:
        return rgb.dtype == depth.dtype == np.float32 and tc.digest(rgb, depth) == manifest()["digests"][name]
    z = golden(name)
    return tc.same(rgb, z["rgb"]) and tc.same(depth, z["depth"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ CPU
def test_fixture_set_is_complete_and_small():
    assert golden_names("g22_transform_") == sorted("g22_transform_" + n for n in STORED)
    for name in STORED:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g22_transform_%s.npz" % name)) <= tc.MAX_FILE_BYTES == 89617
    assert sorted(manifest()["digests"]) == sorted(tc.DIGEST_ONLY) and sorted(manifest()["cases"]) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    """This alone pins the specification without a GPU: running sums, separate roundings, the validity range, the contrast mean."""
    case = tc.CASES[name]
    rgb, depth = tc.restate_case(case)
    assert rgb.shape == (tc.n_frames(case), 3) + tuple(case["out"]) and depth.shape == (tc.n_frames(case), 1) + tuple(case["out"])
    assert equals_reference(name, rgb, depth)
    if name in STORED and case["mode"] == "train":
        assert np.array_equal(golden(name)["params"], tc.params_of(case))     # the stored rows are the case's


def test_fixtures_hold_what_they_are_there_for():
    m = manifest()["cases"]
    # (a) rotated coordinates keep their distance from ties and borders, (b) running sum != closed form in rows and columns,
    # (c) zero-filled corners
    assert all(c["tie_distance"] >= 1e-9 for c in m.values() if "tie_distance" in c)
    assert any(c["table_differs_rows_cols"][0] > 0 for c in m.values()) and any(c["table_differs_rows_cols"][1] > 0 for c in m.values())
    assert m["orders_48x64"]["table_differs_rows_cols"][1] > 0
    assert all(z > 0 for z in m["rot5_48x64"]["zero_filled_pixels"])
    assert not np.array_equal(tc.resize_table(64, 33), tc.closed_form_table(64, 33))
    assert int((tc.resize_table(640, 333) != tc.closed_form_table(640, 333)).sum()) == 1
    assert int((tc.resize_table(480, 250) != tc.closed_form_table(480, 250)).sum()) == 4
    assert tc.resize_table(8, 6)[4] != tc.closed_form_table(8, 6)[4]
    assert sorted(int(p[tc.P_ORDER]) for p in tc.params_of(tc.CASES["orders_48x64"])) == list(range(6))
    z = golden("rot5_48x64")
    case = tc.CASES["rot5_48x64"]
    for b, p in enumerate(tc.params_of(case)):                                                  # the corners the rotation left empty
        empty = ~tc.source_map(p, case["raw"], case["first"], case["out"])[0]
        assert empty.sum() > 0 and (empty[0] | empty[-1]).any() and (z["depth"][b, 0][empty] == 0).all()
        assert p[tc.P_ORDER] >= 0 or (z["rgb"][b][:, empty] == 0).all()                          # (the jitter moves a zero-filled pixel too)
    d = golden("val_48x64")["depth"]
    assert np.isnan(d).any() and np.isinf(d).any() and (np.signbit(d) & (d == 0)).any()
    d = golden("identity_48x64")["depth"]
    assert np.isnan(d).any() and np.isinf(d).any() and (d == 0).any() and not (np.signbit(d) & (d == 0)).any()
    assert (golden("factors_48x64")["rgb"][2] == 1.0).any()                                      # clipped at 255
    # the half-way mean: 100.5 -> 101, where truncation or rounding to even would give 100
    case = tc.CASES["half_mean_8x12"]
    rgb_in, _ = inputs("half_mean_8x12")
    valid, r0, c0 = tc.source_map(tc.params_of(case)[0], case["raw"], case["first"], case["out"])
    assert tc.contrast_constant(rgb_in[0][:, r0, c0].astype(np.int64)) == 101
    assert 2 * int(tc.luma(rgb_in[0][:, r0, c0].astype(np.int64)).sum()) == 201 * valid.size


def test_header_declares_five_symbols_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "cspn_transform.h")).read()
    assert re.search(r"CSPN_TRANSFORM_VAL = 0, CSPN_TRANSFORM_TRAIN = 1", src)
    assert re.search(r"^#define CSPN_TRANSFORM_GATHER_PIXELS 256\b", src, flags=re.M) and re.search(r"^#define CSPN_TRANSFORM_PARAMS 8\b", src, flags=re.M)
    assert (_lib.TRANSFORM_VAL, _lib.TRANSFORM_TRAIN) == (0, 1)
    assert (_lib.TRANSFORM_PARAMS, _lib.TRANSFORM_GATHER_PIXELS) == (8, tc.GATHER_THREADS) == (8, 256)


def test_sizes_and_workspace_bytes_need_no_device():
    L = _lib.lib()
    h1, w1 = ctypes.c_int(), ctypes.c_int()
    for (H, W, first) in ((480, 640, 250.0 / 480), (480, 640, 240.0 / 480), (48, 64, 25.0 / 48), (120, 160, 63.0 / 120), (8, 12, 0.75)):
        assert L.cspn_transform_first_size(H, W, first, ctypes.byref(h1), ctypes.byref(w1)) == 1
        assert (h1.value, w1.value) == (tc.out_len(H, first), tc.out_len(W, first))
    assert L.cspn_transform_first_size(480, 640, 250.0 / 480, ctypes.byref(h1), ctypes.byref(w1)) == 1 and (h1.value, w1.value) == (250, 333)
    assert L.cspn_transform_first_size(8, 12, 0.01, None, None) == 0 and L.cspn_transform_first_size(0, 12, 0.5, None, None) == 0
    assert L.cspn_transform_first_size(8, 12, float("nan"), None, None) == 0
    VAL, TRAIN = _lib.TRANSFORM_VAL, _lib.TRANSFORM_TRAIN
    assert L.cspn_transform_workspace_bytes(VAL, 2, 48, 64, 0.5, 22, 30) == 24 * 4 + 32 * 4
    assert L.cspn_transform_workspace_bytes(VAL, 2, 48, 64, 0.5, 25, 30) == 0            # larger than the resized frame
    assert L.cspn_transform_workspace_bytes(2, 2, 48, 64, 0.5, 22, 30) == 0 and L.cspn_transform_workspace_bytes(TRAIN, 0, 48, 64, 0.5, 22, 30) == 0
    n, G = 22 * 30, 3
    up8 = lambda v: (v + 7) // 8 * 8                                                     # noqa: E731
    assert L.cspn_transform_workspace_bytes(TRAIN, 3, 48, 64, 25.0 / 48, 22, 30) == \
        3 * 72 + up8(25 * 4) + up8(33 * 4) + up8(3 * 22 * 4) + up8(3 * 30 * 4) + up8(3 * G * 4) + up8(3 * n * 4)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Validation happens on the host before any launch: 0 and a message in cspn_last_error()."""
    L = _lib.lib()
    err = lambda: L.cspn_last_error().decode()                                     # noqa: E731
    p, odd, odd4 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)   # never dereferenced: validation fails first
    TRAIN, VAL = _lib.TRANSFORM_TRAIN, _lib.TRANSFORM_VAL

    def call(rgb=p, depth=p, B=2, H=48, W=64, first=25.0 / 48, oh=22, ow=30, mode=TRAIN, params=p, rout=p, rbs=3 * 660, rcs=660, dout=p, dbs=660,
             work=p):
        return L.cspn_transform(rgb, depth, B, H, W, first, oh, ow, mode, params, rout, rbs, rcs, dout, dbs, work, None)

    assert call(rgb=None) == 0 and "null rgb" in err()
    assert call(depth=None) == 0 and "null rgb" in err()
    assert call(mode=2) == 0 and "unknown mode" in err()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(W=-1), dict(oh=0), dict(ow=0)):
        assert call(**bad) == 0 and "bad size" in err()
    assert call(H=1 << 16, W=1 << 15) == 0 and "2^31" in err()
    assert call(first=0.0) == 0 and "first factor" in err()
    assert call(first=0.001) == 0 and "first factor" in err()
    assert call(mode=VAL, params=None, oh=26) == 0 and "larger than the resized frame" in err()
    assert call(params=None) == 0 and "needs params" in err()
    assert call(params=odd4) == 0 and "8-byte aligned" in err()
    assert call(depth=odd) == 0 and "element size" in err()
    assert call(rout=None) == 0 and "null rgb_out" in err()
    assert call(dout=odd) == 0 and "element size" in err()
    assert call(rcs=659) == 0 and "rgb_out_channel_stride" in err()
    assert call(rbs=659) == 0 and "rgb_out_batch_stride" in err()
    assert call(dbs=-660) == 0 and "depth_out_batch_stride" in err()
    assert call(work=None) == 0 and "null work" in err()
    assert call(work=odd4) == 0 and "8-byte aligned" in err()
    draw = L.cspn_transform_draw_params
    assert draw(None, 2, 0, p, None) == 0 and "null frame_ids" in err()
    assert draw(p, 0, 0, p, None) == 0 and "bad size" in err()
    assert draw(odd4, 2, 0, p, None) == 0 and "8-byte aligned" in err()


def test_module_checks_its_arguments_and_has_no_cpu_path():
    rgb, depth = torch.zeros(2, 3, 8, 12, dtype=torch.uint8), torch.rand(2, 1, 8, 12)
    kw = dict(first=0.75, output_size=(4, 6))
    params = torch.zeros(2, 8, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nyu.val_transform(rgb, depth, **kw)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nyu.train_transform(rgb, depth, params=params, **kw)
    with pytest.raises(RuntimeError, match="ROCm device"):
        nyu.draw_train_params(2, frame_ids=torch.arange(2))
    with pytest.raises(RuntimeError, match="ROCm device"):
        nyu.draw_train_params(2, device="cpu")
    for bad in (rgb.float(), rgb.numpy(), rgb.to(torch.int8)):
        with pytest.raises(TypeError, match="rgb"):
            nyu.val_transform(bad, depth, **kw)
    for bad in (depth.half(), depth.double(), depth.numpy()):
        with pytest.raises(TypeError, match="depth"):
            nyu.train_transform(rgb, bad, params=params, **kw)
    for bad in (rgb[0], rgb[:, :2], torch.zeros(0, 3, 8, 12, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="rgb"):
            nyu.val_transform(bad, depth, **kw)
    for bad in (depth[0], depth[:, :, :7], torch.rand(2, 3, 8, 12)):
        with pytest.raises(ValueError, match="depth"):
            nyu.val_transform(rgb, bad, **kw)
    with pytest.raises(TypeError, match="params"):
        nyu.train_transform(rgb, depth, params=params.float(), **kw)
    with pytest.raises(TypeError, match="params"):
        nyu.train_transform(rgb, depth, params=[[1.0] * 8] * 2, **kw)
    with pytest.raises(ValueError, match="params"):
        nyu.train_transform(rgb, depth, params=params[:1], **kw)
    with pytest.raises(TypeError, match="not both"):
        nyu.train_transform(rgb, depth, params=params, frame_ids=torch.arange(2), **kw)
    with pytest.raises(TypeError, match="frame_ids"):
        nyu.train_transform(rgb, depth, frame_ids=[0, 1], **kw)
    with pytest.raises(TypeError, match="frame_ids"):
        nyu.train_transform(rgb, depth, frame_ids=torch.arange(2, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="frame_ids"):
        nyu.train_transform(rgb, depth, frame_ids=torch.arange(3), **kw)
    with pytest.raises(TypeError, match="seed"):
        nyu.train_transform(rgb, depth, seed=1.5, **kw)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            nyu.train_transform(rgb, depth, seed=bad, **kw)
        with pytest.raises(ValueError, match="seed"):
            nyu.draw_train_params(2, seed=bad)
    with pytest.raises(TypeError, match="B must"):
        nyu.draw_train_params(2.0)
    with pytest.raises(ValueError, match="B must"):
        nyu.draw_train_params(0)
    with pytest.raises(TypeError, match="first"):
        nyu.val_transform(rgb, depth, first="half", output_size=(4, 6))
    with pytest.raises(ValueError, match="first"):
        nyu.val_transform(rgb, depth, first=0.0, output_size=(4, 6))
    with pytest.raises(TypeError, match="output_size"):
        nyu.val_transform(rgb, depth, first=0.75, output_size=(4.0, 6))
    with pytest.raises(ValueError, match="output_size"):
        nyu.val_transform(rgb, depth, first=0.75, output_size=(0, 6))
    with pytest.raises(ValueError, match="larger than the resized frame"):
        nyu.val_transform(rgb, depth, first=0.75, output_size=(7, 6))
    good = (torch.empty(2, 3, 4, 6), torch.empty(2, 1, 4, 6))
    with pytest.raises(TypeError, match="out"):
        nyu.val_transform(rgb, depth, out=good[0], **kw)
    with pytest.raises(TypeError, match=r"out\[1\]"):
        nyu.val_transform(rgb, depth, out=(good[0], good[1].double()), **kw)
    with pytest.raises(ValueError, match=r"out\[0\]"):
        nyu.val_transform(rgb, depth, out=(torch.empty(2, 3, 4, 7), good[1]), **kw)
    with pytest.raises(ValueError, match=r"out\[0\].*contiguous"):
        nyu.val_transform(rgb, depth, out=(torch.empty(2, 3, 4, 12)[..., ::2], good[1]), **kw)
    with pytest.raises(ValueError, match=r"out\[1\].*contiguous"):
        nyu.val_transform(rgb, depth, out=(good[0], torch.empty(2, 1, 6, 4).transpose(2, 3)), **kw)
    import inspect
    assert list(inspect.signature(nyu.val_transform).parameters) == ["rgb", "depth", "out", "first", "output_size"]
    assert list(inspect.signature(nyu.train_transform).parameters) == ["rgb", "depth", "params", "frame_ids", "seed", "out", "first", "output_size"]
    assert list(inspect.signature(nyu.draw_train_params).parameters) == ["B", "frame_ids", "seed", "device"]
    assert (nyu.iheight, nyu.iwidth, nyu.OUTPUT_SIZE, nyu.TRAIN_FIRST, nyu.VAL_FIRST) == (480, 640, (228, 304), 250.0 / 480, 240.0 / 480)
    assert pkg.dataloaders.nyu_dataloader.nyu_dataloader is nyu and pkg.dataloaders.nyu_dataloader.train_transform is nyu.train_transform
    assert pkg.dataloaders.nyu_dataloader.val_transform is nyu.val_transform and pkg.dataloaders.nyu_dataloader.draw_train_params is nyu.draw_train_params


def test_numpy_draw_stays_inside_the_reference_ranges():
    p = tc.restate_draw(range(500), 12345)
    assert p.shape == (500, 8) and (p[:, tc.P_S] >= 1).all() and (p[:, tc.P_S] < 1.5).all() and (np.abs(p[:, tc.P_ANGLE]) <= 5).all()
    assert set(np.unique(p[:, tc.P_FLIP])) == {0.0, 1.0} and set(np.unique(p[:, tc.P_ORDER])) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    f = p[:, tc.P_BRIGHTNESS:tc.P_SATURATION + 1]
    assert (f >= 0.6).all() and (f < 1.4).all() and (p[:, tc.P_RESERVED] == 0).all()
    assert 0.4 < p[:, tc.P_FLIP].mean() < 0.6 and abs(p[:, tc.P_S].mean() - 1.25) < 0.03
    # the smallest s keeps the reference's geometry inside the precondition: int(250 * 1.0) >= 228, int(333 * 1.0) >= 304


# ------------------------------------------------------------------------------------------------ GPU
GUARD = 8


def abi_run(name, params=None):
    """One cspn_transform call on caller-owned buffers: RGB into channels 0..2 of a NaN-filled [B,4,oh,ow] buffer, depth into a
    NaN-guarded plane.  -> rgb, depth as numpy (params: other rows than the case's)."""
    L = _lib.lib()
    case = tc.CASES[name]
    rgb_in, depth_in = inputs(name)
    B, (H, W), (oh, ow) = rgb_in.shape[0], case["raw"], case["out"]
    n = oh * ow
    train = case["mode"] == "train"
    mode = _lib.TRANSFORM_TRAIN if train else _lib.TRANSFORM_VAL
    if params is None:
        params = tc.params_of(case)
    rgb, depth = dev(rgb_in), dev(depth_in)
    p = dev(params) if train else None
    rgbd = torch.full((B, 4, oh, ow), float("nan"), dtype=torch.float32, device=DEV)
    dbuf = torch.full((GUARD + B * n + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    nbytes = L.cspn_transform_workspace_bytes(mode, B, H, W, case["first"], oh, ow)
    assert nbytes > 0
    work = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    _lib.check(L.cspn_transform(rgb.data_ptr(), depth.data_ptr(), B, H, W, case["first"], oh, ow, mode, None if p is None else p.data_ptr(),
                                rgbd.data_ptr(), 4 * n, n, dbuf[GUARD:].data_ptr(), n, work.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "cspn_transform")
    torch.cuda.synchronize()
    assert bool(torch.isnan(rgbd[:, 3]).all()) and not bool(torch.isnan(rgbd[:, :3]).any())      # channel 3 untouched, 0..2 written
    assert bool(torch.isnan(dbuf[:GUARD]).all()) and bool(torch.isnan(dbuf[GUARD + B * n:]).all())
    return host(rgbd[:, :3].contiguous()), host(dbuf[GUARD:GUARD + B * n]).reshape(B, 1, oh, ow)


def module_run(name, rgb_in=None, depth_in=None, params=None, out=None):
    case = tc.CASES[name]
    if rgb_in is None:
        rgb_in, depth_in = inputs(name)
    kw = dict(first=case["first"], output_size=case["out"], out=out)
    if case["mode"] == "val":
        rgb, depth = nyu.val_transform(dev(rgb_in), dev(depth_in), **kw)
    else:
        rgb, depth = nyu.train_transform(dev(rgb_in), dev(depth_in), params=dev(tc.params_of(case) if params is None else params), **kw)
    B = rgb_in.shape[0]
    assert rgb.shape == (B, 3) + tuple(case["out"]) and depth.shape == (B, 1) + tuple(case["out"])
    assert rgb.dtype == depth.dtype == torch.float32
    return host(rgb), host(depth)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_through_the_c_abi_is_bit_equal_to_the_reference(name):
    rgb, depth = abi_run(name)
    assert equals_reference(name, rgb, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_through_the_module_is_bit_equal_to_the_reference(name):
    rgb, depth = module_run(name)
    assert equals_reference(name, rgb, depth)
    assert np.isfinite(rgb).all() and rgb.min() >= 0 and rgb.max() <= 1


@pytest.mark.gpu
def test_defaults_are_the_reference_geometry():
    for name in tc.DIGEST_ONLY:
        case = tc.CASES[name]
        rgb_in, depth_in = inputs(name)
        if case["mode"] == "val":
            rgb, depth = nyu.val_transform(dev(rgb_in), dev(depth_in))
        else:
            rgb, depth = nyu.train_transform(dev(rgb_in), dev(depth_in), params=dev(tc.params_of(case)))
        assert equals_reference(name, host(rgb), host(depth))


@pytest.mark.gpu
def test_rgb_lands_in_a_strided_view_and_leaves_channel_3_alone():
    name = "orders_48x64"
    B, (oh, ow) = 6, tc.CASES[name]["out"]
    rgbd = torch.full((B, 4, oh, ow), -7.0, dtype=torch.float32, device=DEV)
    depth_out = torch.empty((B, 1, oh, ow), dtype=torch.float32, device=DEV)
    rgb, depth = module_run(name, out=(rgbd[:, :3], depth_out))
    assert equals_reference(name, rgb, depth) and bool((rgbd[:, 3] == -7.0).all())
    assert equals_reference(name, host(rgbd[:, :3].contiguous()), host(depth_out))
    # depth straight into channel 3 of the same buffer
    rgb, depth = module_run(name, out=(rgbd[:, :3], rgbd[:, 3:4]))
    assert equals_reference(name, host(rgbd[:, :3].contiguous()), host(rgbd[:, 3:4].contiguous()))


@pytest.mark.gpu
def test_a_frame_keeps_its_bits_wherever_it_sits_and_run_after_run():
    """Frame 1 of the case alone (B = 1) and at every position of a batch of 3, twice each."""
    name = "mid_120x160"
    case = tc.CASES[name]
    rgb_in, depth_in = inputs(name)
    params = tc.params_of(case)
    want_rgb, want_depth = golden(name)["rgb"][1:2], golden(name)["depth"][1:2]
    alone = module_run(name, rgb_in[1:2], depth_in[1:2], params[1:2])
    assert tc.same(alone[0], want_rgb) and tc.same(alone[1], want_depth)
    for pos in range(3):
        idx = [0, 0, 0]
        idx[pos] = 1
        for _ in range(2):
            rgb, depth = module_run(name, rgb_in[idx], depth_in[idx], params[idx])
            assert tc.same(rgb[pos:pos + 1], want_rgb) and tc.same(depth[pos:pos + 1], want_depth)
            assert all(tc.same(rgb[q:q + 1], golden(name)["rgb"][0:1]) for q in range(3) if q != pos)


@pytest.mark.gpu
def test_drawn_parameters_equal_the_numpy_philox():
    ids, seed = [0, 5, (1 << 33) + 1, (1 << 63) - 1, 41], 0xfedcba9876543210
    tid = torch.tensor(ids, dtype=torch.int64, device=DEV)
    got = host(nyu.draw_train_params(5, frame_ids=tid, seed=seed))
    want = tc.restate_draw(ids, seed)
    assert got.dtype == np.float64 and got.shape == (5, 8) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (got[:, 0] >= 1).all() and (got[:, 0] < 1.5).all() and (np.abs(got[:, 1]) <= 5).all() and np.isin(got[:, 2], (0, 1)).all()
    assert (got[:, 3:6] >= 0.6).all() and (got[:, 3:6] < 1.4).all() and np.isin(got[:, 6], range(6)).all() and (got[:, 7] == 0).all()
    # (seed, frame id) only: the row of id 41 alone, and under the default ids 0 .. B-1 and the default seed
    alone = host(nyu.draw_train_params(1, frame_ids=tid[4:5], seed=seed))
    assert np.array_equal(alone[0].view(np.uint64), got[4].view(np.uint64))
    assert np.array_equal(host(nyu.draw_train_params(3)).view(np.uint64), tc.restate_draw(range(3), 0).view(np.uint64))
    other = host(nyu.draw_train_params(1, frame_ids=tid[4:5], seed=seed + 1))
    assert not np.array_equal(other[0, :7], got[4, :7])
    # drawn rows drive the transform: equal to the restatement fed the same rows
    name = "orders_48x64"
    case = tc.CASES[name]
    rgb_in, depth_in = inputs(name)
    ids6 = torch.arange(100, 106, dtype=torch.int64, device=DEV)
    rgb, depth = nyu.train_transform(dev(rgb_in), dev(depth_in), frame_ids=ids6, seed=9, first=case["first"], output_size=case["out"])
    want_rgb, want_depth = tc.restate(rgb_in, depth_in, tc.restate_draw(range(100, 106), 9), case["first"], case["out"])
    assert tc.same(host(rgb), want_rgb) and tc.same(host(depth), want_depth)


@pytest.mark.gpu
def test_call_does_not_synchronise():
    name = "tiny_8x12"
    case = tc.CASES[name]
    rgb_in, depth_in = inputs(name)
    rgb, depth, ids = dev(rgb_in), dev(depth_in), torch.arange(3, dtype=torch.int64, device=DEV)
    kw = dict(first=case["first"], output_size=case["out"])
    nyu.train_transform(rgb, depth, frame_ids=ids, seed=3, **kw)                 # first use: library load, allocator warm-up
    nyu.val_transform(rgb, depth, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = nyu.train_transform(rgb, depth, frame_ids=ids, seed=3, **kw)
        nyu.val_transform(rgb, depth, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = tc.restate(rgb_in, depth_in, tc.restate_draw(range(3), 3), case["first"], case["out"])
    assert tc.same(host(out[0]), want[0]) and tc.same(host(out[1]), want[1])


@pytest.mark.gpu
def test_captured_chain_replays_what_eager_calls_compute():
    """train_transform -> create_rgbd -> CSPN_new.AffinityPropagate and `ids += B`, captured into ONE graph and replayed three times =
    three eager chains with the ids advanced: a fresh augmentation and a fresh sparse sample per replay."""
    from oracle import cspn_oracle as orc
    name = "mid_120x160"
    case = tc.CASES[name]
    rgb_in, depth_in = inputs(name)
    B, (oh, ow), seed, start = 2, case["out"], 77, 1000
    g, d, _ = orc.synthetic_inputs(221, B, oh, ow, 8)
    guidance, blur = dev(g), dev(d)
    rgb, depth = dev(rgb_in), dev(np.abs(depth_in) + 0.5)
    us = d2s.UniformSampling(200)
    m = pkg.CSPN_new.AffinityPropagate(12, 3)
    kw = dict(first=case["first"], output_size=case["out"])

    def chain(ids):
        with torch.no_grad():
            t_rgb, t_depth = nyu.train_transform(rgb, depth, frame_ids=ids, seed=seed, **kw)
            rgbd, sparse = d2s.create_rgbd(us, t_rgb, t_depth, frame_ids=ids, seed=seed)
            return rgbd, m(guidance, blur, sparse)

    ids = torch.arange(start, start + B, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            chain(ids)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_rgbd, static_out = chain(ids)
        ids += B
    assert ids.tolist() == [start, start + 1]                                     # a capture runs nothing
    seen = []
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        these = range(start + k * B, start + (k + 1) * B)
        eager_rgbd, eager_out = chain(torch.tensor(list(these), dtype=torch.int64, device=DEV))
        assert torch.equal(static_rgbd.view(torch.int32), eager_rgbd.view(torch.int32))
        assert torch.equal(static_out.view(torch.int32), eager_out.view(torch.int32))
        want_rgb, want_depth = tc.restate(rgb_in, host(depth), tc.restate_draw(these, seed), case["first"], case["out"])
        assert tc.same(host(eager_rgbd[:, :3].contiguous()), want_rgb)
        assert bool(torch.isfinite(eager_out).all())
        seen.append(host(static_rgbd).copy())
    assert ids.tolist() == [start + 3 * B, start + 3 * B + 1]
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


@pytest.mark.gpu
def test_rows_outside_the_precondition_return_and_leave_the_other_frames_alone():
    """s = 0.5 (the second size is smaller than the crop) and angle = NaN: one run; the call completes, the other frames keep
    their bits.  What the two bad frames hold is not specified."""
    name = "orders_48x64"
    params = tc.params_of(tc.CASES[name]).copy()
    params[1, tc.P_S] = 0.5
    params[4, tc.P_ANGLE] = np.nan
    rgb, depth = module_run(name, params=params)
    z = golden(name)
    for b in (0, 2, 3, 5):
        assert tc.same(rgb[b:b + 1], z["rgb"][b:b + 1]) and tc.same(depth[b:b + 1], z["depth"][b:b + 1])
    assert not np.isnan(rgb).any()

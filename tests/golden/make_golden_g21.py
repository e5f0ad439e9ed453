"""Golden G21: the reference's sparse-depth sampler and RGB-D assembly (dataloaders/nyu_dataloader/dense_to_sparse.py:27-52
UniformSampling, dataloader.py:85-97 create_sparse_depth / create_rgbd), per frame, on the CPU.

The maker loads the reference's own dense_to_sparse.py from CSPN_REFERENCE (default /root/reference — nothing of it is copied) by
file path, with a stub `cv2` in sys.modules: only SimulatedStereo touches cv2, and it is not called.  The package around it is not
imported: dataloaders/nyu_dataloader/__init__.py pulls in dataloader.py and transforms.py, which need h5py, scipy.misc and PIL.  So
the statements of MyDataloader.create_sparse_depth / create_rgbd (dataloader.py:90-91 and :96), of the loader's uint8 conversion
(nyu_dataloader.py:29, whose `np.asfarray` numpy 2 no longer has: `np.asarray(rgb, dtype=float) / 255`) and of ToTensor
(transforms.py:216, :224: transpose to C x H x W, `.float()`) are RESTATED below, each with its line; the sampling itself is the
reference's code.

For every case of tests/sparsify_cases.CASES and every frame of it:
  * u = "seeded": np.random.seed(seed + b), the reference's dense_to_sparse draws from the global generator; the maker re-seeds and
    redraws np.random.uniform(0, 1, shape) to record the plane the reference consumed (a frame with n_keep == 0 draws nothing: its
    recorded plane is what it would have drawn);
  * u = "f32" / "hand": np.random.uniform is replaced for the duration of the reference's call by a function that checks its arguments
    and returns the prepared plane — the seeded draw rounded to fp32, or sparsify_cases.hand_uniform — so that the reference consumes
    numbers an fp32 tensor can hold exactly (u = "f32") or the boundary values themselves (u = "hand").
Stored per case: depth, u (fp64), rgb (if any), mask, sparse, rgbd (if rgb) and the parameters; nothing larger than the largest G20
file.  Asserted before anything is written: the outputs equal tests/sparsify_cases.restate bit for bit; each case holds what it is
there for (see `purpose`); max_depth is compared in fp32 by the numpy that ran (recorded in the manifest)."""
import contextlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CSPN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sparsify_cases as sc                                  # noqa: E402


def import_reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_dense_to_sparse", os.path.join(REF, "dataloaders", "nyu_dataloader", "dense_to_sparse.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def given_uniform(plane):
    real = np.random.uniform

    def fake(low, high, size):
        assert (low, high) == (0, 1) and tuple(size) == plane.shape
        return plane
    np.random.uniform = fake
    try:
        yield
    finally:
        np.random.uniform = real


def to_tensor(img):
    return torch.from_numpy(img.transpose((2, 0, 1)).copy()).float()            # transforms.py:216, :224


def reference_frame(ref, case, depth_hw, rgb_chw, seed, hand):
    """One frame through the reference -> (u fp64 [H,W], mask bool [H,W], sparse fp32 [H,W], rgbd fp32 [4,H,W] or None)."""
    sparsifier = ref.UniformSampling(case["num_samples"], case["max_depth"])
    if rgb_chw is None:
        rgb_np = None
    elif rgb_chw.dtype == np.uint8:
        rgb_np = np.asarray(rgb_chw.transpose(1, 2, 0), dtype=float) / 255      # nyu_dataloader.py:29
    else:
        rgb_np = rgb_chw.transpose(1, 2, 0)
    np.random.seed(seed)
    if case["u"] == "seeded":
        mask = sparsifier.dense_to_sparse(rgb_np, depth_hw)
        np.random.seed(seed)
        u = np.random.uniform(0, 1, depth_hw.shape)
    else:
        u = hand if hand is not None else np.random.uniform(0, 1, depth_hw.shape).astype(np.float32).astype(np.float64)
        with given_uniform(u):
            mask = sparsifier.dense_to_sparse(rgb_np, depth_hw)
    sparse_depth = np.zeros(depth_hw.shape)                                     # dataloader.py:90
    sparse_depth[mask] = depth_hw[mask]                                         # dataloader.py:91
    sparse = torch.from_numpy(sparse_depth.copy()).float().numpy()              # transforms.py:218, :224 (modality 'd')
    rgbd = None
    if rgb_np is not None:
        rgbd = to_tensor(np.append(rgb_np, np.expand_dims(sparse_depth, axis=2), axis=2)).numpy()   # dataloader.py:96
    return u, mask, sparse, rgbd


def purpose(ref, name, case, depth, u, mask, sparse):
    """What each case is there for, asserted; -> a dict for the manifest."""
    B = depth.shape[0]
    with np.errstate(invalid="ignore"):
        keep = depth > 0
        if not np.isposinf(case["max_depth"]):
            keep &= depth <= np.float32(case["max_depth"])
    n_keep = [int(keep[b].sum()) for b in range(B)]
    n_mask = [int(mask[b].sum()) for b in range(B)]
    info = dict(n_keep=n_keep, n_sampled=n_mask, u_fits_fp32=bool(sc.fp32_exact(u)))
    if name == "valid_1x1":
        assert n_keep == [1] and n_mask == [1]
    if name == "invalid_1x1":
        assert n_keep == [0] and n_mask == [0]
    if name.startswith("odd_3x5x7"):
        assert (depth.shape[2] * depth.shape[3]) % 4 and all(0 < m < k for m, k in zip(n_mask, n_keep))
    if name.startswith("empty_middle"):
        assert n_keep[1] == 0 and n_keep[0] and n_keep[2] and n_mask[0] and n_mask[2] and n_mask[1] == 0
    if name.startswith("all_sampled"):
        assert n_mask == n_keep and all(case["num_samples"] >= k > 0 for k in n_keep)
    if name.startswith("none_sampled"):
        assert case["num_samples"] == 0 and not mask.any() and all(n_keep)
    if name.startswith("max_depth"):
        md32, md64 = np.float32(case["max_depth"]), case["max_depth"]
        assert float(md32) > md64                                   # fp32(2.7) lies above 2.7: `depth == fp32(2.7)` separates the two comparisons
        flat_d, flat_k = depth.reshape(B, -1), keep.reshape(B, -1)
        assert (flat_d > md32).any() and all(flat_d[b, 1] == md32 for b in range(B))
        info["cut_pixels"] = int(((depth > 0) & ~keep).sum())
        info["depth_equal_to_fp32_max_depth_is_kept"] = bool(flat_k[:, 1].all())
        # the REFERENCE's own keep mask (num_samples so large that every kept pixel is sampled) is the fp32 comparison
        ref_keep = np.stack([ref.UniformSampling(10 ** 9, md64).dense_to_sparse(None, depth[b, 0]) for b in range(B)])[:, None]
        assert np.array_equal(ref_keep, keep) and flat_k[:, 1].all()
    if name.startswith("hostile"):
        assert np.isnan(depth).any() and np.isposinf(depth).any() and np.isneginf(depth).any() and (depth < 0).any()
        assert (np.signbit(depth) & (depth == 0)).any()
        assert not np.signbit(sparse).any() and not np.isnan(sparse).any()
        info["inf_sampled"] = int(np.isposinf(sparse).sum())
    if name == "boundary_quarter":
        assert n_keep == [4] and case["num_samples"] == 1 and mask.reshape(-1).tolist() == [False, True, False, True, False, False]
        assert (u == 0.25).sum() == 2 and (u == np.nextafter(0.25, 0.0)).sum() == 2
    if name in sc.SPANS_SLICES:
        hw = depth.shape[2] * depth.shape[3]
        assert sc.slices(hw) == sc.SPANS_SLICES[name] > 1
        info["count_slices_per_frame"] = sc.slices(hw)
        info["why"] = "%d pixels = %d units of 4 pixels; a count slice covers 256 units (1024 pixels)" % (hw, -(-hw // 4))
    if name == "frame_57x76":
        assert case["num_samples"] == 500
    return info


if __name__ == "__main__":
    ref = import_reference()
    manifest = {"files": {}, "cases": {}, "numpy": np.__version__, "torch": torch.__version__}
    # how the numpy that runs the reference compares an fp32 array with the Python float max_depth
    probe = np.array([np.float32(2.7)], np.float32)
    manifest["max_depth_compared_in_fp32"] = bool((probe <= 2.7)[0])
    assert manifest["max_depth_compared_in_fp32"]
    for name, case in sc.CASES.items():
        B, H, W = case["shape"]
        depth, rgb = sc.make_depth(case), sc.make_rgb(case)
        hand = sc.hand_uniform(case) if case["u"] == "hand" else None
        outs = [reference_frame(ref, case, depth[b, 0], None if rgb is None else rgb[b], case["seed"] + 100 * b,
                                None if hand is None else hand[b, 0]) for b in range(B)]
        u = np.stack([o[0] for o in outs])[:, None]
        mask = np.stack([o[1] for o in outs])[:, None]
        sparse = np.stack([o[2] for o in outs])[:, None]
        rgbd = None if rgb is None else np.stack([o[3] for o in outs])
        assert u.dtype == np.float64 and mask.dtype == bool and sparse.dtype == np.float32
        if case["u"] == "f32":
            assert sc.fp32_exact(u)
        # the independent restatement, bit for bit
        want_mask, want_sparse = sc.restate(depth, u, case["num_samples"], case["max_depth"])
        assert np.array_equal(mask, want_mask) and sc.same_bits(sparse, want_sparse), name
        if rgb is not None:
            assert rgbd.dtype == np.float32 and sc.same_bits(rgbd, sc.restate_rgbd(rgb, want_sparse)), name
            if rgb.dtype == np.uint8 and rgb.size >= 256:
                assert np.unique(rgb).size == 256
        manifest["cases"][name] = dict(purpose(ref, name, case, depth, u, mask, sparse), shape=list(case["shape"]),
                                       num_samples=case["num_samples"], max_depth=repr(float(case["max_depth"])), u=case["u"], rgb=case["rgb"])
        arrs = dict(depth=depth, u=u, mask=mask, sparse=sparse, num_samples=np.int64(case["num_samples"]),
                    max_depth=np.float64(case["max_depth"]), seed=np.int64(case["seed"]))
        if rgb is not None:
            arrs.update(rgb=rgb, rgbd=rgbd)
        path = os.path.join(HERE, "g21_sparsify_%s.npz" % name)
        np.savez_compressed(path, **arrs)
        manifest["files"]["g21_sparsify_" + name] = {"bytes": os.path.getsize(path), "arrays": {k: list(np.shape(v)) for k, v in arrs.items()}}
        assert os.path.getsize(path) <= sc.MAX_FILE_BYTES, (name, os.path.getsize(path))
    with open(os.path.join(HERE, "golden_g21_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest, indent=1, sort_keys=True))

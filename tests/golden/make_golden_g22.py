"""Golden G22: the reference's NYU train / val transforms (dataloaders/nyu_dataloader/nyu_dataloader.py:13-44 with transforms.py and
ColorJitter(0.4, 0.4, 0.4) of dataloader.py:54), per frame, on the CPU.

The maker loads the reference's own transforms.py from CSPN_REFERENCE (default /root/reference — nothing of it is copied) by file
path.  transforms.py calls scipy.misc.imresize, which scipy removed; the maker first puts a Pillow-based stand-in with imresize's
own definition into scipy.misc: Image.fromarray (mode F for 2-D input), size = (np.array(im.size) * f).astype(int),
im.resize(size, resample=NEAREST) — the same kind of stub the other golden makers use for torch._thnn.  NYUDataset itself needs h5py
and np.asfarray, which do not exist here, so the transform lists of nyu_dataloader.py:20-26 and :36-39 are composed below from the
reference's classes, the jitter ops go through the reference's adjust_* functions in the recorded order (ColorJitter.get_params
draws factors and order from numpy's global generator; here they are the case's parameters), `asfarray(x) / 255` is
`np.asarray(x, dtype=float) / 255`, and ToTensor is the reference's class.  s is passed as a Python float.

Stored per case: the parameter rows and the outputs; inputs are rebuilt from the case's seed (tests/transform_cases.make_inputs).
The full-size cases store a SHA-256 of the output words in the manifest in place of arrays.  Asserted before anything is written:
  * the outputs equal tests/transform_cases.restate bit for bit (a NaN may match any NaN);
  * (a) every rotated coordinate of every frame with angle != 0 keeps a distance >= 1e-9 from a rounding tie and from the validity
    borders 0 and n - 1, so a last-bit difference in cos / sin cannot change a pixel (angle == 0: cos = 1 and sin = 0 exactly on
    every implementation, the coordinates are the integers themselves);
  * (b) inside the window actually used the running-sum table differs from the closed form in a row case and in a column case;
  * (c) a case has zero-filled corners;
  * what else each case is there for (see `purpose`)."""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CSPN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import transform_cases as tc                                  # noqa: E402


def imresize(arr, size, interp="nearest", mode=None):
    from PIL import Image
    assert interp == "nearest" and isinstance(size, float)
    im = Image.fromarray(arr, mode="F") if arr.ndim == 2 else Image.fromarray(arr)
    assert (arr.ndim == 2) == (mode == "F")
    size = tuple(int(v) for v in (np.array(im.size) * size).astype(int))
    return np.array(im.resize(size, resample=Image.NEAREST))


def import_reference():
    warnings.simplefilter("ignore", DeprecationWarning)
    import scipy.misc
    scipy.misc.imresize = imresize
    spec = importlib.util.spec_from_file_location("reference_transforms", os.path.join(REF, "dataloaders", "nyu_dataloader", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ADJUST = {tc.OP_BRIGHTNESS: ("adjust_brightness", tc.P_BRIGHTNESS), tc.OP_CONTRAST: ("adjust_contrast", tc.P_CONTRAST),
          tc.OP_SATURATION: ("adjust_saturation", tc.P_SATURATION)}


def reference_frame(T, rgb_chw, depth_hw, p, case):
    """One frame through the reference -> rgb fp32 [3,oh,ow], depth fp32 [oh,ow]"""
    from PIL import Image
    rgb = np.ascontiguousarray(rgb_chw.transpose(1, 2, 0))                      # the h5 layout transposed, dataloader.py:24
    if p is None:
        depth_np = depth_hw                                                     # nyu_dataloader.py:35
        transform = T.Compose([T.Resize(case["first"]), T.CenterCrop(case["out"])])
        rgb_np = transform(rgb)
    else:
        s, angle, do_flip = float(p[tc.P_S]), float(p[tc.P_ANGLE]), bool(p[tc.P_FLIP])
        depth_np = depth_hw / s                                                 # nyu_dataloader.py:15
        assert depth_np.dtype == np.float32
        transform = T.Compose([T.Resize(case["first"]), T.Rotate(angle), T.Resize(s), T.CenterCrop(case["out"]), T.HorizontalFlip(do_flip)])
        rgb_np = transform(rgb)
        if int(p[tc.P_ORDER]) >= 0:                                             # transforms.py:513-516 with the recorded draw
            pil = Image.fromarray(np.ascontiguousarray(rgb_np))
            for op in tc.ORDERS[int(p[tc.P_ORDER])]:
                pil = getattr(T, ADJUST[op][0])(pil, float(p[ADJUST[op][1]]))
            rgb_np = np.array(pil)
    assert rgb_np.dtype == np.uint8
    rgb_np = np.asarray(rgb_np, dtype=float) / 255                              # nyu_dataloader.py:29 / :41
    with np.errstate(all="ignore"):
        depth_np = transform(depth_np)
    to_tensor = T.ToTensor()
    return to_tensor(rgb_np).numpy(), to_tensor(np.ascontiguousarray(depth_np)).numpy()


def tie_distance(case):
    """(a): the smallest distance of a rotated coordinate from k + 0.5, from 0 and from n - 1, over the frames with angle != 0"""
    worst = np.inf
    for p in tc.params_of(case):
        if p[tc.P_ANGLE] == 0:
            continue
        cy, cx, h1, w1 = tc.rotated_coordinates(p, case["raw"], case["first"], case["out"])
        for c, n in ((cy, h1), (cx, w1)):
            frac = c - np.floor(c)
            worst = min(worst, float(np.abs(frac - 0.5).min()), float(np.abs(c).min()), float(np.abs(c - (n - 1)).min()))
    return worst


def table_differences(case):
    """(b): entries inside the used window where the running sum and the closed form differ -> (rows, columns)"""
    raw, out = case["raw"], case["out"]
    h1, w1 = tc.out_len(raw[0], case["first"]), tc.out_len(raw[1], case["first"])
    rows = int((tc.resize_table(raw[0], h1) != tc.closed_form_table(raw[0], h1)).sum())
    cols = int((tc.resize_table(raw[1], w1) != tc.closed_form_table(raw[1], w1)).sum())
    if case["mode"] == "val":                   # the crop window of the first tables; a train frame's rotation reaches all of them
        _, _, _, _, i0, j0 = tc.geometry(raw, case["first"], out)
        rows = int((tc.resize_table(raw[0], h1) != tc.closed_form_table(raw[0], h1))[i0:i0 + out[0]].sum())
        cols = int((tc.resize_table(raw[1], w1) != tc.closed_form_table(raw[1], w1))[j0:j0 + out[1]].sum())
        return rows, cols
    for p in tc.params_of(case):
        _, _, h2, w2, i0, j0 = tc.geometry(raw, case["first"], out, p[tc.P_S])
        rows += int((tc.resize_table(h1, h2) != tc.closed_form_table(h1, h2))[i0:i0 + out[0]].sum())
        cols += int((tc.resize_table(w1, w2) != tc.closed_form_table(w1, w2))[j0:j0 + out[1]].sum())
    return rows, cols


def purpose(name, case, rgb_in, rgb, depth):
    info = {}
    params = tc.params_of(case)
    if params is not None:
        zero_filled = [int((~tc.source_map(p, case["raw"], case["first"], case["out"])[0]).sum()) for p in params]
        info["zero_filled_pixels"] = zero_filled
        if any(p[tc.P_ANGLE] != 0 for p in params):
            info["tie_distance"] = tie_distance(case)
            assert info["tie_distance"] >= 1e-9, (name, info)
        if name.startswith("rot5"):
            assert all(z > 0 for z in zero_filled)                              # (c)
        if name.startswith(("identity", "half_mean", "tiny")):
            assert zero_filled[0] == 0
    info["table_differs_rows_cols"] = list(table_differences(case))
    if name.startswith("orders"):
        assert sorted(int(p[tc.P_ORDER]) for p in params) == list(range(6))
    if name.startswith("factors"):
        f = params[:, tc.P_BRIGHTNESS:tc.P_SATURATION + 1]
        assert (f[0] == 1).all() and (f[1] < 1).all() and (f[2] > 1).all() and params[3, tc.P_ORDER] == -1
        assert (rgb[2] == 1.0).any()                                            # the clipping branch was taken
    if name.startswith("half_mean"):
        for b, p in enumerate(params):
            valid, r0, c0 = tc.source_map(p, case["raw"], case["first"], case["out"])
            lum = tc.luma(rgb_in[b][:, r0, c0].astype(np.int64))
            assert 2 * int(lum.sum()) == 201 * lum.size and tc.contrast_constant(rgb_in[b][:, r0, c0].astype(np.int64)) == 101
    if case["depth"] == "hostile":
        assert np.isnan(depth).any() and np.isposinf(depth).any() and np.isneginf(depth).any() and (depth < 0).any()
        # val copies a -0; a train frame's -0 went through scipy's order-0 sum (`t = 0; t += v`) and left as +0
        assert (depth == 0).any() and bool((np.signbit(depth) & (depth == 0)).any()) == (case["mode"] == "val")
    if name.startswith("mid"):
        assert -(-case["out"][0] * case["out"][1] // tc.GATHER_THREADS) == 17
    return info


if __name__ == "__main__":
    import PIL
    import scipy
    T = import_reference()
    manifest = {"files": {}, "cases": {}, "digests": {}, "numpy": np.__version__, "torch": torch.__version__, "pillow": PIL.__version__,
                "scipy": scipy.__version__}
    rows_differ = cols_differ = 0
    for name, case in tc.CASES.items():
        rgb_in, depth_in = tc.make_inputs(case)
        params = tc.params_of(case)
        B = tc.n_frames(case)
        outs = [reference_frame(T, rgb_in[b], depth_in[b, 0], None if params is None else params[b], case) for b in range(B)]
        rgb = np.stack([o[0] for o in outs])
        depth = np.stack([o[1] for o in outs])[:, None]
        assert rgb.dtype == np.float32 and depth.dtype == np.float32
        assert rgb.shape == (B, 3) + tuple(case["out"]) and depth.shape == (B, 1) + tuple(case["out"])
        want_rgb, want_depth = tc.restate(rgb_in, depth_in, params, case["first"], case["out"])
        n_rgb = int((tc.words(rgb) != tc.words(want_rgb)).sum())
        n_depth = int((tc.words(depth) != tc.words(want_depth)).sum())
        assert n_rgb == 0 and n_depth == 0, (name, n_rgb, n_depth)
        info = purpose(name, case, rgb_in, rgb, depth)
        rows_differ += info["table_differs_rows_cols"][0] > 0
        cols_differ += info["table_differs_rows_cols"][1] > 0
        manifest["cases"][name] = dict(info, raw=list(case["raw"]), first=repr(float(case["first"])), out=list(case["out"]), mode=case["mode"],
                                       frames=B, seed=case["seed"])
        if name in tc.DIGEST_ONLY:
            manifest["digests"][name] = tc.digest(rgb, depth)
            continue
        arrs = dict(rgb=rgb, depth=depth, seed=np.int64(case["seed"]), first=np.float64(case["first"]))
        if params is not None:
            arrs["params"] = params
        path = os.path.join(HERE, "g22_transform_%s.npz" % name)
        np.savez_compressed(path, **arrs)
        manifest["files"]["g22_transform_" + name] = {"bytes": os.path.getsize(path), "arrays": {k: list(np.shape(v)) for k, v in arrs.items()}}
        assert os.path.getsize(path) <= tc.MAX_FILE_BYTES, (name, os.path.getsize(path))
    assert rows_differ >= 1 and cols_differ >= 1                                # (b)
    with open(os.path.join(HERE, "golden_g22_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest, indent=1, sort_keys=True))

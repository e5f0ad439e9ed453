"""Golden G25: the reference's comparison images (libs/utils.py:69-192: colored_depthmap, merge_into_row, merge_into_row_with_gt,
merge_rgb_depth_into_row, merge_features_into_row) on the CPU, with the matplotlib that is installed (recorded in the manifest).

The maker loads the reference's own libs/utils.py from CSPN_REFERENCE (default /root/reference — nothing of it is copied) by file
path, with a stub `tensorboardX` in sys.modules: only get_logger touches SummaryWriter, and it is not called.

For every case of tests/visual_cases.CASES: the inputs of visual_cases.make_inputs go through the reference's function frame by
frame, as torch CPU tensors (the functions call .cpu().numpy() themselves), and the result is cast with astype('uint8') — the cast
of the reference's save_image.  Stored per case: the inputs and `want` (g25_visual_<case>.npz).  Stored once: the 256 x 3 byte table
uint8(255 * jet(i)) (g25_visual_table.npz) — the only thing of matplotlib the package and its tests ever see.

Asserted before anything is written: every result equals tests/visual_cases.restate byte for byte; each case holds what it is there
for (see `purpose`); RGB stays in [0, 1], where the cast is defined."""
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

import visual_cases as vc                                    # noqa: E402


def import_reference():
    stub = types.ModuleType("tensorboardX")
    stub.SummaryWriter = object
    sys.modules.setdefault("tensorboardX", stub)
    spec = importlib.util.spec_from_file_location("reference_libs_utils", os.path.join(REF, "libs", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def u8(img):
    return img.astype("uint8")                               # libs/utils.py:131


def reference(ref, case, arrs):
    t = {k: torch.from_numpy(v.copy()) for k, v in arrs.items()}
    kind = case["kind"]
    if kind == "rgb":
        return np.stack([u8(ref.merge_into_row(t["rgb"][b], t["target"][b], t["pred"][b])) for b in range(t["rgb"].shape[0])])
    if kind == "rgbd":
        return np.stack([u8(ref.merge_into_row_with_gt(t["rgb"][b], t["sparse"][b], t["target"][b], t["pred"][b]))
                         for b in range(t["rgb"].shape[0])])
    if kind == "rgb_depth":
        return u8(ref.merge_rgb_depth_into_row(t["rgb"], t["pred"]))
    if kind == "colored":
        return u8(ref.colored_depthmap(arrs["depth"].copy(), case.get("d_min"), case.get("d_max")))
    if kind == "features":
        return u8(ref.merge_features_into_row(t["features"], case["n"]))
    raise ValueError(kind)


def purpose(name, case, arrs, want, table):
    """What each case is there for, asserted; -> a dict for the manifest."""
    info = {}
    black = (want == 0).all(-1)
    if case["kind"] in ("rgb", "rgbd", "rgb_depth"):
        W = case["shape"][2]
        assert arrs["rgb"].min() >= 0 and arrs["rgb"].max() <= 1
        info["row_bytes"] = int(want.shape[-2] * 3)
        depth_black = black[..., W:]
    if name in ("odd_5x7", "batch_3x20x13"):
        assert info["row_bytes"] % 4 and case["shape"][2] % 4
    if name == "constant_plane":
        assert depth_black.all()                             # 0 / 0
    if name in ("nan_in_target", "nan_in_sparse"):
        assert depth_black.all()                             # the FIRST argument: min(nan, p) keeps the NaN, the whole row is black
    if name in ("nan_in_pred", "nan_in_pred_rgbd", "nan_in_target_rgbd"):
        info["black_depth_pixels"] = int(depth_black.sum())
        assert depth_black.sum() == 1                        # a later argument: `p < t` is false for a NaN p, only the pixel itself is black
    if name == "posinf_max":
        assert depth_black.sum() == 1 and (want[..., case["shape"][2]:, :][~depth_black] == table[0]).all()
    if name == "neginf_min":
        assert depth_black.all()                             # d + inf = inf, inf / inf = NaN
    if name == "rel_is_one":
        assert (want[0, -1, 2 * W - 1] == table[255]).all()
    if name == "table_boundaries":
        got = want[0, :, W:2 * W].reshape(768, 3)
        idx = np.repeat(np.arange(256), 3).reshape(256, 3) + np.array([-1, 0, 0])
        idx[0, 0] = 0
        assert np.array_equal(got, table[idx.reshape(-1)])
        assert (want[0, 0, 2 * W] == table[255]).all() and (want[0, 0, 2 * W + 1] == table[255]).all() and (want[0, 0, 2 * W + 2] == table[128]).all()
    if name == "explicit_range":
        d = arrs["depth"]
        assert (d < case["d_min"]).any() and (d > case["d_max"]).any()
        assert (want[d < case["d_min"]] == table[0]).all() and (want[d > case["d_max"]] == table[255]).all()
    if case["kind"] == "features":
        f, n = arrs["features"], case["n"]
        assert f[:n].min() > f.min() and f[:n].max() < f.max()          # the range is that of ALL planes
    return info


if __name__ == "__main__":
    import matplotlib
    import matplotlib.pyplot as plt
    ref = import_reference()
    assert ref.cmap is plt.cm.jet and ref.fmap is plt.cm.jet
    table = (255 * plt.cm.jet(np.arange(256))[:, :3]).astype("uint8")
    assert table.shape == (256, 3) and int(table[128, 0]) == 124 and 255 * plt.cm.jet(0.5)[0] < 125     # 124.99999…: truncated
    # the integer call and the float call of the colour map meet in the same table row
    mid = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256)
    assert np.array_equal((255 * plt.cm.jet(mid)[:, :3]).astype("uint8"), table)
    np.savez_compressed(os.path.join(HERE, "g25_visual_table.npz"), table=table)
    manifest = {"files": {"g25_visual_table": {"bytes": os.path.getsize(os.path.join(HERE, "g25_visual_table.npz")), "arrays": {"table": [256, 3]}}},
                "cases": {}, "numpy": np.__version__, "torch": torch.__version__, "matplotlib": matplotlib.__version__}
    for name, case in vc.CASES.items():
        arrs = vc.make_inputs(name)
        want = reference(ref, case, arrs)
        assert want.dtype == np.uint8
        mine = vc.restate(table, case, arrs)
        assert mine.shape == want.shape and np.array_equal(mine, want), name
        manifest["cases"][name] = dict(purpose(name, case, arrs, want, table), kind=case["kind"], shape=list(case["shape"]),
                                       **{k: repr(case[k]) for k in ("d_min", "d_max", "n") if k in case})
        stored = dict(arrs, want=want)
        path = os.path.join(HERE, "g25_visual_%s.npz" % name)
        np.savez_compressed(path, **stored)
        manifest["files"]["g25_visual_" + name] = {"bytes": os.path.getsize(path), "arrays": {k: list(np.shape(v)) for k, v in stored.items()}}
        assert os.path.getsize(path) <= vc.MAX_FILE_BYTES, (name, os.path.getsize(path))
    with open(os.path.join(HERE, "golden_g25_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest["cases"], indent=1, sort_keys=True))
    # the table as csrc/cspn_visual.hip embeds it between its <jet-bytes> markers (tests/test_visual.py compares the two)
    print("\n".join("    " + " ".join("{%d,%d,%d}," % tuple(r) for r in table[i:i + 8]) for i in range(0, 256, 8)))

"""The comparison images of the reference (libs/utils.py:69-192), restated in numpy, and the cases golden G25, the CPU tests and the
GPU tests share (tests/golden/make_golden_g25.py, tests/test_visual.py).

The arithmetic, as the reference and matplotlib's Colormap.__call__ perform it on fp32 planes:
    d_min, d_max   np.min / np.max per plane (a NaN anywhere makes the plane's extremum NaN), combined over the planes by Python's
                   min(a, b, ..) / max(a, b, ..): the first argument stays unless a later one compares strictly less / greater
    rel = (d - d_min) / (d_max - d_min)          three separately rounded fp32 operations
    x   = rel * 256                               fp32 (Colormap: `xa *= self.N` on a float32 copy)
    i   = 255 if x == 256; 0 if x < 0; 255 if x >= 256; black if NaN; else trunc(x)
    rgb = uint8(255 * jet(i))                     float64, truncated by astype('uint8'): the 256 x 3 byte table of G25
The RGB panel is uint8(trunc(scale * v)) with the product in fp32; outside [0, 256) and for NaN numpy's cast is platform-defined
and the restatement SATURATES (NaN -> 0), as the kernels do."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_FILE_BYTES = 256 * 1024
F32 = np.float32


def load_table():
    """The 256 x 3 byte table recorded by the golden maker (matplotlib's jet; nothing here imports matplotlib)."""
    return np.load(os.path.join(GOLDEN, "g25_visual_table.npz"))["table"]


def py_min(values):
    m = values[0]
    for v in values[1:]:
        if v < m:
            m = v
    return m


def py_max(values):
    m = values[0]
    for v in values[1:]:
        if v > m:
            m = v
    return m


def plane_range(planes):
    """Python's min / max over the planes' np.min / np.max, in argument order."""
    with np.errstate(all="ignore"):
        return py_min([np.min(p) for p in planes]), py_max([np.max(p) for p in planes])


def colour(depth, d_min, d_max, table):
    """uint8 [H, W, 3] of an fp32 plane."""
    depth = np.asarray(depth, F32)
    with np.errstate(all="ignore"):
        rel = (depth - F32(d_min)) / (F32(d_max) - F32(d_min))
        x = rel * F32(256)
        assert rel.dtype == F32 and x.dtype == F32
        bad = np.isnan(x)
        idx = np.zeros(x.shape, np.int64)
        mid = ~bad & (x > 0) & (x < 256)
        idx[mid] = np.trunc(x[mid]).astype(np.int64)
        idx[~bad & (x >= 256)] = 255
    out = table[idx]
    out[bad] = 0
    return out


def rgb_bytes(rgb, scale):
    """uint8 [H, W, 3] of a [3, H, W] plane set: fp32 -> trunc(scale * v) saturated to [0, 255], NaN -> 0; uint8 -> itself."""
    rgb = np.asarray(rgb)
    if rgb.dtype == np.uint8:
        return np.ascontiguousarray(rgb.transpose(1, 2, 0))
    with np.errstate(all="ignore"):
        x = F32(scale) * rgb.astype(F32)
        assert x.dtype == F32
        out = np.zeros(x.shape, np.uint8)
        mid = (x > 0) & (x < 256)
        out[mid] = np.trunc(x[mid]).astype(np.uint8)
        out[x >= 256] = 255
    return np.ascontiguousarray(out.transpose(1, 2, 0))


def restate_row(table, rgb, planes, scale, d_min=None, d_max=None):
    """One frame: rgb [3, H, W] or None, planes a list of [H, W] -> uint8 [H, P * W, 3]."""
    lo, hi = plane_range(planes)
    lo = lo if d_min is None else d_min
    hi = hi if d_max is None else d_max
    panels = ([] if rgb is None else [rgb_bytes(rgb, scale)]) + [colour(p, lo, hi, table) for p in planes]
    return np.hstack(panels)


def restate_features(table, features, n):
    """[C, H, W] -> uint8 [H, n * W, 3]: one range over ALL C planes (the reference takes np.min / np.max of the whole tensor),
    the first n planes shown."""
    with np.errstate(all="ignore"):
        lo, hi = np.min(features), np.max(features)
    return np.hstack([colour(features[i], lo, hi, table) for i in range(n)])


def restate(table, case, arrs):
    """The expected bytes of a case from its recorded inputs: [B, H, P * W, 3], or [H, P * W, 3] for the single-frame kinds."""
    kind = case["kind"]
    if kind == "rgb":
        return np.stack([restate_row(table, arrs["rgb"][b], [arrs["target"][b, 0], arrs["pred"][b, 0]], 1.0) for b in range(arrs["rgb"].shape[0])])
    if kind == "rgbd":
        return np.stack([restate_row(table, arrs["rgb"][b], [arrs["sparse"][b, 0], arrs["target"][b, 0], arrs["pred"][b, 0]], 255.0)
                         for b in range(arrs["rgb"].shape[0])])
    if kind == "rgb_depth":
        return restate_row(table, arrs["rgb"], [arrs["pred"][0]], 1.0)
    if kind == "colored":
        return restate_row(table, None, [arrs["depth"]], 1.0, case.get("d_min"), case.get("d_max"))
    if kind == "features":
        return restate_features(table, arrs["features"], case["n"])
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------ the cases
# kind: rgb = merge_into_row, rgbd = merge_into_row_with_gt, rgb_depth = merge_rgb_depth_into_row, colored = colored_depthmap,
# features = merge_features_into_row.  shape: (B, H, W), or (C, H, W) for features.  `edit` names what make_inputs does to the planes.
CASES = {
    # H = 1 or W = 1: the reference's merge functions np.squeeze the unit axis away and fail in np.transpose, so colored_depthmap is the
    # only form it defines there; the merge forms of these shapes are RESTATEMENT_ONLY below
    "one_pixel": dict(kind="colored", shape=(1, 1, 1)),                 # a constant plane by construction: 0 / 0
    "row_1x3": dict(kind="colored", shape=(1, 1, 3)),
    "odd_5x7": dict(kind="rgb", shape=(1, 5, 7)),                       # row of 63 bytes, W % 4 = 3
    "batch_3x13x20": dict(kind="rgb", shape=(3, 13, 20)),
    "batch_3x20x13": dict(kind="rgb", shape=(3, 20, 13)),               # row of 117 bytes, W % 4 = 1: every row starts off the dword grid
    "batch_3x57x77": dict(kind="rgb", shape=(3, 57, 77), rgb="bytes"),               # several workgroups and range chunks per frame
    "constant_plane": dict(kind="rgb", shape=(1, 5, 7), edit="constant"),
    "target_is_pred": dict(kind="rgb", shape=(1, 5, 7), edit="same"),
    "nan_in_target": dict(kind="rgb", shape=(1, 5, 7), edit="nan_target"),
    "nan_in_pred": dict(kind="rgb", shape=(1, 5, 7), edit="nan_pred"),
    "nan_in_sparse": dict(kind="rgbd", shape=(1, 5, 7), edit="nan_sparse"),
    "nan_in_target_rgbd": dict(kind="rgbd", shape=(1, 5, 7), edit="nan_target"),     # the target is the SECOND argument there
    "nan_in_pred_rgbd": dict(kind="rgbd", shape=(1, 5, 7), edit="nan_pred"),
    "posinf_max": dict(kind="rgb", shape=(1, 5, 7), edit="posinf"),
    "neginf_min": dict(kind="rgb", shape=(1, 5, 7), edit="neginf"),
    "rel_is_one": dict(kind="rgb", shape=(1, 4, 8), edit="rel_one"),
    "table_boundaries": dict(kind="rgb", shape=(1, 16, 48), edit="boundaries"),
    "explicit_range": dict(kind="colored", shape=(1, 9, 11), d_min=float(F32(1.3)), d_max=float(F32(6.1))),
    "explicit_max_only": dict(kind="colored", shape=(1, 9, 11), d_max=float(F32(6.1))),
    "explicit_min_only": dict(kind="colored", shape=(1, 9, 11), d_min=float(F32(1.3))),
    "own_range": dict(kind="colored", shape=(1, 9, 11)),
    "rgbd_four_panels": dict(kind="rgbd", shape=(2, 13, 21)),
    "rgbd_byte_rgb": dict(kind="rgbd", shape=(1, 13, 21), rgb="bytes"),   # 255 * fl(k / 255) in fp32, truncated
    "rgb_depth": dict(kind="rgb_depth", shape=(1, 5, 7)),
    "features_n9": dict(kind="features", shape=(12, 9, 11), n=9),
    "features_n3": dict(kind="features", shape=(12, 9, 11), n=3),
}


# checked against the restatement alone: shapes the reference fails on, and RGB outside [0, 1], where its cast is platform-defined
RESTATEMENT_ONLY = {
    "merge_one_pixel": dict(kind="rgb", shape=(1, 1, 1)),
    "merge_row_1x3": dict(kind="rgbd", shape=(2, 1, 3)),
    "merge_column_3x1": dict(kind="rgb", shape=(1, 3, 1)),
    "rgb_out_of_range": dict(kind="rgbd", shape=(1, 5, 7), edit="wild_rgb"),
    "rgb_out_of_range_scale1": dict(kind="rgb", shape=(1, 5, 7), edit="wild_rgb"),
}


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)


def make_inputs(name):
    """The fp32 inputs of a case, from a legacy RandomState (the golden RECORDS them; tests read the record)."""
    case = CASES[name] if name in CASES else RESTATEMENT_ONLY[name]
    rng = np.random.RandomState(_seed(name))
    kind, edit = case["kind"], case.get("edit")
    if kind == "features":
        f = rng.normal(0, 1, case["shape"]).astype(F32)
        f[case["shape"][0] - 1, 0, 0], f[case["shape"][0] - 2, 1, 1] = F32(-7.5), F32(9.25)    # the extrema lie in planes that are not shown
        return dict(features=f)
    B, H, W = case["shape"]
    if kind == "colored":
        return dict(depth=rng.uniform(0.5, 9.5, (H, W)).astype(F32))
    rgb = rng.uniform(0, 1, (B, 3, H, W)).astype(F32)
    if case.get("rgb") == "bytes":                                        # k / 255, as a loader makes them: a third of the file size
        rgb = (rng.randint(0, 256, (B, 3, H, W)).astype(F32) / F32(255)).astype(F32)
    rgb.reshape(-1)[0] = 1.0                                              # scale 1: the only value that gives a byte of 1
    if rgb.size > 1:
        rgb.reshape(-1)[-1] = 0.0
    target = rng.uniform(0.7, 9.9, (B, 1, H, W)).astype(F32)
    pred = (target + rng.normal(0, 0.6, target.shape)).astype(F32)
    sparse = np.where(rng.uniform(0, 1, target.shape) < 0.2, target, 0).astype(F32)
    if edit == "constant":
        target[:] = F32(2.5)
        pred[:] = F32(2.5)
    elif edit == "same":
        pred = target.copy()
    elif edit == "nan_target":
        target[0, 0, 2, 3] = np.nan
    elif edit == "nan_pred":
        pred[0, 0, 2, 3] = np.nan
    elif edit == "nan_sparse":
        sparse[0, 0, 2, 3] = np.nan
    elif edit == "posinf":
        pred[0, 0, 1, 1] = np.inf
    elif edit == "neginf":
        target[0, 0, 4, 6] = -np.inf
    elif edit == "rel_one":
        target[:] = np.linspace(0, 1, H * W, dtype=F32).reshape(H, W)     # min 0, max 1: rel == 1 at the last pixel
        pred = (target * F32(0.5) + F32(0.25)).astype(F32)
    elif edit == "boundaries":
        # range [0, 1], so rel = d and x = 256 d exactly: every i / 256 with its two fp32 neighbours
        k = np.arange(256, dtype=F32) / F32(256)
        tri = np.stack([np.nextafter(k, F32(-1)), k, np.nextafter(k, F32(2))], 1).reshape(-1)     # 768 values
        tri[0] = 0.0                                                       # below 0 would move the minimum
        target[:] = tri.reshape(H, W)
        pred[:] = F32(1.0)
        pred.reshape(-1)[1] = np.nextafter(F32(1), F32(0))
        pred.reshape(-1)[2] = F32(0.5)
    elif edit == "wild_rgb":
        rgb.reshape(-1)[:12] = np.array([-0.5, -1e30, 1.5, 255.5, 256.0, 300.0, 1e30, np.inf, -np.inf, np.nan, 1.0 + 2.0 ** -20, -0.0], F32)
    if kind == "rgb":
        return dict(rgb=rgb, target=target, pred=pred)
    if kind == "rgbd":
        return dict(rgb=rgb, sparse=sparse, target=target, pred=pred)
    return dict(rgb=rgb[0], pred=pred[0])                                 # rgb_depth


def panels_of(kind, n=None):
    return {"rgb": 3, "rgbd": 4, "rgb_depth": 2, "colored": 1}.get(kind, n)

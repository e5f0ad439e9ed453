"""The comparison images (cspn_monodepth_amd/utils.py, include/cspn_visual.h).

  * CPU: the numpy restatement (tests/visual_cases.py) against golden G25 — the reference's libs/utils.py with matplotlib's jet,
    recorded by tests/golden/make_golden_g25.py — byte for byte; the table embedded in cspn_visual.hip against the golden's; the
    header / library / loader contract; every refusal that needs no device; the sheet's row bookkeeping.
  * GPU: every G25 case with torch.equal against the golden bytes — no tolerance: every step is one IEEE fp32 operation or a table
    lookup; a frame's bytes alone, first and last in a batch, and through ComparisonSheet; an `out=` slice of a sentinel-filled
    buffer; a captured replay after the inputs changed in place; two runs.  Nothing here reads the reference or matplotlib."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import visual_cases as vc
from conftest import ROOT, golden_names, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import utils

DEV = "cuda:0"
NAMES = sorted(vc.CASES)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def table():
    return vc.load_table()


@pytest.fixture(scope="module")
def golden():
    return {name: load_golden("g25_visual_" + name) for name in NAMES}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_case(case, arrs):
    """A case through the public functions, on device copies of its recorded inputs -> uint8 device tensor shaped like `want`."""
    kind = case["kind"]
    if kind == "rgb":
        return utils.comparison_rows(dev(arrs["rgb"]), dev(arrs["target"]), dev(arrs["pred"]), "rgb")
    if kind == "rgbd":
        return utils.comparison_rows(dev(np.concatenate([arrs["rgb"], arrs["sparse"]], 1)), dev(arrs["target"]), dev(arrs["pred"]), "rgbd")
    if kind == "rgb_depth":
        return utils.merge_rgb_depth_into_row(dev(arrs["rgb"]), dev(arrs["pred"]))
    if kind == "colored":
        return utils.colored_depthmap(dev(arrs["depth"]), case.get("d_min"), case.get("d_max"))
    return utils.merge_features_into_row(dev(arrs["features"]), case["n"])


# ------------------------------------------------------------------------------------------------ CPU: golden and restatement
def test_golden_holds_every_case():
    assert sorted(golden_names("g25_visual_")) == sorted(["g25_visual_" + n for n in NAMES] + ["g25_visual_table"])
    for path in golden_names("g25_visual_"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", path + ".npz")) <= vc.MAX_FILE_BYTES


def test_table_is_matplotlibs_truncated_bytes(table):
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert table[128].tolist() == [124, 255, 121]                 # 255 * jet(0.5)[0] = 124.99999…: truncated, not rounded
    assert table[0].tolist() == [0, 0, 127] and table[255].tolist() == [127, 0, 0]
    assert not (table == 0).all(1).any()                          # no entry is black: black means NaN


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name, table, golden):
    arrs = golden[name]
    want = arrs["want"]
    got = vc.restate(table, vc.CASES[name], arrs)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    for k, v in vc.make_inputs(name).items():                     # the record is what the case list makes
        assert np.array_equal(v, arrs[k], equal_nan=True), k


def test_restatement_of_the_python_min_rule(table):
    nan, f = np.float32("nan"), np.float32
    assert np.isnan(vc.py_min([nan, f(1)])) and vc.py_min([f(1), nan]) == 1 and vc.py_min([f(2), nan, f(1)]) == 1
    assert np.isnan(vc.py_max([nan, f(1)])) and vc.py_max([f(1), nan]) == 1 and vc.py_max([f(1), nan, f(2)]) == 2
    t, p = np.array([[1, nan]], np.float32), np.array([[0, 2]], np.float32)
    assert (vc.restate_row(table, None, [t, p], 1.0) == 0).all()                         # NaN in the first plane: all black
    row = vc.restate_row(table, None, [p, t], 1.0)
    assert (row[0, 3] == 0).all() and row[0, :3].any(1).all()                            # in a later plane: the pixel alone


def test_restatement_saturates_rgb():
    v = np.array([-1, 0, 0.5, 1, 255, 255.9, 256, 1e30, np.inf, -np.inf, np.nan, 1.0 / 255], np.float32).reshape(1, 1, 12).repeat(3, 0)
    assert vc.rgb_bytes(v, 1.0)[0, :, 0].tolist() == [0, 0, 0, 1, 255, 255, 255, 255, 255, 0, 0, 0]
    assert vc.rgb_bytes(v, 255.0)[0, :, 0].tolist() == [0, 0, 127, 255, 255, 255, 255, 255, 255, 0, 0, 1]
    u = np.arange(24, dtype=np.uint8).reshape(3, 2, 4)
    assert np.array_equal(vc.rgb_bytes(u, 255.0), u.transpose(1, 2, 0))


def test_embedded_table_equals_the_goldens(table):
    src = open(os.path.join(_lib.CSRC, "cspn_visual.hip")).read()
    body = re.search(r"// <jet-bytes>\n(.*?)// </jet-bytes>", src, flags=re.S).group(1)
    rows = re.findall(r"\{(\d+),(\d+),(\d+)\}", body)
    assert len(rows) == 256
    assert np.array_equal(np.array(rows, dtype=np.int64), table.astype(np.int64))
    assert "import matplotlib" not in open(os.path.join(ROOT, "cspn_monodepth_amd", "utils.py")).read()


# ------------------------------------------------------------------------------------------------ CPU: contract
def test_header_declares_the_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "cspn_visual.h")).read()
    assert int(re.search(r"^#define CSPN_VISUAL_RANGE_CHUNK (\d+)\b", src, flags=re.M).group(1)) == _lib.VISUAL_RANGE_CHUNK == 4096
    assert int(re.search(r"^#define CSPN_VISUAL_MAX_PLANES (\d+)\b", src, flags=re.M).group(1)) == _lib.VISUAL_MAX_PLANES == 3
    for k, name in enumerate(("NONE", "F32", "U8")):
        assert int(re.search(r"^#define CSPN_VISUAL_RGB_%s (\d+)\b" % name, src, flags=re.M).group(1)) == k == getattr(_lib, "VISUAL_RGB_" + name)
    assert ctypes.sizeof(_lib.cspn_visual_rows) == 104


def test_package_exports_the_module():
    import cspn_monodepth_amd as pkg
    assert pkg.utils is utils and "utils" in pkg.__all__
    for name in ("colored_depthmap", "merge_into_row", "merge_into_row_with_gt", "merge_rgb_depth_into_row", "add_row", "save_image",
                 "feature_map", "merge_features_into_row", "add_features_row", "save_featues_map", "save_features", "comparison_rows",
                 "ComparisonSheet"):
        assert name in utils.__all__ and callable(getattr(utils, name)), name
    for name in ("get_save_path", "get_logger", "write_config_file", "save_checkpoint"):
        assert not hasattr(utils, name) and name in utils.__doc__


def test_workspace_size_needs_no_device():
    chunk = _lib.VISUAL_RANGE_CHUNK
    assert utils.workspace_bytes(1, 1, 1) == 8
    assert utils.workspace_bytes(1, 1, chunk) == 8 and utils.workspace_bytes(1, 1, chunk + 1) == 16
    assert utils.workspace_bytes(3, 2, 57 * 77) == 3 * 2 * 2 * 8
    assert utils.workspace_bytes(24, 3, 228 * 304) == 24 * 3 * 17 * 8
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(RuntimeError, match="cspn_visual_workspace_bytes"):
            utils.workspace_bytes(*bad)


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    a = _lib.cspn_visual_rows()
    a.n_depth = 0
    assert not L.cspn_visual_rows(a, 1, 4, 4, None, 0, None, None) and b"n_depth" in L.cspn_last_error()
    a.n_depth = 4
    assert not L.cspn_visual_rows(a, 1, 4, 4, None, 0, None, None) and b"n_depth" in L.cspn_last_error()
    a.n_depth = 1
    assert not L.cspn_visual_rows(a, 1, 0, 4, None, 0, None, None) and b"H 0" in L.cspn_last_error()
    assert not L.cspn_visual_rows(a, 0, 4, 4, None, 0, None, None) and b"B 0" in L.cspn_last_error()
    assert not L.cspn_visual_rows(a, 1, 4, 4, None, 0, None, None) and b"out is NULL" in L.cspn_last_error()
    assert not L.cspn_visual_rows(None, 1, 4, 4, None, 0, None, None) and b"panels is NULL" in L.cspn_last_error()
    assert not L.cspn_visual_features(None, 0, 1, 3, 4, 4, 4, None, 0, None, None) and b"n 4 of 3" in L.cspn_last_error()
    assert not L.cspn_visual_features(None, 0, 1, 3, 4, 4, 0, None, 0, None, None) and b"n 0 of 3" in L.cspn_last_error()


def test_refusals():
    rgb, d = torch.zeros(3, 5, 7), torch.zeros(1, 5, 7)
    with pytest.raises(RuntimeError, match="ROCm device"):
        utils.merge_into_row(rgb, d, d)
    with pytest.raises(RuntimeError, match="ROCm device"):
        utils.colored_depthmap(d[0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        utils.merge_features_into_row(torch.zeros(9, 5, 7))
    with pytest.raises(RuntimeError, match="must be fp32"):
        utils.merge_into_row(rgb, d.double(), d)
    with pytest.raises(RuntimeError, match="must be fp32"):
        utils.merge_into_row(rgb, d, d.half())
    with pytest.raises(RuntimeError, match="must be fp32"):
        utils.merge_features_into_row(torch.zeros(9, 5, 7, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="fp32 or uint8"):
        utils.merge_into_row(rgb.double(), d, d)
    with pytest.raises(RuntimeError, match="non-contiguous planes"):
        utils.merge_into_row(rgb, torch.zeros(1, 7, 5).transpose(1, 2), d)
    with pytest.raises(RuntimeError, match="non-contiguous planes"):
        utils.merge_into_row(rgb, d, torch.zeros(1, 5, 14)[:, :, ::2])
    with pytest.raises(RuntimeError, match="3 channels"):
        utils.merge_into_row(torch.zeros(4, 5, 7), d, d)
    with pytest.raises(TypeError):
        utils.merge_into_row(rgb.numpy(), d, d)
    with pytest.raises(ValueError, match="modality"):
        utils.comparison_rows(torch.zeros(2, 1, 5, 7), torch.zeros(2, 1, 5, 7), torch.zeros(2, 1, 5, 7), "d")
    with pytest.raises(RuntimeError, match=r"\[B, 4, H, W\]"):
        utils.comparison_rows(torch.zeros(2, 3, 5, 7), torch.zeros(2, 1, 5, 7), torch.zeros(2, 1, 5, 7), "rgbd")


def test_comparison_sheet_bookkeeping():
    sheet = utils.ComparisonSheet()
    assert (sheet.rows, sheet.modality, sheet.panels, sheet.filled, sheet.full) == (8, "rgb", 3, 0, False)
    assert utils.ComparisonSheet(2, "rgbd").panels == 4
    with pytest.raises(ValueError):
        utils.ComparisonSheet(8, "d")
    with pytest.raises(ValueError):
        utils.ComparisonSheet(0)
    with pytest.raises(RuntimeError, match="nothing was added"):
        sheet.image()
    with pytest.raises(RuntimeError, match="ROCm device"):
        sheet.reserve(5, 7, "cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):
        sheet.add(torch.zeros(3, 5, 7), torch.zeros(1, 5, 7), torch.zeros(1, 5, 7))
    assert sheet.filled == 0 and sheet.buffer is None
    sheet.H, sheet.W = 5, 7
    assert [sheet.row_slice(k) for k in (0, 1, 7)] == [slice(0, 5), slice(5, 10), slice(35, 40)]
    with pytest.raises(IndexError):
        sheet.row_slice(8)
    sheet.filled = 8
    assert sheet.full
    with pytest.raises(RuntimeError, match="holds 8 rows"):
        sheet.add(torch.zeros(3, 5, 7), torch.zeros(1, 5, 7), torch.zeros(1, 5, 7))


def test_save_image_writes_the_bytes(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    img = torch.arange(5 * 6 * 3, dtype=torch.uint8).reshape(5, 6, 3)
    path = str(tmp_path / "row.png")
    utils.save_image(img, path)
    assert np.array_equal(np.asarray(Image.open(path)), img.numpy())
    utils.save_featues_map(utils.add_row(img, img), path)
    assert np.array_equal(np.asarray(Image.open(path)), torch.cat([img, img]).numpy())
    assert torch.equal(utils.add_features_row(img, img), torch.cat([img, img]))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_bytes_equal_the_reference(name, golden):
    arrs = golden[name]
    got = run_case(vc.CASES[name], arrs)
    want = dev(arrs["want"])
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want), (name, int((got != want).sum()))
    assert torch.equal(run_case(vc.CASES[name], arrs), got)                  # two runs


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(vc.RESTATEMENT_ONLY))
def test_device_bytes_equal_the_restatement_where_the_reference_has_none(name, table):
    case, arrs = vc.RESTATEMENT_ONLY[name], vc.make_inputs(name)
    want = dev(vc.restate(table, case, arrs))
    got = run_case(case, arrs)
    assert got.shape == want.shape and torch.equal(got, want), (name, int((got != want).sum()))


@pytest.mark.gpu
def test_single_frame_functions_and_views(golden, table):
    arrs = golden["rgbd_four_panels"]
    data = dev(np.concatenate([arrs["rgb"], arrs["sparse"]], 1))             # [B, 4, H, W]: the views below are not contiguous as a whole
    target, pred, want = dev(arrs["target"]), dev(arrs["pred"]), dev(arrs["want"])
    for b in range(data.shape[0]):
        assert torch.equal(utils.merge_into_row_with_gt(data[b, :3], data[b, 3:], target[b], pred[b]), want[b])
    arrs = golden["odd_5x7"]
    rgb, target, pred = dev(arrs["rgb"]), dev(arrs["target"]), dev(arrs["pred"])
    assert torch.equal(utils.merge_into_row(rgb[0], target[0], pred[0]), dev(arrs["want"])[0])
    assert torch.equal(utils.merge_into_row(rgb, target, pred), dev(arrs["want"])[0])          # [1, 3, H, W], as the reference squeezes
    # a uint8 RGB input is copied
    u8 = (arrs["rgb"][0] * 255).astype(np.uint8)
    want = dev(vc.restate_row(table, u8, [arrs["target"][0, 0], arrs["pred"][0, 0]], 1.0))
    assert torch.equal(utils.merge_into_row(dev(u8), target[0], pred[0]), want)
    arrs = golden["batch_3x13x20"]                                            # W % 4 == 0: the 16-byte path, and the same planes off it
    want = dev(arrs["want"])
    shifted = [torch.zeros(t.size + 1, device=DEV)[1:].view(t.shape).copy_(dev(t)) for t in (arrs["rgb"], arrs["target"], arrs["pred"])]
    assert shifted[1].data_ptr() % 16 == 4
    assert torch.equal(utils.comparison_rows(*shifted, "rgb"), want)
    u8 = (arrs["rgb"] * 255).astype(np.uint8)
    want8 = dev(np.stack([vc.restate_row(table, u8[b], [arrs["target"][b, 0], arrs["pred"][b, 0]], 1.0) for b in range(3)]))
    assert torch.equal(utils.comparison_rows(dev(u8), dev(arrs["target"]), dev(arrs["pred"]), "rgb"), want8)
    assert torch.equal(utils.feature_map(dev(golden["explicit_range"]["depth"]), vc.CASES["explicit_range"]["d_min"], vc.CASES["explicit_range"]["d_max"]),
                       dev(golden["explicit_range"]["want"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["batch_3x57x77", "batch_3x20x13", "rgbd_four_panels"])
def test_a_frames_bytes_do_not_depend_on_its_place(name, golden):
    arrs, case = golden[name], vc.CASES[name]
    modality = case["kind"]
    inp = arrs["rgb"] if modality == "rgb" else np.concatenate([arrs["rgb"], arrs["sparse"]], 1)
    inp, target, pred, want = dev(inp), dev(arrs["target"]), dev(arrs["pred"]), dev(arrs["want"])
    B = inp.shape[0]
    for b in range(B):
        alone = utils.comparison_rows(inp[b:b + 1], target[b:b + 1], pred[b:b + 1], modality)
        assert torch.equal(alone[0], want[b])
        order = [b] + [k for k in range(B) if k != b]                        # first in a batch ...
        assert torch.equal(utils.comparison_rows(inp[order], target[order], pred[order], modality)[0], want[b])
        order = order[1:] + [b, b][:3 - len(order[1:])]                      # ... and last in a batch of 3
        assert len(order) == 3 and torch.equal(utils.comparison_rows(inp[order], target[order], pred[order], modality)[2], want[b])
    sheet = utils.ComparisonSheet(B + 1, modality)
    for b in reversed(range(B)):
        sheet.add(inp[b], target[b], pred[b])
    assert sheet.filled == B and not sheet.full
    H = inp.shape[2]
    assert sheet.image().shape == (B * H, want.shape[2], 3)
    assert torch.equal(sheet.image().view(B, H, -1, 3), want.flip(0))
    assert not sheet.buffer[B * H:].any()                                    # the row that was not added
    sheet.add(inp[0], target[0], pred[0], index=B)
    assert sheet.filled == B and torch.equal(sheet.buffer[sheet.row_slice(B)], want[0])


@pytest.mark.gpu
def test_out_slice_leaves_its_surroundings_untouched(golden):
    for name, lead in (("batch_3x20x13", 1), ("odd_5x7", 3), ("batch_3x13x20", 2)):     # rows of 117, 63 and 180 bytes
        arrs = golden[name]
        want = dev(arrs["want"])
        B, H, PW = want.shape[0], want.shape[1], want.shape[2]
        big = torch.full((lead + B * H + 2, PW, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        out = big[lead:lead + B * H]
        assert out.data_ptr() % 4 == (lead * PW * 3) % 4
        got = utils.comparison_rows(dev(arrs["rgb"]), dev(arrs["target"]), dev(arrs["pred"]), "rgb", out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(out.view(B, H, PW, 3), want)
        assert (big[:lead] == SENTINEL).all() and (big[lead + B * H:] == SENTINEL).all()
    with pytest.raises(RuntimeError, match="out must be"):
        utils.comparison_rows(dev(arrs["rgb"]), dev(arrs["target"]), dev(arrs["pred"]), "rgb", out=big)


@pytest.mark.gpu
def test_captured_rows_follow_their_inputs(golden):
    a, b = golden["batch_3x13x20"], golden["batch_3x20x13"]
    flat = lambda arrs, k: arrs[k].reshape(3, -1, 260)                       # both cases hold 260 pixels per plane  # noqa: E731
    rgb, target, pred = (dev(flat(a, k)).view(3, -1, 13, 20) for k in ("rgb", "target", "pred"))
    sheet = utils.ComparisonSheet(3, "rgb").reserve(13, 20, torch.device(DEV))
    out = torch.zeros((3, 13, 60, 3), dtype=torch.uint8, device=DEV)
    work = torch.empty(utils.workspace_bytes(3, 2, 260), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        utils.comparison_rows(rgb, target, pred, "rgb", out=out, work=work)
        sheet.add(rgb[2], target[2], pred[2], index=1)
    graph.replay()
    assert torch.equal(out, dev(a["want"])) and torch.equal(sheet.buffer[sheet.row_slice(1)], dev(a["want"])[2])
    # new values in place, of the same plane size: the 20 x 13 case's planes read as 13 x 20 — the restatement says what that gives
    for t, k in ((rgb, "rgb"), (target, "target"), (pred, "pred")):
        t.copy_(dev(flat(b, k)).view(t.shape))
    graph.replay()
    table = vc.load_table()
    want = np.stack([vc.restate_row(table, flat(b, "rgb")[i].reshape(3, 13, 20), [flat(b, "target")[i].reshape(13, 20), flat(b, "pred")[i].reshape(13, 20)], 1.0)
                     for i in range(3)])
    assert torch.equal(out, dev(want)) and torch.equal(sheet.buffer[sheet.row_slice(1)], dev(want)[2])
    assert not torch.equal(dev(want), dev(a["want"]))


@pytest.mark.gpu
def test_features_and_saving(golden, tmp_path):
    arrs = golden["features_n9"]
    f = dev(arrs["features"])
    want = dev(arrs["want"])
    assert torch.equal(utils.merge_features_into_row(f), want)                               # featuers_num defaults to 9
    assert torch.equal(utils.merge_features_into_row(f.unsqueeze(0), 9), want)
    with pytest.raises(RuntimeError, match="feature panels"):
        utils.merge_features_into_row(f, 13)
    with pytest.raises(RuntimeError, match="not contiguous"):
        utils.merge_features_into_row(f.transpose(1, 2), 3)
    with pytest.raises(RuntimeError, match="same B x H x W"):
        utils.merge_into_row(torch.zeros(3, 9, 11, device=DEV), torch.zeros(1, 9, 11, device=DEV), torch.zeros(1, 9, 12, device=DEV))
    Image = pytest.importorskip("PIL.Image")
    path = str(tmp_path / "features.png")
    utils.save_features(dev(golden["features_n3"]["features"]), path, 3)
    assert np.array_equal(np.asarray(Image.open(path)), golden["features_n3"]["want"])

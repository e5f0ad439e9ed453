"""The fused output heads: network.up_pooling.up_pooling_conv3x3, the `heads` family of the native library (include/cspn_heads.h)
and the `fused_heads` switch of the two models.

References: golden G26 (tests/golden/make_golden_g26.py: the reference's Simple_Gudi_UpConv_Block_Last_Layer and its autograd in fp64)
and the numpy restatement of the three formulas in tests/heads_cases.py, which the CPU part holds to every golden.  Integer-valued
cases are compared bit for bit (every sum is exact in fp32 in any order); real-valued cases against the a-priori bound
n * 2^-24 * A (heads_cases.py says where it comes from), A being the golden's run on absolute values."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import heads_cases as hc
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd._host import launch
from cspn_monodepth_amd.network import unet_cspn_nyu, unet_ours
from cspn_monodepth_amd.network.up_pooling import up_pooling, up_pooling_conv3x3

DEV = "cuda:0"
INT_GOLDENS = golden_names("g26_heads_int_")
REAL_GOLDENS = golden_names("g26_heads_real_")


def unpack(z):
    oh, ow = (int(v) for v in z["geom"][:2])
    heads = tuple(int(v) for v in z["geom"][2:])
    pick = lambda stem: [z[stem + str(h)] for h in range(len(heads))]          # noqa: E731
    return oh, ow, heads, pick


def bounds(z):
    """The per-element bounds of a real-valued golden: (outputs, gx, gws)."""
    oh, ow, heads, pick = unpack(z)
    shape = z["x"].shape
    by = [hc.terms_forward(shape[1]) * hc.U * a for a in pick("ay")]
    bgx = hc.terms_grad_x(heads) * hc.U * z["agx"]
    bgw = [hc.terms_grad_w(shape) * hc.U * a for a in pick("agw")]
    return by, bgx, bgw


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_the_listed_cases():
    assert sorted(INT_GOLDENS + REAL_GOLDENS) == sorted("g26_heads_" + n for n in hc.GOLDEN_CASES)
    assert len(INT_GOLDENS) == 6 and len(REAL_GOLDENS) == 4
    for name in INT_GOLDENS + REAL_GOLDENS:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 550851


@pytest.mark.parametrize("name", INT_GOLDENS + REAL_GOLDENS)
def test_restatement_equals_the_reference(name):
    z = load_golden(name)
    oh, ow, heads, pick = unpack(z)
    shape, _, want_heads, integer = hc.GOLDEN_CASES[name[len("g26_heads_"):]]
    assert z["x"].shape == shape and heads == want_heads
    ys, gx, gws = hc.restate(z["x"], pick("w"), pick("gy"), oh, ow)
    for got, want in zip(ys + [gx] + gws, pick("y") + [z["gx"]] + pick("gw")):
        assert got.shape == want.shape
        if integer:
            assert np.array_equal(got, want.astype(np.float64))
        else:
            assert want.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", REAL_GOLDENS)
def test_bound_admits_the_references_own_fp32_run(name):
    z = load_golden(name)
    oh, ow, heads, pick = unpack(z)
    by, bgx, bgw = bounds(z)
    # the absolute run is the restatement on absolute values (so the bound is one the restatement can rebuild for other shapes)
    ays, agx, agws = hc.restate(np.abs(z["x"]), [np.abs(w) for w in pick("w")], [np.abs(g) for g in pick("gy")], oh, ow)
    for got, want in zip(ays + [agx] + agws, pick("ay") + [z["agx"]] + pick("agw")):
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    worst = 0.0
    for got, want, bound in zip(pick("y32_") + [z["gx32"]] + pick("gw32_"), pick("y") + [z["gx"]] + pick("gw"), by + [bgx] + bgw):
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all()
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print("%s: the reference's fp32 run uses %.3f of the bound" % (name, worst))
    assert 0 < worst <= 1


@pytest.mark.parametrize("net", [unet_ours, unet_cspn_nyu], ids=["unet_ours", "unet_cspn_nyu"])
def test_fused_models_keep_the_state_dict(net):
    torch.manual_seed(3)
    a = net.resnet18()
    torch.manual_seed(3)
    b = net.resnet18(fused_heads=True)
    assert not a.fused_heads and b.fused_heads
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]) for k in sa)
    b.load_state_dict(sa, strict=True)
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    with torch.device("meta"):
        big, plain = net.resnet50(fused_heads=True).state_dict(), net.resnet50().state_dict()
    assert {k: v.shape for k, v in big.items()} == {k: v.shape for k, v in plain.items()} and list(big) == list(plain)
    if net is unet_ours:
        import json
        keys = json.load(open(os.path.join(ROOT, "tests", "golden", "g17_unet_ours_state_dict_keys.json")))
        assert len(big) == 417 and {k: list(v.shape) for k, v in big.items()} == keys


def test_refusals():
    x, w1, w8 = torch.zeros(2, 3, 4, 5), torch.zeros(1, 3, 3, 3), torch.zeros(8, 3, 3, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        up_pooling_conv3x3(x, (w1, w8), 8, 10)                               # CPU tensors
    with pytest.raises(ValueError, match="fp32"):
        up_pooling_conv3x3(x.half(), (w1.half(),), 8, 10)
    with pytest.raises(ValueError, match="fp32"):
        up_pooling_conv3x3(x, (w1.double(),), 8, 10)
    for bad in (torch.zeros(1, 4, 3, 3), torch.zeros(1, 3, 5, 5), torch.zeros(1, 3, 3), torch.zeros(0, 3, 3, 3)):
        with pytest.raises(ValueError, match="weight 1 must be"):
            up_pooling_conv3x3(x, (w1, bad), 8, 10)
    with pytest.raises(ValueError, match="output channels"):
        up_pooling_conv3x3(x, (w8, w8, w1), 8, 10)                           # 17 > 16
    up16 = (w8, w8)                                                           # 16 passes the count (and is then refused as CPU)
    with pytest.raises(RuntimeError, match="ROCm device"):
        up_pooling_conv3x3(x, up16, 8, 10)
    with pytest.raises(ValueError, match="heads"):
        up_pooling_conv3x3(x, (w1,) * 5, 8, 10)
    with pytest.raises(ValueError, match="heads"):
        up_pooling_conv3x3(x, (), 8, 10)
    with pytest.raises(ValueError, match="tuple"):
        up_pooling_conv3x3(x, w1, 8, 10)
    with pytest.raises(ValueError, match=r"\[N,C,H,W\]"):
        up_pooling_conv3x3(x[0], (w1,), 8, 10)
    for oh, ow in ((0, 10), (8, 0), (9, 10), (8, 11), (-1, 4)):
        with pytest.raises(ValueError, match="must lie within"):
            up_pooling_conv3x3(x, (w1,), oh, ow)


def test_heads_family_contract():
    """Header, loader table and library agree on the family, in the terms tests/test_abi_and_host.py uses for the other nine; its
    files stay out of the digest that pins the recorded HBM traffic."""
    fam = _lib.family("heads")
    names = ("cspn_heads_abi_version", "cspn_heads_workspace_bytes", "cspn_heads_forward", "cspn_heads_backward_input",
             "cspn_heads_backward_weights")
    assert fam.header == os.path.join(ROOT, "include", "cspn_heads.h") and fam.files == {"cspn_heads.hip": False}
    text = open(fam.header).read()
    assert re.search(r"^#define CSPN_HEADS_ABI_VERSION 1$", text, flags=re.M)
    assert re.search(r"^#define CSPN_HEADS_MAX_HEADS 4$", text, flags=re.M) and _lib.HEADS_MAX_HEADS == 4
    assert re.search(r"^#define CSPN_HEADS_MAX_OUT_CHANNELS 16$", text, flags=re.M) and _lib.HEADS_MAX_OUT_CHANNELS == 16
    declared = sorted(set(re.findall(r"\b(cspn\w*)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(fam.functions) == sorted(names)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names) and lib.cspn_heads_abi_version() == fam.abi_version == 1
    assert fam in _lib.OPT_IN_FAMILIES and fam not in _lib.FAMILIES and "cspn_heads.hip" in _lib.OPT_IN_SOURCES
    assert "cspn_heads.hip" not in _lib.SOURCES and fam.header in _lib.BUILD_HEADERS and fam.header not in _lib.HEADERS
    for other in _lib.FAMILIES:
        assert not set(other.functions) & set(names) and not any("_heads_" in n for n in other.functions)
    import shutil
    import subprocess
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
        assert sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and "heads" in ln) == declared
    # workspace sizes, callable without a device: the packed filters of a forward, the partial sums of the weight gradient
    ws = lib.cspn_heads_workspace_bytes
    assert ws(_lib.HEADS_FORWARD, 9, 24, 64, 114, 152, 228, 304) == ws(_lib.HEADS_BACKWARD_INPUT, 9, 24, 64, 114, 152, 228, 304) == 9 * 64 * 9 * 4
    assert ws(_lib.HEADS_FORWARD, 9, 1, 3, 2, 2, 4, 4) == 9 * 3 * 9 * 4 and ws(_lib.HEADS_BACKWARD_INPUT, 9, 1, 3, 2, 2, 4, 4) == 9 * 32 * 9 * 4
    assert ws(_lib.HEADS_BACKWARD_WEIGHTS, 9, 1, 3, 2, 2, 4, 4) == 2 * 9 * 3 * 9 * 4            # two row segments -> two partials
    assert ws(_lib.HEADS_BACKWARD_WEIGHTS, 9, 24, 64, 114, 152, 228, 304) == 1024 * 9 * 64 * 9 * 4
    for bad in ((3, 9, 1, 3, 2, 2, 4, 4), (0, 17, 1, 3, 2, 2, 4, 4), (0, 0, 1, 3, 2, 2, 4, 4), (0, 9, 1, 3, 2, 2, 5, 4), (0, 9, 1, 3, 2, 2, 4, 0),
                (0, 9, 65536, 3, 2, 2, 4, 4)):
        assert ws(*bad) == 0
    # argument checks of the entry points come before any launch: no device needed
    one = (ctypes.c_void_p * 1)(8)
    o1 = (ctypes.c_int * 1)(1)
    assert not lib.cspn_heads_forward(8, one, one, o1, 1, 16, 1, 1, 2, 2, 5, 4, None) and b"[1, 2H]" in lib.cspn_last_error()
    assert not lib.cspn_heads_forward(8, one, one, (ctypes.c_int * 1)(17), 1, 16, 1, 1, 2, 2, 4, 4, None) and b"16" in lib.cspn_last_error()
    assert not lib.cspn_heads_forward(8, one, one, o1, 5, 16, 1, 1, 2, 2, 4, 4, None) and b"n_heads" in lib.cspn_last_error()
    assert not lib.cspn_heads_backward_weights(8, one, one, o1, 1, None, 1, 1, 2, 2, 4, 4, None) and b"null" in lib.cspn_last_error()


def test_coverage_table_reaches_what_it_names():
    """heads_cases.COVERAGE_CASES from the formulas alone: every row has the property it is named for, the library's workspace
    agrees on the cap of the weight gradient's grid, and every row keeps the precondition of a bit-for-bit comparison."""
    cases = hc.COVERAGE_CASES
    assert (hc.GW_PX, hc.GW_CB, hc.GX_CB, hc.GW_MAX_GROUPS, hc.MAX_OUT) == (64, 64, 32, 1024, 16) and hc.MAX_OUT == _lib.HEADS_MAX_OUT_CHANNELS
    group = lambda stem: {k: v for k, v in cases.items() if re.fullmatch(stem, k)}          # noqa: E731
    ot, split, chan, width, segs = group(r"ot\d+"), group(r"split_.*"), group(r"c\d+"), group(r"w\d+_(even|odd)"), group(r"segs_.*")
    assert len(ot) + len(split) + len(chan) + len(width) + len(segs) == len(cases) == 16 + 5 + 8 + 10 + 2
    # every instantiation exactly once, as one head; the split rows flatten several heads to the totals named
    assert sorted(sum(v[2]) for v in ot.values()) == list(range(1, 17)) and all(len(v[2]) == 1 and k == "ot%d" % v[2][0] for k, v in ot.items())
    assert tuple(sum(v[2]) for v in split.values()) == hc.SPLIT_TOTALS and all(len(v[2]) > 1 for v in split.values())
    assert len({v[2][0] for v in split.values()}) > 1                         # the first head's frame stride differs from row to row
    for (N, C, H, W), (oh, ow), heads in ot.values():
        Wc = (ow + 1) // 2
        assert Wc > hc.GW_PX and Wc % hc.GW_PX == 6 and ow % 2 == 1           # two width segments, 64 + 6; the scalar stores
        assert C // hc.GW_CB == 1 and C % hc.GW_CB == 1                       # two channel blocks, 64 + 1
        assert -(-C // hc.GX_CB) == 3 and C % hc.GX_CB == 1                   # three passes of gx, one channel in the last
    # the segments: two rows above the cap, with workgroups of different trip counts; every other row below it
    for name, ((N, C, H, W), (oh, ow), heads) in cases.items():
        n = hc.segments(N, oh, ow)
        assert (n == {"segs_2560": 2560, "segs_1040_w65": 1040}[name]) if name in segs else n < hc.GW_MAX_GROUPS, name
    assert 2 * hc.GW_MAX_GROUPS < 2560 < 3 * hc.GW_MAX_GROUPS                 # workgroups with 3 and with 2 trips ...
    assert hc.segments(1, *segs["segs_2560"][1]) == 512 < hc.GW_MAX_GROUPS    # ... a frame has 512: every trip lies two frames on
    assert 1040 - hc.GW_MAX_GROUPS == 16 and (segs["segs_1040_w65"][1][1] + 1) // 2 == 65     # only workgroups 0 .. 15 come back; nJ = 2
    # ragged and exact ends of the channel blocks
    assert [v[0][1] % hc.GX_CB for v in chan.values()] == [31, 0, 1, 31, 1, 1, 0, 2]
    assert [v[0][1] % hc.GW_CB for v in chan.values()] == [31, 32, 33, 63, 1, 33, 0, 2]
    assert [v[0][1] // hc.GW_CB for v in chan.values()] == [0, 0, 0, 0, 1, 1, 2, 2]
    # the last width segment: 63, 64 (exact), 1, 64 (exact, the second), 1 (the third), each with even and odd ow
    for name, ((N, C, H, W), (oh, ow), heads) in width.items():
        Wc = (ow + 1) // 2
        assert name == "w%d_%s" % (Wc, "odd" if ow % 2 else "even") and W == Wc
    assert sorted({((v[1][1] + 1) // 2) % hc.GW_PX for v in width.values()}) == [0, 1, 63]
    assert sorted({-(-((v[1][1] + 1) // 2) // hc.GW_PX) for v in width.values()}) == [1, 2, 3]
    # the library's own count of partial sums, through the entry point that needs no device
    ws = _lib.lib().cspn_heads_workspace_bytes
    for name, (shape, (oh, ow), heads) in cases.items():
        assert ws(_lib.HEADS_BACKWARD_WEIGHTS, sum(heads), *shape, oh, ow) == \
            min(hc.segments(shape[0], oh, ow), hc.GW_MAX_GROUPS) * sum(heads) * shape[1] * 9 * 4, name
    # the precondition of the bit-for-bit comparison: every sum is an integer below 2^24, and no result is identically zero
    for name, key in cases.items():
        x, ws_, gys, ys_w, gx_w, gws_w = restated(*key)
        for a in ys_w + [gx_w] + gws_w:
            assert 0 < np.abs(a).max() < 2 ** 24 and np.array_equal(a, np.rint(a)), name


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(x, ws, gys, oh, ow):
    """One forward + backward on the device: (outputs, gx, gws) as tensors."""
    xt = dev(x).requires_grad_(True)
    wts = [dev(w).requires_grad_(True) for w in ws]
    ys = up_pooling_conv3x3(xt, tuple(wts), oh, ow)
    assert isinstance(ys, tuple) and len(ys) == len(ws)
    grads = torch.autograd.grad(ys, [xt] + wts, [dev(g) for g in gys])
    return [y.detach() for y in ys], grads[0], list(grads[1:])


def same_bits(t, a):
    a = np.asarray(a)
    return t.dtype == torch.float32 and tuple(t.shape) == a.shape and np.array_equal(t.detach().cpu().numpy().view(np.uint32), a.astype(np.float32).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", INT_GOLDENS)
def test_integer_goldens_bit_equal(name):
    z = load_golden(name)
    oh, ow, heads, pick = unpack(z)
    ys, gx, gws = run(z["x"], pick("w"), pick("gy"), oh, ow)
    for got, want in zip(ys + [gx] + gws, pick("y") + [z["gx"]] + pick("gw")):
        assert same_bits(got, want + 0.0)                   # + 0.0: an exact zero sum is +0 on both sides


_RESTATED = {}


def restated(shape, out_hw, heads):
    key = (shape, out_hw, heads)
    if key not in _RESTATED:
        ins = hc.make_inputs(hc.case_seed(*key), shape, out_hw, heads, True)
        _RESTATED[key] = ins + hc.restate(*ins, *out_hw)
    return _RESTATED[key]


@pytest.mark.gpu
@pytest.mark.parametrize("heads", hc.HEAD_SETS, ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("shape,out_hw", hc.INT_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_integer_cases_bit_equal_to_the_restatement(shape, out_hw, heads):
    x, ws, gys, ys_w, gx_w, gws_w = restated(shape, out_hw, heads)
    assert max(np.abs(a).max() for a in ys_w + [gx_w] + gws_w) < 2 ** 24
    ys, gx, gws = run(x, ws, gys, *out_hw)
    for got, want in zip(ys + [gx] + gws, ys_w + [gx_w] + gws_w):
        assert same_bits(got, want + 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hc.COVERAGE_CASES))
def test_coverage_cases_bit_equal_to_the_restatement(name):
    """Every instantiation (OT = 1 .. 16), ragged channel blocks, later width segments and several trips of the weight gradient's
    segment loop (heads_cases.COVERAGE_CASES; the CPU test above holds each row to what it is named for)."""
    shape, out_hw, heads = hc.COVERAGE_CASES[name]
    x, ws, gys, ys_w, gx_w, gws_w = restated(shape, out_hw, heads)
    assert max(np.abs(a).max() for a in ys_w + [gx_w] + gws_w) < 2 ** 24
    ys, gx, gws = run(x, ws, gys, *out_hw)
    for what, got, want in zip(["y"] * len(ys) + ["gx"] + ["gw"] * len(gws), ys + [gx] + gws, ys_w + [gx_w] + gws_w):
        assert same_bits(got, want + 0.0), (name, what)
    if name.startswith("segs_"):                             # the finish adds the partial sums in a fixed order: the same bits again
        again = run(x, ws, gys, *out_hw)
        assert all(torch.equal(a, b) for a, b in zip(ys + [gx] + gws, again[0] + [again[1]] + again[2]))


@pytest.mark.gpu
def test_real_case_over_several_trips_within_the_a_priori_bound():
    """segs_2560 on real values: a workgroup of the weight gradient adds two or three segments into its accumulators, and the finish
    adds 1024 partial sums in sixteen chains of 64.  The bound is the file's own, n * 2^-24 * A with A the restatement on absolute
    values; n = N H W = 5120 for a weight gradient."""
    shape, (oh, ow), heads = hc.COVERAGE_CASES["segs_2560"]
    x, ws, gys = hc.make_inputs(81, shape, (oh, ow), heads, False)
    want = hc.restate(x, ws, gys, oh, ow)
    ays, agx, agws = hc.restate(np.abs(x), [np.abs(w) for w in ws], [np.abs(g) for g in gys], oh, ow)
    by = [hc.terms_forward(shape[1]) * hc.U * a for a in ays]
    bgx = hc.terms_grad_x(heads) * hc.U * agx
    bgw = [hc.terms_grad_w(shape) * hc.U * a for a in agws]
    assert hc.terms_grad_w(shape) == 5120 and hc.segments(shape[0], oh, ow) == 2560
    ys, gx, gws = run(x, ws, gys, oh, ow)
    ratios = []
    for what, got, w, bound in zip(["y"] * len(ys) + ["gx"] + ["gw"] * len(gws), ys + [gx] + gws, want[0] + [want[1]] + want[2], by + [bgx] + bgw):
        err = np.abs(got.cpu().numpy().astype(np.float64) - w)
        ratios.append((what, float((err[bound > 0] / bound[bound > 0]).max())))
        print("segs_2560 real %s: error / bound = %.3g" % ratios[-1])
        assert (err <= bound).all(), ratios
    assert all(r > 0 for _, r in ratios)                    # fp32 results, not a copy of the fp64 ones


def carve(buf, sizes, pad, align=4):
    """Views of `sizes` elements inside `buf`, `pad` elements apart and from both ends, each starting on a multiple of `align`
    elements (16 bytes of fp32, as an allocation does); and the mask of the elements of buf that belong to no view."""
    views, keep, at = [], torch.ones_like(buf, dtype=torch.bool), pad
    for s in sizes:
        views.append(buf[at:at + s])
        keep[at:at + s] = False
        at += -(-s // align) * align + pad
    assert at <= buf.numel()
    return views, keep


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ot7", "c65", "w65_odd", "w64_even", "segs_2560", "deep_crop"])
def test_nothing_outside_outputs_gradients_and_workspace_is_written(name):
    """The three entry points called directly: outputs, gx, every gw and the three workspaces (each exactly as long as
    cspn_heads_workspace_bytes says) are views inside one buffer of sentinels.  For the deep crop (2, 3, 6, 7) -> (4, 5), NaN in the
    compact pixels that take no part changes nothing in the outputs and the weight gradients, and the input gradient is exactly 0
    there."""
    shape, (oh, ow), heads = hc.COVERAGE_CASES[name] if name != "deep_crop" else ((2, 3, 6, 7), (4, 5), (1, 8))
    N, C, H, W = shape
    x, ws, gys, *_ = restated(shape, (oh, ow), heads)
    want = run(x, ws, gys, oh, ow)
    lib, total = _lib.lib(), sum(heads)
    work = [lib.cspn_heads_workspace_bytes(p, total, N, C, H, W, oh, ow) for p in (_lib.HEADS_FORWARD, _lib.HEADS_BACKWARD_INPUT,
                                                                                   _lib.HEADS_BACKWARD_WEIGHTS)]
    assert all(b > 0 and b % 4 == 0 for b in work)
    assert work[2] == min(hc.segments(N, oh, ow), hc.GW_MAX_GROUPS) * total * C * 9 * 4
    pad, sentinel = 4096, -12345.0
    sizes = [N * o * oh * ow for o in heads] + [N * C * H * W] + [o * C * 9 for o in heads] + [b // 4 for b in work]
    buf = torch.full((pad + sum(-(-s // 4) * 4 + pad for s in sizes),), sentinel, device=DEV)
    views, keep = carve(buf, sizes, pad)
    nh = len(heads)
    ys = [v.view(N, o, oh, ow) for v, o in zip(views[:nh], heads)]
    gx = views[nh].view(shape)
    gws = [v.view(o, C, 3, 3) for v, o in zip(views[nh + 1:2 * nh + 1], heads)]
    wf, wx, ww = views[2 * nh + 1:]
    assert all(v.data_ptr() % 16 == 0 for v in views) and ow % 2 == (name != "w64_even")      # the float2 stores at w64_even alone
    xd, wd, gd = dev(x), [dev(w) for w in ws], [dev(g) for g in gys]
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])                # noqa: E731
    oc = (ctypes.c_int * nh)(*heads)
    device = torch.device(DEV)
    launch(device, "cspn_heads_forward", xd.data_ptr(), ptrs(wd), ptrs(ys), oc, nh, wf.data_ptr(), N, C, H, W, oh, ow)
    launch(device, "cspn_heads_backward_input", ptrs(gd), ptrs(wd), oc, nh, gx.data_ptr(), wx.data_ptr(), N, C, H, W, oh, ow)
    launch(device, "cspn_heads_backward_weights", xd.data_ptr(), ptrs(gd), ptrs(gws), oc, nh, ww.data_ptr(), N, C, H, W, oh, ow)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys + [gx] + gws, want[0] + [want[1]] + want[2]))
    assert int(keep.sum()) >= pad * (len(sizes) + 1) and bool((buf[keep] == sentinel).all())
    assert not any(bool((v == sentinel).any()) for v in (wf, wx, ww))      # the packed filters and every partial sum were written
    if name != "deep_crop":
        return
    xn = x.copy()
    xn[:, :, (oh + 1) // 2:, :] = np.nan
    xn[:, :, :, (ow + 1) // 2:] = np.nan
    assert np.isnan(xn).sum() == 2 * 3 * (6 * 7 - 2 * 3)
    ys, gx, gws = run(xn, ws, gys, oh, ow)
    assert all(torch.equal(a, b) for a, b in zip(ys + [gx] + gws, want[0] + [want[1]] + want[2]))
    removed = torch.from_numpy(np.isnan(xn)).to(DEV)
    assert bool((gx[removed] == 0).all()) and bool((gx[~removed] != 0).any())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ot3", "ot16", "c65", "w65_odd", "w65_even", "segs_1040_w65"])
def test_ragged_tiles_under_poisoned_lds(name):
    """heads_gw zero-fills the ragged ends of its two LDS tiles itself: with NaN in the whole LDS of every CU in front of every
    launch, the bits of the plain run."""
    shape, out_hw, heads = hc.COVERAGE_CASES[name]
    x, ws, gys, *_ = restated(shape, out_hw, heads)
    plain = run(x, ws, gys, *out_hw)
    with lds_poison():
        ys, gx, gws = run(x, ws, gys, *out_hw)
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ys + [gx] + gws, plain[0] + [plain[1]] + plain[2]))
    assert not any(bool(torch.isnan(t).any()) for t in ys + [gx] + gws)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REAL_GOLDENS)
def test_real_goldens_within_the_a_priori_bound(name):
    z = load_golden(name)
    oh, ow, heads, pick = unpack(z)
    by, bgx, bgw = bounds(z)
    assert hc.terms_grad_w(z["x"].shape) <= 1500
    ys, gx, gws = run(z["x"], pick("w"), pick("gy"), oh, ow)
    ratios = []
    for what, got, want, bound in zip(["y"] * len(ys) + ["gx"] + ["gw"] * len(gws), ys + [gx] + gws, pick("y") + [z["gx"]] + pick("gw"),
                                      by + [bgx] + bgw):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        ratios.append((what, float((err[bound > 0] / bound[bound > 0]).max())))
        print("%s %s: error / bound = %.4f" % (name, what, ratios[-1][1]))
        assert (err <= bound).all(), ratios
    assert all(r > 0 for _, r in ratios)                    # fp32 results, not a copy of the fp64 ones


@pytest.mark.gpu
def test_batch_place_and_determinism():
    shape, (oh, ow), heads = (3, 5, 19, 37), (37, 73), (1, 8)
    x, ws, gys = hc.make_inputs(77, shape, (oh, ow), heads, False)
    ys, gx, gws = run(x, ws, gys, oh, ow)
    ys2, gx2, gws2 = run(x, ws, gys, oh, ow)
    assert all(torch.equal(a, b) for a, b in zip(ys + [gx] + gws, ys2 + [gx2] + gws2))
    for n in (0, 2):
        ys1, gx1, _ = run(x[n:n + 1], ws, [g[n:n + 1] for g in gys], oh, ow)
        assert all(torch.equal(a[0], b[n]) for a, b in zip(ys1, ys)) and torch.equal(gx1[0], gx[n])


@pytest.mark.gpu
def test_views_missing_gradients_and_no_grad():
    shape, (oh, ow) = (2, 6, 5, 7), (9, 14)
    x, ws, gys = hc.make_inputs(78, shape, (oh, ow), (1, 8), True)
    w12 = np.concatenate([ws[1], np.full((4, 6, 3, 3), 5, np.float32)])
    ys_w, gx_w, gws_w = hc.restate(x, ws, gys, oh, ow)
    # a transposed x and a slice of a wider filter bank; the slice's gradient arrives through autograd's slicing
    xt = dev(x.transpose(0, 1, 3, 2)).transpose(2, 3).requires_grad_(True)
    assert not xt.is_contiguous()
    w0, wide = dev(ws[0]).requires_grad_(True), dev(w12).requires_grad_(True)
    ys = up_pooling_conv3x3(xt, (w0, wide[:8]), oh, ow)
    g = torch.autograd.grad(ys, [xt, w0, wide], [dev(v) for v in gys])
    assert all(same_bits(a, b + 0.0) for a, b in zip(list(ys) + [g[0], g[1], g[2][:8]], ys_w + [gx_w] + gws_w))
    assert not g[2][8:].any()
    # only the second output is used: the first head's gradient counts as zero
    ys = up_pooling_conv3x3(xt, (w0, wide[:8]), oh, ow)
    g = torch.autograd.grad(ys[1], [xt, w0, wide], dev(gys[1]), allow_unused=True)
    only = hc.restate(x, ws[1:], gys[1:], oh, ow)
    assert same_bits(g[0], only[1] + 0.0) and same_bits(g[2][:8], only[2][0] + 0.0) and (g[1] is None or not g[1].any())
    # gradients only where asked for
    xn, wn = dev(x), dev(ws[0]).requires_grad_(True)
    ys = up_pooling_conv3x3(xn, (wn, dev(ws[1])), oh, ow)
    (gw0,) = torch.autograd.grad(ys, [wn], [dev(v) for v in gys])
    assert same_bits(gw0, gws_w[0] + 0.0)
    with torch.no_grad():
        ys = up_pooling_conv3x3(xt, (w0, wide[:8]), oh, ow)
    assert all(y.grad_fn is None and not y.requires_grad for y in ys) and all(same_bits(a, b + 0.0) for a, b in zip(ys, ys_w))
    with pytest.raises(ValueError):
        up_pooling_conv3x3(xt, (w0,), 11, 14)


@pytest.mark.gpu
def test_nan_reaches_only_the_windows_that_cover_it():
    """The stated difference: x[0,1,2,3] = NaN poisons the outputs whose window covers (4, 6) — rows 3..5, columns 5..7 — and nothing
    else; the two-block path (x * 0 at the inserted positions) also poisons the windows over the rest of the 2 x 2 block."""
    x, ws, _ = hc.make_inputs(79, (1, 2, 5, 6), (10, 12), (1, 8), False)
    x[0, 1, 2, 3] = np.nan
    with torch.no_grad():
        ys = up_pooling_conv3x3(dev(x), tuple(dev(w) for w in ws), 10, 12)
        u = up_pooling(dev(x), 2, 10, 12)
        stock = [torch.nn.functional.conv2d(u, dev(w), padding=1) for w in ws]
    for y, s in zip(ys, stock):
        nan = torch.isnan(y[0]).all(0).cpu().numpy()
        assert np.array_equal(np.argwhere(nan), [[r, c] for r in (3, 4, 5) for c in (5, 6, 7)]) and torch.isnan(y[0]).any(0).sum() == 9
        assert torch.isnan(s[0, :, 3:7, 5:9]).all()          # at least the windows over the whole 2 x 2 block, whatever the algorithm
        assert torch.allclose(y[~torch.isnan(s)], s[~torch.isnan(s)], rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
def test_graph_capture_gives_the_eager_bits():
    shape, (oh, ow), heads = (2, 64, 9, 11), (17, 22), (1, 8)
    x, ws, gys = hc.make_inputs(80, shape, (oh, ow), heads, False)
    eager = run(x, ws, gys, oh, ow)
    sx, sw, sg = dev(x).requires_grad_(True), [dev(w).requires_grad_(True) for w in ws], [dev(g) for g in gys]

    def step():
        ys = up_pooling_conv3x3(sx, tuple(sw), oh, ow)
        return list(ys) + list(torch.autograd.grad(ys, [sx] + sw, sg))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for t in outs:
            t.detach().fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a.detach(), b) for a, b in zip(outs, eager[0] + [eager[1]] + eager[2]))


def model_case(kind):
    torch.manual_seed(11)
    sizes = unet_ours.decoder_sizes_for(36, 52)
    if kind == "ours":
        net = unet_ours.resnet18(decoder_sizes=sizes, prop_time=2)
    else:
        net = unet_cspn_nyu.resnet18(decoder_sizes=sizes, prop_time=2, reference_state_dict=False, affinity_channels=int(kind))
    net = net.to(DEV).train()
    torch.manual_seed(12)
    inp = torch.rand(2, 4, 36, 52, device=DEV)
    return net, inp


def features_and_grads(net, inp, fused, cots=None, same_h=None):
    """features() of one model with the switch set, a linear loss on its two head outputs, and what arrived where.  same_h: the
    values gud_up_proj_layer4's output takes in this pass (the stock convolutions of the trunk do not give the same bits in every
    pass, and the comparison below is about the heads): out is replaced by same_h + (out - out.detach()) = same_h + 0, which has
    same_h's values and out's place in the autograd graph."""
    net.fused_heads = fused
    net.zero_grad(set_to_none=True)
    seen = {}

    def keep(module, args, out):
        if same_h is not None:
            seen["trunk_moved_by"] = float((out.detach() - same_h).abs().max())
            out = same_h + (out - out.detach())
        out.retain_grad()
        seen["h"] = out
        return out

    hook = net.gud_up_proj_layer4.register_forward_hook(keep)
    try:
        a, b, _ = net.features(inp)
    finally:
        hook.remove()
    if cots is None:
        torch.manual_seed(13)
        cots = (torch.randn_like(a), torch.randn_like(b))
    ((a * cots[0]).sum() + (b * cots[1]).sum()).backward()
    w5, w6 = net.gud_up_proj_layer5.conv1.weight, net.gud_up_proj_layer6.conv1.weight
    l4 = [p.grad.clone() for p in net.gud_up_proj_layer4.parameters()]
    if same_h is not None:
        print("the trunk's output moved by %.3g between the two passes (largest element %.3g)" % (seen["trunk_moved_by"], float(same_h.abs().max())))
    return dict(a=a.detach(), b=b.detach(), h=seen["h"].detach(), gh=seen["h"].grad.clone(), g5=w5.grad.clone(), g6=w6.grad.clone(),
                l4=l4, cots=cots)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "8", "12"])
def test_models_fused_against_the_two_blocks(kind):
    """Both paths are fp32 sums of the same terms, so each lies within the bound of the exact value and they lie within twice the
    bound of each other: the head outputs, the gradients of both head weights, and the gradient that arrives at gud_up_proj_layer4's
    output (whose parameters then get theirs through the same stock kernels on both sides).  The loss is linear in the head outputs,
    so both paths back-propagate the same output gradients."""
    net, inp = model_case(kind)
    stock = features_and_grads(net, inp, False)
    fused = features_and_grads(net, inp, True, stock["cots"], same_h=stock["h"])
    assert torch.equal(stock["h"], fused["h"])                       # the same decoder output went into both
    w5, w6 = net.gud_up_proj_layer5.conv1.weight.detach(), net.gud_up_proj_layer6.conv1.weight.detach()
    first, second = ("a", "b") if kind == "ours" else ("b", "a")      # unet_cspn_nyu returns (guidance, coarse, sparse)
    O6 = 8 if kind == "ours" else int(kind)
    assert fused[second].shape[1] == O6 and stock[second].shape == fused[second].shape and fused[first].shape[1] == 1
    cot5, cot6 = (stock["cots"][0], stock["cots"][1]) if kind == "ours" else (stock["cots"][1], stock["cots"][0])
    h = stock["h"].cpu().numpy()
    ws = [w5.cpu().numpy(), w6[:O6].cpu().numpy()]
    gys = [cot5.cpu().numpy(), cot6.cpu().numpy()]
    oh, ow = 36, 52
    ays, agx, agws = hc.restate(np.abs(h), [np.abs(w) for w in ws], [np.abs(g) for g in gys], oh, ow)
    assert hc.terms_grad_w(h.shape) <= 1500

    def close(got, want, terms, A, what):
        bound = 2 * terms * hc.U * A
        err = np.abs(got.cpu().numpy().astype(np.float64) - want.cpu().numpy().astype(np.float64))
        print("%s %s: difference / (2 x bound) = %.4f" % (kind, what, float((err[bound > 0] / bound[bound > 0]).max())))
        assert (err <= bound).all(), what

    close(fused[first], stock[first], hc.terms_forward(h.shape[1]), ays[0], "coarse depth")
    close(fused[second], stock[second], hc.terms_forward(h.shape[1]), ays[1], "guidance")
    close(fused["gh"], stock["gh"], hc.terms_grad_x((1, O6)), agx, "gradient at gud_up_proj_layer4's output")
    close(fused["g5"], stock["g5"], hc.terms_grad_w(h.shape), agws[0], "layer5 weight gradient")
    close(fused["g6"][:O6], stock["g6"][:O6], hc.terms_grad_w(h.shape), agws[1], "layer6 weight gradient")
    assert not fused["g6"][O6:].any() and not stock["g6"][O6:].any()
    assert len(fused["l4"]) == len(stock["l4"]) > 0
    # gud_up_proj_layer4's parameters get their gradients from that one through the block's own stock kernels.  Those do not give the
    # same bits in two passes over the same input (the trunk's output moves in its 6th digit, printed above, and a ReLU input that
    # changes sign hands a whole term to a weight's gradient or takes it away), so no bound of the kind above exists for them: they
    # must be there, finite and not zero, and the difference is printed.
    for a, b in zip(fused["l4"], stock["l4"]):
        assert a.shape == b.shape and torch.isfinite(a).all() and a.abs().max() > 0 and b.abs().max() > 0
    print("%s gud_up_proj_layer4 parameter gradients: largest difference %.3g of the largest element"
          % (kind, max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(fused["l4"], stock["l4"]))))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "8"])
def test_default_models_still_run_the_two_blocks(kind):
    net, inp = model_case(kind)
    assert net.fused_heads is False
    seen = {}
    hook = net.gud_up_proj_layer4.register_forward_hook(lambda m, i, o: seen.update(h=o))
    with torch.no_grad():
        a, b, _ = net.features(inp)
        hook.remove()
        l5, l6 = net.gud_up_proj_layer5, net.gud_up_proj_layer6
        if kind == "ours":
            assert torch.equal(a, l5(seen["h"])) and torch.equal(b, l6(seen["h"]))
        else:
            assert torch.equal(b, l5(seen["h"])) and torch.equal(a, l6(seen["h"], 8))

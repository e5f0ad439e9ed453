"""The fused decoder-block head: network.up_pooling.up_pooling_conv5x5 / pack_upconv5x5, the `upconv` family of the native library
(include/cspn_upconv.h) and the `fused_decoder` switch of the two models.

References: golden G27 (tests/golden/make_golden_g27.py: the reference's blocks in fp64, eval mode) and the numpy restatement of the
four-phase formula in tests/upconv_cases.py, which the CPU part holds to every golden and to the dense un-pool + convolution.
Integer-valued cases are compared bit for bit (every sum is exact in fp32 in any order); real-valued cases against the a-priori
bound gamma_n (|scale| sum |w x| + |shift|), n = taps C + 3 (upconv_cases.py says where it comes from)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import upconv_cases as uc
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd._host import launch
from cspn_monodepth_amd.network import unet_cspn_nyu, unet_ours
from cspn_monodepth_amd.network import up_pooling as upmod
from cspn_monodepth_amd.network.up_pooling import UpconvPack, pack_upconv5x5, up_pooling, up_pooling_conv5x5

DEV = "cuda:0"
INT_GOLDENS = golden_names("g27_upconv_int_")
REAL_GOLDENS = golden_names("g27_upconv_real_")
BLOCKS = upmod.DECODER_BLOCKS


def unpack(z):
    oh, ow, O, nf = (int(v) for v in z["geom"])
    ws, bns = [z["w%d" % k] for k in range(nf)], [z["bn%d" % k] for k in range(nf)]
    folded = [uc.fold(*p, float(z["eps"])) for p in bns]
    scale, shift = np.concatenate([f[0] for f in folded]), np.concatenate([f[1] for f in folded])
    return oh, ow, O, ws, bns, scale, shift, [z["y%d" % k] for k in range(nf)]


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_the_listed_cases():
    assert sorted(INT_GOLDENS + REAL_GOLDENS) == sorted("g27_upconv_" + n for n in uc.GOLDEN_CASES)
    shapes = {(v[1], v[2]) for v in uc.GOLDEN_CASES.values()}
    assert ((2, 3, 6, 7), (4, 5)) in shapes and ((1, 3, 8, 10), (15, 19)) in shapes            # the deep crop, the odd crop at C = 3
    assert {v[0] for v in uc.GOLDEN_CASES.values()} == {"Gudi_UpProj_Block", "Gudi_UpProj_Block_Cat", "Simple_Gudi_UpConv_Block"}
    for name in INT_GOLDENS + REAL_GOLDENS:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 131072


@pytest.mark.parametrize("name", INT_GOLDENS + REAL_GOLDENS)
def test_restatement_equals_the_reference(name):
    z = load_golden(name)
    oh, ow, O, ws, bns, scale, shift, want = unpack(z)
    kind, shape, out_hw, O_w, integer = uc.GOLDEN_CASES[name[len("g27_upconv_"):]]
    assert z["x"].shape == shape and (oh, ow) == out_hw and O == O_w and len(ws) == (1 if kind.startswith("Simple") else 2)
    assert all((p[2] != 0).any() and (p[3] != 1).any() and (p[0] != 1).any() for p in bns if O > 1)      # non-trivial statistics
    got = uc.restate(z["x"], ws, oh, ow, scale, shift, O)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape == (shape[0], O, oh, ow)
        if integer:
            assert w.dtype == np.float32 and np.array_equal(g, w.astype(np.float64))
        else:
            assert w.dtype == np.float64 and np.abs(g - w).max() <= 1e-12


@pytest.mark.parametrize("hw,out_hw", uc.GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_equals_the_dense_form(hw, out_hw):
    """Independent of the goldens: zero-insert, crop, and run the stock 5x5 convolution in fp64 on the CPU."""
    shape, filters = (2, 3) + hw, (3, 2)
    x, ws, scale, shift = uc.make_inputs(5, shape, filters, True)
    u = torch.zeros(2, 3, 2 * hw[0], 2 * hw[1], dtype=torch.float64)
    u[:, :, ::2, ::2] = torch.from_numpy(x).double()
    u = u[:, :, :out_hw[0], :out_hw[1]]
    for relu in (0, 3, 5):
        got = uc.restate(x, ws, *out_hw, scale, shift, relu)
        dense = torch.cat([torch.nn.functional.conv2d(u, torch.from_numpy(w).double(), padding=2) for w in ws], 1).numpy()
        dense = dense * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None]
        dense[:, :relu] = np.maximum(dense[:, :relu], 0)
        assert np.array_equal(np.concatenate(got, 1) + 0.0, dense + 0.0)


def test_m_tile_table_reaches_what_it_names():
    """upconv_cases.M_TILE_FILTER_SETS from the sizes alone, and the exactness precondition of every case of the three precisions'
    test_integer_cases_over_several_m_tiles (fp32 sums below 2^24; results inside the fp16 range for the half family)."""
    tiles = [-(-sum(f) // 128) for f in uc.M_TILE_FILTER_SETS]
    assert tiles == [2, 2, 3, 2] and all(sum(f) > max(sum(g) for g in uc.FILTER_SETS + (uc.BIG["filters"],)) for f in uc.M_TILE_FILTER_SETS)
    (a, _), (b, c), (d, e), (f, g) = uc.M_TILE_FILTER_SETS
    assert a - 128 == 1                                                      # one live row in tile 1
    assert 128 < b < b + c < 256                                             # the filter and ReLU boundary, and the end, inside tile 1
    assert d == 128 and 256 < d + e                                          # the boundary on the tile edge, a third tile
    assert f < 128 < f + g                                                   # the boundary in tile 0, live rows in tile 1
    cases = list(uc.m_tile_shapes())
    assert len(cases) == 16 and uc.M_TILE_POISON_CASE in cases and {s[1] for s, _, _ in cases} == {3, 33}
    for shape, out_hw, filters in cases:
        x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters), shape, filters, True)
        acc = uc.accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], *out_hw)
        assert 0 < 4 * acc.max() + 5 < 65504 < 2 ** 24
        assert all(np.array_equal(t.astype(np.float16).astype(np.float32), t) for t in [x] + ws)


def test_refusals():
    x, w3, w2 = torch.zeros(2, 3, 4, 5), torch.zeros(3, 3, 5, 5), torch.zeros(2, 3, 5, 5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        up_pooling_conv5x5(x, (w3, w2), 8, 10)                               # CPU tensors: everything else was in order
    with pytest.raises(ValueError, match="fp32"):
        up_pooling_conv5x5(x.half(), (w3,), 8, 10)
    with pytest.raises(ValueError, match="fp32"):
        up_pooling_conv5x5(x, (w3.double(),), 8, 10)
    with pytest.raises(ValueError, match="fp32"):
        pack_upconv5x5((w3.half(),))
    for bad in (torch.zeros(1, 4, 5, 5), torch.zeros(1, 3, 3, 3), torch.zeros(1, 3, 5, 3), torch.zeros(1, 3, 5), torch.zeros(0, 3, 5, 5)):
        with pytest.raises(ValueError, match="filter 1 must be"):
            up_pooling_conv5x5(x, (w3, bad), 8, 10)
        with pytest.raises(ValueError, match="filter 1 must be"):
            pack_upconv5x5((w3, bad))
    with pytest.raises(ValueError, match="one or two filters"):
        up_pooling_conv5x5(x, (w3, w2, w2), 8, 10)
    with pytest.raises(ValueError, match="one or two filters"):
        pack_upconv5x5(())
    with pytest.raises(ValueError, match="tuple"):
        up_pooling_conv5x5(x, w3, 8, 10)
    with pytest.raises(ValueError, match=r"\[N,C,H,W\]"):
        up_pooling_conv5x5(x[0], (w3,), 8, 10)
    with pytest.raises(ValueError, match="channels"):
        up_pooling_conv5x5(torch.zeros(2, 4, 4, 5), (w3,), 8, 10)
    for oh, ow in ((0, 10), (8, 0), (9, 10), (8, 11), (-1, 4)):
        with pytest.raises(ValueError, match="must lie within"):
            up_pooling_conv5x5(x, (w3,), oh, ow)
    with pytest.raises(ValueError, match="together"):
        up_pooling_conv5x5(x, (w3,), 8, 10, scale=torch.ones(3))
    with pytest.raises(ValueError, match=r"scale must be fp32 \[5\]"):
        up_pooling_conv5x5(x, (w3, w2), 8, 10, scale=torch.ones(3), shift=torch.ones(5))
    for relu in (-1, 6):
        with pytest.raises(ValueError, match="relu_channels"):
            up_pooling_conv5x5(x, (w3, w2), 8, 10, relu_channels=relu)
    with pytest.raises(ValueError, match="ReLU come first"):
        pack_upconv5x5((w3, w2), relu=(False, True))
    with pytest.raises(ValueError, match="batch norm over 2 channels"):
        pack_upconv5x5((w3, w2), (torch.nn.BatchNorm2d(3), torch.nn.BatchNorm2d(3)))
    with pytest.raises(ValueError, match="2\\^31"):                          # sizes only: no memory behind a meta tensor
        up_pooling_conv5x5(torch.zeros(2 ** 16, 1, 2 ** 8, 2 ** 7, device="meta"), (torch.zeros(1, 1, 5, 5),), 1, 1)
    with pytest.raises(ValueError, match="2\\^31"):
        up_pooling_conv5x5(torch.zeros(2 ** 10, 1, 2 ** 10, 2 ** 9, device="meta"), (torch.zeros(1, 1, 5, 5),), 2 ** 11, 2 ** 10)
    pack = UpconvPack(None, None, None, (3,), 3, 3, (w3,))
    with pytest.raises(ValueError, match="come with the pack"):
        up_pooling_conv5x5(x, pack, 8, 10, relu_channels=1)


def test_grad_mode_refusal_names_the_training_path():
    x, w = torch.zeros(1, 3, 2, 2), torch.zeros(2, 3, 5, 5)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="stock blocks.*training path"):
            up_pooling_conv5x5(x.clone().requires_grad_(True), (w,), 4, 4)
        with pytest.raises(RuntimeError, match="stock blocks.*training path"):
            up_pooling_conv5x5(x, (torch.nn.Parameter(w),), 4, 4)
        pack = UpconvPack(None, None, None, (2,), 3, 2, (torch.nn.Parameter(w),))
        with pytest.raises(RuntimeError, match="forward-only"):
            up_pooling_conv5x5(x, pack, 4, 4)
    with torch.no_grad():                                                     # grad mode off: past that check, refused as CPU tensors
        with pytest.raises(RuntimeError, match="ROCm device"):
            up_pooling_conv5x5(x.clone().requires_grad_(True), (torch.nn.Parameter(w),), 4, 4)


def test_pack_stale_logic():
    w, g, m = torch.zeros(2, 3, 5, 5), torch.ones(2), torch.zeros(2)
    pack = UpconvPack(None, None, None, (2,), 3, 2, (w, g, m))
    assert not pack.stale() and pack.made_from([w, g, m]) and not pack.made_from([w, g]) and not pack.made_from([w, g, m.clone()])
    m.add_(1)                                                                 # an in-place update moves _version
    assert pack.stale()
    pack = UpconvPack(None, None, None, (2,), 3, 2, (w, g, m))
    assert not pack.stale()
    lin = torch.nn.Conv2d(3, 2, 5, bias=False)
    pack = UpconvPack(None, None, None, (2,), 3, 2, (lin.weight,))
    lin.load_state_dict({"weight": torch.ones(2, 3, 5, 5)})                   # copies in place
    assert pack.stale() and pack.made_from([lin.weight])
    pack = UpconvPack(None, None, None, (2,), 3, 2, (lin.weight,))
    lin.weight.data = torch.ones(2, 3, 5, 5)                                  # another storage behind the same parameter
    assert pack.stale()
    assert (pack.out_channels, pack.in_channels, pack.relu_channels) == ((2,), 3, 2)


@pytest.mark.parametrize("net", [unet_ours, unet_cspn_nyu], ids=["unet_ours", "unet_cspn_nyu"])
def test_switch_keeps_modules_and_state_dict(net):
    torch.manual_seed(3)
    a = net.resnet18()
    torch.manual_seed(3)
    b = net.resnet18(fused_decoder=BLOCKS, fused_heads=True)
    assert a.fused_decoder == () and b.fused_decoder == BLOCKS and not a.fused_heads and b.fused_heads
    assert all(getattr(b, n).fused_head and not getattr(a, n).fused_head for n in BLOCKS)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    c = net.resnet18(fused_decoder=["gud_up_proj_layer3", "gud_up_proj_layer1"])
    assert c.fused_decoder == ("gud_up_proj_layer1", "gud_up_proj_layer3") and not c.gud_up_proj_layer2.fused_head and not c.fused_heads
    assert net.resnet18(fused_decoder="gud_up_proj_layer4").fused_decoder == ("gud_up_proj_layer4",)
    assert net.resnet18(fused_decoder=True).fused_decoder == tuple(n for n in BLOCKS if n in upmod.FUSED_DECODER_DEFAULT)
    assert set(upmod.FUSED_DECODER_DEFAULT) <= set(BLOCKS)
    with pytest.raises(ValueError, match="gud_up_proj_layer5"):
        net.resnet18(fused_decoder=["gud_up_proj_layer5"])
    with torch.device("meta"):
        big, plain = net.resnet50(fused_decoder=BLOCKS).state_dict(), net.resnet50().state_dict()
    assert {k: v.shape for k, v in big.items()} == {k: v.shape for k, v in plain.items()} and list(big) == list(plain)
    if net is unet_ours:
        assert len(big) == 417


def test_upconv_family_contract(monkeypatch):
    """Header, loader table and library agree on the family, in the terms tests/test_heads.py uses for `heads`; its files stay out of
    the digest that pins the recorded HBM traffic."""
    fam = _lib.family("upconv")
    names = ("cspn_upconv_abi_version", "cspn_upconv_workspace_bytes", "cspn_upconv_pack", "cspn_upconv_forward")
    assert fam.header == os.path.join(ROOT, "include", "cspn_upconv.h") and fam.files == {"cspn_upconv.hip": False, "cspn_upconv_core.hpp": False}
    text = open(fam.header).read()
    assert re.search(r"^#define CSPN_UPCONV_ABI_VERSION 1$", text, flags=re.M)
    assert re.search(r"^#define CSPN_UPCONV_MAX_FILTERS 2$", text, flags=re.M) and _lib.UPCONV_MAX_FILTERS == 2
    declared = sorted(set(re.findall(r"\b(cspn\w*)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(fam.functions) == sorted(names)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names) and lib.cspn_upconv_abi_version() == fam.abi_version == 1
    assert _lib.OPT_IN_FAMILIES[:2] == (_lib.family("heads"), fam) and fam not in _lib.FAMILIES and len(_lib.ALL_FAMILIES) == 13
    assert "cspn_upconv.hip" in _lib.OPT_IN_SOURCES and "cspn_upconv.hip" not in _lib.SOURCES
    assert fam.header in _lib.BUILD_HEADERS and fam.header not in _lib.HEADERS
    # the core both decoder-head families are built on is a header of an opt-in family: seen by the build's staleness hash (and so by
    # the per-object one, which reads the same list), never by the digest behind profiles/
    core = os.path.join(_lib.CSRC, "cspn_upconv_core.hpp")
    assert core in _lib.BUILD_HEADERS and core not in _lib.HEADERS
    with_core = _lib._source_digest(["x"])
    monkeypatch.setattr(_lib, "BUILD_HEADERS", tuple(p for p in _lib.BUILD_HEADERS if p != core))
    assert _lib._source_digest(["x"]) != with_core
    monkeypatch.undo()
    assert _lib._source_digest(["x"]) == with_core
    for other in _lib.ALL_FAMILIES:
        if other is not fam:
            assert not set(other.functions) & set(names) and not any("upconv" in n for n in other.functions)
    assert not any("heads" in n for n in names)
    import shutil
    import subprocess
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
        assert sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and "upconv" in ln) == declared
    # the packed filters, callable without a device: 25 taps x C rounded up to 32 x the flat channels rounded up to 128, fp32
    ws = lib.cspn_upconv_workspace_bytes
    assert ws(2048, 2048) == 25 * 2048 * 2048 * 4 == 419430400 and ws(6, 3) == 25 * 32 * 128 * 4 and ws(129, 67) == 25 * 96 * 256 * 4
    for bad in ((0, 3), (3, 0), (-1, 3), (32768, 4096), (2 ** 30, 2 ** 30)):            # the last two: 2^31 packed elements or more
        assert ws(*bad) == 0
    # argument checks of the entry points come before any launch: no device needed
    one, two, three = (ctypes.c_void_p * 1)(16), (ctypes.c_void_p * 2)(16, 16), (ctypes.c_void_p * 3)(16, 16, 16)
    o1, o3 = (ctypes.c_int * 1)(1), (ctypes.c_int * 3)(1, 1, 1)
    F32, F16 = _lib.CSPN_F32, _lib.CSPN_F16
    err = lib.cspn_last_error
    assert not lib.cspn_upconv_pack(one, o1, 1, 3, 5, 5, F16, 16, None) and b"fp32" in err()
    assert not lib.cspn_upconv_pack(one, o1, 1, 3, 3, 3, F32, 16, None) and b"5x5" in err()
    assert not lib.cspn_upconv_pack(one, o1, 1, 3, 5, 3, F32, 16, None) and b"5x5" in err()
    assert not lib.cspn_upconv_pack(three, o3, 3, 3, 5, 5, F32, 16, None) and b"between 1 and 2 filters" in err()
    assert not lib.cspn_upconv_pack(one, o1, 1, 3, 5, 5, F32, None, None) and b"null" in err()
    assert not lib.cspn_upconv_pack(one, (ctypes.c_int * 1)(0), 1, 3, 5, 5, F32, 16, None) and b"output channels" in err()
    fwd = lib.cspn_upconv_forward
    assert not fwd(16, F16, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"fp32" in err()
    for oh, ow in ((5, 4), (4, 5), (0, 4), (4, 0)):
        assert not fwd(16, F32, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, oh, ow, None) and b"[1, 2H]" in err()
    assert not fwd(16, F32, 16, None, None, 0, three, o3, 3, 1, 1, 2, 2, 4, 4, None) and b"between 1 and 2 filters" in err()
    assert not fwd(16, F32, 16, None, None, 0, one, o1, 1, 2 ** 16, 1, 2 ** 8, 2 ** 7, 1, 1, None) and b"2^31" in err()      # x
    assert not fwd(16, F32, 16, None, None, 0, one, o1, 1, 2 ** 10, 1, 2 ** 10, 2 ** 9, 2 ** 11, 2 ** 10, None) and b"2^31" in err()      # an output
    assert not fwd(16, F32, 16, 16, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"together" in err()
    assert not fwd(16, F32, 16, None, None, 2, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"relu_channels" in err()
    assert not fwd(16, F32, 16, None, None, 0, two, (ctypes.c_int * 2)(1, 0), 2, 1, 1, 2, 2, 4, 4, None) and b"output channels" in err()
    assert not fwd(None, F32, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"null" in err()


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(x, ws, oh, ow, scale=None, shift=None, relu=0):
    with torch.no_grad():
        outs = up_pooling_conv5x5(dev(x), tuple(dev(w) for w in ws), oh, ow, None if scale is None else dev(scale),
                                  None if shift is None else dev(shift), relu)
    assert isinstance(outs, tuple) and len(outs) == len(ws)
    assert all(o.is_contiguous() and tuple(o.shape) == (x.shape[0], w.shape[0], oh, ow) for o, w in zip(outs, ws))
    return outs


def same_bits(t, a):
    a = np.asarray(a)
    return t.dtype == torch.float32 and tuple(t.shape) == a.shape and np.array_equal(t.detach().cpu().numpy().view(np.uint32), a.astype(np.float32).view(np.uint32))


def relu_boundaries(filters):
    return sorted({0, filters[0], sum(filters)})


def integer_case(shape, out_hw, filters):
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters), shape, filters, True)
    acc = uc.accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], *out_hw)
    assert 4 * acc.max() + 5 < 2 ** 24                                      # every partial sum, and the affine map of it, is exact
    for relu in relu_boundaries(filters):
        want = uc.restate(x, ws, *out_hw, scale, shift, relu)
        got = run(x, ws, *out_hw, scale, shift, relu)
        for g, w in zip(got, want):
            assert same_bits(g, w + 0.0), (shape, out_hw, filters, relu)     # + 0.0: an exact zero is +0 on both sides
    plain = run(x, ws, *out_hw)                                              # no affine map at all
    for g, w in zip(plain, uc.restate(x, ws, *out_hw)):
        assert same_bits(g, w + 0.0), (shape, out_hw, filters, "plain")


@pytest.mark.gpu
@pytest.mark.parametrize("hw,out_hw", uc.GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_integer_cases_bit_equal_to_the_restatement(hw, out_hw):
    for C, both, B in itertools.product(uc.CHANNELS, uc.FILTER_SETS, uc.BATCHES):
        integer_case((B, C) + hw, out_hw, uc.filters_of(both))


@pytest.mark.gpu
def test_integer_case_over_several_chunks_and_tiles():
    shape, out_hw, filters = uc.BIG["shape"], uc.BIG["out_hw"], uc.BIG["filters"]
    assert shape[1] > 32 and all(shape[0] * ((out_hw[0] + 1 - a) // 2) * ((out_hw[1] + 1 - b) // 2) > 128 for a, b in uc.PHASES)
    integer_case(shape, out_hw, filters)


@pytest.mark.gpu
def test_integer_cases_over_several_m_tiles():
    """mt > 0 in fwd<F32>: the filter tile's offset, the tap stride with Mp > 128, the m >= M cut, the y0 / y1 switch and the ReLU
    boundary in a tile that is not the first (upconv_cases.M_TILE_FILTER_SETS says what each row is there for)."""
    for shape, out_hw, filters in uc.m_tile_shapes():
        integer_case(shape, out_hw, filters)


@pytest.mark.gpu
def test_ragged_m_tile_under_poisoned_lds():
    shape, out_hw, filters = uc.M_TILE_POISON_CASE
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters), shape, filters, True)
    plain = run(x, ws, *out_hw, scale, shift, filters[0])
    with lds_poison():
        got = run(x, ws, *out_hw, scale, shift, filters[0])
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, plain)) and not any(bool(torch.isnan(g).any()) for g in got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", INT_GOLDENS)
def test_integer_goldens_bit_equal(name):
    z = load_golden(name)
    oh, ow, O, ws, bns, scale, shift, want = unpack(z)
    got = run(z["x"], ws, oh, ow, scale.astype(np.float32), shift.astype(np.float32), O)
    assert np.array_equal(scale, scale.astype(np.float32)) and np.array_equal(shift, shift.astype(np.float32))
    for g, w in zip(got, want):
        assert same_bits(g, w + 0.0)


def check_within_bound(what, got, x, ws, oh, ow, scale, shift, relu, want=None, extra=0):
    """got (device tensors, one per filter) against the fp64 restatement (or `want`) under the a-priori bound; the largest ratio."""
    if want is None:
        want = uc.restate(x, ws, oh, ow, scale, shift, relu)
    bound = uc.bound(x, ws, oh, ow, scale, shift, extra)
    err = np.abs(np.concatenate([g.cpu().numpy().astype(np.float64) for g in got], 1) - np.concatenate(want, 1))
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print("%s: largest error / bound = %.4f" % (what, ratio))
    assert (err <= bound).all(), (what, ratio)
    assert err.max() > 0                                                     # fp32 results, not a copy of the fp64 ones
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out_hw,both", uc.REAL_CASES, ids=lambda v: "x".join(map(str, v)))
def test_real_cases_within_the_a_priori_bound(shape, out_hw, both):
    filters = uc.filters_of(both)
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters) + 1, shape, filters, False)
    for relu in relu_boundaries(filters):
        got = run(x, ws, *out_hw, scale, shift, relu)
        check_within_bound("%s relu %d" % (shape, relu), got, x, ws, *out_hw, scale, shift, relu)
    check_within_bound("%s plain" % (shape,), run(x, ws, *out_hw), x, ws, *out_hw, None, None, 0)


def golden_block(z):
    """The golden's filters and batch norms as device modules in eval mode."""
    oh, ow, O, ws, bns, scale, shift, want = unpack(z)
    mods = []
    for p in bns:
        bn = torch.nn.BatchNorm2d(O, eps=float(z["eps"])).to(DEV).eval()
        with torch.no_grad():
            for t, v in zip((bn.weight, bn.bias, bn.running_mean, bn.running_var), p):
                t.copy_(dev(v))
        mods.append(bn)
    return [torch.nn.Parameter(dev(w)) for w in ws], mods


@pytest.mark.gpu
@pytest.mark.parametrize("name", REAL_GOLDENS + INT_GOLDENS[:2])
def test_batch_norm_fold_against_the_golden(name):
    z = load_golden(name)
    oh, ow, O, ws, bns, scale, shift, want = unpack(z)
    weights, mods = golden_block(z)
    pack = pack_upconv5x5(weights, mods, (True, False)[:len(ws)])
    assert pack.relu_channels == O and pack.out_channels == (O,) * len(ws) and not pack.stale()
    assert pack.scale.dtype == torch.float32 and tuple(pack.scale.shape) == tuple(pack.shift.shape) == (O * len(ws),)
    with torch.no_grad():
        got = up_pooling_conv5x5(dev(z["x"]), pack, oh, ow)
    if name in INT_GOLDENS:                                                  # the fold itself is exact there
        assert all(same_bits(g, w + 0.0) for g, w in zip(got, want))
        return
    check_within_bound(name, got, z["x"], ws, oh, ow, scale, shift, O, want=[w.astype(np.float64) for w in want], extra=4)
    # ... and the stock ops on the device agree with the same golden (what the fused head replaces)
    with torch.no_grad():
        u = up_pooling(dev(z["x"]), 2, oh, ow)
        stock = [torch.relu(mods[0](torch.nn.functional.conv2d(u, weights[0], padding=2)))]
        if len(ws) > 1:
            stock.append(mods[1](torch.nn.functional.conv2d(u, weights[1], padding=2)))
    for s, w in zip(stock, want):
        assert np.abs(s.cpu().numpy() - w).max() <= 1e-4 * max(1.0, np.abs(w).max())
    # an in-place update of a running statistic makes the pack stale
    with torch.no_grad():
        mods[0].running_mean.add_(1.0)
    assert pack.stale()


@pytest.mark.gpu
def test_batch_place_and_determinism():
    shape, out_hw, filters = (3,) + uc.BIG["shape"][1:], uc.BIG["out_hw"], uc.BIG["filters"]
    x, ws, scale, shift = uc.make_inputs(91, shape, filters, False)
    ys = run(x, ws, *out_hw, scale, shift, filters[0])
    again = run(x, ws, *out_hw, scale, shift, filters[0])
    assert all(torch.equal(a, b) for a, b in zip(ys, again))                  # two runs of one call
    for n in (0, 2):                                                         # frame n of B = 3 at position 0 of B = 1
        alone = run(x[n:n + 1], ws, *out_hw, scale, shift, filters[0])
        assert all(torch.equal(a[0], b[n]) for a, b in zip(alone, ys))
    pair = run(x[1:3], ws, *out_hw, scale, shift, filters[0])                # ... and at position 1 of B = 2: other tiles again
    assert all(torch.equal(a[1], b[2]) for a, b in zip(pair, ys))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out_hw,filters", [((2, 5, 5, 7), (9, 13), (17, 16)), ((1, 3, 6, 7), (4, 5), (33,)),
                                                   ((3, 3, 1, 2), (2, 3), (3, 3))], ids=["odd", "deep_crop", "tiny"])
def test_nothing_outside_the_outputs_is_written(shape, out_hw, filters):
    x, ws, scale, shift = uc.make_inputs(92, shape, filters, True)
    want = run(x, ws, *out_hw, scale, shift, filters[0])
    pack = pack_upconv5x5(tuple(dev(w) for w in ws), None, (False,) * len(ws))
    pad, sentinel = 4096, -12345.0
    sizes = [shape[0] * o * out_hw[0] * out_hw[1] for o in filters]
    buf = torch.full((pad + sum(s + pad for s in sizes),), sentinel, device=DEV)
    outs, at = [], pad
    for s, o in zip(sizes, filters):
        outs.append(buf[at:at + s].view(shape[0], o, *out_hw))
        at += s + pad
    xd, sd, hd = dev(x), dev(scale), dev(shift)
    ptrs = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    launch(torch.device(DEV), "cspn_upconv_forward", xd.data_ptr(), _lib.CSPN_F32, pack.packed.data_ptr(), sd.data_ptr(), hd.data_ptr(),
           filters[0], ptrs, (ctypes.c_int * len(outs))(*filters), len(outs), *shape, *out_hw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want))
    keep = torch.ones_like(buf, dtype=torch.bool)
    at = pad
    for s in sizes:
        keep[at:at + s] = False
        at += s + pad
    assert int(keep.sum()) == pad * (len(sizes) + 1) and bool((buf[keep] == sentinel).all())
    # the compact pixels the crop removed are not read either: NaN there changes nothing
    if out_hw[0] < 2 * shape[2] - 1:
        xn = x.copy()
        xn[:, :, (out_hw[0] + 1) // 2:, :] = np.nan
        xn[:, :, :, (out_hw[1] + 1) // 2:] = np.nan
        assert all(torch.equal(a, b) for a, b in zip(run(xn, ws, *out_hw, scale, shift, filters[0]), want))


@pytest.mark.gpu
def test_nan_reaches_only_the_windows_that_cover_it():
    """The stated difference: x[0,1,2,3] = NaN poisons the outputs whose 5x5 window covers (4, 6) — rows 2..6, columns 4..8 — and
    nothing else.  The reference's un-pooling holds x * 0 at the inserted positions, so the stock path also poisons the rest of
    the windows over the 2 x 2 block (rows 2..7, columns 4..9)."""
    x, ws, scale, shift = uc.make_inputs(93, (1, 2, 5, 6), (3, 2), False)
    x[0, 1, 2, 3] = np.nan
    ys = run(x, ws, 10, 12, scale, shift, 3)
    with torch.no_grad():
        u = up_pooling(dev(x), 2, 10, 12)
        stock = [torch.nn.functional.conv2d(u, dev(w), padding=2) for w in ws]
        stock = torch.cat(stock, 1) * dev(scale)[None, :, None, None] + dev(shift)[None, :, None, None]
        stock[:, :3] = torch.relu(stock[:, :3])
    y = torch.cat(ys, 1)
    nan = torch.isnan(y[0])
    assert np.array_equal(np.argwhere(nan.all(0).cpu().numpy()), [[r, c] for r in range(2, 7) for c in range(4, 9)])
    assert int(nan.any(0).sum()) == 25
    assert bool(torch.isnan(stock[0, :, 2:8, 4:10]).all())
    ok = ~torch.isnan(stock)
    assert torch.allclose(y[ok], stock[ok], rtol=1e-4, atol=1e-4)


@pytest.mark.gpu
def test_graph_capture_gives_the_eager_bits():
    shape, out_hw, filters = uc.BIG["shape"], uc.BIG["out_hw"], uc.BIG["filters"]
    x, ws, scale, shift = uc.make_inputs(94, shape, filters, False)
    x2 = uc.make_inputs(95, shape, filters, False)[0]
    weights = [torch.nn.Parameter(dev(w)) for w in ws]
    mods = [torch.nn.BatchNorm2d(o).to(DEV).eval() for o in filters]
    with torch.no_grad():
        for k, bn in enumerate(mods):
            bn.running_mean.copy_(dev(shift[k * 40:(k + 1) * 40]))
            bn.weight.copy_(dev(scale[k * 40:(k + 1) * 40]))
        pack = pack_upconv5x5(weights, mods)
        eager = [up_pooling_conv5x5(dev(v), pack, *out_hw) for v in (x, x2)]
        sx = dev(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            up_pooling_conv5x5(sx, pack, *out_hw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = up_pooling_conv5x5(sx, pack, *out_hw)
        for v, want in ((x2, eager[1]), (x, eager[0]), (x2, eager[1])):      # replays on new input values
            sx.copy_(dev(v))
            for t in outs:
                t.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, want))
    assert not torch.equal(eager[0][0], eager[1][0])


def model_case(kind, fused=BLOCKS, seed=11):
    torch.manual_seed(seed)
    sizes = unet_ours.decoder_sizes_for(36, 52)
    if kind == "ours":
        net = unet_ours.resnet18(decoder_sizes=sizes, prop_time=2, fused_decoder=fused)
    else:
        net = unet_cspn_nyu.resnet18(decoder_sizes=sizes, prop_time=2, reference_state_dict=False, fused_decoder=fused)
    with torch.no_grad():                                                    # running statistics and affine maps that are not the initial ones
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0, 0.1)
    torch.manual_seed(12)
    inp = torch.rand(2, 4, 36, 52)
    return net.to(DEV), inp.to(DEV)


class Recorder(object):
    """Stands in for up_pooling_conv5x5 inside network.up_pooling: counts the calls and keeps what went in and came out."""

    def __init__(self, monkeypatch):
        self.calls, self.real = [], upmod.up_pooling_conv5x5
        monkeypatch.setattr(upmod, "up_pooling_conv5x5", self)

    def __call__(self, x, pack, oh, ow, *rest):
        outs = self.real(x, pack, oh, ow, *rest)
        self.calls.append((x.detach().clone(), pack, (oh, ow), outs))
        return outs


def check_recorded_calls(net, rec, what):
    """Each recorded call against the fp64 restatement on the block's own parameters, under the bound with the fold's n + 4."""
    assert len(rec.calls) == len(BLOCKS)
    for name, (x, pack, (oh, ow), outs) in zip(BLOCKS, rec.calls):
        block = getattr(net, name)
        assert (oh, ow) == (block.oheight, block.owidth) and pack is block._upconv_pack and not pack.stale()
        ws = [block.conv1.weight.detach().cpu().numpy(), block.sc_conv1.weight.detach().cpu().numpy()]
        folded = [uc.fold(*(t.detach().cpu().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)), bn.eps)
                  for bn in (block.bn1, block.sc_bn1)]
        scale, shift = np.concatenate([f[0] for f in folded]), np.concatenate([f[1] for f in folded])
        check_within_bound("%s %s" % (what, name), outs, x.cpu().numpy(), ws, oh, ow, scale, shift, ws[0].shape[0], extra=4)
        assert float(outs[0].min()) == 0.0 and float(outs[1].min()) < 0.0    # the ReLU on the first output only


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_models_fused_blocks_within_the_bound(kind, monkeypatch):
    net, inp = model_case(kind)
    rec = Recorder(monkeypatch)
    net.eval()
    with torch.no_grad():
        fused = net.features(inp)
    check_recorded_calls(net, rec, kind)
    # the whole decoder against the switch-off model on the same input: the same function up to fp32 rounding
    upmod.select_fused_decoder(net, False)
    with torch.no_grad():
        stock = net.features(inp)
    assert len(rec.calls) == len(BLOCKS)                                     # no further call
    for f, s in zip(fused, stock):
        assert f.shape == s.shape and float((f - s).abs().max()) <= 1e-3 * max(1.0, float(s.abs().max()))
    # after load_state_dict of other weights the next eval call runs on them: the packs were stale and made again
    other, _ = model_case(kind, seed=21)
    upmod.select_fused_decoder(net, BLOCKS)
    old = [getattr(net, n)._upconv_pack for n in BLOCKS]
    net.load_state_dict(other.state_dict())
    assert all(p is not None and p.stale() for p in old)
    del rec.calls[:]
    with torch.no_grad():
        net.features(inp)
    assert all(getattr(net, n)._upconv_pack is not p for n, p in zip(BLOCKS, old))
    check_recorded_calls(net, rec, kind + " reloaded")
    assert all(torch.equal(getattr(net, n).conv1.weight, getattr(other, n).conv1.weight) for n in BLOCKS)
    assert list(net.state_dict()) == list(other.state_dict()) == list(model_case(kind, fused=False)[0].state_dict())
    net.train()                                                              # train() drops the packs
    assert all(getattr(net, n)._upconv_pack is None for n in BLOCKS)


def decoder_only(net, ins):
    x = net.gud_up_proj_layer1(ins[0])
    x = net.gud_up_proj_layer2(x, ins[1])
    x = net.gud_up_proj_layer3(x, ins[2])
    return net.gud_up_proj_layer4(x, ins[3])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_train_mode_and_grad_mode_run_the_stock_blocks(kind, monkeypatch):
    net, inp = model_case(kind)
    rec = Recorder(monkeypatch)
    torch.manual_seed(14)
    ins = [torch.randn(2, 512, 2, 2, device=DEV), torch.randn(2, 128, 5, 7, device=DEV), torch.randn(2, 64, 9, 13, device=DEV),
           torch.randn(2, 64, 18, 26, device=DEV)]

    def both_ways(run_it):
        """run_it() with the switch on and off: the outputs, and whether the switch-off run repeats its own bits."""
        upmod.select_fused_decoder(net, BLOCKS)
        on = run_it()
        upmod.select_fused_decoder(net, False)
        off, off2 = run_it(), run_it()
        upmod.select_fused_decoder(net, BLOCKS)
        return on, off, torch.equal(off, off2)

    net.eval()                                                               # eval mode, grad mode on
    with torch.enable_grad():
        net.features(inp)
        on, off, repeatable = both_ways(lambda: decoder_only(net, ins).detach())
        assert not repeatable or torch.equal(on, off)
        out = decoder_only(net, [t.clone().requires_grad_(True) for t in ins])
        assert out.requires_grad and out.grad_fn is not None
    assert rec.calls == []
    state = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()                                                              # train mode, grad mode off: batch statistics, stock ops
    assert all(getattr(net, n)._upconv_pack is None for n in BLOCKS)
    with torch.no_grad():
        net.features(inp)

        def in_train_mode():
            net.load_state_dict(state)                                       # every run starts from the same running statistics
            return decoder_only(net, ins)

        on, off, repeatable = both_ways(in_train_mode)
        assert not repeatable or torch.equal(on, off)
    assert rec.calls == []
    net.eval()                                                               # and back: the fused head runs again
    with torch.no_grad():
        decoder_only(net, ins)
    assert len(rec.calls) == len(BLOCKS)


@pytest.mark.gpu
def test_simple_block_and_independent_switches(monkeypatch):
    """Simple_Gudi_UpConv_Block (one filter) through the same head; fused_heads and fused_decoder do not depend on each other."""
    torch.manual_seed(15)
    block = unet_ours.Simple_Gudi_UpConv_Block(5, 7, 9, 13).to(DEV).eval()
    x = torch.randn(2, 5, 5, 7, device=DEV)
    with torch.no_grad():
        block.bn1.running_mean.normal_()
        stock = block(x)
        block.fused_head = True
        fused = block(x)
    assert block._upconv_pack is not None and block._upconv_pack.out_channels == (7,)
    assert fused.shape == stock.shape and float((fused - stock).abs().max()) <= 1e-4 * float(stock.abs().max())
    rec = Recorder(monkeypatch)
    for heads, decoder, calls in ((True, False, 0), (False, ("gud_up_proj_layer2",), 1), (True, BLOCKS, 4)):
        net, inp = model_case("ours", fused=decoder)
        net.fused_heads = heads
        net.eval()
        del rec.calls[:]
        with torch.no_grad():
            net.features(inp)
        assert len(rec.calls) == calls

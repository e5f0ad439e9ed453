"""The half-precision fused decoder-block head: the `uphalf` family of the native library (include/cspn_uphalf.h), the `dtype` keyword
of network.up_pooling.pack_upconv5x5 / a half `x` of up_pooling_conv5x5, and the `fused_decoder` switch of the two models on half
inputs (torch.autocast and model.half()).

References: the numpy restatement of tests/upconv_cases.py on inputs rounded to fp16, rounded once to fp16 (tests/uphalf_cases.py),
and the integer goldens G27.  Integer-valued cases are compared bit for bit; real-valued cases against the a-priori bound
E + 2^-11 (|y| + E) + 2^-25 of uphalf_cases.bound_half (its docstring says where every term comes from)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import upconv_cases as uc
import uphalf_cases as hc
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd._host import launch
from cspn_monodepth_amd.network import unet_cspn_nyu, unet_ours
from cspn_monodepth_amd.network import up_pooling as upmod
from cspn_monodepth_amd.network.up_pooling import UpconvPack, pack_upconv5x5, up_pooling_conv5x5

DEV = "cuda:0"
INT_GOLDENS = golden_names("g27_upconv_int_")
BLOCKS = upmod.DECODER_BLOCKS
NAMES = ("cspn_uphalf_abi_version", "cspn_uphalf_packed_bytes", "cspn_uphalf_pack", "cspn_uphalf_forward")


def unpack(z):
    oh, ow, O, nf = (int(v) for v in z["geom"])
    ws, bns = [z["w%d" % k] for k in range(nf)], [z["bn%d" % k] for k in range(nf)]
    folded = [uc.fold(*p, float(z["eps"])) for p in bns]
    scale, shift = np.concatenate([f[0] for f in folded]), np.concatenate([f[1] for f in folded])
    return oh, ow, O, ws, scale, shift, [z["y%d" % k] for k in range(nf)]


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_uphalf_family_contract():
    """Header, loader table and library agree on the family, in the terms tests/test_upconv.py uses for `upconv`; the family sits in
    the opt-in part of the table, and its files stay out of the digest that pins the recorded HBM traffic."""
    fam = _lib.family("uphalf")
    assert fam.header == os.path.join(ROOT, "include", "cspn_uphalf.h") and fam.files == {"cspn_uphalf.hip": False}
    text = open(fam.header).read()
    assert re.search(r"^#define CSPN_UPHALF_ABI_VERSION 1$", text, flags=re.M)
    assert re.search(r"^#define CSPN_UPHALF_MAX_FILTERS 2$", text, flags=re.M) and _lib.UPHALF_MAX_FILTERS == 2
    assert "bf16" in text                                                     # out of scope, and said so
    declared = sorted(set(re.findall(r"\b(cspn\w*)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(fam.functions) == sorted(NAMES)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in NAMES) and lib.cspn_uphalf_abi_version() == fam.abi_version == 1
    # the opt-in part of the table, after the nine
    assert [f.name for f in _lib.OPT_IN_FAMILIES] == ["heads", "upconv", "uphalf", "uptail"]
    assert fam in _lib.OPT_IN_FAMILIES and fam not in _lib.FAMILIES
    assert _lib.ALL_FAMILIES == _lib.FAMILIES + _lib.OPT_IN_FAMILIES and len(_lib.ALL_FAMILIES) == 13
    assert "cspn_uphalf.hip" in _lib.OPT_IN_SOURCES and "cspn_uphalf.hip" not in _lib.SOURCES
    assert os.path.exists(os.path.join(_lib.CSRC, "cspn_uphalf.hip"))
    assert fam.header in _lib.BUILD_HEADERS and fam.header not in _lib.HEADERS
    for other in _lib.ALL_FAMILIES:
        if other is not fam:
            assert not set(other.functions) & set(NAMES) and not any("uphalf" in n for n in other.functions)
    # no name of the family holds a word another family's test searches the library for
    words = ("upconv", "heads", "criterion", "max8", "abn", "sparsify", "transform", "losses", "berhu", "mean_loss", "optim", "sgd", "visual")
    assert not any(w in n for w in words for n in NAMES)
    # the build's staleness hash sees the new files, the digest behind profiles/ does not: restated over the benchmarked files,
    # named here in literals
    assert _lib._source_digest(["x"]) != _lib._source_digest(["x"], code_only=True)
    benchmarked = ["cspn_propagate.hip", "cspn_resident.hip", "cspnk_resident.hip", "cspnk_d2.hip", "cspn_prepare.hip", "cspn_backward.hip",
                   "cspn_metrics.hip", "cspn_debug.hip", "cspn_repair.hip", "cspn_common.hpp", "cspnk_helpers.hpp"]
    import hashlib
    h = hashlib.sha256(b"")
    for path in [os.path.join(_lib.CSRC, f) for f in benchmarked] + [os.path.join(ROOT, "include", "cspn_hip.h")]:
        data = re.sub(rb"/\*.*?\*/", b"", open(path, "rb").read(), flags=re.S)
        lines = (re.sub(rb"//.*$", b"", ln).strip() for ln in data.splitlines())
        h.update(b"\n".join(re.sub(rb"\s+", b" ", ln) for ln in lines if ln))
    assert _lib.code_digest() == h.hexdigest()
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
        assert sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and "uphalf" in ln) == declared
    # the packed filters, callable without a device: 25 taps x the flat channels rounded up to 128 x C rounded up to 32, fp16
    pb = lib.cspn_uphalf_packed_bytes
    assert pb(2048, 2048) == 25 * 2048 * 2048 * 2 and pb(6, 3) == 25 * 32 * 128 * 2 and pb(129, 67) == 25 * 96 * 256 * 2
    for bad in ((0, 3), (3, 0), (-1, 3), (32768, 4096), (2 ** 30, 2 ** 30)):            # the last two: 2^31 packed elements or more
        assert pb(*bad) == 0
    # argument checks of the entry points come before any launch: no device needed
    one, two, three = (ctypes.c_void_p * 1)(16), (ctypes.c_void_p * 2)(16, 16), (ctypes.c_void_p * 3)(16, 16, 16)
    o1, o3 = (ctypes.c_int * 1)(1), (ctypes.c_int * 3)(1, 1, 1)
    F32, F16 = _lib.CSPN_F32, _lib.CSPN_F16
    err = lib.cspn_last_error
    pack = lib.cspn_uphalf_pack
    for dt in (F32, F16):
        assert not pack(one, o1, 1, 3, 3, 3, dt, 16, None) and b"5x5" in err()
        assert not pack(one, o1, 1, 3, 5, 3, dt, 16, None) and b"5x5" in err()
        assert not pack(three, o3, 3, 3, 5, 5, dt, 16, None) and b"between 1 and 2 filters" in err()
        assert not pack(one, o1, 1, 3, 5, 5, dt, None, None) and b"null" in err()
        assert not pack(None, o1, 1, 3, 5, 5, dt, 16, None) and b"null" in err()
        assert not pack((ctypes.c_void_p * 1)(None), o1, 1, 3, 5, 5, dt, 16, None) and b"null" in err()
        assert not pack(one, (ctypes.c_int * 1)(0), 1, 3, 5, 5, dt, 16, None) and b"output channels" in err()
        assert not pack(one, (ctypes.c_int * 1)(32768), 1, 4096, 5, 5, dt, 16, None) and b"2^31" in err()
    assert not pack(one, o1, 1, 3, 5, 5, 2, 16, None) and b"fp32 or fp16" in err()
    fwd = lib.cspn_uphalf_forward
    for oh, ow in ((5, 4), (4, 5), (0, 4), (4, 0)):
        assert not fwd(16, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, oh, ow, None) and b"[1, 2H]" in err()
    assert not fwd(16, 16, None, None, 0, three, o3, 3, 1, 1, 2, 2, 4, 4, None) and b"between 1 and 2 filters" in err()
    assert not fwd(16, 16, None, None, 0, one, o1, 1, 2 ** 16, 1, 2 ** 8, 2 ** 7, 1, 1, None) and b"2^31" in err()      # x
    assert not fwd(16, 16, None, None, 0, one, o1, 1, 2 ** 10, 1, 2 ** 10, 2 ** 9, 2 ** 11, 2 ** 10, None) and b"2^31" in err()      # an output
    assert not fwd(16, 16, 16, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"together" in err()
    assert not fwd(16, 16, None, 16, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"together" in err()
    for relu in (2, -1):
        assert not fwd(16, 16, None, None, relu, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"relu_channels" in err()
    assert not fwd(16, 16, None, None, 0, two, (ctypes.c_int * 2)(1, 0), 2, 1, 1, 2, 2, 4, 4, None) and b"output channels" in err()
    assert not fwd(None, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"null" in err()
    assert not fwd(16, None, None, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"null" in err()
    assert not fwd(16, 16, None, None, 0, (ctypes.c_void_p * 1)(None), o1, 1, 1, 1, 2, 2, 4, 4, None) and b"null" in err()
    # ... and the fp32 family still takes fp32 alone
    assert not lib.cspn_upconv_pack(one, o1, 1, 3, 5, 5, F16, 16, None) and b"fp32" in err()


def test_python_refusals_and_the_dtype_keyword():
    x, w3, w2 = torch.zeros(2, 3, 4, 5), torch.zeros(3, 3, 5, 5), torch.zeros(2, 3, 5, 5)
    for ws in ((w3,), (w3.half(),), (w3.half(), w2.half())):                 # past the dtype checks: refused as CPU tensors
        with pytest.raises(RuntimeError, match="ROCm device"):
            pack_upconv5x5(ws, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        pack_upconv5x5((w3,), dtype=torch.float32)
    for dt in (torch.bfloat16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="fp32 or fp16"):
            pack_upconv5x5((w3,), dtype=dt)
    for ws, dt in (((w3.half(),), torch.float32), ((w3.double(),), torch.float16), ((w3.bfloat16(),), torch.float16),
                   ((w3.bfloat16(),), torch.float32)):
        with pytest.raises(ValueError, match="fp32"):
            pack_upconv5x5(ws, dtype=dt)
    with pytest.raises(ValueError, match="fp32"):                            # the default is what it was
        pack_upconv5x5((w3.half(),))
    with pytest.raises(ValueError, match="one dtype"):
        pack_upconv5x5((w3, w2.half()), dtype=torch.float16)
    assert UpconvPack(None, None, None, (3,), 3, 3, (w3,)).dtype == torch.float32
    p32 = UpconvPack(None, None, None, (3,), 3, 3, (w3,), torch.float32)
    p16 = UpconvPack(None, None, None, (3,), 3, 3, (w3,), torch.float16)
    assert p32.dtype == torch.float32 and p16.dtype == torch.float16 and not p16.stale() and p16.made_from([w3])
    with pytest.raises(ValueError, match=r"float16.*float32"):                # a dtype mismatch names both
        up_pooling_conv5x5(x.half(), p32, 8, 10)
    with pytest.raises(ValueError, match=r"float32.*float16"):
        up_pooling_conv5x5(x, p16, 8, 10)
    with pytest.raises(ValueError, match=r"bfloat16.*float16"):
        up_pooling_conv5x5(x.bfloat16(), p16, 8, 10)
    with pytest.raises(ValueError, match="fp32"):                            # the filters themselves stay fp32-only
        up_pooling_conv5x5(x.half(), (w3,), 8, 10)
    with pytest.raises(ValueError, match="fp32"):
        up_pooling_conv5x5(x.half(), (w3.half(),), 8, 10)
    with torch.no_grad():                                                     # matching dtypes: past the checks, refused as CPU tensors
        with pytest.raises(RuntimeError, match="ROCm device"):
            up_pooling_conv5x5(x.half(), p16, 8, 10)
        with pytest.raises(ValueError, match="must lie within"):
            up_pooling_conv5x5(x.half(), p16, 9, 10)
    with torch.enable_grad():                                                 # forward only in half as well
        with pytest.raises(RuntimeError, match="forward-only"):
            up_pooling_conv5x5(x.half().requires_grad_(True), p16, 8, 10)


def test_half_default_is_a_selection_of_the_blocks():
    assert isinstance(upmod.FUSED_DECODER_HALF_DEFAULT, tuple) and set(upmod.FUSED_DECODER_HALF_DEFAULT) <= set(BLOCKS)
    assert upmod.FUSED_DECODER_DEFAULT == BLOCKS                              # the fp32 selection is what it was
    for net in (unet_ours, unet_cspn_nyu):
        m = net.resnet18(fused_decoder=True)
        assert m.fused_decoder == BLOCKS
        assert [getattr(m, n).fused_head_half for n in BLOCKS] == [n in upmod.FUSED_DECODER_HALF_DEFAULT for n in BLOCKS]
        m = net.resnet18(fused_decoder=["gud_up_proj_layer2"])               # named blocks: both precisions
        assert [getattr(m, n).fused_head_half for n in BLOCKS] == [getattr(m, n).fused_head for n in BLOCKS] == [False, True, False, False]
        m = net.resnet18()
        assert not any(getattr(m, n).fused_head_half or getattr(m, n).fused_head for n in BLOCKS)
    # which dtype runs which path: grad mode off, eval mode
    block = unet_ours.Simple_Gudi_UpConv_Block(5, 7, 9, 13).eval()
    x = torch.zeros(1, 5, 5, 7)
    with torch.no_grad():
        assert not block._fuse_head(x) and not block._fuse_head(x.half())
        block.fused_head = True                                               # marked by hand: half follows
        assert block._fuse_head() and block._fuse_head(x) and block._fuse_head(x.half())
        assert not block._fuse_head(x.bfloat16()) and not block._fuse_head(x.double())
        block.fused_head_half = False
        assert block._fuse_head(x) and not block._fuse_head(x.half())
        block.fused_head, block.fused_head_half = False, True
        assert not block._fuse_head(x) and block._fuse_head(x.half())
    with torch.enable_grad():
        assert not block._fuse_head(x.half())
    with torch.no_grad():
        assert not block.train()._fuse_head(x.half())


@pytest.mark.parametrize("name", INT_GOLDENS)
def test_half_restatement_equals_the_integer_goldens(name):
    z = load_golden(name)
    oh, ow, O, ws, scale, shift, want = unpack(z)
    assert np.array_equal(hc.to_half(z["x"]), z["x"]) and all(np.array_equal(hc.to_half(w), w) for w in ws)
    got, exact = hc.restate_half(z["x"], ws, oh, ow, scale, shift, O)
    for g, e, w in zip(got, exact, want):
        assert g.dtype == np.float16 and np.abs(e).max() < hc.HALF_MAX
        assert np.array_equal((g + np.float16(0)).view(np.uint16), (w + 0.0).astype(np.float16).view(np.uint16))      # + 0: one sign of zero


def test_every_case_stays_inside_the_half_range():
    """No case of the GPU tests below overflows fp16: what they compare are finite values, and the bound's 2^-11 |y| term applies."""
    n = 0
    for shape, out_hw, filters in hc.integer_shapes():
        x, ws, scale, shift, acc = hc.integer_case(shape, out_hw, filters)
        assert acc <= 9 * 67 * 9 and 4 * acc + 5 < hc.HALF_MAX and 4 * acc + 5 < 2 ** 24
        n += 1
    assert n == len(uc.GEOMETRIES) * len(uc.CHANNELS) * len(uc.FILTER_SETS) * len(uc.BATCHES) + 1
    for shape, out_hw, both in uc.REAL_CASES:
        x, ws, scale, shift, filters = hc.real_case(shape, out_hw, both)
        for relu in hc.relu_boundaries(filters):
            assert max(np.abs(e).max() for e in hc.restate_half(x, ws, *out_hw, scale, shift, relu)[1]) < hc.HALF_MAX
        assert max(np.abs(e).max() for e in hc.restate_half(x, ws, *out_hw)[1]) < hc.HALF_MAX
    assert hc.gamma_faithful(1000) > 2 * uc.gamma(1000) > 0 and hc.U_FAITHFUL == 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def packed_for(ws, source_dtype):
    """The filters packed for the half kernel from fp32 or from fp16 sources."""
    return pack_upconv5x5(tuple(dev(w, source_dtype) for w in ws), None, (False,) * len(ws), dtype=torch.float16)


def run(x, pack, oh, ow, scale=None, shift=None, relu=0):
    """The half kernel on `pack`'s filters with an affine map and a ReLU count of the test's own."""
    mine = UpconvPack(pack.packed, None if scale is None else dev(scale), None if shift is None else dev(shift), pack.out_channels,
                      pack.in_channels, relu, pack.sources, torch.float16)
    with torch.no_grad():
        outs = up_pooling_conv5x5(dev(x, torch.float16), mine, oh, ow)
    assert isinstance(outs, tuple) and len(outs) == len(pack.out_channels)
    assert all(o.is_contiguous() and o.dtype == torch.float16 and tuple(o.shape) == (x.shape[0], c, oh, ow) for o, c in zip(outs, pack.out_channels))
    return outs


def same_bits(t, a):
    a = np.asarray(a)
    return t.dtype == torch.float16 and a.dtype == np.float16 and tuple(t.shape) == a.shape and \
        np.array_equal(t.detach().cpu().numpy().view(np.uint16), a.view(np.uint16))


def integer_case(shape, out_hw, filters):
    x, ws, scale, shift, _ = hc.integer_case(shape, out_hw, filters)
    packs = [packed_for(ws, torch.float32), packed_for(ws, torch.float16)]
    assert packs[0].packed.dtype == torch.float16 and torch.equal(packs[0].packed, packs[1].packed)
    assert packs[0].packed.numel() * 2 == _lib.lib().cspn_uphalf_packed_bytes(sum(filters), shape[1])
    for relu in hc.relu_boundaries(filters) + [None]:                        # None: no affine map at all
        args = (scale, shift, relu) if relu is not None else ()
        want = hc.restate_half(x, ws, *out_hw, *args)[0]
        for pack in packs:
            for g, w in zip(run(x, pack, *out_hw, *args), want):
                assert same_bits(g, w + np.float16(0)), (shape, out_hw, filters, relu)      # + 0: an exact zero is +0 on both sides


@pytest.mark.gpu
@pytest.mark.parametrize("hw,out_hw", uc.GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_integer_cases_bit_equal_to_the_restatement(hw, out_hw):
    for shape, o, filters in hc.integer_shapes():
        if shape[2:] == hw and o == out_hw and shape != uc.BIG["shape"]:
            integer_case(shape, o, filters)


@pytest.mark.gpu
def test_integer_case_over_several_chunks_and_tiles():
    shape, out_hw, filters = uc.BIG["shape"], uc.BIG["out_hw"], uc.BIG["filters"]
    assert shape[1] > 32 and all(shape[0] * ((out_hw[0] + 1 - a) // 2) * ((out_hw[1] + 1 - b) // 2) > 128 for a, b in uc.PHASES)
    integer_case(shape, out_hw, filters)


@pytest.mark.gpu
def test_integer_cases_over_several_m_tiles():
    """mt > 0 in fwd<F16>, whose filter tile is found by a row index times Cp: upconv_cases.M_TILE_FILTER_SETS, bit for bit
    (tests/test_upconv.py holds every case inside the fp16 range without a GPU)."""
    for shape, out_hw, filters in uc.m_tile_shapes():
        assert 4 * hc.integer_case(shape, out_hw, filters)[4] + 5 < hc.HALF_MAX
        integer_case(shape, out_hw, filters)


@pytest.mark.gpu
def test_ragged_m_tile_under_poisoned_lds():
    shape, out_hw, filters = uc.M_TILE_POISON_CASE
    x, ws, scale, shift, _ = hc.integer_case(shape, out_hw, filters)
    pack = packed_for(ws, torch.float32)
    plain = run(x, pack, *out_hw, scale, shift, filters[0])
    with lds_poison(0x7fc07fc0):                                             # NaN in both fp16 halves of every word
        got = run(x, pack, *out_hw, scale, shift, filters[0])
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, plain)) and not any(bool(torch.isnan(g).any()) for g in got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", INT_GOLDENS)
def test_integer_goldens_bit_equal(name):
    z = load_golden(name)
    oh, ow, O, ws, scale, shift, want = unpack(z)
    for source in (torch.float32, torch.float16):
        got = run(z["x"], packed_for(ws, source), oh, ow, scale.astype(np.float32), shift.astype(np.float32), O)
        for g, w in zip(got, want):
            assert same_bits(g, (w + 0.0).astype(np.float16))


def check_within_bound(what, got, x, ws, oh, ow, scale, shift, relu, extra=0):
    """got (device tensors, one per filter) against the fp64 restatement of the fp16-rounded inputs under the a-priori bound; the
    largest ratio."""
    want = np.concatenate(hc.restate_half(x, ws, oh, ow, scale, shift, relu)[1], 1)
    assert np.abs(want).max() < hc.HALF_MAX
    bound = hc.bound_half(x, ws, oh, ow, scale, shift, relu, extra)
    got = np.concatenate([g.cpu().numpy().astype(np.float64) for g in got], 1)
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print("%s: largest error / bound = %.4f" % (what, ratio))
    assert (err <= bound).all(), (what, ratio)
    assert err.max() > 0                                                     # rounded results, not a copy of the fp64 ones
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out_hw,both", uc.REAL_CASES, ids=lambda v: "x".join(map(str, v)))
def test_real_cases_within_the_a_priori_bound(shape, out_hw, both):
    x, ws, scale, shift, filters = hc.real_case(shape, out_hw, both)
    pack = packed_for(ws, torch.float32)
    assert torch.equal(pack.packed, packed_for(ws, torch.float16).packed)
    for relu in hc.relu_boundaries(filters):
        check_within_bound("%s relu %d" % (shape, relu), run(x, pack, *out_hw, scale, shift, relu), x, ws, *out_hw, scale, shift, relu)
    check_within_bound("%s plain" % (shape,), run(x, pack, *out_hw), x, ws, *out_hw, None, None, 0)


@pytest.mark.gpu
def test_fp32_sources_are_rounded_to_nearest_even_once():
    """Filters that are no fp16 values: the pack from fp32 sources equals the pack from the same filters rounded by numpy."""
    ws = uc.make_inputs(90, (1, 5, 2, 2), (3, 2), False)[1]
    ws[0][0, 0, 0, :4] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 2.0 ** -25]      # ties to even, the largest value that stays finite, a tie at the bottom
    assert any((hc.to_half(w) != w).any() for w in ws)
    assert torch.equal(packed_for(ws, torch.float32).packed, packed_for([hc.to_half(w) for w in ws], torch.float16).packed)
    assert torch.equal(packed_for(ws, torch.float32).packed, packed_for(ws, torch.float16).packed)      # torch's own rounding agrees


@pytest.mark.gpu
def test_batch_place_and_determinism():
    shape, out_hw, filters = (3,) + uc.BIG["shape"][1:], uc.BIG["out_hw"], uc.BIG["filters"]
    x, ws, scale, shift = uc.make_inputs(91, shape, filters, False)
    pack = packed_for(ws, torch.float32)
    ys = run(x, pack, *out_hw, scale, shift, filters[0])
    again = run(x, pack, *out_hw, scale, shift, filters[0])
    assert all(torch.equal(a, b) for a, b in zip(ys, again))                  # two runs of one call
    for n in (0, 2):                                                         # frame n of B = 3 at position 0 of B = 1
        alone = run(x[n:n + 1], pack, *out_hw, scale, shift, filters[0])
        assert all(torch.equal(a[0], b[n]) for a, b in zip(alone, ys))
    pair = run(x[1:3], pack, *out_hw, scale, shift, filters[0])              # ... and at position 1 of B = 2: other tiles again
    assert all(torch.equal(a[1], b[2]) for a, b in zip(pair, ys))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out_hw,filters", [((2, 5, 5, 7), (9, 13), (17, 16)), ((1, 3, 6, 7), (4, 5), (33,)),
                                                   ((3, 3, 1, 2), (2, 3), (3, 3))], ids=["odd", "deep_crop", "tiny"])
def test_nothing_outside_the_outputs_is_written(shape, out_hw, filters):
    x, ws, scale, shift = uc.make_inputs(92, shape, filters, True)
    pack = packed_for(ws, torch.float32)
    want = run(x, pack, *out_hw, scale, shift, filters[0])
    pad, sentinel = 4096, -12288.0                                           # a fp16 value
    sizes = [shape[0] * o * out_hw[0] * out_hw[1] for o in filters]
    sizes8 = [(s + 7) // 8 * 8 for s in sizes]                               # every output starts 16-byte aligned, as an allocation does
    buf = torch.full((pad + sum(s + pad for s in sizes8),), sentinel, device=DEV, dtype=torch.float16)
    outs, at = [], pad
    for s, s8, o in zip(sizes, sizes8, filters):
        outs.append(buf[at:at + s].view(shape[0], o, *out_hw))
        at += s8 + pad
    xd, sd, hd = dev(x, torch.float16), dev(scale), dev(shift)
    ptrs = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    launch(torch.device(DEV), "cspn_uphalf_forward", xd.data_ptr(), pack.packed.data_ptr(), sd.data_ptr(), hd.data_ptr(), filters[0], ptrs,
           (ctypes.c_int * len(outs))(*filters), len(outs), *shape, *out_hw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want))
    keep = torch.ones_like(buf, dtype=torch.bool)
    at = pad
    for s, s8 in zip(sizes, sizes8):
        keep[at:at + s] = False
        at += s8 + pad
    assert int(keep.sum()) == buf.numel() - sum(sizes) and bool((buf[keep] == sentinel).all())
    # the compact pixels the crop removed are not read either: NaN there changes nothing
    if out_hw[0] < 2 * shape[2] - 1:
        xn = x.copy()
        xn[:, :, (out_hw[0] + 1) // 2:, :] = np.nan
        xn[:, :, :, (out_hw[1] + 1) // 2:] = np.nan
        assert all(torch.equal(a, b) for a, b in zip(run(xn, pack, *out_hw, scale, shift, filters[0]), want))


@pytest.mark.gpu
def test_nan_reaches_only_the_windows_that_cover_it():
    """As the fp32 kernel: x[0,1,2,3] = NaN poisons the outputs whose 5x5 window covers (4, 6) — rows 2..6, columns 4..8 — and
    nothing else."""
    x, ws, scale, shift = uc.make_inputs(93, (1, 2, 5, 6), (3, 2), False)
    x[0, 1, 2, 3] = np.nan
    y = torch.cat(run(x, packed_for(ws, torch.float32), 10, 12, scale, shift, 3), 1)
    nan = torch.isnan(y[0])
    assert np.array_equal(np.argwhere(nan.all(0).cpu().numpy()), [[r, c] for r in range(2, 7) for c in range(4, 9)])
    assert int(nan.any(0).sum()) == 25
    x[0, 1, 2, 3] = 0.0                                                      # ... and the rest is what it is without the NaN
    clean = torch.cat(run(x, packed_for(ws, torch.float32), 10, 12, scale, shift, 3), 1)
    assert torch.equal(y[~torch.isnan(y)], clean[~torch.isnan(y)])


@pytest.mark.gpu
def test_graph_capture_of_pack_and_forward_gives_the_eager_bits():
    """Forward only, under no_grad: pack-then-forward captured once, replayed on new input values."""
    shape, out_hw, filters = uc.BIG["shape"], uc.BIG["out_hw"], uc.BIG["filters"]
    x, ws, scale, shift = uc.make_inputs(94, shape, filters, False)
    x2 = uc.make_inputs(95, shape, filters, False)[0]
    weights = [torch.nn.Parameter(dev(w)) for w in ws]
    mods = [torch.nn.BatchNorm2d(o).to(DEV).eval() for o in filters]
    with torch.no_grad():
        for k, bn in enumerate(mods):
            bn.running_mean.copy_(dev(shift[k * 40:(k + 1) * 40]))
            bn.weight.copy_(dev(scale[k * 40:(k + 1) * 40]))

        def pack_and_forward(v):
            return up_pooling_conv5x5(v, pack_upconv5x5(weights, mods, dtype=torch.float16), *out_hw)

        eager = [pack_and_forward(dev(v, torch.float16)) for v in (x, x2)]
        sx = dev(x, torch.float16)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pack_and_forward(sx)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = pack_and_forward(sx)
        for v, want in ((x2, eager[1]), (x, eager[0])):                      # two replays, on new input values
            sx.copy_(dev(v, torch.float16))
            for t in outs:
                t.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, want))
    assert all(o.dtype == torch.float16 for o in outs) and not torch.equal(eager[0][0], eager[1][0])


def model_case(kind, fused=BLOCKS, seed=11):
    """tests/test_upconv.py's model: resnet18 of either network at 36 x 52, B = 2, batch norms with statistics that are not the
    initial ones."""
    torch.manual_seed(seed)
    sizes = unet_ours.decoder_sizes_for(36, 52)
    if kind == "ours":
        net = unet_ours.resnet18(decoder_sizes=sizes, prop_time=2, fused_decoder=fused)
    else:
        net = unet_cspn_nyu.resnet18(decoder_sizes=sizes, prop_time=2, reference_state_dict=False, fused_decoder=fused)
    with torch.no_grad():
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
    """Stands in for up_pooling_conv5x5 and for launch inside network.up_pooling: keeps what went into and came out of every fused
    head, and the name of every native entry point that was called."""

    def __init__(self, monkeypatch):
        self.calls, self.entries, self.real, self.real_launch = [], [], upmod.up_pooling_conv5x5, upmod.launch
        monkeypatch.setattr(upmod, "up_pooling_conv5x5", self)
        monkeypatch.setattr(upmod, "launch", self.launch)

    def __call__(self, x, pack, oh, ow, *rest):
        outs = self.real(x, pack, oh, ow, *rest)
        self.calls.append((x.detach().clone(), pack, (oh, ow), outs))
        return outs

    def launch(self, device, name, *args):
        self.entries.append(name)
        return self.real_launch(device, name, *args)

    def clear(self):
        del self.calls[:], self.entries[:]


def run_model(net, inp, how):
    with torch.no_grad():
        if how == "autocast":
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                return net.features(inp)
        return net.features(inp.to(next(net.parameters()).dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["autocast", "half"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_models_fused_blocks_within_the_bound(kind, how, monkeypatch):
    net, inp = model_case(kind)
    net.eval()
    if how == "half":
        net.half()
    rec = Recorder(monkeypatch)
    run_model(net, inp, how)
    assert len(rec.calls) == len(BLOCKS)
    assert [n for n in rec.entries if "upconv" in n or "uphalf" in n] == ["cspn_uphalf_pack", "cspn_uphalf_forward"] * len(BLOCKS)
    for name, (x, pack, (oh, ow), outs) in zip(BLOCKS, rec.calls):
        block = getattr(net, name)
        assert x.dtype == torch.float16 and pack.dtype == torch.float16 and all(o.dtype == torch.float16 for o in outs)
        assert (oh, ow) == (block.oheight, block.owidth) and pack is block._upconv_pack and not pack.stale()
        assert block.conv1.weight.dtype == (torch.float16 if how == "half" else torch.float32)
        ws = [block.conv1.weight.detach().float().cpu().numpy(), block.sc_conv1.weight.detach().float().cpu().numpy()]
        folded = [uc.fold(*(t.detach().float().cpu().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)), bn.eps)
                  for bn in (block.bn1, block.sc_bn1)]
        scale, shift = np.concatenate([f[0] for f in folded]), np.concatenate([f[1] for f in folded])
        check_within_bound("%s %s %s" % (kind, how, name), outs, x.float().cpu().numpy(), ws, oh, ow, scale, shift, ws[0].shape[0], extra=4)
        assert float(outs[0].min()) == 0.0 and float(outs[1].min()) < 0.0    # the ReLU on the first output only
    # a second forward packs nothing again
    rec.clear()
    run_model(net, inp, how)
    assert [n for n in rec.entries if "upconv" in n or "uphalf" in n] == ["cspn_uphalf_forward"] * len(BLOCKS)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_each_precision_goes_to_its_own_entry_point(kind, monkeypatch):
    net, inp = model_case(kind)
    net.eval()
    rec = Recorder(monkeypatch)

    def fused_entries():
        return [n for n in rec.entries if "upconv" in n or "uphalf" in n]

    run_model(net, inp, "fp32")                                              # fp32: the fp32 family, as before
    assert fused_entries() == ["cspn_upconv_pack", "cspn_upconv_forward"] * 4 and all(c[0].dtype == torch.float32 for c in rec.calls)
    rec.clear()
    run_model(net, inp, "autocast")                                          # the same model under autocast: repacked for half
    assert fused_entries() == ["cspn_uphalf_pack", "cspn_uphalf_forward"] * 4 and all(c[1].dtype == torch.float16 for c in rec.calls)
    rec.clear()
    run_model(net, inp, "fp32")                                              # ... and back
    assert fused_entries() == ["cspn_upconv_pack", "cspn_upconv_forward"] * 4
    rec.clear()
    with torch.autocast(device_type="cuda", dtype=torch.float16):            # grad mode on: the stock blocks
        with torch.enable_grad():
            net.features(inp)
    assert rec.calls == [] and fused_entries() == []
    net.train()                                                              # train mode: the stock blocks, and no pack is kept
    assert all(getattr(net, n)._upconv_pack is None for n in BLOCKS)
    run_model(net, inp, "autocast")
    assert rec.calls == [] and fused_entries() == []
    net.eval()
    upmod.select_fused_decoder(net, True)                                    # True: half inputs take the half selection
    run_model(net, inp, "autocast")
    assert len(rec.calls) == len(upmod.FUSED_DECODER_HALF_DEFAULT)
    rec.clear()
    run_model(net, inp, "fp32")
    assert len(rec.calls) == len(upmod.FUSED_DECODER_DEFAULT)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["autocast", "half"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_end_to_end_no_worse_than_the_stock_half_model(kind, how):
    """The yardstick is the stock half-precision model: on the same inputs and weights, the distance of the fused half model from
    the stock fp32 model is at most 1.5 times the distance of the stock half model from it (blur depth and guidance, each over the
    fp32 output's range).  The fused head rounds once where the stock path rounds after the convolution, the batch norm and the
    ReLU; the factor covers that both distances are single samples of rounding noise."""
    net, inp = model_case(kind, fused=False)
    net.eval()
    ref = run_model(net, inp, "fp32")[:2]
    if how == "half":
        net.half()
    stock = run_model(net, inp, how)[:2]
    upmod.select_fused_decoder(net, BLOCKS)
    fused = run_model(net, inp, how)[:2]
    assert all(getattr(net, n)._upconv_pack is not None and getattr(net, n)._upconv_pack.dtype == torch.float16 for n in BLOCKS)

    def distance(outs):
        return max(float((o.float() - r).abs().max() / (r.max() - r.min())) for o, r in zip(outs, ref))

    d_stock, d_fused = distance(stock), distance(fused)
    print("%s %s: d_stock = %.3e, d_fused = %.3e" % (kind, how, d_stock, d_fused))
    assert all(o.dtype == torch.float16 for o in stock + fused) and 0 < d_stock
    assert d_fused <= 1.5 * d_stock, (d_fused, d_stock)

"""The fused 3x3 tail of the decoder blocks: the `uptail` family of the native library (include/cspn_uptail.h),
network.up_pooling.pack_conv3x3 / conv3x3_bn_act, and the `fused_tail` switch of the two models.

References: the numpy restatement of tests/uptail_cases.py (fp64; for half on inputs rounded to fp16 and rounded once to fp16) and the
goldens G29 (the reference's blocks in fp64).  Integer-valued cases are compared bit for bit; real-valued cases against the a-priori
bounds of uptail_cases.bound / bound_half (the module's docstring says where every term comes from)."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import uptail_cases as tc
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd._host import launch
from cspn_monodepth_amd.network import unet_cspn_nyu, unet_ours
from cspn_monodepth_amd.network import up_pooling as upmod
from cspn_monodepth_amd.network.up_pooling import UpconvPack, conv3x3_bn_act, pack_conv3x3

DEV = "cuda:0"
GOLDENS = golden_names("g29_uptail_")
BLOCKS = upmod.DECODER_BLOCKS
NAMES = ("cspn_uptail_abi_version", "cspn_uptail_packed_bytes", "cspn_uptail_pack", "cspn_uptail_forward")
F32, F16 = _lib.CSPN_F32, _lib.CSPN_F16


def golden_steps(z):
    """The tail of a golden as conv3x3_bn_act steps: (a, side, w, scale, shift, residual, the stored result), fp64."""
    eps, cat = float(z["eps"]), bool(z["geom"][3])
    steps = []
    if cat:
        steps.append((z["out"], z["side"], z["w1_1"], *tc.fold(*z["bn1_1"], eps), None, z["mid"]))
    steps.append((z["mid"] if cat else z["out"], None, z["w2"], *tc.fold(*z["bn2"], eps), z["shortcut"], z["y"]))
    return steps


def close(got, want, integer):
    return np.array_equal(got, want) if integer else np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_the_manifest():
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "g29_uptail_manifest.json")))
    assert sorted(manifest["files"]) == GOLDENS == sorted("g29_uptail_" + n for n in tc.GOLDEN_CASES) and len(GOLDENS) == 12
    for name, row in manifest["files"].items():
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) == row["bytes"] <= 131072
    sizes = {tuple(row["shape"][2:]) for row in manifest["files"].values() if row["integer"]}
    assert sizes == {(1, 1), (2, 3), (6, 8), (4, 5)}
    assert {tuple(row["shape"][2:]) for row in manifest["files"].values() if not row["integer"]} == {(9, 13), (15, 19)}
    assert {row["block"] for row in manifest["files"].values()} == {"Gudi_UpProj_Block", "Gudi_UpProj_Block_Cat"}


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_golden(name):
    z = load_golden(name)
    integer = "_int_" in name
    assert len(golden_steps(z)) == 1 + int(z["geom"][3])
    for a, side, w, scale, shift, r, want in golden_steps(z):
        got = tc.restate(a, side, w, scale, shift, r, True)
        assert got.dtype == np.float64 and got.shape == want.shape and close(got, want, integer)
        assert not close(tc.restate(a, side, w, scale, shift, r, False), want, integer) or want.min() > 0      # the ReLU matters


@pytest.mark.parametrize("shape", tc.SHAPES + (tc.BIG["shape"],), ids=lambda v: "x".join(map(str, v)))
def test_restatement_equals_conv2d_on_the_concatenation(shape):
    """At every shape the GPU tests run: torch's fp64 conv2d on cat(a, b), exactly on the integer-valued inputs and to 1e-12 on
    the real-valued ones."""
    cases = [(tc.BIG["channels"], tc.BIG["O"], shape)] if shape == tc.BIG["shape"] else tc.integer_cases(shape)
    for integer in (True, False):
        for channels, O, _ in cases + [c for c in tc.REAL_CASES if c[2] == shape and not integer]:
            a, b, w, scale, shift, r = tc.make_inputs(channels, O, shape, integer)
            x = torch.from_numpy(a if b is None else np.concatenate((a, b), 1)).double()
            want = torch.nn.functional.conv2d(x, torch.from_numpy(w).double(), padding=1).numpy()
            assert close(tc.accumulate(a.astype(np.float64), None if b is None else b.astype(np.float64), w.astype(np.float64)), want, integer)
            if integer:
                acc = np.abs(want).max()
                assert acc <= 9 * 107 * 9 and 4 * acc + 13 < tc.HALF_MAX and all(np.array_equal(tc.to_half(t), t) for t in (a, w, r))
            want = want * scale[None, :, None, None].astype(np.float64) + shift[None, :, None, None] + r
            assert close(tc.restate(a, b, w, scale, shift, r, True), np.maximum(want, 0), integer)


def test_uptail_family_contract():
    """Header, loader table and library agree on the family, in the terms the older contract tests use for theirs; the family is
    the last of the opt-in ones, and the nine default families are what they were."""
    fam = _lib.family("uptail")
    assert fam.header == os.path.join(ROOT, "include", "cspn_uptail.h") and fam.files == {"cspn_uptail.hip": False}
    text = open(fam.header).read()
    assert re.search(r"^#define CSPN_UPTAIL_ABI_VERSION 1$", text, flags=re.M)
    declared = sorted(set(re.findall(r"\b(cspn\w*)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(fam.functions) == sorted(NAMES)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in NAMES) and lib.cspn_uptail_abi_version() == fam.abi_version == 1
    # the opt-in part of the table, after the nine
    assert fam in _lib.OPT_IN_FAMILIES and fam not in _lib.FAMILIES and fam.opt_in
    assert [f.name for f in _lib.OPT_IN_FAMILIES] == ["heads", "upconv", "uphalf", "uptail"]
    assert _lib.ALL_FAMILIES == _lib.FAMILIES + _lib.OPT_IN_FAMILIES and len(_lib.FAMILIES) == 9 and len(_lib.ALL_FAMILIES) == 13
    assert "cspn_uptail.hip" in _lib.OPT_IN_SOURCES and "cspn_uptail.hip" not in _lib.SOURCES
    assert os.path.exists(os.path.join(_lib.CSRC, "cspn_uptail.hip"))
    assert fam.header in _lib.BUILD_HEADERS and fam.header not in _lib.HEADERS
    assert len([p for p in _lib.BUILD_HEADERS if os.path.dirname(p) == _lib.CSRC]) == 6          # no new header under csrc/
    for other in _lib.ALL_FAMILIES:
        if other is not fam:
            assert not set(other.functions) & set(NAMES) and not any("uptail" in n for n in other.functions)
    words = ("upconv", "uphalf", "heads", "criterion", "max8", "abn", "sparsify", "transform", "losses", "berhu", "mean_loss", "optim",
             "sgd", "visual")
    assert not any(w in n for w in words for n in NAMES)
    # the build's staleness hash sees the new source; the digest behind profiles/ does not: restated over the benchmarked files
    import hashlib
    plain = hashlib.sha256(b"x")
    for path in [os.path.join(_lib.CSRC, f) for f in _lib.SOURCES + _lib.OPT_IN_SOURCES if f != "cspn_uptail.hip"] + \
            list(_lib.BUILD_HEADERS):
        plain.update(open(path, "rb").read())
    assert _lib._source_digest(["x"]) != plain.hexdigest()                       # ... without cspn_uptail.hip it is another hash
    plain = hashlib.sha256(b"x")
    for path in [os.path.join(_lib.CSRC, f) for f in _lib.SOURCES + _lib.OPT_IN_SOURCES] + list(_lib.BUILD_HEADERS):
        plain.update(open(path, "rb").read())
    assert _lib._source_digest(["x"]) == plain.hexdigest()
    benchmarked = ["cspn_propagate.hip", "cspn_resident.hip", "cspnk_resident.hip", "cspnk_d2.hip", "cspn_prepare.hip", "cspn_backward.hip",
                   "cspn_metrics.hip", "cspn_debug.hip", "cspn_repair.hip", "cspn_common.hpp", "cspnk_helpers.hpp"]
    h = hashlib.sha256(b"")
    for path in [os.path.join(_lib.CSRC, f) for f in benchmarked] + [os.path.join(ROOT, "include", "cspn_hip.h")]:
        data = re.sub(rb"/\*.*?\*/", b"", open(path, "rb").read(), flags=re.S)
        lines = (re.sub(rb"//.*$", b"", ln).strip() for ln in data.splitlines())
        h.update(b"\n".join(re.sub(rb"\s+", b" ", ln) for ln in lines if ln))
    assert _lib.code_digest() == h.hexdigest()
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
        assert sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and "uptail" in ln) == declared


def test_packed_bytes_by_hand():
    pb = _lib.lib().cspn_uptail_packed_bytes
    assert pb(6, 3, 0, F32) == 9 * 32 * 128 * 4 and pb(129, 33, 5, F16) == 9 * (64 + 32) * 256 * 2
    assert pb(64, 64, 64, F32) == 9 * 128 * 128 * 4 and pb(64, 64, 64, F16) == 9 * 128 * 128 * 2
    for bad in ((0, 3, 0, F32), (3, 0, 0, F32), (3, 0, 3, F32), (3, 3, -1, F16), (-1, 3, 0, F16), (3, 3, 0, 2), (3, 3, 0, -1),
                (32768, 4096, 4096, F16), (2 ** 24 + 1, 1, 0, F32), (2 ** 14, 2 ** 14, 0, F32)):      # the last ones: 2^31 packed elements or more
        assert pb(*bad) == 0, bad


def test_argument_checks_come_before_any_launch():
    lib = _lib.lib()
    err, pack, fwd = lib.cspn_last_error, lib.cspn_uptail_pack, lib.cspn_uptail_forward
    for kh, kw in ((5, 5), (3, 1), (1, 3)):
        assert not pack(16, 3, 3, 0, kh, kw, F32, F32, 16, None) and b"3x3" in err()
    for src, dst in ((F16, F32), (2, F32), (F32, 2), (-1, F16)):
        assert not pack(16, 3, 3, 0, 3, 3, src, dst, 16, None) and b"fp32 -> fp32, fp32 -> fp16 or fp16 -> fp16" in err()
    for src, dst in ((F32, F32), (F32, F16), (F16, F16)):
        assert not pack(None, 3, 3, 0, 3, 3, src, dst, 16, None) and b"null" in err()
        assert not pack(16, 3, 3, 0, 3, 3, src, dst, None, None) and b"null" in err()
        assert not pack(16, 3, 3, 0, 3, 3, src, dst, 24, None) and b"16-byte" in err()
        assert not pack(16, 0, 3, 0, 3, 3, src, dst, 16, None) and b"bad size" in err()
        assert not pack(16, 3, 0, 3, 3, 3, src, dst, 16, None) and b"bad size" in err()
        assert not pack(16, 3, 3, -1, 3, 3, src, dst, 16, None) and b"bad size" in err()
        assert not pack(16, 32768, 4096, 4096, 3, 3, src, dst, 16, None) and b"2^31" in err()
    # forward(a, b, packed, scale, shift, residual, relu, out, dtype, N, Ca, Cb, O, H, W, stream)
    for dt in (F32, F16):
        assert not fwd(None, None, 16, None, None, None, 1, 16, dt, 1, 3, 0, 3, 2, 2, None) and b"null" in err()
        assert not fwd(16, None, None, None, None, None, 1, 16, dt, 1, 3, 0, 3, 2, 2, None) and b"null" in err()
        assert not fwd(16, None, 16, None, None, None, 1, None, dt, 1, 3, 0, 3, 2, 2, None) and b"null" in err()
        assert not fwd(16, 16, 16, None, None, None, 1, 16, dt, 1, 3, 0, 3, 2, 2, None) and b"Cb = 0" in err()
        assert not fwd(16, None, 16, None, None, None, 1, 16, dt, 1, 3, 2, 3, 2, 2, None) and b"no second map" in err()
        assert not fwd(16, None, 24, None, None, None, 1, 16, dt, 1, 3, 0, 3, 2, 2, None) and b"16-byte" in err()
        assert not fwd(16, None, 16, 16, None, None, 1, 16, dt, 1, 3, 0, 3, 2, 2, None) and b"together" in err()
        assert not fwd(16, None, 16, None, 16, None, 1, 16, dt, 1, 3, 0, 3, 2, 2, None) and b"together" in err()
        assert not fwd(16, None, 16, None, None, None, 1, 16, dt, 2 ** 7, 2 ** 8, 0, 1, 2 ** 8, 2 ** 8, None) and b"2^31" in err()      # a
        assert not fwd(16, 16, 16, None, None, None, 1, 16, dt, 2 ** 7, 1, 2 ** 8, 1, 2 ** 8, 2 ** 8, None) and b"2^31" in err()       # b
        assert not fwd(16, None, 16, None, None, None, 1, 16, dt, 2 ** 7, 1, 0, 2 ** 8, 2 ** 8, 2 ** 8, None) and b"2^31" in err()      # out
        for shape in ((0, 3, 0, 3, 2, 2), (1, 0, 0, 3, 2, 2), (1, 3, -1, 3, 2, 2), (1, 3, 0, 0, 2, 2), (1, 3, 0, 3, 0, 2), (1, 3, 0, 3, 2, 0)):
            assert not fwd(16, None, 16, None, None, None, 1, 16, dt, *shape, None) and b"bad s" in err()
    assert not fwd(16, None, 16, None, None, None, 1, 16, 2, 1, 3, 0, 3, 2, 2, None) and b"fp32 or fp16" in err()


def test_python_refusals():
    w, bn = torch.zeros(4, 6, 3, 3), torch.nn.BatchNorm2d(4).eval()
    for dt in (torch.bfloat16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="fp32 or fp16"):
            pack_conv3x3(w, dtype=dt)
    for bad in (torch.zeros(4, 6, 5, 5), torch.zeros(4, 6, 3), torch.zeros(0, 6, 3, 3), [w]):
        with pytest.raises(ValueError, match=r"\[O,C,3,3\]"):
            pack_conv3x3(bad)
    for bad, dt in ((w.half(), torch.float32), (w.double(), torch.float16), (w.bfloat16(), torch.float16)):
        with pytest.raises(ValueError, match="fp32"):
            pack_conv3x3(bad, dtype=dt)
    for split in (0, 7, -1):
        with pytest.raises(ValueError, match="split"):
            pack_conv3x3(w, split=split)
    with pytest.raises(ValueError, match="batchnorm"):
        pack_conv3x3(w, torch.nn.BatchNorm2d(5))
    with pytest.raises(ValueError, match="batchnorm"):
        pack_conv3x3(w, torch.nn.BatchNorm2d(4, track_running_stats=False))
    for dt, ww in ((torch.float32, w), (torch.float16, w), (torch.float16, w.half())):      # past the checks: refused as CPU tensors
        with pytest.raises(RuntimeError, match="ROCm device"):
            pack_conv3x3(ww, bn, 2, dtype=dt)

    def pack(dtype=torch.float32, split=None):
        return UpconvPack(None, None, None, (4,), 6, 0, (w,), dtype, split)

    assert pack().split is None and pack(split=2).split == 2 and not pack().stale() and pack().made_from([w])
    a, side, res = torch.zeros(2, 6, 3, 5), torch.zeros(2, 4, 3, 5), torch.zeros(2, 4, 3, 5)
    with torch.no_grad():
        with pytest.raises(ValueError, match="pack_conv3x3"):
            conv3x3_bn_act(a, (w,))
        with pytest.raises(ValueError, match="pack_conv3x3"):
            conv3x3_bn_act(a, UpconvPack(None, None, None, (2, 2), 6, 0, (w,)))
        with pytest.raises(ValueError, match=r"a is torch.float16.*torch.float32"):
            conv3x3_bn_act(a.half(), pack())
        with pytest.raises(ValueError, match=r"a is torch.float32.*torch.float16"):
            conv3x3_bn_act(a, pack(torch.float16))
        with pytest.raises(ValueError, match=r"a is torch.bfloat16"):
            conv3x3_bn_act(a.bfloat16(), pack())
        with pytest.raises(ValueError, match=r"side is torch.float16"):
            conv3x3_bn_act(a[:, :2], pack(split=2), side.half())
        with pytest.raises(ValueError, match=r"residual is torch.float32"):
            conv3x3_bn_act(a.half(), pack(torch.float16), residual=res)
        with pytest.raises(ValueError, match="a has 5 channels, the pack takes 6"):
            conv3x3_bn_act(a[:, :5], pack())
        with pytest.raises(ValueError, match="a has 6 channels, the pack takes 2"):
            conv3x3_bn_act(a, pack(split=2), side)
        with pytest.raises(ValueError, match="side has 3 channels, the pack takes 4"):
            conv3x3_bn_act(a[:, :2], pack(split=2), side[:, :3])
        with pytest.raises(ValueError, match="residual has 3 channels, the pack takes 4"):
            conv3x3_bn_act(a, pack(), residual=res[:, :3])
        with pytest.raises(ValueError, match="needs a side"):
            conv3x3_bn_act(a[:, :2], pack(split=2))
        with pytest.raises(ValueError, match="without a split"):
            conv3x3_bn_act(a, pack(), side)
        with pytest.raises(ValueError, match=r"side must be \(2, 4, 3, 5\)"):
            conv3x3_bn_act(a[:, :2], pack(split=2), side[:, :, :2])
        with pytest.raises(ValueError, match=r"residual must be \(2, 4, 3, 5\)"):
            conv3x3_bn_act(a, pack(), residual=res[:1])
        with pytest.raises(ValueError, match=r"\[N,C,H,W\]"):
            conv3x3_bn_act(a[0], pack())
        with pytest.raises(ValueError, match="empty"):
            conv3x3_bn_act(a[:0], pack())
        big = torch.zeros(1, 1, 1, 1).expand(2 ** 7, 6, 2 ** 11, 2 ** 11)                # 2^31 elements or more, no memory behind them
        with pytest.raises(ValueError, match="a has 2\\^31 elements"):
            conv3x3_bn_act(big, pack())
        wide = UpconvPack(None, None, None, (2 ** 12,), 1, 0, (w,))
        with pytest.raises(ValueError, match="output has 2\\^31 elements"):
            conv3x3_bn_act(torch.zeros(1, 1, 1, 1).expand(2 ** 9, 1, 2 ** 5, 2 ** 5), wide)
        for args in ((a, pack()), (a[:, :2], pack(split=2), side), (a, pack(), None, res), (a.half(), pack(torch.float16))):
            with pytest.raises(RuntimeError, match="ROCm device"):                       # past the checks: refused as CPU tensors
                conv3x3_bn_act(*args)
    with torch.enable_grad():                                                            # forward only
        with pytest.raises(RuntimeError, match="forward-only.*stock block"):
            conv3x3_bn_act(a.clone().requires_grad_(True), pack())
        with pytest.raises(RuntimeError, match="forward-only"):
            conv3x3_bn_act(a, pack(), residual=res.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="forward-only"):
            conv3x3_bn_act(a, UpconvPack(None, None, None, (4,), 6, 0, (torch.nn.Parameter(w),)))


def test_the_three_switches_select_independently():
    assert isinstance(upmod.FUSED_TAIL_DEFAULT, tuple) and set(upmod.FUSED_TAIL_DEFAULT) <= set(BLOCKS)
    assert isinstance(upmod.FUSED_TAIL_HALF_DEFAULT, tuple) and set(upmod.FUSED_TAIL_HALF_DEFAULT) <= set(BLOCKS)

    def marks(m, attr):
        return [getattr(getattr(m, n), attr) for n in BLOCKS]

    for net in (unet_ours, unet_cspn_nyu):
        m = net.resnet18()
        assert m.fused_tail == () and m.fused_decoder == () and not m.fused_heads
        assert not any(marks(m, "fused_tail") + marks(m, "fused_tail_half") + marks(m, "fused_head") + marks(m, "fused_head_half"))
        keys = list(m.state_dict())
        assert len(keys) == len(net.resnet18(fused_tail=True, fused_decoder=True, fused_heads=True).state_dict())
        m = net.resnet18(fused_tail=True)
        assert m.fused_tail == tuple(n for n in BLOCKS if n in upmod.FUSED_TAIL_DEFAULT) and m.fused_decoder == () and not m.fused_heads
        assert marks(m, "fused_tail") == [n in upmod.FUSED_TAIL_DEFAULT for n in BLOCKS]
        assert marks(m, "fused_tail_half") == [n in upmod.FUSED_TAIL_HALF_DEFAULT for n in BLOCKS]
        assert not any(marks(m, "fused_head") + marks(m, "fused_head_half")) and list(m.state_dict()) == keys
        m = net.resnet18(fused_tail=["gud_up_proj_layer3", "gud_up_proj_layer1"], fused_decoder=True)      # names: both precisions
        assert m.fused_tail == ("gud_up_proj_layer1", "gud_up_proj_layer3") and m.fused_decoder == BLOCKS
        assert marks(m, "fused_tail") == marks(m, "fused_tail_half") == [True, False, True, False] and all(marks(m, "fused_head"))
        m = net.resnet18(fused_tail="gud_up_proj_layer4", fused_heads=True)
        assert m.fused_tail == ("gud_up_proj_layer4",) and m.fused_heads and m.fused_decoder == ()
        m = net.resnet18(fused_decoder=True)                                             # ... means what it meant
        assert m.fused_tail == () and not any(marks(m, "fused_tail") + marks(m, "fused_tail_half"))
        for bad in ("gud_up_proj_layer5", ["gud_up_proj_layer1", "conv2"]):
            with pytest.raises(ValueError, match="fused_tail.*not among"):
                net.resnet18(fused_tail=bad)
        assert all(getattr(m, n)._tail_packs is None for n in BLOCKS)
        assert not [k for k in m.state_dict() if "pack" in k] and not [n for n, _ in m.named_modules() if "pack" in n]
    assert len(unet_ours.resnet50(decoder_sizes=unet_ours.decoder_sizes_for(36, 52)).state_dict()) == 417
    # which operands run which path: grad mode off, eval mode
    block = unet_ours.Gudi_UpProj_Block_Cat(5, 7, 9, 13).eval()
    x, h, d = torch.zeros(1, 7, 9, 13), torch.zeros(1, 7, 9, 13).half(), torch.zeros(1, 7, 9, 13).double()
    with torch.no_grad():
        assert not block._fuse_tail() and not block._fuse_tail(x, x, x) and not block._fuse_tail(h, h)
        block.fused_tail = True                                                          # marked by hand: half follows
        assert block._fuse_tail() and block._fuse_tail(x, x, x) and block._fuse_tail(h, h, h)
        assert not block._fuse_tail(x, h, x) and not block._fuse_tail(h, h, x)              # one dtype, or the stock lines
        assert not block._fuse_tail(d, d) and not block._fuse_tail(x.bfloat16(), x.bfloat16())
        block.fused_tail_half = False
        assert block._fuse_tail() and block._fuse_tail(x, x) and not block._fuse_tail(h, h)
        block.fused_tail, block.fused_tail_half = False, True
        assert block._fuse_tail() and not block._fuse_tail(x, x) and block._fuse_tail(h, h)
        assert not block._fuse_head(x) and not block._fuse_head(h)                        # the head goes by its own marks
    with torch.enable_grad():
        assert not block._fuse_tail() and not block._fuse_tail(h, h)
    with torch.no_grad():
        assert not block.train()._fuse_tail() and not block._fuse_tail(h, h)


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
TORCH_DT = {np.float32: torch.float32, np.float16: torch.float16}


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def packed_for(w, source_dtype, dtype, split=None):
    return pack_conv3x3(dev(w, source_dtype), None, split, dtype)


def run(pack, a, b=None, scale=None, shift=None, r=None, relu=True):
    """The kernel on `pack`'s filter with an affine map of the test's own."""
    mine = UpconvPack(pack.packed, dev(scale), dev(shift), pack.out_channels, pack.in_channels, 0, pack.sources, pack.dtype, pack.split)
    with torch.no_grad():
        out = conv3x3_bn_act(dev(a, pack.dtype), mine, dev(b, pack.dtype), dev(r, pack.dtype), relu)
    assert out.is_contiguous() and out.dtype == pack.dtype and tuple(out.shape) == (a.shape[0], pack.out_channels[0]) + a.shape[2:]
    return out


def same_bits(t, want):
    """t (device tensor) and want (numpy, fp32 or fp16): the same shape, dtype and bits."""
    got = t.detach().cpu().numpy()
    view = np.uint32 if want.dtype == np.float32 else np.uint16
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(view), want.view(view))


def integer_case(channels, O, shape):
    a, b, w, scale, shift, r = tc.make_inputs(channels, O, shape, True)
    split = channels[0] if channels[1] else None
    p32 = packed_for(w, torch.float32, torch.float32, split)
    p16 = [packed_for(w, torch.float32, torch.float16, split), packed_for(w, torch.float16, torch.float16, split)]
    assert p16[0].packed.dtype == torch.float16 and torch.equal(p16[0].packed, p16[1].packed)
    lib = _lib.lib()
    assert p32.packed.numel() * 4 == lib.cspn_uptail_packed_bytes(O, *channels, F32)
    assert p16[0].packed.numel() * 2 == lib.cspn_uptail_packed_bytes(O, *channels, F16)
    acc = tc.accumulate(a.astype(np.float64), None if b is None else b.astype(np.float64), w.astype(np.float64))
    for res, relu, affine in tc.EPILOGUES:
        args = (scale if affine else None, shift if affine else None, r if res else None, relu)
        exact = tc.epilogue(acc, *args)
        what = (channels, O, shape, res, relu, affine)
        assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact), what          # the fp64 values are fp32 values
        assert same_bits(run(p32, a, b, *args), exact.astype(np.float32)), what
        for pack in p16:
            assert same_bits(run(pack, a, b, *args), exact.astype(np.float16)), what


@pytest.mark.gpu
@pytest.mark.parametrize("shape", tc.SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_integer_cases_bit_equal_to_the_restatement(shape):
    for channels, O, _ in tc.integer_cases(shape):
        integer_case(channels, O, shape)


@pytest.mark.gpu
def test_integer_case_over_several_chunks_and_tiles():
    channels, O, shape = tc.BIG["channels"], tc.BIG["O"], tc.BIG["shape"]
    assert min(channels) > 32 and shape[0] * shape[1] * shape[2] > 3 * 128
    integer_case(channels, O, shape)


def check_within_bound(what, got, want, bound):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and got.shape == want.shape
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print("%s: largest error / bound = %.4f" % (what, ratio))
    assert (err <= bound).all(), (what, ratio)
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("channels,O,shape", tc.REAL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_real_cases_within_the_a_priori_bound(channels, O, shape):
    a, b, w, scale, shift, r = tc.make_inputs(channels, O, shape, False)
    split = channels[0] if channels[1] else None
    p32, p16 = packed_for(w, torch.float32, torch.float32, split), packed_for(w, torch.float32, torch.float16, split)
    assert torch.equal(p16.packed, packed_for(tc.to_half(w), torch.float16, torch.float16, split).packed)      # rounded to nearest even, once
    moved = 0
    for res, relu, affine in tc.EPILOGUES:
        args = (scale if affine else None, shift if affine else None, r if res else None)
        what = "%s O=%d %s res=%d relu=%d affine=%d" % (channels, O, shape, res, relu, affine)
        want = tc.restate(a, b, w, *args, relu)
        got = run(p32, a, b, *args, relu)
        check_within_bound("fp32 " + what, got, want, tc.bound(a, b, w, *args))
        moved += int((got.cpu().numpy().astype(np.float64) != want).sum())
        want = tc.restate_half(a, b, w, *args, relu)[1]
        assert np.abs(want).max() < tc.HALF_MAX
        check_within_bound("fp16 " + what, run(p16, a, b, *args, relu), want, tc.bound_half(a, b, w, *args, relu))
    assert moved > 0                                                         # rounded results, not a copy of the fp64 ones


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_chained_within_the_composed_bound(name):
    """Both calls of the tail chained on the device, each fed the previous device result, against the stored block output.  The
    composed bound of a step, with f the step on the stored fp64 parameters, f_r the step on the operands the device is given (its
    input x, the filter, side and residual rounded to the precision, scale and shift to fp32), both in exact arithmetic, and x* the
    stored input:  |got - f(x*)| <= |got - f_r(x)| + |f_r(x) - f(x)| + |f(x) - f(x*)|
        the a-priori bound of the kernel  +  a difference of two fp64 restatements  +  |scale| sum |w| |x - x*|,
    the last with |x - x*| bounded by the previous step's composed bound (the first step's x is x* rounded: it goes into the second
    term).  Half runs only where every stored value lies in the fp16 range."""
    z = load_golden(name)
    steps = golden_steps(z)
    fits = all(np.abs(t).max() < tc.HALF_MAX for s in steps for t in s if t is not None)
    assert fits or "_int_" in name
    for dtype, np_dt in ((torch.float32, np.float32),) + (((torch.float16, np.float16),) if fits else ()):
        carried, got = None, None
        for a, side, w, scale, shift, r, want in steps:
            x = a.astype(np_dt) if got is None else got.cpu().numpy()                       # what the device is given
            given = [None if t is None else t.astype(np_dt).astype(np.float64) for t in (x, side, w)] + \
                [scale.astype(np.float32).astype(np.float64), shift.astype(np.float32).astype(np.float64), None if r is None else r.astype(np_dt).astype(np.float64)]
            got = run(packed_for(w, torch.float32, dtype, None if side is None else a.shape[1]), x, side, scale.astype(np.float32),
                      shift.astype(np.float32), r, True)
            own = tc.bound(*given) if dtype == torch.float32 else tc.bound_half(*given, True)
            exact_on_x = want if carried is None else tc.restate(given[0], side, w, scale, shift, r, True)
            own = own + np.abs(tc.restate(*given, True) - exact_on_x)
            if carried is not None:
                own = own + tc._terms(carried, None, w, scale, None, None)
            check_within_bound("%s %s" % (name, dtype), got, want, own + 1e-300)
            carried = own
        assert got.dtype == dtype


@pytest.mark.gpu
def test_batch_place_and_determinism():
    channels, O, shape = (33, 40), 129, (3, 7, 9)
    a, b, w, scale, shift, r = tc.make_inputs(channels, O, shape, False)
    for dtype in (torch.float32, torch.float16):
        pack = packed_for(w, torch.float32, dtype, channels[0])
        ys = run(pack, a, b, scale, shift, r)
        assert torch.equal(ys, run(pack, a, b, scale, shift, r))                           # two runs of one call
        for n in (0, 2):                                                                  # frame n of B = 3 at position 0 of B = 1
            alone = run(pack, a[n:n + 1], b[n:n + 1], scale, shift, r[n:n + 1])
            assert torch.equal(alone[0], ys[n])
        pair = run(pack, a[1:3], b[1:3], scale, shift, r[1:3])                             # ... and at position 1 of B = 2: other tiles again
        assert torch.equal(pair[1], ys[2])


@pytest.mark.gpu
@pytest.mark.parametrize("channels,O,shape", [((33, 40), 129, (3, 7, 9)), ((3, 0), 33, (2, 5, 7)), ((1, 1), 1, (1, 1, 1))], ids=["ragged", "one_map", "one_px"])
def test_nothing_outside_the_output_is_written(channels, O, shape):
    a, b, w, scale, shift, r = tc.make_inputs(channels, O, shape, True)
    for dtype in (torch.float32, torch.float16):
        pack = packed_for(w, torch.float32, dtype, channels[0] if channels[1] else None)
        want = run(pack, a, b, scale, shift, r)
        pad, sentinel, size = 4096, -12288.0, want.numel()                               # a fp16 value no case produces in the band
        buf = torch.full((2 * pad + size,), sentinel, device=DEV, dtype=dtype)
        out = buf[pad:pad + size].view(want.shape)
        ad, bd, rd, sd, hd = dev(a, dtype), dev(b, dtype), dev(r, dtype), dev(scale), dev(shift)
        launch(torch.device(DEV), "cspn_uptail_forward", ad.data_ptr(), None if bd is None else bd.data_ptr(), pack.packed.data_ptr(),
               sd.data_ptr(), hd.data_ptr(), rd.data_ptr(), 1, out.data_ptr(), _lib.CSPN_F32 if dtype == torch.float32 else _lib.CSPN_F16,
               shape[0], channels[0], channels[1], O, shape[1], shape[2])
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + size:] == sentinel).all())


@pytest.mark.gpu
def test_ragged_case_under_poisoned_lds():
    """The ragged case above — two maps of 33 and 40 channels, a second M tile with one live row — with NaN in the whole LDS of
    every CU in front of every launch: the bits of the plain run, in both precisions."""
    channels, O, shape = (33, 40), 129, (3, 7, 9)
    a, b, w, scale, shift, r = tc.make_inputs(channels, O, shape, True)
    for dtype, pattern in ((torch.float32, 0x7fc00000), (torch.float16, 0x7fc07fc0)):      # NaN as fp32, and in both fp16 halves
        pack = packed_for(w, torch.float32, dtype, channels[0])
        plain = run(pack, a, b, scale, shift, r)
        with lds_poison(pattern):
            got = run(pack, a, b, scale, shift, r)
            torch.cuda.synchronize()
        assert torch.equal(got, plain) and not bool(torch.isnan(got).any())


@pytest.mark.gpu
def test_nan_reaches_exactly_its_neighbourhood():
    """a[1,2,3,4] = NaN poisons the outputs of frame 1 at rows 2..4, columns 3..5, in every channel, and nothing else; the same for
    a NaN in the second map at a corner."""
    channels, O, shape = (3, 5), 3, (2, 5, 7)
    a, b, w, scale, shift, r = (None if t is None else t.copy() for t in tc.make_inputs(channels, O, shape, False))
    for dtype in (torch.float32, torch.float16):
        pack = packed_for(w, torch.float32, dtype, 3)
        clean = run(pack, a, b, scale, shift, r)
        for which, at, rows, cols in ((0, (1, 2, 3, 4), range(2, 5), range(3, 6)), (1, (0, 4, 0, 6), range(0, 2), range(5, 7))):
            an, bn = a.copy(), b.copy()
            (an, bn)[which][at] = np.nan
            y = run(pack, an, bn, scale, shift, r)
            nan = torch.isnan(y)
            assert not bool(nan[1 - at[0]].any())
            assert np.array_equal(np.argwhere(nan[at[0]].all(0).cpu().numpy()), [[i, j] for i in rows for j in cols])
            assert int(nan[at[0]].any(0).sum()) == len(rows) * len(cols)
            assert torch.equal(y[~nan], clean[~nan])


@pytest.mark.gpu
def test_graph_capture_of_pack_and_forward_gives_the_eager_bits():
    """Forward only, under no_grad: pack-then-forward of both tail steps captured once, replayed on new input values."""
    channels, O, shape = tc.BIG["channels"], tc.BIG["O"], tc.BIG["shape"]
    a, b, w, scale, shift, r = tc.make_inputs(channels, O, shape, False)
    a2 = tc.make_inputs(channels, O + 1, shape, False)[0]
    for dtype in (torch.float32, torch.float16):
        weight = torch.nn.Parameter(dev(w))
        bn = torch.nn.BatchNorm2d(O).to(DEV).eval()
        with torch.no_grad():
            bn.running_mean.copy_(dev(shift))
            bn.weight.copy_(dev(scale))
            bd, rd = dev(b, dtype), dev(r, dtype)

            def pack_and_forward(v):
                return conv3x3_bn_act(v, pack_conv3x3(weight, bn, channels[0], dtype), bd, rd)

            eager = [pack_and_forward(dev(v, dtype)) for v in (a, a2)]
            sx = dev(a, dtype)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                pack_and_forward(sx)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = pack_and_forward(sx)
            for v, want in ((a2, eager[1]), (a, eager[0])):                              # two replays, on new input values
                sx.copy_(dev(v, dtype))
                out.fill_(7.0)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, want)
        assert out.dtype == dtype and not torch.equal(eager[0], eager[1])


class Recorder(object):
    """Stands in for conv3x3_bn_act and for launch inside network.up_pooling: keeps what went into and came out of every fused tail
    step, and the name of every native entry point that was called with the dtype code the tail's were given."""

    def __init__(self, monkeypatch):
        self.calls, self.entries, self.real, self.real_launch = [], [], upmod.conv3x3_bn_act, upmod.launch
        monkeypatch.setattr(upmod, "conv3x3_bn_act", self)
        monkeypatch.setattr(upmod, "launch", self.launch)

    def __call__(self, a, pack, side=None, residual=None, relu=True):
        out = self.real(a, pack, side, residual, relu)
        self.calls.append((a.detach().clone(), pack, None if side is None else side.detach().clone(),
                           None if residual is None else residual.detach().clone(), relu, out.detach().clone()))
        return out

    def launch(self, device, name, *args):
        if "uptail" in name:
            self.entries.append((name, args[7] if name.endswith("pack") else args[8]))      # dst_dtype / dtype
        return self.real_launch(device, name, *args)

    def clear(self):
        del self.calls[:], self.entries[:]


def model_case(kind, seed=11, **switches):
    """tests/test_uphalf.py's model: resnet18 of either network at 36 x 52, B = 2, batch norms with statistics that are not the
    initial ones."""
    torch.manual_seed(seed)
    sizes = unet_ours.decoder_sizes_for(36, 52)
    if kind == "ours":
        net = unet_ours.resnet18(decoder_sizes=sizes, prop_time=2, **switches)
    else:
        net = unet_cspn_nyu.resnet18(decoder_sizes=sizes, prop_time=2, reference_state_dict=False, **switches)
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


def run_model(net, inp, how):
    with torch.no_grad():
        if how == "autocast":
            with torch.autocast(device_type="cuda", dtype=torch.float16):
                return net.features(inp)
        return net.features(inp.to(next(net.parameters()).dtype))


TAIL_CALLS = 1 + 2 * 3                  # gud_up_proj_layer1 is the plain block, 2 .. 4 are _Cat blocks


def expected_entries(code, packs=True):
    step = ([("cspn_uptail_pack", code)] if packs else []) + [("cspn_uptail_forward", code)]
    return step * TAIL_CALLS


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", [False, True], ids=["tail_alone", "with_fused_decoder"])
@pytest.mark.parametrize("how", ["fp32", "autocast", "half"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_models_fused_tails_within_the_bound(kind, how, decoder, monkeypatch):
    net, inp = model_case(kind, fused_tail=BLOCKS, fused_decoder=BLOCKS if decoder else False)
    net.eval()
    keys = list(net.state_dict())
    if how == "half":
        net.half()
    rec = Recorder(monkeypatch)
    run_model(net, inp, how)
    dtype, code = (torch.float32, F32) if how == "fp32" else (torch.float16, F16)
    assert len(rec.calls) == TAIL_CALLS and rec.entries == expected_entries(code)
    assert all((getattr(net, n)._upconv_pack is not None) == decoder for n in BLOCKS) and list(net.state_dict()) == keys
    calls = iter(rec.calls)
    for name in BLOCKS:
        block = getattr(net, name)
        cat = hasattr(block, "conv1_1")
        assert sorted(block._tail_packs) == (["conv1_1", "conv2"] if cat else ["conv2"])
        for conv, bn in ((("conv1_1", "bn1_1"),) if cat else ()) + (("conv2", "bn2"),):
            a, pack, side, residual, relu, out = next(calls)
            first = conv == "conv1_1"
            assert pack is block._tail_packs[conv] and not pack.stale() and pack.dtype == dtype and relu is True
            assert all(t is None or t.dtype == dtype for t in (a, side, residual, out))
            assert (side is not None) == first == (residual is None) and pack.split == (a.shape[1] if first else None)
            conv, bn = getattr(block, conv), getattr(block, bn)
            assert conv.weight.dtype == (torch.float16 if how == "half" else torch.float32)
            w = conv.weight.detach().float().cpu().numpy()
            scale, shift = tc.fold(*(t.detach().float().cpu().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)), bn.eps)
            args = tuple(None if t is None else t.float().cpu().numpy() for t in (a, side)) + (w, scale, shift,
                                                                                              None if residual is None else residual.float().cpu().numpy())
            what = "%s %s %s %s" % (kind, how, name, "conv1_1" if first else "conv2")
            if dtype == torch.float32:
                check_within_bound(what, out, tc.restate(*args, True), tc.bound(*args, extra=4))
            else:
                check_within_bound(what, out, tc.restate_half(*args, True)[1], tc.bound_half(*args, True, extra=4))
            assert float(out.min()) == 0.0 and float(out.max()) > 0.0
    rec.clear()
    run_model(net, inp, how)                                                  # a second forward packs nothing again
    assert rec.entries == expected_entries(code, packs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_modes_dtypes_and_repacking(kind, monkeypatch):
    net, inp = model_case(kind, fused_tail=BLOCKS)
    net.eval()
    rec = Recorder(monkeypatch)
    run_model(net, inp, "fp32")
    assert rec.entries == expected_entries(F32) and all(c[0].dtype == torch.float32 for c in rec.calls)
    first = run_model(net, inp, "fp32")
    rec.clear()
    run_model(net, inp, "autocast")                                          # the same model under autocast: repacked for half
    assert rec.entries == expected_entries(F16) and all(c[1].dtype == torch.float16 for c in rec.calls)
    rec.clear()
    run_model(net, inp, "fp32")                                              # ... and back
    assert rec.entries == expected_entries(F32)
    rec.clear()
    with torch.enable_grad():                                                # grad mode on: the stock lines
        net.features(inp)
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            net.features(inp)
    assert rec.calls == [] and rec.entries == []
    net.train()                                                              # train mode: the stock lines, and no pack is kept
    assert all(getattr(net, n)._tail_packs is None for n in BLOCKS)
    run_model(net, inp, "fp32")
    run_model(net, inp, "autocast")
    assert rec.calls == [] and rec.entries == []
    net.eval()
    other = model_case(kind, seed=13)[0]                                     # other weights: written in place, every pack is stale
    run_model(net, inp, "fp32")
    rec.clear()
    net.load_state_dict(other.state_dict())
    assert all(p.stale() for n in BLOCKS for p in getattr(net, n)._tail_packs.values())
    second = run_model(net, inp, "fp32")
    assert rec.entries == expected_entries(F32)
    want = run_model(other.eval(), inp, "fp32")
    assert not torch.equal(first[0], second[0])
    assert all(float((g - w).abs().max()) <= 1e-3 * float(w.abs().max()) for g, w in zip(second[:2], want[:2]))      # the stock model on those weights
    rec.clear()
    upmod.select_fused_tail(net, True)                                       # True: each precision takes its measured selection
    run_model(net, inp, "fp32")
    assert len(rec.calls) == sum(2 if n != BLOCKS[0] else 1 for n in upmod.FUSED_TAIL_DEFAULT)
    rec.clear()
    run_model(net, inp, "autocast")
    assert len(rec.calls) == sum(2 if n != BLOCKS[0] else 1 for n in upmod.FUSED_TAIL_HALF_DEFAULT)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["autocast", "half"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_end_to_end_no_worse_than_the_stock_half_model(kind, how):
    """tests/test_uphalf.py's yardstick: on the same inputs and weights, the distance of the half model with fused tails from the
    stock fp32 model is at most 1.5 times the distance of the stock half model from it (blur depth and guidance, each over the fp32
    output's range).  The fused tail rounds once where the stock path rounds after the convolution, the batch norm and the add; the
    factor covers that both distances are single samples of rounding noise."""
    net, inp = model_case(kind)
    net.eval()
    ref = run_model(net, inp, "fp32")[:2]
    if how == "half":
        net.half()
    stock = run_model(net, inp, how)[:2]
    upmod.select_fused_tail(net, BLOCKS)
    fused = run_model(net, inp, how)[:2]
    assert all(p.dtype == torch.float16 for n in BLOCKS for p in getattr(net, n)._tail_packs.values())

    def distance(outs):
        return max(float((o.float() - r).abs().max() / (r.max() - r.min())) for o, r in zip(outs, ref))

    d_stock, d_fused = distance(stock), distance(fused)
    print("%s %s: d_stock = %.3e, d_fused = %.3e" % (kind, how, d_stock, d_fused))
    assert all(o.dtype == torch.float16 for o in stock + fused) and 0 < d_stock
    assert d_fused <= 1.5 * d_stock, (d_fused, d_stock)

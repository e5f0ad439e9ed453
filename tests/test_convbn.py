"""The fused convolutions of the encoder: the `convbn` family of the native library (include/cspn_convbn.h),
network.conv_bn.pack_conv_bn / conv_bn_act, and the `fused_encoder` switch of the two models.

References: the numpy restatement of tests/convbn_cases.py (fp64; for half on inputs rounded to fp16 and rounded once to fp16) and the
goldens G30 (the reference's encoder blocks and bridge in fp64).  Integer-valued cases are compared bit for bit; real-valued cases
against the a-priori bounds of convbn_cases.bound / bound_half (the module's docstring says where every term comes from)."""
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import convbn_cases as cc
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd._host import launch
from cspn_monodepth_amd.network import conv_bn as cb
from cspn_monodepth_amd.network import unet_cspn_nyu, unet_ours
from cspn_monodepth_amd.network import up_pooling as upmod
from cspn_monodepth_amd.network.conv_bn import ConvBnPack, conv_bn_act, pack_conv_bn
from cspn_monodepth_amd.network.up_pooling import conv3x3_bn_act, pack_conv3x3

DEV = "cuda:0"
GOLDENS = golden_names("g30_convbn_")
STAGES = cb.ENCODER_STAGES
NAMES = ("cspn_convbn_abi_version", "cspn_convbn_packed_bytes", "cspn_convbn_pack", "cspn_convbn_forward")
F32, F16 = _lib.CSPN_F32, _lib.CSPN_F16


def close(got, want, integer):
    return np.array_equal(got, want) if integer else np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_goldens_are_the_manifest():
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "g30_convbn_manifest.json")))
    assert sorted(manifest["files"]) == GOLDENS == sorted("g30_convbn_" + n for n in cc.GOLDEN_CASES) and len(GOLDENS) == 10
    for name, row in manifest["files"].items():
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) == row["bytes"] <= 131072
    rows = manifest["files"].values()
    assert {(r["block"], r["downsample"], r["stride"]) for r in rows} == {
        ("Bottleneck", False, 1), ("Bottleneck", True, 2), ("BasicBlock", False, 1), ("BasicBlock", True, 2), ("bridge", False, 1)}
    assert {r["integer"] for r in rows} == {True, False}
    assert any(r["x"][2] % 2 and r["x"][3] % 2 and r["stride"] == 2 for r in rows)          # odd H and W under stride 2


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_composed_per_block_reproduces_the_golden(name):
    z = load_golden(name)
    integer = "_int_" in name
    steps = cc.block_steps(z)
    kind, down = str(z["kind"]), "w_downsample" in z
    assert len(steps) == {"bridge": 1, "BasicBlock": 2, "Bottleneck": 3}[kind] + int(down)
    for bn in (k for k in z if k.startswith("bn_")):                                      # not the initial statistics and parameters
        g, b, m, v = z[bn]
        assert not np.array_equal(g, np.ones_like(g)) and b.any() and m.any() and not np.array_equal(v, np.ones_like(v))
    for src, w, s, scale, shift, res, relu, dst in steps:
        got = cc.restate(z[src], w, s, scale, shift, None if res is None else z[res], relu)
        assert got.dtype == np.float64 and got.shape == z[dst].shape and close(got, z[dst], integer), dst
    if kind != "bridge":
        src, w, s, scale, shift, res, relu, dst = steps[-1]
        assert relu and not close(cc.restate(z[src], w, s, scale, shift, z[res], False), z[dst], integer)      # the ReLU matters


@pytest.mark.parametrize("k,s", cc.KS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_equals_conv2d(shape, k, s):
    """At every shape the GPU tests run: torch's fp64 conv2d(stride=s, padding=k // 2), exactly on the integer-valued inputs and to
    1e-12 on the real-valued ones — and every integer-valued row is exact in the kernel's arithmetic: sums below 2^24, and every
    result of the eight epilogues a fp16 value."""
    cases = cc.integer_cases(shape, k, s)
    if shape == cc.SHAPES[0]:
        cases += [c for c in cc.EXTRA_INTEGER_CASES if c[3:] == (k, s)]                     # the further cases, once
    reals = [(C, O, sh, k, s) for C, O, sh in cc.REAL_CASES if sh == shape or (shape == cc.SHAPES[0] and sh == cc.BIG["shape"])]
    for integer, rows in ((True, cases), (False, reals)):
        for C, O, sh, kk, ss in rows:
            x, w, scale, shift, r = cc.make_inputs(C, O, sh, kk, ss, integer)
            want = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), stride=ss, padding=kk // 2).numpy()
            assert want.shape == (sh[0], O, cc.out_size(sh[1], ss), cc.out_size(sh[2], ss)) == r.shape
            acc = cc.accumulate(x.astype(np.float64), w.astype(np.float64), ss)
            assert close(acc, want, integer), (C, O, sh, kk, ss)
            full = want * scale[None, :, None, None].astype(np.float64) + shift[None, :, None, None] + r
            assert close(cc.restate(x, w, ss, scale, shift, r, True), np.maximum(full, 0), integer)
            if integer:
                worst = cc.accumulate(np.abs(x).astype(np.float64), np.abs(w).astype(np.float64), ss).max()      # every partial sum lies below it
                assert worst < 2 ** 24 and all(np.array_equal(cc.to_half(t), t) for t in (x, w, r, scale, shift))
                for res, relu, affine in cc.EPILOGUES:
                    exact = cc.epilogue(acc, scale if affine else None, shift if affine else None, r if res else None, relu)
                    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
                    assert np.array_equal(exact.astype(np.float16).astype(np.float64), exact), (C, O, sh, kk, ss, res, relu, affine)


def test_convbn_family_contract():
    """Header, loader table and library agree on the family, in the terms tests/test_uptail.py uses for `uptail`; the family sits in
    a further part of the table, and the tuples and digests the older tests restate are what they were."""
    fam = _lib.family("convbn")
    assert fam.header == os.path.join(ROOT, "include", "cspn_convbn.h") and fam.files == {"cspn_convbn.hip": False} and fam.opt_in
    text = open(fam.header).read()
    assert re.search(r"^#define CSPN_CONVBN_ABI_VERSION 1$", text, flags=re.M)
    declared = sorted(set(re.findall(r"\b(cspn\w*)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(fam.functions) == sorted(NAMES)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in NAMES) and lib.cspn_convbn_abi_version() == fam.abi_version == 1
    for n in NAMES:                                                                        # the signatures lib() set
        fn, (restype, argtypes) = getattr(lib, n), fam.functions[n]
        assert (fn.argtypes is None and argtypes is None) or list(fn.argtypes) == list(argtypes)
        assert fn.restype is restype
    assert len(fam.functions["cspn_convbn_forward"][1]) == 16 and len(fam.functions["cspn_convbn_pack"][1]) == 9
    # a further part of the table, behind the thirteen
    assert _lib.LATER_FAMILIES == (fam,) and _lib.EVERY_FAMILY == _lib.ALL_FAMILIES + _lib.LATER_FAMILIES
    assert fam not in _lib.ALL_FAMILIES and fam not in _lib.FAMILIES and fam not in _lib.OPT_IN_FAMILIES
    assert [f.name for f in _lib.OPT_IN_FAMILIES] == ["heads", "upconv", "uphalf", "uptail"]
    assert _lib.ALL_FAMILIES == _lib.FAMILIES + _lib.OPT_IN_FAMILIES and len(_lib.FAMILIES) == 9 and len(_lib.ALL_FAMILIES) == 13
    assert _lib.family("uptail").files == {"cspn_uptail.hip": False}
    assert _lib.LATER_SOURCES == ("cspn_convbn.hip",) and _lib.LATER_HEADERS == (fam.header,)
    assert "cspn_convbn.hip" not in _lib.SOURCES + _lib.OPT_IN_SOURCES and os.path.exists(os.path.join(_lib.CSRC, "cspn_convbn.hip"))
    assert fam.header not in _lib.BUILD_HEADERS and fam.header not in _lib.HEADERS
    assert len([p for p in _lib.BUILD_HEADERS if os.path.dirname(p) == _lib.CSRC]) == 6          # no new header under csrc/
    # no existing family's name or prefix in the new names, and the new name in no other family's
    for other in _lib.ALL_FAMILIES:
        assert not set(other.functions) & set(NAMES) and not any("convbn" in n for n in other.functions)
    words = ("upconv", "uphalf", "uptail", "heads", "criterion", "max8", "abn", "sparsify", "transform", "losses", "berhu", "mean_loss",
             "optim", "sgd", "visual")
    assert not any(w in n for w in words for n in NAMES)
    # _source_digest and code_digest() are composed as they were ...
    import hashlib
    plain = hashlib.sha256(b"x")
    for path in [os.path.join(_lib.CSRC, f) for f in _lib.SOURCES + _lib.OPT_IN_SOURCES] + list(_lib.BUILD_HEADERS):
        plain.update(open(path, "rb").read())
    assert _lib._source_digest(["x"]) == plain.hexdigest()
    # ... and the build's stamp carries that digest on over the new source and header: an edit to either is another stamp
    stamp = hashlib.sha256(plain.hexdigest().encode())
    for path in (os.path.join(_lib.CSRC, "cspn_convbn.hip"), fam.header):
        stamp.update(open(path, "rb").read())
    assert _lib._later_digest(plain.hexdigest()) == stamp.hexdigest() != plain.hexdigest()
    for drop in (0, 1):
        less = hashlib.sha256(plain.hexdigest().encode())
        less.update(open((os.path.join(_lib.CSRC, "cspn_convbn.hip"), fam.header)[1 - drop], "rb").read())
        assert less.hexdigest() != stamp.hexdigest()
    assert "_later_digest(_source_digest(" in inspect.getsource(_lib.build)                # what build() writes next to the library
    assert open(_lib.SO_PATH + ".hash").read().strip() == _lib._later_digest(_lib._source_digest(
        ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize"] + os.environ.get("CSPN_HIPCC_FLAGS", "").split()))
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
        assert sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and "convbn" in ln) == declared


def test_packed_bytes_by_hand():
    pb = _lib.lib().cspn_convbn_packed_bytes
    assert pb(6, 3, 3, F32) == 9 * 32 * 128 * 4 and pb(129, 33, 3, F16) == 9 * 64 * 256 * 2
    assert pb(6, 3, 1, F32) == 32 * 128 * 4 and pb(129, 33, 1, F16) == 64 * 256 * 2
    assert pb(2048, 2048, 3, F32) == 9 * 2048 * 2048 * 4 and pb(64, 64, 1, F16) == 64 * 128 * 2
    for bad in ((0, 3, 3, F32), (3, 0, 3, F32), (-1, 3, 1, F16), (3, -1, 1, F16), (3, 3, 0, F32), (3, 3, 2, F32), (3, 3, 5, F16), (3, 3, -1, F32),
                (3, 3, 3, 2), (3, 3, 3, -1), (2 ** 24 + 1, 1, 1, F32), (1, 2 ** 24 + 1, 1, F32),
                (2 ** 14, 2 ** 14, 3, F32), (2 ** 16, 2 ** 15, 1, F16)):                  # the last two: 2^31 packed elements or more
        assert pb(*bad) == 0, bad
    assert pb(2 ** 15, 2 ** 15, 1, F16) == 2 ** 31                                         # 2^30 elements: the largest power of two


def test_argument_checks_come_before_any_launch():
    lib = _lib.lib()
    err, pack, fwd = lib.cspn_last_error, lib.cspn_convbn_pack, lib.cspn_convbn_forward
    for kh, kw in ((5, 5), (3, 1), (1, 3), (2, 2), (0, 0)):
        assert not pack(16, 3, 3, kh, kw, F32, F32, 16, None) and b"1x1 or 3x3" in err()
    for src, dst in ((F16, F32), (2, F32), (F32, 2), (-1, F16)):
        assert not pack(16, 3, 3, 3, 3, src, dst, 16, None) and b"fp32 -> fp32, fp32 -> fp16 or fp16 -> fp16" in err()
    for src, dst in ((F32, F32), (F32, F16), (F16, F16)):
        for k in (1, 3):
            assert not pack(None, 3, 3, k, k, src, dst, 16, None) and b"null" in err()
            assert not pack(16, 3, 3, k, k, src, dst, None, None) and b"null" in err()
            assert not pack(16, 3, 3, k, k, src, dst, 24, None) and b"16-byte" in err()
            assert not pack(16, 0, 3, k, k, src, dst, 16, None) and b"bad size" in err()
            assert not pack(16, 3, 0, k, k, src, dst, 16, None) and b"bad size" in err()
        assert not pack(16, 2 ** 14, 2 ** 14, 3, 3, src, dst, 16, None) and b"2^31" in err()
    # forward(x, packed, scale, shift, residual, relu, out, dtype, N, C, O, H, W, k, stride, stream)
    for dt in (F32, F16):
        assert not fwd(None, 16, None, None, None, 1, 16, dt, 1, 3, 3, 2, 2, 3, 1, None) and b"null" in err()
        assert not fwd(16, None, None, None, None, 1, 16, dt, 1, 3, 3, 2, 2, 3, 1, None) and b"null" in err()
        assert not fwd(16, 16, None, None, None, 1, None, dt, 1, 3, 3, 2, 2, 3, 1, None) and b"null" in err()
        assert not fwd(16, 24, None, None, None, 1, 16, dt, 1, 3, 3, 2, 2, 3, 1, None) and b"16-byte" in err()
        assert not fwd(16, 16, 16, None, None, 1, 16, dt, 1, 3, 3, 2, 2, 3, 1, None) and b"together" in err()
        assert not fwd(16, 16, None, 16, None, 1, 16, dt, 1, 3, 3, 2, 2, 3, 1, None) and b"together" in err()
        for k in (0, 2, 5, -1):
            assert not fwd(16, 16, None, None, None, 1, 16, dt, 1, 3, 3, 2, 2, k, 1, None) and b"k must be 1 or 3" in err()
        for s in (0, 3, -1):
            assert not fwd(16, 16, None, None, None, 1, 16, dt, 1, 3, 3, 2, 2, 3, s, None) and b"stride must be 1 or 2" in err()
        assert not fwd(16, 16, None, None, None, 1, 16, dt, 2 ** 7, 2 ** 8, 1, 2 ** 8, 2 ** 8, 1, 1, None) and b"2^31" in err()      # x
        assert not fwd(16, 16, None, None, None, 1, 16, dt, 2 ** 7, 1, 2 ** 8, 2 ** 8, 2 ** 8, 3, 1, None) and b"2^31" in err()      # out
        assert not fwd(16, 16, None, None, None, 1, 16, dt, 2 ** 7, 1, 2 ** 10, 2 ** 8, 2 ** 8, 3, 2, None) and b"2^31" in err()     # out at stride 2
        for shape in ((0, 3, 3, 2, 2), (1, 0, 3, 2, 2), (1, 3, 0, 2, 2), (1, 3, 3, 0, 2), (1, 3, 3, 2, 0)):
            assert not fwd(16, 16, None, None, None, 1, 16, dt, *shape, 3, 1, None) and b"bad s" in err()
    assert not fwd(16, 16, None, None, None, 1, 16, 2, 1, 3, 3, 2, 2, 3, 1, None) and b"fp32 or fp16" in err()


def test_python_refusals():
    w, w1, bn = torch.zeros(4, 6, 3, 3), torch.zeros(4, 6, 1, 1), torch.nn.BatchNorm2d(4).eval()
    for dt in (torch.bfloat16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="fp32 or fp16"):
            pack_conv_bn(w, dtype=dt)
    for bad in (torch.zeros(4, 6, 5, 5), torch.zeros(4, 6, 3, 1), torch.zeros(4, 6, 3), torch.zeros(0, 6, 3, 3), torch.zeros(4, 0, 1, 1), [w]):
        with pytest.raises(ValueError, match=r"\[O,C,k,k\]"):
            pack_conv_bn(bad)
    for bad, dt in ((w.half(), torch.float32), (w.double(), torch.float16), (w1.bfloat16(), torch.float16)):
        with pytest.raises(ValueError, match="fp32"):
            pack_conv_bn(bad, dtype=dt)
    for stride in (0, 3, -1, None):
        with pytest.raises(ValueError, match="stride"):
            pack_conv_bn(w, stride=stride)
    with pytest.raises(ValueError, match="batchnorm"):
        pack_conv_bn(w, torch.nn.BatchNorm2d(5))
    with pytest.raises(ValueError, match="batchnorm"):
        pack_conv_bn(w1, torch.nn.BatchNorm2d(4, track_running_stats=False))
    for dt, ww in ((torch.float32, w), (torch.float16, w1), (torch.float16, w.half())):      # past the checks: refused as CPU tensors
        with pytest.raises(RuntimeError, match="ROCm device"):
            pack_conv_bn(ww, bn, 2, dtype=dt)

    def pack(dtype=torch.float32, k=3, stride=1, weight=w):
        return ConvBnPack(None, None, None, 4, 6, k, stride, (weight,), dtype)

    p = pack(torch.float16, 1, 2)
    assert (p.k, p.stride, p.dtype, p.out_channels, p.in_channels, p.split) == (1, 2, torch.float16, (4,), 6, None)
    assert isinstance(p, upmod.UpconvPack) and not p.stale() and p.made_from([w]) and not p.made_from([w.clone()])
    seen = pack()
    w.add_(1)
    assert seen.stale() and not pack().stale()
    x, res = torch.zeros(2, 6, 5, 7), torch.zeros(2, 4, 5, 7)
    with torch.no_grad():
        for bad in ((w,), upmod.UpconvPack(None, None, None, (4,), 6, 0, (w,))):          # a tail's pack carries no window and no stride
            with pytest.raises(ValueError, match="pack_conv_bn"):
                conv_bn_act(x, bad)
        with pytest.raises(ValueError, match=r"x is torch.float16.*torch.float32"):
            conv_bn_act(x.half(), pack())
        with pytest.raises(ValueError, match=r"x is torch.float32.*torch.float16"):
            conv_bn_act(x, pack(torch.float16))
        with pytest.raises(ValueError, match=r"x is torch.bfloat16"):
            conv_bn_act(x.bfloat16(), pack())
        with pytest.raises(ValueError, match=r"residual is torch.float32"):
            conv_bn_act(x.half(), pack(torch.float16), residual=res)
        with pytest.raises(ValueError, match="x has 5 channels, the pack takes 6"):
            conv_bn_act(x[:, :5], pack())
        with pytest.raises(ValueError, match="residual has 3 channels, the pack takes 4"):
            conv_bn_act(x, pack(), residual=res[:, :3])
        with pytest.raises(ValueError, match=r"residual must be \(2, 4, 5, 7\)"):
            conv_bn_act(x, pack(), residual=res[:1])
        with pytest.raises(ValueError, match=r"residual must be \(2, 4, 3, 4\)"):          # the OUTPUT's size under stride 2
            conv_bn_act(x, pack(stride=2), residual=res)
        with pytest.raises(ValueError, match=r"\[N,C,H,W\]"):
            conv_bn_act(x[0], pack())
        with pytest.raises(ValueError, match="empty"):
            conv_bn_act(x[:0], pack())
        big = torch.zeros(1, 1, 1, 1).expand(2 ** 7, 6, 2 ** 11, 2 ** 11)                  # 2^31 elements or more, no memory behind them
        with pytest.raises(ValueError, match="x has 2\\^31 elements"):
            conv_bn_act(big, pack())
        wide = ConvBnPack(None, None, None, 2 ** 12, 1, 1, 1, (w,))
        with pytest.raises(ValueError, match="output has 2\\^31 elements"):
            conv_bn_act(torch.zeros(1, 1, 1, 1).expand(2 ** 9, 1, 2 ** 5, 2 ** 5), wide)
        for args in ((x, pack()), (x, pack(k=1, stride=2)), (x, pack(), res), (x.half(), pack(torch.float16)), (x, pack(stride=2), res[:, :, :3, :4])):
            with pytest.raises(RuntimeError, match="ROCm device"):                         # past the checks: refused as CPU tensors
                conv_bn_act(*args)
    with torch.enable_grad():                                                              # forward only
        with pytest.raises(RuntimeError, match="forward-only.*stock block"):
            conv_bn_act(x.clone().requires_grad_(True), pack())
        with pytest.raises(RuntimeError, match="forward-only"):
            conv_bn_act(x, pack(), residual=res.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match="forward-only"):
            conv_bn_act(x, pack(weight=torch.nn.Parameter(w)))


def test_the_keyword_and_what_it_selects():
    assert isinstance(cb.FUSED_ENCODER_DEFAULT, tuple) and set(cb.FUSED_ENCODER_DEFAULT) <= set(STAGES)
    assert isinstance(cb.FUSED_ENCODER_HALF_DEFAULT, tuple) and set(cb.FUSED_ENCODER_HALF_DEFAULT) <= set(STAGES)
    assert STAGES == ("layer1", "layer2", "layer3", "layer4", "conv2")

    def marks(m, attr):
        return [all(getattr(b, attr) for b in getattr(m, n)) for n in STAGES[:4]] + [getattr(m, attr.replace("encoder", "bridge"))]

    for net in (unet_ours, unet_cspn_nyu):
        params = list(inspect.signature(net.ResNet.__init__).parameters.values())
        assert [p.name for p in params[-2:]] == ["fused_encoder", "fused_decoder_precision"] and params[-2].default is False
        assert params[-1].default is None and [p.name for p in params[-5:-2]] == ["fused_heads", "fused_decoder", "fused_tail"]
        m = net.resnet18()
        assert m.fused_encoder == () and not any(marks(m, "fused_encoder") + marks(m, "fused_encoder_half"))
        keys = list(m.state_dict())
        m = net.resnet18(fused_encoder=True)
        assert m.fused_encoder == tuple(n for n in STAGES if n in cb.FUSED_ENCODER_DEFAULT) and list(m.state_dict()) == keys
        assert marks(m, "fused_encoder") == [n in cb.FUSED_ENCODER_DEFAULT for n in STAGES]
        assert marks(m, "fused_encoder_half") == [n in cb.FUSED_ENCODER_HALF_DEFAULT for n in STAGES]
        assert m.fused_tail == () and m.fused_decoder == () and not m.fused_heads
        m = net.resnet18(fused_encoder=["conv2", "layer3", "layer1"], fused_tail=True)     # names: both precisions, encoder order
        assert m.fused_encoder == ("layer1", "layer3", "conv2") and m.fused_decoder == ()
        assert marks(m, "fused_encoder") == marks(m, "fused_encoder_half") == [True, False, True, False, True]
        assert m.fused_tail == tuple(n for n in upmod.DECODER_BLOCKS if n in upmod.FUSED_TAIL_DEFAULT)
        m = net.resnet18(fused_encoder="layer4", fused_heads=True, fused_decoder=True, fused_decoder_precision="bf16x3")
        assert m.fused_encoder == ("layer4",) and m.fused_heads and m.fused_decoder == upmod.DECODER_BLOCKS
        assert marks(m, "fused_encoder") == [False, False, False, True, False] and m.fused_decoder_precision == "bf16x3"
        for bad in ("layer5", ["layer1", "gud_up_proj_layer1"], "bn2"):
            with pytest.raises(ValueError, match="fused_encoder.*not among"):
                net.resnet18(fused_encoder=bad)
        m = net.resnet18(fused_encoder=STAGES)
        assert all(b._convbn_packs is None for n in STAGES[:4] for b in getattr(m, n)) and m._convbn_packs is None
        assert list(m.state_dict()) == keys and [n for n, _ in m.named_modules()] == [n for n, _ in net.resnet18().named_modules()]
        assert not [k for k in m.state_dict() if "pack" in k]
    assert len(unet_ours.resnet50(decoder_sizes=unet_ours.decoder_sizes_for(36, 52), fused_encoder=True).state_dict()) == 417
    # which inputs run which path: grad mode off, eval mode
    block = unet_ours.Bottleneck(8, 2).eval()
    x = torch.zeros(1, 8, 5, 7)
    with torch.no_grad():
        assert not block._fuse_encoder() and not block._fuse_encoder(x) and not block._fuse_encoder(x.half())
        block.fused_encoder = True                                                         # marked by hand: half follows
        assert block._fuse_encoder() and block._fuse_encoder(x) and block._fuse_encoder(x.half())
        assert not block._fuse_encoder(x.double()) and not block._fuse_encoder(x.bfloat16())
        block.fused_encoder_half = False
        assert block._fuse_encoder() and block._fuse_encoder(x) and not block._fuse_encoder(x.half())
        block.fused_encoder, block.fused_encoder_half = False, True
        assert block._fuse_encoder() and not block._fuse_encoder(x) and block._fuse_encoder(x.half())
    with torch.enable_grad():
        assert not block._fuse_encoder() and not block._fuse_encoder(x.half())
    with torch.no_grad():
        assert not block.train()._fuse_encoder() and not block._fuse_encoder(x.half())


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
NP_DT = {torch.float32: np.float32, torch.float16: np.float16}


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def packed_for(w, source_dtype, dtype, stride):
    return pack_conv_bn(dev(w, source_dtype), None, stride, dtype)


def run(pack, x, scale=None, shift=None, r=None, relu=True):
    """The kernel on `pack`'s filter with an affine map of the test's own."""
    mine = ConvBnPack(pack.packed, dev(scale), dev(shift), pack.out_channels[0], pack.in_channels, pack.k, pack.stride, pack.sources, pack.dtype)
    with torch.no_grad():
        out = conv_bn_act(dev(x, pack.dtype), mine, dev(r, pack.dtype), relu)
    want = (x.shape[0], pack.out_channels[0], cc.out_size(x.shape[2], pack.stride), cc.out_size(x.shape[3], pack.stride))
    assert out.is_contiguous() and out.dtype == pack.dtype and tuple(out.shape) == want
    return out


def same_bits(t, want):
    """t (device tensor) and want (numpy, fp32 or fp16): the same shape, dtype and bits."""
    got = t.detach().cpu().numpy()
    view = np.uint32 if want.dtype == np.float32 else np.uint16
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(view), want.view(view))


def integer_case(C, O, shape, k, s):
    x, w, scale, shift, r = cc.make_inputs(C, O, shape, k, s, True)
    p32 = packed_for(w, torch.float32, torch.float32, s)
    p16 = [packed_for(w, torch.float32, torch.float16, s), packed_for(w, torch.float16, torch.float16, s)]
    assert p16[0].packed.dtype == torch.float16 and torch.equal(p16[0].packed, p16[1].packed) and (p32.k, p32.stride) == (k, s)
    lib = _lib.lib()
    assert p32.packed.numel() * 4 == lib.cspn_convbn_packed_bytes(O, C, k, F32)
    assert p16[0].packed.numel() * 2 == lib.cspn_convbn_packed_bytes(O, C, k, F16)
    acc = cc.accumulate(x.astype(np.float64), w.astype(np.float64), s)
    for res, relu, affine in cc.EPILOGUES:
        args = (scale if affine else None, shift if affine else None, r if res else None, relu)
        exact = cc.epilogue(acc, *args)
        what = (C, O, shape, k, s, res, relu, affine)
        assert same_bits(run(p32, x, *args), exact.astype(np.float32)), what
        for pack in p16:
            assert same_bits(run(pack, x, *args), exact.astype(np.float16)), what


@pytest.mark.gpu
@pytest.mark.parametrize("k,s", cc.KS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_integer_cases_bit_equal_to_the_restatement(shape, k, s):
    for case in cc.integer_cases(shape, k, s):
        integer_case(*case)


@pytest.mark.gpu
@pytest.mark.parametrize("k,s", cc.KS, ids=lambda v: str(v))
def test_integer_cases_over_several_chunks_and_tiles(k, s):
    big, wide = cc.BIG, cc.WIDE
    assert big["C"] > 32 and big["shape"][0] * cc.out_size(big["shape"][1], 2) * cc.out_size(big["shape"][2], 2) > 128      # tiles at stride 2 too
    assert wide["O"] > 2 * 128
    for d in (big, wide):
        integer_case(d["C"], d["O"], d["shape"], k, s)


def check_within_bound(what, got, want, bound):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and got.shape == want.shape
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print("%s: largest error / bound = %.4f" % (what, ratio))
    assert (err <= bound).all(), (what, ratio)
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("k,s", cc.KS, ids=lambda v: str(v))
@pytest.mark.parametrize("C,O,shape", cc.REAL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_real_cases_within_the_a_priori_bound(C, O, shape, k, s):
    x, w, scale, shift, r = cc.make_inputs(C, O, shape, k, s, False)
    p32, p16 = packed_for(w, torch.float32, torch.float32, s), packed_for(w, torch.float32, torch.float16, s)
    assert torch.equal(p16.packed, packed_for(cc.to_half(w), torch.float16, torch.float16, s).packed)      # rounded to nearest even, once
    moved = 0
    for res, relu, affine in cc.EPILOGUES:
        args = (scale if affine else None, shift if affine else None, r if res else None)
        what = "C=%d O=%d %s k=%d s=%d res=%d relu=%d affine=%d" % (C, O, shape, k, s, res, relu, affine)
        want = cc.restate(x, w, s, *args, relu)
        got = run(p32, x, *args, relu)
        check_within_bound("fp32 " + what, got, want, cc.bound(x, w, s, *args) + 1e-300)
        moved += int((got.cpu().numpy().astype(np.float64) != want).sum())
        want = cc.restate_half(x, w, s, *args, relu)[1]
        assert np.abs(want).max() < cc.HALF_MAX
        check_within_bound("fp16 " + what, run(p16, x, *args, relu), want, cc.bound_half(x, w, s, *args, relu))
    assert moved > 0                                                         # rounded results, not a copy of the fp64 ones


@pytest.mark.gpu
@pytest.mark.parametrize("C,O,shape", cc.REAL_CASES + ((1, 1, (1, 1, 1)), (3, 33, (2, 5, 7))),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_k3_s1_gives_the_bits_of_the_decoder_tail(C, O, shape):
    """The one-map case of conv3x3_bn_act on real-valued inputs: the same K order through the same instructions, so the same bits,
    in both precisions and with every epilogue."""
    x, w, scale, shift, r = cc.make_inputs(C, O, shape, 3, 1, False)
    for dtype in (torch.float32, torch.float16):
        mine, tail = packed_for(w, torch.float32, dtype, 1), pack_conv3x3(dev(w), None, None, dtype)
        assert torch.equal(mine.packed, tail.packed)
        for res, relu, affine in cc.EPILOGUES:
            sc, sh = (dev(scale), dev(shift)) if affine else (None, None)
            rr = dev(r, dtype) if res else None
            with torch.no_grad():
                want = conv3x3_bn_act(dev(x, dtype), upmod.UpconvPack(tail.packed, sc, sh, (O,), C, 0, tail.sources, dtype), None, rr, relu)
            got = run(mine, x, scale if affine else None, shift if affine else None, r if res else None, relu)
            assert got.dtype == want.dtype == dtype and torch.equal(got.view(torch.int16 if dtype == torch.float16 else torch.int32),
                                                                    want.view(torch.int16 if dtype == torch.float16 else torch.int32)), (dtype, res, relu, affine)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_chained_within_the_composed_bound(name):
    """The calls of a block chained on the device as the fused block chains them, each fed the previous device results, against the
    stored fp64 values.  The composed bound of a step, with f the step on the stored fp64 parameters, f_r the step on the operands the
    device is given (its inputs and the filter rounded to the precision, scale and shift to fp32), both in exact arithmetic, and x*,
    r* the stored inputs:  |got - f(x*, r*)| <= |got - f_r(x, r)| + |f_r(x, r) - f(x, r)| + |f(x, r) - f(x*, r*)|
        the a-priori bound of the kernel  +  a difference of two fp64 restatements  +  |scale| sum |w| |x - x*| + |r - r*|,
    the last from the composed bounds of the steps that made x and r.  Half runs only where every stored value lies in the fp16
    range."""
    z = load_golden(name)
    steps = cc.block_steps(z)
    fits = all(np.abs(v).max() < cc.HALF_MAX for k, v in z.items() if v.dtype.kind == "f" and v.ndim == 4)
    assert fits or "_int_" in name
    for dtype in (torch.float32,) + ((torch.float16,) if fits else ()):
        np_dt = NP_DT[dtype]
        x0 = z["x"].astype(np_dt)
        have = {"x": (x0, np.abs(x0.astype(np.float64) - z["x"]))}                          # key -> (what the device holds, the bound on its distance from the stored one)
        for src, w, s, scale, shift, res, relu, dst in steps:
            x, xb = have[src]
            r, rb = have[res] if res else (None, 0.0)
            s32, h32 = scale.astype(np.float32), shift.astype(np.float32)
            given = (x.astype(np.float64), w.astype(np_dt).astype(np.float64), s, s32.astype(np.float64), h32.astype(np.float64),
                     None if r is None else r.astype(np.float64))
            got = run(packed_for(w, torch.float32, dtype, s), x, s32, h32, r, relu)
            own = cc.bound(*given) if dtype == torch.float32 else cc.bound_half(*given, relu)
            own = own + np.abs(cc.restate(*given, relu) - cc.restate(given[0], w, s, scale, shift, given[5], relu))
            own = own + cc._terms(xb, w, s, scale, None, None) + rb
            check_within_bound("%s %s %s" % (name, dtype, dst), got, z[dst], own + 1e-300)
            have[dst] = (got.cpu().numpy(), own)
        assert got.dtype == dtype and "y" in have


@pytest.mark.gpu
def test_batch_place_and_determinism():
    d = cc.RAGGED
    for k, s in ((d["k"], d["s"]), (1, 1)):
        x, w, scale, shift, r = cc.make_inputs(d["C"], d["O"], d["shape"], k, s, False)
        for dtype in (torch.float32, torch.float16):
            pack = packed_for(w, torch.float32, dtype, s)
            ys = run(pack, x, scale, shift, r)
            assert torch.equal(ys, run(pack, x, scale, shift, r))                           # two runs of one call
            for n in (0, 2):                                                                # frame n of B = 3 at position 0 of B = 1
                alone = run(pack, x[n:n + 1], scale, shift, r[n:n + 1])
                assert torch.equal(alone[0], ys[n])
            pair = run(pack, x[1:3], scale, shift, r[1:3])                                  # ... and at position 1 of B = 2: other tiles again
            assert torch.equal(pair[1], ys[2])


@pytest.mark.gpu
@pytest.mark.parametrize("C,O,shape,k,s", [(33, 129, (3, 7, 9), 3, 2), (33, 129, (3, 7, 9), 1, 2), (3, 33, (2, 5, 7), 3, 1), (67, 3, (1, 15, 19), 1, 1),
                                           (1, 1, (1, 1, 1), 3, 2)], ids=["ragged", "ragged_1x1", "same", "pointwise", "one_px"])
def test_nothing_outside_the_output_is_written(C, O, shape, k, s):
    x, w, scale, shift, r = cc.make_inputs(C, O, shape, k, s, True)
    for dtype in (torch.float32, torch.float16):
        pack = packed_for(w, torch.float32, dtype, s)
        want = run(pack, x, scale, shift, r)
        pad, sentinel, size = 4096, -12288.0, want.numel()                               # a fp16 value no case produces in the band
        assert not bool((want == sentinel).any())
        buf = torch.full((2 * pad + size,), sentinel, device=DEV, dtype=dtype)
        out = buf[pad:pad + size].view(want.shape)
        xd, rd, sd, hd = dev(x, dtype), dev(r, dtype), dev(scale), dev(shift)
        launch(torch.device(DEV), "cspn_convbn_forward", xd.data_ptr(), pack.packed.data_ptr(), sd.data_ptr(), hd.data_ptr(), rd.data_ptr(), 1,
               out.data_ptr(), F32 if dtype == torch.float32 else F16, shape[0], C, O, shape[1], shape[2], k, s)
        torch.cuda.synchronize()
        assert torch.equal(out, want)
        assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + size:] == sentinel).all())


@pytest.mark.gpu
def test_ragged_case_under_poisoned_lds():
    """The ragged case — 33 channels, a second M tile with one live row, odd H and W under stride 2 — with NaN in the whole LDS of
    every CU in front of every launch: the bits of the plain run, in both precisions."""
    d = cc.RAGGED
    assert (d["C"], d["O"], d["shape"], d["k"], d["s"]) == (33, 129, (3, 7, 9), 3, 2)
    x, w, scale, shift, r = cc.make_inputs(d["C"], d["O"], d["shape"], d["k"], d["s"], True)
    for dtype, pattern in ((torch.float32, 0x7fc00000), (torch.float16, 0x7fc07fc0)):      # NaN as fp32, and in both fp16 halves
        pack = packed_for(w, torch.float32, dtype, d["s"])
        plain = run(pack, x, scale, shift, r)
        with lds_poison(pattern):
            got = run(pack, x, scale, shift, r)
            torch.cuda.synchronize()
        assert torch.equal(got, plain) and not bool(torch.isnan(got).any())


def seeded_block(cls, inplanes, planes, stride, seed=5):
    torch.manual_seed(seed)
    down = None
    if stride != 1 or inplanes != planes * cls.expansion:
        down = torch.nn.Sequential(unet_cspn_nyu._conv(inplanes, planes * cls.expansion, 1, stride), torch.nn.BatchNorm2d(planes * cls.expansion))
    block = cls(inplanes, planes, stride, down)
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0, 0.1)
    return block.to(DEV).eval()


@pytest.mark.gpu
def test_graph_capture_of_a_stride2_bottleneck_gives_the_eager_bits(monkeypatch):
    """Forward only, under no_grad: the four calls of a Bottleneck with a stride-2 downsample branch captured once, replayed on new
    input values."""
    for dtype in (torch.float32, torch.float16):
        block = seeded_block(unet_ours.Bottleneck, 40, 10, 2)
        block.fused_encoder = True
        if dtype == torch.float16:
            block.half()
        torch.manual_seed(3)
        a, a2 = (torch.randn(2, 40, 9, 13, device=DEV).to(dtype) for _ in range(2))
        calls = []
        real = cb.conv_bn_act
        monkeypatch.setattr(cb, "conv_bn_act", lambda *args, **kw: (calls.append(1), real(*args, **kw))[1])
        with torch.no_grad():
            eager = [block(v) for v in (a, a2)]
            assert len(calls) == 8 and eager[0].shape == (2, 40, 5, 7) and eager[0].dtype == dtype
            stock = seeded_block(unet_ours.Bottleneck, 40, 10, 2).to(dtype)(a)
            assert float((stock.float() - eager[0].float()).abs().max()) <= (1e-5 if dtype == torch.float32 else 2e-2) * float(stock.float().abs().max())
            sx = a.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                block(sx)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            del calls[:]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = block(sx)
            assert len(calls) == 4
            for v, want in ((a2, eager[1]), (a, eager[0])):                                # two replays, on new input values
                sx.copy_(v)
                out.fill_(7.0)
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, want)
        assert not torch.equal(eager[0], eager[1])
        monkeypatch.undo()


class Recorder(object):
    """Stands in for conv_bn_act and for launch inside network.conv_bn: keeps what went into and came out of every fused call, and the
    name of every native entry point that was called with the dtype code it was given."""

    def __init__(self, monkeypatch, keep=True):
        self.calls, self.entries, self.real, self.real_launch, self.keep = [], [], cb.conv_bn_act, cb.launch, keep
        monkeypatch.setattr(cb, "conv_bn_act", self)
        monkeypatch.setattr(cb, "launch", self.launch)

    def __call__(self, x, pack, residual=None, relu=True):
        out = self.real(x, pack, residual, relu)
        self.calls.append((x.detach().clone(), pack, None if residual is None else residual.detach().clone(), relu, out.detach().clone())
                          if self.keep else (None, pack, None, relu, None))
        return out

    def launch(self, device, name, *args):
        self.entries.append((name, args[6] if name.endswith("pack") else args[7]))          # dst_dtype / dtype
        return self.real_launch(device, name, *args)

    def clear(self):
        del self.calls[:], self.entries[:]


def model_case(kind, arch="resnet18", seed=11, **switches):
    """tests/test_uptail.py's model: either network at 36 x 52, B = 2, batch norms with statistics that are not the initial ones."""
    torch.manual_seed(seed)
    sizes = unet_ours.decoder_sizes_for(36, 52)
    if kind == "ours":
        net = getattr(unet_ours, arch)(decoder_sizes=sizes, prop_time=2, **switches)
    else:
        net = getattr(unet_cspn_nyu, arch)(decoder_sizes=sizes, prop_time=2, reference_state_dict=False, **switches)
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


def fused_convs(net):
    """(what, conv, bn, stride, has a residual, relu, the module that keeps the pack, its key) of every fused call, in call order."""
    rows = []
    for stage in STAGES[:4]:
        for i, block in enumerate(getattr(net, stage)):
            convs = [n for n in ("conv1", "conv2", "conv3") if hasattr(block, n)]
            for n in convs[:-1]:
                rows.append(("%s.%d.%s" % (stage, i, n), getattr(block, n), getattr(block, "bn" + n[4:]), False, True, block, n))
            if block.downsample is not None:
                rows.append(("%s.%d.downsample" % (stage, i), block.downsample[0], block.downsample[1], False, False, block, "downsample"))
            n = convs[-1]
            rows.append(("%s.%d.%s" % (stage, i, n), getattr(block, n), getattr(block, "bn" + n[4:]), True, True, block, n))
    rows.append(("conv2", net.conv2, net.bn2, False, False, net, "conv2"))
    return rows


def expected_entries(net, code, packs=True):
    step = ([("cspn_convbn_pack", code)] if packs else []) + [("cspn_convbn_forward", code)]
    return step * len(fused_convs(net))


def check_calls(rec, net, how, what):
    """Every recorded call against the fp64 restatement on the block's own parameters, within the a-priori bound."""
    dtype = torch.float32 if how == "fp32" else torch.float16
    rows = fused_convs(net)
    assert len(rec.calls) == len(rows)
    for (name, conv, bn, has_res, relu, owner, key), (x, pack, residual, got_relu, out) in zip(rows, rec.calls):
        assert pack is owner._convbn_packs[key] and not pack.stale() and pack.dtype == dtype and got_relu is relu
        assert (pack.k, pack.stride) == (conv.kernel_size[0], conv.stride[0]) and (residual is not None) == has_res
        assert all(t is None or t.dtype == dtype for t in (x, residual, out))
        assert conv.weight.dtype == (torch.float16 if how == "half" else torch.float32)
        w = conv.weight.detach().float().cpu().numpy()
        scale, shift = cc.fold(*(t.detach().float().cpu().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)), bn.eps)
        args = (x.float().cpu().numpy(), w, pack.stride, scale, shift, None if residual is None else residual.float().cpu().numpy())
        label = "%s %s %s" % (what, how, name)
        if dtype == torch.float32:
            check_within_bound(label, out, cc.restate(*args, relu), cc.bound(*args, extra=4))
        else:
            check_within_bound(label, out, cc.restate_half(*args, relu)[1], cc.bound_half(*args, relu, extra=4))
        if relu:
            assert float(out.min()) == 0.0 and float(out.max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["fp32", "autocast", "half"])
@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_models_fused_encoder_within_the_bound(kind, arch, how, monkeypatch):
    net, inp = model_case(kind, arch, fused_encoder=STAGES)
    net.eval()
    keys = list(net.state_dict())
    assert len(fused_convs(net)) == {"resnet18": 20, "resnet50": 53}[arch]
    if how == "half":
        net.half()
    rec = Recorder(monkeypatch)
    outs = run_model(net, inp, how)
    code = F32 if how == "fp32" else F16
    assert rec.entries == expected_entries(net, code) and list(net.state_dict()) == keys
    check_calls(rec, net, how, "%s %s" % (kind, arch))
    assert all(bool(torch.isfinite(o).all()) for o in outs[:2])
    rec.clear()
    run_model(net, inp, how)                                                  # a second forward packs nothing again
    assert rec.entries == expected_entries(net, code, packs=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_modes_dtypes_and_repacking(kind, monkeypatch):
    net, inp = model_case(kind, fused_encoder=STAGES)
    plain = model_case(kind)[0].eval()
    assert list(net.state_dict()) == list(plain.state_dict()) and all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), plain.state_dict().values()))
    net.eval()
    n = len(fused_convs(net))
    rec = Recorder(monkeypatch)
    first = run_model(net, inp, "fp32")
    assert rec.entries == expected_entries(net, F32) and all(c[0].dtype == torch.float32 for c in rec.calls)
    want = run_model(plain, inp, "fp32")                                     # the stock model on the same weights
    assert all(float((g - w).abs().max()) <= 1e-3 * float(w.abs().max()) for g, w in zip(first[:2], want[:2]))
    rec.clear()
    run_model(net, inp, "autocast")                                          # the same model under autocast: repacked for half
    assert rec.entries == expected_entries(net, F16) and all(c[1].dtype == torch.float16 for c in rec.calls)
    rec.clear()
    run_model(net, inp, "fp32")                                              # ... and back
    assert rec.entries == expected_entries(net, F32)
    rec.clear()
    with torch.enable_grad():                                                # grad mode on: the stock lines
        net.features(inp)
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            net.features(inp)
    assert rec.calls == [] and rec.entries == []
    net.train()                                                              # train mode: the stock lines, and no pack is kept
    assert net._convbn_packs is None and all(b._convbn_packs is None for s in STAGES[:4] for b in getattr(net, s))
    run_model(net, inp, "fp32")
    run_model(net, inp, "autocast")
    assert rec.calls == [] and rec.entries == []
    net.eval()
    other = model_case(kind, seed=13)[0]                                     # other weights: written in place, every pack is stale
    run_model(net, inp, "fp32")
    rec.clear()
    net.load_state_dict(other.state_dict())
    packs = [p for s in STAGES[:4] for b in getattr(net, s) for p in b._convbn_packs.values()] + list(net._convbn_packs.values())
    assert len(packs) == n and all(p.stale() for p in packs)
    second = run_model(net, inp, "fp32")
    assert rec.entries == expected_entries(net, F32)                         # every pack was made again
    check_calls(rec, net, "fp32", kind + " after load_state_dict")
    want = run_model(other.eval(), inp, "fp32")
    assert not torch.equal(first[0], second[0])
    assert all(float((g - w).abs().max()) <= 1e-3 * float(w.abs().max()) for g, w in zip(second[:2], want[:2]))
    rec.clear()
    cb.select_fused_encoder(net, True)                                       # True: each precision takes its measured selection
    per_stage = dict((s, sum(1 for r in fused_convs(net) if r[0].split(".")[0] == s)) for s in STAGES)
    run_model(net, inp, "fp32")
    assert len(rec.calls) == sum(per_stage[s] for s in cb.FUSED_ENCODER_DEFAULT)
    rec.clear()
    run_model(net, inp, "autocast")
    assert len(rec.calls) == sum(per_stage[s] for s in cb.FUSED_ENCODER_HALF_DEFAULT)
    rec.clear()
    cb.select_fused_encoder(net, ["layer2", "conv2"])                        # names: those stages alone, in both precisions
    run_model(net, inp, "fp32")
    run_model(net, inp, "autocast")
    assert len(rec.calls) == 2 * (per_stage["layer2"] + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["fp32", "autocast"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_fused_encoder_composes_with_the_other_switches(kind, how, monkeypatch):
    """All four switches in one model: the encoder's entry points are called as often as with the switch alone, the other switches'
    packs are made, the state_dict is the one of the plain model and the outputs stay with the stock model's."""
    net, inp = model_case(kind, fused_encoder=STAGES, fused_heads=(how == "fp32"), fused_decoder=upmod.DECODER_BLOCKS, fused_tail=upmod.DECODER_BLOCKS)
    plain = model_case(kind)[0].eval()
    net.eval()
    assert list(net.state_dict()) == list(plain.state_dict())
    rec = Recorder(monkeypatch, keep=False)
    got = run_model(net, inp, how)
    assert rec.entries == expected_entries(net, F32 if how == "fp32" else F16)
    assert all(getattr(net, n)._upconv_pack is not None and getattr(net, n)._tail_packs for n in upmod.DECODER_BLOCKS)
    assert all(bool(torch.isfinite(g).all()) for g in got[:2])
    if how == "fp32":                                                        # tests/test_uptail.py's distance from the stock model on those weights
        want = run_model(plain, inp, "fp32")
        assert all(float((g - w).abs().max()) <= 1e-3 * float(w.abs().max()) for g, w in zip(got[:2], want[:2]))
    alone = model_case(kind, fused_encoder=STAGES)[0].eval()
    rec.clear()
    run_model(alone, inp, how)
    assert rec.entries == expected_entries(alone, F32 if how == "fp32" else F16)

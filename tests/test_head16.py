"""The fused output heads in half precision: the `head16` family of the native library (include/cspn_head16.h),
network.up_pooling.up_pooling_conv3x3_half, and what `fused_heads` of the two models does with a half map.

References: heads_cases.forward in fp64 on inputs rounded to fp16, rounded once to fp16 (head16_cases.reference), and the goldens
G26.  Integer-valued cases are compared bit for bit; real-valued cases against the a-priori bound of head16_cases.bound_half (the
module's docstring says where every term comes from)."""
import ctypes
import hashlib
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import head16_cases as c16
import heads_cases as hc
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd._host import launch
from cspn_monodepth_amd.network import unet_cspn_nyu, unet_ours
from cspn_monodepth_amd.network import up_pooling as upmod
from cspn_monodepth_amd.network.up_pooling import up_pooling_conv3x3, up_pooling_conv3x3_half

DEV = "cuda:0"
NAMES = ("cspn_head16_abi_version", "cspn_head16_workspace_bytes", "cspn_head16_forward")
INT_GOLDENS = golden_names("g26_heads_int_")
REAL_GOLDENS = golden_names("g26_heads_real_")
F32, F16 = _lib.CSPN_F32, _lib.CSPN_F16
PINNED_WORDS = ("heads", "upconv", "uphalf", "uptail", "convbn", "criterion", "max8", "abn", "sparsify", "transform", "losses", "berhu",
                "mean_loss", "optim", "sgd", "visual")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize"]


def unpack(z):
    oh, ow = (int(v) for v in z["geom"][:2])
    heads = tuple(int(v) for v in z["geom"][2:])
    pick = lambda stem: [z[stem + str(h)] for h in range(len(heads))]          # noqa: E731
    return oh, ow, heads, pick


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_head16_family_contract():
    """Header, loader table and library agree on the family, in the terms of test_convbn_family_contract; the family sits in a third
    part of the table, and every tuple, digest and stamp the older tests restate is what it was."""
    fam = _lib.family("head16")
    assert fam.header == os.path.join(ROOT, "include", "cspn_head16.h") and fam.files == {"cspn_head16.hip": False} and fam.opt_in
    text = open(fam.header).read()
    assert re.search(r"^#define CSPN_HEAD16_ABI_VERSION 1$", text, flags=re.M)
    for macro, value in (("MAX_HEADS", _lib.HEAD16_MAX_HEADS), ("MAX_OUT_CHANNELS", _lib.HEAD16_MAX_OUT_CHANNELS), ("TILE_H", _lib.HEAD16_TILE_H),
                         ("TILE_W", _lib.HEAD16_TILE_W), ("CHANNEL_BLOCK", _lib.HEAD16_CHANNEL_BLOCK)):
        assert re.search(r"^#define CSPN_HEAD16_%s %d$" % (macro, value), text, flags=re.M), macro
    assert (_lib.HEAD16_MAX_HEADS, _lib.HEAD16_MAX_OUT_CHANNELS) == (_lib.HEADS_MAX_HEADS, _lib.HEADS_MAX_OUT_CHANNELS) == (4, 16)
    declared = sorted(set(re.findall(r"\b(cspn\w*)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(fam.functions) == sorted(NAMES)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in NAMES) and lib.cspn_head16_abi_version() == fam.abi_version == 1
    for n in NAMES:                                                                        # the signatures lib() set
        fn, (restype, argtypes) = getattr(lib, n), fam.functions[n]
        assert (fn.argtypes is None and argtypes is None) or list(fn.argtypes) == list(argtypes)
        assert fn.restype is restype
    assert len(fam.functions["cspn_head16_forward"][1]) == 14 and fam.functions["cspn_head16_workspace_bytes"][0] is ctypes.c_size_t
    # a third part of the table: in none of the tuples the older tests count
    assert _lib.LATEST_FAMILIES == (fam,)
    for part in (_lib.FAMILIES, _lib.OPT_IN_FAMILIES, _lib.ALL_FAMILIES, _lib.LATER_FAMILIES, _lib.EVERY_FAMILY):
        assert fam not in part and "head16" not in [f.name for f in part]
    assert [f.name for f in _lib.LATER_FAMILIES] == ["convbn"] and _lib.EVERY_FAMILY == _lib.ALL_FAMILIES + _lib.LATER_FAMILIES
    assert [f.name for f in _lib.OPT_IN_FAMILIES] == ["heads", "upconv", "uphalf", "uptail"]
    assert len(_lib.FAMILIES) == 9 and len(_lib.ALL_FAMILIES) == 13
    assert _lib.LATER_SOURCES == ("cspn_convbn.hip",) and _lib.LATER_HEADERS == (_lib.family("convbn").header,)
    assert _lib.LATEST_SOURCES == ("cspn_head16.hip",) and _lib.LATEST_HEADERS == (fam.header,)
    assert "cspn_head16.hip" not in _lib.SOURCES + _lib.OPT_IN_SOURCES + _lib.LATER_SOURCES
    assert os.path.exists(os.path.join(_lib.CSRC, "cspn_head16.hip"))
    assert fam.header not in _lib.BUILD_HEADERS + _lib.HEADERS + _lib.LATER_HEADERS
    assert len([p for p in _lib.BUILD_HEADERS if os.path.dirname(p) == _lib.CSRC]) == 6          # no new header under csrc/
    # no pinned word in the new names, and the new name in no other family's
    for other in _lib.EVERY_FAMILY:
        assert not set(other.functions) & set(NAMES) and not any("head16" in n for n in other.functions)
    assert not any(w in n for w in PINNED_WORDS for n in NAMES)
    # the first stamp is composed as it was: _source_digest over the thirteen, carried on over convbn's source and header ...
    plain = hashlib.sha256(b"x")
    for path in [os.path.join(_lib.CSRC, f) for f in _lib.SOURCES + _lib.OPT_IN_SOURCES] + list(_lib.BUILD_HEADERS):
        plain.update(open(path, "rb").read())
    assert _lib._source_digest(["x"]) == plain.hexdigest()
    first = hashlib.sha256(plain.hexdigest().encode())
    for path in (os.path.join(_lib.CSRC, "cspn_convbn.hip"), _lib.family("convbn").header):
        first.update(open(path, "rb").read())
    assert _lib._later_digest(plain.hexdigest()) == first.hexdigest()
    flags = FLAGS + os.environ.get("CSPN_HIPCC_FLAGS", "").split()
    assert open(_lib.SO_PATH + ".hash").read().strip() == _lib._later_digest(_lib._source_digest(flags))
    # ... and the second stamp is the flags, the new source and the new header: an edit to either is another stamp
    files = (os.path.join(_lib.CSRC, "cspn_head16.hip"), fam.header)
    second = hashlib.sha256(" ".join(flags).encode())
    for path in files:
        second.update(open(path, "rb").read())
    assert _lib._latest_digest(flags) == second.hexdigest() == open(_lib.SO_PATH + ".hash2").read().strip()
    for keep in (0, 1):
        less = hashlib.sha256(" ".join(flags).encode())
        less.update(open(files[keep], "rb").read())
        assert less.hexdigest() != second.hexdigest()
    edited = hashlib.sha256(" ".join(flags).encode())
    edited.update(open(files[0], "rb").read() + b"\n")
    edited.update(open(files[1], "rb").read())
    assert edited.hexdigest() != second.hexdigest()
    source = inspect.getsource(_lib.build)
    assert "_later_digest(_source_digest(" in source and "_latest_digest(" in source and "LATEST_SOURCES" in source
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
        assert sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and "head16" in ln) == declared


def test_workspace_bytes_by_hand():
    wb = _lib.lib().cspn_head16_workspace_bytes
    assert wb(1, 1) == wb(16, 1) == wb(9, 32) == 9 * 16 * 32 * 2                              # rows padded to 16, channels to 32
    assert wb(9, 33) == wb(9, 64) == 9 * 16 * 64 * 2 and wb(13, 67) == 9 * 16 * 96 * 2
    assert wb(16, 2048) == 9 * 16 * 2048 * 2
    for bad in ((0, 64), (17, 64), (-1, 64), (9, 0), (9, -3), (9, 2 ** 24)):                   # the last: 2^31 packed elements or more
        assert wb(*bad) == 0, bad


def test_argument_checks_come_before_any_launch():
    lib = _lib.lib()
    err, fwd = lib.cspn_last_error, lib.cspn_head16_forward
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)                                       # noqa: E731
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                                          # noqa: E731
    ok = dict(x=16, w=ptrs(16, 16), dt=F32, outs=ptrs(16, 16), oc=ints(1, 8), n=2, work=16, shape=(2, 64, 3, 5), out=(6, 10))

    def call(**kw):
        a = dict(ok, **kw)
        return fwd(a["x"], a["w"], a["dt"], a["outs"], a["oc"], a["n"], a["work"], *a["shape"], *a["out"], None)

    for name in ("x", "w", "outs", "oc", "work"):
        assert not call(**{name: None}) and b"null" in err(), name
    assert not call(w=ptrs(16, None)) and b"null pointer (head 1)" in err()
    assert not call(outs=ptrs(None, 16)) and b"null pointer (head 0)" in err()
    assert not call(work=24) and b"16-byte" in err()
    for n in (0, 5, -1):
        assert not call(n=n, w=ptrs(16, 16, 16, 16, 16), outs=ptrs(16, 16, 16, 16, 16), oc=ints(1, 1, 1, 1, 1)) and b"n_heads must be in [1, 4]" in err()
    assert not call(oc=ints(9, 8)) and b"more than 16 output channels" in err()            # 17 over all heads
    assert not call(oc=ints(17), n=1) and b"more than 16 output channels" in err()
    assert not call(oc=ints(1, 0)) and b"head 1 has 0 output channels" in err()
    assert not call(oc=ints(-2, 8)) and b"head 0 has -2 output channels" in err()
    for out in ((0, 10), (7, 10), (6, 0), (6, 11), (-1, 4)):
        assert not call(out=out) and b"must lie in [1, 2H] x [1, 2W] = 6x10" in err(), out
    for dt in (2, -1, 7):
        assert not call(dt=dt) and b"weight_dtype must be fp32 or fp16" in err()
    for shape in ((0, 64, 3, 5), (2, 0, 3, 5), (2, 64, 0, 5), (2, 64, 3, 0)):
        assert not call(shape=shape) and b"bad shape" in err()
    assert not call(shape=(65536, 1, 3, 5)) and b"65535" in err()
    assert not call(shape=(2 ** 7, 2 ** 8, 2 ** 8, 2 ** 8), out=(1, 1)) and b"x has 2^31 elements" in err()
    assert not call(shape=(2 ** 7, 1, 2 ** 10, 2 ** 10), out=(2 ** 11, 2 ** 11), oc=ints(1, 4)) and b"output 1 has 2^31 elements" in err()
    assert not call(shape=(1, 2 ** 24, 1, 1), out=(1, 1)) and b"filters" in err()


def test_python_refusals():
    x, w1, w8 = torch.zeros(2, 6, 3, 5).half(), torch.zeros(1, 6, 3, 3), torch.zeros(8, 6, 3, 3)
    with torch.no_grad():
        for ws in ((w1, w8), (w1.half(), w8.half()), [w8]):                                # past the checks: refused as CPU tensors
            with pytest.raises(RuntimeError, match="ROCm device"):
                up_pooling_conv3x3_half(x, ws, 6, 10)
        for bad in (x.float(), x.bfloat16(), x.double()):
            with pytest.raises(ValueError, match="x must be fp16"):
                up_pooling_conv3x3_half(bad, (w1, w8), 6, 10)
        with pytest.raises(ValueError, match="one dtype"):
            up_pooling_conv3x3_half(x, (w1, w8.half()), 6, 10)
        for dt in (torch.bfloat16, torch.float64):
            with pytest.raises(ValueError, match="fp32 or fp16"):
                up_pooling_conv3x3_half(x, (w1.to(dt), w8.to(dt)), 6, 10)
        with pytest.raises(ValueError, match="tuple"):
            up_pooling_conv3x3_half(x, w8, 6, 10)
        with pytest.raises(ValueError, match=r"\[N,C,H,W\]"):
            up_pooling_conv3x3_half(x[0], (w8,), 6, 10)
        for ws in ((), (w1,) * 5):
            with pytest.raises(ValueError, match="between 1 and 4 heads"):
                up_pooling_conv3x3_half(x, ws, 6, 10)
        for bad in (torch.zeros(8, 5, 3, 3), torch.zeros(8, 6, 5, 5), torch.zeros(8, 6, 3), torch.zeros(0, 6, 3, 3)):
            with pytest.raises(ValueError, match=r"weight 1 must be \[O,6,3,3\]"):
                up_pooling_conv3x3_half(x, (w1, bad), 6, 10)
        with pytest.raises(ValueError, match="17 output channels"):
            up_pooling_conv3x3_half(x, (w8, w8, w1), 6, 10)
        for out in ((0, 10), (7, 10), (6, 11), (6, 0)):
            with pytest.raises(ValueError, match="must lie within"):
                up_pooling_conv3x3_half(x, (w8,), *out)
        with pytest.raises(ValueError, match="empty"):
            up_pooling_conv3x3_half(x[:0], (w8,), 6, 10)
        big = torch.zeros(1, 1, 1, 1).half().expand(2 ** 7, 6, 2 ** 11, 2 ** 11)           # 2^31 elements or more, no memory behind them
        with pytest.raises(ValueError, match="2\\^31"):
            up_pooling_conv3x3_half(big, (w8,), 1, 1)
    with torch.enable_grad():                                                              # forward only
        with pytest.raises(RuntimeError, match="forward-only.*stock blocks"):
            up_pooling_conv3x3_half(x.clone().requires_grad_(True), (w1, w8), 6, 10)
        with pytest.raises(RuntimeError, match="forward-only"):
            up_pooling_conv3x3_half(x, (w1, torch.nn.Parameter(w8)), 6, 10)
        with pytest.raises(RuntimeError, match="ROCm device"):                             # nothing requires a gradient: not refused for that
            up_pooling_conv3x3_half(x, (w1, w8), 6, 10)
    with torch.no_grad():                                                                  # the fp32 entry point is what it was
        with pytest.raises(ValueError, match="fp32 only"):
            up_pooling_conv3x3(x, (w1, w8), 6, 10)
        with pytest.raises(ValueError, match="fp32 only"):
            up_pooling_conv3x3(x, (w1.half(), w8.half()), 6, 10)


def test_model_dispatch_by_dtype_and_gradient(monkeypatch):
    """`fused_heads_forward`, which both models call: fp32 -> up_pooling_conv3x3, fp16 with no gradient needed -> the half entry,
    fp16 with one needed -> None (the stock blocks).  Decided on CPU tensors: both entry points are stood in for."""
    calls = []
    monkeypatch.setattr(upmod, "up_pooling_conv3x3", lambda *a: (calls.append("fp32"), "old")[1])
    monkeypatch.setattr(upmod, "up_pooling_conv3x3_half", lambda *a: (calls.append("half"), "new")[1])
    x, w = torch.zeros(1, 6, 3, 5), torch.nn.Parameter(torch.zeros(8, 6, 3, 3))
    with torch.no_grad():
        assert upmod.fused_heads_forward(x, (w,), 6, 10) == "old" and upmod.fused_heads_forward(x.half(), (w,), 6, 10) == "new"
        assert upmod.fused_heads_forward(x.half(), (w.half(),), 6, 10) == "new"
        assert upmod.fused_heads_forward(x.double(), (w,), 6, 10) == "old" and upmod.fused_heads_forward(x.bfloat16(), (w,), 6, 10) == "old"
    assert calls == ["fp32", "half", "half", "fp32", "fp32"]
    del calls[:]
    with torch.enable_grad():
        assert upmod.fused_heads_forward(x, (w,), 6, 10) == "old"                          # fp32: its own autograd path
        assert upmod.fused_heads_forward(x.half(), (w,), 6, 10) is None                    # a weight requires one
        assert upmod.fused_heads_forward(x.half().requires_grad_(True), (w.detach(),), 6, 10) is None
        assert upmod.fused_heads_forward(x.half(), (w.detach(),), 6, 10) == "new"          # nothing involved requires one
    assert calls == ["fp32", "half"]
    for net in (unet_ours, unet_cspn_nyu):
        src = inspect.getsource(net.ResNet.features)
        assert src.count("fused_heads_forward(") == 1 and "gud_up_proj_layer5(x)" in src
        assert len(net.resnet18(fused_heads=True).state_dict()) == len(net.resnet18().state_dict())
    assert len(unet_ours.resnet50(fused_heads=True).state_dict()) == 417


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def run(x, ws, oh, ow, weight_dtype=torch.float32):
    """The kernel through the Python entry point; the outputs as numpy fp16."""
    with torch.no_grad():
        outs = up_pooling_conv3x3_half(dev(x, torch.float16), [dev(w, weight_dtype) for w in ws], oh, ow)
    assert all(o.dtype == torch.float16 and o.is_contiguous() and tuple(o.shape) == (x.shape[0], w.shape[0], oh, ow) for o, w in zip(outs, ws))
    return [o.cpu().numpy() for o in outs]


def same_bits(got, want):
    return got.dtype == want.dtype == np.float16 and got.shape == want.shape and np.array_equal(got.view(np.uint16), want.view(np.uint16))


def check_integer_case(shape, out_hw, heads):
    x, ws, want, worst = c16.integer_case(shape, out_hw, heads)
    assert worst < 2048                                                                    # every sum exact, every result a fp16 value
    got = run(x, ws, *out_hw)
    assert all(same_bits(g, w + np.float16(0)) for g, w in zip(got, want)), (shape, out_hw, heads)      # + 0: an exact zero sum is +0
    return 1


def check_within_bound(what, got, want, bound):
    got = got.astype(np.float64)
    assert np.isfinite(got).all() and got.shape == want.shape == bound.shape
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print("%s: largest error / bound = %.4f" % (what, ratio))
    assert (err <= bound).all(), (what, ratio)
    return ratio


@pytest.mark.gpu
def test_integer_goldens_bit_equal():
    used = 0
    for name in INT_GOLDENS:
        z = load_golden(name)
        oh, ow, heads, pick = unpack(z)
        ys = pick("y")
        assert max(np.abs(y).max() for y in ys) < 2048 and np.abs(z["x"]).max() <= 3                                 # exact in fp16
        assert all(np.array_equal(y.astype(np.float16).astype(np.float64), y.astype(np.float64)) for y in ys)
        for weight_dtype in (torch.float32, torch.float16):
            got = run(z["x"].astype(np.float32), [w.astype(np.float32) for w in pick("w")], oh, ow, weight_dtype)
            assert all(same_bits(g, y.astype(np.float16) + np.float16(0)) for g, y in zip(got, ys)), name
        used += 1
    assert used == len(INT_GOLDENS) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("name", REAL_GOLDENS)
def test_real_goldens_within_the_bound(name):
    """Against the reference on the golden's inputs rounded to fp16, within the a-priori bound — and against the golden's own outputs,
    with what the rounding of the inputs can move them by: a factor is within 2^-11 relative (normal) or 2^-25 absolute (subnormal) of
    its fp16 value, so a product moves by at most (2^-10 + 2^-22) |w| |x| + 2^-25 (|w| + |x|) + 2^-50."""
    z = load_golden(name)
    oh, ow, heads, pick = unpack(z)
    x, ws = z["x"].astype(np.float64), [w.astype(np.float64) for w in pick("w")]
    assert max(np.abs(y).max() for y in pick("y")) < c16.HALF_MAX
    got = run(x, ws, oh, ow)
    _, exact = c16.reference(x, ws, oh, ow)
    bounds = c16.bound_half(x, ws, oh, ow)
    ax, aws = np.abs(x), [np.abs(w) for w in ws]
    moved = [(2.0 ** -10 + 2.0 ** -22) * p + 2.0 ** -25 * (q + r) + 2.0 ** -50 * 4 * x.shape[1]
             for p, q, r in zip(hc.forward(ax, aws, oh, ow), hc.forward(np.ones_like(x), aws, oh, ow), hc.forward(ax, [np.ones_like(w) for w in ws], oh, ow))]
    for h, (g, y, b, gold, m) in enumerate(zip(got, exact, bounds, pick("y"), moved)):
        check_within_bound("%s head %d" % (name, h), g, y, b)
        check_within_bound("%s head %d against the golden" % (name, h), g, gold.astype(np.float64), b + m)
    assert len(REAL_GOLDENS) == 4 and any(load_golden(n)["x"].shape[1] == 64 for n in REAL_GOLDENS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(c16.GEOMETRIES))
def test_integer_table_bit_equal(name):
    cases = c16.table_cases(name)
    assert len(cases) == len(c16.HEAD_SETS) * len(c16.CHANNELS) * len(c16.BATCHES) == 21 * 5 * 2
    assert {h for _, _, h in cases} >= {(o,) for o in range(1, 17)} | set(hc.HEAD_SETS)
    assert sum(check_integer_case(*case) for case in cases) == len(cases)                  # none skipped


@pytest.mark.gpu
def test_integer_shapes_of_the_fp32_heads_bit_equal():
    """heads_cases.INT_SHAPES x HEAD_SETS as the fp32 heads run them (the model's 114 x 152 map among them), and the 3 x 3-tile ragged
    geometry."""
    cases = [(shape, out_hw, heads) for shape, out_hw in hc.INT_SHAPES for heads in hc.HEAD_SETS]
    H, W, oh, ow = c16.RAGGED
    cases += [((B, C, H, W), (oh, ow), heads) for heads in hc.HEAD_SETS for C in (5, 67) for B in c16.BATCHES]
    assert len(cases) == 50 + 20 and sum(check_integer_case(*case) for case in cases) == len(cases)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 64, 67])
def test_real_cases_within_the_bound(C):
    H, W, oh, ow = c16.RAGGED
    x, ws = c16.make_inputs((2, C, H, W), (1, 8), False)
    want, exact = c16.reference(x, ws, oh, ow)
    got = run(x, ws, oh, ow)
    moved = 0
    for h, (g, y, b) in enumerate(zip(got, exact, c16.bound_half(x, ws, oh, ow))):
        check_within_bound("C=%d head %d" % (C, h), g, y, b)
        moved += int((g.astype(np.float64) != y).sum())
    assert moved > 0                                                                       # rounded results, not a copy of the fp64 ones
    half = run(x, ws, oh, ow, torch.float16)
    assert all(same_bits(a, b) for a, b in zip(got, half))


def run_raw(x, ws, oh, ow, out_offset=0, weight_dtype=torch.float16, pad=2048):
    """The entry point itself on buffers of the test's own: x between NaN guards, every output `out_offset` elements into a larger
    buffer of a sentinel, the workspace inside a larger buffer of a sentinel byte.  Returns the outputs (numpy) after checking the
    bands."""
    N, C, H, W = x.shape
    sentinel = -12288.0
    xbuf = torch.full((2 * pad + x.size,), float("nan"), device=DEV, dtype=torch.float16)
    xbuf[pad:pad + x.size] = dev(x, torch.float16).flatten()
    wd = [dev(w, weight_dtype) for w in ws]
    sizes = [N * w.shape[0] * oh * ow for w in ws]
    bufs = [torch.full((2 * pad + out_offset + s,), sentinel, device=DEV, dtype=torch.float16) for s in sizes]
    outs = [b[pad + out_offset:pad + out_offset + s] for b, s in zip(bufs, sizes)]
    nbytes = _lib.lib().cspn_head16_workspace_bytes(sum(w.shape[0] for w in ws), C)
    assert nbytes == 9 * 16 * (-(-C // c16.KC) * c16.KC) * 2
    wbuf = torch.full((2 * 4096 + nbytes,), 0xA5, device=DEV, dtype=torch.uint8)
    work = wbuf[4096:4096 + nbytes]
    assert work.data_ptr() % 16 == 0 and all(o.data_ptr() % 4 == (2 * out_offset) % 4 for o in outs)
    launch(torch.device(DEV), "cspn_head16_forward", xbuf[pad:].data_ptr(), upmod._ptrs(wd), F32 if weight_dtype == torch.float32 else F16,
           upmod._ptrs(outs), upmod._channels(wd), len(wd), work.data_ptr(), N, C, H, W, oh, ow)
    torch.cuda.synchronize()
    for b, s in zip(bufs, sizes):
        assert bool((b[:pad + out_offset] == sentinel).all()) and bool((b[pad + out_offset + s:] == sentinel).all())
    assert bool((wbuf[:4096] == 0xA5).all()) and bool((wbuf[4096 + nbytes:] == 0xA5).all())
    assert bool(torch.isnan(xbuf[:pad]).all()) and bool(torch.isnan(xbuf[pad + x.size:]).all())
    packed = work.view(torch.float16).view(9, 16, -1)                                      # [tap][row][channel], zero past the filters
    flat = torch.cat([w.to(torch.float16) for w in wd]).permute(2, 3, 0, 1).reshape(9, -1, C)
    assert torch.equal(packed[:, :flat.shape[1], :C], flat) and not bool(packed[:, flat.shape[1]:].any()) and not bool(packed[:, :, C:].any())
    return [o.view(N, w.shape[0], oh, ow).cpu().numpy() for o, w in zip(outs, ws)]


@pytest.mark.gpu
@pytest.mark.parametrize("what,out_hw_delta,out_offset", [("even_ow_aligned", (0, 1), 0), ("odd_ow", (0, 0), 0), ("even_ow_odd_offset", (0, 1), 1),
                                                          ("odd_ow_odd_offset", (1, 0), 3)])
def test_store_paths_and_guard_bands(what, out_hw_delta, out_offset):
    """The 4-byte stores (even ow, aligned outputs) and the 2-byte stores (odd ow; an output at an odd element offset), each inside
    sentinel bands, with NaN around x and a sentinel around the workspace."""
    H, W, oh, ow = c16.RAGGED
    oh, ow = oh + out_hw_delta[0], ow + out_hw_delta[1]
    assert (ow % 2 == 0) == what.startswith("even") and oh <= 2 * H and ow <= 2 * W
    for heads, C in (((1, 8), 67), ((3, 4, 3), 5), ((16,), 33)):                           # frame strides of the heads differ
        shape = (2, C, H, W)
        x, ws, want, worst = c16.integer_case(shape, (oh, ow), heads)
        assert worst < 2048
        for weight_dtype in (torch.float32, torch.float16):
            got = run_raw(x, ws, oh, ow, out_offset, weight_dtype)
            assert all(same_bits(g, w + np.float16(0)) for g, w in zip(got, want)), (what, heads, C)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", [0x7e007e00, 0x7c007c00], ids=["nan", "inf"])
def test_ragged_case_under_poisoned_lds(pattern):
    """NaN, and Inf, in both fp16 halves of every LDS word in front of every launch: the bits of the reference."""
    H, W, oh, ow = c16.RAGGED
    x, ws, want, worst = c16.integer_case((2, 35, H, W), (oh, ow), (1, 8))
    assert worst < 2048
    with lds_poison(pattern):
        got = run(x, ws, oh, ow)
        torch.cuda.synchronize()
    assert all(same_bits(g, w + np.float16(0)) for g, w in zip(got, want))


@pytest.mark.gpu
def test_batch_place_runs_and_weight_dtype_give_equal_bits():
    H, W, oh, ow = c16.RAGGED
    x, ws = c16.make_inputs((3, 67, H, W), (1, 8), False)
    ys = run(x, ws, oh, ow)
    assert all(same_bits(a, b) for a, b in zip(ys, run(x, ws, oh, ow)))                    # two runs
    for n in (0, 2):                                                                       # the frame alone at B = 1
        alone = run(x[n:n + 1], ws, oh, ow)
        assert all(same_bits(a[0], y[n]) for a, y in zip(alone, ys))
    pair = run(x[[2, 1, 2]], ws, oh, ow)                                                   # ... and at positions 0 and 2 of another B = 3
    assert all(same_bits(p[0], y[2]) and same_bits(p[2], y[2]) and same_bits(p[1], y[1]) for p, y in zip(pair, ys))
    w32 = [w + np.float32(2.0 ** -13) * np.sign(w) for w in ws]                            # fp32 filters that are no fp16 values
    assert any((c16.to_half(w) != w).any() for w in w32)
    a = run(x, w32, oh, ow, torch.float32)                                                 # rounded by the pack kernel ...
    b = run(x, [c16.to_half(w) for w in w32], oh, ow, torch.float16)                       # ... and beforehand, to nearest even
    assert all(same_bits(p, q) for p, q in zip(a, b))
    _, exact = c16.reference(x, w32, oh, ow)                                               # the reference rounds the filters itself
    for h, (p, y, bd) in enumerate(zip(a, exact, c16.bound_half(x, w32, oh, ow))):
        check_within_bound("fp32 filters, head %d" % h, p, y, bd)


@pytest.mark.gpu
def test_graph_capture_gives_the_eager_bits():
    H, W, oh, ow = c16.RAGGED
    x, ws = c16.make_inputs((2, 64, H, W), (1, 8), False)
    x2, _ = c16.make_inputs((2, 64, H, W), (1, 8), False, seed=1)
    wd = [dev(w) for w in ws]
    with torch.no_grad():
        a, a2 = dev(x, torch.float16), dev(x2, torch.float16)
        eager = [up_pooling_conv3x3_half(v, wd, oh, ow) for v in (a, a2)]
        sx = a.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            up_pooling_conv3x3_half(sx, wd, oh, ow)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = up_pooling_conv3x3_half(sx, wd, oh, ow)
        for v, want in ((a2, eager[1]), (a, eager[0])):                                    # two replays, the outputs overwritten in between
            sx.copy_(v)
            for o in outs:
                o.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(o.view(torch.int16), w.view(torch.int16)) for o, w in zip(outs, want))
    assert not torch.equal(eager[0][1], eager[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_non_finite_pixel_reaches_its_3x3_block_only(value):
    H, W, oh, ow = c16.RAGGED
    x, ws = c16.make_inputs((2, 35, H, W), (1, 8), False)
    ws = [np.where(w == 0, np.float32(0.5), w) for w in ws]                                # no zero weight: Inf x w is never NaN for that
    clean = run(x, ws, oh, ow)
    Hc, Wc = (oh + 1) // 2, (ow + 1) // 2
    spots = [(0, 0), (Hc - 1, Wc - 1), (c16.TH - 1, c16.TW - 1), (c16.TH, c16.TW), (3, c16.TW), (H - 1, W - 1)]      # the last: cropped away
    assert spots[-1][0] >= Hc and spots[-1][1] >= Wc
    for i, j in spots:
        bad = x.copy()
        bad[1, 17, i, j] = value
        got, want = run(bad, ws, oh, ow), c16.reference(bad, ws, oh, ow)[0]
        hit = np.zeros((oh, ow), bool)
        if i < Hc and j < Wc:
            hit[max(2 * i - 1, 0):2 * i + 2, max(2 * j - 1, 0):2 * j + 2] = True          # the 3 x 3 block around (2i, 2j), clipped
        for g, cl, w in zip(got, clean, want):
            assert same_bits(g[0], cl[0])                                                  # the other frame
            assert np.array_equal(g[1][:, ~hit].view(np.uint16), cl[1][:, ~hit].view(np.uint16))
            assert not np.isfinite(g[1][:, hit]).any()
            if not np.isnan(value):                                                        # +-Inf with the reference's signs
                assert np.array_equal(g[1][:, hit], w[1][:, hit])


@pytest.mark.gpu
def test_results_beyond_the_half_range_become_infinite():
    """Sums that are exact in fp32, so the conversion alone decides: 65519 -> 65504, the tie 65520 -> Inf (to even), 65521 -> Inf."""
    x = np.zeros((1, 2, 2, 2), np.float32)
    x[0, :, 0, 0], x[0, :, 0, 1], x[0, :, 1, 0], x[0, :, 1, 1] = (2047, 15), (2047, 16), (-2047, -16), (2047, 17)
    w = np.zeros((2, 2, 3, 3), np.float32)
    w[0, :, 1, 1], w[1, :, 1, 1] = (32, 1), (-32, -1)
    w[:, :, 0, 0] = 1
    want, exact = c16.reference(x, [w], 4, 4)
    assert [exact[0][0, 0, Y, X] for Y, X in ((0, 0), (0, 2), (2, 0), (2, 2))] == [65519, 65520, -65520, 65521]
    inf = np.float16("inf")
    assert [want[0][0, 0, Y, X] for Y, X in ((0, 0), (0, 2), (2, 0), (2, 2))] == [65504, inf, -inf, inf]
    assert want[0][0, 1, 0, 0] == -65504 and want[0][0, 1, 2, 0] == inf and np.isfinite(want[0][0, :, 1::2, 1::2]).all()
    got = run(x, [w], 4, 4)
    assert same_bits(got[0], want[0])
    big = np.full((1, 40, 3, 3), 60.0, np.float32)                                         # and far beyond: 40 x 60 x 30 per tap
    big[0, :, 1, 1] = -60.0
    ws = [np.full((2, 40, 3, 3), 30.0, np.float32)]
    ws[0][1] = 0.25
    want, _ = c16.reference(big, ws, 6, 6)
    assert (want[0] == inf).any() and (want[0] == -inf).any() and np.isfinite(want[0][0, 1]).all()
    assert same_bits(run(big, ws, 6, 6)[0], want[0])


def model_case(kind, seed=11, **switches):
    """tests/test_uptail.py's model: either network at 36 x 52, B = 2, batch norms with statistics that are not the initial ones."""
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
    return net.to(DEV), torch.rand(2, 4, 36, 52).to(DEV)


class Counter(object):
    """Stands in for the two fused entry points and the forward of the two stock blocks: counts, and keeps what the half entry saw."""

    def __init__(self, monkeypatch, net):
        self.n = dict(half=0, fp32=0, stock=0)
        self.seen = None
        real_half, real_fp32 = upmod.up_pooling_conv3x3_half, upmod.up_pooling_conv3x3

        def half(x, weights, oh, ow):
            self.n["half"] += 1
            outs = real_half(x, weights, oh, ow)
            self.seen = (x.detach().clone(), [w.detach().clone() for w in weights], oh, ow, [o.detach().clone() for o in outs])
            return outs

        def fp32(x, weights, oh, ow):
            self.n["fp32"] += 1
            outs = real_fp32(x, weights, oh, ow)
            self.seen32 = (x.detach().clone(), [w.detach() for w in weights], oh, ow, [o.detach().clone() for o in outs])
            return outs

        monkeypatch.setattr(upmod, "up_pooling_conv3x3_half", half)
        monkeypatch.setattr(upmod, "up_pooling_conv3x3", fp32)
        for block in (net.gud_up_proj_layer5, net.gud_up_proj_layer6):
            block.register_forward_hook(lambda *a: self.n.__setitem__("stock", self.n["stock"] + 1))

    def take(self):
        n, self.n = self.n, dict(half=0, fp32=0, stock=0)
        return (n["half"], n["fp32"], n["stock"])


def features(net, inp, how):
    if how == "autocast":
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            return net.features(inp)
    return net.features(inp.to(next(net.parameters()).dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["half", "autocast"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_models_half_heads_within_the_bound(kind, how, monkeypatch):
    """`resnet18(fused_heads=True)` after .half() and under fp16 autocast — a ValueError before the half entry existed."""
    net, inp = model_case(kind, fused_heads=True)
    net.eval()
    keys = list(net.state_dict())
    assert keys == list(model_case(kind)[0].state_dict())
    if how == "half":
        net.half()
    count = Counter(monkeypatch, net)
    with torch.no_grad():
        outs = features(net, inp, how)
    assert count.take() == (1, 0, 0) and list(net.state_dict()) == keys
    depth, guidance = (outs[0], outs[1]) if kind == "ours" else (outs[1], outs[0])
    assert depth.dtype == guidance.dtype == torch.float16 and depth.shape == (2, 1, 36, 52) and guidance.shape == (2, 8, 36, 52)
    x, ws, oh, ow, got = count.seen
    l5, l6 = net.gud_up_proj_layer5, net.gud_up_proj_layer6
    assert x.dtype == torch.float16 and x.shape == (2, 64, 18, 26) and (oh, ow) == (36, 52)
    assert all(w.dtype == (torch.float16 if how == "half" else torch.float32) for w in ws)
    assert torch.equal(ws[0], l5.conv1.weight) and torch.equal(ws[1], l6.conv1.weight[:8]) and ws[1].shape[0] == 8
    assert torch.equal(got[0], depth) and torch.equal(got[1], guidance)
    xn, wn = x.float().cpu().numpy(), [w.float().cpu().numpy() for w in ws]
    _, exact = c16.reference(xn, wn, oh, ow)
    for h, (g, y, b) in enumerate(zip(got, exact, c16.bound_half(xn, wn, oh, ow))):
        check_within_bound("%s %s head %d" % (kind, how, h), g.cpu().numpy(), y, b)
    # grad mode on, and train(): the stock blocks, the new entry not at all
    with torch.enable_grad():
        features(net, inp, how)
    assert count.take() == (0, 0, 2)
    net.train()
    with torch.enable_grad():
        features(net, inp, how)
    assert count.take() == (0, 0, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_fp32_model_runs_the_fp32_heads_as_before(kind, monkeypatch):
    net, inp = model_case(kind, fused_heads=True)
    net.eval()
    count = Counter(monkeypatch, net)
    with torch.no_grad():
        outs = features(net, inp, "fp32")
        assert count.take() == (0, 1, 0)
        x, ws, oh, ow, got = count.seen32
        depth, guidance = (outs[0], outs[1]) if kind == "ours" else (outs[1], outs[0])
        again = up_pooling_conv3x3(x, ws, oh, ow)                                           # the same function on what it was given
        count.take()
    assert depth.dtype == torch.float32 and torch.equal(got[0], depth) and torch.equal(got[1], guidance)
    assert torch.equal(again[0], depth) and torch.equal(again[1], guidance)
    with torch.enable_grad():                                                              # its autograd path, not the stock blocks
        outs = features(net, inp, "fp32")
        assert count.take() == (0, 1, 0) and outs[0].grad_fn is not None


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["half", "autocast"])
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_all_four_switches_in_half(kind, how, monkeypatch):
    net, inp = model_case(kind, fused_heads=True, fused_encoder=True, fused_decoder=upmod.DECODER_BLOCKS, fused_tail=upmod.DECODER_BLOCKS)
    net.eval()
    assert list(net.state_dict()) == list(model_case(kind)[0].state_dict())
    if how == "half":
        net.half()
    count = Counter(monkeypatch, net)
    with torch.no_grad():
        got = features(net, inp, how)
    assert count.take() == (1, 0, 0)
    assert all(getattr(net, n)._upconv_pack is not None and getattr(net, n)._tail_packs for n in upmod.DECODER_BLOCKS)
    assert all(g.dtype == torch.float16 and bool(torch.isfinite(g).all()) for g in got[:2])

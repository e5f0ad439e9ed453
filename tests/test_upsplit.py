"""The split products of the fused decoder-block head: ``up_pooling_conv5x5(..., precision="bf16x3")``, the dtype
CSPN_UPCONV_F32_BF16X3 of cspn_upconv_forward (include/cspn_upconv.h) and the `fused_decoder_precision` keyword of the two models.

References: the numpy restatements of tests/upconv_cases.py (the four-phase formula) and tests/upsplit_cases.py (the split and the
six kept products).  Integer-valued and dyadic cases are compared bit for bit — every kept term and every partial sum is exact in
fp32 there — real-valued cases against the a-priori bound of upsplit_cases.bound.

Largest error / bound seen on an MI355X (real-valued cases; the exact kernel on the same inputs against its own bound):
DESIGN.md §8 f-15."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import upconv_cases as uc
import upsplit_cases as us
from conftest import ROOT, lds_poison
from cspn_monodepth_amd import _host, _lib
from cspn_monodepth_amd._host import launch
from cspn_monodepth_amd.network import unet_cspn_nyu, unet_ours
from cspn_monodepth_amd.network import up_pooling as upmod
from cspn_monodepth_amd.network.up_pooling import UpconvPack, pack_upconv5x5, up_pooling, up_pooling_conv5x5

DEV = "cuda:0"
BLOCKS = upmod.DECODER_BLOCKS
X3 = 2


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_constant_in_header_and_loader():
    text = open(os.path.join(ROOT, "include", "cspn_upconv.h")).read()
    assert re.search(r"^#define CSPN_UPCONV_F32_BF16X3 2$", text, flags=re.M)
    assert re.search(r"^#define CSPN_UPCONV_ABI_VERSION 1$", text, flags=re.M)
    assert _lib.UPCONV_F32_BF16X3 == X3 and X3 not in (_lib.CSPN_F32, _lib.CSPN_F16)
    assert "BF16X3" not in open(os.path.join(ROOT, "include", "cspn_hip.h")).read()       # that header is part of code_digest()


def test_forward_reaches_the_argument_checks_with_the_new_dtype():
    lib = _lib.lib()
    fwd, err = lib.cspn_upconv_forward, lib.cspn_last_error
    one, o1 = (ctypes.c_void_p * 1)(16), (ctypes.c_int * 1)(1)
    assert not fwd(16, X3, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, 5, 4, None)
    assert b"[1, 2H]" in err() and b"fp32" not in err()
    assert not fwd(16, X3, 16, 16, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"together" in err()
    assert not fwd(None, X3, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"null" in err()
    for other in (3, _lib.CSPN_F16, -1):
        assert not fwd(16, other, 16, None, None, 0, one, o1, 1, 1, 1, 2, 2, 4, 4, None) and b"fp32" in err()
    assert not lib.cspn_upconv_pack(one, o1, 1, 3, 5, 5, X3, 16, None) and b"fp32" in err()      # the pack is unchanged


def test_signatures_end_with_the_new_keyword():
    p = list(inspect.signature(up_pooling_conv5x5).parameters.values())[-1]
    assert p.name == "precision" and p.default is None
    for net in (unet_ours, unet_cspn_nyu):
        p = list(inspect.signature(net.ResNet.__init__).parameters.values())[-1]
        assert p.name == "fused_decoder_precision" and p.default is None
        with torch.device("meta"):
            a, b = net.resnet18(fused_decoder=True), net.resnet50(fused_decoder=True, fused_decoder_precision="bf16x3")
            with pytest.raises(ValueError, match="fused_decoder_precision"):
                net.resnet18(fused_decoder_precision="tf32")
        assert a.fused_decoder_precision is None and all(getattr(a, n).fused_precision is None for n in BLOCKS)
        assert b.fused_decoder_precision == "bf16x3" and all(getattr(b, n).fused_precision == "bf16x3" for n in BLOCKS)
        assert a.fused_decoder == b.fused_decoder                            # the keyword selects no block
        assert net.resnet18(fused_decoder_precision="bf16x3").fused_decoder == ()
    assert upmod.FusedHead.fused_precision is None


def test_python_refusals_need_no_device():
    x, w3 = torch.zeros(2, 3, 4, 5), torch.zeros(3, 3, 5, 5)
    for bad in ("tf32", "BF16X3", "", "fp32"):
        with pytest.raises(ValueError, match="precision must be"):
            up_pooling_conv5x5(x, (w3,), 8, 10, precision=bad)
    with pytest.raises(ValueError, match='precision="bf16x3".*fp32 x'):
        up_pooling_conv5x5(x.half(), (w3,), 8, 10, precision="bf16x3")
    half_pack = UpconvPack(None, None, None, (3,), 3, 3, (w3,), dtype=torch.float16)
    with pytest.raises(ValueError, match='precision="bf16x3".*pack of torch.float16'):
        up_pooling_conv5x5(x, half_pack, 8, 10, precision="bf16x3")
    with pytest.raises(ValueError, match='precision="bf16x3"'):
        up_pooling_conv5x5(x.half(), half_pack, 8, 10, precision="bf16x3")
    for ok in (None, "exact", "bf16x3"):                                     # everything in order: refused as CPU tensors
        with pytest.raises(RuntimeError, match="ROCm device"):
            up_pooling_conv5x5(x, (w3,), 8, 10, precision=ok)


def test_split_is_exact_and_the_dropped_terms_are_small():
    rng = np.random.RandomState(7)
    v = (rng.standard_normal(1 << 16) * np.exp2(rng.randint(-40, 40, size=1 << 16))).astype(np.float32)
    v1, v2, v3 = us.split(v)
    for t in (v1, v2, v3):
        assert not (t.view(np.uint32) & 0xFFFF).any()                        # bf16 values
    assert np.array_equal(v1.astype(np.float64) + v2.astype(np.float64) + v3.astype(np.float64), v.astype(np.float64))
    assert np.array_equal((v - v1) - v2, v3)                                 # the second residual is a bf16 number as it stands
    assert np.array_equal(us.bf16(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], np.float32)),
                          np.array([1, 1 + 2.0 ** -6, 1 + 2.0 ** -7], np.float32))      # ties to even, and above a tie
    w = (rng.standard_normal(1 << 16) * np.exp2(rng.randint(-40, 40, size=1 << 16))).astype(np.float32)
    xs, ws = [t.astype(np.float64) for t in us.split(v)], [t.astype(np.float64) for t in us.split(w)]
    six = sum(ws[i - 1] * xs[j - 1] for i, j in us.TERMS)
    exact = v.astype(np.float64) * w.astype(np.float64)
    assert (np.abs(six - exact) <= us.DROPPED * np.abs(exact)).all() and (six != exact).any()
    for i, j in us.TERMS:                                                    # each kept product is exact in fp32
        p = ws[i - 1] * xs[j - 1]
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)


@pytest.mark.parametrize("shape,out_hw,both", us.REAL_CASES[:2], ids=lambda v: "x".join(map(str, v)))
def test_six_product_sum_within_the_dropped_bound(shape, out_hw, both):
    filters = uc.filters_of(both)
    x, ws, _, _ = uc.make_inputs(uc.case_seed(shape, out_hw, filters) + 1, shape, filters, False)
    six = sum(us.six_terms(x, ws, *out_hw))
    exact = uc.accumulate(x.astype(np.float64), [w.astype(np.float64) for w in ws], *out_hw)
    A = uc.accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], *out_hw)
    assert (np.abs(six - exact) <= us.DROPPED * A).all() and (six != exact).any()


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(x, ws, oh, ow, scale=None, shift=None, relu=0, precision="bf16x3"):
    with torch.no_grad():
        outs = up_pooling_conv5x5(dev(x), tuple(dev(w) for w in ws), oh, ow, None if scale is None else dev(scale),
                                  None if shift is None else dev(shift), relu, precision=precision)
    assert isinstance(outs, tuple) and len(outs) == len(ws)
    assert all(o.is_contiguous() and o.dtype == torch.float32 and tuple(o.shape) == (x.shape[0], w.shape[0], oh, ow) for o, w in zip(outs, ws))
    return outs


def same_bits(t, a):
    a = np.asarray(a)
    return t.dtype == torch.float32 and tuple(t.shape) == a.shape and np.array_equal(t.detach().cpu().numpy().view(np.uint32), a.astype(np.float32).view(np.uint32))


def relu_boundaries(filters):
    return sorted({0, filters[0], sum(filters)})


def integer_case(shape, out_hw, filters):
    """Integers split into v2 = v3 = 0: tiles, taps, phases, edges and the epilogue, bit for bit."""
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters), shape, filters, True)
    acc = uc.accumulate(np.abs(x.astype(np.float64)), [np.abs(w.astype(np.float64)) for w in ws], *out_hw)
    assert 4 * acc.max() + 5 < 2 ** 24
    for relu in relu_boundaries(filters):
        want = uc.restate(x, ws, *out_hw, scale, shift, relu)
        for g, w in zip(run(x, ws, *out_hw, scale, shift, relu), want):
            assert same_bits(g, w + 0.0), (shape, out_hw, filters, relu)
    for g, w in zip(run(x, ws, *out_hw), uc.restate(x, ws, *out_hw)):
        assert same_bits(g, w + 0.0), (shape, out_hw, filters, "plain")


@pytest.mark.gpu
@pytest.mark.parametrize("hw,out_hw", uc.GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_integer_cases_bit_equal_to_the_restatement(hw, out_hw):
    for C, both, B in itertools.product(us.CHANNELS, us.FILTER_SETS, uc.BATCHES):
        integer_case((B, C) + hw, out_hw, uc.filters_of(both))


@pytest.mark.gpu
def test_integer_case_over_several_chunks_and_tiles():
    integer_case(uc.BIG["shape"], uc.BIG["out_hw"], uc.BIG["filters"])


@pytest.mark.gpu
def test_integer_cases_over_several_m_tiles():
    """mt > 0 in fwd<F32X3>, whose filter tile is found two flat channels per thread: upconv_cases.M_TILE_FILTER_SETS, bit for bit."""
    for shape, out_hw, filters in uc.m_tile_shapes():
        integer_case(shape, out_hw, filters)


@pytest.mark.gpu
def test_ragged_m_tile_under_poisoned_lds():
    shape, out_hw, filters = uc.M_TILE_POISON_CASE
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters), shape, filters, True)
    plain = run(x, ws, *out_hw, scale, shift, filters[0])
    with lds_poison(0x7fc07fc0):                                             # NaN in both bf16 halves of every word
        got = run(x, ws, *out_hw, scale, shift, filters[0])
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, plain)) and not any(bool(torch.isnan(g).any()) for g in got)


def dyadic_case(kind, seed, shape, out_hw, filters, live=None):
    x, ws = us.dyadic_inputs(kind, seed, shape, filters, live)
    xs, wss = us.split(x), [us.split(w) for w in ws]
    for i, j in us.TERMS:                                                    # every kept term is a multiple of 2^-18
        assert us.grain(xs[j - 1]) + max(us.grain(w[i - 1]) for w in wss) <= 18
    for i, j in ((2, 3), (3, 2), (3, 3)):                                    # nothing is dropped
        assert not xs[j - 1].any() or not any(w[i - 1].any() for w in wss)
    used = {(i, j) for i, j in us.TERMS if xs[j - 1].any() and any(w[i - 1].any() for w in wss)}
    assert used == {"a": {(1, 1), (1, 2), (1, 3)}, "b": {(1, 1), (2, 1), (3, 1)}, "c": {(1, 1), (1, 2), (2, 1), (2, 2)}}[kind]
    assert sum(us.six_terms(x, ws, *out_hw, absolute=True)).max() < 2 ** 6  # sum |terms| of every output
    want = uc.restate(x, ws, *out_hw)
    assert np.array_equal(np.concatenate(want, 1), sum(us.six_terms(x, ws, *out_hw)))
    for w in want:
        assert np.array_equal(w.astype(np.float32).astype(np.float64), w)   # representable in fp32
    for relu in (0, filters[0]):
        for g, w in zip(run(x, ws, *out_hw, relu=relu), uc.restate(x, ws, *out_hw, relu_channels=relu)):
            assert same_bits(g, w + 0.0), (kind, shape, out_hw, relu)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("kind", us.DYADIC_KINDS)
def test_dyadic_cases_pin_every_kept_product_class(kind):
    for n, (C, (hw, out_hw)) in enumerate(itertools.product(us.DYADIC_DENSE_CHANNELS, us.DYADIC_GEOMETRIES)):
        dyadic_case(kind, 100 + n, (2, C) + hw, out_hw, (3, 3))
    C, live = us.DYADIC_SPARSE
    for n, (hw, out_hw) in enumerate(us.DYADIC_GEOMETRIES):
        want = dyadic_case(kind, 200 + n, (1, C) + hw, out_hw, (17, 16), live)
        assert all(w.any() for w in want)


def errors_against_fp64(what, x, ws, oh, ow, scale, shift, relu, extra=0):
    """This path and the exact kernel on the same inputs against the fp64 restatement: the largest error / bound of each under its
    own bound (printed), and this path's held to its bound."""
    want = np.concatenate(uc.restate(x, ws, oh, ow, scale, shift, relu), 1)
    got = np.concatenate([g.cpu().numpy().astype(np.float64) for g in run(x, ws, oh, ow, scale, shift, relu)], 1)
    exact = np.concatenate([g.cpu().numpy().astype(np.float64) for g in run(x, ws, oh, ow, scale, shift, relu, precision="exact")], 1)
    b_split, b_exact = us.bound(x, ws, oh, ow, scale, shift, extra), uc.bound(x, ws, oh, ow, scale, shift, extra)
    e_split, e_exact = np.abs(got - want), np.abs(exact - want)
    big = np.abs(want).max()
    print("%s: bf16x3 error / bound = %.4f (max error %.3e), exact kernel error / its bound = %.4f (max error %.3e), max |bf16x3 - exact| "
          "/ max |y| = %.3e" % (what, (e_split[b_split > 0] / b_split[b_split > 0]).max(), e_split.max(),
                                (e_exact[b_exact > 0] / b_exact[b_exact > 0]).max(), e_exact.max(), np.abs(got - exact).max() / big))
    assert (e_split <= b_split).all(), what
    assert e_split.max() > 0 and (got != exact).any()                        # fp32 results of another arithmetic


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out_hw,both", us.REAL_CASES, ids=lambda v: "x".join(map(str, v)))
def test_real_cases_within_the_a_priori_bound(shape, out_hw, both):
    filters = uc.filters_of(both)
    x, ws, scale, shift = uc.make_inputs(uc.case_seed(shape, out_hw, filters) + 1, shape, filters, False)
    assert min(np.abs(t[t != 0]).min() for t in [x] + ws) > 2.0 ** -103 and max(np.abs(t).max() for t in [x] + ws) < 2.0 ** 100
    for relu in relu_boundaries(filters):
        errors_against_fp64("%s relu %d" % (shape, relu), x, ws, *out_hw, scale, shift, relu)
    errors_against_fp64("%s plain" % (shape,), x, ws, *out_hw, None, None, 0)


@pytest.mark.gpu
def test_batch_place_and_determinism():
    shape, out_hw, filters = (3,) + uc.BIG["shape"][1:], uc.BIG["out_hw"], uc.BIG["filters"]
    x, ws, scale, shift = uc.make_inputs(91, shape, filters, False)
    ys = run(x, ws, *out_hw, scale, shift, filters[0])
    again = run(x, ws, *out_hw, scale, shift, filters[0])
    assert all(torch.equal(a, b) for a, b in zip(ys, again))
    for n in range(3):                                                       # B = 3 against three B = 1 calls
        alone = run(x[n:n + 1], ws, *out_hw, scale, shift, filters[0])
        assert all(torch.equal(a[0], b[n]) for a, b in zip(alone, ys))


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
    launch(torch.device(DEV), "cspn_upconv_forward", xd.data_ptr(), X3, pack.packed.data_ptr(), sd.data_ptr(), hd.data_ptr(),
           filters[0], ptrs, (ctypes.c_int * len(outs))(*filters), len(outs), *shape, *out_hw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, want))
    keep = torch.ones_like(buf, dtype=torch.bool)
    at = pad
    for s in sizes:
        keep[at:at + s] = False
        at += s + pad
    assert int(keep.sum()) == pad * (len(sizes) + 1) and bool((buf[keep] == sentinel).all())      # guard bands on both sides
    if out_hw[0] < 2 * shape[2] - 1:                                         # the compact pixels the crop removed are not read
        xn = x.copy()
        xn[:, :, (out_hw[0] + 1) // 2:, :] = np.nan
        xn[:, :, :, (out_hw[1] + 1) // 2:] = np.nan
        assert all(torch.equal(a, b) for a, b in zip(run(xn, ws, *out_hw, scale, shift, filters[0]), want))


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf, 3.4e38], ids=["nan", "inf", "-inf", "above_bf16"])
def test_non_finite_values_reach_only_the_windows_that_cover_them(poison):
    """x[0,1,2,3] is covered by the windows of rows 2..6, columns 4..8.  A NaN gives NaN there, as in the exact kernel.  An Inf — or
    a finite value that rounds to Inf in bf16 — has v - v1 = NaN: NaN at every such output.  For an Inf the exact kernel gives +-Inf
    there (0 where a ReLU meets -Inf): whatever it makes non-finite is non-finite here too, the header's rule.  Everything else
    keeps its bits."""
    x, ws, scale, shift = uc.make_inputs(93, (1, 2, 5, 6), (3, 2), False)
    clean = torch.cat(run(x, ws, 10, 12, scale, shift, 3), 1)
    x[0, 1, 2, 3] = poison
    y = torch.cat(run(x, ws, 10, 12, scale, shift, 3), 1)
    exact = torch.cat(run(x, ws, 10, 12, scale, shift, 3, precision="exact"), 1)
    window = torch.zeros(10, 12, dtype=torch.bool, device=DEV)
    window[2:7, 4:9] = True
    assert bool(torch.isnan(y[0, :, window]).all())
    assert bool(torch.isfinite(y[0, :, ~window]).all()) and torch.equal(y[0, :, ~window], clean[0, :, ~window])
    assert not bool((~torch.isfinite(exact) & torch.isfinite(y)).any())      # non-finite in the exact kernel: non-finite here
    if np.isinf(poison):
        assert bool(torch.isinf(exact[0, :, window]).any())                  # ... Inf there, NaN here: as stated


@pytest.mark.gpu
def test_graph_capture_of_forward_calls_replays_with_equal_bits():
    shape, out_hw, filters = uc.BIG["shape"], uc.BIG["out_hw"], uc.BIG["filters"]
    x, ws, scale, shift = uc.make_inputs(94, shape, filters, False)
    with torch.no_grad():
        pack = pack_upconv5x5(tuple(dev(w) for w in ws), None, (True, False))
        sx = dev(x)
        eager = up_pooling_conv5x5(sx, pack, *out_hw, precision="bf16x3")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            up_pooling_conv5x5(sx, pack, *out_hw, precision="bf16x3")
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                        # forward-only calls under no_grad; no backward is captured
            outs = up_pooling_conv5x5(sx, pack, *out_hw, precision="bf16x3")
        for _ in range(2):
            for t in outs:
                t.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, eager))


@pytest.mark.gpu
def test_one_pack_serves_both_precisions():
    shape, out_hw, filters = (2, 33, 5, 7), (9, 13), (17, 16)
    x, ws, scale, shift = uc.make_inputs(96, shape, filters, False)
    with torch.no_grad():
        pack = pack_upconv5x5(tuple(dev(w) for w in ws), None, (True, False))
        before = pack.packed.clone()
        xd = dev(x)
        first = up_pooling_conv5x5(xd, pack, *out_hw, precision="exact")
        split = up_pooling_conv5x5(xd, pack, *out_hw, precision="bf16x3")
        second = up_pooling_conv5x5(xd, pack, *out_hw)
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(pack.packed, before) and not pack.stale()
    assert pack.dtype == torch.float32 and any(not torch.equal(a, b) for a, b in zip(first, split))
    assert all(torch.allclose(a, b, rtol=1e-4, atol=1e-4) for a, b in zip(first, split))


def model_case(kind, seed=11, **switches):
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
    return net.to(DEV).eval(), inp.to(DEV)


class Recorder(object):
    """Stands in for up_pooling_conv5x5 and for launch inside network.up_pooling: keeps what went into and came out of the first,
    and the entry point and dtype argument of every decoder-head launch."""

    def __init__(self, monkeypatch):
        self.calls, self.launches, self.real, self.real_launch = [], [], upmod.up_pooling_conv5x5, upmod.launch
        monkeypatch.setattr(upmod, "up_pooling_conv5x5", self)
        monkeypatch.setattr(upmod, "launch", self.launch)

    def __call__(self, x, pack, oh, ow, *rest, **kw):
        outs = self.real(x, pack, oh, ow, *rest, **kw)
        self.calls.append((x.detach().clone(), pack, (oh, ow), outs, kw))
        return outs

    def launch(self, device, name, *args):
        if name in ("cspn_upconv_forward", "cspn_uphalf_forward"):
            self.launches.append((name, args[1] if name == "cspn_upconv_forward" else None, args))
        return self.real_launch(device, name, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_models_fused_blocks_within_the_bound(kind, monkeypatch):
    net, inp = model_case(kind, fused_decoder=True, fused_decoder_precision="bf16x3")
    plain, _ = model_case(kind, fused_decoder=True)
    assert list(net.state_dict()) == list(plain.state_dict()) == list(model_case(kind)[0].state_dict())
    rec = Recorder(monkeypatch)
    with torch.no_grad():
        net.features(inp)
    assert len(rec.calls) == len(BLOCKS) and [(n, d) for n, d, _ in rec.launches] == [("cspn_upconv_forward", X3)] * len(BLOCKS)
    for name, (x, pack, (oh, ow), outs, kw) in zip(BLOCKS, rec.calls):
        block = getattr(net, name)
        assert kw == {"precision": "bf16x3"} and pack is block._upconv_pack and pack.dtype == torch.float32
        ws = [block.conv1.weight.detach().cpu().numpy(), block.sc_conv1.weight.detach().cpu().numpy()]
        folded = [uc.fold(*(t.detach().cpu().numpy() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)), bn.eps)
                  for bn in (block.bn1, block.sc_bn1)]
        scale, shift = np.concatenate([f[0] for f in folded]), np.concatenate([f[1] for f in folded])
        xn = x.cpu().numpy()
        want = np.concatenate(uc.restate(xn, ws, oh, ow, scale, shift, ws[0].shape[0]), 1)
        err = np.abs(np.concatenate([o.cpu().numpy().astype(np.float64) for o in outs], 1) - want)
        bound = us.bound(xn, ws, oh, ow, scale, shift, extra=4)
        print("%s %s: largest error / bound = %.4f" % (kind, name, (err[bound > 0] / bound[bound > 0]).max()))
        assert (err <= bound).all(), name
    # the recorded arguments: fp32 x and outputs, the block's own fp32 pack
    for (name, dtype, args), (x, pack, (oh, ow), outs, _) in zip(rec.launches, rec.calls):
        assert args[2] == pack.packed.data_ptr() and tuple(args[-6:]) == tuple(x.shape) + (oh, ow) and all(o.dtype == torch.float32 for o in outs)
    del rec.calls[:], rec.launches[:]
    with torch.no_grad():                                                    # without the keyword: the exact kernel
        plain.features(inp)
    assert [(n, d) for n, d, _ in rec.launches] == [("cspn_upconv_forward", _lib.CSPN_F32)] * len(BLOCKS)
    assert all(kw == {} for _, _, _, _, kw in rec.calls)
    del rec.calls[:], rec.launches[:]
    with torch.no_grad():                                                    # a half input under the same model: the fp16 family
        net.half().features(inp.half())
    assert [n for n, _, _ in rec.launches] == ["cspn_uphalf_forward"] * len(BLOCKS) and all(kw == {} for _, _, _, _, kw in rec.calls)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_train_mode_and_grad_mode_do_not_call_the_entry_point(kind, monkeypatch):
    net, inp = model_case(kind, fused_decoder=True, fused_decoder_precision="bf16x3")
    rec = Recorder(monkeypatch)
    with torch.enable_grad():                                                # eval mode, grad mode on
        net.features(inp)
    net.train()
    with torch.no_grad():                                                    # train mode, grad mode off
        net.features(inp)
    assert rec.calls == [] and rec.launches == []
    net.eval()
    with torch.no_grad():
        net.features(inp)
    assert len(rec.calls) == len(BLOCKS) and all(d == X3 for _, d, _ in rec.launches)


# d = max |model - exact-fused fp32 model| over blur depth and guidance.  The stock fp32 model (MIOpen convolutions, which do not repeat
# the exact kernel's bits) sets the scale: an fp32-class arithmetic stays within a small multiple of it.  F is twice the largest ratio
# d_split / d_stock seen in four runs on an MI355X, and never above 8.  The four runs, d_split / d_stock in units
# of 1e-8: unet_ours 5.2 / 4.5, 5.2 / 6.0, 5.2 / 6.0, 5.2 / 5.2 (ratios 1.17, 0.88, 0.88, 1.00); unet_cspn_nyu 5.6 / 5.2, 4.5 / 6.0,
# 6.0 / 4.5, 5.2 / 4.5 (1.07, 0.75, 1.33, 1.17).  Both distances are 6 to 8 units in the last place of the outputs.
END_TO_END_FACTOR = 2 * 1.334


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ours", "nyu"])
def test_end_to_end_distance_to_the_exact_fused_model(kind):
    net, inp = model_case(kind, fused_decoder=True, fused_decoder_precision="bf16x3")

    def outputs():
        with torch.no_grad():
            f = net.features(inp)
        return (f[0], f[1]) if kind == "ours" else (f[1], f[0])             # blur depth, guidance

    split = outputs()
    upmod.select_fused_precision(net, None)
    exact = outputs()
    upmod.select_fused_decoder(net, False)
    stock = outputs()
    d_split = max(float((a - b).abs().max()) for a, b in zip(split, exact))
    d_stock = max(float((a - b).abs().max()) for a, b in zip(stock, exact))
    print("%s: d_split = %.3e, d_stock = %.3e, ratio = %.3f" % (kind, d_split, d_stock, d_split / d_stock))
    assert d_stock > 0 and d_split > 0
    assert d_split <= END_TO_END_FACTOR * d_stock

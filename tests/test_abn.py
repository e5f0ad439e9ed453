"""In-Place Activated BatchNorm (cspn_monodepth_amd/network/inplace_abn.py, include/cspn_abn.h) against golden G20: the
reference's own bn.InPlaceABN on the CPU in fp32, itself held to the fp64 restatement tests/abn_cases.restate at 2e-6
(tests/golden/make_golden_g20.py).

  * CPU: the header / library / loader contract, the digest lists, the plan, the fixtures against the restatement, every
    refusal of the Python layer, the module surface and convert_batchnorm;
  * GPU: every G20 case at README "Parity"'s fp32 bar (max |got - want| <= 1e-5 max |want|; dx of a zero-weight channel:
    abn_cases.zero_channel_dx_bar) for the output, dx, dweight, dbias and both running statistics; the sizes at which the plan
    changes path against the restatement; the in-place contract; equal bits run after run; a captured training forward; a decoder
    block through convert_batchnorm against stock ops; InPlaceABNSync at world size 2."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import abn_cases as ac
from conftest import ROOT, golden_names, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import network
from cspn_monodepth_amd.network import inplace_abn as A

DEV = "cuda:0"
NAMES = ["g20_abn_" + n for n in ac.CASES]
gpu = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def case_of(name):
    """(case, inputs, golden arrays) of a G20 file; the inputs are regenerated where the file holds a sub-sample."""
    z = load_golden(name)
    case = ac.CASES[name[len("g20_abn_"):]]
    inp = ac.make_inputs(case, float(z["offset"]))
    return case, inp, z


def module_for(case, inp, cls=None, device=DEV):
    mod = (cls or A.InPlaceABN)(case["shape"][1], eps=case["eps"], momentum=case["momentum"], affine=case["affine"],
                                activation=case["activation"], slope=case["slope"]).to(device)
    with torch.no_grad():
        if case["affine"]:
            mod.weight.copy_(torch.from_numpy(inp["weight"]))
            mod.bias.copy_(torch.from_numpy(inp["bias"]))
        mod.running_mean.copy_(torch.from_numpy(inp["running_mean"]))
        mod.running_var.copy_(torch.from_numpy(inp["running_var"]))
    return mod.train(case["training"])


def run_device(case, inp, x=None):
    """dict of abn_cases.FIELDS (numpy) from one forward + backward of the module on the device; checks the in-place contract."""
    mod = module_for(case, inp)
    leaf = (dev(inp["x"]) if x is None else x).requires_grad_(True)
    work = leaf.clone()
    out = mod(work)
    assert out.data_ptr() == work.data_ptr() and out.shape == leaf.shape
    kept = out.detach().clone()
    cot = dev(inp["cot"])
    cot_before = cot.clone()
    out.backward(cot)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(kept)) and torch.equal(bits(cot), bits(cot_before))      # neither is modified
    res = dict(out=kept, dx=leaf.grad, running_mean=mod.running_mean, running_var=mod.running_var,
               dweight=mod.weight.grad if case["affine"] else None, dbias=mod.bias.grad if case["affine"] else None)
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in res.items()}


def assert_within(errs, what):
    print(what, {k: "%.3g" % (v * ac.DEVICE_BAR) if "zero" not in k else "%.3g of its bar" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= 1.0}
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------ CPU
def test_fixture_set_is_complete():
    assert sorted(golden_names("g20_abn_")) == sorted(NAMES)
    for n in NAMES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) <= ac.MAX_FILE_BYTES


def test_header_declares_six_symbols_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "cspn_abn.h")).read()
    assert re.search(r"CSPN_ABN_ACT_LEAKY_RELU = 0, CSPN_ABN_ACT_ELU = 1, CSPN_ABN_ACT_NONE = 2", src)
    assert (_lib.ABN_ACT_LEAKY_RELU, _lib.ABN_ACT_ELU, _lib.ABN_ACT_NONE) == (0, 1, 2)


def test_plan_needs_no_device_and_has_two_regimes():
    deep, wide = A.abn_plan(3, 2048, 8 * 10), A.abn_plan(3, 64, 114 * 152)
    assert deep["regime"] == "small" and deep["channels_per_workgroup"] > 1 and deep["workgroups_per_channel"] == 1
    assert wide["regime"] == "split" and wide["channels_per_workgroup"] == 1
    assert 64 * wide["workgroups_per_channel"] >= 256                       # a 64-channel layer still fills the part
    assert wide["elements_per_workgroup"] % 4 == 0
    assert wide["elements_per_workgroup"] * wide["workgroups_per_channel"] >= 3 * 114 * 152
    limit = deep["small_limit"]
    assert A.abn_plan(1, 3, limit)["regime"] == "small" and A.abn_plan(1, 3, limit + 1)["regime"] == "split"
    L = _lib.lib()
    assert L.cspn_abn_workspace_bytes(1, 3, limit) == 0 and L.cspn_abn_workspace_bytes(1, 3, limit + 1) > 0
    with pytest.raises(RuntimeError, match="at least 1"):
        A.abn_plan(0, 3, 4)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_fixture(name):
    case, inp, z = case_of(name)
    assert tuple(int(v) for v in z["shape"]) == case["shape"] and str(z["activation"]) == case["activation"]
    assert bool(z["training"]) == case["training"] and bool(z["affine"]) == case["affine"] and float(z["momentum"]) == case["momentum"]
    want = ac.restate_case(case, inp)
    if case["full"]:
        index = np.arange(0, int(np.prod(case["shape"])), int(z["stride"]))
        got = dict(out=z["out_sub"], dx=z["dx_sub"], dweight=z["dweight"], dbias=z["dbias"], running_mean=z["running_mean"],
                   running_var=z["running_var"])
        errs = ac.compare(got, want, inp["weight"], ac.ORACLE_BAR, case["eps"], index=index)
    else:
        for k, src in (("x", "x"), ("cot", "cot"), ("running_mean", "running_mean_in"), ("running_var", "running_var_in")):
            assert np.array_equal(inp[k], z[src]), k
        errs = ac.compare({f: z.get(f) for f in ac.FIELDS}, want, inp["weight"], ac.ORACLE_BAR, case["eps"])
    assert errs and all(v <= 1.0 for v in errs.values()), errs
    if "offset" in name:
        assert float(z["offset"]) >= 16.0                                   # the channel means sit that many deviations from 0


def test_every_refusal_comes_before_any_launch():
    rm, rv = torch.zeros(3), torch.ones(3)
    with pytest.raises(ValueError, match="Non-contiguous input"):
        A.inplace_abn(torch.rand(2, 5, 4, 3).transpose(1, 3), None, None, rm, rv)
    with pytest.raises(ValueError, match="Non-contiguous input"):
        A.InPlaceABN(3)(torch.rand(2, 3, 4, 8)[..., ::2])
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with pytest.raises(TypeError, match="fp32 only"):
            A.inplace_abn(torch.rand(2, 3, 4, 4).to(dt), None, None, rm, rv)
    with pytest.raises(TypeError, match="fp32 only"):
        A.InPlaceABN(3).double()(torch.rand(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):                  # no CPU fallback
        A.inplace_abn(torch.rand(2, 3, 4, 4), None, None, rm, rv)
    with pytest.raises(RuntimeError, match="ROCm device"):
        A.InPlaceABNSync(3).eval()(torch.rand(2, 3, 4, 4))
    with pytest.raises(ValueError, match="more than 1 value per channel"):  # the reference divides by n - 1 = 0 here
        A.InPlaceABN(3)(torch.rand(1, 3, 1, 1))
    with pytest.raises(RuntimeError, match="ROCm device"):                  # ... eval mode has no such limit: next refusal
        A.InPlaceABN(3).eval()(torch.rand(1, 3, 1, 1))
    with pytest.raises(ValueError, match="unknown activation"):
        A.inplace_abn(torch.rand(2, 3, 4, 4), None, None, rm, rv, activation="relu")
    with pytest.raises(ValueError, match="unknown activation"):
        A.InPlaceABN(3, activation="relu")
    with pytest.raises(ValueError, match="shape"):
        A.inplace_abn(torch.rand(2, 3, 4, 4), torch.ones(4), None, rm, rv)


def test_double_backward_raises(monkeypatch):
    """once_differentiable: the autograd function with its two native calls replaced by stock statements (this test is about the
    autograd wiring, which needs no device)."""
    def forward(x, weight, bias, rm, rv, mean, var, training, phase, momentum, eps, activation, slope):
        x.mul_(2.0)

    def backward(z, dz, var, weight, bias, edz, eydz, dx, dweight, dbias, training, eps, activation, slope):
        dx.copy_(dz * 2.0)
    monkeypatch.setattr(A, "_native_forward", forward)
    monkeypatch.setattr(A, "_native_backward", backward)
    leaf = torch.rand(2, 3, 4, 4, requires_grad=True)
    work = leaf * 1.0
    out = A._InPlaceABN.apply(work, None, None, torch.zeros(3), torch.ones(3), True, 0.1, 1e-5, "none", 0.01)
    assert out.data_ptr() == work.data_ptr()                                # mark_dirty: the input IS the output
    cot = torch.ones_like(out, requires_grad=True)                          # a cotangent with a history of its own
    (g,) = torch.autograd.grad(out, leaf, grad_outputs=cot, create_graph=True)
    assert torch.equal(g.detach(), torch.full_like(g, 2.0))
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g.sum().backward()


def test_module_surface_is_the_reference_s():
    m = A.InPlaceABN(7)
    assert list(m.state_dict()) == ["weight", "bias", "running_mean", "running_var"]        # no num_batches_tracked
    assert [n for n, _ in m.named_parameters()] == ["weight", "bias"]
    assert torch.equal(m.weight.data, torch.ones(7)) and not m.bias.data.any() and torch.equal(m.running_var, torch.ones(7))
    assert repr(m) == "InPlaceABN(7, eps=1e-05, momentum=0.1, affine=True, activation=leaky_relu slope=0.01)"
    assert repr(A.InPlaceABN(7, activation="elu", affine=False)) == "InPlaceABN(7, eps=1e-05, momentum=0.1, affine=False, activation=elu)"
    n = A.InPlaceABN(7, affine=False)
    assert n.weight is None and n.bias is None and list(n.state_dict()) == ["running_mean", "running_var"]
    s = A.InPlaceABNSync(7, devices=[0, 1], activation="none")
    assert repr(s) == "InPlaceABNSync(7, eps=1e-05, momentum=0.1, affine=True, devices=[0, 1], activation=none)"
    assert list(s.state_dict()) == list(m.state_dict()) and s.process_group is None
    w = A.InPlaceABNWrapper(5, activation="none")
    assert isinstance(w.bn, A.InPlaceABN) and list(w.state_dict())[0] == "bn.weight"
    assert isinstance(A.InPlaceABNSyncWrapper(5).bn, A.InPlaceABNSync)
    abn = A.ABN(5, momentum=0.2)
    assert isinstance(abn, nn.Sequential) and isinstance(abn.bn, nn.BatchNorm2d) and isinstance(abn.act, nn.ReLU) and abn.bn.momentum == 0.2
    assert abn(torch.rand(2, 5, 3, 3)).min() >= 0                            # stock ops: runs anywhere
    assert network.inplace_abn is A and network.InPlaceABN is A.InPlaceABN and network.InPlaceABNSync is A.InPlaceABNSync
    assert network.convert_batchnorm is A.convert_batchnorm and network.ABN is A.ABN
    assert callable(A.inplace_abn) and callable(A.inplace_abn_sync)


def test_convert_batchnorm_swaps_every_layer_and_carries_the_state():
    from cspn_monodepth_amd.network import unet_ours
    torch.manual_seed(3)
    blk = unet_ours.Gudi_UpProj_Block(8, 4, 6, 8)
    for bn in (blk.bn1, blk.bn2, blk.sc_bn1):
        with torch.no_grad():
            bn.weight.uniform_(-2, 2)
            bn.bias.uniform_(-1, 1)
            bn.running_mean.uniform_(-1, 1)
            bn.running_var.uniform_(0.5, 2)
    blk.bn2.weight.requires_grad_(False)
    blk.sc_bn1.eval()
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    conv = A.convert_batchnorm(blk)
    assert conv is blk and not any(isinstance(m, nn.BatchNorm2d) for m in conv.modules())
    assert [type(conv.bn1), type(conv.bn2), type(conv.sc_bn1)] == [A.InPlaceABN] * 3
    assert conv.bn1.activation == "none" and conv.bn1.eps == 1e-5 and conv.bn1.momentum == 0.1
    assert not conv.bn2.weight.requires_grad and conv.bn1.weight.requires_grad and not conv.sc_bn1.training and conv.bn1.training
    after = conv.state_dict()
    assert sorted(after) == sorted(k for k in before if not k.endswith("num_batches_tracked"))
    assert all(torch.equal(after[k], before[k]) for k in after)
    sync = A.convert_batchnorm(unet_ours.Gudi_UpProj_Block(8, 4, 6, 8), activation="leaky_relu", sync=True)
    assert type(sync.bn1) is A.InPlaceABNSync and sync.bn1.activation == "leaky_relu"
    # a checkpoint of the converted layout loads into a freshly converted model, strictly
    A.convert_batchnorm(unet_ours.Gudi_UpProj_Block(8, 4, 6, 8), sync=True).load_state_dict(after, strict=True)
    assert type(A.convert_batchnorm(nn.BatchNorm2d(3))) is A.InPlaceABN         # the root itself
    with pytest.raises(ValueError, match="running statistics"):
        A.convert_batchnorm(nn.Sequential(nn.BatchNorm2d(3, track_running_stats=False)))


# ------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_matches_the_reference(name):
    case, inp, z = case_of(name)
    got = run_device(case, inp)
    if case["full"]:
        want = ac.restate_case(case, inp)                                   # only for the shape of the bars; the numbers are G20's
        index = np.arange(0, int(np.prod(case["shape"])), int(z["stride"]))
        ref = dict(want, out=None, dx=None, **{f: z[f] for f in ("dweight", "dbias", "running_mean", "running_var")})
        errs = ac.compare({f: got[f] for f in ("dweight", "dbias", "running_mean", "running_var")}, ref, inp["weight"], ac.DEVICE_BAR)
        for f in ("out", "dx"):
            d = float(np.abs(got[f].reshape(-1)[index].astype(np.float64) - z[f + "_sub"]).max())
            errs[f] = d / float(z[f + "_absmax"]) / ac.DEVICE_BAR
        # ... and every element, not the sub-sample alone, against the restatement
        errs.update({"restated_" + k: v for k, v in ac.compare(got, want, inp["weight"], ac.DEVICE_BAR).items()})
    else:
        want = ac.restate_case(case, inp)
        ref = dict(want, **{f: z[f] for f in ac.FIELDS if f in z})
        errs = ac.compare(got, ref, inp["weight"], ac.DEVICE_BAR, case["eps"])
        assert set(errs) >= {"out", "dx", "running_mean", "running_var"} and (("dweight" in errs) == case["affine"])
    assert_within(errs, name)
    plan = A.abn_plan(*ac.ncs(case["shape"]))
    if name.endswith("full_small_regime"):
        assert plan["regime"] == "small" and plan["channels_per_workgroup"] > 1
    if "full_split" in name:
        assert plan["regime"] == "split" and plan["workgroups_per_channel"] > 1


def _path_shapes():
    """The sizes at which the code takes another path, from the plan itself: the last SMALL size and the first SPLIT one, the
    last size at which channels share a workgroup and the next, planes just below / at the length from which they are moved in
    16-byte units, and an odd plane length whose ranges cross plane boundaries in the SPLIT regime."""
    limit = A.abn_plan(1, 3, 8)["small_limit"]
    shared = max(n for n in (256, 512, 1024, 2048, 4096) if A.abn_plan(1, 5, n)["channels_per_workgroup"] > 1)
    assert A.abn_plan(1, 5, shared + 1)["channels_per_workgroup"] == 1
    return [(1, 3, limit), (1, 3, limit + 1), (1, 5, shared), (1, 5, shared + 1), (3, 2, 31), (3, 2, 32), (3, 3, limit // 2 + 1)]


@gpu
@pytest.mark.parametrize("k", range(7))
def test_every_path_of_the_plan_against_the_restatement(k):
    shape = _path_shapes()[k]
    plan = A.abn_plan(*shape)
    limit = plan["small_limit"]
    assert plan["regime"] == ("small" if shape[0] * shape[2] <= limit else "split")
    case = ac._case(shape, ac.ACTIVATIONS[k % 3], 300 + k)
    inp = ac.make_inputs(case)
    errs = ac.compare(run_device(case, inp), ac.restate_case(case, inp), inp["weight"], ac.DEVICE_BAR)
    assert_within(errs, "%s %s %s" % (shape, case["activation"], plan["regime"]))


@gpu
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 2049)])
def test_a_view_that_starts_inside_a_buffer(shape):
    """x one float into a larger buffer: contiguous, not 16-byte aligned (the forward then peels from another phase); in the
    backward z and dz / dx differ in phase, and everything is moved element by element.  Forward through the module, backward
    through the native call on the same view."""
    case = ac._case(shape, "leaky_relu", 310)
    inp = ac.make_inputs(case)
    want = ac.restate_case(case, inp)
    n = int(np.prod(shape))
    holder = torch.zeros(n + 8, device=DEV)
    view = holder[1:1 + n].view(shape)
    view.copy_(dev(inp["x"]))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    mod = module_for(case, inp)
    with torch.no_grad():
        out = mod(view)
    assert out.data_ptr() == view.data_ptr()
    var = dev(inp["x"]).double().transpose(0, 1).reshape(shape[1], -1).var(dim=1, unbiased=False).float()
    cot, dx = dev(inp["cot"]), torch.empty(shape, device=DEV)
    dweight, dbias = torch.empty(shape[1], device=DEV), torch.empty(shape[1], device=DEV)
    assert dx.data_ptr() % 16 == 0
    A._native_backward(view, cot, var, mod.weight.detach(), mod.bias.detach(), None, None, dx, dweight, dbias, True, case["eps"],
                       case["activation"], case["slope"])
    got = dict(out=out, dx=dx, dweight=dweight, dbias=dbias, running_mean=mod.running_mean, running_var=mod.running_var)
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    assert_within(ac.compare(got, want, inp["weight"], ac.DEVICE_BAR), "view %s" % (shape,))
    assert not holder[0].item() and not holder[1 + n:].any().item()          # nothing written around the view


@gpu
@pytest.mark.parametrize("name", ["g20_abn_elu_3x5x9x11", "g20_abn_full_small_regime", "g20_abn_full_split_regime"])
def test_two_runs_give_equal_bits(name):
    case, inp, _ = case_of(name)
    a, b = run_device(case, inp), run_device(case, inp)
    for f in ac.FIELDS:
        assert np.array_equal(a[f].view(np.int32), b[f].view(np.int32)), f


@gpu
def test_eval_mode_leaves_the_running_statistics_alone_and_backward_runs():
    case, inp, z = case_of("g20_abn_eval_elu")
    got = run_device(case, inp)
    assert np.array_equal(got["running_mean"], inp["running_mean"]) and np.array_equal(got["running_var"], inp["running_var"])
    assert not got["dweight"].any() and not got["dbias"].any()             # as the reference leaves them (functions.py:144-147)


@gpu
@pytest.mark.parametrize("shape", [(3, 5, 9, 11), (1, 8, 70, 60)])
def test_captured_training_forward_replays_what_eager_steps_compute(shape):
    """A training-mode forward inside torch.cuda.graph, replayed k times, leaves the running statistics where k eager calls leave
    them, bit for bit: nothing synchronises and nothing is computed on the host (SMALL and SPLIT regime)."""
    case = ac._case(shape, "leaky_relu", 320)
    inp = ac.make_inputs(case)
    k = 3
    eager, graphed = module_for(case, inp), module_for(case, inp)
    x = dev(inp["x"])
    with torch.no_grad():
        for _ in range(k):
            want_out = eager(x.clone())
    state = {n: b.clone() for n, b in graphed.named_buffers()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        graphed(x.clone())                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for n, b in graphed.named_buffers():
            b.copy_(state[n])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = graphed(x.clone())
    assert torch.equal(bits(graphed.running_mean), bits(state["running_mean"]))     # a capture runs nothing
    for _ in range(k):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want_out))
    assert torch.equal(bits(graphed.running_mean), bits(eager.running_mean))
    assert torch.equal(bits(graphed.running_var), bits(eager.running_var))
    assert not torch.equal(bits(eager.running_mean), bits(state["running_mean"]))


def _stock_unpool(x, scale, oh, ow):
    y = x.new_zeros(x.shape[0], x.shape[1], x.shape[2] * scale, x.shape[3] * scale)
    y[:, :, ::scale, ::scale] = x
    return y[:, :, :oh, :ow]


@gpu
def test_converted_decoder_block_against_stock_ops():
    """Gudi_UpProj_Block(8, 4, 6, 8) through convert_batchnorm against an unconverted copy whose BN weights are |w| + eps.  The
    yardstick is the unconverted block in fp64 on the CPU (the un-pooling restated with stock indexing: it only copies);
    the stock fp32 device run's distance to it is measured here, and the converted block must stay within 4 x that distance (two
    differently ordered fp32 reductions), floor 1e-5 of the range."""
    import copy
    from cspn_monodepth_amd.network import unet_ours
    torch.manual_seed(11)
    proto = unet_ours.Gudi_UpProj_Block(8, 4, 6, 8)
    with torch.no_grad():
        for bn in (proto.bn1, proto.bn2, proto.sc_bn1):
            bn.weight.uniform_(0.25, 2.0).mul_(torch.tensor([1.0, -1.0, 1.0, -1.0]))
            bn.bias.uniform_(-0.5, 0.5)
    x = torch.randn(2, 8, 3, 4)
    cot = torch.randn(2, 4, 6, 8)
    converted = A.convert_batchnorm(copy.deepcopy(proto)).to(DEV)
    signs = {n: torch.sign(getattr(proto, n).weight.detach()) for n in ("bn1", "bn2", "sc_bn1")}
    stock = copy.deepcopy(proto)
    with torch.no_grad():
        for bn in (stock.bn1, stock.bn2, stock.sc_bn1):
            bn.weight.copy_(bn.weight.abs() + bn.eps)
    yard = copy.deepcopy(stock).double()
    yard._up_pooling = lambda t, s: _stock_unpool(t, s, 6, 8)
    stock = stock.to(DEV)

    def run(block, xin, g):
        leaf = xin.clone().requires_grad_(True)
        out = block(leaf)
        out.backward(g)
        res = {"out": out, "dx": leaf.grad}
        for n, p in block.named_parameters():
            grad = p.grad
            if block is converted and n.endswith("weight") and n.split(".")[0] in signs:
                grad = grad * signs[n.split(".")[0]].to(grad.device)        # d / d w = sign(w) d / d (|w| + eps)
            res["grad " + n] = grad
        for n, b in block.named_buffers():
            if "running" in n:
                res[n] = b
        return {k: v.detach().double().cpu() for k, v in res.items()}

    want = run(yard, x.double(), cot.double())
    got_stock, got_conv = run(stock, x.to(DEV), cot.to(DEV)), run(converted, x.to(DEV), cot.to(DEV))
    assert set(want) == set(got_stock) == set(got_conv) and len(want) == 2 + 9 + 6

    def dist(a, k):
        return float((a[k] - want[k]).abs().max() / want[k].abs().max())
    worst = {}
    for k in sorted(want):
        ds, dc = dist(got_stock, k), dist(got_conv, k)
        print("%-24s stock fp32 %.3g   converted %.3g" % (k, ds, dc))
        worst[k] = dc / max(4.0 * ds, 1e-5)
    assert all(v <= 1.0 for v in worst.values()), worst


def _torchrun(nproc, port, script_args, timeout=300):
    # as tests/test_distributed_gpu.py launches its workers: the ranks share the one GPU, so the weight-resident launches stay off
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="4", CSPN_RESIDENT="off")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port)] + script_args
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        print("---- stdout ----\n%s\n---- stderr ----\n%s" % (out.stdout[-4000:], out.stderr[-12000:]))
    assert out.returncode == 0, "torchrun %s failed (rc %d): see the captured output" % (script_args[0], out.returncode)
    return out.stdout


@gpu
def test_sync_variant_two_ranks_equal_one_process_on_the_whole_batch():
    """InPlaceABNSync at world size 2 over gloo on the one GPU: each rank takes half of a batch of 4; outputs, dx, parameter
    gradients (summed over the ranks) and running statistics equal a single-process InPlaceABN on the whole batch to 1e-5, and
    the statistics are identical across the ranks bit for bit (tests/dist_abn_worker.py asserts; SMALL and SPLIT regime)."""
    out = _torchrun(2, 29733, [os.path.join("tests", "dist_abn_worker.py"), "gloo"])
    print(out[-1500:])
    assert "ABN_SYNC_OK world=2" in out, out[-2000:]


@gpu
def test_sync_variant_without_a_process_group_is_the_plain_module():
    case, inp, _ = case_of("g20_abn_leaky_relu_2x3x5x7")
    plain, sync = module_for(case, inp), module_for(case, inp, cls=A.InPlaceABNSync)
    a, b = plain(dev(inp["x"])), sync(dev(inp["x"]))
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(plain.running_var), bits(sync.running_var))

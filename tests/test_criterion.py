"""The training criteria (cspn_monodepth_amd/criterion.py, include/cspn_criterion.h) against golden G18: the reference's
libs/criterion on the CPU in fp32, itself held to an fp64 restatement at 2e-6 (tests/golden/make_golden_g18.py).

  * CPU: the header / library / loader contract, get_criteria, the fixtures against the restatement, the host-side argument checks;
  * GPU: every G18 case at README "Parity"'s fp32 bar — loss 1e-5 relative, gradient max|got - want| <= 1e-5 max|want|, NaN and
    +-Inf position for position — and what include/cspn_criterion.h promises beyond it, exactly (torch.equal on the bits):
    alignment, shape and history do not change a bit, every gradient element is written, no LDS is read before it is written,
    nothing synchronises, and a captured step replays what the eager step computes.

Sizes not covered here: element counts past 2^31 (all indices in the kernels are size_t; three such fp32 planes are 26 GB)."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import criterion_cases as cc
import cspn_monodepth_amd as pkg
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import criterion as crit

DEV = "cuda:0"
SMALL = [n for n in golden_names("g18_criterion_") if not n.endswith("_full") and not n.endswith("dsn_l1")]
FULL = ["g18_criterion_%s_full" % k for k in cc.KINDS]
MODULES = {"l1": crit.MaskedL1Loss, "l2": crit.MaskedMSELoss, "l1_log": crit.L1_log}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return a.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def full_inputs(seed):
    return cc.make_inputs(seed, cc.FULL_SHAPE)


def run(kind, pred, target, g=1.0):
    """loss (0-dim device tensor) and d (g * loss) / d pred through the module of that kind."""
    p = pred.detach().requires_grad_(True)
    loss = MODULES[kind]()(p, target)
    (loss if g == 1.0 else loss * g).backward()
    return loss.detach(), p.grad


# ------------------------------------------------------------------------------------------------ CPU
def test_fixture_set_is_complete():
    want = ["%s_%s_%s" % (k, s, g) for k in cc.KINDS for s in ("1", "3x5", "3x57x77") for g in ("g10", "g04")]
    want += ["%s_%s" % (k, c) for k in cc.KINDS for c in ("ties", "empty")] + ["l1_log_pred_zero", "l1_log_pred_neg"]
    assert sorted(SMALL) == sorted("g18_criterion_" + w for w in want)
    assert all(os.path.exists(os.path.join(ROOT, "tests", "golden", n + ".npz")) for n in FULL + ["g18_criterion_dsn_l1"])


def test_header_declares_four_symbols_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "cspn_criterion.h")).read()
    assert re.search(r"CSPN_LOSS_L1 = 0, CSPN_LOSS_L2 = 1, CSPN_LOSS_L1_LOG = 2", src)
    assert (_lib.LOSS_L1, _lib.LOSS_L2, _lib.LOSS_L1_LOG) == (0, 1, 2)


def test_workspace_bytes_are_a_function_of_n():
    L = _lib.lib()
    assert L.cspn_criterion_workspace_bytes(0) == 0
    assert L.cspn_criterion_workspace_bytes(1) == 16 and L.cspn_criterion_workspace_bytes(1024) == 16
    assert L.cspn_criterion_workspace_bytes(1025) == 32
    assert L.cspn_criterion_workspace_bytes(13167) == 13 * 16
    assert L.cspn_criterion_workspace_bytes(24 * 228 * 304) == 1024 * 16 == L.cspn_criterion_workspace_bytes(1 << 33)


def test_get_criteria_maps_keys_and_wrappers_like_the_reference():
    assert crit.key_to_criteria == {"l1": crit.MaskedL1Loss, "l2": crit.MaskedMSELoss, "l1_log": crit.L1_log}
    for key, cls in crit.key_to_criteria.items():
        for wrapper, wcls in (("dsn", crit.CriterionDSN), ("DSN", crit.CriterionDSN), ("no_dsn", crit.Criterion_No_DSN),
                              ("", crit.Criterion_No_DSN)):
            c = crit.get_criteria(types.SimpleNamespace(criterion=key, loss_wrapper=wrapper))
            assert type(c) is wcls and type(c.criterion) is cls
    for key in ("berhu", "rmse", "L1", None):
        with pytest.raises(NotImplementedError):
            crit.get_criteria(types.SimpleNamespace(criterion=key, loss_wrapper="dsn", arch="x"))
    import inspect
    assert list(inspect.signature(crit.MaskedL1Loss.forward).parameters) == ["self", "pred", "target"]
    assert list(inspect.signature(crit.MaskedMSELoss.forward).parameters) == ["self", "pred", "target"]
    assert list(inspect.signature(crit.L1_log.forward).parameters) == ["self", "fake", "real"]
    assert list(inspect.signature(crit.CriterionDSN.forward).parameters) == ["self", "preds", "target"]
    assert pkg.criterion is crit


def test_no_cpu_fallback_and_no_half():
    with pytest.raises(RuntimeError, match="ROCm device"):
        crit.masked_loss(torch.rand(1, 1, 3, 5), torch.rand(1, 1, 3, 5), "l1")
    with pytest.raises(TypeError, match="fp16"):
        crit.MaskedL1Loss()(torch.rand(1, 1, 3, 5).half(), torch.rand(1, 1, 3, 5).half())
    with pytest.raises(NotImplementedError):
        crit.masked_loss(torch.rand(2), torch.rand(2), "berhu")


@pytest.mark.parametrize("name", SMALL)
def test_fixture_agrees_with_the_fp64_restatement(name):
    z = load_golden(name)
    kind = str(z["kind"])
    pred, target = cc.make_inputs(int(z["seed"]), tuple(int(v) for v in z["shape"]),
                                  tie_frac=0.10 if name.endswith("_ties") else 0.0, all_invalid=name.endswith("_empty"),
                                  hostile="zero" if name.endswith("pred_zero") else "neg" if name.endswith("pred_neg") else None)
    assert np.array_equal(pred, z["pred"]) and np.array_equal(target, z["target"])       # the stored seed gives the stored inputs
    assert cc.no_tie_ok(z["pred"], z["target"])
    loss, grad = cc.restate(z["pred"], z["target"], kind, float(z["g"]))
    el, eg = cc.loss_err(z["loss"], loss), cc.grad_err(z["grad"], grad)
    print("%s: loss %.3e grad %.3e" % (name, el, eg))
    assert el <= cc.ORACLE_BAR and eg <= cc.ORACLE_BAR
    if name.endswith("_empty"):
        assert np.isnan(z["loss"]) and not z["grad"].any()
    if name.endswith("pred_zero"):
        hit = (z["target"] > 0) & (z["pred"] == 0)
        assert hit.any() and z["loss"] == np.inf and np.all(z["grad"][hit] == -np.inf)
    if name.endswith("pred_neg"):
        hit = (z["target"] > 0) & (z["pred"] < 0)
        assert hit.any() and np.isnan(z["loss"]) and not z["grad"][hit].any()
    if name.endswith("_ties"):
        tie = (z["target"] > 0) & (z["pred"] == z["target"])
        assert tie.sum() > 0.05 * (z["target"] > 0).sum() and not z["grad"][tie].any()


@pytest.mark.parametrize("name", FULL)
def test_full_size_fixture_agrees_with_the_fp64_restatement(name):
    z = load_golden(name)
    assert tuple(int(v) for v in z["shape"]) == cc.FULL_SHAPE and int(z["stride"]) == cc.FULL_STRIDE
    pred, target = full_inputs(int(z["seed"]))
    assert cc.no_tie_ok(pred, target)
    loss, grad = cc.restate(pred, target, str(z["kind"]))
    el = cc.loss_err(z["loss"], loss)
    eg = float(np.abs(z["grad_sub"] - grad.reshape(-1)[::cc.FULL_STRIDE]).max() / np.abs(grad).max())
    print("%s: loss %.3e grad %.3e" % (name, el, eg))
    assert el <= cc.ORACLE_BAR and eg <= cc.ORACLE_BAR
    assert np.isclose(float(z["grad_absmax"]), np.abs(grad).max(), rtol=cc.ORACLE_BAR)


def test_dsn_fixture_agrees_with_the_fp64_restatement():
    z = load_golden("g18_criterion_dsn_l1")
    assert z["target"].shape == (2, 1, 8, 12) and z["pred0"].shape == (2, 1, 8, 12) and z["pred1"].shape == (2, 1, 4, 6)
    loss, g0, g1 = cc.restate_dsn(z["pred0"], z["pred1"], z["target"], str(z["kind"]))
    errs = (cc.loss_err(z["loss"], loss), cc.grad_err(z["grad0"], g0), cc.grad_err(z["grad1"], g1))
    print("dsn: loss %.3e grads %.3e %.3e" % errs)
    assert max(errs) <= cc.ORACLE_BAR


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Validation happens on the host before any launch: 0 and a message in cspn_last_error()."""
    L = _lib.lib()
    err = lambda: L.cspn_last_error().decode()                                     # noqa: E731
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)                            # never dereferenced: validation fails first
    F32, F16 = _lib.CSPN_F32, _lib.CSPN_F16
    assert L.cspn_criterion_forward(None, one, F32, 0, 4, one, one, None) == 0 and "null" in err()
    assert L.cspn_criterion_forward(one, None, F32, 0, 4, one, one, None) == 0 and "null" in err()
    assert L.cspn_criterion_forward(one, one, F32, 0, 4, None, one, None) == 0 and "null" in err()
    assert L.cspn_criterion_forward(one, one, F32, 0, 4, one, None, None) == 0 and "null" in err()
    assert L.cspn_criterion_forward(one, one, F32, 0, 0, one, one, None) == 0 and "n must be" in err()
    assert L.cspn_criterion_forward(one, one, F32, 3, 4, one, one, None) == 0 and "unknown kind" in err()
    assert L.cspn_criterion_forward(one, one, F32, -1, 4, one, one, None) == 0 and "unknown kind" in err()
    assert L.cspn_criterion_forward(one, one, F16, 0, 4, one, one, None) == 0 and "fp32 only" in err() and "fp16" in err()
    assert L.cspn_criterion_forward(one, one, 7, 0, 4, one, one, None) == 0 and "dtype" in err()
    assert L.cspn_criterion_forward(one, one, F32, 0, 4, odd, one, None) == 0 and "8-byte aligned" in err()
    assert L.cspn_criterion_forward(one, one, F32, 0, 4, one, odd, None) == 0 and "8-byte aligned" in err()
    assert L.cspn_criterion_forward(ctypes.c_void_p(66), one, F32, 0, 4, one, one, None) == 0 and "element size" in err()
    assert L.cspn_criterion_backward(None, one, F32, 0, 4, one, one, one, None) == 0 and "null" in err()
    assert L.cspn_criterion_backward(one, one, F32, 0, 4, None, one, one, None) == 0 and "null" in err()
    assert L.cspn_criterion_backward(one, one, F32, 0, 4, one, None, one, None) == 0 and "null" in err()
    assert L.cspn_criterion_backward(one, one, F32, 0, 4, one, one, None, None) == 0 and "null" in err()
    assert L.cspn_criterion_backward(one, one, F32, 0, 0, one, one, one, None) == 0 and "n must be" in err()
    assert L.cspn_criterion_backward(one, one, F32, 5, 4, one, one, one, None) == 0 and "unknown kind" in err()
    assert L.cspn_criterion_backward(one, one, F16, 0, 4, one, one, one, None) == 0 and "fp32 only" in err()
    assert L.cspn_criterion_backward(one, one, F32, 0, 4, odd, one, one, None) == 0 and "8-byte aligned" in err()
    assert L.cspn_criterion_backward(one, one, F32, 0, 4, one, one, ctypes.c_void_p(65), None) == 0 and "element size" in err()


# ------------------------------------------------------------------------------------------------ GPU
def check_against(z, loss, grad, what):
    el, eg = cc.loss_err(float(loss), z["loss"]), cc.grad_err(grad.cpu().numpy(), z["grad"])
    print("%s: loss %.3e grad %.3e" % (what, el, eg))
    assert el <= cc.TEST_RTOL and eg <= cc.TEST_RTOL, (what, el, eg)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_case_matches_the_reference(name):
    z = load_golden(name)
    loss, grad = run(str(z["kind"]), dev(z["pred"]), dev(z["target"]), float(z["g"]))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and grad.shape == z["grad"].shape
    check_against(z, loss, grad, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL)
def test_full_size_case_matches_the_reference(name):
    z = load_golden(name)
    pred, target = full_inputs(int(z["seed"]))
    loss, grad = run(str(z["kind"]), dev(pred), dev(target))
    el = cc.loss_err(float(loss), z["loss"])
    eg = float((grad.reshape(-1)[::cc.FULL_STRIDE].cpu().double() - torch.from_numpy(z["grad_sub"]).double()).abs().max()) / float(z["grad_absmax"])
    print("%s: loss %.3e grad %.3e" % (name, el, eg))
    assert el <= cc.TEST_RTOL and eg <= cc.TEST_RTOL
    # what the sub-sample cannot see: zeros exactly where the target is invalid, and nowhere a NaN
    t = dev(target)
    assert not bool(grad[~(t > 0)].any()) and bool(torch.isfinite(grad).all())


@pytest.mark.gpu
def test_dsn_wrapper_matches_the_reference():
    z = load_golden("g18_criterion_dsn_l1")
    p0, p1 = dev(z["pred0"]).requires_grad_(True), dev(z["pred1"]).requires_grad_(True)
    c = crit.get_criteria(types.SimpleNamespace(criterion="l1", loss_wrapper="dsn"))
    loss = c([p0, p1], dev(z["target"]))
    loss.backward()
    errs = (cc.loss_err(float(loss), z["loss"]), cc.grad_err(p0.grad.cpu().numpy(), z["grad0"]), cc.grad_err(p1.grad.cpu().numpy(), z["grad1"]))
    print("dsn: loss %.3e grads %.3e %.3e" % errs)
    assert max(errs) <= cc.TEST_RTOL
    single = crit.get_criteria(types.SimpleNamespace(criterion="l1", loss_wrapper="none"))([p1], dev(z["target"]))      # resized too
    assert single.dim() == 0 and bool(torch.isfinite(single))


def abi_run(kind, pred, target, g, grad):
    """The three launches through the C ABI on caller-owned buffers -> (state [8 floats], grad)."""
    L = _lib.lib()
    n = pred.numel()
    work = torch.empty((L.cspn_criterion_workspace_bytes(n) // 8,), dtype=torch.float64, device=DEV)
    state = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    gl = torch.tensor(g, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.cspn_criterion_forward(pred.data_ptr(), target.data_ptr(), _lib.CSPN_F32, kind, n, work.data_ptr(), state.data_ptr(), st),
               "cspn_criterion_forward")
    _lib.check(L.cspn_criterion_backward(pred.data_ptr(), target.data_ptr(), _lib.CSPN_F32, kind, n, state.data_ptr(), gl.data_ptr(),
                                         grad.data_ptr(), st), "cspn_criterion_backward")
    torch.cuda.synchronize()
    return state, grad


@pytest.mark.gpu
@pytest.mark.parametrize("kind", cc.KINDS)
def test_alignment_shape_and_history_do_not_change_a_bit(kind):
    """13 167 elements (odd: the last unit is partial).  The same values behind a base that is not 16-byte aligned — pred, target
    and the gradient buffer each start one element into a larger buffer — give the same bits; so do a second run and the same
    values seen as (1,1,1,13167).  Every gradient buffer is NaN-filled first, with a guard element either side: the backward
    writes every element and nothing else."""
    z = load_golden("g18_criterion_%s_3x57x77_g04" % kind)
    k, g, n = crit.KINDS[kind], float(z["g"]), z["pred"].size
    pred, target = dev(z["pred"]), dev(z["target"])
    assert pred.data_ptr() % 16 == 0 and target.data_ptr() % 16 == 0
    nan = float("nan")
    buf = torch.full((n + 2,), nan, device=DEV)
    assert buf.data_ptr() % 16 == 0
    state, _ = abi_run(k, pred, target, g, buf[1:])             # only the gradient unaligned
    guards = bits(buf[[0, n + 1]])
    assert bool(torch.isnan(buf[[0, n + 1]]).all()) and not bool(torch.isnan(buf[1:n + 1]).any())
    grad = buf[1:n + 1].clone()
    check_against(z, state[0], grad.view(z["grad"].shape), "abi " + kind)
    assert float(state[1]) == np.float32(1.0 / (z["target"] > 0).sum()) and float(state[6]) == 0 and float(state[7]) == 0
    assert float(state[2:6].view(torch.float64)[1]) == float((z["target"] > 0).sum())
    # aligned everything, twice
    for _ in range(2):
        s2, g2 = abi_run(k, pred, target, g, torch.full((n,), nan, device=DEV))
        assert same_bits(s2, state) and same_bits(g2, grad)
    # everything one element off
    pb, tb = torch.zeros(n + 5, device=DEV), torch.zeros(n + 5, device=DEV)
    pb[1:n + 1], tb[1:n + 1] = pred.reshape(-1), target.reshape(-1)
    pb[n + 1:], tb[n + 1:] = 3.0, 7.0                            # valid-looking pixels past the end must not be read into the sum
    gb = torch.full((n + 2,), nan, device=DEV)
    assert pb[1:].data_ptr() % 16 == 4
    s3, _ = abi_run(k, pb[1:n + 1], tb[1:n + 1], g, gb[1:])
    assert same_bits(s3, state) and same_bits(gb[1:n + 1], grad) and torch.equal(bits(gb[[0, n + 1]]), guards)
    # through the module: unaligned views, and another shape of the same values
    loss_a, grad_a = run(kind, pred, target, g)
    loss_u, grad_u = run(kind, pb[1:n + 1].view(pred.shape), tb[1:n + 1].view(pred.shape), g)
    loss_f, grad_f = run(kind, pred.reshape(1, 1, 1, n), target.reshape(1, 1, 1, n), g)
    assert same_bits(loss_a, state[0]) and same_bits(loss_u, loss_a) and same_bits(loss_f, loss_a)
    assert same_bits(grad_a.reshape(-1), grad) and same_bits(grad_u, grad_a) and same_bits(grad_f.reshape(-1), grad)


@pytest.mark.gpu
def test_more_than_one_trip_of_the_slice_loop_is_deterministic():
    """1 100 000 elements: 275 000 units over 1024 slices of 256 threads — some threads add two units, some one.  Against the fp64
    restatement at the same bar, and twice for the bits."""
    pred, target = cc.make_inputs(188, (1, 1, 1000, 1100))
    for kind in ("l2", "l1_log"):
        want_loss, want_grad = cc.restate(pred, target, kind)
        loss, grad = run(kind, dev(pred), dev(target))
        loss2, grad2 = run(kind, dev(pred), dev(target))
        el, eg = cc.loss_err(float(loss), want_loss), cc.grad_err(grad.cpu().numpy(), want_grad)
        print("%s 1000x1100: loss %.3e grad %.3e" % (kind, el, eg))
        assert el <= cc.TEST_RTOL and eg <= cc.TEST_RTOL
        assert same_bits(loss, loss2) and same_bits(grad, grad2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", cc.KINDS)
def test_no_lds_is_read_before_it_is_written(kind):
    z = load_golden("g18_criterion_%s_3x57x77_g10" % kind)
    loss, grad = run(kind, dev(z["pred"]), dev(z["target"]))
    with lds_poison():
        loss_p, grad_p = run(kind, dev(z["pred"]), dev(z["target"]))
        torch.cuda.synchronize()
    assert same_bits(loss_p, loss) and same_bits(grad_p, grad)
    check_against(z, loss_p, grad_p, "poisoned " + kind)


@pytest.mark.gpu
def test_step_does_not_synchronise():
    """Forward and backward under torch's sync debug mode "error": a .item(), a nonzero or a blocking copy would raise."""
    z = load_golden("g18_criterion_l1_3x57x77_g10")
    pred, target = dev(z["pred"]).requires_grad_(True), dev(z["target"])
    c = crit.Criterion_No_DSN(crit.MaskedL1Loss())
    c([pred], target).backward()                                 # first use: library load, allocator warm-up
    pred.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = c([pred], target)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_against(z, loss.detach(), pred.grad, "sync-free")
    assert c.criterion.loss is loss
    with pytest.raises(RuntimeError, match="synchroniz"):        # the mode does catch the reference's formulation
        torch.cuda.set_sync_debug_mode("error")
        try:
            (target - pred.detach())[target > 0].abs().mean()
        finally:
            torch.cuda.set_sync_debug_mode("default")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", cc.KINDS)
def test_captured_step_replays_the_eager_step(kind):
    """loss = crit(pred, target); loss.backward() captured as a (linear) graph; replays with two targets whose valid-pixel counts
    differ give the eager bits each time."""
    z = load_golden("g18_criterion_%s_3x57x77_g10" % kind)
    t1 = dev(z["target"])
    t2 = torch.where(dev(cc.make_inputs(189, z["target"].shape)[1]) > 0, t1, torch.zeros_like(t1))
    assert int((t2 > 0).sum()) not in (0, int((t1 > 0).sum()))
    static_p, static_t = dev(z["pred"]).requires_grad_(True), t1.clone()
    c = MODULES[kind]()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            c(static_p, static_t).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    static_p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = c(static_p, static_t)
        static_loss.backward()
    for t in (t2, t1, t2):
        static_t.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        loss, grad = run(kind, dev(z["pred"]), t)
        assert same_bits(static_loss, loss) and same_bits(static_p.grad, grad)
    check_against(z, *run(kind, dev(z["pred"]), t1), "eager " + kind)


@pytest.mark.gpu
def test_autograd_contract():
    z = load_golden("g18_criterion_l2_3x57x77_g10")
    pred, target = dev(z["pred"]), dev(z["target"])
    # a non-contiguous prediction is made contiguous, its gradient comes back in its own layout's terms
    pt = pred.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    assert not pt.is_contiguous()
    loss = crit.masked_loss(pt, target, "l2")
    loss.backward()
    check_against(z, loss.detach(), pt.grad, "non-contiguous")
    # the target never gets a gradient; a prediction that does not need one costs no backward launch
    tg = target.clone().requires_grad_(True)
    p = pred.clone().requires_grad_(True)
    crit.masked_loss(p, tg, "l2").backward()
    assert tg.grad is None and p.grad is not None
    assert not crit.masked_loss(pred, tg, "l2").requires_grad
    # double backward raises
    p2 = pred.clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(crit.masked_loss(p2, target, "l2"), p2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    with pytest.raises(TypeError, match="fp16"):
        crit.masked_loss(pred.half(), target.half(), "l2")
    with pytest.raises(ValueError):
        crit.masked_loss(pred, target[:, :, :5], "l2")


@pytest.mark.gpu
def test_criterion_behind_the_cspn_module_gives_the_hand_written_formula_its_gradients():
    """CSPN_new.AffinityPropagate(24, 3) -> Criterion_No_DSN(MaskedL1Loss()) -> backward on 2 x 57 x 76, against the same chain
    with the stock formula the benchmark's training step spells out: the guidance gradients agree to 1e-5 of their largest."""
    from oracle import cspn_oracle as orc
    B, H, W = 2, 57, 76
    g, d, _ = orc.synthetic_inputs(191, B, H, W, 8)
    _, target = cc.make_inputs(192, (B, 1, H, W))
    target = dev(target)
    m = pkg.CSPN_new.AffinityPropagate(24, 3)
    grads = []
    for form in ("criterion", "stock"):
        gt, dt = dev(g).requires_grad_(True), dev(d).requires_grad_(True)
        pred = m(gt, dt)
        if form == "criterion":
            loss = crit.Criterion_No_DSN(crit.MaskedL1Loss())([pred], target)
        else:
            valid = target > 0
            loss = ((target - pred).abs() * valid).sum() / valid.sum()
        loss.backward()
        grads.append((float(loss), gt.grad.cpu().numpy(), dt.grad.cpu().numpy()))
    (la, ga, da), (lb, gb, db) = grads
    eg, ed = cc.grad_err(ga, gb), cc.grad_err(da, db)
    print("criterion vs stock: loss %.3e guidance %.3e depth %.3e" % (abs(la - lb) / abs(lb), eg, ed))
    assert abs(la - lb) <= cc.TEST_RTOL * abs(lb) and eg <= cc.TEST_RTOL and ed <= cc.TEST_RTOL
    assert np.abs(gb).max() > 0

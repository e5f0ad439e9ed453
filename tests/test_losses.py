"""berHuLoss and the unmasked criteria L1, GradLoss, RMSE, RMSE_log (cspn_monodepth_amd/criterion.py, include/cspn_losses.h)
against golden G23: the reference's libs/criterion/criteria.py on the CPU in fp32, itself held to an fp64 restatement at 2e-6
(tests/golden/make_golden_g23.py).

  * CPU: the header / library / loader contract, the fixtures against the restatement, the host-side argument checks;
  * GPU: every G23 case at README "Parity"'s fp32 bar — loss 1e-5 relative, gradient max|got - want| <= 1e-5 max|want|, NaN and
    +-Inf position for position; berHu's threshold (as fp32 bits) and both counts EXACTLY, read from the state; the maximum
    wherever it sits; and what include/cspn_losses.h promises beyond that, on the bits: alignment, shape and history change
    nothing, every gradient element is written, nothing synchronises, a captured step replays what the eager step computes."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import losses_cases as lc
from conftest import ROOT, golden_names, lds_poison, load_golden
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import criterion as crit

DEV = "cuda:0"
PREFIX = "g23_losses_"
FULL = [n for n, s in lc.CASES.items() if tuple(s["shape"]) == lc.FULL_SHAPE]
SMALL = [n for n in lc.CASES if n not in FULL]
MODULES = {"berhu": crit.berHuLoss, "l1": crit.L1, "grad": crit.GradLoss, "rmse": crit.RMSE, "rmse_log": crit.RMSE_log}
N13 = 3 * 57 * 77


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return a.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def f32_bits(x):
    """The bits of a fp32 value; every NaN as 0x7fc00000.  A NaN's sign and payload are not part of what torch.max promises: the
    reference's CPU run returns 0xffffffff from its vectorised path (the 874-element fixtures) and would return the input's own
    payload from its scalar path."""
    x = np.asarray(x, np.float32).reshape(1)
    return 0x7fc00000 if np.isnan(x[0]) else int(x.view(np.uint32)[0])


@functools.lru_cache(maxsize=None)
def inputs(name):
    return lc.make_inputs(name)


def run(loss_name, a, b, g=1.0):
    """loss (0-dim device tensor) and d (g * loss) / d a through the module of that loss."""
    x = a.detach().requires_grad_(True)
    loss = MODULES[loss_name]()(x, b)
    (loss if g == 1.0 else loss * g).backward()
    return loss.detach(), x.grad


def abi_run(loss_name, a, b, g, grad):
    """The launches through the C ABI on caller-owned buffers -> (state [12 floats], grad)."""
    L = _lib.lib()
    n = a.numel()
    work = torch.full((L.cspn_losses_workspace_bytes(n) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    state = torch.full((12,), float("nan"), dtype=torch.float32, device=DEV)
    gl = torch.tensor(g, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    if loss_name == "berhu":
        _lib.check(L.cspn_berhu_forward(a.data_ptr(), b.data_ptr(), _lib.CSPN_F32, n, work.data_ptr(), state.data_ptr(), st), "forward")
        _lib.check(L.cspn_berhu_backward(a.data_ptr(), b.data_ptr(), _lib.CSPN_F32, n, state.data_ptr(), gl.data_ptr(), grad.data_ptr(), st),
                   "backward")
    else:
        k = crit.MEAN_KINDS[loss_name]
        _lib.check(L.cspn_mean_loss_forward(a.data_ptr(), b.data_ptr(), _lib.CSPN_F32, k, n, work.data_ptr(), state.data_ptr(), st), "forward")
        _lib.check(L.cspn_mean_loss_backward(a.data_ptr(), b.data_ptr(), _lib.CSPN_F32, k, n, state.data_ptr(), gl.data_ptr(),
                                             grad.data_ptr(), st), "backward")
    torch.cuda.synchronize()
    return state, grad


def state_fields(state):
    """include/cspn_losses.h's layout -> dict(loss, factor, c_bits, sum, sum2, n_valid, n_huber)."""
    s = state.cpu()
    d = s[4:12].view(torch.float64)
    return dict(loss=float(s[0]), factor=float(s[1]), c_bits=f32_bits(s[2:3].numpy()), reserved=float(s[3]),
                sum=float(d[0]), sum2=float(d[1]), n_valid=float(d[2]), n_huber=float(d[3]))


# ------------------------------------------------------------------------------------------------ CPU
def test_fixture_set_is_complete():
    want = ["%s_%s_%s" % (k, s, g) for k in ("berhu",) + lc.MEAN_KINDS for s in ("1", "3x5", "3x57x77") for g in ("g10", "g04")]
    want += ["%s_%s" % (k, c) for k in lc.MEAN_KINDS for c in ("full", "equal")] + ["rmse_log_real_nonpositive", "rmse_log_fake_zero"]
    want += ["berhu_" + c for c in ("ties", "full", "c_negative", "c_from_invalid", "c_from_valid", "nan_invalid", "nan_valid", "empty")]
    assert sorted(want) == sorted(lc.CASES)
    assert sorted(golden_names(PREFIX)) == sorted(PREFIX + w for w in want + list(lc.EXTRA))
    assert os.path.exists(os.path.join(ROOT, "tests", "golden", "golden_g23_manifest.json"))


def test_header_declares_the_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "cspn_losses.h")).read()
    assert re.search(r"^#define CSPN_LOSSES_STATE_BYTES 48$", src, flags=re.M)
    assert re.search(r"CSPN_MEAN_L1 = 0, CSPN_MEAN_GRAD = 1, CSPN_MEAN_RMSE = 2, CSPN_MEAN_RMSE_LOG = 3", src)
    assert (_lib.MEAN_L1, _lib.MEAN_GRAD, _lib.MEAN_RMSE, _lib.MEAN_RMSE_LOG) == (0, 1, 2, 3) and _lib.LOSSES_STATE_BYTES == 48


def test_losses_sources_stay_out_of_the_benchmark_digest():
    # one copy of the slice discipline: both translation units take the cut, the passes, both stages of the sums, the streaming
    # backward and the checks from the shared header, and hold no loop over units or slices of their own
    core = open(os.path.join(_lib.CSRC, "cspn_loss_units.hpp")).read()
    shared = ("criterion_slices", "load_unit", "slice_pass", "block_sums_to_work", "wave_sum_of_slices", "loss_backward_grid", "stream_grad",
              "check_planes", "check_forward", "check_backward")
    defined = r"\b(?:void|int|double|unsigned) (%s)\(" % "|".join(shared)
    assert sorted(re.findall(defined, core)) == sorted(shared)
    for tu in ("cspn_criterion.hip", "cspn_losses.hip"):
        code = re.sub(r"//.*$", "", open(os.path.join(_lib.CSRC, tu)).read(), flags=re.M)
        assert '#include "cspn_loss_units.hpp"' in code and not re.findall(defined, code)
        assert "load_unit" not in code and "wave_sum_to_lane63" not in code
        loops = re.findall(r"\bfor \(([^;]*);", code)                      # berHu's maximum over lanes and over slice maxima, nothing else
        assert loops == ([] if tu == "cspn_criterion.hip" else ["int off = 32", "int s = threadIdx.x"]), (tu, loops)


def test_workspace_bytes_are_a_function_of_n():
    L = _lib.lib()
    assert L.cspn_losses_workspace_bytes(0) == 0
    assert L.cspn_losses_workspace_bytes(1) == 40 == L.cspn_losses_workspace_bytes(1024)
    assert L.cspn_losses_workspace_bytes(1025) == 80 and L.cspn_losses_workspace_bytes(N13) == 13 * 40
    assert L.cspn_losses_workspace_bytes(24 * 228 * 304) == 1024 * 40 == L.cspn_losses_workspace_bytes(1 << 33)


def check_fixture(z, want_loss, want_grad, what):
    el, eg = lc.loss_err(z["loss"], want_loss), lc.grad_err(z["grad"], want_grad)
    print("%s: loss %.3e grad %.3e" % (what, el, eg))
    assert el <= lc.ORACLE_BAR and eg <= lc.ORACLE_BAR, (what, el, eg)


@pytest.mark.parametrize("name", SMALL)
def test_fixture_agrees_with_the_fp64_restatement(name):
    z, s = load_golden(PREFIX + name), lc.CASES[name]
    a, b = inputs(name)
    assert np.array_equal(a, z["a"], equal_nan=True) and np.array_equal(b, z["b"], equal_nan=True)    # the table gives the stored inputs
    assert str(z["loss_name"]) == s["loss"] and float(z["g"]) == s["g"] and str(z["variant"]) == s["variant"]
    loss, grad, extra = lc.restate(name, a, b)
    check_fixture(z, loss, grad, name)
    if extra is not None:
        assert f32_bits(z["c"]) == f32_bits(extra["c"]) and int(z["n_valid"]) == extra["n_valid"]
        assert ("n_huber" in z) == (s["variant"] != "nan_valid")
        if "n_huber" in z:
            assert int(z["n_huber"]) == extra["n_huber"]
        assert bool(z["max_at_valid"]) == extra["max_at_valid"]
        if s["variant"] == "main" and a.size >= 15:
            assert 0.10 * extra["n_valid"] <= extra["n_huber"] <= 0.90 * extra["n_valid"]
        if s["variant"] == "c_negative":
            assert extra["c"] < 0 and extra["n_huber"] == extra["n_valid"] > 0
        if s["variant"] == "nan_invalid":
            assert np.isnan(extra["c"]) and extra["n_huber"] == 0 and np.isfinite(z["loss"])


@pytest.mark.parametrize("name", FULL)
def test_full_size_fixture_agrees_with_the_fp64_restatement(name):
    z = load_golden(PREFIX + name)
    assert tuple(int(v) for v in z["shape"]) == lc.FULL_SHAPE and int(z["stride"]) == lc.FULL_STRIDE and "a" not in z
    a, b = inputs(name)
    loss, grad, extra = lc.restate(name, a, b)
    el = lc.loss_err(z["loss"], loss)
    eg = float(np.abs(z["grad_sub"] - grad.reshape(-1)[::lc.FULL_STRIDE]).max() / np.abs(grad).max())
    print("%s: loss %.3e grad %.3e" % (name, el, eg))
    assert el <= lc.ORACLE_BAR and eg <= lc.ORACLE_BAR
    assert np.isclose(float(z["grad_absmax"]), np.abs(grad).max(), rtol=lc.ORACLE_BAR)
    if extra is not None:
        assert f32_bits(z["c"]) == f32_bits(extra["c"]) and int(z["n_valid"]) == extra["n_valid"] and int(z["n_huber"]) == extra["n_huber"]
        assert 0.10 * extra["n_valid"] <= extra["n_huber"] <= 0.90 * extra["n_valid"]


def test_dsn_and_resize_fixtures_agree_with_the_fp64_restatement():
    z = load_golden(PREFIX + "dsn_berhu")
    p0, p1, t = lc.dsn_inputs()
    assert np.array_equal(p0, z["pred0"]) and np.array_equal(p1, z["pred1"]) and np.array_equal(t, z["target"])
    assert p0.shape == (2, 1, 8, 12) and p1.shape == (2, 1, 4, 6)
    loss, g0, g1 = lc.restate_dsn_berhu(p0, p1, t)
    errs = (lc.loss_err(z["loss"], loss), lc.grad_err(z["grad0"], g0), lc.grad_err(z["grad1"], g1))
    print("dsn: loss %.3e grads %.3e %.3e" % errs)
    assert max(errs) <= lc.ORACLE_BAR
    z = load_golden(PREFIX + "rmse_resize")
    fake, real = lc.resize_inputs()
    assert np.array_equal(fake, z["fake"]) and np.array_equal(real, z["real"]) and fake.shape == (2, 1, 4, 6) and real.shape == (2, 1, 8, 12)
    check_fixture(z, *lc.restate_resize(fake, real, "rmse"), "rmse_resize")


def test_input_errors_follow_masked_loss():
    a = torch.rand(1, 1, 3, 5)
    for fn in (crit.berhu_loss, lambda x, y: crit.unmasked_loss(x, y, "rmse"), crit.berHuLoss(), crit.GradLoss(), crit.RMSE(), crit.RMSE_log(),
               crit.L1()):
        with pytest.raises(TypeError, match="fp16"):
            fn(a.half(), a.half())
        with pytest.raises(RuntimeError, match="ROCm device"):
            fn(a, a)
        with pytest.raises(ValueError, match="empty"):
            fn(a[:0], a[:0])
    for fn in (crit.berhu_loss, lambda x, y: crit.unmasked_loss(x, y, "l1"), crit.berHuLoss(), crit.GradLoss()):
        with pytest.raises(ValueError, match="same shape"):
            fn(a, a[:, :, :2])
    with pytest.raises(ValueError, match="same shape"):              # three dimensions: nothing to resize
        crit.RMSE()(a[0], a[0, :, :2])
    with pytest.raises(NotImplementedError):
        crit.unmasked_loss(a, a, "l2")
    with pytest.raises(AssertionError):
        crit.berHuLoss()(a, a[0])
    import inspect
    for cls, names in ((crit.berHuLoss, ["pred", "target"]), (crit.GradLoss, ["pred", "target"]), (crit.RMSE, ["fake", "real"]),
                       (crit.RMSE_log, ["fake", "real"]), (crit.L1, ["fake", "real"])):
        assert list(inspect.signature(cls.forward).parameters) == ["self"] + names
    assert not hasattr(crit, "BerHu") and not hasattr(crit, "NormalLoss")
    assert set(crit.key_to_criteria) == {"l1", "l2", "l1_log"}               # get_criteria offers what the reference's does


def test_entry_points_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    err = lambda: L.cspn_last_error().decode()                                     # noqa: E731
    one, odd = ctypes.c_void_p(64), ctypes.c_void_p(68)                            # never dereferenced: validation fails first
    F32, F16 = _lib.CSPN_F32, _lib.CSPN_F16
    assert L.cspn_berhu_forward(None, one, F32, 4, one, one, None) == 0 and "null" in err()
    assert L.cspn_berhu_forward(one, one, F32, 4, None, one, None) == 0 and "null" in err()
    assert L.cspn_berhu_forward(one, one, F32, 4, one, None, None) == 0 and "null" in err()
    assert L.cspn_berhu_forward(one, one, F32, 0, one, one, None) == 0 and "n must be" in err()
    assert L.cspn_berhu_forward(one, one, F16, 4, one, one, None) == 0 and "fp32 only" in err() and "fp16" in err()
    assert L.cspn_berhu_forward(one, one, F32, 4, odd, one, None) == 0 and "8-byte aligned" in err()
    assert L.cspn_berhu_forward(ctypes.c_void_p(66), one, F32, 4, one, one, None) == 0 and "element size" in err()
    assert L.cspn_berhu_backward(one, None, F32, 4, one, one, one, None) == 0 and "null" in err()
    assert L.cspn_berhu_backward(one, one, F32, 4, one, None, one, None) == 0 and "null" in err()
    assert L.cspn_berhu_backward(one, one, F16, 4, one, one, one, None) == 0 and "fp32 only" in err()
    assert L.cspn_berhu_backward(one, one, F32, 4, odd, one, one, None) == 0 and "8-byte aligned" in err()
    assert L.cspn_berhu_backward(one, one, F32, 4, one, one, ctypes.c_void_p(65), None) == 0 and "element size" in err()
    assert L.cspn_mean_loss_forward(one, one, F32, 4, 4, one, one, None) == 0 and "unknown kind" in err()
    assert L.cspn_mean_loss_forward(one, one, F32, -1, 4, one, one, None) == 0 and "unknown kind" in err()
    assert L.cspn_mean_loss_forward(one, one, F16, 0, 4, one, one, None) == 0 and "fp32 only" in err()
    assert L.cspn_mean_loss_forward(one, one, F32, 0, 0, one, one, None) == 0 and "n must be" in err()
    assert L.cspn_mean_loss_forward(one, one, F32, 0, 4, one, odd, None) == 0 and "8-byte aligned" in err()
    assert L.cspn_mean_loss_backward(one, one, F32, 7, 4, one, one, one, None) == 0 and "unknown kind" in err()
    assert L.cspn_mean_loss_backward(one, one, F32, 0, 4, None, one, one, None) == 0 and "null" in err()
    assert L.cspn_mean_loss_backward(one, one, F16, 0, 4, one, one, one, None) == 0 and "fp32 only" in err()


# ------------------------------------------------------------------------------------------------ GPU
def check_against(want_loss, want_grad, loss, grad, what):
    el, eg = lc.loss_err(float(loss), want_loss), lc.grad_err(grad.cpu().numpy(), want_grad)
    print("%s: loss %.3e grad %.3e" % (what, el, eg))
    assert el <= lc.TEST_RTOL and eg <= lc.TEST_RTOL, (what, el, eg)


def check_berhu_state(state, c, n_valid, n_huber, what):
    f = state_fields(state)
    print("%s: c %08x (want %08x) n_valid %r n_huber %r" % (what, f["c_bits"], f32_bits(c), f["n_valid"], f["n_huber"]))
    assert f["c_bits"] == f32_bits(c), what
    assert f["n_valid"] == float(n_valid), what
    if n_huber is not None:
        assert f["n_huber"] == float(n_huber), what
        count = float(n_valid) + float(n_huber)
        assert f["factor"] == (np.float32(1.0 / count) if count else np.inf) and f["reserved"] == 0
        if count and np.isfinite(f["loss"]):
            assert f["loss"] == np.float32((f["sum"] + f["sum2"]) / count)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_case_matches_the_reference(name):
    z, s = load_golden(PREFIX + name), lc.CASES[name]
    a, b = dev(z["a"]), dev(z["b"])
    loss, grad = run(s["loss"], a, b, s["g"])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and grad.shape == z["grad"].shape
    check_against(z["loss"], z["grad"], loss, grad, name)
    state, grad_abi = abi_run(s["loss"], a, b, s["g"], torch.full_like(a, float("nan")))
    assert same_bits(state[0], loss) and same_bits(grad_abi, grad)
    if s["loss"] == "berhu":
        check_berhu_state(state, z["c"], z["n_valid"], z["n_huber"] if "n_huber" in z else None, name)
    else:
        f = state_fields(state)
        assert f["n_valid"] == a.numel() and f["n_huber"] == 0 and f["sum2"] == 0 and f["c_bits"] == 0 and f["reserved"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL)
def test_full_size_case_matches_the_reference(name):
    z, s = load_golden(PREFIX + name), lc.CASES[name]
    a, b = (dev(v) for v in inputs(name))
    loss, grad = run(s["loss"], a, b)
    el = lc.loss_err(float(loss), z["loss"])
    eg = float((grad.reshape(-1)[::lc.FULL_STRIDE].cpu().double() - torch.from_numpy(z["grad_sub"]).double()).abs().max()) / float(z["grad_absmax"])
    print("%s: loss %.3e grad %.3e" % (name, el, eg))
    assert el <= lc.TEST_RTOL and eg <= lc.TEST_RTOL and bool(torch.isfinite(grad).all())
    if s["loss"] == "berhu":
        assert not bool(grad[~(b > 0)].any())            # what the sub-sample cannot see: zeros exactly where the target is invalid
        state, grad_abi = abi_run("berhu", a, b, 1.0, torch.full_like(a, float("nan")))
        assert same_bits(state[0], loss) and same_bits(grad_abi, grad)
        check_berhu_state(state, z["c"], z["n_valid"], z["n_huber"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("where", (0, 1023, 1024, N13 - 1))
@pytest.mark.parametrize("at_valid", (True, False))
def test_the_maximum_is_found_wherever_it_sits(where, at_valid):
    """13 167 elements are 13 slices: flat index 0 is the first thread of slice 0, 1023 the last pixel of slice 0's only trip, 1024
    the first of slice 1, n - 1 the partial last unit of slice 12.  pred = target + 20 there moves c from 0.64 to 4, above every
    other |target - pred|: the Huber set shrinks from 4447 pixels to that pixel alone (when it is valid) or to nothing.  The state
    must carry that c, and the counts of the restatement, from every position."""
    pred, target = (v.copy().reshape(-1) for v in inputs("berhu_3x57x77_g10"))
    target[where] = np.float32(2.5 if at_valid else 0.0)
    pred[where] = target[where] + np.float32(20)
    want = lc.restate_berhu(pred, target)
    assert want["max_at_valid"] == at_valid and f32_bits(want["c"]) == f32_bits(np.float32(0.2) * np.float32(20))
    base = lc.restate_berhu(*inputs("berhu_3x57x77_g10"))
    assert want["n_huber"] == (1 if at_valid else 0) and base["n_huber"] > 4000
    a, b = dev(pred), dev(target)
    loss, grad = run("berhu", a, b)
    check_against(want["loss"], want["grad"], loss, grad, "max at %d" % where)
    state, _ = abi_run("berhu", a, b, 1.0, torch.empty_like(a))
    check_berhu_state(state, want["c"], want["n_valid"], want["n_huber"], "max at %d" % where)


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ("berhu",) + lc.MEAN_KINDS)
def test_alignment_shape_and_history_do_not_change_a_bit(loss_name):
    """13 167 elements (odd: the last unit is partial).  The same values behind a base that is 4 bytes past a 16-byte boundary give
    the same bits; so do a second run and the same values seen as (13167,).  Every gradient buffer is NaN-filled first, with a
    guard element either side: the backward writes every element and nothing else."""
    name = "%s_3x57x77_g04" % loss_name
    z = load_golden(PREFIX + name)
    g, n = float(z["g"]), N13
    a, b = dev(z["a"]), dev(z["b"])
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
    nan = float("nan")
    buf = torch.full((n + 2,), nan, device=DEV)
    state, _ = abi_run(loss_name, a, b, g, buf[1:])              # only the gradient unaligned
    guards = bits(buf[[0, n + 1]])
    assert bool(torch.isnan(buf[[0, n + 1]]).all()) and not bool(torch.isnan(buf[1:n + 1]).any())
    grad = buf[1:n + 1].clone()
    check_against(z["loss"], z["grad"], state[0], grad.view(z["grad"].shape), "abi " + name)
    for _ in range(2):                                           # aligned everything, twice
        s2, g2 = abi_run(loss_name, a, b, g, torch.full((n,), nan, device=DEV))
        assert same_bits(s2, state) and same_bits(g2, grad)
    # everything one element off; valid-looking pixels with a huge pred - target past the end must not be read
    pb, tb = torch.zeros(n + 5, device=DEV), torch.zeros(n + 5, device=DEV)
    pb[1:n + 1], tb[1:n + 1] = a.reshape(-1), b.reshape(-1)
    pb[0], tb[0], pb[n + 1:], tb[n + 1:] = 900.0, 7.0, 900.0, 7.0
    gb = torch.full((n + 2,), nan, device=DEV)
    assert pb[1:].data_ptr() % 16 == 4
    s3, _ = abi_run(loss_name, pb[1:n + 1], tb[1:n + 1], g, gb[1:])
    assert same_bits(s3, state) and same_bits(gb[1:n + 1], grad) and torch.equal(bits(gb[[0, n + 1]]), guards)
    # through the module: unaligned views, and another fold of the same values
    loss_a, grad_a = run(loss_name, a, b, g)
    loss_u, grad_u = run(loss_name, pb[1:n + 1].view(a.shape), tb[1:n + 1].view(a.shape), g)
    loss_f, grad_f = run(loss_name, a.reshape(n), b.reshape(n), g)
    assert same_bits(loss_a, state[0]) and same_bits(loss_u, loss_a) and same_bits(loss_f, loss_a)
    assert same_bits(grad_a.reshape(-1), grad) and same_bits(grad_u, grad_a) and same_bits(grad_f.reshape(-1), grad)


@pytest.mark.gpu
def test_slices_wrap_past_the_cap():
    """1024 * 1024 + 1 elements: the 1024 slices of 1024 pixels are full and the one extra pixel (a partial unit) wraps into
    slice 0's second trip.  That pixel carries the maximum and is valid, so a dropped wrap shows in c, in the counts and in the loss."""
    n = 1024 * 1024 + 1
    pred, target = lc.berhu_inputs(199, (n,))
    target[n - 1] = np.float32(3.0)
    pred[n - 1] = np.float32(12.0)
    want = lc.restate_berhu(pred, target)
    assert want["max_at_valid"] and f32_bits(want["c"]) == f32_bits(np.float32(0.2) * np.float32(9.0))
    a, b = dev(pred), dev(target)
    loss, grad = run("berhu", a, b)
    loss2, grad2 = run("berhu", a, b)
    check_against(want["loss"], want["grad"], loss, grad, "berhu 2^20 + 1")
    assert same_bits(loss, loss2) and same_bits(grad, grad2)
    state, _ = abi_run("berhu", a, b, 1.0, torch.empty_like(a))
    check_berhu_state(state, want["c"], want["n_valid"], want["n_huber"], "berhu 2^20 + 1")
    fake = np.where(target > 0, pred, np.float32(1.0)).astype(np.float32)
    real = (np.abs(target) + np.float32(0.5)).astype(np.float32)
    want_loss, want_grad = lc.restate_mean(fake, real, "rmse_log")
    loss, grad = run("rmse_log", dev(fake).view(1, 1, 1, n), dev(real).view(1, 1, 1, n))
    check_against(want_loss, want_grad.reshape(1, 1, 1, n), loss, grad, "rmse_log 2^20 + 1")


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ("berhu", "rmse_log"))
def test_no_lds_is_read_before_it_is_written(loss_name):
    z = load_golden(PREFIX + "%s_3x57x77_g10" % loss_name)
    loss, grad = run(loss_name, dev(z["a"]), dev(z["b"]))
    with lds_poison():
        loss_p, grad_p = run(loss_name, dev(z["a"]), dev(z["b"]))
        torch.cuda.synchronize()
    assert same_bits(loss_p, loss) and same_bits(grad_p, grad)
    check_against(z["loss"], z["grad"], loss_p, grad_p, "poisoned " + loss_name)


@pytest.mark.gpu
def test_step_does_not_synchronise():
    """Forward and backward under torch's sync debug mode "error": a .item(), a nonzero or a blocking copy would raise."""
    z = load_golden(PREFIX + "berhu_3x57x77_g10")
    pred, target = dev(z["a"]).requires_grad_(True), dev(z["b"])
    c = crit.Criterion_No_DSN(crit.berHuLoss())
    c([pred], target).backward()                                 # first use: library load, allocator warm-up
    pred.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = c([pred], target)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_against(z["loss"], z["grad"], loss.detach(), pred.grad, "sync-free")
    assert c.criterion.loss is loss


@pytest.mark.gpu
@pytest.mark.parametrize("loss_name", ("berhu", "rmse"))
def test_captured_step_replays_the_eager_step(loss_name):
    """Forward and backward captured once on static buffers; replays with inputs A, then B written into the same buffers, then A
    again give the eager bits each time.  B has another c and another Huber set (another loss, for rmse): a threshold or a
    factor cached on the host at capture time would replay A's."""
    za = load_golden(PREFIX + "%s_3x57x77_g10" % loss_name)
    a_in = (za["a"], za["b"])
    if loss_name == "berhu":
        b_in = tuple(v.reshape(za["a"].shape) for v in lc.berhu_inputs(200, (N13,)))
        ra, rb = lc.restate_berhu(*a_in), lc.restate_berhu(*b_in)
        assert f32_bits(ra["c"]) != f32_bits(rb["c"]) and ra["n_huber"] != rb["n_huber"]
    else:
        b_in = lc.mean_inputs(loss_name, 200, za["a"].shape)
    static_a, static_b = dev(a_in[0]).requires_grad_(True), dev(a_in[1])
    c = MODULES[loss_name]()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            c(static_a, static_b).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    static_a.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = c(static_a, static_b)
        static_loss.backward()
    losses = []
    for pa, pb in (a_in, b_in, a_in):
        with torch.no_grad():
            static_a.copy_(dev(pa))
            static_b.copy_(dev(pb))
        graph.replay()
        torch.cuda.synchronize()
        loss, grad = run(loss_name, dev(pa), dev(pb))
        assert same_bits(static_loss, loss) and same_bits(static_a.grad, grad)
        losses.append(float(loss))
    assert losses[0] == losses[2] != losses[1]
    check_against(za["loss"], za["grad"], *run(loss_name, dev(a_in[0]), dev(a_in[1])), "eager " + loss_name)


@pytest.mark.gpu
def test_dsn_wrapper_matches_the_reference():
    z = load_golden(PREFIX + "dsn_berhu")
    p0, p1 = dev(z["pred0"]).requires_grad_(True), dev(z["pred1"]).requires_grad_(True)
    loss = crit.CriterionDSN(crit.berHuLoss())([p0, p1], dev(z["target"]))
    loss.backward()
    errs = (lc.loss_err(float(loss), z["loss"]), lc.grad_err(p0.grad.cpu().numpy(), z["grad0"]), lc.grad_err(p1.grad.cpu().numpy(), z["grad1"]))
    print("dsn: loss %.3e grads %.3e %.3e" % errs)
    assert max(errs) <= lc.TEST_RTOL


@pytest.mark.gpu
def test_resized_fake_matches_the_reference():
    z = load_golden(PREFIX + "rmse_resize")
    loss, grad = run("rmse", dev(z["fake"]), dev(z["real"]))
    assert grad.shape == z["fake"].shape
    check_against(z["loss"], z["grad"], loss, grad, "rmse_resize")


@pytest.mark.gpu
def test_autograd_contract():
    """What masked_loss documents: a non-contiguous prediction is made contiguous and its gradient comes back in its own
    layout's terms; a target of another dtype is cast to fp32; the target never gets a gradient; double backward raises."""
    z = load_golden(PREFIX + "berhu_3x57x77_g10")
    pred, target = dev(z["a"]), dev(z["b"])
    pt = pred.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    assert not pt.is_contiguous()
    loss = crit.berhu_loss(pt, target)
    loss.backward()
    check_against(z["loss"], z["grad"], loss.detach(), pt.grad, "non-contiguous")
    ref_loss, ref_grad = run("berhu", pred, target)
    loss64, grad64 = run("berhu", pred, target.double())
    assert same_bits(loss64, ref_loss) and same_bits(grad64, ref_grad)
    tg = target.clone().requires_grad_(True)
    p = pred.clone().requires_grad_(True)
    crit.berhu_loss(p, tg).backward()
    assert tg.grad is None and p.grad is not None
    assert not crit.berhu_loss(pred, tg).requires_grad
    for fn in (crit.berhu_loss, lambda x, y: crit.unmasked_loss(x, y, "rmse")):
        p2 = pred.clone().requires_grad_(True)
        (g1,) = torch.autograd.grad(fn(p2, target), p2, create_graph=True)
        with pytest.raises(RuntimeError):
            g1.sum().backward()
    with pytest.raises(TypeError, match="fp16"):
        crit.berhu_loss(pred.half(), target.half())
    with pytest.raises(ValueError):
        crit.berhu_loss(pred, target[:, :, :5])

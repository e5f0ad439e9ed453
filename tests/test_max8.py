"""The max-of-8 propagation (cspn_monodepth_amd/post_process/CSPN.py, include/cspn_max8.h) against golden G19: the reference's
network/libs/post_process/CSPN.py on the CPU in fp32, itself held to an fp64 restatement at 2e-6 (tests/golden/make_golden_g19.py).

  * CPU: the header / library / loader contract, the fixtures against the restatement, the tie rule, the modules' signatures,
    the host-side argument checks;
  * GPU: every G19 case at README "Parity"'s fp32 bar (1e-5 relative, NaN position for position; gradients
    max|got - want| <= 1e-5 max|want|), and what include/cspn_max8.h promises beyond it, exactly (torch.equal on the bits):
    steps_per_launch, the place in the batch, history, poisoned LDS and a graph replay do not change a bit.

Selection.  Where two gates' values are closer than 1e-5 (relative) fp32 may pick the other one, and the gradient follows the
pick.  So the large-shape gradient tests compare against the restatement evaluated WITH THE DEVICE'S OWN MASKS, and a separate
test holds those masks to the fp64 ones wherever the fp64 gap is >= 1e-5 — which must leave out at most 1 % of the pixel-steps."""
import ctypes
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import max8_cases as mc
import cspn_monodepth_amd as pkg
from conftest import ROOT, golden_names, lds_poison, load_golden, rel_err
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import functional as F
from cspn_monodepth_amd.post_process import CSPN

DEV = "cuda:0"
CASES = mc.golden_cases()
NAMES = sorted(CASES)
GRAD_NAMES = sorted(n for n in CASES if CASES[n][4])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@functools.lru_cache(maxsize=None)
def golden(name):
    z = load_golden("g19_max8_" + name)
    return z, mc.case_inputs(z, name)


@functools.lru_cache(maxsize=None)
def big(shape, sparse, T=16):
    """inputs, cotangent and the fp64 forward of a large shape — computed once, shared, never modified"""
    g, d, s = mc.make_inputs(mc.BIG_SEEDS[shape], shape, sparse)
    return g, d, s, mc.make_cotangent(mc.BIG_SEEDS[shape], shape), mc.restate(g, d, s, T)


def module_run(g, d, s, T=16):
    if s is None:
        return CSPN.AffinityPropagate_prediction(prop_time=T)(g, d)
    return CSPN.AffinityPropagate(prop_time=T)(g, d, s)


# ------------------------------------------------------------------------------------------------ CPU
def test_fixture_set_is_complete():
    assert golden_names("g19_max8_") == sorted("g19_max8_" + n for n in CASES)
    assert len(CASES) == 25
    for shape in mc.FWD_SHAPES:
        assert {"fwd_%s_sp" % mc.shape_tag(shape), "fwd_%s_nosp" % mc.shape_tag(shape)} <= set(CASES)
    limit = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) for n in golden_names("g") if not n.startswith("g19_"))
    assert all(os.path.getsize(os.path.join(ROOT, "tests", "golden", n + ".npz")) <= limit for n in golden_names("g19_max8_"))


def test_workspace_bytes():
    L = _lib.lib()
    assert L.cspn_max8_workspace_bytes(0, 5, 5, 16, 0) == 0 and L.cspn_max8_workspace_bytes(1, 5, 5, 0, 1) == 0
    assert L.cspn_max8_workspace_bytes(1, 1, 1, 16, 0) == 2 * 256 and L.cspn_max8_workspace_bytes(1, 1, 1, 16, 1) == 26 * 256
    plane = 24 * 228 * 304 * 4
    assert plane % 256 == 0 and L.cspn_max8_workspace_bytes(24, 228, 304, 16, 0) == 2 * plane
    assert L.cspn_max8_workspace_bytes(24, 228, 304, 16, 1) == 26 * plane == L.cspn_max8_workspace_bytes(24, 228, 304, 3, 1)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_agrees_with_the_fp64_restatement(name):
    z, (g, d, s, T, cot) = golden(name)
    kind, shape, sp, T2, with_grad = CASES[name]
    assert T == T2 == int(z["T"]) and g.shape == shape and (s is not None) == sp and z["out"].shape == d.shape
    want = mc.restate(g, d, s, T, cot)
    errs = [rel_err(z["out"], want["out"])]
    if with_grad:
        errs += [mc.grad_err(z["grad_guidance"], want["grad_guidance"]), mc.grad_err(z["grad_blur"], want["grad_blur"])]
        gap = float(np.nanmin(want["gap"])) if np.isfinite(want["gap"]).any() else float("inf")
        assert gap >= mc.GAP_BAR and gap == float(z["gap"])
    print("%s: %s" % (name, " ".join("%.3e" % e for e in errs)))
    assert max(errs) <= mc.ORACLE_BAR
    nan = np.isnan(z["out"])
    if kind == "zero_block" and shape[2] == 6:
        assert nan.all()                                                        # a 4x4 block of zero gates: the whole 6x8 image
    elif kind == "zero_block":
        assert nan[0, 0, 3:5, 4:6].all() and 0 < nan.sum() < nan.size            # S = 0 inside the block, one more ring per step
    elif kind == "nan_blur":
        assert 0 < nan.sum() < nan.size
    else:
        assert not nan.any()
    if kind == "neg_sparse":
        assert (s < 0).sum() == 2 and not np.array_equal(z["out"][s < 0], s[s < 0])       # m = -1: 2 e - s, not s
        assert np.array_equal(z["out"][s > 0], s[s > 0])
    if kind == "tie015":
        gg = z["grad_guidance"]
        assert np.array_equal(gg[:, 0], gg[:, 1]) and not np.array_equal(np.abs(gg[:, 5]), np.abs(gg[:, 0])) and np.abs(gg[:, 5]).max() > 0


def test_tie_weights_follow_the_pairwise_tree():
    w = mc.tree_weights(np.array([0b00010011, 0b00000001, 0b11111111, 0b10000000, 0b00001100, 0b00100110, 0], np.uint8))
    assert w[0].tolist() == [0.25, 0.25, 0, 0, 0.5, 0, 0, 0]                    # o0 = o1 = o4 maximal
    assert w[1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and w[3].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert w[2].tolist() == [0.125] * 8 and w[4].tolist() == [0, 0, 0.5, 0.5, 0, 0, 0, 0]
    assert w[5].tolist() == [0, 0.25, 0.25, 0, 0, 0.5, 0, 0] and not w[6].any()
    assert np.all(w[:6].sum(axis=1) == 1)
    # ... and the restatement's own masks on a three-way tie: channels 0, 1 and 4 carry the same gate
    g, d, _ = mc.make_inputs(7, (1, 8, 5, 6), False)
    g[:, 1], g[:, 4] = g[:, 0], -g[:, 0]
    r = mc.restate(g, d, None, 2)
    m = r["masks"]
    assert np.all(((m & 0b10011) == 0) | ((m & 0b10011) == 0b10011)) and ((m & 0b10011) == 0b10011).any()


def test_modules_keep_the_reference_signatures_and_have_no_state():
    assert list(inspect.signature(CSPN.AffinityPropagate.__init__).parameters) == ["self", "spn", "prop_time"]
    assert list(inspect.signature(CSPN.AffinityPropagate_prediction.__init__).parameters) == ["self", "spn", "prop_time"]
    assert list(inspect.signature(CSPN.AffinityPropagate.forward).parameters) == ["self", "guidance", "blur_depth", "sparse_depth"]
    assert list(inspect.signature(CSPN.AffinityPropagate_prediction.forward).parameters) == ["self", "guidance", "blur_depth"]
    for cls in (CSPN.AffinityPropagate, CSPN.AffinityPropagate_prediction):
        m = cls()
        assert m.spn is False and m.prop_time == 16 and len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
        assert cls(True).spn is True and cls(False, 5).prop_time == 5
    sig = inspect.signature(F.cspn_max8_propagate)
    assert list(sig.parameters) == ["guidance", "blur_depth", "sparse_depth", "prop_time", "steps_per_launch"]
    assert sig.parameters["prop_time"].default == 16 and sig.parameters["steps_per_launch"].default == 0
    assert pkg.CSPN is CSPN and pkg.post_process.CSPN is CSPN and pkg.cspn_max8_propagate is F.cspn_max8_propagate
    assert pkg.post_process.AffinityPropagate is pkg.CSPN_new.AffinityPropagate      # the package default did not move


def test_python_entry_rejects_bad_arguments_without_a_gpu():
    g, d = torch.rand(1, 8, 3, 5), torch.rand(1, 1, 3, 5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.cspn_max8_propagate(g, d)
    with pytest.raises(RuntimeError, match="ROCm device"):
        CSPN.AffinityPropagate()(g, d, d)
    with pytest.raises(ValueError, match="needs sparse_depth"):
        CSPN.AffinityPropagate()(g, d, None)


def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Validation happens on the host before any launch: 0 and a message in cspn_last_error()."""
    L = _lib.lib()
    err = lambda: L.cspn_last_error().decode()                                     # noqa: E731
    p, odd, w8 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(72)    # never dereferenced: validation fails first
    q = ctypes.c_void_p(128)

    def fwd(g=p, bs=8, cs=1, d0=p, sp=None, out=q, hist=None, mask=None, work=p, B=1, H=1, W=1, T=16, S=0):
        return L.cspn_max8_forward(g, bs, cs, d0, sp, out, hist, mask, work, B, H, W, T, S, None)

    def bwd(g=p, bs=8, cs=1, C=8, blur=p, sp=None, hist=p, mask=p, go=p, gg=q, gb=q, work=p, B=1, H=1, W=1, T=16):
        return L.cspn_max8_backward(g, bs, cs, C, blur, sp, hist, mask, go, gg, gb, work, B, H, W, T, None)

    assert fwd(g=None) == 0 and "null" in err()
    assert fwd(d0=None) == 0 and "null" in err()
    assert fwd(out=None) == 0 and "null" in err()
    assert fwd(work=None) == 0 and "null" in err()
    assert fwd(B=0) == 0 and "at least 1" in err()
    assert fwd(W=0) == 0 and "at least 1" in err()
    assert fwd(T=0) == 0 and "T must be" in err()
    assert fwd(S=-1) == 0 and "steps_per_launch" in err()
    assert fwd(S=17) == 0 and "steps_per_launch" in err()
    assert fwd(hist=p) == 0 and "both or neither" in err()
    assert fwd(mask=p) == 0 and "both or neither" in err()
    assert fwd(g=odd) == 0 and "element size" in err()
    assert fwd(work=w8) == 0 and "16-byte aligned" in err()
    assert fwd(out=p) == 0 and "alias" in err()
    assert fwd(bs=-8) == 0 and "stride" in err()
    assert fwd(H=70000, W=70000) == 0 and "does not fit" in err()
    assert bwd(g=None) == 0 and "null" in err()
    assert bwd(hist=None) == 0 and "null" in err()
    assert bwd(mask=None) == 0 and "null" in err()
    assert bwd(go=None) == 0 and "null" in err()
    assert bwd(gg=None) == 0 and "null" in err()
    assert bwd(gb=None) == 0 and "null" in err()
    assert bwd(work=None) == 0 and "null" in err()
    assert bwd(C=7) == 0 and "at least 8 channels" in err()
    assert bwd(T=0) == 0 and "T must be" in err()
    assert bwd(H=0) == 0 and "at least 1" in err()
    assert bwd(gg=odd) == 0 and "element size" in err()
    assert bwd(work=w8) == 0 and "16-byte aligned" in err()


# ------------------------------------------------------------------------------------------------ GPU
def abi_forward(g, d, s, T=16, S=0, history=True):
    """cspn_max8_forward on caller-owned, NaN / 0xff-filled buffers -> out [B,1,H,W], hist, mask ([T,B,H,W] or None)."""
    L = _lib.lib()
    B, C, H, W = g.shape
    out = torch.full((B, 1, H, W), float("nan"), device=DEV)
    hist = torch.full((T, B, H, W), float("nan"), device=DEV) if history else None
    mask = torch.full((T, B, H, W), 0xEE, dtype=torch.uint8, device=DEV) if history else None
    work = torch.full((L.cspn_max8_workspace_bytes(B, H, W, T, 0) // 4,), float("nan"), device=DEV)
    ptr = lambda t: None if t is None else t.data_ptr()                            # noqa: E731
    _lib.check(L.cspn_max8_forward(g.data_ptr(), g.stride(0), g.stride(1), d.data_ptr(), ptr(s), out.data_ptr(), ptr(hist), ptr(mask),
                                   work.data_ptr(), B, H, W, T, S, torch.cuda.current_stream().cuda_stream), "cspn_max8_forward")
    torch.cuda.synchronize()
    return out, hist, mask


def grads(g, d, s, cot, T=16, S=0):
    gt, dt = g.detach().clone().requires_grad_(True), d.detach().clone().requires_grad_(True)
    out = F.cspn_max8_propagate(gt, dt, s, T, S)
    out.backward(cot)
    return out.detach(), gt.grad, dt.grad


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_the_reference(name):
    """Through the class, through functional, and on a channel-slice view of a wider tensor: 1e-5, NaN position for position."""
    z, (g, d, s, T, _) = golden(name)
    gt, dt, st = dev(g), dev(d), dev(s)
    out = module_run(gt, dt, st, T)
    assert out.shape == z["out"].shape and out.dtype == torch.float32
    e = rel_err(out.cpu().numpy(), z["out"])
    print("%s: %.3e" % (name, e))
    assert e <= mc.TEST_RTOL
    assert same_bits(F.cspn_max8_propagate(gt, dt, st, T), out)
    B, C, H, W = g.shape
    wide = torch.full((B, C + 5, H, W), float("nan"), device=DEV)
    wide[:, 3:3 + C] = gt
    view = wide[:, 3:3 + C]
    assert not view.is_contiguous() or B == 1
    assert same_bits(module_run(view, dt, st, T), out)
    assert same_bits(module_run(gt[:, :8], dt, st, T), out)                      # only channels 0..7 are read


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.BIG_SHAPES, ids=mc.shape_tag)
@pytest.mark.parametrize("sparse", (True, False), ids=("sp", "nosp"))
def test_steps_per_launch_batch_place_and_history_do_not_change_a_bit(shape, sparse):
    g, d, s, _, ref = big(shape, sparse)
    gt, dt, st = dev(g), dev(d), dev(s)
    for T in (16, 5):
        base, hist, mask = abi_forward(gt, dt, st, T, 1)
        assert not bool(torch.isnan(base).any()) and not bool(torch.isnan(hist).any()) and same_bits(hist[T - 1], base[:, 0])
        assert bool((mask != 0).all()) and bool(((mask & (mask - 1)) == 0).float().mean() > 0.99)     # one winner nearly everywhere
        if T == 16:
            base16 = base
            e = rel_err(base.cpu().numpy(), ref["out"])
            print("%s sparse=%d: %.3e" % (mc.shape_tag(shape), sparse, e))
            assert e <= mc.TEST_RTOL
        for S in (2, 3, 16, 0):
            o2, h2, m2 = abi_forward(gt, dt, st, T, S)
            assert same_bits(o2, base) and same_bits(h2, hist) and torch.equal(m2, mask), (T, S)
            o3, _, _ = abi_forward(gt, dt, st, T, S, history=False)
            assert same_bits(o3, base), (T, S, "no history")
        assert same_bits(F.cspn_max8_propagate(gt, dt, st, T), base)              # two runs, another route
    # a frame alone equals the same frame inside a batch of 3
    last = g.shape[0] - 1
    pick = [last, 0, last]
    g3, d3 = gt[pick].contiguous(), dt[pick].contiguous()
    s3 = None if st is None else st[pick].contiguous()
    o_b, h_b, m_b = abi_forward(g3, d3, s3, 16, 0)
    o_1, h_1, m_1 = abi_forward(g3[1:2].contiguous(), d3[1:2].contiguous(), None if s3 is None else s3[1:2].contiguous(), 16, 0)
    assert same_bits(o_b[1:2], o_1) and same_bits(h_b[:, 1:2], h_1) and torch.equal(m_b[:, 1:2], m_1)
    assert same_bits(o_b[0], o_b[2]) and same_bits(o_b[1], base16[0])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.BIG_SHAPES, ids=mc.shape_tag)
@pytest.mark.parametrize("sparse", (True, False), ids=("sp", "nosp"))
def test_selection_matches_fp64_where_the_gap_allows(shape, sparse):
    g, d, s, _, ref = big(shape, sparse)
    _, hist, mask = abi_forward(dev(g), dev(d), dev(s), 16, 0)
    sure = ref["gap"] >= mc.GAP_BAR
    share = mc.excluded_share(ref["gap"])
    agree = mask.cpu().numpy() == ref["masks"]
    print("%s sparse=%d: %.3f %% excluded, %d of %d differ overall" % (mc.shape_tag(shape), sparse, 100 * share, (~agree).sum(), agree.size))
    assert share <= mc.EXCLUDED_CAP
    assert agree[sure].all()
    assert rel_err(hist.cpu().numpy(), ref["hist"]) <= mc.TEST_RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.BIG_SHAPES, ids=mc.shape_tag)
@pytest.mark.parametrize("sparse", (True, False), ids=("sp", "nosp"))
def test_gradients_match_the_restatement_under_the_device_masks(shape, sparse):
    g, d, s, cot, _ = big(shape, sparse)
    gt, dt, st = dev(g), dev(d), dev(s)
    _, _, mask = abi_forward(gt, dt, st, 16, 0)
    want = mc.restate(g, d, s, 16, cot, masks=mask.cpu().numpy())
    _, gg, gb = grads(gt, dt, st, dev(cot))
    eg, eb = mc.grad_err(gg.cpu().numpy(), want["grad_guidance"]), mc.grad_err(gb.cpu().numpy(), want["grad_blur"])
    print("%s sparse=%d: guidance %.3e blur %.3e" % (mc.shape_tag(shape), sparse, eg, eb))
    assert eg <= mc.TEST_RTOL and eb <= mc.TEST_RTOL
    assert gg.shape == gt.shape and gb.shape == dt.shape and float(gg.abs().max()) > 0
    # steps_per_launch does not reach the gradients, and neither does a second run
    for S in (1, 16):
        _, gg2, gb2 = grads(gt, dt, st, dev(cot), 16, S)
        assert same_bits(gg2, gg) and same_bits(gb2, gb)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_NAMES)
def test_gradients_match_the_reference(name):
    z, (g, d, s, T, cot) = golden(name)
    out, gg, gb = grads(dev(g), dev(d), dev(s), dev(cot), T)
    errs = (rel_err(out.cpu().numpy(), z["out"]), mc.grad_err(gg.cpu().numpy(), z["grad_guidance"]), mc.grad_err(gb.cpu().numpy(), z["grad_blur"]))
    print("%s: out %.3e guidance %.3e blur %.3e" % ((name,) + errs))
    assert max(errs) <= mc.TEST_RTOL
    if name.startswith("tie015"):
        assert same_bits(gg[:, 0], gg[:, 1]) and not same_bits(gg[:, 5].abs(), gg[:, 0].abs())


@pytest.mark.gpu
def test_wide_guidance_gets_exact_zeros_past_channel_7_and_every_element_is_written():
    z, (g, d, s, T, _) = golden("fwd_2x12x57x77_sp")
    cot = mc.make_cotangent(5, g.shape)
    gt, dt, st = dev(g), dev(d), dev(s)
    _, gg, gb = grads(gt, dt, st, dev(cot))
    assert gg.shape == (2, 12, 57, 77) and not bool(gg[:, 8:].any()) and bool(torch.isfinite(gg).all()) and bool(torch.isfinite(gb).all())
    assert float(gg[:, :8].abs().max()) > 0
    _, g8, b8 = grads(gt[:, :8].contiguous(), dt, st, dev(cot))
    assert same_bits(g8, gg[:, :8]) and same_bits(b8, gb)
    # through the ABI into NaN-filled buffers with a guard element either side
    L = _lib.lib()
    B, C, H, W = g.shape
    _, hist, mask = abi_forward(gt, dt, st, 16, 0)
    gbuf = torch.full((B * C * H * W + 2,), float("nan"), device=DEV)
    bbuf = torch.full((B * H * W + 2,), float("nan"), device=DEV)
    work = torch.full((L.cspn_max8_workspace_bytes(B, H, W, 16, 1) // 4,), float("nan"), device=DEV)
    ct = dev(cot)
    _lib.check(L.cspn_max8_backward(gt.data_ptr(), gt.stride(0), gt.stride(1), C, dt.data_ptr(), st.data_ptr(), hist.data_ptr(), mask.data_ptr(),
                                    ct.data_ptr(), gbuf[1:].data_ptr(), bbuf[1:].data_ptr(), work.data_ptr(), B, H, W, 16,
                                    torch.cuda.current_stream().cuda_stream), "cspn_max8_backward")
    torch.cuda.synchronize()
    assert bool(torch.isnan(gbuf[[0, -1]]).all()) and bool(torch.isnan(bbuf[[0, -1]]).all())
    assert same_bits(gbuf[1:-1].view(B, C, H, W), gg) and same_bits(bbuf[1:-1].view(B, 1, H, W), gb)
    # the sparse pixels keep their value, so no gradient passes them
    assert not bool(gb[st > 0].any())


@pytest.mark.gpu
def test_needs_input_grad_combinations():
    z, (g, d, s, T, cot) = golden("grad_1x8x9x7_sp")
    ct = dev(cot)
    _, gg, gb = grads(dev(g), dev(d), dev(s), ct)
    gt, dt, st = dev(g).requires_grad_(True), dev(d), dev(s).requires_grad_(True)
    F.cspn_max8_propagate(gt, dt, st).backward(ct)
    assert same_bits(gt.grad, gg) and dt.grad is None and st.grad is None       # the sparse plane never gets a gradient
    gt, dt = dev(g), dev(d).requires_grad_(True)
    F.cspn_max8_propagate(gt, dt, dev(s)).backward(ct)
    assert same_bits(dt.grad, gb) and gt.grad is None
    assert not F.cspn_max8_propagate(dev(g), dev(d), st).requires_grad
    with torch.no_grad():
        assert not F.cspn_max8_propagate(dev(g).requires_grad_(True), dev(d), dev(s)).requires_grad
    p2 = dev(g).requires_grad_(True)
    (g1,) = torch.autograd.grad(F.cspn_max8_propagate(p2, dev(d), dev(s)), p2, ct, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()                                                      # double backward raises


@pytest.mark.gpu
def test_argument_errors_on_the_device():
    g, d = torch.rand(1, 8, 3, 5, device=DEV), torch.rand(1, 1, 3, 5, device=DEV)
    with pytest.raises(TypeError, match="fp32 only"):
        F.cspn_max8_propagate(g.half(), d.half())
    with pytest.raises(TypeError, match="fp32 only"):
        CSPN.AffinityPropagate()(g, d, d.double())
    with pytest.raises(ValueError, match="guidance must be"):
        F.cspn_max8_propagate(g[:, :7], d)
    with pytest.raises(ValueError, match="blur_depth has shape"):
        F.cspn_max8_propagate(g, d[:, :, :2])
    with pytest.raises(ValueError, match="exactly one channel"):
        F.cspn_max8_propagate(g, d, torch.rand(1, 2, 3, 5, device=DEV))
    with pytest.raises(ValueError, match="prop_time"):
        F.cspn_max8_propagate(g, d, None, 0)
    with pytest.raises(ValueError, match="steps_per_launch"):
        F.cspn_max8_propagate(g, d, None, 16, 17)
    with pytest.raises(RuntimeError, match="ROCm device"):
        F.cspn_max8_propagate(g, d.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", (True, False), ids=("sp", "nosp"))
def test_three_regions_along_both_axes_do_not_change_a_bit(sparse):
    """1 x 8 x 120 x 200: for steps_per_launch 16 there are 6 x 6 regions, for 8 four by four, for 4 four by three — interior
    regions whose owned range comes from the halo on both sides, as the production shapes have them."""
    g, d, s = mc.make_inputs(1903, (1, 8, 120, 200), sparse)
    gt, dt, st = dev(g), dev(d), dev(s)
    base, hist, mask = abi_forward(gt, dt, st, 16, 1)
    e = rel_err(base.cpu().numpy(), mc.restate(g, d, s, 16)["out"])
    print("120x200 sparse=%d: %.3e" % (sparse, e))
    assert e <= mc.TEST_RTOL and not bool(torch.isnan(hist).any())
    for S in (2, 4, 8, 16, 0):
        o2, h2, m2 = abi_forward(gt, dt, st, 16, S)
        assert same_bits(o2, base) and same_bits(h2, hist) and torch.equal(m2, mask), S
    cot = dev(mc.make_cotangent(1903, (1, 8, 120, 200)))
    _, gg, gb = grads(gt, dt, st, cot, 16, 1)
    _, gg2, gb2 = grads(gt, dt, st, cot, 16, 16)
    assert same_bits(gg2, gg) and same_bits(gb2, gb)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.BIG_SHAPES, ids=mc.shape_tag)
@pytest.mark.parametrize("sparse", (True, False), ids=("sp", "nosp"))
def test_no_lds_is_read_before_it_is_written(shape, sparse):
    g, d, s, cot, _ = big(shape, sparse)
    gt, dt, st, ct = dev(g), dev(d), dev(s), dev(cot)
    out, gg, gb = grads(gt, dt, st, ct)
    with lds_poison():
        out_p, gg_p, gb_p = grads(gt, dt, st, ct)
        inf_p = F.cspn_max8_propagate(gt, dt, st, 16, 3)
        torch.cuda.synchronize()
    assert same_bits(out_p, out) and same_bits(gg_p, gg) and same_bits(gb_p, gb) and same_bits(inf_p, out)
    assert not bool(torch.isnan(out).any())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", mc.BIG_SHAPES, ids=mc.shape_tag)
@pytest.mark.parametrize("sparse", (True, False), ids=("sp", "nosp"))
def test_captured_forward_and_backward_replay_the_eager_bits(shape, sparse):
    g, d, s, cot, _ = big(shape, sparse)
    g2, d2, _ = mc.make_inputs(77, shape, sparse)
    static_g, static_d, st, ct = dev(g).requires_grad_(True), dev(d).requires_grad_(True), dev(s), dev(cot)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            F.cspn_max8_propagate(static_g, static_d, st).backward(ct)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    static_g.grad = static_d.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = F.cspn_max8_propagate(static_g, static_d, st)
        static_out.backward(ct)
    for ga, da in ((g2, d2), (g, d), (g2, d2)):
        with torch.no_grad():
            static_g.copy_(dev(ga))
            static_d.copy_(dev(da))
        graph.replay()
        torch.cuda.synchronize()
        out, gg, gb = grads(dev(ga), dev(da), st, ct)
        assert same_bits(static_out, out) and same_bits(static_g.grad, gg) and same_bits(static_d.grad, gb)


@pytest.mark.gpu
def test_step_does_not_synchronise():
    z, (g, d, s, T, cot) = golden("grad_1x8x9x7_sp")
    gt, dt, st, ct = dev(g).requires_grad_(True), dev(d).requires_grad_(True), dev(s), dev(cot)
    F.cspn_max8_propagate(gt, dt, st).backward(ct)
    gt.grad = dt.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        F.cspn_max8_propagate(gt, dt, st).backward(ct)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert mc.grad_err(gt.grad.cpu().numpy(), z["grad_guidance"]) <= mc.TEST_RTOL

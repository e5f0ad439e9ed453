"""Config 3's fp16 paths (K = 5 softmax affinity, fp16 guidance: BASELINE config 3) held PER FRAME, per input regime and for the
gradients to the distance the reference's OWN half-precision runs keep from the fp32 oracle (goldens G16, tests/golden/make_golden_g16.py).

The reference can run half inputs two ways (CSPN_ours.py:24-54): `taps16` — fp16 softmax taps, fp32 state (its promotion rules under the
default dtype float32) — and `half` — half precision end to end.  Each path of this package that keeps an fp32 state is held to the
taps16 run's distance, each path with fp16 planes to the half run's, x 1.1 for the different rounding points (G15's single frame: the
package's paths are at or below the reference there).  Per frame: a fault that hits only some frames of a batch (the second 12-frame
round of the one-launch kernel, a ragged tile, frame 0's halo) moves that frame and no other."""
import ctypes

import numpy as np
import pytest
import torch

import cspn_monodepth_amd as pkg
from cspn_monodepth_amd import functional as F
from conftest import bits_equal, golden_names, load_golden, rmse
from oracle import cspn_oracle as orc
from test_hip_kres import _spin_limit, dev, multi_launch, resident

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR = 1.1
# path -> the reference run it is held to
PATHS = {"d2_default": "half", "reference": "taps16", "fma16": "half", "multi16": "half", "history": "half"}


def f32(a):
    return None if a is None else a.astype(np.float32)


def dist(o, want):
    """(max |o - want|, rmse) / max |want| of one frame (or one batch)."""
    scale = float(np.abs(want).max())
    return float(np.abs(o - want).max()) / scale, rmse(o, want) / scale


def run_path(path, gd, x, sp, T):
    """One call of `path` on fp16 numpy inputs (guidance [B,24,H,W], x / sparse [B,1,H,W]) -> the refined depth as fp32 [B,H,W]."""
    gt, xt, st = dev(gd), dev(x), dev(sp)
    x0, s0 = xt[:, 0].contiguous(), None if st is None else st[:, 0].contiguous()
    with torch.no_grad():
        if path == "d2_default":                                   # the module's default no-grad call: cspnk_d2 where one oct per thread fits
            with resident("on"):
                out = pkg.CSPN_ours.AffinityPropagate(T, state_dtype=None)(xt, gt, sparse_depth=st)[:, 0]
        elif path == "reference":                                  # fp32 state: the FMA kernel cspnk_resident
            with resident("on"):
                out = pkg.CSPN_ours.AffinityPropagate(T, state_dtype="reference")(xt, gt, sparse_depth=st)[:, 0]
            assert out.dtype == torch.float32
        elif path == "fma16":                                      # fp16 planes on the FMA kernel
            with resident("on"):
                out = F.pac_forward_resident(gt, x0, s0, T, step_form=F.STEP_FMA)
        elif path == "multi16":                                    # fp16 planes on the multi-launch schedule
            with resident("off"):
                out = pkg.CSPN_ours.AffinityPropagate(T, state_dtype=None)(xt, gt, sparse_depth=st)[:, 0]
        else:                                                      # the training forward (history + published taps)
            with resident("on"):
                out, hist, _ = F.pac_forward_resident_history(gt, x0, s0, T)
            assert bits_equal(out, hist[T - 1])
    torch.cuda.synchronize()
    F.ensure_resident_ok()
    if path != "reference":
        assert out.dtype == torch.float16, path
    o = out.float().cpu().numpy()
    assert np.isfinite(o).all(), path
    return o


@pytest.mark.parametrize("tag", ["nosp", "sp"])
def test_config3_paths_per_frame_against_the_references_half_runs(tag, c_oracle):
    """G16a: 24 distinct 228 x 304 frames at config 3.  Every path runs the batch in one call and every frame in a call of its own:
    each frame's distance from the fp32 oracle is at most 1.1 x the reference run's distance FOR THAT FRAME (max and rmse), and on
    the resident paths frame b of the batch call has the bits of frame b run alone (no round / tile indexing that depends on where
    a frame sits in the batch).  The default call is asserted to be the one-launch dot-product instance, as in test_config3_full_size_fp16."""
    from test_hip_production import assert_resident_instance
    z = load_golden("g16a_k5_t12_fp16_b24_%s" % tag)
    B, H, W = (int(v) for v in z["shape"])
    T = int(z["T"])
    gd, x, sp = orc.g16_inputs(z, c_oracle)
    with resident("on"):
        kp = F.pac_resident_supported(dev(gd), dev(x)[:, 0], None if sp is None else dev(sp)[:, 0], T)
    assert_resident_instance(kp, (4, 2, 10, 152, 23, 1, 12, 2), "config3")
    assert kp["threads"] == 768 and F._KRES_STEP_FORM == F._lib.STEP_AUTO
    want = c_oracle.pac_forward(f32(x), f32(gd), f32(sp), T)[:, 0]
    worst = {}
    for path, run in PATHS.items():
        ref = z["ref_err_" + run]
        batch = run_path(path, gd, x, sp, T)
        single = np.stack([run_path(path, gd[b:b + 1], x[b:b + 1], None if sp is None else sp[b:b + 1], T)[0] for b in range(B)])
        if path != "multi16":
            bad = [b for b in range(B) if not np.array_equal(batch[b], single[b])]
            assert not bad, (path, "frames whose bits depend on their place in the batch", bad)
        ratios = []
        for b in range(B):
            for o in (batch[b], single[b]):
                emax, erms = dist(o, want[b])
                ratios.append((emax / float(ref[b, 0]), erms / float(ref[b, 1]), b))
                assert emax <= FACTOR * float(ref[b, 0]) and erms <= FACTOR * float(ref[b, 1]), (path, b, emax, erms, ref[b])
        worst[path] = (max(r[0] for r in ratios), max(r[1] for r in ratios))
    print("G16a %s worst per-frame ratio to the reference (max, rmse):" % tag, {k: ("%.3f" % v[0], "%.3f" % v[1]) for k, v in worst.items()})


@pytest.mark.parametrize("name", golden_names("g16b_"))
def test_config3_paths_in_four_input_regimes(name, c_oracle):
    """G16b: peaky softmax (guidance x 8: taps in fp16's subnormal range), near-uniform taps (x 0.05), a KITTI depth range (0-85) and a
    saturated softmax (one channel at +30 on a tenth of the pixels), on shapes where the dot-product kernel runs: every path within
    1.1 x the corresponding reference run's distance from the fp32 oracle (max and rmse)."""
    z = load_golden(name)
    B, H, W = (int(v) for v in z["shape"])
    T = int(z["T"])
    gd, x, sp = orc.g16_inputs(z, c_oracle)
    assert F.kres_plan(5, B, H, W, T, int(sp is not None))["quads_per_thread"] == 1       # (the default call is cspnk_d2)
    want = c_oracle.pac_forward(f32(x), f32(gd), f32(sp), T)[:, 0]
    ratios = {}
    for path, run in PATHS.items():
        ref = z["ref_err_" + run]
        emax, erms = dist(run_path(path, gd, x, sp, T), want)
        ratios[path] = ("%.3f" % (emax / float(ref[0])), "%.3f" % (erms / float(ref[1])))
        assert emax <= FACTOR * float(ref[0]) and erms <= FACTOR * float(ref[1]), (path, emax, erms, ref)
    print("G16b %s ratio to the reference (max, rmse):" % name, ratios)


_FP64_GRADS = {}


@pytest.mark.parametrize("mode", ["on", "off"])
@pytest.mark.parametrize("name", golden_names("g16c_"))
def test_fp16_gradients_against_the_references_half_autograd(name, mode, c_oracle):
    """G16c: dL/dx and dL/dguided through CSPN_ours.AffinityPropagate(T, state_dtype=None) on fp16 inputs and an fp16 cotangent, resident
    launches on and off: at most 1.1 x the distance of the reference's half-precision autograd from the fp64 oracle (max and rmse over
    max |fp64 gradient|).  The hand-written backward accumulates in fp32, so it has no reason to be further away than the reference."""
    z = load_golden(name)
    B, H, W = (int(v) for v in z["shape"])
    T, seed = int(z["T"]), int(z["seed"])
    gd, x, sp = orc.g16_inputs(z, c_oracle)
    cot = c_oracle.hash_normal(seed, 9, (B, 1, H, W)).astype(np.float16)
    if name not in _FP64_GRADS:                                    # (the fp64 oracle is the slow part: once per case, not per mode)
        _FP64_GRADS[name] = orc.pac_backward(f32(x), f32(gd), f32(sp), f32(cot), T, np.float64)
    wx, wg = _FP64_GRADS[name]
    xg, gg = dev(x).requires_grad_(True), dev(gd).requires_grad_(True)
    with resident(mode):
        out = pkg.CSPN_ours.AffinityPropagate(T, state_dtype=None)(xg, gg, sparse_depth=dev(sp))
        out.backward(dev(cot))
    torch.cuda.synchronize()
    F.ensure_resident_ok()
    ref = z["ref_grad_err_half"]
    got = [dist(xg.grad.float().cpu().numpy(), wx), dist(gg.grad.float().cpu().numpy(), wg)]
    print("G16c %s resident %s ratio to the reference (dx max, rmse; dguided max, rmse): %.3f %.3f %.3f %.3f"
          % (name, mode, got[0][0] / ref[0, 0], got[0][1] / ref[0, 1], got[1][0] / ref[1, 0], got[1][1] / ref[1, 1]))
    for i, what in enumerate(("dL/dx", "dL/dguided")):
        assert got[i][0] <= FACTOR * float(ref[i, 0]) and got[i][1] <= FACTOR * float(ref[i, 1]), (what, got[i], ref[i])


# ------------------------------------------------------------------------------------------------ the guard at phase length 1
def _inputs(c_oracle, B, H, W, sparse, seed):
    gd = c_oracle.hash_normal(seed, 1, (B, 24, H, W)).astype(np.float16)
    x = c_oracle.hash_uniform(seed, 2, (B, 1, H, W), 0.0, 10.0).astype(np.float16)
    s = c_oracle.hash_sparse(seed, 3, x.astype(np.float32), max(500.0 / (H * W), 0.02)).astype(np.float16) if sparse else None
    return gd, x, s


def test_fma_phase_length_1_exists_at_one_step_only():
    """Why the guarded FMA calls below run T = 1: a phase length of 1 has no tiling when there is more than one phase (every phase must
    start in buffer 0: kgeom_fill), so the FMA form rounds after every step only when T = 1 — and the default plan of a T = 1 call is it."""
    for B, H, W in ((2, 40, 64), (24, 228, 304), (5, 60, 72)):
        for sp in (0, 1):
            assert F.kres_plan(5, B, H, W, 12, sp, 256, 1) is None
            assert F.kres_plan(5, B, H, W, 1, sp, 256)["steps_per_phase"] == 1


G1 = [(2, 40, 64, True), (24, 228, 304, False), (8, 352, 1216, False)]


@pytest.mark.parametrize("B,H,W,explicit", G1, ids=["%dx%dx%d_%s" % (c[0], c[1], c[2], "S1" if c[3] else "default") for c in G1])
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
def test_guarded_fma_call_at_phase_length_1_has_the_multi_launch_bits(B, H, W, explicit, sparse, c_oracle):
    """fp16 guidance + fp16 planes on the FMA form with phase length 1, every tile forced to give up (one poll): steps_per_phase = 1 with
    STEP_FMA pinned, and DEFAULT calls that land on the FMA kernel at T = 1 (shapes whose plan has two octs per thread, where the
    dot-product kernel does not run).  The result is the multi-launch schedule's bits at one step per launch.  (A single-phase launch
    has no neighbour to wait for, so these calls finish without the guard's re-computation; the next test runs that re-computation.)"""
    import warnings
    T = 1
    gd, x, s = _inputs(c_oracle, B, H, W, sparse, 230 + B)
    gt, xt, st = dev(gd), dev(x), dev(s)
    x0, s0 = xt[:, 0].contiguous(), None if st is None else st[:, 0].contiguous()
    rp = F.kres_plan(5, B, H, W, T, int(sparse))
    assert rp["steps_per_phase"] == 1 and (explicit or rp["quads_per_thread"] != 1), rp
    ref = multi_launch(xt, gt, st, T, 1, None)[:, 0]
    with torch.no_grad(), resident("on"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with _spin_limit(1):
            if explicit:
                out = F.pac_forward_resident(gt, x0, s0, T, steps_per_phase=1, spin_limit=1, step_form=F.STEP_FMA)
            else:
                out = F.pac_forward_resident(gt, x0, s0, T)
        total = out.double().sum()                      # a GPU consumer right behind the call
        assert float(total) == float(ref.double().sum())
        assert bits_equal(out, ref, which="FMA form at phase length 1, guarded")
        F.ensure_resident_ok()
    F.check_resident_errors()


def _repair_entry():
    """The guard's re-computation of cspnk_forward_resident (cspn_detail::kres_repair_launch, csrc/cspn_repair.hip), launched on its own
    through the library's exported symbol: the public calls reach it only after a real time-out."""
    fn = getattr(pkg._lib.lib(), "_ZN11cspn_detail18kres_repair_launchEPKviiS1_S1_PviPKjjiiiiiiiiS2_")
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_uint] + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    return fn


@pytest.mark.parametrize("T,S", [(12, 1), (1, 1), (12, 2), (12, 4)], ids=lambda v: str(v))
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
def test_guard_recomputes_the_form_its_launch_ran(T, S, sparse, c_oracle):
    """The guard is told which step form its launch ran, and re-computes THAT form (it inferred the dot-product form from
    round_every == 1, so an FMA launch of phase length 1 with fp16 guidance and planes — T = 1 — would have been re-computed with the
    dot-product arithmetic).  With the abort word set to the call's sequence number the guard re-computes every tile: FMA form at
    round_every = S, fp16 and fp32 planes -> the multi-launch schedule's bits at S steps per launch; dot-product form -> a clean
    cspnk_d2 call's bits."""
    B, H, W = 2, 40, 64
    gd, x, s = _inputs(c_oracle, B, H, W, sparse, 240)
    gt, xt, st = dev(gd), dev(x), dev(s)
    fn = _repair_entry()
    seq = 7
    abort = torch.full((4,), seq, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count

    def repair(form, sdt, round_every):
        x0 = xt[:, 0].to(sdt).contiguous()
        s0 = None if st is None else st[:, 0].to(sdt).contiguous()
        out = torch.full((B, H, W), float("nan"), dtype=sdt, device=DEV)
        ok = fn(gt.data_ptr(), F.CSPN_F16, 5, x0.data_ptr(), None if s0 is None else s0.data_ptr(), out.data_ptr(), F._dt(x0),
                abort.data_ptr(), seq, B, H, W, T, round_every, form, int(sparse), n_cu, stream)
        assert ok == 1
        torch.cuda.synchronize()
        return out, x0, s0

    for sdt, state in ((torch.float16, None), (torch.float32, torch.float32)):
        out, _, _ = repair(F.STEP_FMA, sdt, S)
        with torch.no_grad():
            ref = multi_launch(xt, gt, st, T, S, state)[:, 0]
        assert bits_equal(out, ref, which="FMA form re-computed by the guard, round_every %d, %s" % (S, sdt))
    if S == 1:
        out, x0, s0 = repair(F.STEP_DOT2, torch.float16, 1)
        with torch.no_grad(), resident("on"):
            clean = F.pac_forward_resident(gt, x0, s0, T, step_form=F.STEP_DOT2)
        F.ensure_resident_ok()
        assert bits_equal(out, clean, which="dot-product form re-computed by the guard")

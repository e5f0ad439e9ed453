"""CPU tests of the boundary: the C-ABI library loads and exports every symbol the header declares,
the host-side mirror of the reference interface behaves like the reference's module API, and nothing
in the product path can silently fall back to a CPU implementation."""
import ctypes
import os
import re

import pytest
import torch

import cspn_monodepth_amd as pkg
from cspn_monodepth_amd import _lib
from conftest import ROOT


# The contract of every family of the native library, stated here in literals (nothing below is read from the code under test):
# name -> (header under include/, version macro, version, translation units, words a name of the family starts with after "cspn",
# every function the header declares).  A new family is one more row.
FAMILY_CONTRACT = {
    "core": ("cspn_hip.h", "CSPN_ABI_VERSION", 10,
             ("cspn_propagate.hip", "cspn_resident.hip", "cspnk_resident.hip", "cspnk_d2.hip", "cspn_prepare.hip", "cspn_backward.hip",
              "cspn_metrics.hip", "cspn_metrics_frame.hip", "cspn_debug.hip", "cspn_repair.hip", "pac_conv2d.hip", "pac_conv2d_s2.hip",
              "cspn_unpool.hip"), ("",),
             ("cspn_abi_version", "cspn_last_error", "cspn_plan_resolve", "cspn3_prepare", "cspn_pac_prepare",
              "cspn_propagate_workspace_bytes", "cspn_propagate", "cspn_propagate_scored", "cspn_propagate_transposed",
              "cspn3_propagate_from_guidance", "cspn_transpose_weights", "cspn3_resident_plan", "cspn3_resident_workspace_bytes",
              "cspn3_forward_resident", "cspn3_transposed_resident", "cspn3_transposed_resident_guidance", "cspnk_resident_plan",
              "cspnk_resident_workspace_bytes", "cspnk_forward_resident", "cspnk_forward_resident_history", "cspnk_transposed_resident",
              "cspn_grad_weights", "cspn3_grad_guidance", "cspn_pac_grad_guided", "cspn3_backward_tail", "cspn_pac_backward_tail",
              "cspn_metrics_accumulate", "cspn_metrics_per_frame_workspace_bytes", "cspn_metrics_per_frame", "cspn_meter_update",
              "cspn_pac_out_size", "cspn_pac_force_generic", "cspn_pac_conv2d", "cspn_pac_conv2d_grad_input", "cspn_pac_conv2d_grad_kernel",
              "cspn_pac_nd2col", "cspn_unpool2d", "cspn_unpool2d_backward", "cspn_debug_set_lds_poison")),
    "criterion": ("cspn_criterion.h", "CSPN_CRITERION_ABI_VERSION", 1, ("cspn_criterion.hip",), ("_criterion_",),
                  ("cspn_criterion_abi_version", "cspn_criterion_workspace_bytes", "cspn_criterion_forward", "cspn_criterion_backward")),
    "max8": ("cspn_max8.h", "CSPN_MAX8_ABI_VERSION", 1, ("cspn_max8.hip",), ("_max8_",),
             ("cspn_max8_abi_version", "cspn_max8_workspace_bytes", "cspn_max8_forward", "cspn_max8_backward")),
    "abn": ("cspn_abn.h", "CSPN_ABN_ABI_VERSION", 1, ("cspn_abn.hip",), ("_abn_",),
            ("cspn_abn_abi_version", "cspn_abn_plan", "cspn_abn_workspace_bytes", "cspn_abn_forward", "cspn_abn_backward_reduce",
             "cspn_abn_backward")),
    "sparsify": ("cspn_sparsify.h", "CSPN_SPARSIFY_ABI_VERSION", 1, ("cspn_sparsify.hip",), ("_sparsify",),
                 ("cspn_sparsify_abi_version", "cspn_sparsify_slices", "cspn_sparsify_workspace_bytes", "cspn_sparsify")),
    "transform": ("cspn_transform.h", "CSPN_TRANSFORM_ABI_VERSION", 1, ("cspn_transform.hip",), ("_transform",),
                  ("cspn_transform_abi_version", "cspn_transform_first_size", "cspn_transform_workspace_bytes", "cspn_transform",
                   "cspn_transform_draw_params")),
    "losses": ("cspn_losses.h", "CSPN_LOSSES_ABI_VERSION", 1, ("cspn_losses.hip",), ("_losses_", "_berhu_", "_mean_loss_"),
               ("cspn_losses_abi_version", "cspn_losses_workspace_bytes", "cspn_berhu_forward", "cspn_berhu_backward",
                "cspn_mean_loss_forward", "cspn_mean_loss_backward")),
    "optim": ("cspn_optim.h", "CSPN_OPTIM_ABI_VERSION", 1, ("cspn_optim.hip",), ("_optim_", "_sgd_"),
              ("cspn_optim_abi_version", "cspn_sgd_plan", "cspn_sgd_step")),
    "visual": ("cspn_visual.h", "CSPN_VISUAL_ABI_VERSION", 1, ("cspn_visual.hip",), ("_visual_",),
               ("cspn_visual_abi_version", "cspn_visual_workspace_bytes", "cspn_visual_rows", "cspn_visual_features")),
}
BUILD_ONLY_HPP = ("pac_launch.hpp", "cspn_loss_units.hpp", "cspn_philox.hpp", "cspn_upconv_core.hpp")


def _header_source(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_families_are_the_nine_in_the_order_they_were_added():
    assert [f.name for f in _lib.FAMILIES] == list(FAMILY_CONTRACT)
    assert _lib.EXPORTS == FAMILY_CONTRACT["core"][5] and _lib.family("visual") is _lib.FAMILIES[-1]
    assert _lib.SOURCES == tuple(tu for row in FAMILY_CONTRACT.values() for tu in row[3])


@pytest.mark.parametrize("name", list(FAMILY_CONTRACT))
def test_family_contract(name):
    """Header, table, library and loader agree on one family: the version macro, the declared functions, their names' prefix,
    the symbols of a fresh build, the running version, and which hash the family's files belong to."""
    header, macro, version, tus, prefixes, names = FAMILY_CONTRACT[name]
    fam = _lib.family(name)
    assert fam.header == os.path.join(ROOT, "include", header)
    assert re.search(r"^#define %s %d$" % (macro, version), open(fam.header).read(), flags=re.M)
    src = _header_source(header)
    declared = sorted(set(re.findall(r"\b(cspn\w*)\s*\(", src)))
    assert declared == sorted(fam.functions) == sorted(names), (declared, list(fam.functions))
    assert all(n.startswith(tuple("cspn" + p for p in prefixes)) for n in names)
    lib = ctypes.CDLL(_lib.build())
    for n in names:
        assert hasattr(lib, n), n
    version_fn = macro.lower()
    assert version_fn in names and getattr(_lib.lib(), version_fn)() == fam.abi_version == version
    assert set(tus) <= set(_lib.SOURCES) and set(tus) == {f for f in fam.files if f.endswith(".hip")}
    if name == "core":
        assert _lib.ABI_VERSION == 10 and fam.header in _lib.HEADERS
        assert _lib.lib().cspn_propagate_workspace_bytes(24, 228, 304, 24, _lib.CSPN_F32, 0) == 2 * 24 * 228 * 304 * 4
        assert _lib.lib().cspn_propagate_workspace_bytes(24, 228, 304, 24, _lib.CSPN_F32, 1) == 0
        return
    assert set(tus) <= set(_lib.BENCH_UNRELATED)
    assert fam.header in _lib.BUILD_HEADERS and fam.header not in _lib.HEADERS
    # no family's name inside another's: not in the main header, not in a function name of any other family
    assert name not in _header_source("cspn_hip.h")
    for other, row in FAMILY_CONTRACT.items():
        if other != name:
            assert not any("cspn" + p in n for p in prefixes for n in row[5]), other
    # nothing else of the family's translation unit leaves the library: every dynamic symbol that names it is a declared one
    import shutil
    import subprocess
    if shutil.which("nm"):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True)
        ours = sorted(ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and any(p.strip("_") in ln for p in prefixes))
        assert ours == declared


def test_family_names_are_pairwise_disjoint():
    rows = [(name, set(row[5])) for name, row in FAMILY_CONTRACT.items()]
    assert all(len(row[5]) == len(set(row[5])) for row in FAMILY_CONTRACT.values())
    for i, (a, na) in enumerate(rows):
        for b, nb in rows[i + 1:]:
            assert not na & nb, (a, b, na & nb)
            assert not set(_lib.family(a).functions) & set(_lib.family(b).functions), (a, b)


def test_code_digest_covers_the_benchmarked_files_only():
    """code_digest() pins the HBM traffic recorded under profiles/ to the benchmarked kernels.  Restated here over its own file
    list; the headers only the other families see are part of the build's staleness hash, and not part of that digest."""
    for hpp in BUILD_ONLY_HPP:
        path = os.path.join(_lib.CSRC, hpp)
        assert path in _lib.BUILD_HEADERS and path not in _lib.HEADERS
    assert set(_lib.HEADERS) <= set(_lib.BUILD_HEADERS) and len(_lib.HEADERS) == 3
    import hashlib
    h = hashlib.sha256(b"")
    for path in [os.path.join(_lib.CSRC, f) for f in _lib.SOURCES if f not in _lib.BENCH_UNRELATED] + list(_lib.HEADERS):
        data = re.sub(rb"/\*.*?\*/", b"", open(path, "rb").read(), flags=re.S)
        lines = (re.sub(rb"//.*$", b"", ln).strip() for ln in data.splitlines())
        h.update(b"\n".join(re.sub(rb"\s+", b" ", ln) for ln in lines if ln))
    assert _lib.code_digest() == h.hexdigest()
    assert _lib._source_digest(["x"]) != _lib._source_digest(["x"], code_only=True)


def test_kernel_sources_carry_no_compile_time_switches():
    """csrc/ holds one form of every kernel: no conditional compilation and no object-like CSPN_* macro a -D could override.  A finished
    experiment lives as a patch under tools/probes/ (its README lists them); CSPN_PRELAUNCH, CSPN_PRE and HIP_OK are function-like."""
    conditional = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b")
    switch = re.compile(r"^\s*#\s*define\s+CSPN_[A-Z0-9_]+\s+\S")
    paths = [os.path.join(_lib.CSRC, f) for f in _lib.SOURCES] + [p for p in _lib.BUILD_HEADERS if os.path.dirname(p) == _lib.CSRC]
    assert len(paths) == len(_lib.SOURCES) + 6
    for path in paths:
        with open(path, encoding="utf-8") as fh:
            hits = [(no, ln.rstrip()) for no, ln in enumerate(fh, 1) if conditional.match(ln) or switch.match(ln)]
        assert not hits, (os.path.basename(path), hits)


def test_ctypes_signatures_match_the_recorded_ones():
    """Every exported function carries the restype and argtypes recorded in tests/golden/g26_ctypes_signatures.json
    (tools/dump_ctypes_signatures.py, written when every declaration was still a hand-written line)."""
    import json
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "g26_ctypes_signatures.json")))
    assert sorted(want) == sorted(n for row in FAMILY_CONTRACT.values() for n in row[5])
    for name, sig in want.items():
        fn = getattr(_lib.lib(), name)
        got = {"restype": getattr(fn.restype, "__name__", None), "argtypes": fn.argtypes and [t.__name__ for t in fn.argtypes]}
        assert got == sig, (name, got, sig)


def test_module_api_matches_reference_contract():
    m = pkg.CSPN_new.AffinityPropagate(24, 3)            # unet_cspn_nyu.py:357-358
    assert (m.prop_time, m.prop_kernel, m.in_feature, m.out_feature) == (24, 3, 1, 1)
    assert len(m.state_dict()) == 0 and len(list(m.parameters())) == 0
    with pytest.raises(ValueError):
        pkg.CSPN_new.AffinityPropagate(24, 5)
    p = pkg.CSPN_ours.AffinityPropagate(prop_time=24)    # unet_ours.py:304-305
    assert p.times == 24 and len(p.state_dict()) == 0
    import inspect
    assert list(inspect.signature(m.forward).parameters) == ["guidance", "blur_depth", "sparse_depth"]
    assert list(inspect.signature(p.forward).parameters) == ["x", "guided", "sparse_depth"]


def test_no_cpu_fallback():
    m = pkg.CSPN_new.AffinityPropagate(24, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(torch.randn(1, 8, 4, 4), torch.rand(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        pkg.CSPN_ours.AffinityPropagate(3)(torch.rand(1, 1, 4, 4), torch.randn(1, 8, 4, 4))
    with pytest.raises(RuntimeError):
        pkg.evaluation.metric_sums(torch.rand(4), torch.rand(4))
    # the product package never imports the oracle
    for root, _, files in os.walk(os.path.join(ROOT, "cspn_monodepth_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, flags=re.M), f


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_shard_bounds_and_finalize():
    ev = pkg.evaluation
    for n, w in ((24, 8), (8, 8), (24, 5), (3, 4)):
        spans = [ev.shard_bounds(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
        assert max(hi - lo for lo, hi in spans) - min(hi - lo for lo, hi in spans) <= 1
    import numpy as np
    from oracle import cspn_oracle as orc
    from conftest import load_golden
    z = load_golden("g7_metrics")
    fin = ev.finalize_metrics(orc.metric_sums(z["pred"], z["target"]))
    for k, v in zip(ev.METRIC_NAMES, z["metrics"]):
        assert np.isclose(fin[k], v, rtol=2e-6), k


def test_widening_entry_points_reject_bad_arguments_without_a_gpu():
    """Argument validation of the PAC-conv / un-pooling entries happens on the host before any launch: a failing call
    returns 0 and leaves a message in cspn_last_error() (the In-Place ABN convention the header adopts)."""
    L = _lib.lib()
    G = _lib.cspn_conv_geometry
    err = lambda: L.cspn_last_error().decode()                                     # noqa: E731
    ok_geom = G(3, 3, 1, 1, 1, 1, 1, 1, 0, 0, 0)
    one = ctypes.c_void_p(16)                                                      # never dereferenced: validation fails first
    assert L.cspn_pac_conv2d(one, one, one, _lib.CSPN_F32, 1, 3, 2, 8, 8, ctypes.byref(ok_geom), None) == 0
    assert "Incompatible input and kernel sizes" in err()                          # kernel_ch must be 1 or C (pac.py:77-78)
    assert L.cspn_pac_conv2d(one, one, one, 7, 1, 3, 1, 8, 8, ctypes.byref(ok_geom), None) == 0 and "dtype" in err()
    assert L.cspn_pac_conv2d(None, one, one, _lib.CSPN_F32, 1, 3, 1, 8, 8, ctypes.byref(ok_geom), None) == 0 and "null" in err()
    assert L.cspn_pac_conv2d(one, one, one, _lib.CSPN_F32, 1, 3, 1, 8, 8, None, None) == 0 and "geom" in err()
    big = G(9, 9, 1, 1, 0, 0, 1, 1, 0, 0, 0)                                       # window larger than the padded input
    assert L.cspn_pac_conv2d(one, one, one, _lib.CSPN_F32, 1, 1, 1, 4, 4, ctypes.byref(big), None) == 0 and "empty output" in err()
    tr = G(3, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1)                                        # transposed geometry is nd2col-only
    assert L.cspn_pac_conv2d_grad_input(one, one, one, _lib.CSPN_F32, 1, 1, 1, 4, 4, ctypes.byref(tr), None) == 0
    assert "nd2col only" in err()
    ho, wo = ctypes.c_int(), ctypes.c_int()
    assert L.cspn_pac_out_size(6, 7, ctypes.byref(tr), ctypes.byref(ho), ctypes.byref(wo)) == 1 and (ho.value, wo.value) == (12, 14)
    assert L.cspn_unpool2d(one, one, _lib.CSPN_F32, 4, 5, 6, 2, 11, 12, None) == 0 and "must lie in" in err()   # oH > 2*H
    assert L.cspn_unpool2d(one, one, _lib.CSPN_F32, 4, 5, 6, 0, 5, 6, None) == 0 and "scale" in err()
    assert L.cspn_unpool2d_backward(one, None, _lib.CSPN_F32, 4, 5, 6, 2, 10, 12, None) == 0 and "null" in err()


def test_batch_average_meter_reproduces_reference_averaging():
    """the reference's eval prints the batch-weighted mean of per-batch metrics (Result.evaluate +
    AverageMeter, libs/metrics.py:49-127), not the pixel-weighted global figure.  Checked against the numpy oracle's
    restatement of Result.evaluate (pinned by golden G7) on batches with unequal valid-pixel counts."""
    import numpy as np
    import torch
    from cspn_monodepth_amd import evaluation as ev
    from oracle import cspn_oracle as orc
    rng = np.random.default_rng(3)
    meter = ev.BatchAverageMeter()
    want = np.zeros(10)
    total = np.zeros(10)
    n_tot = 0
    for n, frac in ((1, 0.9), (3, 0.4), (2, 0.7)):
        t = rng.uniform(0.5, 10, (n, 1, 12, 16)).astype(np.float32)
        t[rng.random(t.shape) > frac] = 0
        p = (np.abs(t + rng.normal(0, 0.3, t.shape)) + 0.05).astype(np.float32)
        sums = orc.metric_sums(p, t)
        meter.update(torch.from_numpy(sums), n=n)
        ref, _ = orc.evaluate_metrics(p, t)                       # Result.evaluate of this batch
        want += n * np.asarray(ref)
        total += sums
        n_tot += n
    avg = meter.average()
    assert avg["count"] == n_tot
    for k, v in zip(ev.METRIC_NAMES, want / n_tot):
        assert np.isclose(avg[k], v, rtol=1e-6), k
    glob = ev.finalize_metrics(torch.from_numpy(total))
    assert not np.isclose(glob["rmse"], avg["rmse"], rtol=1e-4)   # the two conventions really differ


def test_resident_plan_host_rules():
    """Host-side tiling rules of the weight-resident launch (no GPU needed: cspn3_resident_plan is pure host code).
    * a launch never has more workgroups than CUs, whole images per launch;
    * phases have an even number of steps whenever there is more than one phase (every phase starts in LDS buffer 0,
      the other buffer being a compile-time distance away), an odd request with several phases has no plan;
    * one depth buffer fits the fixed slot (16352 floats) and the launch fits 160 KB of LDS."""
    from cspn_monodepth_amd import functional as F
    for (B, H, W) in ((24, 228, 304), (8, 352, 1216), (1, 352, 1216), (3, 228, 304), (5, 100, 64)):
        for blend in (0, 1):
            p = F.resident_plan(B, H, W, 24, blend, 256)
            assert p is not None, (B, H, W)
            assert p["tiles_x"] * p["tiles_y"] * p["images_per_launch"] <= 256
            assert p["launches"] == -(-B // p["images_per_launch"])
            assert p["steps_per_phase"] % 2 == 0 and p["lds_bytes"] <= 160 * 1024
            hx = -(-(p["steps_per_phase"] - 1) // 4) * 4
            dr, ls = p["tile_h"] + 2 * (p["steps_per_phase"] - 1) + 2, p["tile_w"] + 2 * hx + 8
            assert dr * ls <= 16352, p
            assert p["quads_per_thread"] <= 5 and p["threads"] == 512
    assert F.resident_plan(24, 228, 304, 24, 0, 256)["steps_per_phase"] == 8            # the fitted cost model's choice
    assert F.resident_plan(8, 352, 1216, 24, 0, 256)["steps_per_phase"] == 8
    assert F.resident_plan(24, 228, 304, 24, 0, 256, steps_per_phase=5) is None         # 5 phases of 5 steps: odd
    assert F.resident_plan(24, 228, 304, 5, 0, 256, steps_per_phase=5) is not None      # a single phase may be odd
    assert F.resident_plan(24, 228, 304, 24, 0, 256, steps_per_phase=6)["steps_per_phase"] == 6
    assert F.resident_plan(4, 64, 30, 24, 0, 256) is None                               # W % 4 != 0


def test_production_shapes_keep_their_resident_instances():
    """The tilings (hence the kernel instances: NQ = quads per thread, CLEAN, phases) the default path runs for the BASELINE
    configs on the 256 CUs of an MI355X — the same table tests/test_hip_production.py asserts on the GPU, checked here without one
    (cspn3_resident_plan / cspnk_resident_plan are pure host code): a change to resident_geometry that moves a production shape to
    another instance fails on the CPU suite already."""
    from cspn_monodepth_amd import functional as F
    keys = ("steps_per_phase", "tiles_x", "tiles_y", "tile_w", "tile_h", "quads_per_thread", "images_per_launch", "launches")
    want = {(24, 228, 304): (8, 2, 5, 152, 46, 5, 24, 1), (3, 228, 304): (8, 7, 12, 44, 19, 1, 3, 1),
            (1, 352, 1216): (8, 11, 22, 112, 16, 2, 1, 1), (8, 352, 1216): (8, 8, 8, 152, 44, 5, 4, 2)}
    for (B, H, W), w in want.items():
        for blend in (0, 1):
            p = F.resident_plan(B, H, W, 24, blend, 256)
            assert tuple(p[k] for k in keys) == w and p["threads"] == 512, ((B, H, W), {k: p[k] for k in keys})
    for blend in (0, 1):            # config 3: K = 5, fp16 guidance — cspnk_d2 with 768 threads, both 12-image halves in one launch
        p = F.kres_plan(5, 24, 228, 304, 12, blend, 256)
        assert tuple(p[k] for k in keys) == (4, 2, 10, 152, 23, 1, 12, 2) and p["threads"] == 768, p


_PLAN_TABLE = os.path.join(ROOT, "tests", "golden", "g20_resident_plans.json")
_PLAN_FIELDS = tuple(name for name, _ in _lib.cspn_resident_plan._fields_)
_PLAN_SHAPES = ((7, 12), (37, 8), (60, 64), (61, 76), (100, 148), (228, 304), (352, 1216), (64, 30), (40, 152))


def _resident_plan_cases():
    """The arguments of the recorded plan calls: the full grid over batch, shape, steps, blend, CU count, requested phase length
    and workgroup size (and K / guidance dtype for the K x K engine), thinned to every 23rd / 71st point — strides that share no
    factor with an axis length, so every value of every axis and every pair of neighbouring axes' values still occurs."""
    import itertools
    Bs, Ts, cus, spps = (1, 2, 3, 5, 8, 24, 48), (1, 3, 7, 12, 24, 60), (64, 256), (0, 2, 5, 6, 8, 12)
    grid3 = itertools.product(Bs, _PLAN_SHAPES, Ts, (0, 1), cus, spps, (0, 512, 768, 1024))
    gridk = itertools.product((3, 5), (_lib.CSPN_F16, _lib.CSPN_F32), Bs, _PLAN_SHAPES, Ts, (0, 1), cus, spps, (0, 512, 768))
    cases = [("cspn3", B, H, W, T, bl, cu, spp, th) for B, (H, W), T, bl, cu, spp, th in itertools.islice(grid3, 0, None, 23)]
    cases += [("cspnk", K, gdt, B, H, W, T, bl, cu, spp, th) for K, gdt, B, (H, W), T, bl, cu, spp, th in itertools.islice(gridk, 0, None, 71)]
    # the production shapes and the requests the thinning is most likely to miss: each workgroup size at the BASELINE configs
    for B, H, W in ((24, 228, 304), (3, 228, 304), (1, 352, 1216), (8, 352, 1216)):
        cases += [("cspn3", B, H, W, 24, bl, 256, 0, th) for bl in (0, 1) for th in (0, 512, 768, 1024)]
        cases += [("cspnk", K, gdt, B, H, W, 12, bl, 256, 0, th) for K in (3, 5) for gdt in (_lib.CSPN_F16, _lib.CSPN_F32)
                  for bl in (0, 1) for th in (0, 512, 768)]
    return list(dict.fromkeys(cases))


def _resident_plan_of(case):
    from cspn_monodepth_amd import functional as F
    if case[0] == "cspn3":
        _, B, H, W, T, bl, cu, spp, th = case
        p = F.resident_plan(B, H, W, T, bl, cu, steps_per_phase=spp, threads=th)
    else:
        _, K, gdt, B, H, W, T, bl, cu, spp, th = case
        p = F.kres_plan(K, B, H, W, T, bl, cu, steps_per_phase=spp, threads=th, g_dtype=gdt)
    return None if p is None else [p[name] for name in _PLAN_FIELDS]


def make_resident_plan_table():
    """Writes tests/golden/g20_resident_plans.json from the library in the tree.  Run once, at the commit whose plans are the
    reference (`python -c "import test_abi_and_host as t; t.make_resident_plan_table()"` from tests/)."""
    import json
    rows = [list(case) + [_resident_plan_of(case)] for case in _resident_plan_cases()]
    with open(_PLAN_TABLE, "w") as fh:
        fh.write(json.dumps({"fields": list(_PLAN_FIELDS), "rows": rows}, separators=(",", ":")).replace("],[", "],\n["))
        fh.write("\n")


def test_resident_plans_match_the_recorded_table():
    """cspn3_resident_plan / cspnk_resident_plan (pure host code with n_cu > 0) return, field for field, the plans recorded in
    tests/golden/g20_resident_plans.json — or no plan where none was recorded — over a grid that reaches every branch of both
    searches: one- and multi-launch batches, one and several phases, odd requests, the 512 / 768 (clipped) / 1024-thread 3x3
    instances, both K, both guidance dtypes, widths that are no multiple of 4 / 8.  The table was written by
    make_resident_plan_table() before the geometry code was restructured."""
    import json
    import numpy as np
    table = json.load(open(_PLAN_TABLE))
    assert tuple(table["fields"]) == _PLAN_FIELDS
    rows = {tuple(r[:-1]): r[-1] for r in table["rows"]}
    cases = _resident_plan_cases()
    assert set(rows) == set(cases) and len(rows) == len(table["rows"])
    fi = _PLAN_FIELDS.index("region_over_tile")
    n_plans = 0
    for case in cases:
        want, got = rows[case], _resident_plan_of(case)
        assert (want is None) == (got is None), (case, want, got)
        if want is None:
            continue
        n_plans += 1
        assert np.float32(got[fi]) == np.float32(want[fi]), (case, got[fi], want[fi])
        assert got[:fi] + got[fi + 1:] == want[:fi] + want[fi + 1:], (case, dict(zip(_PLAN_FIELDS, got)), dict(zip(_PLAN_FIELDS, want)))
    assert n_plans > len(cases) // 4                     # the grid is not mostly refusals


def test_resident_entry_points_reject_bad_arguments_without_a_gpu():
    """Every validation rule of the six weight-resident entry points that precedes the device query: the call returns 0 and
    cspn_last_error() names the entry point and the rule.  The pointers (value 16, or 8 for a misaligned one) are never
    dereferenced.  The rules that the three 3x3 entries share are checked by their common launcher, whose messages carry the
    name cspn3_forward_resident.  Where there is no device, one fully valid call per entry point shows that validation lets it
    through: it fails at the device query ("no device").  (With a device that call would launch on the made-up pointers, so it
    is only made without one.)"""
    L = _lib.lib()
    F16, F32 = _lib.CSPN_F16, _lib.CSPN_F32
    p, odd = 16, 8
    B, H, W, T = 2, 8, 16, 4
    no_device = not torch.cuda.is_available()

    def run(entry, order, valid, rules, prefix=None):
        fn = getattr(L, entry)
        for change, rule, *who in rules:
            args = dict(valid, **change)
            assert fn(*[args[k] for k in order]) == 0, (entry, change)
            msg = L.cspn_last_error().decode()
            assert rule in msg and msg.startswith((who[0] if who else prefix or entry) + ":"), (entry, change, msg)
        if no_device:
            assert fn(*[valid[k] for k in order]) == 0
            msg = L.cspn_last_error().decode()
            assert "no device" in msg and msg.startswith((prefix or entry) + ":"), (entry, msg)

    shape = dict(B=B, H=H, W=W, T=T)
    seqs = [(dict(seq=0), "seq must be in [1, 2^31 - 256]"), (dict(seq=0x7fffff01), "seq must be in [1, 2^31 - 256]")]
    q = "cspn3_forward_resident"                                     # the launcher the three 3x3 entries share

    order = "g bs cs d0 sparse out hist w8 s_out work seq host_err B H W Wv T blend target acc nslots plan stream".split()
    valid = dict(shape, g=p, bs=8 * H * W, cs=H * W, d0=p, sparse=None, out=p, hist=None, w8=None, s_out=None, work=p, seq=256, host_err=None,
                 Wv=0, blend=0, target=None, acc=None, nslots=0, plan=None, stream=None)
    run("cspn3_forward_resident", order, valid, [
        (dict(g=None), "bad arguments"), (dict(B=0), "bad arguments"), (dict(H=-1), "bad arguments"), (dict(T=0), "bad arguments"),
        (dict(out=None), "bad arguments"), (dict(blend=2), "blend 2"), (dict(blend=1), "blend needs sparse"),
        (dict(target=p), "scoring needs target"), (dict(acc=p, nslots=1), "scoring needs target"),
        (dict(target=p, acc=p, nslots=0), "scoring needs target"), (dict(d0=odd), "16-byte aligned"), (dict(work=odd), "16-byte aligned"),
        (dict(sparse=odd, blend=1), "16-byte aligned"), (dict(target=odd, acc=p, nslots=1), "16-byte aligned"),
        (dict(W=30, cs=H * 30, bs=8 * H * 30), "multiples of 4"), (dict(cs=H * W + 2), "multiples of 4"),
        (dict(s_out=p), "outputs of the training form"), (dict(hist=p, out=None), "the training form (history) needs s_out"),
        (dict(hist=odd, s_out=p, out=None), "16-byte aligned"), (dict(Wv=W + 1), "W_valid")] + seqs)

    order = "w8 g_T sparse hist work seq host_err B H W Wv T premask plan stream".split()
    valid = dict(shape, w8=p, g_T=p, sparse=None, hist=p, work=p, seq=256, host_err=None, Wv=0, premask=0, plan=None, stream=None)
    run("cspn3_transposed_resident", order, valid, [
        (dict(w8=None), "bad arguments", "cspn3_transposed_resident"), (dict(hist=None), "bad arguments", "cspn3_transposed_resident"),
        (dict(B=0), "bad arguments"), (dict(work=None), "bad arguments"),
        (dict(premask=1), "premask needs sparse", "cspn3_transposed_resident"),
        (dict(hist=odd), "history must be 16-byte aligned", "cspn3_transposed_resident"),
        (dict(g_T=odd), "16-byte aligned"), (dict(sparse=odd, premask=1), "16-byte aligned"), (dict(W=30), "multiples of 4")] + seqs, prefix=q)

    order = "g bs cs S g_T sparse hist work seq host_err B H W Wv T premask plan stream".split()
    valid = dict(shape, g=p, bs=8 * H * W, cs=H * W, S=p, g_T=p, sparse=None, hist=p, work=p, seq=256, host_err=None, Wv=0, premask=0,
                 plan=None, stream=None)
    e = "cspn3_transposed_resident_guidance"
    run(e, order, valid, [
        (dict(g=None), "bad arguments", e), (dict(S=None), "bad arguments", e), (dict(H=0), "bad arguments"),
        (dict(premask=1), "premask needs sparse", e), (dict(S=odd), "S must be 16-byte aligned", e),
        (dict(hist=odd), "history must be 16-byte aligned", "cspn3_transposed_resident"), (dict(g=odd), "16-byte aligned"),
        (dict(W=30, cs=H * 30, bs=8 * H * 30), "multiples of 4"), (dict(bs=8 * H * W + 1), "multiples of 4")] + seqs, prefix=q)

    order = "g g_dtype K x0 sparse out sdt work seq host_err B H W T blend target acc nslots plan stream".split()
    valid = dict(shape, g=p, g_dtype=F16, K=5, x0=p, sparse=None, out=p, sdt=F16, work=p, seq=256, host_err=None, blend=0, target=None, acc=None,
                 nslots=0, plan=None, stream=None)
    run("cspnk_forward_resident", order, valid, [
        (dict(g=None), "bad arguments"), (dict(out=None), "bad arguments"), (dict(B=0), "bad arguments"), (dict(T=0), "bad arguments"),
        (dict(K=4), "K=4 (3 or 5)"), (dict(K=7), "K=7 (3 or 5)"), (dict(sdt=2), "state dtype 2"), (dict(g_dtype=2), "guidance dtype 2"),
        (dict(g_dtype=F32), "fp32 guidance runs with fp32 depth planes"), (dict(blend=2), "blend 2"), (dict(blend=1), "blend needs sparse"),
        (dict(target=p), "scoring needs target"), (dict(acc=p, nslots=1), "scoring needs target"), (dict(W=12), "multiple of 8"),
        (dict(x0=odd), "16-byte aligned"), (dict(target=odd, acc=p, nslots=1), "16-byte aligned"), (dict(sparse=odd, blend=1), "16-byte aligned")] + seqs)
    if no_device:                                   # K = 3 with fp32 guidance runs on the quad kernel: its launcher answers
        args = dict(valid, K=3, g_dtype=F32, sdt=F32)
        assert L.cspnk_forward_resident(*[args[k] for k in order]) == 0 and L.cspn_last_error().decode().endswith("no device")

    order = "wk w_dtype K g_T sparse in_dtype g32 hist work seq host_err B H W T premask plan stream".split()
    valid = dict(shape, wk=p, w_dtype=F16, K=5, g_T=p, sparse=None, in_dtype=F32, g32=None, hist=p, work=p, seq=256, host_err=None, premask=0,
                 plan=None, stream=None)
    run("cspnk_transposed_resident", order, valid, [
        (dict(wk=None), "bad arguments"), (dict(hist=None), "bad arguments"), (dict(W=0), "bad arguments"),
        (dict(K=3), "K = 5 with an fp16 tap volume"), (dict(w_dtype=F32), "K = 5 with an fp16 tap volume"),
        (dict(premask=1), "premask needs sparse"), (dict(in_dtype=2), "bad in_dtype 2"),
        (dict(g32=p), "g_T_f32_out goes with fp16 inputs"), (dict(g32=odd, in_dtype=F16), "g_T_f32_out goes with fp16 inputs"),
        (dict(W=12), "multiple of 8"), (dict(g_T=odd), "16-byte aligned"), (dict(hist=odd), "16-byte aligned")] + seqs)

    order = "g g_dtype K x0 sparse hist wk_out work seq host_err B H W T blend plan stream".split()
    valid = dict(shape, g=p, g_dtype=F16, K=5, x0=p, sparse=None, hist=p, wk_out=p, work=p, seq=256, host_err=None, blend=0, plan=None, stream=None)
    run("cspnk_forward_resident_history", order, valid, [
        (dict(g=None), "bad arguments"), (dict(wk_out=None), "bad arguments"), (dict(B=-2), "bad arguments"),
        (dict(K=4), "the training form exists for K = 3 with fp32 guidance and for K = 5 with fp16"),
        (dict(g_dtype=F32), "the training form exists for K = 3 with fp32 guidance and for K = 5 with fp16"),
        (dict(blend=2), "blend 2"), (dict(blend=1), "blend needs sparse"), (dict(W=12), "multiple of 8"),
        (dict(hist=odd), "16-byte aligned"), (dict(wk_out=odd), "16-byte aligned")] + seqs)
    if no_device:
        args = dict(valid, K=3, g_dtype=F32)
        assert L.cspnk_forward_resident_history(*[args[k] for k in order]) == 0 and L.cspn_last_error().decode().endswith("no device")


def test_journal_entries_demote_to_weak_references():
    """Host logic of the resident launches' journal (no GPU needed): an old entry holds its tensors weakly — through the tensor
    that owns the storage, so that a view made inside the package can be rebuilt — and reports a dropped output as "nothing to
    repair" and dropped inputs as "cannot be repaired"; version counters tell an in-place overwrite."""
    import gc
    from cspn_monodepth_amd import functional as F
    g = torch.arange(2 * 12 * 4 * 8, dtype=torch.float32).reshape(2, 12, 4, 8)
    d = torch.ones(2, 1, 4, 8)
    d0 = d[:, 0]                                       # a view, as functional._plane makes it
    out = torch.zeros(2, 4, 8)
    e = F._JournalEntry(lambda *a: None, out, (g, d0, None, None), "test")
    assert e.nbytes == (g.numel() + d0.numel() + out.numel()) * 4 and not e.weak
    e.demote()
    assert e.weak
    del d0
    gc.collect()
    o2, ins = e.resolve()
    assert o2.data_ptr() == out.data_ptr() and ins[0].data_ptr() == g.data_ptr()
    assert ins[1].data_ptr() == d.data_ptr() and tuple(ins[1].shape) == (2, 4, 8) and ins[2] is None      # the view, rebuilt from its base
    assert e.untouched(ins)
    g.add_(1.0)
    assert not e.untouched(e.resolve()[1])            # an in-place overwrite shows in the version counter
    del out, o2
    gc.collect()
    assert e.resolve()[0] is None                     # the result was dropped: nobody can read it
    del g, ins
    gc.collect()
    assert e.resolve()[1] is None                     # an input is gone: the call cannot be re-run


def test_journal_entries_accept_inference_tensors_and_training_entries_pin_nothing():
    """ADVICE r5.  (1) Tensors made under torch.inference_mode() have no version counter (reading it raises): a journal entry
    built from them — every unguarded launch builds one, the default scored forward among them — records "cannot verify" instead
    of crashing after the kernel was enqueued, and the repair trusts such inputs.  (2) A training-form entry (redo None) keeps no
    inputs and holds the plane a failed tile poisons weakly from the start."""
    import gc
    from cspn_monodepth_amd import functional as F
    with torch.inference_mode():
        g = torch.ones(2, 12, 4, 8)
        d0 = torch.ones(2, 4, 8)
        out = torch.zeros(2, 4, 8)
        assert g.is_inference()
        e = F._JournalEntry(lambda *a: None, out, (g, d0, None, None), "test")
        assert e.versions[0] is F._NO_VERSION and e.versions[2] is None
        assert e.untouched(e.inputs)
        e.demote()
        o2, ins = e.resolve()
        assert o2.data_ptr() == out.data_ptr() and e.untouched(ins)
    # mixed: an ordinary tensor next to an inference one is still checked
    h = torch.ones(2, 4, 8)
    e2 = F._JournalEntry(lambda *a: None, torch.zeros(1), (g, h), "test")
    h.add_(1.0)
    assert not e2.untouched(e2.inputs)
    # training form: no inputs, weak output, nothing pinned
    hist = torch.zeros(3, 2, 4, 8)
    e3 = F._JournalEntry(None, hist[2], (g, h), "training")
    assert e3.inputs == () and e3.weak and e3.nbytes == 0
    assert e3.out.get().data_ptr() == hist[2].data_ptr()
    del hist
    gc.collect()
    assert e3.out.get() is None


def test_guard_rule_truth_table(monkeypatch):
    """functional._guard_default is the one place that says which resident calls carry the device-side guard when the caller does
    not: the switch is on, the halo of the re-computation (T for the 3x3 entries, T * (K // 2) for the K x K ones) fits
    _GUARD_MAX_T = 54, and the scored policy allows it — every call site's decision, row by row."""
    from cspn_monodepth_amd import functional as F
    assert F._GUARD_MAX_T == 54
    for switch in (False, True, "all"):
        monkeypatch.setattr(F, "_RESIDENT_GUARD", switch)
        on = int(bool(switch))
        # transposed_resident(_guidance), the unscored forward_resident: h = T
        assert [F._guard_default(T) for T in (1, 24, 54, 55)] == [on, on, on, 0]
        # pac_transposed_resident, the K = 5 forms of pac_forward_resident(_history): h = T * (5 // 2)
        assert [F._guard_default(T * (5 // 2)) for T in (1, 24, 27, 28)] == [on, on, on, 0]
        # K = 3 K x K: h = T * (3 // 2)
        assert [F._guard_default(T * (3 // 2)) for T in (24, 54, 55)] == [on, on, 0]
        # the scored 3x3 forward (forward_resident with score=, _ScoredFast): only under "all"
        assert [F._guard_default(T, "scored") for T in (24, 54, 55)] == [int(switch == "all"), int(switch == "all"), 0]
        # the scored K x K forward: never; so a history form without a guard kernel
        assert [F._guard_default(T * (K // 2), "never") for K in (3, 5) for T in (1, 24, 27, 28, 54, 55)] == [0] * 12
    # the history form takes "plain" for exactly these (K, guidance dtype), "never" for every other
    assert F._GUARDED_HISTORY_FORMS == {(3, torch.float32), (5, torch.float16)}
    assert (3, torch.float16) not in F._GUARDED_HISTORY_FORMS and (5, torch.float32) not in F._GUARDED_HISTORY_FORMS


def test_journal_demotion_passes_over_training_entries(monkeypatch):
    """a training-form entry (redo None: weak from birth) between strong inference entries must not end the
    newest-first demotion walk — the entries older than it would stay pinned past _JOURNAL_STRONG_BYTES.  Oldest to newest:
    inference, inference, training, inference, inference; three inference entries exceed the budget, so the two oldest are
    demoted and the newest two stay strong (the "at least the last two" rule).  The same list without the training entry
    gives the same answer for the inference entries."""
    from cspn_monodepth_amd import functional as F

    def inference():
        out, g = torch.zeros(2, 4, 8), torch.ones(2, 12, 4, 8)
        return F._JournalEntry(lambda *a: None, out, (g, None), "test")

    one = inference().nbytes
    assert one == (2 * 4 * 8 + 2 * 12 * 4 * 8) * 4
    monkeypatch.setattr(F, "_JOURNAL_STRONG_BYTES", 2 * one + one // 2)       # two entries fit, three do not
    hist = torch.zeros(3, 2, 4, 8)
    for with_training in (True, False):
        inf = [inference() for _ in range(4)]
        j = inf[:2] + ([F._JournalEntry(None, hist[2], (), "training")] if with_training else []) + inf[2:]
        assert sum(e.nbytes for e in j[:2]) + j[-1].nbytes > F._JOURNAL_STRONG_BYTES
        F._journal_demote(j)
        assert [e.weak for e in inf] == [True, True, False, False], with_training
        assert inf[0].resolve()[0] is None and inf[3].resolve()[0] is not None      # demoted: nothing kept alive; strong: held
        F._journal_demote(j)                                                      # a second walk changes nothing
        assert [e.weak for e in inf] == [True, True, False, False]


def test_device_state_has_every_key_from_the_start(monkeypatch):
    """The per-device state of the resident launches is created whole (functional._new_state, the device-free part of
    _resident_state): no host-side function that can run without a device adds a key to it, whichever runs first."""
    from cspn_monodepth_amd import functional as F
    st = F._new_state(torch.zeros(4, dtype=torch.int32), 256)
    keys = set(st)
    assert keys >= {"seq", "host_err_np", "dirty", "journal", "last_seq", "work", "marks", "mark_pool", "jcount", "guarded_pending",
                    "need_bwd_check", "last_raw", "last_stream", "last_reports", "lost", "lock", "n_cu"}
    assert st["seq"] == F._RES_SEQ_STEP and not st["dirty"] and st["guarded_pending"] == 0 and st["last_raw"] is None
    monkeypatch.setattr(F, "_RES", {0: st})
    dev = torch.device("cuda", 0)
    out, g = torch.zeros(2, 4, 8), torch.ones(2, 12, 4, 8)
    for k in range(15):                                    # (the 16th add records a HIP event: that needs a device)
        F._journal_add(dev, st, F._JournalEntry(lambda *a: None, out, (g,), "test") if k % 2 else F._JournalEntry(None, out), None)
        assert set(st) == keys
    assert len(st["journal"]) == 15 and st["jcount"] == 15
    assert F._resident_state(dev) is st
    F.check_resident_errors()
    F.check_resident_errors(dev)
    cp = F._ResidentCheckpoint(dev)
    cp.wait_and_check()
    assert set(st) == keys and len(st["journal"]) == 15   # nothing reports completion: the checkpoint clears nothing
    st["guarded_pending"] = 3
    F.ensure_resident_ok()                                 # nothing is pending on a stream: everything issued has finished cleanly
    assert set(st) == keys and not st["journal"] and st["guarded_pending"] == 0
    F._journal_clear(st)
    assert set(st) == keys


def test_bench_cpu_binding_narrows_and_restores_the_affinity_mask():
    """bench.py --cpu-bind auto: a rank's host threads go to its share of the first allowed cores; the CPU baseline leg gets the
    whole mask back (full_affinity), and the reported host budget is the original one."""
    import importlib.util
    import os
    if not hasattr(os, "sched_getaffinity"):
        pytest.skip("no sched_getaffinity on this platform")
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    before = os.sched_getaffinity(0)
    try:
        assert bench.bind_cpus(0, 1, "off") is None and os.sched_getaffinity(0) == before
        mine = bench.bind_cpus(1, 2, "auto")
        if len(before) >= 4:
            k = 4 if len(before) >= 8 else len(before) // 2
            assert mine == sorted(before)[k:2 * k] and os.sched_getaffinity(0) == set(mine)
            assert bench.host_cpu_budget()["sched_affinity"] == len(before)
            with bench.full_affinity():
                assert os.sched_getaffinity(0) == before
            assert os.sched_getaffinity(0) == set(mine)
    finally:
        os.sched_setaffinity(0, before)


def test_bench_dump_outputs_writes_float_arrays_and_samples_past_the_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: float64 stays float64, other dtypes become float32; past the byte budget every array is cut to
    its share of elements at seeded flat indices, the same in every call."""
    import importlib.util
    import os
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = torch.arange(24, dtype=torch.float16).reshape(2, 3, 4)
    b = torch.linspace(0, 1, 10, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "whole"), {"a": a, "b": b})
    ga, gb = np.load(str(tmp_path / "whole" / "a.npy")), np.load(str(tmp_path / "whole" / "b.npy"))
    assert ga.dtype == np.float32 and ga.shape == (2, 3, 4) and np.array_equal(ga, a.float().numpy())
    assert gb.dtype == np.float64 and np.array_equal(gb, b.numpy())
    big = torch.arange(100000, dtype=torch.float32)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40000)
    for run in ("one", "two"):
        bench.dump_outputs(str(tmp_path / run), {"big": big})
    s1, s2 = np.load(str(tmp_path / "one" / "big.npy")), np.load(str(tmp_path / "two" / "big.npy"))
    assert s1.dtype == np.float32 and 0 < s1.nbytes <= 40000 and np.array_equal(s1, s2)
    assert np.all(np.diff(s1) > 0) and np.isin(s1, big.numpy()).all()


@pytest.mark.gpu
def test_a_device_without_an_index_is_the_current_device():
    """The launch helpers read `dev.index`; a caller's torch.device("cuda") has none.  The entries that take a device from the
    caller — the frame meter, the drawn transform parameters — and tensors made on "cuda" give what "cuda:0" gives."""
    from cspn_monodepth_amd import evaluation as ev
    from cspn_monodepth_amd import utils
    from cspn_monodepth_amd.dataloaders.nyu_dataloader import draw_train_params
    g = torch.Generator().manual_seed(5)
    target = torch.rand(2, 1, 3, 5, generator=g) + 0.5
    pred = target + 0.1 * torch.rand(2, 1, 3, 5, generator=g)
    depth = torch.tensor([[[[0.5, 1.0, 2.0]]]])                      # 1 x 1 x 1 x 3
    rgb = torch.arange(9, dtype=torch.uint8).reshape(1, 3, 1, 3)
    got = []
    for dev in (torch.device("cuda"), torch.device("cuda:0")):
        assert torch.cuda.current_device() == 0
        meter = ev.FrameAverageMeter(dev).update(pred.to(dev), target.to(dev))
        got.append((meter.state().cpu(), utils.colored_depthmap(depth[0, 0].to(dev)).cpu(),
                    utils.comparison_rows(rgb.to(dev), depth.to(dev), (2 * depth).to(dev), "rgb").cpu(),
                    draw_train_params(2, seed=7, device=dev).cpu()))
    assert got[0][0][10] == 2 and got[0][1].shape == (1, 3, 3) and got[0][2].shape == (1, 1, 9, 3) and got[0][3].shape == (2, 8)
    for a, b in zip(*got):
        assert torch.equal(a, b)

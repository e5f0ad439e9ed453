"""Loader / builder of libcspn_hip.so (the C-ABI HIP engine, include/cspn_hip.h).

The reference loaded its native code through torch.utils.ffi (network/libs/inplace_abn/build.py:3-21,
_ext/__init__.py:2-13 — removed from PyTorch 1.0); here it is a plain ``ctypes.CDLL``.
There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised
(the reference's ``_check`` does the same, inplace_abn/functions.py:13-16).
"""
import ctypes
import os
import shutil
import subprocess
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
SO_PATH = os.environ.get("CSPN_HIP_LIB") or os.path.join(_PKG, "libcspn_hip.so")   # env override: A/B builds
CSRC = os.path.join(_PKG, "csrc")
SOURCES = ("cspn_propagate.hip", "cspn_resident.hip", "cspnk_resident.hip", "cspnk_d2.hip", "cspn_prepare.hip", "cspn_backward.hip", "cspn_metrics.hip", "cspn_metrics_frame.hip", "cspn_debug.hip", "cspn_repair.hip", "pac_conv2d.hip", "pac_conv2d_s2.hip", "cspn_unpool.hip", "cspn_criterion.hip", "cspn_max8.hip", "cspn_abn.hip", "cspn_sparsify.hip", "cspn_transform.hip", "cspn_losses.hip", "cspn_optim.hip", "cspn_visual.hip")   # one TU each
HEADERS = (os.path.join(CSRC, "cspn_common.hpp"), os.path.join(CSRC, "cspnk_helpers.hpp"), os.path.join(_ROOT, "include", "cspn_hip.h"))
INCLUDE = os.path.join(_ROOT, "include")
# include/cspn_criterion.h, include/cspn_max8.h, include/cspn_abn.h, include/cspn_sparsify.h, include/cspn_transform.h, include/cspn_losses.h,
# include/cspn_optim.h, include/cspn_visual.h, csrc/pac_launch.hpp, csrc/cspn_loss_units.hpp: part of the build's staleness hash, NOT of code_digest() — no benchmarked
# kernel sees it, and a digest that moved would mark the HBM traffic recorded under profiles/ as stale (bench.py `traffic_stale`)
BUILD_HEADERS = HEADERS + (os.path.join(INCLUDE, "cspn_criterion.h"), os.path.join(INCLUDE, "cspn_max8.h"), os.path.join(INCLUDE, "cspn_abn.h"),
                           os.path.join(INCLUDE, "cspn_sparsify.h"), os.path.join(INCLUDE, "cspn_transform.h"), os.path.join(CSRC, "pac_launch.hpp"),
                           os.path.join(INCLUDE, "cspn_losses.h"), os.path.join(CSRC, "cspn_loss_units.hpp"), os.path.join(INCLUDE, "cspn_optim.h"),
                           os.path.join(INCLUDE, "cspn_visual.h"))

CSPN_F32, CSPN_F16 = 0, 1
ABI_VERSION = 10         # CSPN_ABI_VERSION of include/cspn_hip.h this host code was written against
CRITERION_ABI_VERSION = 1   # CSPN_CRITERION_ABI_VERSION of include/cspn_criterion.h
MAX8_ABI_VERSION = 1        # CSPN_MAX8_ABI_VERSION of include/cspn_max8.h
MAX8_MAX_STEPS_PER_LAUNCH = 16
ABN_ABI_VERSION = 1         # CSPN_ABN_ABI_VERSION of include/cspn_abn.h
ABN_ACT_LEAKY_RELU, ABN_ACT_ELU, ABN_ACT_NONE = 0, 1, 2
ABN_SMALL, ABN_SPLIT = 0, 1                                 # cspn_abn_plan_t.regime
ABN_FULL, ABN_STATS_ONLY, ABN_APPLY_ONLY = 0, 1, 2          # the `phase` of a training-mode cspn_abn_forward
SPARSIFY_ABI_VERSION = 1    # CSPN_SPARSIFY_ABI_VERSION of include/cspn_sparsify.h
SPARSIFY_UAR, SPARSIFY_DENSE = 0, 1                         # cspn_sparsify's `mode`
UNIFORM_PHILOX, UNIFORM_F32, UNIFORM_F64 = 0, 1, 2          # ... `uniform_kind`
RGB_NONE, RGB_F32, RGB_U8 = 0, 1, 2                         # ... `rgb_kind`
SPARSIFY_SLICE_PIXELS, SPARSIFY_MAX_SLICES = 1024, 64
TRANSFORM_ABI_VERSION = 1   # CSPN_TRANSFORM_ABI_VERSION of include/cspn_transform.h
TRANSFORM_VAL, TRANSFORM_TRAIN = 0, 1                       # cspn_transform's `mode`
TRANSFORM_PARAMS, TRANSFORM_GATHER_PIXELS, TRANSFORM_MAX_SECOND = 8, 256, 32768
LOSS_L1, LOSS_L2, LOSS_L1_LOG = 0, 1, 2
LOSSES_ABI_VERSION = 1      # CSPN_LOSSES_ABI_VERSION of include/cspn_losses.h
MEAN_L1, MEAN_GRAD, MEAN_RMSE, MEAN_RMSE_LOG = 0, 1, 2, 3   # the `kind` of cspn_mean_loss_*
LOSSES_STATE_BYTES = 48
OPTIM_ABI_VERSION = 1       # CSPN_OPTIM_ABI_VERSION of include/cspn_optim.h
SGD_CHUNK, SGD_TENSORS_PER_LAUNCH, SGD_MAX_WORKGROUPS = 4096, 109, 2048
VISUAL_ABI_VERSION = 1      # CSPN_VISUAL_ABI_VERSION of include/cspn_visual.h
VISUAL_RANGE_CHUNK, VISUAL_MAX_PLANES = 4096, 3
VISUAL_RGB_NONE, VISUAL_RGB_F32, VISUAL_RGB_U8 = 0, 1, 2      # cspn_visual_rows_t.rgb_kind
BLEND_NONE, BLEND_SPARSE, BLEND_PREMASK = 0, 1, 2

# every symbol include/cspn_hip.h declares (tests check the .so exports all of them)
EXPORTS = (
    "cspn_abi_version", "cspn_last_error", "cspn_plan_resolve", "cspn3_prepare", "cspn_pac_prepare",
    "cspn_propagate_workspace_bytes", "cspn_propagate", "cspn_propagate_scored", "cspn_propagate_transposed", "cspn3_propagate_from_guidance",
    "cspn_transpose_weights", "cspn3_resident_plan", "cspn3_resident_workspace_bytes", "cspn3_forward_resident", "cspn3_transposed_resident", "cspn3_transposed_resident_guidance",
    "cspnk_resident_plan", "cspnk_resident_workspace_bytes", "cspnk_forward_resident", "cspnk_forward_resident_history", "cspnk_transposed_resident",
    "cspn_grad_weights", "cspn3_grad_guidance", "cspn_pac_grad_guided", "cspn3_backward_tail",
    "cspn_pac_backward_tail", "cspn_metrics_accumulate", "cspn_metrics_per_frame_workspace_bytes", "cspn_metrics_per_frame", "cspn_meter_update",
    "cspn_pac_out_size", "cspn_pac_force_generic", "cspn_pac_conv2d", "cspn_pac_conv2d_grad_input", "cspn_pac_conv2d_grad_kernel", "cspn_pac_nd2col", "cspn_unpool2d", "cspn_unpool2d_backward", "cspn_debug_set_lds_poison",
)
# every symbol include/cspn_criterion.h declares
CRITERION_EXPORTS = ("cspn_criterion_abi_version", "cspn_criterion_workspace_bytes", "cspn_criterion_forward", "cspn_criterion_backward")
# every symbol include/cspn_max8.h declares
MAX8_EXPORTS = ("cspn_max8_abi_version", "cspn_max8_workspace_bytes", "cspn_max8_forward", "cspn_max8_backward")
# every symbol include/cspn_abn.h declares
ABN_EXPORTS = ("cspn_abn_abi_version", "cspn_abn_plan", "cspn_abn_workspace_bytes", "cspn_abn_forward", "cspn_abn_backward_reduce",
               "cspn_abn_backward")
# every symbol include/cspn_sparsify.h declares
SPARSIFY_EXPORTS = ("cspn_sparsify_abi_version", "cspn_sparsify_slices", "cspn_sparsify_workspace_bytes", "cspn_sparsify")
# every symbol include/cspn_transform.h declares
TRANSFORM_EXPORTS = ("cspn_transform_abi_version", "cspn_transform_first_size", "cspn_transform_workspace_bytes", "cspn_transform",
                     "cspn_transform_draw_params")
# every symbol include/cspn_losses.h declares
LOSSES_EXPORTS = ("cspn_losses_abi_version", "cspn_losses_workspace_bytes", "cspn_berhu_forward", "cspn_berhu_backward",
                  "cspn_mean_loss_forward", "cspn_mean_loss_backward")
# every symbol include/cspn_optim.h declares
OPTIM_EXPORTS = ("cspn_optim_abi_version", "cspn_sgd_plan", "cspn_sgd_step")
# every symbol include/cspn_visual.h declares
VISUAL_EXPORTS = ("cspn_visual_abi_version", "cspn_visual_workspace_bytes", "cspn_visual_rows", "cspn_visual_features")


class cspn_plan(ctypes.Structure):
    _fields_ = [("steps_per_launch", ctypes.c_int), ("tile_w", ctypes.c_int), ("tile_h", ctypes.c_int),
                ("quads_per_thread", ctypes.c_int), ("threads", ctypes.c_int), ("force_scalar", ctypes.c_int)]


class cspn_resident_plan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("steps_per_phase", "tiles_x", "tiles_y", "tile_w", "tile_h", "quads_per_thread",
                                            "threads", "images_per_launch", "launches", "lds_bytes", "n_cu")] + \
               [("region_over_tile", ctypes.c_float), ("spin_limit", ctypes.c_uint), ("debug_stamps", ctypes.c_void_p),
                ("step_form", ctypes.c_int), ("guard", ctypes.c_int)]


STEP_AUTO, STEP_FMA, STEP_DOT2 = 0, 1, 2       # cspn_resident_plan.step_form (include/cspn_hip.h)


class cspn_conv_geometry(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "oph", "opw", "transposed")]


class cspn_abn_plan(ctypes.Structure):           # cspn_abn_plan_t (include/cspn_abn.h)
    _fields_ = [(n, ctypes.c_int) for n in ("regime", "channels_per_workgroup", "workgroups_per_channel", "threads")] + \
               [("elements_per_workgroup", ctypes.c_size_t), ("small_limit", ctypes.c_size_t)]


class cspn_sgd_tensor(ctypes.Structure):         # cspn_sgd_tensor_t (include/cspn_optim.h)
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("momentum_buffer", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("first", ctypes.c_int)]


class cspn_sgd_hyper(ctypes.Structure):          # cspn_sgd_hyper_t (include/cspn_optim.h)
    _fields_ = [("lr", ctypes.c_double), ("lr_device", ctypes.c_void_p), ("momentum", ctypes.c_double), ("dampening", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("nesterov", ctypes.c_int), ("maximize", ctypes.c_int)]


class cspn_visual_rows(ctypes.Structure):       # cspn_visual_rows_t (include/cspn_visual.h)
    _fields_ = [("rgb", ctypes.c_void_p), ("rgb_kind", ctypes.c_int), ("rgb_scale", ctypes.c_float), ("rgb_frame_stride", ctypes.c_long),
                ("rgb_channel_stride", ctypes.c_long), ("depth", ctypes.c_void_p * 3), ("depth_frame_stride", ctypes.c_long * 3),
                ("n_depth", ctypes.c_int), ("use_min", ctypes.c_int), ("use_max", ctypes.c_int), ("d_min", ctypes.c_float),
                ("d_max", ctypes.c_float)]


BENCH_UNRELATED = ("pac_conv2d.hip", "pac_conv2d_s2.hip", "cspn_unpool.hip", "cspn_metrics_frame.hip", "cspn_criterion.hip", "cspn_max8.hip",
                   "cspn_abn.hip", "cspn_sparsify.hip", "cspn_transform.hip", "cspn_losses.hip", "cspn_optim.hip", "cspn_visual.hip")       # kernels no bench.py workload launches


def _source_digest(flags, code_only=False):
    """Content hash of the kernel sources (+ flags).  code_only: the hash profiles/ pins measured HBM traffic to (bench.py
    `traffic_stale`) — `//` comments and blank space are left out (a reworded comment must not invalidate a measurement),
    and so are the translation units of the widening rows, which no bench workload launches."""
    import hashlib
    import re
    h = hashlib.sha256(" ".join(flags).encode())
    for path in [os.path.join(CSRC, f) for f in SOURCES if not (code_only and f in BENCH_UNRELATED)] + list(HEADERS if code_only else BUILD_HEADERS):
        with open(path, "rb") as fh:
            data = fh.read()
        if code_only:
            data = re.sub(rb"/\*.*?\*/", b"", data, flags=re.S)
            lines = (re.sub(rb"//.*$", b"", ln).strip() for ln in data.splitlines())
            data = b"\n".join(re.sub(rb"\s+", b" ", ln) for ln in lines if ln)
        h.update(data)
    return h.hexdigest()


def code_digest():
    return _source_digest([], code_only=True)


def build(force=False, verbose=False):
    """hipcc cross-compiles for gfx950 without a GPU: the translation units are compiled in parallel to
    csrc/_build/*.o and linked into the in-tree .so (which travels with gpurun snapshots).  Staleness is decided by
    a content hash of the sources + flags stored next to the library (file times do not survive every copy)."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, f) for f in SOURCES]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # -fno-slp-vectorize: the SLP pass pairs the stencil FMAs into v_pk_fma_f32 and pays for it with ~50 v_mov
    # per step to build operand pairs; scalar v_fma_f32 measured 4 % faster (profiles/).  No fast-math: 0/0 = NaN.
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize"] + \
        os.environ.get("CSPN_HIPCC_FLAGS", "").split() + ["-I", INCLUDE]
    digest = _source_digest(flags[:-2])
    stamp = SO_PATH + ".hash"
    if not force and os.path.exists(SO_PATH) and os.path.exists(stamp) and open(stamp).read().strip() == digest:
        return SO_PATH
    bdir = os.path.join(CSRC, "_build")
    os.makedirs(bdir, exist_ok=True)

    import hashlib
    hdr = hashlib.sha256(" ".join(flags[:-2]).encode())
    for path in BUILD_HEADERS:
        with open(path, "rb") as fh:
            hdr.update(fh.read())

    def compile_one(src):
        # per-object staleness: flags + headers + this translation unit (an edit to one kernel recompiles one file)
        obj = os.path.join(bdir, os.path.basename(src)[:-4] + ".o")
        h = hdr.copy()
        with open(src, "rb") as fh:
            h.update(fh.read())
        want = h.hexdigest()
        if not force and os.path.exists(obj) and os.path.exists(obj + ".hash") and open(obj + ".hash").read().strip() == want:
            return obj
        cmd = [hipcc] + flags + ["-c", "-o", obj, src]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        with open(obj + ".hash", "w") as fh:
            fh.write(want + "\n")
        return obj

    with ThreadPoolExecutor(max_workers=len(srcs)) as pool:
        objs = list(pool.map(compile_one, srcs))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO_PATH + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(SO_PATH + ".tmp", SO_PATH)
    with open(stamp, "w") as fh:
        fh.write(digest + "\n")
    return SO_PATH


_lib = None
_lock = threading.Lock()


def _declare(lib):
    vp, ci, cl, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t
    lib.cspn_abi_version.restype = ci
    lib.cspn_last_error.restype = ctypes.c_char_p
    lib.cspn_plan_resolve.argtypes = [ci, ci, ci, ci, ci, ci, ctypes.POINTER(cspn_plan), ctypes.POINTER(cspn_plan)]
    lib.cspn3_prepare.argtypes = [vp, ci, cl, cl, ci, ci, ci, ci, vp, ci, vp, vp]
    lib.cspn_pac_prepare.argtypes = [vp, ci, ci, ci, ci, ci, vp, ci, vp]
    lib.cspn_propagate_workspace_bytes.argtypes = [ci, ci, ci, ci, ci, ci]
    lib.cspn_propagate_workspace_bytes.restype = cs
    lib.cspn_propagate.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci,
                                   ctypes.POINTER(cspn_plan), vp]
    lib.cspn_propagate_scored.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, ci,
                                          ctypes.POINTER(cspn_plan), vp]
    lib.cspn_propagate_transposed.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(cspn_plan), vp]
    lib.cspn3_propagate_from_guidance.argtypes = [vp, ci, cl, cl, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci,
                                                  vp, vp, ci,
                                                  ctypes.POINTER(cspn_plan), vp]
    lib.cspn3_resident_plan.argtypes = [ci, ci, ci, ci, ci, ci, ctypes.POINTER(cspn_resident_plan)]
    lib.cspn3_resident_workspace_bytes.argtypes = [ci, ci, ci]
    lib.cspn3_resident_workspace_bytes.restype = cs
    lib.cspn3_forward_resident.argtypes = [vp, cl, cl, vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint, vp, ci, ci, ci, ci, ci, ci, vp, vp, ci,
                                           ctypes.POINTER(cspn_resident_plan), vp]
    lib.cspn3_transposed_resident.argtypes = [vp, vp, vp, vp, vp, ctypes.c_uint, vp, ci, ci, ci, ci, ci, ci,
                                              ctypes.POINTER(cspn_resident_plan), vp]
    lib.cspn3_transposed_resident_guidance.argtypes = [vp, cl, cl, vp, vp, vp, vp, vp, ctypes.c_uint, vp, ci, ci, ci, ci, ci, ci,
                                                       ctypes.POINTER(cspn_resident_plan), vp]
    lib.cspnk_resident_plan.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci, ctypes.POINTER(cspn_resident_plan)]
    lib.cspnk_resident_workspace_bytes.argtypes = [ci, ci, ci, ci]
    lib.cspnk_resident_workspace_bytes.restype = cs
    lib.cspnk_forward_resident.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, ctypes.c_uint, vp, ci, ci, ci, ci, ci, vp, vp, ci,
                                           ctypes.POINTER(cspn_resident_plan), vp]
    lib.cspnk_forward_resident_history.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, ctypes.c_uint, vp, ci, ci, ci, ci, ci,
                                                   ctypes.POINTER(cspn_resident_plan), vp]
    lib.cspnk_transposed_resident.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp, ctypes.c_uint, vp, ci, ci, ci, ci, ci,
                                              ctypes.POINTER(cspn_resident_plan), vp]
    lib.cspn_transpose_weights.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp]
    lib.cspn_grad_weights.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.cspn3_grad_guidance.argtypes = [vp, ci, cl, cl, ci, vp, ci, vp, vp, vp, ci, ci, ci, vp]
    lib.cspn_pac_grad_guided.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.cspn3_backward_tail.argtypes = [vp, vp, vp, vp, vp, vp, cl, cl, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.cspn_pac_backward_tail.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    lib.cspn_metrics_accumulate.argtypes = [vp, vp, ci, cs, vp, ci, vp]
    lib.cspn_metrics_per_frame_workspace_bytes.argtypes = [ci, cs]
    lib.cspn_metrics_per_frame_workspace_bytes.restype = cs
    lib.cspn_metrics_per_frame.argtypes = [vp, vp, ci, ci, cs, vp, vp, vp]
    lib.cspn_meter_update.argtypes = [vp, ci, vp, vp]
    geom = ctypes.POINTER(cspn_conv_geometry)
    lib.cspn_pac_out_size.argtypes = [ci, ci, geom, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.cspn_pac_force_generic.argtypes = [ci, ctypes.POINTER(ci)]
    lib.cspn_pac_conv2d.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, geom, vp]
    lib.cspn_pac_conv2d_grad_input.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, geom, vp]
    lib.cspn_pac_conv2d_grad_kernel.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, geom, vp]
    lib.cspn_pac_nd2col.argtypes = [vp, vp, ci, ci, ci, ci, ci, geom, vp]
    lib.cspn_unpool2d.argtypes = [vp, vp, ci, cl, ci, ci, ci, ci, ci, vp]
    lib.cspn_unpool2d_backward.argtypes = [vp, vp, ci, cl, ci, ci, ci, ci, ci, vp]
    lib.cspn_debug_set_lds_poison.argtypes = [ci, ctypes.c_uint, ctypes.POINTER(ci)]
    lib.cspn_criterion_abi_version.restype = ci
    lib.cspn_criterion_workspace_bytes.argtypes = [cs]
    lib.cspn_criterion_workspace_bytes.restype = cs
    lib.cspn_criterion_forward.argtypes = [vp, vp, ci, ci, cs, vp, vp, vp]
    lib.cspn_criterion_forward.restype = ci
    lib.cspn_criterion_backward.argtypes = [vp, vp, ci, ci, cs, vp, vp, vp, vp]
    lib.cspn_criterion_backward.restype = ci
    lib.cspn_max8_abi_version.restype = ci
    lib.cspn_max8_workspace_bytes.argtypes = [ci, ci, ci, ci, ci]
    lib.cspn_max8_workspace_bytes.restype = cs
    lib.cspn_max8_forward.argtypes = [vp, cl, cl, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.cspn_max8_forward.restype = ci
    lib.cspn_max8_backward.argtypes = [vp, cl, cl, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.cspn_max8_backward.restype = ci
    cf = ctypes.c_float
    lib.cspn_abn_abi_version.restype = ci
    lib.cspn_abn_plan.argtypes = [ci, ci, ci, ctypes.POINTER(cspn_abn_plan)]
    lib.cspn_abn_plan.restype = ci
    lib.cspn_abn_workspace_bytes.argtypes = [ci, ci, ci]
    lib.cspn_abn_workspace_bytes.restype = cs
    lib.cspn_abn_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, ci, cf, vp, vp]
    lib.cspn_abn_forward.restype = ci
    lib.cspn_abn_backward_reduce.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, cf, ci, cf, vp, vp]
    lib.cspn_abn_backward_reduce.restype = ci
    lib.cspn_abn_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, ci, cf, vp, vp]
    lib.cspn_abn_backward.restype = ci
    ll, ull = ctypes.c_longlong, ctypes.c_ulonglong
    lib.cspn_sparsify_abi_version.restype = ci
    lib.cspn_sparsify_slices.argtypes = [cs]
    lib.cspn_sparsify_slices.restype = ci
    lib.cspn_sparsify_workspace_bytes.argtypes = [ci, cs]
    lib.cspn_sparsify_workspace_bytes.restype = cs
    lib.cspn_sparsify.argtypes = [vp, ci, ci, ci, ci, ci, ll, cf, vp, ci, vp, ull, vp, cl, vp, ci, vp, cl, cl, vp, vp, vp]
    lib.cspn_sparsify.restype = ci
    cd = ctypes.c_double
    lib.cspn_transform_abi_version.restype = ci
    lib.cspn_transform_first_size.argtypes = [ci, ci, cd, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.cspn_transform_first_size.restype = ci
    lib.cspn_transform_workspace_bytes.argtypes = [ci, ci, ci, ci, cd, ci, ci]
    lib.cspn_transform_workspace_bytes.restype = cs
    lib.cspn_transform.argtypes = [vp, vp, ci, ci, ci, cd, ci, ci, ci, vp, vp, cl, cl, vp, cl, vp, vp]
    lib.cspn_transform.restype = ci
    lib.cspn_transform_draw_params.argtypes = [vp, ci, ull, vp, vp]
    lib.cspn_transform_draw_params.restype = ci
    lib.cspn_losses_abi_version.restype = ci
    lib.cspn_losses_workspace_bytes.argtypes = [cs]
    lib.cspn_losses_workspace_bytes.restype = cs
    lib.cspn_berhu_forward.argtypes = [vp, vp, ci, cs, vp, vp, vp]
    lib.cspn_berhu_forward.restype = ci
    lib.cspn_berhu_backward.argtypes = [vp, vp, ci, cs, vp, vp, vp, vp]
    lib.cspn_berhu_backward.restype = ci
    lib.cspn_mean_loss_forward.argtypes = [vp, vp, ci, ci, cs, vp, vp, vp]
    lib.cspn_mean_loss_forward.restype = ci
    lib.cspn_mean_loss_backward.argtypes = [vp, vp, ci, ci, cs, vp, vp, vp, vp]
    lib.cspn_mean_loss_backward.restype = ci
    lib.cspn_optim_abi_version.restype = ci
    lib.cspn_sgd_plan.argtypes = [ctypes.POINTER(cs), ci, ci, ctypes.POINTER(ci), ctypes.POINTER(cs)]
    lib.cspn_sgd_plan.restype = ci
    lib.cspn_sgd_step.argtypes = [ctypes.POINTER(cspn_sgd_tensor), ci, ctypes.POINTER(cspn_sgd_hyper), ci, ci, vp]
    lib.cspn_sgd_step.restype = ci
    lib.cspn_visual_abi_version.restype = ci
    lib.cspn_visual_workspace_bytes.argtypes = [ci, ci, cs]
    lib.cspn_visual_workspace_bytes.restype = cs
    lib.cspn_visual_rows.argtypes = [ctypes.POINTER(cspn_visual_rows), ci, ci, ci, vp, cs, vp, vp]
    lib.cspn_visual_rows.restype = ci
    lib.cspn_visual_features.argtypes = [vp, cl, ci, ci, ci, ci, ci, vp, cs, vp, vp]
    lib.cspn_visual_features.restype = ci
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("cspn_last_error", "cspn_propagate_workspace_bytes", "cspn3_resident_workspace_bytes",
                        "cspnk_resident_workspace_bytes", "cspn_metrics_per_frame_workspace_bytes"):
            fn.restype = ci
    return lib


def lib():
    """The loaded engine.  Raises RuntimeError (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(SO_PATH):
                    raise RuntimeError(
                        "cspn_monodepth_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % SO_PATH)
                _lib = _declare(ctypes.CDLL(SO_PATH))
                if _lib.cspn_abi_version() != ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: ABI version mismatch")
                if _lib.cspn_criterion_abi_version() != CRITERION_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: criterion ABI version mismatch")
                if _lib.cspn_max8_abi_version() != MAX8_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: max8 ABI version mismatch")
                if _lib.cspn_abn_abi_version() != ABN_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: abn ABI version mismatch")
                if _lib.cspn_sparsify_abi_version() != SPARSIFY_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: sparsify ABI version mismatch")
                if _lib.cspn_transform_abi_version() != TRANSFORM_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: transform ABI version mismatch")
                if _lib.cspn_losses_abi_version() != LOSSES_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: losses ABI version mismatch")
                if _lib.cspn_optim_abi_version() != OPTIM_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: optim ABI version mismatch")
                if _lib.cspn_visual_abi_version() != VISUAL_ABI_VERSION:
                    raise RuntimeError("cspn_monodepth_amd: visual ABI version mismatch")
                poison = os.environ.get("CSPN_DEBUG_LDS_POISON", "")      # debugging aid (include/cspn_hip.h): "nan" or a hex word
                if poison and poison != "0":
                    _lib.cspn_debug_set_lds_poison(1, 0x7fc00000 if poison in ("1", "nan") else int(poison, 16), None)
    return _lib


def check(ok, what):
    """Truthy = success, as the reference's native convention (inplace_abn/functions.py:13-16)."""
    if not ok:
        raise RuntimeError("%s failed: %s" % (what, lib().cspn_last_error().decode()))

"""Loader / builder of libcspn_hip.so (the C-ABI HIP engine, include/cspn_hip.h).

The reference loaded its native code through torch.utils.ffi (network/libs/inplace_abn/build.py:3-21,
_ext/__init__.py:2-13 — removed from PyTorch 1.0); here it is a plain ``ctypes.CDLL``.
There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised
(the reference's ``_check`` does the same, inplace_abn/functions.py:13-16).
"""
import collections
import ctypes
import os
import shutil
import subprocess
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
SO_PATH = os.environ.get("CSPN_HIP_LIB") or os.path.join(_PKG, "libcspn_hip.so")   # env override: A/B builds
CSRC = os.path.join(_PKG, "csrc")
INCLUDE = os.path.join(_ROOT, "include")

CSPN_F32, CSPN_F16 = 0, 1
ABI_VERSION = 10         # CSPN_ABI_VERSION of include/cspn_hip.h this host code was written against
MAX8_MAX_STEPS_PER_LAUNCH = 16
ABN_ACT_LEAKY_RELU, ABN_ACT_ELU, ABN_ACT_NONE = 0, 1, 2
ABN_SMALL, ABN_SPLIT = 0, 1                                 # cspn_abn_plan_t.regime
ABN_FULL, ABN_STATS_ONLY, ABN_APPLY_ONLY = 0, 1, 2          # the `phase` of a training-mode cspn_abn_forward
SPARSIFY_UAR, SPARSIFY_DENSE = 0, 1                         # cspn_sparsify's `mode`
UNIFORM_PHILOX, UNIFORM_F32, UNIFORM_F64 = 0, 1, 2          # ... `uniform_kind`
RGB_NONE, RGB_F32, RGB_U8 = 0, 1, 2                         # ... `rgb_kind`
SPARSIFY_SLICE_PIXELS, SPARSIFY_MAX_SLICES = 1024, 64
TRANSFORM_VAL, TRANSFORM_TRAIN = 0, 1                       # cspn_transform's `mode`
TRANSFORM_PARAMS, TRANSFORM_GATHER_PIXELS, TRANSFORM_MAX_SECOND = 8, 256, 32768
LOSS_L1, LOSS_L2, LOSS_L1_LOG = 0, 1, 2
MEAN_L1, MEAN_GRAD, MEAN_RMSE, MEAN_RMSE_LOG = 0, 1, 2, 3   # the `kind` of cspn_mean_loss_*
LOSSES_STATE_BYTES = 48
SGD_CHUNK, SGD_TENSORS_PER_LAUNCH, SGD_MAX_WORKGROUPS = 4096, 109, 2048
VISUAL_RANGE_CHUNK, VISUAL_MAX_PLANES = 4096, 3
VISUAL_RGB_NONE, VISUAL_RGB_F32, VISUAL_RGB_U8 = 0, 1, 2      # cspn_visual_rows_t.rgb_kind
BLEND_NONE, BLEND_SPARSE, BLEND_PREMASK = 0, 1, 2
HEADS_MAX_HEADS, HEADS_MAX_OUT_CHANNELS = 4, 16              # CSPN_HEADS_MAX_* (include/cspn_heads.h)
HEADS_FORWARD, HEADS_BACKWARD_INPUT, HEADS_BACKWARD_WEIGHTS = 0, 1, 2      # the `pass` of cspn_heads_workspace_bytes
UPCONV_MAX_FILTERS = 2                                       # CSPN_UPCONV_MAX_FILTERS (include/cspn_upconv.h)
UPCONV_F32_BF16X3 = 2                                        # CSPN_UPCONV_F32_BF16X3: a `dtype` of cspn_upconv_forward alone
UPHALF_MAX_FILTERS = 2                                       # CSPN_UPHALF_MAX_FILTERS (include/cspn_uphalf.h)
HEAD16_MAX_HEADS, HEAD16_MAX_OUT_CHANNELS = 4, 16            # CSPN_HEAD16_MAX_* (include/cspn_head16.h)
HEAD16_TILE_H, HEAD16_TILE_W, HEAD16_CHANNEL_BLOCK = 8, 32, 32      # CSPN_HEAD16_TILE_*, CSPN_HEAD16_CHANNEL_BLOCK: the kernel's tiling


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


Family = collections.namedtuple("Family", "name header abi_version files functions opt_in")


def _families():
    """The one list of what the library is made of: everything below that names a file or a function reads it.  A family is a
    header under include/, the ABI version of it this host code was written against, its files under csrc/, its functions and
    whether it is opt-in.
    A file marked True is run by a bench.py workload and so part of code_digest(), as is the header of a family with such a file;
    the others are part of the build's staleness hash only (a digest that moved would mark the HBM traffic recorded under
    profiles/ as stale, bench.py `traffic_stale`).  A function is name -> argtypes (None: left unset) where it returns int, and
    name -> (restype, argtypes) where it does not."""
    vp, ci, cu, cl, cs, cf, cd = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_long, ctypes.c_size_t, ctypes.c_float,
                                  ctypes.c_double)
    ll, ull, ptr = ctypes.c_longlong, ctypes.c_ulonglong, ctypes.POINTER
    plan, rplan, geom = ptr(cspn_plan), ptr(cspn_resident_plan), ptr(cspn_conv_geometry)

    def family(name, header, abi_version, files, functions, opt_in=False):
        return Family(name, os.path.join(INCLUDE, header), abi_version, files,
                      {n: sig if isinstance(sig, tuple) else (ci, sig) for n, sig in functions.items()}, opt_in)

    return (
        family("core", "cspn_hip.h", ABI_VERSION, {
            "cspn_propagate.hip": True, "cspn_resident.hip": True, "cspnk_resident.hip": True, "cspnk_d2.hip": True,
            "cspn_prepare.hip": True, "cspn_backward.hip": True, "cspn_metrics.hip": True, "cspn_metrics_frame.hip": False,
            "cspn_debug.hip": True, "cspn_repair.hip": True, "pac_conv2d.hip": False, "pac_conv2d_s2.hip": False,
            "cspn_unpool.hip": False, "cspn_common.hpp": True, "cspnk_helpers.hpp": True, "pac_launch.hpp": False}, {
            "cspn_abi_version": None,
            "cspn_last_error": (ctypes.c_char_p, None),
            "cspn_plan_resolve": [ci, ci, ci, ci, ci, ci, plan, plan],
            "cspn3_prepare": [vp, ci, cl, cl, ci, ci, ci, ci, vp, ci, vp, vp],
            "cspn_pac_prepare": [vp, ci, ci, ci, ci, ci, vp, ci, vp],
            "cspn_propagate_workspace_bytes": (cs, [ci, ci, ci, ci, ci, ci]),
            "cspn_propagate": [vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, plan, vp],
            "cspn_propagate_scored": [vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, ci, plan, vp],
            "cspn_propagate_transposed": [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, plan, vp],
            "cspn3_propagate_from_guidance": [vp, ci, cl, cl, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, ci, plan, vp],
            "cspn_transpose_weights": [vp, vp, ci, ci, ci, ci, ci, vp],
            "cspn3_resident_plan": [ci, ci, ci, ci, ci, ci, rplan],
            "cspn3_resident_workspace_bytes": (cs, [ci, ci, ci]),
            "cspn3_forward_resident": [vp, cl, cl, vp, vp, vp, vp, vp, vp, vp, cu, vp, ci, ci, ci, ci, ci, ci, vp, vp, ci, rplan, vp],
            "cspn3_transposed_resident": [vp, vp, vp, vp, vp, cu, vp, ci, ci, ci, ci, ci, ci, rplan, vp],
            "cspn3_transposed_resident_guidance": [vp, cl, cl, vp, vp, vp, vp, vp, cu, vp, ci, ci, ci, ci, ci, ci, rplan, vp],
            "cspnk_resident_plan": [ci, ci, ci, ci, ci, ci, ci, ci, rplan],
            "cspnk_resident_workspace_bytes": (cs, [ci, ci, ci, ci]),
            "cspnk_forward_resident": [vp, ci, ci, vp, vp, vp, ci, vp, cu, vp, ci, ci, ci, ci, ci, vp, vp, ci, rplan, vp],
            "cspnk_forward_resident_history": [vp, ci, ci, vp, vp, vp, vp, vp, cu, vp, ci, ci, ci, ci, ci, rplan, vp],
            "cspnk_transposed_resident": [vp, ci, ci, vp, vp, ci, vp, vp, vp, cu, vp, ci, ci, ci, ci, ci, rplan, vp],
            "cspn_grad_weights": [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp],
            "cspn3_grad_guidance": [vp, ci, cl, cl, ci, vp, ci, vp, vp, vp, ci, ci, ci, vp],
            "cspn_pac_grad_guided": [vp, ci, vp, vp, ci, ci, ci, ci, ci, vp],
            "cspn3_backward_tail": [vp, vp, vp, vp, vp, vp, cl, cl, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp],
            "cspn_pac_backward_tail": [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp],
            "cspn_metrics_accumulate": [vp, vp, ci, cs, vp, ci, vp],
            "cspn_metrics_per_frame_workspace_bytes": (cs, [ci, cs]),
            "cspn_metrics_per_frame": [vp, vp, ci, ci, cs, vp, vp, vp],
            "cspn_meter_update": [vp, ci, vp, vp],
            "cspn_pac_out_size": [ci, ci, geom, ptr(ci), ptr(ci)],
            "cspn_pac_force_generic": [ci, ptr(ci)],
            "cspn_pac_conv2d": [vp, vp, vp, ci, ci, ci, ci, ci, ci, geom, vp],
            "cspn_pac_conv2d_grad_input": [vp, vp, vp, ci, ci, ci, ci, ci, ci, geom, vp],
            "cspn_pac_conv2d_grad_kernel": [vp, vp, vp, ci, ci, ci, ci, ci, ci, geom, vp],
            "cspn_pac_nd2col": [vp, vp, ci, ci, ci, ci, ci, geom, vp],
            "cspn_unpool2d": [vp, vp, ci, cl, ci, ci, ci, ci, ci, vp],
            "cspn_unpool2d_backward": [vp, vp, ci, cl, ci, ci, ci, ci, ci, vp],
            "cspn_debug_set_lds_poison": [ci, cu, ptr(ci)]}),
        family("criterion", "cspn_criterion.h", 1, {"cspn_criterion.hip": False, "cspn_loss_units.hpp": False}, {
            "cspn_criterion_abi_version": None,
            "cspn_criterion_workspace_bytes": (cs, [cs]),
            "cspn_criterion_forward": [vp, vp, ci, ci, cs, vp, vp, vp],
            "cspn_criterion_backward": [vp, vp, ci, ci, cs, vp, vp, vp, vp]}),
        family("max8", "cspn_max8.h", 1, {"cspn_max8.hip": False}, {
            "cspn_max8_abi_version": None,
            "cspn_max8_workspace_bytes": (cs, [ci, ci, ci, ci, ci]),
            "cspn_max8_forward": [vp, cl, cl, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp],
            "cspn_max8_backward": [vp, cl, cl, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]}),
        family("abn", "cspn_abn.h", 1, {"cspn_abn.hip": False}, {
            "cspn_abn_abi_version": None,
            "cspn_abn_plan": [ci, ci, ci, ptr(cspn_abn_plan)],
            "cspn_abn_workspace_bytes": (cs, [ci, ci, ci]),
            "cspn_abn_forward": [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, ci, cf, vp, vp],
            "cspn_abn_backward_reduce": [vp, vp, vp, vp, vp, vp, ci, ci, ci, cf, ci, cf, vp, vp],
            "cspn_abn_backward": [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, ci, cf, vp, vp]}),
        family("sparsify", "cspn_sparsify.h", 1, {"cspn_sparsify.hip": False, "cspn_philox.hpp": False}, {
            "cspn_sparsify_abi_version": None,
            "cspn_sparsify_slices": [cs],
            "cspn_sparsify_workspace_bytes": (cs, [ci, cs]),
            "cspn_sparsify": [vp, ci, ci, ci, ci, ci, ll, cf, vp, ci, vp, ull, vp, cl, vp, ci, vp, cl, cl, vp, vp, vp]}),
        family("transform", "cspn_transform.h", 1, {"cspn_transform.hip": False}, {
            "cspn_transform_abi_version": None,
            "cspn_transform_first_size": [ci, ci, cd, ptr(ci), ptr(ci)],
            "cspn_transform_workspace_bytes": (cs, [ci, ci, ci, ci, cd, ci, ci]),
            "cspn_transform": [vp, vp, ci, ci, ci, cd, ci, ci, ci, vp, vp, cl, cl, vp, cl, vp, vp],
            "cspn_transform_draw_params": [vp, ci, ull, vp, vp]}),
        family("losses", "cspn_losses.h", 1, {"cspn_losses.hip": False}, {
            "cspn_losses_abi_version": None,
            "cspn_losses_workspace_bytes": (cs, [cs]),
            "cspn_berhu_forward": [vp, vp, ci, cs, vp, vp, vp],
            "cspn_berhu_backward": [vp, vp, ci, cs, vp, vp, vp, vp],
            "cspn_mean_loss_forward": [vp, vp, ci, ci, cs, vp, vp, vp],
            "cspn_mean_loss_backward": [vp, vp, ci, ci, cs, vp, vp, vp, vp]}),
        family("optim", "cspn_optim.h", 1, {"cspn_optim.hip": False}, {
            "cspn_optim_abi_version": None,
            "cspn_sgd_plan": [ptr(cs), ci, ci, ptr(ci), ptr(cs)],
            "cspn_sgd_step": [ptr(cspn_sgd_tensor), ci, ptr(cspn_sgd_hyper), ci, ci, vp]}),
        family("visual", "cspn_visual.h", 1, {"cspn_visual.hip": False}, {
            "cspn_visual_abi_version": None,
            "cspn_visual_workspace_bytes": (cs, [ci, ci, cs]),
            "cspn_visual_rows": [ptr(cspn_visual_rows), ci, ci, ci, vp, cs, vp, vp],
            "cspn_visual_features": [vp, cl, ci, ci, ci, ci, ci, vp, cs, vp, vp]}),
        family("heads", "cspn_heads.h", 1, {"cspn_heads.hip": False}, {
            "cspn_heads_abi_version": None,
            "cspn_heads_workspace_bytes": (cs, [ci, ci, ci, ci, ci, ci, ci, ci]),
            "cspn_heads_forward": [vp, ptr(vp), ptr(vp), ptr(ci), ci, vp, ci, ci, ci, ci, ci, ci, vp],
            "cspn_heads_backward_input": [ptr(vp), ptr(vp), ptr(ci), ci, vp, vp, ci, ci, ci, ci, ci, ci, vp],
            "cspn_heads_backward_weights": [vp, ptr(vp), ptr(vp), ptr(ci), ci, vp, ci, ci, ci, ci, ci, ci, vp]}, opt_in=True),
        family("upconv", "cspn_upconv.h", 1, {"cspn_upconv.hip": False, "cspn_upconv_core.hpp": False}, {
            "cspn_upconv_abi_version": None,
            "cspn_upconv_workspace_bytes": (cs, [ci, ci]),
            "cspn_upconv_pack": [ptr(vp), ptr(ci), ci, ci, ci, ci, ci, vp, vp],
            "cspn_upconv_forward": [vp, ci, vp, vp, vp, ci, ptr(vp), ptr(ci), ci, ci, ci, ci, ci, ci, ci, vp]}, opt_in=True),
        family("uphalf", "cspn_uphalf.h", 1, {"cspn_uphalf.hip": False}, {
            "cspn_uphalf_abi_version": None,
            "cspn_uphalf_packed_bytes": (cs, [ci, ci]),
            "cspn_uphalf_pack": [ptr(vp), ptr(ci), ci, ci, ci, ci, ci, vp, vp],
            "cspn_uphalf_forward": [vp, vp, vp, vp, ci, ptr(vp), ptr(ci), ci, ci, ci, ci, ci, ci, ci, vp]}, opt_in=True),
        family("uptail", "cspn_uptail.h", 1, {"cspn_uptail.hip": False}, {
            "cspn_uptail_abi_version": None,
            "cspn_uptail_packed_bytes": (cs, [ci, ci, ci, ci]),
            "cspn_uptail_pack": [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp],
            "cspn_uptail_forward": [vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp]}, opt_in=True),
    ), (
        family("convbn", "cspn_convbn.h", 1, {"cspn_convbn.hip": False}, {
            "cspn_convbn_abi_version": None,
            "cspn_convbn_packed_bytes": (cs, [ci, ci, ci, ci]),
            "cspn_convbn_pack": [vp, ci, ci, ci, ci, ci, ci, vp, vp],
            "cspn_convbn_forward": [vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]}, opt_in=True),
    ), (
        family("head16", "cspn_head16.h", 1, {"cspn_head16.hip": False}, {
            "cspn_head16_abi_version": None,
            "cspn_head16_workspace_bytes": (cs, [ci, ci]),
            "cspn_head16_forward": [vp, ptr(vp), ci, ptr(vp), ptr(ci), ci, vp, ci, ci, ci, ci, ci, ci, vp]}, opt_in=True),
    )


# A family with `opt_in` set sits behind a switch of the models that is off by default (`fused_heads`, `fused_decoder`, `fused_tail`,
# network/up_pooling.py); the others are what a default call of the package can reach.  All are built, declared and version-checked
# alike, and no file of an opt-in family is part of code_digest().
#
# LATER_FAMILIES is a further part of the table: opt-in families added after those thirteen, which the older tests count and whose
# tuples and digests they restate (convbn: `fused_encoder`, network/conv_bn.py).  They are built, declared and version-checked as
# the opt-in ones and found by family(); their sources and headers are LATER_SOURCES / LATER_HEADERS, part of the build's staleness
# stamp (_later_digest) and of no tuple or digest above.
#
# LATEST_FAMILIES is a third part, for the families added after those tests were written in turn (head16: the half path of
# `fused_heads`, network/up_pooling.py).  Built, declared, version-checked and found by family() as the others; their sources and
# headers are LATEST_SOURCES / LATEST_HEADERS and carry a stamp of their own (_latest_digest) in a second file next to the library,
# so that the first stamp is what it was.  No tuple or digest above contains them.
ALL_FAMILIES, LATER_FAMILIES, LATEST_FAMILIES = _families()
FAMILIES = tuple(f for f in ALL_FAMILIES if not f.opt_in)
OPT_IN_FAMILIES = tuple(f for f in ALL_FAMILIES if f.opt_in)
EVERY_FAMILY = ALL_FAMILIES + LATER_FAMILIES


def family(name):
    return next(f for f in EVERY_FAMILY + LATEST_FAMILIES if f.name == name)


def _files(suffix, benchmarked=None, families=FAMILIES):
    return tuple(f for fam in families for f, b in fam.files.items() if f.endswith(suffix) and benchmarked in (None, b))


SOURCES = _files(".hip")                      # one TU each
OPT_IN_SOURCES = _files(".hip", families=OPT_IN_FAMILIES)
BENCH_UNRELATED = _files(".hip", False)       # kernels no bench.py workload launches
HEADERS = tuple(os.path.join(CSRC, f) for f in _files(".hpp", True)) + tuple(f.header for f in FAMILIES if any(f.files.values()))
BUILD_HEADERS = HEADERS + tuple(os.path.join(CSRC, f) for f in _files(".hpp", False, ALL_FAMILIES)) + \
    tuple(f.header for f in ALL_FAMILIES if not any(f.files.values()))
EXPORTS = tuple(family("core").functions)      # every symbol include/cspn_hip.h declares
LATER_SOURCES = _files(".hip", families=LATER_FAMILIES)
LATER_HEADERS = tuple(os.path.join(CSRC, f) for f in _files(".hpp", families=LATER_FAMILIES)) + tuple(f.header for f in LATER_FAMILIES)
LATEST_SOURCES = _files(".hip", families=LATEST_FAMILIES)
LATEST_HEADERS = tuple(os.path.join(CSRC, f) for f in _files(".hpp", families=LATEST_FAMILIES)) + tuple(f.header for f in LATEST_FAMILIES)


def _source_digest(flags, code_only=False):
    """Content hash of the kernel sources (+ flags).  code_only: the hash profiles/ pins measured HBM traffic to (bench.py
    `traffic_stale`) — `//` comments and blank space are left out (a reworded comment must not invalidate a measurement),
    and so are the translation units of the widening rows, which no bench workload launches."""
    import hashlib
    import re
    h = hashlib.sha256(" ".join(flags).encode())
    tus = [f for f in SOURCES if f not in BENCH_UNRELATED] if code_only else SOURCES + OPT_IN_SOURCES
    for path in [os.path.join(CSRC, f) for f in tus] + list(HEADERS if code_only else BUILD_HEADERS):
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


def _later_digest(digest):
    """The build's staleness stamp: `digest` (_source_digest of the flags) carried on over the sources and headers of LATER_FAMILIES."""
    import hashlib
    h = hashlib.sha256(digest.encode())
    for path in [os.path.join(CSRC, f) for f in LATER_SOURCES] + list(LATER_HEADERS):
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _latest_digest(flags):
    """The second stamp: the flags, then the sources and headers of LATEST_FAMILIES."""
    import hashlib
    h = hashlib.sha256(" ".join(flags).encode())
    for path in [os.path.join(CSRC, f) for f in LATEST_SOURCES] + list(LATEST_HEADERS):
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _stamped(path, digest):
    return os.path.exists(path) and open(path).read().strip() == digest


def build(force=False, verbose=False):
    """hipcc cross-compiles for gfx950 without a GPU: the translation units are compiled in parallel to
    csrc/_build/*.o and linked into the in-tree .so (which travels with gpurun snapshots).  Staleness is decided by
    a content hash of the sources + flags stored next to the library (file times do not survive every copy), and for the
    LATEST_FAMILIES by a second one in a file of its own: the build is current only if both match."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(CSRC, f) for f in SOURCES + OPT_IN_SOURCES + LATER_SOURCES + LATEST_SOURCES]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    # -fno-slp-vectorize: the SLP pass pairs the stencil FMAs into v_pk_fma_f32 and pays for it with ~50 v_mov
    # per step to build operand pairs; scalar v_fma_f32 measured 4 % faster (profiles/).  No fast-math: 0/0 = NaN.
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize"] + \
        os.environ.get("CSPN_HIPCC_FLAGS", "").split() + ["-I", INCLUDE]
    digest = _later_digest(_source_digest(flags[:-2]))
    latest = _latest_digest(flags[:-2])
    stamp, stamp2 = SO_PATH + ".hash", SO_PATH + ".hash2"
    if not force and os.path.exists(SO_PATH) and _stamped(stamp, digest) and _stamped(stamp2, latest):
        return SO_PATH
    bdir = os.path.join(CSRC, "_build")
    os.makedirs(bdir, exist_ok=True)

    import hashlib
    hdr = hashlib.sha256(" ".join(flags[:-2]).encode())
    for path in BUILD_HEADERS + LATER_HEADERS:
        with open(path, "rb") as fh:
            hdr.update(fh.read())
    hdr2 = hdr.copy()                         # the translation units of LATEST_FAMILIES see their headers too; the others do not
    for path in LATEST_HEADERS:
        with open(path, "rb") as fh:
            hdr2.update(fh.read())

    def compile_one(src):
        # per-object staleness: flags + headers + this translation unit (an edit to one kernel recompiles one file)
        obj = os.path.join(bdir, os.path.basename(src)[:-4] + ".o")
        h = (hdr2 if os.path.basename(src) in LATEST_SOURCES else hdr).copy()
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
    for path, value in ((stamp, digest), (stamp2, latest)):
        with open(path, "w") as fh:
            fh.write(value + "\n")
    return SO_PATH


_lib = None
_lock = threading.Lock()


def _declare(lib):
    for fam in EVERY_FAMILY + LATEST_FAMILIES:
        for name, (restype, argtypes) in fam.functions.items():
            fn = getattr(lib, name)
            if restype is not ctypes.c_int:           # ctypes' default
                fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
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
                for fam in EVERY_FAMILY + LATEST_FAMILIES:
                    sub = "" if fam.name == "core" else fam.name      # cspn_abi_version, cspn_<family>_abi_version
                    if getattr(_lib, "cspn_%sabi_version" % (sub and sub + "_"))() != fam.abi_version:
                        raise RuntimeError("cspn_monodepth_amd: %sABI version mismatch" % (sub and sub + " "))
                poison = os.environ.get("CSPN_DEBUG_LDS_POISON", "")      # debugging aid (include/cspn_hip.h): "nan" or a hex word
                if poison and poison != "0":
                    _lib.cspn_debug_set_lds_poison(1, 0x7fc00000 if poison in ("1", "nan") else int(poison, 16), None)
    return _lib


def check(ok, what):
    """Truthy = success, as the reference's native convention (inplace_abn/functions.py:13-16)."""
    if not ok:
        raise RuntimeError("%s failed: %s" % (what, lib().cspn_last_error().decode()))

"""Tensor-level host API over the C ABI (include/cspn_hip.h): validation, buffer ownership, autograd.

Mirrors the calling discipline of the reference's native wrappers (network/libs/inplace_abn/
functions.py:13-16 `_check`, :65-67 contiguity checks, lib_cffi.cpp:37 current stream): PyTorch owns
every buffer, the engine enqueues on the tensor's current HIP stream, failures raise RuntimeError.
PyTorch is plumbing here (device memory, streams, autograd bookkeeping); all arithmetic of the hot
path runs in libcspn_hip.so.  There is no CPU fallback.
"""
import ctypes
import math
import os
import threading
import weakref
import time

import torch

from . import _lib
from ._host import _device_guard, _dt, _p, _require_device, _stream
from ._lib import BLEND_NONE, BLEND_PREMASK, BLEND_SPARSE, CSPN_F16, CSPN_F32, STEP_AUTO, STEP_DOT2, STEP_FMA, cspn_plan

_DEFAULT_PLANS = {}   # K -> dict, set by set_default_plan (e.g. from a tuning run)
_EVENT_LOG = None     # when an EventLog: propagate() records (start_event, end_event, n_launches, steps_per_launch)


class EventLog(list):
    """bench.py hook: HIP events recorded on the launch stream around every propagation loop.

    Event objects are created (and recorded once, which is what actually allocates them) up front: creating
    them inside a timed region costs ~100 us each for the first few hundred."""

    def __init__(self, n_pairs=0, every=1):
        super(EventLog, self).__init__()
        self.every = max(1, int(every))      # sample every n-th instrumented call (two event records cost ~3 us of stream time)
        self.calls = 0
        self.pool = []
        for _ in range(2 * int(n_pairs)):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.pool.append(ev)
        self.plan_cache = {}

    def take(self):
        # the sampled call is the MIDDLE one of every `every`: the first call after a device-wide fence is the one call of a
        # timed region the GPU waits for (its queue is empty), and two event records cost that call ~15 us of host time
        self.calls += 1
        return (self.calls - 1) % self.every == self.every // 2

    def pair(self):
        if len(self.pool) >= 2:
            return self.pool.pop(), self.pool.pop()
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def set_event_log(log):
    global _EVENT_LOG
    _EVENT_LOG = log


def _sampled_log():
    """The event log if there is one and it samples this call, else None: THE sampling decision — a call asks exactly once."""
    log = _EVENT_LOG
    return log if log is not None and log.take() else None


_RESOLVED = {}       # (K,B,H,W,T,history,plan items) -> resolved plan dict (cspn_plan_resolve is pure)


def resolve_plan(K, B, H, W, T, keep_history=False, plan=None):
    """The plan the engine will actually use (dict), via cspn_plan_resolve (memoised: it is a pure function)."""
    eff = _DEFAULT_PLANS.get(int(K)) if plan is None else plan
    key = None
    if eff is None or isinstance(eff, dict):
        key = (int(K), int(B), int(H), int(W), int(T), bool(keep_history),
               None if eff is None else tuple(sorted(eff.items())))
        hit = _RESOLVED.get(key)
        if hit is not None:
            return dict(hit)
    out = cspn_plan()
    ok = _lib.lib().cspn_plan_resolve(int(K), int(B), int(H), int(W), int(T), int(bool(keep_history)),
                                      _plan_ptr(K, plan), ctypes.byref(out))
    _lib.check(ok, "cspn_plan_resolve")
    res = {name: int(getattr(out, name)) for name, _ in cspn_plan._fields_}
    if key is not None:
        if len(_RESOLVED) > 4096:
            _RESOLVED.clear()
        _RESOLVED[key] = dict(res)
    return res


_FROM_GUIDANCE = True    # see set_from_guidance


def set_from_guidance(enabled):
    """Route no-grad 3x3 forwards through cspn3_propagate_from_guidance: the first launch derives the weights
    from the raw guidance and publishes them for the later launches, so there is no separate prepare pass
    (bit-identical results; ~8 % faster per forward at config 2 on MI355X).  False = cspn3_prepare + propagate."""
    global _FROM_GUIDANCE
    _FROM_GUIDANCE = bool(enabled)


_TUNED = {}          # autotune cache: problem key -> plan dict
_NQ_THREADS = {3: ((1, 256), (2, 256), (4, 256), (1, 512), (2, 512), (4, 512), (1, 1024), (2, 1024)),
               5: ((1, 256), (2, 256), (3, 256), (1, 512)),
               7: ((1, 256),)}
_S_LIST = {3: (1, 3, 4, 5, 6, 8, 12), 5: (1, 2, 3, 4), 7: (1, 2)}


def candidate_plans(K, H, W, T):
    """Launch plans worth timing for a problem (the sweep space of tools/tune.py, pruned)."""
    R = K // 2
    widths = sorted({w for w in (32, 48, 64, 80, 96, 128) if w <= W + 3} |
                    {-(-(-(-W // n)) // 4) * 4 for n in (1, 2, 3, 4, 5, 6, 8) if -(-W // n) >= 16} or {-(-W // 4) * 4})
    plans = []
    for S in _S_LIST[K]:
        if S > max(T, 1):
            continue
        hyw = (S - 1) * R
        hxw = -(-hyw // 4) * 4
        for nq, threads in _NQ_THREADS[K]:
            for tw in widths:
                wq = (tw + 2 * hxw) // 4
                if wq > threads:
                    continue
                th_max = min(nq * (threads // wq) - 2 * hyw, H)
                if th_max < min(4, H):
                    continue
                for th in {th_max, -(-H // -(-H // th_max))}:
                    plans.append(dict(steps_per_launch=S, tile_w=tw, tile_h=th, quads_per_thread=nq, threads=threads))
    return plans


def autotune_plan(w, d0, sparse, K, T, blend, keep_history=False, reps=5, verbose=False, guidance=None, score=None):
    """Time candidate_plans() on the actual tensors (HIP events on the current stream) and cache the fastest.

    Opt-in (`plan="auto"`): costs a few tens of ms once per (shape, dtype, blend) key.  The built-in plan is always a
    contender and keeps its place unless a candidate beats it by more than 2 % (two timing passes, best of each), so
    tuning never makes things worse than the heuristic.  With `guidance` (3x3) the entry that is timed is the one
    inference runs — weights derived in the first launch, and with `score=(target, acc)` the metrics fused into the last
    — whose instances differ in register pressure."""
    B, H, W = d0.shape
    key = (int(K), B, H, W, int(T), w.dtype, d0.dtype, int(blend), bool(keep_history), w.device.index,
           guidance is not None, score is not None)
    if key in _TUNED:
        return _TUNED[key]
    use_g = guidance is not None and K == 3 and not keep_history

    use_g = use_g and from_guidance_supported(guidance, d0, sparse, None)

    def run(plan):
        if use_g:
            # plans without a from-guidance instance would silently time the prepared-weights path instead
            if plan is not None and not from_guidance_supported(guidance, d0, sparse, plan):
                raise RuntimeError("no from-guidance instance")
            propagate_from_guidance(guidance, d0, sparse, T, blend, plan=plan, score=score)
        else:
            propagate(w, d0, sparse, K, T, blend, keep_history, plan)

    def time_plan(plan):
        try:
            if plan is not None:
                resolve_plan(K, B, H, W, T, keep_history, plan)
            run(plan)                                                             # warm-up / validates the launch
            best = float("inf")
            for _ in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run(plan)
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
            return best
        except RuntimeError:
            return float("inf")

    best, best_us = None, float("inf")
    if W % 4 == 0 and T > 0:
        base_us = time_plan(None)
        for plan in candidate_plans(K, H, W, T):
            us = time_plan(plan)
            if us < best_us:
                best, best_us = plan, us
        if not best_us < 0.98 * base_us:
            best, best_us = None, base_us
    if verbose:
        print("autotune K=%d B=%d %dx%d T=%d -> %s (%.1f us)" % (K, B, H, W, T, best, best_us))
    _TUNED[key] = best        # None = keep the built-in heuristic
    return best


# Built-in plans that depend on the tap-volume dtype (the C heuristic only sees the geometry).  5x5 with fp16 weights:
# the packed tap registers leave room for three quads per thread, and the plan sweeps (profiles/r01_plan_sweep_pac5.txt)
# put S = 4 with NQ = 3 at 256 threads ahead of the fp32-safe S = 3 / NQ = 1 default (config 3: +7 % end to end).
_DTYPE_DEFAULT_PLANS = {(5, torch.float16): dict(steps_per_launch=4, quads_per_thread=3, threads=256)}


def dtype_default_plan(K, w_dtype, plan=None):
    """`plan` unless it is None and nothing was set with set_default_plan: then the dtype-specific built-in, if any
    (a partial plan — the engine completes it with the cheapest tiling for those settings)."""
    if plan is not None or int(K) in _DEFAULT_PLANS:
        return plan
    return _DTYPE_DEFAULT_PLANS.get((int(K), w_dtype))


def set_default_plan(K, plan):
    """plan: None or dict(steps_per_launch=, tile_w=, tile_h=, quads_per_thread=, threads=, force_scalar=)."""
    if plan is None:
        _DEFAULT_PLANS.pop(int(K), None)
    else:
        _DEFAULT_PLANS[int(K)] = dict(plan)


def _plan_ptr(K, plan):
    plan = _DEFAULT_PLANS.get(int(K)) if plan is None else plan
    if plan is None or isinstance(plan, str):
        return None
    if isinstance(plan, cspn_plan):
        return ctypes.pointer(plan)
    p = cspn_plan()
    for k, v in plan.items():
        if not hasattr(p, k):
            raise ValueError("unknown plan field %r" % k)
        setattr(p, k, int(v))
    return ctypes.pointer(p)


def _plane(t, B, H, W, name):
    """[B,1,H,W] / [B,H,W] -> contiguous; returns tensor viewed as [B,H,W]."""
    if t is None:
        return None
    if t.dim() == 4:
        if t.shape[1] != 1:
            raise ValueError("%s must have exactly one channel, got shape %s" % (name, tuple(t.shape)))
        t = t[:, 0]
    if tuple(t.shape) != (B, H, W):
        raise ValueError("%s has shape %s, expected [%d,1,%d,%d]" % (name, tuple(t.shape), B, H, W))
    return t.contiguous()


def _weight_buffer(B, NT, H, W, dtype, device):
    """Tap volume for the engine (include/cspn_hip.h "tap-volume layout"): fp32 is the planar [B,NT,H,W];
    fp16 is opaque — tap pairs interleaved per 4-pixel quad, [B, NT/2, ceil(HW/4), 2, 4] — returned as a
    [B, NT, ceil4(HW)] tensor.  Only the engine's own kernels read or write it."""
    if dtype == torch.float16:
        return torch.empty((B, NT, (H * W + 3) // 4 * 4), dtype=dtype, device=device)
    return torch.empty((B, NT, H, W), dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------------ raw ops
def cspn3_prepare(guidance, want_s=False, w_dtype=None, valid_w=0):
    """|g| -> shift -> /S: the 8 normalised weight planes of the 3x3 variant (CSPN_new.py:29-70,:124-127).

    Reads channels 0..7 of a [B,C>=8,H,W] guidance in place (C=12 from unet_cspn_nyu.py:332)."""
    dev = _require_device(guidance)
    if guidance.dim() != 4 or guidance.shape[1] < 8:
        raise ValueError("guidance must be [B,C>=8,H,W], got %s" % (tuple(guidance.shape),))
    B, C, H, W = guidance.shape
    g = guidance if guidance.is_contiguous() else guidance.contiguous()
    w_dtype = g.dtype if w_dtype is None else w_dtype
    w8 = _weight_buffer(B, 8, H, W, w_dtype, dev)
    S = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_s else None
    with _device_guard(dev):
        ok = _lib.lib().cspn3_prepare(_p(g), _dt(g), g.stride(0), g.stride(1), B, H, W, int(valid_w), _p(w8), _dt(w8),
                                      _p(S), _stream(dev))
    _lib.check(ok, "cspn3_prepare")
    return w8, S, g


def pac_prepare(guided, w_dtype=None):
    """softmax over the K^2-1 taps at the centre pixel (CSPN_ours.py:35-41; the centre tap is implicit)."""
    dev = _require_device(guided)
    if guided.dim() != 4:
        raise ValueError("guided must be [B,K*K-1,H,W]")
    B, C, H, W = guided.shape
    K = int(math.sqrt(C + 1))                      # CSPN_ours.py:32
    if K * K != C + 1 or K not in (3, 5, 7):
        raise ValueError("guided has %d channels; supported K*K-1 for K in (3,5,7)" % C)
    g = guided.contiguous()
    w_dtype = g.dtype if w_dtype is None else w_dtype
    if w_dtype != g.dtype:
        raise TypeError("pac_prepare: weight dtype must equal guided dtype")
    wk = _weight_buffer(B, C, H, W, w_dtype, dev)
    with _device_guard(dev):
        ok = _lib.lib().cspn_pac_prepare(_p(g), _dt(g), B, H, W, K, _p(wk), _dt(wk), _stream(dev))
    _lib.check(ok, "cspn_pac_prepare")
    return wk, K


def propagate(w, d0, sparse, K, T, blend, keep_history=False, plan=None, valid_w=0):
    """T steps of d <- blend(sum_j w_j * d[.+off_j]).  w: tap volume from cspn3_prepare / pac_prepare /
    transpose_weights (see _weight_buffer); d0, sparse [B,H,W].

    Returns (d_T [B,H,W], history [T,B,H,W] or None); with history, d_T is history[T-1] (a view)."""
    dev = _require_device(w, d0, sparse)
    B, H, W = d0.shape
    NT = K * K - 1
    hw = (H * W + 3) // 4 * 4 if w.dtype == torch.float16 else H * W
    if w.shape[0] != B or w.shape[1] != NT or w.numel() != B * NT * hw:
        raise ValueError("weight volume of shape %s does not match K=%d and depth %s" % (
            tuple(w.shape), K, tuple(d0.shape)))
    if not (w.is_contiguous() and d0.is_contiguous() and (sparse is None or sparse.is_contiguous())):
        raise ValueError("propagate: tensors must be contiguous")
    if sparse is not None and sparse.dtype != d0.dtype:
        raise TypeError("sparse dtype must equal the depth dtype")
    if blend != BLEND_NONE and sparse is None:
        raise ValueError("blend mode needs sparse")
    L = _lib.lib()
    hist = out = work = None
    T = int(T)
    if isinstance(plan, str):
        if plan != "auto":
            raise ValueError("plan must be None, a dict, a cspn_plan or 'auto'")
        plan = autotune_plan(w, d0, sparse, K, T, blend, keep_history)
    if keep_history and T > 0:
        hist = torch.empty((T, B, H, W), dtype=d0.dtype, device=dev)
    else:
        out = torch.empty((B, H, W), dtype=d0.dtype, device=dev)
        nbytes = L.cspn_propagate_workspace_bytes(B, H, W, T, _dt(d0), 0)
        if nbytes:
            work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    log = _sampled_log()
    with _device_guard(dev):
        if log is not None:
            ev0, ev1 = log.pair()
            ev0.record(torch.cuda.current_stream(dev))
        ok = L.cspn_propagate(_p(w), _dt(w), _p(d0), _p(sparse), _p(out), _p(hist), _p(work), _dt(d0),
                              B, H, W, int(valid_w), int(K), T, int(blend), _plan_ptr(K, plan), _stream(dev))
        if log is not None:
            ev1.record(torch.cuda.current_stream(dev))
            key = (K, B, H, W, T, keep_history, id(plan))
            if key not in log.plan_cache:
                log.plan_cache[key] = resolve_plan(K, B, H, W, T, keep_history, plan)["steps_per_launch"]
            S = log.plan_cache[key]
            log.append((ev0, ev1, -(-T // max(S, 1)), S))
    _lib.check(ok, "cspn_propagate")
    if hist is not None:
        return hist[T - 1], hist
    return out, None


_FROM_GUIDANCE_INSTANCES = ((1, 256), (2, 256), (1, 512), (2, 512), (1, 1024), (2, 1024))
_TRANSPOSED_INSTANCES = {3: ((1, 256), (2, 256), (1, 512), (2, 512), (1, 1024), (2, 1024)),
                         5: ((1, 256), (1, 512)), 7: ((1, 256),)}
_SCORED_INSTANCES = {3: ((1, 256), (1, 512), (1, 1024), (2, 512)), 5: ((1, 256), (1, 512))}


def scored_supported(w, d0, sparse, target, K, T, plan=None):
    """Can cspn_propagate_scored take this problem (else: propagate + evaluation.metric_sums)?"""
    B, H, W = d0.shape
    if K not in _SCORED_INSTANCES or T < 1 or W % 4 or w.dtype != d0.dtype or target.dtype != d0.dtype:
        return False
    if any(t is not None and t.data_ptr() % 16 for t in (w, d0, sparse, target)):
        return False
    p = resolve_plan(K, B, H, W, T, False, plan)
    return not p["force_scalar"] and (p["quads_per_thread"], p["threads"]) in _SCORED_INSTANCES[K]


def propagate_scored(w, d0, sparse, K, T, blend, target, acc, plan=None, valid_w=0):
    """propagate() whose final launch also adds the depth metrics of d_T vs `target` [B,H,W] into `acc`
    (evaluation.new_accumulator): the refined batch is not re-read by a separate metrics pass."""
    dev = _require_device(w, d0, sparse, target)
    B, H, W = d0.shape
    if acc.dtype != torch.float64 or acc.dim() != 2 or acc.shape[1] != 10 or not acc.is_contiguous():
        raise ValueError("acc must be a contiguous float64 [nslots, 10] tensor (evaluation.new_accumulator)")
    if not (target.is_contiguous() and tuple(target.shape) == (B, H, W)):
        raise ValueError("target must be a contiguous [B,H,W] tensor")
    L = _lib.lib()
    out = torch.empty((B, H, W), dtype=d0.dtype, device=dev)
    nbytes = L.cspn_propagate_workspace_bytes(B, H, W, int(T), _dt(d0), 0)
    work = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
    log = _sampled_log()
    with _device_guard(dev):
        if log is not None:
            ev0, ev1 = log.pair()
            ev0.record(torch.cuda.current_stream(dev))
        ok = L.cspn_propagate_scored(_p(w), _dt(w), _p(d0), _p(sparse), _p(out), _p(work), _dt(d0), B, H, W,
                                     int(valid_w), int(K), int(T), int(blend), _p(target), _p(acc), int(acc.shape[0]),
                                     _plan_ptr(K, plan), _stream(dev))
        if log is not None:
            ev1.record(torch.cuda.current_stream(dev))
            key = (K, B, H, W, T, False, id(plan))
            if key not in log.plan_cache:
                log.plan_cache[key] = resolve_plan(K, B, H, W, T, False, plan)["steps_per_launch"]
            S = log.plan_cache[key]
            log.append((ev0, ev1, -(-int(T) // max(S, 1)), S))
    _lib.check(ok, "cspn_propagate_scored")
    return out


def from_guidance_supported(guidance, d0, sparse, plan=None):
    """The fused prepare+propagate entry needs whole, 16-byte aligned quads (W % 4 == 0) and a vector plan."""
    W = guidance.shape[-1]
    forced = plan if plan is not None else _DEFAULT_PLANS.get(3)
    if forced is not None:      # explicit plan: must resolve to one of the from-guidance kernel instances
        if isinstance(forced, str):
            return False
        B, _, H, _ = guidance.shape
        try:
            p = resolve_plan(3, B, H, W, 1, False, forced)
        except RuntimeError:
            return False
        if p["force_scalar"] or (p["quads_per_thread"], p["threads"]) not in _FROM_GUIDANCE_INSTANCES:
            return False
    tensors = [t for t in (guidance, d0, sparse) if t is not None]
    return (W % 4 == 0 and guidance.is_contiguous() and guidance.stride(0) % 4 == 0 and guidance.stride(1) % 4 == 0
            and all(t.data_ptr() % 16 == 0 for t in tensors))


def propagate_from_guidance(guidance, d0, sparse, T, blend, keep_history=False, plan=None, publish_weights=True,
                            score=None, valid_w=0, return_weights=False):
    """3x3 variant without a prepare pass: every launch derives the normalised weights from `guidance`
    (cspn3_propagate_from_guidance).  fp32: same results, bit for bit, as cspn3_prepare + propagate, whatever the plan.
    fp16 storage is plan-dependent by construction: the deriving launch uses the unrounded fp32 weights for its S steps
    and keeps the state in fp32 inside a launch, later launches stream the fp16-rounded volume and the state is rounded
    to half between launches — results differ by fp16 rounding (<= 4e-3 of the range, the tolerance of the fp16 tests)
    between plans and from the prepare + propagate form.

    return_weights=True (the training forward) also returns the published tap volume and the normaliser S the
    first launch wrote: (d_T, history, w8, S)."""
    dev = _require_device(guidance, d0, sparse)
    B, C, H, W = guidance.shape
    if C < 8:
        raise ValueError("guidance must have >= 8 channels")
    g = guidance if guidance.is_contiguous() else guidance.contiguous()
    if not (d0.is_contiguous() and (sparse is None or sparse.is_contiguous())):
        raise ValueError("propagate_from_guidance: tensors must be contiguous")
    L = _lib.lib()
    T = int(T)
    hist = out = work = None
    if isinstance(plan, str):
        plan = None if plan != "auto" else _TUNED.get(("g3", B, H, W, T, g.dtype, d0.dtype, int(blend), dev.index))
    if keep_history and T > 0:
        hist = torch.empty((T, B, H, W), dtype=d0.dtype, device=dev)
    else:
        out = torch.empty((B, H, W), dtype=d0.dtype, device=dev)
        nbytes = L.cspn_propagate_workspace_bytes(B, H, W, T, _dt(d0), 0)
        if nbytes:
            work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    log = _sampled_log()
    with _device_guard(dev):
        if log is not None:
            ev0, ev1 = log.pair()
            ev0.record(torch.cuda.current_stream(dev))
        w8 = _weight_buffer(B, 8, H, W, g.dtype, dev) if (publish_weights or return_weights) else None
        S_out = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_weights else None
        tg, acc = score if score is not None else (None, None)
        ok = L.cspn3_propagate_from_guidance(_p(g), _dt(g), g.stride(0), g.stride(1), _p(w8), _p(S_out), _p(d0), _p(sparse), _p(out),
                                             _p(hist), _p(work), _dt(d0), B, H, W, int(valid_w), T, int(blend),
                                             _p(tg), _p(acc), 0 if acc is None else int(acc.shape[0]),
                                             _plan_ptr(3, plan), _stream(dev))
        if log is not None:
            ev1.record(torch.cuda.current_stream(dev))
            S = resolve_plan(3, B, H, W, T, keep_history, plan)["steps_per_launch"]
            log.append((ev0, ev1, -(-T // max(S, 1)), S))
    _lib.check(ok, "cspn3_propagate_from_guidance")
    res = (hist[T - 1], hist) if hist is not None else (out, None)
    return res + (w8, S_out) if return_weights else res


# ------------------------------------------------------------------------------------------------ resident forward
# cspn3_forward_resident (include/cspn_hip.h): ONE launch per chunk of whole images, weights resident in registers for
# all T steps, tile borders exchanged between co-resident workgroups.  Its launches must not overlap on a device, so
# this module serialises them: a lock around (order after the previous resident launch's stream, launch), per device.
#
# Reader's map of the host protocol below (it is the largest part of this file; each piece has one job):
#   _resident_state(dev)      per-device dict (_new_state: every key, with its neutral value): launch lock, workspaces per shape,
#                             sequence number, the pinned error / completion words the kernels write (host_err), the journal
#   _issue(...)               the ONE locked issue sequence: error word looked at first (-> _recover), workspace and stream ordering,
#                             sequence number, event-log pair, the C call, then either a count (guarded) or a journal entry
#   _resident_launch(...)     the general way into _issue: sampling decision, HIP-graph capture, lock, device switch, the check of
#                             the C entry's answer.  _ScoredFast.issue (cspn3_refine_and_score) is the lean way in
#   guard (plan.guard)        device side, csrc/cspn_repair.hip: a timed-out call is re-computed on the stream before anything can
#                             read it — every unscored call (_guard_default is the rule); such launches leave NO host state behind
#   _JournalEntry / _journal_add / _recover    host side, for what carries no guard (the scored forward by default, anything with
#                             set_resident_guard(False)): weak references to a call's tensors + how to redo it; _recover re-runs
#                             exactly the entries whose output holds the poison pattern, or raises for training forms
#   ensure_resident_ok / check_resident_errors / _check_resident_at_end_of_backward / _ResidentCheckpoint
#                             the host-side touch-points where the error word is looked at (metric gather, graph replays, the
#                             end of an UNGUARDED backward pass)
#   forward_resident, transposed_resident(_guidance), pac_forward_resident(_history), pac_transposed_resident
#                             one thin function per C entry: outputs, plan, the launch closure, one _resident_launch (_redo3: the
#                             3x3 repair closure, also the lean path's; _kxk_workspace: the workspace of the K x K entries)
_RESIDENT_MODE = os.environ.get("CSPN_RESIDENT", "auto")      # "auto" | "on" | "off"
_RES = {}                 # device index -> state dict (each with its OWN launch lock: devices never serialise each other)
_RES_NEW_LOCK = threading.Lock()      # guards the creation of a device's state only
# A resident launch whose workgroups were not co-resident (another tenant held CUs past the bounded wait) leaves NaN tiles and
# an error word.  Inference calls are REPAIRED, not raised: every resident inference launch is journaled (inputs, outputs) and
# when the error word turns up — at the next launch on the device or wherever the host is about to trust a result
# (ensure_resident_ok: metric gather / finalise, GraphedForward) — the journaled calls are re-run on the multi-launch
# schedule into the SAME output tensors (bit-identical by construction) and fused metric sums are corrected.  After
# _FALLBACK_LIMIT such events mode "auto" switches itself off for the process with one warning.  The reference's runtime
# surfaces worker errors and never returns partial results (network/libs/base/encoding.py:172-174, :193-194); a co-residency
# time-out is not an error of the computation, so it is absorbed where that can be done exactly, and raised (as a
# ResidentLaunchTimeout, after switching "auto" off so that a retry succeeds) where it cannot: training-form launches, whose
# results were consumed on the GPU before the host could know, and HIP-graph replays.
_JOURNAL_MAX = 32
_FALLBACK_LIMIT = 3
_FALLBACKS = 0
_FALLBACK_WARNED = False


class ResidentLaunchTimeout(RuntimeError):
    """A weight-resident launch gave up waiting for a neighbouring tile and its result could not be repaired in place (a
    training step, a HIP-graph replay, or more than _JOURNAL_MAX unchecked launches ago).  Mode "auto" has been switched off
    for this process: re-running the step takes the multi-launch schedule."""


def resident_fallbacks():
    """Number of times a timed-out resident launch was detected in this process (repaired in place or raised)."""
    return _FALLBACKS
# Flag values of one call span seq+1 .. seq+n_phase-1 (a tile that finished phase p publishes seq + p + 1) and the engine
# refuses more than 255 phases, so a step of 256 keeps the values of consecutive calls on one workspace disjoint
# (include/cspn_hip.h: "grows by at least 256").
_RES_SEQ_STEP = 256
_RES_SEQ_MAX = (1 << 31) - 4096
_RESIDENT_SPIN_LIMIT = 0   # test hook: polls before a neighbour wait gives up (0 = the engine's default, ~seconds)
# The guard (include/cspn_hip.h: cspn_resident_plan.guard): plain inference calls — whose result goes to a consumer this package
# does not know (a loss, a .cpu(), an image writer) — carry a device-side repair behind the resident launch, so that a timed-out
# launch is re-computed ON THE STREAM before anything can read it; so do the training forms (3x3, unet_ours, K = 5 fp16: no host
# wait at the end of backward).  The scored calls (consumer = this package's metric gather, which repairs on the host first) do
# not by default.  Costs one empty launch (~2 us); CSPN_RESIDENT_GUARD=0 or set_resident_guard(False) for A/B runs.
# "all" (CSPN_RESIDENT_GUARD=all): the scored forward carries the guard as well (its re-computation also adds the metric terms of
# the pixels the failed launch left unscored) — for a host that hands the refined depth of forward_scored to other GPU work before it
# gathers the metrics; it costs the headline path the same 1-2 us per call, which is why it is not the default.
_RESIDENT_GUARD = {"0": False, "all": "all"}.get(os.environ.get("CSPN_RESIDENT_GUARD", "1"), True)
_GUARD_MAX_T = 54
_GUARDED_HISTORY_FORMS = frozenset(((3, torch.float32), (5, torch.float16)))      # (K, guidance dtype) of the K x K training forwards that have a guard kernel


def set_resident_guard(enabled):
    """True (default): every unscored resident call carries the device-side guard; "all": the scored forward too; False: none."""
    global _RESIDENT_GUARD
    _RESIDENT_GUARD = "all" if enabled == "all" else bool(enabled)


def _guard_default(halo, policy="plain"):
    """Does a call carry the device-side guard when its caller does not say (1 / 0)?  halo: what the re-computation needs around a
    tile, which must fit the guard kernel's LDS tile — T pixels for the 3x3 entries, T * (K // 2) for the K x K ones; policy: "plain"
    = whenever the switch is on (every unscored call), "scored" = only under set_resident_guard("all") (the 3x3 scored forward),
    "never" (the K x K scored forward, a history form outside _GUARDED_HISTORY_FORMS)."""
    switch = _RESIDENT_GUARD
    return int(bool(switch) and halo <= _GUARD_MAX_T and (policy == "plain" or (policy == "scored" and switch == "all")))


def set_resident(mode):
    """"auto" (default): the weight-resident single-launch forward serves the no-grad 3x3 calls it fits and pays for;
    "on": whenever it fits; "off": never (always the multi-launch schedule).  Results are bit-identical either way."""
    global _RESIDENT_MODE
    if mode not in ("auto", "on", "off"):
        raise ValueError("set_resident: mode must be 'auto', 'on' or 'off'")
    _RESIDENT_MODE = mode


def _plan_copy(cp=None, **fields):
    """A new ctypes plan: a copy of `cp` (None: all zero) with `fields` set."""
    c2 = _lib.cspn_resident_plan()
    if cp is not None:
        ctypes.memmove(ctypes.byref(c2), ctypes.byref(cp), ctypes.sizeof(c2))
    for name, value in fields.items():
        setattr(c2, name, value)
    return c2


def _ctypes_plan(plan_dict):
    """The ctypes plan of a plan dict (resident_plan / kres_plan); None stays None.  debug_stamps is a per-call probe, not part of a plan."""
    if plan_dict is None:
        return None
    return _plan_copy(**{name: plan_dict[name] for name, _ in _lib.cspn_resident_plan._fields_ if name != "debug_stamps"})


def resident_plan(B, H, W, T, blend=0, n_cu=0, steps_per_phase=0, threads=0):
    """The tiling cspn3_forward_resident would use (dict), or None when the shape has none (W % 4 != 0, T < 1, ...).
    threads: 0 / 512 = the 512-thread workgroups, 1024 = one quad per thread on 1024 threads (inference forms only), 768 = three
    quads per thread on regions clipped to the image (inference forms only; `tile_h` is then the FIRST tile row's height)."""
    rp = _plan_copy(steps_per_phase=int(steps_per_phase), threads=int(threads))
    ok = _lib.lib().cspn3_resident_plan(int(B), int(H), int(W), int(T), int(blend), int(n_cu), ctypes.byref(rp))
    if not ok:
        return None
    return {name: getattr(rp, name) for name, _ in _lib.cspn_resident_plan._fields_}


def _new_state(host_err, n_cu):
    """A device's state: EVERY key this module uses, at its neutral value (needs no device: host_err is any int32 [4] tensor).
    last_*: the newest launch; journal / lost / marks / mark_pool / jcount: _journal_add; guarded_pending: launches since the last
    clean check that carried their own guard; need_bwd_check: an unguarded training-form launch awaits the end of backward."""
    return dict(seq=_RES_SEQ_STEP, work={}, host_err=host_err, host_err_np=host_err.numpy(),
                host_err_ptr=ctypes.c_void_p(host_err.data_ptr()), dirty=False, last_stream=None, last_raw=None, n_cu=n_cu,
                lock=threading.RLock(), journal=[], lost=False, last_seq=None, last_reports=False, marks=[], mark_pool=[],
                jcount=0, guarded_pending=0, need_bwd_check=False)


def _resident_state(dev):
    st = _RES.get(dev.index)
    if st is None:
        with _RES_NEW_LOCK:
            st = _RES.get(dev.index)
            if st is None:
                st = _RES[dev.index] = _new_state(torch.zeros(4, dtype=torch.int32).pin_memory(),
                                                  torch.cuda.get_device_properties(dev).multi_processor_count)
    return st


def _note_fallback(training=False):
    """Count a detected time-out and say so — every time, in every mode (a silent repair hides a mis-shared GPU) —
    and switch mode "auto" off after _FALLBACK_LIMIT of them (at once for a training-form launch: the step that raised is about
    to be retried)."""
    global _FALLBACKS, _RESIDENT_MODE, _FALLBACK_WARNED
    import warnings
    _FALLBACKS += 1
    if _RESIDENT_MODE == "auto" and (training or _FALLBACKS >= _FALLBACK_LIMIT):
        _RESIDENT_MODE = "off"
        if not _FALLBACK_WARNED:
            _FALLBACK_WARNED = True
            warnings.warn("cspn_monodepth_amd: %d weight-resident launch(es) timed out waiting for co-residency (the GPU is shared "
                          "with another tenant); the resident schedule is switched off for this process — results are unchanged, "
                          "calls take the multi-launch schedule from now on (functional.set_resident('auto') re-enables it)"
                          % _FALLBACKS, RuntimeWarning, stacklevel=3)
            return
    warnings.warn("cspn_monodepth_amd: weight-resident launch time-out #%d on this process (the GPU is shared with another tenant, so "
                  "the launch's workgroups were not co-resident): the affected inference results are re-computed on the multi-launch "
                  "schedule (same bits); until that repair their missing tiles read as NaN — see functional.set_resident('safe' / 'off')"
                  % _FALLBACKS, RuntimeWarning, stacklevel=3)


POISON_F32, POISON_F16 = 0x7fc0dead, 0x7ead      # include/cspn_hip.h: CSPN_POISON_F32 / CSPN_POISON_F16


def _holds_poison(t):
    """Does `t` hold the NaN pattern a tile that gave up writes (CSPN_POISON_*)?  Exact: no arithmetic produces that payload, so a
    NaN the recurrence itself produced (0/0 at an all-zero gate pixel, as in the reference) is not mistaken for a failed tile."""
    return bool(_poison_mask(t).any())


def _poison_mask(t):
    return (t.view(torch.int32) == POISON_F32) if t.dtype == torch.float32 else (t.view(torch.int16) == POISON_F16)


class _WeakT(object):
    """A tensor of an old journal entry, held WEAKLY (through the tensor object that owns the storage: a view made inside this
    package dies with the call, its base is the caller's) — enough to rebuild the same view if the caller still has it."""
    __slots__ = ("ref", "size", "stride", "off")

    def __init__(self, t):
        base = t._base if t._base is not None else t
        self.ref, self.size, self.stride, self.off = weakref.ref(base), t.size(), t.stride(), t.storage_offset()

    def get(self):
        base = self.ref()
        return None if base is None else torch.as_strided(base, self.size, self.stride, self.off)


_NO_VERSION = object()      # an inference tensor: no version counter to compare


def _tensor_version(t):
    """t._version, or _NO_VERSION for tensors made under torch.inference_mode() (reading their counter raises; ADVICE r5: every
    unguarded launch — the default scored forward among them — builds a journal entry, so eval under inference_mode crashed AFTER
    the kernel had been enqueued).  Such an input cannot be checked for in-place modification: the repair trusts it, as it must
    trust any tensor whose storage was rewritten through another view."""
    if t is None:
        return None
    try:
        return t._version
    except RuntimeError:
        return _NO_VERSION


class _JournalEntry(object):
    """One resident launch that may still turn out to have timed out.  redo(out, *inputs): re-runs the call on the multi-launch
    schedule into `out` (None: a training-form launch / anything that cannot be repaired after the fact); out: the tensor a
    failed tile poisons; inputs: the tensors the repair would read, with their version counters at launch time — a repair from
    inputs the caller has since overwritten in place would silently produce the result of ANOTHER batch.
    The newest entries hold their tensors strongly (the failing call is found at the NEXT launch, when an eval loop has already
    rebound its variables to the next batch); older ones are demoted to weak references (`demote`): a journal of unchecked
    launches then pins at most _JOURNAL_STRONG_BYTES of the caller's tensors, and a late repair happens only if they still exist."""
    __slots__ = ("redo", "out", "inputs", "versions", "nbytes", "what", "weak")

    def __init__(self, redo, out=None, inputs=(), what="resident launch", nbytes=None):
        self.redo, self.out, self.what, self.weak = redo, out, what, False
        # a launch that cannot be repaired after the fact (redo None: the training forms) needs no inputs, and holds its output —
        # the plane a tile that gave up poisons — weakly from the start: such an entry pins nothing of the caller's
        self.inputs = tuple(inputs) if redo is not None else ()
        self.versions = tuple(_tensor_version(t) for t in self.inputs)
        self.nbytes = nbytes if nbytes is not None else (
            sum(t.numel() * t.element_size() for t in self.inputs if t is not None) + (0 if out is None else out.numel() * out.element_size()))
        if redo is None:
            self.nbytes = 0
            self.demote()

    def demote(self):
        if not self.weak:
            self.out = None if self.out is None else _WeakT(self.out)
            self.inputs = tuple(None if t is None else _WeakT(t) for t in self.inputs)
            self.weak = True

    def resolve(self):
        """(out, inputs) as tensors; out None = the caller dropped it (nobody can read it: nothing to repair), inputs None = one of
        them is gone (cannot be repaired)."""
        if not self.weak:
            return self.out, self.inputs
        out = None if self.out is None else self.out.get()
        ins = tuple(None if t is None else t.get() for t in self.inputs)
        if any(t is None and w is not None for t, w in zip(ins, self.inputs)):
            ins = None
        return out, ins

    def untouched(self, ins):
        return all(t is None or v is _NO_VERSION or _tensor_version(t) == v for t, v in zip(ins, self.versions))


def _recover(dev, st):
    """The error word of `dev` is set: wait for the journaled launches, clear the word, and re-run — on the multi-launch schedule,
    into their own output tensors — exactly the journaled inference calls whose output holds the poison pattern of a tile that gave
    up.  Calls that finished cleanly are left alone (their inputs may have been reused since).  Raises ResidentLaunchTimeout
    when a launch that cannot be repaired is among the suspects: a training-form launch, a graph replay, a journal that overflowed
    since the last clean check, or a failed call whose inputs were modified in place after the launch."""
    with st["lock"]:
        if st["host_err_np"][0] == 0:
            return
        last = st["last_stream"]
        if last is not None and not torch.cuda.is_current_stream_capturing():
            last.synchronize()                     # every journaled launch has finished: its outputs may be rewritten
        st["host_err_np"][0] = 0
        st["dirty"] = False
        # launches that carried their own guard (cspn_resident_plan.guard) left no entry: if it was one of them, its guard kernel has
        # re-computed the result on the stream already
        journal, lost, repaired = list(st["journal"]), st["lost"], st["guarded_pending"]
        _journal_clear(st)
        stale, training = [], False
        with _device_guard(dev):
            for e in journal:
                if e.redo is None:
                    # an unguarded training-form launch: decided per entry, as the inference entries are (one CLEAN
                    # training entry in the journal turned a guarded — already repaired — time-out of another launch into a raise).
                    # Its `out` is the plane a tile that gave up poisons (d_T / G_0), held weakly.  Alive and clean: this launch
                    # finished.  Freed — the reverse sweep's history dies with `backward`, AFTER the tail has read it on the GPU — or
                    # never recorded: cannot tell, so it counts as failed (gradients built on it may already be in .grad).
                    tout = e.out.get() if isinstance(e.out, _WeakT) else e.out
                    if tout is None or _holds_poison(tout):
                        training = True
                    continue
                out, ins = e.resolve()
                if out is None or not _holds_poison(out):
                    continue                       # finished cleanly — or the caller dropped the result: nobody can read it
                if ins is None:
                    stale.append(e.what + " (its input tensors no longer exist)")
                    continue
                if not e.untouched(ins):
                    stale.append(e.what)
                    continue
                e.redo(out, *ins)
                repaired += 1
        _note_fallback(training=training)
        # (nothing repaired and nothing wrong with the journal: the failed call's result was dropped by its caller, or its guard
        #  kernel has dealt with it — the event is counted and warned about, there is nothing to raise)
        if lost or training or stale:
            why = ("a training-form launch" if training else
                   "the inputs of the failed call (%s) were modified in place (or freed) before the time-out was detected" % ", ".join(stale) if stale
                   else "graph replay / unchecked launches beyond the journal")
            raise ResidentLaunchTimeout(
                "a weight-resident launch on cuda:%d timed out waiting for a neighbouring tile (the GPU was shared with another "
                "long-running tenant, so the launch was not co-resident) and its result cannot be repaired in place (%s); the "
                "output of that call is incomplete (its missing tiles are NaN).  The resident schedule is now off for this "
                "process (functional.set_resident): re-run the step." % (dev.index, why))


_JOURNAL_STRONG_BYTES = 256 << 20     # tensors of unchecked launches held strongly (the newest entries; at least the last two)


def _journal_demote(j):
    """Demote what the newest entries of journal `j` (a list, oldest first) push past _JOURNAL_STRONG_BYTES: a walk from the newest
    entry back, up to the first inference entry an earlier walk demoted.  Training-form entries (redo None: weak from birth, holding
    nothing) are passed over — one of them between strong inference entries must not end the walk and keep the older ones pinned."""
    strong = 0
    for k in range(len(j) - 1, -1, -1):
        e = j[k]
        if e.redo is None:
            continue
        if e.weak:
            break
        strong += e.nbytes
        if k < len(j) - 2 and strong > _JOURNAL_STRONG_BYTES:
            e.demote()


def _journal_clear(st):
    del st["journal"][:]
    st["lost"] = False
    st["guarded_pending"] = 0
    st["mark_pool"].extend(ev for _, ev in st["marks"])
    st["marks"] = []


def _journal_add(dev, st, entry, stream):
    """Remember how to repair the launch just issued on `stream`.  The journal never loses an entry that may still fail: every
    16th launch records an event behind itself, every add drops what lies before the marks that have completed (a poll, no
    wait), and a full journal waits for its oldest mark (16+ launches back: normally long finished).  It does not pin the
    caller's memory either (32 unchecked config-2 batches were 2.5 GB): only the newest entries — the last two, and
    as many more as fit _JOURNAL_STRONG_BYTES — hold their tensors; older ones are demoted to weak references.  (A mark per
    64 MB was tried first: an event record between two kernels costs ~2 us of stream time — config 3 read 76.8 instead of 72 us
    per scored forward.)"""
    j = st["journal"]
    j.append(entry)
    _journal_demote(j)
    st["jcount"] = n = st["jcount"] + 1
    marks = st["marks"]
    if n % 16 == 0:
        pool = st["mark_pool"]
        ev = pool.pop() if pool else torch.cuda.Event()
        ev.record(stream)
        marks.append([len(j), ev])
    if marks and st["host_err_np"][0] == 0:
        cut = 0
        while marks:
            c, ev = marks[0]
            if not ev.query():
                if len(j) - cut < _JOURNAL_MAX:
                    break
                ev.synchronize()                   # a full journal waits for its oldest mark
            marks.pop(0)
            st["mark_pool"].append(ev)
            cut = c
        if cut and st["host_err_np"][0] == 0:      # everything up to the mark has finished cleanly
            del j[:cut]
            for m in marks:
                m[0] -= cut
    if st["host_err_np"][0] != 0:
        _recover(dev, st)


def _device_is_oversubscribed():
    """More ranks of this job than GPUs on the node (torchrun's LOCAL_WORLD_SIZE): several processes share a device, and
    their resident launches could starve each other — mode "auto" then keeps to the multi-launch schedule."""
    try:
        return int(os.environ.get("LOCAL_WORLD_SIZE", "1")) > max(torch.cuda.device_count(), 1)
    except ValueError:
        return False


_RES_PLAN_CACHE = {}      # (B, H, W, T, blend, device index, mode) -> (plan dict | None, ctypes plan | None)


def _resident_plan_cached(B, H, W, T, blend, dev):
    key = (B, H, W, T, blend, dev.index, _RESIDENT_MODE)
    hit = _RES_PLAN_CACHE.get(key)
    if hit is None:
        n_cu = _resident_state(dev)["n_cu"]
        if _RESIDENT_MODE == "on":
            rp = resident_plan(B, H, W, T, blend, n_cu)
        else:
            rp = None if _device_is_oversubscribed() else resident_pays(B, H, W, T, blend, dev)
        if len(_RES_PLAN_CACHE) > 1024:
            _RES_PLAN_CACHE.clear()
        hit = _RES_PLAN_CACHE[key] = (rp, _ctypes_plan(rp))
    return hit


_RES_SCORED_PLAN_CACHE = {}      # (id of the default ctypes plan, B, H, W, T, blend) -> ctypes plan of the scored call
_CLIPPED_SCORED = os.environ.get("CSPN_RESIDENT_CLIPPED", "1") != "0"      # A/B switch: "0" keeps the scored calls on the default plan


def _scored_plan(cp, B, H, W, T, blend, dev):
    """The plan of a scored inference call whose default plan is `cp`: the clipped 768-thread plan (three wavefronts per SIMD) where
    it does less work per SIMD than the default — one launch either way, and a default of more than 3 quads per thread, i.e.
    tiles whose halo the image edge makes partly unnecessary; config 2 is the measured case (profiles/r07_clipped_ab.txt).  Shards
    and multi-launch batches (NYU B = 3, KITTI B = 1 / 8) keep `cp`."""
    if cp is None or not _CLIPPED_SCORED or cp.launches != 1 or cp.quads_per_thread <= 3 or cp.threads != 512:
        return cp
    key = (id(cp), B, H, W, T, blend)
    hit = _RES_SCORED_PLAN_CACHE.get(key)
    if hit is None or hit[0] is not cp:
        rp = resident_plan(B, H, W, T, blend, _resident_state(dev)["n_cu"], threads=768)
        c2 = cp
        if rp is not None and rp["launches"] == 1 and rp["steps_per_phase"] == cp.steps_per_phase:
            c2 = _ctypes_plan(rp)
        if len(_RES_SCORED_PLAN_CACHE) > 256:
            _RES_SCORED_PLAN_CACHE.clear()
        hit = _RES_SCORED_PLAN_CACHE[key] = (cp, c2)
    return hit[1]


def resident_pays(B, H, W, T, blend, dev):
    """Policy of mode "auto": the resident launch needs enough tiles to occupy the chip (one workgroup per CU) and a
    halo overhead that the saved weight passes pay for."""
    rp = resident_plan(B, H, W, T, blend, _resident_state(dev)["n_cu"])
    if rp is None:
        return None
    # measured on MI355X (tools/bench_resident.py -> profiles/r02_resident_vs_multilaunch.jsonl): the resident schedule beats
    # the three-launch one by 35 % at config 2, ~32 % when the batch needs two resident launches (KITTI B=8, NYU B=48),
    # 25-29 % with four and eight (NYU B=96 / 192, KITTI B=32: tools/probes/bench_resident_big.py) and 25-40 % on per-GPU shards
    # (B <= 6): every launch refines whole images, so the gain does not depend on their number; only extreme halo
    # overheads are left to the multi-launch schedule
    if rp["region_over_tile"] > 3.6:
        return None
    return rp


def resident_supported(guidance, d0, sparse, T, plan=None, target=None):
    """Can this no-grad 3x3 forward take the weight-resident launch?  (fp32, whole 16-byte quads, no explicit plan.)"""
    if _RESIDENT_MODE == "off" or plan is not None or _DEFAULT_PLANS.get(3) is not None or T < 1:
        return None
    if guidance.dtype != torch.float32 or d0.dtype != torch.float32 or not from_guidance_supported(guidance, d0, sparse, None):
        return None
    if target is not None and (target.dtype != torch.float32 or target.data_ptr() % 16):
        return None
    B, H, W = d0.shape
    if guidance.stride(1) >= (1 << 27) or H * W >= (1 << 27):
        return None                                        # the kernel addresses an image with 32-bit element offsets
    return _resident_plan_cached(B, H, W, int(T), int(sparse is not None), guidance.device)[0]


def check_resident_errors(dev=None):
    """If a resident launch on `dev` (default: every device used so far) gave up waiting for a neighbouring tile — its workgroups
    were not co-resident because something else held the GPU — repair the journaled inference calls in place (see the note at
    the top of this section), or raise ResidentLaunchTimeout when that is not possible.  Only sees the error words of launches
    that have FINISHED: call it after a synchronisation that covers them, or use ensure_resident_ok, which synchronises first.
    Called at the start of every resident launch, by ensure_resident_ok, and at the end of a backward pass."""
    for idx, st in list(_RES.items()):
        if (dev is None or dev.index == idx) and st["host_err_np"][0] != 0:
            _recover(torch.device("cuda", idx), st)


def ensure_resident_ok(dev=None):
    """Wait for the resident launches issued so far on `dev` (default: every device) and make their results trustworthy: a
    launch that timed out is re-run on the multi-launch schedule (same bits, fused metric sums corrected), or raised as a
    ResidentLaunchTimeout when it cannot be (training form, graph replay).  This is what every consumer of a result on the
    host calls before it trusts the numbers — evaluation.all_gather_metric_sums / finalize_metrics do; a training step gets
    the equivalent at the end of its backward pass (CSPN3Function.backward).  Costs nothing when no resident launch is pending
    (no synchronisation then)."""
    for idx, st in list(_RES.items()):
        if dev is not None and dev.index != idx:
            continue
        if st["dirty"]:
            last = st["last_stream"]
            if last is not None and not torch.cuda.is_current_stream_capturing():
                last.synchronize()
            st["dirty"] = False
        if st["host_err_np"][0] != 0:
            _recover(torch.device("cuda", idx), st)
        elif st["journal"] or st["guarded_pending"]:
            with st["lock"]:
                if st["host_err_np"][0] == 0 and not st["dirty"]:      # everything issued so far has finished cleanly
                    _journal_clear(st)


def mark_resident_pending(t=None):
    """A HIP-graph replay may have run resident launches this module did not see: make the next ensure_resident_ok on
    that device wait for its stream."""
    dev = t.device if t is not None and t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    st = _RES.get(dev.index)
    if st is not None:
        st["dirty"] = True
        st["last_stream"] = torch.cuda.current_stream(dev)
        st["last_raw"] = st["last_stream"].cuda_stream
        st["lost"] = True                 # a replayed launch cannot be re-run from here: a time-out inside it raises
        st["last_seq"] = None             # (and a pending end-of-backward checkpoint must not poll for a captured seq)


class _ResidentCheckpoint(object):
    """A mark behind the resident launches issued so far on a device.  `wait_and_check` waits until the LAST of them has
    finished and raises if one of them timed out — without a HIP call: the engine's launches store their sequence number
    to a pinned host word when their last workgroup has counted itself out (include/cspn_hip.h: host_err[1]), so the
    wait is a poll of host memory; nothing is recorded on the stream and whatever was enqueued later keeps running.
    (An event + hipEventSynchronize in every backward pass measured +40 us per CSPN forward/backward pair.)"""
    __slots__ = ("dev", "seq", "stream")

    def __init__(self, dev):
        self.dev = dev
        st = _resident_state(dev)
        self.seq = st["last_seq"]
        self.stream = st["last_stream"]

    def wait_and_check(self, budget_s=20.0):
        st = _resident_state(self.dev)
        if self.seq is not None:
            words = st["host_err_np"]
            t_end = None
            spins = 0
            while True:
                spins += 1
                if words[0] != 0:
                    break
                if ((int(words[1]) - self.seq) & 0xffffffff) < 0x80000000:      # done word has reached (or passed) this call
                    break
                if st["last_seq"] is None:               # a graph replay or a sequence wrap came in between: the completion
                    if self.stream is not None:          # word no longer counts this call's way — wait the plain way, at once
                        self.stream.synchronize()
                    break
                if spins > 2048:                         # past ~0.2 ms this is a stalled device, not the tail of a step: back
                    time.sleep(5e-5)                     # off and let other threads have the interpreter
                    if t_end is None:
                        t_end = time.perf_counter() + budget_s
                    elif time.perf_counter() > t_end:
                        if self.stream is not None:
                            self.stream.synchronize()
                        break
            if words[0] == 0 and st["last_reports"] and st["last_seq"] == self.seq:
                with st["lock"]:                         # the newest launch has finished cleanly: nothing is left to repair
                    if words[0] == 0 and st["last_seq"] == self.seq:
                        _journal_clear(st)
        check_resident_errors(self.dev)


def _issue(dev, st, raw, log, T, launch, args, reports_done, journal, work=None, ws=None):
    """The locked issue sequence of every resident launch: the caller holds st["lock"] and has `dev` current; raw: the current
    stream's handle; log: the event log if this call is sampled.  Error word first (a time-out of an earlier launch is repaired or
    raised there: _recover); the workspace ws = (B, H, W, kind, state bytes, bytes_fn | None) and the stream order — unless the
    caller hands in `work`: the lean path, whose bail-out test has settled both —; sequence number, event pair, the C call
    `launch(work, seq, host_err_ptr, raw, *args)`; then what the host keeps: journal = the _JournalEntry arguments of a call without
    the device-side guard, None for a guarded one (repaired on the stream: a count, no entry, no tensor kept alive)."""
    if st["host_err_np"][0] != 0:
        _recover(dev, st)                               # repairs the journaled calls, or raises
    if work is not None:
        cur = st["last_stream"]
    else:
        work = st["work"].get(ws[:5])
        if work is None:
            if len(st["work"]) > 16:                    # (more than 16 shapes: start the cache over — behind whatever still uses it)
                if st["last_stream"] is not None:
                    st["last_stream"].synchronize()
                st["work"].clear()
            nbytes = ws[5]() if ws[5] is not None else _lib.lib().cspn3_resident_workspace_bytes(*ws[:3])
            work = st["work"][ws[:5]] = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
        if raw == st["last_raw"]:
            cur = st["last_stream"]
        else:
            cur = torch.cuda.current_stream(dev)
            last = st["last_stream"]
            if last is not None and last != cur:
                cur.wait_stream(last)                   # resident launches never overlap on a device
        if st["seq"] > _RES_SEQ_MAX:                    # flag values wrap: start over on clean workspaces (zeroed on `cur`,
            for w_ in st["work"].values():              # behind every earlier resident launch)
                w_.zero_()
            st["seq"] = _RES_SEQ_STEP
            cur.synchronize()                           # (once per ~8 M calls) the completion word starts over as well
            st["host_err_np"][1] = 0
            st["last_seq"] = None                       # ... and a pending checkpoint of the old numbering waits the plain way
    seq = st["seq"]
    st["seq"] = seq + _RES_SEQ_STEP
    if log is not None:
        ev0, ev1 = log.pair()
        ev0.record(cur)
    ok = launch(work, seq, st["host_err_ptr"], raw, *args)
    if log is not None:
        ev1.record(cur)
        log.append((ev0, ev1, 1, T))
    if ok:                                              # (a call that failed at submit has enqueued nothing)
        st["last_stream"] = cur
        st["last_raw"] = raw
        st["dirty"] = True
        st["last_reports"] = reports_done
        if reports_done:                                # training-form launches store `seq` to the completion word
            st["last_seq"] = seq
            if journal is not None:                     # ... and an unguarded one must be looked at by the end-of-backward check
                st["need_bwd_check"] = True
        if journal is None:
            st["guarded_pending"] += 1
        else:
            _journal_add(dev, st, _JournalEntry(*journal), cur)
    return ok


def _resident_launch(dev, B, H, W, T, launch, name, ws=("3", 4, None), reports_done=False, redo=None, out=None, inputs=(), guarded=False):
    """The general way into _issue, for the C entry `name`: one launch at a time per device (the device's own lock), on a
    zero-initialised workspace per (B,H,W) and `ws` = (kind, bytes per state element, bytes_fn | None: the 3x3 engine's size).
    `launch(work, seq, host_err_ptr, stream_ptr)` makes the C call — a falsy answer raises under `name` —; `redo()` re-runs the call
    on the multi-launch schedule into the same outputs (None: the launch cannot be repaired — training forms).

    Under HIP-graph capture a replay cannot bring a new sequence number, so the capture records a memset of the
    workspace's control words (status + tile flags, a few KB behind the two exchange planes: include/cspn_hip.h) in front
    of the launch and uses a constant sequence number — every replay starts from zeroed flags.  The workspace comes from
    the graph's private pool (it lives as long as the graph).  Replays are ordered by their stream like any launch; the
    caller must not replay two graphs holding resident launches concurrently on one device (they could not both be
    co-resident: the bounded wait would flag it)."""
    log = _sampled_log()
    idx = dev.index
    if torch._C._cuda_isCurrentStreamCapturing():
        nbytes = ws[2]() if ws[2] is not None else _lib.lib().cspn3_resident_workspace_bytes(B, H, W)
        work = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        work[(2 * B * H * W * ws[1] + 15) & ~15:].zero_()
        st = _resident_state(dev)
        with _device_guard(dev):
            cur = torch.cuda.current_stream(dev)
            return _lib.check(launch(work, _RES_SEQ_STEP, st["host_err_ptr"], cur.cuda_stream), name)
    st = _RES.get(idx) or _resident_state(dev)
    journal = None if guarded else (redo, out, inputs, "%s %dx%dx%d" % (name, B, H, W))
    with st["lock"]:
        # (this function is most of the host time of a small call: no context-manager object when `dev` is current already, raw
        #  stream handles, no journal entry for a launch that carries its own guard — tools/probes/r05_host_timing_train.py)
        ctx = None if torch._C._cuda_getDevice() == idx else torch.cuda.device(dev)
        if ctx is not None:
            ctx.__enter__()
        try:
            ok = _issue(dev, st, torch._C._cuda_getCurrentRawStream(idx), log, T, launch, (), reports_done, journal, None, (B, H, W) + ws)
        finally:
            if ctx is not None:
                ctx.__exit__(None, None, None)
    _lib.check(ok, name)


def _with_spin_limit(cp, step_form=0, guard=0):
    """The cached ctypes plan, or a copy carrying the test hook's spin limit / a pinned step form / the guard flag."""
    if (not _RESIDENT_SPIN_LIMIT and not step_form and not guard) or cp is None:
        return cp
    if guard and not _RESIDENT_SPIN_LIMIT and not step_form:      # the common case: one guarded copy per cached plan
        c2 = getattr(cp, "_guarded", None)
        if c2 is None:
            c2 = cp._guarded = _plan_copy(cp, guard=1)
        return c2
    c2 = _plan_copy(cp, step_form=int(step_form), guard=int(guard))
    if _RESIDENT_SPIN_LIMIT:
        c2.spin_limit = int(_RESIDENT_SPIN_LIMIT)
    return c2


def _unscore_failed_launch(out, tg, acc):
    """A scored resident launch that timed out has added the sums of the tiles that DID finish to `acc` (the tiles that gave up
    return before their scoring; their part of `out` is NaN).  Take those sums out again, so that the re-run can score the whole
    batch exactly once: they are the metric sums over the finite part of the failed output."""
    from . import evaluation
    bad = _poison_mask(out)
    part = evaluation.metric_sums(torch.where(bad, torch.ones_like(out), out), torch.where(bad, torch.zeros_like(tg), tg))
    acc[0] -= part


def _redo3(B, H, W, T, blend, valid_w=0, acc=None):
    """The repair of a 3x3 inference call: the same call on the multi-launch schedule, into the same tensors (bit-identical: DESIGN.md
    §4.1b) — the journal hands them in (it may hold them weakly).  acc: the accumulator of a scored call, which is re-scored whole."""
    def redo(out, guidance, d0, sparse, tg):
        from . import evaluation
        tgp = None if tg is None else tg.reshape(B, H, W)
        if acc is not None:
            _unscore_failed_launch(out, tgp, acc)
        res, _ = propagate_from_guidance(guidance, d0.reshape(B, H, W), None if sparse is None else sparse.reshape(B, H, W), T, blend,
                                         valid_w=valid_w)
        out.copy_(res)
        if acc is not None:
            evaluation.metric_sums(out, tgp, out=acc)
    return redo


def _kxk_workspace(B, H, W, state_dt):
    """`ws` of _resident_launch for the K x K entries; state_dt: the dtype code of the exchange planes."""
    return "k", 2 if state_dt == CSPN_F16 else 4, lambda: _lib.lib().cspnk_resident_workspace_bytes(B, H, W, state_dt)


# (the plan argument of the C entries is the ctypes plan itself, or None: ctypes passes a structure by reference where the
#  signature says pointer, and None as NULL — the engine then finds its own plan)
def _transposed3(name, head, dev, g_T, sparse_f32, T, valid_w, _plan=None):
    """The 3x3 reverse sweep as one weight-resident launch per chunk, by the C entry `name`, whose arguments open with `head` (where
    the taps come from): ghist [T,B,H,W] (G_{T-1} .. G_0).  _plan: CSPN3Function's fast path, with the guarded plan in hand."""
    B, H, W = g_T.shape
    T, premask = int(T), int(sparse_f32 is not None)
    cfunc = getattr(_lib.lib(), name)
    guard = 1 if _plan is not None else _guard_default(T)
    rp = _plan if _plan is not None else _with_spin_limit(_resident_plan_cached(B, H, W, T, premask, dev)[1], guard=guard)
    ghist = torch.empty((T, B, H, W), dtype=torch.float32, device=dev)

    def launch(work, seq, host_err_ptr, stream_ptr):
        return cfunc(*head, _p(g_T), _p(sparse_f32), _p(ghist), _p(work), seq, host_err_ptr, B, H, W, int(valid_w), T, premask, rp, stream_ptr)

    _resident_launch(dev, B, H, W, T, launch, name, reports_done=True, guarded=bool(guard), out=ghist[T - 1])
    return ghist


def transposed_resident(w8, g_T, sparse_f32, T, valid_w=0):
    """Reverse sweep of the backward as one weight-resident launch per chunk: ghist [T,B,H,W] (G_{T-1} .. G_0)."""
    return _transposed3("cspn3_transposed_resident", (_p(w8),), _require_device(w8, g_T, sparse_f32), g_T, sparse_f32, T, valid_w)


def transposed_resident_guidance(guidance, S, g_T, sparse_f32, T, valid_w=0, _plan=None):
    """The same reverse sweep without a tap volume: the transposed taps |g_j[p]| / S[p + off_j] are rebuilt from the raw guidance
    and the normaliser S the training forward published (include/cspn_hip.h cspn3_transposed_resident_guidance)."""
    dev = guidance.device if _plan is not None else _require_device(guidance, S, g_T, sparse_f32)      # (fast path: validated with the forward)
    return _transposed3("cspn3_transposed_resident_guidance", (_p(guidance), guidance.stride(0), guidance.stride(1), _p(S)), dev, g_T,
                        sparse_f32, T, valid_w, _plan)


def pac_transposed_resident(wk, g_T, sparse, T, debug_stamps=None):
    """K = 5 reverse sweep on the forward's fp16 tap volume as weight-resident launches.  Returns (G_T as fp32 [B,H,W], ghist
    [T,B,H,W] f32 = G_{T-1} .. G_0).  The transposed taps are gathered once per launch and stay packed in registers; no
    transposed copy of the volume.  g_T / sparse: both fp32, or both fp16 (the kernel converts where it stages them and writes
    the fp32 G_T the tail reads: planes 0 and 1.. of one allocation)."""
    dev = _require_device(wk, g_T, sparse)
    B, H, W = g_T.shape
    L = _lib.lib()
    half_in = g_T.dtype == torch.float16
    if sparse is not None and sparse.dtype != g_T.dtype:
        raise ValueError("pac_transposed_resident: g_T and sparse must share a dtype")
    planes = torch.empty((int(T) + int(half_in), B, H, W), dtype=torch.float32, device=dev)
    g32, ghist = (planes[0], planes[1:]) if half_in else (g_T, planes)
    premask = int(sparse is not None)
    guard = _guard_default(int(T) * (5 // 2))
    rp = _with_spin_limit(_kres_plan_cached(5, B, H, W, int(T), premask, dev, 0, CSPN_F16)[1], guard=guard)
    if debug_stamps is not None and rp is not None:     # developer probe: in-kernel time stamps of round 0's workgroups [images_per_launch x tiles][16]
        rp = _plan_copy(rp, debug_stamps=debug_stamps.data_ptr())

    def launch(work, seq, host_err_ptr, stream_ptr):
        return L.cspnk_transposed_resident(_p(wk), CSPN_F16, 5, _p(g_T), _p(sparse), _dt(g_T), _p(g32) if half_in else None, _p(ghist),
                                           _p(work), seq, host_err_ptr, B, H, W, int(T), premask, rp, stream_ptr)

    _resident_launch(dev, B, H, W, int(T), launch, "cspnk_transposed_resident", _kxk_workspace(B, H, W, CSPN_F32), reports_done=True,
                     guarded=bool(guard), out=ghist[int(T) - 1])
    return g32, ghist


def forward_resident(guidance, d0, sparse, T, blend, score=None, valid_w=0, steps_per_phase=0, spin_limit=0, debug_stamps=None,
                     keep_history=False, publish_weights=True, guard=None, _plan=None, threads=0):
    """Refined depth [B,H,W] by the weight-resident launch; `score=(target, acc)` fuses the depth metrics into it.

    keep_history=True is the training forward: returns (d_T [view of history[T-1]], history [T,B,H,W], w8 [B,8,H,W],
    S [B,H,W]) — the launch writes every step's state to its history plane and publishes the weights and S once;
    publish_weights=False publishes S only (w8 is None): the backward rebuilds the taps from guidance and S."""
    dev = guidance.device
    if not guidance.is_cuda:
        _require_device(guidance, d0, sparse)          # raises
    B, C, H, W = guidance.shape
    L = _lib.lib()
    hist = w8 = S_out = out = None
    if keep_history:
        hist = torch.empty((int(T), B, H, W), dtype=torch.float32, device=dev)
        w8 = torch.empty((B, 8, H, W), dtype=torch.float32, device=dev) if publish_weights else None
        S_out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    else:
        out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    tg, acc = score if score is not None else (None, None)
    guard = _guard_default(int(T), "plain" if score is None else "scored") if guard is None else int(guard)
    if _plan is not None and not _RESIDENT_SPIN_LIMIT:
        rp = _plan                                     # the caller's cached (guarded) plan: CSPN3Function's fast path
    elif steps_per_phase or spin_limit or debug_stamps is not None or threads:
        rp = _plan_copy(steps_per_phase=int(steps_per_phase), threads=int(threads), spin_limit=int(spin_limit),
                        debug_stamps=None if debug_stamps is None else debug_stamps.data_ptr(), guard=guard)
    else:
        cp = _resident_plan_cached(B, H, W, int(T), int(blend), dev)[1]      # found once per shape: the C side skips its search
        if score is not None and not keep_history and not valid_w:
            cp = _scored_plan(cp, B, H, W, int(T), int(blend), dev)
        rp = _with_spin_limit(cp, guard=guard)

    def launch(work, seq, host_err_ptr, stream_ptr):
        return L.cspn3_forward_resident(_p(guidance), guidance.stride(0), guidance.stride(1), _p(d0), _p(sparse), _p(out),
                                        _p(hist), _p(w8), _p(S_out), _p(work), seq, host_err_ptr, B, H, W, int(valid_w),
                                        int(T), int(blend), _p(tg), _p(acc), 0 if acc is None else int(acc.shape[0]), rp, stream_ptr)

    # (a training-form launch cannot be repaired after the fact: its entry keeps no inputs, and the plane a tile that gave up poisons weakly)
    _resident_launch(dev, B, H, W, int(T), launch, "cspn3_forward_resident", reports_done=bool(keep_history),
                     redo=None if keep_history or guard else _redo3(B, H, W, T, blend, valid_w, acc),
                     out=hist[int(T) - 1] if keep_history else out, inputs=() if keep_history else (guidance, d0, sparse, tg),
                     guarded=bool(guard))
    if keep_history:
        return hist[int(T) - 1], hist, w8, S_out
    return out


# ------------------------------------------------------------------------------------------------ K x K resident forward
def kres_plan(K, B, H, W, T, blend=0, n_cu=0, steps_per_phase=0, threads=0, g_dtype=CSPN_F16):
    """The tiling cspnk_forward_resident would use (dict; `quads_per_thread` holds the OCTS per thread), or None.
    g_dtype: CSPN_F16 (packed taps) or CSPN_F32 (fp32 taps: fewer octs fit a thread)."""
    rp = _plan_copy(steps_per_phase=int(steps_per_phase), threads=int(threads))
    ok = _lib.lib().cspnk_resident_plan(int(K), int(g_dtype), int(B), int(H), int(W), int(T), int(blend), int(n_cu), ctypes.byref(rp))
    if not ok:
        return None
    return {name: getattr(rp, name) for name, _ in _lib.cspn_resident_plan._fields_}


_KRES_PLAN_CACHE = {}


def _kres_plan_cached(K, B, H, W, T, blend, dev, steps_per_phase=0, g_dtype=CSPN_F16):
    key = (K, B, H, W, T, blend, dev.index, _RESIDENT_MODE, steps_per_phase, g_dtype)
    hit = _KRES_PLAN_CACHE.get(key)
    if hit is None:
        rp = None
        if _RESIDENT_MODE == "on" or not _device_is_oversubscribed():
            rp = kres_plan(K, B, H, W, T, blend, _resident_state(dev)["n_cu"], steps_per_phase, 0, g_dtype)
        if len(_KRES_PLAN_CACHE) > 1024:
            _KRES_PLAN_CACHE.clear()
        hit = _KRES_PLAN_CACHE[key] = (rp, _ctypes_plan(rp))
    return hit


def pac_resident_supported(guided, x0, sparse, T, plan=None, target=None):
    """Can this no-grad K x K forward take the weight-resident launches?  fp16 guidance (the taps stay packed in registers) or
    fp32 guidance with fp32 planes (fp32 taps), K = 3 or 5, whole 16-byte octs (W % 8 == 0), fp16 or fp32 depth planes, no explicit launch plan.  x0 / sparse / target
    are the [B,H,W] planes the engine would get.  Returns the plan dict or None."""
    B, C, H, W = guided.shape
    K = int(math.sqrt(C + 1))
    if _RESIDENT_MODE == "off" or plan is not None or _DEFAULT_PLANS.get(K) is not None or T < 1:
        return None
    if K * K != C + 1 or K not in (3, 5) or W % 8 or guided.dtype not in (torch.float16, torch.float32) or not guided.is_contiguous():
        return None
    if x0.dtype not in (torch.float16, torch.float32) or C * H * W >= (1 << 30):
        return None
    if guided.dtype == torch.float32 and x0.dtype != torch.float32:
        return None
    for t in (guided, x0, sparse, target):
        if t is not None and (t.data_ptr() % 16 or (t is not guided and t.dtype != x0.dtype)):
            return None
    return _kres_plan_cached(K, B, H, W, int(T), int(sparse is not None), guided.device, 0, _dt(guided))[0]


_KRES_STEP_FORM = {"auto": _lib.STEP_AUTO, "fma": _lib.STEP_FMA, "dot2": _lib.STEP_DOT2}[os.environ.get("CSPN_KRES_STEP", "auto")]


def set_kres_step_form(form):
    """Step form of the K x K resident launches (include/cspn_hip.h: cspn_resident_plan.step_form): "auto" (default) takes the
    dot-product kernel where it exists — K = 5, fp16 guidance, fp16 planes: BASELINE config 3 — "fma" keeps every call on the
    FMA kernel (the bits of the multi-launch schedule with steps_per_launch = steps_per_phase).  Env: CSPN_KRES_STEP."""
    global _KRES_STEP_FORM
    _KRES_STEP_FORM = {"auto": _lib.STEP_AUTO, "fma": _lib.STEP_FMA, "dot2": _lib.STEP_DOT2}[form]


def pac_forward_resident(guided, x0, sparse, T, score=None, steps_per_phase=0, spin_limit=0, debug_stamps=None, threads=0,
                         step_form=None, guard=None):
    """CSPN_ours.AffinityPropagate.forward (CSPN_ours.py:24-54) as weight-resident launches (cspnk_forward_resident):
    guided [B,K*K-1,H,W] fp16, x0 / sparse [B,H,W] fp16 or fp32 -> refined [B,H,W] of that dtype; `score=(target, acc)`
    fuses the depth metrics into the last launch.  step_form: None = the module setting (set_kres_step_form), or
    _lib.STEP_AUTO / STEP_FMA / STEP_DOT2."""
    dev = _require_device(guided, x0, sparse)
    B, C, H, W = guided.shape
    K = int(math.sqrt(C + 1))
    L = _lib.lib()
    out = torch.empty((B, H, W), dtype=x0.dtype, device=dev)
    tg, acc = score if score is not None else (None, None)
    blend = BLEND_SPARSE if sparse is not None else BLEND_NONE
    sdt = _dt(x0)
    form = _KRES_STEP_FORM if step_form is None else int(step_form)
    if form == _lib.STEP_DOT2 and not (K == 5 and guided.dtype == torch.float16 and x0.dtype == torch.float16):
        form = _lib.STEP_AUTO                      # a process-wide "dot2" only pins the calls that have the kernel
    # every unscored K x K call carries the device-side guard (csrc/cspn_repair.hip: the softmax forms of the quad kernel for the K = 3 /
    # fp32-guidance model the reference's unet_ours runs, cspnk_resident_repair for the oct kernels); scored calls keep the host repair
    guard = _guard_default(int(T) * (K // 2), "plain" if score is None else "never") if guard is None else int(guard)
    if steps_per_phase or spin_limit or debug_stamps is not None or threads:
        rp = _plan_copy(steps_per_phase=int(steps_per_phase), threads=int(threads), spin_limit=int(spin_limit),
                        debug_stamps=None if debug_stamps is None else debug_stamps.data_ptr(), step_form=form, guard=guard)
    else:
        rp = _with_spin_limit(_kres_plan_cached(K, B, H, W, int(T), int(blend), dev, 0, _dt(guided))[1], form, guard)

    def launch(work, seq, host_err_ptr, stream_ptr):
        return L.cspnk_forward_resident(_p(guided), _dt(guided), K, _p(x0), _p(sparse), _p(out), sdt, _p(work), seq, host_err_ptr, B, H, W,
                                        int(T), int(blend), _p(tg), _p(acc), 0 if acc is None else int(acc.shape[0]), rp, stream_ptr)

    scored = score is not None
    # does this call run the dot-product form (cspnk_d2: K = 5, fp16 guidance and planes, one oct per thread)?  Its state is rounded to half
    # after every step, so NO multi-launch plan has its bits: a failed call of that form is repaired by the same launch once more, unscored
    # and with the device-side guard — which re-computes the form with its own arithmetic (csrc/cspn_repair.hip, round 6) — so that a
    # timed-out call and a clean one return the same numbers on config 3's default path as well
    uses_d2 = False
    if (K == 5 and guided.dtype == torch.float16 and x0.dtype == torch.float16 and form != _lib.STEP_FMA and not steps_per_phase and not threads
            and int(T) * (K // 2) <= _GUARD_MAX_T):
        pd = _kres_plan_cached(K, B, H, W, int(T), int(blend), dev, 0, _dt(guided))[0]
        uses_d2 = pd is not None and pd["quads_per_thread"] == 1

    def redo(out, guided, x0, sparse, tg):     # the same result into the same tensor: prepare + multi-launch propagation (the FMA forms: the
        from . import evaluation               # same bits), or the guarded relaunch of the dot-product form (the same bits as well)
        if scored:
            _unscore_failed_launch(out, tg, acc)
        if uses_d2:
            out.copy_(pac_forward_resident(guided, x0, sparse, T, step_form=form, guard=1))
        else:
            wk, _ = pac_prepare(guided)
            res, _ = propagate(wk, x0, sparse, K, int(T), blend, plan=dtype_default_plan(K, wk.dtype, None))
            out.copy_(res)
        if scored:
            evaluation.metric_sums(out, tg, out=acc)

    _resident_launch(dev, B, H, W, int(T), launch, "cspnk_forward_resident", _kxk_workspace(B, H, W, sdt), redo=redo, out=out,
                     inputs=(guided, x0, sparse, tg), guarded=bool(guard))
    return out


def pac_forward_resident_history(guided, x0, sparse, T):
    """Training forward of CSPN_ours as one weight-resident launch: returns (x_T [view of history[T-1]], history [T,B,H,W],
    wk tap volume).  K = 3, fp32: what pac_prepare + propagate(keep_history=True) return, bit for bit.  K = 5, fp16 guidance and
    fp16 planes (BASELINE config 3's shape): the dot-product kernel — the state is rounded to half after every step — with the
    taps published in the fp16 tap-volume layout; within fp16 rounding of the multi-launch forward."""
    dev = _require_device(guided, x0, sparse)
    B, C, H, W = guided.shape
    K = int(math.sqrt(C + 1))
    L = _lib.lib()
    hist = torch.empty((int(T), B, H, W), dtype=x0.dtype, device=dev)
    wk = _weight_buffer(B, C, H, W, guided.dtype, dev)
    blend = BLEND_SPARSE if sparse is not None else BLEND_NONE
    gdt = _dt(guided)
    # the device-side guard (a launch that gave up is re-computed on the stream: csrc/cspn_repair.hip), for the forms that have one
    guard = _guard_default(int(T) * (K // 2), "plain" if (K, guided.dtype) in _GUARDED_HISTORY_FORMS else "never")
    rp = _with_spin_limit(_kres_plan_cached(K, B, H, W, int(T), int(blend), dev, 0, gdt)[1], guard=guard)

    def launch(work, seq, host_err_ptr, stream_ptr):
        return L.cspnk_forward_resident_history(_p(guided), gdt, K, _p(x0), _p(sparse), _p(hist), _p(wk), _p(work), seq, host_err_ptr,
                                                B, H, W, int(T), int(blend), rp, stream_ptr)

    _resident_launch(dev, B, H, W, int(T), launch, "cspnk_forward_resident_history", _kxk_workspace(B, H, W, _dt(x0)), reports_done=True,
                     guarded=bool(guard), out=hist[int(T) - 1])
    return hist[int(T) - 1], hist, wk


def transpose_weights(w, K, H, W):
    dev = _require_device(w)
    B = w.shape[0]
    wT = torch.empty_like(w)
    with _device_guard(dev):
        ok = _lib.lib().cspn_transpose_weights(_p(w), _p(wT), _dt(w), B, H, W, int(K), _stream(dev))
    _lib.check(ok, "cspn_transpose_weights")
    return wT


def _resident_sweep_plan(K, plan, B, H, W, T, premask, dev):
    """What every weight-resident form of the reverse sweep asks: mode not "off", no launch plan given or set as default, no HIP-graph
    capture — and then, last (it may create the device's state), the cached plan dict (K = 3: the 3x3 engine's, K = 5: the fp16 oct
    kernel's; None where the shape has none)."""
    if _RESIDENT_MODE == "off" or plan is not None or _DEFAULT_PLANS.get(K) is not None or torch.cuda.is_current_stream_capturing():
        return None
    if K == 3:
        return _resident_plan_cached(B, H, W, int(T), int(premask), dev)[0]
    return _kres_plan_cached(5, B, H, W, int(T), int(premask), dev, 0, CSPN_F16)[0]


def _reverse_sweep(w, K, T, sparse, grad_out, plan, valid_w=0, guidance_S=None):
    """G_T = dL/dout, G_t = stencil^T((1-m) G_{t+1}): the forward kernel on the transposed weights.
    w may be None for K = 3 when guidance_S = (guidance, S) is given (the forward published S only): the weight-resident
    sweep rebuilds the taps from them; any other schedule first rebuilds the volume with cspn3_prepare (the same bits).
    Returns (g_T [B,H,W] f32 — grad_out itself, not a copy, when it is fp32 —, ghist [T,B,H,W] f32 in backward order:
    ghist[s] = G_{T-1-s}; None when T == 0)."""
    dev = grad_out.device
    B, H, W = grad_out.shape[0], grad_out.shape[-2], grad_out.shape[-1]
    g_T = grad_out.reshape(B, H, W)
    if w is None:
        gd, S = guidance_S
        sp32 = None if sparse is None else sparse.float()
        g32 = g_T.float()
        if g32.data_ptr() % 16:
            g32 = g32.clone()
        if (K == 3 and T > 0 and gd.dtype == torch.float32 and W % 4 == 0 and gd.data_ptr() % 16 == 0 and gd.stride(0) % 4 == 0
                and gd.stride(1) % 4 == 0 and gd.stride(1) < (1 << 27) and gd.stride(3) == 1 and gd.stride(2) == W
                and (sp32 is None or sp32.data_ptr() % 16 == 0) and H * W < (1 << 27)
                and _resident_sweep_plan(3, plan, B, H, W, T, sp32 is not None, dev) is not None):
            return g32, transposed_resident_guidance(gd, S, g32, sp32, T, valid_w)
        w = cspn3_prepare(gd, want_s=False, valid_w=valid_w)[0]
    if g_T.data_ptr() % 16:
        g_T = g_T.clone()
    ghist = None
    if (T > 0 and K == 5 and w.dtype == torch.float16 and w.dim() == 3 and W % 8 == 0 and not valid_w
            and (sparse is None or sparse.data_ptr() % 16 == 0) and 24 * H * W < (1 << 30)
            and os.environ.get("CSPN_REVERSE_SWEEP", "auto") == "auto"
            and (_resident_sweep_plan(5, plan, B, H, W, T, sparse is not None, dev) or {}).get("quads_per_thread") == 1):
        # weight-resident reverse sweep on the forward's fp16 volume; half cotangent / sparse planes go in as they are
        if g_T.dtype == torch.float16 and (sparse is None or sparse.dtype == torch.float16):
            return pac_transposed_resident(w, g_T, sparse, T)
        return pac_transposed_resident(w, g_T.float(), None if sparse is None else sparse.float(), T)
    g_T = g_T.float()
    if T > 0:
        sp32 = None if sparse is None else sparse.float()
        L = _lib.lib()
        if (K == 3 and w.dtype == torch.float32 and w.dim() == 4 and W % 4 == 0 and w.data_ptr() % 16 == 0 and g_T.data_ptr() % 16 == 0
                and (sp32 is None or sp32.data_ptr() % 16 == 0) and H * W < (1 << 27)
                and _resident_sweep_plan(3, plan, B, H, W, T, sp32 is not None, dev) is not None):
            # weight-resident reverse sweep: the transposed taps are gathered once and stay in registers for all T steps
            return g_T, transposed_resident(w, g_T, sp32, T, valid_w)
        ghist = torch.empty((T, B, H, W), dtype=torch.float32, device=dev)
        p = None
        if W % 4 == 0 and w.data_ptr() % 16 == 0 and (sp32 is None or sp32.data_ptr() % 16 == 0):
            p = resolve_plan(K, B, H, W, T, True, plan)
        gather = os.environ.get("CSPN_REVERSE_SWEEP", "auto")      # "gather" | "copy": A/B switch; auto = the measured choice
        if gather == "auto":
            gather = "copy" if K >= 5 else "gather"
        if (gather == "gather" and p is not None and not p["force_scalar"]
                and (p["quads_per_thread"], p["threads"]) in _TRANSPOSED_INSTANCES[K]):
            # transposed recurrence straight on the forward tap volume (no transposed copy)
            with _device_guard(dev):
                ok = L.cspn_propagate_transposed(_p(w), _dt(w), _p(g_T), _p(sp32), _p(ghist), B, H, W,
                                                 int(valid_w), int(K), T, int(sparse is not None),
                                                 _plan_ptr(K, plan), _stream(dev))
            _lib.check(ok, "cspn_propagate_transposed")
        else:
            # K >= 5: one pass that writes the transposed tap volume, then the streaming launches (packed fp16 taps, the
            # forward's plan) — the gathering launches read 24 / 48 shifted planes with per-lane patches and measured 2.5x
            # slower per step than streaming a prepared volume (profiles/r03_kernel_stats_train_leg_pac5.csv)
            wT = transpose_weights(w, K, H, W)
            with _device_guard(dev):
                ok = L.cspn_propagate(_p(wT), _dt(wT), _p(g_T), _p(sp32), None, _p(ghist), None,
                                      CSPN_F32, B, H, W, int(valid_w), int(K), T,
                                      BLEND_PREMASK if sparse is not None else BLEND_NONE,
                                      _plan_ptr(K, dtype_default_plan(K, wT.dtype, plan)), _stream(dev))
            _lib.check(ok, "cspn_propagate(backward)")
    return g_T, ghist


def _tail_vector_ok(W, *tensors):
    return W % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def _grad_weights(w, K, T, d0, dhist, sparse, g_T, ghist):
    """Unfused dL/dw + dL/dd0 (any shape / alignment)."""
    B, H, W = d0.shape
    NT = K * K - 1
    gw = torch.empty((B, NT, H, W), dtype=torch.float32, device=w.device)
    gd0 = torch.empty((B, H, W), dtype=torch.float32, device=w.device)
    with _device_guard(w.device):
        ok = _lib.lib().cspn_grad_weights(_p(d0), _p(dhist), _p(g_T), _p(ghist), _p(sparse), _p(gw), _p(gd0), _dt(d0),
                                          B, H, W, int(K), T, _stream(w.device))
    _lib.check(ok, "cspn_grad_weights")
    return gw, gd0


# ------------------------------------------------------------------------------------------------ autograd
def _check_resident_at_end_of_backward(dev):
    """A training step must not apply gradients built on a resident launch that timed out (the forward with history, or
    the reverse sweep just enqueued).  Waiting here would stall the host in the middle of the backward pass; instead an
    event is recorded behind those launches and the autograd engine runs the check when the whole backward pass has
    been enqueued (queue_callback: before `.backward()` returns, i.e. before any optimiser step) — by then the CSPN
    kernels, the first of the backward pass, have long finished, so the wait is free in a real model.  The reference
    re-raises worker errors the same way, never swallowing them (network/libs/base/encoding.py:172-174, :193-194)."""
    st = _RES.get(dev.index)
    if st is None or not st["dirty"] or torch.cuda.is_current_stream_capturing() or _BWD_CHECK_OFF:
        return                     # (CSPN_BWD_CHECK=off: A/B switch for measurements; the next resident launch still raises)
    if not st["need_bwd_check"]:
        return                     # every training-form launch since the last check carried its device-side guard (round 5): whatever
    st["need_bwd_check"] = False   # the loss and the optimiser read is complete by stream order — nothing for the host to wait for
    cp = _ResidentCheckpoint(dev)
    if st["last_reports"]:     # the newest launch is the one the checkpoint waits for: everything issued so far is covered
        st["dirty"] = False        # (a later inference launch does not report completion: the next ensure_resident_ok still waits)
    try:
        torch.autograd.Variable._execution_engine.queue_callback(cp.wait_and_check)
    except RuntimeError:           # not inside an engine-driven backward (a direct call of .backward on the ctx): check now
        cp.wait_and_check()


class _NoGradCtx(object):
    """Stand-in ctx for inference calls that skip torch.autograd.Function.apply (saves ~10 us of host time)."""
    needs_input_grad = (False,) * 8


# A/B switches read ONCE at import (they sat on the per-call path of CSPN3Function until round 6): CSPN_TRAIN_VOLUME=1 keeps the
# 8-plane tap volume of the 3x3 training forward, CSPN_BWD_CHECK=off skips the end-of-backward host check (measurements only)
_TRAIN_VOLUME = os.environ.get("CSPN_TRAIN_VOLUME", "0") == "1"
_BWD_CHECK_OFF = os.environ.get("CSPN_BWD_CHECK") == "off"
_TRAIN_FAST = {}       # call signature -> (cached guarded resident plan, blend): CSPN3Function's resident training form, checks done once


def _train_fast_key(guidance, blur_depth, sparse_depth, prop_time, plan, valid_w):
    """Everything the slow path's checks depend on that does not change from step to step in a training loop; what can
    (contiguity, alignment, the module-level switches) is re-checked per call."""
    if plan is not None or _DEFAULT_PLANS or _RESIDENT_MODE == "off" or _RESIDENT_SPIN_LIMIT or not _RESIDENT_GUARD:
        return None
    return (guidance.shape, guidance.stride(), guidance.dtype, blur_depth.shape, blur_depth.dtype,
            None if sparse_depth is None else (sparse_depth.shape, sparse_depth.dtype), prop_time, valid_w, _RESIDENT_MODE, guidance.device)


class CSPN3Function(torch.autograd.Function):
    """3x3 variant, forward + hand-written backward (SURVEY.md §3.2 closed form)."""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, prop_time, plan, valid_w=0):
        B, C, H, W = guidance.shape
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        # Fast path of a training loop (round 5: the step was HOST-bound, 217 us of host time for 209 us of kernels): a call whose
        # signature took the weight-resident training form before goes straight to it — no re-validation, no plan look-ups.
        key = _train_fast_key(guidance, blur_depth, sparse_depth, prop_time, plan, valid_w) if need_grad else None
        hit = _TRAIN_FAST.get(key) if key is not None else None
        if (hit is not None and blur_depth.is_contiguous() and (sparse_depth is None or sparse_depth.is_contiguous())
                and not ((guidance.data_ptr() | blur_depth.data_ptr() | (0 if sparse_depth is None else sparse_depth.data_ptr())) & 15)
                and blur_depth.device == guidance.device and (sparse_depth is None or sparse_depth.device == guidance.device)
                and not torch._C._cuda_isCurrentStreamCapturing()):
            d0 = blur_depth.view(B, H, W)
            sp = None if sparse_depth is None else sparse_depth.view(B, H, W)
            out, hist, w8, S = forward_resident(guidance, d0, sp, prop_time, hit[1], valid_w=valid_w, keep_history=True,
                                                publish_weights=_TRAIN_VOLUME, guard=1, _plan=hit[0])
            ctx.save_for_backward(guidance, w8, S, d0, sp, hist)
            ctx.prop_time, ctx.plan, ctx.valid_w = prop_time, None, valid_w
            ctx.in_shape = tuple(blur_depth.shape)
            ctx.fast = hit
            return out.unsqueeze(1)
        d0 = _plane(blur_depth, B, H, W, "blur_depth")
        sp = _plane(sparse_depth, B, H, W, "sparse_depth")
        if d0.dtype != guidance.dtype or (sp is not None and sp.dtype != guidance.dtype):
            raise TypeError("guidance / blur_depth / sparse_depth must share one dtype")
        blend = BLEND_SPARSE if sp is not None else BLEND_NONE
        if not need_grad and resident_supported(guidance, d0, sp, prop_time, plan) is not None:
            # inference, weight-resident: one launch for all T steps, no tap volume at all
            return forward_resident(guidance, d0, sp, prop_time, blend, valid_w=valid_w).unsqueeze(1)
        if not need_grad and _FROM_GUIDANCE and from_guidance_supported(guidance, d0, sp, plan):
            # inference: no separate prepare pass (the first launch derives and publishes the weights)
            out, _ = propagate_from_guidance(guidance, d0, sp, prop_time, blend, plan=plan, valid_w=valid_w)
            return out.unsqueeze(1)
        if need_grad and prop_time > 0 and resident_supported(guidance, d0, sp, prop_time, plan) is not None:
            # training, weight-resident: one launch writes the T depth planes and publishes the weights + S for the backward
            g = guidance
            # (S only: the reverse sweep and the tail rebuild the taps from guidance + S — no 8-plane volume to write or read;
            #  CSPN_TRAIN_VOLUME=1 keeps it, for A/B runs)
            out, hist, w8, S = forward_resident(g, d0, sp, prop_time, blend, valid_w=valid_w, keep_history=True,
                                                publish_weights=_TRAIN_VOLUME)
            if key is not None and prop_time <= _GUARD_MAX_T and blur_depth.dim() == 4 and (sparse_depth is None or sparse_depth.dim() == 4):
                # remember: this signature is served by the resident training form (with the guard: no host check at the end of backward)
                cp = _with_spin_limit(_resident_plan_cached(B, H, W, int(prop_time), int(blend), guidance.device)[1], guard=1)
                if cp is not None:
                    if len(_TRAIN_FAST) > 256:
                        _TRAIN_FAST.clear()
                    _TRAIN_FAST[key] = (cp, blend)
        elif need_grad and _FROM_GUIDANCE and prop_time > 0 and from_guidance_supported(guidance, d0, sp, plan):
            # training: the first launch derives the weights, publishes them and S for the backward, and the loop keeps
            # the T depth planes — one pass over the guidance instead of a prepare pass + a re-read of the volume
            g = guidance
            out, hist, w8, S = propagate_from_guidance(g, d0, sp, prop_time, blend, keep_history=True, plan=plan,
                                                       valid_w=valid_w, return_weights=True)
        else:
            w8, S, g = cspn3_prepare(guidance, want_s=need_grad, valid_w=valid_w)
            out, hist = propagate(w8, d0, sp, 3, prop_time, blend, keep_history=need_grad, plan=plan, valid_w=valid_w)
        if need_grad:
            ctx.save_for_backward(g, w8, S, d0, sp, hist)
            ctx.prop_time, ctx.plan, ctx.valid_w = int(prop_time), plan, int(valid_w)
            ctx.in_shape = tuple(blur_depth.shape)
        return out.unsqueeze(1)

    @staticmethod
    def backward(ctx, grad_out):
        g, w8, S, d0, sp, hist = ctx.saved_tensors
        B, C, H, W = g.shape
        T = ctx.prop_time
        L = _lib.lib()
        fast = getattr(ctx, "fast", None)
        if (fast is not None and w8 is None and grad_out.dtype == torch.float32 and grad_out.is_contiguous() and not (grad_out.data_ptr() & 15)
                and _RESIDENT_MODE != "off" and _RESIDENT_GUARD and not _RESIDENT_SPIN_LIMIT and not _DEFAULT_PLANS
                and not torch._C._cuda_isCurrentStreamCapturing()):
            # the forward took the fast path: same tensors, same checks — volume-free reverse sweep + fused tail, straight away
            g_T = grad_out.view(B, H, W)
            ghist = transposed_resident_guidance(g, S, g_T, sp, T, ctx.valid_w, _plan=fast[0])
            gg = torch.empty_like(g)
            gd0 = torch.empty((B, H, W), dtype=torch.float32, device=g.device)
            dev_switch = None if torch._C._cuda_getDevice() == g.device.index else torch.cuda.device(g.device)
            if dev_switch is not None:
                dev_switch.__enter__()
            try:
                ok = L.cspn3_backward_tail(d0.data_ptr(), hist.data_ptr(), g_T.data_ptr(), ghist.data_ptr(), _p(sp), g.data_ptr(), g.stride(0),
                                           g.stride(1), C, None, S.data_ptr(), gg.data_ptr(), gd0.data_ptr(), CSPN_F32, B, H, W, T,
                                           torch._C._cuda_getCurrentRawStream(g.device.index))
            finally:
                if dev_switch is not None:
                    dev_switch.__exit__(None, None, None)
            _lib.check(ok, "cspn3_backward_tail")
            return (gg if ctx.needs_input_grad[0] else None, gd0.view(ctx.in_shape) if ctx.needs_input_grad[1] else None,
                    None, None, None, None)
        g_T, ghist = _reverse_sweep(w8, 3, T, sp, grad_out.contiguous().float(), ctx.plan, ctx.valid_w, guidance_S=(g, S))
        _check_resident_at_end_of_backward(g.device)
        gg = torch.empty_like(g)
        if _tail_vector_ok(W, g, S, d0, sp, hist, gg) and (w8 is None or w8.data_ptr() % 16 == 0) and g.stride(0) % 4 == 0 and g.stride(1) % 4 == 0:
            gd0 = torch.empty((B, H, W), dtype=torch.float32, device=g.device)
            with _device_guard(g.device):
                ok = L.cspn3_backward_tail(_p(d0), _p(hist), _p(g_T), _p(ghist), _p(sp), _p(g), g.stride(0), g.stride(1), C,
                                           _p(w8), _p(S), _p(gg), _p(gd0), _dt(g), B, H, W, T, _stream(g.device))
            _lib.check(ok, "cspn3_backward_tail")
        else:
            if w8 is None:
                w8 = cspn3_prepare(g, want_s=False, valid_w=ctx.valid_w)[0]
            gw, gd0 = _grad_weights(w8, 3, T, d0, hist, sp, g_T, ghist)
            with _device_guard(g.device):
                ok = L.cspn3_grad_guidance(_p(g), _dt(g), g.stride(0), g.stride(1), C, _p(w8), _dt(w8),
                                           _p(S), _p(gw), _p(gg), B, H, W, _stream(g.device))
            _lib.check(ok, "cspn3_grad_guidance")
        if not ctx.needs_input_grad[0]:
            gg = None
        gd = gd0.to(d0.dtype).reshape(ctx.in_shape) if ctx.needs_input_grad[1] else None
        return gg, gd, None, None, None, None


class PACFunction(torch.autograd.Function):
    """K x K softmax variant (CSPN_ours.py / pac.py) forward + backward.

    x is [B,C,H,W] as the reference documents it (CSPN_ours.py:24-29): pac.conv2d broadcasts the shared [B,1,K,K,H,W]
    kernel over the channels (pac.py:89-92) and the [B,1,H,W] sparse mask broadcasts in the blend (:51-53), so the C
    planes are independent recurrences over ONE tap volume.  C = 1 (the depth map, unet_ours.py:333) is the tuned path;
    C > 1 runs the same launches once per plane against the shared volume (softmax / prepare done once, dL/dguided
    summed over the planes — the softmax backward is linear in dL/dkernel)."""

    @staticmethod
    def forward(ctx, x, guided, sparse_depth, prop_time, plan, state_dtype, valid_w=0):
        B, C, H, W = guided.shape
        if x.dim() != 4 or x.shape[0] != B or tuple(x.shape[2:]) != (H, W) or x.shape[1] < 1:
            raise ValueError("x must be [B,C,H,W] matching guided [B,K*K-1,H,W]; got %s and %s" % (
                tuple(x.shape), tuple(guided.shape)))
        CX = x.shape[1]
        sdt = x.dtype if state_dtype is None else state_dtype
        sp = _plane(sparse_depth, B, H, W, "sparse_depth")
        sp = None if sp is None else sp.to(sdt)
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if not need_grad and CX == 1 and not valid_w:       # (row padding — W_valid — is the multi-launch kernels' business)
            g = guided if guided.is_contiguous() else guided.contiguous()
            d0 = _plane(x, B, H, W, "x").to(sdt)
            if pac_resident_supported(g, d0, sp, prop_time, plan) is not None:
                # inference, weight-resident: the softmax taps never leave the registers, no tap volume
                return pac_forward_resident(g, d0, sp, prop_time).unsqueeze(1)
        k3_f32 = C == 8 and guided.dtype == torch.float32 and sdt == torch.float32
        k5_f16 = C == 24 and guided.dtype == torch.float16 and sdt == torch.float16 and _KRES_STEP_FORM != STEP_FMA
        if (need_grad and CX == 1 and not valid_w and (k3_f32 or k5_f16) and prop_time > 0
                and not torch.cuda.is_current_stream_capturing()):
            g = guided if guided.is_contiguous() else guided.contiguous()
            d0 = _plane(x, B, H, W, "x").to(sdt)
            rpl = pac_resident_supported(g, d0, sp, prop_time, plan)
            if rpl is not None and (k3_f32 or rpl["quads_per_thread"] == 1):
                # training, weight-resident (the configuration the reference trains: K = 3, fp32): one launch writes the T depth
                # planes and publishes the softmax taps for the backward — no prepare pass, no re-streamed tap volume
                out, hist, wk = pac_forward_resident_history(g, d0, sp, prop_time)
                ctx.save_for_backward(wk, sp, d0, hist)
                ctx.K, ctx.prop_time, ctx.plan, ctx.valid_w = (3 if k3_f32 else 5), int(prop_time), plan, int(valid_w)
                ctx.x_dtype, ctx.g_dtype = x.dtype, guided.dtype
                return out.unsqueeze(1)
        wk, K = pac_prepare(guided)
        # the dtype-specific built-in plan serves the forward only: the reverse sweep has its own instances
        fplan = dtype_default_plan(K, wk.dtype, plan)
        blend = BLEND_SPARSE if sp is not None else BLEND_NONE
        outs, saved = [], []
        for c in range(CX):
            d0 = _plane(x[:, c:c + 1], B, H, W, "x").to(sdt)
            out, hist = propagate(wk, d0, sp, K, prop_time, blend, keep_history=need_grad, plan=fplan, valid_w=valid_w)
            outs.append(out)
            saved += [d0, hist]
        if need_grad:
            ctx.save_for_backward(wk, sp, *saved)
            ctx.K, ctx.prop_time, ctx.plan, ctx.valid_w = K, int(prop_time), plan, int(valid_w)
            ctx.x_dtype, ctx.g_dtype = x.dtype, guided.dtype
        return outs[0].unsqueeze(1) if CX == 1 else torch.stack(outs, 1)

    @staticmethod
    def backward(ctx, grad_out):
        wk, sp = ctx.saved_tensors[:2]
        planes = ctx.saved_tensors[2:]
        CX = len(planes) // 2
        B, H, W = planes[0].shape
        K, T = ctx.K, ctx.prop_time
        NT = K * K - 1
        L = _lib.lib()
        go = grad_out.contiguous()          # _reverse_sweep converts where its launches need fp32 (the K = 5 resident sweep takes half)
        gg_sum, gxs = None, []
        for c in range(CX):
            d0, hist = planes[2 * c], planes[2 * c + 1]
            g_T, ghist = _reverse_sweep(wk, K, T, sp, go[:, c].contiguous(), ctx.plan, ctx.valid_w)
            _check_resident_at_end_of_backward(wk.device)
            gg = torch.empty((B, NT, H, W), dtype=ctx.g_dtype, device=wk.device)
            if _tail_vector_ok(W, wk, d0, sp, hist, gg):
                gx0 = torch.empty((B, H, W), dtype=ctx.x_dtype if ctx.x_dtype == torch.float16 else torch.float32, device=wk.device)
                with _device_guard(wk.device):
                    ok = L.cspn_pac_backward_tail(_p(d0), _p(hist), _p(g_T), _p(ghist), _p(sp), _p(wk), _p(gg), _p(gx0), _dt(gx0), _dt(d0),
                                                  _dt(wk), B, H, W, K, T, _stream(wk.device))
                _lib.check(ok, "cspn_pac_backward_tail")
            else:
                gw, gx0 = _grad_weights(wk, K, T, d0, hist, sp, g_T, ghist)
                with _device_guard(wk.device):
                    ok = L.cspn_pac_grad_guided(_p(wk), _dt(wk), _p(gw), _p(gg), _dt(gg), B, H, W, K, _stream(wk.device))
                _lib.check(ok, "cspn_pac_grad_guided")
            gxs.append(gx0)
            if CX > 1:
                gg_sum = gg.float() if gg_sum is None else gg_sum.add_(gg)
            else:
                gg_sum = gg
        gg = gg_sum.to(ctx.g_dtype) if ctx.needs_input_grad[1] else None
        gx = None
        if ctx.needs_input_grad[0]:
            gx = (gxs[0].unsqueeze(1) if CX == 1 else torch.stack(gxs, 1)).to(ctx.x_dtype)
        return gx, gg, None, None, None, None, None


_SCORED_FAST = {}      # call signature -> _ScoredFast: cspn3_refine_and_score goes straight to the scored resident launch


class _ScoredFast(object):
    """Everything a scored resident forward of one call signature needs, resolved once (round 5: at per-GPU shard sizes the call is
    HOST-bound — 20 us of host time against 17 us of kernel, tools/probes/r05_shard_host.py): the cached plan, the device's
    state, the constant arguments of the C call.  `issue` is the lean way into _issue — forward_resident + _resident_launch with
    nothing left to look up: no Stream object, no device switch, no launch closure; whatever it does not handle (a spin limit,
    another device current, HIP-graph capture, a stream change, an evicted workspace, a sequence wrap) returns None BEFORE anything
    is consumed or allocated — the sampling slot of an event log, the output — and the caller takes the general path."""
    __slots__ = ("plan", "plan_guarded", "dev", "idx", "st", "wkey", "B", "H", "W", "T", "blend", "gs0", "gs1", "nslots", "nbytes",
                 "what", "cfunc")

    def __init__(self, plan, guidance, T, blend, acc):
        B, C, H, W = guidance.shape
        self.plan, self.dev, self.idx = plan, guidance.device, guidance.device.index
        self.st = _resident_state(guidance.device)
        self.wkey = (B, H, W, "3", 4)
        self.B, self.H, self.W, self.T, self.blend = B, H, W, int(T), int(blend)
        self.gs0, self.gs1, self.nslots = guidance.stride(0), guidance.stride(1), int(acc.shape[0])
        self.nbytes = (guidance.numel() + (3 + int(bool(blend))) * B * H * W) * 4
        self.what = "cspn3_forward_resident %dx%dx%d (scored)" % (B, H, W)
        self.cfunc = _lib.lib().cspn3_forward_resident
        # the guarded copy of the plan (whether a call takes it is _guard_default's business); a spin limit keeps calls off this path
        self.plan_guarded = None if _RESIDENT_SPIN_LIMIT else _with_spin_limit(plan, guard=1)

    def _launch(self, work, seq, host_err_ptr, raw, guidance, d0, sparse, out, target, acc, plan):
        return self.cfunc(guidance.data_ptr(), self.gs0, self.gs1, d0.data_ptr(), None if sparse is None else sparse.data_ptr(), out.data_ptr(),
                          None, None, None, work.data_ptr(), seq, host_err_ptr, self.B, self.H, self.W, 0, self.T, self.blend,
                          target.data_ptr(), acc.data_ptr(), self.nslots, plan, raw)

    def issue(self, guidance, d0, sparse, target, acc):
        st = self.st
        if (_RESIDENT_SPIN_LIMIT or torch._C._cuda_getDevice() != self.idx or torch._C._cuda_isCurrentStreamCapturing()):
            return None
        raw = torch._C._cuda_getCurrentRawStream(self.idx)
        with st["lock"]:
            # everything another thread's launch can change is read under the device's lock (read before it, a launch from
            # another stream in between let this one skip wait_stream and overlap a resident launch — time-outs, not wrong output)
            work = st["work"].get(self.wkey)       # (looked up per call: the workspace cache may have been started over)
            if work is None or raw != st["last_raw"] or st["seq"] > _RES_SEQ_MAX:
                return None                        # stream change / evicted workspace / sequence wrap: the general path
            log = _sampled_log()                   # (bench.py's HIP events: an instrumented loop runs the same lean path: round 6)
            out = torch.empty((self.B, self.H, self.W), dtype=torch.float32, device=self.dev)
            # (guarded: the guard re-computes the depth AND the missing metric terms on the stream: no entry)
            guarded = self.plan_guarded is not None and _guard_default(self.T, "scored")
            journal = None if guarded else (_redo3(self.B, self.H, self.W, self.T, self.blend, 0, acc), out, (guidance, d0, sparse, target),
                                            self.what, self.nbytes)
            ok = _issue(self.dev, st, raw, log, self.T, self._launch,
                        (guidance, d0, sparse, out, target, acc, self.plan_guarded if guarded else self.plan), False, journal, work)
        _lib.check(ok, "cspn3_forward_resident")
        return out


def cspn3_refine_and_score(guidance, blur_depth, sparse_depth, target, acc, prop_time=24, plan=None):
    """Inference forward of the 3x3 module + metrics of the result vs `target` accumulated into `acc`
    (evaluation.new_accumulator) — the eval loop's `model(input)` + `Result.evaluate` for the CSPN stage
    (libs/trainers/single_gpu_trainer.py:129-140) with the metrics fused into the last propagation launch."""
    from . import evaluation
    # Fast path: an eval loop calls this with the same shapes every time, and at per-GPU shard sizes (one KITTI frame, three NYU
    # frames) the call's HOST time (~25 us of validation, views and plan look-ups) exceeded the kernel's (19-22 us).  A key made of
    # everything the checks below depend on remembers that the weight-resident scored launch serves this call; what can still
    # change from call to call (contiguity, alignment, the module-level switches) is re-checked here.
    key = None
    if plan is None and not _DEFAULT_PLANS and acc.dtype == torch.float64:
        key = (guidance.shape, guidance.stride(), guidance.dtype, blur_depth.shape, blur_depth.dtype,
               None if sparse_depth is None else (sparse_depth.shape, sparse_depth.dtype), target.shape, target.dtype,
               acc.shape, int(prop_time), _RESIDENT_MODE, guidance.device)
        fast_plan = _SCORED_FAST.get(key)
        if (fast_plan is not None and blur_depth.is_contiguous() and target.is_contiguous() and acc.is_contiguous()
                and (sparse_depth is None or sparse_depth.is_contiguous())
                and not ((guidance.data_ptr() | blur_depth.data_ptr() | target.data_ptr() |
                          (0 if sparse_depth is None else sparse_depth.data_ptr())) & 15)
                and blur_depth.device == target.device == guidance.device and (sparse_depth is None or sparse_depth.device == guidance.device)):
            out = fast_plan.issue(guidance, blur_depth, sparse_depth, target, acc)
            if out is None:        # something the lean path does not handle (stream change, capture, ...): the general one
                with torch.no_grad():
                    out = forward_resident(guidance, blur_depth, sparse_depth, prop_time, fast_plan.blend, score=(target, acc),
                                           _plan=fast_plan.plan if _RESIDENT_GUARD != "all" else None)
            return out.unsqueeze(1)
    _require_device(guidance, blur_depth, sparse_depth, target)
    W0 = guidance.shape[-1]
    pad = _row_padding(W0, plan)
    if pad:
        guidance, blur_depth, sparse_depth, target = (_pad_w(t, pad) for t in (guidance[:, :8], blur_depth, sparse_depth,
                                                                               target))
    vw = W0 if pad else 0
    B, C, H, W = guidance.shape
    d0 = _plane(blur_depth, B, H, W, "blur_depth")
    sp = _plane(sparse_depth, B, H, W, "sparse_depth")
    tg = _plane(target, B, H, W, "target")
    blend = BLEND_SPARSE if sp is not None else BLEND_NONE
    with torch.no_grad():
        if guidance.dtype == d0.dtype == tg.dtype and resident_supported(guidance, d0, sp, prop_time, plan, tg) is not None:
            out = forward_resident(guidance, d0, sp, prop_time, blend, score=(tg, acc), valid_w=vw)
            if key is not None and not pad and blur_depth.dim() == 4 and target.dim() == 4 and (sparse_depth is None or sparse_depth.dim() == 4):
                if len(_SCORED_FAST) > 256:
                    _SCORED_FAST.clear()
                _SCORED_FAST[key] = _ScoredFast(_scored_plan(_resident_plan_cached(B, H, W, int(prop_time), int(blend), guidance.device)[1],
                                                             B, H, W, int(prop_time), int(blend), guidance.device), guidance,
                                                prop_time, blend, acc)
            return out.unsqueeze(1)[..., :W0]
        if (_FROM_GUIDANCE and from_guidance_supported(guidance, d0, sp, plan) and guidance.dtype == d0.dtype
                and tg.dtype == d0.dtype and tg.data_ptr() % 16 == 0):
            p = resolve_plan(3, B, H, W, prop_time, False, plan)
            if (prop_time > p["steps_per_launch"] and not p["force_scalar"]
                    and (p["quads_per_thread"], p["threads"]) in _SCORED_INSTANCES[3]):
                out, _ = propagate_from_guidance(guidance, d0, sp, prop_time, blend, plan=plan, score=(tg, acc),
                                                 valid_w=vw)
                return out.unsqueeze(1)[..., :W0]
        w8, _, _ = cspn3_prepare(guidance, valid_w=vw)
        if scored_supported(w8, d0, sp, tg, 3, prop_time, plan):
            out = propagate_scored(w8, d0, sp, 3, prop_time, blend, tg, acc, plan, valid_w=vw)
        else:
            out, _ = propagate(w8, d0, sp, 3, prop_time, blend, plan=plan, valid_w=vw)
            evaluation.metric_sums(out, tg, out=acc)
    return out.unsqueeze(1)[..., :W0]


def pac_refine_and_score(x, guided, sparse_depth, target, acc, prop_time=24, plan=None, state_dtype=None):
    """K x K twin of cspn3_refine_and_score."""
    from . import evaluation
    _require_device(x, guided, sparse_depth, target)
    W0 = guided.shape[-1]
    pad = _row_padding(W0, plan)
    if pad:
        x, guided, sparse_depth, target = (_pad_w(t, pad) for t in (x, guided, sparse_depth, target))
    vw = W0 if pad else 0
    B, C, H, W = guided.shape
    with torch.no_grad():
        sdt = x.dtype if state_dtype is None else state_dtype
        d0 = _plane(x, B, H, W, "x").to(sdt)
        sp = _plane(sparse_depth, B, H, W, "sparse_depth")
        sp = None if sp is None else sp.to(sdt)
        tg = _plane(target, B, H, W, "target").to(sdt)
        if not pad and x.shape[1] == 1:
            g = guided if guided.is_contiguous() else guided.contiguous()
            if pac_resident_supported(g, d0, sp, prop_time, plan, tg) is not None:
                return pac_forward_resident(g, d0, sp, prop_time, score=(tg, acc)).unsqueeze(1)
        wk, K = pac_prepare(guided)
        plan = dtype_default_plan(K, wk.dtype, plan)
        blend = BLEND_SPARSE if sp is not None else BLEND_NONE
        if scored_supported(wk, d0, sp, tg, K, prop_time, plan):
            out = propagate_scored(wk, d0, sp, K, prop_time, blend, tg, acc, plan, valid_w=vw)
        else:
            out, _ = propagate(wk, d0, sp, K, prop_time, blend, plan=plan, valid_w=vw)
            evaluation.metric_sums(out, tg, out=acc)
    return out.unsqueeze(1)[..., :W0]


def _row_padding(W, plan):
    """Columns to append so that rows are whole quads (0 when W % 4 == 0 or the plan forces the generic kernels).
    The padded columns are passed to the engine as row padding (W_valid), i.e. treated as outside the image."""
    if W % 4 == 0 or (isinstance(plan, dict) and plan.get("force_scalar")):
        return 0
    forced = _DEFAULT_PLANS.get(3)
    if plan is None and isinstance(forced, dict) and forced.get("force_scalar"):
        return 0
    return -W % 4


def _pad_w(t, pad):
    return None if t is None else torch.nn.functional.pad(t, (0, pad))


def cspn3_affinity_propagate(guidance, blur_depth, sparse_depth=None, prop_time=24, plan=None):
    """Functional form of CSPN_new.AffinityPropagate.forward (CSPN_new.py:26-92)."""
    _require_device(guidance, blur_depth, sparse_depth)
    W = guidance.shape[-1]
    pad = _row_padding(W, plan)
    if pad:     # any width: zero-pad the rows to whole quads and tell the engine the true width
        # (only the 8 channels the module reads are copied; the others get a zero gradient from the slice)
        guidance, blur_depth, sparse_depth = (_pad_w(guidance[:, :8], pad), _pad_w(blur_depth, pad),
                                              _pad_w(sparse_depth, pad))
    vw = W if pad else 0
    if not (torch.is_grad_enabled() and (guidance.requires_grad or blur_depth.requires_grad)):
        out = CSPN3Function.forward(_NoGradCtx, guidance, blur_depth, sparse_depth, int(prop_time), plan, vw)
    else:
        out = CSPN3Function.apply(guidance, blur_depth, sparse_depth, int(prop_time), plan, vw)
    return out[..., :W] if pad else out


def pac_affinity_propagate(x, guided, sparse_depth=None, prop_time=24, plan=None, state_dtype=None):
    """Functional form of CSPN_ours.AffinityPropagate.forward (CSPN_ours.py:24-54)."""
    _require_device(x, guided, sparse_depth)
    W = guided.shape[-1]
    pad = _row_padding(W, plan)
    if pad:
        x, guided, sparse_depth = _pad_w(x, pad), _pad_w(guided, pad), _pad_w(sparse_depth, pad)
    vw = W if pad else 0
    if not (torch.is_grad_enabled() and (x.requires_grad or guided.requires_grad)):
        out = PACFunction.forward(_NoGradCtx, x, guided, sparse_depth, int(prop_time), plan, state_dtype, vw)
    else:
        out = PACFunction.apply(x, guided, sparse_depth, int(prop_time), plan, state_dtype, vw)
    return out[..., :W] if pad else out


# ------------------------------------------------------------------------------------------------ max-of-8 (the original CSPN.py)
def max8_workspace(B, H, W, T, keep_history, device):
    """`work` of one cspn_max8 call, fresh from torch's caching allocator (no synchronisation, also inside a graph capture)."""
    nbytes = _lib.lib().cspn_max8_workspace_bytes(B, H, W, T, 1 if keep_history else 0)
    return torch.empty((nbytes // 4,), dtype=torch.float32, device=device)


def _max8_guidance(guidance):
    """The guidance as the engine reads it — arbitrary batch and channel strides, rows contiguous — without a copy when it can."""
    H, W = guidance.shape[2], guidance.shape[3]
    if guidance.stride(3) != 1 or guidance.stride(2) != W or guidance.stride(0) < 0 or guidance.stride(1) < 0 or guidance.data_ptr() & 3:
        guidance = guidance[:, :8].contiguous()
    return guidance


class Max8Function(torch.autograd.Function):
    """network/libs/post_process/CSPN.py's recurrence: cspn_max8_forward / cspn_max8_backward (include/cspn_max8.h)."""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, prop_time, steps_per_launch):
        B, C, H, W = guidance.shape
        dev = guidance.device
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        g = _max8_guidance(guidance)
        d0 = _plane(blur_depth, B, H, W, "blur_depth")
        sp = _plane(sparse_depth, B, H, W, "sparse_depth")
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        hist = mask = None
        if need_grad:
            hist = torch.empty((prop_time, B, H, W), dtype=torch.float32, device=dev)
            mask = torch.empty((prop_time, B, H, W), dtype=torch.uint8, device=dev)
        work = max8_workspace(B, H, W, prop_time, False, dev)
        with _device_guard(dev):
            ok = _lib.lib().cspn_max8_forward(_p(g), g.stride(0), g.stride(1), _p(d0), _p(sp), _p(out), _p(hist), _p(mask), _p(work),
                                         B, H, W, prop_time, steps_per_launch, _stream(dev))
        _lib.check(ok, "cspn_max8_forward")
        if need_grad:
            ctx.save_for_backward(g, d0, sp, hist, mask)
            ctx.dims = (B, C, H, W, prop_time)
            ctx.blur_shape = tuple(blur_depth.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        g, d0, sp, hist, mask = ctx.saved_tensors
        B, C, H, W, T = ctx.dims
        dev = g.device
        go = grad_out
        if go.dtype != torch.float32:
            go = go.float()
        go = go.contiguous()
        grad_g = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
        grad_b = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        work = max8_workspace(B, H, W, T, True, dev)
        with _device_guard(dev):
            ok = _lib.lib().cspn_max8_backward(_p(g), g.stride(0), g.stride(1), C, _p(d0), _p(sp), _p(hist), _p(mask), _p(go), _p(grad_g),
                                          _p(grad_b), _p(work), B, H, W, T, _stream(dev))
        _lib.check(ok, "cspn_max8_backward")
        return (grad_g if ctx.needs_input_grad[0] else None, grad_b.view(ctx.blur_shape) if ctx.needs_input_grad[1] else None,
                None, None, None)


def cspn_max8_propagate(guidance, blur_depth, sparse_depth=None, prop_time=16, steps_per_launch=0):
    """Functional form of CSPN.AffinityPropagate.forward (network/libs/post_process/CSPN.py:20-55) and, with sparse_depth=None,
    of AffinityPropagate_prediction.forward (:132-163): eight |guidance| gates as box-normalised 3x3 filters on the depth, their
    element-wise maximum, the sparse blend — prop_time times.  guidance [B,C>=8,H,W] (channels 0..7 read, any batch / channel
    stride), blur_depth / sparse_depth [B,1,H,W]; fp32 only.  Gradients for guidance and blur_depth.  steps_per_launch: 0 = the
    engine's choice, 1..16 = steps one launch advances (the result's bits do not depend on it)."""
    dev = _require_device(guidance, blur_depth, sparse_depth)
    if dev is None:
        raise RuntimeError("CSPN HIP engine: tensors must live on a ROCm device")
    if guidance.dim() != 4 or guidance.shape[1] < 8:
        raise ValueError("guidance must be [B,C>=8,H,W], got %s" % (tuple(guidance.shape),))
    for name, t in (("guidance", guidance), ("blur_depth", blur_depth), ("sparse_depth", sparse_depth)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("cspn_max8_propagate: fp32 only (the reference's precision), %s is %s" % (name, t.dtype))
    prop_time, steps_per_launch = int(prop_time), int(steps_per_launch)
    if prop_time < 1:
        raise ValueError("prop_time must be at least 1, got %d" % prop_time)
    if not 0 <= steps_per_launch <= _lib.MAX8_MAX_STEPS_PER_LAUNCH:
        raise ValueError("steps_per_launch must be 0 (the engine's choice) or 1..%d, got %d" % (_lib.MAX8_MAX_STEPS_PER_LAUNCH, steps_per_launch))
    if guidance.numel() == 0:
        raise ValueError("guidance must be [B,C>=8,H,W], got %s" % (tuple(guidance.shape),))
    if sparse_depth is not None:
        sparse_depth = sparse_depth.detach()
    if not (torch.is_grad_enabled() and (guidance.requires_grad or blur_depth.requires_grad)):
        return Max8Function.forward(_NoGradCtx, guidance, blur_depth, sparse_depth, prop_time, steps_per_launch)
    return Max8Function.apply(guidance, blur_depth, sparse_depth, prop_time, steps_per_launch)

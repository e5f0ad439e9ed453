#!/usr/bin/env python3
"""Time of one SGD step (momentum 0.9, weight_decay 1e-4) over the parameter list of unet_ours.resnet50() with synthetic gradients
(fp32), four formulations on the same GPU in the same process:

  ours      cspn_monodepth_amd.optim.SGD (include/cspn_optim.h)      the reference's bits, ceil(tensors / 109) launches
  fused     torch.optim.SGD(fused=True)                              other bits (a double rate, separately rounded)
  foreach   torch.optim.SGD(foreach=True)                            three passes over the parameters
  single    torch.optim.SGD(foreach=False, fused=False)              what the reference runs: launches per tensor (eager only)

    python tools/optim_bench.py [--rounds 5] [--replays 10] [--eager-iters 20] [--caps 256,512,1024,2048,4096,8192] [--out profiles/optim_bench.json]

Method: every formulation steps its own copy of the parameters.  A replay leg is one captured `step()`, `--replays` replays back
to back between two HIP events, the legs alternating over `--rounds` rounds of 10 such windows each, the median per replay —
device time with the replay's own launch floor.  An eager leg is HIP events around `--eager-iters` steps, host included.  Beside
each time: the bytes per second it amounts to at the step's floor of 20 B per parameter (read p, g, buf; write p, buf), and its
share of the 8 TB/s HBM peak.  `--caps` also times this package's step at other grid caps (max_workgroups; the library's default
is 2048).  Launches per step: counted from a profiler trace of one eager step (null if the profiler is not available); ours also
from cspn_sgd_plan.  Before timing, three steps from the same start are compared bit for bit: which of torch's forms on the device
give the bits of this package's step.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
BYTES_PER_PARAMETER = 20
WINDOWS = 10
HYPER = dict(lr=1e-3, momentum=0.9, weight_decay=1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=10)
    ap.add_argument("--eager-iters", type=int, default=20)
    ap.add_argument("--caps", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    caps = [int(c) for c in a.caps.split(",") if c]
    import torch
    from cspn_monodepth_amd import _lib, optim
    from cspn_monodepth_amd.network import unet_ours
    if not torch.cuda.is_available():
        sys.exit("optim_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)

    def note(msg):
        print("optim_bench: " + msg, file=sys.stderr, flush=True)

    shapes = [tuple(p.shape) for p in unet_ours.resnet50().parameters() if p.requires_grad]
    numel = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numel)
    gen = torch.Generator(device=dev).manual_seed(0)
    start = [torch.randn(s, generator=gen, device=dev) * 0.05 for s in shapes]
    grads = [torch.randn(s, generator=gen, device=dev) * 0.01 for s in shapes]

    def fresh():
        ps = [torch.nn.Parameter(t.clone()) for t in start]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    makers = {"ours": lambda ps: optim.SGD(ps, **HYPER),
              "fused": lambda ps: torch.optim.SGD(ps, fused=True, **HYPER),
              "foreach": lambda ps: torch.optim.SGD(ps, foreach=True, **HYPER),
              "single": lambda ps: torch.optim.SGD(ps, foreach=False, fused=False, **HYPER)}

    # ---- which of torch's forms give this package's bits on the device: three steps from the same start
    params = {k: fresh() for k in makers}
    opts = {k: makers[k](params[k]) for k in makers}
    for _ in range(3):
        for o in opts.values():
            o.step()
    torch.cuda.synchronize()
    differing = {}
    for k in ("fused", "foreach", "single"):
        differing[k] = int(sum(int((p.detach().view(torch.int32) != q.detach().view(torch.int32)).sum())
                               for p, q in zip(params["ours"], params[k])))
    note("elements (of %d) whose bits differ from ours after three steps: %s" % (total, differing))

    # ---- launches per step
    arr = (ctypes.c_size_t * len(numel))(*numel)
    launches, chunks = ctypes.c_int(0), ctypes.c_size_t(0)
    _lib.check(_lib.lib().cspn_sgd_plan(arr, len(numel), 0, ctypes.byref(launches), ctypes.byref(chunks)), "cspn_sgd_plan")
    kernels = {}
    for k, o in opts.items():
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                o.step()
                torch.cuda.synchronize()
            kernels[k] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name
                             and "emset" not in e.name)
        except Exception as exc:       # noqa: BLE001 — the count is information, not the measurement
            note("profiler: %r" % (exc,))
            kernels[k] = None
    note("launches per step: ours %d by plan; traced %s" % (launches.value, kernels))

    # ---- graph replays
    graphs, keep, errors = {}, [], {}

    def capture(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    for k in ("ours", "fused", "foreach"):
        try:
            graphs[k] = capture(opts[k].step)
        except Exception as exc:       # noqa: BLE001
            errors[k] = repr(exc)
            note("%s cannot be captured: %r" % (k, exc))
    ps = fresh()
    bufs = [torch.zeros_like(p) for p in ps]
    gs = [p.grad for p in ps]
    for cap in caps:
        def capped(cap=cap):
            with torch.no_grad():
                optim.sgd_step(ps, gs, bufs, max_workgroups=cap, **HYPER)
        graphs["ours_cap_%d" % cap] = capture(capped)
        keep.append(capped)
    times = {k: [] for k in graphs}
    for g in graphs.values():
        for _ in range(a.replays):
            g.replay()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, g in graphs.items():
            for _ in range(WINDOWS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.replays):
                    g.replay()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.replays)
    # ---- eager steps, host included
    eager = {k: [] for k in opts}
    for _ in range(a.rounds):
        for k, o in opts.items():
            o.step()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.eager_iters):
                o.step()
            e1.record()
            torch.cuda.synchronize()
            eager[k].append(e0.elapsed_time(e1) * 1e3 / a.eager_iters)

    def summary(ts):
        med = statistics.median(ts)
        return dict(us=round(med, 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2),
                    bytes_per_s=round(BYTES_PER_PARAMETER * total / (med * 1e-6), 0),
                    hbm_peak_fraction=round(BYTES_PER_PARAMETER * total / (med * 1e-6) / HBM_PEAK, 4))

    out = dict(tool="optim_bench", model="unet_ours.resnet50", tensors=len(numel), parameters=total, dtype="float32", hyper=HYPER,
               floor_bytes_per_step=BYTES_PER_PARAMETER * total, hbm_peak_bytes_per_s=HBM_PEAK, rounds=a.rounds, replays_per_window=a.replays,
               windows_per_round=WINDOWS, eager_iters=a.eager_iters, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               tensors_per_launch=_lib.SGD_TENSORS_PER_LAUNCH, chunk=_lib.SGD_CHUNK, default_max_workgroups=_lib.SGD_MAX_WORKGROUPS,
               planned_launches=launches.value, planned_chunks=chunks.value, traced_kernels_per_step=kernels,
               elements_differing_from_ours_after_3_steps=differing, capture_errors=errors,
               method="replay: one captured step, %d replays back to back between two HIP events, legs alternating, median per replay "
                      "(device time, the replay's launch floor included); eager: HIP events around %d steps (host included)"
                      % (a.replays, a.eager_iters),
               replay={k: summary(ts) for k, ts in times.items()}, eager={k: summary(ts) for k, ts in eager.items()})
    for k in ("fused", "foreach"):
        if k in times:
            out["%s_over_ours_replay" % k] = round(out["replay"][k]["us"] / out["replay"]["ours"]["us"], 3)
        out["%s_over_ours_eager" % k] = round(out["eager"][k]["us"] / out["eager"]["ours"]["us"], 3)
    note("replay us: %s" % {k: v["us"] for k, v in out["replay"].items()})
    note("eager us: %s" % {k: v["us"] for k, v in out["eager"].items()})
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

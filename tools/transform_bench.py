#!/usr/bin/env python3
"""Time of the NYU train / val transforms at 24 x 480 x 640 -> 228 x 304 (uint8 RGB + fp32 depth in, fp32 RGB + depth out), three
formulations of the reference's per-frame semantics:

  device   train_transform / val_transform (the launches of include/cspn_transform.h), parameters given
  stock    the same result composed from stock PyTorch ops on the device: a gather through index tables BUILT ON THE HOST from the
           frames' parameters (numpy, outside the timed region — a real loop would pay for them per batch), then elementwise ops:
           depth / s, the validity mask, the three blends with a per-frame sum for the contrast constant, / 255 in fp64
  numpy    the restatement of tests/transform_cases.py, frame by frame, on the CPU cores the process may use (a pool of them; the
           reference itself — Pillow + scipy in loader workers — is not part of this repository)

    python tools/transform_bench.py [--iters 200] [--warmup 30] [--graph] [--out profiles/transform_bench.json]

All frames use the op order brightness, contrast, saturation (the stock form would need one code path per order); every other
parameter differs per frame.  device and stock are checked to give the restatement's bits before anything is timed.

Method: HIP events around every single call, the formulations alternating in rounds of iters / 4; the median and the min .. max range
over all of a formulation's calls.  Eager figures contain the host's launch gaps, so they are call times, not kernel times;
`device_time_resolved` says whether anything here measured device time: only --graph does, by timing replays of the captured calls.
numpy is a wall clock around the whole batch.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
B, H, W = 24, 480, 640
OUT = (228, 304)
ROUNDS = 4
FIRST = {"train": 250.0 / 480, "val": 240.0 / 480}


def make_inputs(np):
    r = np.random.RandomState(22)
    rgb = r.randint(0, 256, size=(B, 3, H, W)).astype(np.uint8)
    depth = r.uniform(0.5, 10.0, (B, 1, H, W)).astype(np.float32)
    depth[r.uniform(size=depth.shape) < 0.03] = 0.0
    params = np.zeros((B, 8), np.float64)
    params[:, 0] = r.uniform(1.0, 1.5, B)
    params[:, 1] = r.uniform(-5.0, 5.0, B)
    params[:, 2] = r.uniform(size=B) < 0.5
    params[:, 3:6] = r.uniform(0.6, 1.4, (B, 3))
    return rgb, depth, params                                   # order code 0: brightness, contrast, saturation


def _numpy_frame(job):
    import transform_cases as tc
    rgb, depth, p, mode = job
    return tc.restate_frame(rgb, depth, p, (H, W), FIRST[mode], OUT)


def time_numpy(np, rgb, depth, params, workers):
    """-> {mode: (seconds for the batch on the pool, seconds per frame on one core), ...} and the outputs"""
    import multiprocessing
    res, outs = {}, {}
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        for mode in ("train", "val"):
            jobs = [(rgb[b], depth[b, 0], params[b] if mode == "train" else None, mode) for b in range(B)]
            pool.map(_numpy_frame, jobs[:workers])                                  # imports, first touches
            t0 = time.perf_counter()
            frames = pool.map(_numpy_frame, jobs, chunksize=1)
            t_pool = time.perf_counter() - t0
            t0 = time.perf_counter()
            for job in jobs[:4]:
                _numpy_frame(job)
            res[mode] = (t_pool, (time.perf_counter() - t0) / 4)
            outs[mode] = (np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])[:, None])
    return res, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--graph", action="store_true", help="also time replays of the captured device and stock calls (device time)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 100:
        ap.error("--iters must be at least 100")
    import numpy as np
    import transform_cases as tc

    def note(msg):
        print("transform_bench: " + msg, file=sys.stderr, flush=True)

    rgb_np, depth_np, params_np = make_inputs(np)
    workers = max(1, min(16, len(os.sched_getaffinity(0)), B))
    cpu, want = time_numpy(np, rgb_np, depth_np, params_np, workers)                 # before the GPU is opened: the pool forks
    note("numpy restatement timed on %d workers" % workers)

    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.dataloaders.nyu_dataloader.nyu_dataloader import train_transform, val_transform
    if not torch.cuda.is_available():
        sys.exit("transform_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)
    rgb, depth, params = (torch.from_numpy(v).to(dev) for v in (rgb_np, depth_np, params_np))
    n = OUT[0] * OUT[1]

    # the stock form's tables, built on the host: per frame the flat raw index of every output pixel and its validity
    tables = {}
    for mode in ("train", "val"):
        idx, ok = np.zeros((B, n), np.int64), np.zeros((B, 1, OUT[0], OUT[1]), bool)
        for b in range(B):
            valid, r0, c0 = tc.source_map(params_np[b] if mode == "train" else None, (H, W), FIRST[mode], OUT)
            idx[b], ok[b, 0] = (r0 * W + c0).reshape(-1), valid
        tables[mode] = (torch.from_numpy(idx).to(dev), torch.from_numpy(ok).to(dev))
    sf = params[:, 0].float().view(B, 1, 1, 1)
    fb, fc, fs = (params[:, k].float().view(B, 1, 1, 1) for k in (3, 4, 5))
    zero_f = torch.zeros((), dtype=torch.float32, device=dev)

    def gather(mode):
        idx, ok = tables[mode]
        c = torch.gather(rgb.view(B, 3, H * W), 2, idx[:, None, :].expand(B, 3, n)).view(B, 3, *OUT)
        d = torch.gather(depth.view(B, 1, H * W), 2, idx[:, None, :]).view(B, 1, *OUT)
        return c, d, ok

    def blend(deg, img, f):
        t = deg.float() + f * (img - deg).float()                                  # two kernels: no fused rounding
        return t.clamp(0, 255).to(torch.int32)                                     # truncation; t is never NaN here

    def luma(v):
        return (v[:, 0:1] * 19595 + v[:, 1:2] * 38470 + v[:, 2:3] * 7471 + 0x8000) >> 16

    def stock_train():
        c, d, ok = gather("train")
        d = torch.where(ok, (d / sf) + zero_f, zero_f)
        v = torch.where(ok, c, torch.zeros((), dtype=torch.uint8, device=dev)).to(torch.int32)
        v = blend(torch.zeros_like(v), v, fb)
        mean = (luma(v).sum(dim=(1, 2, 3), keepdim=True).double() / n + 0.5).floor().to(torch.int32)
        v = blend(mean.expand_as(v), v, fc)
        v = blend(luma(v).expand_as(v), v, fs)
        return (v.double() / 255.0).float(), d

    def stock_val():
        c, d, _ = gather("val")
        return (c.double() / 255.0).float(), d

    forms = {"device_train": lambda: train_transform(rgb, depth, params=params), "stock_train": stock_train,
             "device_val": lambda: val_transform(rgb, depth), "stock_val": stock_val}
    for name, fn in forms.items():
        got = [t.cpu().numpy() for t in fn()]
        ref = want[name.split("_")[1]]
        assert tc.same(got[0], ref[0]) and tc.same(got[1], ref[1]), name + " differs from the restatement"
    note("device and stock give the restatement's bits, train and val")
    times = {}

    def measure(runners):
        for name, fn in runners.items():
            times.setdefault(name, [])
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for name, fn in runners.items():
                evs = []
                for _ in range(a.iters // ROUNDS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                times[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]

    measure(forms)
    note("eager calls timed")
    if a.graph:
        replays, keep = {}, []
        for name, fn in forms.items():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep.append(fn())
            replays[name + "_graph"] = graph.replay
            note("captured the %s call" % name)
        measure(replays)
        note("replays timed")

    # what a call must move: 3 + 4 bytes read per OUTPUT pixel (scattered), 16 written
    out = dict(tool="transform_bench", raw=[B, H, W], output=list(OUT), iters=len(times["device_train"]), warmup=a.warmup,
               compulsory_bytes=23 * B * n, device=torch.cuda.get_device_name(0), torch=torch.__version__, code_digest=_lib.code_digest(),
               device_time_resolved=bool(a.graph), numpy_workers=workers,
               method="HIP events around each call, formulations alternating in %d rounds, median and min .. max; eager calls, host launch "
                      "gaps included; *_graph: replays of the captured call, device time; stock's host-built tables are not timed; "
                      "numpy: wall clock around the batch on a pool of numpy_workers processes, and per frame on one core" % ROUNDS)
    for name, ts in times.items():
        out[name + "_us"] = round(statistics.median(ts), 2)
        out[name + "_us_min"] = round(min(ts), 2)
        out[name + "_us_max"] = round(max(ts), 2)
    for mode in ("train", "val"):
        out["numpy_%s_batch_ms" % mode] = round(cpu[mode][0] * 1e3, 1)
        out["numpy_%s_frame_ms_one_core" % mode] = round(cpu[mode][1] * 1e3, 2)
        out["stock_over_device_" + mode] = round(out["stock_%s_us" % mode] / out["device_%s_us" % mode], 2)
        if a.graph:
            out["stock_graph_over_device_graph_" + mode] = round(out["stock_%s_graph_us" % mode] / out["device_%s_graph_us" % mode], 2)
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

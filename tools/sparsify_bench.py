#!/usr/bin/env python3
"""Time of the sparse-depth sampler + RGB-D assembly at 24 x 228 x 304 (fp32 depth, fp32 RGB, 500 samples per frame), three
formulations of the reference's per-frame semantics on the same GPU in the same process:

  device        create_rgbd with Philox in the kernel (the two launches of include/cspn_sparsify.h)
  device_rand   torch.rand for u, then create_rgbd(uniform=u): torch's generator, the same two launches
  stock         torch.rand for u, then stock ops: valid = depth > 0, valid.sum per frame, u.double() < 500 / n_keep, where, cat

    python tools/sparsify_bench.py [--iters 240] [--warmup 30] [--graph] [--out profiles/sparsify_bench.json]

Method: HIP events around every single call, the formulations alternating in rounds of iters / 4, the median over all of a
formulation's calls.  These are eager calls: the figures contain the host's launch gaps (the stock form launches about a dozen
kernels one by one, the device form two and an allocation), so they are call times, not kernel times, and `device_time_resolved`
says whether anything here measured device time at all: only --graph does, by timing replays of the captured calls.
Beside each time: the share of the 8 TB/s HBM peak that the 32 bytes per pixel the call must move (depth and three RGB planes
read once, four planes written) would amount to in that time.  device_rand and stock are checked to give the same bits on the same
u before anything is timed.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, H, W = 24, 228, 304
NUM_SAMPLES = 500
HBM_PEAK = 8e12
ROUNDS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--graph", action="store_true", help="also time replays of the captured device and stock calls (device time)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.dataloaders.nyu_dataloader.dense_to_sparse import UniformSampling, create_rgbd
    if not torch.cuda.is_available():
        sys.exit("sparsify_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    depth = torch.rand((B, 1, H, W), generator=gen, device=dev) * 9.5 + 0.5
    depth = depth * (torch.rand((B, 1, H, W), generator=gen, device=dev) >= 0.03)           # 3 % invalid, as NYU's missing returns
    rgb = torch.rand((B, 3, H, W), generator=gen, device=dev)
    ids = torch.arange(B, dtype=torch.int64, device=dev)
    us = UniformSampling(NUM_SAMPLES)

    def device():
        return create_rgbd(us, rgb, depth, frame_ids=ids, seed=1)[0]

    def device_rand():
        u = torch.rand((B, 1, H, W), device=dev)                  # the default generator: a capture registers it
        return create_rgbd(us, rgb, depth, uniform=u)[0]

    def stock():
        u = torch.rand((B, 1, H, W), device=dev)
        valid = depth > 0
        n_keep = valid.sum(dim=(1, 2, 3), keepdim=True)
        mask = valid & (u.double() < float(NUM_SAMPLES) / n_keep.double()) & (n_keep > 0)
        return torch.cat([rgb, torch.where(mask, depth, torch.zeros_like(depth))], 1)

    forms = {"device": device, "device_rand": device_rand, "stock": stock}

    def note(msg):
        print("sparsify_bench: " + msg, file=sys.stderr, flush=True)

    torch.manual_seed(1)
    x = device_rand()
    torch.manual_seed(1)
    y = stock()
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "device_rand and stock differ on the same u"
    per_frame = [int(v) for v in (device()[:, 3] != 0).sum(dim=(1, 2)).cpu()]
    note("device_rand and stock give the same bits; samples per frame (Philox) %d .. %d" % (min(per_frame), max(per_frame)))
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
        for name in ("device", "stock"):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    forms[name]()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep.append(forms[name]())
            replays[name + "_graph"] = graph.replay
            note("captured the %s call" % name)
        measure(replays)
        note("replays timed")

    n = B * H * W
    nbytes = 32 * n
    out = dict(tool="sparsify_bench", shape=[B, 1, H, W], rgb="float32", num_samples=NUM_SAMPLES, iters=len(times["device"]), warmup=a.warmup,
               compulsory_bytes=nbytes, bytes_per_pixel=32, valid_fraction=float((depth > 0).float().mean()),
               samples_per_frame_min=min(per_frame), samples_per_frame_max=max(per_frame),
               device=torch.cuda.get_device_name(0), torch=torch.__version__, code_digest=_lib.code_digest(),
               device_time_resolved=bool(a.graph),
               method="HIP events around each call, formulations alternating in %d rounds, median; eager calls, host launch gaps "
                      "included; *_graph: replays of the captured call, device time" % ROUNDS)
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name + "_us"] = round(med, 2)
        out[name + "_us_min"] = round(min(ts), 2)
        out[name + "_hbm_peak_fraction"] = round(nbytes / (med * 1e-6) / HBM_PEAK, 4)
    out["stock_over_device"] = round(out["stock_us"] / out["device_us"], 2)
    out["stock_over_device_rand"] = round(out["stock_us"] / out["device_rand_us"], 2)
    if a.graph:
        out["stock_graph_over_device_graph"] = round(out["stock_graph_us"] / out["device_graph_us"], 2)
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

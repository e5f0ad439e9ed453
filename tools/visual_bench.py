#!/usr/bin/env python3
"""Time of the comparison rows of one evaluation batch (24 frames of 228 x 304, synthetic NYU-range values), for 'rgb' (3 panels,
merge_into_row) and 'rgbd' (4 panels, merge_into_row_with_gt), three formulations on the same GPU in the same process:

  ours    cspn_monodepth_amd.utils.comparison_rows (include/cspn_visual.h)      two launches, captured
  stock   the same arithmetic with stock ops: amin / amax per plane, Python's min / max rule as torch.where, sub, div, mul, the index
          rules, a gather from the 257-row byte table, cat — capturable, captured
  host    what the reference does per saved row (libs/utils.py:78-109): .cpu().numpy() of every panel, np.min / np.max, the colour map
          on the CPU (matplotlib's jet if it can be imported, else the same table in numpy — the JSON says which), np.hstack,
          astype('uint8'); wall clock per batch, copies included

    python tools/visual_bench.py [--rounds 5] [--replays 20] [--host-iters 3] [--out profiles/visual_bench.json]

Method: a replay leg is `--replays` replays back to back between two HIP events, 10 such windows per round, the legs alternating
over `--rounds` rounds; median and min - max per replay — device time, the replay's own launch floor included.  Beside each time:
the bytes per second it amounts to at the floor of one read of each depth plane per launch (two launches) plus 3 B written per
output pixel, and its share of the 8 TB/s HBM peak (the read of the RGB planes, 12 B per pixel, is NOT in that floor; the JSON
gives the figure with it too).  Before timing, the three forms are compared byte for byte.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8e12
WINDOWS = 10
B, H, W = 24, 228, 304


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import visual_cases as vc
    from cspn_monodepth_amd import utils
    if not torch.cuda.is_available():
        sys.exit("visual_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)
    table_np = vc.load_table()
    table = torch.cat([torch.from_numpy(table_np), torch.zeros(1, 3, dtype=torch.uint8)]).to(dev)      # row 256: black
    try:
        import matplotlib.pyplot as plt
        cmap, cmap_name = plt.cm.jet, "matplotlib " + __import__("matplotlib").__version__
    except Exception:       # noqa: BLE001
        cmap, cmap_name = None, "numpy table lookup (matplotlib not importable)"

    gen = torch.Generator(device=dev).manual_seed(0)
    rgb = torch.rand(B, 3, H, W, generator=gen, device=dev)
    target = torch.rand(B, 1, H, W, generator=gen, device=dev) * 9.2 + 0.7
    pred = target + 0.4 * torch.randn(B, 1, H, W, generator=gen, device=dev)
    sparse = target * (torch.rand(B, 1, H, W, generator=gen, device=dev) < 500.0 / (H * W))
    data = torch.cat([rgb, sparse], 1)

    def stock(inp, modality, out):
        planes = [target, pred] if modality == "rgb" else [inp[:, 3:], target, pred]
        scale = 1.0 if modality == "rgb" else 255.0
        lo = hi = None
        for p in planes:
            mn, mx = p.amin((1, 2, 3), keepdim=True), p.amax((1, 2, 3), keepdim=True)
            lo = mn if lo is None else torch.where(mn < lo, mn, lo)
            hi = mx if hi is None else torch.where(mx > hi, mx, hi)
        panels = [(inp[:, :3] * scale).clamp(0, 255).nan_to_num(0.0).to(torch.uint8).permute(0, 2, 3, 1)]
        for p in planes:
            x = (p[:, 0] - lo[:, 0]) / (hi[:, 0] - lo[:, 0]) * 256.0
            idx = torch.where(x.isnan(), 256, x.clamp(0, 255).nan_to_num(0.0).to(torch.int64))
            panels.append(table[idx])
        torch.cat(panels, 2, out=out)
        return out

    def host(inp, modality):
        rows = []
        for b in range(B):
            scale = np.float32(1.0 if modality == "rgb" else 255.0)
            rgb_np = scale * np.transpose(inp[b, :3].cpu().numpy(), (1, 2, 0))
            planes = ([] if modality == "rgb" else [inp[b, 3].cpu().numpy()]) + [target[b, 0].cpu().numpy(), pred[b, 0].cpu().numpy()]
            d_min, d_max = min(np.min(p) for p in planes), max(np.max(p) for p in planes)
            cols = []
            for p in planes:
                rel = (p - d_min) / (d_max - d_min)
                cols.append(255 * cmap(rel)[:, :, :3] if cmap is not None else vc.colour(p, d_min, d_max, table_np).astype(np.float64))
            rows.append(np.hstack([rgb_np] + cols).astype("uint8"))
        return np.stack(rows)

    res = {"shape": [B, H, W], "host_colour_map": cmap_name, "replays_per_window": a.replays, "windows_per_round": WINDOWS, "rounds": a.rounds,
           "hbm_peak": HBM_PEAK, "device": torch.cuda.get_device_name(0)}
    for modality, inp, P in (("rgb", rgb, 3), ("rgbd", data, 4)):
        n_depth = P - 1
        out_ours = torch.zeros(B, H, P * W, 3, dtype=torch.uint8, device=dev)
        out_stock = torch.zeros_like(out_ours)
        work = torch.empty(utils.workspace_bytes(B, n_depth, H * W), dtype=torch.uint8, device=dev)
        graphs = {}
        for name, fn in (("ours", lambda: utils.comparison_rows(inp, target, pred, modality, out=out_ours, work=work)),
                         ("stock", lambda: stock(inp, modality, out_stock))):
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        want = host(inp, modality)
        same = {"ours_equals_host": bool(np.array_equal(out_ours.cpu().numpy(), want)),
                "stock_equals_ours": bool(torch.equal(out_stock, out_ours))}
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for name, g in graphs.items():
                for _ in range(WINDOWS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.replays):
                        g.replay()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.replays)
        host_us = []
        for _ in range(a.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host(inp, modality)
            host_us.append((time.perf_counter() - t0) * 1e6)
        floor = B * H * W * (2 * n_depth * 4 + 3 * P)
        floor_rgb = floor + B * H * W * 12
        leg = {"panels": P, "floor_bytes": floor, "floor_bytes_with_rgb_read": floor_rgb, **same,
               "host_us_per_batch": {"median": statistics.median(host_us), "min": min(host_us), "max": max(host_us)}}
        for name, t in times.items():
            med = statistics.median(t)
            leg[name + "_us_per_replay"] = {"median": med, "min": min(t), "max": max(t)}
            leg[name + "_bytes_per_second_at_floor"] = floor / (med * 1e-6)
            leg[name + "_fraction_of_hbm_peak"] = floor / (med * 1e-6) / HBM_PEAK
            leg[name + "_fraction_of_hbm_peak_with_rgb_read"] = floor_rgb / (med * 1e-6) / HBM_PEAK
        leg["stock_over_ours"] = leg["stock_us_per_replay"]["median"] / leg["ours_us_per_replay"]["median"]
        leg["host_over_ours"] = leg["host_us_per_batch"]["median"] / leg["ours_us_per_replay"]["median"]
        res[modality] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

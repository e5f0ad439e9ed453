#!/usr/bin/env python3
"""Kernel time of the per-frame evaluation pair (cspn_metrics_per_frame + cspn_meter_update) against the batch reduction
cspn_metrics_accumulate on the same tensors, by `rocprofv3 --kernel-trace --stats` (one profiled child process per shape), and
the whole-model seconds per frame of examples/eval_loop.py (profiler off).  Writes profiles/r07_eval_protocol.json.

    python tools/bench_eval_meter.py [--out profiles/r07_eval_protocol.json] [--no-loop]

`--child B H W` is the profiled workload: 20 warm-up + 200 timed launches of each form, fp32, back to back on one stream."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((24, 228, 304), (1, 352, 1216))
ITERS, WARMUP = 200, 20


def child(B, H, W):
    sys.path.insert(0, ROOT)
    import torch
    from cspn_monodepth_amd import evaluation as ev
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.rand(B, 1, H, W, generator=gen, device=dev) * 9.5 + 0.5
    p = (t + 0.1 * torch.randn(B, 1, H, W, generator=gen, device=dev)).clamp_(min=0.1)
    t = t * (torch.rand(B, 1, H, W, generator=gen, device=dev) >= 0.05)
    acc = ev.new_accumulator(dev)
    meter = ev.FrameAverageMeter(dev)
    for _ in range(WARMUP + ITERS):
        ev.metric_sums(p, t, out=acc)
    torch.cuda.synchronize()
    for _ in range(WARMUP + ITERS):
        meter.update(p, t)
    torch.cuda.synchronize()
    got, want = ev.average_from_state(meter.state().cpu()), ev.finalize_metrics(acc.cpu())
    print("CHILD_OK frames=%d per_frame_rmse=%.6f pooled_rmse=%.6f" % (got["count"], got["rmse"], want["rmse"]), flush=True)


def kernel_stats(B, H, W, keep):
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="evalmeter_", dir=keep)
    cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "evalmeter", "--",
           sys.executable, os.path.abspath(__file__), "--child", str(B), str(H), str(W)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    if r.returncode != 0 or "CHILD_OK" not in r.stdout:
        raise RuntimeError("profiled run failed (rc %d):\n%s" % (r.returncode, r.stdout[-3000:]))
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("no kernel_stats.csv under %s" % d)
    rows = {}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            for tag in ("cspn_metrics_kernel", "cspn_metrics_frame_kernel", "cspn_metrics_frame_combine_kernel", "cspn_meter_update_kernel"):
                if tag + "<" in row["Name"] or tag + "(" in row["Name"]:
                    rows[tag] = dict(calls=int(row["Calls"]), avg_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                     max_us=float(row["MaxNs"]) / 1e3)
    need = ("cspn_metrics_kernel", "cspn_metrics_frame_kernel", "cspn_metrics_frame_combine_kernel", "cspn_meter_update_kernel")
    if any(k not in rows for k in need):
        raise RuntimeError("kernels missing from the trace: %s" % sorted(set(need) - set(rows)))
    esz = 4
    pair = sum(rows[k]["avg_us"] for k in need[1:])
    return dict(shape=[B, H, W], dtype="float32", bytes_read=2 * B * H * W * esz, kernels=rows, per_frame_pair_avg_us=pair,
                accumulate_avg_us=rows["cspn_metrics_kernel"]["avg_us"], pair_over_accumulate=pair / rows["cspn_metrics_kernel"]["avg_us"],
                frame_kernel_tb_per_s=2 * B * H * W * esz / rows["cspn_metrics_frame_kernel"]["avg_us"] / 1e6,
                accumulate_tb_per_s=2 * B * H * W * esz / rows["cspn_metrics_kernel"]["avg_us"] / 1e6,
                note="averages include the %d warm-up launches; launches back to back on one stream, inputs cache-warm" % WARMUP)


def eval_loop(args):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "eval_loop.py"), "--frames", "96"] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("eval_loop %s failed:\n%s" % (args, r.stderr[-3000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    return dict(args=args, seconds_per_frame=res["seconds_per_frame"], rmse=res["rmse"], count=res["count"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_eval_protocol.json"))
    ap.add_argument("--no-loop", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    keep = tempfile.mkdtemp(prefix="evalmeter_run_")
    out = dict(method="rocprofv3 --kernel-trace --stats, one profiled process per shape; eval_loop rows: wall clock between two device "
                      "synchronisations around 96 frames of the resnet50 model, profiler off, whole-model figures dominated by the stock convolutions",
               kernel_time=[kernel_stats(B, H, W, keep) for B, H, W in SHAPES])
    if not a.no_loop:
        out["eval_loop"] = [eval_loop(x) for x in (["--compare-host-meter"], ["--batch", "1"], ["--batch", "1", "--graph"],
                                                   ["--batch", "24"], ["--batch", "24", "--graph"])]
    shutil.rmtree(keep, ignore_errors=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

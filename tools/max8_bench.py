#!/usr/bin/env python3
"""Times of the max-of-8 propagation (cspn_monodepth_amd/post_process/CSPN.py, include/cspn_max8.h), fp32, T = 16, on one GPU in
one process, at 24 x 8 x 228 x 304 with and without the sparse blend and at 1 x 8 x 352 x 1216 with it:

  fwd_s<S>    the inference forward with steps_per_launch = S for S in 1, 2, 4, 8, 16, and fwd_s0: the built-in choice
  step        forward with history + backward (torch.autograd.grad with a random cotangent), built-in steps_per_launch
  stock_fwd   a stock-ops port written here from the arithmetic: per step ONE grouped 3x3 ones-convolution over the 8 products,
  stock_step  a division, the pairwise torch.max tree, the blend.  (The reference runs 8 single-channel convolutions per step and
              rebuilds its Conv2d modules every call — about 650 launches a forward; this port is the kinder yardstick.)

    python tools/max8_bench.py [--iters 200] [--warmup 20] [--stock-iters 40] [--out profiles/r08_max8_bench.json]

Method: HIP events around every single call, the variants of a shape alternating in 4 rounds, the median over all of a variant's
iterations; every variant is warmed up first.  These are eager calls, so a figure contains the host's launch gaps (they matter
for steps_per_launch = 1: 16 launches).  Before anything is timed the forwards of all steps_per_launch must agree bit for bit
and with the stock port (a sanity bound of 1e-4 on the relative error — MIOpen's convolution adds in another order; the figure
is recorded), and so must the two gradients of `step` against the stock port's: the inputs are random, so a few near-tie
selections differ between two fp32 implementations and move the gradient near those pixels — at most 0.1 % of the elements may
be off by more than 1e-4 of the largest, and the share is recorded.
Beside each forward: the compulsory-traffic floor, (32 + 4 + 4 [+ 4]) bytes per pixel — 8 gates, depth in, depth out, the sparse
plane — at the 8 TB/s HBM peak, and the time's multiple of it.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
ROUNDS = 4
T = 16
SWEEP = (1, 2, 4, 8, 16)
SHAPES = (("nyu_b24_sparse", (24, 8, 228, 304), True), ("nyu_b24", (24, 8, 228, 304), False), ("kitti_b1_sparse", (1, 8, 352, 1216), True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--stock-iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 100 or a.iters % ROUNDS or a.stock_iters % ROUNDS:
        ap.error("--iters must be at least 100, and both iteration counts multiples of %d" % ROUNDS)
    import torch
    import torch.nn.functional as TF
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.functional import cspn_max8_propagate
    if not torch.cuda.is_available():
        sys.exit("max8_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)

    def note(msg):
        print("max8_bench: " + msg, file=sys.stderr, flush=True)

    ones = torch.ones(8, 1, 3, 3, device=dev)

    def stock(g, d, s):
        gate = g[:, :8].abs()
        norm = TF.conv2d(gate, ones, padding=1, groups=8)
        if s is not None:
            m = s.sign()
            d = (1 - m) * d + m * s
        for _ in range(T):
            o = TF.conv2d(gate * d, ones, padding=1, groups=8) / norm
            o0, o1, o2, o3, o4, o5, o6, o7 = o.split(1, dim=1)
            d = torch.max(torch.max(torch.max(o0, o1), torch.max(o2, o3)), torch.max(torch.max(o4, o5), torch.max(o6, o7)))
            if s is not None:
                d = (1 - m) * d + m * s
        return d

    def measure(runners, iters, times):
        for name, fn in runners.items():
            times.setdefault(name, [])
            for _ in range(a.warmup if iters == a.iters else 4):
                fn()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for name, fn in runners.items():
                evs = []
                for _ in range(iters // ROUNDS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                times[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]

    results = {}
    for tag, shape, sparse in SHAPES:
        B, C, H, W = shape
        gen = torch.Generator(device=dev).manual_seed(19)
        g = torch.randn(shape, generator=gen, device=dev).requires_grad_(True)
        d = (torch.rand((B, 1, H, W), generator=gen, device=dev) * 9.5 + 0.5).requires_grad_(True)
        s = None
        if sparse:
            u = torch.rand((B, 1, H, W), generator=gen, device=dev)
            s = torch.where(u < 0.05, torch.rand((B, 1, H, W), generator=gen, device=dev) * 9.5 + 0.5, torch.zeros_like(u))
        cot = torch.randn((B, 1, H, W), generator=gen, device=dev)

        def fwd(S):
            with torch.no_grad():
                return cspn_max8_propagate(g, d, s, T, S)

        def step():
            return torch.autograd.grad(cspn_max8_propagate(g, d, s, T), (g, d), cot)

        def stock_fwd():
            with torch.no_grad():
                return stock(g, d, s)

        def stock_step():
            return torch.autograd.grad(stock(g, d, s), (g, d), cot)

        base = fwd(0)
        for S in SWEEP:
            assert torch.equal(fwd(S).view(torch.int32), base.view(torch.int32)), "steps_per_launch %d changes bits" % S
        want = stock_fwd()
        fwd_err = float(((base - want).abs() / want.abs().clamp_min(1e-6)).max())
        assert fwd_err <= 1e-4, fwd_err
        gg, gb = step()
        sg, sb = stock_step()
        grad_err = tuple(float(((x - y).abs() > 1e-4 * y.abs().max()).float().mean()) for x, y in ((gg[:, :8], sg[:, :8]), (gb, sb)))
        assert max(grad_err) <= 1e-3, grad_err
        note("%s: forwards agree (%.2e against the stock port), share of gradient elements off by more than 1e-4 of the largest: "
             "%.2e %.2e" % ((tag, fwd_err) + grad_err))
        del want, gg, gb, sg, sb

        times = {}
        runners = dict(("fwd_s%d" % S, (lambda S=S: fwd(S))) for S in SWEEP + (0,))
        runners["step"] = step
        measure(runners, a.iters, times)
        note("%s: engine timed" % tag)
        measure(dict(stock_fwd=stock_fwd, stock_step=stock_step), a.stock_iters, times)
        note("%s: stock port timed" % tag)

        floor_bytes = (32 + 4 + 4 + (4 if sparse else 0)) * B * H * W
        floor_us = floor_bytes / HBM_PEAK * 1e6
        r = dict(shape=list(shape), sparse=sparse, T=T, compulsory_bytes=floor_bytes, floor_us=round(floor_us, 2),
                 forward_rel_err_vs_stock=fwd_err, grad_share_off_vs_stock=list(grad_err))
        for name, ts in times.items():
            med = statistics.median(ts)
            r[name + "_us"] = round(med, 2)
            r[name + "_us_min"] = round(min(ts), 2)
            r[name + "_iters"] = len(ts)
            if name.startswith("fwd_s"):
                r[name + "_over_floor"] = round(med / floor_us, 2)
        sweep = dict((S, r["fwd_s%d_us" % S]) for S in SWEEP)
        r["fastest_steps_per_launch"] = min(sweep, key=sweep.get)
        r["stock_fwd_over_fwd"] = round(r["stock_fwd_us"] / r["fwd_s0_us"], 2)
        r["stock_step_over_step"] = round(r["stock_step_us"] / r["step_us"], 2)
        results[tag] = r
        del g, d, s, cot, base
        torch.cuda.empty_cache()

    out = dict(tool="max8_bench", dtype="float32", warmup=a.warmup, results=results, device=torch.cuda.get_device_name(0),
               torch=torch.__version__, code_digest=_lib.code_digest(), hbm_peak_bytes_per_s=HBM_PEAK,
               method="HIP events around each call, variants alternating in %d rounds, median; eager calls, host launch gaps included"
                      % ROUNDS)
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

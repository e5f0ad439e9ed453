#!/usr/bin/env python3
"""Times of the two output heads at 24 x 64 x 114 x 152 -> 228 x 304 with heads (1, 8), fp32, on one GPU in one process:

  fused_fwd / fused_step    network.up_pooling.up_pooling_conv3x3 (include/cspn_heads.h): forward; forward + backward
  stock_fwd / stock_step    the two Simple_Gudi_UpConv_Block_Last_Layer blocks as the models run them by default (cspn_unpool2d +
                            the stock convolution, per head)

    python tools/heads_bench.py [--iters 200] [--warmup 10] [--out profiles/r17_heads_bench.json]
    python tools/heads_bench.py --half [--out profiles/r24_head16_bench.json]

--half: the same shape in half precision, forward only — `fused_fwd` is network.up_pooling.up_pooling_conv3x3_half
(include/cspn_head16.h) on fp32 filters (autocast) and `fused_fwd_w16` on fp16 filters (``half()``), `stock_fwd` the two stock
blocks on half tensors — with the ratio to stock and the share of the HBM floor (x once plus the outputs once, at 2 bytes).

Method: every variant is captured once in a graph (forward + backward: torch.autograd.grad to x and both weights with fixed output
gradients) and timed as graph replays with HIP events around each replay, the variants alternating in 4 rounds, the median over all
of a variant's replays.  `warm`: replays back to back.  `cold`: a 512 MB buffer is overwritten before every replay, outside the
events, so that neither the L2 nor the Infinity Cache holds the inputs.  Before anything is timed the fused outputs and gradients
must agree with the stock ones to 1e-4 of the largest element (both are fp32 sums of the same terms; the figures are recorded).
Beside the fused forward: the floor counted from the shapes — x read once and the outputs written once at the 8 TB/s HBM peak, and
9 multiply-adds per compact pixel, channel and output channel at the fp32 vector peak (157.3 TFLOP/s) — and the time's multiple
of each.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
VECTOR_PEAK_FMAS = 157.3e12 / 2
ROUNDS = 4
SHAPE, OUT, HEADS = (24, 64, 114, 152), (228, 304), (1, 8)


def capture_and_time(torch, dev, variants, iters, warmup, note):
    """name -> function: each captured once in a graph and timed as replays, alternating; {mode: {name: [us, ...]}}."""
    graphs = {}
    for name, fn in variants.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = fn()
        graphs[name] = (g, keep)
        for _ in range(warmup):
            g.replay()
        torch.cuda.synchronize()
        note(name + " captured")
    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)
    times = dict((mode, dict((n, []) for n in variants)) for mode in ("warm", "cold"))
    for mode in ("warm", "cold"):
        for _ in range(ROUNDS):
            for name, (g, _) in graphs.items():
                evs = []
                for _ in range(iters // ROUNDS):
                    if mode == "cold":
                        flush.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    g.replay()
                    e1.record()
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                times[mode][name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]
        note(mode + " timed")
    return times


def half_leg(a, torch, dev, note):
    """The --half leg: the fused half heads against the two stock blocks on half tensors, forward only."""
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.network import unet_ours
    from cspn_monodepth_amd.network.up_pooling import up_pooling_conv3x3_half
    N, C, H, W = SHAPE
    oh, ow = OUT
    gen = torch.Generator(device=dev).manual_seed(26)
    x = torch.randn(SHAPE, generator=gen, device=dev).half()
    blocks = [unet_ours.Simple_Gudi_UpConv_Block_Last_Layer(C, o, oh, ow).to(dev) for o in HEADS]
    w32 = [b.conv1.weight.detach().clone() for b in blocks]
    for b in blocks:
        b.half()
    w16 = [b.conv1.weight.detach() for b in blocks]

    def no_grad(f):
        def run():
            with torch.no_grad():
                return list(f())
        return run

    variants = dict(fused_fwd=no_grad(lambda: up_pooling_conv3x3_half(x, w32, oh, ow)),
                    fused_fwd_w16=no_grad(lambda: up_pooling_conv3x3_half(x, w16, oh, ow)),
                    stock_fwd=no_grad(lambda: tuple(b(x) for b in blocks)))
    got, got16, want = variants["fused_fwd"](), variants["fused_fwd_w16"](), variants["stock_fwd"]()
    assert all(torch.equal(p, q) for p, q in zip(got, got16))
    agree = [float((g.float() - w_.float()).abs().max() / w_.float().abs().max()) for g, w_ in zip(got, want)]
    assert max(agree) <= 1e-2, agree          # a sanity check on the wiring, not a bound: how the stock half convolution accumulates is its own
    note("fused against stock in half, largest difference over largest element (y0, y1): " + " ".join("%.2e" % v for v in agree))
    del got, got16, want
    times = capture_and_time(torch, dev, variants, a.iters, a.warmup, note)
    x_bytes = N * C * H * W * 2
    out_bytes = N * sum(HEADS) * oh * ow * 2
    macs = N * H * W * C * 9 * sum(HEADS)
    hbm_floor_us = (x_bytes + out_bytes) / HBM_PEAK * 1e6
    r = dict(shape=list(SHAPE), out=list(OUT), heads=list(HEADS), x_bytes=x_bytes, out_bytes=out_bytes, macs=macs,
             hbm_floor_us=round(hbm_floor_us, 2), stock_unpooled_map_bytes=N * C * oh * ow * 2, fused_vs_stock_max_diff_over_max=agree)
    for mode in times:
        for name, ts in times[mode].items():
            key = "%s_%s" % (name, mode)
            r[key + "_us"] = round(statistics.median(ts), 2)
            r[key + "_us_min"] = round(min(ts), 2)
            q = statistics.quantiles(ts, n=10)
            r[key + "_us_p10"], r[key + "_us_p90"] = round(q[0], 2), round(q[-1], 2)
            r[key + "_iters"] = len(ts)
        for name in ("fused_fwd", "fused_fwd_w16"):
            r["%s_%s_hbm_fraction" % (name, mode)] = round(hbm_floor_us / r["%s_%s_us" % (name, mode)], 3)
            r["stock_fwd_over_%s_%s" % (name, mode)] = round(r["stock_fwd_%s_us" % mode] / r["%s_%s_us" % (name, mode)], 2)
    return dict(tool="heads_bench", dtype="float16", warmup=a.warmup, result=r, device=torch.cuda.get_device_name(0),
                torch=torch.__version__, code_digest=_lib.code_digest(), hbm_peak_bytes_per_s=HBM_PEAK,
                method="graph replays, HIP events around each, variants alternating in %d rounds, median; cold: 512 MB overwritten "
                       "before every replay, outside the events" % ROUNDS)


def emit(out, path):
    line = json.dumps(out, sort_keys=True)
    if path:
        with open(path, "w") as fh:
            fh.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--half", action="store_true", help="the half-precision forward (include/cspn_head16.h) against the stock half blocks")
    a = ap.parse_args()
    if a.iters < 40 or a.iters % ROUNDS:
        ap.error("--iters must be at least 40 and a multiple of %d" % ROUNDS)
    if a.half:
        import torch
        if not torch.cuda.is_available():
            sys.exit("heads_bench: needs a ROCm GPU (a CPU run says nothing about the time)")

        def note(msg):
            print("heads_bench: " + msg, file=sys.stderr, flush=True)

        return emit(half_leg(a, torch, torch.device("cuda", 0), note), a.out)
    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.network import unet_ours
    from cspn_monodepth_amd.network.up_pooling import up_pooling_conv3x3
    if not torch.cuda.is_available():
        sys.exit("heads_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)

    def note(msg):
        print("heads_bench: " + msg, file=sys.stderr, flush=True)

    N, C, H, W = SHAPE
    oh, ow = OUT
    gen = torch.Generator(device=dev).manual_seed(26)
    x = torch.randn(SHAPE, generator=gen, device=dev).requires_grad_(True)
    blocks = [unet_ours.Simple_Gudi_UpConv_Block_Last_Layer(C, o, oh, ow).to(dev) for o in HEADS]
    ws = [b.conv1.weight for b in blocks]
    gys = [torch.randn((N, o, oh, ow), generator=gen, device=dev) for o in HEADS]

    def fused():
        return up_pooling_conv3x3(x, tuple(ws), oh, ow)

    def stock():
        return tuple(b(x) for b in blocks)

    def forward_only(f):
        def run():
            with torch.no_grad():
                return list(f())
        return run

    def step(f):
        def run():
            ys = f()
            return list(ys) + list(torch.autograd.grad(ys, [x] + ws, gys))
        return run

    variants = dict(fused_fwd=forward_only(fused), stock_fwd=forward_only(stock), fused_step=step(fused), stock_step=step(stock))

    got, want = variants["fused_step"](), variants["stock_step"]()
    agree = [float((g - w_).abs().max() / w_.abs().max()) for g, w_ in zip(got, want)]
    assert max(agree) <= 1e-4, agree
    note("fused against stock, largest difference over largest element (y0, y1, gx, gw0, gw1): " + " ".join("%.2e" % v for v in agree))
    del got, want

    times = capture_and_time(torch, dev, variants, a.iters, a.warmup, note)

    x_bytes = N * C * H * W * 4
    out_bytes = N * sum(HEADS) * oh * ow * 4
    fmas = N * H * W * C * 9 * sum(HEADS)
    hbm_floor_us = (x_bytes + out_bytes) / HBM_PEAK * 1e6
    vector_floor_us = fmas / VECTOR_PEAK_FMAS * 1e6
    r = dict(shape=list(SHAPE), out=list(OUT), heads=list(HEADS), x_bytes=x_bytes, out_bytes=out_bytes, fmas=fmas,
             hbm_floor_us=round(hbm_floor_us, 2), vector_floor_us=round(vector_floor_us, 2),
             stock_unpooled_map_bytes=N * C * oh * ow * 4, fused_vs_stock_max_diff_over_max=agree)
    for mode in times:
        for name, ts in times[mode].items():
            key = "%s_%s" % (name, mode)
            r[key + "_us"] = round(statistics.median(ts), 2)
            r[key + "_us_min"] = round(min(ts), 2)
            r[key + "_iters"] = len(ts)
        r["fused_fwd_%s_hbm_fraction" % mode] = round(hbm_floor_us / r["fused_fwd_%s_us" % mode], 3)
        r["fused_fwd_%s_vector_fraction" % mode] = round(vector_floor_us / r["fused_fwd_%s_us" % mode], 3)
        r["stock_fwd_over_fused_fwd_%s" % mode] = round(r["stock_fwd_%s_us" % mode] / r["fused_fwd_%s_us" % mode], 2)
        r["stock_step_over_fused_step_%s" % mode] = round(r["stock_step_%s_us" % mode] / r["fused_step_%s_us" % mode], 2)
    out = dict(tool="heads_bench", dtype="float32", warmup=a.warmup, result=r, device=torch.cuda.get_device_name(0),
               torch=torch.__version__, code_digest=_lib.code_digest(), hbm_peak_bytes_per_s=HBM_PEAK,
               vector_peak_fmas_per_s=VECTOR_PEAK_FMAS,
               method="graph replays, HIP events around each, variants alternating in %d rounds, median; cold: 512 MB overwritten "
                      "before every replay, outside the events" % ROUNDS)
    emit(out, a.out)


if __name__ == "__main__":
    main()

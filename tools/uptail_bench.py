#!/usr/bin/env python3
"""Times of the 3x3 tail of the four NYU decoder blocks of unet_ours.resnet50 at B = 24, eval mode, fp32 and fp16, on one GPU in one
process (the stages of tools/upconv_bench.py and tools/uphalf_bench.py):

  stage 1  gud_up_proj_layer1  Gudi_UpProj_Block      1024 ch  15 x 19     conv2 1024 -> 1024
  stage 2  gud_up_proj_layer2  Gudi_UpProj_Block_Cat   512 ch  29 x 38     conv1_1 512 + 512 -> 512, conv2 512 -> 512
  stage 3  gud_up_proj_layer3  Gudi_UpProj_Block_Cat   256 ch  57 x 76     conv1_1 256 + 256 -> 256, conv2 256 -> 256
  stage 4  gud_up_proj_layer4  Gudi_UpProj_Block_Cat    64 ch  114 x 152   conv1_1 64 + 64 -> 64, conv2 64 -> 64

  fused  network.up_pooling.conv3x3_bn_act per convolution on packs made once (include/cspn_uptail.h): one launch for stage 1, two
         for the others, no ``cat``
  stock  the same sub-graph as the blocks run it by default: ``cat``, conv1_1, bn1_1, ReLU, conv2, bn2, the shortcut add and the ReLU on
         stock ops (half: on the modules of ``block.half()``), with the package's MIOpen tuning database in place as bench.py puts it
         (network.conv_tuning)

    python tools/uptail_bench.py [--iters 40] [--warmup 5] [--stages 1,2,3,4] [--out profiles/r21_uptail_bench.json]

Method, as uphalf_bench: every variant of a stage is captured once in a graph under no_grad and timed as graph replays with HIP
events around each replay, the variants alternating in 4 rounds; median, 10th and 90th percentile over all of a variant's replays.
`warm`: replays back to back.  `cold`: a 512 MB buffer is overwritten before every replay, outside the events.  Before anything is
timed the two paths must agree (fp32: 1e-3, fp16: 1e-2 of the largest element; the figures are recorded).  `fused_ahead`: the fused
tail's 90th percentile is below the stock tail's 10th percentile, warm and cold — the rule behind up_pooling.FUSED_TAIL_DEFAULT and
FUSED_TAIL_HALF_DEFAULT.  Beside the fused times the floors counted from the shapes: 9 Cin O B H W multiply-adds per convolution at
the dense matrix peak of the precision (fp32 157.3 TFLOP/s, fp16 2.5 PFLOP/s), and every operand, the packed filters, the
intermediate (written and read) and the result moved once at the 8 TB/s HBM peak.  Needs a ROCm GPU; prints one JSON line."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
MATRIX_PEAK_FLOPS = {"float32": 157.3e12, "float16": 2.5e15}
ROUNDS = 4
BATCH = 24
STAGES = {1: ("gud_up_proj_layer1", False, 1024, (15, 19)), 2: ("gud_up_proj_layer2", True, 512, (29, 38)),
          3: ("gud_up_proj_layer3", True, 256, (57, 76)), 4: ("gud_up_proj_layer4", True, 64, (114, 152))}


def percentile(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


def counted(cat, O, H, W, esize):
    """Multiply-adds and bytes of one tail, from the shapes."""
    pixels = BATCH * H * W
    macs = 9 * O * O * pixels * (3 if cat else 1)                 # conv1_1 reads 2 O channels
    maps = (6 if cat else 3) * O * pixels                        # out, shortcut, result; side, and the intermediate twice
    packed = 9 * O * O * (3 if cat else 1)
    return macs, (maps + packed) * esize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stages", default="1,2,3,4")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20 or a.iters % ROUNDS:
        ap.error("--iters must be at least 20 and a multiple of %d" % ROUNDS)
    stages = [int(s) for s in a.stages.split(",")]
    from cspn_monodepth_amd.network import conv_tuning
    conv_db = conv_tuning.use_tuned_conv_db()
    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.network import unet_ours
    from cspn_monodepth_amd.network.up_pooling import conv3x3_bn_act, pack_conv3x3
    if not torch.cuda.is_available():
        sys.exit("uptail_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)

    def note(msg):
        print("uptail_bench: " + msg, file=sys.stderr, flush=True)

    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)
    results = {}
    for s in stages:
        name, cat, O, (H, W) = STAGES[s]
        gen = torch.Generator(device=dev).manual_seed(31 + s)
        torch.manual_seed(31 + s)
        block = (unet_ours.Gudi_UpProj_Block_Cat if cat else unet_ours.Gudi_UpProj_Block)(2 * O, O, H, W).to(dev).eval()
        with torch.no_grad():
            for bn in [block.bn2] + ([block.bn1_1] if cat else []):
                bn.running_mean.normal_(0, 0.1, generator=gen)
                bn.running_var.uniform_(0.5, 1.5, generator=gen)
                bn.weight.normal_(1.0, 0.2, generator=gen)
                bn.bias.normal_(0, 0.1, generator=gen)
        out32 = torch.randn((BATCH, O, H, W), generator=gen, device=dev).relu_()
        short32 = torch.randn((BATCH, O, H, W), generator=gen, device=dev)
        side32 = torch.randn((BATCH, O, H, W), generator=gen, device=dev) if cat else None
        r = dict(block=name, maps=[BATCH, O, H, W], cat=cat)
        for dtype, key, tol in ((torch.float32, "float32", 1e-3), (torch.float16, "float16", 1e-2)):
            blk = block if dtype == torch.float32 else copy.deepcopy(block).half()
            out, short, side = (None if t is None else t.to(dtype) for t in (out32, short32, side32))
            p1 = pack_conv3x3(blk.conv1_1.weight, blk.bn1_1, O, dtype) if cat else None
            p2 = pack_conv3x3(blk.conv2.weight, blk.bn2, None, dtype)

            def fused():
                with torch.no_grad():
                    mid = conv3x3_bn_act(out, p1, side) if cat else out
                    return conv3x3_bn_act(mid, p2, residual=short)

            def stock():
                with torch.no_grad():
                    mid = blk.relu(blk.bn1_1(blk.conv1_1(torch.cat((out, side), 1)))) if cat else out
                    return blk.relu(blk.bn2(blk.conv2(mid)) + short)

            variants = dict(fused=fused, stock=stock)
            got, want = fused(), stock()
            assert got.dtype == want.dtype == dtype and got.shape == want.shape
            agree = float((got.float() - want.float()).abs().max() / want.float().abs().max())
            assert agree <= tol, (name, key, agree)
            note("%s %s: fused against stock, largest difference over largest element: %.2e" % (name, key, agree))
            del got, want

            graphs = {}
            for vname, fn in variants.items():
                side_stream = torch.cuda.Stream()
                side_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side_stream):
                    for _ in range(3):
                        fn()
                torch.cuda.current_stream().wait_stream(side_stream)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    keep = fn()
                graphs[vname] = (g, keep)
                for _ in range(a.warmup):
                    g.replay()
                torch.cuda.synchronize()
            times = dict((mode, dict((n, []) for n in variants)) for mode in ("warm", "cold"))
            for mode in ("warm", "cold"):
                for _ in range(ROUNDS):
                    for vname, (g, _) in graphs.items():
                        evs = []
                        for _ in range(a.iters // ROUNDS):
                            if mode == "cold":
                                flush.zero_()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            g.replay()
                            e1.record()
                            evs.append((e0, e1))
                        torch.cuda.synchronize()
                        times[mode][vname] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]
            macs, nbytes = counted(cat, O, H, W, 4 if dtype == torch.float32 else 2)
            matrix_floor_us = 2 * macs / MATRIX_PEAK_FLOPS[key] * 1e6
            hbm_floor_us = nbytes / HBM_PEAK * 1e6
            d = dict(multiply_adds=macs, bytes=nbytes, matrix_floor_us=round(matrix_floor_us, 2), hbm_floor_us=round(hbm_floor_us, 2),
                     floor_bound="matrix" if matrix_floor_us > hbm_floor_us else "hbm", fused_vs_stock_max_diff_over_max=agree,
                     launches_fused=2 if cat else 1)
            ahead = True
            for mode in times:
                for vname, ts in times[mode].items():
                    k = "%s_%s" % (vname, mode)
                    d[k + "_us"] = round(statistics.median(ts), 2)
                    d[k + "_us_p10"] = round(percentile(ts, 0.1), 2)
                    d[k + "_us_p90"] = round(percentile(ts, 0.9), 2)
                    d[k + "_iters"] = len(ts)
                d["fused_%s_matrix_fraction" % mode] = round(matrix_floor_us / d["fused_%s_us" % mode], 3)
                d["fused_%s_hbm_fraction" % mode] = round(hbm_floor_us / d["fused_%s_us" % mode], 3)
                d["stock_over_fused_%s" % mode] = round(d["stock_%s_us" % mode] / d["fused_%s_us" % mode], 2)
                ahead = ahead and d["fused_%s_us_p90" % mode] < d["stock_%s_us_p10" % mode]
            d["fused_ahead"] = ahead
            r[key] = d
            note("%s %s: fused %.0f / %.0f us, stock %.0f / %.0f us (warm / cold), ahead: %s" % (
                name, key, d["fused_warm_us"], d["fused_cold_us"], d["stock_warm_us"], d["stock_cold_us"], ahead))
            del graphs, variants, fused, stock, keep, g, p1, p2, out, short, side, blk
            torch.cuda.empty_cache()
        results[name] = r
        del block, out32, short32, side32
        torch.cuda.empty_cache()

    def total(key, what):
        return round(sum(r[key][what] for r in results.values()), 2)

    sums = dict((key, dict((what, total(key, what)) for what in ("fused_warm_us", "fused_cold_us", "stock_warm_us", "stock_cold_us", "matrix_floor_us")))
                for key in MATRIX_PEAK_FLOPS)
    out = dict(tool="uptail_bench", batch=BATCH, warmup=a.warmup, stages=results, sums=sums,
               fused_ahead=dict((key, [n for n, r in results.items() if r[key]["fused_ahead"]]) for key in MATRIX_PEAK_FLOPS),
               device=torch.cuda.get_device_name(0), torch=torch.__version__, code_digest=_lib.code_digest(),
               conv_db=bool(conv_db or os.environ.get("MIOPEN_USER_DB_PATH")), hbm_peak_bytes_per_s=HBM_PEAK,
               matrix_peak_flops_per_s=MATRIX_PEAK_FLOPS,
               method="graph replays, HIP events around each, variants alternating in %d rounds, median and 10th / 90th percentile; cold: "
                      "512 MB overwritten before every replay, outside the events" % ROUNDS)
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

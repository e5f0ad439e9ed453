#!/usr/bin/env python3
"""Times of the head of the four NYU decoder blocks of unet_ours.resnet50 at B = 24 in half precision, eval mode, on one GPU in one
process (the stages of tools/upconv_bench.py):

  stage 1  gud_up_proj_layer1  2048 -> 2 x 1024   8 x 10  -> 15 x 19
  stage 2  gud_up_proj_layer2  1024 -> 2 x 512    15 x 19 -> 29 x 38
  stage 3  gud_up_proj_layer3   512 -> 2 x 256    29 x 38 -> 57 x 76
  stage 4  gud_up_proj_layer4   256 -> 2 x 64     57 x 76 -> 114 x 152

  half        network.up_pooling.up_pooling_conv5x5 on a half x and a pack of dtype fp16 made once (include/cspn_uphalf.h)
  stock_half  the same sub-graph as the blocks of model.half() run it by default: cspn_unpool2d, conv1, bn1, ReLU, sc_conv1, sc_bn1
              on half tensors (stock convolutions and batch norms), with the package's MIOpen tuning database in place as bench.py
              puts it (network.conv_tuning)
  fused_fp32  the fp32 kernel (include/cspn_upconv.h) on the same values in fp32: what a user of `fused_decoder` has today

    python tools/uphalf_bench.py [--iters 40] [--warmup 5] [--stages 1,2,3,4] [--out profiles/r19_uphalf_bench.json]

Method, as upconv_bench: every variant of a stage is captured once in a graph under no_grad and timed as graph replays with HIP
events around each replay, the variants alternating in 4 rounds; median, 10th and 90th percentile over all of a variant's replays.
`warm`: replays back to back.  `cold`: a 512 MB buffer is overwritten before every replay, outside the events, so that neither the
L2 nor the Infinity Cache holds the inputs.  Before anything is timed the half outputs must agree with the stock half ones to 1e-2
of the largest element (a few fp16 roundings on either side; the figures are recorded).  `half_ahead`: the half kernel's 90th
percentile is below the stock half head's 10th percentile, warm and cold — the rule behind up_pooling.FUSED_DECODER_HALF_DEFAULT.
Beside the half kernel's times the floors counted from the shapes: 25 C (O1 + O2) B H W multiply-adds at the dense fp16 matrix peak
(2.5 PFLOP/s), and x, the packed filters and both outputs moved once at the 8 TB/s HBM peak.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
MATRIX_PEAK_FLOPS_F16 = 2.5e15
ROUNDS = 4
BATCH = 24
STAGES = {1: ("gud_up_proj_layer1", 2048, 1024, (8, 10), (15, 19)), 2: ("gud_up_proj_layer2", 1024, 512, (15, 19), (29, 38)),
          3: ("gud_up_proj_layer3", 512, 256, (29, 38), (57, 76)), 4: ("gud_up_proj_layer4", 256, 64, (57, 76), (114, 152))}


def percentile(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


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
    import copy
    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.network import unet_ours
    from cspn_monodepth_amd.network.up_pooling import pack_upconv5x5, up_pooling_conv5x5
    if not torch.cuda.is_available():
        sys.exit("uphalf_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)

    def note(msg):
        print("uphalf_bench: " + msg, file=sys.stderr, flush=True)

    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)
    results = {}
    for s in stages:
        name, C, O, (H, W), (oh, ow) = STAGES[s]
        gen = torch.Generator(device=dev).manual_seed(27 + s)
        torch.manual_seed(27 + s)
        block = unet_ours.Gudi_UpProj_Block(C, O, oh, ow).to(dev).eval()       # the head is the same in the _Cat blocks
        with torch.no_grad():
            for bn in (block.bn1, block.sc_bn1):
                bn.running_mean.normal_(0, 0.1, generator=gen)
                bn.running_var.uniform_(0.5, 1.5, generator=gen)
                bn.weight.normal_(1.0, 0.2, generator=gen)
                bn.bias.normal_(0, 0.1, generator=gen)
        x = torch.randn((BATCH, C, H, W), generator=gen, device=dev)
        xh = x.half()
        hblock = copy.deepcopy(block).half()                                  # what model.half() makes of the block
        pack32 = pack_upconv5x5((block.conv1.weight, block.sc_conv1.weight), (block.bn1, block.sc_bn1))
        pack16 = pack_upconv5x5((hblock.conv1.weight, hblock.sc_conv1.weight), (hblock.bn1, hblock.sc_bn1), dtype=torch.float16)

        def half():
            with torch.no_grad():
                return list(up_pooling_conv5x5(xh, pack16, oh, ow))

        def stock_half():
            with torch.no_grad():
                u = hblock._up_pooling(xh, 2)
                return [hblock.relu(hblock.bn1(hblock.conv1(u))), hblock.sc_bn1(hblock.sc_conv1(u))]

        def fused_fp32():
            with torch.no_grad():
                return list(up_pooling_conv5x5(x, pack32, oh, ow))

        variants = dict(half=half, stock_half=stock_half, fused_fp32=fused_fp32)
        got, want, full = half(), stock_half(), fused_fp32()
        assert all(g.dtype == torch.float16 and w_.dtype == torch.float16 for g, w_ in zip(got, want))
        agree = [float((g.float() - w_.float()).abs().max() / w_.float().abs().max()) for g, w_ in zip(got, want)]
        agree32 = [float((g.float() - f).abs().max() / f.abs().max()) for g, f in zip(got, full)]
        stock32 = [float((w_.float() - f).abs().max() / f.abs().max()) for w_, f in zip(want, full)]
        assert max(agree) <= 1e-2, (name, agree)
        note("%s: half against stock half, largest difference over largest element: %s; against the fp32 kernel: half %s, stock half %s"
             % (name, " ".join("%.2e" % v for v in agree), " ".join("%.2e" % v for v in agree32), " ".join("%.2e" % v for v in stock32)))
        del got, want, full

        graphs = {}
        for vname, fn in variants.items():
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
        x_bytes, out_bytes, packed_bytes = xh.numel() * 2, 2 * BATCH * O * oh * ow * 2, pack16.packed.numel() * 2
        flops = 25 * C * 2 * O * BATCH * H * W * 2
        matrix_floor_us = flops / MATRIX_PEAK_FLOPS_F16 * 1e6
        hbm_floor_us = (x_bytes + packed_bytes + out_bytes) / HBM_PEAK * 1e6
        r = dict(block=name, x=[BATCH, C, H, W], out=[oh, ow], out_channels=[O, O], x_bytes=x_bytes, packed_bytes=packed_bytes,
                 out_bytes=out_bytes, flops=flops, stock_flops=2 * 25 * C * 2 * O * BATCH * oh * ow, matrix_floor_us=round(matrix_floor_us, 2),
                 hbm_floor_us=round(hbm_floor_us, 2), floor_bound="matrix" if matrix_floor_us > hbm_floor_us else "hbm",
                 stock_unpooled_map_bytes=BATCH * C * oh * ow * 2, half_vs_stock_half_max_diff_over_max=agree,
                 half_vs_fused_fp32_max_diff_over_max=agree32, stock_half_vs_fused_fp32_max_diff_over_max=stock32)
        ahead = True
        for mode in times:
            for vname, ts in times[mode].items():
                key = "%s_%s" % (vname, mode)
                r[key + "_us"] = round(statistics.median(ts), 2)
                r[key + "_us_p10"] = round(percentile(ts, 0.1), 2)
                r[key + "_us_p90"] = round(percentile(ts, 0.9), 2)
                r[key + "_iters"] = len(ts)
            r["half_%s_matrix_fraction" % mode] = round(matrix_floor_us / r["half_%s_us" % mode], 3)
            r["half_%s_hbm_fraction" % mode] = round(hbm_floor_us / r["half_%s_us" % mode], 3)
            r["stock_half_over_half_%s" % mode] = round(r["stock_half_%s_us" % mode] / r["half_%s_us" % mode], 2)
            r["fused_fp32_over_half_%s" % mode] = round(r["fused_fp32_%s_us" % mode] / r["half_%s_us" % mode], 2)
            ahead = ahead and r["half_%s_us_p90" % mode] < r["stock_half_%s_us_p10" % mode]
        r["half_ahead"] = ahead
        results[name] = r
        note("%s: half %.0f / %.0f us, stock half %.0f / %.0f us, fp32 kernel %.0f / %.0f us (warm / cold), ahead: %s" % (
            name, r["half_warm_us"], r["half_cold_us"], r["stock_half_warm_us"], r["stock_half_cold_us"], r["fused_fp32_warm_us"],
            r["fused_fp32_cold_us"], ahead))
        del graphs, block, hblock, pack16, pack32, x, xh, variants, half, stock_half, fused_fp32, keep, g
        torch.cuda.empty_cache()

    out = dict(tool="uphalf_bench", dtype="float16", batch=BATCH, warmup=a.warmup, stages=results,
               half_ahead=[n for n, r in results.items() if r["half_ahead"]], device=torch.cuda.get_device_name(0),
               torch=torch.__version__, code_digest=_lib.code_digest(), conv_db=bool(conv_db or os.environ.get("MIOPEN_USER_DB_PATH")),
               hbm_peak_bytes_per_s=HBM_PEAK, matrix_peak_flops_per_s=MATRIX_PEAK_FLOPS_F16,
               method="graph replays, HIP events around each, variants alternating in %d rounds, median and 10th / 90th percentile; cold: "
                      "512 MB overwritten before every replay, outside the events" % ROUNDS)
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

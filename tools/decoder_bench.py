#!/usr/bin/env python3
"""Times of the fused kernels of the four NYU decoder blocks of unet_ours.resnet50 at B = 24, eval mode, against the stock ops they
replace, on one GPU in one process:

  stage 1  gud_up_proj_layer1  Gudi_UpProj_Block      2048 -> 2 x 1024   8 x 10  -> 15 x 19
  stage 2  gud_up_proj_layer2  Gudi_UpProj_Block_Cat  1024 -> 2 x 512    15 x 19 -> 29 x 38
  stage 3  gud_up_proj_layer3  Gudi_UpProj_Block_Cat   512 -> 2 x 256    29 x 38 -> 57 x 76
  stage 4  gud_up_proj_layer4  Gudi_UpProj_Block_Cat   256 -> 2 x 64     57 x 76 -> 114 x 152

    python tools/decoder_bench.py {upconv,uphalf,upsplit,uptail,encoder} [--iters 40] [--warmup 5] [--stages 1,2,3,4] [--out profiles/NAME.json]

upconv, the fp32 head (include/cspn_upconv.h):
  fused       network.up_pooling.up_pooling_conv5x5 on a pack made once: both outputs in one kernel
  stock       the same sub-graph as the blocks run it by default: cspn_unpool2d, conv1, bn1, ReLU, sc_conv1, sc_bn1
uphalf, the fp16 head (include/cspn_uphalf.h):
  half        up_pooling_conv5x5 on a half x and a pack of dtype fp16 made once
  stock_half  the stock sub-graph on the modules of ``block.half()``, as model.half() runs it
  fused_fp32  the fp32 kernel on the same values in fp32: what `fused_decoder` gives without the half kernel
upsplit, the fp32 head with split products (include/cspn_upconv.h, CSPN_UPCONV_F32_BF16X3):
  split       up_pooling_conv5x5(..., precision="bf16x3") on the fp32 x and the fp32 pack of `fused`
  fused       the exact fp32 head on the same pack: what it has to be ahead of
  stock       the stock fp32 sub-graph, as under upconv
  The matrix floor is the split's own: 6 x 25 C (O1 + O2) B H W multiply-adds at the bf16 peak (2.5 PFLOP/s).  Before anything is
  timed the split must agree with the exact head to 1e-5 of the largest element; the figure is recorded.
uptail, the 3x3 tail in fp32 and in fp16 (include/cspn_uptail.h), over O channels at the stage's output size:
  fused       network.up_pooling.conv3x3_bn_act per convolution on packs made once: conv2 alone at stage 1 (one launch), conv1_1 over
              2 O channels and conv2 at the others (two launches), no ``cat``
  stock       ``cat``, conv1_1, bn1_1, ReLU, conv2, bn2, the shortcut add and the ReLU on stock ops (half: of ``block.half()``)
encoder, the residual stages layer1 .. layer4 (57 x 76 -> 8 x 10) and the bridge bn2(conv2(x)) of the same model in fp32 and in fp16
(include/cspn_convbn.h), stages 1 .. 5, and as stage 0 the whole of ``features`` (everything below the CSPN module):
  fused       network.conv_bn.conv_bn_act per convolution on packs made once, as `fused_encoder` runs a stage (stage 0: every stage)
  stock       the stage on stock ops: MIOpen convolutions, eval batch norms, adds and ReLUs (half: of ``.half()``)
  The line carries the stages' sums and `encoder_share_of_features`: the stock stages' sum over the stock time of stage 0.
The stock convolutions run with the package's MIOpen tuning database in place as bench.py puts it (network.conv_tuning).

Method: every variant of a case is captured once in a graph under no_grad and timed as graph replays with HIP events around each
replay, the variants alternating in 4 rounds; median, 10th and 90th percentile over all of a variant's replays.  `warm`: replays
back to back.  `cold`: a 512 MB buffer is overwritten before every replay, outside the events, so that neither the L2 nor the
Infinity Cache holds the inputs.  Before anything is timed the family's kernel must agree with the stock path to a share of the
largest element (fp32 head 1e-4: fp32 sums of the same terms; fp32 tail 1e-3; fp16 1e-2: a few fp16 roundings on either side); the
figures are recorded.  `<kernel>_ahead`: the 90th percentile of the family's kernel (the first variant) is below the 10th percentile
of the stock path (the second), warm and cold — the one rule behind up_pooling.FUSED_DECODER_DEFAULT, FUSED_DECODER_HALF_DEFAULT,
FUSED_TAIL_DEFAULT, FUSED_TAIL_HALF_DEFAULT and conv_bn.FUSED_ENCODER_DEFAULT / FUSED_ENCODER_HALF_DEFAULT.  Beside the kernel's times the floors counted from the shapes: its multiply-adds (head:
25 C (O1 + O2) B H W, tail: 9 Cin O B H W per convolution) at the dense matrix peak of the precision (fp32 157.3 TFLOP/s, the vector
peak as well; fp16 2.5 PFLOP/s), and every operand, the packed filters, the tail's intermediate (written and read) and the results
moved once at the 8 TB/s HBM peak.  Prints one JSON line, with the keys and the `tool` name (`<family>_bench`) of the recorded
profiles/*_bench*.json."""
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
PEAK_FLOPS = dict(MATRIX_PEAK_FLOPS, bfloat16=2.5e15)      # ... and the bf16 matrix cores the split products of upsplit run on
ROUNDS = 4
BATCH = 24
STAGES = {1: ("gud_up_proj_layer1", 2048, 1024, (8, 10), (15, 19)), 2: ("gud_up_proj_layer2", 1024, 512, (15, 19), (29, 38)),
          3: ("gud_up_proj_layer3", 512, 256, (29, 38), (57, 76)), 4: ("gud_up_proj_layer4", 256, 64, (57, 76), (114, 152))}


def percentile(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, int(q * len(ts)))]


def off(got, want):
    """Largest difference over largest element."""
    return float((got.float() - want.float()).abs().max() / want.float().abs().max())


def seeded_block(cls, C, s, seed, norms, dev):
    """Block `cls` of stage s over C channels with seeded filters and batch norms, and the generator its inputs are drawn from."""
    _, _, O, _, (oh, ow) = STAGES[s]
    gen = torch.Generator(device=dev).manual_seed(seed + s)
    torch.manual_seed(seed + s)
    block = cls(C, O, oh, ow).to(dev).eval()
    with torch.no_grad():
        for bn in (getattr(block, n) for n in norms):
            bn.running_mean.normal_(0, 0.1, generator=gen)
            bn.running_var.uniform_(0.5, 1.5, generator=gen)
            bn.weight.normal_(1.0, 0.2, generator=gen)
            bn.bias.normal_(0, 0.1, generator=gen)
    return block, gen


def replay_times(variants, iters, warmup, flush):
    """Microseconds per replay: {"warm" | "cold": {variant: [...]}}."""
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
        for _ in range(warmup):
            g.replay()
        torch.cuda.synchronize()
    times = dict((mode, dict((n, []) for n in variants)) for mode in ("warm", "cold"))
    for mode in times:
        for _ in range(ROUNDS):
            for vname, (g, _) in graphs.items():
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
                times[mode][vname] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]
    return times


def summarise(d, times, matrix_floor_us, hbm_floor_us):
    """The timed keys of a case into d.  The first variant is the family's kernel: the floors and every `<other>_over_<kernel>` ratio
    are taken against it; the second is the stock path it has to be ahead of."""
    kernel, stock = list(times["warm"])[:2]
    ahead = True
    for mode, by_variant in times.items():
        for vname, ts in by_variant.items():
            key = "%s_%s" % (vname, mode)
            d[key + "_us"] = round(statistics.median(ts), 2)
            d[key + "_us_p10"] = round(percentile(ts, 0.1), 2)
            d[key + "_us_p90"] = round(percentile(ts, 0.9), 2)
            d[key + "_iters"] = len(ts)
        us = d["%s_%s_us" % (kernel, mode)]
        d["%s_%s_matrix_fraction" % (kernel, mode)] = round(matrix_floor_us / us, 3)
        d["%s_%s_hbm_fraction" % (kernel, mode)] = round(hbm_floor_us / us, 3)
        for other in by_variant:
            if other != kernel:
                d["%s_over_%s_%s" % (other, kernel, mode)] = round(d["%s_%s_us" % (other, mode)] / us, 2)
        ahead = ahead and d["%s_%s_us_p90" % (kernel, mode)] < d["%s_%s_us_p10" % (stock, mode)]
    d["%s_ahead" % kernel] = ahead


# A family is a generator of the cases of a stage and the family's part of the JSON line.  A case is (d, label, variants, flops, bytes,
# precision): d, somewhere in the stage's result r, holds what the family counted and is given the floors and the times; the agreement
# of the variants has been asserted by then.


def head(s, dev):
    """What both heads run on: the block, its input and what is counted from the shapes per element size."""
    name, C, O, (H, W), (oh, ow) = STAGES[s]
    block, gen = seeded_block(unet_ours.Gudi_UpProj_Block, C, s, 27, ("bn1", "sc_bn1"), dev)       # the head is the same in the _Cat blocks
    x = torch.randn((BATCH, C, H, W), generator=gen, device=dev)

    def counted(r, pack, esize):
        r.update(block=name, x=[BATCH, C, H, W], out=[oh, ow], out_channels=[O, O], x_bytes=x.numel() * esize,
                 packed_bytes=pack.packed.numel() * esize, out_bytes=2 * BATCH * O * oh * ow * esize, flops=25 * C * 2 * O * BATCH * H * W * 2,
                 stock_flops=2 * 25 * C * 2 * O * BATCH * oh * ow, stock_unpooled_map_bytes=BATCH * C * oh * ow * esize)
        return r["flops"], r["x_bytes"] + r["packed_bytes"] + r["out_bytes"]

    def stock(blk, xs):
        with torch.no_grad():
            u = blk._up_pooling(xs, 2)
            return [blk.relu(blk.bn1(blk.conv1(u))), blk.sc_bn1(blk.sc_conv1(u))]

    def fused(xs, pack):
        with torch.no_grad():
            return list(up.up_pooling_conv5x5(xs, pack, oh, ow))

    return name, block, x, counted, stock, fused


def upconv_cases(s, r, dev, note):
    name, block, x, counted, stock, fused = head(s, dev)
    pack = up.pack_upconv5x5((block.conv1.weight, block.sc_conv1.weight), (block.bn1, block.sc_bn1))
    variants = dict(fused=lambda: fused(x, pack), stock=lambda: stock(block, x))
    agree = [off(g, w) for g, w in zip(variants["fused"](), variants["stock"]())]
    assert max(agree) <= 1e-4, (name, agree)
    note("%s: fused against stock, largest difference over largest element: %s" % (name, " ".join("%.2e" % v for v in agree)))
    r["fused_vs_stock_max_diff_over_max"] = agree
    yield (r, name, variants) + counted(r, pack, 4) + ("float32",)


def uphalf_cases(s, r, dev, note):
    name, block, x, counted, stock, fused = head(s, dev)
    xh = x.half()
    hblock = copy.deepcopy(block).half()                                  # what model.half() makes of the block
    pack32 = up.pack_upconv5x5((block.conv1.weight, block.sc_conv1.weight), (block.bn1, block.sc_bn1))
    pack16 = up.pack_upconv5x5((hblock.conv1.weight, hblock.sc_conv1.weight), (hblock.bn1, hblock.sc_bn1), dtype=torch.float16)
    variants = dict(half=lambda: fused(xh, pack16), stock_half=lambda: stock(hblock, xh), fused_fp32=lambda: fused(x, pack32))
    got, want, full = (fn() for fn in variants.values())
    assert all(g.dtype == torch.float16 and w.dtype == torch.float16 for g, w in zip(got, want))
    agree, agree32, stock32 = ([off(p, q) for p, q in zip(*pair)] for pair in ((got, want), (got, full), (want, full)))
    assert max(agree) <= 1e-2, (name, agree)
    note("%s: half against stock half, largest difference over largest element: %s; against the fp32 kernel: half %s, stock half %s"
         % (name, " ".join("%.2e" % v for v in agree), " ".join("%.2e" % v for v in agree32), " ".join("%.2e" % v for v in stock32)))
    del got, want, full
    r.update(half_vs_stock_half_max_diff_over_max=agree, half_vs_fused_fp32_max_diff_over_max=agree32,
             stock_half_vs_fused_fp32_max_diff_over_max=stock32)
    yield (r, name, variants) + counted(r, pack16, 2) + ("float16",)


def upsplit_cases(s, r, dev, note):
    name, block, x, counted, stock, fused = head(s, dev)
    _, _, _, _, (oh, ow) = STAGES[s]
    pack = up.pack_upconv5x5((block.conv1.weight, block.sc_conv1.weight), (block.bn1, block.sc_bn1))      # one pack for both precisions

    def split():
        with torch.no_grad():
            return list(up.up_pooling_conv5x5(x, pack, oh, ow, precision="bf16x3"))

    variants = dict(split=split, fused=lambda: fused(x, pack), stock=lambda: stock(block, x))
    got, exact, want = (fn() for fn in variants.values())
    agree, agree_stock, exact_stock = ([off(p, q) for p, q in zip(*pair)] for pair in ((got, exact), (got, want), (exact, want)))
    assert max(agree) <= 1e-5 and max(agree_stock) <= 1e-4, (name, agree, agree_stock)
    note("%s: bf16x3 against the exact fused head, largest difference over largest element: %s; against stock: bf16x3 %s, exact %s"
         % (name, " ".join("%.2e" % v for v in agree), " ".join("%.2e" % v for v in agree_stock), " ".join("%.2e" % v for v in exact_stock)))
    del got, exact, want
    r.update(split_vs_fused_max_diff_over_max=agree, split_vs_stock_max_diff_over_max=agree_stock, fused_vs_stock_max_diff_over_max=exact_stock)
    flops, nbytes = counted(r, pack, 4)
    r["split_flops"] = 6 * flops                                          # six bf16 products per fp32 one
    yield r, name, variants, r["split_flops"], nbytes, "bfloat16"


def head_line(kernel, key):
    def line(results):
        return {"dtype": key, kernel + "_ahead": [n for n, r in results.items() if r[kernel + "_ahead"]],
                "matrix_peak_flops_per_s": PEAK_FLOPS[key]}
    return line


def uptail_cases(s, r, dev, note):
    name, _, O, _, (H, W) = STAGES[s]
    cat = s > 1
    block, gen = seeded_block(unet_ours.Gudi_UpProj_Block_Cat if cat else unet_ours.Gudi_UpProj_Block, 2 * O, s, 31,
                              ("bn2", "bn1_1") if cat else ("bn2",), dev)
    out32 = torch.randn((BATCH, O, H, W), generator=gen, device=dev).relu_()
    short32 = torch.randn((BATCH, O, H, W), generator=gen, device=dev)
    side32 = torch.randn((BATCH, O, H, W), generator=gen, device=dev) if cat else None
    r.update(block=name, maps=[BATCH, O, H, W], cat=cat)
    pixels = BATCH * H * W
    macs = 9 * O * O * pixels * (3 if cat else 1)                 # conv1_1 reads 2 O channels
    maps = (6 if cat else 3) * O * pixels                        # out, shortcut, result; side, and the intermediate twice
    packed = 9 * O * O * (3 if cat else 1)
    for dtype, key, tol in ((torch.float32, "float32", 1e-3), (torch.float16, "float16", 1e-2)):
        blk = block if dtype == torch.float32 else copy.deepcopy(block).half()
        out, short, side = (None if t is None else t.to(dtype) for t in (out32, short32, side32))
        p1 = up.pack_conv3x3(blk.conv1_1.weight, blk.bn1_1, O, dtype) if cat else None
        p2 = up.pack_conv3x3(blk.conv2.weight, blk.bn2, None, dtype)

        def fused():
            with torch.no_grad():
                mid = up.conv3x3_bn_act(out, p1, side) if cat else out
                return up.conv3x3_bn_act(mid, p2, residual=short)

        def stock():
            with torch.no_grad():
                mid = blk.relu(blk.bn1_1(blk.conv1_1(torch.cat((out, side), 1)))) if cat else out
                return blk.relu(blk.bn2(blk.conv2(mid)) + short)

        got, want = fused(), stock()
        assert got.dtype == want.dtype == dtype and got.shape == want.shape
        agree = off(got, want)
        assert agree <= tol, (name, key, agree)
        note("%s %s: fused against stock, largest difference over largest element: %.2e" % (name, key, agree))
        del got, want
        nbytes = (maps + packed) * (4 if dtype == torch.float32 else 2)
        r[key] = dict(multiply_adds=macs, bytes=nbytes, fused_vs_stock_max_diff_over_max=agree, launches_fused=2 if cat else 1)
        yield r[key], "%s %s" % (name, key), dict(fused=fused, stock=stock), 2 * macs, nbytes, key


def uptail_line(results):
    whats = ("fused_warm_us", "fused_cold_us", "stock_warm_us", "stock_cold_us", "matrix_floor_us")
    return dict(sums=dict((key, dict((what, round(sum(r[key][what] for r in results.values()), 2)) for what in whats))
                          for key in MATRIX_PEAK_FLOPS),
                fused_ahead=dict((key, [n for n, r in results.items() if r[key]["fused_ahead"]]) for key in MATRIX_PEAK_FLOPS),
                matrix_peak_flops_per_s=MATRIX_PEAK_FLOPS)


# The encoder's stages: name, input channels and input size at 228 x 304 (the stem and the max-pool in front of layer1 leave 57 x 76).
# Stage 0 is the whole of `features` — everything below the CSPN module — with the switch on every stage against the stock model: the
# rest of a forward is its stock time less the stock stages'.
ENCODER_STAGES = {0: ("features", 4, (228, 304)), 1: ("layer1", 64, (57, 76)), 2: ("layer2", 256, (57, 76)), 3: ("layer3", 512, (29, 38)),
                  4: ("layer4", 1024, (15, 19)), 5: ("conv2", 2048, (8, 10))}
_encoder_model = {}


def encoder_convs(stage, C, H, W):
    """(multiply-adds, elements moved once) of a stage's fused calls on one frame, from the shapes."""
    macs = moved = 0
    blocks = list(stage) if isinstance(stage, torch.nn.Sequential) else []
    rows = []
    for b in blocks:
        convs = [getattr(b, n) for n in ("conv1", "conv2", "conv3") if hasattr(b, n)]
        rows += [(c, False) for c in convs[:-1]] + ([(b.downsample[0], False)] if b.downsample is not None else []) + [(convs[-1], True)]
    size = {}
    for b in blocks:                                             # the input size of every convolution of the block
        h, w = H, W
        for n in ("conv1", "conv2", "conv3"):
            if hasattr(b, n):
                size[getattr(b, n)] = (h, w)
                s = getattr(b, n).stride[0]
                h, w = (h - 1) // s + 1, (w - 1) // s + 1
        if b.downsample is not None:
            size[b.downsample[0]] = (H, W)
        H, W = h, w
    for conv, residual in rows:
        h, w = size[conv]
        s, k = conv.stride[0], conv.kernel_size[0]
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        macs += k * k * conv.in_channels * conv.out_channels * ho * wo
        moved += conv.in_channels * h * w + conv.out_channels * ho * wo * (2 if residual else 1)
    return macs, moved, sum(c.weight.numel() for c, _ in rows)


def encoder_cases(s, r, dev, note):
    """The residual stages and the bridge of unet_ours.resnet50 (include/cspn_convbn.h), in fp32 and in fp16:
      fused   every convolution of the stage as one network.conv_bn.conv_bn_act call on packs made once (`fused_encoder`)
      stock   the stage as the model runs it by default: MIOpen convolutions, eval batch norms, adds and ReLUs (half: of ``.half()``)"""
    from cspn_monodepth_amd.network import conv_bn
    name, C, (H, W) = ENCODER_STAGES[s]
    if "net" not in _encoder_model:
        torch.manual_seed(41)
        net = unet_ours.resnet50(prop_time=24).to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(41)
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0, 0.1, generator=gen)
                    m.running_var.uniform_(0.5, 1.5, generator=gen)
                    m.weight.normal_(1.0, 0.2, generator=gen)
                    m.bias.normal_(0, 0.1, generator=gen)
        _encoder_model["net"] = net
    net = _encoder_model["net"]
    gen = torch.Generator(device=dev).manual_seed(43 + s)
    x32 = torch.rand((BATCH, C, H, W), generator=gen, device=dev) if s == 0 else torch.randn((BATCH, C, H, W), generator=gen, device=dev).relu_()
    r.update(stage=name, x=[BATCH, C, H, W])
    for dtype, key, tol in ((torch.float32, "float32", 1e-3), (torch.float16, "float16", 1e-1 if s == 0 else 2e-2)):      # features: ~160 roundings deep
        x = x32.to(dtype)
        if s == 0:
            stock_m = net if dtype == torch.float32 else copy.deepcopy(net).half()
            fused_m = copy.deepcopy(stock_m)
            conv_bn.select_fused_encoder(fused_m, conv_bn.ENCODER_STAGES)
            macs = moved = packed = 0
            for t in range(1, 6):
                _, c, (h, w) = ENCODER_STAGES[t]
                m, v, p = encoder_convs(getattr(net, ENCODER_STAGES[t][0]), c, h, w) if t < 5 else (9 * c * c * h * w, 2 * c * h * w, 9 * c * c)
                macs, moved, packed = macs + m, moved + v, packed + p

            def fused(m=fused_m, x=x):
                with torch.no_grad():
                    return list(m.features(x)[:2])

            def stock(m=stock_m, x=x):
                with torch.no_grad():
                    return list(m.features(x)[:2])
            launches = sum(len(list(getattr(net, ENCODER_STAGES[t][0]))) for t in range(1, 5))      # blocks; the calls are counted per stage
        elif s == 5:
            conv, bn = (net.conv2, net.bn2) if dtype == torch.float32 else (copy.deepcopy(net.conv2).half(), copy.deepcopy(net.bn2).half())
            pack = conv_bn.pack_conv_bn(conv.weight, bn, 1, dtype)
            macs, moved, packed, launches = 9 * C * C * H * W, 2 * C * H * W, 9 * C * C, 1

            def fused(pack=pack, x=x):
                with torch.no_grad():
                    return [conv_bn.conv_bn_act(x, pack, relu=False)]

            def stock(conv=conv, bn=bn, x=x):
                with torch.no_grad():
                    return [bn(conv(x))]
        else:
            stock_m = getattr(net, name) if dtype == torch.float32 else copy.deepcopy(getattr(net, name)).half()
            fused_m = copy.deepcopy(stock_m)
            for b in fused_m:
                b.fused_encoder = b.fused_encoder_half = True
            macs, moved, packed = encoder_convs(stock_m, C, H, W)
            launches = sum(3 + (b.downsample is not None) for b in stock_m)

            def fused(m=fused_m, x=x):
                with torch.no_grad():
                    return [m(x)]

            def stock(m=stock_m, x=x):
                with torch.no_grad():
                    return [m(x)]

        got, want = fused(), stock()
        assert all(g.dtype == w.dtype == dtype and g.shape == w.shape for g, w in zip(got, want))
        agree = max(off(g, w) for g, w in zip(got, want))
        assert agree <= tol, (name, key, agree)
        note("%s %s: fused against stock, largest difference over largest element: %.2e" % (name, key, agree))
        del got, want
        esize = 4 if dtype == torch.float32 else 2
        nbytes = (BATCH * moved + packed) * esize
        r[key] = dict(multiply_adds=BATCH * macs, bytes=nbytes, fused_vs_stock_max_diff_over_max=agree, launches_fused=launches)
        yield r[key], "%s %s" % (name, key), dict(fused=fused, stock=stock), 2 * BATCH * macs, nbytes, key


def encoder_line(results):
    whats = ("fused_warm_us", "fused_cold_us", "stock_warm_us", "stock_cold_us", "matrix_floor_us")
    stages = dict((n, r) for n, r in results.items() if n != "features")
    line = dict(sums=dict((key, dict((what, round(sum(r[key][what] for r in stages.values()), 2)) for what in whats)) for key in MATRIX_PEAK_FLOPS),
                fused_ahead=dict((key, [n for n, r in stages.items() if r[key]["fused_ahead"]]) for key in MATRIX_PEAK_FLOPS),
                matrix_peak_flops_per_s=MATRIX_PEAK_FLOPS)
    if "features" in results:                                    # the encoder's share of everything below the CSPN module, stock ops
        line["encoder_share_of_features"] = dict(
            (key, dict((mode, round(line["sums"][key]["stock_%s_us" % mode] / results["features"][key]["stock_%s_us" % mode], 3)) for mode in ("warm", "cold")))
            for key in MATRIX_PEAK_FLOPS)
    return line


# cases, the family's keys of the line, whether a case records which floor binds
FAMILIES = {"upconv": (upconv_cases, head_line("fused", "float32"), False), "uphalf": (uphalf_cases, head_line("half", "float16"), True),
            "uptail": (uptail_cases, uptail_line, True), "upsplit": (upsplit_cases, head_line("split", "bfloat16"), True),
            "encoder": (encoder_cases, encoder_line, True)}


def main():
    global torch, unet_ours, up
    ap = argparse.ArgumentParser()
    ap.add_argument("family", choices=sorted(FAMILIES))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stages", default=None, help="default: 1,2,3,4; encoder: 0,1,2,3,4,5 (0: the whole of features)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20 or a.iters % ROUNDS:
        ap.error("--iters must be at least 20 and a multiple of %d" % ROUNDS)
    names = dict((s, row[0]) for s, row in (ENCODER_STAGES if a.family == "encoder" else STAGES).items())
    stages = [int(s) for s in a.stages.split(",")] if a.stages else sorted(names)
    tool = a.family + "_bench"
    cases, line, floor_bound = FAMILIES[a.family]
    from cspn_monodepth_amd.network import conv_tuning
    conv_db = conv_tuning.use_tuned_conv_db()
    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.network import unet_ours, up_pooling as up
    if not torch.cuda.is_available():
        sys.exit("%s: needs a ROCm GPU (a CPU run says nothing about the time)" % tool)
    dev = torch.device("cuda", 0)

    def note(msg):
        print("%s: %s" % (tool, msg), file=sys.stderr, flush=True)

    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)
    results = {}
    for s in stages:
        r = results[names[s]] = {}
        for d, label, variants, flops, nbytes, key in cases(s, r, dev, note):
            times = replay_times(variants, a.iters, a.warmup, flush)
            matrix_floor_us, hbm_floor_us = flops / PEAK_FLOPS[key] * 1e6, nbytes / HBM_PEAK * 1e6
            d.update(matrix_floor_us=round(matrix_floor_us, 2), hbm_floor_us=round(hbm_floor_us, 2))
            if floor_bound:
                d["floor_bound"] = "matrix" if matrix_floor_us > hbm_floor_us else "hbm"
            summarise(d, times, matrix_floor_us, hbm_floor_us)
            kernel = next(iter(variants))
            note("%s: %s (warm / cold), ahead: %s" % (label, ", ".join("%s %.0f / %.0f us" % (v, d[v + "_warm_us"], d[v + "_cold_us"])
                                                                         for v in variants), d[kernel + "_ahead"]))
            del variants, times
            torch.cuda.empty_cache()

    out = dict(tool=tool, batch=BATCH, warmup=a.warmup, stages=results, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               code_digest=_lib.code_digest(), conv_db=bool(conv_db or os.environ.get("MIOPEN_USER_DB_PATH")), hbm_peak_bytes_per_s=HBM_PEAK,
               method="graph replays, HIP events around each, variants alternating in %d rounds, median and 10th / 90th percentile; cold: "
                      "512 MB overwritten before every replay, outside the events" % ROUNDS, **line(results))
    text = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

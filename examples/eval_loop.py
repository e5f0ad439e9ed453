#!/usr/bin/env python3
"""The reference's evaluation protocol at any batch size: N synthetic NYU-sized RGB-D frames through the model its
`get_model` returns (cspn_monodepth_amd/network/unet_ours.py), scored PER FRAME on the device
(evaluation.FrameAverageMeter: Result.evaluate on every frame + AverageMeter over frames, libs/metrics.py:49-127), with no
host synchronisation per batch and one `average()` at the end.

    python examples/eval_loop.py --batch 24 --frames 96                  # batched, sync-free
    python examples/eval_loop.py --batch 24 --frames 96 --graph          # one captured replay per batch, the meter inside it
    python examples/eval_loop.py --frames 96 --compare-host-meter        # the old way: batch 1, metric_sums + a .cpu() per frame
    python examples/eval_loop.py --batch 24 --frames 96 --graph --sparsifier device   # the reference's sampler inside the replay
    python examples/eval_loop.py --batch 24 --frames 96 --graph --transform device    # ... from RAW 480 x 640 frames: val_transform too
    python examples/eval_loop.py --batch 8 --frames 96 --graph --comparison sheet.png # ... and the reference's comparison sheet

Synthetic data (device RNG, one seed per frame, so a frame does not depend on the batch it is generated in; SURVEY.md §8d
value distributions): `prior` = a dense depth U(0.5, 10); input = RGB U(0, 1) + sparse samples of `prior` (500 per frame);
target = prior + N(0, sigma_i^2), sigma_i between 0.05 and 0.4 from frame to frame, clamped to >= 0.1, 3 % of its pixels invalid
(0).  The network is UNTRAINED and emits ~0, so the scored prediction is `prior + model(x)[0]` clamped to >= 0.1: predictions
stay in the NYU depth range and every metric term is finite.  --sparsifier stock (the default) keeps a pixel of `prior` with
probability 500 / (H W) with stock ops while the frames are made; --sparsifier device draws the sample inside the step (and inside
the captured replay) with the reference's own rule — dataloaders.nyu_dataloader.dense_to_sparse.UniformSampling(500): probability
500 / n_keep, n_keep counted per frame — and assembles the 4-channel input in the same launch (create_rgbd); a frame's sample
depends on (--seed, frame index) only, not on the batch size.  --transform device starts one step earlier: the frames are RAW
480 x 640 — RGB uint8, `prior` and target fp32 — and the reference's val_transform (dataloaders.nyu_dataloader.nyu_dataloader:
Resize(240 / 480), CenterCrop to --height x --width) runs inside the step and inside the captured replay, in front of the device
sampler, which it implies; target goes through the same geometry as `prior`.  The numbers say nothing about depth estimation — they exercise
the protocol, and tests/test_eval_protocol.py checks them against a per-frame fp64 evaluation of the dumped tensors.

--comparison FILE draws the sheet trainer.eval saves (libs/trainers/single_gpu_trainer.py:140-175): frame 0 of the batches 0, skip, ..,
7 * skip with skip = batches // 9 (at least 1), each as one merge_into_row_with_gt row — RGB, sparse input, target, prediction —
written by cspn_monodepth_amd.utils.ComparisonSheet straight into one device buffer, two launches per row and no host
synchronisation; the file is written after the loop, from the sheet's only copy to the host.  The printed line does not change.

Prints one JSON line: the ten averages, `count` (frames) and `seconds_per_frame` (whole loop, model included, wall clock
between two device synchronisations — a whole-model figure dominated by the stock convolutions).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cspn_monodepth_amd import evaluation as ev                           # noqa: E402
from cspn_monodepth_amd.dataloaders.nyu_dataloader.dense_to_sparse import UniformSampling, create_rgbd      # noqa: E402
from cspn_monodepth_amd.dataloaders.nyu_dataloader.nyu_dataloader import iheight, iwidth, val_transform      # noqa: E402
from cspn_monodepth_amd.graphs import GraphedForward                      # noqa: E402
from cspn_monodepth_amd.network import unet_ours                          # noqa: E402


def make_frames(n, H, W, seed, dev, sparsifier="stock", raw=False):
    """-> x [n,4,H,W], prior [n,1,H,W], target [n,1,H,W] on the device; sparsifier "device": x is the RGB planes alone [n,3,H,W],
    and the step samples `prior` itself; raw: those RGB planes as uint8 (H x W is then the raw frame)."""
    gen = torch.Generator(device=dev)
    xs, priors, targets = [], [], []
    for i in range(n):
        gen.manual_seed(seed * 1000003 + i)
        rnd = lambda *s: torch.rand(*s, generator=gen, device=dev)        # noqa: E731
        prior = rnd(1, H, W) * 9.5 + 0.5
        if sparsifier == "stock":
            sparse = prior * (rnd(1, H, W) < 500.0 / (H * W))
        sigma = 0.05 + 0.35 * ((i * 7) % 16) / 15.0
        target = (prior + sigma * torch.randn(1, H, W, generator=gen, device=dev)).clamp_(min=0.1)
        target = target * (rnd(1, H, W) >= 0.03)
        if raw:
            xs.append(torch.randint(0, 256, (3, H, W), generator=gen, device=dev, dtype=torch.uint8))
        else:
            xs.append(torch.cat([rnd(3, H, W), sparse], 0) if sparsifier == "stock" else rnd(3, H, W))
        priors.append(prior)
        targets.append(target)
    return torch.stack(xs), torch.stack(priors), torch.stack(targets)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--model", choices=("resnet50", "resnet18"), default="resnet50")
    ap.add_argument("--height", type=int, default=228)
    ap.add_argument("--width", type=int, default=304)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dump", metavar="DIR", help="write pred.npy / target.npy ([frames,H,W] float32) there")
    ap.add_argument("--graph", action="store_true", help="capture forward + meter update once per batch shape and replay it")
    ap.add_argument("--compare-host-meter", action="store_true",
                    help="batch 1 with metric_sums + BatchAverageMeter (a host synchronisation per frame) instead of the device meter")
    ap.add_argument("--sparsifier", choices=("stock", "device"), default="stock",
                    help="stock: sparse samples made with the frames by stock ops, probability 500 / (H W); device: the reference's "
                         "UniformSampling(500) + create_rgbd on the device inside every step (include/cspn_sparsify.h)")
    ap.add_argument("--transform", choices=("none", "device"), default="none",
                    help="none: the frames are made at --height x --width; device: raw 480 x 640 uint8 + depth frames, the reference's "
                         "val_transform on the device inside every step (include/cspn_transform.h); implies --sparsifier device")
    ap.add_argument("--comparison", metavar="FILE",
                    help="save the reference's comparison sheet there: 8 rows of RGB | sparse input | target | prediction, drawn on the device "
                         "(include/cspn_visual.h) without a host synchronisation")
    a = ap.parse_args()
    if a.compare_host_meter:
        a.batch, a.graph = 1, False
    raw = a.transform == "device"
    if raw:
        a.sparsifier = "device"
    dev = torch.device("cuda", 0)
    torch.manual_seed(a.seed)
    net = getattr(unet_ours, a.model)(decoder_sizes=unet_ours.decoder_sizes_for(a.height, a.width)).to(dev).eval()
    x, prior, target = make_frames(a.frames, *((iheight, iwidth) if raw else (a.height, a.width)), a.seed, dev, a.sparsifier, raw)
    uar = UniformSampling(500)
    # --sparsifier device: one more input per batch, the frame indices (the Philox frame ids), copied into the replay like the rest
    ids = (torch.arange(a.frames, dtype=torch.int64, device=dev),) if a.sparsifier == "device" else ()
    meter = ev.FrameAverageMeter(dev)
    host_meter = ev.BatchAverageMeter()
    sheet, drawn = None, {}
    if a.comparison:
        from cspn_monodepth_amd.utils import ComparisonSheet
        sheet = ComparisonSheet(8, "rgbd")
        skip = max(-(-a.frames // a.batch) // 9, 1)

    def predict(xb, pb):
        return (pb + net(xb)[0]).clamp_(min=0.1)                           # the plain forward: device-guarded, safe to score unsynchronised

    def prepare(xb, pb, tb, *ib):
        if raw:
            tb = val_transform(xb, tb, output_size=(a.height, a.width))[1]
            xb, pb = val_transform(xb, pb, output_size=(a.height, a.width))
        if ib:
            xb = create_rgbd(uar, xb, pb, frame_ids=ib[0], seed=a.seed)[0]
        return xb, pb, tb

    def step(xb, pb, tb, *ib):
        xb, pb, tb = prepare(xb, pb, tb, *ib)
        pred = predict(xb, pb)
        meter.update(pred, tb)
        drawn["eager"] = (xb, tb)                                          # what the network saw: under capture, the replay's own tensors
        return pred

    nb = min(a.batch, a.frames)
    with torch.no_grad():
        step(x[:nb], prior[:nb], target[:nb], *(i[:nb] for i in ids))      # warm-up: kernel selection of the convolutions, meter buffers
        graphed = GraphedForward(step, x[:nb], prior[:nb], target[:nb], *(i[:nb] for i in ids)) if a.graph else None
        drawn["graph"] = drawn["eager"]                                    # the captured step's tensors: every replay refills them
        meter.reset()
        preds = []
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for lo in range(0, a.frames, a.batch):
            hi = min(lo + a.batch, a.frames)
            xb, pb, tb, ib = x[lo:hi], prior[lo:hi], target[lo:hi], tuple(i[lo:hi] for i in ids)
            if a.compare_host_meter:
                xb, pb, tb = prepare(xb, pb, tb, *ib)
                pred = predict(xb, pb)
                host_meter.update(ev.metric_sums(pred, tb), n=1)
            elif graphed is not None and hi - lo == nb:
                pred = graphed(xb, pb, tb, *ib)
            else:                                                          # eager (and the ragged last batch of a --graph run)
                pred = step(xb, pb, tb, *ib)
            if sheet is not None and not sheet.full and (lo // a.batch) % skip == 0:
                if a.compare_host_meter:
                    xin, tin = xb, tb
                else:
                    xin, tin = drawn["graph" if graphed is not None and hi - lo == nb else "eager"]
                sheet.add(xin[0], tin[0], pred[0])
            if a.dump:
                preds.append(pred.clone())
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
    if sheet is not None:
        sheet.save(a.comparison)
    res = host_meter.average() if a.compare_host_meter else meter.average()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        np.save(os.path.join(a.dump, "pred.npy"), torch.cat(preds)[:, 0].cpu().numpy())
        dumped = val_transform(x, target, output_size=(a.height, a.width))[1] if raw else target
        np.save(os.path.join(a.dump, "target.npy"), dumped[:, 0].cpu().numpy())
    if a.sparsifier == "device":
        res.update(sparsifier="device")
    if raw:
        res.update(transform="device")
    res.update(model=a.model, batch=a.batch, graph=bool(a.graph), meter="host" if a.compare_host_meter else "device",
               count=int(res["count"]), seconds_per_frame=dt / a.frames)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

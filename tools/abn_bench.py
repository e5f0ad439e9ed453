#!/usr/bin/env python3
"""Time of In-Place ABN (cspn_monodepth_amd/network/inplace_abn.py, include/cspn_abn.h) on the batch-norm layer shapes of
unet_ours.resnet50 at B = 3 (228 x 304 input), for the three activations, against stock batch norm + activation on the same GPU
in the same process.

    python tools/abn_bench.py [--batch 3] [--replays 20] [--rounds 5] [--out profiles/abn_bench.json]

What is timed, per layer shape and activation (all fp32, training mode, affine):
  abn_forward / abn_step      the native forward in place on a resident buffer; forward + backward (cspn_abn_forward,
                              cspn_abn_backward: dx, dweight, dbias) — the launches the autograd function makes, without autograd
  stock_forward / stock_step  F.batch_norm + F.leaky_relu / F.elu / nothing; forward + torch.autograd.grad for x, weight, bias
Method: each of the four is captured ONCE in a graph and replayed back to back `replays` times between two HIP events; the forms
alternate over `rounds` rounds and the median round is reported, per replay.  Replays are device time: no host launch gaps, for
either side (an eager step of a 2048 x 8 x 10 layer is all launch gap).  A buffer of 512 MB is overwritten between rounds so that
no round starts with its tensor in the 256 MB last-level cache; within a round the replays follow each other, so the SMALL layers (a
few MB) are cache-resident for both sides — which is also how they meet a training step, straight after the convolution that
wrote them.
Beside each time: the share of the 8 TB/s HBM peak that the compulsory traffic would amount to in that time — 3 passes of the
tensor for the forward (read, read, write), 5 more for the backward (read z and dz twice, write dx).  In the SMALL regime our
forward moves 2 passes and the backward 3; the share is still quoted against 3 and 5, the reference's traffic.
Also: torch.cuda.max_memory_allocated of forward + backward through conv3x3 -> norm -> leaky_relu -> square -> sum at 64
channels, 114 x 152, both ways.  The shapes are collected by forward hooks from one forward of the model.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8e12
EPS, SLOPE, MOMENTUM = 1e-5, 0.01, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.network import inplace_abn as A
    from cspn_monodepth_amd.network import unet_ours
    if not torch.cuda.is_available():
        sys.exit("abn_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)

    def note(msg):
        print("abn_bench: " + msg, file=sys.stderr, flush=True)

    # ---- the layer shapes, from the model itself
    shapes = {}
    model = unet_ours.resnet50().to(dev).eval()
    hooks = [m.register_forward_hook(lambda _m, inp, _o: shapes.__setitem__(tuple(inp[0].shape), shapes.get(tuple(inp[0].shape), 0) + 1))
             for m in model.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        model.features(torch.rand(a.batch, 4, 228, 304, device=dev))
    for h in hooks:
        h.remove()
    n_layers = sum(shapes.values())
    del model
    torch.cuda.empty_cache()
    note("%d batch-norm layers, %d shapes" % (n_layers, len(shapes)))
    flush = torch.empty(128 << 20, dtype=torch.float32, device=dev)

    def stock_act(y, act):
        return F.leaky_relu(y, SLOPE) if act == "leaky_relu" else (F.elu(y) if act == "elu" else y)

    def graph_of(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = fn()
        return g, keep

    layers = []
    for shape, count in sorted(shapes.items(), key=lambda kv: -kv[0][1] * 10 ** 6 - kv[0][2]):
        n, c, s = shape[0], shape[1], shape[2] * shape[3]
        plan = A.abn_plan(n, c, s)
        gen = torch.Generator(device=dev).manual_seed(c + s)
        x0 = torch.randn(shape, generator=gen, device=dev)
        cot = torch.randn(shape, generator=gen, device=dev)
        weight = torch.rand(c, generator=gen, device=dev) + 0.5
        bias = torch.rand(c, generator=gen, device=dev) - 0.5
        for act in ("none", "leaky_relu", "elu"):
            xbuf, dx = x0.clone(), torch.empty_like(x0)
            rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
            mean, var, dw, db = (torch.empty(c, device=dev) for _ in range(4))
            leaf = x0.clone().requires_grad_(True)
            w_s, b_s = weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
            rm_s, rv_s = torch.zeros(c, device=dev), torch.ones(c, device=dev)

            def abn_forward():
                A._native_forward(xbuf, weight, bias, rm, rv, mean, var, True, _lib.ABN_FULL, MOMENTUM, EPS, act, SLOPE)

            def abn_step():
                abn_forward()
                A._native_backward(xbuf, cot, var, weight, bias, None, None, dx, dw, db, True, EPS, act, SLOPE)

            def stock_forward():
                with torch.no_grad():
                    return stock_act(F.batch_norm(leaf, rm_s, rv_s, w_s, b_s, True, MOMENTUM, EPS), act)

            def stock_step():
                y = stock_act(F.batch_norm(leaf, rm_s, rv_s, w_s, b_s, True, MOMENTUM, EPS), act)
                return torch.autograd.grad(y, (leaf, w_s, b_s), cot)

            # right numbers first: one step of each from the same input, both against the same formula in fp64 on the device
            # (scale |w| + eps).  Only our side is asserted; the stock side's distance is reported (`stock_dx_err`).
            # leaky_relu's slope jumps at 0: the few pre-activations within rounding of 0 may fall on either side in two correct
            # implementations, so dx is judged by the share of elements further than 1e-4 of the largest away, not by the worst one
            xbuf.copy_(x0)
            abn_step()
            got32 = stock_step()
            leaf64 = x0.double().requires_grad_(True)
            out64 = stock_act(F.batch_norm(leaf64, None, None, weight.double() + EPS, bias.double(), True, MOMENTUM, EPS), act)
            (dx64,) = torch.autograd.grad(out64, leaf64, cot.double())
            out64 = out64.detach()

            def far(got):
                return float(((got.double() - dx64).abs() > 1e-4 * dx64.abs().max()).double().mean())
            out_err = float((xbuf.double() - out64).abs().max() / out64.abs().max())
            checks = dict(abn_out_err=out_err, abn_dx_far_share=far(dx), stock_dx_far_share=far(got32[0]))
            assert out_err <= 1e-5 and checks["abn_dx_far_share"] <= 1e-5, (shape, act, checks)
            del leaf64, out64, dx64, got32
            forms = {"abn_forward": abn_forward, "abn_step": abn_step, "stock_forward": stock_forward, "stock_step": stock_step}
            graphs = {k: graph_of(f) for k, f in forms.items()}
            times = {k: [] for k in forms}
            for _ in range(a.rounds):
                for k, (g, _keep) in graphs.items():
                    flush.zero_()
                    g.replay()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.replays):
                        g.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / a.replays)
            nbytes = 4 * n * c * s
            row = dict(shape=list(shape), layers=count, activation=act, regime=plan["regime"],
                       workgroups=(c + plan["channels_per_workgroup"] - 1) // plan["channels_per_workgroup"] * plan["workgroups_per_channel"],
                       tensor_bytes=nbytes, **checks)
            for k, ts in times.items():
                med = statistics.median(ts)
                row[k + "_us"] = round(med, 2)
                row[k + "_hbm_peak_fraction"] = round((3 if k.endswith("forward") else 8) * nbytes / (med * 1e-6) / HBM_PEAK, 4)
            row["stock_over_abn_forward"] = round(row["stock_forward_us"] / row["abn_forward_us"], 2)
            row["stock_over_abn_step"] = round(row["stock_step_us"] / row["abn_step_us"], 2)
            layers.append(row)
            del graphs
        note("%s x%d done" % (shape, count))

    # ---- peak memory of conv -> norm -> act, forward + backward
    def peak(norm_act):
        torch.manual_seed(0)
        net = nn.Sequential(nn.Conv2d(64, 64, 3, padding=1, bias=False), *norm_act).to(dev)
        xin = torch.randn(a.batch, 64, 114, 152, device=dev)
        for _ in range(2):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            net(xin).square().sum().backward()      # a dense cotangent, as a following layer hands back (sum() alone hands an expanded scalar)
            torch.cuda.synchronize()
            got = torch.cuda.max_memory_allocated() - base
            net.zero_grad(set_to_none=True)
        return int(got)
    mem = dict(shape=[a.batch, 64, 114, 152], activation_bytes=4 * a.batch * 64 * 114 * 152,
               stock_peak_bytes=peak([nn.BatchNorm2d(64), nn.LeakyReLU(SLOPE)]),
               abn_peak_bytes=peak([A.InPlaceABN(64, activation="leaky_relu", slope=SLOPE)]))

    totals = {}
    for act in ("none", "leaky_relu", "elu"):
        rows = [r for r in layers if r["activation"] == act]
        t = {k: round(sum(r[k + "_us"] * r["layers"] for r in rows), 1) for k in ("abn_forward", "abn_step", "stock_forward", "stock_step")}
        t["stock_over_abn_step"] = round(t["stock_step"] / t["abn_step"], 2)
        t["slower_than_stock"] = [r["shape"] for r in rows if r["abn_step_us"] > r["stock_step_us"]]
        t["stock_dx_off"] = [r["shape"] for r in rows if r["stock_dx_far_share"] > 1e-3]       # stock gradients that are not the formula's
        totals[act] = t
    out = dict(tool="abn_bench", batch=a.batch, dtype="float32", bn_layers=n_layers, replays=a.replays, rounds=a.rounds, layers=layers,
               all_layers_us=totals, conv_norm_act_memory=mem, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               code_digest=_lib.code_digest(),
               method="graph replays back to back between two HIP events, forms alternating, median round, per replay; device time")
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

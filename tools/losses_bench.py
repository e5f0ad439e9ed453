#!/usr/bin/env python3
"""Forward + backward time of berHuLoss and the unmasked criteria (L1, GradLoss, RMSE, RMSE_log) at 24 x 1 x 228 x 304 (fp32),
three formulations per loss on the same GPU in the same process:

  ours        cspn_monodepth_amd.criterion (include/cspn_losses.h), captured in a graph and replayed       -> device time
  stock       a capturable restatement in stock ops (`where`, `amax`, no boolean indexing), captured too   -> device time
  reference   the formula as libs/criterion/criteria.py spells it, eager: berHu's two boolean selections and its `cat` call
              nonzero, a device-to-host copy each, so this leg cannot be captured                          -> step time, host included

    python tools/losses_bench.py [--losses berhu,l1,grad,rmse,rmse_log] [--rounds 5] [--replays 20] [--out profiles/losses_bench.json]

Method: the tool first checks that the three formulations agree (loss and gradient to 1e-5).  A replay leg is `--replays`
replays back to back between two HIP events, the legs alternating over `--rounds` rounds of 10 such windows each, the median per
replay — device time with the replay's own launch floor on both sides.  The reference leg is HIP events around each eager step.  Beside each time: the share of the 8 TB/s HBM peak that the bytes the loss must move would
amount to in that time — 2 planes read forward, 2 read and 1 written backward (33.3 MB); berHu's dependent pass re-reads 2 planes
(46.6 MB).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (24, 1, 228, 304)
HBM_PEAK = 8e12
WINDOWS = 10
ALL = ("berhu", "l1", "grad", "rmse", "rmse_log")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--losses", default=",".join(ALL))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--eager-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = [n for n in a.losses.split(",") if n]
    if not names or any(n not in ALL for n in names):
        ap.error("--losses: a comma-separated subset of " + ",".join(ALL))
    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd import criterion as crit
    if not torch.cuda.is_available():
        sys.exit("losses_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    mag = torch.rand(SHAPE, generator=gen, device=dev) * 9.5 + 0.5
    noise = torch.randn(SHAPE, generator=gen, device=dev).clamp_(-3.4, 3.4)
    u = torch.rand(SHAPE, generator=gen, device=dev)
    # berHu: ~30 % zeros and ~5 % small negatives in the target; pred = |target| + N(0, 1): c ~ 0.7, about half the valid pixels in the set
    target = torch.where(u < 0.30, torch.zeros_like(mag), torch.where(u < 0.35, -0.01 * mag, mag))
    pred = (target.abs() + noise).clamp_(min=0.05)
    # l1 / grad: a pixel within 1e-3 of a tie is moved away, so that the sign of 10 r - 10 f does not hang on a last bit
    pred = torch.where(((pred - target).abs() < 1e-3) & (pred != target), target + 0.01, pred).requires_grad_(True)
    real_log = target.abs() + 0.5                                             # rmse_log: every element positive

    def second(name):
        return real_log if name == "rmse_log" else target

    def ours(name):
        if name == "berhu":
            return crit.berhu_loss(pred, target)
        return crit.unmasked_loss(pred, second(name), name)

    def x_of(name, f, r):
        if name == "rmse_log":
            return torch.log(r) - torch.log(f)
        return r - f if name == "grad" else 10.0 * r - 10.0 * f

    def stock(name):
        if name == "berhu":
            c = (0.2 * (pred - target).amax()).detach()
            valid = target > 0
            d = (target - pred).abs()
            huber = valid & (d > c)
            zero = torch.zeros_like(d)
            return (torch.where(valid, d, zero).sum() + torch.where(huber, d * d, zero).sum()) / (valid.sum() + huber.sum())
        x = x_of(name, pred, second(name))
        return x.abs().mean() if name in ("l1", "grad") else torch.sqrt((x * x).mean())

    def reference(name):
        if name == "berhu":
            c = 0.2 * torch.max(pred - target)
            d = (target - pred)[(target > 0).detach()].abs()
            return torch.cat((d, d[(d > c).detach()] ** 2)).mean()
        x = x_of(name, pred, second(name)).abs()
        return torch.mean(x) if name in ("l1", "grad") else torch.sqrt(torch.mean(x ** 2))

    forms = {"ours": ours, "stock": stock, "reference": reference}

    def step(fn, name):
        loss = fn(name)
        (grad,) = torch.autograd.grad(loss, pred)
        return loss.detach(), grad

    def note(msg):
        print("losses_bench: " + msg, file=sys.stderr, flush=True)

    n = pred.numel()
    out = dict(tool="losses_bench", shape=list(SHAPE), dtype="float32", rounds=a.rounds, replays_per_window=a.replays, windows_per_round=WINDOWS,
               eager_iters=a.eager_iters, device=torch.cuda.get_device_name(0), torch=torch.__version__, code_digest=_lib.code_digest(),
               hbm_peak_bytes_per_s=HBM_PEAK, valid_fraction=float((target > 0).float().mean()),
               method="ours / stock: graph replays, %d back to back between two HIP events, legs alternating, median per replay (device "
                      "time, the replay's launch floor included); reference: HIP events around each eager step (host included)" % a.replays,
               losses={})
    for name in names:
        got = dict((k, step(fn, name)) for k, fn in forms.items())
        loss0, grad0 = got["ours"]
        for k in ("stock", "reference"):
            loss, grad = got[k]
            assert float((loss - loss0).abs()) <= 1e-5 * float(loss0.abs()), (name, k, float(loss), float(loss0))
            assert float((grad - grad0).abs().max()) <= 1e-5 * float(grad0.abs().max()), (name, k)
        res = dict(loss=float(loss0), compulsory_bytes=(7 if name == "berhu" else 5) * 4 * n)
        if name == "berhu":
            with torch.no_grad():
                c = 0.2 * (pred - target).amax()
                nh = int(((target > 0) & ((target - pred).abs() > c)).sum())
            res.update(c=float(c), huber_fraction_of_valid=nh / int((target > 0).sum()))
        note("%s: the three formulations agree, loss %.6f" % (name, float(loss0)))
        replays, keep = {}, []
        for k in ("ours", "stock"):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step(forms[k], name)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep.append(step(forms[k], name))
            replays[k] = graph
        times = {"ours": [], "stock": [], "reference": []}
        for graph in replays.values():
            for _ in range(a.replays):
                graph.replay()
        for _ in range(20):
            step(reference, name)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, graph in replays.items():
                for _ in range(WINDOWS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.replays):
                        graph.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / a.replays)
            evs = []
            for _ in range(a.eager_iters // a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(reference, name)
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            times["reference"] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]
        for k, ts in times.items():
            med = statistics.median(ts)
            res[k + "_us"] = round(med, 2)
            res[k + "_us_min"] = round(min(ts), 2)
            res[k + "_us_max"] = round(max(ts), 2)
            res[k + "_hbm_peak_fraction"] = round(res["compulsory_bytes"] / (med * 1e-6) / HBM_PEAK, 4)
        res["stock_over_ours"] = round(res["stock_us"] / res["ours_us"], 2)
        res["reference_over_ours"] = round(res["reference_us"] / res["ours_us"], 2)
        note("%s: ours %.1f us, stock %.1f us, reference (eager) %.1f us" % (name, res["ours_us"], res["stock_us"], res["reference_us"]))
        out["losses"][name] = res
        del replays, keep
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

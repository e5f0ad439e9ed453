#!/usr/bin/env python3
"""Forward + backward time of the masked training loss at 24 x 1 x 228 x 304 (fp32), three formulations on the same GPU in the
same process:

  criterion   cspn_monodepth_amd.criterion (three launches of include/cspn_criterion.h)
  stock       ((target - pred).abs() * valid).sum() / valid.sum() — what bench.py --workload train spells out (the yardstick)
  reference   (target - pred)[target > 0].abs().mean() — libs/criterion/criteria.py: boolean indexing, a host sync per step

    python tools/criterion_bench.py [--kind l1|l2|l1_log] [--iters 240] [--warmup 30] [--graph] [--out profiles/criterion_bench.json]

Method: HIP events around every single forward + backward, the formulations alternating in rounds of iters / 4, the median over
all of a formulation's iterations.  These are eager steps: the figures contain the host's launch gaps (a dozen stock kernels
are launched one by one, the criterion's three likewise), so they are step times, not kernel times.  --graph adds replays
of the captured criterion and stock steps, which are device time (the reference formulation cannot be captured).
Beside each time: the share of the 8 TB/s HBM peak that the 5 x 4 bytes per pixel the criterion has to move (two reads
forward, two reads and a write backward) would amount to in that time.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (24, 1, 228, 304)
HBM_PEAK = 8e12
ROUNDS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="l1", choices=("l1", "l2", "l1_log"))
    ap.add_argument("--iters", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--graph", action="store_true", help="also time replays of the captured criterion and stock steps (device time)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters must be at least 200")
    import torch
    from cspn_monodepth_amd import _lib
    from cspn_monodepth_amd.criterion import masked_loss
    if not torch.cuda.is_available():
        sys.exit("criterion_bench: needs a ROCm GPU (a CPU run says nothing about the time)")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(SHAPE, generator=gen, device=dev) * 9.5 + 0.5
    pred = (target + torch.randn(SHAPE, generator=gen, device=dev)).clamp_(min=0.05)
    # l1_log: where pred is within 1e-3 of target the sign of log t - log p depends on the last bit of each logarithm, and two
    # correct implementations may differ there; such pixels are moved away (as in golden G18) so that the agreement check holds
    pred = torch.where((pred / target - 1).abs() < 1e-3, target * 1.002, pred).requires_grad_(True)
    u = torch.rand(SHAPE, generator=gen, device=dev)
    target = torch.where(u < 0.30, torch.zeros_like(target), torch.where(u < 0.35, -target, target))

    def term(t, p, select):
        if a.kind == "l1_log":
            # the stock form cannot multiply a NaN of an invalid pixel away: select before the logarithm
            d = torch.log(torch.where(t > 0, t, torch.ones_like(t)) if select else t) - torch.log(p)
        else:
            d = t - p
        return d * d if a.kind == "l2" else d.abs()

    def criterion():
        return masked_loss(pred, target, a.kind)

    def stock():
        valid = target > 0
        return (term(target, pred, True) * valid).sum() / valid.sum()

    def reference():
        valid = target > 0
        return term(target[valid], pred[valid], False).mean()

    forms = {"criterion": criterion, "stock": stock, "reference": reference}

    def step(fn):
        """One forward + backward; the gradient is returned, not accumulated into pred.grad."""
        loss = fn()
        (grad,) = torch.autograd.grad(loss, pred)
        return loss.detach(), grad

    def same_numbers():
        got = dict((name, step(fn)) for name, fn in forms.items())
        loss0, grad0 = got["criterion"]
        for name in ("stock", "reference"):
            loss, grad = got[name]
            assert float((loss - loss0).abs()) <= 1e-5 * float(loss0.abs()), (name, float(loss), float(loss0))
            assert float((grad - grad0).abs().max()) <= 1e-5 * float(grad0.abs().max()), name
        return float(loss0)

    def note(msg):
        print("criterion_bench: " + msg, file=sys.stderr, flush=True)

    loss_value = same_numbers()
    note("the three formulations agree, loss %.6f" % loss_value)
    times = {}

    def measure(runners):
        for name, fn in runners.items():
            times.setdefault(name, [])
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for name, fn in runners.items():
                evs = []
                for _ in range(a.iters // ROUNDS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                times[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]

    measure(dict((k, (lambda f=f: step(f))) for k, f in forms.items()))
    note("eager steps timed")

    if a.graph:
        replays, keep = {}, []
        for name in ("criterion", "stock"):                    # static pred / target, the gradient allocated inside the capture
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    step(forms[name])
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                keep.append(step(forms[name]))
            replays[name + "_graph"] = graph.replay
            note("captured the %s step" % name)
        measure(replays)
        note("replays timed")

    n = pred.numel()
    nbytes = 5 * 4 * n
    out = dict(tool="criterion_bench", kind=a.kind, shape=list(SHAPE), dtype="float32", iters=len(times["criterion"]), warmup=a.warmup,
               compulsory_bytes=nbytes, valid_fraction=float((target > 0).float().mean()), loss=loss_value,
               device=torch.cuda.get_device_name(0), torch=torch.__version__, code_digest=_lib.code_digest(),
               method="HIP events around each forward + backward, formulations alternating in %d rounds, median; eager steps, host "
                      "launch gaps included" % ROUNDS)
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name + "_us"] = round(med, 2)
        out[name + "_us_min"] = round(min(ts), 2)
        out[name + "_hbm_peak_fraction"] = round(nbytes / (med * 1e-6) / HBM_PEAK, 4)
    out["stock_over_criterion"] = round(out["stock_us"] / out["criterion_us"], 2)
    if a.graph:
        out["stock_graph_over_criterion_graph"] = round(out["stock_graph_us"] / out["criterion_graph_us"], 2)
    out["reference_over_criterion"] = round(out["reference_us"] / out["criterion_us"], 2)
    line = json.dumps(out, sort_keys=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

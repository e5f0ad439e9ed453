"""Golden G24: the per-iteration learning rates of the reference's schedules (libs/scheduler/__init__.py, scheduler.py).

Imports the reference (CSPN_REFERENCE, default: `reference` next to this repository) — nothing of it is copied — and drives its `get_schedular`,
`do_schedule`, `PolynomialLR` and `WarmUpLR` through the cases of tests/optim_cases.py:g24_run on a plain torch.optim.SGD with two
groups (rates 0.01 and 0.003):

  poly_40_1, poly_40_10, poly_25_4    poly_lr (gamma 0.9) with (max_iter, decay_iter), run 7 iterations past max_iter
  warmup_linear, warmup_constant      WarmUpLR(warmup_iters 5, gamma 0.2) over PolynomialLR(40, 1), 12 iterations
  reduce_lr                           reduce_lr (factor 0.2, patience 2) through do_schedule with len 5 and a metric per epoch that
                                      plateaus twice (optim_cases.PLATEAU_METRICS)

Only data is recorded: tests/golden/g24_schedules.json holds, per case, the rate of every group after construction and after
every iteration as a hex double.  cspn_monodepth_amd.scheduler must reproduce every one exactly (tests/test_optim.py).

    python tests/golden/make_golden_g24.py
"""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("CSPN_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import torch                               # noqa: E402
import optim_cases as oc                   # noqa: E402
import libs.scheduler as ref               # noqa: E402  (reference)


def main():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")    # the epoch argument of ReduceLROnPlateau.step is deprecated; the reference passes it
        cases = oc.g24_run(ref)
    # self-checks: the golden shows each branch it is there for
    p = [[float.fromhex(v) for v in row] for row in cases["poly_40_10"]]
    assert p[9] == p[0] and p[10] != p[9] and p[11] == p[10], "decay_iter 10: the rate is kept between multiples of ten"
    p = [[float.fromhex(v) for v in row] for row in cases["poly_25_4"]]
    assert p[-1] == p[-2] == p[25] and p[25][0] > 0, "past max_iter the rate is kept"
    w = [[float.fromhex(v) for v in row] for row in cases["warmup_linear"]]
    assert w[0][0] == 0.2 * oc.G24_BASE_RATES[0] and w[-1] == list(oc.G24_BASE_RATES), "after warm-up: the wrapped scheduler's rates"
    r = [float.fromhex(row[0]) for row in cases["reduce_lr"]]
    assert len(set(r)) == 3, "the metric plateaus twice: three distinct rates"
    out = dict(torch=torch.__version__, base_rates=list(oc.G24_BASE_RATES), plateau_metrics=list(oc.PLATEAU_METRICS),
               plateau_len=oc.PLATEAU_LEN, cases=cases)
    path = os.path.join(ROOT, "tests", "golden", "g24_schedules.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", path, {k: len(v) for k, v in cases.items()})


if __name__ == "__main__":
    main()

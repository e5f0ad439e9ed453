"""The SGD step (cspn_monodepth_amd/optim.py, include/cspn_optim.h) and the learning-rate schedules (cspn_monodepth_amd/
scheduler.py).

  * CPU: the header / library / loader contract; the numpy restatement of the arithmetic (tests/optim_cases.py) against torch's
    single-tensor SGD itself, bit for bit; cspn_sgd_plan; the schedules against golden G24 (the reference's libs.scheduler,
    tests/golden/make_golden_g24.py), double for double; every refusal that needs no device; pickle and state_dict round trips.
  * GPU: the yardstick is torch.optim.SGD(foreach=False, fused=False) on the CPU, run here on copies of the same tensors.  The
    comparison rule (optim_cases.same): bit for bit on every finite value, +-Inf and +-0, NaN position for position."""
import copy
import ctypes
import io
import json
import os
import pickle
import re
import warnings

import numpy as np
import pytest
import torch

import optim_cases as oc
from conftest import ROOT
from cspn_monodepth_amd import _lib
from cspn_monodepth_amd import optim, scheduler

DEV = "cuda:0"
CHUNK, PER_LAUNCH = oc.CHUNK, oc.TENSORS_PER_LAUNCH
COMBO_IDS = [oc.combo_id(c) for c in oc.COMBOS]


def torch_sgd(params, **kw):
    return torch.optim.SGD(params, foreach=False, fused=False, **kw)


def plan(sizes, max_workgroups=0):
    arr = (ctypes.c_size_t * max(len(sizes), 1))(*sizes)
    launches, chunks = ctypes.c_int(-1), ctypes.c_size_t(0)
    ok = _lib.lib().cspn_sgd_plan(arr, len(sizes), max_workgroups, ctypes.byref(launches), ctypes.byref(chunks))
    return ok, launches.value, chunks.value


# ------------------------------------------------------------------------------------------------ CPU: contract
def test_header_declares_the_exports_and_the_library_has_them():
    src = open(os.path.join(ROOT, "include", "cspn_optim.h")).read()
    assert int(re.search(r"^#define CSPN_SGD_CHUNK (\d+)\b", src, flags=re.M).group(1)) == CHUNK == _lib.SGD_CHUNK
    assert int(re.search(r"^#define CSPN_SGD_TENSORS_PER_LAUNCH (\d+)\b", src, flags=re.M).group(1)) == PER_LAUNCH == _lib.SGD_TENSORS_PER_LAUNCH
    assert int(re.search(r"^#define CSPN_SGD_MAX_WORKGROUPS (\d+)\b", src, flags=re.M).group(1)) == _lib.SGD_MAX_WORKGROUPS == 2048
    # descriptors (3 pointers + a count), the chunk prefix, a first-step byte each and 32 bytes of hyper-parameters: within 4 KB,
    # and one more tensor would not be
    assert 32 + PER_LAUNCH * 32 + (PER_LAUNCH + 1) * 4 + PER_LAUNCH <= 4096 < 32 + (PER_LAUNCH + 1) * 32 + (PER_LAUNCH + 2) * 4 + PER_LAUNCH + 1
    assert ctypes.sizeof(_lib.cspn_sgd_tensor) == 40 and ctypes.sizeof(_lib.cspn_sgd_hyper) == 48


def test_package_exports_the_modules():
    import cspn_monodepth_amd as pkg
    assert pkg.optim is optim and pkg.scheduler is scheduler and "optim" in pkg.__all__ and "scheduler" in pkg.__all__


# ------------------------------------------------------------------------------------------------ CPU: the arithmetic
@pytest.mark.parametrize("combo", oc.COMBOS, ids=COMBO_IDS)
def test_restatement_is_torchs_single_tensor_sgd(combo):
    lr = 0.01
    for n in oc.CPU_SIZES:
        p0 = oc.values(n, n)
        p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
        opt = torch_sgd([p], lr=lr, **combo)
        rp, rb = p0.copy(), None
        for step in range(3):
            g = oc.values(1000 * step + n + 7, n)
            p.grad = torch.from_numpy(g.copy())
            opt.step()
            rp, rb = oc.sgd_restated(rp, g, rb, step == 0, lr, **combo)
            assert np.array_equal(oc.bits(p.detach().numpy()), oc.bits(rp)), (n, step)
            if combo["momentum"] != 0:
                assert np.array_equal(oc.bits(opt.state[p]["momentum_buffer"].numpy()), oc.bits(rb)), (n, step)
            else:
                assert "momentum_buffer" not in opt.state[p] or opt.state[p]["momentum_buffer"] is None


def test_restatement_keeps_torchs_signed_zeros():
    p0 = np.array([-0.0, 0.0, 1.0], np.float32)
    g = np.full(3, -0.0, np.float32)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch_sgd([p], lr=0.1, momentum=0.9)
    p.grad = torch.from_numpy(g.copy())
    opt.step()
    rp, rb = oc.sgd_restated(p0, g, None, True, 0.1, momentum=0.9)
    for got_p, got_b in ((p.detach().numpy(), opt.state[p]["momentum_buffer"].numpy()), (rp, rb)):
        assert oc.bits(got_p).tolist() == [0, 0, 0x3f800000]
        assert oc.bits(got_b).tolist() == [0x80000000] * 3


def test_fma32_rounds_once():
    # 4097 * 16773121 = 2^36 + 1: the product is 2^-24 + 2^-60, so 1 + product lies just ABOVE a tie of fp32 — which fp64 cannot see
    a, b = np.array([4097 * 2.0 ** -30], np.float32), np.array([16773121 * 2.0 ** -30], np.float32)
    one = np.ones(1, np.float32)
    assert float(a[0]) * float(b[0]) == 2.0 ** -24 + 2.0 ** -60
    assert np.float32(float(a[0]) * float(b[0]) + 1.0) == np.float32(1.0)                 # two roundings: to the tie, then to even
    assert oc.fma32(a, b, one)[0] == np.float32(1.0 + 2.0 ** -23)                         # one rounding: up
    assert oc.fma32(-a, b, -one)[0] == -np.float32(1.0 + 2.0 ** -23)
    assert oc.fma32(a, b, -one)[0] == -np.float32(1.0 - 2.0 ** -24) and oc.fma32(one, one, one)[0] == 2.0


# ------------------------------------------------------------------------------------------------ CPU: the plan
def test_plan_counts_launches_and_chunks():
    assert plan([]) == (1, 0, 0)
    assert plan([0, 0]) == (1, 0, 0)
    assert plan([CHUNK - 1, CHUNK, CHUNK + 1]) == (1, 1, 4)
    assert plan([0, 5, 0, 2 * CHUNK + 5, 0]) == (1, 1, 4)
    assert plan([3] * PER_LAUNCH) == (1, 1, PER_LAUNCH)
    assert plan([3] * (PER_LAUNCH + 1)) == (1, 2, PER_LAUNCH + 1)
    assert plan([0] * 40 + [3] * PER_LAUNCH + [0] * 40) == (1, 1, PER_LAUNCH)              # zero-element tensors take no slot
    assert plan([3] * (2 * PER_LAUNCH + 1), max_workgroups=1) == (1, 3, 2 * PER_LAUNCH + 1)
    assert plan([1 << 33]) == (1, 1, (1 << 33) // CHUNK)
    assert plan([3] * 5, max_workgroups=1 << 30) == (1, 1, 5)                               # above 65535: taken as 65535
    ok, _, _ = plan([3], max_workgroups=-1)
    assert ok == 0 and b"max_workgroups" in _lib.lib().cspn_last_error()
    ok = _lib.lib().cspn_sgd_plan(None, 0, 0, None, None)                                   # the outputs are optional
    assert ok == 1


# ------------------------------------------------------------------------------------------------ CPU: golden G24
def test_schedules_reproduce_the_reference_double_for_double():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "g24_schedules.json")))
    assert tuple(want["base_rates"]) == oc.G24_BASE_RATES and tuple(want["plateau_metrics"]) == oc.PLATEAU_METRICS
    assert want["plateau_len"] == oc.PLATEAU_LEN
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = oc.g24_run(scheduler)
    assert sorted(got) == sorted(want["cases"]) == sorted(["poly_%d_%d" % c for c in oc.POLY_CASES] + ["warmup_linear", "warmup_constant", "reduce_lr"])
    for name in got:
        assert got[name] == want["cases"][name], name


def test_schedules_on_this_optimiser_with_float_rates():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "g24_schedules.json")))["cases"]["poly_25_4"]
    p = torch.nn.Parameter(torch.zeros(2))
    opt = optim.SGD([dict(params=[p], lr=oc.G24_BASE_RATES[0])], momentum=0.9)
    s = scheduler.PolynomialLR(opt, max_iter=25, decay_iter=4)
    rows = [opt.param_groups[0]["lr"].hex()]
    for _ in range(len(want) - 1):
        s.step()
        rows.append(opt.param_groups[0]["lr"].hex())
    assert rows == [w[0] for w in want]
    assert s.get_last_lr() == [float.fromhex(rows[-1])]


def test_warmup_mode_is_checked_at_construction():
    opt = torch_sgd([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    with pytest.raises(ValueError, match="cosine"):
        scheduler.WarmUpLR(opt, scheduler.PolynomialLR(opt, max_iter=4), mode="cosine")
    assert opt.param_groups[0]["lr"] == 0.1                                  # refused before a rate was written


def test_scheduler_names_that_are_not_offered():
    import types
    args = types.SimpleNamespace(scheduler="cosine")
    with pytest.raises(NotImplementedError):
        scheduler.get_schedular(torch_sgd([torch.nn.Parameter(torch.zeros(1))], lr=0.1), args)
    with pytest.raises(NotImplementedError):
        scheduler.do_schedule(args, None)
    with pytest.raises(RuntimeError):
        scheduler.do_schedule(types.SimpleNamespace(scheduler="reduce_lr"), None, it=3)


# ------------------------------------------------------------------------------------------------ CPU: refusals
def cpu_param(n=4, dtype=torch.float32, grad=True):
    p = torch.nn.Parameter(torch.zeros(n, dtype=dtype))
    if grad:
        p.grad = torch.ones(n, dtype=dtype)
    return p


def test_argument_validation_is_torchs():
    p = cpu_param()
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(momentum=0.0, nesterov=True),
               dict(momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            torch_sgd([p], **dict(dict(lr=0.1), **kw))
        with pytest.raises(ValueError):
            optim.SGD([p], **dict(dict(lr=0.1), **kw))
    with pytest.raises(ValueError):
        optim.SGD([])                                                      # torch: an empty parameter list
    opt = optim.SGD([dict(params=[cpu_param()], lr=0.5, weight_decay=0.1), dict(params=[cpu_param()])], lr=0.2, momentum=0.9)
    assert [g["lr"] for g in opt.param_groups] == [0.5, 0.2] and [g["weight_decay"] for g in opt.param_groups] == [0.1, 0]
    assert opt.defaults == dict(lr=0.2, momentum=0.9, dampening=0, weight_decay=0, nesterov=False, maximize=False)


def test_refusals_without_a_device():
    with pytest.raises(RuntimeError, match="ROCm device"):
        optim.SGD([cpu_param()], lr=0.1).step()                            # CPU parameters: no fallback
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="fp32 only"):
            optim.SGD([cpu_param(dtype=dtype)], lr=0.1).step()
    p = cpu_param()
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (4,))
    with pytest.raises(RuntimeError, match="sparse"):
        optim.SGD([p], lr=0.1).step()
    base = torch.zeros(4, 6)
    p = torch.nn.Parameter(base.t())                                       # a transposed view
    p.grad = torch.ones(6, 4)
    assert not p.is_contiguous()
    with pytest.raises(RuntimeError, match="not contiguous"):
        optim.SGD([p], lr=0.1).step()
    q = torch.nn.Parameter(torch.zeros(4, device="meta"))
    q.grad = torch.zeros(4, device="meta")
    with pytest.raises(RuntimeError, match="more than one device"):
        optim.SGD([cpu_param(), q], lr=0.1).step()
    with pytest.raises(RuntimeError, match="more than one device"):
        optim.SGD([dict(params=[cpu_param()]), dict(params=[q])], lr=0.1).step()
    for bad in (torch.zeros(1), torch.zeros((), dtype=torch.float64), torch.zeros(2)):
        with pytest.raises(ValueError, match="0-dim fp32"):
            optim.SGD([cpu_param()], lr=bad)
        opt = optim.SGD([cpu_param()], lr=0.1)
        opt.param_groups[0]["lr"] = bad
        with pytest.raises(ValueError, match="0-dim fp32"):
            opt.step()
    with pytest.raises(ValueError, match="0-dim fp32 tensor on cpu"):
        optim.SGD([cpu_param()], lr=torch.zeros((), device="meta")).step()  # a rate on another device than the parameters
    assert optim.SGD([cpu_param(grad=False)], lr=0.1).step() is None       # nothing has a gradient: nothing to refuse
    assert optim.SGD([cpu_param(grad=False)], lr=0.1).step(lambda: 3.5) == 3.5
    with pytest.raises(ValueError):
        optim.sgd_step([cpu_param()], [], [], lr=0.1)


# ------------------------------------------------------------------------------------------------ CPU: pickle, state_dict
def test_pickle_and_state_dict_round_trips():
    ps = [cpu_param(5), cpu_param(3)]
    theirs = torch_sgd([dict(params=[ps[0]], lr=0.05), dict(params=[ps[1]], weight_decay=1e-4)], lr=0.1, momentum=0.9)
    theirs.step()
    theirs.step()
    sd = theirs.state_dict()
    qs = [cpu_param(5), cpu_param(3)]
    mine = optim.SGD([dict(params=[qs[0]]), dict(params=[qs[1]])], lr=7.0)
    mine.load_state_dict(copy.deepcopy(sd))
    assert [g["lr"] for g in mine.param_groups] == [0.05, 0.1] and [g["weight_decay"] for g in mine.param_groups] == [0, 1e-4]
    assert [g["momentum"] for g in mine.param_groups] == [0.9, 0.9]
    for q, p in zip(qs, ps):
        assert torch.equal(mine.state[q]["momentum_buffer"], theirs.state[p]["momentum_buffer"])
    back = mine.state_dict()
    assert back["state"].keys() == sd["state"].keys() and all(list(back["state"][k]) == ["momentum_buffer"] for k in back["state"])
    assert [g["params"] for g in back["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    again = torch_sgd([dict(params=[ps[0]]), dict(params=[ps[1]])], lr=3.0)
    again.load_state_dict(back)                                            # ... and into torch's again
    again.step()
    assert again.param_groups[1]["weight_decay"] == 1e-4 and again.param_groups[0]["lr"] == 0.05
    # the reference's checkpoint stores the optimiser object itself
    clone = pickle.loads(pickle.dumps(mine))
    assert type(clone) is optim.SGD and clone.defaults == mine.defaults
    assert [{k: v for k, v in g.items() if k != "params"} for g in clone.param_groups] == \
        [{k: v for k, v in g.items() if k != "params"} for g in mine.param_groups]
    for cg, mg in zip(clone.param_groups, mine.param_groups):
        for cp, mp in zip(cg["params"], mg["params"]):
            assert torch.equal(cp, mp) and torch.equal(clone.state[cp]["momentum_buffer"], mine.state[mp]["momentum_buffer"])
    s = scheduler.PolynomialLR(mine, max_iter=10)                          # a scheduler patches step(): the object still pickles
    s.step()
    assert pickle.loads(pickle.dumps(mine)).param_groups[0]["lr"] == mine.param_groups[0]["lr"]
    fresh = optim.SGD([cpu_param()], lr=0.1, momentum=0.9)
    assert fresh.state_dict()["state"] == {} and set(fresh.__getstate__()) == {"defaults", "state", "param_groups"}


# ------------------------------------------------------------------------------------------------ GPU
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().contiguous().numpy().copy()                    # a copy: a CPU tensor's own memory goes on changing


# (name, number of elements or a 2-d shape, kind)
MIXED = [("n1", 1, "plain"), ("n3", 3, "plain"), ("n4", 4, "plain"), ("n5", 5, "plain"), ("n1023", 1023, "plain"), ("chunk", CHUNK, "plain"),
         ("chunk_p1", CHUNK + 1, "plain"), ("two_chunks_p5", 2 * CHUNK + 5, "plain"), ("empty", 0, "plain"), ("no_grad", 37, "no_grad"),
         ("misaligned_param", CHUNK + 7, "misaligned_param"), ("misaligned_grad", 1030, "misaligned_grad"),
         ("strided_grad", (33, 35), "strided_grad")]


LATE = 3                      # the step at which the "no_grad" parameter receives its first gradient


def numel(shape):
    return int(np.prod(shape))


def device_param(values, kind):
    if kind == "misaligned_param":
        flat = torch.zeros(values.size + 8, device=DEV)
        p = torch.nn.Parameter(flat[1:1 + values.size])
        with torch.no_grad():
            p.copy_(dev(values))
        assert p.data_ptr() % 16 == 4
        return p
    return torch.nn.Parameter(dev(values))


def device_grad(values, kind):
    if kind == "misaligned_grad":
        flat = torch.zeros(values.size + 8, device=DEV)
        flat[1:1 + values.size] = dev(values)
        g = flat[1:1 + values.size]
        assert g.data_ptr() % 16 == 4 and g.is_contiguous()
        return g
    if kind == "strided_grad":
        g = dev(values.T.copy()).t()
        assert not g.is_contiguous() and g.shape == values.shape
        return g
    return dev(values)


class Twin(object):
    """One list of tensors twice: on the device, and as the yardstick's CPU copies."""

    def __init__(self, entries, seed=0):
        self.entries = entries
        self.start = [oc.values(seed + 31 * i, numel(shape)).reshape(shape) for i, (_, shape, _) in enumerate(entries)]
        self.device = [device_param(v, kind) for v, (_, _, kind) in zip(self.start, entries)]
        self.cpu = [torch.nn.Parameter(torch.from_numpy(v.copy())) for v in self.start]

    def grads(self, step, seed=0):
        """A "no_grad" parameter gets its first gradient at step LATE."""
        return [None if kind == "no_grad" and step < LATE else oc.values(seed + 977 * (step + 1) + 13 * i, numel(shape)).reshape(shape)
                for i, (_, shape, kind) in enumerate(self.entries)]

    def set_grads(self, step, seed=0):
        for p, c, g, (_, _, kind) in zip(self.device, self.cpu, self.grads(step, seed), self.entries):
            p.grad = None if g is None else device_grad(g, kind)
            c.grad = None if g is None else torch.from_numpy(g.copy())

    def assert_same(self, mine, theirs, what=""):
        torch.cuda.synchronize()
        for (name, _, _), p, c in zip(self.entries, self.device, self.cpu):
            assert oc.same(host(p), host(c)), "%s %s: %d parameter elements differ" % (what, name, oc.n_differing(host(p), host(c)))
            mb = mine.state[p].get("momentum_buffer") if p in mine.state else None
            tb = theirs.state[c].get("momentum_buffer") if c in theirs.state else None
            assert (mb is None) == (tb is None), "%s %s: momentum buffer present %s / %s" % (what, name, mb is not None, tb is not None)
            if mb is not None:
                assert oc.same(host(mb), host(tb)), "%s %s: %d buffer elements differ" % (what, name, oc.n_differing(host(mb), host(tb)))


@pytest.mark.gpu
@pytest.mark.parametrize("combo", oc.COMBOS, ids=COMBO_IDS)
def test_every_combination_matches_the_yardstick(combo):
    twin = Twin(MIXED)
    mine, theirs = optim.SGD(twin.device, lr=0.01, **combo), torch_sgd(twin.cpu, lr=0.01, **combo)
    for step in range(3):
        twin.set_grads(step)
        mine.step()
        theirs.step()
        twin.assert_same(mine, theirs, "step %d" % step)
    assert twin.device[9].grad is None and oc.same(host(twin.device[9]), twin.start[9])     # no gradient: untouched
    # one more step in which that parameter receives its first gradient: ONE launch whose descriptors mix a first step (buf = g,
    # the buffer not read) with tensors that have their buffers
    assert MIXED[9][2] == "no_grad" and len(MIXED) <= PER_LAUNCH
    twin.set_grads(LATE)
    mine.step()
    theirs.step()
    twin.assert_same(mine, theirs, "step %d" % LATE)
    assert not oc.same(host(twin.device[9]), twin.start[9])
    if combo["momentum"] != 0:
        first_buffer = oc.sgd_restated(twin.start[9], twin.grads(LATE)[9], None, True, 0.01, **combo)[1]
        assert oc.same(host(mine.state[twin.device[9]]["momentum_buffer"]), first_buffer)


@pytest.mark.gpu
def test_launch_split():
    entries = [("t%d" % i, 1 + i % 7, "plain") for i in range(PER_LAUNCH + 3)]
    assert plan([numel(s) for _, s, _ in entries])[1] == 2
    twin = Twin(entries, seed=5)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
    mine, theirs = optim.SGD(twin.device, **kw), torch_sgd(twin.cpu, **kw)
    for step in range(2):
        twin.set_grads(step)
        mine.step()
        theirs.step()
        twin.assert_same(mine, theirs, "step %d" % step)


@pytest.mark.gpu
def test_two_groups():
    twin = Twin(MIXED[:8], seed=9)

    def groups(ps):
        return [dict(params=ps[:3], lr=0.02, weight_decay=1e-4), dict(params=ps[3:], lr=0.003, weight_decay=0.0, nesterov=True)]
    mine, theirs = optim.SGD(groups(twin.device), lr=1.0, momentum=0.9), torch_sgd(groups(twin.cpu), lr=1.0, momentum=0.9)
    for step in range(3):
        twin.set_grads(step)
        mine.step()
        theirs.step()
        twin.assert_same(mine, theirs, "step %d" % step)


@pytest.mark.gpu
def test_stride_loop_and_search_give_the_same_bits():
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    entries = [e for e in MIXED if e[2] != "no_grad"]
    results = []
    for cap in (1, 3, 0):
        twin = Twin(entries, seed=3)
        buffers = [None] * len(entries)
        for step in range(2):
            gs = [device_grad(g, kind) for g, (_, _, kind) in zip(twin.grads(step), entries)]
            with torch.no_grad():
                optim.sgd_step(twin.device, gs, buffers, max_workgroups=cap, **kw)
        torch.cuda.synchronize()
        results.append(([host(p) for p in twin.device], [host(b) for b in buffers]))
    theirs = torch_sgd(twin.cpu, **kw)
    for step in range(2):
        for c, g in zip(twin.cpu, twin.grads(step)):
            c.grad = torch.from_numpy(g.copy())
        theirs.step()
    for ps, bs in results:
        for (name, _, _), p, b, c in zip(entries, ps, bs, twin.cpu):
            assert oc.same(p, host(c)), name
            assert oc.same(b, host(theirs.state[c]["momentum_buffer"])), name
            assert np.array_equal(oc.bits(p), oc.bits(results[0][0][[e[0] for e in entries].index(name)])), name


def hostile_run(vals, kw, steps=2):
    """p, g and buf over vals^3, the buffer preloaded on both sides -> (mine, theirs) after `steps` steps: [(p, buf)] per step."""
    p0, g0, b0 = oc.cross3(vals)
    p, c = torch.nn.Parameter(dev(p0)), torch.nn.Parameter(torch.from_numpy(p0.copy()))
    mine, theirs = optim.SGD([p], **kw), torch_sgd([c], **kw)
    mine.state[p]["momentum_buffer"] = dev(b0)
    theirs.state[c]["momentum_buffer"] = torch.from_numpy(b0.copy())
    out = []
    for step in range(steps):
        g = np.roll(g0, step)
        p.grad, c.grad = dev(g), torch.from_numpy(g.copy())
        mine.step()
        theirs.step()
        torch.cuda.synchronize()
        out.append(((host(p), host(mine.state[p]["momentum_buffer"])), (host(c), host(theirs.state[c]["momentum_buffer"]))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_hostile_values(nesterov):
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=nesterov)
    for step, ((mp, mb), (tp, tb)) in enumerate(hostile_run(oc.SPECIALS, kw)):
        assert oc.same(mp, tp), "step %d: %d parameter elements differ" % (step, oc.n_differing(mp, tp))
        assert oc.same(mb, tb), "step %d: %d buffer elements differ" % (step, oc.n_differing(mb, tb))
        assert np.isinf(tp).any() and np.isnan(tp).any() and (step > 0 or (oc.bits(tp) == 0x80000000).any())


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(lr=0.5, momentum=0.9, weight_decay=1e-4), dict(lr=0.25, momentum=0.5, dampening=0.3),
                                dict(lr=0.5, momentum=0.9, nesterov=True, maximize=True)], ids=["decay", "dampening", "nesterov_max"])
def test_denormals_are_kept(kw):
    """fp32 denormals in p, g and buf, and results that land among them: the device neither flushes its inputs nor its results."""
    for step, ((mp, mb), (tp, tb)) in enumerate(hostile_run(oc.DENORMALS, kw)):
        tiny = (np.abs(tp) > 0) & (np.abs(tp) < 1.1754943508222875e-38)
        assert tiny.sum() > 100
        assert oc.same(mp, tp), "step %d: %d parameter elements differ" % (step, oc.n_differing(mp, tp))
        assert oc.same(mb, tb), "step %d: %d buffer elements differ" % (step, oc.n_differing(mb, tb))


@pytest.mark.gpu
def test_float_rate_and_tensor_rate_give_the_same_bits():
    kw = dict(momentum=0.9, weight_decay=1e-4)
    a, b = Twin(MIXED[:8], seed=2), Twin(MIXED[:8], seed=2)
    by_value = optim.SGD(a.device, lr=0.1, **kw)
    by_pointer = optim.SGD(b.device, lr=torch.tensor(0.1, dtype=torch.float32, device=DEV), **kw)
    converted = Twin(MIXED[:8], seed=2)
    conv = optim.SGD(converted.device, lr=0.1, **kw).lr_to_device()
    assert conv.param_groups[0]["lr"].shape == () and conv.param_groups[0]["lr"].dtype == torch.float32
    assert conv.param_groups[0]["lr"].device == converted.device[0].device and conv.param_groups[0]["lr_host"] == 0.1
    theirs = torch_sgd(a.cpu, lr=0.1, **kw)
    for step in range(2):
        for t in (a, b, converted):
            t.set_grads(step)
        for o in (by_value, by_pointer, conv, theirs):
            o.step()
    a.assert_same(by_value, theirs)
    for other in (b, converted):
        for p, q in zip(a.device, other.device):
            assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    with pytest.raises(ValueError, match="0-dim fp32"):
        optim.SGD(a.device, lr=torch.tensor(0.1)).step()                  # a rate on the CPU for parameters on the device


CAPTURE = [("n5", 5, "plain"), ("chunk_p1", CHUNK + 1, "plain"), ("n1023", 1023, "plain")]


@pytest.mark.gpu
def test_captured_step_follows_the_schedule():
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    graphed, eager = Twin(CAPTURE, seed=4), Twin(CAPTURE, seed=4)
    opt_g, opt_e, opt_c = optim.SGD(graphed.device, **kw).lr_to_device(), optim.SGD(eager.device, **kw), torch_sgd(graphed.cpu, **kw)
    scheds = [scheduler.PolynomialLR(o, max_iter=12, decay_iter=2) for o in (opt_g, opt_e, opt_c)]
    assert isinstance(opt_g.param_groups[0]["lr"], torch.Tensor) and isinstance(opt_e.param_groups[0]["lr"], float)
    static = [torch.zeros_like(p) for p in graphed.device]
    for p, s in zip(graphed.device, static):
        p.grad = s

    def load(step):
        gs = graphed.grads(step)
        for s, p, c, g in zip(static, eager.device, graphed.cpu, gs):
            s.copy_(dev(g))
            p.grad = dev(g)
            c.grad = torch.from_numpy(g.copy())

    load(0)                                                                # one eager step creates the buffers
    for o in (opt_g, opt_e, opt_c):
        o.step()
    for s in scheds:
        s.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    fresh = [[dev(g) for g in graphed.grads(k + 1)] for k in range(6)]
    snaps = []
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                # nothing below may read a device value back
    try:
        for k in range(6):
            for s, g in zip(static, fresh[k]):
                s.copy_(g)
            graph.replay()
            snaps.append(([p.detach().clone() for p in graphed.device], [opt_g.state[p]["momentum_buffer"].clone() for p in graphed.device]))
            scheds[0].step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    rates = []
    for k in range(6):
        load(k + 1)
        opt_e.step()
        opt_c.step()
        rates.append(opt_e.param_groups[0]["lr"])
        torch.cuda.synchronize()
        for i, (name, _, _) in enumerate(CAPTURE):
            ps, bs = snaps[k]
            assert torch.equal(ps[i].view(torch.int32), eager.device[i].view(torch.int32)), (k, name)
            assert torch.equal(bs[i].view(torch.int32), opt_e.state[eager.device[i]]["momentum_buffer"].view(torch.int32)), (k, name)
            assert oc.same(host(ps[i]), host(graphed.cpu[i])), (k, name)
            assert oc.same(host(bs[i]), host(opt_c.state[graphed.cpu[i]]["momentum_buffer"])), (k, name)
        scheds[1].step()
        scheds[2].step()
    assert len(set(rates)) == 4                                            # decay_iter 2: the six replays ran at four rates
    assert float(opt_g.param_groups[0]["lr"]) == float(np.float32(opt_e.param_groups[0]["lr"])) == float(np.float32(opt_g.param_groups[0]["lr_host"]))


@pytest.mark.gpu
def test_capture_with_a_missing_buffer_raises():
    twin = Twin(CAPTURE, seed=6)
    opt = optim.SGD(twin.device, lr=0.01, momentum=0.9).lr_to_device()
    twin.set_grads(0)
    before = [p.detach().clone() for p in twin.device]
    scratch = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="momentum buffers are missing"):
            opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(b, p) for b, p in zip(before, twin.device))
    assert all("momentum_buffer" not in st for st in opt.state.values())
    plain = optim.SGD(twin.device, lr=0.01)                                # without momentum there is no buffer to miss
    second = torch.cuda.CUDAGraph()
    with torch.cuda.graph(second):
        plain.step()


@pytest.mark.gpu
def test_step_and_schedule_do_not_synchronise():
    twin = Twin(MIXED, seed=8)
    opt = optim.SGD(twin.device, lr=0.01, momentum=0.9, weight_decay=1e-4).lr_to_device()
    sched = scheduler.PolynomialLR(opt, max_iter=12, decay_iter=2)
    warm = scheduler.WarmUpLR(opt, scheduler.PolynomialLR(opt, max_iter=12), warmup_iters=3)
    twin.set_grads(0)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()                                                         # creates the buffers
        opt.step()
        for _ in range(4):
            sched.step()                                                   # both branches of PolynomialLR
            warm.step()
        plateau = scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.2, patience=0)
        plateau.step(1.0)
        plateau.step(1.0)                                                  # reduces
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert float(opt.param_groups[0]["lr"]) == float(np.float32(opt.param_groups[0]["lr_host"]))
    # a rate tensor the caller made (no lr_host): its one read happens when the scheduler is constructed, none in a step
    own = optim.SGD(twin.device, lr=torch.tensor(0.5, dtype=torch.float32, device=DEV))
    plateau = scheduler.ReduceLROnPlateau(own, mode="min", factor=0.2, patience=0)
    assert own.param_groups[0]["lr_host"] == 0.5
    torch.cuda.set_sync_debug_mode("error")
    try:
        plateau.step(1.0)
        plateau.step(1.0)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert float(own.param_groups[0]["lr"]) == float(np.float32(0.5 * 0.2))


@pytest.mark.gpu
def test_state_dict_interchange_with_torch():
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    for mine_first in (False, True):
        twin = Twin(MIXED[:8], seed=11)
        ours, torchs, theirs = optim.SGD(twin.device, **kw), torch_sgd(twin.device, **kw), torch_sgd(twin.cpu, **kw)
        first, second = (ours, torchs) if mine_first else (torchs, ours)
        for step in range(4):
            twin.set_grads(step)
            if step == 2:
                second.load_state_dict(first.state_dict())
            (first if step < 2 else second).step()
            theirs.step()
        twin.assert_same(second, theirs, "mine first" if mine_first else "torch first")


@pytest.mark.gpu
def test_saved_optimiser_object_continues_on_the_same_bits():
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    twin = Twin(MIXED[:8], seed=12)
    mine, theirs = optim.SGD(twin.device, **kw), torch_sgd(twin.cpu, **kw)
    for step in range(2):
        twin.set_grads(step)
        mine.step()
        theirs.step()
    blob = io.BytesIO()
    torch.save(mine, blob)
    blob.seek(0)
    loaded = torch.load(blob, weights_only=False)
    assert type(loaded) is optim.SGD
    twin.device = [p for g in loaded.param_groups for p in g["params"]]     # the object brought its parameters along
    for step in range(2, 4):
        twin.set_grads(step)
        loaded.step()
        theirs.step()
    twin.assert_same(loaded, theirs)


@pytest.mark.gpu
def test_abi_on_caller_owned_buffers():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    GUARD = 0x5A5A5A5A
    # (elements, padded): per tensor [guard x 4 | p | guard x 4 | g | guard x 4 | buf | guard x 4] in one arena.  Padded: every
    # region is rounded up to 16 bytes, so all three bases are 16-byte aligned (the 16-byte path and its tail) and the padding is
    # guard too; the unpadded ones that follow sit off the 16-byte grid (the element path, over more than one chunk)
    layout = [(2 * CHUNK + 5, True), (1023, True), (5, False), (CHUNK, False)]
    sizes = [s for s, _ in layout]
    total = sum(3 * ((s + 3) // 4 * 4 if pad else s) + 16 for s, pad in layout)
    arena = torch.full((total,), GUARD, dtype=torch.int32, device=DEV)
    fl = arena.view(torch.float32)
    tensors = (_lib.cspn_sgd_tensor * len(sizes))()
    spans, guards, off = [], torch.ones(total, dtype=torch.bool), 0
    for i, (s, pad) in enumerate(layout):
        r = (s + 3) // 4 * 4 if pad else s
        at = [off + 4, off + 8 + r, off + 12 + 2 * r]
        for j, a in enumerate(at):
            fl[a:a + s] = dev(oc.values(100 * i + j, s))
            guards[a:a + s] = False
        tensors[i].param, tensors[i].grad, tensors[i].momentum_buffer = (fl[a:].data_ptr() for a in at)
        tensors[i].n, tensors[i].first = s, 0
        assert all(fl[a:].data_ptr() % 16 == 0 for a in at) == pad
        spans.append(at)
        off += 3 * r + 16
    before = fl.clone()
    hyper = _lib.cspn_sgd_hyper(lr=0.1, lr_device=None, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=0, maximize=0)
    assert L.cspn_sgd_step(tensors, len(sizes), ctypes.byref(hyper), _lib.CSPN_F16, 0, st) == 0
    assert b"dtype" in L.cspn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(arena, before.view(torch.int32))                    # a refused call launches nothing
    bad = _lib.cspn_sgd_hyper(lr=0.1, lr_device=None, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=1, maximize=0)
    assert L.cspn_sgd_step(tensors, len(sizes), ctypes.byref(bad), _lib.CSPN_F32, 0, st) == 0 and b"nesterov" in L.cspn_last_error()
    _lib.check(L.cspn_sgd_step(tensors, len(sizes), ctypes.byref(hyper), _lib.CSPN_F32, 2, st), "cspn_sgd_step")
    torch.cuda.synchronize()
    gmask = guards.to(DEV)
    assert bool((arena[gmask] == GUARD).all())                             # the elements around every buffer
    for (pa, ga, ba), s in zip(spans, sizes):
        assert torch.equal(fl[ga:ga + s].view(torch.int32), before[ga:ga + s].view(torch.int32))      # the gradient is only read
        want_p, want_b = oc.sgd_restated(host(before[pa:pa + s]), host(before[ga:ga + s]), host(before[ba:ba + s]), False, 0.1,
                                         momentum=0.9, weight_decay=1e-4)
        assert oc.same(host(fl[pa:pa + s]), want_p) and oc.same(host(fl[ba:ba + s]), want_b)

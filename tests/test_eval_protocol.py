"""Per-frame metric sums (cspn_metrics_per_frame) and the reference's evaluation protocol on the device (cspn_meter_update,
evaluation.FrameAverageMeter): Result.evaluate on every frame + AverageMeter over frames (libs/metrics.py:49-127), at any
batch size, without a host synchronisation per batch.

Bars (none of them derived from what the kernels give):
  * sums against the fp64 numpy oracle: rtol 1e-5, what tests/test_hip_parity.py holds cspn_metrics_accumulate to;
  * averages against the reference's recorded ones (golden G17, tests/golden/make_golden_g17.py): rtol 1e-5, what
    finalize_metrics is held to against G7 — the generator asserts the reference's own fp32 arithmetic is within 2e-6 of fp64;
  * everything the determinism contract of include/cspn_hip.h promises: exact (torch.equal on the float64 words)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cspn_monodepth_amd as pkg
from cspn_monodepth_amd import _lib
from conftest import ROOT, golden_names, load_golden
from oracle import cspn_oracle as orc

DEV = "cuda:0"
ev = pkg.evaluation
CASES = golden_names("g17_eval_protocol_")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def frames_np(B, H, W, seed, dtype=np.float32):
    """target U(0.5, 10) with 2..40 % invalid pixels (another fraction per frame), prediction = target + N(0, 0.1^2) >= 0.05."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.5, 10, (B, H, W)).astype(np.float32)
    p = np.maximum(t + rng.normal(0, 0.1, t.shape).astype(np.float32), np.float32(0.05)).astype(np.float32)
    frac = np.linspace(0.02, 0.4, B)[rng.permutation(B)].reshape(B, 1, 1)
    t[rng.random(t.shape) < frac] = 0
    return p.astype(dtype), t.astype(dtype)


# ------------------------------------------------------------------------------------------------ CPU
def test_protocol_goldens_are_present():
    assert set(CASES) >= {"g17_eval_protocol_small", "g17_eval_protocol_odd", "g17_eval_protocol_fp16", "g17_eval_protocol_empty"}
    z = load_golden("g17_eval_protocol_odd")
    assert (z["pred"].shape[-1] * z["pred"].shape[-2]) % 4 != 0
    assert load_golden("g17_eval_protocol_fp16")["pred"].dtype == np.float16
    assert np.isnan(load_golden("g17_eval_protocol_empty")["average"]).all()


def test_workspace_bytes_is_linear_in_the_batch_and_needs_no_gpu():
    fn = _lib.lib().cspn_metrics_per_frame_workspace_bytes
    for n in (1, 7, 37 * 51, 228 * 304, 352 * 1216, 4000 * 3000):
        one = fn(1, n)
        assert one >= 80 and one % 80 == 0
        for B in (2, 24, 513):
            assert fn(B, n) == B * one
    assert fn(1, 352 * 1216) // 80 > 64                      # one KITTI frame alone is spread over many workgroups
    assert fn(0, 100) == 0 and fn(3, 0) == 0
    # bad arguments come back as 0 + a message, never as a launch
    assert _lib.lib().cspn_metrics_per_frame(None, None, 0, 1, 16, None, None, None) == 0
    assert b"cspn_metrics_per_frame" in _lib.lib().cspn_last_error()
    assert _lib.lib().cspn_meter_update(None, 1, None, None) == 0


def test_cpu_tensors_raise():
    p = torch.rand(2, 1, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ev.metric_sums_per_frame(p, p)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ev.FrameAverageMeter("cuda:0").update(p, p)
    with pytest.raises(RuntimeError):
        ev.FrameAverageMeter("cpu")


def test_average_from_state_and_local_gather():
    st = torch.tensor([2.0, 4, 6, 8, 10, 12, 14, 16, 18, 20, 4, 1000], dtype=torch.float64)
    avg = ev.average_from_state(st)
    assert avg["count"] == 4 and [avg[k] for k in ev.METRIC_NAMES] == [0.5 * (i + 1) for i in range(10)]
    assert ev.average_from_state(torch.zeros(12, dtype=torch.float64))["count"] == 0
    out = ev.all_gather_frame_meter(st)                      # no process group: the local state, as a copy
    assert torch.equal(out, st) and out.data_ptr() != st.data_ptr()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rows(z):
    """[frames, 12] host rows of a golden case: the ten per-frame metrics, 1 frame, its valid pixels."""
    valid = (z["target"].astype(np.float32) > 0).reshape(z["target"].shape[0], -1).sum(1)
    return np.concatenate([z["per_frame"], np.ones((len(valid), 1)), valid[:, None].astype(np.float64)], 1)


def _gather_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cspn_monodepth_amd import evaluation as ev_
    rows = _rows(load_golden("g17_eval_protocol_small"))
    lo, hi = (0, 9) if rank == 0 else (9, rows.shape[0])     # uneven shards: 9 + 4 frames
    total = ev_.all_gather_frame_meter(torch.from_numpy(rows[lo:hi].sum(0)))
    np.save(os.path.join(outdir, "rank%d.npy" % rank), total.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_frame_meter_all_gather_over_gloo(tmp_path):
    world = 2
    mp.spawn(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    z = load_golden("g17_eval_protocol_small")
    rows = _rows(z)
    res = [np.load(tmp_path / ("rank%d.npy" % r)) for r in range(world)]
    assert np.array_equal(res[0], res[1])                    # every rank ends with the same 12 numbers
    assert np.allclose(res[0], rows.sum(0), rtol=1e-14)
    avg = ev.average_from_state(torch.from_numpy(res[0]))
    assert avg["count"] == rows.shape[0]
    for k, want in zip(ev.METRIC_NAMES, z["average"]):       # ... and the averages of the unsharded list of frames
        assert np.isclose(avg[k], want, rtol=1e-12), k


# ------------------------------------------------------------------------------------------------ GPU: sums
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,dtype", [(24, 228, 304, np.float32), (8, 352, 1216, np.float32), (5, 37, 51, np.float32),
                                         (6, 33, 35, np.float16), (24, 228, 304, np.float16), (1, 228, 304, np.float32),
                                         (1, 352, 1216, np.float32), (3, 1, 5, np.float32)])
def test_per_frame_sums_match_the_oracle(B, H, W, dtype):
    p, t = frames_np(B, H, W, seed=B * 1000 + W, dtype=dtype)
    got = ev.metric_sums_per_frame(dev(p), dev(t))
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 10)
    g = got.cpu().numpy()
    for i in range(B):
        want = orc.metric_sums(p[i].astype(np.float32), t[i].astype(np.float32))
        err = np.abs(g[i] - want) / np.maximum(np.abs(want), 1e-300)
        print("frame %d: worst rel %.3g" % (i, err.max()))
        assert np.allclose(g[i], want, rtol=1e-5), (i, g[i], want)
    whole = ev.metric_sums(dev(p), dev(t)).cpu().numpy()     # the existing batch kernel on the same tensors
    assert np.allclose(g.sum(0), whole, rtol=1e-5)
    # [B,1,H,W] is the same batch; `out` is overwritten, whatever it held
    out = torch.full((B, 10), float("nan"), dtype=torch.float64, device=DEV)
    assert ev.metric_sums_per_frame(dev(p)[:, None], dev(t)[:, None], out=out) is out and torch.equal(out, got)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,dtype", [(228, 304, torch.float32), (37, 51, torch.float32), (33, 35, torch.float16),
                                       (228, 304, torch.float16)])
def test_a_frames_sums_do_not_depend_on_where_the_frame_lies(H, W, dtype):
    B = 24
    npdt = np.float32 if dtype == torch.float32 else np.float16
    p, t = (dev(a) for a in frames_np(B, H, W, seed=H, dtype=npdt))
    ref = ev.metric_sums_per_frame(p, t)
    assert torch.equal(ref, ev.metric_sums_per_frame(p, t))                                 # twice: the same bits
    for i in (0, 1, 7, 23):                                                                 # the frame scored alone
        assert torch.equal(ev.metric_sums_per_frame(p[i:i + 1], t[i:i + 1])[0], ref[i]), i
    perm = torch.from_numpy(np.random.default_rng(1).permutation(B)).to(DEV)                # another position of another batch
    assert torch.equal(ev.metric_sums_per_frame(p[perm].contiguous(), t[perm].contiguous()), ref[perm])
    assert torch.equal(ev.metric_sums_per_frame(p[5:16], t[5:16]), ref[5:16])               # a smaller batch
    # a [B,H,W] view whose base is one element off: no frame of it is 16-byte aligned
    n = B * H * W
    pb, tb = torch.empty(n + 9, dtype=dtype, device=DEV), torch.empty(n + 9, dtype=dtype, device=DEV)
    for off in (1, 3):
        pv, tv = pb[off:off + n].view(B, H, W), tb[off:off + n].view(B, H, W)
        pv.copy_(p), tv.copy_(t)
        assert pv.data_ptr() % 16 != 0 and pv.is_contiguous()
        assert torch.equal(ev.metric_sums_per_frame(pv, tv), ref), off
    # prediction and target misaligned differently
    pv, tv = pb[0:n].view(B, H, W), tb[2:2 + n].view(B, H, W)
    pv.copy_(p), tv.copy_(t)
    assert torch.equal(ev.metric_sums_per_frame(pv, tv), ref)


# ------------------------------------------------------------------------------------------------ GPU: protocol
def _batches(n, how):
    if how == "one":
        return [(0, n)]
    if how == "single":
        return [(i, i + 1) for i in range(n)]
    cuts = [0, 5, 10, n] if n > 10 else [0, 3, 5, n]         # ragged: 5 + 5 + 3 (or 3 + 2 + 2 for the 7-frame case)
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_frame_average_meter_reproduces_the_references_protocol(case):
    z = load_golden(case)
    p, t = dev(z["pred"]), dev(z["target"])                  # the fp16 case reaches the device as fp16 tensors
    n = p.shape[0]
    states = []
    for how in ("one", "single", "ragged"):
        meter = ev.FrameAverageMeter(DEV)
        for lo, hi in _batches(n, how):
            meter.update(p[lo:hi], t[lo:hi])
        states.append(meter.state().clone())
        avg = meter.average()
        assert avg["count"] == n
        got = np.array([avg[k] for k in ev.METRIC_NAMES])
        print(case, how, "worst rel", np.nanmax(np.abs(got - z["average"]) / np.abs(z["average"])) if np.isfinite(z["average"]).any() else "nan")
        assert np.array_equal(np.isnan(got), np.isnan(z["average"]))
        assert np.allclose(got, z["average"], rtol=1e-5, equal_nan=True), (how, got, z["average"])
    assert _same_bits(states[0], states[1]) and _same_bits(states[0], states[2])
    # the per-frame figures themselves, every frame and metric (NaN where the reference has NaN)
    sums = ev.metric_sums_per_frame(p, t).cpu()
    for i in range(n):
        if float(sums[i, 9]) == 0:
            assert np.isnan(z["per_frame"][i]).all()
            continue
        fin = ev.finalize_metrics(sums[i])
        assert np.allclose([fin[k] for k in ev.METRIC_NAMES], z["per_frame"][i], rtol=1e-5), i
    # update_from_sums is the second half of update; reset() starts over
    m2 = ev.FrameAverageMeter(DEV)
    m2.update(p, t)
    m2.reset()
    m2.update_from_sums(ev.metric_sums_per_frame(p, t))
    assert _same_bits(m2.state(), states[0])
    assert float(m2.state()[11]) == float((z["target"].astype(np.float32) > 0).sum())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.gpu
def test_meter_resizes_the_prediction_like_the_reference():
    """libs/metrics.py:52-55: a prediction of another size is brought to the target's by a bilinear, align_corners resize."""
    p, t = (dev(a) for a in frames_np(3, 20, 26, seed=3))
    small = torch.nn.functional.avg_pool2d(p[:, None], 2)
    a, b = ev.FrameAverageMeter(DEV), ev.FrameAverageMeter(DEV)
    a.update(small, t[:, None])
    b.update(torch.nn.functional.interpolate(small, size=(20, 26), mode="bilinear", align_corners=True), t[:, None])
    assert _same_bits(a.state(), b.state()) and a.average()["count"] == 3


@pytest.mark.gpu
def test_meter_update_is_capturable_and_replays_accumulate():
    """Captured in a graph after one warm-up call with that batch shape: a synchronisation or an allocation inside `update`
    would make the capture raise.  k replays leave exactly the state k eager updates leave (the same additions in the same
    order), which is k times one update's contribution up to the rounding of those additions; the two counters are exact."""
    B, H, W = 6, 37, 51
    p, t = (dev(a) for a in frames_np(B, H, W, seed=5))
    meter = ev.FrameAverageMeter(DEV)
    meter.update(p, t)                                                   # warm-up: buffers for this shape
    torch.cuda.synchronize()
    meter.reset()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            meter.update(p, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert float(meter.state().abs().sum()) == 0.0                       # capturing ran nothing
    eager = ev.FrameAverageMeter(DEV)
    graph.replay()
    eager.update(p, t)
    torch.cuda.synchronize()
    one = meter.state().clone()
    assert _same_bits(one, eager.state()) and float(one[10]) == B and float(one[11]) == float((t > 0).sum())
    k = 5
    for _ in range(k - 1):
        graph.replay()
        eager.update(p, t)
    torch.cuda.synchronize()
    got = meter.state().clone()
    assert _same_bits(got, eager.state())
    assert float(got[10]) == k * B and float(got[11]) == k * float(one[11])
    assert np.allclose(got.cpu().numpy(), k * one.cpu().numpy(), rtol=1e-14, atol=0)
    assert meter.average()["count"] == k * B


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("batch,graph", [(1, False), (8, False), (1, True), (8, True)])
def test_eval_loop_example_prints_the_per_frame_averages_of_what_it_scored(tmp_path, batch, graph):
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "examples", "eval_loop.py"), "--model", "resnet18",
           "--frames", "16", "--batch", str(batch), "--dump", str(tmp_path)] + (["--graph"] if graph else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    pred, target = np.load(tmp_path / "pred.npy"), np.load(tmp_path / "target.npy")
    assert pred.shape == target.shape == (16, 228, 304) and res["count"] == 16 and res["meter"] == "device"
    per_frame = np.array([orc.evaluate_metrics(pred[i], target[i])[0] for i in range(16)])
    want = per_frame.mean(0)
    got = np.array([res[k] for k in ev.METRIC_NAMES])
    print("batch", batch, "graph", graph, "worst rel", np.max(np.abs(got - want) / np.abs(want)), "s/frame", res["seconds_per_frame"])
    assert np.isfinite(want).all() and np.allclose(got, want, rtol=1e-5), (got, want)
    assert per_frame[:, 3].std() > 0.05 * want[3]            # the frames do differ: an average over frames is not a pooled figure

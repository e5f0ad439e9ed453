"""Golden G17: the model the reference's get_model returns, and the reference's evaluation protocol.

Imports the reference (CSPN_REFERENCE, default /root/reference) — nothing of it is copied — and writes

  g17_unet_ours_state_dict_keys.json   key -> shape of network/unet_ours.py resnet50() (+ the parameter count in the manifest)
  g17_unet_ours_full.npz               the seeded, untrained resnet50().eval() on one hash-generated 228 x 304 RGB-D frame:
                                       [x, guidance] and the head output blur_depth, sub-sampled (the test regenerates the input
                                       from the hash generator and the weights from the same seed and construction order —
                                       asserted here against this package's network/unet_ours.py)
  g17_eval_protocol_<case>.npz         libs/metrics.py Result.evaluate on every frame + AverageMeter.update(n = 1): frames
                                       (pred, target), the ten per-frame metrics, the ten averages.  Frames differ in noise
                                       level and valid-pixel count, so per-frame and pixel-weighted averages differ visibly.

The tests hold the device meter to rtol 1e-5 against these numbers.  That bar means something only if the reference's own fp32
arithmetic sits well inside it: every finite per-frame metric and every average is compared with oracle.evaluate_metrics (fp64)
here and must agree to 2e-6, or no fixture is written.
"""
import json
import os
import sys
import types
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CSPN_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

_stub = types.ModuleType("torch._thnn")          # pac.py:20 imports torch._thnn (removed in torch>=1.0)
_stub.type2backend = defaultdict(lambda: None)
sys.modules.setdefault("torch._thnn", _stub)

from libs import metrics as ref_metrics                     # noqa: E402  (reference)
from oracle import cspn_oracle as orc                       # noqa: E402

torch.set_num_threads(4)
manifest = {"files": {}, "protocol": {}}
NAMES = ("irmse", "imae", "mse", "rmse", "mae", "absrel", "lg10", "delta1", "delta2", "delta3")
TEST_RTOL = 1e-5
ORACLE_BAR = TEST_RTOL / 5


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    manifest["files"][name] = {"bytes": os.path.getsize(path), "arrays": {k: list(np.shape(v)) for k, v in arrs.items()}}
    assert os.path.getsize(path) <= 580000, (name, os.path.getsize(path))


def model():
    from network import unet_ours as ref_net                                   # reference
    from cspn_monodepth_amd.network import unet_ours as our_net                # this package: same seed => same weights
    torch.manual_seed(0)
    net = ref_net.resnet50(pretrained=False).eval()
    sd = net.state_dict()
    keys = {k: list(v.shape) for k, v in sd.items()}
    with open(os.path.join(HERE, "g17_unet_ours_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
    manifest["g17_keys"] = len(keys)
    manifest["g17_params"] = int(sum(p.numel() for p in net.parameters()))
    torch.manual_seed(0)
    ours = our_net.resnet50().state_dict()
    assert list(ours) == list(sd) and all(torch.equal(ours[k], sd[k]) for k in sd), "construction order differs from the reference's"
    del ours
    cap = {}
    net.post_process_layer.register_forward_hook(lambda m, i, kw, o: cap.update(i=i, kw=kw), with_kwargs=True)
    rgb = orc.hash_uniform(170, 1, (1, 3, 228, 304), 0.0, 1.0)
    dep = orc.hash_uniform(170, 2, (1, 1, 228, 304), 0.5, 10.0)
    sp = orc.hash_sparse(170, 3, dep, 500.0 / (228 * 304))
    with torch.no_grad():
        x, guidance = net(t(np.concatenate([rgb, sp], 1)))
    blur = cap["i"][0].numpy()
    assert np.array_equal(cap["i"][1].numpy(), guidance.numpy()) and np.array_equal(cap["kw"]["sparse_depth"].numpy(), sp)
    x, guidance = x.numpy(), guidance.numpy()
    sub = 4
    save("g17_unet_ours_full", seed=np.int32(0), sub=np.int32(sub), x_sub=x[:, :, ::sub, ::sub],
         guidance_sub=guidance[:, :, ::sub, ::sub], blur_sub=blur[:, :, ::sub, ::sub],
         moments=np.array([x.astype(np.float64).sum(), (x.astype(np.float64) ** 2).sum(),
                           guidance.astype(np.float64).sum(), (guidance.astype(np.float64) ** 2).sum()]))


def frames(seed, n, H, W, empty_frame=None, half=False):
    """n frames: target U(0.5, 10) with 5..80 % invalid pixels, prediction = target + N(0, sigma^2) clamped to >= 0.1, sigma from
    0.05 to 0.4 over the frames (the NYU depth range: every metric term is finite in fp32)."""
    pred, target = [], []
    for i in range(n):
        sigma = np.float32(0.05 + 0.35 * i / max(n - 1, 1))
        frac = 0.05 + 0.75 * ((i * 5) % n) / max(n - 1, 1)                     # invalid fraction, not monotonic in sigma
        tg = orc.hash_uniform(seed, 10 * i + 1, (1, H, W), 0.5, 10.0)
        pr = np.maximum(tg + orc.hash_normal(seed, 10 * i + 2, (1, H, W)) * sigma, np.float32(0.1)).astype(np.float32)
        inval = orc.hash_u24(seed, 10 * i + 3, tg.size).reshape(tg.shape) < int(frac * 2 ** 24)
        if i == empty_frame:
            inval[:] = True
        tg = np.where(inval, np.float32(0), tg).astype(np.float32)
        if half:                # values rounded to half; the reference gets them as fp32 tensors, the device as fp16 tensors
            pr, tg = pr.astype(np.float16), tg.astype(np.float16)
        pred.append(pr)
        target.append(tg)
    return np.stack(pred), np.stack(target)                                    # [n,1,H,W]


def protocol(case, pred, target):
    meter = ref_metrics.AverageMeter()
    per_frame, want_frames = [], []
    p32, t32 = pred.astype(np.float32), target.astype(np.float32)
    for i in range(pred.shape[0]):
        r = ref_metrics.Result()
        r.evaluate(t(p32[i:i + 1]), t(t32[i:i + 1]))                           # batch size 1, as the reference's eval loader
        meter.update(r, 0.0, 0.0, 1)
        per_frame.append([getattr(r, k) for k in NAMES])
        n = int((t32[i] > 0).sum())
        want_frames.append(orc.evaluate_metrics(p32[i], t32[i])[0] if n else np.full(10, np.nan))
    avg = meter.average()
    per_frame = np.array(per_frame, np.float64)
    average = np.array([getattr(avg, k) for k in NAMES], np.float64)
    want_frames = np.array(want_frames, np.float64)
    want_avg = want_frames.mean(0)
    # the reference's fp32 arithmetic against fp64: well inside the bar the tests hold the device to
    assert np.array_equal(np.isnan(per_frame), np.isnan(want_frames)) and np.array_equal(np.isnan(average), np.isnan(want_avg))
    fin = np.isfinite(want_frames)
    worst = float(np.max(np.abs(per_frame[fin] - want_frames[fin]) / np.abs(want_frames[fin])))
    fa = np.isfinite(want_avg)
    if fa.any():
        worst = max(worst, float(np.max(np.abs(average[fa] - want_avg[fa]) / np.abs(want_avg[fa]))))
    assert worst <= ORACLE_BAR, (case, worst)
    # per-frame and pixel-weighted averages are different figures: rmse must differ by far more than the test tolerance
    valid = (t32 > 0).reshape(t32.shape[0], -1).sum(1)
    info = {"reference_vs_fp64_worst_rel": worst, "frames": int(pred.shape[0]), "valid_pixels": valid.tolist()}
    if fa.all():
        pooled = orc.evaluate_metrics(p32, t32)[0]
        gap = abs(pooled[3] - average[3]) / average[3]
        assert gap > 100 * TEST_RTOL, (case, gap)
        info["rmse_per_frame_vs_pixel_weighted_rel"] = float(gap)
    assert len(set(valid.tolist())) == len(valid)
    manifest["protocol"][case] = info
    save("g17_eval_protocol_" + case, pred=pred, target=target, per_frame=per_frame, average=average)


if __name__ == "__main__":
    model()
    protocol("small", *frames(171, 13, 40, 52))
    protocol("odd", *frames(172, 13, 37, 51))                                  # 1887 pixels per frame: not a multiple of 4
    protocol("fp16", *frames(173, 13, 40, 52, half=True))
    protocol("empty", *frames(174, 7, 40, 52, empty_frame=3))                  # a frame without a valid pixel: NaN averages
    manifest["torch"] = torch.__version__
    manifest["numpy"] = np.__version__
    with open(os.path.join(HERE, "golden_g17_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print(json.dumps(manifest, indent=1, sort_keys=True))

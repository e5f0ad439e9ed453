"""The model the reference's get_model returns (cspn_monodepth_amd/network/unet_ours.py = the topology of the reference's
network/unet_ours.py:251-335 on stock PyTorch-ROCm ops + the HIP un-pooling + the HIP K x K CSPN module).

CPU: state_dict keys / shapes / parameter count equal the reference's (golden G17, tests/golden/make_golden_g17.py).
GPU: the seeded network against the reference's CPU run on G17's frame, the CSPN stage against the C oracle at the
north-star bar, one training step, and the G14 tail chain with this module's block classes."""
import json
import os

import numpy as np
import pytest
import torch

import cspn_monodepth_amd as pkg
from conftest import GOLDEN, load_golden, rmse

DEV = "cuda:0"
KEYS = json.load(open(os.path.join(GOLDEN, "g17_unet_ours_state_dict_keys.json")))


def test_state_dict_matches_reference_keys_and_shapes():
    from cspn_monodepth_amd.network import unet_ours
    m = unet_ours.resnet50()
    sd = m.state_dict()
    assert len(KEYS) == 417 and set(sd) == set(KEYS)
    assert all(list(sd[k].shape) == KEYS[k] for k in KEYS)
    assert sum(p.numel() for p in m.parameters()) == 218123072            # golden_g17_manifest.json g17_params
    assert len(m.post_process_layer.state_dict()) == 0                     # the CSPN module is checkpoint-transparent
    assert m.post_process_layer.times == 24 and isinstance(m.post_process_layer, pkg.CSPN_ours.AffinityPropagate)
    # a checkpoint of the reference (built here from its recorded shapes) loads strictly
    ckpt = {k: torch.full(shape, 0.5, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, shape in KEYS.items()}
    res = m.load_state_dict(ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(m.gud_up_proj_layer6.conv1.weight.detach().mean()) == 0.5 and tuple(m.gud_up_proj_layer6.conv1.weight.shape) == (8, 64, 3, 3)
    # conv3 is built and never called (unet_ours.py:270): the one thing DDP must not wait for
    unused = m.unused_parameters()
    assert len(unused) == 1 and unused[0] is m.conv3.weight
    with pytest.raises(RuntimeError):
        unet_ours.resnet50(pretrained=True)
    from cspn_monodepth_amd.network import up_pooling
    for cls in (unet_ours.UpProj_Block, unet_ours.Gudi_UpProj_Block, unet_ours.Gudi_UpProj_Block_Cat,
                unet_ours.Simple_Gudi_UpConv_Block, unet_ours.Simple_Gudi_UpConv_Block_Last_Layer):
        assert issubclass(cls, up_pooling.MyBlock)
    assert unet_ours.decoder_sizes_for(228, 304) == unet_ours.DECODER_SIZES_NYU
    assert pkg.network.unet_ours is unet_ours                              # exported lazily from the network package


def test_unused_parameters_are_exactly_those_no_forward_touches(monkeypatch):
    """On the CPU, with stand-ins for the two HIP pieces (zero insertion written with stock ops; blur + mean of the guidance for
    the CSPN stage): after a backward from both outputs, the parameters without a gradient are unused_parameters()."""
    from cspn_monodepth_amd.network import unet_ours, up_pooling

    def unpool(self, x, scale):
        y = x.new_zeros(x.shape[0], x.shape[1], scale * x.shape[2], scale * x.shape[3])
        y[:, :, ::scale, ::scale] = x
        return y[:, :, :self.oheight, :self.owidth]

    monkeypatch.setattr(up_pooling.MyBlock, "_up_pooling", unpool)
    torch.manual_seed(0)
    m = unet_ours.resnet18(decoder_sizes=unet_ours.decoder_sizes_for(36, 44)).train()
    m.post_process_layer.forward = lambda x, guided, sparse_depth=None: x + guided.mean(1, keepdim=True) + 0 * sparse_depth
    x, guidance = m(torch.rand(2, 4, 36, 44))
    assert tuple(x.shape) == (2, 1, 36, 44) and tuple(guidance.shape) == (2, 8, 36, 44)
    (x.sum() + guidance.sum()).backward()
    no_grad = set(n for n, p in m.named_parameters() if p.grad is None)
    unused = set(id(p) for p in m.unused_parameters())
    assert no_grad == set(n for n, p in m.named_parameters() if id(p) in unused) == {"conv3.weight"}


def _g17_input():
    from oracle import cspn_oracle as orc
    rgb = orc.hash_uniform(170, 1, (1, 3, 228, 304), 0.0, 1.0)
    dep = orc.hash_uniform(170, 2, (1, 1, 228, 304), 0.5, 10.0)
    sp = orc.hash_sparse(170, 3, dep, 500.0 / (228 * 304))
    return np.concatenate([rgb, sp], 1), sp


@pytest.mark.gpu
def test_full_network_matches_reference_and_cspn_stage_matches_oracle(c_oracle):
    """The seeded, untrained resnet50 (same construction order => same weights as the reference's, asserted when the golden
    was made) in eval() mode on the golden's RGB-D frame: blur_depth, guidance and the refined x against the reference's CPU
    run; the CSPN stage on the tensors this network handed it against the C oracle's K x K forward."""
    from cspn_monodepth_amd.network import unet_ours as net
    z = load_golden("g17_unet_ours_full")
    torch.manual_seed(int(z["seed"]))
    m = net.resnet50().eval().to(DEV)
    xin, sp = _g17_input()
    with torch.no_grad():
        plain = m(torch.from_numpy(xin).to(DEV))
        m.return_cspn_io = True
        (x, guidance), (blur, g_in, s_in) = m(torch.from_numpy(xin).to(DEV))
    assert isinstance(plain, list) and len(plain) == 2 and tuple(plain[0].shape) == (1, 1, 228, 304) and tuple(plain[1].shape) == (1, 8, 228, 304)
    assert g_in is guidance and np.array_equal(s_in.cpu().numpy(), sp)
    sub = int(z["sub"])
    xn, gn, bn = x.cpu().numpy(), guidance.cpu().numpy(), blur.cpu().numpy()
    for name, got, want in (("blur", bn, z["blur_sub"]), ("guidance", gn, z["guidance_sub"]), ("x", xn, z["x_sub"])):
        scale = float(np.abs(want).max())
        err = float(np.abs(got[:, :, ::sub, ::sub] - want).max())
        print(name, "max err / range", err / scale)
        assert err <= 2e-3 * scale, (name, err, scale)          # ~170 stacked fp32 convolutions, MIOpen vs oneDNN
    want = c_oracle.pac_forward(bn, gn, s_in.cpu().numpy(), 24)
    print("cspn stage: max err / max|want|", float(np.abs(xn - want).max()) / float(np.abs(want).max()), "rmse", rmse(xn, want))
    assert float(np.abs(xn - want).max()) <= 1e-5 * float(np.abs(want).max()) and rmse(xn, want) <= 1e-4


@pytest.mark.gpu
def test_training_step_reaches_both_heads_through_the_hip_backward():
    from cspn_monodepth_amd.network import unet_ours as net
    torch.manual_seed(1)
    m = net.resnet50().to(DEV).train()
    B, H, W = 3, 228, 304
    depth = torch.rand(B, 1, H, W, device=DEV) * 9.5 + 0.5
    sparse = depth * (torch.rand(B, 1, H, W, device=DEV) < 500.0 / (H * W))
    x, guidance = m(torch.cat([torch.rand(B, 3, H, W, device=DEV), sparse], 1))
    assert tuple(x.shape) == (B, 1, H, W) and tuple(guidance.shape) == (B, 8, H, W)
    (depth - x).abs().mean().backward()
    for head in (m.gud_up_proj_layer5, m.gud_up_proj_layer6):
        g = head.conv1.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert bool(torch.isfinite(m.conv1_1.weight.grad).all()) and float(m.conv1_1.weight.grad.abs().max()) > 0
    unused = set(id(p) for p in m.unused_parameters())
    assert set(id(p) for p in m.parameters() if p.grad is None) == unused
    assert "libcspn_hip.so" in open("/proc/self/maps").read()


@pytest.mark.gpu
def test_unet_ours_tail_chain_matches_the_reference_with_this_modules_blocks():
    """Golden G14 (tests/golden/make_golden_r03.py, imported reference in fp64), under the assertions of
    tests/test_unet_host_model.py::test_unet_ours_tail_chain_matches_the_reference, with the block classes of
    network/unet_ours.py (MyBlock subclasses) in place of unet_cspn_nyu's: network/unet_ours.py:325-333 of the reference as ONE
    chain — Gudi_UpProj_Block_Cat (un-pooling with a crop) -> the depth and guidance heads ->
    CSPN_ours.AffinityPropagate(blur, guidance, sparse_depth=...), forward and backward."""
    from cspn_monodepth_amd.network import unet_ours as net
    from cspn_monodepth_amd.network.up_pooling import up_pooling
    z = load_golden("g14_unet_ours_tail")
    oh1, ow1, oh2, ow2 = (int(v) for v in z["sizes"])
    T = int(z["T"])
    C, Co = z["feat"].shape[1], z["x"].shape[1]
    blocks = {"cat": net.Gudi_UpProj_Block_Cat(C, Co, oh1, ow1), "head_d": net.Simple_Gudi_UpConv_Block_Last_Layer(Co, 1, oh2, ow2),
              "head_g": net.Simple_Gudi_UpConv_Block_Last_Layer(Co, 8, oh2, ow2)}
    for name, m in blocks.items():
        sd = {k[len(name) + 1:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(name + ".")}
        # the golden holds the buffers AFTER the recorded training-mode pass; the pass here starts from fresh statistics
        missing = m.load_state_dict({k: v for k, v in sd.items() if "running_" not in k}, strict=False)
        assert all("running_" in k or "num_batches" in k for k in missing.missing_keys) and not missing.unexpected_keys
        m.to(DEV).float().train()
    cspn = pkg.CSPN_ours.AffinityPropagate(T)
    feat = torch.from_numpy(z["feat"]).float().to(DEV).requires_grad_(True)
    side = torch.from_numpy(z["side"]).float().to(DEV).requires_grad_(True)
    sparse = torch.from_numpy(z["sparse"]).float().to(DEV)
    with torch.no_grad():
        up = up_pooling(feat.detach(), 2, oh1, ow1)
    assert np.array_equal(up.cpu().numpy(), z["up"].astype(np.float32))          # zero insertion + crop: exact
    x = blocks["cat"](feat, side)
    blur, guid = blocks["head_d"](x), blocks["head_g"](x)
    out = cspn(blur, guid, sparse_depth=sparse)
    (out * torch.from_numpy(z["cot"]).float().to(DEV)).sum().backward()

    def close(got, want, tol):
        want = np.asarray(want, np.float64)
        err = float(np.abs(got.detach().double().cpu().numpy() - want).max())
        return err <= tol * max(1.0, float(np.abs(want).max())), err

    for got, key, tol in ((x, "x", 2e-5), (blur, "blur", 2e-5), (guid, "guidance", 2e-5), (out, "out", 5e-5),
                          (feat.grad, "grad_feat", 5e-4), (side.grad, "grad_side", 5e-4),
                          (blocks["head_g"].conv1.weight.grad, "grad_head_g_weight", 5e-4),
                          (blocks["cat"].conv1.weight.grad, "grad_cat_conv1_weight", 5e-4)):
        ok, err = close(got, z[key], tol)
        assert ok, (key, err)
    # the running statistics after one training-mode pass equal the reference's
    for k in ("bn1.running_mean", "bn2.running_var", "sc_bn1.running_mean"):
        ok, err = close(blocks["cat"].state_dict()[k], z["cat." + k], 2e-5)
        assert ok, (k, err)
    # inference route of the same chain (no grad): the CSPN stage may take another schedule, the numbers stay
    with torch.no_grad():
        out2 = cspn(blur.detach(), guid.detach(), sparse_depth=sparse)
    assert float((out2 - out.detach()).abs().max()) <= 1e-5 * float(out.detach().abs().max())

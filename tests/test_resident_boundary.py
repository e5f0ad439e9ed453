"""The phase boundaries and the scoring tail of the 768-thread instances of cspn3_resident (csrc/cspn_resident.hip): the last step of
every phase but the last one is a peeled copy that stores each row to the exchange plane as soon as it is computed (no separate
publish pass, one barrier less), and the scored instances request the target quads inside the peeled final step.  Both are changes of
schedule only: the refined depth must stay the bits of the multi-launch schedule and of the 512-thread plan, the fused sums those of
the metric kernel on that result, and a publish that runs ahead of a neighbour still reading the plane would show as a forward that
differs from the one before it.

Shapes: the explicit plans tests/test_resident_clipped.py proves valid (B = 2, S = 8) — 60 x 64 in 2 x 3 tiles with a first row of 24
(region of 31 rows: the last strip of a thread column lies partly past the region) at T = 24 (three phases, both planes used), T = 17
(the final phase is ONE step: the peeled final step follows the exchange directly) and T = 7 (a single phase: no publish, the target
request alone); 60 x 96 in 3 x 3 tiles with a first row of 23 at T = 17 (inner columns with a two-sided halo).

Reference: network/libs/post_process/CSPN_new.py:26-92."""
import numpy as np
import pytest
import torch

import cspn_monodepth_amd as pkg
from cspn_monodepth_amd import functional as F
from conftest import bits_equal, lds_poison
from test_resident_clipped import dev, inputs, plan768

DEV = "cuda:0"
B = 2
# (H, W, tiles_x, tiles_y, tile_w, first row, T)
CASES = [(60, 64, 2, 3, 32, 24, 24), (60, 64, 2, 3, 32, 24, 17), (60, 96, 3, 3, 32, 23, 17), (60, 64, 2, 3, 32, 24, 7)]
IDS = ["%dx%d-%dx%d-h%d-T%d" % (c[0], c[1], c[2], c[3], c[5], c[6]) for c in CASES]

_TARGETS = {}


def target(c_oracle, d0, H, W):
    """A target with holes (5 % zeros: the metric's mask), made once per shape and never written."""
    if (H, W) not in _TARGETS:
        tgt = np.maximum(d0.cpu().numpy() + 0.1 * c_oracle.hash_normal(92, 9, (B, H, W)), 0.0).astype(np.float32)
        tgt[c_oracle.hash_uniform(93, 9, (B, H, W)) < 0.05] = 0.0
        _TARGETS[(H, W)] = dev(tgt)
    return _TARGETS[(H, W)]


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,nx,ny,tw,th0,T", CASES, ids=IDS)
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
def test_plain_forward_keeps_the_bits(H, W, nx, ny, tw, th0, T, sparse, c_oracle):
    gt, d0, sp, ref = inputs(c_oracle, B, H, W, T, sparse)
    with torch.no_grad():
        out = F.forward_resident(gt, d0, sp, T, int(sparse), _plan=plan768(B, nx, ny, tw, th0), guard=0)
        r512 = F.forward_resident(gt, d0, sp, T, int(sparse), threads=512, guard=0)
        with lds_poison():
            outp = F.forward_resident(gt, d0, sp, T, int(sparse), _plan=plan768(B, nx, ny, tw, th0), guard=0)
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert bits_equal(out, ref, T=T, sparse=sparse, which="768 vs multi-launch")
    assert bits_equal(out, r512, T=T, sparse=sparse, which="768 vs 512")
    assert bits_equal(outp, ref, T=T, sparse=sparse, which="768 under poisoned LDS")


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,nx,ny,tw,th0,T", CASES, ids=IDS)
@pytest.mark.parametrize("sparse", [False, True], ids=["nosparse", "sparse"])
def test_scored_forward_keeps_the_bits_and_the_sums(H, W, nx, ny, tw, th0, T, sparse, c_oracle):
    ev = pkg.evaluation
    gt, d0, sp, ref = inputs(c_oracle, B, H, W, T, sparse)
    tt = target(c_oracle, d0, H, W)
    with torch.no_grad():
        acc, acc2, acc512, accp, want = (ev.new_accumulator(DEV) for _ in range(5))
        out = F.forward_resident(gt, d0, sp, T, int(sparse), score=(tt, acc), _plan=plan768(B, nx, ny, tw, th0), guard=0)
        out2 = F.forward_resident(gt, d0, sp, T, int(sparse), score=(tt, acc2), _plan=plan768(B, nx, ny, tw, th0), guard=0)
        r512 = F.forward_resident(gt, d0, sp, T, int(sparse), score=(tt, acc512), threads=512, guard=0)
        with lds_poison():
            outp = F.forward_resident(gt, d0, sp, T, int(sparse), score=(tt, accp), _plan=plan768(B, nx, ny, tw, th0), guard=0)
        ev.metric_sums(ref, tt, out=want)
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert bits_equal(out, ref, T=T, sparse=sparse, which="scored 768 vs multi-launch")
    assert bits_equal(out, r512, T=T, sparse=sparse, which="scored 768 vs scored 512")
    assert bits_equal(out2, ref, T=T, sparse=sparse, which="second scored 768")
    assert bits_equal(outp, ref, T=T, sparse=sparse, which="scored 768 under poisoned LDS")
    got, exp = acc.sum(0).cpu().numpy(), want.sum(0).cpu().numpy()
    print("scored sums", got, exp)
    assert np.abs(exp).sum() > 0 and np.allclose(got, exp, rtol=2e-5)
    assert np.allclose(accp.sum(0).cpu().numpy(), exp, rtol=2e-5)
    # the same launch on a fresh accumulator: every slot receives the same additions in the same order
    assert same_bits(acc, acc2), (acc - acc2).abs().max().item()
    assert same_bits(acc, accp)


@pytest.mark.gpu
def test_200_scored_forwards_back_to_back_are_one_result(c_oracle):
    """Three phases on one workspace, 200 times without a host wait in between: a tile's early store to an exchange plane meets the
    neighbours' reads of that plane from the phase before last, the planes of the forward before, and the flag base as it advances
    from call to call.  Every forward must be the first one, depth and sums."""
    ev = pkg.evaluation
    H, W, nx, ny, tw, th0, T = CASES[0]
    gt, d0, sp, ref = inputs(c_oracle, B, H, W, T, False)
    tt = target(c_oracle, d0, H, W)
    plan = plan768(B, nx, ny, tw, th0)
    with torch.no_grad():
        accs = torch.zeros((200,) + tuple(ev.new_accumulator(DEV).shape), dtype=torch.float64, device=DEV)
        first = F.forward_resident(gt, d0, None, T, 0, score=(tt, accs[0]), _plan=plan, guard=0)
        differing = torch.zeros((), dtype=torch.int64, device=DEV)
        for k in range(1, 200):
            out = F.forward_resident(gt, d0, None, T, 0, score=(tt, accs[k]), _plan=plan, guard=0)
            differing += (out.view(torch.int32) != first.view(torch.int32)).any()
    torch.cuda.synchronize()
    F.check_resident_errors()
    assert bits_equal(first, ref, T=T, which="first of 200")
    assert int(differing.item()) == 0
    assert bool((accs.view(torch.int64) == accs[0].view(torch.int64)).all())
    assert accs[0].abs().sum().item() > 0

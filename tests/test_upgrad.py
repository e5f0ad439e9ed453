"""The gradients of the fused decoder-block head, as far as they exist: the numpy restatement of the two formulas on the compact map
(tests/upgrad_cases.py) and golden G28 (tests/golden/make_golden_g28.py: the reference's blocks in fp64, train() mode,
torch.autograd).  The restatement is held to torch.autograd on the dense un-pool + convolution and to every golden; integer-valued
cases agree exactly, real-valued ones to 1e-12.  No device code computes these gradients yet, so nothing here needs a GPU."""
import itertools
import json
import os

import numpy as np
import pytest

import upconv_cases as uc
import upgrad_cases as ug
from conftest import ROOT, golden_names, load_golden

INT_GOLDENS = golden_names("g28_upgrad_int_")
REAL_GOLDENS = golden_names("g28_upgrad_real_")
BLOCK_GOLDENS = golden_names("g28_upgrad_block_")
KINDS = ("Gudi_UpProj_Block", "Gudi_UpProj_Block_Cat", "Simple_Gudi_UpConv_Block")


def unpack(z):
    oh, ow, O, nf = (int(v) for v in z["geom"])
    return (oh, ow), O, [z["w%d" % k] for k in range(nf)], [z["g%d" % k] for k in range(nf)], z["gx"], [z["gw%d" % k] for k in range(nf)]


@pytest.mark.parametrize("hw,out_hw", uc.GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_restatement_equals_autograd_on_the_dense_form(hw, out_hw):
    for C, filters, integer in itertools.product((1, 3), ((3, 3), (2,)), (True, False)):
        shape = (2, C) + hw
        x, ws, _, _ = uc.make_inputs(7, shape, filters, integer)
        gys = ug.make_cotangents(7, shape, filters, out_hw, integer)
        for absent in (None, 0):                                                 # every cotangent given; the first one absent
            given = [None if k == absent and len(filters) > 1 else g for k, g in enumerate(gys)]
            gx, gws = ug.restate(x, ws, given, out_hw)
            dx, dws = ug.dense(x, ws, given, out_hw)
            for got, want in zip([gx] + gws, [dx] + dws):
                assert got.shape == want.shape and got.dtype == np.float64
                if integer:
                    assert np.array_equal(got, want)
                else:
                    assert np.abs(got - want).max() <= 1e-12
        # the pixels the crop removed get no gradient
        assert np.abs(gx).max() > 0 and not gx[:, :, (out_hw[0] + 1) // 2:].any() and not gx[:, :, :, (out_hw[1] + 1) // 2:].any()


def test_goldens_are_the_listed_cases():
    assert sorted(INT_GOLDENS + REAL_GOLDENS) == sorted("g28_upgrad_" + n for n in uc.GOLDEN_CASES) and len(uc.GOLDEN_CASES) == 11
    assert len(BLOCK_GOLDENS) == 3
    assert {uc.GOLDEN_CASES[n[len("g28_upgrad_block_"):]][0] for n in BLOCK_GOLDENS} == set(KINDS)
    manifest = json.load(open(os.path.join(ROOT, "tests", "golden", "g28_upgrad_manifest.json")))
    assert sorted(manifest["files"]) == sorted(INT_GOLDENS + REAL_GOLDENS + BLOCK_GOLDENS)
    for name in manifest["files"]:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) == manifest["files"][name]["bytes"] <= 131072


@pytest.mark.parametrize("name", INT_GOLDENS + REAL_GOLDENS)
def test_restatement_reproduces_the_golden(name):
    z = load_golden(name)
    out_hw, O, ws, gys, gx, gws = unpack(z)
    kind, shape, want_hw, O_w, integer = uc.GOLDEN_CASES[name[len("g28_upgrad_"):]]
    assert z["x"].shape == shape and out_hw == want_hw and O == O_w and len(ws) == (1 if kind.startswith("Simple") else 2)
    rx, rws = ug.restate(z["x"], ws, gys, out_hw)
    for got, want in zip([rx] + rws, [gx] + gws):
        assert got.shape == want.shape
        if integer:
            assert want.dtype == np.float32 and np.array_equal(got, want.astype(np.float64))
        else:
            assert want.dtype == np.float64 and np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("name", BLOCK_GOLDENS)
def test_block_goldens_hold_a_whole_training_step(name):
    """What a later device path is compared with: output, running statistics, and the gradient of x and of every parameter."""
    z = load_golden(name)
    kind, shape, out_hw, O, integer = uc.GOLDEN_CASES[name[len("g28_upgrad_block_"):]]
    params = sorted(k[2:] for k in z if k.startswith("p_"))
    assert sorted(k[2:] for k in z if k.startswith("g_")) == params and "conv1.weight" in params
    assert ("sc_conv1.weight" in params) == (kind != "Simple_Gudi_UpConv_Block") and ("side" in z) == kind.endswith("_Cat")
    assert z["out"].shape == z["cot"].shape == (shape[0], O) + out_hw and z["out"].dtype == np.float64 and z["gx"].shape == shape
    bns = sorted(k[3:] for k in z if k.startswith("rm_"))
    assert bns == sorted(k[3:] for k in z if k.startswith("rv_")) == sorted(p[:-7] for p in params if p.endswith(".weight") and z["p_" + p].ndim == 1)
    # one forward with momentum 0.1 from the initial (0, 1): the statistics moved, and the variance stayed positive
    assert all(np.abs(z["rm_" + b]).max() > 0 and (z["rv_" + b] > 0).all() for b in bns)
    # the block ran on the x of the head golden of the same case (kept there, not twice), with conv1 / sc_conv1 holding its filters
    head = load_golden("g28_upgrad_" + name[len("g28_upgrad_block_"):])
    assert "x" not in z and head["x"].shape == z["gx"].shape and np.array_equal(z["p_conv1.weight"], head["w0"])
    assert "p_sc_conv1.weight" not in z or np.array_equal(z["p_sc_conv1.weight"], head["w1"])

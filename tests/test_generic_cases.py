"""CPU test of the case table of tests/test_generic_paths.py (tests/generic_cases.py): the oracle gradients every GPU case is
compared with are finite and large enough that an error relative to max|want| — no floor — means something, and the table
covers the shapes the generic kernels can go wrong at."""
import numpy as np
import pytest

import generic_cases as gc


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_oracle_gradients_are_finite_and_scaled(case):
    z, ref = gc.inputs(case), gc.reference(case)
    B, H, W = case.shape
    assert z["a"].shape == (B, case.C, H, W) and z["b"].shape == (B, case.CX, H, W) and z["cot"].shape == (B, case.CX, H, W)
    assert ref["out"].shape == z["b"].shape and ref["grad_a"].shape == z["a"].shape and ref["grad_b"].shape == z["b"].shape
    for name in ("out", "grad_a", "grad_b"):
        assert np.isfinite(ref[name]).all(), name
    for name in ("grad_a", "grad_b"):
        assert float(np.abs(ref[name]).max()) >= gc.MIN_GRAD_SCALE, (name, float(np.abs(ref[name]).max()))
        # the border ring is compared on its own, against its own maximum: that scale must not be tiny either
        assert float(np.abs(gc.ring(ref[name])).max()) >= 0.1 * float(np.abs(ref[name]).max()), name
    # a cotangent scale is a power of two (exact in fp16 and fp32)
    assert np.log2(case.cot_scale) == int(np.log2(case.cot_scale))
    if case.sparse:
        anchors = int((z["s"] > 0).sum())
        assert z["s"].shape == (B, 1, H, W) and 0 < anchors < B * H * W          # some pixels blended, some not
        assert all(int((z["s"][b] > 0).sum()) > 0 for b in range(B))                     # every image holds an anchor
    else:
        assert z["s"] is None
    if case.module == "new" and case.C > 8:
        assert not ref["grad_a"][:, 8:].any() and np.abs(z["a"][:, 8:]).max() > 0
    if case.dtype == "f16":
        for name in ("a", "b", "s", "cot"):
            if z[name] is not None:
                assert np.array_equal(z[name].astype(np.float16).astype(np.float32), z[name]), name


def test_references_are_shared_and_read_only():
    a, b = gc.BY_NAME["new-g-12x16-view-a-f32"], gc.BY_NAME["new-g-12x16-view-all-f32"]
    assert gc.numeric_key(a) == gc.numeric_key(b) == gc.numeric_key(gc.BY_NAME["new-g-12x16-scalar-f32"])
    assert gc.reference(a) is gc.reference(b) and gc.inputs(a) is gc.inputs(b)
    with pytest.raises(ValueError):
        gc.reference(a)["grad_a"][0, 0, 0, 0] = 1.0
    seeds = {}
    for c in gc.CASES:
        seeds.setdefault(c.seed, set()).add(gc.numeric_key(c))
    assert all(len(v) == 1 for v in seeds.values())               # fresh seeds per numeric case


def test_table_covers_the_shapes_and_routes():
    cases = gc.CASES
    generic_backward = [c for c in cases if gc.expected_calls(c)[0] > 0]
    # the padded fp16 tap-volume index, with its batch offset, in the backward direction: H*W % 4 in {1, 2, 3}, B = 2, fp16
    for module_cases in (cases, [c for c in generic_backward if c.dtype == "f16"]):
        assert {c.shape[1] * c.shape[2] % 4 for c in module_cases} >= ({0, 1, 2, 3} if module_cases is cases else {1, 2, 3})
    assert all(c.shape[0] >= 2 for c in cases)
    pixels = [c.shape[0] * c.shape[1] * c.shape[2] for c in generic_backward]
    assert any(n < 256 for n in pixels) and any(n > 256 and n % 256 for n in pixels)      # less than a block; a partial second block
    for module in ("new", "ours"):
        mine = [c for c in cases if c.module == module]
        assert {c.route for c in mine} == {"scalar", "view"}
        assert {c.dtype for c in mine} == {"f32", "f16"}
        assert {c.sparse for c in mine} == {True, False}
        views = {(c.dtype, c.k, c.mis) for c in mine if c.route == "view"}
        for mis in gc.ONE_AT_A_TIME:
            assert ("f32", 1, mis) in views and ("f16", 1, mis) in views and ("f16", 4, mis) in views
        assert all(c.shape[2] % 4 == 0 for c in mine if c.route == "view")
    ours = [c for c in cases if c.module == "ours"]
    assert {c.K for c in ours if c.route == "scalar" and c.dtype == "f32"} == {3, 5, 7}
    assert any(c.K > 2 * min(c.shape[1:]) for c in ours)                                   # smaller than the window
    assert any(c.CX == 2 for c in ours) and {c.state for c in ours if c.dtype == "f16"} == {"reference", None}
    for K in (3, 5, 7):
        assert any(c.T == 1 for c in ours if c.K == K)
    assert any(c.C == 8 for c in cases if c.module == "new") and any(c.C == 12 for c in cases if c.module == "new")
    # force_scalar at W % 4 == 0 keeps the fused tail; at any other width both unfused stages run
    assert gc.expected_calls(gc.BY_NAME["new-g-12x16-scalar-f32"]) == (0, 1)
    assert gc.expected_calls(gc.BY_NAME["new-g-7x5-scalar-f32"]) == (1, 1)
    assert gc.expected_calls(gc.BY_NAME["new-g-12x16-view-all-f32"]) == (1, 1)
    assert gc.expected_calls(gc.BY_NAME["new-g-12x16-view-cot-f32"]) == (0, 0)
    assert gc.expected_calls(gc.BY_NAME["ours-k3-7x5-cx2-scalar-f32"]) == (2, 2)


@pytest.mark.parametrize("vc", gc.VIEW_CASES, ids=lambda v: v.name)
def test_view_case_gradients_are_finite_and_scaled(vc):
    z = gc.view_inputs(vc)
    for name in ("grad_a", "grad_b"):
        assert np.isfinite(z[name]).all() and float(np.abs(z[name]).max()) >= gc.MIN_GRAD_SCALE, (name, float(np.abs(z[name]).max()))
        assert float(np.abs(gc.ring(z[name])).max()) >= 0.1 * float(np.abs(z[name]).max()), name
    assert 0 < int((z["s"] > 0).sum()) < z["s"].size
    if vc.kind == "halfcot":
        assert np.array_equal(z["cot"].astype(np.float16).astype(np.float32), z["cot"])
    assert {v.kind for v in gc.VIEW_CASES if v.module == vc.module and v.K == vc.K and v.shape == vc.shape} == set(gc.VIEW_KINDS)

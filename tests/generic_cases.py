"""Case table of tests/test_generic_paths.py (the generic one-pixel kernels and view inputs of both propagation modules):
the cases, their seeded inputs, the oracle references and the route each case is expected to take through the host dispatch.
No torch and no package code: numpy and the oracle only, so tests/test_generic_cases.py checks the table without a GPU.

A case reaches the generic kernels in one of two ways:
  route "scalar": plan=dict(force_scalar=1) — no row padding, every launch of the propagation loop is cspn_prop_scalar;
  route "view":   plan None, W % 4 == 0, and the tensors named in `mis` are contiguous views that start `k` elements into a
                  buffer one quad longer than needed (fp32: 4 bytes off; fp16: 2 bytes off at k = 1, 8 bytes off at k = 4 —
                  8-byte aligned, which the engine's 16-byte predicates must still refuse).
"""
import collections
import functools

import numpy as np

from oracle import cspn_oracle as orc

Case = collections.namedtuple("Case", "name module K shape C T sparse dtype route mis k state CX seed cot_scale")
# module "new" (CSPN_new, 3x3: C guidance channels, CX = 1) / "ours" (CSPN_ours, K x K: C = K*K-1 guided channels, x of CX channels)
# mis: subset of ("a", "b", "s", "cot") — a = guidance / guided, b = blur depth / x, s = sparse depth, cot = the cotangent
# state: CSPN_ours state_dtype for fp16 inputs ("reference" = fp32 planes, None = fp16 planes)
# cot_scale: power of two the unit-normal cotangent is multiplied by, so that max|gradient| >= MIN_GRAD_SCALE (the gradient is
#            linear in the cotangent; the errors are relative to max|want|, so the bars are unchanged)

SPARSE_DENSITY = 0.1
MIN_GRAD_SCALE = 0.5
ALL = ("a", "b", "s", "cot")
ONE_AT_A_TIME = (("a",), ("b",), ("s",), ("cot",), ALL)

# fp32 bars (relative to max|want|, no floor): the suite's bars against the fp64 oracle
BAR_F32 = {"new": (5e-4, 5e-5), "ours": (5e-4, 5e-5)}           # (guidance | guided, depth | x)
REL_TOL = 1e-5                                                   # fp32 forward against the fp32 oracle (conftest.rel_err)
# fp16 bars (relative to max(1, max|want|)): the suite's bars for fp16 storage
BAR_F16_FWD = {"new": 4e-3, "ours": 6e-3}
BAR_F16_GRAD = (3e-2, 1e-2)                                      # (guidance | guided, depth | x)

RESEED_3X3 = 1
RESEED_KXK = {("k7-4x3", 3): 2, ("k7-4x3", 1): 2}
_NUMERIC = {}      # numeric key -> seed: cases that differ only in the route share inputs and references


def _case(name, module, K, shape, T, sparse, dtype="f32", route="scalar", mis=(), k=0, state="reference", C=None, CX=1,
          cot_scale=1.0, reseed=0):
    """reseed: picks another seed for a tiny sparse case whose first seed left an image without an anchor."""
    C = (12 if module == "new" else K * K - 1) if C is None else C
    key = (module, K, shape, C, T, sparse, dtype, CX)
    seed = _NUMERIC.setdefault(key, 7001 + 2 * len(_NUMERIC) + 1000 * reseed)
    return Case(name, module, K, shape, C, T, sparse, dtype, route, tuple(mis), k, state, CX, seed, float(cot_scale))


def _build():
    cases = []
    # ---- 3x3, force_scalar.  C = 12: channels 8..11 must come back exactly zero; g-3x3 uses C = 8
    for name, shape, T, sparse, C in (("g-7x5", (2, 7, 5), 4, True, 12), ("g-9x18", (2, 9, 18), 5, True, 12),
                                      ("g-5x9", (2, 5, 9), 3, False, 12), ("g-3x3", (2, 3, 3), 3, True, 8),
                                      ("g-12x16", (2, 12, 16), 5, True, 12), ("g-12x16-nosp", (2, 12, 16), 5, False, 12)):
        cases.append(_case("new-%s-scalar-f32" % name, "new", 3, shape, T, sparse, C=C, reseed=RESEED_3X3 if name == "g-3x3" else 0))
        if name != "g-3x3":
            cases.append(_case("new-%s-scalar-f16" % name, "new", 3, shape, T, sparse, "f16", C=C))
    # ---- 3x3, misaligned views of g-12x16
    for mis in ONE_AT_A_TIME:
        tag = "all" if mis == ALL else mis[0]
        cases.append(_case("new-g-12x16-view-%s-f32" % tag, "new", 3, (2, 12, 16), 5, True, "f32", "view", mis, 1))
        for k in (1, 4):
            cases.append(_case("new-g-12x16-view-%s-f16-k%d" % (tag, k), "new", 3, (2, 12, 16), 5, True, "f16", "view", mis, k))
    cases.append(_case("new-g-12x16-nosp-view-all-f32", "new", 3, (2, 12, 16), 5, False, "f32", "view", ALL, 1))
    # ---- K x K, force_scalar; the two shapes smaller than their window need a scaled cotangent (see the CPU test)
    # (K, shape, T, cotangent scale with sparse / without / at T = 1)
    for K, shape, T, scales in ((3, (2, 7, 5), 4, (1, 2, 1)), (5, (2, 9, 18), 4, (1, 2, 1)), (7, (2, 5, 9), 3, (2, 16, 1)),
                                (7, (2, 4, 3), 3, (2, 128, 1)), (5, (2, 3, 2), 3, (1, 128, 2))):
        tag = "k%d-%dx%d" % (K, shape[1], shape[2])
        for sparse in (True, False):
            cases.append(_case("ours-%s-%s-scalar-f32" % (tag, "sp" if sparse else "nosp"), "ours", K, shape, T, sparse,
                               cot_scale=scales[0 if sparse else 1], reseed=RESEED_KXK.get((tag, T), 0)))
        # T = 1: dhist is unused
        cases.append(_case("ours-%s-t1-scalar-f32" % tag, "ours", K, shape, 1, K != 5, cot_scale=scales[2],
                           reseed=RESEED_KXK.get((tag, 1), 0)))
    cases.append(_case("ours-k3-7x5-cx2-scalar-f32", "ours", 3, (2, 7, 5), 4, True, CX=2))
    # ---- K x K, misaligned views at 2,6,8: W % 8 == 0, so alignment alone keeps the resident kernels out
    for K in (5, 3):
        for mis in ONE_AT_A_TIME:
            tag = "all" if mis == ALL else mis[0]
            cases.append(_case("ours-k%d-6x8-view-%s-f32" % (K, tag), "ours", K, (2, 6, 8), 3, True, "f32", "view", mis, 1))
        cases.append(_case("ours-k%d-6x8-nosp-view-all-f32" % K, "ours", K, (2, 6, 8), 3, False, "f32", "view", ALL, 1,
                           cot_scale=4 if K == 5 else 2))
        cases.append(_case("ours-k%d-6x8-t1-view-all-f32" % K, "ours", K, (2, 6, 8), 1, True, "f32", "view", ALL, 1))
    # ---- K = 5, fp16 storage, both state dtypes
    for state in ("reference", None):
        st = "ref" if state == "reference" else "half"
        for sparse in (True, False):
            cases.append(_case("ours-k5-9x18-%s-scalar-f16-%s" % ("sp" if sparse else "nosp", st), "ours", 5, (2, 9, 18), 4, sparse,
                               "f16", state=state, cot_scale=1 if sparse else 4))
        for mis in ONE_AT_A_TIME:
            tag = "all" if mis == ALL else mis[0]
            for k in (1, 4):
                cases.append(_case("ours-k5-6x8-view-%s-f16-k%d-%s" % (tag, k, st), "ours", 5, (2, 6, 8), 3, True, "f16", "view",
                                   mis, k, state))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def numeric_key(case):
    """What the values of a case depend on: cases with one key share inputs, references and the vector-path results."""
    return (case.module, case.K, case.shape, case.C, case.T, case.sparse, case.dtype, case.CX, case.seed, case.cot_scale)


def _gen():
    from oracle import c_oracle
    c_oracle.build()
    return c_oracle


def _round(a, dtype):
    """fp16 cases: the inputs are rounded to half first and the oracle gets the rounded values."""
    if a is None or dtype == "f32":
        return a
    return a.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(key):
    module, K, (B, H, W), C, T, sparse, dtype, CX, seed, cot_scale = key
    gen = _gen()
    if module == "new":
        a, b, s = gen.synthetic_inputs(seed, B, H, W, C, SPARSE_DENSITY * H * W if sparse else None)
    else:
        a = gen.hash_normal(seed, 1, (B, C, H, W))
        b = gen.hash_uniform(seed, 2, (B, CX, H, W), 0.0, 10.0)
        s = gen.hash_sparse(seed, 3, b[:, :1], SPARSE_DENSITY) if sparse else None
    cot = gen.hash_normal(seed + 1, 9, (B, CX, H, W)) * np.float32(cot_scale)
    out = {n: _round(v, dtype) for n, v in (("a", a), ("b", b), ("s", s), ("cot", cot))}
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def inputs(case):
    """dict a, b, s (or None), cot: fp32 numpy arrays (fp16 cases: values representable in half).  Read-only, shared."""
    return _inputs(numeric_key(case))


@functools.lru_cache(maxsize=None)
def _reference(key):
    module, K, (B, H, W), C, T, sparse, dtype, CX, seed, cot_scale = key
    z = _inputs(key)
    gen = _gen()
    if module == "new":
        out = gen.cspn3_forward(z["a"], z["b"], z["s"], T)
        ga, gb = gen.cspn3_backward(z["a"], z["b"], z["s"], z["cot"], T, np.float64)
    else:
        out = np.concatenate([gen.pac_forward(z["b"][:, c:c + 1], z["a"], z["s"], T) for c in range(CX)], axis=1)
        gb, ga = orc.pac_backward_multichannel(z["b"], z["a"], z["s"], z["cot"], T, np.float64)
    ref = dict(out=out, grad_a=np.asarray(ga, np.float64), grad_b=np.asarray(gb, np.float64))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def reference(case):
    """dict out (fp32 restatement of the forward), grad_a (guidance | guided), grad_b (depth | x) in fp64.  Read-only, shared."""
    return _reference(numeric_key(case))


def ring(a):
    """The border ring of [..., H, W]: first and last row and column, as a flat array."""
    m = np.zeros(a.shape[-2:], bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return a[..., m]


def max_err(got, want):
    """(max |got - want| / max |want|, the same over the border ring alone): no floor under the scale."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    return (float(np.abs(got - want).max() / np.abs(want).max()),
            float(np.abs(ring(got) - ring(want)).max() / np.abs(ring(want)).max()))


def floored_err(got, want):
    """max |got - want| / max(1, max |want|): the scale of the suite's fp16 bars."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    return float(np.abs(got - want).max() / max(1.0, float(np.abs(want).max())))


# ------------------------------------------------------------------------------------------------ expected route
def engine_misaligned(case):
    """The misaligned tensors that REACH the engine misaligned (route "view").  The cotangent never does: the reverse sweep
    clones a misaligned G_T.  CSPN_ours with fp16 inputs and the reference's fp32 state converts x and sparse into fresh
    (aligned) fp32 planes.  A sparse view of a case without sparse depth does not exist."""
    if case.route != "view":
        return ()
    keep = [n for n in case.mis if n != "cot" and (n != "s" or case.sparse)]
    if case.module == "ours" and case.dtype == "f16" and case.state == "reference":
        keep = [n for n in keep if n == "a"]
    return tuple(keep)


def forward_generic(case):
    """Does the forward run generic kernels (prepare and / or cspn_prop_scalar)?"""
    return case.route == "scalar" or bool(engine_misaligned(case))


def loop_generic(case):
    """Is every launch of the forward propagation loop cspn_prop_scalar?  (force_scalar, or a misaligned depth / sparse plane;
    a misaligned guidance alone only puts the prepare pass — and the guidance / guided gradient — on the generic kernels.)"""
    return case.route == "scalar" or any(n in ("b", "s") for n in engine_misaligned(case))


def expected_calls(case):
    """(calls of functional._grad_weights, calls of functional.transpose_weights or None = not asserted) in one backward.

    _grad_weights (the unfused tail: cspn_grad_weights + cspn3_grad_guidance | cspn_pac_grad_guided) runs when the fused
    tail's predicate fails: W % 4 != 0, or a misaligned guidance (3x3 only: the K x K tail writes a fresh gradient), depth
    or sparse plane.  transpose_weights (reverse sweep by copy + cspn_propagate with BLEND_PREMASK | BLEND_NONE) runs under
    force_scalar, and for views when the fp32 sparse plane is misaligned (a half sparse plane is converted to a fresh fp32
    one for the sweep).  K >= 5 takes the copy by default — or a weight-resident sweep — so the count shows nothing there."""
    W = case.shape[2]
    mis = engine_misaligned(case)
    if case.route == "scalar":
        return (case.CX if W % 4 else 0), case.CX
    tail_inputs = ("a", "b", "s") if case.module == "new" else ("b", "s")
    gw = case.CX * int(any(n in tail_inputs for n in mis))
    if case.K >= 5:
        return gw, None
    return gw, case.CX * int("s" in mis and case.dtype == "f32")


def sweep_generic(case):
    """Does the reverse sweep run on the generic kernels (cspn_transpose_kernel + cspn_prop_scalar)?"""
    if case.route == "scalar":
        return True
    return "s" in engine_misaligned(case) and case.dtype == "f32"


# ------------------------------------------------------------------------------------------------ views through autograd
ViewCase = collections.namedtuple("ViewCase", "name module K shape T kind seed")
# kind: "head"  — both inputs are channel slices [:, :1] / [:, 1:] of ONE leaf (non-contiguous, guidance at a channel offset)
#       "batch" — the inputs are batch slices big[1:B+1] of leaves with B + 2 images
#       "expanded" — out.sum().backward(): an expanded cotangent of ones
#       "transposed" — out.transpose(2, 3) fed a contiguous gradient: a non-contiguous cotangent
#       "halfcot" — out.half() fed a half gradient: a cotangent rounded to half arrives at an fp32 module
VIEW_KINDS = ("head", "batch", "expanded", "transposed", "halfcot")
VIEW_CASES = tuple(ViewCase("%s-k%d-%dx%dx%d-%s" % (module, K, shape[0], shape[1], shape[2], kind), module, K, shape, T, kind,
                            8101 + 2 * (3 * si + mi))
                   for mi, (module, K, T) in enumerate((("new", 3, 4), ("ours", 3, 3), ("ours", 5, 3)))
                   for si, shape in enumerate(((2, 12, 16), (3, 8, 12)))
                   for kind in VIEW_KINDS)


@functools.lru_cache(maxsize=None)
def _view_inputs(key):
    module, K, (B, H, W), T, seed, cot_kind = key
    gen = _gen()
    if module == "new":
        a, b, s = gen.synthetic_inputs(seed, B, H, W, 12, SPARSE_DENSITY * H * W)
    else:
        a = gen.hash_normal(seed, 1, (B, K * K - 1, H, W))
        b = gen.hash_uniform(seed, 2, (B, 1, H, W), 0.0, 10.0)
        s = gen.hash_sparse(seed, 3, b, SPARSE_DENSITY)
    cot = gen.hash_normal(seed + 1, 9, (B, 1, H, W))
    if cot_kind == "expanded":
        cot = np.ones_like(cot)
    elif cot_kind == "halfcot":
        cot = _round(cot, "f16")
    z = dict(a=a, b=b, s=s, cot=cot)
    if module == "new":
        ga, gb = gen.cspn3_backward(a, b, s, cot, T, np.float64)
    else:
        gb, ga = orc.pac_backward(b, a, s, cot, T, np.float64)
    z.update(grad_a=np.asarray(ga, np.float64), grad_b=np.asarray(gb, np.float64))
    for v in z.values():
        v.setflags(write=False)
    return z


def view_inputs(vc):
    """dict a, b, s, cot (fp32) and the fp64 oracle gradients grad_a, grad_b for that cotangent.  Read-only; the kinds that
    share a cotangent ("head", "batch", "transposed": unit normal) share one entry."""
    cot_kind = vc.kind if vc.kind in ("expanded", "halfcot") else "normal"
    return _view_inputs((vc.module, vc.K, vc.shape, vc.T, vc.seed, cot_kind))

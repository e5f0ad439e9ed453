"""GPU tests of the generic one-pixel-per-thread kernels and of view inputs of both propagation modules (CSPN_new, CSPN_ours).

The host dispatch sends every call through predicates on width, alignment, strides and contiguity; where one fails the call
runs on the generic kernels.  Odd widths alone never get there (the modules pad rows to whole quads), so the cases of
tests/generic_cases.py force the route with plan=dict(force_scalar=1) or with misaligned contiguous views, and every case also
shows WHICH route ran (call counters on functional._grad_weights / transpose_weights, the *_supported predicates, and the
vector-only C entries, which must refuse the same pointers before any launch).

kernel                                   reaching predicate                                            cases
---------------------------------------  ------------------------------------------------------------  -----------------------------------
cspn_prop_scalar BLEND_NONE              propagate_typed `vec` false: force_scalar | W % 4 | misaligned  new-g-5x9-scalar-*, ours-*-nosp-scalar-*
cspn_prop_scalar BLEND_SPARSE            the same, with a sparse plane                                   new-g-7x5-scalar-*, new-*-view-b-*, ours-*-sp-scalar-*
cspn_prop_scalar BLEND_PREMASK           reverse sweep by copy: force_scalar, or misaligned fp32 sparse  *-scalar-* with sparse, *-view-s-f32, *-view-all-f32
cspn3_prepare_kernel                     not from_guidance_supported / resident_supported               every new-* case but view-cot
cspn_pac_prepare_kernel                  fp32 guided; fp16: H*W % 4 != 0 or misaligned guided           ours-*-f32, ours-k5-9x18-*-f16-*, ours-*-view-a-f16-*
cspn_transpose_kernel                    _reverse_sweep: force_scalar plan | p is None | K >= 5          *-scalar-*, *-view-s-f32, *-view-all-f32; ABI test K = 3, 5, 7
cspn_grad_weights_kernel<K, float>       tail_vector_ok false: W % 4 | misaligned d0 / sparse / output   *-scalar-f32 at W % 4 != 0, *-view-b-f32, *-view-s-f32; ABI test
cspn_grad_weights_kernel<K, half>        the same with half planes                                       new-*-scalar-f16 at W % 4 != 0, *-view-b-f16-*, ours-*-f16-*-half
cspn3_grad_guidance_kernel               _tail_vector_ok false (incl. misaligned guidance, strides)      new-*-scalar-* at W % 4 != 0, new-*-view-a|b|s|all-*; ABI test
cspn_pac_grad_guided_kernel              _tail_vector_ok false                                          ours-*-scalar-*, ours-*-view-b|s|all-f32, ours-*-f16-*-half
Taps<__half>::idx, H*W % 4 != 0, B = 2   fp16 tap volume with padded images and the batch offset         new-g-7x5|9x18|5x9-scalar-f16, ours-k5-9x18-*-scalar-f16-*

Bars: fp32 forward 1e-5 (conftest.rel_err) against the fp32 oracle, fp32 gradients 5e-4 (guidance / guided) and 5e-5 (depth / x)
of max|want| against the fp64 oracle — no floor under the scale, and once more over the border ring alone; fp16 storage at the
suite's bars for these dtypes.  Generic against vector on the same values: rtol 1e-5, atol 1e-6 max|ref| (fp32).
"""
import numpy as np
import pytest
import torch

import cspn_monodepth_amd as pkg
from cspn_monodepth_amd import functional as F
from conftest import rel_err
import generic_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALAR = dict(force_scalar=1)
NAN = float("nan")


def put(a, half=False, k=0, grad=False):
    """numpy -> device tensor; k > 0: a contiguous view that starts k elements into a buffer one quad longer than needed
    (one element where k elements of this dtype are a whole quad: the fp32 cotangent of a k = 4 fp16 case)."""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(DEV)              # (a copy: the shared inputs are read-only)
    if half:
        t = t.half()
    if k and (k * t.element_size()) % 16 == 0:
        k = 1
    if k:
        n, quad = t.numel(), 16 // t.element_size()
        flat = torch.empty(n + quad, dtype=t.dtype, device=DEV)
        flat[k:k + n] = t.reshape(-1)
        t = flat[k:k + n].view(t.shape).detach()
        assert t.is_contiguous() and t.data_ptr() % 16 == k * t.element_size()
    return t.requires_grad_(True) if grad else t


def module(case, plan):
    if case.module == "new":
        return pkg.CSPN_new.AffinityPropagate(case.T, 3, plan=plan)
    return pkg.CSPN_ours.AffinityPropagate(case.T, plan=plan, state_dtype=case.state)


def call(m, case, a, b, s):
    return m(a, b, s) if case.module == "new" else m(b, a, sparse_depth=s)


def run(case, plan, mis=(), k=0):
    """Forward + backward + the no-grad forward of one case; the tensors named in `mis` are misaligned views."""
    z, half = gc.inputs(case), case.dtype == "f16"

    def off(name):
        return k if name in mis else 0

    a, b, s = put(z["a"], half, off("a"), grad=True), put(z["b"], half, off("b"), grad=True), put(z["s"], half, off("s"))
    m = module(case, plan)
    out = call(m, case, a, b, s)
    cot = put(z["cot"], out.dtype == torch.float16, off("cot"))
    out.backward(cot)
    with torch.no_grad():
        out2 = call(m, case, a.detach(), b.detach(), s)
    torch.cuda.synchronize()
    return dict(a=a, b=b, s=s, cot=cot, out=out.detach(), out_nograd=out2)


_VECTOR = {}      # numeric key, state -> the default (quad) modules' results on aligned copies: computed once, shared, left unchanged


def vector_run(case):
    key = (gc.numeric_key(case), case.state)
    if key not in _VECTOR:
        r = run(case, None)
        _VECTOR[key] = dict(out=r["out_nograd"], ga=r["a"].grad, gb=r["b"].grad)
    return _VECTOR[key]


def count_calls(monkeypatch):
    calls = dict(gw=0, tr=0)
    gw, tr = F._grad_weights, F.transpose_weights

    def counted_gw(*args, **kw):
        calls["gw"] += 1
        return gw(*args, **kw)

    def counted_tr(*args, **kw):
        calls["tr"] += 1
        return tr(*args, **kw)

    monkeypatch.setattr(F, "_grad_weights", counted_gw)
    monkeypatch.setattr(F, "transpose_weights", counted_tr)
    return calls


def last_error():
    return F._lib.lib().cspn_last_error().decode()


def np32(t):
    return t.detach().float().cpu().numpy()


def engine_planes(case, r):
    """(a, d0, sparse) as the engine gets them: [B,H,W] planes, CSPN_ours in its state dtype."""
    a, b, s = r["a"].detach(), r["b"].detach(), r["s"]
    d0, sp = b[:, 0], None if s is None else s[:, 0]
    if case.module == "ours":
        sdt = torch.float32 if (case.state == "reference" and b.dtype == torch.float16) else b.dtype
        d0, sp = d0.to(sdt), None if sp is None else sp.to(sdt)
    return a, d0.contiguous(), None if sp is None else sp.contiguous()


def check_route(case, r, plan, calls):
    """The case really ran generic: Python-side counters and predicates, then the vector-only C entries on the same pointers."""
    B, H, W = case.shape
    K, T, NT = case.K, case.T, case.K * case.K - 1
    gw_want, tr_want = gc.expected_calls(case)
    assert calls["gw"] == gw_want, (calls, gw_want, tr_want)
    if tr_want is not None:
        assert calls["tr"] == tr_want, (calls, gw_want, tr_want)
    a, d0, sp = engine_planes(case, r)
    mis = gc.engine_misaligned(case)
    for name, t in (("a", a), ("b", d0), ("s", sp)):
        if t is not None and case.CX == 1:
            assert (t.data_ptr() % 16 != 0) == (name in mis), (name, mis)
    if case.module == "new":
        if gc.forward_generic(case):
            assert F.from_guidance_supported(a, d0, sp, plan) is False
            assert F.resident_supported(a, d0, sp, T, plan) is None
        else:       # only the cotangent is misaligned: the reverse sweep clones it, and every launch is a vector one
            assert F.from_guidance_supported(a, d0, sp, plan) is True
    elif gc.forward_generic(case):
        assert F.pac_resident_supported(a, d0, sp, T, plan) is None
    L, P, st = F._lib.lib(), F._p, F._stream(torch.device(DEV))
    hist = torch.empty((T, B, H, W), dtype=d0.dtype, device=DEV)
    ghist = torch.empty((T, B, H, W), dtype=torch.float32, device=DEV)
    g_T = torch.empty((B, H, W), dtype=torch.float32, device=DEV)
    gd0 = torch.empty((B, H, W), dtype=torch.float32, device=DEV)
    w = F._weight_buffer(B, NT, H, W, a.dtype, DEV)
    if gw_want:
        # tail_vector_ok is shared by the fused tails and cspn_grad_weights: the tail must refuse these pointers (no launch)
        if case.module == "new":
            S, gg = torch.empty((B, H, W), dtype=torch.float32, device=DEV), torch.empty_like(a)
            ok = L.cspn3_backward_tail(P(d0), P(hist), P(g_T), P(ghist), P(sp), P(a), a.stride(0), a.stride(1), case.C, None, P(S),
                                       P(gg), P(gd0), F._dt(a), B, H, W, T, st)
        else:
            gg = torch.empty((B, NT, H, W), dtype=a.dtype, device=DEV)
            ok = L.cspn_pac_backward_tail(P(d0), P(hist), P(g_T), P(ghist), P(sp), P(w), P(gg), P(gd0), 0, F._dt(d0), F._dt(w),
                                          B, H, W, K, T, st)
        assert ok == 0 and "16-byte aligned" in last_error(), last_error()
    if gc.loop_generic(case):
        # `vec` of propagate_typed is shared by cspn_propagate and cspn_propagate_transposed: the plane / sparse pointers (and the
        # plan) that keep the loop off the vector kernel must make the vector-only entry refuse (only the addresses are looked at)
        plane = d0 if "b" in mis else g_T
        sweep_sp = sp if (case.route == "scalar" or "s" in mis) else None
        ok = L.cspn_propagate_transposed(P(w), F._dt(w), P(plane), P(sweep_sp), P(ghist), B, H, W, 0, K, T, int(sweep_sp is not None),
                                         F._plan_ptr(K, plan), st)
        assert ok == 0 and "16-byte aligned" in last_error(), last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_generic_case(case, monkeypatch):
    ref = gc.reference(case)
    vec = vector_run(case)
    calls = count_calls(monkeypatch)
    plan = SCALAR if case.route == "scalar" else None
    r = run(case, plan, case.mis, case.k)
    a, b, out = r["a"], r["b"], r["out"]
    ga, gb = a.grad, b.grad
    figures = dict(case=case.name, calls=dict(calls))
    # shapes, dtypes, exact zeros, autograd forward == no-grad forward
    half_out = case.dtype == "f16" and (case.module == "new" or case.state is None)
    assert out.dtype == (torch.float16 if half_out else torch.float32) and tuple(out.shape) == tuple(b.shape)
    assert ga.shape == a.shape and ga.dtype == a.dtype and gb.shape == b.shape and gb.dtype == b.dtype
    if case.module == "new" and case.C > 8:
        assert torch.count_nonzero(ga[:, 8:]) == 0
    assert torch.equal(out, r["out_nograd"])
    o, na, nb = np32(out), np32(ga), np32(gb)
    if case.dtype == "f32":
        figures["fwd"] = rel_err(o, ref["out"])
        figures["bit_equal_to_quad"] = bool(torch.equal(out, vec["out"]))
        (figures["ga"], figures["ga_ring"]), (figures["gb"], figures["gb_ring"]) = gc.max_err(na, ref["grad_a"]), gc.max_err(nb, ref["grad_b"])
        print("GENERIC", figures)
        assert figures["fwd"] <= gc.REL_TOL
        if case.module == "new":
            assert figures["bit_equal_to_quad"]
        bar_a, bar_b = gc.BAR_F32[case.module]
        assert figures["ga"] <= bar_a and figures["ga_ring"] <= bar_a
        assert figures["gb"] <= bar_b and figures["gb_ring"] <= bar_b
        if case.route == "view":
            assert torch.allclose(ga, vec["ga"], rtol=1e-5, atol=1e-6 * float(vec["ga"].abs().max()))
            assert torch.allclose(gb, vec["gb"], rtol=1e-5, atol=1e-6 * float(vec["gb"].abs().max()))
    else:
        figures.update(fwd=gc.floored_err(o, ref["out"]), ga=gc.floored_err(na, ref["grad_a"]), gb=gc.floored_err(nb, ref["grad_b"]),
                       vec_fwd=gc.floored_err(np32(vec["out"]), ref["out"]), vec_ga=gc.floored_err(np32(vec["ga"]), ref["grad_a"]),
                       vec_gb=gc.floored_err(np32(vec["gb"]), ref["grad_b"]),
                       generic_vs_vec=[gc.floored_err(o, np32(vec["out"])), gc.floored_err(na, np32(vec["ga"])), gc.floored_err(nb, np32(vec["gb"]))])
        print("GENERIC", figures)
        assert figures["fwd"] <= gc.BAR_F16_FWD[case.module]
        assert figures["ga"] <= gc.BAR_F16_GRAD[0] and figures["gb"] <= gc.BAR_F16_GRAD[1]
    check_route(case, r, plan, calls)


# ------------------------------------------------------------------------------------------------ ABI level: a kernel in isolation
ABI_SHAPES = {3: (2, 12, 16, 5), 5: (2, 6, 8, 3), 7: (2, 6, 8, 3)}      # K -> B, H, W, T
_HIST = {}


def histories(K, half, sparse, c_oracle):
    """Tap volume, forward history and reverse sweep of one problem, produced once by the vector path."""
    key = (K, half, sparse)
    if key not in _HIST:
        B, H, W, T = ABI_SHAPES[K]
        seed = 8301 + 8 * K + 2 * int(half) + int(sparse)
        d = c_oracle.hash_uniform(seed, 2, (B, H, W), 0.0, 10.0)
        sp = put(c_oracle.hash_sparse(seed, 3, d, gc.SPARSE_DENSITY), half) if sparse else None
        d0 = put(d, half)
        cot = put(c_oracle.hash_normal(seed, 9, (B, 1, H, W)))
        S = None
        if K == 3:
            w, S, _ = F.cspn3_prepare(put(c_oracle.hash_normal(seed, 1, (B, 8, H, W)), half), want_s=True)
        else:
            w, _ = F.pac_prepare(put(c_oracle.hash_normal(seed, 1, (B, K * K - 1, H, W)), half))
        _, hist = F.propagate(w, d0, sp, K, T, F.BLEND_SPARSE if sparse else F.BLEND_NONE, keep_history=True)
        g_T, ghist = F._reverse_sweep(w, K, T, sp, cot, None)
        torch.cuda.synchronize()
        _HIST[key] = dict(w=w, S=S, d0=d0, sp=sp, hist=hist, g_T=g_T.contiguous(), ghist=ghist)
    return _HIST[key]


@pytest.mark.parametrize("sparse", [False, True], ids=["nosp", "sp"])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("K", [3, 5, 7])
def test_abi_grad_weights_generic_equals_vector(K, half, sparse, c_oracle):
    """cspn_grad_weights with aligned outputs (the fused tail without epilogue) against outputs one element in
    (cspn_grad_weights_kernel): every element written, nothing beyond, same values."""
    B, H, W, T = ABI_SHAPES[K]
    h = histories(K, half, sparse, c_oracle)
    L, P, st = F._lib.lib(), F._p, F._stream(torch.device(DEV))
    nw, nd = B * (K * K - 1) * H * W, B * H * W
    res = []
    for off in (0, 1):
        bw, bd = torch.full((nw + 8,), NAN, device=DEV), torch.full((nd + 8,), NAN, device=DEV)
        gw, gd0 = bw[4 + off:4 + off + nw], bd[4 + off:4 + off + nd]
        assert (gw.data_ptr() % 16 == 0) == (off == 0) and (gd0.data_ptr() % 16 == 0) == (off == 0)
        ok = L.cspn_grad_weights(P(h["d0"]), P(h["hist"]), P(h["g_T"]), P(h["ghist"]), P(h["sp"]), P(gw), P(gd0), F._dt(h["d0"]),
                                 B, H, W, K, T, st)
        assert ok, last_error()
        torch.cuda.synchronize()
        for buf, n in ((bw, nw), (bd, nd)):
            assert torch.isnan(buf[:4 + off]).all() and torch.isnan(buf[4 + off + n:]).all()      # the guards either side
            assert not torch.isnan(buf[4 + off:4 + off + n]).any()                                  # every element written
        res.append((gw.clone(), gd0.clone()))
    (vw, vd), (sw, sd) = res
    print("GENERIC", dict(abi="grad_weights", K=K, half=half, sparse=sparse, gw=float((sw - vw).abs().max() / vw.abs().max()),
                          gd0=float((sd - vd).abs().max() / vd.abs().max())))
    assert torch.allclose(sw, vw, rtol=1e-5, atol=1e-6 * float(vw.abs().max()))
    assert torch.allclose(sd, vd, rtol=1e-5, atol=1e-6 * float(vd.abs().max()))


@pytest.mark.parametrize("sparse", [False, True], ids=["nosp", "sp"])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("K", [3, 5, 7])
def test_abi_reverse_sweep_copy_equals_gather(K, half, sparse, c_oracle):
    """cspn_transpose_weights + cspn_propagate (BLEND_PREMASK | BLEND_NONE on cspn_prop_scalar) against
    cspn_propagate_transposed on the same volume and cotangent: every G_t plane."""
    B, H, W, T = ABI_SHAPES[K]
    h = histories(K, half, sparse, c_oracle)
    L, P, st = F._lib.lib(), F._p, F._stream(torch.device(DEV))
    w, g_T = h["w"], h["g_T"]
    sp32 = None if h["sp"] is None else h["sp"].float()
    wT = F.transpose_weights(w, K, H, W)
    by_copy = torch.full((T, B, H, W), NAN, device=DEV)
    by_gather = torch.full((T, B, H, W), NAN, device=DEV)
    ok = L.cspn_propagate(P(wT), F._dt(wT), P(g_T), P(sp32), None, P(by_copy), None, F.CSPN_F32, B, H, W, 0, K, T,
                          F.BLEND_PREMASK if sparse else F.BLEND_NONE, F._plan_ptr(K, SCALAR), st)
    assert ok, last_error()
    ok = L.cspn_propagate_transposed(P(w), F._dt(w), P(g_T), P(sp32), P(by_gather), B, H, W, 0, K, T, int(sparse), None, st)
    assert ok, last_error()
    torch.cuda.synchronize()
    errs = [rel_err(by_copy[t].cpu().numpy(), by_gather[t].cpu().numpy()) for t in range(T)]
    print("GENERIC", dict(abi="reverse_sweep", K=K, half=half, sparse=sparse, rel_err=max(errs), bit_equal=bool(torch.equal(by_copy, by_gather))))
    assert max(errs) <= gc.REL_TOL
    assert rel_err(by_copy.cpu().numpy(), h["ghist"].cpu().numpy()) <= gc.REL_TOL      # and the sweep the module itself took


@pytest.mark.parametrize("sparse", [False, True], ids=["nosp", "sp"])
def test_reverse_sweep_env_copy_equals_default(sparse, monkeypatch, c_oracle):
    """K = 3 through functional._reverse_sweep: CSPN_REVERSE_SWEEP=copy (read per call) against the default gather."""
    B, H, W, T = ABI_SHAPES[3]
    h = histories(3, False, sparse, c_oracle)
    monkeypatch.setattr(F, "_RESIDENT_MODE", "off")          # the weight-resident sweep does not consult the switch
    calls = count_calls(monkeypatch)
    cot = h["g_T"].view(B, 1, H, W)
    _, default = F._reverse_sweep(h["w"], 3, T, h["sp"], cot, None)
    assert calls["tr"] == 0
    monkeypatch.setenv("CSPN_REVERSE_SWEEP", "copy")
    _, by_copy = F._reverse_sweep(h["w"], 3, T, h["sp"], cot, None)
    assert calls["tr"] == 1
    torch.cuda.synchronize()
    assert rel_err(by_copy.cpu().numpy(), default.cpu().numpy()) <= gc.REL_TOL


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_abi_grad_guidance_reads_and_writes_through_strides(half, c_oracle):
    """cspn3_grad_guidance on a 12-channel guidance that is the [:, 1:13] slice of a 13-channel tensor (aligned, batch-strided)
    against the same call on a contiguous copy: same bits, channels 8..11 exactly zero, the channel outside the slice untouched."""
    B, H, W = 2, 12, 16
    L, P, st = F._lib.lib(), F._p, F._stream(torch.device(DEV))
    g13 = put(c_oracle.hash_normal(8401, 1, (B, 13, H, W)), half)
    g, gcopy = g13[:, 1:13], g13[:, 1:13].contiguous()
    assert not g.is_contiguous() and g.data_ptr() % 16 == 0 and g.stride(0) == 13 * H * W
    w8, S, _ = F.cspn3_prepare(g, want_s=True)
    gw = put(c_oracle.hash_normal(8402, 2, (B, 8, H, W)))
    out13 = torch.full_like(g13, 77.0)
    out, want = out13[:, 1:13], torch.full_like(gcopy, NAN)
    dt = F._dt(g13)
    assert L.cspn3_grad_guidance(P(g), dt, g.stride(0), g.stride(1), 12, P(w8), dt, P(S), P(gw), P(out), B, H, W, st), last_error()
    assert L.cspn3_grad_guidance(P(gcopy), dt, gcopy.stride(0), gcopy.stride(1), 12, P(w8), dt, P(S), P(gw), P(want), B, H, W, st), last_error()
    torch.cuda.synchronize()
    assert not torch.isnan(want).any() and torch.equal(out, want)
    assert torch.count_nonzero(out[:, 8:]) == 0 and torch.count_nonzero(out[:, :8]) > 0
    assert bool((out13[:, 0] == 77.0).all())


# ------------------------------------------------------------------------------------------------ views through autograd
def view_module(vc):
    return pkg.CSPN_new.AffinityPropagate(vc.T, 3) if vc.module == "new" else pkg.CSPN_ours.AffinityPropagate(vc.T)


@pytest.mark.parametrize("vc", gc.VIEW_CASES, ids=lambda v: v.name)
def test_views_through_autograd(vc):
    z = gc.view_inputs(vc)
    B, H, W = vc.shape
    m, s = view_module(vc), put(z["s"])
    assert float(np.abs(z["grad_a"]).max()) >= gc.MIN_GRAD_SCALE and float(np.abs(z["grad_b"]).max()) >= gc.MIN_GRAD_SCALE

    def fwd(a, b):
        return m(a, b, s) if vc.module == "new" else m(b, a, sparse_depth=s)

    cot = put(z["cot"])
    if vc.kind == "head":
        head = put(np.concatenate([z["b"], z["a"]], axis=1), grad=True)          # one leaf: depth | x first, guidance | guided behind
        a, b = head[:, 1:], head[:, :1]
        assert not a.is_contiguous()
        fwd(a, b).backward(cot)
        assert head.grad.shape == head.shape
        ga, gb = head.grad[:, 1:], head.grad[:, :1]
    elif vc.kind == "batch":
        def big(x):
            pad = np.zeros((1,) + x.shape[1:], np.float32)
            return put(np.concatenate([pad + 3.0, x, pad + 5.0], axis=0), grad=True)
        biga, bigb = big(z["a"]), big(z["b"])
        fwd(biga[1:B + 1], bigb[1:B + 1]).backward(cot)
        for t in (biga, bigb):
            assert torch.count_nonzero(t.grad[0]) == 0 and torch.count_nonzero(t.grad[B + 1]) == 0      # the other rows: exactly zero
        ga, gb = biga.grad[1:B + 1], bigb.grad[1:B + 1]
    else:
        a, b = put(z["a"], grad=True), put(z["b"], grad=True)
        out = fwd(a, b)
        if vc.kind == "expanded":
            out.sum().backward()
        elif vc.kind == "transposed":
            out.transpose(2, 3).backward(cot.transpose(2, 3).contiguous())
        else:
            out.half().backward(cot.half())
        ga, gb = a.grad, b.grad
    torch.cuda.synchronize()
    (ea, ea_ring), (eb, eb_ring) = gc.max_err(np32(ga), z["grad_a"]), gc.max_err(np32(gb), z["grad_b"])
    print("GENERIC", dict(view=vc.name, ga=ea, ga_ring=ea_ring, gb=eb, gb_ring=eb_ring))
    bar_a, bar_b = gc.BAR_F32[vc.module]
    assert ea <= bar_a and ea_ring <= bar_a and eb <= bar_b and eb_ring <= bar_b
    if vc.module == "new":
        assert torch.count_nonzero(ga[:, 8:]) == 0

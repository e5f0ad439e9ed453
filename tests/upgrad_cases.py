"""The gradients of the fused decoder-block head (the arithmetic of include/cspn_upconv.h, differentiated) restated in numpy, and what
tests/test_upgrad.py and tests/golden/make_golden_g28.py share.  The shape lists and make_inputs are those of tests/upconv_cases.py.

The formulas are written on the COMPACT map — not through the un-pooled map the stock path builds.  With acc[n, q, Y, X] the raw
fused convolution over the flat output channels q of the one or two filters, gy its cotangent (one [N, O_k, oh, ow] array per
filter), Hc = ceil(oh / 2) and Wc = ceil(ow / 2):

    gx[n, c, i, j]   = sum_{ky, kx} sum_q w[q, c, ky, kx] gy[n, q, 2i + 2 - ky, 2j + 2 - kx]      i < Hc, j < Wc;  0 for the other pixels
    gw[q, c, ky, kx] = sum_{n, i < Hc, j < Wc} x[n, c, i, j] gy[n, q, 2i + 2 - ky, 2j + 2 - kx]

where a term whose gy index falls outside [0, oh) x [0, ow) is absent — 25 products per compact pixel, channel and output channel
each, where the un-pooled map costs 100.  A cotangent that is None counts as zero: its filter's channels leave gx, and its gw is zeros.

No kernel computes these yet ("Not built"); golden G28 and this restatement are the yardsticks one will be held to.

Every function keeps the dtype it is given (fp64 for the references; integer-valued inputs are exact in any float type).
"""
import numpy as np


def _axis(k, n_out, n_compact):
    """One axis of tap k: the compact positions i < n_compact whose gy index 2i + 2 - k lies in [0, n_out), and those indices."""
    i = np.arange(n_compact)
    y = 2 * i + 2 - k
    ok = (y >= 0) & (y < n_out)
    return i[ok], y[ok]


def make_cotangents(seed, shape, filters, out_hw, integer):
    """One fp32 cotangent per filter, drawn as make_inputs draws x; a fixed function of its arguments."""
    rng = np.random.RandomState(seed + 77)
    sizes = [(shape[0], o) + tuple(out_hw) for o in filters]
    if integer:
        return [rng.randint(-3, 4, size=s).astype(np.float32) for s in sizes]
    return [rng.standard_normal(s).astype(np.float32) for s in sizes]


def grad_input(ws, gys, hw, out_hw):
    """gx [N, C, H, W] from the filters and the cotangents (None: absent)."""
    live = [k for k, g in enumerate(gys) if g is not None]
    N, C = gys[live[0]].shape[0], ws[0].shape[1]
    dtype = gys[live[0]].dtype
    w = np.concatenate([ws[k] for k in live], 0).astype(dtype)
    gy = np.concatenate([gys[k] for k in live], 1)
    (H, W), (oh, ow) = hw, out_hw
    Hc, Wc = (oh + 1) // 2, (ow + 1) // 2
    gx = np.zeros((N, C, H, W), dtype)
    for ky in range(5):
        ii, yy = _axis(ky, oh, Hc)
        for kx in range(5):
            jj, xx = _axis(kx, ow, Wc)
            if ii.size and jj.size:
                gx[np.ix_(range(N), range(C), ii, jj)] += np.einsum("qc,nqij->ncij", w[:, :, ky, kx], gy[np.ix_(range(N), range(w.shape[0]), yy, xx)])
    return gx


def grad_weights(x, gys, filters, out_hw):
    """One gw [O_k, C, 5, 5] per filter from x and the cotangents (None: absent, zeros)."""
    N, C = x.shape[:2]
    oh, ow = out_hw
    Hc, Wc = (oh + 1) // 2, (ow + 1) // 2
    out = []
    for o, gy in zip(filters, gys):
        gw = np.zeros((o, C, 5, 5), x.dtype)
        if gy is not None:
            for ky in range(5):
                ii, yy = _axis(ky, oh, Hc)
                for kx in range(5):
                    jj, xx = _axis(kx, ow, Wc)
                    if ii.size and jj.size:
                        gw[:, :, ky, kx] = np.einsum("ncij,nqij->qc", x[np.ix_(range(N), range(C), ii, jj)], gy.astype(x.dtype)[np.ix_(range(N), range(o), yy, xx)])
        out.append(gw)
    return out


def restate(x, ws, gys, out_hw, dtype=np.float64):
    """(gx, [gw_k]) in `dtype`."""
    x, ws = x.astype(dtype), [w.astype(dtype) for w in ws]
    gys = [None if g is None else g.astype(dtype) for g in gys]
    return grad_input(ws, gys, x.shape[2:], out_hw), grad_weights(x, gys, [w.shape[0] for w in ws], out_hw)


def dense(x, ws, gys, out_hw):
    """The same through the dense form on the CPU in fp64: zero-insert, crop, F.conv2d(padding=2), torch.autograd."""
    import torch
    oh, ow = out_hw
    xt = torch.from_numpy(x).double().requires_grad_(True)
    wt = [torch.from_numpy(w).double().requires_grad_(True) for w in ws]
    u = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=torch.float64)
    u[:, :, ::2, ::2] = xt
    u = u[:, :, :oh, :ow]
    loss = sum((torch.nn.functional.conv2d(u, w, padding=2) * torch.from_numpy(g).double()).sum() for w, g in zip(wt, gys) if g is not None)
    grads = torch.autograd.grad(loss, [xt] + wt, allow_unused=True)
    return grads[0].numpy(), [np.zeros(w.shape) if g is None else g.numpy() for w, g in zip(ws, grads[1:])]

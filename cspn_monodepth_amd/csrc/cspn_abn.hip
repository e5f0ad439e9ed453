// cspn_abn.hip — In-Place Activated BatchNorm (the reference's network/libs/inplace_abn/src/bn.cu:125-232, :302-377), forward
// and backward, for wave64 and a 256-CU part (include/cspn_abn.h).  What differs from a port of the CUDA:
//   * reductions are over 64 lanes (shuffle / DPP), then over the wavefronts of a workgroup through LDS, then — SPLIT regime —
//     over the workgroups of a channel by a finalise launch in a fixed order: no atomics, equal bits run after run;
//   * the statistics read x once: (count, mean, M2) triples merged with Chan's formula at every level;
//   * the activation, its gradient and its inverse are part of the apply / gradient passes, not whole-tensor passes of their own;
//   * a channel is not one workgroup: tiny channels share a workgroup and keep their elements in LDS between the statistics and
//     the apply (one launch, one read), big ones are cut into ranges that fill the part.
// ONE traversal (abn_for_range) serves every kernel: a range [e0, e1) of a channel's (n, s) index space is visited plane by
// plane, each plane's piece as a scalar head up to the next 16-byte boundary, 16-byte units, and a scalar tail.
#include "cspn_common.hpp"
#include "cspn_abn.h"

namespace {

constexpr int ABN_THREADS = 256;                 // 4 wavefronts
constexpr size_t ABN_SMALL_LIMIT = 4096;         // elements of one channel the SMALL regime keeps in LDS (16 KB forward, 32 KB backward)
constexpr size_t ABN_SHARED_LIMIT = 1024;        // up to here four channels share a workgroup, one wavefront each
constexpr int ABN_FLAT_BELOW = 32;               // planes shorter than this are visited element by element
constexpr size_t ABN_MIN_RANGE = 2048;           // SPLIT: a range is at least this long ...
constexpr size_t ABN_MAX_RANGE = (size_t)1 << 22;   // ... and at most this long (a thread's fp32 count stays exact)
constexpr size_t ABN_TARGET_WORKGROUPS = 1024;   // SPLIT: four workgroups per CU

struct AbnShape {
    int N, C, S;
    size_t NS;            // N * S
    size_t L;             // elements of a range
    int W;                // ranges per channel
    int vec;              // every tensor's base has the same 16-byte phase: 16-byte units may be used
    unsigned phase;       // (base address / 4) % 4
};

// ------------------------------------------------------------------------------------------------ traversal
// Elements [e0, e1) of channel c's index space e = n * S + s, shared among `nthr` threads (this one is `tid`).
// one(g, l) / four(g, l): g = offset of the element (of the first of 4) in the tensor, l = e - e0.  four() is only called with
// (base + g) 16-byte aligned and all four elements inside one plane.
template <class F1, class F4>
__device__ __forceinline__ void abn_for_range(const AbnShape& sh, int c, size_t e0, size_t e1, int tid, int nthr, F1&& one, F4&& four) {
    if (e0 >= e1) return;
    const size_t S = (size_t)sh.S;
    if (!sh.vec || sh.S < ABN_FLAT_BELOW) {
        for (size_t e = e0 + tid; e < e1; e += nthr) {
            const size_t n = e / S, s = e - n * S;
            one((n * sh.C + c) * S + s, (unsigned)(e - e0));
        }
        return;
    }
    const size_t n0 = e0 / S, n1 = (e1 - 1) / S;
    for (size_t n = n0; n <= n1; ++n) {
        const size_t pe = n * S;
        const size_t lo = e0 > pe ? e0 : pe, hi = e1 < pe + S ? e1 : pe + S;
        const size_t g0 = (n * sh.C + c) * S + (lo - pe);
        const unsigned l0 = (unsigned)(lo - e0);
        const size_t len = hi - lo;
        size_t head = (4 - ((g0 + sh.phase) & 3)) & 3;
        if (head > len) head = len;
        const size_t nvec = (len - head) >> 2;
        const size_t done = head + 4 * nvec, tail = len - done;
        if ((size_t)tid < head) one(g0 + tid, l0 + (unsigned)tid);
        for (size_t u = tid; u < nvec; u += nthr) four(g0 + head + 4 * u, l0 + (unsigned)(head + 4 * u));
        if ((size_t)tid < tail) one(g0 + done + tid, l0 + (unsigned)(done + tid));
    }
}

// ------------------------------------------------------------------------------------------------ (count, mean, M2)
struct Moments { float n, mean, m2; };

__device__ __forceinline__ void moments_add(Moments& a, float x) {
    a.n += 1.f;
    const float d = x - a.mean;
    a.mean += d / a.n;
    a.m2 = fmaf(d, x - a.mean, a.m2);
}
// a unit of 4: its own mean and M2 first, then one Chan merge
__device__ __forceinline__ void moments_add(Moments& a, const float4& v) {
    const float um = ((v.x + v.y) + (v.z + v.w)) * 0.25f;
    const float d0 = v.x - um, d1 = v.y - um, d2 = v.z - um, d3 = v.w - um;
    const float um2 = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    const float nn = a.n + 4.f, delta = um - a.mean, r = 4.f / nn;
    a.mean = fmaf(delta, r, a.mean);
    a.m2 += um2 + delta * delta * a.n * r;
    a.n = nn;
}
__device__ __forceinline__ Moments moments_merge(const Moments& a, const Moments& b) {
    const float nn = a.n + b.n;
    if (!(nn > 0.f)) return a;
    const float delta = b.mean - a.mean, r = b.n / nn;
    Moments o;
    o.n = nn;
    o.mean = fmaf(delta, r, a.mean);
    o.m2 = a.m2 + b.m2 + delta * delta * a.n * r;
    return o;
}

// The merge of a group of G threads (G = 64: one wavefront; G = 256: the workgroup, `red` = 4 slots of LDS), in every thread.
template <int G>
__device__ __forceinline__ Moments moments_group(Moments a, Moments* red) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Moments b;
        b.n = __shfl_down(a.n, off, 64);
        b.mean = __shfl_down(a.mean, off, 64);
        b.m2 = __shfl_down(a.m2, off, 64);
        a = moments_merge(a, b);            // only lane 0's chain is used: it merged lanes 0..63 in a fixed tree
    }
    if (G == 64) {
        a.n = __shfl(a.n, 0, 64);
        a.mean = __shfl(a.mean, 0, 64);
        a.m2 = __shfl(a.m2, 0, 64);
        return a;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    Moments t = red[0];
#pragma unroll
    for (int w = 1; w < ABN_THREADS / 64; ++w) t = moments_merge(t, red[w]);
    return t;
}

// the sums of two values over a group, in every thread
template <int G>
__device__ __forceinline__ void sum2_group(float& a, float& b, float (*red)[2]) {
    a = wave_sum_to_lane63(a);
    b = wave_sum_to_lane63(b);
    if (G == 64) {
        a = __shfl(a, 63, 64);
        b = __shfl(b, 63, 64);
        return;
    }
    if ((threadIdx.x & 63) == 63) {
        red[threadIdx.x >> 6][0] = a;
        red[threadIdx.x >> 6][1] = b;
    }
    __syncthreads();
    a = red[0][0];
    b = red[0][1];
#pragma unroll
    for (int w = 1; w < ABN_THREADS / 64; ++w) {
        a += red[w][0];
        b += red[w][1];
    }
}

// ------------------------------------------------------------------------------------------------ per-element arithmetic
__device__ __forceinline__ float abn_act(float z, int act, float slope) {
    if (act == CSPN_ABN_ACT_LEAKY_RELU) return z < 0.f ? z * slope : z;
    if (act == CSPN_ABN_ACT_ELU) return z < 0.f ? expm1f(z) : z;
    return z;
}
// the activation undone: z -> pre-activation, dz -> gradient at the pre-activation
__device__ __forceinline__ void abn_act_inverse(float& z, float& dz, int act, float slope, float inv_slope) {
    if (act == CSPN_ABN_ACT_LEAKY_RELU) {
        if (z < 0.f) { dz *= slope; z *= inv_slope; }
    } else if (act == CSPN_ABN_ACT_ELU) {
        if (z < 0.f) { dz *= z + 1.f; z = log1pf(z); }
    }
}
__device__ __forceinline__ float abn_invstd(float var, float eps) { return (var != 0.f || eps != 0.f) ? 1.f / sqrtf(var + eps) : 0.f; }

struct AbnChannel { float mean, invstd, gamma, beta; };
__device__ __forceinline__ AbnChannel abn_channel(const float* weight, const float* bias, int c, float mean, float var, float eps) {
    AbnChannel ch;
    ch.mean = mean;
    ch.invstd = abn_invstd(var, eps);
    ch.gamma = weight ? fabsf(weight[c]) + eps : 1.f;
    ch.beta = bias ? bias[c] : 0.f;
    return ch;
}
__device__ __forceinline__ float abn_forward_one(float x, const AbnChannel& ch, int act, float slope) {
    const float y = (x - ch.mean) * ch.invstd;
    return abn_act(y * ch.gamma + ch.beta, act, slope);
}
__device__ __forceinline__ float4 abn_forward_four(const float4& v, const AbnChannel& ch, int act, float slope) {
    return make_float4(abn_forward_one(v.x, ch, act, slope), abn_forward_one(v.y, ch, act, slope),
                       abn_forward_one(v.z, ch, act, slope), abn_forward_one(v.w, ch, act, slope));
}

__device__ __forceinline__ void abn_update_running(float* running_mean, float* running_var, int c, float mean, float var, size_t NS,
                                                   float momentum) {
    if (!running_mean || !running_var) return;
    const float keep = (float)(1.0 - (double)momentum), n = (float)NS;
    running_mean[c] = running_mean[c] * keep + momentum * mean;
    running_var[c] = running_var[c] * keep + momentum * var * n / (n - 1.f);
}

// ------------------------------------------------------------------------------------------------ forward kernels
struct AbnForwardArgs {
    AbnShape sh;
    float* x;
    const float *weight, *bias;
    float *running_mean, *running_var;      // updated by the statistics when non-null
    float *mean, *var;                      // written by the statistics, read by the apply
    float* partial;                         // SPLIT: [C][W][4]
    float momentum, eps, slope;
    int act;
};

// SMALL: G threads per channel, 256 / G channels per workgroup.  APPLY: keep the elements in LDS and write z.
template <int G, bool APPLY>
__global__ __launch_bounds__(ABN_THREADS) void abn_small_forward_kernel(AbnForwardArgs a) {
    constexpr int CPW = ABN_THREADS / G;
    __shared__ float buf[APPLY ? ABN_SMALL_LIMIT : 1];
    __shared__ Moments red[ABN_THREADS / 64];
    const int sub = threadIdx.x / G, tid = threadIdx.x % G;
    const int c = blockIdx.x * CPW + sub;
    const bool active = c < a.sh.C;
    float* slice = buf + (APPLY ? sub * (ABN_SMALL_LIMIT / CPW) : 0);
    Moments acc = {0.f, 0.f, 0.f};
    if (active)
        abn_for_range(a.sh, c, 0, a.sh.NS, tid, G,
                      [&](size_t g, unsigned l) {
                          const float v = ld1(a.x + g);
                          if (APPLY) slice[l] = v;
                          moments_add(acc, v);
                      },
                      [&](size_t g, unsigned l) {
                          const float4 v = ld4(a.x + g);
                          if (APPLY) { slice[l] = v.x; slice[l + 1] = v.y; slice[l + 2] = v.z; slice[l + 3] = v.w; }
                          moments_add(acc, v);
                      });
    const Moments tot = moments_group<G>(acc, red);
    if (!active) return;                     // after the group's only barrier
    const float mean = tot.mean, var = tot.m2 / tot.n;
    if (tid == 0) {
        a.mean[c] = mean;
        a.var[c] = var;
        if (APPLY) abn_update_running(a.running_mean, a.running_var, c, mean, var, a.sh.NS, a.momentum);
    }
    if (APPLY) {
        const AbnChannel ch = abn_channel(a.weight, a.bias, c, mean, var, a.eps);
        // the same thread visits the same elements as above: what it reads from LDS it wrote itself
        abn_for_range(a.sh, c, 0, a.sh.NS, tid, G,
                      [&](size_t g, unsigned l) { st1(a.x + g, abn_forward_one(slice[l], ch, a.act, a.slope)); },
                      [&](size_t g, unsigned l) {
                          const float4 v = make_float4(slice[l], slice[l + 1], slice[l + 2], slice[l + 3]);
                          st4(a.x + g, abn_forward_four(v, ch, a.act, a.slope));
                      });
    }
}

// SPLIT, first launch: workgroup (c, w) -> partial[c][w] = (count, mean, M2) of its range
__global__ __launch_bounds__(ABN_THREADS) void abn_partial_stats_kernel(AbnForwardArgs a) {
    __shared__ Moments red[ABN_THREADS / 64];
    const int c = blockIdx.x / a.sh.W, w = blockIdx.x % a.sh.W;
    const size_t e0 = (size_t)w * a.sh.L, e1 = e0 + a.sh.L < a.sh.NS ? e0 + a.sh.L : a.sh.NS;
    Moments acc = {0.f, 0.f, 0.f};
    abn_for_range(a.sh, c, e0, e1, threadIdx.x, ABN_THREADS,
                  [&](size_t g, unsigned) { moments_add(acc, ld1(a.x + g)); },
                  [&](size_t g, unsigned) { moments_add(acc, ld4(a.x + g)); });
    const Moments tot = moments_group<ABN_THREADS>(acc, red);
    if (threadIdx.x == 0) st4(a.partial + (size_t)blockIdx.x * 4, make_float4(tot.n, tot.mean, tot.m2, 0.f));
}

// SPLIT, second launch: one thread per channel merges its W partials in increasing w, in fp64
__global__ __launch_bounds__(64) void abn_finalise_stats_kernel(AbnForwardArgs a, int update_running) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.sh.C) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int w = 0; w < a.sh.W; ++w) {
        const float4 p = ld4(a.partial + ((size_t)c * a.sh.W + w) * 4);
        const double nb = p.x, nn = n + nb;
        if (!(nn > 0.0)) continue;
        const double delta = (double)p.y - mean, r = nb / nn;
        mean += delta * r;
        m2 += (double)p.z + delta * delta * n * r;
        n = nn;
    }
    const float fm = (float)mean, fv = (float)(m2 / n);
    a.mean[c] = fm;
    a.var[c] = fv;
    if (update_running) abn_update_running(a.running_mean, a.running_var, c, fm, fv, a.sh.NS, a.momentum);
}

// the apply pass on its own: SPLIT's third launch, an eval-mode forward, the second half of the synchronised forward
__global__ __launch_bounds__(ABN_THREADS) void abn_apply_kernel(AbnForwardArgs a) {
    const int c = blockIdx.x / a.sh.W, w = blockIdx.x % a.sh.W;
    const size_t e0 = (size_t)w * a.sh.L, e1 = e0 + a.sh.L < a.sh.NS ? e0 + a.sh.L : a.sh.NS;
    const AbnChannel ch = abn_channel(a.weight, a.bias, c, a.mean[c], a.var[c], a.eps);
    abn_for_range(a.sh, c, e0, e1, threadIdx.x, ABN_THREADS,
                  [&](size_t g, unsigned) { st1(a.x + g, abn_forward_one(ld1(a.x + g), ch, a.act, a.slope)); },
                  [&](size_t g, unsigned) { st4(a.x + g, abn_forward_four(ld4(a.x + g), ch, a.act, a.slope)); });
}

// ------------------------------------------------------------------------------------------------ backward kernels
struct AbnBackwardArgs {
    AbnShape sh;
    const float *z, *dz;
    const float *var, *weight, *bias;
    const float *edz_in, *eydz_in;          // dx kernel: null = 0
    float *edz_out, *eydz_out;              // written by the reductions (may be null in the fused SMALL launch)
    float *dx, *dweight, *dbias;
    float* partial;                         // SPLIT: [C][W][4]
    float eps, slope, inv_slope;
    int act;
};

// (y, dz') of one element
__device__ __forceinline__ void abn_undo(float z, float dz, float gamma, float beta, int act, float slope, float inv_slope, float& y,
                                         float& g) {
    abn_act_inverse(z, dz, act, slope, inv_slope);
    y = (z - beta) / gamma;
    g = dz;
}
__device__ __forceinline__ float abn_dx_one(float y, float g, float edz, float eydz, float mul) { return (g - edz - y * eydz) * mul; }

__device__ __forceinline__ void abn_write_param_grads(const AbnBackwardArgs& a, int c, float edz, float eydz) {
    const float norm = (float)a.sh.NS;
    if (a.dweight) {
        const float w = a.weight[c];
        a.dweight[c] = w > 0.f ? eydz * norm : (w < 0.f ? -(eydz * norm) : 0.f);
    }
    if (a.dbias) a.dbias[c] = edz * norm;
}

// SMALL: reduce (and, DX, the gradient) in one launch; (y, dz') wait in LDS between the two
template <int G, bool DX>
__global__ __launch_bounds__(ABN_THREADS) void abn_small_backward_kernel(AbnBackwardArgs a) {
    constexpr int CPW = ABN_THREADS / G;
    __shared__ float ybuf[DX ? ABN_SMALL_LIMIT : 1];
    __shared__ float gbuf[DX ? ABN_SMALL_LIMIT : 1];
    __shared__ float red[ABN_THREADS / 64][2];
    const int sub = threadIdx.x / G, tid = threadIdx.x % G;
    const int c = blockIdx.x * CPW + sub;
    const bool active = c < a.sh.C;
    float* ys = ybuf + (DX ? sub * (ABN_SMALL_LIMIT / CPW) : 0);
    float* gs = gbuf + (DX ? sub * (ABN_SMALL_LIMIT / CPW) : 0);
    const float gamma = active && a.weight ? fabsf(a.weight[c]) + a.eps : 1.f;
    const float beta = active && a.bias ? a.bias[c] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    if (active)
        abn_for_range(a.sh, c, 0, a.sh.NS, tid, G,
                      [&](size_t o, unsigned l) {
                          float y, g;
                          abn_undo(ld1(a.z + o), ld1(a.dz + o), gamma, beta, a.act, a.slope, a.inv_slope, y, g);
                          if (DX) { ys[l] = y; gs[l] = g; }
                          s1 += g;
                          s2 = fmaf(y, g, s2);
                      },
                      [&](size_t o, unsigned l) {
                          const float4 zz = ld4(a.z + o), dd = ld4(a.dz + o);
                          const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, dv[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
                          for (int k = 0; k < 4; ++k) {
                              float y, g;
                              abn_undo(zv[k], dv[k], gamma, beta, a.act, a.slope, a.inv_slope, y, g);
                              if (DX) { ys[l + k] = y; gs[l + k] = g; }
                              s1 += g;
                              s2 = fmaf(y, g, s2);
                          }
                      });
    sum2_group<G>(s1, s2, red);
    if (!active) return;
    const float norm = 1.f / (float)a.sh.NS;
    const float edz = s1 * norm, eydz = s2 * norm;
    if (tid == 0) {
        if (a.edz_out) a.edz_out[c] = edz;
        if (a.eydz_out) a.eydz_out[c] = eydz;
        if (DX) abn_write_param_grads(a, c, edz, eydz);
    }
    if (DX) {
        const float mul = gamma * abn_invstd(a.var[c], a.eps);
        abn_for_range(a.sh, c, 0, a.sh.NS, tid, G,
                      [&](size_t o, unsigned l) { st1(a.dx + o, abn_dx_one(ys[l], gs[l], edz, eydz, mul)); },
                      [&](size_t o, unsigned l) {
                          st4(a.dx + o, make_float4(abn_dx_one(ys[l], gs[l], edz, eydz, mul), abn_dx_one(ys[l + 1], gs[l + 1], edz, eydz, mul),
                                                    abn_dx_one(ys[l + 2], gs[l + 2], edz, eydz, mul), abn_dx_one(ys[l + 3], gs[l + 3], edz, eydz, mul)));
                      });
    }
}

// SPLIT, first launch: partial[c][w] = (sum dz', sum y dz') of a range
__global__ __launch_bounds__(ABN_THREADS) void abn_partial_grad_kernel(AbnBackwardArgs a) {
    __shared__ float red[ABN_THREADS / 64][2];
    const int c = blockIdx.x / a.sh.W, w = blockIdx.x % a.sh.W;
    const size_t e0 = (size_t)w * a.sh.L, e1 = e0 + a.sh.L < a.sh.NS ? e0 + a.sh.L : a.sh.NS;
    const float gamma = a.weight ? fabsf(a.weight[c]) + a.eps : 1.f;
    const float beta = a.bias ? a.bias[c] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    abn_for_range(a.sh, c, e0, e1, threadIdx.x, ABN_THREADS,
                  [&](size_t o, unsigned) {
                      float y, g;
                      abn_undo(ld1(a.z + o), ld1(a.dz + o), gamma, beta, a.act, a.slope, a.inv_slope, y, g);
                      s1 += g;
                      s2 = fmaf(y, g, s2);
                  },
                  [&](size_t o, unsigned) {
                      const float4 zz = ld4(a.z + o), dd = ld4(a.dz + o);
                      const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, dv[4] = {dd.x, dd.y, dd.z, dd.w};
                      float u1 = 0.f, u2 = 0.f;
#pragma unroll
                      for (int k = 0; k < 4; ++k) {
                          float y, g;
                          abn_undo(zv[k], dv[k], gamma, beta, a.act, a.slope, a.inv_slope, y, g);
                          u1 += g;
                          u2 = fmaf(y, g, u2);
                      }
                      s1 += u1;
                      s2 += u2;
                  });
    sum2_group<ABN_THREADS>(s1, s2, red);
    if (threadIdx.x == 0) st4(a.partial + (size_t)blockIdx.x * 4, make_float4(s1, s2, 0.f, 0.f));
}

// SPLIT, second launch: one thread per channel adds its W partials in increasing w, in fp64
__global__ __launch_bounds__(64) void abn_finalise_grad_kernel(AbnBackwardArgs a) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= a.sh.C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int w = 0; w < a.sh.W; ++w) {
        const float4 p = ld4(a.partial + ((size_t)c * a.sh.W + w) * 4);
        s1 += (double)p.x;
        s2 += (double)p.y;
    }
    a.edz_out[c] = (float)(s1 / (double)a.sh.NS);
    a.eydz_out[c] = (float)(s2 / (double)a.sh.NS);
}

// the gradient pass on its own; the first workgroup of a channel also writes dweight / dbias
__global__ __launch_bounds__(ABN_THREADS) void abn_dx_kernel(AbnBackwardArgs a) {
    const int c = blockIdx.x / a.sh.W, w = blockIdx.x % a.sh.W;
    const size_t e0 = (size_t)w * a.sh.L, e1 = e0 + a.sh.L < a.sh.NS ? e0 + a.sh.L : a.sh.NS;
    const float gamma = a.weight ? fabsf(a.weight[c]) + a.eps : 1.f;
    const float beta = a.bias ? a.bias[c] : 0.f;
    const float edz = a.edz_in ? a.edz_in[c] : 0.f, eydz = a.eydz_in ? a.eydz_in[c] : 0.f;
    const float mul = gamma * abn_invstd(a.var[c], a.eps);
    if (w == 0 && threadIdx.x == 0) abn_write_param_grads(a, c, edz, eydz);
    abn_for_range(a.sh, c, e0, e1, threadIdx.x, ABN_THREADS,
                  [&](size_t o, unsigned) {
                      float y, g;
                      abn_undo(ld1(a.z + o), ld1(a.dz + o), gamma, beta, a.act, a.slope, a.inv_slope, y, g);
                      st1(a.dx + o, abn_dx_one(y, g, edz, eydz, mul));
                  },
                  [&](size_t o, unsigned) {
                      const float4 zz = ld4(a.z + o), dd = ld4(a.dz + o);
                      const float zv[4] = {zz.x, zz.y, zz.z, zz.w}, dv[4] = {dd.x, dd.y, dd.z, dd.w};
                      float r[4];
#pragma unroll
                      for (int k = 0; k < 4; ++k) {
                          float y, g;
                          abn_undo(zv[k], dv[k], gamma, beta, a.act, a.slope, a.inv_slope, y, g);
                          r[k] = abn_dx_one(y, g, edz, eydz, mul);
                      }
                      st4(a.dx + o, make_float4(r[0], r[1], r[2], r[3]));
                  });
}

// ------------------------------------------------------------------------------------------------ host side
int abn_plan(int N, int C, int S, cspn_abn_plan_t* plan) {
    if (N < 1 || C < 1 || S < 1) return fail("cspn_abn_plan: N, C, S must be at least 1 (got %d, %d, %d)", N, C, S);
    if (!plan) return fail("cspn_abn_plan: null plan");
    const size_t NS = (size_t)N * S;
    plan->threads = ABN_THREADS;
    plan->small_limit = ABN_SMALL_LIMIT;
    if (NS <= ABN_SMALL_LIMIT) {
        plan->regime = CSPN_ABN_SMALL;
        plan->channels_per_workgroup = NS <= ABN_SHARED_LIMIT ? ABN_THREADS / 64 : 1;
        plan->workgroups_per_channel = 1;
        plan->elements_per_workgroup = NS;
        return 1;
    }
    size_t W = (ABN_TARGET_WORKGROUPS + C - 1) / C;
    const size_t wmax = (NS + ABN_MIN_RANGE - 1) / ABN_MIN_RANGE, wmin = (NS + ABN_MAX_RANGE - 1) / ABN_MAX_RANGE;
    if (W > wmax) W = wmax;
    if (W < wmin) W = wmin;
    if (W < 1) W = 1;
    const size_t L = ((NS + W - 1) / W + 3) & ~(size_t)3;
    W = (NS + L - 1) / L;
    if (W * (size_t)C > 0x7fffffffu) return fail("cspn_abn_plan: %zu workgroups are more than a grid holds", W * (size_t)C);
    plan->regime = CSPN_ABN_SPLIT;
    plan->channels_per_workgroup = 1;
    plan->workgroups_per_channel = (int)W;
    plan->elements_per_workgroup = L;
    return 1;
}

inline unsigned phase_of(const void* p) { return (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }

// the shape of a launch (a SMALL shape is one range per channel, also for the stand-alone passes) and the phase of its tensors
int abn_shape(const char* who, int N, int C, int S, std::initializer_list<const void*> tensors, AbnShape* sh, cspn_abn_plan_t* plan) {
    if (!abn_plan(N, C, S, plan)) return 0;
    sh->N = N; sh->C = C; sh->S = S;
    sh->NS = (size_t)N * S;
    sh->L = plan->elements_per_workgroup;
    sh->W = plan->workgroups_per_channel;
    sh->vec = 1;
    sh->phase = 0;
    bool first = true;
    for (const void* p : tensors) {
        if (!p) return fail("%s: null tensor", who);
        if (reinterpret_cast<uintptr_t>(p) & 3) return fail("%s: tensors must be aligned to 4 bytes", who);
        if (first) sh->phase = phase_of(p);
        else if (phase_of(p) != sh->phase) sh->vec = 0;
        first = false;
    }
    return 1;
}

int check_activation(const char* who, int activation) {
    if (activation != CSPN_ABN_ACT_LEAKY_RELU && activation != CSPN_ABN_ACT_ELU && activation != CSPN_ABN_ACT_NONE)
        return fail("%s: unknown activation %d", who, activation);
    return 1;
}

int check_work(const char* who, const cspn_abn_plan_t& plan, const void* work) {
    if (plan.regime == CSPN_ABN_SPLIT && (!work || !aligned16(work))) return fail("%s: the split regime needs a 16-byte aligned workspace", who);
    return 1;
}

inline int small_grid(const cspn_abn_plan_t& plan, int C) { return ceil_div(C, plan.channels_per_workgroup); }
// SPLIT workspace: [C][W][4] partials, then 2 x C floats (edz, eydz of a backward that computes them itself)
inline size_t partial_floats(const cspn_abn_plan_t& plan, int C) { return (size_t)C * plan.workgroups_per_channel * 4; }

}  // namespace

extern "C" {

int cspn_abn_abi_version(void) { return CSPN_ABN_ABI_VERSION; }

int cspn_abn_plan(int N, int C, int S, cspn_abn_plan_t* plan) { return abn_plan(N, C, S, plan); }

size_t cspn_abn_workspace_bytes(int N, int C, int S) {
    cspn_abn_plan_t plan;
    if (!abn_plan(N, C, S, &plan) || plan.regime == CSPN_ABN_SMALL) return 0;
    return (partial_floats(plan, C) + 2 * (size_t)C) * sizeof(float);
}

int cspn_abn_forward(void* x, const float* weight, const float* bias, float* running_mean, float* running_var, float* mean,
                     float* var, int N, int C, int S, int training, int phase, float momentum, float eps, int activation,
                     float slope, void* work, cspn_stream_t stream) {
    const char* who = "cspn_abn_forward";
    AbnForwardArgs a;
    cspn_abn_plan_t plan;
    if (!abn_shape(who, N, C, S, {x}, &a.sh, &plan) || !check_activation(who, activation)) return 0;
    if (phase != CSPN_ABN_FULL && phase != CSPN_ABN_STATS_ONLY && phase != CSPN_ABN_APPLY_ONLY) return fail("%s: unknown phase %d", who, phase);
    if (!training && phase != CSPN_ABN_FULL) return fail("%s: an eval-mode call has no halves", who);
    if (!training && (!running_mean || !running_var)) return fail("%s: eval mode needs running_mean / running_var", who);
    if (training && (!mean || !var)) return fail("%s: training mode needs mean / var", who);
    if (training && phase == CSPN_ABN_FULL && a.sh.NS < 2)
        return fail("%s: training statistics need more than 1 value per channel (N * S = %zu)", who, a.sh.NS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.x = static_cast<float*>(x);
    a.weight = weight; a.bias = bias;
    a.running_mean = running_mean; a.running_var = running_var;
    a.mean = training ? mean : running_mean;
    a.var = training ? var : running_var;
    a.partial = static_cast<float*>(work);
    a.momentum = momentum; a.eps = eps; a.slope = slope; a.act = activation;
    const int grid = C * a.sh.W;
    if (!training || phase == CSPN_ABN_APPLY_ONLY) {
        hipLaunchKernelGGL(abn_apply_kernel, dim3(grid), dim3(ABN_THREADS), 0, st, a);
        HIP_OK(hipGetLastError());
        return 1;
    }
    if (plan.regime == CSPN_ABN_SMALL) {
        const dim3 g(small_grid(plan, C)), b(ABN_THREADS);
        const bool shared = plan.channels_per_workgroup > 1, apply = phase == CSPN_ABN_FULL;
        if (shared && apply) hipLaunchKernelGGL((abn_small_forward_kernel<64, true>), g, b, 0, st, a);
        else if (shared) hipLaunchKernelGGL((abn_small_forward_kernel<64, false>), g, b, 0, st, a);
        else if (apply) hipLaunchKernelGGL((abn_small_forward_kernel<ABN_THREADS, true>), g, b, 0, st, a);
        else hipLaunchKernelGGL((abn_small_forward_kernel<ABN_THREADS, false>), g, b, 0, st, a);
        HIP_OK(hipGetLastError());
        return 1;
    }
    if (!check_work(who, plan, work)) return 0;
    hipLaunchKernelGGL(abn_partial_stats_kernel, dim3(grid), dim3(ABN_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(abn_finalise_stats_kernel, dim3(ceil_div(C, 64)), dim3(64), 0, st, a, phase == CSPN_ABN_FULL ? 1 : 0);
    HIP_OK(hipGetLastError());
    if (phase == CSPN_ABN_FULL) {
        hipLaunchKernelGGL(abn_apply_kernel, dim3(grid), dim3(ABN_THREADS), 0, st, a);
        HIP_OK(hipGetLastError());
    }
    return 1;
}

namespace {
int backward_args(const char* who, AbnBackwardArgs& a, const float* weight, const float* bias, float eps, int activation, float slope) {
    if (!check_activation(who, activation)) return 0;
    a.weight = weight; a.bias = bias;
    a.eps = eps; a.slope = slope; a.act = activation;
    a.inv_slope = (float)(1.0 / (double)slope);
    a.var = nullptr;
    a.edz_in = a.eydz_in = nullptr;
    a.edz_out = a.eydz_out = nullptr;
    a.dx = a.dweight = a.dbias = nullptr;
    a.partial = nullptr;
    return 1;
}

// edz / eydz of (z, dz) into a.edz_out / a.eydz_out: one launch (SMALL) or partials + finalise (SPLIT)
int launch_reduce(const cspn_abn_plan_t& plan, AbnBackwardArgs& a, hipStream_t st) {
    const int C = a.sh.C;
    if (plan.regime == CSPN_ABN_SMALL) {
        const dim3 g(small_grid(plan, C)), b(ABN_THREADS);
        if (plan.channels_per_workgroup > 1) hipLaunchKernelGGL((abn_small_backward_kernel<64, false>), g, b, 0, st, a);
        else hipLaunchKernelGGL((abn_small_backward_kernel<ABN_THREADS, false>), g, b, 0, st, a);
        HIP_OK(hipGetLastError());
        return 1;
    }
    hipLaunchKernelGGL(abn_partial_grad_kernel, dim3(C * a.sh.W), dim3(ABN_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(abn_finalise_grad_kernel, dim3(ceil_div(C, 64)), dim3(64), 0, st, a);
    HIP_OK(hipGetLastError());
    return 1;
}
}  // namespace

int cspn_abn_backward_reduce(const void* z, const void* dz, const float* weight, const float* bias, float* edz, float* eydz, int N,
                             int C, int S, float eps, int activation, float slope, void* work, cspn_stream_t stream) {
    const char* who = "cspn_abn_backward_reduce";
    AbnBackwardArgs a;
    cspn_abn_plan_t plan;
    if (!abn_shape(who, N, C, S, {z, dz}, &a.sh, &plan) || !backward_args(who, a, weight, bias, eps, activation, slope)) return 0;
    if (!edz || !eydz) return fail("%s: null edz / eydz", who);
    if (!check_work(who, plan, work)) return 0;
    a.z = static_cast<const float*>(z);
    a.dz = static_cast<const float*>(dz);
    a.edz_out = edz; a.eydz_out = eydz;
    a.partial = static_cast<float*>(work);
    return launch_reduce(plan, a, static_cast<hipStream_t>(stream));
}

int cspn_abn_backward(const void* z, const void* dz, const float* var, const float* weight, const float* bias, const float* edz,
                      const float* eydz, void* dx, float* dweight, float* dbias, int N, int C, int S, int training, float eps,
                      int activation, float slope, void* work, cspn_stream_t stream) {
    const char* who = "cspn_abn_backward";
    AbnBackwardArgs a;
    cspn_abn_plan_t plan;
    if (!abn_shape(who, N, C, S, {z, dz, dx}, &a.sh, &plan) || !backward_args(who, a, weight, bias, eps, activation, slope)) return 0;
    if (!var) return fail("%s: null var", who);
    if ((edz == nullptr) != (eydz == nullptr)) return fail("%s: edz and eydz come together", who);
    if (dweight && !weight) return fail("%s: dweight without weight", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.z = static_cast<const float*>(z);
    a.dz = static_cast<const float*>(dz);
    a.var = var;
    a.dx = static_cast<float*>(dx);
    a.dweight = dweight; a.dbias = dbias;
    const bool own = training && !edz;          // the reduction is ours to do
    if (own && plan.regime == CSPN_ABN_SMALL) {
        const dim3 g(small_grid(plan, C)), b(ABN_THREADS);
        if (plan.channels_per_workgroup > 1) hipLaunchKernelGGL((abn_small_backward_kernel<64, true>), g, b, 0, st, a);
        else hipLaunchKernelGGL((abn_small_backward_kernel<ABN_THREADS, true>), g, b, 0, st, a);
        HIP_OK(hipGetLastError());
        return 1;
    }
    if (own) {
        if (!check_work(who, plan, work)) return 0;
        a.partial = static_cast<float*>(work);
        a.edz_out = a.partial + partial_floats(plan, C);
        a.eydz_out = a.edz_out + C;
        if (!launch_reduce(plan, a, st)) return 0;
        a.edz_in = a.edz_out;
        a.eydz_in = a.eydz_out;
    } else if (training) {
        a.edz_in = edz;
        a.eydz_in = eydz;
    }
    hipLaunchKernelGGL(abn_dx_kernel, dim3(C * a.sh.W), dim3(ABN_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

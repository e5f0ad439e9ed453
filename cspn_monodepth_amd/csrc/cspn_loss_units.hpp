// cspn_loss_units.hpp — the one sliced-reduction core of the loss kernels (cspn_criterion.hip, cspn_losses.hip): the cut of n
// elements into 16-byte units and slices, the load of one unit, the per-slice pass, both stages of the sums, the streaming
// backward and the argument checks of the entry points.  A family adds its TERM / GRAD structs, its state and its kind check.
//
// Determinism contract (include/cspn_criterion.h, include/cspn_losses.h): a state depends only on the n values of both planes,
// the kind and n.
//   * the n elements are cut into UNITS of 16 bytes (4 floats), unit u = elements [4u, 4u + 4);
//   * unit u belongs to slice (u / 256) % S, thread u % 256 of that slice's workgroup, S = criterion_slices(n);
//     a thread adds its units in increasing u: fp32 over a group of 4 units, groups into fp64 (slice_pass);
//   * a workgroup adds its 256 threads by wave_sum_to_lane63 (cspn_common.hpp) and its 4 wavefronts in wavefront order
//     (block_sums_to_work);
//   * the second stage adds the S slices in an order that depends on S only: lane l adds slices l, l + 64, ..., then the lanes
//     (wave_sum_of_slices).
// Whether the 16 bytes of a unit come in one load (16-byte aligned bases) or element by element (a view that starts inside a
// larger buffer, the partial last unit) changes the load instructions only: both fill the same registers in front of ONE copy
// of the arithmetic.  The backward (stream_grad) is element-wise, so it has no order to fix.
#pragma once
#include "cspn_common.hpp"

namespace {

constexpr int CRIT_THREADS = 256;      // 4 wavefronts per slice workgroup
constexpr int CRIT_GROUP = 4;          // units a thread adds in fp32 before the partial goes to fp64 (16 pixels)
constexpr int CRIT_MAX_SLICES = 1024;
constexpr int CRIT_BWD_MAX_GRID = 2048;

// Slices (workgroups) of the forward: a function of n ONLY — one slice per 256 units (1024 pixels) up to 1024 slices, so a
// 3 x 228 x 304 batch already spreads over 204 workgroups and 24 x 228 x 304 over four per CU; larger inputs grid-stride.
inline int criterion_slices(size_t n) {
    const size_t nu = (n + 3) / 4;
    size_t s = (nu + CRIT_THREADS - 1) / CRIT_THREADS;
    if (s < 1) s = 1;
    if (s > CRIT_MAX_SLICES) s = CRIT_MAX_SLICES;
    return (int)s;
}

// pixels [4u, 4u + 4) of both planes; past the end: (pad_a, pad_b), a pixel that adds nothing to the caller's reduction
__device__ __forceinline__ void load_unit(const float* __restrict__ a, const float* __restrict__ b, size_t u, size_t n, bool vec,
                                          float (&va)[4], float (&vb)[4], float pad_a, float pad_b) {
    const size_t e0 = u * 4;
    if (vec && e0 + 4 <= n) {
        const float4 x = ld4(a + e0), y = ld4(b + e0);
        va[0] = x.x; va[1] = x.y; va[2] = x.z; va[3] = x.w;
        vb[0] = y.x; vb[1] = y.y; vb[2] = y.z; vb[3] = y.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool in = e0 + e < n;
            va[e] = in ? ld1(a + e0 + e) : pad_a;
            vb[e] = in ? ld1(b + e0 + e) : pad_b;
        }
    }
}

// One trip structure for every sliced pass, grid (S): TERM::add(a, b, fs, fc) is called for the 16 pixels of a group with fp32
// partials, which then go to fp64.  All loads of a group come first, then the arithmetic; a thread has more than one unit only
// past 1024 x 256 units (n > 1 M elements: 24 x 228 x 304 gives 1 or 2), and a full group of 4 from 4 M elements on.  Past the
// end of the planes a pixel is (TERM::pad_a, TERM::pad_b), which adds nothing.
template <class TERM>
__device__ __forceinline__ void slice_pass(const float* __restrict__ a, const float* __restrict__ b, size_t n, TERM& term,
                                           double (&acc)[2]) {
    const int S = gridDim.x, s = blockIdx.x;
    const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;              // workgroup-uniform
    const size_t nu = (n + 3) / 4;                                           // the last unit may be partial
    const size_t stride = (size_t)S * CRIT_THREADS;
    acc[0] = 0.0;
    acc[1] = 0.0;
    for (size_t u0 = (size_t)s * CRIT_THREADS + threadIdx.x; u0 < nu; u0 += CRIT_GROUP * stride) {
        float va[CRIT_GROUP][4], vb[CRIT_GROUP][4];
#pragma unroll
        for (int j = 0; j < CRIT_GROUP; ++j) {
            const size_t u = u0 + (size_t)j * stride;
            if (u < nu) {
                load_unit(a, b, u, n, vec, va[j], vb[j], TERM::pad_a(), TERM::pad_b());
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) { va[j][e] = TERM::pad_a(); vb[j][e] = TERM::pad_b(); }
            }
        }
        float fs = 0.f, fc = 0.f;
#pragma unroll
        for (int j = 0; j < CRIT_GROUP; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) term.add(va[j][e], vb[j][e], fs, fc);
        acc[0] += (double)fs;
        acc[1] += (double)fc;
    }
}

// the workgroup's sums of K per-thread fp64 partials -> out[0..K): wave_sum_to_lane63 (all 64 lanes are here: the loop of
// slice_pass has rejoined), then the 4 wavefronts in wavefront order
template <int K>
__device__ __forceinline__ void block_sums_to_work(const double (&acc)[K], double (&part)[CRIT_THREADS / 64][K], double* __restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum_to_lane63(acc[k]);
        if (lane == 63) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CRIT_THREADS / 64; ++w) v += part[w][threadIdx.x];
        out[threadIdx.x] = v;
    }
}

// Quantity k of the S <= 1024 slices (WORK doubles per slice), added by one wavefront: lane l adds slices l, l + 64, ... in
// increasing order, the lanes go through wave_sum_to_lane63 (valid in lane 63).  All of a lane's loads are issued before its
// first add — the slices were written by other workgroups, so each load is a trip past the L2, and sixteen of them one after
// the other were the launch's whole time; a slice past S adds +0.0, which changes no bit (a lane's sum starts from +0.0, so it
// is never -0.0).
template <int WORK>
__device__ __forceinline__ double wave_sum_of_slices(const double* __restrict__ work, int S, int k, int lane) {
    constexpr int PER_LANE = CRIT_MAX_SLICES / 64;
    double part[PER_LANE];
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        const int s = lane + 64 * j;
        part[j] = s < S ? work[(size_t)s * WORK + k] : 0.0;
    }
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) v += part[j];
    return wave_sum_to_lane63(v);
}

// the streaming grid of a backward over n elements: one unit per thread and trip
inline unsigned loss_backward_grid(size_t n) {
    const size_t nu = (n + 3) / 4;
    size_t grid = (nu + CRIT_THREADS - 1) / CRIT_THREADS;
    if (grid > CRIT_BWD_MAX_GRID) grid = CRIT_BWD_MAX_GRID;
    return (unsigned)grid;
}

// grid-stride over units, one unit (16 bytes of each plane) per thread and trip; GRAD is built from the state on the device.
// Past the end of the planes a lane computes grad(1, 1) for every family and never stores it.
template <class GRAD>
__device__ __forceinline__ void stream_grad(const float* __restrict__ a, const float* __restrict__ b, size_t n, const GRAD& grad,
                                            float* __restrict__ out) {
    const bool vec = (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0;
    const size_t nu = (n + 3) / 4;
    const size_t stride = (size_t)gridDim.x * CRIT_THREADS;
    for (size_t u = (size_t)blockIdx.x * CRIT_THREADS + threadIdx.x; u < nu; u += stride) {
        const size_t e0 = u * 4;
        float va[4], vb[4], g[4];
        load_unit(a, b, u, n, vec, va, vb, 1.f, 1.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = grad(va[e], vb[e]);
        if (vec && e0 + 4 <= n) {
            st4(out + e0, make_float4(g[0], g[1], g[2], g[3]));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e0 + e < n) st1(out + e0 + e, g[e]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the entry points' checks
inline int check_planes(const char* who, const void* a, const void* b, int dtype, size_t n) {
    if (!a || !b) return fail("%s: null input plane", who);
    if (n < 1) return fail("%s: n must be at least 1", who);
    if (dtype != CSPN_F32)
        return fail("%s: unsupported dtype %d, fp32 only: the gradient of a mean over ~1e6 pixels is below what fp16 can hold "
                    "(include/cspn_criterion.h)", who, dtype);
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3)
        return fail("%s: the input planes are not aligned to their element size", who);
    return 1;
}

inline int check_forward(const char* who, const void* work, const void* state) {
    if (!work || !state) return fail("%s: null work / state", who);
    if (reinterpret_cast<uintptr_t>(work) & 7 || reinterpret_cast<uintptr_t>(state) & 7)
        return fail("%s: work / state must be 8-byte aligned", who);
    return 1;
}

inline int check_backward(const char* who, const void* state, const float* grad_loss, const void* grad) {
    if (!state || !grad_loss || !grad) return fail("%s: null state / grad_loss / gradient plane", who);
    if (reinterpret_cast<uintptr_t>(state) & 7) return fail("%s: state must be 8-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(grad_loss) | reinterpret_cast<uintptr_t>(grad)) & 3)
        return fail("%s: grad_loss / the gradient plane are not aligned to their element size", who);
    return 1;
}

}  // namespace

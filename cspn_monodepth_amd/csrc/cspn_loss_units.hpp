// cspn_loss_units.hpp — what the sliced loss reductions share (cspn_criterion.hip, cspn_losses.hip): the cut of n elements into
// 16-byte units and slices, and the load of one unit.  The wavefront sums are cspn_common.hpp's wave_sum_to_lane63.
//
// The slice discipline (include/cspn_criterion.h): unit u = elements [4u, 4u + 4) belongs to slice (u / 256) % S, thread u % 256
// of that slice's workgroup, S = criterion_slices(n); a thread adds its units in increasing u, fp32 over a group of 4 units,
// groups into fp64; a workgroup adds its 4 wavefronts in wavefront order; the S slices are added in an order that depends on S only.
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

// the streaming grid of a backward over n elements: one unit per thread and trip
inline unsigned loss_backward_grid(size_t n) {
    const size_t nu = (n + 3) / 4;
    size_t grid = (nu + CRIT_THREADS - 1) / CRIT_THREADS;
    if (grid > CRIT_BWD_MAX_GRID) grid = CRIT_BWD_MAX_GRID;
    return (unsigned)grid;
}

}  // namespace

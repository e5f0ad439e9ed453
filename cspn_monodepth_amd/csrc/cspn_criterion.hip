// cspn_criterion.hip — the reference's training criteria (libs/criterion/criteria.py:14-39 MaskedMSELoss / MaskedL1Loss,
// :91-107 L1_log: the mean of a per-pixel term over target > 0), forward and backward, as kernels without atomics
// (include/cspn_criterion.h).
//
// Determinism contract: the state depends only on the n values of pred and target, the kind and n.
//   * the n elements are cut into UNITS of 16 bytes (4 floats), unit u = elements [4u, 4u + 4);
//   * unit u belongs to slice (u / 256) % S, thread u % 256 of that slice's workgroup, S = criterion_slices(n);
//     a thread adds its units in increasing u: fp32 over a group of 4 units, groups into fp64;
//   * a workgroup adds its 256 threads by wave_sum_to_lane63 and its 4 wavefronts in wavefront order -> work[s][0..1];
//   * the second stage adds the S slices in an order that depends on S only (lane l: slices l, l + 64, ...; then the lanes).
// Whether the 16 bytes of a unit come in one load (16-byte aligned bases) or element by element (a view that starts inside a
// larger buffer, the partial last unit) changes the load instructions only: both fill the same registers in front of ONE copy
// of the arithmetic.  The backward is element-wise, so it has no order to fix.
#include "cspn_loss_units.hpp"
#include "cspn_criterion.h"

namespace {

struct CriterionState {                // include/cspn_criterion.h: CSPN_CRITERION_STATE_BYTES
    float loss, inv_count;
    double sum, count, reserved;
};
static_assert(sizeof(CriterionState) == CSPN_CRITERION_STATE_BYTES, "state layout");

// the term of one pixel, 0 for an invalid one (the selects keep a NaN / Inf of an invalid pixel out of the sum)
template <int KIND>
__device__ __forceinline__ void criterion_term(float p, float t, float& sum, float& cnt) {
    const bool valid = t > 0.f;                 // false for NaN
    float v;
    if (KIND == CSPN_LOSS_L1) {
        v = fabsf(t - p);
    } else if (KIND == CSPN_LOSS_L2) {
        const float d = t - p;
        v = d * d;
    } else {
        v = fabsf(logf(t) - logf(p));
    }
    sum += valid ? v : 0.f;
    cnt += valid ? 1.f : 0.f;
}

// grid (S): workgroup s -> work[s][0] = sum of the term, work[s][1] = valid pixels; past the end of the planes load_unit
// (cspn_loss_units.hpp) gives an invalid pixel: pred 1, target 0
template <int KIND>
__global__ __launch_bounds__(CRIT_THREADS) void cspn_criterion_slice_kernel(const float* __restrict__ pred,
                                                                            const float* __restrict__ target, size_t n,
                                                                            double* __restrict__ work) {
    const int S = gridDim.x, s = blockIdx.x;
    const bool vec = (((uintptr_t)pred | (uintptr_t)target) & 15) == 0;     // workgroup-uniform
    const size_t nu = (n + 3) / 4;                                           // the last unit may be partial
    const size_t stride = (size_t)S * CRIT_THREADS;
    double acc_sum = 0.0, acc_cnt = 0.0;
    for (size_t u0 = (size_t)s * CRIT_THREADS + threadIdx.x; u0 < nu; u0 += CRIT_GROUP * stride) {
        float p[CRIT_GROUP][4], t[CRIT_GROUP][4];
        // all loads of the group first, then the arithmetic.  A thread has more than one unit only past 1024 x 256 units
        // (n > 1 M elements: 24 x 228 x 304 gives 1 or 2), and a full group of 4 from 4 M elements on
#pragma unroll
        for (int j = 0; j < CRIT_GROUP; ++j) {
            const size_t u = u0 + (size_t)j * stride;
            if (u < nu) {
                load_unit(pred, target, u, n, vec, p[j], t[j], 1.f, 0.f);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) { p[j][e] = 1.f; t[j][e] = 0.f; }
            }
        }
        float fs = 0.f, fc = 0.f;
#pragma unroll
        for (int j = 0; j < CRIT_GROUP; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) criterion_term<KIND>(p[j][e], t[j][e], fs, fc);
        acc_sum += (double)fs;
        acc_cnt += (double)fc;
    }
    // wavefront sum by DPP (all 64 lanes are here: the loop has rejoined), then the 4 wavefronts in order
    __shared__ double part[CRIT_THREADS / 64][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double vs = wave_sum_to_lane63(acc_sum), vc = wave_sum_to_lane63(acc_cnt);
    if (lane == 63) {
        part[wave][0] = vs;
        part[wave][1] = vc;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CRIT_THREADS / 64; ++w) v += part[w][threadIdx.x];
        work[(size_t)s * 2 + threadIdx.x] = v;
    }
}

// One workgroup, one wavefront per quantity (0: sum, 1: count): lane l adds slices l, l + 64, ... in increasing order, the 64
// lane sums go through wave_sum_to_lane63; thread 0 then writes the state.
constexpr int CRIT_COMBINE_THREADS = 128;
__global__ __launch_bounds__(CRIT_COMBINE_THREADS) void cspn_criterion_combine_kernel(const double* __restrict__ work, int S,
                                                                                      CriterionState* __restrict__ state) {
    __shared__ double tot[2];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double v = 0.0;
    for (int s = lane; s < S; s += 64) v += work[(size_t)s * 2 + k];
    v = wave_sum_to_lane63(v);
    if (lane == 63) tot[k] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = tot[0], count = tot[1];
        state->loss = (float)(sum / count);             // no valid pixel: 0 / 0 = NaN, as the reference's mean over nothing
        state->inv_count = (float)(1.0 / count);
        state->sum = sum;
        state->count = count;
        state->reserved = 0.0;
    }
}

// d loss / d pred of one pixel; scale = g / count
template <int KIND>
__device__ __forceinline__ float criterion_grad(float p, float t, float scale) {
    if (!(t > 0.f)) return 0.f;
    if (KIND == CSPN_LOSS_L2) return scale * (2.f * (p - t));
    // the backward of abs multiplies by sgn(d), and sgn(0) = sgn(NaN) = 0
    const float d = KIND == CSPN_LOSS_L1 ? t - p : logf(t) - logf(p);
    const float a = scale * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
    // l1_log: d(-log p) = -1 / p — p == 0 gives -inf, p < 0 had d = NaN, so -0 / p = 0
    return KIND == CSPN_LOSS_L1 ? -a : -a / p;
}

// grid-stride over units, one unit (16 bytes of each plane) per thread and trip
template <int KIND>
__global__ __launch_bounds__(CRIT_THREADS) void cspn_criterion_backward_kernel(const float* __restrict__ pred,
                                                                               const float* __restrict__ target, size_t n,
                                                                               const CriterionState* __restrict__ state,
                                                                               const float* __restrict__ grad_loss,
                                                                               float* __restrict__ grad_pred) {
    const bool vec = (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)grad_pred) & 15) == 0;
    const size_t nu = (n + 3) / 4;
    const size_t stride = (size_t)gridDim.x * CRIT_THREADS;
    const float scale = *grad_loss * state->inv_count;
    for (size_t u = (size_t)blockIdx.x * CRIT_THREADS + threadIdx.x; u < nu; u += stride) {
        const size_t e0 = u * 4;
        float p[4], t[4], g[4];
        load_unit(pred, target, u, n, vec, p, t, 1.f, 0.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = criterion_grad<KIND>(p[e], t[e], scale);
        if (vec && e0 + 4 <= n) {
            st4(grad_pred + e0, make_float4(g[0], g[1], g[2], g[3]));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e0 + e < n) st1(grad_pred + e0 + e, g[e]);
        }
    }
}

int check_common(const char* who, const void* pred, const void* target, int dtype, int kind, size_t n) {
    if (!pred || !target) return fail("%s: null pred / target", who);
    if (n < 1) return fail("%s: n must be at least 1", who);
    if (dtype != CSPN_F32)
        return fail("%s: unsupported dtype %d, fp32 only: the gradient of a mean over ~1e6 pixels is below what fp16 can hold "
                    "(include/cspn_criterion.h)", who, dtype);
    if (kind != CSPN_LOSS_L1 && kind != CSPN_LOSS_L2 && kind != CSPN_LOSS_L1_LOG) return fail("%s: unknown kind %d", who, kind);
    if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & 3)
        return fail("%s: pred / target are not aligned to their element size", who);
    return 1;
}

}  // namespace

extern "C" {

int cspn_criterion_abi_version(void) { return CSPN_CRITERION_ABI_VERSION; }

size_t cspn_criterion_workspace_bytes(size_t n) {
    if (n < 1) return 0;
    return (size_t)criterion_slices(n) * 2 * sizeof(double);
}

int cspn_criterion_forward(const void* pred, const void* target, int dtype, int kind, size_t n, void* work, void* state,
                           cspn_stream_t stream) {
    if (!check_common("cspn_criterion_forward", pred, target, dtype, kind, n)) return 0;
    if (!work || !state) return fail("cspn_criterion_forward: null work / state");
    if (reinterpret_cast<uintptr_t>(work) & 7 || reinterpret_cast<uintptr_t>(state) & 7)
        return fail("cspn_criterion_forward: work / state must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = criterion_slices(n);
    const float* p = static_cast<const float*>(pred);
    const float* t = static_cast<const float*>(target);
    double* w = static_cast<double*>(work);
    if (kind == CSPN_LOSS_L1)
        hipLaunchKernelGGL((cspn_criterion_slice_kernel<CSPN_LOSS_L1>), dim3(S), dim3(CRIT_THREADS), 0, st, p, t, n, w);
    else if (kind == CSPN_LOSS_L2)
        hipLaunchKernelGGL((cspn_criterion_slice_kernel<CSPN_LOSS_L2>), dim3(S), dim3(CRIT_THREADS), 0, st, p, t, n, w);
    else
        hipLaunchKernelGGL((cspn_criterion_slice_kernel<CSPN_LOSS_L1_LOG>), dim3(S), dim3(CRIT_THREADS), 0, st, p, t, n, w);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(cspn_criterion_combine_kernel, dim3(1), dim3(CRIT_COMBINE_THREADS), 0, st, static_cast<const double*>(w), S,
                       static_cast<CriterionState*>(state));
    HIP_OK(hipGetLastError());
    return 1;
}

int cspn_criterion_backward(const void* pred, const void* target, int dtype, int kind, size_t n, const void* state,
                            const float* grad_loss, void* grad_pred, cspn_stream_t stream) {
    if (!check_common("cspn_criterion_backward", pred, target, dtype, kind, n)) return 0;
    if (!state || !grad_loss || !grad_pred) return fail("cspn_criterion_backward: null state / grad_loss / grad_pred");
    if (reinterpret_cast<uintptr_t>(state) & 7) return fail("cspn_criterion_backward: state must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(grad_loss) | reinterpret_cast<uintptr_t>(grad_pred)) & 3)
        return fail("cspn_criterion_backward: grad_loss / grad_pred are not aligned to their element size");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = loss_backward_grid(n);
    const float* p = static_cast<const float*>(pred);
    const float* t = static_cast<const float*>(target);
    const CriterionState* s = static_cast<const CriterionState*>(state);
    float* g = static_cast<float*>(grad_pred);
    if (kind == CSPN_LOSS_L1)
        hipLaunchKernelGGL((cspn_criterion_backward_kernel<CSPN_LOSS_L1>), dim3(grid), dim3(CRIT_THREADS), 0, st, p, t, n, s, grad_loss, g);
    else if (kind == CSPN_LOSS_L2)
        hipLaunchKernelGGL((cspn_criterion_backward_kernel<CSPN_LOSS_L2>), dim3(grid), dim3(CRIT_THREADS), 0, st, p, t, n, s, grad_loss, g);
    else
        hipLaunchKernelGGL((cspn_criterion_backward_kernel<CSPN_LOSS_L1_LOG>), dim3(grid), dim3(CRIT_THREADS), 0, st, p, t, n, s, grad_loss, g);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

// cspn_criterion.hip — the reference's training criteria (libs/criterion/criteria.py:14-39 MaskedMSELoss / MaskedL1Loss,
// :91-107 L1_log: the mean of a per-pixel term over target > 0), forward and backward, as kernels without atomics
// (include/cspn_criterion.h).
//
// Every pass, sum, streaming backward and argument check is the core of cspn_loss_units.hpp, where the determinism contract is
// written out; this file holds the masked term and its gradient, the state and the kind check.  work[s] = {sum of the term,
// valid pixels} of slice s.
#include "cspn_loss_units.hpp"
#include "cspn_criterion.h"

namespace {

constexpr int CRIT_WORK = 2;           // doubles per slice: sum, count

struct CriterionState {                // include/cspn_criterion.h: CSPN_CRITERION_STATE_BYTES
    float loss, inv_count;
    double sum, count, reserved;
};
static_assert(sizeof(CriterionState) == CSPN_CRITERION_STATE_BYTES, "state layout");

// the term of one pixel, 0 for an invalid one (the selects keep a NaN / Inf of an invalid pixel out of the sum); a padding
// pixel is invalid: pred 1, target 0
template <int KIND>
struct MaskedTerm {
    static __device__ __forceinline__ float pad_a() { return 1.f; }
    static __device__ __forceinline__ float pad_b() { return 0.f; }
    __device__ __forceinline__ void add(float p, float t, float& sum, float& cnt) {
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
};

template <int KIND>
__global__ __launch_bounds__(CRIT_THREADS) void cspn_criterion_slice_kernel(const float* __restrict__ pred,
                                                                            const float* __restrict__ target, size_t n,
                                                                            double* __restrict__ work) {
    __shared__ double part[CRIT_THREADS / 64][CRIT_WORK];
    MaskedTerm<KIND> term;
    double acc[2];
    slice_pass(pred, target, n, term, acc);
    block_sums_to_work<CRIT_WORK>(acc, part, work + (size_t)blockIdx.x * CRIT_WORK);
}

// One workgroup, one wavefront per quantity (0: sum, 1: count); thread 0 then writes the state.
constexpr int CRIT_COMBINE_THREADS = 128;
__global__ __launch_bounds__(CRIT_COMBINE_THREADS) void cspn_criterion_combine_kernel(const double* __restrict__ work, int S,
                                                                                      CriterionState* __restrict__ state) {
    __shared__ double tot[2];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double v = wave_sum_of_slices<CRIT_WORK>(work, S, k, lane);
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

// d loss / d pred of one pixel
template <int KIND>
struct MaskedGrad {
    float scale;                       // g / count
    __device__ __forceinline__ float operator()(float p, float t) const {
        if (!(t > 0.f)) return 0.f;
        if (KIND == CSPN_LOSS_L2) return scale * (2.f * (p - t));
        // the backward of abs multiplies by sgn(d), and sgn(0) = sgn(NaN) = 0
        const float d = KIND == CSPN_LOSS_L1 ? t - p : logf(t) - logf(p);
        const float a = scale * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
        // l1_log: d(-log p) = -1 / p — p == 0 gives -inf, p < 0 had d = NaN, so -0 / p = 0
        return KIND == CSPN_LOSS_L1 ? -a : -a / p;
    }
};

template <int KIND>
__global__ __launch_bounds__(CRIT_THREADS) void cspn_criterion_backward_kernel(const float* __restrict__ pred,
                                                                               const float* __restrict__ target, size_t n,
                                                                               const CriterionState* __restrict__ state,
                                                                               const float* __restrict__ grad_loss,
                                                                               float* __restrict__ grad_pred) {
    MaskedGrad<KIND> grad;
    grad.scale = *grad_loss * state->inv_count;
    stream_grad(pred, target, n, grad, grad_pred);
}

bool masked_kind_ok(int kind) { return kind >= CSPN_LOSS_L1 && kind <= CSPN_LOSS_L1_LOG; }

}  // namespace

extern "C" {

int cspn_criterion_abi_version(void) { return CSPN_CRITERION_ABI_VERSION; }

size_t cspn_criterion_workspace_bytes(size_t n) {
    if (n < 1) return 0;
    return (size_t)criterion_slices(n) * CRIT_WORK * sizeof(double);
}

int cspn_criterion_forward(const void* pred, const void* target, int dtype, int kind, size_t n, void* work, void* state,
                           cspn_stream_t stream) {
    if (!check_planes("cspn_criterion_forward", pred, target, dtype, n)) return 0;
    if (!masked_kind_ok(kind)) return fail("cspn_criterion_forward: unknown kind %d", kind);
    if (!check_forward("cspn_criterion_forward", work, state)) return 0;
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
    if (!check_planes("cspn_criterion_backward", pred, target, dtype, n)) return 0;
    if (!masked_kind_ok(kind)) return fail("cspn_criterion_backward: unknown kind %d", kind);
    if (!check_backward("cspn_criterion_backward", state, grad_loss, grad_pred)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(loss_backward_grid(n)), block(CRIT_THREADS);
    const float* p = static_cast<const float*>(pred);
    const float* t = static_cast<const float*>(target);
    const CriterionState* s = static_cast<const CriterionState*>(state);
    float* g = static_cast<float*>(grad_pred);
    if (kind == CSPN_LOSS_L1)
        hipLaunchKernelGGL((cspn_criterion_backward_kernel<CSPN_LOSS_L1>), grid, block, 0, st, p, t, n, s, grad_loss, g);
    else if (kind == CSPN_LOSS_L2)
        hipLaunchKernelGGL((cspn_criterion_backward_kernel<CSPN_LOSS_L2>), grid, block, 0, st, p, t, n, s, grad_loss, g);
    else
        hipLaunchKernelGGL((cspn_criterion_backward_kernel<CSPN_LOSS_L1_LOG>), grid, block, 0, st, p, t, n, s, grad_loss, g);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

// cspn_losses.hip — the reference's berHuLoss (libs/criterion/criteria.py:42-64) and its unmasked means L1, GradLoss, RMSE and
// RMSE_log (:79-88, :145-152, :133-142, :67-76), forward and backward, as kernels without atomics (include/cspn_losses.h).
//
// Every pass, sum, streaming backward and argument check is the core of cspn_loss_units.hpp, where the determinism contract is
// written out; this file holds the TERM / GRAD structs, the state and berHu's maximum.  berHu needs max(pred - target) in front
// of its second sum:
//   launch 1, grid S: work[s] = {sum_valid d, n_valid, -, -, max e} of slice s;
//   launch 2, grid S: every workgroup reduces the S <= 1024 slice maxima itself, c = 0.2f * m, then adds {sum_huber d^2, n_huber}
//                     over the SAME units its slice had in launch 1 (a second read of both planes);
//   launch 3, one workgroup: the same reduction of the maxima, the four sums over the slices -> state.
// The maximum is combined by nanmax, which returns a NaN operand: unlike fmaxf it keeps a NaN, as torch.max does, and its result
// does not depend on the order (every e is a fp32 value; max over a set is that set's largest element or NaN).
#include "cspn_loss_units.hpp"
#include "cspn_losses.h"

namespace {

constexpr int LOSS_WORK = 5;           // doubles per slice: sum, count, sum2, count2, max
constexpr float BERHU_RATIO = 0.2f;

struct LossState {                     // include/cspn_losses.h: CSPN_LOSSES_STATE_BYTES
    float loss, factor, c, reserved;
    double sum, sum2, n_valid, n_huber;
};
static_assert(sizeof(LossState) == CSPN_LOSSES_STATE_BYTES, "state layout");

__device__ __forceinline__ float nanmax(float a, float b) { return (a > b || a != a) ? a : b; }

// the maximum over the workgroup's 256 threads, in every thread
__device__ __forceinline__ float block_nanmax(float m, float (&wave_max)[CRIT_THREADS / 64]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = nanmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    return nanmax(nanmax(wave_max[0], wave_max[1]), nanmax(wave_max[2], wave_max[3]));
}

// max e over the S slices of launch 1, in every thread of a 256-thread workgroup
__device__ __forceinline__ float max_of_slices(const double* __restrict__ work, int S, float (&wave_max)[CRIT_THREADS / 64]) {
    float m = -INFINITY;
    for (int s = threadIdx.x; s < S; s += CRIT_THREADS) m = nanmax(m, (float)work[(size_t)s * LOSS_WORK + 4]);
    return block_nanmax(m, wave_max);
}

// ------------------------------------------------------------------------------------------------ berHu
struct BerhuFirst {                    // sum_valid d, n_valid and max e; a padding pixel has e = -inf and target 0
    float m = -INFINITY;
    static __device__ __forceinline__ float pad_a() { return -INFINITY; }
    static __device__ __forceinline__ float pad_b() { return 0.f; }
    __device__ __forceinline__ void add(float p, float t, float& sum, float& cnt) {
        m = nanmax(m, p - t);
        const bool valid = t > 0.f;                 // false for NaN
        const float d = fabsf(t - p);
        sum += valid ? d : 0.f;
        cnt += valid ? 1.f : 0.f;
    }
};

struct BerhuSecond {                   // sum_huber d^2 and n_huber
    float c;
    static __device__ __forceinline__ float pad_a() { return 1.f; }
    static __device__ __forceinline__ float pad_b() { return 0.f; }
    __device__ __forceinline__ void add(float p, float t, float& sum, float& cnt) {
        const float d = fabsf(t - p);
        const bool huber = t > 0.f && d > c;        // false when c is NaN; d == 0 is in when c < 0
        sum += huber ? d * d : 0.f;
        cnt += huber ? 1.f : 0.f;
    }
};

__global__ __launch_bounds__(CRIT_THREADS) void cspn_berhu_first_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                        size_t n, double* __restrict__ work) {
    __shared__ double part[CRIT_THREADS / 64][2];
    __shared__ float wave_max[CRIT_THREADS / 64];
    BerhuFirst term;
    double acc[2];
    slice_pass(pred, target, n, term, acc);
    double* out = work + (size_t)blockIdx.x * LOSS_WORK;
    block_sums_to_work<2>(acc, part, out);
    const float m = block_nanmax(term.m, wave_max);
    if (threadIdx.x == 0) out[4] = (double)m;       // exact, and a NaN stays one
}

__global__ __launch_bounds__(CRIT_THREADS) void cspn_berhu_second_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                         size_t n, double* __restrict__ work) {
    __shared__ double part[CRIT_THREADS / 64][2];
    __shared__ float wave_max[CRIT_THREADS / 64];
    BerhuSecond term;
    term.c = BERHU_RATIO * max_of_slices(work, gridDim.x, wave_max);
    double acc[2];
    slice_pass(pred, target, n, term, acc);
    block_sums_to_work<2>(acc, part, work + (size_t)blockIdx.x * LOSS_WORK + 2);
}

// One workgroup: the threshold as launch 2 computed it, then wavefront k adds quantity k of the S slices; thread 0 writes the state.
__global__ __launch_bounds__(CRIT_THREADS) void cspn_berhu_combine_kernel(const double* __restrict__ work, int S, LossState* __restrict__ state) {
    __shared__ double tot[4];
    __shared__ float wave_max[CRIT_THREADS / 64];
    const float c = BERHU_RATIO * max_of_slices(work, S, wave_max);
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double v = wave_sum_of_slices<LOSS_WORK>(work, S, k, lane);
    if (lane == 63) tot[k] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = tot[0], n_valid = tot[1], sum2 = tot[2], n_huber = tot[3];
        const double count = n_valid + n_huber;
        state->loss = (float)((sum + sum2) / count);     // no valid pixel: 0 / 0 = NaN, the reference's mean over nothing
        state->factor = (float)(1.0 / count);
        state->c = c;
        state->reserved = 0.f;
        state->sum = sum;
        state->sum2 = sum2;
        state->n_valid = n_valid;
        state->n_huber = n_huber;
    }
}

// ------------------------------------------------------------------------------------------------ the unmasked means
// x of one element.  Contraction is off here: each product of 10 r - 10 f is rounded on its own, as in the reference — as
// fma(10, r, -(10 f)) the difference is the rounding error of 10 f where r == f, not 0 (HIP's __fmul_rn is a plain `*` and is
// contracted like one).
template <int KIND>
__device__ __forceinline__ float mean_x(float f, float r) {
#pragma clang fp contract(off)
    if (KIND == CSPN_MEAN_GRAD) return r - f;
    if (KIND == CSPN_MEAN_RMSE_LOG) return logf(r) - logf(f);
    const float tr = 10.f * r, tf = 10.f * f;
    return tr - tf;
}

template <int KIND>
struct MeanTerm {                      // the sum of |x| or x^2; a padding pixel is (1, 1): x = 0 for every kind
    static __device__ __forceinline__ float pad_a() { return 1.f; }
    static __device__ __forceinline__ float pad_b() { return 1.f; }
    __device__ __forceinline__ void add(float f, float r, float& sum, float&) {
        const float x = mean_x<KIND>(f, r);
        sum += (KIND == CSPN_MEAN_L1 || KIND == CSPN_MEAN_GRAD) ? fabsf(x) : x * x;
    }
};

template <int KIND>
__global__ __launch_bounds__(CRIT_THREADS) void cspn_mean_slice_kernel(const float* __restrict__ fake, const float* __restrict__ real,
                                                                       size_t n, double* __restrict__ work) {
    __shared__ double part[CRIT_THREADS / 64][1];
    MeanTerm<KIND> term;
    double acc[2];
    slice_pass(fake, real, n, term, acc);
    const double one[1] = {acc[0]};
    block_sums_to_work<1>(one, part, work + (size_t)blockIdx.x * LOSS_WORK);
}

// One wavefront adds the S slices; lane 63 writes the state.
__global__ __launch_bounds__(64) void cspn_mean_combine_kernel(const double* __restrict__ work, int S, int kind, double n,
                                                               LossState* __restrict__ state) {
    const double v = wave_sum_of_slices<LOSS_WORK>(work, S, 0, threadIdx.x);
    if (threadIdx.x == 63) {
        const double mean = v / n;
        const bool root = kind == CSPN_MEAN_RMSE || kind == CSPN_MEAN_RMSE_LOG;
        const double loss = root ? sqrt(mean) : mean;
        state->loss = (float)loss;
        state->factor = (float)(root ? 1.0 / (n * loss) : 1.0 / n);     // loss == 0: +inf, and the backward gives 0 * inf = NaN
        state->c = 0.f;
        state->reserved = 0.f;
        state->sum = v;
        state->sum2 = 0.0;
        state->n_valid = n;
        state->n_huber = 0.0;
    }
}

// ------------------------------------------------------------------------------------------------ the backwards
struct BerhuGrad {
    float scale, c;                    // g / (n_valid + n_huber), the threshold
    __device__ __forceinline__ float operator()(float p, float t) const {
        if (!(t > 0.f)) return 0.f;
        const float x = t - p, d = fabsf(x);
        // the backward of abs multiplies by sgn(x), and sgn(0) = sgn(NaN) = 0
        const float a = scale * (x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f);
        return d > c ? -a * (1.f + 2.f * d) : -a;
    }
};

template <int KIND>
struct MeanGrad {
    float scale;                       // g / n or g / (n * loss)
    __device__ __forceinline__ float operator()(float f, float r) const {
        const float x = mean_x<KIND>(f, r);
        if (KIND == CSPN_MEAN_RMSE) return (-10.f * x) * scale;
        if (KIND == CSPN_MEAN_RMSE_LOG) return (-x * scale) / f;
        const float s = x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f;
        return KIND == CSPN_MEAN_L1 ? (-10.f * s) * scale : -s * scale;
    }
};

__global__ __launch_bounds__(CRIT_THREADS) void cspn_berhu_backward_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                           size_t n, const LossState* __restrict__ state,
                                                                           const float* __restrict__ grad_loss, float* __restrict__ grad_pred) {
    BerhuGrad grad;
    grad.scale = *grad_loss * state->factor;
    grad.c = state->c;
    stream_grad(pred, target, n, grad, grad_pred);
}

template <int KIND>
__global__ __launch_bounds__(CRIT_THREADS) void cspn_mean_backward_kernel(const float* __restrict__ fake, const float* __restrict__ real,
                                                                          size_t n, const LossState* __restrict__ state,
                                                                          const float* __restrict__ grad_loss, float* __restrict__ grad_fake) {
    MeanGrad<KIND> grad;
    grad.scale = *grad_loss * state->factor;
    stream_grad(fake, real, n, grad, grad_fake);
}

bool mean_kind_ok(int kind) { return kind >= CSPN_MEAN_L1 && kind <= CSPN_MEAN_RMSE_LOG; }

}  // namespace

extern "C" {

int cspn_losses_abi_version(void) { return CSPN_LOSSES_ABI_VERSION; }

size_t cspn_losses_workspace_bytes(size_t n) {
    if (n < 1) return 0;
    return (size_t)criterion_slices(n) * LOSS_WORK * sizeof(double);
}

int cspn_berhu_forward(const void* pred, const void* target, int dtype, size_t n, void* work, void* state, cspn_stream_t stream) {
    if (!check_planes("cspn_berhu_forward", pred, target, dtype, n)) return 0;
    if (!check_forward("cspn_berhu_forward", work, state)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = criterion_slices(n);
    const float* p = static_cast<const float*>(pred);
    const float* t = static_cast<const float*>(target);
    double* w = static_cast<double*>(work);
    hipLaunchKernelGGL(cspn_berhu_first_kernel, dim3(S), dim3(CRIT_THREADS), 0, st, p, t, n, w);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(cspn_berhu_second_kernel, dim3(S), dim3(CRIT_THREADS), 0, st, p, t, n, w);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(cspn_berhu_combine_kernel, dim3(1), dim3(CRIT_THREADS), 0, st, static_cast<const double*>(w), S,
                       static_cast<LossState*>(state));
    HIP_OK(hipGetLastError());
    return 1;
}

int cspn_berhu_backward(const void* pred, const void* target, int dtype, size_t n, const void* state, const float* grad_loss,
                        void* grad_pred, cspn_stream_t stream) {
    if (!check_planes("cspn_berhu_backward", pred, target, dtype, n)) return 0;
    if (!check_backward("cspn_berhu_backward", state, grad_loss, grad_pred)) return 0;
    hipLaunchKernelGGL(cspn_berhu_backward_kernel, dim3(loss_backward_grid(n)), dim3(CRIT_THREADS), 0, static_cast<hipStream_t>(stream),
                       static_cast<const float*>(pred), static_cast<const float*>(target), n, static_cast<const LossState*>(state),
                       grad_loss, static_cast<float*>(grad_pred));
    HIP_OK(hipGetLastError());
    return 1;
}

int cspn_mean_loss_forward(const void* fake, const void* real, int dtype, int kind, size_t n, void* work, void* state,
                           cspn_stream_t stream) {
    if (!check_planes("cspn_mean_loss_forward", fake, real, dtype, n)) return 0;
    if (!mean_kind_ok(kind)) return fail("cspn_mean_loss_forward: unknown kind %d", kind);
    if (!check_forward("cspn_mean_loss_forward", work, state)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = criterion_slices(n);
    const float* f = static_cast<const float*>(fake);
    const float* r = static_cast<const float*>(real);
    double* w = static_cast<double*>(work);
    if (kind == CSPN_MEAN_L1)
        hipLaunchKernelGGL((cspn_mean_slice_kernel<CSPN_MEAN_L1>), dim3(S), dim3(CRIT_THREADS), 0, st, f, r, n, w);
    else if (kind == CSPN_MEAN_GRAD)
        hipLaunchKernelGGL((cspn_mean_slice_kernel<CSPN_MEAN_GRAD>), dim3(S), dim3(CRIT_THREADS), 0, st, f, r, n, w);
    else if (kind == CSPN_MEAN_RMSE)
        hipLaunchKernelGGL((cspn_mean_slice_kernel<CSPN_MEAN_RMSE>), dim3(S), dim3(CRIT_THREADS), 0, st, f, r, n, w);
    else
        hipLaunchKernelGGL((cspn_mean_slice_kernel<CSPN_MEAN_RMSE_LOG>), dim3(S), dim3(CRIT_THREADS), 0, st, f, r, n, w);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(cspn_mean_combine_kernel, dim3(1), dim3(64), 0, st, static_cast<const double*>(w), S, kind, (double)n,
                       static_cast<LossState*>(state));
    HIP_OK(hipGetLastError());
    return 1;
}

int cspn_mean_loss_backward(const void* fake, const void* real, int dtype, int kind, size_t n, const void* state,
                            const float* grad_loss, void* grad_fake, cspn_stream_t stream) {
    if (!check_planes("cspn_mean_loss_backward", fake, real, dtype, n)) return 0;
    if (!mean_kind_ok(kind)) return fail("cspn_mean_loss_backward: unknown kind %d", kind);
    if (!check_backward("cspn_mean_loss_backward", state, grad_loss, grad_fake)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(loss_backward_grid(n)), block(CRIT_THREADS);
    const float* f = static_cast<const float*>(fake);
    const float* r = static_cast<const float*>(real);
    const LossState* s = static_cast<const LossState*>(state);
    float* g = static_cast<float*>(grad_fake);
    if (kind == CSPN_MEAN_L1)
        hipLaunchKernelGGL((cspn_mean_backward_kernel<CSPN_MEAN_L1>), grid, block, 0, st, f, r, n, s, grad_loss, g);
    else if (kind == CSPN_MEAN_GRAD)
        hipLaunchKernelGGL((cspn_mean_backward_kernel<CSPN_MEAN_GRAD>), grid, block, 0, st, f, r, n, s, grad_loss, g);
    else if (kind == CSPN_MEAN_RMSE)
        hipLaunchKernelGGL((cspn_mean_backward_kernel<CSPN_MEAN_RMSE>), grid, block, 0, st, f, r, n, s, grad_loss, g);
    else
        hipLaunchKernelGGL((cspn_mean_backward_kernel<CSPN_MEAN_RMSE_LOG>), grid, block, 0, st, f, r, n, s, grad_loss, g);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

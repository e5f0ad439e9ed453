// cspn_losses.hip — the reference's berHuLoss (libs/criterion/criteria.py:42-64) and its unmasked means L1, GradLoss, RMSE and
// RMSE_log (:79-88, :145-152, :133-142, :67-76), forward and backward, as kernels without atomics (include/cspn_losses.h).
//
// The sums follow the slice discipline of cspn_loss_units.hpp, shared with cspn_criterion.hip.  berHu needs max(pred - target)
// in front of its second sum:
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

// Quantity k of the S <= 1024 slices, added by one wavefront: lane l adds slices l, l + 64, ... in increasing order, the lanes go
// through wave_sum_to_lane63 (valid in lane 63).  All of a lane's loads are issued before its first add — the slices were written
// by other workgroups, so each load is a trip past the L2, and sixteen of them one after the other were the launch's whole time;
// a slice past S adds +0.0, which changes no bit.
__device__ __forceinline__ double wave_sum_of_slices(const double* __restrict__ work, int S, int k, int lane) {
    constexpr int PER_LANE = CRIT_MAX_SLICES / 64;
    double part[PER_LANE];
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        const int s = lane + 64 * j;
        part[j] = s < S ? work[(size_t)s * LOSS_WORK + k] : 0.0;
    }
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) v += part[j];
    return wave_sum_to_lane63(v);
}

// the workgroup's sums of K per-thread fp64 partials -> work[s * LOSS_WORK + slot0 + k]: wave_sum_to_lane63, then the 4
// wavefronts in wavefront order
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

// One trip structure for every sliced pass: TERM::add(a, b, fs, fc) is called for the 16 pixels of a group with fp32 partials,
// which then go to fp64.  Past the end of the planes a pixel is (TERM::pad_a, TERM::pad_b), which adds nothing.
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
    const double v = wave_sum_of_slices(work, S, k, lane);
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
    const double v = wave_sum_of_slices(work, S, 0, threadIdx.x);
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

// grid-stride over units, one unit (16 bytes of each plane) per thread and trip; GRAD is built from the state on the device
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

int check_planes(const char* who, const void* a, const void* b, int dtype, size_t n) {
    if (!a || !b) return fail("%s: null input plane", who);
    if (n < 1) return fail("%s: n must be at least 1", who);
    if (dtype != CSPN_F32)
        return fail("%s: unsupported dtype %d, fp32 only: the gradient of a mean over ~1e6 pixels is below what fp16 can hold "
                    "(include/cspn_criterion.h)", who, dtype);
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3)
        return fail("%s: the input planes are not aligned to their element size", who);
    return 1;
}

int check_forward(const char* who, const void* work, const void* state) {
    if (!work || !state) return fail("%s: null work / state", who);
    if (reinterpret_cast<uintptr_t>(work) & 7 || reinterpret_cast<uintptr_t>(state) & 7)
        return fail("%s: work / state must be 8-byte aligned", who);
    return 1;
}

int check_backward(const char* who, const void* state, const float* grad_loss, const void* grad) {
    if (!state || !grad_loss || !grad) return fail("%s: null state / grad_loss / gradient plane", who);
    if (reinterpret_cast<uintptr_t>(state) & 7) return fail("%s: state must be 8-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(grad_loss) | reinterpret_cast<uintptr_t>(grad)) & 3)
        return fail("%s: grad_loss / the gradient plane are not aligned to their element size", who);
    return 1;
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

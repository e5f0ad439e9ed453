// cspn_metrics_frame.hip — per-frame depth-metric sums and the reference's per-frame meter (libs/metrics.py:49-127:
// Result.evaluate on every frame, AverageMeter.update(n = 1) over frames) as kernels without atomics.
//
// Determinism contract: the ten doubles of a frame depend only on that frame's pixels, the dtype and pixels_per_frame.
//   * a frame is cut into UNITS of 16 bytes (4 floats / 8 halfs), unit u = pixels [u*V, u*V + V) of the frame;
//   * unit u belongs to slice (u / 256) % S, thread u % 256 of that slice's workgroup, S = frame_slices(pixels_per_frame);
//     a thread adds its units in increasing u: fp32 over a group of 4 units, groups into fp64;
//   * a workgroup adds its 256 threads by wave_sum_to_lane63 and its 4 wavefronts in wavefront order -> work[b][s][:];
//   * the second stage adds the S slices of a frame in an order that depends on S only (lane l: slices l, l + 64, ...; then the lanes).
// Whether the 16 bytes of a unit come in one load (frame base 16-byte aligned) or element by element (it is not: frames
// whose pixel count is not a multiple of V start unaligned from the second one on) changes the load instructions only:
// both fill the same registers in front of ONE copy of the arithmetic.
#include "cspn_common.hpp"

namespace {

constexpr int FRAME_THREADS = 256;     // 4 wavefronts per slice workgroup
constexpr int FRAME_GROUP = 4;         // units a thread adds in fp32 before the partial goes to fp64 (16 / 32 pixels)
constexpr int FRAME_MAX_SLICES = 1024;

// Slices (workgroups) per frame: a function of pixels_per_frame ONLY — one slice per 1024 four-pixel quads (a thread then sees
// ~4 units), so one 1216 x 352 frame alone spreads over 105 workgroups and a 304 x 228 one over 17.
inline int frame_slices(size_t ppf) {
    const size_t quads = (ppf + 3) / 4;
    size_t s = (quads + FRAME_THREADS * FRAME_GROUP - 1) / (FRAME_THREADS * FRAME_GROUP);
    if (s < 1) s = 1;
    if (s > FRAME_MAX_SLICES) s = FRAME_MAX_SLICES;
    return (int)s;
}

template <typename DT> struct FrameUnit;
template <> struct FrameUnit<float> {
    static constexpr int V = 4;
    __device__ static void load16(const float* p, float (&v)[4]) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    }
};
template <> struct FrameUnit<__half> {
    static constexpr int V = 8;
    __device__ static void load16(const __half* p, float (&v)[8]) {
        const uint4 raw = *reinterpret_cast<const uint4*>(p);
        const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&raw.x));
        const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&raw.y));
        const float2 c = __half22float2(*reinterpret_cast<const __half2*>(&raw.z));
        const float2 d = __half22float2(*reinterpret_cast<const __half2*>(&raw.w));
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y; v[4] = c.x; v[5] = c.y; v[6] = d.x; v[7] = d.y;
    }
};

// grid (S, B): workgroup (s, b) -> work[b][s][0..9]
template <typename DT>
__global__ __launch_bounds__(FRAME_THREADS) void cspn_metrics_frame_kernel(const DT* __restrict__ pred, const DT* __restrict__ target,
                                                                           size_t ppf, double* __restrict__ work) {
    constexpr int V = FrameUnit<DT>::V;
    const int S = gridDim.x, s = blockIdx.x, b = blockIdx.y;
    const DT* __restrict__ fp = pred + (size_t)b * ppf;
    const DT* __restrict__ ft = target + (size_t)b * ppf;
    // workgroup-uniform: one 16-byte load per unit and plane, or V element loads of the same pixels
    const bool vec = (((uintptr_t)fp | (uintptr_t)ft) & 15) == 0;
    const size_t nu = (ppf + V - 1) / V;                                 // units of this frame, the last one may be partial
    const size_t stride = (size_t)S * FRAME_THREADS;
    double acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (size_t u0 = (size_t)s * FRAME_THREADS + threadIdx.x; u0 < nu; u0 += FRAME_GROUP * stride) {
        float f[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) f[k] = 0.f;
#pragma unroll
        for (int j = 0; j < FRAME_GROUP; ++j) {
            const size_t u = u0 + (size_t)j * stride;
            if (u < nu) {
                const size_t p0 = u * V;
                float o[V], t[V];
                if (vec && p0 + V <= ppf) {
                    FrameUnit<DT>::load16(fp + p0, o);
                    FrameUnit<DT>::load16(ft + p0, t);
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        // past the frame's end: an invalid pixel (adds exactly 0 to every sum, as any target <= 0 does)
                        const bool in = p0 + e < ppf;
                        o[e] = in ? ld1(fp + p0 + e) : 1.f;
                        t[e] = in ? ld1(ft + p0 + e) : 0.f;
                    }
                }
#pragma unroll
                for (int e = 0; e < V; ++e) metric_terms(o[e], t[e], f);
            }
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) acc[k] += (double)f[k];
    }
    // wavefront sum by DPP (all 64 lanes are here: the loops above have rejoined), then the 4 wavefronts in order
    __shared__ double part[FRAME_THREADS / 64][10];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const double v = wave_sum_to_lane63(acc[k]);
        if (lane == 63) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        double v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < FRAME_THREADS / 64; ++w) v += part[w][threadIdx.x];
        work[((size_t)b * S + s) * 10 + threadIdx.x] = v;
    }
}

// One workgroup per frame, one wavefront per quantity: lane l adds slices l, l + 64, ... in increasing order, the 64 lane sums go
// through wave_sum_to_lane63 -> sums[b][k] (overwritten).  The order is a function of S, i.e. of pixels_per_frame, only; a single
// thread walking S dependent loads took 16 us for the 105 slices of one 1216 x 352 frame.
constexpr int COMBINE_THREADS = 640;
__global__ __launch_bounds__(COMBINE_THREADS) void cspn_metrics_frame_combine_kernel(const double* __restrict__ work, int S,
                                                                                      double* __restrict__ sums) {
    const int b = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* w = work + (size_t)b * S * 10 + k;
    double v = 0.0;
    for (int s = lane; s < S; s += 64) v += w[(size_t)s * 10];
    v = wave_sum_to_lane63(v);
    if (lane == 63) sums[(size_t)b * 10 + k] = v;
}

// Result.evaluate of every frame (libs/metrics.py:49-83) + AverageMeter.update(result, n = 1) (:101-127), frames in index order.
// One workgroup.  The divisions and square roots of 64 frames at a time run in parallel (16 threads per frame: the ten metrics,
// 1 for the frame count, n for the valid-pixel count) into LDS; threads 0..11 then add their column frame by frame, so the state
// is the same sequence of additions however the frames were cut into batches.
constexpr int METER_THREADS = 1024, METER_CHUNK = METER_THREADS / 16;
__global__ __launch_bounds__(METER_THREADS) void cspn_meter_update_kernel(const double* __restrict__ sums, int B, double* __restrict__ meter) {
    __shared__ double val[METER_CHUNK][12];
    const int tid = threadIdx.x, fl = tid >> 4, k = tid & 15;
    double m = tid < 12 ? meter[tid] : 0.0;
    for (int base = 0; base < B; base += METER_CHUNK) {
        const int b = base + fl;
        if (b < B && k < 12) {
            // metric k is sums[src] / n, square-rooted for irmse (0) and rmse (3); a frame without a valid pixel gives 0 / 0 = NaN,
            // as the reference's mean over an empty selection does, and the NaN stays in the meter
            const double n = sums[(size_t)b * 10 + 9];
            double v;
            if (k == 10) {
                v = 1.0;
            } else if (k == 11) {
                v = n;
            } else {
                const double q = sums[(size_t)b * 10 + (k < 3 ? k : k - 1)] / n;
                v = (k == 0 || k == 3) ? sqrt(q) : q;
            }
            val[fl][k] = v;
        }
        __syncthreads();
        if (tid < 12) {
            const int cnt = B - base < METER_CHUNK ? B - base : METER_CHUNK;
            for (int i = 0; i < cnt; ++i) m += val[i][tid];
        }
        __syncthreads();
    }
    if (tid < 12) meter[tid] = m;
}

}  // namespace

extern "C" {

size_t cspn_metrics_per_frame_workspace_bytes(int B, size_t pixels_per_frame) {
    if (B < 1 || pixels_per_frame < 1) return 0;
    return (size_t)B * frame_slices(pixels_per_frame) * 10 * sizeof(double);
}

int cspn_metrics_per_frame(const void* pred, const void* target, int dtype, int B, size_t pixels_per_frame, void* work,
                           double* sums, cspn_stream_t stream) {
    if (!pred || !target || !work || !sums || B < 1 || pixels_per_frame < 1) return fail("cspn_metrics_per_frame: bad arguments");
    if (B > 65535) return fail("cspn_metrics_per_frame: B = %d exceeds the 65535 frames of one launch", B);
    if (dtype != CSPN_F32 && dtype != CSPN_F16) return fail("cspn_metrics_per_frame: unsupported dtype %d", dtype);
    if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & (esize(dtype) - 1))
        return fail("cspn_metrics_per_frame: pred / target are not aligned to their element size");
    if (reinterpret_cast<uintptr_t>(work) & 7 || reinterpret_cast<uintptr_t>(sums) & 7)
        return fail("cspn_metrics_per_frame: work / sums must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = frame_slices(pixels_per_frame);
    double* w = static_cast<double*>(work);
    if (dtype == CSPN_F32)
        hipLaunchKernelGGL((cspn_metrics_frame_kernel<float>), dim3(S, B), dim3(FRAME_THREADS), 0, st,
                           static_cast<const float*>(pred), static_cast<const float*>(target), pixels_per_frame, w);
    else
        hipLaunchKernelGGL((cspn_metrics_frame_kernel<__half>), dim3(S, B), dim3(FRAME_THREADS), 0, st,
                           static_cast<const __half*>(pred), static_cast<const __half*>(target), pixels_per_frame, w);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(cspn_metrics_frame_combine_kernel, dim3(B), dim3(COMBINE_THREADS), 0, st, static_cast<const double*>(w), S, sums);
    HIP_OK(hipGetLastError());
    return 1;
}

int cspn_meter_update(const double* sums, int B, double* meter, cspn_stream_t stream) {
    if (!sums || !meter || B < 1) return fail("cspn_meter_update: bad arguments");
    hipLaunchKernelGGL(cspn_meter_update_kernel, dim3(1), dim3(METER_THREADS), 0, static_cast<hipStream_t>(stream), sums, B, meter);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

// cspn_sparsify.hip — the reference's sparse-depth sampler (dataloaders/nyu_dataloader/dense_to_sparse.py:27-52 UniformSampling,
// "uar") and its RGB-D assembly (dataloader.py:85-97 create_sparse_depth / create_rgbd) for a batch of frames on the device
// (include/cspn_sparsify.h): a count pass and an apply pass, no atomics, no wait between workgroups, nothing read back.
//
// Both kernels are streaming and wave64: 256 threads, a thread moves UNITS of 4 pixels of one frame, 16 bytes per fp32 plane
// where that plane of that frame starts 16-byte aligned and element by element where it does not (HW % 4 != 0 puts every other
// frame there).  The choice is workgroup-uniform — blockIdx.y is the frame — and changes the load / store instructions only: both
// forms fill the same registers in front of ONE copy of the predicate, so they give the same bits.
//
// Every pixel index is checked against HW before its load and before its store; the partial last unit of a frame always goes
// element by element.
#include "cspn_common.hpp"
#include "cspn_philox.hpp"
#include "cspn_sparsify.h"

namespace {

constexpr int SP_THREADS = 256;                 // 4 wavefronts; also the size of the uint8 -> float table of the apply pass
constexpr int SP_APPLY_MAX_GRID_X = 256;        // workgroups per frame of the apply pass; larger frames grid-stride
static_assert(SP_THREADS * 4 == CSPN_SPARSIFY_SLICE_PIXELS, "a slice is one trip of a 256-thread workgroup");

struct SparsifyArgs {
    const float* depth;
    const void* uniform;
    const long long* frame_ids;
    const unsigned* work;
    float* sparse;
    const void* rgb;
    float* rgb_out;
    unsigned char* mask;
    size_t HW;
    long sparse_bs, rgb_out_bs, rgb_out_cs;
    double num_samples;
    unsigned long long seed;
    float max_depth;
    int S, dense;
};

__device__ __forceinline__ bool aligned_to(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

// dense_to_sparse.py:44-46.  A NaN depth fails `> 0`, a NaN max_depth fails everything, +inf cuts nothing.
__device__ __forceinline__ bool keep_pixel(float d, float max_depth) { return d > 0.f && d <= max_depth; }

// pixels [p0, p0 + 4) of one fp32 plane of one frame; past the end of the frame: `pad`
__device__ __forceinline__ void load_unit_f32(const float* __restrict__ plane, size_t p0, size_t HW, bool vec, float pad, float (&v)[4]) {
    if (vec && p0 + 4 <= HW) {
        const float4 a = ld4(plane + p0);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p0 + e < HW ? ld1(plane + p0 + e) : pad;
    }
}
__device__ __forceinline__ void store_unit_f32(float* __restrict__ plane, size_t p0, size_t HW, bool vec, const float (&v)[4]) {
    if (vec && p0 + 4 <= HW) {
        st4(plane + p0, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p0 + e < HW) st1(plane + p0 + e, v[e]);
    }
}

// grid (S, B): work[b * S + s] = kept pixels of the units q of frame b with (q / 256) % S == s
__global__ __launch_bounds__(SP_THREADS) void cspn_sparsify_count_kernel(const float* __restrict__ depth, size_t HW, float max_depth,
                                                                         unsigned* __restrict__ work) {
    const int S = gridDim.x, s = blockIdx.x, b = blockIdx.y;
    const float* frame = depth + (size_t)b * HW;
    const bool vec = aligned_to(frame, 15);
    const size_t nq = (HW + 3) / 4;
    unsigned n = 0;
    for (size_t q = (size_t)s * SP_THREADS + threadIdx.x; q < nq; q += (size_t)S * SP_THREADS) {
        float d[4];
        load_unit_f32(frame, q * 4, HW, vec, 0.f, d);
#pragma unroll
        for (int e = 0; e < 4; ++e) n += keep_pixel(d[e], max_depth) ? 1u : 0u;
    }
    // counts below 2^32 are exact in fp64: the wavefront sum by DPP (all 64 lanes are here: the loop has rejoined)
    __shared__ double part[SP_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double v = wave_sum_to_lane63((double)n);
    if (lane == 63) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) work[(size_t)b * S + s] = (unsigned)(part[0] + part[1] + part[2] + part[3]);
}

// grid (G, B), grid-stride over the units of frame blockIdx.y.  UK: where u comes from, RK: the form of the RGB planes.
template <int UK, int RK>
__global__ __launch_bounds__(SP_THREADS) void cspn_sparsify_apply_kernel(SparsifyArgs a) {
    const int b = blockIdx.y;
    const size_t HW = a.HW;
    __shared__ double s_prob;
    __shared__ float lut[RK == CSPN_RGB_U8 ? SP_THREADS : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if constexpr (RK == CSPN_RGB_U8) lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);     // nyu_dataloader.py:29 + ToTensor's .float()
    if (wave == 0) {
        // lane l takes partial l (S <= 64), the 64 lanes go through one fixed tree; integers, so any order gives this sum
        double n_keep = 0.0;
        if (!a.dense && lane < a.S) n_keep = (double)a.work[(size_t)b * a.S + lane];
        n_keep = wave_sum_to_lane63(n_keep);
        if (lane == 63) s_prob = n_keep > 0.0 ? a.num_samples / n_keep : 0.0;           // dense_to_sparse.py:51
    }
    __syncthreads();
    const double prob = s_prob;
    const bool dense = a.dense != 0;
    const float max_depth = a.max_depth;

    const float* dframe = a.depth + (size_t)b * HW;
    const bool vec_d = aligned_to(dframe, 15);
    const float* u32 = UK == CSPN_UNIFORM_F32 ? static_cast<const float*>(a.uniform) + (size_t)b * HW : nullptr;
    const double* u64 = UK == CSPN_UNIFORM_F64 ? static_cast<const double*>(a.uniform) + (size_t)b * HW : nullptr;
    const bool vec_u = aligned_to(UK == CSPN_UNIFORM_F32 ? (const void*)u32 : (const void*)u64, 15);
    unsigned fid_lo = 0u, fid_hi = 0u;
    if (UK == CSPN_UNIFORM_PHILOX && !dense) {
        const unsigned long long fid = (unsigned long long)a.frame_ids[b];
        fid_lo = (unsigned)fid;
        fid_hi = (unsigned)(fid >> 32);
    }
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
    float* sframe = a.sparse ? a.sparse + (ptrdiff_t)b * a.sparse_bs : nullptr;
    const bool vec_s = aligned_to(sframe, 15);
    unsigned char* mframe = a.mask ? a.mask + (size_t)b * HW : nullptr;
    const bool vec_m = aligned_to(mframe, 3);
    const float* rin32[3] = {nullptr, nullptr, nullptr};
    const unsigned char* rin8[3] = {nullptr, nullptr, nullptr};
    float* rout[3] = {nullptr, nullptr, nullptr};
    bool vec_ri[3] = {false, false, false}, vec_ro[3] = {false, false, false};
    if (RK != CSPN_RGB_NONE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const size_t off = ((size_t)b * 3 + c) * HW;
            if (RK == CSPN_RGB_F32) {
                rin32[c] = static_cast<const float*>(a.rgb) + off;
                vec_ri[c] = aligned_to(rin32[c], 15);
            } else {
                rin8[c] = static_cast<const unsigned char*>(a.rgb) + off;
                vec_ri[c] = aligned_to(rin8[c], 3);
            }
            rout[c] = a.rgb_out + (ptrdiff_t)b * a.rgb_out_bs + (ptrdiff_t)c * a.rgb_out_cs;
            vec_ro[c] = aligned_to(rout[c], 15);
        }
    }

    const size_t nq = (HW + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * SP_THREADS + threadIdx.x; q < nq; q += (size_t)gridDim.x * SP_THREADS) {
        const size_t p0 = q * 4;
        const bool full = p0 + 4 <= HW;
        // every load of the unit first, then the predicate, then the stores
        float d[4];
        load_unit_f32(dframe, p0, HW, vec_d, 0.f, d);
        double u[4] = {1.0, 1.0, 1.0, 1.0};
        if (!dense) {
            if (UK == CSPN_UNIFORM_F32) {
                float uf[4];
                load_unit_f32(u32, p0, HW, vec_u, 1.f, uf);
#pragma unroll
                for (int e = 0; e < 4; ++e) u[e] = (double)uf[e];
            } else if (UK == CSPN_UNIFORM_F64) {
                if (vec_u && full) {
                    const double2 lo = *reinterpret_cast<const double2*>(u64 + p0), hi = *reinterpret_cast<const double2*>(u64 + p0 + 2);
                    u[0] = lo.x; u[1] = lo.y; u[2] = hi.x; u[3] = hi.y;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (p0 + e < HW) u[e] = u64[p0 + e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) u[e] = philox_uniform<0u>((unsigned)(p0 + e), fid_lo, fid_hi, k0, k1);
            }
        }
        float rgb[3][4];
        if constexpr (RK == CSPN_RGB_F32) {
#pragma unroll
            for (int c = 0; c < 3; ++c) load_unit_f32(rin32[c], p0, HW, vec_ri[c], 0.f, rgb[c]);
        } else if constexpr (RK == CSPN_RGB_U8) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned w = 0u;
                if (vec_ri[c] && full) {
                    w = *reinterpret_cast<const unsigned*>(rin8[c] + p0);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (p0 + e < HW) w |= (unsigned)rin8[c][p0 + e] << (8 * e);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) rgb[c][e] = lut[(w >> (8 * e)) & 255u];
            }
        }

        bool m[4];
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[e] = dense || (keep_pixel(d[e], max_depth) && u[e] < prob);      // dense_to_sparse.py:52
            o[e] = m[e] ? d[e] : 0.f;                                          // dataloader.py:90-91: a copy or +0
        }

        if (sframe) store_unit_f32(sframe, p0, HW, vec_s, o);
        if (mframe) {
            if (vec_m && full) {
                *reinterpret_cast<unsigned*>(mframe + p0) = (m[0] ? 1u : 0u) | (m[1] ? 0x100u : 0u) | (m[2] ? 0x10000u : 0u) | (m[3] ? 0x1000000u : 0u);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (p0 + e < HW) mframe[p0 + e] = m[e] ? 1 : 0;
            }
        }
        if (RK != CSPN_RGB_NONE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) store_unit_f32(rout[c], p0, HW, vec_ro[c], rgb[c]);
        }
    }
}

template <int UK>
void launch_apply(int rgb_kind, dim3 grid, hipStream_t st, const SparsifyArgs& a) {
    if (rgb_kind == CSPN_RGB_F32)
        hipLaunchKernelGGL((cspn_sparsify_apply_kernel<UK, CSPN_RGB_F32>), grid, dim3(SP_THREADS), 0, st, a);
    else if (rgb_kind == CSPN_RGB_U8)
        hipLaunchKernelGGL((cspn_sparsify_apply_kernel<UK, CSPN_RGB_U8>), grid, dim3(SP_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((cspn_sparsify_apply_kernel<UK, CSPN_RGB_NONE>), grid, dim3(SP_THREADS), 0, st, a);
}

inline bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

}  // namespace

extern "C" {

int cspn_sparsify_abi_version(void) { return CSPN_SPARSIFY_ABI_VERSION; }

int cspn_sparsify_slices(size_t HW) {
    size_t s = (HW + CSPN_SPARSIFY_SLICE_PIXELS - 1) / CSPN_SPARSIFY_SLICE_PIXELS;
    if (s < 1) s = 1;
    if (s > CSPN_SPARSIFY_MAX_SLICES) s = CSPN_SPARSIFY_MAX_SLICES;
    return (int)s;
}

size_t cspn_sparsify_workspace_bytes(int B, size_t HW) {
    if (B < 1 || HW < 1) return 0;
    return (size_t)B * cspn_sparsify_slices(HW) * sizeof(unsigned);
}

int cspn_sparsify(const void* depth, int dtype, int B, int H, int W, int mode, long long num_samples, float max_depth,
                  const void* uniform, int uniform_kind, const long long* frame_ids, unsigned long long seed,
                  void* sparse, long sparse_batch_stride,
                  const void* rgb, int rgb_kind, void* rgb_out, long rgb_out_batch_stride, long rgb_out_channel_stride,
                  unsigned char* mask, void* work, cspn_stream_t stream) {
    const char* who = "cspn_sparsify";
    if (!depth) return fail("%s: null depth", who);
    if (dtype != CSPN_F32)
        return fail("%s: unsupported dtype %d, fp32 only: a sparse sample is a copy of the measured depth, and the reference's depth is "
                    "fp32 (include/cspn_sparsify.h)", who, dtype);
    if (B < 1 || B > 65535 || H < 1 || W < 1) return fail("%s: bad size B=%d H=%d W=%d (1 <= B <= 65535)", who, B, H, W);
    const size_t HW = (size_t)H * (size_t)W;
    if (HW >= ((size_t)1 << 32)) return fail("%s: H * W must be below 2^32", who);
    if (mode != CSPN_SPARSIFY_UAR && mode != CSPN_SPARSIFY_DENSE) return fail("%s: unknown mode %d", who, mode);
    if (misaligned(depth, 3)) return fail("%s: depth is not aligned to its element size", who);
    const bool dense = mode == CSPN_SPARSIFY_DENSE;
    if (uniform_kind != CSPN_UNIFORM_PHILOX && uniform_kind != CSPN_UNIFORM_F32 && uniform_kind != CSPN_UNIFORM_F64)
        return fail("%s: unknown uniform_kind %d", who, uniform_kind);
    if (!dense) {
        if (uniform_kind == CSPN_UNIFORM_PHILOX) {
            if (!frame_ids) return fail("%s: CSPN_UNIFORM_PHILOX needs frame_ids", who);
            if (misaligned(frame_ids, 7)) return fail("%s: frame_ids must be 8-byte aligned", who);
        } else {
            if (!uniform) return fail("%s: null uniform plane", who);
            if (misaligned(uniform, uniform_kind == CSPN_UNIFORM_F64 ? 7 : 3)) return fail("%s: uniform is not aligned to its element size", who);
        }
        if (!work) return fail("%s: null work", who);
        if (misaligned(work, 3)) return fail("%s: work must be 4-byte aligned", who);
    }
    if (!sparse && !mask) return fail("%s: needs a sparse or a mask output", who);
    if (sparse) {
        if (misaligned(sparse, 3)) return fail("%s: sparse is not aligned to its element size", who);
        if (B > 1 && (sparse_batch_stride < 0 || (size_t)sparse_batch_stride < HW)) return fail("%s: sparse_batch_stride below H * W", who);
    }
    if (rgb_kind != CSPN_RGB_NONE && rgb_kind != CSPN_RGB_F32 && rgb_kind != CSPN_RGB_U8) return fail("%s: unknown rgb_kind %d", who, rgb_kind);
    if (rgb_kind != CSPN_RGB_NONE) {
        if (!rgb || !rgb_out) return fail("%s: null rgb / rgb_out", who);
        if ((rgb_kind == CSPN_RGB_F32 && misaligned(rgb, 3)) || misaligned(rgb_out, 3)) return fail("%s: rgb / rgb_out are not aligned to their element size", who);
        if (rgb_out_channel_stride < 0 || (size_t)rgb_out_channel_stride < HW) return fail("%s: rgb_out_channel_stride below H * W", who);
        if (B > 1 && (rgb_out_batch_stride < 0 || (size_t)rgb_out_batch_stride < HW)) return fail("%s: rgb_out_batch_stride below H * W", who);
    }

    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = cspn_sparsify_slices(HW);
    if (!dense) {
        hipLaunchKernelGGL(cspn_sparsify_count_kernel, dim3(S, B), dim3(SP_THREADS), 0, st, static_cast<const float*>(depth), HW, max_depth,
                           static_cast<unsigned*>(work));
        HIP_OK(hipGetLastError());
    }
    SparsifyArgs a;
    a.depth = static_cast<const float*>(depth);
    a.uniform = uniform;
    a.frame_ids = frame_ids;
    a.work = static_cast<const unsigned*>(work);
    a.sparse = static_cast<float*>(sparse);
    a.rgb = rgb_kind != CSPN_RGB_NONE ? rgb : nullptr;
    a.rgb_out = rgb_kind != CSPN_RGB_NONE ? static_cast<float*>(rgb_out) : nullptr;
    a.mask = mask;
    a.HW = HW;
    a.sparse_bs = sparse_batch_stride;
    a.rgb_out_bs = rgb_out_batch_stride;
    a.rgb_out_cs = rgb_out_channel_stride;
    a.num_samples = (double)num_samples;
    a.seed = seed;
    a.max_depth = max_depth;
    a.S = S;
    a.dense = dense ? 1 : 0;
    const size_t nq = (HW + 3) / 4;
    size_t gx = (nq + SP_THREADS - 1) / SP_THREADS;
    if (gx > SP_APPLY_MAX_GRID_X) gx = SP_APPLY_MAX_GRID_X;
    const dim3 grid((unsigned)gx, (unsigned)B);
    if (dense || uniform_kind == CSPN_UNIFORM_PHILOX)
        launch_apply<CSPN_UNIFORM_PHILOX>(rgb_kind, grid, st, a);
    else if (uniform_kind == CSPN_UNIFORM_F32)
        launch_apply<CSPN_UNIFORM_F32>(rgb_kind, grid, st, a);
    else
        launch_apply<CSPN_UNIFORM_F64>(rgb_kind, grid, st, a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

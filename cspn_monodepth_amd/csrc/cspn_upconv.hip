// cspn_upconv.hip — the head of a decoder block fused with its un-pooling (include/cspn_upconv.h).
//
// The computation, the decomposition into four phases, the kernels and the argument checks are those of cspn_upconv_core.hpp; here is
// the fp32 form of a chunk.
//   pack  wp[25 taps, phase-major][Cp][Mp] fp32: filter-contiguous, a row of the chunk is TM consecutive floats
//   fwd   the filter chunk [KC][TM] and the gathered pixels [KC][TN] go through LDS as they are loaded: a thread fetches 4 x 16 bytes of
//         the filter chunk (rows (t >> 5) + 8 r) and pixel t & 127 of the channels (t >> 7) + 2 r, consecutive lanes on consecutive
//         pixels of a row.  v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31], so a step reads two rows
//         of each tile.  Exact fp32 products.
// fp32 only.
#include "cspn_upconv_core.hpp"
#include "cspn_upconv.h"

namespace {

struct F32 {
    using T = float;
    using ATile = float[KC][TM];
    using BTile = float[KC][TN];
    struct Chunk {
        v4f wv[4];
        float xv[16];
    };
    static constexpr bool CHANNEL_INNER = false;

    static __device__ __forceinline__ const float* wtile(const Args<float>& a, int mt, int t) {
        return a.wp + (size_t)mt * TM + (size_t)(t >> 5) * a.Mp + 4 * (t & 31);
    }
    static __device__ __forceinline__ void load(Chunk& k, const Args<float>& a, const float* wt, const float* xt, int c0, int t, bool there,
                                                size_t hw) {
        const int kb = t >> 7;
#pragma unroll
        for (int r = 0; r < 4; ++r) k.wv[r] = *reinterpret_cast<const v4f*>(wt + (size_t)(c0 + 8 * r) * a.Mp);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = c0 + kb + 2 * r;
            k.xv[r] = (there && c < a.C) ? xt[(size_t)c * hw] : 0.f;
        }
    }
    static __device__ __forceinline__ void stage(ATile& As, BTile& Bs, const Chunk& k, int t) {
        const int kb = t >> 7;
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<v4f*>(&As[(t >> 5) + 8 * r][4 * (t & 31)]) = k.wv[r];
#pragma unroll
        for (int r = 0; r < 16; ++r) Bs[kb + 2 * r][t & 127] = k.xv[r];
    }
    static __device__ __forceinline__ void products(const ATile& As, const BTile& Bs, v16f (&acc)[2][2], int wm, int wn, int l31, int lh) {
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const int kk = 2 * s + lh;
            const float a0 = As[kk][wm * 64 + l31], a1 = As[kk][wm * 64 + 32 + l31];
            const float b0 = Bs[kk][wn * 64 + l31], b1 = Bs[kk][wn * 64 + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
};

}  // namespace

extern "C" {

int cspn_upconv_abi_version(void) { return CSPN_UPCONV_ABI_VERSION; }

size_t cspn_upconv_workspace_bytes(int out_channels, int C) { return packed_elems(out_channels, C) * sizeof(float); }

int cspn_upconv_pack(const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, int dtype, void* packed,
                     cspn_stream_t stream) {
    const char* who = "cspn_upconv_pack";
    if (dtype != CSPN_F32) return fail("%s: fp32 only", who);
    int O0 = 0, M = 0;
    size_t elems = 0;
    if (!check_pack(who, weights, out_channels, n_filters, C, kh, kw, packed, CSPN_UPCONV_MAX_FILTERS, O0, M, elems)) return 0;
    return launch_pack<float, F32>(weights, n_filters, packed, O0, M, C, elems, stream);
}

int cspn_upconv_forward(const void* x, int dtype, const void* packed, const void* scale, const void* shift, int relu_channels,
                        void* const* outs, const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow,
                        cspn_stream_t stream) {
    const char* who = "cspn_upconv_forward";
    if (dtype != CSPN_F32) return fail("%s: fp32 only", who);
    return forward<F32>(who, x, packed, scale, shift, relu_channels, outs, out_channels, n_outs, N, C, H, W, oh, ow, CSPN_UPCONV_MAX_FILTERS,
                        stream);
}

}  // extern "C"

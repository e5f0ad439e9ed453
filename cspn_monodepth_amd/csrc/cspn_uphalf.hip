// cspn_uphalf.hip — the head of a decoder block fused with its un-pooling, in half precision (include/cspn_uphalf.h).
//
// The computation, the decomposition into four phases, the kernels and the argument checks are those of cspn_upconv_core.hpp; here is
// the fp16 form of a chunk.
//   pack  wp[25 taps, phase-major][Mp][Cp] fp16, from fp32 (rounded to nearest even) or fp16 filters.  Channel-contiguous: the 8 channels
//         lane l of v_mfma_f32_32x32x16_f16 holds of row l & 31 (A[l & 31][8 (l >> 5) + j]) are 16 consecutive bytes.
//   fwd   a chunk is two blocks of 16 channels.  The filter chunk [TM][KC] and the gathered pixels [TN][KC] go through LDS, both
//         channel-contiguous with rows of 80 bytes (64 of data + 16 of padding): the 16 lanes a ds_read_b128 serves in one cycle then
//         start at 20 l mod 64 banks, all different, so the operand reads are conflict-free without a swizzle.  A thread fetches
//         2 x 16 bytes of the filter chunk (rows (t >> 2) + 64 r, fragment t & 3) and pixel t & 127 of the channel groups of 8
//         (t >> 7) + 2 r.  The NCHW gather is 2-byte loads, consecutive lanes on consecutive pixels of a row (pairs are not formed: the
//         column offset of a tap and the row length make half of them misaligned).  fp32 accumulation, one rounding of the result.
#include "cspn_upconv_core.hpp"
#include "cspn_uphalf.h"

namespace {

constexpr int ROW8 = KC / 8 + 1;          // an LDS row in 16-byte fragments: 4 of data, 1 of padding

typedef _Float16 v8h __attribute__((ext_vector_type(8)));

struct F16 {
    using T = _Float16;
    using ATile = v8h[TM][ROW8];
    using BTile = v8h[TN][ROW8];
    struct Chunk {
        v8h wv[2];
        _Float16 xv[2][8];      // scalars: the two 16-byte vectors are formed in stage(), behind the barrier, not in front of it
    };
    static constexpr bool CHANNEL_INNER = true;

    static __device__ __forceinline__ const _Float16* wtile(const Args<_Float16>& a, int mt, int t) {
        return a.wp + ((size_t)mt * TM + (t >> 2)) * a.Cp + 8 * (t & 3);
    }
    static __device__ __forceinline__ void load(Chunk& k, const Args<_Float16>& a, const _Float16* wt, const _Float16* xt, int c0, int t,
                                                bool there, size_t hw) {
        const int cb = c0 + 8 * (t >> 7);      // c = cb + a constant, one add: known not to wrap, c * hw needs no sign extension
#pragma unroll
        for (int r = 0; r < 2; ++r) k.wv[r] = *reinterpret_cast<const v8h*>(wt + (size_t)(64 * r) * a.Cp + c0);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = cb + 16 * r + j;
                k.xv[r][j] = (there && c < a.C) ? xt[(size_t)c * hw] : (_Float16)0.f;
            }
    }
    static __device__ __forceinline__ void stage(ATile& As, BTile& Bs, const Chunk& k, int t) {
        const int px = t & 127, kb = t >> 7, wrow = t >> 2, wseg = t & 3;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            As[wrow + 64 * r][wseg] = k.wv[r];
            v8h xv;
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = k.xv[r][j];
            Bs[px][kb + 2 * r] = xv;
        }
    }
    static __device__ __forceinline__ void products(const ATile& As, const BTile& Bs, v16f (&acc)[2][2], int wm, int wn, int l31, int lh) {
#pragma unroll
        for (int s = 0; s < KC / 16; ++s) {
            const int f = 2 * s + lh;                        // channels 16 s + 8 (lane >> 5) .. + 7
            const v8h a0 = As[wm * 64 + l31][f], a1 = As[wm * 64 + 32 + l31][f];
            const v8h b0 = Bs[wn * 64 + l31][f], b1 = Bs[wn * 64 + 32 + l31][f];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
};

}  // namespace

extern "C" {

int cspn_uphalf_abi_version(void) { return CSPN_UPHALF_ABI_VERSION; }

size_t cspn_uphalf_packed_bytes(int out_channels, int C) { return packed_elems(out_channels, C) * sizeof(_Float16); }

int cspn_uphalf_pack(const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, int src_dtype,
                     void* packed, cspn_stream_t stream) {
    const char* who = "cspn_uphalf_pack";
    if (src_dtype != CSPN_F32 && src_dtype != CSPN_F16) return fail("%s: the filters must be fp32 or fp16, got dtype %d", who, src_dtype);
    int O0 = 0, M = 0;
    size_t elems = 0;
    if (!check_pack(who, weights, out_channels, n_filters, C, kh, kw, packed, CSPN_UPHALF_MAX_FILTERS, O0, M, elems)) return 0;
    return src_dtype == CSPN_F32 ? launch_pack<float, F16>(weights, n_filters, packed, O0, M, C, elems, stream)
                                 : launch_pack<_Float16, F16>(weights, n_filters, packed, O0, M, C, elems, stream);
}

int cspn_uphalf_forward(const void* x, const void* packed, const void* scale, const void* shift, int relu_channels, void* const* outs,
                        const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream) {
    return forward<F16>("cspn_uphalf_forward", x, packed, scale, shift, relu_channels, outs, out_channels, n_outs, N, C, H, W, oh, ow,
                        CSPN_UPHALF_MAX_FILTERS, stream);
}

}  // extern "C"

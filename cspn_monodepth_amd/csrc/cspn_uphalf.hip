// cspn_uphalf.hip — the head of a decoder block fused with its un-pooling, in half precision (include/cspn_uphalf.h).
//
// The computation and the decomposition are those of cspn_upconv.hip: output pixel (2i + a, 2j + b) of a pad-2 5x5 window over the
// un-pooled map meets the compact map through the taps with a + ky and b + kx even — 9, 6, 6, 4 taps for the phases (0,0), (0,1), (1,0),
// (1,1) — and each phase is an implicit GEMM: M = flat channels, N = the phase's pixels over the whole batch, K = (tap, channel).
//   uphalf_pack  the filters -> wp[25 taps, phase-major][Mp][Cp] fp16: tap t of phase p, flat output channel m, channel c; Mp = the flat
//                channels rounded up to TM, Cp = C rounded up to KC, zero-filled.  Channel-contiguous: the 8 channels lane l of
//                v_mfma_f32_32x32x16_f16 holds of row l & 31 (A[l & 31][8 (l >> 5) + j]) are 16 consecutive bytes.
//   uphalf_fwd   a workgroup of 4 wavefronts owns a TM x TN = 128 x 128 tile and walks K in chunks of KC = 32 channels of one tap (two
//                blocks of 16).  The filter chunk [TM][KC] and the gathered pixels [TN][KC] go through LDS, both channel-contiguous with
//                rows of 80 bytes (64 of data + 16 of padding): the 16 lanes a ds_read_b128 serves in one cycle then start at
//                20 l mod 64 banks, all different, so the operand reads are conflict-free without a swizzle.  A wavefront holds 2 x 2
//                accumulators (64 x 64).  Single-buffered as the fp32 kernel: the loads of a chunk are issued before the barrier that
//                ends the previous chunk's products, and several workgroups per CU cover each other's loads.  The NCHW gather is
//                2-byte loads, consecutive lanes on consecutive pixels of a row (pairs are not formed: the column offset of a tap and
//                the row length make half of them misaligned).
// An output element is one chain over K in the packed order, whatever its tile: no split-K, no atomics.
#include "cspn_common.hpp"
#include "cspn_uphalf.h"

namespace {

constexpr int TM = 128, TN = 128, KC = 32, THREADS = 256;
constexpr int TAPS = 25;
constexpr int ROW8 = KC / 8 + 1;          // an LDS row in 16-byte fragments: 4 of data, 1 of padding

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

struct Args {
    const _Float16* x;
    const _Float16* wp;
    const float* scale;       // null: no affine map
    const float* shift;
    _Float16* y0;
    _Float16* y1;
    int O0, O1, M, Mp, relu;
    int N, C, Cp, H, W, oh, ow;
    int mtiles;
    unsigned first[5];        // first workgroup of phase p (p = 2a + b), first[4] = the grid
};

// phase p = 2a + b: rows of taps, columns of taps, first tap in the packed order
__host__ __device__ constexpr int tap_rows(int p) { return (p >> 1) ? 2 : 3; }
__host__ __device__ constexpr int tap_cols(int p) { return (p & 1) ? 2 : 3; }
__host__ __device__ constexpr int tap_base(int p) { return p == 0 ? 0 : p == 1 ? 9 : p == 2 ? 15 : 21; }

__device__ __forceinline__ _Float16 to_half(float v) { return (_Float16)v; }      // round to nearest even
__device__ __forceinline__ _Float16 to_half(_Float16 v) { return v; }

// e = (packed tap, flat output channel, channel)
template <typename S>
__global__ __launch_bounds__(256) void uphalf_pack(const S* __restrict__ w0, const S* __restrict__ w1, _Float16* __restrict__ wp, int O0,
                                                   int M, int Mp, int C, int Cp, size_t elems) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    const int c = (int)(e % Cp);
    const size_t row = e / Cp;
    const int m = (int)(row % Mp), tg = (int)(row / Mp);
    const int p = tg < 9 ? 0 : tg < 15 ? 1 : tg < 21 ? 2 : 3;
    const int t = tg - tap_base(p);
    const int tr = t / tap_cols(p), tc = t - tr * tap_cols(p);
    const int ky = 2 * tr + (p >> 1), kx = 2 * tc + (p & 1);
    _Float16 v = (_Float16)0.f;
    if (m < M && c < C) {
        const S* src = m < O0 ? w0 + (size_t)m * C * 25 : w1 + (size_t)(m - O0) * C * 25;
        v = to_half(src[(size_t)c * 25 + ky * 5 + kx]);
    }
    wp[e] = v;
}

// pixel n of phase p -> frame, compact row and column
struct Pixel {
    int frame, i, j;
    bool ok;
};
__device__ __forceinline__ Pixel decode(unsigned n, unsigned npix, int Ha, int Wb) {
    Pixel q;
    q.ok = n < npix;
    const unsigned nn = q.ok ? n : 0u;
    const unsigned per = (unsigned)Ha * Wb;
    q.frame = nn / per;
    const unsigned r = nn - q.frame * per;
    q.i = r / Wb;
    q.j = r - q.i * Wb;
    return q;
}

__global__ __launch_bounds__(THREADS) void uphalf_fwd(const Args a) {
    __shared__ __attribute__((aligned(16))) v8h As[TM][ROW8];
    __shared__ __attribute__((aligned(16))) v8h Bs[TN][ROW8];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const unsigned bid = blockIdx.x;
    const int p = bid >= a.first[3] ? 3 : bid >= a.first[2] ? 2 : bid >= a.first[1] ? 1 : 0;
    const unsigned local = bid - (p == 3 ? a.first[3] : p == 2 ? a.first[2] : p == 1 ? a.first[1] : 0u);
    const int mt = local % a.mtiles;
    const unsigned nt = local / a.mtiles;
    const int pa = p >> 1, pb = p & 1;
    const int Hc = (a.oh + 1) >> 1, Wc = (a.ow + 1) >> 1;        // the compact pixels that take part
    const int Ha = (a.oh + 1 - pa) >> 1, Wb = (a.ow + 1 - pb) >> 1;      // the phase's output pixels: 2i + a < oh, 2j + b < ow
    const unsigned npix = (unsigned)a.N * Ha * Wb;
    const int ntc = tap_cols(p), ntaps = tap_rows(p) * ntc;
    const int di0 = pa ? 0 : -1, dj0 = pb ? 0 : -1;
    const size_t hw = (size_t)a.H * a.W;

    // the loads of this thread: pixel t & 127 for the channel groups of 8 (t >> 7) + 2 r of a chunk; 2 x 16 bytes of the filter chunk
    const int px = t & 127, kb = t >> 7;
    const Pixel mine = decode(nt * TN + px, npix, Ha, Wb);
    const _Float16* xpix = a.x + (size_t)mine.frame * a.C * hw + (size_t)mine.i * a.W + mine.j;
    const int wrow = t >> 2, wseg = t & 3;                      // rows wrow + 64 r, fragment wseg
    const _Float16* wtile = a.wp + ((size_t)mt * TM + wrow) * a.Cp + 8 * wseg;

    v16f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int cchunks = a.Cp / KC;
    for (int tap = 0; tap < ntaps; ++tap) {
        const int tr = tap / ntc, tc = tap - tr * ntc;
        const int di = di0 + tr, dj = dj0 + tc;
        const int ii = mine.i + di, jj = mine.j + dj;
        const bool there = mine.ok && ii >= 0 && ii < Hc && jj >= 0 && jj < Wc;
        const _Float16* xt = xpix + (long)di * a.W + dj;
        const _Float16* wt = wtile + (size_t)(tap_base(p) + tap) * a.Mp * a.Cp;
        for (int cc = 0; cc < cchunks; ++cc) {
            const int c0 = cc * KC;
            v8h wv[2], xv[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) wv[r] = *reinterpret_cast<const v8h*>(wt + (size_t)(64 * r) * a.Cp + c0);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = c0 + 8 * (kb + 2 * r) + j;
                    xv[r][j] = (there && c < a.C) ? xt[(size_t)c * hw] : (_Float16)0.f;
                }
            __syncthreads();                                     // the previous chunk has been read
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                As[wrow + 64 * r][wseg] = wv[r];
                Bs[px][kb + 2 * r] = xv[r];
            }
            __syncthreads();
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
    }

    // accumulator register r of a 32 x 32 tile: column (pixel) lane & 31, row (channel) (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const size_t plane = (size_t)a.oh * a.ow;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const Pixel q = decode(nt * TN + wn * 64 + tn * 32 + l31, npix, Ha, Wb);
        if (!q.ok) continue;
        const size_t at = (size_t)(2 * q.i + pa) * a.ow + (2 * q.j + pb);
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * TM + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= a.M) continue;
                float y = acc[tm][tn][r];
                if (a.scale) y = fmaf(y, a.scale[m], a.shift[m]);
                if (m < a.relu) y = y < 0.f ? 0.f : y;           // NaN stays NaN
                _Float16* dst = m < a.O0 ? a.y0 + ((size_t)q.frame * a.O0 + m) * plane : a.y1 + ((size_t)q.frame * a.O1 + (m - a.O0)) * plane;
                dst[at] = (_Float16)y;                           // the one rounding to fp16, to nearest even; overflow gives +-Inf
            }
        }
    }
}

inline int round_up(int v, int to) { return ceil_div(v, to) * to; }

// the packed filters: elements, or 0 for a bad size
size_t packed_elems(int M, int C) {
    if (M < 1 || C < 1 || M > (1 << 24) || C > (1 << 24)) return 0;
    const double e = (double)TAPS * round_up(C, KC) * round_up(M, TM);
    return e >= 2147483648.0 ? 0 : (size_t)e;
}

int check_filters(const char* who, const int* out_channels, int n, int& O0, int& O1) {
    if (!out_channels || n < 1 || n > CSPN_UPHALF_MAX_FILTERS) return fail("%s: between 1 and %d filters, got %d", who, CSPN_UPHALF_MAX_FILTERS, n);
    for (int k = 0; k < n; ++k)
        if (out_channels[k] < 1 || out_channels[k] > (1 << 23)) return fail("%s: filter %d has %d output channels", who, k, out_channels[k]);
    O0 = out_channels[0], O1 = n > 1 ? out_channels[1] : 0;
    return 1;
}

}  // namespace

extern "C" {

int cspn_uphalf_abi_version(void) { return CSPN_UPHALF_ABI_VERSION; }

size_t cspn_uphalf_packed_bytes(int out_channels, int C) { return packed_elems(out_channels, C) * sizeof(_Float16); }

int cspn_uphalf_pack(const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, int src_dtype,
                     void* packed, cspn_stream_t stream) {
    const char* who = "cspn_uphalf_pack";
    if (src_dtype != CSPN_F32 && src_dtype != CSPN_F16) return fail("%s: the filters must be fp32 or fp16, got dtype %d", who, src_dtype);
    if (kh != 5 || kw != 5) return fail("%s: the filters must be 5x5, got %dx%d", who, kh, kw);
    int O0 = 0, O1 = 0;
    if (!check_filters(who, out_channels, n_filters, O0, O1)) return 0;
    if (!weights || !packed) return fail("%s: null pointer", who);
    for (int k = 0; k < n_filters; ++k)
        if (!weights[k]) return fail("%s: null pointer (filter %d)", who, k);
    if (!aligned16(packed)) return fail("%s: packed must be 16-byte aligned", who);
    const int M = O0 + O1;
    const size_t elems = packed_elems(M, C);
    if (!elems) return fail("%s: bad size (%d output channels, C=%d), or a packed form of 2^31 elements or more", who, M, C);
    if ((double)out_channels[0] * C * 25 >= 2147483648.0 || (double)O1 * C * 25 >= 2147483648.0) return fail("%s: a filter of 2^31 elements or more", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((elems + 255) / 256)), block(256);
    const void* w1 = n_filters > 1 ? weights[1] : nullptr;
    _Float16* wp = static_cast<_Float16*>(packed);
    const int Mp = round_up(M, TM), Cp = round_up(C, KC);
    if (src_dtype == CSPN_F32)
        CSPN_PRE(st), uphalf_pack<float><<<grid, block, 0, st>>>(static_cast<const float*>(weights[0]), static_cast<const float*>(w1), wp, O0, M, Mp,
                                                                  C, Cp, elems);
    else
        CSPN_PRE(st), uphalf_pack<_Float16><<<grid, block, 0, st>>>(static_cast<const _Float16*>(weights[0]), static_cast<const _Float16*>(w1), wp,
                                                                     O0, M, Mp, C, Cp, elems);
    HIP_OK(hipGetLastError());
    return 1;
}

int cspn_uphalf_forward(const void* x, const void* packed, const void* scale, const void* shift, int relu_channels, void* const* outs,
                        const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream) {
    const char* who = "cspn_uphalf_forward";
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail("%s: bad shape (N=%d, C=%d, H=%d, W=%d)", who, N, C, H, W);
    if (oh < 1 || ow < 1 || (long)oh > 2L * H || (long)ow > 2L * W)
        return fail("%s: output %dx%d must lie in [1, 2H] x [1, 2W] = %ldx%ld", who, oh, ow, 2L * H, 2L * W);
    Args a;
    if (!check_filters(who, out_channels, n_outs, a.O0, a.O1)) return 0;
    a.M = a.O0 + a.O1;
    if (!packed_elems(a.M, C)) return fail("%s: bad size (%d output channels, C=%d)", who, a.M, C);
    if ((double)N * C * H * W >= 2147483648.0 || (double)N * a.O0 * oh * ow >= 2147483648.0 || (double)N * a.O1 * oh * ow >= 2147483648.0)
        return fail("%s: a tensor of 2^31 elements or more; split the batch", who);
    if (!x || !packed || !outs) return fail("%s: null pointer", who);
    for (int k = 0; k < n_outs; ++k)
        if (!outs[k]) return fail("%s: null pointer (output %d)", who, k);
    if (!aligned16(packed)) return fail("%s: packed must be 16-byte aligned", who);
    if (!scale != !shift) return fail("%s: scale and shift come together", who);
    if (relu_channels < 0 || relu_channels > a.M) return fail("%s: relu_channels %d outside [0, %d]", who, relu_channels, a.M);
    a.x = static_cast<const _Float16*>(x), a.wp = static_cast<const _Float16*>(packed);
    a.scale = static_cast<const float*>(scale), a.shift = static_cast<const float*>(shift);
    a.y0 = static_cast<_Float16*>(outs[0]), a.y1 = n_outs > 1 ? static_cast<_Float16*>(outs[1]) : nullptr;
    a.Mp = round_up(a.M, TM), a.relu = relu_channels;
    a.N = N, a.C = C, a.Cp = round_up(C, KC), a.H = H, a.W = W, a.oh = oh, a.ow = ow;
    a.mtiles = a.Mp / TM;
    double blocks = 0;
    for (int p = 0; p < 4; ++p) {
        a.first[p] = (unsigned)blocks;
        const double npix = (double)N * ((oh + 1 - (p >> 1)) / 2) * ((ow + 1 - (p & 1)) / 2);      // < 2^31: an output has fewer elements
        blocks += (double)(((long)npix + TN - 1) / TN) * a.mtiles;
        if (blocks >= 2147483648.0) return fail("%s: more than 2^31 tiles; split the batch", who);
    }
    a.first[4] = (unsigned)blocks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CSPN_PRE(st), uphalf_fwd<<<dim3(a.first[4]), dim3(THREADS), 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

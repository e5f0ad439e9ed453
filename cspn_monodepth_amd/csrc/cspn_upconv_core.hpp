// cspn_upconv_core.hpp — what the fused decoder-block kernels share: the heads cspn_upconv.hip (fp32) and
// cspn_uphalf.hip (fp16, f-13), and the 3x3 tail cspn_uptail.hip (f-14).
//   shared by all three   the tile constants, Args, the pixel decode, round_up and the precision policies F32 / F16: how a chunk of the
//                         implicit GEMM is found, loaded, staged in LDS and multiplied
//   the heads' alone      the phase tables, pack, the forward fwd<P>, the argument checks and the launches
// NOT shared, on purpose: the forward.  The tail's tail_fwd<P, G> is fwd<P> with a geometry parameter; with the heads instantiated from
// that generic form the fp32 head kept its registers and LDS but compiled to gather loads that wait for one another (9 more s_waitcnt)
// and ran 20 to 24 % slower on the MI355X (RESULTS.md row 36).  That is a finding about the forward: with the policies alone moved
// here, every kernel of the three units compiles to the instructions it had with a copy of its own.
//
// The heads:
//   network/unet_ours.py:160-248 UpProj_Block / Gudi_UpProj_Block / Gudi_UpProj_Block_Cat / Simple_Gudi_UpConv_Block: zero-insertion
//   un-pooling by 2, crop to oh x ow, then one or two bias-free 5x5 convolutions over that map, each followed by a batch norm (in eval
//   mode a per-channel affine map) and, for the first, a ReLU.
// The un-pooled map is never formed.  Output pixel (2i + a, 2j + b) of a pad-2 5x5 window over it meets the compact map through the
// taps (ky, kx) with a + ky and b + kx even: rows i - 1, i, i + 1 (ky = 0, 2, 4) for a = 0 and i, i + 1 (ky = 1, 3) for a = 1,
// likewise the columns — 9, 6, 6, 4 taps for the phases (0,0), (0,1), (1,0), (1,1).  A neighbour outside the compact pixels that take
// part contributes zeros.
//   pack   the filters -> 25 taps, phase-major, of a Cp x Mp matrix each (tap t of phase p, channel c, flat output channel m; Cp = C
//          rounded up to KC, Mp = the flat channels rounded up to TM, zero-filled, so that the forward loads whole tiles unguarded),
//          in the element type and the order (channel- or filter-contiguous) of the precision
//   fwd    an implicit GEMM per phase: M = flat channels, N = the phase's pixels over the whole batch, K = (tap, channel).  A workgroup
//          of 4 wavefronts owns a TM x TN = 128 x 128 tile and walks K in chunks of KC = 32 channels of one tap: the filter chunk and
//          the gathered pixels go through LDS, a wavefront holds 2 x 2 accumulators of a 32 x 32 matrix instruction (64 x 64).
//          Single-buffered: the loads of a chunk are issued before the barrier that ends the previous chunk's products, and several
//          workgroups per CU cover each other's loads.
// An output element is one chain over K in the packed order, whatever its tile: no split-K, no atomics.
// A precision is a policy P (F32, F16 and, for the heads' fp32 family alone, F32X3 below): the element type T, the two LDS tiles, the registers of a chunk, and how a chunk is found
// (wtile), loaded, staged and multiplied; everything else of the heads, the argument checks of the entry points included, is here once.
#pragma once
#include "cspn_common.hpp"

namespace {

constexpr int TM = 128, TN = 128, KC = 32, THREADS = 256;
constexpr int TAPS = 25;

typedef float v16f __attribute__((ext_vector_type(16)));

template <typename T>
struct Args {
    const T* x;
    const T* wp;
    const float* scale;       // null: no affine map
    const float* shift;
    T* y0;
    T* y1;
    int O0, O1, M, Mp, relu;
    int N, C, Cp, H, W, oh, ow;
    int mtiles;
    unsigned first[5];        // first workgroup of phase p (p = 2a + b), first[4] = the grid
};

// phase p = 2a + b: rows of taps, columns of taps, first tap in the packed order
__host__ __device__ constexpr int tap_rows(int p) { return (p >> 1) ? 2 : 3; }
__host__ __device__ constexpr int tap_cols(int p) { return (p & 1) ? 2 : 3; }
__host__ __device__ constexpr int tap_base(int p) { return p == 0 ? 0 : p == 1 ? 9 : p == 2 ? 15 : 21; }

// e = (packed tap, channel, flat output channel), or with CHANNEL_INNER (packed tap, flat output channel, channel); S -> D rounds to
// nearest even
template <typename S, typename D, bool CHANNEL_INNER>
__global__ __launch_bounds__(256) void pack(const S* __restrict__ w0, const S* __restrict__ w1, D* __restrict__ wp, int O0, int M, int Mp,
                                            int C, int Cp, size_t elems) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    const int inner = CHANNEL_INNER ? Cp : Mp, outer = CHANNEL_INNER ? Mp : Cp;
    const int in = (int)(e % inner);
    const size_t row = e / inner;
    const int out = (int)(row % outer), tg = (int)(row / outer);
    const int m = CHANNEL_INNER ? out : in, c = CHANNEL_INNER ? in : out;
    const int p = tg < 9 ? 0 : tg < 15 ? 1 : tg < 21 ? 2 : 3;
    const int t = tg - tap_base(p);
    const int tr = t / tap_cols(p), tc = t - tr * tap_cols(p);
    const int ky = 2 * tr + (p >> 1), kx = 2 * tc + (p & 1);
    D v = (D)0.f;
    if (m < M && c < C) {
        const S* src = m < O0 ? w0 + (size_t)m * C * 25 : w1 + (size_t)(m - O0) * C * 25;
        v = (D)src[(size_t)c * 25 + ky * 5 + kx];
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

// The fp32 form of a chunk.
//   pack  wp[taps][Cp][Mp] fp32: filter-contiguous, a row of the chunk is TM consecutive floats
//   fwd   the filter chunk [KC][TM] and the gathered pixels [KC][TN] go through LDS as they are loaded: a thread fetches 4 x 16 bytes of
//         the filter chunk (rows (t >> 5) + 8 r) and pixel t & 127 of the channels (t >> 7) + 2 r, consecutive lanes on consecutive
//         pixels of a row.  v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][l >> 5] and B[l >> 5][l & 31], so a step reads two rows
//         of each tile.  Exact fp32 products.
// load(): c0 is the chunk's first channel within its map, C the map's channels, wt the filter chunk's tap at that map's channel 0.
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
    static __device__ __forceinline__ void load(Chunk& k, const Args<float>& a, const float* wt, const float* xt, int c0, int C, int t,
                                                bool there, size_t hw) {
        const int kb = t >> 7;
#pragma unroll
        for (int r = 0; r < 4; ++r) k.wv[r] = *reinterpret_cast<const v4f*>(wt + (size_t)(c0 + 8 * r) * a.Mp);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = c0 + kb + 2 * r;
            k.xv[r] = (there && c < C) ? xt[(size_t)c * hw] : 0.f;
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

// The fp16 form of a chunk.
//   pack  wp[taps][Mp][Cp] fp16, from fp32 (rounded to nearest even) or fp16 filters.  Channel-contiguous: the 8 channels lane l of
//         v_mfma_f32_32x32x16_f16 holds of row l & 31 (A[l & 31][8 (l >> 5) + j]) are 16 consecutive bytes.
//   fwd   a chunk is two blocks of 16 channels.  The filter chunk [TM][KC] and the gathered pixels [TN][KC] go through LDS, both
//         channel-contiguous with rows of 80 bytes (64 of data + 16 of padding): the 16 lanes a ds_read_b128 serves in one cycle then
//         start at 20 l mod 64 banks, all different, so the operand reads are conflict-free without a swizzle.  A thread fetches
//         2 x 16 bytes of the filter chunk (rows (t >> 2) + 64 r, fragment t & 3) and pixel t & 127 of the channel groups of 8
//         (t >> 7) + 2 r.  The NCHW gather is 2-byte loads, consecutive lanes on consecutive pixels of a row (pairs are not formed: the
//         column offset of a tap and the row length make half of them misaligned).  fp32 accumulation, one rounding of the result.
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
    static __device__ __forceinline__ void load(Chunk& k, const Args<_Float16>& a, const _Float16* wt, const _Float16* xt, int c0, int C,
                                                int t, bool there, size_t hw) {
        const int cb = c0 + 8 * (t >> 7);      // c = cb + a constant, one add: known not to wrap, c * hw needs no sign extension
#pragma unroll
        for (int r = 0; r < 2; ++r) k.wv[r] = *reinterpret_cast<const v8h*>(wt + (size_t)(64 * r) * a.Cp + c0);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = cb + 16 * r + j;
                k.xv[r][j] = (there && c < C) ? xt[(size_t)c * hw] : (_Float16)0.f;
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

// The split form of a chunk: fp32 in and out, the products on the bf16 matrix cores.
//   split every fp32 value v, filter or pixel, becomes three bf16 terms, conversions to nearest even:
//             v1 = bf16(v),  v2 = bf16(v - v1),  v3 = bf16(v - v1 - v2)
//         Both subtractions are exact in fp32 and v1 + v2 + v3 == v (8 + 8 + 8 significant bits cover the 24 of v).  A product x w
//         is the six terms x_i w_j with i + j <= 4, each exact in fp32; the three left out are below (2^-23 + 2^-32) |x w|.
//   pack  the fp32 pack of F32 as it is, wp[taps][Cp][Mp]: one pack serves both forms.
//   fwd   a thread fetches 8 x 8 bytes of the filter chunk — the channels 8 (t >> 6) .. + 7 of the flat channels 2 (t & 63), + 1 —
//         and pixel t & 127 of the channel groups of 8 (t >> 7) + 2 r as F16 does, splits them in registers behind the barrier and
//         stages the three planes of each tile channel-contiguous in F16's rows of 80 bytes: one ds_read_b128 per fragment, 60 KiB of
//         LDS per workgroup.  A chunk is two blocks of 16 channels; per block the six terms go to v_mfma_f32_32x32x16_bf16 in the
//         order (1,1) (1,2) (2,1) (1,3) (2,2) (3,1) (filter term, pixel term), accumulating in fp32.  An output element is still one
//         chain: taps, chunks, blocks and terms in that order; the order of the 16 products inside an instruction is the hardware's.
typedef __bf16 v8b __attribute__((ext_vector_type(8)));
typedef float v2f __attribute__((ext_vector_type(2)));

struct F32X3 {
    using T = float;
    using ATile = v8b[3][TM][ROW8];
    using BTile = v8b[3][TN][ROW8];
    struct Chunk {
        v2f wv[8];
        float xv[2][8];
    };
    static constexpr bool CHANNEL_INNER = false;

    static __device__ __forceinline__ const float* wtile(const Args<float>& a, int mt, int t) {
        return a.wp + (size_t)mt * TM + (size_t)(8 * (t >> 6)) * a.Mp + 2 * (t & 63);
    }
    static __device__ __forceinline__ void load(Chunk& k, const Args<float>& a, const float* wt, const float* xt, int c0, int C, int t,
                                                bool there, size_t hw) {
        const int cb = c0 + 8 * (t >> 7);
#pragma unroll
        for (int j = 0; j < 8; ++j) k.wv[j] = *reinterpret_cast<const v2f*>(wt + (size_t)(c0 + j) * a.Mp);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = cb + 16 * r + j;
                k.xv[r][j] = (there && c < C) ? xt[(size_t)c * hw] : 0.f;
            }
    }
    // element j of the three planes' fragments <- the three terms of v
    static __device__ __forceinline__ void split(float v, v8b (&p)[3], int j) {
        const __bf16 v1 = (__bf16)v;
        const float r1 = v - (float)v1;
        const __bf16 v2 = (__bf16)r1;
        p[0][j] = v1, p[1][j] = v2, p[2][j] = (__bf16)(r1 - (float)v2);
    }
    static __device__ __forceinline__ void stage(ATile& As, BTile& Bs, const Chunk& k, int t) {
        const int px = t & 127, kb = t >> 7, wrow = 2 * (t & 63), wseg = t >> 6;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            v8b w[3], x[3];
#pragma unroll
            for (int j = 0; j < 8; ++j) split(k.wv[j][r], w, j), split(k.xv[r][j], x, j);
#pragma unroll
            for (int i = 0; i < 3; ++i) As[i][wrow + r][wseg] = w[i], Bs[i][px][kb + 2 * r] = x[i];
        }
    }
    static __device__ __forceinline__ void products(const ATile& As, const BTile& Bs, v16f (&acc)[2][2], int wm, int wn, int l31, int lh) {
        constexpr int TERMS[6][2] = {{0, 0}, {0, 1}, {1, 0}, {0, 2}, {1, 1}, {2, 0}};      // (filter plane, pixel plane)
#pragma unroll
        for (int s = 0; s < KC / 16; ++s) {
            const int f = 2 * s + lh;                        // channels 16 s + 8 (lane >> 5) .. + 7
            v8b a[3][2], b[3][2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                a[i][0] = As[i][wm * 64 + l31][f], a[i][1] = As[i][wm * 64 + 32 + l31][f];
                b[i][0] = Bs[i][wn * 64 + l31][f], b[i][1] = Bs[i][wn * 64 + 32 + l31][f];
            }
#pragma unroll
            for (int e = 0; e < 6; ++e) {
                const int i = TERMS[e][0], j = TERMS[e][1];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][1], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j][0], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j][1], acc[1][1], 0, 0, 0);
            }
        }
    }
};

// The heads' forward.  The tail's (cspn_uptail.hip, tail_fwd<P, G>) is this text with a geometry parameter, and the two stay two: see
// the head of this file.
template <class P>
__global__ __launch_bounds__(THREADS) void fwd(const Args<typename P::T> a) {
    using T = typename P::T;
    __shared__ __attribute__((aligned(16))) typename P::ATile As;
    __shared__ __attribute__((aligned(16))) typename P::BTile Bs;
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

    // the loads of this thread: pixel t & 127 for the policy's share of a chunk's channels, and its share of the filter chunk
    const Pixel mine = decode(nt * TN + (t & 127), npix, Ha, Wb);
    const T* xpix = a.x + (size_t)mine.frame * a.C * hw + (size_t)mine.i * a.W + mine.j;
    const T* wtile = P::wtile(a, mt, t);

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
        const T* xt = xpix + (long)di * a.W + dj;
        const T* wt = wtile + (size_t)(tap_base(p) + tap) * a.Mp * a.Cp;
        for (int cc = 0; cc < cchunks; ++cc) {
            typename P::Chunk k;
            P::load(k, a, wt, xt, cc * KC, a.C, t, there, hw);
            __syncthreads();                                     // the previous chunk has been read
            P::stage(As, Bs, k, t);
            __syncthreads();
            P::products(As, Bs, acc, wm, wn, l31, lh);
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
                T* dst = m < a.O0 ? a.y0 + ((size_t)q.frame * a.O0 + m) * plane : a.y1 + ((size_t)q.frame * a.O1 + (m - a.O0)) * plane;
                dst[at] = (T)y;                                  // the one rounding to T, to nearest even; overflow gives +-Inf
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

int check_filters(const char* who, const int* out_channels, int n, int& O0, int& O1, int max_filters) {
    if (!out_channels || n < 1 || n > max_filters) return fail("%s: between 1 and %d filters, got %d", who, max_filters, n);
    for (int k = 0; k < n; ++k)
        if (out_channels[k] < 1 || out_channels[k] > (1 << 23)) return fail("%s: filter %d has %d output channels", who, k, out_channels[k]);
    O0 = out_channels[0], O1 = n > 1 ? out_channels[1] : 0;
    return 1;
}

// The argument rules of a pack entry point behind its own rule for the dtype; `who` is the entry point's name.
int check_pack(const char* who, const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, const void* packed,
               int max_filters, int& O0, int& M, size_t& elems) {
    if (kh != 5 || kw != 5) return fail("%s: the filters must be 5x5, got %dx%d", who, kh, kw);
    int O1 = 0;
    if (!check_filters(who, out_channels, n_filters, O0, O1, max_filters)) return 0;
    if (!weights || !packed) return fail("%s: null pointer", who);
    for (int k = 0; k < n_filters; ++k)
        if (!weights[k]) return fail("%s: null pointer (filter %d)", who, k);
    if (!aligned16(packed)) return fail("%s: packed must be 16-byte aligned", who);
    M = O0 + O1;
    elems = packed_elems(M, C);
    if (!elems) return fail("%s: bad size (%d output channels, C=%d), or a packed form of 2^31 elements or more", who, M, C);
    if ((double)out_channels[0] * C * 25 >= 2147483648.0 || (double)O1 * C * 25 >= 2147483648.0) return fail("%s: a filter of 2^31 elements or more", who);
    return 1;
}

// ... and the launch: filters of type S into the packed form of the precision P
template <typename S, class P>
int launch_pack(const void* const* weights, int n_filters, void* packed, int O0, int M, int C, size_t elems, cspn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    CSPN_PRE(st), pack<S, typename P::T, P::CHANNEL_INNER><<<dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st>>>(
        static_cast<const S*>(weights[0]), n_filters > 1 ? static_cast<const S*>(weights[1]) : nullptr, static_cast<typename P::T*>(packed), O0, M,
        round_up(M, TM), C, round_up(C, KC), elems);
    HIP_OK(hipGetLastError());
    return 1;
}

// The argument rules of a forward entry point behind its own rule for the dtype, and the arguments of the kernel with its grid.
template <typename T>
int fill_forward_args(const char* who, Args<T>& a, const void* x, const void* packed, const void* scale, const void* shift, int relu_channels,
                      void* const* outs, const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow, int max_filters) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail("%s: bad shape (N=%d, C=%d, H=%d, W=%d)", who, N, C, H, W);
    if (oh < 1 || ow < 1 || (long)oh > 2L * H || (long)ow > 2L * W)
        return fail("%s: output %dx%d must lie in [1, 2H] x [1, 2W] = %ldx%ld", who, oh, ow, 2L * H, 2L * W);
    if (!check_filters(who, out_channels, n_outs, a.O0, a.O1, max_filters)) return 0;
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
    a.x = static_cast<const T*>(x), a.wp = static_cast<const T*>(packed);
    a.scale = static_cast<const float*>(scale), a.shift = static_cast<const float*>(shift);
    a.y0 = static_cast<T*>(outs[0]), a.y1 = n_outs > 1 ? static_cast<T*>(outs[1]) : nullptr;
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
    return 1;
}

// ... and the launch in the precision P
template <class P>
int forward(const char* who, const void* x, const void* packed, const void* scale, const void* shift, int relu_channels, void* const* outs,
            const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow, int max_filters, cspn_stream_t stream) {
    Args<typename P::T> a;
    if (!fill_forward_args(who, a, x, packed, scale, shift, relu_channels, outs, out_channels, n_outs, N, C, H, W, oh, ow, max_filters)) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CSPN_PRE(st), fwd<P><<<dim3(a.first[4]), dim3(THREADS), 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // namespace

// cspn_uptail.hip — the 3x3 tail of a decoder block: convolution over one or two maps, folded batch norm, residual, ReLU
// (include/cspn_uptail.h).
//
// An implicit GEMM as the fused heads': M = O, N = the pixels of the whole batch in tiles of 128, K = (tap, channel) in chunks of 32
// channels of one tap.  From cspn_upconv_core.hpp come Args, the pixel decode, the tile constants and round_up.  The forward below is
// the core's forward with a geometry parameter G beside the precision policy P (Same3: one phase of 9 taps at offsets -1 .. 1, the
// store at y W + x, a per-chunk choice between two maps, a residual in the epilogue), and the policies F32 / F16 are the heads'
// with the map's channel count as an argument of load().  They are HERE and not in the core on purpose: with the forward of the
// heads instantiated from this generic form, the fp32 head compiled to the same registers and LDS but to gather loads that wait
// for one another (9 more s_waitcnt) and ran 20 to 24 % slower on the MI355X (RESULTS.md row 36).  Until a shared form compiles
// to the parent's schedule the heads keep their own text.
//   pack  wp[9 taps][Cp][Mp] fp32 or wp[9][Mp][Cp] fp16, as the precision's wtile() expects; Cp = roundup(Ca, KC) + roundup(Cb, KC),
//         so that a chunk of KC packed channels never straddles the two maps.  Zero-filled.
#include "cspn_upconv_core.hpp"
#include "cspn_uptail.h"

namespace {

// what Same3 adds: the second map, whose channels follow the first's in the filter, and the residual
template <typename T>
struct TailArgs : Args<T> {
    const T* xb;              // [N, Cb, H, W], null with Cb = 0
    const T* r;               // [N, M, H, W] added after the affine map, or null
    int Cb, Cap;              // channels of xb; C rounded up to KC: the packed channels in front of xb's
};

// where a chunk's gathered channels come from: channel 0 of the map at this thread's pixel, the packed channels in front of the
// map's, and its channels
template <typename T>
struct Source {
    const T* x;
    int skip, C;
};

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

// The tail: one phase, the 9 taps at offsets -1 .. 1 of a pad-1 3x3 window over the maps themselves (oh = H, ow = W).  The packed
// channels are C rounded up to KC of map x, then those of xb, so a chunk lies in one map and picking it is a wavefront-uniform choice
// between two pointers.
struct Same3 {
    template <typename T>
    using A = TailArgs<T>;
    template <typename T>
    struct Pixels {
        const T* a;
        const T* b;
    };
    static constexpr bool RESIDUAL = true;
    static constexpr int pa = 0, pb = 0, ntc = 3, ntaps = 9, di0 = -1, dj0 = -1;
    __device__ __forceinline__ int packed_tap(int tap) const { return tap; }
    unsigned local;
    int Hc, Wc, Ha, Wb;

    template <typename T>
    __device__ __forceinline__ Same3(const TailArgs<T>& a, unsigned bid) : local(bid), Hc(a.H), Wc(a.W), Ha(a.H), Wb(a.W) {}
    template <typename T>
    __device__ __forceinline__ Pixels<T> pixels(const TailArgs<T>& a, const Pixel& q, size_t hw) const {
        const size_t at = (size_t)q.i * a.W + q.j;
        return {a.x + (size_t)q.frame * a.C * hw + at, a.xb + (size_t)q.frame * a.Cb * hw + at};      // b: used with Cb > 0 only
    }
    template <typename T>
    __device__ __forceinline__ Pixels<T> moved(const Pixels<T>& xpix, long off) const {
        return {xpix.a + off, xpix.b + off};
    }
    // the chunk at packed channel c0: map x below Cap, map xb from there on, its channels counted from 0 and the filter chunk moved
    // along by the packed channels in front of it
    template <class P>
    __device__ __forceinline__ void load(typename P::Chunk& k, const TailArgs<typename P::T>& a, const typename P::T* wt,
                                         const Pixels<typename P::T>& xt, int c0, int t, bool there, size_t hw) const {
        const Source<typename P::T> s = c0 < a.Cap ? Source<typename P::T>{xt.a, 0, a.C} : Source<typename P::T>{xt.b, a.Cap, a.Cb};
        P::load(k, a, wt + (size_t)s.skip * (P::CHANNEL_INNER ? 1 : a.Mp), s.x, c0 - s.skip, s.C, t, there, hw);
    }
    template <typename T>
    __device__ __forceinline__ size_t at(const TailArgs<T>& a, const Pixel& q) const {
        return (size_t)q.i * a.W + q.j;
    }
};

template <class P, class G>
__global__ __launch_bounds__(THREADS) void tail_fwd(const typename G::template A<typename P::T> a) {
    using T = typename P::T;
    __shared__ __attribute__((aligned(16))) typename P::ATile As;
    __shared__ __attribute__((aligned(16))) typename P::BTile Bs;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const G g(a, blockIdx.x);
    const int mt = g.local % a.mtiles;
    const unsigned nt = g.local / a.mtiles;
    const unsigned npix = (unsigned)a.N * g.Ha * g.Wb;
    const size_t hw = (size_t)a.H * a.W;

    // the loads of this thread: pixel t & 127 for the policy's share of a chunk's channels, and its share of the filter chunk
    const Pixel mine = decode(nt * TN + (t & 127), npix, g.Ha, g.Wb);
    const typename G::template Pixels<T> xpix = g.pixels(a, mine, hw);
    const T* wtile = P::wtile(a, mt, t);

    v16f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int cchunks = a.Cp / KC;
    for (int tap = 0; tap < g.ntaps; ++tap) {
        const int tr = tap / g.ntc, tc = tap - tr * g.ntc;
        const int di = g.di0 + tr, dj = g.dj0 + tc;
        const int ii = mine.i + di, jj = mine.j + dj;
        const bool there = mine.ok && ii >= 0 && ii < g.Hc && jj >= 0 && jj < g.Wc;
        const typename G::template Pixels<T> xt = g.moved(xpix, (long)di * a.W + dj);
        const T* wt = wtile + (size_t)g.packed_tap(tap) * a.Mp * a.Cp;
        for (int cc = 0; cc < cchunks; ++cc) {
            typename P::Chunk k;
            g.template load<P>(k, a, wt, xt, cc * KC, t, there, hw);
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
        const Pixel q = decode(nt * TN + wn * 64 + tn * 32 + l31, npix, g.Ha, g.Wb);
        if (!q.ok) continue;
        const size_t at = g.at(a, q);
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * TM + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= a.M) continue;
                float y = acc[tm][tn][r];
                if (a.scale) y = fmaf(y, a.scale[m], a.shift[m]);
                if constexpr (G::RESIDUAL)
                    if (a.r) y += (float)a.r[((size_t)q.frame * a.M + m) * plane + at];      // an add of its own, rounded as the stock add is
                if (m < a.relu) y = y < 0.f ? 0.f : y;           // NaN stays NaN
                T* dst = m < a.O0 ? a.y0 + ((size_t)q.frame * a.O0 + m) * plane : a.y1 + ((size_t)q.frame * a.O1 + (m - a.O0)) * plane;
                dst[at] = (T)y;                                  // the one rounding to T, to nearest even; overflow gives +-Inf
            }
        }
    }
}

// e = (tap, packed channel, output channel), or with CHANNEL_INNER (tap, output channel, packed channel); S -> D rounds to nearest even
template <typename S, typename D, bool CHANNEL_INNER>
__global__ __launch_bounds__(256) void pack3(const S* __restrict__ w, D* __restrict__ wp, int O, int Mp, int Ca, int Cap, int Cb, int Cp,
                                             size_t elems) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    const int inner = CHANNEL_INNER ? Cp : Mp, outer = CHANNEL_INNER ? Mp : Cp;
    const int in = (int)(e % inner);
    const size_t row = e / inner;
    const int out = (int)(row % outer), tap = (int)(row / outer);
    const int m = CHANNEL_INNER ? out : in, c = CHANNEL_INNER ? in : out;
    const int src = c < Cap ? (c < Ca ? c : -1) : (c - Cap < Cb ? Ca + (c - Cap) : -1);      // the filter's channel, -1: padding
    D v = (D)0.f;
    if (m < O && src >= 0) v = (D)w[((size_t)m * (Ca + Cb) + src) * 9 + tap];
    wp[e] = v;
}

size_t tail_elems(int O, int Ca, int Cb) {
    if (O < 1 || Ca < 1 || Cb < 0 || O > (1 << 24) || Ca > (1 << 24) || Cb > (1 << 24)) return 0;
    const double e = 9.0 * ((double)round_up(Ca, KC) + round_up(Cb, KC)) * round_up(O, TM);
    return e >= 2147483648.0 ? 0 : (size_t)e;
}

template <typename S, class P>
int launch_pack3(const void* w, void* packed, int O, int Ca, int Cb, size_t elems, cspn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Cap = round_up(Ca, KC);
    CSPN_PRE(st), pack3<S, typename P::T, P::CHANNEL_INNER><<<dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st>>>(
        static_cast<const S*>(w), static_cast<typename P::T*>(packed), O, round_up(O, TM), Ca, Cap, Cb, Cap + round_up(Cb, KC), elems);
    HIP_OK(hipGetLastError());
    return 1;
}

template <class P>
int tail_forward(const char* who, const void* xa, const void* xb, const void* packed, const float* scale, const float* shift,
                 const void* residual, int relu, void* out, int N, int Ca, int Cb, int O, int H, int W, cspn_stream_t stream) {
    using T = typename P::T;
    TailArgs<T> a;
    a.x = static_cast<const T*>(xa), a.xb = static_cast<const T*>(xb), a.r = static_cast<const T*>(residual);
    a.wp = static_cast<const T*>(packed), a.scale = scale, a.shift = shift;
    a.y0 = static_cast<T*>(out), a.y1 = nullptr;
    a.O0 = a.M = O, a.O1 = 0, a.Mp = round_up(O, TM), a.relu = relu ? O : 0;
    a.N = N, a.C = Ca, a.Cb = Cb, a.Cap = round_up(Ca, KC), a.Cp = a.Cap + round_up(Cb, KC);
    a.H = a.oh = H, a.W = a.ow = W;
    a.mtiles = a.Mp / TM;
    const double blocks = (double)(((long)N * H * W + TN - 1) / TN) * a.mtiles;      // N H W < 2^31: out has fewer elements
    if (blocks >= 2147483648.0) return fail("%s: more than 2^31 tiles; split the batch", who);
    a.first[0] = 0;
    for (int p = 1; p < 5; ++p) a.first[p] = (unsigned)blocks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CSPN_PRE(st), tail_fwd<P, Same3><<<dim3(a.first[4]), dim3(THREADS), 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // namespace

extern "C" {

int cspn_uptail_abi_version(void) { return CSPN_UPTAIL_ABI_VERSION; }

size_t cspn_uptail_packed_bytes(int O, int Ca, int Cb, int dtype) {
    if (dtype != CSPN_F32 && dtype != CSPN_F16) return 0;
    return tail_elems(O, Ca, Cb) * (dtype == CSPN_F32 ? sizeof(float) : sizeof(_Float16));
}

int cspn_uptail_pack(const void* w, int O, int Ca, int Cb, int kh, int kw, int src_dtype, int dst_dtype, void* packed,
                     cspn_stream_t stream) {
    const char* who = "cspn_uptail_pack";
    if (kh != 3 || kw != 3) return fail("%s: the filter must be 3x3, got %dx%d", who, kh, kw);
    if (!((src_dtype == CSPN_F32 && (dst_dtype == CSPN_F32 || dst_dtype == CSPN_F16)) || (src_dtype == CSPN_F16 && dst_dtype == CSPN_F16)))
        return fail("%s: fp32 -> fp32, fp32 -> fp16 or fp16 -> fp16, got dtypes %d -> %d", who, src_dtype, dst_dtype);
    if (!w || !packed) return fail("%s: null pointer", who);
    if (!aligned16(packed)) return fail("%s: packed must be 16-byte aligned", who);
    const size_t elems = tail_elems(O, Ca, Cb);
    if (!elems) return fail("%s: bad size (O=%d, Ca=%d, Cb=%d), or a packed form of 2^31 elements or more", who, O, Ca, Cb);
    if ((double)O * ((double)Ca + Cb) * 9 >= 2147483648.0) return fail("%s: a filter of 2^31 elements or more", who);
    if (dst_dtype == CSPN_F32) return launch_pack3<float, F32>(w, packed, O, Ca, Cb, elems, stream);
    return src_dtype == CSPN_F32 ? launch_pack3<float, F16>(w, packed, O, Ca, Cb, elems, stream)
                                 : launch_pack3<_Float16, F16>(w, packed, O, Ca, Cb, elems, stream);
}

int cspn_uptail_forward(const void* a, const void* b, const void* packed, const float* scale, const float* shift, const void* residual,
                        int relu, void* out, int dtype, int N, int Ca, int Cb, int O, int H, int W, cspn_stream_t stream) {
    const char* who = "cspn_uptail_forward";
    if (dtype != CSPN_F32 && dtype != CSPN_F16) return fail("%s: fp32 or fp16, got dtype %d", who, dtype);
    if (N < 1 || H < 1 || W < 1) return fail("%s: bad shape (N=%d, H=%d, W=%d)", who, N, H, W);
    if (!tail_elems(O, Ca, Cb)) return fail("%s: bad size (O=%d, Ca=%d, Cb=%d)", who, O, Ca, Cb);
    const double pixels = (double)N * H * W;
    if (pixels * Ca >= 2147483648.0 || pixels * Cb >= 2147483648.0 || pixels * O >= 2147483648.0)
        return fail("%s: a tensor of 2^31 elements or more; split the batch", who);
    if (!a || !packed || !out) return fail("%s: null pointer", who);
    if (b && !Cb) return fail("%s: a second map with Cb = 0", who);
    if (!b && Cb) return fail("%s: Cb = %d and no second map (null pointer)", who, Cb);
    if (!aligned16(packed)) return fail("%s: packed must be 16-byte aligned", who);
    if (!scale != !shift) return fail("%s: scale and shift come together", who);
    return dtype == CSPN_F32 ? tail_forward<F32>(who, a, b, packed, scale, shift, residual, relu, out, N, Ca, Cb, O, H, W, stream)
                             : tail_forward<F16>(who, a, b, packed, scale, shift, residual, relu, out, N, Ca, Cb, O, H, W, stream);
}

}  // extern "C"

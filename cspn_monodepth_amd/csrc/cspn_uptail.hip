// cspn_uptail.hip — the 3x3 tail of a decoder block: convolution over one or two maps, folded batch norm, residual, ReLU
// (include/cspn_uptail.h).
//
// An implicit GEMM as the fused heads': M = O, N = the pixels of the whole batch in tiles of 128, K = (tap, channel) in chunks of 32
// channels of one tap.  From cspn_upconv_core.hpp come Args, the pixel decode, the tile constants, round_up and the precision
// policies F32 / F16, whose load() takes the channel count of the map a chunk lies in.  The forward is NOT shared: tail_fwd<P, G> below
// is the core's fwd<P> with a geometry parameter G (Same3: one phase of 9 taps at offsets -1 .. 1, the store at y W + x, a per-chunk
// choice between two maps, a residual in the epilogue), and the heads keep their own text because, instantiated from this generic
// form, the fp32 head ran 20 to 24 % slower (RESULTS.md row 36; the head of the core has the detail).
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

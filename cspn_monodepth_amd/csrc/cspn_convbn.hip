// cspn_convbn.hip — the encoder's convolutions: a bias-free k x k convolution (k = 1 or 3, pad k / 2, stride 1 or 2) over one map,
// folded batch norm, residual, ReLU (include/cspn_convbn.h).
//
// The implicit GEMM of the 3x3 tail (cspn_uptail.hip): M = O, N = the OUTPUT pixels of the whole batch in tiles of 128, K = (tap,
// channel) in chunks of 32 channels of one tap.  From cspn_upconv_core.hpp come Args, the pixel decode, the tile constants, round_up and
// the precision policies F32 / F16.  The forward is NOT shared, as the tail's is not shared with the heads' (the head of the core says
// why): conv_fwd<P, K, S> below is tail_fwd<P, Same3> with one map, the taps of a k x k window and a stride — a thread gathers around
// the input pixel (S i, S j) of its output pixel (i, j), tests the edge against the input H x W and stores at the output pixel — and the
// existing units keep their text, so their kernels keep their instructions.  With K = 3, S = 1 the chain of an output element is the
// tail's over one map: the same taps, chunks and matrix instructions in the same order, the same epilogue, the same bits.
//   pack  wp[k k taps][Cp][Mp] fp32 or wp[k k][Mp][Cp] fp16, as the precision's wtile() expects; Cp = roundup(C, KC), Mp = roundup(O,
//         TM).  Zero-filled, so that tiles load unguarded.
#include "cspn_upconv_core.hpp"
#include "cspn_convbn.h"

namespace {

template <typename T>
struct ConvArgs : Args<T> {
    const T* r;               // [N, M, oh, ow] added after the affine map, or null
};

// K: the window (taps K K at offsets -K / 2 .. K / 2), S: the stride.  a.H x a.W is the input frame, a.oh x a.ow the output frame.
template <class P, int K, int S>
__global__ __launch_bounds__(THREADS) void conv_fwd(const ConvArgs<typename P::T> a) {
    using T = typename P::T;
    __shared__ __attribute__((aligned(16))) typename P::ATile As;
    __shared__ __attribute__((aligned(16))) typename P::BTile Bs;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    const unsigned bid = blockIdx.x;
    const int mt = bid % a.mtiles;
    const unsigned nt = bid / a.mtiles;
    const unsigned npix = (unsigned)a.N * a.oh * a.ow;
    const size_t hw = (size_t)a.H * a.W;

    // the loads of this thread: output pixel t & 127 for the policy's share of a chunk's channels, and its share of the filter chunk
    const Pixel mine = decode(nt * TN + (t & 127), npix, a.oh, a.ow);
    const int ci = S * mine.i, cj = S * mine.j;                  // the input pixel under the window's centre: inside the frame
    const T* xpix = a.x + (size_t)mine.frame * a.C * hw + (size_t)ci * a.W + cj;
    const T* wtile = P::wtile(a, mt, t);

    v16f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int cchunks = a.Cp / KC;
    for (int tap = 0; tap < K * K; ++tap) {
        const int tr = tap / K, tc = tap - tr * K;
        const int di = tr - K / 2, dj = tc - K / 2;
        const int ii = ci + di, jj = cj + dj;
        const bool there = mine.ok && ii >= 0 && ii < a.H && jj >= 0 && jj < a.W;
        const T* xt = xpix + ((long)di * a.W + dj);
        const T* wt = wtile + (size_t)tap * a.Mp * a.Cp;
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
        const Pixel q = decode(nt * TN + wn * 64 + tn * 32 + l31, npix, a.oh, a.ow);
        if (!q.ok) continue;
        const size_t at = (size_t)q.i * a.ow + q.j;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * TM + wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= a.M) continue;
                float y = acc[tm][tn][r];
                if (a.scale) y = fmaf(y, a.scale[m], a.shift[m]);
                const size_t e = ((size_t)q.frame * a.M + m) * plane + at;
                if (a.r) y += (float)a.r[e];                     // an add of its own, rounded as the stock add is
                if (a.relu) y = y < 0.f ? 0.f : y;               // NaN stays NaN
                a.y0[e] = (T)y;                                  // the one rounding to T, to nearest even; overflow gives +-Inf
            }
        }
    }
}

// e = (tap, packed channel, output channel), or with CHANNEL_INNER (tap, output channel, packed channel); S -> D rounds to nearest even
template <typename S, typename D, bool CHANNEL_INNER>
__global__ __launch_bounds__(256) void packk(const S* __restrict__ w, D* __restrict__ wp, int O, int Mp, int C, int Cp, int taps, size_t elems) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    const int inner = CHANNEL_INNER ? Cp : Mp, outer = CHANNEL_INNER ? Mp : Cp;
    const int in = (int)(e % inner);
    const size_t row = e / inner;
    const int out = (int)(row % outer), tap = (int)(row / outer);
    const int m = CHANNEL_INNER ? out : in, c = CHANNEL_INNER ? in : out;
    D v = (D)0.f;
    if (m < O && c < C) v = (D)w[((size_t)m * C + c) * taps + tap];
    wp[e] = v;
}

// the packed filter: elements, or 0 for a bad size
size_t conv_elems(int O, int C, int k) {
    if ((k != 1 && k != 3) || O < 1 || C < 1 || O > (1 << 24) || C > (1 << 24)) return 0;
    const double e = (double)(k * k) * round_up(C, KC) * round_up(O, TM);
    return e >= 2147483648.0 ? 0 : (size_t)e;
}

template <typename S, class P>
int launch_packk(const void* w, void* packed, int O, int C, int k, size_t elems, cspn_stream_t stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    CSPN_PRE(st), packk<S, typename P::T, P::CHANNEL_INNER><<<dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st>>>(
        static_cast<const S*>(w), static_cast<typename P::T*>(packed), O, round_up(O, TM), C, round_up(C, KC), k * k, elems);
    HIP_OK(hipGetLastError());
    return 1;
}

template <class P>
int conv_forward(const char* who, const void* x, const void* packed, const float* scale, const float* shift, const void* residual, int relu,
                 void* out, int N, int C, int O, int H, int W, int k, int stride, cspn_stream_t stream) {
    using T = typename P::T;
    ConvArgs<T> a;
    a.x = static_cast<const T*>(x), a.r = static_cast<const T*>(residual);
    a.wp = static_cast<const T*>(packed), a.scale = scale, a.shift = shift;
    a.y0 = static_cast<T*>(out), a.y1 = nullptr;
    a.O0 = a.M = O, a.O1 = 0, a.Mp = round_up(O, TM), a.relu = relu ? O : 0;
    a.N = N, a.C = C, a.Cp = round_up(C, KC);
    a.H = H, a.W = W, a.oh = (H - 1) / stride + 1, a.ow = (W - 1) / stride + 1;
    a.mtiles = a.Mp / TM;
    const double blocks = (double)(((long)N * a.oh * a.ow + TN - 1) / TN) * a.mtiles;      // N oh ow < 2^31: out has fewer elements
    if (blocks >= 2147483648.0) return fail("%s: more than 2^31 tiles; split the batch", who);
    a.first[0] = 0;
    for (int p = 1; p < 5; ++p) a.first[p] = (unsigned)blocks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(a.first[4]), block(THREADS);
    if (k == 1 && stride == 1) CSPN_PRE(st), conv_fwd<P, 1, 1><<<grid, block, 0, st>>>(a);
    else if (k == 1) CSPN_PRE(st), conv_fwd<P, 1, 2><<<grid, block, 0, st>>>(a);
    else if (stride == 1) CSPN_PRE(st), conv_fwd<P, 3, 1><<<grid, block, 0, st>>>(a);
    else CSPN_PRE(st), conv_fwd<P, 3, 2><<<grid, block, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // namespace

extern "C" {

int cspn_convbn_abi_version(void) { return CSPN_CONVBN_ABI_VERSION; }

size_t cspn_convbn_packed_bytes(int O, int C, int k, int dtype) {
    if (dtype != CSPN_F32 && dtype != CSPN_F16) return 0;
    return conv_elems(O, C, k) * (dtype == CSPN_F32 ? sizeof(float) : sizeof(_Float16));
}

int cspn_convbn_pack(const void* w, int O, int C, int kh, int kw, int src_dtype, int dst_dtype, void* packed, cspn_stream_t stream) {
    const char* who = "cspn_convbn_pack";
    if (kh != kw || (kh != 1 && kh != 3)) return fail("%s: the filter must be 1x1 or 3x3, got %dx%d", who, kh, kw);
    if (!((src_dtype == CSPN_F32 && (dst_dtype == CSPN_F32 || dst_dtype == CSPN_F16)) || (src_dtype == CSPN_F16 && dst_dtype == CSPN_F16)))
        return fail("%s: fp32 -> fp32, fp32 -> fp16 or fp16 -> fp16, got dtypes %d -> %d", who, src_dtype, dst_dtype);
    if (!w || !packed) return fail("%s: null pointer", who);
    if (!aligned16(packed)) return fail("%s: packed must be 16-byte aligned", who);
    const size_t elems = conv_elems(O, C, kh);
    if (!elems) return fail("%s: bad size (O=%d, C=%d), or a packed form of 2^31 elements or more", who, O, C);
    if ((double)O * C * kh * kw >= 2147483648.0) return fail("%s: a filter of 2^31 elements or more", who);
    if (dst_dtype == CSPN_F32) return launch_packk<float, F32>(w, packed, O, C, kh, elems, stream);
    return src_dtype == CSPN_F32 ? launch_packk<float, F16>(w, packed, O, C, kh, elems, stream)
                                 : launch_packk<_Float16, F16>(w, packed, O, C, kh, elems, stream);
}

int cspn_convbn_forward(const void* x, const void* packed, const float* scale, const float* shift, const void* residual, int relu,
                        void* out, int dtype, int N, int C, int O, int H, int W, int k, int stride, cspn_stream_t stream) {
    const char* who = "cspn_convbn_forward";
    if (dtype != CSPN_F32 && dtype != CSPN_F16) return fail("%s: fp32 or fp16, got dtype %d", who, dtype);
    if (k != 1 && k != 3) return fail("%s: k must be 1 or 3, got %d", who, k);
    if (stride != 1 && stride != 2) return fail("%s: stride must be 1 or 2, got %d", who, stride);
    if (N < 1 || H < 1 || W < 1) return fail("%s: bad shape (N=%d, H=%d, W=%d)", who, N, H, W);
    if (!conv_elems(O, C, k)) return fail("%s: bad size (O=%d, C=%d)", who, O, C);
    const double outs = (double)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    if ((double)N * H * W * C >= 2147483648.0 || outs * O >= 2147483648.0)
        return fail("%s: a tensor of 2^31 elements or more; split the batch", who);
    if (!x || !packed || !out) return fail("%s: null pointer", who);
    if (!aligned16(packed)) return fail("%s: packed must be 16-byte aligned", who);
    if (!scale != !shift) return fail("%s: scale and shift come together", who);
    return dtype == CSPN_F32 ? conv_forward<F32>(who, x, packed, scale, shift, residual, relu, out, N, C, O, H, W, k, stride, stream)
                             : conv_forward<F16>(who, x, packed, scale, shift, residual, relu, out, N, C, O, H, W, k, stride, stream);
}

}  // extern "C"

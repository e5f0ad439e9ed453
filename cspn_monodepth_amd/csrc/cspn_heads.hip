// cspn_heads.hip — the two output heads of the decoders fused with their un-pooling (include/cspn_heads.h).
//
//   network/unet_ours.py:194-202 Simple_Gudi_UpConv_Block_Last_Layer: zero-insertion un-pooling by 2, crop to oh x ow, one bias-free
//   3x3 convolution — twice over the same [B,64,114,152] map (64 -> 1 coarse depth, 64 -> 8 affinity guidance).
// The un-pooled map is never formed.  Output pixel (2i + a, 2j + b) of a pad-1 3x3 window over it touches compact pixels
//   (0,0): (i,j) under tap (1,1)            (0,1): (i,j) (1,0), (i,j+1) (1,2)
//   (1,0): (i,j) (0,1), (i+1,j) (2,1)       (1,1): (i,j) (0,0), (i,j+1) (0,2), (i+1,j) (2,0), (i+1,j+1) (2,2)
// so a compact pixel costs 9 multiplies per channel and output channel.  All heads are run as one list of OT <= 16 output channels
// ("flat" channel q: its filter, its plane in frame 0 and its frame stride), and every kernel is instantiated for OT = 1..16, so that
// the loops over them unroll.  heads_pack first gathers the filters of a call into one buffer (the `work` of the call) in the order the
// kernel walks them — [C][OT][9] for the forward, [OT][9][C rounded up to 32, zero-filled] for gx — so that the weights of an inner
// loop are one contiguous, wave-uniform run that the scalar unit loads.
//   heads_fwd  thread = compact pixel -> its 2 x 2 output block for all OT channels (4 OT accumulators), channels ascending
//   heads_gx   thread = compact pixel -> 32 channels of gx at a time: for every flat channel and tap one value of the output gradient
//              around (2i, 2j) times 32 weights; a gather over all heads, no atomics, no add of per-head gradients
//   heads_gw   split-K: a workgroup owns a strided set of 64-pixel row segments; thread = (4 channels, one flat output channel) with
//              36 accumulators; x and the gradient windows of a segment are staged in LDS; partial sums go to the workspace and
//              heads_gw_finish adds them in a fixed order
// Nothing waits on another workgroup; fp32 only.
#include <array>
#include <utility>

#include "cspn_common.hpp"
#include "cspn_heads.h"

namespace {

constexpr int MAXQ = CSPN_HEADS_MAX_OUT_CHANNELS;
constexpr int GW_PX = 64;                 // compact pixels of a row per segment
constexpr int GW_CB = 64;                 // channels per workgroup (grid.y walks the blocks of a wider map)
constexpr int GW_XS = GW_CB + 4;          // row stride of the staged x tile [pixel][channel] (16-byte aligned rows)
constexpr int GW_GS = 2 * GW_PX + 4;      // row stride of a staged gradient row: column X of the segment sits at X - 2 j0 + 2
constexpr int GW_MAX_GROUPS = 1024;       // partial sums per weight element at most
constexpr int GX_CB = 32;                 // channels of gx a thread holds at a time

// flat output channel q: filter [C][3][3], plane in frame 0 (output, output gradient or — for the finish — filter gradient), frame stride
struct Flat {
    const float* w[MAXQ];
    float* y[MAXQ];
    long ys[MAXQ];
};

// Cp = 0: wp[(c * OT + q) * 9 + k] <- filter q, channel c, tap k.  Cp > 0: wp[(q * 9 + k) * Cp + c] <- the same, 0 for c >= C
__global__ __launch_bounds__(256) void heads_pack(const Flat a, float* __restrict__ wp, int C, int OT, int Cp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= (Cp ? Cp : C) * OT * 9) return;
    int c, q, k;
    if (Cp) {
        const int qk = e / Cp;
        c = e - qk * Cp, q = qk / 9, k = qk - q * 9;
    } else {
        c = e / (OT * 9);
        const int r = e - c * (OT * 9);
        q = r / 9, k = r - q * 9;
    }
    const float* src = nullptr;
#pragma unroll
    for (int m = 0; m < MAXQ; ++m)
        if (q == m) src = a.w[m];
    wp[e] = c < C ? src[c * 9 + k] : 0.f;
}

template <int OT>
__global__ __launch_bounds__(256) void heads_fwd(const float* __restrict__ x, const float* __restrict__ wp, const Flat a, int C, int H, int W,
                                                 int oh, int ow, int Hc, int Wc, int vec) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)Hc * Wc) return;
    const int n = blockIdx.y;
    const int i = p / Wc, j = p - i * Wc;
    const bool right = j + 1 < Wc, down = i + 1 < Hc;          // the neighbour exists in the cropped un-pooled map
    const size_t hw = (size_t)H * W;
    const float* xp = x + (size_t)n * C * hw + (size_t)i * W + j;
    const int o01 = right ? 1 : 0, o10 = down ? W : 0, o11 = o01 + o10;      // a missing neighbour: the load stays inside the frame, the value is dropped
    float acc[OT][4];
#pragma unroll
    for (int q = 0; q < OT; ++q) acc[q][0] = acc[q][1] = acc[q][2] = acc[q][3] = 0.f;
    for (int c = 0; c < C; ++c) {
        const float x00 = xp[0], v01 = xp[o01], v10 = xp[o10], v11 = xp[o11];
        const float x01 = right ? v01 : 0.f;
        const float x10 = down ? v10 : 0.f;
        const float x11 = (right && down) ? v11 : 0.f;
        xp += hw;
#pragma unroll
        for (int q = 0; q < OT; ++q) {
            const float* w = wp + ((size_t)c * OT + q) * 9;     // wave-uniform
            acc[q][0] = fmaf(w[4], x00, acc[q][0]);
            acc[q][1] = fmaf(w[3], x00, acc[q][1]);
            acc[q][1] = fmaf(w[5], x01, acc[q][1]);
            acc[q][2] = fmaf(w[1], x00, acc[q][2]);
            acc[q][2] = fmaf(w[7], x10, acc[q][2]);
            acc[q][3] = fmaf(w[0], x00, acc[q][3]);
            acc[q][3] = fmaf(w[2], x01, acc[q][3]);
            acc[q][3] = fmaf(w[6], x10, acc[q][3]);
            acc[q][3] = fmaf(w[8], x11, acc[q][3]);
        }
    }
    const int Y = 2 * i, X = 2 * j;
    const bool row1 = Y + 1 < oh, col1 = X + 1 < ow;
#pragma unroll
    for (int q = 0; q < OT; ++q) {
        float* dst = a.y[q] + (size_t)n * a.ys[q] + (size_t)Y * ow + X;
        if (vec) {                                               // ow even: both columns exist and both rows are 8-byte aligned
            *reinterpret_cast<float2*>(dst) = make_float2(acc[q][0], acc[q][1]);
            if (row1) *reinterpret_cast<float2*>(dst + ow) = make_float2(acc[q][2], acc[q][3]);
        } else {
            dst[0] = acc[q][0];
            if (col1) dst[1] = acc[q][1];
            if (row1) {
                dst[ow] = acc[q][2];
                if (col1) dst[ow + 1] = acc[q][3];
            }
        }
    }
}

template <int OT>
__global__ __launch_bounds__(256) void heads_gx(const Flat a, const float* __restrict__ wq, float* __restrict__ gx, int C, int Cp, int H,
                                                int W, int oh, int ow) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)H * W) return;
    const int n = blockIdx.y;
    const int i = p / W, j = p - i * W;
    const bool present = 2 * i < oh && 2 * j < ow;               // a pixel the crop removed took no part in the forward
    const size_t hw = (size_t)H * W;
    float* dst = gx + (size_t)n * C * hw + p;
    for (int c0 = 0; c0 < C; c0 += GX_CB) {
        float acc[GX_CB];
#pragma unroll
        for (int c = 0; c < GX_CB; ++c) acc[c] = 0.f;
#pragma unroll
        for (int q = 0; q < OT; ++q) {
            const float* gp = a.y[q] + (size_t)n * a.ys[q];
#pragma unroll 1
            for (int ky = 0; ky < 3; ++ky) {
                const int Y = 2 * i + 1 - ky;                    // tap (ky, kx) meets gy at (2i + 1 - ky, 2j + 1 - kx)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int X = 2 * j + 1 - kx;
                    const bool ok = present && Y >= 0 && Y < oh && X >= 0 && X < ow;
                    const float v = gp[ok ? (size_t)Y * ow + X : 0];      // outside: a load that stays inside the plane, dropped
                    const float g = ok ? v : 0.f;
                    const float* w = wq + (size_t)(q * 9 + ky * 3 + kx) * Cp + c0;      // wave-uniform, 32 in a row
#pragma unroll
                    for (int c = 0; c < GX_CB; ++c) acc[c] = fmaf(w[c], g, acc[c]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < GX_CB; ++c)
            if (c0 + c < C) dst[(size_t)(c0 + c) * hw] = acc[c];
    }
}

template <int OT>
__global__ __launch_bounds__(16 * OT) void heads_gw(const float* __restrict__ x, const Flat a, float* __restrict__ part, int C, int H,
                                                    int W, int oh, int ow, int Hc, int Wc, int nJ, int nsegs) {
    constexpr int T = 16 * OT;
    __shared__ __attribute__((aligned(16))) float xs[GW_PX][GW_XS];
    __shared__ __attribute__((aligned(16))) float gs[OT][3][GW_GS];
    const int t = threadIdx.x, cg = t & 15, q = t >> 4;
    const int c0 = blockIdx.y * GW_CB;
    const size_t hw = (size_t)H * W;
    float acc[4][9];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[ch][k] = 0.f;

    for (int s = blockIdx.x; s < nsegs; s += gridDim.x) {
        const int n = s / (Hc * nJ), rem = s - n * (Hc * nJ);
        const int i = rem / nJ, j0 = (rem - i * nJ) * GW_PX;
        const int npx = min(GW_PX, Wc - j0);
        __syncthreads();                                         // the previous segment has been read
        for (int idx = t; idx < GW_PX * GW_CB; idx += T) {
            const int c = idx / GW_PX, px = idx - c * GW_PX;
            const bool ok = c0 + c < C && px < npx;
            xs[px][c] = ok ? x[((size_t)n * C + c0 + c) * hw + (size_t)i * W + j0 + px] : 0.f;
        }
#pragma unroll
        for (int qq = 0; qq < OT; ++qq) {
            const float* gp = a.y[qq] + (size_t)n * a.ys[qq];
            for (int idx = t; idx < 3 * GW_GS; idx += T) {
                const int r = idx / GW_GS, k = idx - r * GW_GS;
                const int Y = 2 * i - 1 + r, X = 2 * j0 + k - 2;
                const bool ok = k >= 1 && Y >= 0 && Y < oh && X >= 0 && X < ow;
                gs[qq][r][k] = ok ? gp[(size_t)Y * ow + X] : 0.f;
            }
        }
        __syncthreads();
        float left[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) left[r] = gs[q][r][1];       // column 2 j0 - 1
        for (int px = 0; px < npx; ++px) {
            const float4 xv = *reinterpret_cast<const float4*>(&xs[px][4 * cg]);
            const float xc[4] = {xv.x, xv.y, xv.z, xv.w};
            float win[9];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float2 m = *reinterpret_cast<const float2*>(&gs[q][r][2 * px + 2]);     // columns 2j, 2j + 1
                win[r * 3] = left[r];
                win[r * 3 + 1] = m.x;
                win[r * 3 + 2] = m.y;
                left[r] = m.y;
            }
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[ch][k] = fmaf(win[8 - k], xc[ch], acc[ch][k]);
        }
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const int c = c0 + 4 * cg + ch;
        if (c < C) {
            float* dst = part + (((size_t)blockIdx.x * OT + q) * C + c) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) dst[k] = acc[ch][k];
        }
    }
}

// gw element e = (q, c, tap) <- the sum of its `groups` partials: sixteen strided chains, then their sum in slice order
__global__ __launch_bounds__(256) void heads_gw_finish(const float* __restrict__ part, const Flat a, int groups, int C, int elems) {
    __shared__ float red[16][16];
    const int lane = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + lane;
    float s = 0.f;
    if (e < elems)
        for (int g = sl; g < groups; g += 16) s += part[(size_t)g * elems + e];
    red[sl][lane] = s;
    __syncthreads();
    if (sl == 0 && e < elems) {
        const int q = e / (C * 9);
        float* dst = nullptr;
#pragma unroll
        for (int k = 0; k < MAXQ; ++k)
            if (q == k) dst = a.y[k];
        float total = red[0][lane];
#pragma unroll
        for (int k = 1; k < 16; ++k) total += red[k][lane];
        dst[e - q * (C * 9)] = total;
    }
}

int check_shape(const char* who, int N, int C, int H, int W, int oh, int ow) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail("%s: bad shape (N=%d, C=%d, H=%d, W=%d)", who, N, C, H, W);
    if (N > 65535) return fail("%s: more than 65535 frames in one call; split the batch", who);
    if (oh < 1 || ow < 1 || (long)oh > 2L * H || (long)ow > 2L * W)
        return fail("%s: output %dx%d must lie in [1, 2H] x [1, 2W] = %ldx%ld", who, oh, ow, 2L * H, 2L * W);
    if ((double)H * W >= 1073741824.0 || (double)C * 9 * MAXQ >= 2147483648.0) return fail("%s: frame or channel count too large", who);
    return 1;
}

// the heads as flat output channels; per_channel: elements between two channels of `planes[h]`, frame_stride_per_channel: elements
// between two frames of it, divided by O_h (0: the tensor has no frame axis)
int flatten(const char* who, const void* const* weights, void* const* planes, const int* out_channels, int n_heads, int C,
            size_t per_channel, Flat& f, int& total) {
    if (!out_channels || n_heads < 1 || n_heads > CSPN_HEADS_MAX_HEADS) return fail("%s: n_heads must be in [1, %d]", who, CSPN_HEADS_MAX_HEADS);
    total = 0;
    for (int h = 0; h < n_heads; ++h) {
        if (out_channels[h] < 1) return fail("%s: head %d has %d output channels", who, h, out_channels[h]);
        if (total + out_channels[h] > MAXQ) return fail("%s: more than %d output channels over all heads", who, MAXQ);
        if ((weights && !weights[h]) || (planes && !planes[h])) return fail("%s: null pointer (head %d)", who, h);
        for (int o = 0; o < out_channels[h]; ++o, ++total) {
            f.w[total] = weights ? static_cast<const float*>(weights[h]) + (size_t)o * C * 9 : nullptr;
            f.y[total] = planes ? static_cast<float*>(planes[h]) + (size_t)o * per_channel : nullptr;
            f.ys[total] = (long)((size_t)out_channels[h] * per_channel);
        }
    }
    for (int q = total; q < MAXQ; ++q) f.w[q] = nullptr, f.y[q] = nullptr, f.ys[q] = 0;
    return 1;
}

int gw_segments(int N, int oh, int ow, int* nJ) {
    const int Hc = (oh + 1) / 2, Wc = (ow + 1) / 2;
    *nJ = ceil_div(Wc, GW_PX);
    const double segs = (double)N * Hc * *nJ;
    return segs >= 2147483648.0 ? 0 : (int)segs;
}

int launch_pack(const Flat& f, float* wp, int C, int OT, int Cp, hipStream_t st) {
    CSPN_PRE(st), heads_pack<<<dim3(ceil_div((Cp ? Cp : C) * OT * 9, 256)), dim3(256), 0, st>>>(f, wp, C, OT, Cp);
    HIP_OK(hipGetLastError());
    return 1;
}

template <int OT>
int launch_fwd(const float* x, const Flat& f, float* wp, int N, int C, int H, int W, int oh, int ow, hipStream_t st) {
    if (!launch_pack(f, wp, C, OT, 0, st)) return 0;
    const int Hc = (oh + 1) / 2, Wc = (ow + 1) / 2;
    int vec = ow % 2 == 0;
    for (int q = 0; q < OT; ++q) vec = vec && (reinterpret_cast<uintptr_t>(f.y[q]) & 7) == 0 && f.ys[q] % 2 == 0;
    const dim3 grid(((unsigned)Hc * Wc + 255u) / 256u, N), block(256);
    CSPN_PRE(st), heads_fwd<OT><<<grid, block, 0, st>>>(x, wp, f, C, H, W, oh, ow, Hc, Wc, vec);
    HIP_OK(hipGetLastError());
    return 1;
}

template <int OT>
int launch_gx(const Flat& f, float* wp, float* gx, int N, int C, int H, int W, int oh, int ow, hipStream_t st) {
    const int Cp = ceil_div(C, GX_CB) * GX_CB;
    if (!launch_pack(f, wp, C, OT, Cp, st)) return 0;
    const dim3 grid(((unsigned)H * W + 255u) / 256u, N), block(256);
    CSPN_PRE(st), heads_gx<OT><<<grid, block, 0, st>>>(f, wp, gx, C, Cp, H, W, oh, ow);
    HIP_OK(hipGetLastError());
    return 1;
}

template <int OT>
int launch_gw(const float* x, const Flat& gy, const Flat& gw, float* part, int N, int C, int H, int W, int oh, int ow, hipStream_t st) {
    int nJ = 0;
    const int nsegs = gw_segments(N, oh, ow, &nJ);
    const int groups = nsegs < GW_MAX_GROUPS ? nsegs : GW_MAX_GROUPS;
    const dim3 grid(groups, ceil_div(C, GW_CB)), block(16 * OT);
    CSPN_PRE(st), heads_gw<OT><<<grid, block, 0, st>>>(x, gy, part, C, H, W, oh, ow, (oh + 1) / 2, (ow + 1) / 2, nJ, nsegs);
    HIP_OK(hipGetLastError());
    const int elems = OT * C * 9;
    CSPN_PRE(st), heads_gw_finish<<<dim3(ceil_div(elems, 16)), dim3(256), 0, st>>>(part, gw, groups, C, elems);
    HIP_OK(hipGetLastError());
    return 1;
}

template <int... I> constexpr auto fwd_table(std::integer_sequence<int, I...>) { return std::array{&launch_fwd<I + 1>...}; }
template <int... I> constexpr auto gx_table(std::integer_sequence<int, I...>) { return std::array{&launch_gx<I + 1>...}; }
template <int... I> constexpr auto gw_table(std::integer_sequence<int, I...>) { return std::array{&launch_gw<I + 1>...}; }

}  // namespace

extern "C" {

int cspn_heads_abi_version(void) { return CSPN_HEADS_ABI_VERSION; }

size_t cspn_heads_workspace_bytes(int pass, int out_channels, int N, int C, int H, int W, int oh, int ow) {
    if (pass < CSPN_HEADS_FORWARD || pass > CSPN_HEADS_BACKWARD_WEIGHTS || out_channels < 1 || out_channels > MAXQ || N < 1 || N > 65535 || C < 1 || H < 1 || W < 1 || oh < 1 || ow < 1 || (long)oh > 2L * H ||
        (long)ow > 2L * W || (double)C * 9 * MAXQ >= 2147483648.0)
        return 0;
    if (pass == CSPN_HEADS_FORWARD) return (size_t)out_channels * C * 9 * sizeof(float);
    if (pass == CSPN_HEADS_BACKWARD_INPUT) return (size_t)out_channels * 9 * (ceil_div(C, GX_CB) * GX_CB) * sizeof(float);
    int nJ = 0;
    const int nsegs = gw_segments(N, oh, ow, &nJ);
    if (nsegs < 1) return 0;
    const size_t groups = nsegs < GW_MAX_GROUPS ? nsegs : GW_MAX_GROUPS;
    return groups * out_channels * C * 9 * sizeof(float);
}

int cspn_heads_forward(const void* x, const void* const* weights, void* const* outs, const int* out_channels, int n_heads, void* work, int N,
                       int C, int H, int W, int oh, int ow, cspn_stream_t stream) {
    const char* who = "cspn_heads_forward";
    if (!check_shape(who, N, C, H, W, oh, ow)) return 0;
    if (!x || !weights || !outs || !work) return fail("%s: null pointer", who);
    if (!aligned16(work)) return fail("%s: work must be 16-byte aligned", who);
    Flat f;
    int total = 0;
    if (!flatten(who, weights, outs, out_channels, n_heads, C, (size_t)oh * ow, f, total)) return 0;
    static constexpr auto table = fwd_table(std::make_integer_sequence<int, MAXQ>());
    return table[total - 1](static_cast<const float*>(x), f, static_cast<float*>(work), N, C, H, W, oh, ow, static_cast<hipStream_t>(stream));
}

int cspn_heads_backward_input(const void* const* grad_outs, const void* const* weights, const int* out_channels, int n_heads, void* grad_x,
                              void* work, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream) {
    const char* who = "cspn_heads_backward_input";
    if (!check_shape(who, N, C, H, W, oh, ow)) return 0;
    if (!grad_outs || !weights || !grad_x || !work) return fail("%s: null pointer", who);
    if (!aligned16(work)) return fail("%s: work must be 16-byte aligned", who);
    Flat f;
    int total = 0;
    if (!flatten(who, weights, const_cast<void* const*>(grad_outs), out_channels, n_heads, C, (size_t)oh * ow, f, total)) return 0;
    static constexpr auto table = gx_table(std::make_integer_sequence<int, MAXQ>());
    return table[total - 1](f, static_cast<float*>(work), static_cast<float*>(grad_x), N, C, H, W, oh, ow, static_cast<hipStream_t>(stream));
}

int cspn_heads_backward_weights(const void* x, const void* const* grad_outs, void* const* grad_weights, const int* out_channels, int n_heads,
                                void* work, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream) {
    const char* who = "cspn_heads_backward_weights";
    if (!check_shape(who, N, C, H, W, oh, ow)) return 0;
    if (!x || !grad_outs || !grad_weights || !work) return fail("%s: null pointer", who);
    if (!aligned16(work)) return fail("%s: work must be 16-byte aligned", who);
    Flat gy, gw;
    int total = 0, total2 = 0;
    if (!flatten(who, nullptr, const_cast<void* const*>(grad_outs), out_channels, n_heads, C, (size_t)oh * ow, gy, total)) return 0;
    if (!flatten(who, nullptr, grad_weights, out_channels, n_heads, C, (size_t)C * 9, gw, total2)) return 0;
    int nJ = 0;
    if (gw_segments(N, oh, ow, &nJ) < 1) return fail("%s: more than 2^31 row segments; split the batch", who);
    static constexpr auto table = gw_table(std::make_integer_sequence<int, MAXQ>());
    return table[total - 1](static_cast<const float*>(x), gy, gw, static_cast<float*>(work), N, C, H, W, oh, ow, static_cast<hipStream_t>(stream));
}

}  // extern "C"

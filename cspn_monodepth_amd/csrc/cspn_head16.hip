// cspn_head16.hip — the two output heads of the decoders fused with their un-pooling, in half precision, on the fp16 matrix cores
// (include/cspn_head16.h).  The fp32 forward and the gradients are cspn_heads.hip.
//
// All heads are run as one list of OT <= 16 flat output channels: exactly the M tile of v_mfma_f32_16x16x32_f16.  Output pixel
// (2i + a, 2j + b) of the pad-1 3x3 window over the un-pooled map touches compact pixels
//   (0,0): (i,j) under tap (1,1)            (0,1): (i,j) (1,0), (i,j+1) (1,2)
//   (1,0): (i,j) (0,1), (i+1,j) (2,1)       (1,1): (i,j) (0,0), (i,j+1) (0,2), (i+1,j) (2,0), (i+1,j+1) (2,2)
// so each of the four phases is a GEMM  [16 channels] x [K = taps of the phase x C] x [compact pixels]  with 1, 2, 2 and 4 taps: nine
// matrix instructions per 32 channels and 16 pixels, and their results ARE the outputs — nothing is combined across lanes.
//   pack   head16_pack writes the filters of the call as fp16 into the caller's workspace, wp[tap][16][Cp], Cp = C rounded up to 32,
//          rows past OT and channels past C zero.  Channel-contiguous: the 8 channels lane l holds of row l & 15
//          (A[l & 15][8 (l >> 4) + j]) are 16 consecutive bytes, read from global memory (9 KiB per 32 channels, in L1 / L2).
//   fwd    a workgroup of 4 wavefronts owns a tile of 8 x 32 compact pixels of one frame and walks the channels in blocks of 32.  The
//          tile with a halo of one pixel to the right and below (9 x 33 pixels) is staged in LDS channel-contiguous, in rows of 80 bytes
//          (64 of data + 16 of padding, the rows of the F16 policy of cspn_upconv_core.hpp: the 16 lanes a ds_read_b128 serves in one
//          cycle start 20 banks apart, all different).  The NCHW gather is 2-byte loads, consecutive lanes on consecutive pixels of a
//          row; the next block's loads are in flight while this block's products run.  A wavefront takes two tile rows as four groups
//          of 16 pixels: lane l holds pixel l & 15 of a group as the B operand (B[8 (l >> 4) + j][l & 15]), reads the pixel, its right,
//          lower and lower-right neighbour once per block (4 x ds_read_b128) and issues the 9 instructions on them.  A pixel the crop
//          removed (2i >= oh or 2j >= ow) is staged as zeros and never loaded.
//   store  lane l holds rows 4 (l >> 4) + r, r = 0..3, of column l & 15 of every phase: both b-phases of its pixel, stored as one
//          4-byte pair per channel and output row where ow is even and the outputs are 4-byte aligned, as 2-byte stores otherwise.
// LDS: 23 760 bytes per workgroup.  Nothing waits on another workgroup; no atomics.
#include "cspn_common.hpp"
#include "cspn_head16.h"

namespace {

constexpr int MAXQ = CSPN_HEAD16_MAX_OUT_CHANNELS;
constexpr int TH = CSPN_HEAD16_TILE_H, TW = CSPN_HEAD16_TILE_W;       // compact pixels of a tile
constexpr int KC = CSPN_HEAD16_CHANNEL_BLOCK;                         // channels per step: the K of the instruction
constexpr int PH = TH + 1, PW = TW + 1, NPX = PH * PW;                // the staged tile: a halo of one pixel to the right and below
constexpr int ROW8 = KC / 8 + 1;                                      // an LDS row in 16-byte fragments: 4 of data, 1 of padding
constexpr int THREADS = 256;
constexpr int ITEMS = NPX * (KC / 8);                                 // (pixel, group of 8 channels) pairs of a block
constexpr int LOADS = (ITEMS + THREADS - 1) / THREADS;
static_assert(MAXQ == 16 && KC == 32 && TW % 16 == 0 && (TW / 16) * TH == 4 * (THREADS / 64), "a wavefront takes four groups of 16 pixels");

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef _Float16 v2h __attribute__((ext_vector_type(2)));

// flat output channel q: filter [C][3][3] (fp32 or fp16), plane in frame 0, frame stride in elements
struct Flat {
    const void* w[MAXQ];
    _Float16* y[MAXQ];
    long ys[MAXQ];
};

// wp[(tap * 16 + q) * Cp + c] <- fp16(filter q, channel c, tap), 0 for q >= OT or c >= C
template <typename WT>
__global__ __launch_bounds__(256) void head16_pack(const Flat a, _Float16* __restrict__ wp, int C, int OT, int Cp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 9 * MAXQ * Cp) return;
    const int r = e / Cp, c = e - r * Cp, q = r & (MAXQ - 1), tap = r / MAXQ;
    const WT* src = nullptr;
#pragma unroll
    for (int m = 0; m < MAXQ; ++m)
        if (q == m) src = static_cast<const WT*>(a.w[m]);
    _Float16 v = (_Float16)0.f;
    if (q < OT && c < C) v = (_Float16)src[c * 9 + tap];              // fp32 -> fp16: to nearest even
    wp[e] = v;
}

__device__ __forceinline__ v4f mma(v8h a, v8h b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(THREADS) void head16_fwd(const _Float16* __restrict__ x, const _Float16* __restrict__ wp, const Flat a, int C, int Cp,
                                                      int H, int W, int oh, int ow, int Hc, int Wc, int tiles_x, int OT, int vec) {
    __shared__ v8h Bs[NPX][ROW8];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, col = l & 15, f = l >> 4;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int i0 = ty * TH, j0 = tx * TW, n = blockIdx.y;
    const size_t hw = (size_t)H * W;
    const _Float16* xn = x + (size_t)n * C * hw;

    // what this thread fetches of every block: pixel p of the staged tile, channels 8 kg .. 8 kg + 7 of the block
    int off[LOADS], slot[LOADS];
    bool there[LOADS];
#pragma unroll
    for (int r = 0; r < LOADS; ++r) {
        const int idx = t + THREADS * r, kg = idx / NPX, p = idx - kg * NPX;
        const int pr = p / PW, pc = p - pr * PW, gi = i0 + pr, gj = j0 + pc;
        slot[r] = idx < ITEMS ? p * ROW8 + kg : -1;
        there[r] = idx < ITEMS && gi < Hc && gj < Wc;                 // inside the frame, and not removed by the crop
        off[r] = there[r] ? gi * W + gj : 0;
    }
    v8h xv[LOADS];
    auto load = [&](int c0) {
#pragma unroll
        for (int r = 0; r < LOADS; ++r) {
            const int idx = t + THREADS * r, kg = idx / NPX;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = c0 + 8 * kg + j;
                xv[r][j] = (there[r] && c < C) ? xn[(size_t)c * hw + off[r]] : (_Float16)0.f;
            }
        }
    };

    v4f acc[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) acc[g][ph] = v4f{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int c0 = 0; c0 < Cp; c0 += KC) {
        v8h wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const v8h*>(wp + (size_t)(k * MAXQ + col) * Cp + c0 + 8 * f);
        __syncthreads();                                              // the previous block has been read
#pragma unroll
        for (int r = 0; r < LOADS; ++r)
            if (slot[r] >= 0) (&Bs[0][0])[slot[r]] = xv[r];
        __syncthreads();
        if (c0 + KC < Cp) load(c0 + KC);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int base = (2 * wv + (g >> 1)) * PW + 16 * (g & 1) + col;
            const v8h p00 = Bs[base][f], p01 = Bs[base + 1][f], p10 = Bs[base + PW][f], p11 = Bs[base + PW + 1][f];
            acc[g][0] = mma(wt[4], p00, acc[g][0]);
            acc[g][1] = mma(wt[3], p00, acc[g][1]);
            acc[g][1] = mma(wt[5], p01, acc[g][1]);
            acc[g][2] = mma(wt[1], p00, acc[g][2]);
            acc[g][2] = mma(wt[7], p10, acc[g][2]);
            acc[g][3] = mma(wt[0], p00, acc[g][3]);
            acc[g][3] = mma(wt[2], p01, acc[g][3]);
            acc[g][3] = mma(wt[6], p10, acc[g][3]);
            acc[g][3] = mma(wt[8], p11, acc[g][3]);
        }
    }

    // rows 4 f + r of this lane: their planes and frame strides (static indices into the kernel arguments)
    _Float16* yq[4];
    long ysq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        yq[r] = a.y[r], ysq[r] = a.ys[r];
#pragma unroll
        for (int ff = 1; ff < 4; ++ff)
            if (f == ff) yq[r] = a.y[4 * ff + r], ysq[r] = a.ys[4 * ff + r];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int i = i0 + 2 * wv + (g >> 1), j = j0 + 16 * (g & 1) + col;
        if (i >= Hc || j >= Wc) continue;
        const int Y = 2 * i, X = 2 * j;
        const bool row1 = Y + 1 < oh, col1 = X + 1 < ow;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (4 * f + r >= OT) continue;                            // computed, not stored
            _Float16* dst = yq[r] + (size_t)n * ysq[r] + (size_t)Y * ow + X;
            const _Float16 v00 = (_Float16)acc[g][0][r], v01 = (_Float16)acc[g][1][r], v10 = (_Float16)acc[g][2][r], v11 = (_Float16)acc[g][3][r];
            if (vec) {                                                // ow even: both columns exist and both rows are 4-byte aligned
                *reinterpret_cast<v2h*>(dst) = v2h{v00, v01};
                if (row1) *reinterpret_cast<v2h*>(dst + ow) = v2h{v10, v11};
            } else {
                dst[0] = v00;
                if (col1) dst[1] = v01;
                if (row1) {
                    dst[ow] = v10;
                    if (col1) dst[ow + 1] = v11;
                }
            }
        }
    }
}

int padded_channels(int C) { return ceil_div(C, KC) * KC; }

bool sizes_ok(int out_channels, int C) {
    return out_channels >= 1 && out_channels <= MAXQ && C >= 1 && (double)9 * MAXQ * ((double)C + KC) < 2147483648.0;
}

}  // namespace

extern "C" {

int cspn_head16_abi_version(void) { return CSPN_HEAD16_ABI_VERSION; }

size_t cspn_head16_workspace_bytes(int out_channels, int C) {
    if (!sizes_ok(out_channels, C)) return 0;
    return (size_t)9 * MAXQ * padded_channels(C) * sizeof(_Float16);
}

int cspn_head16_forward(const void* x, const void* const* weights, int weight_dtype, void* const* outs, const int* out_channels, int n_heads,
                        void* work, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream) {
    const char* who = "cspn_head16_forward";
    if (N < 1 || C < 1 || H < 1 || W < 1) return fail("%s: bad shape (N=%d, C=%d, H=%d, W=%d)", who, N, C, H, W);
    if (N > 65535) return fail("%s: more than 65535 frames in one call; split the batch", who);
    if (oh < 1 || ow < 1 || (long)oh > 2L * H || (long)ow > 2L * W)
        return fail("%s: output %dx%d must lie in [1, 2H] x [1, 2W] = %ldx%ld", who, oh, ow, 2L * H, 2L * W);
    if (weight_dtype != CSPN_F32 && weight_dtype != CSPN_F16) return fail("%s: weight_dtype must be fp32 or fp16, got %d", who, weight_dtype);
    if (!x || !weights || !outs || !out_channels || !work) return fail("%s: null pointer", who);
    if (!aligned16(work)) return fail("%s: work must be 16-byte aligned", who);
    if (n_heads < 1 || n_heads > CSPN_HEAD16_MAX_HEADS) return fail("%s: n_heads must be in [1, %d]", who, CSPN_HEAD16_MAX_HEADS);
    if ((double)N * C * H * W >= 2147483648.0) return fail("%s: x has 2^31 elements or more; split the batch", who);
    if (!sizes_ok(1, C)) return fail("%s: the filters of %d channels have 2^31 elements or more", who, C);
    Flat f;
    int total = 0;
    const size_t plane = (size_t)oh * ow, wsize = weight_dtype == CSPN_F32 ? 4 : 2;
    for (int h = 0; h < n_heads; ++h) {
        const int O = out_channels[h];
        if (O < 1) return fail("%s: head %d has %d output channels", who, h, O);
        if (total + O > MAXQ) return fail("%s: more than %d output channels over all heads", who, MAXQ);
        if (!weights[h] || !outs[h]) return fail("%s: null pointer (head %d)", who, h);
        if ((double)N * O * oh * ow >= 2147483648.0) return fail("%s: output %d has 2^31 elements or more; split the batch", who, h);
        for (int o = 0; o < O; ++o, ++total) {
            f.w[total] = static_cast<const char*>(weights[h]) + (size_t)o * C * 9 * wsize;
            f.y[total] = static_cast<_Float16*>(outs[h]) + (size_t)o * plane;
            f.ys[total] = (long)((size_t)O * plane);
        }
    }
    int vec = ow % 2 == 0;
    for (int q = 0; q < total; ++q) vec = vec && (reinterpret_cast<uintptr_t>(f.y[q]) & 3) == 0 && f.ys[q] % 2 == 0;
    for (int q = total; q < MAXQ; ++q) f.w[q] = nullptr, f.y[q] = nullptr, f.ys[q] = 0;

    hipStream_t st = static_cast<hipStream_t>(stream);
    _Float16* wp = static_cast<_Float16*>(work);
    const int Cp = padded_channels(C);
    const dim3 pgrid(ceil_div(9 * MAXQ * Cp, 256)), pblock(256);
    if (weight_dtype == CSPN_F32) CSPN_PRE(st), head16_pack<float><<<pgrid, pblock, 0, st>>>(f, wp, C, total, Cp);
    else CSPN_PRE(st), head16_pack<_Float16><<<pgrid, pblock, 0, st>>>(f, wp, C, total, Cp);
    HIP_OK(hipGetLastError());
    const int Hc = (oh + 1) / 2, Wc = (ow + 1) / 2;
    const int tiles_x = ceil_div(Wc, TW), tiles_y = ceil_div(Hc, TH);
    const dim3 grid((unsigned)tiles_x * tiles_y, N), block(THREADS);
    CSPN_PRE(st), head16_fwd<<<grid, block, 0, st>>>(static_cast<const _Float16*>(x), wp, f, C, Cp, H, W, oh, ow, Hc, Wc, tiles_x, total, vec);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

// cspn_visual.hip — the reference's comparison images (libs/utils.py:69-192; the sheet of trainer.eval,
// libs/trainers/single_gpu_trainer.py:140-175) as two launches (include/cspn_visual.h).
//
// Launch 1, cspn_visual_range_kernel: grid (chunks, range units, frames).  A workgroup reduces one chunk of CSPN_VISUAL_RANGE_CHUNK
// elements of one unit of one frame to a NaN-propagating (min, max) pair — wave64 butterflies, then the 4 wavefronts through LDS —
// and writes it to its own slot of the workspace.  No atomics, no counters: launch 2 reads every slot its frame owns.
//
// Launch 2, cspn_visual_colour_kernel: grid (ceil(H * quads per row / 256), frames).  Every workgroup stages the 256 x 3 byte table
// as 257 packed words in LDS (entry 256: black, for NaN), folds ITS frame's partials (a few dozen floats, L2 hits), combines the
// units in argument order by Python's min / max rule, and then each thread turns 4 consecutive pixels of an output row into 12
// bytes.  A row is P * W * 3 bytes and may start anywhere: the three words are stored as dwords when the thread's 12 bytes begin
// on the 4-byte grid, otherwise as (4 - a) head bytes, two funnel-shifted dwords and a tail bytes; a row's last, partial quad goes
// out byte by byte.  Adjacent lanes write adjacent 12-byte spans.  With W % 4 == 0 and 16-byte aligned planes a quad lies in one
// panel and is read with one 16-byte load per plane; otherwise pixel by pixel, each with its own panel.
//
// Every arithmetic step is one rounded fp32 operation (__fsub_rn, __fdiv_rn, __fmul_rn; contraction off); the division is IEEE.
#include <climits>

#include "cspn_common.hpp"
#include "cspn_visual.h"

namespace {

constexpr int VIS_THREADS = 256;
constexpr int VIS_WAVES = VIS_THREADS / 64;
constexpr int VIS_QUADS = CSPN_VISUAL_RANGE_CHUNK / (4 * VIS_THREADS);
static_assert(VIS_QUADS * 4 * VIS_THREADS == CSPN_VISUAL_RANGE_CHUNK, "a chunk is a whole number of 16-byte units per thread");
constexpr int VIS_GRID_YZ = 65535;

// uint8(255 * matplotlib.cm.jet(i)[:3]) for i = 0 .. 255, truncated in float64 (golden G25: tests/golden/g25_visual_table.npz)
__device__ const unsigned char VIS_JET[256][3] = {
    // <jet-bytes>
    {0,0,127}, {0,0,132}, {0,0,136}, {0,0,141}, {0,0,145}, {0,0,150}, {0,0,154}, {0,0,159},
    {0,0,163}, {0,0,168}, {0,0,172}, {0,0,177}, {0,0,182}, {0,0,186}, {0,0,191}, {0,0,195},
    {0,0,200}, {0,0,204}, {0,0,209}, {0,0,213}, {0,0,218}, {0,0,222}, {0,0,227}, {0,0,232},
    {0,0,236}, {0,0,241}, {0,0,245}, {0,0,250}, {0,0,254}, {0,0,255}, {0,0,255}, {0,0,255},
    {0,0,255}, {0,4,255}, {0,8,255}, {0,12,255}, {0,16,255}, {0,20,255}, {0,24,255}, {0,28,255},
    {0,32,255}, {0,36,255}, {0,40,255}, {0,44,255}, {0,48,255}, {0,52,255}, {0,56,255}, {0,60,255},
    {0,64,255}, {0,68,255}, {0,72,255}, {0,76,255}, {0,80,255}, {0,84,255}, {0,88,255}, {0,92,255},
    {0,96,255}, {0,100,255}, {0,104,255}, {0,108,255}, {0,112,255}, {0,116,255}, {0,120,255}, {0,124,255},
    {0,128,255}, {0,132,255}, {0,136,255}, {0,140,255}, {0,144,255}, {0,148,255}, {0,152,255}, {0,156,255},
    {0,160,255}, {0,164,255}, {0,168,255}, {0,172,255}, {0,176,255}, {0,180,255}, {0,184,255}, {0,188,255},
    {0,192,255}, {0,196,255}, {0,200,255}, {0,204,255}, {0,208,255}, {0,212,255}, {0,216,255}, {0,220,254},
    {0,224,250}, {0,228,247}, {2,232,244}, {5,236,241}, {8,240,237}, {12,244,234}, {15,248,231}, {18,252,228},
    {21,255,225}, {24,255,221}, {28,255,218}, {31,255,215}, {34,255,212}, {37,255,208}, {41,255,205}, {44,255,202},
    {47,255,199}, {50,255,195}, {54,255,192}, {57,255,189}, {60,255,186}, {63,255,183}, {66,255,179}, {70,255,176},
    {73,255,173}, {76,255,170}, {79,255,166}, {83,255,163}, {86,255,160}, {89,255,157}, {92,255,154}, {95,255,150},
    {99,255,147}, {102,255,144}, {105,255,141}, {108,255,137}, {112,255,134}, {115,255,131}, {118,255,128}, {121,255,125},
    {124,255,121}, {128,255,118}, {131,255,115}, {134,255,112}, {137,255,108}, {141,255,105}, {144,255,102}, {147,255,99},
    {150,255,95}, {154,255,92}, {157,255,89}, {160,255,86}, {163,255,83}, {166,255,79}, {170,255,76}, {173,255,73},
    {176,255,70}, {179,255,66}, {183,255,63}, {186,255,60}, {189,255,57}, {192,255,54}, {195,255,50}, {199,255,47},
    {202,255,44}, {205,255,41}, {208,255,37}, {212,255,34}, {215,255,31}, {218,255,28}, {221,255,24}, {224,255,21},
    {228,255,18}, {231,255,15}, {234,255,12}, {237,255,8}, {241,252,5}, {244,248,2}, {247,244,0}, {250,240,0},
    {254,237,0}, {255,233,0}, {255,229,0}, {255,226,0}, {255,222,0}, {255,218,0}, {255,215,0}, {255,211,0},
    {255,207,0}, {255,203,0}, {255,200,0}, {255,196,0}, {255,192,0}, {255,189,0}, {255,185,0}, {255,181,0},
    {255,177,0}, {255,174,0}, {255,170,0}, {255,166,0}, {255,163,0}, {255,159,0}, {255,155,0}, {255,152,0},
    {255,148,0}, {255,144,0}, {255,140,0}, {255,137,0}, {255,133,0}, {255,129,0}, {255,126,0}, {255,122,0},
    {255,118,0}, {255,115,0}, {255,111,0}, {255,107,0}, {255,103,0}, {255,100,0}, {255,96,0}, {255,92,0},
    {255,89,0}, {255,85,0}, {255,81,0}, {255,77,0}, {255,74,0}, {255,70,0}, {255,66,0}, {255,63,0},
    {255,59,0}, {255,55,0}, {255,52,0}, {255,48,0}, {255,44,0}, {255,40,0}, {255,37,0}, {255,33,0},
    {255,29,0}, {255,26,0}, {255,22,0}, {254,18,0}, {250,15,0}, {245,11,0}, {241,7,0}, {236,3,0},
    {232,0,0}, {227,0,0}, {222,0,0}, {218,0,0}, {213,0,0}, {209,0,0}, {204,0,0}, {200,0,0},
    {195,0,0}, {191,0,0}, {186,0,0}, {182,0,0}, {177,0,0}, {172,0,0}, {168,0,0}, {163,0,0},
    {159,0,0}, {154,0,0}, {150,0,0}, {145,0,0}, {141,0,0}, {136,0,0}, {132,0,0}, {127,0,0},
    // </jet-bytes>
};

struct VisArgs {
    const void* rgb;
    long rgb_fs, rgb_cs;
    const float* src[CSPN_VISUAL_MAX_PLANES];
    long src_fs[CSPN_VISUAL_MAX_PLANES];
    long panel_stride;              // features: colour panel k is src[0] + k * panel_stride; rows: panel k is src[k]
    size_t range_elems;             // elements of one range unit
    unsigned char* out;
    size_t out_fs;
    float* work;                    // [B][n_range][n_chunks][2]
    int rgb_kind, n_range, n_chunks, n_colour, feature, use_min, use_max, H, W, vec;
    float rgb_scale, d_min, d_max;
};

// np.min / np.max of two values: a NaN on either side stays
__device__ __forceinline__ float nan_min(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

// (min, max) over the workgroup, in every thread.  red: VIS_WAVES x 2 floats of LDS; ends behind a barrier that frees it again
__device__ __forceinline__ void block_range(float& mn, float& mx, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = nan_min(mn, __shfl_xor(mn, off, 64));
        mx = nan_max(mx, __shfl_xor(mx, off, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[2 * wave] = mn;
        red[2 * wave + 1] = mx;
    }
    __syncthreads();
    mn = red[0];
    mx = red[1];
#pragma unroll
    for (int w = 1; w < VIS_WAVES; ++w) {
        mn = nan_min(mn, red[2 * w]);
        mx = nan_max(mx, red[2 * w + 1]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(VIS_THREADS) void cspn_visual_range_kernel(const VisArgs a) {
    __shared__ float red[2 * VIS_WAVES];
    const int c = blockIdx.x, u = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const float* base = (u == 0 ? a.src[0] : (u == 1 ? a.src[1] : a.src[2])) + (size_t)b * (u == 0 ? a.src_fs[0] : (u == 1 ? a.src_fs[1] : a.src_fs[2]));
    const size_t off = (size_t)c * CSPN_VISUAL_RANGE_CHUNK;
    const size_t left = a.range_elems - off;
    const int len = left < (size_t)CSPN_VISUAL_RANGE_CHUNK ? (int)left : CSPN_VISUAL_RANGE_CHUNK;
    const float* p = base + off;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(base) & 15) == 0) {          // off keeps the alignment
        done = len & ~3;
#pragma unroll
        for (int k = 0; k < VIS_QUADS; ++k) {
            const int i = (k * VIS_THREADS + tid) * 4;
            if (i < done) {
                const float4 v = ld4(p + i);
                mn = nan_min(nan_min(nan_min(nan_min(mn, v.x), v.y), v.z), v.w);
                mx = nan_max(nan_max(nan_max(nan_max(mx, v.x), v.y), v.z), v.w);
            }
        }
    }
    for (int i = done + tid; i < len; i += VIS_THREADS) {
        const float v = p[i];
        mn = nan_min(mn, v);
        mx = nan_max(mx, v);
    }
    block_range(mn, mx, red);
    if (tid == 0) {
        float* slot = a.work + (((size_t)b * a.n_range + u) * a.n_chunks + c) * 2;
        slot[0] = mn;
        slot[1] = mx;
    }
}

__device__ __forceinline__ unsigned colour_of(float d, float d_min, float span, const unsigned* lut) {
#pragma clang fp contract(off)
    const float rel = __fdiv_rn(__fsub_rn(d, d_min), span);
    const float x = __fmul_rn(rel, 256.f);
    const int i = (x != x) ? 256 : (x >= 256.f ? 255 : (x > 0.f ? (int)x : 0));
    return lut[i];
}

__device__ __forceinline__ unsigned byte_of(float v, float scale) {     // trunc(scale * v), saturated; NaN -> 0
#pragma clang fp contract(off)
    const float x = __fmul_rn(scale, v);
    return x >= 256.f ? 255u : (x > 0.f ? (unsigned)x : 0u);
}

template <int I> __device__ __forceinline__ unsigned char span_byte(const unsigned (&w)[3]) { return (unsigned char)(w[I / 4] >> (8 * (I % 4))); }

// the 12 bytes of w to p, p % 4 == A != 0: 4 - A bytes, the two dwords on the grid, A bytes
template <int A> __device__ __forceinline__ void store_span_off_grid(unsigned char* p, const unsigned (&w)[3]) {
    p[0] = span_byte<0>(w);
    if (A <= 2) p[1] = span_byte<1>(w);
    if (A <= 1) p[2] = span_byte<2>(w);
    constexpr int O = 4 - A, S = 8 * O;
    unsigned* q = reinterpret_cast<unsigned*>(p + O);
    q[0] = (w[0] >> S) | (w[1] << (32 - S));
    q[1] = (w[1] >> S) | (w[2] << (32 - S));
    if (A >= 3) p[9] = span_byte<9>(w);
    if (A >= 2) p[10] = span_byte<10>(w);
    p[11] = span_byte<11>(w);
}

template <int I> __device__ __forceinline__ void store_span_bytes(unsigned char* p, const unsigned (&w)[3], int nb) {
    if constexpr (I < 9) {
        if (I < nb) p[I] = span_byte<I>(w);
        store_span_bytes<I + 1>(p, w, nb);
    }
}

__global__ __launch_bounds__(VIS_THREADS) void cspn_visual_colour_kernel(const VisArgs a) {
    __shared__ unsigned lut[257];
    __shared__ float red[2 * VIS_WAVES];
    const int tid = threadIdx.x, b = blockIdx.y;
    lut[tid] = (unsigned)VIS_JET[tid][0] | ((unsigned)VIS_JET[tid][1] << 8) | ((unsigned)VIS_JET[tid][2] << 16);
    if (tid == 0) lut[256] = 0u;
    float d_min = a.d_min, d_max = a.d_max;
    if (!(a.use_min && a.use_max)) {
        float lo = 0.f, hi = 0.f;
        for (int u = 0; u < a.n_range; ++u) {
            const float* part = a.work + ((size_t)b * a.n_range + u) * a.n_chunks * 2;
            float mn = __builtin_inff(), mx = -__builtin_inff();
            for (int c = tid; c < a.n_chunks; c += VIS_THREADS) {
                const float2 v = *reinterpret_cast<const float2*>(part + 2 * (size_t)c);
                mn = nan_min(mn, v.x);
                mx = nan_max(mx, v.y);
            }
            block_range(mn, mx, red);
            // Python's min(a, b, ..) / max(a, b, ..): the first stays unless a later one compares strictly less / greater
            lo = (u == 0 || mn < lo) ? mn : lo;
            hi = (u == 0 || mx > hi) ? mx : hi;
        }
        if (!a.use_min) d_min = lo;
        if (!a.use_max) d_max = hi;
    }
    __syncthreads();                                              // the table is staged
    const int has_rgb = a.rgb_kind != CSPN_VISUAL_RGB_NONE;
    const int W = a.W, PW = (has_rgb + a.n_colour) * W, QR = (PW + 3) >> 2;
    const long long t = (long long)blockIdx.x * VIS_THREADS + tid;
    if (t >= (long long)a.H * QR) return;
    const int y = (int)(t / QR), q = (int)(t - (long long)y * QR);
    const int x0 = 4 * q;
    const int npix = PW - x0 < 4 ? PW - x0 : 4;
    const float span = __fsub_rn(d_max, d_min);
    const size_t row = (size_t)y * W;
    unsigned c[4] = {0u, 0u, 0u, 0u};
    if (a.vec) {                                                  // W % 4 == 0: the quad lies in one panel, npix == 4
        const int panel = x0 / W, xx = x0 - panel * W;
        if (panel < has_rgb) {
            if (a.rgb_kind == CSPN_VISUAL_RGB_F32) {
                const float* r = static_cast<const float*>(a.rgb) + (size_t)b * a.rgb_fs + row + xx;
                const float4 v0 = ld4(r), v1 = ld4(r + a.rgb_cs), v2 = ld4(r + 2 * a.rgb_cs);
                c[0] = byte_of(v0.x, a.rgb_scale) | (byte_of(v1.x, a.rgb_scale) << 8) | (byte_of(v2.x, a.rgb_scale) << 16);
                c[1] = byte_of(v0.y, a.rgb_scale) | (byte_of(v1.y, a.rgb_scale) << 8) | (byte_of(v2.y, a.rgb_scale) << 16);
                c[2] = byte_of(v0.z, a.rgb_scale) | (byte_of(v1.z, a.rgb_scale) << 8) | (byte_of(v2.z, a.rgb_scale) << 16);
                c[3] = byte_of(v0.w, a.rgb_scale) | (byte_of(v1.w, a.rgb_scale) << 8) | (byte_of(v2.w, a.rgb_scale) << 16);
            } else {
                const unsigned char* r = static_cast<const unsigned char*>(a.rgb) + (size_t)b * a.rgb_fs + row + xx;
                const unsigned v0 = *reinterpret_cast<const unsigned*>(r), v1 = *reinterpret_cast<const unsigned*>(r + a.rgb_cs),
                               v2 = *reinterpret_cast<const unsigned*>(r + 2 * a.rgb_cs);
#pragma unroll
                for (int j = 0; j < 4; ++j) c[j] = ((v0 >> (8 * j)) & 255u) | (((v1 >> (8 * j)) & 255u) << 8) | (((v2 >> (8 * j)) & 255u) << 16);
            }
        } else {
            const int k = panel - has_rgb;
            const float* s = a.feature ? a.src[0] + (size_t)b * a.src_fs[0] + (size_t)k * a.panel_stride
                                       : (k == 0 ? a.src[0] + (size_t)b * a.src_fs[0] : (k == 1 ? a.src[1] + (size_t)b * a.src_fs[1] : a.src[2] + (size_t)b * a.src_fs[2]));
            const float4 v = ld4(s + row + xx);
            c[0] = colour_of(v.x, d_min, span, lut);
            c[1] = colour_of(v.y, d_min, span, lut);
            c[2] = colour_of(v.z, d_min, span, lut);
            c[3] = colour_of(v.w, d_min, span, lut);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= npix) break;
            const int x = x0 + j, panel = x / W, xx = x - panel * W;
            if (panel < has_rgb) {
                if (a.rgb_kind == CSPN_VISUAL_RGB_F32) {
                    const float* r = static_cast<const float*>(a.rgb) + (size_t)b * a.rgb_fs + row + xx;
                    c[j] = byte_of(r[0], a.rgb_scale) | (byte_of(r[a.rgb_cs], a.rgb_scale) << 8) | (byte_of(r[2 * a.rgb_cs], a.rgb_scale) << 16);
                } else {
                    const unsigned char* r = static_cast<const unsigned char*>(a.rgb) + (size_t)b * a.rgb_fs + row + xx;
                    c[j] = (unsigned)r[0] | ((unsigned)r[a.rgb_cs] << 8) | ((unsigned)r[2 * a.rgb_cs] << 16);
                }
            } else {
                const int k = panel - has_rgb;
                const float* s = a.feature ? a.src[0] + (size_t)b * a.src_fs[0] + (size_t)k * a.panel_stride
                                           : (k == 0 ? a.src[0] + (size_t)b * a.src_fs[0] : (k == 1 ? a.src[1] + (size_t)b * a.src_fs[1] : a.src[2] + (size_t)b * a.src_fs[2]));
                c[j] = colour_of(s[row + xx], d_min, span, lut);
            }
        }
    }
    const unsigned w[3] = {c[0] | (c[1] << 24), (c[1] >> 8) | (c[2] << 16), (c[2] >> 16) | (c[3] << 8)};
    unsigned char* p = a.out + (size_t)b * a.out_fs + (size_t)y * PW * 3 + (size_t)q * 12;
    if (npix == 4) {
        switch (reinterpret_cast<uintptr_t>(p) & 3) {
            case 0: {
                unsigned* d = reinterpret_cast<unsigned*>(p);
                d[0] = w[0];
                d[1] = w[1];
                d[2] = w[2];
                break;
            }
            case 1: store_span_off_grid<1>(p, w); break;
            case 2: store_span_off_grid<2>(p, w); break;
            default: store_span_off_grid<3>(p, w); break;
        }
    } else {
        store_span_bytes<0>(p, w, 3 * npix);
    }
}

int visual_chunks(const char* who, size_t elements, int* out) {
    const size_t c = elements / CSPN_VISUAL_RANGE_CHUNK + (elements % CSPN_VISUAL_RANGE_CHUNK ? 1 : 0);
    if (elements == 0 || c > (size_t)INT_MAX) return fail("%s: %zu elements per range unit", who, elements);
    *out = (int)c;
    return 1;
}

// the checks and the two launches behind both entry points; `a` holds everything but n_chunks and vec
int visual_launch(const char* who, VisArgs a, int B, void* work, hipStream_t st) {
    if (B < 1 || B > VIS_GRID_YZ) return fail("%s: B %d (1 .. %d)", who, B, VIS_GRID_YZ);
    if (a.H < 1 || a.W < 1) return fail("%s: H %d, W %d", who, a.H, a.W);
    const int panels = (a.rgb_kind != CSPN_VISUAL_RGB_NONE) + a.n_colour;
    if ((long long)panels * a.W > INT_MAX / 4) return fail("%s: a row of %d panels of %d pixels is too long", who, panels, a.W);
    const int QR = (panels * a.W + 3) / 4;
    const long long blocks = ((long long)a.H * QR + VIS_THREADS - 1) / VIS_THREADS;
    if (blocks > INT_MAX) return fail("%s: %d rows of %d pixels are more than a launch covers", who, a.H, panels * a.W);
    if (!a.out) return fail("%s: out is NULL", who);
    if (a.rgb_kind != CSPN_VISUAL_RGB_NONE && a.rgb_kind != CSPN_VISUAL_RGB_F32 && a.rgb_kind != CSPN_VISUAL_RGB_U8) return fail("%s: rgb_kind %d", who, a.rgb_kind);
    if (a.rgb_kind != CSPN_VISUAL_RGB_NONE && !a.rgb) return fail("%s: rgb is NULL", who);
    if (a.rgb_kind == CSPN_VISUAL_RGB_F32 && (reinterpret_cast<uintptr_t>(a.rgb) & 3)) return fail("%s: rgb is not aligned to its element size", who);
    bool vec = a.W % 4 == 0;
    for (int k = 0; k < a.n_range; ++k) {
        if (!a.src[k]) return fail("%s: plane %d is NULL", who, k);
        if (reinterpret_cast<uintptr_t>(a.src[k]) & 3) return fail("%s: plane %d is not aligned to its element size", who, k);
        vec = vec && aligned16(a.src[k]) && a.src_fs[k] % 4 == 0;
    }
    vec = vec && a.panel_stride % 4 == 0;
    if (a.rgb_kind == CSPN_VISUAL_RGB_F32) vec = vec && aligned16(a.rgb) && a.rgb_fs % 4 == 0 && a.rgb_cs % 4 == 0;
    if (a.rgb_kind == CSPN_VISUAL_RGB_U8) vec = vec && (reinterpret_cast<uintptr_t>(a.rgb) & 3) == 0 && a.rgb_fs % 4 == 0 && a.rgb_cs % 4 == 0;
    a.vec = vec ? 1 : 0;
    if (!visual_chunks(who, a.range_elems, &a.n_chunks)) return 0;
    a.work = static_cast<float*>(work);
    if (!(a.use_min && a.use_max)) {
        if (!work || (reinterpret_cast<uintptr_t>(work) & 7)) return fail("%s: work %p (8-byte aligned, cspn_visual_workspace_bytes)", who, work);
        hipLaunchKernelGGL(cspn_visual_range_kernel, dim3(a.n_chunks, a.n_range, B), dim3(VIS_THREADS), 0, st, a);
        HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(cspn_visual_colour_kernel, dim3((unsigned)blocks, B), dim3(VIS_THREADS), 0, st, a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // namespace

extern "C" {

int cspn_visual_abi_version(void) { return CSPN_VISUAL_ABI_VERSION; }

size_t cspn_visual_workspace_bytes(int B, int n_planes, size_t elements) {
    int chunks = 0;
    if (B < 1 || n_planes < 1) {
        fail("cspn_visual_workspace_bytes: B %d, n_planes %d", B, n_planes);
        return 0;
    }
    if (!visual_chunks("cspn_visual_workspace_bytes", elements, &chunks)) return 0;
    return (size_t)B * n_planes * chunks * 2 * sizeof(float);
}

int cspn_visual_rows(const cspn_visual_rows_t* panels, int B, int H, int W, void* out, size_t out_frame_stride, void* work,
                     cspn_stream_t stream) {
    const char* who = "cspn_visual_rows";
    if (!panels) return fail("%s: panels is NULL", who);
    if (panels->n_depth < 1 || panels->n_depth > CSPN_VISUAL_MAX_PLANES) return fail("%s: n_depth %d (1 .. %d)", who, panels->n_depth, CSPN_VISUAL_MAX_PLANES);
    if (H < 1 || W < 1) return fail("%s: H %d, W %d", who, H, W);
    VisArgs a = {};
    a.rgb = panels->rgb_kind != CSPN_VISUAL_RGB_NONE ? panels->rgb : nullptr;
    a.rgb_kind = panels->rgb_kind;
    a.rgb_scale = panels->rgb_scale;
    a.rgb_fs = panels->rgb_frame_stride;
    a.rgb_cs = panels->rgb_channel_stride;
    for (int k = 0; k < panels->n_depth; ++k) {
        a.src[k] = static_cast<const float*>(panels->depth[k]);
        a.src_fs[k] = panels->depth_frame_stride[k];
    }
    a.n_range = a.n_colour = panels->n_depth;
    a.range_elems = (size_t)H * W;
    a.use_min = panels->use_min != 0;
    a.use_max = panels->use_max != 0;
    a.d_min = panels->d_min;
    a.d_max = panels->d_max;
    a.H = H;
    a.W = W;
    a.out = static_cast<unsigned char*>(out);
    a.out_fs = out_frame_stride;
    return visual_launch(who, a, B, work, static_cast<hipStream_t>(stream));
}

int cspn_visual_features(const void* features, long frame_stride, int B, int C, int H, int W, int n, void* out,
                         size_t out_frame_stride, void* work, cspn_stream_t stream) {
    const char* who = "cspn_visual_features";
    if (H < 1 || W < 1 || C < 1) return fail("%s: C %d, H %d, W %d", who, C, H, W);
    if (n < 1 || n > C) return fail("%s: n %d of %d planes", who, n, C);
    VisArgs a = {};
    a.rgb_kind = CSPN_VISUAL_RGB_NONE;
    a.src[0] = static_cast<const float*>(features);
    a.src_fs[0] = frame_stride;
    a.panel_stride = (long)H * W;
    a.feature = 1;
    a.n_range = 1;
    a.n_colour = n;
    a.range_elems = (size_t)C * H * W;
    a.H = H;
    a.W = W;
    a.out = static_cast<unsigned char*>(out);
    a.out_fs = out_frame_stride;
    return visual_launch(who, a, B, work, static_cast<hipStream_t>(stream));
}

}  // extern "C"

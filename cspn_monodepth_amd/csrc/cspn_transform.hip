// cspn_transform.hip — the reference's NYU train / val transforms (dataloaders/nyu_dataloader/nyu_dataloader.py:13-44 with
// transforms.py and ColorJitter(0.4, 0.4, 0.4)) for a batch of raw frames on the device (include/cspn_transform.h): a tables pass,
// a gather pass and, for train, a finish pass; no atomics, no wait between workgroups, nothing read back.
//
// The geometry is nearest-neighbour, so an output pixel is a copy of one raw pixel.  Which one is decided in fp64 with every
// operation rounded on its own: hipcc contracts a * b + c into one fused rounding by default, which moves a coordinate across a .5
// boundary where scipy's separate multiply and add do not.  So this translation unit switches contraction off for its own code
// (`#pragma clang fp contract(off)` below) and spells every such operation through mul_rn / add_rn / div_rn, which are compiled under
// that pragma — the toolkit's __dmul_rn / __dadd_rn are a plain `x * y` / `x + y` compiled with contraction ON and fuse once inlined.
// The resize tables are Pillow's running sums, built serially by one thread each.
//
// Addresses.  Parameters are device data and may hold anything: every table entry is clamped to its source range when it is written,
// a rotated coordinate is turned into an index only after it passed 0 <= c <= n - 1 (a NaN fails that), and the second sizes are
// clamped to [1, CSPN_TRANSFORM_MAX_SECOND].  Every pixel index is checked against oh * ow before its load and its store.
#include "cspn_common.hpp"
#include "cspn_philox.hpp"
#include "cspn_transform.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }

constexpr int TF_THREADS = CSPN_TRANSFORM_GATHER_PIXELS;        // 4 wavefronts; also the size of the uint8 -> float table
constexpr int TF_DRAW_THREADS = 64;
constexpr int TF_TABLE_WAVES = 3;           // the tables pass: one wavefront per serial job, lane 0 of each works

// what the tables pass leaves for a frame of a train call
struct FrameGeo {
    double m00, m01, m10, m11, off0, off1;
    float sf, fb, fc, fs;           // (float)s and the three factors as C floats
    int order;                      // 0..5, or -1: no jitter
    int pad;
};

// where the pieces of `work` start (bytes; every piece 8-byte aligned)
struct Layout {
    size_t geo, tab1r, tab1c, tab2r, tab2c, partial, staged, total;
    int G;                          // workgroups of the gather pass per frame = partial sums of L per frame
};

inline size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

inline Layout layout_of(int mode, int B, int h1, int w1, int oh, int ow) {
    Layout l;
    const size_t n = (size_t)oh * ow;
    const bool train = mode == CSPN_TRANSFORM_TRAIN;
    l.G = (int)((n + TF_THREADS - 1) / TF_THREADS);
    size_t at = 0;
    l.geo = at;     at += train ? up8((size_t)B * sizeof(FrameGeo)) : 0;
    l.tab1r = at;   at += up8((size_t)h1 * sizeof(int));
    l.tab1c = at;   at += up8((size_t)w1 * sizeof(int));
    l.tab2r = at;   at += train ? up8((size_t)B * oh * sizeof(int)) : 0;
    l.tab2c = at;   at += train ? up8((size_t)B * ow * sizeof(int)) : 0;
    l.partial = at; at += train ? up8((size_t)B * l.G * sizeof(unsigned)) : 0;
    l.staged = at;  at += train ? up8((size_t)B * n * sizeof(unsigned)) : 0;
    l.total = at;
    return l;
}

struct TransformArgs {
    const unsigned char* rgb;
    const float* depth;
    const double* params;
    float* rgb_out;
    float* depth_out;
    FrameGeo* geo;
    int *tab1r, *tab1c, *tab2r, *tab2c;
    unsigned *partial, *staged;
    long rgb_bs, rgb_cs, depth_bs;
    int B, H, W, h1, w1, oh, ow, i0, j0, G;     // i0, j0: the crop offsets of a val call
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Pillow's nearest resize n_in -> n_out: entries [first, first + count) of the running-sum table into dst (mirrored: back to front),
// each clamped to [0, n_in - 1].  The sum starts from index 0 whatever the window is.
__device__ void resize_table(int n_in, int n_out, int first, int count, bool mirrored, int* __restrict__ dst) {
    const double a = div_rn((double)n_in, (double)n_out);
    double o = mul_rn(a, 0.5);
    for (int i = 0; i < first + count; ++i) {
        if (i >= first) {
            const int k = i - first;
            dst[mirrored ? count - 1 - k : k] = o < (double)n_in ? clampi((int)o, 0, n_in - 1) : n_in - 1;
        }
        o = add_rn(o, a);
    }
}

// (int)(n * s) clamped to [1, CSPN_TRANSFORM_MAX_SECOND]; a NaN gives 1
__device__ __forceinline__ int second_size(int n, double s) {
    const double v = mul_rn((double)n, s);
    return v >= 1.0 ? (v <= (double)CSPN_TRANSFORM_MAX_SECOND ? (int)v : CSPN_TRANSFORM_MAX_SECOND) : 1;
}

// int(round((n - o) / 2.)) with ties to even, clamped so that the window [i0, i0 + o) starts inside [0, MAX_SECOND]
__device__ __forceinline__ int crop_offset(int n, int o) {
    const int i0 = (int)rint((double)(n - o) * 0.5);
    return clampi(i0, 0, CSPN_TRANSFORM_MAX_SECOND);
}

// grid B + 1 (train) or 1 (val).  Workgroup b < B: the second tables, M, off and the factors of frame b; the last workgroup: the
// first tables.  One thread per table: a table is a serial sum.  The jobs of a workgroup sit in different WAVEFRONTS (lane 0 of
// each): as lanes of one wavefront their loops would run one after the other.
__global__ __launch_bounds__(TF_TABLE_WAVES * 64) void cspn_transform_tables_kernel(TransformArgs a, int train) {
    if (threadIdx.x & 63) return;
    const int b = blockIdx.x, t = threadIdx.x >> 6;
    if (!train || b == a.B) {
        if (t == 0) resize_table(a.H, a.h1, 0, a.h1, false, a.tab1r);
        if (t == 1) resize_table(a.W, a.w1, 0, a.w1, false, a.tab1c);
        return;
    }
    const double* p = a.params + (size_t)b * CSPN_TRANSFORM_PARAMS;
    const double s = p[0];
    if (t == 0) {
        const int h2 = second_size(a.h1, s);
        resize_table(a.h1, h2, crop_offset(h2, a.oh), a.oh, false, a.tab2r + (size_t)b * a.oh);
    } else if (t == 1) {
        const int w2 = second_size(a.w1, s);
        resize_table(a.w1, w2, crop_offset(w2, a.ow), a.ow, p[2] != 0.0, a.tab2c + (size_t)b * a.ow);
    } else if (t == 2) {
        FrameGeo g;
        const double th = mul_rn(p[1], 3.14159265358979323846 / 180.0);           // numpy's deg2rad
        const double c = cos(th), sn = sin(th);
        const double c0 = add_rn(mul_rn((double)a.h1, 0.5), -0.5), c1 = add_rn(mul_rn((double)a.w1, 0.5), -0.5);
        g.m00 = c; g.m01 = sn; g.m10 = -sn; g.m11 = c;
        g.off0 = add_rn(c0, -add_rn(mul_rn(c, c0), mul_rn(sn, c1)));
        g.off1 = add_rn(c1, -add_rn(mul_rn(-sn, c0), mul_rn(c, c1)));
        g.sf = (float)s; g.fb = (float)p[3]; g.fc = (float)p[4]; g.fs = (float)p[5];
        const double code = p[6];
        g.order = (code >= 0.0 && code <= 5.0) ? (int)code : -1;
        g.pad = 0;
        a.geo[b] = g;
    }
}

// ---------------------------------------------------------------------------------------------- colour jitter
struct Pixel { int r, g, b; };

__device__ __forceinline__ int luma(const Pixel& v) { return (v.r * 19595 + v.g * 38470 + v.b * 7471 + 0x8000) >> 16; }

// Pillow's blend(degenerate, img, f): two fp32 roundings.  For 0 <= f <= 1 Pillow stores (uint8)t unclipped; t lies in [0, 255]
// there, where the clipped form below gives the same byte.  A NaN gives 0.
__device__ __forceinline__ int blend1(int deg, int img, float f) {
    const float t = add_rn((float)deg, mul_rn(f, (float)(img - deg)));
    return t > 0.f ? (t >= 255.f ? 255 : (int)t) : 0;
}
__device__ __forceinline__ Pixel brightness(const Pixel& v, float f) { return {blend1(0, v.r, f), blend1(0, v.g, f), blend1(0, v.b, f)}; }
__device__ __forceinline__ Pixel saturation(const Pixel& v, float f) {
    const int l = luma(v);
    return {blend1(l, v.r, f), blend1(l, v.g, f), blend1(l, v.b, f)};
}
__device__ __forceinline__ Pixel contrast(const Pixel& v, int mean, float f) { return {blend1(mean, v.r, f), blend1(mean, v.g, f), blend1(mean, v.b, f)}; }

// order code -> (brightness, contrast, saturation) in lexicographic permutations: 0 bcs, 1 bsc, 2 cbs, 3 csb, 4 sbc, 5 scb
__device__ __forceinline__ Pixel ops_before_contrast(Pixel v, const FrameGeo& g) {
    switch (g.order) {
        case 0: return brightness(v, g.fb);
        case 1: return saturation(brightness(v, g.fb), g.fs);
        case 4: return brightness(saturation(v, g.fs), g.fb);
        case 5: return saturation(v, g.fs);
        default: return v;
    }
}
__device__ __forceinline__ Pixel ops_after_contrast(Pixel v, const FrameGeo& g) {
    switch (g.order) {
        case 0: return saturation(v, g.fs);
        case 2: return saturation(brightness(v, g.fb), g.fs);
        case 3: return brightness(saturation(v, g.fs), g.fb);
        case 5: return brightness(v, g.fb);
        default: return v;
    }
}

// the sum of v over the workgroup, in every thread; a fixed tree over integers
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int half = TF_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ void store_rgb(const TransformArgs& a, int b, size_t pix, const Pixel& v, const float* lut) {
    float* o = a.rgb_out + (ptrdiff_t)b * a.rgb_bs + pix;
    o[0] = lut[v.r];
    o[a.rgb_cs] = lut[v.g];
    o[2 * a.rgb_cs] = lut[v.b];
}

// grid (G, B): one thread per output pixel of frame blockIdx.y
template <bool TRAIN>
__global__ __launch_bounds__(TF_THREADS) void cspn_transform_gather_kernel(TransformArgs a) {
    __shared__ float lut[TF_THREADS];
    __shared__ unsigned long long red[TRAIN ? TF_THREADS : 1];
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);             // nyu_dataloader.py:29 + ToTensor's .float()
    __syncthreads();
    const int b = blockIdx.y;
    const size_t n = (size_t)a.oh * a.ow, HW = (size_t)a.H * a.W;
    const size_t pix = (size_t)blockIdx.x * TF_THREADS + threadIdx.x;
    const bool active = pix < n;
    const int y = active ? (int)(pix / a.ow) : 0, x = active ? (int)(pix % a.ow) : 0;
    bool valid = active;
    int r0 = 0, c0 = 0;
    FrameGeo g;
    if constexpr (TRAIN) {
        g = a.geo[b];
        const double Y = (double)a.tab2r[(size_t)b * a.oh + y], X = (double)a.tab2c[(size_t)b * a.ow + x];
        double cy = add_rn(g.off0, mul_rn(Y, g.m00));
        cy = add_rn(cy, mul_rn(X, g.m01));
        double cx = add_rn(g.off1, mul_rn(Y, g.m10));
        cx = add_rn(cx, mul_rn(X, g.m11));
        valid = active && cy >= 0.0 && cy <= (double)(a.h1 - 1) && cx >= 0.0 && cx <= (double)(a.w1 - 1);      // a NaN is not valid
        if (valid) {
            r0 = a.tab1r[clampi((int)floor(add_rn(cy, 0.5)), 0, a.h1 - 1)];
            c0 = a.tab1c[clampi((int)floor(add_rn(cx, 0.5)), 0, a.w1 - 1)];
        }
    } else {
        r0 = a.tab1r[clampi(a.i0 + y, 0, a.h1 - 1)];
        c0 = a.tab1c[clampi(a.j0 + x, 0, a.w1 - 1)];
    }
    Pixel v = {0, 0, 0};
    float d = 0.f;
    if (valid) {
        const size_t src = (size_t)r0 * a.W + c0;                       // r0 <= H - 1, c0 <= W - 1: the tables are clamped
        const unsigned char* f = a.rgb + (size_t)b * 3 * HW + src;
        v.r = f[0]; v.g = f[HW]; v.b = f[2 * HW];
        d = a.depth[(size_t)b * HW + src];
        // depth / s before the gather (fp32 / fp32), then scipy's order-0 sum `t = 0; t += v`: a -0 leaves as +0
        if constexpr (TRAIN) d = add_rn(0.f, div_rn(d, g.sf));
    }
    if (active) a.depth_out[(ptrdiff_t)b * a.depth_bs + pix] = d;
    if constexpr (!TRAIN) {
        if (active) store_rgb(a, b, pix, v, lut);
    } else {
        if (g.order < 0) {                                              // uniform over the workgroup: g is the frame's
            if (active) store_rgb(a, b, pix, v, lut);
            return;
        }
        v = ops_before_contrast(v, g);
        const unsigned long long sum = block_sum(active ? (unsigned long long)luma(v) : 0ull, red);
        if (threadIdx.x == 0) a.partial[(size_t)b * a.G + blockIdx.x] = (unsigned)sum;             // <= 256 * 255
        if (active) a.staged[(size_t)b * n + pix] = (unsigned)v.r | ((unsigned)v.g << 8) | ((unsigned)v.b << 16);
    }
}

// grid (G, B): contrast and what follows it for the frames with jitter
__global__ __launch_bounds__(TF_THREADS) void cspn_transform_finish_kernel(TransformArgs a) {
    __shared__ float lut[TF_THREADS];
    __shared__ unsigned long long red[TF_THREADS];
    const int b = blockIdx.y;
    const FrameGeo g = a.geo[b];
    if (g.order < 0) return;                                            // the gather pass wrote this frame
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
    unsigned long long part = 0;
    for (int i = threadIdx.x; i < a.G; i += TF_THREADS) part += a.partial[(size_t)b * a.G + i];
    const size_t n = (size_t)a.oh * a.ow;
    const unsigned long long sum = block_sum(part, red);                // also orders the lut writes before the reads below
    // ImageStat's mean in fp64 (sums below 2^53 are exact), + 0.5, truncated
    const int mean = clampi((int)add_rn(div_rn((double)sum, (double)n), 0.5), 0, 255);
    const size_t pix = (size_t)blockIdx.x * TF_THREADS + threadIdx.x;
    if (pix >= n) return;
    const unsigned w = a.staged[(size_t)b * n + pix];
    Pixel v = {(int)(w & 255u), (int)((w >> 8) & 255u), (int)((w >> 16) & 255u)};
    v = ops_after_contrast(contrast(v, mean, g.fc), g);
    store_rgb(a, b, pix, v, lut);
}

// one thread per frame
__global__ __launch_bounds__(TF_DRAW_THREADS) void cspn_transform_draw_kernel(const long long* __restrict__ frame_ids, int B, unsigned long long seed,
                                                                               double* __restrict__ params) {
    const int b = blockIdx.x * TF_DRAW_THREADS + threadIdx.x;
    if (b >= B) return;
    const unsigned long long fid = (unsigned long long)frame_ids[b];
    const unsigned lo = (unsigned)fid, hi = (unsigned)(fid >> 32), k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    double u[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) u[k] = philox_uniform<1u>((unsigned)k, lo, hi, k0, k1);
    double* p = params + (size_t)b * CSPN_TRANSFORM_PARAMS;
    p[0] = add_rn(1.0, mul_rn(0.5, u[0]));
    p[1] = add_rn(-5.0, mul_rn(10.0, u[1]));
    p[2] = u[2] < 0.5 ? 1.0 : 0.0;
#pragma unroll
    for (int k = 3; k < 6; ++k) p[k] = add_rn(0.6, mul_rn(0.8, u[k]));
    p[6] = floor(mul_rn(6.0, u[6]));
    p[7] = 0.0;
}

inline bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// the sizes after the first resize, or false
inline bool first_size(int H, int W, double first, int* h1, int* w1) {
    if (H < 1 || W < 1 || !(first > 0.0)) return false;
    const double ph = (double)H * first, pw = (double)W * first;                // the fp64 products, truncated
    if (!(ph >= 1.0 && ph <= 2147483647.0 && pw >= 1.0 && pw <= 2147483647.0)) return false;
    *h1 = (int)ph;
    *w1 = (int)pw;
    return true;
}

// every rule cspn_transform and cspn_transform_workspace_bytes share; nullptr: fine
inline const char* bad_geometry(int mode, int B, int H, int W, double first, int oh, int ow, int* h1, int* w1) {
    if (mode != CSPN_TRANSFORM_VAL && mode != CSPN_TRANSFORM_TRAIN) return "unknown mode";
    if (B < 1 || B > 65535 || H < 1 || W < 1 || oh < 1 || ow < 1) return "bad size (1 <= B <= 65535, H, W, oh, ow >= 1)";
    if ((size_t)H * (size_t)W >= ((size_t)1 << 31) || (size_t)oh * (size_t)ow >= ((size_t)1 << 31)) return "H * W and oh * ow must be below 2^31";
    if (!first_size(H, W, first, h1, w1)) return "the first factor must give a size of at least 1 x 1";
    if (mode == CSPN_TRANSFORM_VAL && (oh > *h1 || ow > *w1)) return "the output is larger than the resized frame";
    return nullptr;
}

inline int host_crop_offset(int n, int o) {                  // Python's round((n - o) / 2.), n >= o
    const int d = n - o, k = d / 2;
    return (d & 1) ? k + (k & 1) : k;                        // k + 0.5 goes to the even neighbour
}

}  // namespace

extern "C" {

int cspn_transform_abi_version(void) { return CSPN_TRANSFORM_ABI_VERSION; }

int cspn_transform_first_size(int H, int W, double first, int* h1, int* w1) {
    int a = 0, b = 0;
    if (!first_size(H, W, first, &a, &b)) return 0;
    if (h1) *h1 = a;
    if (w1) *w1 = b;
    return 1;
}

size_t cspn_transform_workspace_bytes(int mode, int B, int H, int W, double first, int oh, int ow) {
    int h1 = 0, w1 = 0;
    if (bad_geometry(mode, B, H, W, first, oh, ow, &h1, &w1)) return 0;
    return layout_of(mode, B, h1, w1, oh, ow).total;
}

int cspn_transform(const unsigned char* rgb, const float* depth, int B, int H, int W, double first, int oh, int ow, int mode,
                   const double* params, float* rgb_out, long rgb_out_batch_stride, long rgb_out_channel_stride,
                   float* depth_out, long depth_out_batch_stride, void* work, cspn_stream_t stream) {
    const char* who = "cspn_transform";
    if (!rgb || !depth) return fail("%s: null rgb / depth", who);
    int h1 = 0, w1 = 0;
    if (const char* why = bad_geometry(mode, B, H, W, first, oh, ow, &h1, &w1))
        return fail("%s: %s (B=%d H=%d W=%d first=%g oh=%d ow=%d mode=%d)", who, why, B, H, W, first, oh, ow, mode);
    const bool train = mode == CSPN_TRANSFORM_TRAIN;
    if (train && !params) return fail("%s: CSPN_TRANSFORM_TRAIN needs params", who);
    if (train && misaligned(params, 7)) return fail("%s: params must be 8-byte aligned", who);
    if (misaligned(depth, 3)) return fail("%s: depth is not aligned to its element size", who);
    if (!rgb_out || !depth_out) return fail("%s: null rgb_out / depth_out", who);
    if (misaligned(rgb_out, 3) || misaligned(depth_out, 3)) return fail("%s: rgb_out / depth_out are not aligned to their element size", who);
    const size_t n = (size_t)oh * ow;
    if (rgb_out_channel_stride < 0 || (size_t)rgb_out_channel_stride < n) return fail("%s: rgb_out_channel_stride below oh * ow", who);
    if (B > 1 && (rgb_out_batch_stride < 0 || (size_t)rgb_out_batch_stride < n)) return fail("%s: rgb_out_batch_stride below oh * ow", who);
    if (B > 1 && (depth_out_batch_stride < 0 || (size_t)depth_out_batch_stride < n)) return fail("%s: depth_out_batch_stride below oh * ow", who);
    if (!work) return fail("%s: null work", who);
    if (misaligned(work, 7)) return fail("%s: work must be 8-byte aligned", who);

    const Layout l = layout_of(mode, B, h1, w1, oh, ow);
    char* w = static_cast<char*>(work);
    TransformArgs a;
    a.rgb = rgb; a.depth = depth; a.params = params; a.rgb_out = rgb_out; a.depth_out = depth_out;
    a.geo = reinterpret_cast<FrameGeo*>(w + l.geo);
    a.tab1r = reinterpret_cast<int*>(w + l.tab1r); a.tab1c = reinterpret_cast<int*>(w + l.tab1c);
    a.tab2r = reinterpret_cast<int*>(w + l.tab2r); a.tab2c = reinterpret_cast<int*>(w + l.tab2c);
    a.partial = reinterpret_cast<unsigned*>(w + l.partial); a.staged = reinterpret_cast<unsigned*>(w + l.staged);
    a.rgb_bs = rgb_out_batch_stride; a.rgb_cs = rgb_out_channel_stride; a.depth_bs = depth_out_batch_stride;
    a.B = B; a.H = H; a.W = W; a.h1 = h1; a.w1 = w1; a.oh = oh; a.ow = ow; a.G = l.G;
    a.i0 = train ? 0 : host_crop_offset(h1, oh);
    a.j0 = train ? 0 : host_crop_offset(w1, ow);

    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cspn_transform_tables_kernel, dim3(train ? B + 1 : 1), dim3(TF_TABLE_WAVES * 64), 0, st, a, train ? 1 : 0);
    HIP_OK(hipGetLastError());
    const dim3 grid((unsigned)l.G, (unsigned)B);
    if (train) {
        hipLaunchKernelGGL(cspn_transform_gather_kernel<true>, grid, dim3(TF_THREADS), 0, st, a);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(cspn_transform_finish_kernel, grid, dim3(TF_THREADS), 0, st, a);
    } else {
        hipLaunchKernelGGL(cspn_transform_gather_kernel<false>, grid, dim3(TF_THREADS), 0, st, a);
    }
    HIP_OK(hipGetLastError());
    return 1;
}

int cspn_transform_draw_params(const long long* frame_ids, int B, unsigned long long seed, double* params, cspn_stream_t stream) {
    const char* who = "cspn_transform_draw_params";
    if (!frame_ids || !params) return fail("%s: null frame_ids / params", who);
    if (B < 1 || B > 65535) return fail("%s: bad size B=%d (1 <= B <= 65535)", who, B);
    if (misaligned(frame_ids, 7) || misaligned(params, 7)) return fail("%s: frame_ids and params must be 8-byte aligned", who);
    hipLaunchKernelGGL(cspn_transform_draw_kernel, dim3((B + TF_DRAW_THREADS - 1) / TF_DRAW_THREADS), dim3(TF_DRAW_THREADS), 0,
                       static_cast<hipStream_t>(stream), frame_ids, B, seed, params);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

// cspn_max8.hip — the original CSPN release's propagation (network/libs/post_process/CSPN.py: AffinityPropagate and
// AffinityPropagate_prediction), forward and backward, fp32 (include/cspn_max8.h).
//
//   S_k = box(g_k),  o_k = box(g_k d) / S_k,  e = max_k o_k (NaN-propagating),  d' = (1 - m) e + m s
//
// The gates weight the SOURCE pixel, so a step cannot gather a per-destination tap volume: the owner of a pixel forms the
// eight products g_k d and the box sum runs over products.  Forward layout ("column per lane"): a workgroup of 8 wavefronts
// owns a 64 x 48 region, lane l of wavefront w the 6 rows [6w, 6w + 6) of column l.  A thread keeps its pixels' 8 gates and
// 8 reciprocals of S_k — and the gates of the row above and below its segment — in registers for all steps of the launch.
// Horizontal neighbours come by DPP wave shifts (lanes 0 / 63 read 0: the region's edge), vertical ones are the thread's own
// registers; per step only the two rows at a segment's ends cross wavefronts, as two floats per lane through LDS, double
// buffered so that one barrier per step is enough.  The region carries a halo of S pixels that loses one ring per step;
// regions start every 64 - 2 S (48 - 2 S) pixels from the image's corner, so the first and last region of a row spend no halo
// outside.  Budget (hipcc 6 rows per lane): 210-228 VGPRs, no scratch, 8 KB LDS, two wavefronts per SIMD; 7 rows spill 2
// registers, 8 rows 8-50.
//
// Determinism: every box sum is (left + centre) + right, then (upper + middle) + lower, with +0 for pixels outside the image;
// contraction is off for the whole file, so no launch shape changes which products are fused.
#include "cspn_common.hpp"
#include "cspn_max8.h"

#pragma clang fp contract(off)

namespace {

constexpr int M8_R = 6;                       // rows per lane
constexpr int M8_WAVES = 8;
constexpr int M8_THREADS = 64 * M8_WAVES;     // 512: two wavefronts per SIMD, up to 256 VGPRs each
constexpr int M8_REGION = 64;                 // region width = the 64 lanes
constexpr int M8_REGION_H = M8_WAVES * M8_R;  // region height
static_assert(M8_REGION_H > 2 * CSPN_MAX8_MAX_STEPS_PER_LAUNCH, "a region must keep rows of its own under the largest halo");
constexpr int M8_DEFAULT_STEPS = 8;           // steps_per_launch = 0: the sweep's fastest at 24 x 228 x 304 (profiles/r08_max8_bench.json)
constexpr int M8_PLANES_FWD = 2, M8_PLANES_BWD = 26;     // work: ping-pong | 1/S [8], gbar [8], Sbar [8], c ping-pong

constexpr int BW_TW = 32, BW_TH = 8, BW_THREADS = BW_TW * BW_TH;      // tile of the reverse step
constexpr int BW_RW = BW_TW + 2, BW_RH = BW_TH + 2, BW_REGION = BW_RW * BW_RH;

struct Max8Fwd {
    const float* g;
    long gbs, gcs;
    const float* d_in;            // the first launch: blur (blended with the sparse plane on load); later: a work plane
    const float* sparse;
    float* d_out;
    float* hist;
    unsigned char* mask;
    int B, H, W;
    int halo, nsteps, t0, first;  // t0: steps done by earlier launches
    int tiles_x, tiles_y;
};

__device__ __forceinline__ float nanf32() { return __int_as_float(0x7fc00000); }

template <bool SPARSE, bool HIST>
__global__ __launch_bounds__(M8_THREADS) void max8_forward_kernel(const Max8Fwd a) {
    __shared__ float edge[2][2][M8_WAVES][64];            // [step parity][first / last row of a segment][wavefront][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tpi = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tpi, tt = blockIdx.x - b * tpi;
    const int ty = tt / a.tiles_x, tx = tt - ty * a.tiles_x;
    const int H = a.H, W = a.W;
    const int rx0 = tx * (M8_REGION - 2 * a.halo), ry0 = ty * (M8_REGION_H - 2 * a.halo);
    const int x = rx0 + lane, y0 = ry0 + wave * M8_R;
    // the pixels this region owns at the end of the launch: its interior, and its rim where the rim is the image's
    const int vx0 = rx0 + (tx > 0 ? a.halo : 0), vx1 = rx0 + M8_REGION >= W ? W : rx0 + M8_REGION - a.halo;
    const int vy0 = ry0 + (ty > 0 ? a.halo : 0), vy1 = ry0 + M8_REGION_H >= H ? H : ry0 + M8_REGION_H - a.halo;
    const bool xin = x < W, xown = x >= vx0 && x < vx1;
    const size_t HW = (size_t)H * W;
    const float* gb = a.g + (size_t)b * a.gbs + x;
    const size_t img = (size_t)b * HW + x;

    float g[M8_R + 2][8], r[M8_R][8], d[M8_R + 2], s[M8_R], m[M8_R];
    bool in[M8_R], own[M8_R];
#pragma unroll
    for (int j = 0; j < M8_R + 2; ++j) {
        const int y = y0 + j - 1;
        const bool ok = xin && y >= 0 && y < H;
#pragma unroll
        for (int k = 0; k < 8; ++k) g[j][k] = ok ? fabsf(gb[(size_t)k * a.gcs + (size_t)y * W]) : 0.f;
    }
    d[0] = d[M8_R + 1] = 0.f;
#pragma unroll
    for (int i = 0; i < M8_R; ++i) {
        const int y = y0 + i;
        in[i] = xin && y < H;
        own[i] = xown && y >= vy0 && y < vy1;
        float v = in[i] ? a.d_in[img + (size_t)y * W] : 0.f;
        if (SPARSE) {
            s[i] = in[i] ? a.sparse[img + (size_t)y * W] : 0.f;
            m[i] = sgnf(s[i]);
            if (a.first) {
                const float keep = (1.f - m[i]) * v, put = m[i] * s[i];
                v = in[i] ? keep + put : 0.f;
            }
        }
        d[i + 1] = v;
    }
    // 1 / S_k of the thread's pixels
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float h[M8_R + 2];
#pragma unroll
        for (int j = 0; j < M8_R + 2; ++j) h[j] = (dpp_from_prev_lane(g[j][k]) + g[j][k]) + dpp_from_next_lane(g[j][k]);
#pragma unroll
        for (int i = 0; i < M8_R; ++i) r[i][k] = 1.0f / ((h[i] + h[i + 1]) + h[i + 2]);
    }

    for (int n = 0; n < a.nsteps; ++n) {
        const int par = n & 1;
        edge[par][0][wave][lane] = d[1];
        edge[par][1][wave][lane] = d[M8_R];
        __syncthreads();
        d[0] = wave > 0 ? edge[par][1][wave - 1][lane] : 0.f;
        d[M8_R + 1] = wave < M8_WAVES - 1 ? edge[par][0][wave + 1][lane] : 0.f;

        float e[M8_R];
        unsigned mk[M8_R];
        bool bad[M8_R];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float h[M8_R + 2];
#pragma unroll
            for (int j = 0; j < M8_R + 2; ++j) {
                const float p = g[j][k] * d[j];
                h[j] = (dpp_from_prev_lane(p) + p) + dpp_from_next_lane(p);
            }
#pragma unroll
            for (int i = 0; i < M8_R; ++i) {
                const float o = ((h[i] + h[i + 1]) + h[i + 2]) * r[i][k];
                if (k == 0) {
                    e[i] = o;
                    bad[i] = o != o;
                    if (HIST) mk[i] = 1u;
                } else {
                    if (HIST) {
                        const bool gt = o > e[i], eq = o == e[i];
                        mk[i] = gt ? (1u << k) : (eq ? (mk[i] | (1u << k)) : mk[i]);
                    }
                    bad[i] = bad[i] || o != o;
                    e[i] = fmaxf(e[i], o);              // skips a NaN: `bad` carries it
                }
            }
        }
        unsigned char* mp = HIST ? a.mask + ((size_t)(a.t0 + n) * a.B) * HW + img : nullptr;
        float* hp = HIST ? a.hist + ((size_t)(a.t0 + n) * a.B) * HW + img : nullptr;
#pragma unroll
        for (int i = 0; i < M8_R; ++i) {
            float v = bad[i] ? nanf32() : e[i];
            if (SPARSE) {
                const float keep = (1.f - m[i]) * v, put = m[i] * s[i];
                v = keep + put;
            }
            d[i + 1] = in[i] ? v : 0.f;                 // a pixel outside the image stays +0: its products are g = 0 times this
            if (HIST && own[i]) {
                const size_t o = (size_t)(y0 + i) * W;
                hp[o] = v;
                mp[o] = (unsigned char)(bad[i] ? 0u : mk[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < M8_R; ++i)
        if (own[i]) a.d_out[img + (size_t)(y0 + i) * W] = d[i + 1];
}

// ------------------------------------------------------------------------------------------------ backward
struct Max8Bwd {
    const float* g;
    long gbs, gcs;
    int C;
    const float* blur;
    const float* sparse;
    const float* hist;
    const unsigned char* mask;
    const float* c_in;
    float* c_out;
    float* rs;                    // [B][8][HW] 1 / S_k
    float* gbar;                  // [B][8][HW]
    float* sbar;                  // [B][8][HW]
    float* grad_g;
    float* grad_blur;
    int B, H, W, T, t;
};

__device__ __forceinline__ float gate_at(const float* gk, int y, int x, int H, int W) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? fabsf(gk[(size_t)y * W + x]) : 0.f;
}
__device__ __forceinline__ float plane_at(const float* pl, int y, int x, int H, int W) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? pl[(size_t)y * W + x] : 0.f;
}

// 1 / S_k in the forward's order of operations, and zeros in both accumulators.  One thread per pixel.
__global__ __launch_bounds__(256) void max8_backward_prepare_kernel(const Max8Bwd a) {
    const size_t HW = (size_t)a.H * a.W, n = (size_t)a.B * HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int b = (int)(i / HW);
        const size_t p = i - (size_t)b * HW;
        const int y = (int)(p / a.W), x = (int)(p - (size_t)y * a.W);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float* gk = a.g + (size_t)b * a.gbs + (size_t)k * a.gcs;
            float h[3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
                h[dy] = (gate_at(gk, y + dy - 1, x - 1, a.H, a.W) + gate_at(gk, y + dy - 1, x, a.H, a.W)) + gate_at(gk, y + dy - 1, x + 1, a.H, a.W);
            const size_t o = ((size_t)b * 8 + k) * HW + p;
            a.rs[o] = 1.0f / ((h[0] + h[1]) + h[2]);
            a.gbar[o] = 0.f;
            a.sbar[o] = 0.f;
        }
    }
}

// the share of gate k in the gradient of max(max(max(o0,o1),max(o2,o3)),max(max(o4,o5),max(o6,o7))) when the gates of `mk`
// attain the maximum: every node whose two operands both attain it halves the gradient (torch.max on equal operands)
__device__ __forceinline__ float tree_weight(unsigned mk, int k) {
    const unsigned half = (mk >> (k & 4)) & 15u, other_half = (mk >> ((k & 4) ^ 4)) & 15u;
    const unsigned quarter = (half >> (k & 2)) & 3u, other_quarter = (half >> ((k & 2) ^ 2)) & 3u;
    float w = other_half ? 0.5f : 1.f;
    if (other_quarter) w *= 0.5f;
    if (quarter == 3u) w *= 0.5f;
    return w;
}

// One step t of the reverse sweep on a 32 x 8 tile: a_k of the tile and a one-pixel rim into LDS, then every pixel gathers the
// eight 3 x 3 sums.  A pixel with one winner (the generic case) reads one reciprocal and writes one non-zero.
template <bool SPARSE>
__global__ __launch_bounds__(BW_THREADS) void max8_backward_step_kernel(const Max8Bwd a) {
    __shared__ float4 alo[BW_REGION], ahi[BW_REGION];
    const int b = blockIdx.z, H = a.H, W = a.W;
    const int x0 = blockIdx.x * BW_TW, y0 = blockIdx.y * BW_TH;
    const size_t HW = (size_t)H * W, img = (size_t)b * HW;
    const size_t step_img = ((size_t)(a.t - 1) * a.B + b) * HW;
    for (int i = threadIdx.x; i < BW_REGION; i += BW_THREADS) {
        const int ry = i / BW_RW, rx = i - ry * BW_RW;
        const int y = y0 + ry - 1, x = x0 + rx - 1;
        float av[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) av[k] = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t p = (size_t)y * W + x;
            const unsigned mk = a.mask[step_img + p];
            if (mk) {
                const float c = a.c_in[img + p];
                const float sv = SPARSE ? a.sparse[img + p] : 0.f;
                const float mm = SPARSE ? sgnf(sv) : 0.f;
                const float u = SPARSE ? (1.f - mm) * c : c;
                const bool mine = rx >= 1 && rx <= BW_TW && ry >= 1 && ry <= BW_TH;
                float e = 0.f;
                if (mine) {
                    e = a.hist[step_img + p];                       // d_t = (1 - m) e_t + m s: m = -1 gives e_t = (d_t + s) / 2
                    if (SPARSE && mm < 0.f) e = (e + sv) * 0.5f;
                }
                if ((mk & (mk - 1u)) == 0u) {
                    const int kw = __builtin_ctz(mk);
                    const size_t o = ((size_t)b * 8 + kw) * HW + p;
                    const float v = u * a.rs[o];
#pragma unroll
                    for (int k = 0; k < 8; ++k) av[k] = k == kw ? v : 0.f;
                    if (mine) a.sbar[o] -= v * e;
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (mk & (1u << k)) {
                            const size_t o = ((size_t)b * 8 + k) * HW + p;
                            av[k] = (tree_weight(mk, k) * u) * a.rs[o];
                            if (mine) a.sbar[o] -= av[k] * e;
                        }
                    }
                }
            }
        }
        alo[i] = make_float4(av[0], av[1], av[2], av[3]);
        ahi[i] = make_float4(av[4], av[5], av[6], av[7]);
    }
    __syncthreads();
    const int lx = threadIdx.x & (BW_TW - 1), ly = threadIdx.x / BW_TW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    float bx[8];
    {
        float4 hl[3], hh[3];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int o = (ly + dy) * BW_RW + lx;
            const float4 l0 = alo[o], l1 = alo[o + 1], l2 = alo[o + 2];
            const float4 h0 = ahi[o], h1 = ahi[o + 1], h2 = ahi[o + 2];
            hl[dy] = make_float4((l0.x + l1.x) + l2.x, (l0.y + l1.y) + l2.y, (l0.z + l1.z) + l2.z, (l0.w + l1.w) + l2.w);
            hh[dy] = make_float4((h0.x + h1.x) + h2.x, (h0.y + h1.y) + h2.y, (h0.z + h1.z) + h2.z, (h0.w + h1.w) + h2.w);
        }
        bx[0] = (hl[0].x + hl[1].x) + hl[2].x; bx[1] = (hl[0].y + hl[1].y) + hl[2].y;
        bx[2] = (hl[0].z + hl[1].z) + hl[2].z; bx[3] = (hl[0].w + hl[1].w) + hl[2].w;
        bx[4] = (hh[0].x + hh[1].x) + hh[2].x; bx[5] = (hh[0].y + hh[1].y) + hh[2].y;
        bx[6] = (hh[0].z + hh[1].z) + hh[2].z; bx[7] = (hh[0].w + hh[1].w) + hh[2].w;
    }
    const size_t p = (size_t)y * W + x;
    float dprev;
    if (a.t > 1) {
        dprev = a.hist[((size_t)(a.t - 2) * a.B + b) * HW + p];
    } else {
        dprev = a.blur[img + p];
        if (SPARSE) {
            const float sv = a.sparse[img + p], mm = sgnf(sv);
            const float keep = (1.f - mm) * dprev, put = mm * sv;
            dprev = keep + put;
        }
    }
    float cprev = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float gk = fabsf(a.g[(size_t)b * a.gbs + (size_t)k * a.gcs + p]);
        cprev += gk * bx[k];
        const size_t o = ((size_t)b * 8 + k) * HW + p;
        a.gbar[o] += dprev * bx[k];
    }
    a.c_out[img + p] = cprev;
}

// grad_guidance = (gbar_k + box(Sbar_k)) sign(G_k), zeros for the channels past 7; grad_blur = (1 - m) c_0.  c_0 is a.c_in.
template <bool SPARSE>
__global__ __launch_bounds__(256) void max8_backward_final_kernel(const Max8Bwd a) {
    const size_t HW = (size_t)a.H * a.W, n = (size_t)a.B * HW;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int b = (int)(i / HW);
        const size_t p = i - (size_t)b * HW;
        const int y = (int)(p / a.W), x = (int)(p - (size_t)y * a.W);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float* sb = a.sbar + ((size_t)b * 8 + k) * HW;
            float h[3];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
                h[dy] = (plane_at(sb, y + dy - 1, x - 1, a.H, a.W) + plane_at(sb, y + dy - 1, x, a.H, a.W)) + plane_at(sb, y + dy - 1, x + 1, a.H, a.W);
            const float gg = a.gbar[((size_t)b * 8 + k) * HW + p] + ((h[0] + h[1]) + h[2]);
            a.grad_g[((size_t)b * a.C + k) * HW + p] = gg * sgnf(a.g[(size_t)b * a.gbs + (size_t)k * a.gcs + p]);
        }
        for (int k = 8; k < a.C; ++k) a.grad_g[((size_t)b * a.C + k) * HW + p] = 0.f;
        const float c0 = a.c_in[i];
        a.grad_blur[i] = SPARSE ? (1.f - sgnf(a.sparse[i])) * c0 : c0;
    }
}

int check_shape(const char* who, int B, int H, int W, int T) {
    if (B < 1 || H < 1 || W < 1) return fail("%s: B, H, W must be at least 1, got %d x %d x %d", who, B, H, W);
    if (T < 1) return fail("%s: T must be at least 1, got %d", who, T);
    if ((size_t)H * W > 0x7fffffffu) return fail("%s: H * W = %zu does not fit an int", who, (size_t)H * W);
    return 1;
}
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline int region_count(int extent, int edge, int halo) { return extent <= edge ? 1 : ceil_div(extent - edge, edge - 2 * halo) + 1; }

}  // namespace

extern "C" {

int cspn_max8_abi_version(void) { return CSPN_MAX8_ABI_VERSION; }

size_t cspn_max8_workspace_bytes(int B, int H, int W, int T, int keep_history) {
    if (B < 1 || H < 1 || W < 1 || T < 1) return 0;
    const size_t plane = ((size_t)B * H * W * sizeof(float) + 255) & ~(size_t)255;
    return plane * (keep_history ? M8_PLANES_BWD : M8_PLANES_FWD);
}

int cspn_max8_forward(const void* guidance, long batch_stride, long channel_stride, const void* d0, const void* sparse_or_null,
                      void* out, void* history_or_null, void* mask_or_null, void* work, int B, int H, int W, int T,
                      int steps_per_launch, cspn_stream_t stream) {
    const char* who = "cspn_max8_forward";
    if (!check_shape(who, B, H, W, T)) return 0;
    if (!guidance || !d0 || !out || !work) return fail("%s: null guidance / d0 / out / work", who);
    if ((history_or_null == nullptr) != (mask_or_null == nullptr)) return fail("%s: history and mask go together: both or neither", who);
    if (steps_per_launch < 0 || steps_per_launch > CSPN_MAX8_MAX_STEPS_PER_LAUNCH)
        return fail("%s: steps_per_launch must be 0 (built-in) or 1..%d, got %d", who, CSPN_MAX8_MAX_STEPS_PER_LAUNCH, steps_per_launch);
    if (batch_stride < 0 || channel_stride < 0) return fail("%s: negative guidance stride", who);
    if (!aligned4(guidance) || !aligned4(d0) || !aligned4(sparse_or_null) || !aligned4(out) || !aligned4(history_or_null))
        return fail("%s: a plane is not aligned to its element size", who);
    if (!aligned16(work)) return fail("%s: work must be 16-byte aligned", who);
    if (out == d0 || out == sparse_or_null) return fail("%s: out must not alias an input", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int S = steps_per_launch ? steps_per_launch : M8_DEFAULT_STEPS;
    if (S > T) S = T;
    const size_t plane = cspn_max8_workspace_bytes(B, H, W, T, 0) / M8_PLANES_FWD;
    float* pp[2] = {static_cast<float*>(work), reinterpret_cast<float*>(static_cast<char*>(work) + plane)};
    Max8Fwd a;
    a.g = static_cast<const float*>(guidance);
    a.gbs = batch_stride;
    a.gcs = channel_stride;
    a.sparse = static_cast<const float*>(sparse_or_null);
    a.hist = static_cast<float*>(history_or_null);
    a.mask = static_cast<unsigned char*>(mask_or_null);
    a.B = B; a.H = H; a.W = W;
    a.halo = S;
    a.tiles_x = region_count(W, M8_REGION, S);
    a.tiles_y = region_count(H, M8_REGION_H, S);
    const size_t grid = (size_t)B * a.tiles_x * a.tiles_y;
    if (grid > 0x7fffffffu) return fail("%s: %zu regions are more than one launch takes", who, grid);
    int done = 0, j = 0;
    while (done < T) {
        const int n = T - done < S ? T - done : S;
        a.first = done == 0;
        a.d_in = done == 0 ? static_cast<const float*>(d0) : pp[(j - 1) & 1];
        a.d_out = done + n == T ? static_cast<float*>(out) : pp[j & 1];
        a.nsteps = n;
        a.t0 = done;
        const dim3 gr((unsigned)grid), bl(M8_THREADS);
        if (a.sparse && a.hist) hipLaunchKernelGGL((max8_forward_kernel<true, true>), gr, bl, 0, st, a);
        else if (a.sparse) hipLaunchKernelGGL((max8_forward_kernel<true, false>), gr, bl, 0, st, a);
        else if (a.hist) hipLaunchKernelGGL((max8_forward_kernel<false, true>), gr, bl, 0, st, a);
        else hipLaunchKernelGGL((max8_forward_kernel<false, false>), gr, bl, 0, st, a);
        HIP_OK(hipGetLastError());
        done += n;
        ++j;
    }
    return 1;
}

int cspn_max8_backward(const void* guidance, long batch_stride, long channel_stride, int C, const void* blur,
                       const void* sparse_or_null, const void* history, const void* mask, const void* grad_out,
                       void* grad_guidance, void* grad_blur, void* work, int B, int H, int W, int T, cspn_stream_t stream) {
    const char* who = "cspn_max8_backward";
    if (!check_shape(who, B, H, W, T)) return 0;
    if (C < 8) return fail("%s: guidance needs at least 8 channels, got %d", who, C);
    if (B > 65535) return fail("%s: B = %d is more than one launch takes", who, B);
    if (ceil_div(H, BW_TH) > 65535) return fail("%s: H = %d is more than one launch takes", who, H);
    if (!guidance || !blur || !history || !mask || !grad_out || !grad_guidance || !grad_blur || !work)
        return fail("%s: null guidance / blur / history / mask / grad_out / grad_guidance / grad_blur / work", who);
    if (batch_stride < 0 || channel_stride < 0) return fail("%s: negative guidance stride", who);
    if (!aligned4(guidance) || !aligned4(blur) || !aligned4(sparse_or_null) || !aligned4(history) || !aligned4(grad_out) ||
        !aligned4(grad_guidance) || !aligned4(grad_blur))
        return fail("%s: a plane is not aligned to its element size", who);
    if (!aligned16(work)) return fail("%s: work must be 16-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t plane = cspn_max8_workspace_bytes(B, H, W, T, 1) / M8_PLANES_BWD;
    char* w = static_cast<char*>(work);
    Max8Bwd a;
    a.g = static_cast<const float*>(guidance);
    a.gbs = batch_stride;
    a.gcs = channel_stride;
    a.C = C;
    a.blur = static_cast<const float*>(blur);
    a.sparse = static_cast<const float*>(sparse_or_null);
    a.hist = static_cast<const float*>(history);
    a.mask = static_cast<const unsigned char*>(mask);
    a.rs = reinterpret_cast<float*>(w + 2 * plane);
    a.gbar = reinterpret_cast<float*>(w + 10 * plane);
    a.sbar = reinterpret_cast<float*>(w + 18 * plane);
    float* cp[2] = {reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plane)};
    a.grad_g = static_cast<float*>(grad_guidance);
    a.grad_blur = static_cast<float*>(grad_blur);
    a.B = B; a.H = H; a.W = W; a.T = T; a.t = 0;
    a.c_in = nullptr;
    a.c_out = nullptr;
    const int flat = grid_for((size_t)B * H * W, 256);
    hipLaunchKernelGGL(max8_backward_prepare_kernel, dim3(flat), dim3(256), 0, st, a);
    HIP_OK(hipGetLastError());
    const dim3 gr(ceil_div(W, BW_TW), ceil_div(H, BW_TH), B), bl(BW_THREADS);
    for (int i = 0; i < T; ++i) {
        a.t = T - i;
        a.c_in = i == 0 ? static_cast<const float*>(grad_out) : cp[(i - 1) & 1];
        a.c_out = cp[i & 1];
        if (a.sparse) hipLaunchKernelGGL((max8_backward_step_kernel<true>), gr, bl, 0, st, a);
        else hipLaunchKernelGGL((max8_backward_step_kernel<false>), gr, bl, 0, st, a);
        HIP_OK(hipGetLastError());
    }
    a.c_in = cp[(T - 1) & 1];
    if (a.sparse) hipLaunchKernelGGL((max8_backward_final_kernel<true>), dim3(flat), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((max8_backward_final_kernel<false>), dim3(flat), dim3(256), 0, st, a);
    HIP_OK(hipGetLastError());
    return 1;
}

}  // extern "C"

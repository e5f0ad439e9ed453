// cspn_repair.hip — the guard behind a weight-resident launch (include/cspn_hip.h: cspn_resident_plan.guard).
//
// A resident launch whose workgroups could not all become co-resident in time (the GPU shared with a tenant that holds CUs for
// seconds) gives up: its abort word receives the call's sequence number and the tiles that gave up leave the poison NaN.  The host
// repairs that where the package is the next consumer (functional.py: journal) — but the reference module is plain ATen
// (network/libs/post_process/CSPN_new.py:80-92): whatever consumes its output ON THE GPU sees the finished tensor.  A guard kernel
// restores that property from the stream: launched behind the resident launch(es) of a call, every workgroup reads the abort word and
// returns at once when it is not this call's sequence number (the success path: one empty launch, priced in DESIGN.md §4.1b);
// otherwise the whole batch is re-computed here — slowly, but with the guarded kernel's arithmetic, operation for operation, so the
// repaired result is bit-identical to a clean call's.
//
// Re-computation (guard_tiles): a workgroup takes a 32 x 32 output tile and the T * (K / 2) pixel halo its T steps depend on (two
// planes of (32 + 2 halo)^2 floats in LDS: halo <= 54), and advances the region step by step; the taps of a pixel are rebuilt from
// the guidance at every step (no register residency, no exchange between workgroups — nothing here can wait for anybody).  The four
// kernels differ in what a pixel starts as, what it becomes at a step and what is stored; the weight derives they share with the
// guarded kernels are functions of cspn_common.hpp (softmax_in_channel_order, abs_gates8, div8_shared_reciprocal) and
// cspnk_helpers.hpp (softmax_to_pairs: the dot-product form, shared with cspnk_d2.hip).
#include "cspn_common.hpp"
#include "cspnk_helpers.hpp"

#include <array>
#include <utility>

namespace {

constexpr int REP_TILE = 32, REP_THREADS = 256;

// what every guard kernel's arguments begin with (tiles_x / tiles_y: guard_launch)
struct GuardGeom {
    const unsigned* abort_word; unsigned seq;
    int B, H, W, T, tiles_x, tiles_y;
};
// the call finished: nothing to do
__device__ __forceinline__ bool guard_idle(const GuardGeom& t) {
    return __hip_atomic_load(t.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != t.seq;
}

// The region of one tile: region pixel (ry, rx) is pixel (y(ry), x(rx)) of image b; the tile itself is the REP_TILE^2 pixels behind
// the halo.
struct Region {
    int b, ty, tx, ry0, rx0, R, HALO, H, W;
    __device__ int y(int ry) const { return ry0 + ry; }
    __device__ int x(int rx) const { return rx0 + rx; }
    __device__ bool own(int ry, int rx) const { return ry >= HALO && ry < HALO + REP_TILE && rx >= HALO && rx < HALO + REP_TILE; }
    __device__ bool image(int y, int x) const { return y >= 0 && y < H && x >= 0 && x < W; }
};

// The tile loop of every guard kernel: the tiles of the batch over the workgroups, a tile's region staged into `cur` (the second
// plane zeroed: its border is never computed and must read as 0), T steps of which step s advances the pixels whose stencil
// inputs are still exact — the window shrinks by RK = K / 2 per step — and at the end the tile's own pixels.
//   start(region, ry, rx)            -> what a region pixel starts as
//   step(region, s, ry, rx, centre)  -> what it becomes at step s; centre points at its state in `cur` (row stride region.R)
//   finish(region, y, x, v)          <- the final state v of the tile pixel at image position (y, x), which may lie past the image
// Everything a form stores on the way (history planes, published taps, padding columns) is its callables' own business.
template <int RK, typename Start, typename Step, typename Finish>
__device__ __forceinline__ void guard_tiles(const GuardGeom& t, float* lds, Start start, Step step, Finish finish) {
    const int HALO = t.T * RK, R = REP_TILE + 2 * HALO;
    float* cur = lds;
    float* nxt = lds + (size_t)R * R;
    const int tiles = t.tiles_x * t.tiles_y;
    for (int k = blockIdx.x; k < t.B * tiles; k += gridDim.x) {
        const int b = k / tiles, tr = k - b * tiles, ty = tr / t.tiles_x, tx = tr - ty * t.tiles_x;
        const Region r{b, ty, tx, ty * REP_TILE - HALO, tx * REP_TILE - HALO, R, HALO, t.H, t.W};
        __syncthreads();                                                   // (the previous tile's readers are done)
        for (int i = threadIdx.x; i < R * R; i += REP_THREADS) {
            const int ry = i / R, rx = i - ry * R;
            cur[i] = start(r, ry, rx);
            nxt[i] = 0.f;
        }
        __syncthreads();
        for (int s = 1; s <= t.T; ++s) {
            // after step s the pixels within (T - s) * RK of the tile are exact: only those are advanced
            const int lo = s * RK, n = R - 2 * lo;
            for (int i = threadIdx.x; i < n * n; i += REP_THREADS) {
                const int ry = lo + i / n, rx = lo + i % n;
                nxt[ry * R + rx] = step(r, s, ry, rx, cur + ry * R + rx);
            }
            __syncthreads();
            float* tmp = cur; cur = nxt; nxt = tmp;
        }
        for (int i = threadIdx.x; i < REP_TILE * REP_TILE; i += REP_THREADS) {
            const int ly = i / REP_TILE, lx = i - ly * REP_TILE;
            finish(r, ty * REP_TILE + ly, tx * REP_TILE + lx, cur[(HALO + ly) * R + HALO + lx]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the 3 x 3 forms (cspn3_resident)
struct RepArgs {
    GuardGeom t;
    const float* g; long g_bs, g_cs;
    const float* d0; const float* sparse; float* out;
    float* hist; float* s_out; float* w_out; const float* s_in;
    const float* target; double* macc; int nslots;      // MODE 1: the fused depth metrics of the pixels the failed launch did not score
    int Wv;
};

// The arithmetic of cspn3_resident, operation for operation: |g| gathered with the reference's shifts and S summed in channel order
// (abs_gates8), div8_shared_reciprocal, the blend folded into the taps, the eight FMAs in tap order from 0, + m * d0.
// MODE 0: inference (refined depth -> out).  MODE 1: inference with the depth metrics fused — the launch that gave up has scored the
// tiles that finished and poisoned the others, so the re-computation adds the metric terms of exactly the pixels it finds poisoned
// (summation order differs from the fused epilogue's: the sums agree to ~1e-7, the refined depth to the bit).  MODE 2: the training forward — every step's state goes to its history plane, the
// normaliser S (and, when asked for, the taps) is published.  MODE 4: the volume-free reverse sweep G_t = stencil^T((1-m) G_{t+1}) on
// the taps |g_j[p]| / S[p + off_j]; d0 is G_T, the history receives G_{T-1} .. G_0, (1-m) G travels.  MODE 3: the same sweep on taps
// gathered from a forward tap volume (a.g = [B,8,H,W]): tap j = w_{7-j}[p + off_j].
// PAC = 1 (MODE 0 / 2): the K = 3 softmax form of CSPN_ours.py:35-41 — tap j = softmax over the 8 guidance channels at the pixel
// itself (softmax_in_channel_order<float>, as cspn3_resident's PAC instances and cspn_pac_prepare_kernel); MODE 2 publishes the taps
// (no S).
template <int BLEND, int MODE, int PAC>
__global__ __launch_bounds__(REP_THREADS) void cspn3_resident_repair(const RepArgs a) {
    if (guard_idle(a.t)) return;
    constexpr bool TRANSG = MODE == 4, TRANS = MODE == 3 || MODE == 4, HIST = MODE >= 2, SCORE = MODE == 1;
    float mf[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) mf[k] = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.t.H, W = a.t.W, Wv = a.Wv;
    const size_t HW = (size_t)H * W, plane = (size_t)a.t.B * HW;
    // a pixel the launch computes (rows [0, H), columns [0, Wv)), and a row-padding column inside the last valid quad: the resident
    // launch stores (and, giving up, poisons) that quad as a whole, with zeros in its padding columns
    auto valid = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < Wv; };
    auto padding = [&](int y, int x) { return y >= 0 && y < H && x >= Wv && x < W && (x & ~3) < Wv; };
    guard_tiles<1>(a.t, lds,
        [&](const Region& r, int ry, int rx) -> float {
            const int y = r.y(ry), x = r.x(rx);
            if (!valid(y, x)) return 0.f;
            const size_t p = r.b * HW + (size_t)y * W + x;
            float v = a.d0[p];
            if (TRANS && BLEND) v *= 1.f - sgnf(a.sparse[p]);      // the sweep starts from (1-m) G_T
            return v;
        },
        [&](const Region& r, int s, int ry, int rx, const float* c) -> float {
            const int b = r.b, y = r.y(ry), x = r.x(rx);
            const bool mine = r.own(ry, rx);
            const size_t p = b * HW + (size_t)y * W + x;      // (an index only where (y, x) is valid or padding)
            const float* __restrict__ gb = a.g + (size_t)b * a.g_bs;
            float* const hp = HIST ? a.hist + (size_t)(s - 1) * plane : nullptr;
            float keep = 0.f;
            if (valid(y, x)) {
                float qv[8];
                float m = 0.f;
                if (BLEND) m = sgnf(a.sparse[p]);
                if (TRANSG) {
                    // tap j = |channel j at p| x 1 / S[p + off_j] (the forward's refined reciprocal), 0 where p + off_j is outside
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int yy = y + tap_dy<3>(j), xx = x + tap_dx<3>(j);
                        const float rs = valid(yy, xx) ? reciprocal_as_forward(a.s_in[b * HW + (size_t)yy * W + xx]) : 0.f;
                        qv[j] = fabsf(gb[(size_t)j * a.g_cs + (size_t)y * W + x]) * rs;
                    }
                } else if (TRANS) {
                    // tap j = w_{7-j}[p + off_j] from the forward's tap volume, 0 outside the image
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int yy = y + tap_dy<3>(j), xx = x + tap_dx<3>(j);
                        qv[j] = r.image(yy, xx) ? gb[(size_t)(7 - j) * a.g_cs + (size_t)yy * W + xx] : 0.f;
                    }
                } else if (PAC) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) qv[j] = gb[(size_t)j * a.g_cs + (size_t)y * W + x];
                    softmax_in_channel_order<float>(qv);
                } else {
                    // (rows: [0, H); columns: [0, W) — the row padding [Wv, W) holds the caller's zeros)
                    float av[8];
                    const float S = abs_gates8(gb, a.g_cs, y, x, H, W, av);
                    div8_shared_reciprocal(av, S, qv);
                    if (MODE == 2 && mine && s == 1) a.s_out[p] = S;
                }
                if (!TRANS) {
                    if (MODE == 2 && mine && s == 1 && (PAC || a.w_out)) {      // published before the blend is folded in
#pragma unroll
                        for (int j = 0; j < 8; ++j) a.w_out[((size_t)b * 8 + j) * HW + (size_t)y * W + x] = qv[j];
                    }
                    if (BLEND) {
                        const float om = 1.f - m;                          // 0, 1 or 2: exact
#pragma unroll
                        for (int j = 0; j < 8; ++j) qv[j] *= om;
                    }
                }
                float u = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) u = fmaf(qv[j], c[tap_dy<3>(j) * r.R + tap_dx<3>(j)], u);
                if (TRANS) {
                    keep = BLEND ? __fmul_rn(1.f - m, u) : u;              // (1-m) G travels, G itself goes to the history
                } else {
                    // + m * d0: a product rounded on its own, then an addition (the resident kernel keeps m * d0 in LDS) — never one FMA
                    if (BLEND) u = __fadd_rn(u, __fmul_rn(m, a.d0[p]));
                    keep = u;
                }
                if (HIST && mine) hp[p] = u;
            } else if (MODE == 2 && !PAC && s == 1 && mine && padding(y, x)) {
                // the resident launch stores the padding columns' S (and zero taps) with their quad
                float av[8];
                a.s_out[p] = abs_gates8(gb, a.g_cs, y, x, H, W, av);
                if (a.w_out) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) a.w_out[((size_t)b * 8 + j) * HW + (size_t)y * W + x] = 0.f;
                }
            }
            // ... and zeros in the history: a C-API reader of the repaired plane must find them again
            if (HIST && mine && padding(y, x)) hp[p] = 0.f;
            return keep;
        },
        [&](const Region& r, int y, int x, float v) {
            if constexpr (!HIST) {
                const size_t p = r.b * HW + (size_t)y * W + x;
                if (y < H && x < Wv) {
                    if (SCORE && __float_as_uint(a.out[p]) == CSPN_POISON_F32) metric_terms(v, a.target[p], mf);
                    a.out[p] = v;
                } else if (padding(y, x)) {
                    a.out[p] = 0.f;      // zeros, as the clean launch stores them
                }
            }
        });
    if (SCORE) {
        __syncthreads();
        float* part = lds;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const float v = wave_sum_to_lane63(mf[k]);
            if (lane == 63) part[wave * 10 + k] = v;
        }
        __syncthreads();
        if (threadIdx.x < 10) {
            double v = 0.0;
            for (int w = 0; w < REP_THREADS / 64; ++w) v += (double)part[w * 10 + threadIdx.x];
            if (v != 0.0) atomicAdd(a.macc + (size_t)(blockIdx.x % a.nslots) * 10 + threadIdx.x, v);
        }
    }
}


// ------------------------------------------------------------------------------------------------ K x K softmax forms (CSPN_ours)
// The guard of cspnk_forward_resident's unscored inference calls: the arithmetic of the FMA kernel cspnk_resident (kxk_fma_pixel),
// the state rounded to the plane dtype where that kernel rounds it: after every `round_every` steps (its phase length) and at the
// end.  For the FMA step form the re-computed depth is therefore the multi-launch schedule's bits, whatever its phase length.
// The dot-product form (cspnk_d2: state rounded after EVERY step, two taps per v_dot2_f32_f16) is re-computed with its own arithmetic
// (d2_pixel).  Which of the two is re-computed is the launch site's explicit step_form argument, never inferred from round_every: an FMA
// launch of phase length 1 (T = 1) rounds after every step as well, and must still get the FMA arithmetic.
struct KRepArgs {
    GuardGeom t;
    const void* g; const void* x0; const void* sparse; void* out;
    int round_every;
};
template <typename T> __device__ __forceinline__ float ldf(const void* p, size_t i);
template <> __device__ __forceinline__ float ldf<float>(const void* p, size_t i) { return static_cast<const float*>(p)[i]; }
template <> __device__ __forceinline__ float ldf<__half>(const void* p, size_t i) { return __half2float(static_cast<const __half*>(p)[i]); }
template <typename T> __device__ __forceinline__ float round_to(float v);
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_to<__half>(float v) { return __half2float(__float2half_rn(v)); }
__device__ __forceinline__ void stf(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void stf(__half* p, size_t i, float v) { p[i] = __float2half_rn(v); }

// a region pixel of a [B,H,W] plane of type ST, 0 outside the image: what the K x K forward forms start from
template <typename ST>
__device__ __forceinline__ float plane_pixel(const Region& r, const void* plane, int ry, int rx) {
    const int y = r.y(ry), x = r.x(rx);
    return r.image(y, x) ? ldf<ST>(plane, ((size_t)r.b * r.H + y) * r.W + x) : 0.f;
}

// One pixel of one K x K FMA step, as cspnk_resident (and cspn_pac_prepare + cspn_propagate) compute it: the softmax over the K*K-1
// channels at the pixel itself (softmax_in_channel_order<GT>: for fp16 guidance ONE rounding to half), (1-m) folded into the taps
// (1-m in {0, 1, 2}: exact in either tap dtype), one FMA per tap in row-major tap order from 0, + m * x0 as a product, then a sum;
// `publish` sees the taps before the fold, `round_now` rounds the state to the plane dtype.  p: the pixel's index in its image,
// gbase / pbase: the image's first element in the guidance / in a plane; centre: the pixel's state (row stride R).
template <int K, typename GT, typename ST, int BLEND, typename Publish>
__device__ __forceinline__ float kxk_fma_pixel(const void* g, const void* x0, const void* sparse, size_t gbase, size_t pbase, size_t p, size_t HW,
                                               const float* centre, int R, bool round_now, Publish publish) {
    constexpr int NT = K * K - 1;
    float w[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) w[c] = ldf<GT>(g, gbase + (size_t)c * HW + p);
    softmax_in_channel_order<GT>(w);
    publish(w);
    float m = 0.f;
    if (BLEND) {
        m = sgnf(ldf<ST>(sparse, pbase + p));
#pragma unroll
        for (int c = 0; c < NT; ++c) w[c] = round_to<GT>(w[c] * (1.f - m));
    }
    float u = 0.f;
#pragma unroll
    for (int c = 0; c < NT; ++c) u = fmaf(w[c], centre[tap_dy<K>(c) * R + tap_dx<K>(c)], u);
    if (BLEND) u = __fadd_rn(u, __fmul_rn(m, ldf<ST>(x0, pbase + p)));
    // (opaque: left to the compiler, the last FMA and the conversion fuse into ONE v_fma_mixlo_f16 — a single rounding of
    // the exact sum where cspnk_resident rounds twice, fp32 then half: 2e-4 of the pixels differed by a half ulp)
    asm volatile("" : "+v"(u));
    return round_now ? round_to<ST>(u) : u;
}

// One pixel of one step of the DOT-PRODUCT form (cspnk_d2.hip: K = 5, fp16 guidance, fp16 planes) with that kernel's own arithmetic —
// the softmax as softmax_to_pairs forms it (max folded into the exponent's scale, v_exp_f32, sum in channel order, refined
// reciprocal, numerator x 1 / sum rounded by v_cvt_pk_f16_f32), the taps as tap PAIRS, a window row as dot2(pair dx -2 -1), dot2(pair dx 0 +1)
// [centre row: dx +1 +2], then the single dx +2 tap as v_fma_mix_f32, rows top to bottom, + m x0 as the sum's start value, one v_cvt_pk_f16_f32
// per step — so that a timed-out call of config 3's shape returns the BITS of a clean one.
template <int BLEND>
__device__ __forceinline__ float d2_pixel(const KRepArgs& a, size_t gbase, size_t pbase, size_t p, size_t HW, const float* centre, int R) {
    unsigned gw[24], tp[12];
    unsigned mx2 = 0xfc00fc00u;
#pragma unroll
    for (int c = 0; c < 24; ++c) {
        gw[c] = (unsigned)__half_as_ushort(static_cast<const __half*>(a.g)[gbase + (size_t)c * HW + p]);
        mx2 = pk_max_f16(mx2, gw[c] | 0xfc000000u);           // (the high half stays -inf)
    }
    constexpr float L2E = 1.44269502162933349609375f;
    softmax_to_pairs<0>(gw, -h2f_lo(mx2) * L2E, tp);
    float acc = 0.f;
    if (BLEND) {
        const float m = sgnf(ldf<__half>(a.sparse, pbase + p));
        acc = m * ldf<__half>(a.x0, pbase + p);
        const unsigned om = pack_h2(1.f - m, 1.f - m);
#pragma unroll
        for (int t = 0; t < 12; ++t) tp[t] = pk_mul_f16(tp[t], om);
    }
    asm volatile("" : "+v"(tp[10]), "+v"(tp[11]));        // (as the step loop of cspnk_d2: see mix_hh)
#pragma unroll
    for (int rr = 0; rr < 5; ++rr) {
        const float* row = centre + (rr - 2) * R;
        const unsigned pm = pack_h2(row[-2], row[-1]);       // the state is half-rounded every step: packing is exact
        if (rr == 2) {
            acc = dot2(tp[4], pm, acc);
            acc = dot2(tp[5], pack_h2(row[1], row[2]), acc);
        } else {
            const int s0 = rr < 2 ? 2 * rr : 6 + 2 * (rr - 3);
            acc = dot2(tp[s0], pm, acc);
            acc = dot2(tp[s0 + 1], pack_h2(row[0], row[1]), acc);
            const unsigned ps = pack_h2(row[2], 0.f);
            if (rr == 0) acc = mix_hh<0, 0>(tp[10], ps, acc);
            if (rr == 1) acc = mix_hh<1, 0>(tp[10], ps, acc);
            if (rr == 3) acc = mix_hh<0, 0>(tp[11], ps, acc);
            if (rr == 4) acc = mix_hh<1, 0>(tp[11], ps, acc);
        }
    }
    return h2f_lo(cvt_pk_f16(acc, 0.f));
}

// D2 = 1: the dot-product form (K = 5, GT = ST = __half)
template <int K, typename GT, typename ST, int BLEND, int D2 = 0>
__global__ __launch_bounds__(REP_THREADS) void cspnk_resident_repair(const KRepArgs a) {
    if (guard_idle(a.t)) return;
    constexpr int NT = K * K - 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.t.H, W = a.t.W, T = a.t.T;
    const size_t HW = (size_t)H * W;
    guard_tiles<K / 2>(a.t, lds,
        [&](const Region& r, int ry, int rx) -> float { return plane_pixel<ST>(r, a.x0, ry, rx); },
        [&](const Region& r, int s, int ry, int rx, const float* c) -> float {
            const int y = r.y(ry), x = r.x(rx);
            if (!r.image(y, x)) return 0.f;
            const size_t gbase = (size_t)r.b * NT * HW, pbase = (size_t)r.b * HW, p = (size_t)y * W + x;
            if constexpr (D2 != 0) {
                return d2_pixel<BLEND>(a, gbase, pbase, p, HW, c, r.R);
            } else {
                const bool round_now = (s % a.round_every) == 0 || s == T;
                return kxk_fma_pixel<K, GT, ST, BLEND>(a.g, a.x0, a.sparse, gbase, pbase, p, HW, c, r.R, round_now, [](const float (&)[NT]) {});
            }
        },
        [&](const Region& r, int y, int x, float v) {
            if (y < H && x < W) stf(static_cast<ST*>(a.out) + (size_t)r.b * HW, (size_t)y * W + x, v);
        });
}


// ---- the K = 5 fp16 training forms (BASELINE config 3's shape) -----------------------------------------------------------------------
// Guard of cspnk_forward_resident_history's dot-product launch (cspnk_d2<HIST>): history [T,B,H,W] receives x_1 .. x_T, the state rounded
// to the plane dtype after EVERY step, wk_out the softmax taps BEFORE the blend is folded in, in the Taps<__half> layout — kxk_fma_pixel
// rounding every step, i.e. the arithmetic of cspn_pac_prepare + cspn_propagate (history) at one step per launch: what the multi-launch
// training path stores; the dot-product kernel's own bits are within the fp16 tolerance of it, and the backward differentiates whichever
// history and taps it is handed.
struct KHistRepArgs {
    GuardGeom t;
    const void* g; const void* x0; const void* sparse; void* hist; void* wk_out;
};

template <int K, typename GT, typename ST, int BLEND>
__global__ __launch_bounds__(REP_THREADS) void cspnk_history_repair(const KHistRepArgs a) {
    if (guard_idle(a.t)) return;
    constexpr int NT = K * K - 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int W = a.t.W;
    const size_t HW = (size_t)a.t.H * W, plane = (size_t)a.t.B * HW;
    guard_tiles<K / 2>(a.t, lds,
        [&](const Region& r, int ry, int rx) -> float { return plane_pixel<ST>(r, a.x0, ry, rx); },
        [&](const Region& r, int s, int ry, int rx, const float* c) -> float {
            const int y = r.y(ry), x = r.x(rx);
            if (!r.image(y, x)) return 0.f;
            const size_t gbase = (size_t)r.b * NT * HW, pbase = (size_t)r.b * HW, p = (size_t)y * W + x;
            const bool own = r.own(ry, rx);
            GT* const wkb = static_cast<GT*>(a.wk_out) + (size_t)r.b * Taps<GT>::image_elems(NT, HW);
            const float u = kxk_fma_pixel<K, GT, ST, BLEND>(a.g, a.x0, a.sparse, gbase, pbase, p, HW, c, r.R, true, [&](const float (&w)[NT]) {
                if (s == 1 && own) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) stf(wkb, Taps<GT>::idx(j, p, HW), w[j]);
                }
            });
            if (own) stf(static_cast<ST*>(a.hist) + (size_t)(s - 1) * plane + pbase, p, u);
            return u;
        },
        [](const Region&, int, int, float) {});
}

// Guard of cspnk_transposed_resident: G_t = stencil^T((1-m) G_{t+1}) with the transposed taps w_{NT-1-j}[p + off_j] read from the forward's
// tap volume (zero where p + off_j leaves the image), one FMA per tap in row-major tap order from 0, fp32 state; history [T,B,H,W] f32
// receives G_{T-1} .. G_0 (the UNMASKED G_t; what travels is (1-m) G_t), g32_out — when given — G_T as fp32.  The arithmetic of
// cspnk_resident<TRANS>, i.e. of cspn_transpose_weights + cspn_propagate (history, CSPN_BLEND_PREMASK), bit for bit.
struct KSweepRepArgs {
    GuardGeom t;
    const void* wk; const void* g_T; const void* sparse; float* g32_out; float* hist;
};

template <int K, typename WT, typename INT, int PREMASK>
__global__ __launch_bounds__(REP_THREADS) void cspnk_sweep_repair(const KSweepRepArgs a) {
    if (guard_idle(a.t)) return;
    constexpr int NT = K * K - 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int W = a.t.W;
    const size_t HW = (size_t)a.t.H * W, plane = (size_t)a.t.B * HW;
    guard_tiles<K / 2>(a.t, lds,
        [&](const Region& r, int ry, int rx) -> float {
            const int y = r.y(ry), x = r.x(rx);
            if (!r.image(y, x)) return 0.f;
            const size_t p = (size_t)r.b * HW + (size_t)y * W + x;
            float v = ldf<INT>(a.g_T, p);
            if (a.g32_out && r.own(ry, rx)) a.g32_out[p] = v;
            if (PREMASK) v = __fmul_rn(v, 1.f - sgnf(ldf<INT>(a.sparse, p)));
            return v;
        },
        [&](const Region& r, int s, int ry, int rx, const float* c) -> float {
            const int y = r.y(ry), x = r.x(rx);
            if (!r.image(y, x)) return 0.f;
            const size_t p = (size_t)r.b * HW + (size_t)y * W + x;
            const WT* const wkb = static_cast<const WT*>(a.wk) + (size_t)r.b * Taps<WT>::image_elems(NT, HW);
            float u = 0.f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int ys = y + tap_dy<K>(j), xs = x + tap_dx<K>(j);
                const float wt = r.image(ys, xs) ? ldf<WT>(wkb, Taps<WT>::idx(NT - 1 - j, (size_t)ys * W + xs, HW)) : 0.f;
                u = fmaf(wt, c[tap_dy<K>(j) * r.R + tap_dx<K>(j)], u);
            }
            if (r.own(ry, rx)) a.hist[(size_t)(s - 1) * plane + p] = u;
            if (PREMASK) u = __fmul_rn(1.f - sgnf(ldf<INT>(a.sparse, p)), u);
            return u;
        },
        [](const Region&, int, int, float) {});
}

}  // namespace

namespace cspn_detail {

// The guard's LDS: two fp32 planes of the region, R = tile + 2 halo pixels wide, within the 160 KB of a CU; 0 where there is no fit.
static size_t repair_lds_bytes(int K, int T) {
    const long R = REP_TILE + 2L * T * (K / 2);
    const size_t bytes = T >= 1 && R <= 1024 ? (size_t)2 * R * R * sizeof(float) : 0;      // (R bounded first: no overflow for any T)
    return bytes <= 160 * 1024 ? bytes : 0;
}
bool resident_repair_fits(int T) { return repair_lds_bytes(3, T) != 0; }
bool kres_repair_fits(int K, int T) { return (K == 3 || K == 5) && repair_lds_bytes(K, T) != 0; }

// A few workgroups that loop over the tiles: the success path — every launch of a healthy deployment — is `grid` workgroups
// that read one word and return, and its cost is their dispatch (rocprofv3, config 2's training step: 5.1 us with one workgroup
// per CU and 51 KB of LDS each; n_cu / 8 of them — 32 on an MI355X — keep the failure path at tens of milliseconds)
static int guard_grid(int n_tiles, int n_cu) {
    const int cap = n_cu >= 64 ? n_cu / 8 : 8;
    return n_tiles > cap ? cap : n_tiles;
}

static GuardGeom guard_geom(const unsigned* abort_word, unsigned seq, int B, int H, int W, int T) { return {abort_word, seq, B, H, W, T, 0, 0}; }

// the launch of a guard kernel for K x K stencils: the tiling, the grid and the LDS of a.t
template <int K, auto Kern, typename Args>
static int guard_launch(Args a, int n_cu, void* stream) {
    a.t.tiles_x = ceil_div(a.t.W, REP_TILE);
    a.t.tiles_y = ceil_div(a.t.H, REP_TILE);
    const int grid = guard_grid(a.t.B * a.t.tiles_x * a.t.tiles_y, n_cu);
    return launch_dynamic_lds<Kern>(grid, REP_THREADS, repair_lds_bytes(K, a.t.T), static_cast<hipStream_t>(stream), a);
}

// the guard's instance per (blend, form); null where it has none (resident_form_guarded)
using RepLaunchFn = int (*)(RepArgs, int, void*);
template <int BLEND, int F>
constexpr RepLaunchFn rep_instance() {
    constexpr ResidentForm f = static_cast<ResidentForm>(F);
    if constexpr (resident_form_guarded(f)) return &guard_launch<3, cspn3_resident_repair<BLEND, resident_form_mode(f), resident_form_pac(f)>, RepArgs>;
    else return nullptr;
}
template <int BLEND, int... F>
constexpr std::array<RepLaunchFn, sizeof...(F)> rep_instances(std::integer_sequence<int, F...>) { return {rep_instance<BLEND, F>()...}; }

int resident_repair_launch(const float* g, long bs, long cs, const float* d0, const float* sparse, float* out, float* hist, float* s_out,
                           float* w_out, const float* s_in, ResidentForm form, const unsigned* abort_word, unsigned seq, int B, int H, int W, int Wv,
                           int T, int blend, int n_cu, void* stream, const float* target, double* acc, int nslots) {
    constexpr auto forms = std::make_integer_sequence<int, (int)ResidentForm::Count>{};
    static constexpr std::array<RepLaunchFn, (size_t)ResidentForm::Count> instances[2] = {rep_instances<0>(forms), rep_instances<1>(forms)};
    if (!resident_repair_fits(T)) return fail("cspn3_forward_resident: the guard re-computes at most 54 steps (T=%d)", T);
    const RepLaunchFn launch = form < ResidentForm::Count ? instances[blend ? 1 : 0][(int)form] : nullptr;
    if (!launch) return fail("cspn3_forward_resident: the guard has no form for this launch");
    return launch(RepArgs{guard_geom(abort_word, seq, B, H, W, T), g, bs, cs, d0, sparse, out, hist, s_out, w_out, s_in, target, acc, nslots > 0 ? nslots : 1, Wv},
                  n_cu, stream);
}

template <int K, typename GT, typename ST, int D2 = 0>
static int kres_repair_launch_t(const KRepArgs& a, int blend, int n_cu, void* stream) {
    return blend ? guard_launch<K, cspnk_resident_repair<K, GT, ST, 1, D2>>(a, n_cu, stream)
                 : guard_launch<K, cspnk_resident_repair<K, GT, ST, 0, D2>>(a, n_cu, stream);
}

int kres_repair_launch(const void* g, int g_dtype, int K, const void* x0, const void* sparse, void* out, int state_dtype,
                       const unsigned* abort_word, unsigned seq, int B, int H, int W, int T, int round_every, int step_form, int blend, int n_cu,
                       void* stream) {
    if (!kres_repair_fits(K, T)) return fail("cspnk_forward_resident: the guard re-computes at most T * (K / 2) = 54 halo pixels (K=%d, T=%d)", K, T);
    if (step_form != CSPN_STEP_FMA && step_form != CSPN_STEP_DOT2) return fail("cspnk_forward_resident: the guard needs the launch's step form (%d)", step_form);
    const KRepArgs a{guard_geom(abort_word, seq, B, H, W, T), g, x0, sparse, out, round_every > 0 ? round_every : T};
    const bool gh = g_dtype == CSPN_F16, sh = state_dtype == CSPN_F16;
    if (!gh && sh) return fail("cspnk_forward_resident: fp32 guidance with fp16 planes has no kernel");
    if (step_form == CSPN_STEP_DOT2 && !(K == 5 && gh && sh)) return fail("cspnk_forward_resident: the dot-product form is K = 5 with fp16 guidance and planes");
    if (K == 3) {
        if (gh) return sh ? kres_repair_launch_t<3, __half, __half>(a, blend, n_cu, stream) : kres_repair_launch_t<3, __half, float>(a, blend, n_cu, stream);
        // (cspnk_forward_resident hands K = 3 with fp32 guidance to the quad kernel, whose guard is resident_repair_launch's softmax form)
        return fail("cspnk_forward_resident: K = 3 with fp32 guidance is guarded behind the quad kernel's launch");
    }
    // the dot-product form's launch (cspnk_d2.hip) is re-computed with ITS arithmetic; the FMA form's at phase length 1 (T = 1) is not
    if (step_form == CSPN_STEP_DOT2) return kres_repair_launch_t<5, __half, __half, 1>(a, blend, n_cu, stream);
    if (gh) return sh ? kres_repair_launch_t<5, __half, __half>(a, blend, n_cu, stream) : kres_repair_launch_t<5, __half, float>(a, blend, n_cu, stream);
    return kres_repair_launch_t<5, float, float>(a, blend, n_cu, stream);
}

int kres_history_repair_launch(const void* g, const void* x0, const void* sparse, void* hist, void* wk_out, const unsigned* abort_word, unsigned seq,
                               int B, int H, int W, int T, int blend, int n_cu, void* stream) {
    if (!kres_repair_fits(5, T)) return fail("cspnk_forward_resident_history: the guard re-computes at most 27 steps of a 5 x 5 stencil (T=%d)", T);
    const KHistRepArgs a{guard_geom(abort_word, seq, B, H, W, T), g, x0, sparse, hist, wk_out};
    return blend ? guard_launch<5, cspnk_history_repair<5, __half, __half, 1>>(a, n_cu, stream)
                 : guard_launch<5, cspnk_history_repair<5, __half, __half, 0>>(a, n_cu, stream);
}

int kres_sweep_repair_launch(const void* wk, const void* g_T, const void* sparse, int in_dtype, float* g32_out, float* hist, const unsigned* abort_word,
                             unsigned seq, int B, int H, int W, int T, int premask, int n_cu, void* stream) {
    if (!kres_repair_fits(5, T)) return fail("cspnk_transposed_resident: the guard re-computes at most 27 steps of a 5 x 5 stencil (T=%d)", T);
    const KSweepRepArgs a{guard_geom(abort_word, seq, B, H, W, T), wk, g_T, sparse, g32_out, hist};
    if (in_dtype == CSPN_F16)
        return premask ? guard_launch<5, cspnk_sweep_repair<5, __half, __half, 1>>(a, n_cu, stream)
                       : guard_launch<5, cspnk_sweep_repair<5, __half, __half, 0>>(a, n_cu, stream);
    return premask ? guard_launch<5, cspnk_sweep_repair<5, __half, float, 1>>(a, n_cu, stream)
                   : guard_launch<5, cspnk_sweep_repair<5, __half, float, 0>>(a, n_cu, stream);
}

}  // namespace cspn_detail

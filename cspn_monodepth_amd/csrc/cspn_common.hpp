// cspn_common.hpp — shared device/host helpers of the CSPN HIP engine (included by every translation unit).
// Everything here has internal linkage (anonymous namespace / inline) except the thread-local error channel.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "cspn_hip.h"

namespace cspn_detail {
// thread-local message of the last failing entry point on this thread (defined in cspn_metrics.hip)
int fail(const char* fmt, ...);
const char* last_error();
// cspn_resident.hip: the K = 3 softmax-weight form of the quad-based resident kernel (used by cspnk_forward_resident)
int resident_pac3_f32(const void* guided, const void* x0, const void* sparse, void* out, void* history, void* wk_out, void* work,
                      unsigned seq, unsigned* host_err, int B, int H, int W, int T, int blend, const void* target, double* acc,
                      int nslots, const cspn_resident_plan* plan, void* stream);
// cspnk_d2.hip: the K = 5 fp16 form with the state packed as fp16 pairs in LDS and v_dot2_f32_f16 steps (launched by cspnk_forward_resident)
int kres_d2_row_stride(int wo);
size_t kres_d2_lds_bytes(int dr, int ls, int threads);
int kres_d2_launch(const void* kres_args, int threads, int grid, size_t lds_bytes, int blend, int mode, int clean, void* stream);   // mode 0 plain, 1 scored, 2 history
// pac_conv2d_s2.hip: the pixel-adaptive convolution and its gradients for stride 2 x 2, dilation 1, K in {3, 5}, padding K / 2,
// W % 8 == 0 (launched by the cspn_pac_conv2d* entry points of pac_conv2d.hip when every base pointer is 16-byte aligned)
struct PacS2Args {
    int B, C, CK, H, W, Ho, Wo, WQ;      // WQ = Wo / 4 = W / 8 quads per output row
    int cchunk, nchunk, gx;              // channels per chunk, chunks, spatial workgroups per image (set by the launcher)
};
bool pac_s2_geometry(int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int W);
int pac_s2_forward(const void* in, const void* kern, void* out, int dtype, int K, const PacS2Args& a, void* stream);
int pac_s2_grad_input(const void* gout, const void* kern, void* gin, int dtype, int K, const PacS2Args& a, void* stream);
int pac_s2_grad_kernel(const void* gout, const void* in, void* gk, int dtype, int K, const PacS2Args& a, void* stream);
// cspn_repair.hip: the guard behind a plain resident inference launch (cspn_resident_plan.guard): re-computes the call's result
// on the stream when — and only when — its launches gave up (abort word == seq)
bool resident_repair_fits(int T);
// The form of a 3x3 resident launch: which instance of cspn3_resident runs it (cspn_resident.hip) and which instance of the guard
// re-computes it (cspn_repair.hip).  Both kernels take it as the template arguments MODE (resident_form_mode) and PAC (resident_form_pac:
// the softmax weights of CSPN_ours at K = 3).
enum class ResidentForm : int {
    Inference,             // refined depth -> out
    Scored,                // ... + the fused depth metrics
    Training,              // the training forward: every step's state -> history, the weights and / or S published
    SweepVolume,           // the backward's reverse sweep on a tap volume
    SweepGuidance,         // ... on taps rebuilt from the raw guidance + S
    SoftmaxInference, SoftmaxScored, SoftmaxTraining,      // the first three with softmax weights
    Count
};
constexpr int resident_form_pac(ResidentForm f) { return f >= ResidentForm::SoftmaxInference ? 1 : 0; }
constexpr int resident_form_mode(ResidentForm f) { return (int)f - (resident_form_pac(f) ? (int)ResidentForm::SoftmaxInference : 0); }
constexpr bool resident_form_guarded(ResidentForm f) { return f != ResidentForm::SoftmaxScored; }     // the forms the guard re-computes
int resident_repair_launch(const float* g, long bs, long cs, const float* d0, const float* sparse, float* out, float* hist, float* s_out,
                           float* w_out, const float* s_in, ResidentForm form, const unsigned* abort_word, unsigned seq, int B, int H, int W, int Wv,
                           int T, int blend, int n_cu, void* stream, const float* target = nullptr, double* acc = nullptr, int nslots = 0);
// ... and of cspnk_forward_resident's unscored inference calls (round_every: the steps between two roundings of the state to the plane dtype;
// step_form: CSPN_STEP_FMA or CSPN_STEP_DOT2, the form the guarded launch ran — its arithmetic is the one re-computed)
bool kres_repair_fits(int K, int T);
int kres_repair_launch(const void* g, int g_dtype, int K, const void* x0, const void* sparse, void* out, int state_dtype,
                       const unsigned* abort_word, unsigned seq, int B, int H, int W, int T, int round_every, int step_form, int blend, int n_cu,
                       void* stream);
// ... and of the K = 5 fp16 training forms: cspnk_forward_resident_history's dot-product launch and cspnk_transposed_resident
int kres_history_repair_launch(const void* g, const void* x0, const void* sparse, void* hist, void* wk_out, const unsigned* abort_word, unsigned seq,
                               int B, int H, int W, int T, int blend, int n_cu, void* stream);
int kres_sweep_repair_launch(const void* wk, const void* g_T, const void* sparse, int in_dtype, float* g32_out, float* hist, const unsigned* abort_word,
                             unsigned seq, int B, int H, int W, int T, int premask, int n_cu, void* stream);
// cspn_debug.hip: the poisoned-LDS debugging aid (include/cspn_hip.h: cspn_debug_set_lds_poison)
extern int g_lds_poison_on;
void lds_poison(hipStream_t st);
}  // namespace cspn_detail

// Every launch of the library goes through this hook: with the poisoned-LDS switch on, the whole LDS of every CU is filled with
// a pattern in front of the kernel (a kernel that reads LDS it never wrote then shows it).  Off: one predictable branch.
#define CSPN_PRELAUNCH(st)                                                                \
    do {                                                                                  \
        if (__builtin_expect(cspn_detail::g_lds_poison_on, 0)) cspn_detail::lds_poison(st);   \
    } while (0)
#define CSPN_PRE(st) (__builtin_expect(cspn_detail::g_lds_poison_on, 0) ? cspn_detail::lds_poison(st) : (void)0)   // expression form: `CSPN_PRE(st), kernel<<<...>>>(...)`
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, st, ...)                                \
    do {                                                                                  \
        CSPN_PRELAUNCH(st);                                                               \
        hipLaunchKernelGGLInternal((kern), (grid), (block), (lds), (st), __VA_ARGS__);    \
    } while (0)

namespace {

using cspn_detail::fail;
using cspn_detail::ResidentForm;
using cspn_detail::resident_form_guarded;
using cspn_detail::resident_form_mode;
using cspn_detail::resident_form_pac;

#define HIP_OK(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) return fail("%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

// ------------------------------------------------------------------------------------------------
// element access helpers: everything is computed in fp32, storage is f32 or f16
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const __half* p) {
    const uint2 raw = *reinterpret_cast<const uint2*>(p);
    const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&raw.x));
    const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&raw.y));
    return make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void st4(__half* p, float4 v) {
    uint2 raw;
    *reinterpret_cast<__half2*>(&raw.x) = __floats2half2_rn(v.x, v.y);
    *reinterpret_cast<__half2*>(&raw.y) = __floats2half2_rn(v.z, v.w);
    *reinterpret_cast<uint2*>(p) = raw;
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const __half* p) { return __half2float(*p); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(__half* p, float v) { *p = __float2half_rn(v); }

__device__ __forceinline__ float sgnf(float v) { return (float)((v > 0.f) - (v < 0.f)); }
__device__ __forceinline__ float4 sgn4(float4 v) { return make_float4(sgnf(v.x), sgnf(v.y), sgnf(v.z), sgnf(v.w)); }

// q[k] = a[k] / S for the 8 gates of one pixel (0 <= a[k] <= S), sharing one reciprocal:
//   r = v_rcp_f32(S) refined by one Newton step (r <- r + r (1 - S r)), q[k] = a[k] * r
// — 3 + 8 VALU operations.  Each quotient is within ~1.5 ulp of the IEEE one; the reference itself never forms these
// quotients (it divides the weighted SUM by S every step, CSPN_new.py:124-127), so neither rounding is "the" reference
// one: measured against it on full frames the refined depth moves from 4.6e-7 to 5.7e-7 max relative error (bar: 1e-5)
// while the derive launch loses 9 us of division sequences (v_div_scale / v_div_fmas / v_div_fixup + two residual
// corrections per quotient: 43 operations, kept as tools/probes/ieee_normalise.patch for A/B runs).
// S = 0 (all gates zero, also every padding pixel) needs no branch: rcp(0) = inf, the Newton step makes it NaN and
// 0 * NaN = NaN = 0 / 0.  Only a denormal-range or huge S — where v_rcp_f32 flushes — takes the true division.
__device__ __forceinline__ void div8_shared_reciprocal(const float (&a)[8], float S, float (&q)[8]) {
    const bool okr = (S <= 0x1p+100f) && (S >= 0x1p-100f || S == 0.f);
    if (okr) {
        float r = __builtin_amdgcn_rcpf(S);
        const float e = fmaf(-S, r, 1.0f);
        r = fmaf(e, r, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = a[k] * r;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = a[k] / S;
    }
}
// The reciprocal of that recipe on its own: 1 / S refined by one Newton step, with the true division outside [2^-100, 2^100] unless
// S is 0 — what the reverse sweep (cspn3_resident MODE 4) and the guard (cspn_repair.hip) multiply |g_j| by to rebuild the forward's gates.
__device__ __forceinline__ float reciprocal_as_forward(float S) {
    const bool okr = (S <= 0x1p+100f) && (S >= 0x1p-100f || S == 0.f);
    float r = __builtin_amdgcn_rcpf(S);
    r = fmaf(fmaf(-S, r, 1.0f), r, r);
    return okr ? r : 1.0f / S;
}
// The same for the four pixels of a quad, in place (w[k][e]: gate k of pixel e -> its quotient), with the true division behind ONE
// wave-uniform test (a ballot over the wavefront) per quad.  In the per-pixel form above the compiler gives each of the 8 quotients
// its own exec-masked division sequence (v_div_scale x 2 / v_div_fmas / v_div_fixup inside s_and_saveexec + s_cbranch_execz): in the
// derive of the 768-thread resident launch 88 such regions per wavefront, issued or skipped for an S that real guidance never
// produces.  Here the shared reciprocal is formed branch-free for every pixel, and a wavefront that holds an out-of-range S takes one
// cold block that redoes the quad with a select per quotient.  Both sides give every lane the bits of div8_shared_reciprocal.
// `keep` = false zeroes the quad instead (w must then hold zeros already: the reciprocal is replaced by 0, which costs 4 selects
// where zeroing the 32 quotients costs 32).
// (`&` / `|`, not `&&` / `||`: three compares and two scalar mask operations; the short-circuit form becomes exec-masked regions)
__device__ __forceinline__ bool reciprocal_in_range(float S) { return (S <= 0x1p+100f) & ((S >= 0x1p-100f) | (S == 0.f)); }
__device__ __forceinline__ float reciprocal_newton(float S) {
    float r = __builtin_amdgcn_rcpf(S);
    const float e = fmaf(-S, r, 1.0f);
    return fmaf(e, r, r);
}
__device__ __forceinline__ void div8_quad_shared_reciprocal(float (&w)[8][4], const float (&S)[4], bool keep = true) {
    float r[4];
    bool okr[4], bad = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        okr[e] = !keep | reciprocal_in_range(S[e]);
        r[e] = keep ? reciprocal_newton(S[e]) : 0.f;
        bad |= !okr[e];
    }
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(bad) != 0ull, 0)) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k][e] = okr[e] ? w[k][e] * r[e] : w[k][e] / S[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k][e] *= r[e];
    }
}

// exp(x) for x <= 0 (the max-subtracted logits) on the hardware exponential: v_exp_f32 is 2^t to 1 ulp; the product
// x * log2(e) is formed in two pieces (fma recovers its rounding error) so that the result stays within ~2 ulp of
// expf for every x instead of drifting by |x| * 2^-24.  libm's expf made both prepare kernels VALU-bound (~25 VALU
// operations per call, 24 calls per pixel at K = 5: 33.6 us for a pass whose HBM floor is 20 us).
__device__ __forceinline__ float exp_nonpositive(float x) {
    const float L2E = 1.44269502162933349609375f;          // float(log2(e))
    const float L2E_LO = 1.925963033500011e-8f;            // log2(e) - float(log2(e))
    const float t = x * L2E;
    const float r = fmaf(x, L2E, -t) + x * L2E_LO;         // what t lost
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147180559945f, e);             // 2^(t+r) = 2^t (1 + r ln 2 + ...)
}
__device__ __forceinline__ float reciprocal_refined(float d) {
    const float r = __builtin_amdgcn_rcpf(d);
    return fmaf(fmaf(-d, r, 1.0f), r, r);
}

// The softmax numerator exp(v - max) for a tap volume of type WT (CSPN_ours.py:35).  fp32 weights: the two-piece form above.
// fp16 weights: one multiply + v_exp_f32 — the argument's error (<= 24 * 1.4e-7 for every result that does not underflow in
// fp16) moves the numerator by ~2e-6 relative, 200x below half an fp16 ulp, and the derive of the weight-resident K x K
// launch (cspnk_resident.hip: 24 exponentials per pixel over tile + halo) is VALU-bound on exactly these operations.
// Every producer of fp16 softmax weights goes through this one function, so they all agree bit for bit.
// half(a * b) with ONE rounding (v_fma_mixlo_f16 / v_fma_mixhi_f16 round the exact product to fp16, and write the low / high
// half of `dst` leaving the other half alone): how every producer of fp16 softmax weights forms numerator * 1/sum.  Left to
// the compiler, `__float2half_rn(e * inv)` is fused into this instruction in some kernels and stays a multiply + a conversion
// (two roundings) in others — 6e-5 of the weights then differ by an fp16 ulp between kernels that must agree bit for bit.
__device__ __forceinline__ unsigned mul_into_half_lo(unsigned dst, float a, float b) {
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(dst) : "v"(a), "v"(b));
    return dst;
}
__device__ __forceinline__ unsigned mul_into_half_hi(unsigned dst, float a, float b) {
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(dst) : "v"(a), "v"(b));
    return dst;
}
// numerator * (1 / sum) as the value the tap volume of type WT will hold
template <typename WT> __device__ __forceinline__ float softmax_weight(float e, float inv) { return e * inv; }
template <> __device__ __forceinline__ float softmax_weight<__half>(float e, float inv) {
    const unsigned r = mul_into_half_lo(0u, e, inv);
    return __half2float(__ushort_as_half((unsigned short)(r & 0xffffu)));
}

template <typename WT> __device__ __forceinline__ float softmax_exp(float d) { return exp_nonpositive(d); }
template <> __device__ __forceinline__ float softmax_exp<__half>(float d) {
    return __builtin_amdgcn_exp2f(d * 1.44269502162933349609375f);
}

// The softmax weights of one pixel (CSPN_ours.py:35), in place: raw logits in, the values a tap volume of type WT holds out.
// Maximum, softmax_exp<WT>, the sum in channel order from 0, one refined reciprocal, softmax_weight<WT>: the arithmetic of every
// producer of softmax taps, and the one copy of it behind the guard kernels of cspn_repair.hip.
// Remaining copies — hot kernels whose device code changes when they call this (another schedule; in the quad kernel commuted
// v_add_f32 operands), which therefore keep the five operations spelled out and are held to them by the guard tests' bit
// comparisons: cspn_pac_prepare_kernel and cspn_pac_prepare_vec_kernel (cspn_prepare.hip), the PAC derive of cspn3_resident
// (cspn_resident.hip), the fp32 derive of cspnk_resident (cspnk_resident.hip).
template <typename WT, int NT>
__device__ __forceinline__ void softmax_in_channel_order(float (&v)[NT]) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < NT; ++c) mx = fmaxf(mx, v[c]);
    float den = 0.f;
#pragma unroll
    for (int c = 0; c < NT; ++c) { v[c] = softmax_exp<WT>(v[c] - mx); den += v[c]; }
    const float inv = reciprocal_refined(den);
#pragma unroll
    for (int c = 0; c < NT; ++c) v[c] = softmax_weight<WT>(v[c], inv);
}

// The taps of a K x K stencil are its pixels in row-major order without the centre: tap j reads the pixel at (tap_dy, tap_dx).
template <int K> constexpr int tap_lin(int j) { return j < (K * K - 1) / 2 ? j : j + 1; }
template <int K> constexpr int tap_dy(int j) { return tap_lin<K>(j) / K - K / 2; }
template <int K> constexpr int tap_dx(int j) { return tap_lin<K>(j) % K - K / 2; }

// The 3x3 gates of pixel (y, x): a[j] = |g_{7-j}[p + off_j]| (the reference's shifts, CSPN_new.py:29-70; 0 outside rows [0, H) and
// columns [0, W)), and their sum S in the reference's channel order k = 0..7, i.e. tap 7..0 (CSPN_new.py:124-127): what the guard of
// the 3x3 resident launch (cspn_repair.hip) normalises by.  gb: channel 0 of the image.  Remaining copy: cspn3_prepare_kernel (its
// device code changes when it calls this).
template <typename GT>
__device__ __forceinline__ float abs_gates8(const GT* gb, long cs, int y, int x, int H, int W, float (&a)[8]) {
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int j = 7 - k, yy = y + tap_dy<3>(j), xx = x + tap_dx<3>(j);
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = fabsf(ld1(gb + (size_t)k * cs + (size_t)yy * W + xx));
        a[j] = v;
        S = (k == 0) ? v : S + v;
    }
    return S;
}

// The 10 masked terms of Result.evaluate (libs/metrics.py:49-83) for one pixel, added to f[0..9]:
// {inv^2, inv, diff^2, diff, diff/t, |log10 o - log10 t|, #(r<1.25), #(r<1.25^2), #(r<1.25^3), 1} over t > 0.
// Algebraically equal forms that avoid cancellation and redundant divisions:
//   |1/o - 1/t| = |o-t| / |o t|,   |log10 o - log10 t| = |log10(o/t)| = |log2(o/t)| log10(2),
//   max(o/t, t/o) < c  <=>  |log2(o/t)| < log2(c)  for o > 0;  o < 0 counts (both ratios are negative), o = 0 and NaN do not
//   (torch.max semantics) — the one logarithm of the log-error term serves the three thresholds.
// Reciprocals and the logarithm use the hardware v_rcp_f32 / v_log_f32 (1 ulp): the terms are summed over
// ~10^5..10^6 pixels and compared at 1e-5, and IEEE divisions + log10f made this reduction VALU-bound.
// Branch- and select-free masking: an invalid pixel (t <= 0 or NaN) is scored as o = t = 1, which adds exactly 0 to the six
// error sums, and the four counters take the validity as a condition.  ~30 VALU operations + 3 transcendentals per pixel;
// the form with six products and twelve compares per pixel (86 instructions with its masking) was 5.7 us of every scored
// config-2 forward.
__device__ __forceinline__ void metric_terms(float o, float t, float (&f)[10]) {
    const bool valid = t > 0.f;
    const float tt = valid ? t : 1.f, oo = valid ? o : 1.f;
    const float ad = fabsf(oo - tt);
    const float rt = __builtin_amdgcn_rcpf(tt);
    const float inv = ad * __builtin_amdgcn_rcpf(fabsf(oo * tt));
    f[0] = fmaf(inv, inv, f[0]);
    f[1] += inv;
    f[2] = fmaf(ad, ad, f[2]);
    f[3] += ad;
    f[4] = fmaf(ad, rt, f[4]);
    const float r = oo * rt;
    const float lg = fabsf(__builtin_amdgcn_logf(r));                       // |log2(o/t)|; NaN for o < 0 (as log10 of a negative)
    f[5] = fmaf(lg, 0.30102999566398120f, f[5]);
    const bool neg = r < 0.f;
    constexpr float L1 = 0.32192809488736235f;                             // log2(1.25)
    f[6] += (valid && (lg < L1 || neg)) ? 1.f : 0.f;
    f[7] += (valid && (lg < 2.f * L1 || neg)) ? 1.f : 0.f;
    f[8] += (valid && (lg < 3.f * L1 || neg)) ? 1.f : 0.f;
    f[9] += valid ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------------
// Tap-volume layout (the [B, K*K-1, H, W] weight volume the propagation streams)
//   f32: planar, tap plane j of image b at ((b*NT + j)*HW + p).
//   f16: taps interleaved in PAIRS per 4-pixel quad — [B][NT/2][ceil(HW/4)][2][4] — so that one 16-byte load
//        returns taps (2i, 2i+1) of a quad.  8-byte loads run at about half the per-byte rate of 16-byte loads
//        on gfx950; with planar f16 planes the kernel was slower than its f32 twin.
// p = y*W + x is the linear pixel index inside an image; every kernel goes through Taps<WT>.
// ------------------------------------------------------------------------------------------------
template <typename WT> struct Taps;
template <> struct Taps<float> {
    __host__ __device__ static size_t image_elems(int NT, size_t HW) { return (size_t)NT * HW; }
    __device__ static size_t idx(int j, size_t p, size_t HW) { return (size_t)j * HW + p; }
};
template <> struct Taps<__half> {
    __host__ __device__ static size_t hw4(size_t HW) { return (HW + 3) & ~(size_t)3; }
    __host__ __device__ static size_t image_elems(int NT, size_t HW) { return (size_t)NT * hw4(HW); }
    __device__ static size_t idx(int j, size_t p, size_t HW) {
        return (size_t)(j >> 1) * 2 * hw4(HW) + ((p >> 2) << 3) + ((size_t)(j & 1) << 2) + (p & 3);
    }
};

typedef float v4f __attribute__((ext_vector_type(4)));
typedef const volatile __attribute__((address_space(3))) v4f* lds_cv4f_ptr;   // LDS (addrspace 3) volatile b128

// Wavefront-level halo exchange: value held by lane-1 / lane+1 (DPP wave shift, VALU only).  Lanes without
// a source (0 / 63) or with an exec-masked source get 0 (bound_ctrl) and are patched from LDS by the caller.
__device__ __forceinline__ float dpp_from_prev_lane(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_from_next_lane(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
}

// Sum of v over the 64 lanes of a wavefront, valid in lane 63.  VALU only (DPP row shifts + the gfx9 row broadcasts):
// the __shfl_down ladder is 6 ds_bpermute_b32 per value and the LDS crossbar became the cost of the fused metrics
// reduction (10 values x 16 waves per workgroup).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_step(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
    v = dpp_add_step<0x111, 0xf>(v);      // row_shr:1
    v = dpp_add_step<0x112, 0xf>(v);      // row_shr:2
    v = dpp_add_step<0x114, 0xf>(v);      // row_shr:4
    v = dpp_add_step<0x118, 0xf>(v);      // row_shr:8   -> lane 15 of every row of 16 holds its row sum
    v = dpp_add_step<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = dpp_add_step<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wavefront sum
    return v;
}

// The same for fp64 (the standalone metrics kernel accumulates arbitrarily many pixels per thread): DPP moves the two
// 32-bit halves, the add is a plain v_add_f64.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_step(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, true);
    return x + __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_sum_to_lane63(double v) {
    v = dpp_add_step<0x111, 0xf>(v);
    v = dpp_add_step<0x112, 0xf>(v);
    v = dpp_add_step<0x114, 0xf>(v);
    v = dpp_add_step<0x118, 0xf>(v);
    v = dpp_add_step<0x142, 0xa>(v);
    v = dpp_add_step<0x143, 0xc>(v);
    return v;
}

// All NT taps of the quad starting at pixel p (p % 4 == 0) of one image's tap volume -> out[NT][4] (fp32).
template <int NT>
__device__ __forceinline__ void load_taps_quad(const float* img, size_t p, size_t HW, bool ok, float (&out)[NT][4]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const float4 v = ok ? ld4(img + (size_t)j * HW + p) : make_float4(0.f, 0.f, 0.f, 0.f);
        out[j][0] = v.x; out[j][1] = v.y; out[j][2] = v.z; out[j][3] = v.w;
    }
}
template <int NT>
__device__ __forceinline__ void load_taps_quad(const __half* img, size_t p, size_t HW, bool ok, float (&out)[NT][4]) {
    const size_t pair_stride = 2 * Taps<__half>::hw4(HW);
#pragma unroll
    for (int jp = 0; jp < NT / 2; ++jp) {
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (ok) raw = *reinterpret_cast<const uint4*>(img + (size_t)jp * pair_stride + 2 * p);
        const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&raw.x));
        const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&raw.y));
        const float2 c = __half22float2(*reinterpret_cast<const __half2*>(&raw.z));
        const float2 d = __half22float2(*reinterpret_cast<const __half2*>(&raw.w));
        out[2 * jp][0] = a.x; out[2 * jp][1] = a.y; out[2 * jp][2] = b.x; out[2 * jp][3] = b.y;
        out[2 * jp + 1][0] = c.x; out[2 * jp + 1][1] = c.y; out[2 * jp + 1][2] = d.x; out[2 * jp + 1][3] = d.y;
    }
}
// acc + w * x with w = element e of tap (2i + odd) taken straight from a packed pair register set (see the f16
// tap-volume layout: words x,y hold the even tap's pixels (0,1),(2,3), words z,w the odd tap's).  One
// v_fma_mix_f32 (f16 source selected by op_sel) — written as asm because, given C++ conversions, the optimiser
// hoists all of them out of the step loop and materialises the weights as fp32 again (197 instead of ~110 VGPRs).
__device__ __forceinline__ float fma_packed_tap(const uint4& r, int odd, int e, float x, float acc) {
    const unsigned w = odd ? ((e >> 1) ? r.w : r.z) : ((e >> 1) ? r.y : r.x);
    float out;
    if (e & 1) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(out) : "v"(w), "v"(x), "v"(acc));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(out) : "v"(w), "v"(x), "v"(acc));
    return out;
}

// acc + w * x with w = half e (0..7) of an OCT register set: r.x = pixels (0,1), r.y = (2,3), r.z = (4,5), r.w = (6,7) of one
// tap — the layout of a 16-byte load from a planar fp16 tap / kernel plane.  One v_fma_mix_f32 (see fma_packed_tap).
__device__ __forceinline__ float fma_h8(const uint4& r, int e, float x, float acc) {
    const unsigned w = (e >> 1) == 0 ? r.x : ((e >> 1) == 1 ? r.y : ((e >> 1) == 2 ? r.z : r.w));
    float out;
    if (e & 1) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(out) : "v"(w), "v"(x), "v"(acc));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(out) : "v"(w), "v"(x), "v"(acc));
    return out;
}

// the matching quad stores
template <int NT>
__device__ __forceinline__ void store_taps_quad(float* img, size_t p, size_t HW, const float (&v)[NT][4]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) st4(img + (size_t)j * HW + p, make_float4(v[j][0], v[j][1], v[j][2], v[j][3]));
}
template <int NT>
__device__ __forceinline__ void store_taps_quad(__half* img, size_t p, size_t HW, const float (&v)[NT][4]) {
    const size_t pair_stride = 2 * Taps<__half>::hw4(HW);
#pragma unroll
    for (int jp = 0; jp < NT / 2; ++jp) {
        uint4 raw;
        *reinterpret_cast<__half2*>(&raw.x) = __floats2half2_rn(v[2 * jp][0], v[2 * jp][1]);
        *reinterpret_cast<__half2*>(&raw.y) = __floats2half2_rn(v[2 * jp][2], v[2 * jp][3]);
        *reinterpret_cast<__half2*>(&raw.z) = __floats2half2_rn(v[2 * jp + 1][0], v[2 * jp + 1][1]);
        *reinterpret_cast<__half2*>(&raw.w) = __floats2half2_rn(v[2 * jp + 1][2], v[2 * jp + 1][3]);
        *reinterpret_cast<uint4*>(img + (size_t)jp * pair_stride + 2 * p) = raw;
    }
}

// blockIdx -> logical tile id such that XCD x (= blockIdx % 8, observed dispatch order; speed only,
// never correctness) processes one contiguous range of tiles.
__device__ __forceinline__ int xcd_contiguous_id(int bid, int nb) {
    const int q = nb >> 3, r = nb & 7;
    const int x = bid & 7, j = bid >> 3;
    return x * q + (x < r ? x : r) + j;
}

// ------------------------------------------------------------------------------------------------
// small host helpers
// ------------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up4(int a) { return (a + 3) & ~3; }
inline size_t esize(int dt) { return dt == CSPN_F16 ? 2 : 4; }

int grid_for(size_t n, int block) {
    size_t g = (n + block - 1) / block;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

// Launches with more than 64 KiB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised once per
// (kernel instance, device); the granted size is remembered so the hot loop does not repeat the driver call.
template <auto Kern>
int ensure_dynamic_lds(size_t bytes) {
    static std::atomic<size_t> granted[64];
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    std::atomic<size_t>& slot = granted[dev & 63];
    if (slot.load(std::memory_order_acquire) >= bytes) return 1;
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    size_t seen = slot.load(std::memory_order_relaxed);
    while (seen < bytes && !slot.compare_exchange_weak(seen, bytes, std::memory_order_release)) {}
    return 1;
}
// ... and the launch behind it (through the library's hipLaunchKernelGGL: the poisoned-LDS hook runs).  Its address is what the
// tables of instances hold where the kernel is chosen at run time.
template <auto Kern, typename Args>
int launch_dynamic_lds(int grid, int threads, size_t lds_bytes, hipStream_t st, const Args& a) {
    if (lds_bytes > 64 * 1024 && !ensure_dynamic_lds<Kern>(lds_bytes)) return 0;
    hipLaunchKernelGGL(Kern, dim3(grid), dim3(threads), lds_bytes, st, a);
    HIP_OK(hipGetLastError());
    return 1;
}

// ------------------------------------------------------------------------------------------------
// what the weight-resident engines (cspn_resident.hip, cspnk_resident.hip) share on the host
// ------------------------------------------------------------------------------------------------
// Workspace of a resident call: 2 exchange planes of B x H x W elements, then — at a fixed place, whatever the tiling — 4 status
// words (abort, error, 2 reserved), then one phase flag per tile (a tile has at least `min_tile_pixels` pixels).
inline size_t resident_planes_bytes(int B, int H, int W, size_t elem_size) { return ((size_t)2 * B * H * W * elem_size + 15) & ~(size_t)15; }
inline size_t resident_workspace_bytes(int B, int H, int W, size_t elem_size, int min_tile_pixels) {
    const size_t flags = ((size_t)B * (((size_t)H * W) / min_tile_pixels + 1) + 4) * sizeof(unsigned);
    return resident_planes_bytes(B, H, W, elem_size) + ((flags + 15) & ~(size_t)15);
}
inline unsigned* resident_status_words(void* work, int B, int H, int W, size_t elem_size) {
    return reinterpret_cast<unsigned*>(static_cast<char*>(work) + resident_planes_bytes(B, H, W, elem_size));
}
inline unsigned* resident_phase_flags(unsigned* status) { return status + 4; }

// does the plan carry a tiling (one that came out of cspn3_resident_plan / cspnk_resident_plan: the launch then skips its search)?
inline bool plan_has_tiling(const cspn_resident_plan& rp) {
    return rp.tiles_x > 0 && rp.tiles_y > 0 && rp.tile_w > 0 && rp.tile_h > 0 && rp.steps_per_phase > 0 && rp.images_per_launch > 0;
}
inline unsigned plan_spin_limit(const cspn_resident_plan& rp) { return rp.spin_limit ? rp.spin_limit : (4u << 20); }   // x (sc1 load + s_sleep) ~ seconds

// Argument rules of the resident entry points; `who` is the entry point's name.  (A null pointer counts as aligned: whether a tensor
// may be absent is the entry point's own rule.)
inline bool all_aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (!aligned16(p)) return false;
    return true;
}
inline int check_tensors_aligned16(const char* who, std::initializer_list<const void*> ps) {
    return all_aligned16(ps) ? 1 : fail("%s: tensors must be 16-byte aligned", who);
}
inline int check_blend(const char* who, int blend, const void* sparse) {
    if (blend != CSPN_BLEND_NONE && blend != CSPN_BLEND_SPARSE) return fail("%s: blend %d", who, blend);
    if (blend && !sparse) return fail("%s: blend needs sparse", who);
    return 1;
}
inline int check_premask(const char* who, int premask, const void* sparse) {
    return premask && !sparse ? fail("%s: premask needs sparse", who) : 1;
}
inline int check_scoring(const char* who, const void* target, const void* acc, int nslots) {
    if ((target || acc) && (!target || !acc || nslots < 1 || !aligned16(target)))
        return fail("%s: scoring needs target (16-byte aligned), acc and nslots >= 1", who);
    return 1;
}
// a tile that finished phase p publishes seq + p + 1, and the next call on the workspace brings seq + 256
inline int check_seq(const char* who, unsigned seq) {
    return seq == 0 || seq > 0x7fffff00u ? fail("%s: seq must be in [1, 2^31 - 256]", who) : 1;
}

}  // namespace

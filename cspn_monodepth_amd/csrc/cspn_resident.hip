// cspn_resident.hip — the 3x3 inference forward as ONE launch with the weights RESIDENT in registers for all T steps.
//
// Reference path: network/libs/post_process/CSPN_new.py:26-92 (abs / shift / normalise once, then 24 x {8-way propagate,
// blend}).  The multi-launch schedule of cspn_propagate.hip re-streams the 8 weight planes once per launch of S steps
// (config 2: 53 MB written once, read twice = 160 of the 271 MB a forward moves).  Here a workgroup owns ONE tile for the
// whole forward:
//   * it derives the normalised weights of its tile + (S-1)-pixel halo from the raw guidance ONCE (same arithmetic as
//     cspn3_prepare_kernel / the WSRC=1 launch, div8_shared_reciprocal) and keeps them in VGPRs: no weight volume exists;
//   * the T steps run in phases of S steps on the depth tile in LDS (the step loop of cspn_prop_fused);
//   * between phases the workgroups exchange their tile borders through a global scratch plane with DEVICE-SCOPE (sc1)
//     stores / loads — coherent across the 8 XCDs' private L2s without any cache-wide write-back or invalidate — and a
//     per-tile phase flag the 8 neighbouring tiles poll (point-to-point, no grid barrier).
// HBM traffic of a forward drops to ~the compulsory 8 guidance planes + depth in / out (+ the border exchange).
//
// All workgroups of a launch must be co-resident (they wait for each other): a launch never has more workgroups than the
// device has CUs (every instance fits at least once per CU), images are chunked over several launches when a batch needs
// more tiles than CUs.  The neighbour wait is bounded: on time-out (another tenant holding CUs for seconds) the launch
// sets the abort / error words of its workspace, the remaining workgroups drain, and the host raises on the next call
// instead of hanging (include/cspn_hip.h: cspn3_forward_resident).
//
// Measured on MI355X (config 2: B=24, 228x304, T=24; profiles/r02_*): 2x5 tiles of 152x46 per image = 240 workgroups of
// 512 threads x 5 quads (160 weight registers per thread, 256 VGPRs, 2 wavefronts per SIMD), 8-step phases.  Timeline per
// workgroup (tools/resident_stamps.py): weights derived 11.0 us (the guidance stream, HBM-bound) + 3.0 us until the
// slowest wavefront has parked, 3 x 6.0 us of steps (VALU-bound: 228 instructions per wavefront-step, 160 of them FMAs),
// 2 x (2.6 us exchange + 1.35 us halo staging), fused metrics 3.6 us + launch ~2 us: 46 us per scored forward against 73 us for
// the three S=8 launches, with 2.3x less HBM traffic.
//
// The 768-thread instances (config 2 today: 3 quads per thread on clipped regions, three wavefronts per SIMD) publish their borders INSIDE
// the last step of a phase: a peeled form of the step body stores every interior row to the exchange plane right behind the row's
// ds_write, waits for vmcnt(0) in front of its closing barrier, and that barrier stands for "everybody's stores have landed" — no
// separate publish pass, one barrier less per boundary, the store acknowledge under the FMAs of the rows that follow (exchange 2.5 ->
// 1.45 us, the scored forward 40.0-40.2 -> 39.0-39.2 us, sparse 45.9-46.0 -> 43.5-43.8: profiles/r15_boundary_ab.txt).  The same
// instances stamp their tail (target consumed, sums added) for tools/resident_stamps.py.  The 512- / 1024-thread instances keep their code.
//
// What keeps the 256-VGPR instances spill-free (each item was a measured regression before it was written this way):
//   * every scratch reload inside the derive is an s_waitcnt vmcnt(0) in the middle of the in-order guidance stream, so
//     the derive carries nothing it does not need: loads / stores go through an SGPR base + 32-bit byte offset in address
//     space 1 (at32: no address pairs, no flat loads), staging addresses advance without divisions, and everything the
//     later stages address with is recomputed from late, opaque copies of the strip coordinates;
//   * the step loop is unrolled by two with the LDS buffers RES_PP apart (the other buffer is an immediate offset, the
//     carried quads alternate between two register sets instead of being copied), sits inside a wave-uniform branch,
//     and computes unconditionally with masked stores;
//   * v_pk_fma_f32 does not help: it issues at half the rate of v_fma_f32 here (tools/probes/pk_fma_probe.hip).
#include "cspn_common.hpp"

#include <array>
#include <utility>

namespace {

struct ResArgs {
    const float* g;          // guidance [B,C>=8,H,W], channels 0..7 read in place
    long g_bs, g_cs;
    const float* d0;         // [B,H,W]
    const float* sparse;     // [B,H,W] or null
    float* out;              // [B,H,W]
    float* xbuf;             // exchange planes [2][B,H,W] (workspace)
    unsigned* flags;         // [B * tiles_per_img] phase flags (workspace, zero-initialised once)
    unsigned* status;        // [0] abort word of the running launch chain, [1] sticky error word (workspace)
    unsigned* host_err;      // optional TWO host-mapped words: [0] receives the error as well, [1] receives `seq` when the
                             // last launch of the call has finished (all workgroups passed their end)
    int last_chunk;          // this launch is the last one of the call
    unsigned seq;            // flag base of this call: a tile that finished phase p publishes seq + p + 1
    float* hist;             // MODE 2: [T][B,H,W] receives the state after every step (d_1 .. d_T), `out` is unused
    float* w_out;            // MODE 2: [B,8,H,W] receives the normalised weights (the backward streams them)
    float* s_out;            // MODE 2: [B,H,W] receives the normaliser S (the backward's quotient rule needs it)
    const float* s_in;       // MODE 4: [B,H,W] the normaliser S the training forward published (a.g is the raw guidance)
    const float* target;     // MODE 1: [B,H,W]
    double* macc;
    int nslots;
    int B, H, W, Wv, T, S;
    int tw, th, tiles_x, tiles_y;
    int wq, wr, hxw, hyw, dr, ls;
    int b0, nb;              // images [b0, b0 + nb) are refined by this launch
    unsigned spin_limit;
    unsigned long long* dbg;  // developer probe: [grid][16] wall-clock stamps (100 MHz) per workgroup, or null
    int th0, thl;            // heights of the first / last tile row (res_row_h); th is the height of the rows in between.  (Last: only the
                             // clipped instances read them, and the kernel arguments of the others stay where their code was tuned.)
    // Quotients the kernel needs in front of its first load, as host-made reciprocals (res_magic / res_div): a division by a run-time
    // value is ~20 dependent instructions, and five of them stood between the kernel's entry and the request for the depth region.
    unsigned mg_wq, mg_tiles_x, mg_tpi, mg_round;       // of wq, tiles_x, tiles_x * tiles_y, nb * tiles_x * tiles_y
    int step_r, step_q;                                 // NTHREADS / wq and NTHREADS % wq of the launch's instance
};
// n / d for 0 <= n < 2^16, 1 <= d < 2^16 as the high word of n * ceil(2^32 / d): exact, because the excess n * (d * m - 2^32) / (d * 2^32)
// of n * m / 2^32 over n / d stays below 1 / d while n * d < 2^32.  d == 1 has no 32-bit reciprocal: m = 0 stands for it.
inline unsigned res_magic(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)d - 1u) / (unsigned)d); }
__device__ __forceinline__ int res_div(int n, unsigned m) { return m ? (int)__umulhi((unsigned)n, m) : n; }

__device__ __forceinline__ void st4_dev(float* base, unsigned elem, float a, float b, float c, float d) {
    // ONE 16-byte device-scope store (global_store_dwordx4 ... sc1): visible to every XCD once vmcnt drops.  Written as
    // asm because the compiler only offers <= 8-byte atomics, and two 8-byte stores per quad touch every 64-byte line
    // twice with half masks (PMC: 2x the written bytes).  The caller waits with s_waitcnt vmcnt(0) before it signals.
    // `base` is wave-uniform (the image's exchange plane): SGPR base + 32-bit VGPR byte offset, no 64-bit address math.
    const v4f v = {a, b, c, d};
    asm volatile("global_store_dwordx4 %0, %1, %2 sc1" ::"v"(elem * 4u), "v"(v), "s"(base) : "memory");
}
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {      // a wave-uniform pointer, pinned to an SGPR pair
    const unsigned long long u = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}
// element `e` of a wave-uniform plane as SGPR base + 32-bit VGPR BYTE offset (planes stay below 2^30 elements: the host
// checks), so that no load / store of the kernel needs 64-bit address arithmetic or an address register pair
// The result is typed as a GLOBAL (address space 1) pointer: a pointer rebuilt from integers is otherwise generic, and a
// flat_load counts on vmcnt AND lgkmcnt and may return out of order — every wait after one becomes vmcnt(0).
#define GLB __attribute__((address_space(1)))
typedef GLB char* gptr;
__device__ __forceinline__ gptr at32(const float* base, unsigned e) {
    return (gptr) reinterpret_cast<unsigned long long>(base) + (e << 2);
}
__device__ __forceinline__ float4 ld4(gptr p) {
    const v4f v = *reinterpret_cast<const GLB v4f*>(p);
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float ld1(gptr p) { return *reinterpret_cast<const GLB float*>(p); }
__device__ __forceinline__ void st4(gptr p, float4 v) {
    const v4f w = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<GLB v4f*>(p) = w;
}
// The history planes of the training forms (d_1..d_T of MODE 2, G_{T-1}..G_0 of MODE 3 / 4: 160 MB per launch at config 2) are
// written once and read by a LATER kernel: stored non-temporally they do not push the guidance / exchange lines out of the L2
// while the launch runs, and the tail that streams them afterwards runs faster as well — same-box A/B, two alternating
// repetitions: tail 95.2-97.1 -> 86.8-87.3 us, sparse training forward 69.7-70.3 -> 64.9-65.4, sparse reverse sweep 75.4-76.9 ->
// 72.4-73.7, the plain forward / sweep -0 / -1.4 us (the other side of the A/B: the plain store of st4 above).
__device__ __forceinline__ void st4_hist(gptr p, float4 v) {
    const v4f w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<GLB v4f*>(p));
}
// Round 6, measured and NOT the default (NEGATIVE_RESULTS #53-#55; profiles/r06_step_pipe_ab.txt): the step's LDS round trips.  A step is
//   barrier -> ds_read of the two halo rows -> wait -> DPP of all rows -> exec-masked ds_read of the strip-end lanes' columns -> wait -> FMAs
//   -> ds_write -> wait -> barrier:  two LDS read latencies in series behind every barrier.
// tools/probes/res_step_pipe.patch takes the own rows' neighbour columns (DPP: registers of the neighbouring lanes, no LDS) BEFORE the barrier, from the rows
// just computed, in the shadow of the ds_write latency, and issues EVERY LDS read of the step right behind the barrier (the halo rows' strip-end
// columns into temporaries, merged with one select after the halo rows' DPP): one read latency instead of two, bit-identical — and SLOWER on every
// shape (config 2 +1.6 us, shards +1.0 / +1.2 us).  The two perf-only experiments of tools/probes/res_step_bounds.patch (wrong results, timing only) say why nothing of this kind can pay: without ANY
// strip-end read the forward is no faster (+-0.3 us), and without ANY step barrier it gains 2.3 us at config 2, 0.4 us at NYU B = 3, 1.4 us at
// KITTI B = 1 — the step is bound by VALU issue (one instruction per wavefront every ~5 cycles, 2.5 per SIMD with its two wavefronts:
// tools/probes/vgpr_bank_probe.hip), not by its barrier or its LDS latency, so "two steps per barrier" (+20..100 % FMAs for half of that) loses.
__device__ __forceinline__ float4 ld4_dev(gptr p) {
    const unsigned long long lo = __hip_atomic_load(reinterpret_cast<const GLB unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load(reinterpret_cast<const GLB unsigned long long*>(p) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float4(__uint_as_float((unsigned)lo), __uint_as_float((unsigned)(lo >> 32)), __uint_as_float((unsigned)hi),
                       __uint_as_float((unsigned)(hi >> 32)));
}
__device__ __forceinline__ float ld1_dev(gptr p) {
    return __uint_as_float(__hip_atomic_load(reinterpret_cast<const GLB unsigned*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

constexpr int RES_THREADS = 512;
constexpr int RES_THREADS_CLIPPED = 768;     // three wavefronts per SIMD, NQ = 3, clipped regions (resident_geometry_clipped)

// Tile rows and region origins, shared by the kernel and the host's checks (regions_inside_image).  Tile columns are all tw wide.
// Tile rows may be uneven: row 0 is th0 high, the last row thl, the rows in between th (the 512- / 1024-thread plans: all three are
// the same; the clipped plans make the first and the last row taller by the halo they do not need at the image edge, so that all
// regions are equally high).  The last row may still be cut short by the image.
// UNEVEN = false is the same arithmetic for instances whose rows are known to be all th high (the kernel's 512- / 1024-thread
// instances: their register allocation is tuned to the last scratch slot, and must not see the general form); the host uses the
// general form for every plan.
template <bool UNEVEN = true>
__host__ __device__ __forceinline__ int res_row_y0(int ty, int th0, int th) {
    if (!UNEVEN) return ty * th;
    return ty <= 0 ? 0 : th0 + (ty - 1) * th;
}
template <bool UNEVEN = true>
__host__ __device__ __forceinline__ int res_row_h(int ty, int tiles_y, int th0, int th, int thl) {
    if (!UNEVEN) return th;
    return ty == 0 ? th0 : (ty == tiles_y - 1 ? thl : th);
}
// Region origin: tile - halo, moved back into the image where a region of the launch's (fixed) size would stick out, but never
// before the previous tile's start when the launch exchanges borders (the halo must come from the 8 adjacent tiles).
__host__ __device__ __forceinline__ int res_region_x0(int tx, int tw, int hxw, int wq, int W, bool exch) {
    const int x0 = tx * tw;
    return max(exch ? max(0, x0 - tw) : 0, min(x0 - hxw, W - 4 * wq));
}
template <bool UNEVEN = true>
__host__ __device__ __forceinline__ int res_region_y0(int ty, int th0, int th, int hyw, int wr, int H, bool exch) {
    const int y0 = res_row_y0<UNEVEN>(ty, th0, th);
    const int lo = exch ? (UNEVEN ? res_row_y0(ty - 1, th0, th) : max(0, y0 - th)) : 0;
    return max(lo, min(y0 - hyw, H - wr));
}
// The two depth buffers of the step loop sit a COMPILE-TIME distance apart (RES_PP floats; the second one starts there
// whatever the region size): with the step loop unrolled by two, "the other buffer" is then an immediate offset of the
// ds_read / ds_write instead of a second set of row addresses (7 VGPRs the 256-register instances do not have), and no
// pointer is swapped per step.  65408 bytes + the largest row-relative offset still fit the 16-bit offset field.
constexpr int RES_PP = 16352;

// CLEAN = 1: the host verified that every region of the launch lies inside the image (shifted regions, image at least one
// region large, no row padding): the step body carries no zero-padding selects.  A launch-level property, so that each
// instance holds ONE copy of the step body (+ the peeled final step) — two copies in one kernel cost the 256-VGPR
// instances their spill-free hot loop.
// MODE 0: inference; 1: inference + fused depth metrics; 2: training forward — every step's state goes to its history
// plane and the weights + S are published once (what cspn3_propagate_from_guidance hands the backward).
// PAC = 1: the weights are the softmax over the 8 guidance channels at the CENTRE pixel (tap j = channel j: the K = 3 case of
// CSPN_ours.py:35-41) instead of the neighbour-indexed, sum-normalised gates of CSPN_new — everything after the derive (steps,
// exchange, blend, metrics, history planes) is the same recurrence.  MODE 2 publishes the softmax taps as the [B,8,H,W] volume the
// backward streams (no S: the softmax backward does not need one); the reverse sweep is the plain MODE 3 on that volume.
template <int NQ, int NTHREADS, int BLEND, int MODE, int CLEAN, int PAC = 0>
__global__ __launch_bounds__(NTHREADS, NTHREADS / 256) void cspn3_resident(const ResArgs a) {
    static_assert(!PAC || MODE <= 2, "the softmax-weight form has no transposed sweep of its own (the published volume feeds MODE 3)");
    constexpr int R = 1, NT = 8, WIN = 6;
    // MODE 3: the backward's reverse sweep  G_t = stencil^T((1-m) G_{t+1})  as the same recurrence on the TRANSPOSED taps:
    // tap j = w_{7-j}[p + off_j], gathered from the forward tap volume [B,8,H,W] (a.g) exactly like channel 7-j of the
    // guidance is gathered for the forward — minus |.| and the normalisation.  BLEND then means PREMASK: the state that
    // travels (LDS, exchange planes) is (1-m) G, the history planes receive G itself.  d0 is G_T = dL/dout.
    // MODE 4: the same reverse sweep with the transposed taps REBUILT from the raw guidance and the published normaliser instead
    // of gathered from a tap volume:  w_{7-j}[p + off_j] = |g_j[p]| / S[p + off_j]  — the guidance channel j at the quad itself
    // (no shifted gather at all), times the forward's refined reciprocal of S at the 3 x 3 neighbours (NQ + 2 aligned row quads
    // of ONE plane per thread, neighbours by DPP, strip ends by scalars).  The training forward then publishes S only: the
    // 53 MB volume of config 2 is neither written nor read (the tail rebuilds its w_j the same way, cspn_backward.hip).
    // LEAN: the 768-thread instances (CLEAN by construction, the flagship's) run the derive with host-made reciprocals in place of their
    // prologue divisions, without the selects a CLEAN launch cannot need, with one pixel offset per thread and with ONE cold division
    // block per quad (div8_quad_shared_reciprocal).  Same bits.  The 512- / 1024-thread instances keep their code: the NQ = 5 ones are
    // register-tuned to the last scratch slot, and this form cost them 6-17 more spilled VGPRs (8 x 352 x 1216: +1.4 us, sparse +3.5 us).
    constexpr bool LEAN = NTHREADS == RES_THREADS_CLIPPED;
    static_assert(!LEAN || CLEAN, "the clipped instances are CLEAN only");
    constexpr bool SCORE = MODE == 1, TRANSG = MODE == 4, TRANS = MODE == 3 || TRANSG, HIST = MODE == 2 || TRANS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int wg_bad;

    const int tid = threadIdx.x;
    const int tiles_per_img = a.tiles_x * a.tiles_y;
    // A launch may hold several ROUNDS of nb images (RES_ROUNDS_PER_LAUNCH; the host launches one round at a time): rounds x (nb x tiles)
    // workgroups, round 0's — images b0 .. b0 + nb - 1, at most one workgroup per CU — resident at once, those of round r + 1 dispatched
    // in blockIdx order as round r's finish.  Flags and exchange planes are per image, so the rounds share nothing.  (cspnk_resident's
    // reverse sweep runs that way: cspnk_resident.hip.)
    const int wg_round = a.nb * tiles_per_img;
    const int round = LEAN ? res_div((int)blockIdx.x, a.mg_round) : (int)blockIdx.x / wg_round;
    const int tile = xcd_contiguous_id((int)blockIdx.x - round * wg_round, wg_round);
    const int bl = LEAN ? res_div(tile, a.mg_tpi) : tile / tiles_per_img;                 // image within this round
    const int trem = tile - bl * tiles_per_img;
    const int ty = LEAN ? res_div(trem, a.mg_tiles_x) : trem / a.tiles_x;
    const int tx = trem - ty * a.tiles_x;
    const int b = a.b0 + round * a.nb + bl;
    const int H = a.H, W = a.W;
    constexpr bool UNEVEN = NTHREADS == RES_THREADS_CLIPPED;             // only the clipped plans have uneven tile rows
    const int y0 = res_row_y0<UNEVEN>(ty, a.th0, a.th), x0 = tx * a.tw;
    const int th_t = res_row_h<UNEVEN>(ty, a.tiles_y, a.th0, a.th, a.thl);      // this tile row's height
    const size_t HW = (size_t)H * W;
    const size_t plane = (size_t)a.B * HW;
    if (tid == 0) wg_bad = 0;
    int n_stamp = 0;
    auto stamp = [&]() { if (a.dbg && tid == 0 && round == 0 && n_stamp < 16) a.dbg[(size_t)blockIdx.x * 16 + n_stamp++] = wall_clock64(); };   // (round 0's workgroups: [nb x tiles][16])
    stamp();
    // Completion word: every workgroup counts itself out (status word 2); the last one re-arms the counter for the next
    // launch — launches on a workspace never overlap — and, in the last launch of a call, stores `seq` to the second host
    // word.  A host that polls that word (no HIP call, no event on the stream) knows the call has finished and that
    // host_err[0] is final: a workgroup that gave up stored the error, fenced at system scope, and only then counted out.
    // Only the training-form launches (MODE 2 / 3) report: their reader is the end-of-backward check, inference results are
    // checked where the host synchronises anyway.  (Same-box A/B at config 2: the returning atomic at the end of every
    // workgroup costs the inference launch 0.6 us; counting out at the start of the last phase instead — a tile that waits
    // for nobody any more cannot time out — costs 1.3 us, the atomic then sits in the register-bound loop nest.)
    auto count_out = [&]() {
        if (HIST && tid == 0) {
            const unsigned old = __hip_atomic_fetch_add(a.status + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old + 1u == gridDim.x) {
                __hip_atomic_store(a.status + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (a.host_err && a.last_chunk) __hip_atomic_store(a.host_err + 1, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    };

    if (b >= a.B) { count_out(); return; }               // the last round of a ragged batch has fewer images

    const float* __restrict__ din0 = uniform_ptr(a.d0 + (size_t)b * HW);
    const float* __restrict__ spg = BLEND ? uniform_ptr(a.sparse + (size_t)b * HW) : nullptr;

    // ---- ownership: strip (sx, sy) = NQ vertically consecutive quads of the weight region (tile + halo) -------------
    const int wq = a.wq, wr = a.wr;
    const int sy = LEAN ? res_div(tid, a.mg_wq) : tid / wq;
    const int sx = tid - sy * wq;
    const int r0 = sy * NQ;
    // Region origin: the tile's halo is laid out around it, but SHIFTED back into the image at image edges (a region that
    // would stick out on one side extends further on the other instead).  With W >= 4 wq and H >= wr every owned quad then
    // lies inside the image: no zero-padding selects in the step loop, no wasted halo, equal work for edge and inner tiles.
    // The shift never moves a region start before the previous tile's start, so that the halo always comes from the 8
    // ADJACENT tiles (the ones the exchange waits for) — a last tile cut short by the image edge keeps some out-of-image
    // rows / columns instead, and its wavefronts run the step body with the zero-padding selects.
    // (the "previous tile's start" bound belongs to the exchange: a single-phase launch stages everything from the coarse
    // depth, and its halo may be deeper than a tile — there the bound would cut the region short of y0 - hyw)
    const bool exch = a.T > a.S;
    const int rx0 = res_region_x0(tx, a.tw, a.hxw, wq, W, exch);
    const int ry0 = res_region_y0<UNEVEN>(ty, a.th0, a.th, a.hyw, wr, H, exch);
    const int xq = rx0 + 4 * sx;
    const int yq0 = ry0 + r0;
    const bool x_in = (xq >= 0) && (xq < a.Wv);
    const int nval = a.Wv - xq;
    const int lane = tid & 63;
    const bool fix_left = (sx == 0) || (lane == 0);
    const bool fix_right = (sx == wq - 1) || (lane == 63);

    // ---- 0. the coarse-depth region of phase 0 is requested FIRST: loads return in order, so it lands in LDS while the
    //         (8x larger) guidance stream below is still in flight, and the staging costs no round trip of its own
    const int dr = a.dr, ls = a.ls;
    float* const cur = lds;                    // buffer 0: where every phase starts (phases have an even number of steps)
    float* const nxt = lds + RES_PP;
    const int yd0 = ry0 - R;                   // image y of depth-region row 0
    const int xd0 = rx0 - 4;                   // image x of LDS column 0
    float4 st0[NQ + 1];                        // dr * wq <= (NQ + 1) * NTHREADS quads
    unsigned st0_in = 0;
    // quad u * NTHREADS + tid of the region, row-major: (row, qx) advances by a uniform (NTHREADS / wq, NTHREADS % wq) per
    // u — no per-quad division, whose temporaries the register-bound derive cannot afford
    const int step_r = LEAN ? a.step_r : NTHREADS / wq, step_q = LEAN ? a.step_q : NTHREADS - step_r * wq;
    {
    int row = sy, qx = sx;
    // ... LEAN: and no per-quad multiply either, the pixel offset advances with (row, qx)
    int soff = (yd0 + sy) * W + xd0 + 4 + 4 * sx;
    const int soff_step = step_r * W + 4 * step_q, soff_wrap = W - 4 * wq;
#pragma unroll
    for (int u = 0; u <= NQ; ++u) {
        const int y = yd0 + row, x = xd0 + 4 + 4 * qx;
        const bool valid = row < dr;
        const bool in = valid && (y >= 0 && y < H && x >= 0 && x < a.Wv);
        if (in) st0_in |= 1u << u;
        st0[u] = ld4(at32(din0, in ? (unsigned)(LEAN ? soff : y * W + x) : 0u));
        if (TRANS && BLEND) {                          // PREMASK: the sweep starts from (1-m) G_T
            const float4 sp = ld4(at32(spg, in ? (unsigned)(y * W + x) : 0u));
            st0[u].x *= 1.f - sgnf(sp.x); st0[u].y *= 1.f - sgnf(sp.y); st0[u].z *= 1.f - sgnf(sp.z); st0[u].w *= 1.f - sgnf(sp.w);
        }
        row += step_r; qx += step_q; soff += soff_step;
        if (qx >= wq) { qx -= wq; ++row; soff += soff_wrap; }
    }
    }
    float ring0 = 0.f;
    bool ring0_in = false;
    if (tid < dr * 2 * R) {
        const int row = tid / (2 * R), c = tid - row * (2 * R);
        const int lc = (c < R) ? (4 - R + c) : (4 + 4 * wq + (c - R));
        const int y = yd0 + row, x = xd0 + lc;
        ring0_in = (y >= 0 && y < H && x >= 0 && x < a.Wv);
        ring0 = ld1(at32(din0, ring0_in ? (unsigned)(y * W + x) : 0u));
        if (TRANS && BLEND) ring0 *= 1.f - sgnf(ld1(at32(spg, ring0_in ? (unsigned)(y * W + x) : 0u)));
    }

    // ---- 1. weights of the owned quads, derived once from the raw guidance (CSPN_new.py:29-70, :124-127) -------------
    float wreg[NQ][NT][4];
    unsigned in_img = 0, interior = 0;
    // private slots: m * d0 of the owned quads, NQ consecutive 16-byte slots per THREAD — quad i is base + an immediate offset, so
    // the step loop carries no address arithmetic for them (indexed by region row and column they cost the blended training
    // instances 6-7 scratch reloads per step: +25 us per launch); stride NQ * 16 bytes is bank-conflict free for NQ = 1, 3, 5
    float* const md_lds = lds + RES_PP + (size_t)a.dr * a.ls;
    const float* __restrict__ gq = uniform_ptr(a.g + (size_t)b * a.g_bs);
    // tap j = (dy,dx) row-major without the centre reads channel 7-j at p+off_j: the aligned quad of row y+dy gives three of
    // the four shifted values, the fourth is the neighbouring lane's quad (DPP) or, at strip ends / wave edges, a scalar.
    // All loads are branch-free (safe address + select: a conditional load becomes its own basic block with its own wait)
    // and are requested for every owned quad before the arithmetic starts.
    // (32-bit element offsets from the image's guidance base: the loads take the SGPR-base + VGPR-offset form and cost no
    // 64-bit address arithmetic; the host refuses guidance images of >= 2^30 elements.  Loads return in order, so quad i's
    // scalars are requested right behind quad i's planes and the arithmetic below can start on quad 0 while quads 1.. stream.)
    float edge[NQ][6];                     // [0..2]: column xq-1 of the dx<0 taps (j = 0,3,5); [3..5]: column xq+4 of the dx>0 taps (j = 2,4,7)
    const unsigned ucs = (unsigned)a.g_cs;
    // LEAN: one pixel offset per thread (the quad of row yq0) and uniform multiples of W from there; the channel sits in the (scalar)
    // base of the load, not in its offset: no multiply and no addition per load.
    const int o0 = yq0 * W + xq;
    // MODE 4: rows yq0-1 .. yq0+NQ of S, requested in front of the guidance (in-order return: the reciprocals are formed while
    // the guidance streams); [m][0..3] the aligned quad, [m][4] / [m][5] columns xq-1 / xq+4 for the strip-end lanes
    float srow[TRANSG ? NQ + 2 : 1][6];
    if constexpr (TRANSG) {
        const float* __restrict__ sq = uniform_ptr(a.s_in + (size_t)b * HW);
#pragma unroll
        for (int m = 0; m < NQ + 2; ++m) {
            const int ys = yq0 - 1 + m;
            const bool v = x_in && ys >= 0 && ys < H;
            const unsigned o = v ? (unsigned)(ys * W + xq) : 0u;
            const float4 q4 = ld4(at32(sq, o));
            srow[m][0] = q4.x; srow[m][1] = q4.y; srow[m][2] = q4.z; srow[m][3] = q4.w;
            srow[m][4] = ld1(at32(sq, (v && fix_left && xq >= 1) ? o - 1u : 0u));
            srow[m][5] = ld1(at32(sq, (v && fix_right && xq + 4 < a.Wv) ? o + 4u : 0u));
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int r = r0 + i, y = yq0 + i;
        // LEAN (CLEAN): every region lies inside the image and Wv == W, so a row of the region is a row of the image and every owned quad
        // has its four columns: what is left is the rows past the region and, for the dy = +-1 taps, the image's first and last row
        const bool ok = LEAN ? (r < wr) : ((r < wr) && x_in && (y >= 0) && (y < H));
        if (ok) in_img |= 1u << i;
        if (ok && y >= y0 && y < y0 + th_t && xq >= x0 && xq < x0 + a.tw) interior |= 1u << i;
        unsigned orow[3];
        bool rokv[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int row = y + d - 1;
            rokv[d] = ok && row >= 0 && row < H;
            orow[d] = rokv[d] ? (unsigned)(LEAN ? o0 + (i + d - 1) * W : row * W + xq) : 0u;   // outside the image: a safe address of the plane, zeroed below
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int d = (PAC || TRANSG) ? 1 : tap_dy<3>(j) + 1;              // PAC / MODE 4: channel j at the quad itself
            const int ch = (PAC || TRANSG) ? j : 7 - j;
            const float4 v = ld4(LEAN ? at32(gq + (size_t)ch * a.g_cs, orow[d]) : at32(gq, (unsigned)ch * ucs + orow[d]));
            wreg[i][j][0] = rokv[d] ? v.x : 0.f; wreg[i][j][1] = rokv[d] ? v.y : 0.f;
            wreg[i][j][2] = rokv[d] ? v.z : 0.f; wreg[i][j][3] = rokv[d] ? v.w : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) edge[i][t] = 0.f;
        if (!PAC && !TRANSG && (fix_left || fix_right)) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const bool lft = t < 3;
                const int j = lft ? (t == 0 ? 0 : (t == 1 ? 3 : 5)) : (t == 3 ? 2 : (t == 4 ? 4 : 7));
                const int d = tap_dy<3>(j) + 1;
                const int xx = lft ? xq - 1 : xq + 4;
                const bool c = rokv[d] && (lft ? fix_left : fix_right) && xx >= 0 && xx < W;
                // raw value only: consuming it here would make this block wait for the quad's loads (in-order return)
                edge[i][t] = ld1(LEAN ? at32(gq + (size_t)(7 - j) * a.g_cs, c ? orow[d] + (unsigned)(xx - xq) : 0u)
                                      : at32(gq, (unsigned)(7 - j) * ucs + (c ? orow[d] + (unsigned)(xx - xq) : 0u)));
            }
        }
    }
    // park the depth region (its loads were requested before the guidance: only those are waited for here)
    // (the LDS slots are worked out here, from an opaque copy of the thread id: the derive above is register-bound, and a
    // spilled value reloaded in the middle of it waits for every outstanding guidance load)
    int tidk = tid, prow = sy, pqx = sx;
    asm volatile("" : "+v"(tidk), "+v"(prow), "+v"(pqx));
#pragma unroll
    for (int u = 0; u <= NQ; ++u) {
        const bool in = (st0_in >> u) & 1u;
        if (prow < dr)
            *reinterpret_cast<float4*>(&cur[prow * ls + 4 + 4 * pqx]) = make_float4(in ? st0[u].x : 0.f, in ? st0[u].y : 0.f, in ? st0[u].z : 0.f, in ? st0[u].w : 0.f);
        prow += step_r; pqx += step_q;
        if (pqx >= wq) { pqx -= wq; ++prow; }
    }
    if (tidk < dr * 2 * R) {
        const int row = tidk / (2 * R), c = tidk - row * (2 * R);
        const int ring0_at = row * ls + ((c < R) ? (4 - R + c) : (4 + 4 * wq + (c - R)));
        cur[ring0_at] = ring0_in ? ring0 : 0.f; nxt[ring0_at] = 0.f;
    }
    // The ring ROWS of the second buffer are never computed either.  With the regions shifted into the image they ARE the
    // zero padding above / below the image for edge tiles, so they must read as exactly 0 in both buffers (LDS keeps
    // whatever the previous kernel left there).
    for (int c = tidk; c < 2 * ls; c += NTHREADS) nxt[(c < ls ? 0 : (dr - 1) * ls - ls) + c] = 0.f;
    // sparse blend: the masks of the owned quads are requested now, behind the guidance (loads return in order: they are
    // there when the last quad's weights are), into the registers the parked depth quads just left
    float4 mraw[BLEND ? NQ : 1];
    if (BLEND) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const bool ok = (in_img >> i) & 1u;
            mraw[i] = ld4(at32(spg, ok ? (unsigned)((yq0 + i) * W + xq) : 0u));
        }
    }
    if constexpr (TRANSG) {
        // 1 / S by the forward's recipe (div8_shared_reciprocal), 0 where the neighbour lies outside the (valid) image: in place,
        // columns xq-1 .. xq+4 of every row end up as srow[m][4], [0..3], [5]
#pragma unroll
        for (int m = 0; m < NQ + 2; ++m) {
            const int ys = yq0 - 1 + m;
            const bool v = x_in && ys >= 0 && ys < H;
#pragma unroll
            for (int e = 0; e < 4; ++e) srow[m][e] = (v && e < nval) ? reciprocal_as_forward(srow[m][e]) : 0.f;
            const float nl = dpp_from_prev_lane(srow[m][3]), nr = dpp_from_next_lane(srow[m][0]);
            srow[m][4] = fix_left ? ((v && xq >= 1) ? reciprocal_as_forward(srow[m][4]) : 0.f) : nl;
            srow[m][5] = fix_right ? ((v && xq + 4 < a.Wv) ? reciprocal_as_forward(srow[m][5]) : 0.f) : nr;
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const bool ok = (in_img >> i) & 1u;
        if constexpr (TRANSG) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int m = i + tap_dy<3>(j) + 1, dx = tap_dx<3>(j);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = e + dx;
                    const float rs = c < 0 ? srow[m][4] : (c > 3 ? srow[m][5] : srow[m][c]);
                    wreg[i][j][e] = (ok && e < nval) ? fabsf(wreg[i][j][e]) * rs : 0.f;
                }
            }
            continue;
        }
        // does edge[i][t] hold a pixel inside the image?  (recomputed: a bit mask built while the loads are issued is one
        // more live register there)
        auto edge_in = [&](int j, bool lft) -> bool {
            const int lin = j < 4 ? j : j + 1;        // (tap_dy<3>(j), spelled out: a call inside this lambda changes the kernel's code)
            const int row = yq0 + i + lin / 3 - 1;
            return ok && row >= 0 && row < H && (lft ? xq - 1 >= 0 : xq + 4 < W);
        };
        const unsigned off = ok ? (unsigned)((yq0 + i) * W + xq) : 0u;
        if constexpr (PAC) {
            // softmax over the 8 channels per pixel: the arithmetic of cspn_pac_prepare_kernel<3, float, float> (maximum,
            // two-piece exponential, sum in channel order, one refined reciprocal), so the taps are those of the prepared volume
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < NT; ++j) mx = fmaxf(mx, wreg[i][j][e]);
                float den = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) { wreg[i][j][e] = softmax_exp<float>(wreg[i][j][e] - mx); den += wreg[i][j][e]; }
                const float inv = reciprocal_refined(den);
#pragma unroll
                for (int j = 0; j < NT; ++j) wreg[i][j][e] = (ok && e < nval) ? softmax_weight<float>(wreg[i][j][e], inv) : 0.f;
            }
            if (MODE == 2 && ((interior >> i) & 1u)) store_taps_quad<NT>(a.w_out + (size_t)b * NT * HW, off, HW, wreg[i]);
            continue;
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int dx = tap_dx<3>(j);
            const float q0 = wreg[i][j][0], q1 = wreg[i][j][1], q2 = wreg[i][j][2], q3 = wreg[i][j][3];
            if (dx < 0) {
                const int t = j == 0 ? 0 : (j == 3 ? 1 : 2);
                const float nb = dpp_from_prev_lane(q3);
                const float lf = fix_left ? (edge_in(j, true) ? edge[i][t] : 0.f) : nb;
                wreg[i][j][0] = TRANS ? lf : fabsf(lf); wreg[i][j][1] = TRANS ? q0 : fabsf(q0); wreg[i][j][2] = TRANS ? q1 : fabsf(q1); wreg[i][j][3] = TRANS ? q2 : fabsf(q2);
            } else if (dx > 0) {
                const int t = j == 2 ? 3 : (j == 4 ? 4 : 5);
                const float nb = dpp_from_next_lane(q0);
                const float rt = fix_right ? (edge_in(j, false) ? edge[i][t] : 0.f) : nb;
                wreg[i][j][0] = TRANS ? q1 : fabsf(q1); wreg[i][j][1] = TRANS ? q2 : fabsf(q2); wreg[i][j][2] = TRANS ? q3 : fabsf(q3); wreg[i][j][3] = TRANS ? rt : fabsf(rt);
            } else {
                wreg[i][j][0] = TRANS ? q0 : fabsf(q0); wreg[i][j][1] = TRANS ? q1 : fabsf(q1); wreg[i][j][2] = TRANS ? q2 : fabsf(q2); wreg[i][j][3] = TRANS ? q3 : fabsf(q3);
            }
        }
        // S in the reference's channel order k = 0..7 (tap 7..0), one shared refined reciprocal; 0 for padding quads
        float Sq[4] = {0.f, 0.f, 0.f, 0.f};
        if (TRANS) {                                   // the taps are final: only quads outside the image are zeroed
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < NT; ++j) wreg[i][j][e] = (ok && e < nval) ? wreg[i][j][e] : 0.f;
        } else if constexpr (LEAN) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float S = wreg[i][7][e];
#pragma unroll
                for (int k = 1; k < 8; ++k) S += wreg[i][7 - k][e];
                Sq[e] = S;
            }
            // a quad is kept or dropped as a whole, and a dropped one holds zero gates (every tap select above has `ok` in it)
            div8_quad_shared_reciprocal(wreg[i], Sq, ok);
        } else
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float S = wreg[i][7][e];
#pragma unroll
            for (int k = 1; k < 8; ++k) S += wreg[i][7 - k][e];
            Sq[e] = S;
            float av[8], qv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = wreg[i][j][e];
            div8_shared_reciprocal(av, S, qv);
#pragma unroll
            for (int j = 0; j < NT; ++j) wreg[i][j][e] = (ok && e < nval) ? qv[j] : 0.f;
        }
        if (MODE == 2 && ((interior >> i) & 1u)) {   // publish before the blend is folded in: the backward wants w and S themselves
            if (a.w_out) store_taps_quad<NT>(a.w_out + (size_t)b * NT * HW, off, HW, wreg[i]);     // null: S only (the backward rebuilds w)
            st4(at32(uniform_ptr(a.s_out + (size_t)b * HW), off), make_float4(Sq[0], Sq[1], Sq[2], Sq[3]));
        }
    }
    // the blend is folded in by a second pass: the masks were requested BEHIND the guidance, so touching the first one
    // waits for the whole stream — after the weight arithmetic, which consumes the stream as it arrives, that wait is free
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const bool ok = (in_img >> i) & 1u;
        // EVERY slot of the thread is written, also those of rows past the region (r0 + i >= wr: m = 0 there).  The step body
        // computes those rows too (zero taps) and a CLEAN instance trusts the result to be exactly 0 — it is the lower neighbour
        // of the region's last row, i.e. the zero padding below the image for a bottom-edge tile — so the blend term it adds must
        // not be whatever the previous kernel on this CU left in LDS (round 5: the root cause of the one-off bit mismatch at
        // KITTI B = 8 with sparse depth, the one production shape with wr % NQ != 0; tests: the poisoned-LDS runs).
        if (BLEND) {
            // (1-m) u + m d0  ==  sum_j ((1-m) w_j) d_j + m d0 with 1-m in {0,1,2}: exact, so bit-identical (CSPN_new.py:90)
            const float4 m = make_float4(ok ? sgnf(mraw[i].x) : 0.f, ok ? sgnf(mraw[i].y) : 0.f, ok ? sgnf(mraw[i].z) : 0.f, ok ? sgnf(mraw[i].w) : 0.f);
            const float omq[4] = {1.f - m.x, 1.f - m.y, 1.f - m.z, 1.f - m.w};
            if (TRANS) {                               // PREMASK: the private plane holds 1-m, applied to every step's result
                *reinterpret_cast<float4*>(md_lds + (tid * NQ + i) * 4) = make_float4(omq[0], omq[1], omq[2], omq[3]);
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) wreg[i][j][e] *= omq[e];
                // the private slot receives m now and becomes m * d0 once the depth region is staged (the owned quads of
                // d0 are read from LDS there anyway: no second global load, no exposed round trip)
                *reinterpret_cast<float4*>(md_lds + (tid * NQ + i) * 4) = m;
            }
        }
    }

    stamp();                                   // weights derived
    // Everything below addresses through LATE, opaque copies of the strip coordinates: row / pixel offsets of the step loop,
    // the staging and the epilogue are then computed here, after the derive — computed early they sit in registers the
    // derive needs, get spilled, and every scratch reload in the derive waits for ALL outstanding guidance loads
    // (s_waitcnt vmcnt(0): loads return in order), which serialises the load stream and the weight arithmetic.
    int r0L = r0, sxL = sx, yq0L = yq0, xqL = xq;
    asm volatile("" : "+v"(r0L), "+v"(sxL), "+v"(yq0L), "+v"(xqL));
    // ---- 2. phases of S steps; between phases the tile borders travel through the exchange planes ---------------------
    const bool active = (r0L < wr);
    const int cb = 4 + 4 * sxL;
    float* __restrict__ dout = HIST ? nullptr : uniform_ptr(a.out + (size_t)b * HW);
    float* hist_step = HIST ? uniform_ptr(a.hist + (size_t)b * HW) : nullptr;      // plane of the step being computed (uniform)
    const int n_phase = (a.T + a.S - 1) / a.S;
    const int tile_global = b * tiles_per_img + trem;
    float own[NQ][4];

    for (int p = 0; p < n_phase; ++p) {
        const int steps = (a.T - p * a.S) < a.S ? (a.T - p * a.S) : a.S;
        const bool last_phase = (p == n_phase - 1);
        // -- stage the depth region (weight region + 1 ring).  Phase 0: everything from the coarse depth.  Later phases:
        //    the tile's own interior is already in LDS (`cur`), only the halo comes from the neighbours' published borders
        const float* __restrict__ xin = uniform_ptr(a.xbuf + (size_t)((p + 1) & 1) * plane + (size_t)b * HW);   // written in phase p-1
        if (p > 0) {
            // halo quads only: the full rows above and below the tile rows, the quads left and right of the tile columns.  All
            // device-scope loads of a batch are requested before the first one is consumed (branch-free: safe address + select).
            int tidp = tid;                                    // opaque copy: the per-thread halo addressing below is recomputed
            asm volatile("" : "+v"(tidp));                     // every phase instead of living (spilled) across the step loop
            const int tq_in = min(a.tw, rx0 + 4 * wq - x0) >> 2;   // tile columns / rows that lie inside the region (the last
            const int th_in = min(th_t, ry0 + wr - y0);            // tile of an image may be cut short by the image edge)
            const int nl = (x0 - rx0) >> 2;                    // quads left of the tile columns inside the region
            const int nside = wq - tq_in;                      // ... left + right
            const int nrow_t = (y0 - ry0) + R;                 // depth-region rows above the tile rows (ring row included)
            const int n_top = nrow_t * wq;
            const int n_bot = (dr - nrow_t - th_in) * wq;
            const int n_side = th_in * nside;
            const int n_halo = n_top + n_bot + n_side;
            // the 1-pixel ring columns left / right of the region: one scalar per row and side
            float ring_v = 0.f;
            int ring_at = -1;
            if (tidp < dr * 2 * R) {
                const int row = tidp / (2 * R), c = tidp - row * (2 * R);
                const int lc = (c < R) ? (4 - R + c) : (4 + 4 * wq + (c - R));
                const int y = yd0 + row, x = xd0 + lc;
                const bool in = (y >= 0 && y < H && x >= 0 && x < a.Wv);
                const float v = ld1_dev(at32(xin, in ? (unsigned)(y * W + x) : 0u));
                ring_v = in ? v : 0.f;
                ring_at = row * ls + lc;
            }
            for (int base = 0; base < n_halo; base += 2 * NTHREADS) {
                float4 hv[2];
                int at[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int h = base + u * NTHREADS + tidp;
                    int row, qx;
                    if (h < n_top) { row = h / wq; qx = h - row * wq; }
                    else if (h < n_top + n_bot) { const int h2 = h - n_top; row = h2 / wq; qx = h2 - row * wq; row += nrow_t + th_in; }
                    else {
                        const int h3 = h - n_top - n_bot;
                        const int ns = nside > 0 ? nside : 1;
                        row = h3 / ns;
                        const int c = h3 - row * ns;
                        row += nrow_t;
                        qx = c < nl ? c : c + tq_in;
                    }
                    const int y = yd0 + row, x = xd0 + 4 + 4 * qx;
                    const bool valid = h < n_halo;
                    const bool in = valid && y >= 0 && y < H && x >= 0 && x < a.Wv;
                    const float4 v = ld4_dev(at32(xin, in ? (unsigned)(y * W + x) : 0u));
                    hv[u] = make_float4(in ? v.x : 0.f, in ? v.y : 0.f, in ? v.z : 0.f, in ? v.w : 0.f);
                    at[u] = valid ? row * ls + 4 + 4 * qx : -1;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (at[u] >= 0) *reinterpret_cast<float4*>(&cur[at[u]]) = hv[u];
            }
            if (ring_at >= 0) { cur[ring_at] = ring_v; nxt[ring_at] = 0.f; }
            for (int c = tidp; c < 2 * ls; c += NTHREADS) nxt[(c < ls ? 0 : (dr - 1) * ls - ls) + c] = 0.f;   // see phase 0
        }
        __syncthreads();

#pragma unroll
        for (int i = 0; i < NQ; ++i) {             // rows past the region read the clamped last row; they are never stored
            int drow = r0L + i + R;
            drow = drow < dr ? drow : dr - 1;
            const v4f mid = *(lds_cv4f_ptr)(cur + drow * ls + cb);
            own[i][0] = mid.x; own[i][1] = mid.y; own[i][2] = mid.z; own[i][3] = mid.w;
        }
        if (BLEND && !TRANS && p == 0) {           // private slots: m -> m * d0 (own = d0 here)
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                if (r0L + i < wr) {
                    float4* slot = reinterpret_cast<float4*>(md_lds + (tid * NQ + i) * 4);
                    const float4 m = *slot;
                    // plain products, as the reference's  m * d0  (0 * inf = nan spreads like there); quads outside the
                    // image hold m = 0 and a zero-padded d0
                    *slot = make_float4(m.x * own[i][0], m.y * own[i][1], m.z * own[i][2], m.w * own[i][3]);
                }
            }
        }
        // One propagation step on the LDS tile.  FINAL (the very last step of the forward) is peeled into its own copy so
        // that the target quads of the fused metrics are only live there, not across the hot loop.
        // PUBLISH (form 2, the 768-thread instances only): the last step of a phase that is not the last one, peeled as well.  It stores
        // every interior row to the exchange plane right behind the row's ds_write, so that the device-scope acknowledge of row 0
        // overlaps the FMAs of rows 1 .. NQ-1, and its closing barrier — behind s_waitcnt vmcnt(0) — IS "everybody's stores have
        // landed": the separate publish pass, its wait and its barrier are gone.  Storing that early is safe by the argument the
        // exchange already makes: a tile is in phase p only after all eight neighbours have flagged phase p - 1, so they have finished
        // reading plane p & 1 (they read it while staging phase p - 1).
        // (The exchange plane comes in as a trailing argument of that form alone: the lambda of the other instances then captures what it
        // always did, and the 512- / 1024-thread instances compile to the code they had.)
        auto step = [&](auto form_c, auto on_c, auto par_c, int final_par, float* xpub = nullptr) __attribute__((always_inline)) {
            constexpr int FORM = (int)decltype(form_c)::value;  // 0 (std::false_type): plain, 1 (std::true_type): FINAL, 2: PUBLISH
            constexpr bool FINAL = FORM == 1, PUBLISH = FORM == 2;
            static_assert(!PUBLISH || (LEAN && !HIST), "the publishing step belongs to the 768-thread inference instances");
            constexpr int PAR = decltype(par_c)::value;       // buffer this step reads (the final step: `final_par`)
            if (decltype(on_c)::value) {
                float win[NQ + 2 * R][WIN];
                const float* const rd = FINAL ? lds + final_par * RES_PP : lds + PAR * RES_PP;
                float* const wrb = lds + (1 - PAR) * RES_PP;
                // the peeled final step runs once: its row / pixel offsets are recomputed from opaque copies instead of being
                // kept (spilled) across the hot loop
                int r0x = r0L, yqx = yq0L;
                if (FINAL) asm volatile("" : "+v"(r0x), "+v"(yqx));
                if (PUBLISH) asm volatile("" : "+v"(yqx));      // (its rows are the hot loop's: only the pixel offset is formed here)
                // ... and ONE pixel offset for its stores: formed per row from the strip coordinates, a spilled coordinate was reloaded from
                // scratch — with a wait for the reload — in front of every row's store (5 x ~0.7 us in the blended scored instance: round 6)
                unsigned o0x = 0u;
                if ((FINAL && !HIST) || PUBLISH) { o0x = (unsigned)(yqx * W + xqL); asm volatile("" : "+v"(o0x)); }
                auto row_ptr = [&](int rr) -> const float* {
                    int drow = r0x + rr;
                    drow = drow < dr ? drow : dr - 1;
                    return rd + drow * ls + cb;
                };
#pragma unroll
                for (int rr = 0; rr < NQ + 2 * R; ++rr) {
                    float m4[4];
                    const bool own_row = rr >= R && rr < R + NQ;
                    if (own_row) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) m4[c] = own[rr - R][c];
                    } else {
                        const v4f mid = *(lds_cv4f_ptr)(row_ptr(rr));
                        m4[0] = mid.x; m4[1] = mid.y; m4[2] = mid.z; m4[3] = mid.w;
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c) win[rr][R + c] = m4[c];
                    win[rr][0] = dpp_from_prev_lane(m4[3]);
                    win[rr][5] = dpp_from_next_lane(m4[0]);
                }
                // strip-end / wave-edge lanes patch their halo column from LDS: exec-masked ds_read straight into the window
                // registers (a merged block with selects costs 28 v_mov per step and measured 7 % slower)
                if (fix_left) {
#pragma unroll
                    for (int rr = 0; rr < NQ + 2 * R; ++rr) win[rr][0] = row_ptr(rr)[-1];
                }
                if (fix_right) {
#pragma unroll
                    for (int rr = 0; rr < NQ + 2 * R; ++rr) win[rr][5] = row_ptr(rr)[4];
                }
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
                    // rows past the region (r0L + i >= wr, only in the last row group) are computed too — their taps are
                    // zero — and only their LDS store is masked: a branch around the arithmetic costs exec-masked copies of
                    // the carried quads on every step
                    {
                        float u[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                            for (int dx = -1; dx <= 1; ++dx) {
                                if (dy == 0 && dx == 0) continue;
                                const int lin = (dy + 1) * 3 + (dx + 1);
                                const int j = lin < 4 ? lin : lin - 1;
#pragma unroll
                                for (int e = 0; e < 4; ++e) u[e] = fmaf(wreg[i][j][e], win[i + dy + 1][e + dx + 1], u[e]);
                            }
                        float keep[4];                 // the state carried to the next step
                        if (BLEND) {
                            const float4 m4 = *reinterpret_cast<const float4*>(md_lds + (tid * NQ + i) * 4);
                            if (TRANS) {
                                keep[0] = m4.x * u[0]; keep[1] = m4.y * u[1]; keep[2] = m4.z * u[2]; keep[3] = m4.w * u[3];
                            } else {
                                u[0] += m4.x; u[1] += m4.y; u[2] += m4.z; u[3] += m4.w;
                            }
                        }
                        if (!(TRANS && BLEND)) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) keep[e] = u[e];
                        }
                        if (!CLEAN) {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (!((in_img >> i) & 1u) || e >= nval) { u[e] = 0.f; keep[e] = 0.f; }   // zero padding stays exactly zero
                        }
                        if (!FINAL && r0L + i < wr)
                            *reinterpret_cast<float4*>(&wrb[(r0L + i + R) * ls + cb]) = make_float4(keep[0], keep[1], keep[2], keep[3]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) own[i][e] = keep[e];
                        if (HIST) {
                            if ((interior >> i) & 1u) st4_hist(at32(hist_step, (unsigned)((yq0L + i) * W + xqL)), make_float4(u[0], u[1], u[2], u[3]));
                        } else if (FINAL && ((interior >> i) & 1u)) {
                            st4(at32(dout, o0x + (unsigned)(i * W)), make_float4(u[0], u[1], u[2], u[3]));
                        }
                        if constexpr (PUBLISH) {
                            if ((interior >> i) & 1u) st4_dev(xpub, o0x + (unsigned)(i * W), keep[0], keep[1], keep[2], keep[3]);
                        }
                    }
                }
            }
            if (HIST) hist_step += plane;
            // PUBLISH: this thread's device-scope stores have landed before it arrives, so behind the barrier everybody's have
            if (PUBLISH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (!FINAL) __syncthreads();
        };
        stamp();                               // depth staged
        // (768 threads: a phase that is not the last one ends in the peeled publishing step.  Such a phase has an even number of steps, so
        // that step always reads buffer 1: pairs, one single step, then the peeled one)
        const int plain_steps = (LEAN || last_phase) ? steps - 1 : steps;
        // Wavefronts without a single owned row (the tail of the last row group) only keep the barriers company.  The test is
        // wave-uniform (a scalar branch), and the step loop sits INSIDE it: a per-step `if (active)` makes every carried quad
        // a phi of "old" and "new" that is resolved with 20 v_mov per step.  Idle lanes of a working wavefront run the
        // arithmetic on clamped rows with zero taps; only their stores are masked.  Two steps per trip let the carried
        // quads alternate between two register sets.
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        using PublishStep = std::integral_constant<int, 2>;
        if (__ballot(active) != 0ull) {
            int s = 0;
            for (; s + 1 < plain_steps; s += 2) {
                step(std::false_type{}, std::true_type{}, P0{}, 0);
                step(std::false_type{}, std::true_type{}, P1{}, 0);
            }
            if (s < plain_steps) step(std::false_type{}, std::true_type{}, P0{}, 0);
            if (last_phase) step(std::true_type{}, std::true_type{}, P0{}, plain_steps & 1);
            if constexpr (LEAN) {
                if (!last_phase) step(PublishStep{}, std::true_type{}, P1{}, 0, uniform_ptr(a.xbuf + (size_t)(p & 1) * plane + (size_t)b * HW));
            }
        } else {
            for (int s = 0; s < plain_steps; ++s) step(std::false_type{}, std::false_type{}, P0{}, 0);
            if (last_phase) step(std::true_type{}, std::false_type{}, P0{}, 0);
            if constexpr (LEAN) { if (!last_phase) step(PublishStep{}, std::false_type{}, P1{}, 0); }
        }
        stamp();                               // steps of the phase done
        if (!last_phase) {
            // -- publish the interior quads (device scope), then the phase flag; wait for the 8 neighbouring tiles
            if constexpr (!LEAN) {                 // (768 threads: published inside the phase's last step, see `step`)
            float* __restrict__ xout = uniform_ptr(a.xbuf + (size_t)(p & 1) * plane + (size_t)b * HW);
            if (active) {
                // (opaque to the optimiser: the per-quad offsets are recomputed here, not hoisted out of the phase loop into
                // registers the step loop needs — they would be spilled and reloaded from scratch every phase)
                unsigned o0 = (unsigned)(yq0L * W + xqL);
                asm volatile("" : "+v"(o0));
                // Every interior quad is published.  tools/probes/res_publish_borders_only.patch (round 5 experiment): only what a neighbour
                // will READ is published — the columns / rows of this
                // tile that lie inside an adjacent tile's depth region (its weight region + the 1-pixel ring), worked out from the
                // neighbours' region origins exactly as they work them out themselves.  Corner neighbours read the intersection of
                // a column band and a row band, so the union of the four bands covers all eight.  At config 2 that is 57 % of the
                // interior quads: fewer device-scope stores to wait for before the flag, 6 MB less write traffic per forward — but
                // NOT faster (same-box A/B, profiles/r05_publish_ab.txt: 48.0 vs 47.8 us, sparse 53.9 vs 53.1).
#pragma unroll
                for (int i = 0; i < NQ; ++i) {
                    if ((interior >> i) & 1u) st4_dev(xout, o0 + (unsigned)(i * W), own[i][0], own[i][1], own[i][2], own[i][3]);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this thread's device-scope stores have landed
            __syncthreads();                                       // ... and so have everybody else's in the workgroup
            }
            const unsigned want = a.seq + (unsigned)p + 1u;
            if (tid == 0) __hip_atomic_store(a.flags + tile_global, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tid < 9 && tid != 4) {
                const int ny = ty + tid / 3 - 1, nx = tx + tid % 3 - 1;
                if (ny >= 0 && ny < a.tiles_y && nx >= 0 && nx < a.tiles_x) {
                    // (SGPR base + a 32-bit VGPR offset: as a 64-bit per-thread pointer the flag address was spilled in the blended instances and
                    //  re-loaded from scratch — with a wait — in front of EVERY poll)
                    const gptr f = (gptr) reinterpret_cast<unsigned long long>(uniform_ptr(a.flags)) + ((unsigned)(b * tiles_per_img + ny * a.tiles_x + nx) << 2);
                    unsigned spins = 0;
                    while ((int)(__hip_atomic_load(reinterpret_cast<const GLB unsigned*>(f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
                        ++spins;
                        if ((spins & 255u) == 0u && __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == a.seq) {
                            wg_bad = 1;
                            break;
                        }
                        if (spins >= a.spin_limit) {                // a neighbour never became resident / finished: give up
                            __hip_atomic_store(a.status, a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            wg_bad = 1;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                }
            }
            __syncthreads();
            stamp();                           // neighbours' borders published
            if (wg_bad) {
                if (tid == 0) {
                    __hip_atomic_store(a.status + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (a.host_err) __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __atomic_thread_fence(__ATOMIC_SEQ_CST);       // the error is visible to the host before this tile counts out
                }
                // Poison what this tile will never produce: its part of the refined depth (or of the last history plane —
                // d_T in the training forward, G_0 in the reverse sweep) becomes NaN, so that a result consumed before the
                // host has looked at the error word is visibly wrong instead of stale allocator memory.
                {
                    const float qnan = __uint_as_float(CSPN_POISON_F32);      // NaN with the payload the host looks for
                    float* const pz = HIST ? uniform_ptr(a.hist + (size_t)(a.T - 1) * plane + (size_t)b * HW) : dout;
                    unsigned o0 = (unsigned)(yq0L * W + xqL);
                    asm volatile("" : "+v"(o0));
#pragma unroll
                    for (int i = 0; i < NQ; ++i)
                        if ((interior >> i) & 1u) st4(at32(pz, o0 + (unsigned)(i * W)), make_float4(qnan, qnan, qnan, qnan));
                }
                count_out();
                return;
            }
        }
    }
    if (SCORE) {
        float mf[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) mf[k] = 0.f;
        if (active) {
            // the target quads are requested only now: the weight registers are dead, nothing spills, and the one exposed
            // round trip costs less than carrying NQ quads through the final step did.  (Requested inside the peeled final step of the
            // 768-thread instances, behind row 0 — 32 dead tap registers there — they do not stay inside that copy: the compiler carries
            // the 12 registers around the phase loop whichever way the loop is left, 43-52 spilled VGPRs against 1: NEGATIVE_RESULTS #62.)
            float4 scored_t[NQ];
            const float* tgt_b = uniform_ptr(a.target + (size_t)b * HW);
            unsigned o0s = (unsigned)(yq0L * W + xqL);       // one offset for all rows (see the final step's stores)
            asm volatile("" : "+v"(o0s));
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const bool in = (interior >> i) & 1u;
                scored_t[i] = ld4(at32(tgt_b, in ? o0s + (unsigned)(i * W) : 0u));
            }
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                if ((interior >> i) & 1u) {
                    const float4 tg = scored_t[i];
                    const float t4[4] = {tg.x, tg.y, tg.z, tg.w};
                    const float o4[4] = {own[i][0], own[i][1], own[i][2], own[i][3]};
#pragma unroll
                    for (int e = 0; e < 4; ++e) metric_terms(o4[e], t4[e], mf);
                }
            }
        }
        if constexpr (LEAN) stamp();           // target there (thread 0 has consumed its quads)
        float* part = lds + RES_PP + (size_t)a.dr * a.ls + (size_t)(BLEND ? 1 : 0) * NTHREADS * NQ * 4;
        const int wave = tid >> 6;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const float v = wave_sum_to_lane63(mf[k]);
            if (lane == 63) part[wave * 10 + k] = v;
        }
        __syncthreads();
        if (tid < 10) {
            double v = 0.0;
            for (int w = 0; w < NTHREADS / 64; ++w) v += (double)part[w * 10 + tid];
            if (v != 0.0) atomicAdd(a.macc + (size_t)(blockIdx.x % a.nslots) * 10 + tid, v);
        }
        if constexpr (LEAN) {
            if (a.dbg) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the probe only: the stamp below is taken when the additions are acknowledged)
            stamp();                           // sums added
        }
    }
    count_out();
}

// ------------------------------------------------------------------------------------------------ host side
constexpr int RES_MAX_NQ = 5;

// Rounds of images_per_launch images in one launch: the kernel takes any number (the A/B ran 8), the host loop launches one.  Measured, NOT the default (same box, three alternating passes, profiles/r05_rounds_ab.txt): KITTI B = 8 (2 rounds of
// 4 images on 256 workgroups) 92.4-93.4 us per scored forward against 92.2-93.7 with one launch per round, NYU B = 48 91.7-92.1 against
// 90.4-90.9 (slower), only a ragged third round gains (KITTI B = 9: 121-123 against 126-127).  A round-1 workgroup starts when a CU is freed,
// but its neighbours start as scattered as round 0's workgroups finish: the neighbour waits pay what the drain and the launch gap cost.
// The K = 5 reverse sweep (cspnk_resident.hip) does gain (2 x 45.7 + gap -> 88.5 us) and runs its rounds in one launch.
constexpr int RES_ROUNDS_PER_LAUNCH = 1;
struct ResGeom {
    int S, tiles_x, tiles_y, tw, th, nq, wq, wr, hxw, hyw, dr, ls;
    int imgs_per_launch, launches;
    size_t lds_bytes;
    double cost;
    int threads = RES_THREADS;      // 512, or 1024 with one quad per thread (four wavefronts per SIMD: small shards, round 5),
                                    // or 768 with three quads per thread on clipped regions (three wavefronts per SIMD)
    int th0 = 0, thl = 0;           // first / last tile row (res_row_h); set_uniform_rows() for the plans whose rows are all th high
};
void set_uniform_rows(ResGeom* g) { g->th0 = g->thl = g->th; }

int cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    int n = cached[dev & 63].load(std::memory_order_relaxed);
    if (n > 0) return n;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    cached[dev & 63].store(prop.multiProcessorCount, std::memory_order_relaxed);
    return prop.multiProcessorCount;
}

// LDS of one workgroup: buffer 0 in the first RES_PP floats, buffer 1 behind it, then the private m * d0 quads (sparse
// blend) and the 10 x 16 partial sums of the fused metrics.
size_t res_lds_bytes(int dr, int ls, int nq, int blend, int threads = RES_THREADS) {
    return ((size_t)RES_PP + (size_t)dr * ls + (size_t)(blend ? 1 : 0) * threads * nq * 4 + 16 * 10) * sizeof(float);
}

// Row stride (floats) of a depth buffer in LDS: 4 wq + 8 at least ([4 pad incl. ring][wq quads][ring + pad]).  Round 5 (against
// the plain 4 wq + 8; same-box, profiles/r05_swizzle_ab.txt: NYU B = 3 20.8 -> 20.1 us per scored forward, the other shapes within noise): the smallest such stride for which the next strip of a thread column (NQ rows further down) continues the bank
// sequence of this one inside a wavefront — NQ ls = 4 wq (mod 64 dwords) — so that the 16 lanes of a ds_read_b128 / ds_write_b128
// pass that straddle two strips do not share banks (SQ counters of round 4: 16.5 % of the LDS cycles were bank conflicts).
int res_row_stride(int wq, int nq, int dr) {
    const int lo = 4 * wq + 8;
    for (int cand = lo; cand < lo + 64; cand += 4)
        if ((((nq * cand - 4 * wq) % 64) + 64) % 64 == 0 && (size_t)dr * cand <= (size_t)RES_PP) return cand;
    return lo;
}

// Does every region of every tile lie inside the (valid part of the) image?  (The kernel's own region placement: res_region_x0 / _y0.)
bool regions_inside_image(const ResGeom& g, int H, int W, int Wv, int T) {
    if (Wv != W) return false;
    const bool exch = T > g.S;            // see the region origin in the kernel
    for (int tx = 0; tx < g.tiles_x; ++tx) {
        const int rx0 = res_region_x0(tx, g.tw, g.hxw, g.wq, W, exch);
        if (rx0 < 0 || rx0 + 4 * g.wq > W) return false;
    }
    for (int ty = 0; ty < g.tiles_y; ++ty) {
        const int ry0 = res_region_y0(ty, g.th0, g.th, g.hyw, g.wr, H, exch);
        if (ry0 < 0 || ry0 + g.wr > H) return false;
    }
    return true;
}

// The clipped geometry of the 768-thread instance.  The region is as large as a tile really needs: per axis the largest extent of
// (tile +- halo) cut to the image.  A tile at an image edge needs its halo on one side only, so with two tile columns the region is
// tw + hxw wide instead of tw + 2 hxw, and the first and the last tile ROW are made taller than the rows in between (th0 = wr - hyw
// against th = wr - 2 hyw; the last row takes the rest of the image, at most th0), so that every row's region is wr high.  With three
// or more columns the inner tiles keep their two-sided halo: wq is then what the 512-thread plans use.  Every thread owns a strip of
// 3 quads: ceil(wr / 3) wq <= 768.  Fills *g for `tiles_x` x `tiles_y` tiles of width tw with a first row of th0 (tiles_y == 1: the
// whole image); false when that is no valid clipped tiling: rows that do not cover the image, a halo reaching past the adjacent
// tile, a region outside the image, or more than the instance / LDS holds.
bool clipped_geometry(int H, int W, int T, int Se, int tiles_x, int tiles_y, int tw, int th0, int blend, ResGeom* g) {
    if (tiles_x < 1 || tiles_y < 1 || tw < 4 || (tw & 3) || th0 < 1 || Se < 1) return false;
    const int hyw = Se - 1, hxw = round_up4(Se - 1), phases = ceil_div(T, Se);
    if (phases > 1 && (Se & 1)) return false;
    if (tiles_x * tw < W || (tiles_x - 1) * tw >= W) return false;
    if (phases > 1 && tiles_x > 1 && tw < 2 * hxw) return false;
    int th = th0, thl = th0, wr = H;
    if (tiles_y == 1) {
        if (th0 < H) return false;
        th = thl = th0 = H;
    } else {
        wr = th0 + hyw;
        th = wr - 2 * hyw;
        thl = H - th0 - (tiles_y - 2) * th;
        if (th < 1 || thl < 1 || thl > th0) return false;
        if (phases > 1 && (th0 < 2 * hyw || (tiles_y > 2 && th < 2 * hyw) || thl < hyw)) return false;
    }
    int wx = 0;                            // widest (tile +- halo) within the image
    for (int tx = 0; tx < tiles_x; ++tx) {
        const int lo = tx * tw - hxw > 0 ? tx * tw - hxw : 0, hi = (tx + 1) * tw + hxw < W ? (tx + 1) * tw + hxw : W;
        if (hi - lo > wx) wx = hi - lo;
    }
    const int wq = wx / 4;
    if (wq < 1 || ceil_div(wr, 3) * wq > RES_THREADS_CLIPPED) return false;
    const int dr = wr + 2, ls = res_row_stride(wq, 3, dr);
    if ((size_t)dr * ls > (size_t)RES_PP) return false;
    const size_t ldsb = res_lds_bytes(dr, ls, 3, blend, RES_THREADS_CLIPPED);
    if (ldsb > 160 * 1024) return false;
    *g = ResGeom{Se, tiles_x, tiles_y, tw, th, 3, wq, wr, hxw, hyw, dr, ls, 0, 0, ldsb, 0.0};
    g->threads = RES_THREADS_CLIPPED; g->th0 = th0; g->thl = thl;
    return regions_inside_image(*g, H, W, W, T);          // the instance is CLEAN only
}

// The search over clipped tilings (threads = 768): same phase lengths and tile widths as resident_geometry, the smallest region
// height that covers the image with `ty` rows.
bool resident_geometry_clipped(int B, int H, int W, int T, int blend, int ncu, int S_user, ResGeom* best) {
    if (W % 4 != 0 || ncu < 1 || T < 1) return false;
    bool found = false;
    for (int S = (S_user > 0 ? S_user : 12); S >= (S_user > 0 ? S_user : 4); S -= (S > 8 ? 4 : 2)) {
        const int Se = S > T ? T : S;
        const int hyw = Se - 1, phases = ceil_div(T, Se);
        for (int tx = 1; tx <= 32; ++tx) {
            const int tw = round_up4(ceil_div(W, tx));
            if (tx > 1 && (tw < 16 || ceil_div(W, tw) != tx)) continue;
            for (int ty = 1; ty <= 64 && tx * ty <= ncu; ++ty) {
                const int wr = ty == 1 ? H : ceil_div(H + 2 * hyw * (ty - 1), ty);
                ResGeom cand;
                if (!clipped_geometry(H, W, T, Se, tx, ty, tw, ty == 1 ? H : wr - hyw, blend, &cand)) continue;
                int ipl = ncu / (tx * ty);
                if (ipl > B) ipl = B;
                cand.imgs_per_launch = ipl; cand.launches = ceil_div(B, ipl);
                // the 512-thread model with the quads a thread really holds (its strips are 3 quads, the region's rows rarely fill the
                // last one) and three wavefronts per SIMD; fitted at config 2 (profiles/r07_clipped_ab.txt)
                const double q = (double)cand.wq * cand.wr / 256.0 / 3.0;
                cand.cost = cand.launches * (8.0 + 2.0 * q + T * (0.13 * q + 0.1) + (phases - 1) * (3.0 + 0.6 * q));
                if (!found || cand.cost < best->cost) { found = true; *best = cand; }
            }
        }
    }
    return found;
}

// The geometry of `tiles_x` x `tiles_y` tiles of tw x th pixels with uniform rows, on 512 threads (up to RES_MAX_NQ quads per thread) or
// 1024 (one quad per thread: 128 VGPRs hold one quad's weights): fills the dependent fields of *g (not imgs_per_launch / launches /
// cost); false when that is no valid tiling.  The one statement of the feasibility rules: the search calls it per candidate, the
// launch with the tiling of a plan.  (The two used to carry a copy each.  They agreed except that the plan's copy also asked for
// tw % 4 == 0 and for tiles that cover the image — both hold for every candidate the search forms, so asking here changes neither
// the plans the search returns nor the plans the launch accepts.)
bool rgeom_fill(int H, int W, int T, int Se, int tiles_x, int tiles_y, int tw, int th, int threads, int blend, ResGeom* g) {
    if (tiles_x < 1 || tiles_y < 1 || tw < 4 || (tw & 3) || th < 1 || Se < 1) return false;
    const int hyw = Se - 1, hxw = round_up4(Se - 1), phases = ceil_div(T, Se);
    if (phases > 1 && (Se & 1)) return false;          // every phase must start in buffer 0 (see RES_PP)
    if (tiles_x * tw < W || tiles_y * th < H) return false;
    // the (shifted) halo must come from adjacent tiles only
    if (phases > 1 && ((tiles_x > 1 && tw < 2 * hxw) || (tiles_y > 1 && th < 2 * hyw))) return false;
    const int wq = (tw + 2 * hxw) / 4, wr = th + 2 * hyw;
    if (wq > threads) return false;
    const int nq = ceil_div(wr, threads / wq);            // threads / wq strips per quad column
    if (nq > (threads == 1024 ? 1 : RES_MAX_NQ)) return false;
    const int dr = wr + 2, ls = res_row_stride(wq, nq, dr);
    if ((size_t)dr * ls > (size_t)RES_PP) return false;                      // one depth buffer per RES_PP slot
    const size_t ldsb = res_lds_bytes(dr, ls, nq, blend, threads);
    if (ldsb > 160 * 1024) return false;
    *g = ResGeom{Se, tiles_x, tiles_y, tw, th, nq, wq, wr, hxw, hyw, dr, ls, 0, 0, ldsb, 0.0};
    g->threads = threads;
    set_uniform_rows(g);
    return true;
}

// Tiling of one image for the resident kernel: every workgroup owns a tw x th tile + (S-1) halo; a launch holds
// imgs_per_launch whole images on at most `ncu` workgroups.  Cost model: launches x (quads per thread + latency floor).
bool resident_geometry(int B, int H, int W, int T, int blend, int ncu, int S_user, ResGeom* best, int threads = RES_THREADS) {
    if (threads == RES_THREADS_CLIPPED) return resident_geometry_clipped(B, H, W, T, blend, ncu, S_user, best);
    if (W % 4 != 0 || ncu < 1 || T < 1) return false;
    if (threads != 1024) threads = RES_THREADS;
    bool found = false;
    // phase lengths 12 / 8 / 6 / 4: twelve (one exchange at T = 24) wins on small shards whose tiles stay at two quads per
    // thread (NYU B = 6: 22.2 vs 23.9 us), eight everywhere else (tools/probes/resident_s_sweep.py)
    for (int S = (S_user > 0 ? S_user : 12); S >= (S_user > 0 ? S_user : 4); S -= (S > 8 ? 4 : 2)) {
        const int Se = S > T ? T : S;
        const int phases = ceil_div(T, Se);
        for (int tx = 1; tx <= 32; ++tx) {
            const int tw = round_up4(ceil_div(W, tx));
            if (tx > 1 && (tw < 16 || ceil_div(W, tw) != tx)) continue;
            for (int ty = 1; ty <= 64; ++ty) {
                const int th = ceil_div(H, ty);
                if (ty > 1 && (th < 4 || ceil_div(H, th) != ty)) continue;
                const int tiles = tx * ty;
                if (tiles > ncu) continue;
                ResGeom cand;
                if (!rgeom_fill(H, W, T, Se, tx, ty, tw, th, threads, blend, &cand)) continue;
                int ipl = ncu / tiles;
                if (ipl > B) ipl = B;
                cand.imgs_per_launch = ipl; cand.launches = ceil_div(B, ipl);
                // microseconds per launch, fitted on MI355X (profiles/r02_resident_vs_multilaunch.jsonl): launch + epilogue,
                // derive (~2 us per quad of a thread), T steps (VALU-bound: 0.13 us per quad; x 1.13 with the zero-padding
                // selects of a launch whose regions stick out of the image), and per phase boundary the publish / wait /
                // halo staging (3 us + the border bytes)
                const double pen = regions_inside_image(cand, H, W, W, T) ? 1.0 : 1.13;
                cand.cost = cand.launches * (8.0 + 2.0 * cand.nq + T * (0.13 * cand.nq + 0.1) * pen + (phases - 1) * (3.0 + 0.6 * cand.nq));
                if (!found || cand.cost < best->cost) { found = true; *best = cand; }
            }
        }
    }
    return found;
}

// The geometry of a launch: the plan's tiling when it carries one — re-derived and re-checked by clipped_geometry / rgeom_fill, the
// search is skipped (it is ~6000 candidate tilings: tens of microseconds per call on the host) — else the search's.
int resident_resolve(int B, int H, int W, int T, int blend, int ncu, const cspn_resident_plan& rp, ResGeom* g) {
    if (!plan_has_tiling(rp)) {
        if (!resident_geometry(B, H, W, T, blend, ncu, rp.steps_per_phase, g, rp.threads))
            return fail("cspn3_forward_resident: no resident tiling for B=%d %dx%d T=%d", B, H, W, T);
        return 1;
    }
    const int Se = rp.steps_per_phase > T ? T : rp.steps_per_phase;
    const bool clipped = rp.threads == RES_THREADS_CLIPPED;       // tile_h is then the FIRST tile row's height, the uneven rows follow from it
    const bool ok = clipped ? clipped_geometry(H, W, T, Se, rp.tiles_x, rp.tiles_y, rp.tile_w, rp.tile_h, blend, g)
                            : rgeom_fill(H, W, T, Se, rp.tiles_x, rp.tiles_y, rp.tile_w, rp.tile_h, rp.threads == 1024 ? 1024 : RES_THREADS, blend, g);
    if (!ok || (long)rp.images_per_launch * g->tiles_x * g->tiles_y > ncu)
        return fail("cspn3_forward_resident: the %splan does not fit this problem / device (use cspn3_resident_plan)", clipped ? "clipped " : "");
    g->imgs_per_launch = rp.images_per_launch;
    return 1;
}

// The instances of cspn3_resident.  512 threads: every form, 1 .. RES_MAX_NQ quads per thread.  1024 threads (one quad per thread)
// and 768 (three quads per thread on clipped regions, CLEAN only): the inference forms — plain / scored — with CSPN_new weights.
using ResLaunchFn = int (*)(int, int, size_t, hipStream_t, const ResArgs&);
template <int NQ, int NTH, int CLEAN, int BLEND, int F>
constexpr ResLaunchFn res_instance() {
    constexpr ResidentForm f = static_cast<ResidentForm>(F);
    if constexpr (NTH == RES_THREADS || (f <= ResidentForm::Scored && (NTH == 1024 || CLEAN)))
        return &launch_dynamic_lds<cspn3_resident<NQ, NTH, BLEND, resident_form_mode(f), CLEAN, resident_form_pac(f)>, ResArgs>;
    else
        return nullptr;
}
template <int NQ, int NTH, int CLEAN, int BLEND, int... F>
constexpr std::array<ResLaunchFn, sizeof...(F)> res_instances(std::integer_sequence<int, F...>) { return {res_instance<NQ, NTH, CLEAN, BLEND, F>()...}; }
// the instance for (clean, blend, form) at NQ quads per thread on NTH threads, or null
template <int NQ, int NTH = RES_THREADS>
ResLaunchFn res_lookup(bool clean, int blend, ResidentForm form) {
    constexpr auto forms = std::make_integer_sequence<int, (int)ResidentForm::Count>{};
    static constexpr std::array<ResLaunchFn, (size_t)ResidentForm::Count> table[2][2] = {
        {res_instances<NQ, NTH, 0, 0>(forms), res_instances<NQ, NTH, 0, 1>(forms)}, {res_instances<NQ, NTH, 1, 0>(forms), res_instances<NQ, NTH, 1, 1>(forms)}};
    return table[clean ? 1 : 0][blend ? 1 : 0][(int)form];
}

}  // namespace

namespace {
int resident_launch(const void* guidance, long bs, long cs, const void* d0, const void* sparse, void* out, void* history,
                    void* w8_out, float* s_out, void* work, unsigned seq, unsigned* host_err, int B, int H, int W, int W_valid,
                    int T, int blend, const void* target, double* acc, int nslots, const cspn_resident_plan* plan,
                    cspn_stream_t stream, bool transposed, bool pac = false, const float* s_in = nullptr);
}

extern "C" {

int cspn3_resident_plan(int B, int H, int W, int T, int blend, int n_cu, cspn_resident_plan* out) {
    if (!out || B < 1 || H < 1 || W < 1 || T < 0) return fail("cspn3_resident_plan: bad arguments");
    if (n_cu <= 0) n_cu = cu_count();
    if (n_cu <= 0) return fail("cspn3_resident_plan: no device (pass n_cu > 0 to plan without one)");
    ResGeom g;
    if (T < 1 || !resident_geometry(B, H, W, T, blend, n_cu, out->steps_per_phase, &g, out->threads))
        return fail("cspn3_resident_plan: no resident tiling for B=%d %dx%d T=%d on %d CUs (W %% 4 == 0 needed)", B, H, W, T, n_cu);
    if (ceil_div(T, g.S) > 255) return fail("cspn3_resident_plan: T=%d in %d-step phases is more than 255 phases", T, g.S);
    out->steps_per_phase = g.S; out->tiles_x = g.tiles_x; out->tiles_y = g.tiles_y; out->tile_w = g.tw;
    out->tile_h = g.threads == RES_THREADS_CLIPPED ? g.th0 : g.th;       // (clipped plans: the first row; the others follow from it)
    out->quads_per_thread = g.nq; out->threads = g.threads; out->images_per_launch = g.imgs_per_launch;
    out->launches = g.launches; out->lds_bytes = (int)g.lds_bytes; out->n_cu = n_cu;
    out->region_over_tile = g.threads == RES_THREADS_CLIPPED
        ? (float)((double)(4 * g.wq) * g.wr * g.tiles_x * g.tiles_y / ((double)H * W))
        : (float)((double)(4 * g.wq) * g.wr / ((double)g.tw * g.th));
    return 1;
}

size_t cspn3_resident_workspace_bytes(int B, int H, int W) {
    return resident_workspace_bytes(B, H, W, sizeof(float), 16);       // tiles are >= 4 x 4
}

int cspn3_forward_resident(const void* guidance, long bs, long cs, const void* d0, const void* sparse, void* out,
                           void* history, void* w8_out, float* s_out,
                           void* work, unsigned seq, unsigned* host_err, int B, int H, int W, int W_valid, int T, int blend,
                           const void* target, double* acc, int nslots, const cspn_resident_plan* plan,
                           cspn_stream_t stream) {
    return resident_launch(guidance, bs, cs, d0, sparse, out, history, w8_out, s_out, work, seq, host_err, B, H, W, W_valid, T,
                           blend, target, acc, nslots, plan, stream, /*transposed=*/false);
}

int cspn3_transposed_resident(const void* w8, const float* g_T, const float* sparse_f32, float* history, void* work,
                              unsigned seq, unsigned* host_err, int B, int H, int W, int W_valid, int T, int premask,
                              const cspn_resident_plan* plan, cspn_stream_t stream) {
    if (!w8 || !g_T || !history) return fail("cspn3_transposed_resident: bad arguments");
    if (!check_premask("cspn3_transposed_resident", premask, sparse_f32)) return 0;
    return resident_launch(w8, (long)8 * H * W, (long)H * W, g_T, premask ? sparse_f32 : nullptr, nullptr, history, nullptr, nullptr,
                           work, seq, host_err, B, H, W, W_valid, T, premask ? 1 : 0, nullptr, nullptr, 0, plan, stream,
                           /*transposed=*/true);
}

int cspn3_transposed_resident_guidance(const void* guidance, long bs, long cs, const float* S, const float* g_T,
                                       const float* sparse_f32, float* history, void* work, unsigned seq, unsigned* host_err,
                                       int B, int H, int W, int W_valid, int T, int premask, const cspn_resident_plan* plan,
                                       cspn_stream_t stream) {
    if (!guidance || !S || !g_T || !history) return fail("cspn3_transposed_resident_guidance: bad arguments");
    if (!check_premask("cspn3_transposed_resident_guidance", premask, sparse_f32)) return 0;
    if (!aligned16(S)) return fail("cspn3_transposed_resident_guidance: S must be 16-byte aligned");
    return resident_launch(guidance, bs, cs, g_T, premask ? sparse_f32 : nullptr, nullptr, history, nullptr, nullptr, work, seq,
                           host_err, B, H, W, W_valid, T, premask ? 1 : 0, nullptr, nullptr, 0, plan, stream,
                           /*transposed=*/true, /*pac=*/false, S);
}

}  // extern "C"

namespace cspn_detail {
// K = 3 softmax (CSPN_ours) forward with fp32 guidance [B,8,H,W] on the quad kernel: called by cspnk_forward_resident
// (cspnk_resident.hip), whose oct kernel holds only two or three octs of fp32 taps per thread.
int resident_pac3_f32(const void* guided, const void* x0, const void* sparse, void* out, void* history, void* wk_out, void* work,
                      unsigned seq, unsigned* host_err, int B, int H, int W, int T, int blend, const void* target, double* acc,
                      int nslots, const cspn_resident_plan* plan, cspn_stream_t stream) {
    return resident_launch(guided, (long)8 * H * W, (long)H * W, x0, sparse, out, history, wk_out, nullptr, work, seq, host_err, B, H, W, 0, T,
                           blend, target, acc, nslots, plan, stream, /*transposed=*/false, /*pac=*/true);
}
}  // namespace cspn_detail

namespace {

int resident_launch(const void* guidance, long bs, long cs, const void* d0, const void* sparse, void* out,
                    void* history, void* w8_out, float* s_out,
                    void* work, unsigned seq, unsigned* host_err, int B, int H, int W, int W_valid, int T, int blend,
                    const void* target, double* acc, int nslots, const cspn_resident_plan* plan,
                    cspn_stream_t stream, bool transposed, bool pac, const float* s_in) {
    if (!guidance || !d0 || !work || B <= 0 || H <= 0 || W <= 0 || T < 1 || (!out && !history))
        return fail("cspn3_forward_resident: bad arguments");
    if (!transposed && history && ((pac && !w8_out) || (!pac && !s_out) || target || acc || !aligned16(history) || (w8_out && !aligned16(w8_out)) || (s_out && !aligned16(s_out))))
        return fail("cspn3_forward_resident: the training form (history) needs s_out (w8_out is optional: null publishes S only), 16-byte aligned, and no scoring");
    if (!history && (w8_out || s_out)) return fail("cspn3_forward_resident: w8_out / s_out are outputs of the training form (history)");
    if (transposed && !aligned16(history)) return fail("cspn3_transposed_resident: history must be 16-byte aligned");
    const char* const who = "cspn3_forward_resident";         // (the name every rule of the three 3x3 entry points' common part reports)
    if (!check_blend(who, blend, sparse) || !check_scoring(who, target, acc, nslots)) return 0;
    if ((W & 3) || (cs & 3) || (bs & 3)) return fail("cspn3_forward_resident: W and the guidance strides must be multiples of 4");
    if (cs < 0 || bs < 0 || cs >= (1L << 27) || (long)H * W >= (1L << 27))
        return fail("cspn3_forward_resident: images of >= 2^27 pixels / channel strides >= 2^27 elements are not supported (32-bit offsets)");
    if (!check_tensors_aligned16(who, {guidance, d0, out, work, sparse})) return 0;
    if (W_valid < 0 || W_valid > W) return fail("cspn3_forward_resident: W_valid=%d outside (0, W=%d]", W_valid, W);
    if (!check_seq(who, seq)) return 0;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ncu = cu_count();
    if (ncu <= 0) return fail("cspn3_forward_resident: no device");
    ResGeom g;
    cspn_resident_plan rp{};
    if (plan) rp = *plan;
    const int Wv = (W_valid > 0 && W_valid < W) ? W_valid : W;
    if (rp.threads == RES_THREADS_CLIPPED && (transposed || history || pac || Wv != W)) {
        // the clipped instance serves plain / scored inference on unpadded rows: everything else takes the 512-thread plan of the
        // same phase length (its tiling is searched for: the clipped plan's tile fields mean nothing to it)
        rp.threads = RES_THREADS;
        rp.tiles_x = rp.tiles_y = rp.tile_w = rp.tile_h = rp.images_per_launch = 0;
    }
    if (!resident_resolve(B, H, W, T, blend, ncu, rp, &g)) return 0;
    // a tile that finished phase p publishes seq + p + 1, and the next call on the workspace brings seq + 256: more than
    // 255 phases would let one call's flags satisfy the next call's waits
    if (ceil_div(T, g.S) > 255)
        return fail("cspn3_forward_resident: T=%d in %d-step phases is more than 255 phases (use the multi-launch schedule)", T, g.S);
    ResArgs a{};
    a.g = static_cast<const float*>(guidance); a.g_bs = bs; a.g_cs = cs;
    a.d0 = static_cast<const float*>(d0); a.sparse = static_cast<const float*>(sparse); a.out = static_cast<float*>(out);
    a.xbuf = static_cast<float*>(work);
    a.status = resident_status_words(work, B, H, W, sizeof(float));
    a.flags = resident_phase_flags(a.status);
    if ((size_t)B * g.tiles_x * g.tiles_y > (size_t)B * (((size_t)H * W) / 16 + 1))
        return fail("cspn3_forward_resident: workspace too small for %d tiles", B * g.tiles_x * g.tiles_y);
    a.host_err = host_err;
    a.hist = static_cast<float*>(history); a.w_out = static_cast<float*>(w8_out); a.s_out = s_out;
    if (pac && transposed) return fail("cspn3_forward_resident: the softmax-weight form has no transposed sweep (use cspn3_transposed_resident on the volume)");
    const ResidentForm plain = history ? ResidentForm::Training : acc ? ResidentForm::Scored : ResidentForm::Inference;
    const ResidentForm form = transposed ? (s_in ? ResidentForm::SweepGuidance : ResidentForm::SweepVolume)
                                         : pac ? static_cast<ResidentForm>((int)plain + (int)ResidentForm::SoftmaxInference) : plain;
    a.s_in = s_in;
    a.seq = seq;
    a.target = static_cast<const float*>(target); a.macc = acc; a.nslots = nslots;
    a.B = B; a.H = H; a.W = W; a.Wv = Wv; a.T = T; a.S = g.S;
    a.tw = g.tw; a.th = g.th; a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y; a.th0 = g.th0; a.thl = g.thl;
    a.wq = g.wq; a.wr = g.wr; a.hxw = g.hxw; a.hyw = g.hyw; a.dr = g.dr; a.ls = g.ls;
    a.spin_limit = plan_spin_limit(rp);
    a.dbg = rp.debug_stamps;
    a.mg_wq = res_magic(g.wq); a.mg_tiles_x = res_magic(g.tiles_x); a.mg_tpi = res_magic(g.tiles_x * g.tiles_y);
    a.step_r = g.threads / g.wq; a.step_q = g.threads % g.wq;
    const bool clean = regions_inside_image(g, H, W, a.Wv, T);
    // (refused rather than ignored: a host that asked for the guard relies on `out` being complete for GPU-side consumers)
    if (rp.guard && (!resident_form_guarded(form) || (resident_form_mode(form) <= 1 && !out) || !cspn_detail::resident_repair_fits(T)))
        return fail("cspn3_forward_resident: plan->guard serves inference (plain / scored), the training forward and the reverse sweeps, T <= 54 steps");
    ResLaunchFn launch = nullptr;
    if (g.threads == RES_THREADS_CLIPPED) {
        if (!clean) return fail("cspn3_forward_resident: a clipped plan whose regions leave the image");
        launch = res_lookup<3, RES_THREADS_CLIPPED>(clean, blend, form);
    } else if (g.threads == 1024) {
        launch = res_lookup<1, 1024>(clean, blend, form);
    } else {
        switch (g.nq) {
            case 1: launch = res_lookup<1>(clean, blend, form); break;
            case 2: launch = res_lookup<2>(clean, blend, form); break;
            case 3: launch = res_lookup<3>(clean, blend, form); break;
            case 4: launch = res_lookup<4>(clean, blend, form); break;
            case 5: launch = res_lookup<5>(clean, blend, form); break;
            default: return fail("cspn3_forward_resident: no instance for %d quads per thread", g.nq);
        }
    }
    if (!launch) return fail("cspn3_forward_resident: %d-thread workgroups serve the inference forms only", g.threads);
    // one launch per RES_ROUNDS_PER_LAUNCH rounds of images_per_launch images (more than one round: measured, not faster: see there)
    const int ipl = g.imgs_per_launch < B ? g.imgs_per_launch : B;
    constexpr int max_rounds = RES_ROUNDS_PER_LAUNCH;
    for (int b0 = 0; b0 < B; b0 += ipl * max_rounds) {
        a.b0 = b0;
        a.nb = (B - b0) < ipl ? (B - b0) : ipl;
        a.mg_round = res_magic(a.nb * g.tiles_x * g.tiles_y);
        const int rounds = ceil_div(B - b0, ipl) < max_rounds ? ceil_div(B - b0, ipl) : max_rounds;
        a.last_chunk = (b0 + ipl * max_rounds >= B) ? 1 : 0;
        if (!launch(rounds * a.nb * g.tiles_x * g.tiles_y, g.threads, g.lds_bytes, st, a)) return 0;
    }
    if (rp.guard)
        return cspn_detail::resident_repair_launch(a.g, bs, cs, a.d0, a.sparse, a.out, a.hist, a.s_out, a.w_out, a.s_in, form, a.status, seq, B, H, W,
                                                   a.Wv, T, blend ? 1 : 0, ncu, st, a.target, a.macc, a.nslots);
    return 1;
}

}  // namespace

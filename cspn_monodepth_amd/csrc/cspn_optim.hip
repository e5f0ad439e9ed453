// cspn_optim.hip — the reference's optimiser step, torch.optim.SGD(lr, momentum, weight_decay) (main.py:72-74), as one multi-tensor
// kernel (include/cspn_optim.h).
//
// A launch carries, BY VALUE in its kernel arguments, the group's hyper-parameters, up to CSPN_SGD_TENSORS_PER_LAUNCH tensor
// descriptors and the exclusive prefix of their chunk counts: 4072 bytes of explicit arguments (the compiler's hidden arguments
// come on top: a 4328-byte argument segment).  Workgroup b takes the chunk ids b, b + grid, ...; the
// tensor of a chunk id is found by a binary search over the prefix (7 steps cover 128 >= 109 entries), on values that are uniform
// over the workgroup: the descriptor reads are scalar loads from the argument segment.  No LDS, no atomics, no waiting: a chunk
// belongs to one workgroup and every element is read and written by one thread.
//
// The arithmetic is written out operation by operation (__fmaf_rn, __fmul_rn under contraction switched off): the compiler's
// default contraction would fuse momentum * buf into the add that follows it, which torch's single-tensor form rounds on its own.
#include "cspn_common.hpp"
#include "cspn_optim.h"

namespace {

constexpr int SGD_THREADS = 256;
constexpr int SGD_QUADS = CSPN_SGD_CHUNK / (4 * SGD_THREADS);      // 16-byte units per thread and chunk
static_assert(SGD_QUADS * 4 * SGD_THREADS == CSPN_SGD_CHUNK, "a chunk is a whole number of 16-byte units per thread");
constexpr unsigned SGD_MAX_LAUNCH_CHUNKS = 0x7fffffffu;            // the prefix is 32-bit
constexpr int SGD_GRID_LIMIT = 65535;                              // x 256 threads: far inside HIP's 2^32 threads per launch

enum { SGD_NESTEROV = 1, SGD_MAXIMIZE = 2, SGD_MOMENTUM = 4, SGD_DECAY = 8 };

struct SgdSlot {
    float* p;
    const float* g;
    float* buf;
    size_t n;
};

struct SgdArgs {
    const float* lr_device;
    float lr, momentum, one_minus_dampening, weight_decay;
    int flags, n_tensors;
    SgdSlot t[CSPN_SGD_TENSORS_PER_LAUNCH];
    unsigned prefix[CSPN_SGD_TENSORS_PER_LAUNCH + 1];              // prefix[i]: chunks of the tensors before i; prefix[n_tensors]: all
    unsigned char first[CSPN_SGD_TENSORS_PER_LAUNCH];
};
static_assert(sizeof(SgdArgs) <= 4096, "a launch's explicit arguments stay within 4 KB");
static_assert(CSPN_SGD_TENSORS_PER_LAUNCH <= 128, "the search below takes 7 steps");

struct SgdHyper {
    float lr, momentum, one_minus_dampening, weight_decay;
    bool nesterov, maximize, has_momentum, has_decay, first;
};

// one element: p and buf in, p and buf out (buf untouched without momentum)
__device__ __forceinline__ void sgd_element(float& p, float g, float& buf, const SgdHyper& h) {
#pragma clang fp contract(off)
    if (h.maximize) g = -g;
    if (h.has_decay) g = __fmaf_rn(h.weight_decay, p, g);
    float d = g;
    if (h.has_momentum) {
        const float b = h.first ? g : __fmaf_rn(h.one_minus_dampening, g, __fmul_rn(h.momentum, buf));
        buf = b;
        d = h.nesterov ? __fmaf_rn(h.momentum, b, g) : b;
    }
    p = __fmaf_rn(-h.lr, d, p);
}

__device__ __forceinline__ void sgd_quad(float4& p, const float4& g, float4& b, const SgdHyper& h) {
    sgd_element(p.x, g.x, b.x, h);
    sgd_element(p.y, g.y, b.y, h);
    sgd_element(p.z, g.z, b.z, h);
    sgd_element(p.w, g.w, b.w, h);
}

__global__ __launch_bounds__(SGD_THREADS) void cspn_sgd_kernel(const SgdArgs a) {
    SgdHyper h;
    h.lr = a.lr_device ? *a.lr_device : a.lr;                      // one scalar load per workgroup
    h.momentum = a.momentum;
    h.one_minus_dampening = a.one_minus_dampening;
    h.weight_decay = a.weight_decay;
    h.nesterov = a.flags & SGD_NESTEROV;
    h.maximize = a.flags & SGD_MAXIMIZE;
    h.has_momentum = a.flags & SGD_MOMENTUM;
    h.has_decay = a.flags & SGD_DECAY;
    const unsigned total = a.prefix[a.n_tensors];
    const int tid = threadIdx.x;
    for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
        int lo = 0, hi = a.n_tensors;                              // prefix[lo] <= c < prefix[hi]
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            const int mid = (lo + hi) >> 1;
            if (mid > lo) {
                if (a.prefix[mid] <= c) lo = mid; else hi = mid;
            }
        }
        const SgdSlot t = a.t[lo];
        h.first = a.first[lo] != 0;
        const size_t off = (size_t)(c - a.prefix[lo]) * CSPN_SGD_CHUNK;
        const size_t left = t.n - off;
        const int len = left < (size_t)CSPN_SGD_CHUNK ? (int)left : CSPN_SGD_CHUNK;
        float* p = t.p + off;
        const float* g = t.g + off;
        float* buf = h.has_momentum ? t.buf + off : nullptr;
        const bool load_buf = h.has_momentum && !h.first;
        const bool vec = (((uintptr_t)t.p | (uintptr_t)t.g | (h.has_momentum ? (uintptr_t)t.buf : 0)) & 15) == 0;   // off keeps alignment
        int done = 0;                                             // elements the 16-byte path covers
        if (vec) {
            done = len & ~3;
            float4 vp[SGD_QUADS], vg[SGD_QUADS], vb[SGD_QUADS];
#pragma unroll
            for (int k = 0; k < SGD_QUADS; ++k) {
                const int i = (k * SGD_THREADS + tid) * 4;
                if (i < done) {
                    vp[k] = ld4(p + i);
                    vg[k] = ld4(g + i);
                    vb[k] = load_buf ? ld4(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (int k = 0; k < SGD_QUADS; ++k) {
                const int i = (k * SGD_THREADS + tid) * 4;
                if (i < done) {
                    sgd_quad(vp[k], vg[k], vb[k], h);
                    st4(p + i, vp[k]);
                    if (h.has_momentum) st4(buf + i, vb[k]);
                }
            }
        }
        for (int i = done + tid; i < len; i += SGD_THREADS) {      // a tensor's tail, or a tensor off the 16-byte grid
            float pe = p[i], be = load_buf ? buf[i] : 0.f;
            sgd_element(pe, g[i], be, h);
            p[i] = pe;
            if (h.has_momentum) buf[i] = be;
        }
    }
}

inline size_t chunks_of(size_t n) { return n / CSPN_SGD_CHUNK + (n % CSPN_SGD_CHUNK ? 1 : 0); }

// The split of a tensor list into launches, shared by the plan and the step: a launch closes when it holds
// CSPN_SGD_TENSORS_PER_LAUNCH tensors or when the next tensor would take its chunk count past 32 bits.  `emit(first, last, chunks)`
// is called per launch with the index range [first, last) of the ORIGINAL list (empty tensors inside it are skipped by the caller).
template <class NUMEL, class EMIT>
int split_launches(const char* who, int n_tensors, NUMEL numel, EMIT emit) {
    int begin = 0, held = 0;
    size_t chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const size_t c = chunks_of(numel(i));
        if (c == 0) continue;
        if (c > SGD_MAX_LAUNCH_CHUNKS) return fail("%s: tensor %d has %zu elements, more than a launch can index", who, i, numel(i));
        if (held == CSPN_SGD_TENSORS_PER_LAUNCH || chunks + c > SGD_MAX_LAUNCH_CHUNKS) {
            if (!emit(begin, i, chunks)) return 0;
            begin = i;
            held = 0;
            chunks = 0;
        }
        ++held;
        chunks += c;
    }
    if (held && !emit(begin, n_tensors, chunks)) return 0;
    return 1;
}

int resolve_workgroups(const char* who, int max_workgroups, int* out) {
    if (max_workgroups < 0) return fail("%s: max_workgroups %d (0 = the default %d)", who, max_workgroups, CSPN_SGD_MAX_WORKGROUPS);
    *out = max_workgroups ? max_workgroups : CSPN_SGD_MAX_WORKGROUPS;
    if (*out > SGD_GRID_LIMIT) *out = SGD_GRID_LIMIT;              // a larger grid buys nothing: the workgroups stride
    return 1;
}

}  // namespace

extern "C" {

int cspn_optim_abi_version(void) { return CSPN_OPTIM_ABI_VERSION; }

int cspn_sgd_plan(const size_t* numel, int n_tensors, int max_workgroups, int* launches, size_t* chunks) {
    int cap = 0;
    if (n_tensors < 0 || (n_tensors > 0 && !numel)) return fail("cspn_sgd_plan: n_tensors %d, numel %p", n_tensors, (const void*)numel);
    if (!resolve_workgroups("cspn_sgd_plan", max_workgroups, &cap)) return 0;
    int nl = 0;
    size_t total = 0;
    if (!split_launches("cspn_sgd_plan", n_tensors, [&](int i) { return numel[i]; }, [&](int, int, size_t c) {
            ++nl;
            total += c;
            return 1;
        }))
        return 0;
    if (launches) *launches = nl;
    if (chunks) *chunks = total;
    return 1;
}

int cspn_sgd_step(const cspn_sgd_tensor_t* tensors, int n_tensors, const cspn_sgd_hyper_t* hyper, int dtype, int max_workgroups,
                  cspn_stream_t stream) {
    const char* who = "cspn_sgd_step";
    int cap = 0;
    if (dtype != CSPN_F32) return fail("%s: dtype %d is not supported (CSPN_F32 only)", who, dtype);
    if (n_tensors < 0 || (n_tensors > 0 && !tensors) || !hyper) return fail("%s: n_tensors %d, tensors %p, hyper %p", who, n_tensors,
                                                                             (const void*)tensors, (const void*)hyper);
    if (!resolve_workgroups(who, max_workgroups, &cap)) return 0;
    const bool has_momentum = hyper->momentum != 0.0;
    if (hyper->nesterov && (!has_momentum || hyper->dampening != 0.0))
        return fail("%s: nesterov needs a momentum and zero dampening", who);
    if (((uintptr_t)hyper->lr_device & 3) != 0) return fail("%s: lr_device must be 4-byte aligned", who);
    for (int i = 0; i < n_tensors; ++i) {
        const cspn_sgd_tensor_t& t = tensors[i];
        if (t.n == 0) continue;
        if (!t.param || !t.grad || (has_momentum && !t.momentum_buffer))
            return fail("%s: tensor %d: param %p, grad %p, momentum_buffer %p", who, i, t.param, t.grad, t.momentum_buffer);
        if ((((uintptr_t)t.param | (uintptr_t)t.grad | (has_momentum ? (uintptr_t)t.momentum_buffer : 0)) & 3) != 0)
            return fail("%s: tensor %d is not aligned to its element size", who, i);
    }
    SgdArgs a;
    a.lr_device = hyper->lr_device;
    a.lr = (float)hyper->lr;
    a.momentum = (float)hyper->momentum;
    a.one_minus_dampening = (float)(1.0 - hyper->dampening);
    a.weight_decay = (float)hyper->weight_decay;
    a.flags = (hyper->nesterov ? SGD_NESTEROV : 0) | (hyper->maximize ? SGD_MAXIMIZE : 0) | (has_momentum ? SGD_MOMENTUM : 0) |
              (hyper->weight_decay != 0.0 ? SGD_DECAY : 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return split_launches(who, n_tensors, [&](int i) { return tensors[i].n; }, [&](int first, int last, size_t chunks) {
        int k = 0;
        unsigned run = 0;
        for (int i = first; i < last; ++i) {
            const cspn_sgd_tensor_t& t = tensors[i];
            if (t.n == 0) continue;
            a.t[k] = SgdSlot{static_cast<float*>(t.param), static_cast<const float*>(t.grad), static_cast<float*>(t.momentum_buffer), t.n};
            a.prefix[k] = run;
            a.first[k] = t.first ? 1 : 0;
            run += (unsigned)chunks_of(t.n);
            ++k;
        }
        a.prefix[k] = run;
        a.n_tensors = k;
        for (int j = k; j < CSPN_SGD_TENSORS_PER_LAUNCH; ++j) {    // no stale host stack in the arguments
            a.t[j] = SgdSlot{nullptr, nullptr, nullptr, 0};
            a.prefix[j + 1] = run;
            a.first[j] = 0;
        }
        const unsigned grid = chunks < (size_t)cap ? (unsigned)chunks : (unsigned)cap;
        hipLaunchKernelGGL(cspn_sgd_kernel, dim3(grid), dim3(SGD_THREADS), 0, st, a);
        HIP_OK(hipGetLastError());
        return 1;
    });
}

}  // extern "C"

/*
 * cspn_abn.h — C ABI of In-Place Activated BatchNorm in libcspn_hip.so (paths relative to the reference repo):
 *   network/libs/inplace_abn/src/bn.cu:125-232   mean_var / forward / edz_eydz / backward kernels
 *   network/libs/inplace_abn/src/bn.cu:302-377   leaky_relu / elu, their gradients and inverses (thrust passes)
 *   network/libs/inplace_abn/functions.py        the autograd functions that drive them
 * This is the component the library's convention comes from: `extern "C" int ...(..., stream)` returning 1 on success and 0 on
 * failure (+ cspn_last_error()).  A header of its own with a version of its own: CSPN_ABI_VERSION (cspn_hip.h) does not move.
 * The caller owns every buffer and selects the device; the library enqueues on the given stream and never synchronises, so a
 * whole step can sit inside a graph capture.
 *
 * Storage: fp32, contiguous NCHW seen as (N, C, S = H * W); an NC input is S = 1.  Per-channel vectors hold C floats.
 *
 * Arithmetic (gamma = |weight| + eps, or 1 for a null weight; beta = bias, or 0 for a null bias):
 *   forward    y = (x - mean) * invstd,  invstd = 1 / sqrt(var + eps), 0 when var == 0 && eps == 0
 *              z = act(y * gamma + beta), written over x
 *   training   mean / var = the biased statistics over the N * S elements of a channel, read ONCE: every thread, wavefront and
 *              workgroup keeps (count, mean, M2) and they are merged pairwise with Chan's formula (units of 4 elements enter a
 *              thread's triple the same way), so a channel mean many standard deviations from 0 costs no accuracy;
 *              running_mean = (1 - momentum) running_mean + momentum mean
 *              running_var  = (1 - momentum) running_var  + momentum var n / (n - 1),  n = N * S      (on the device)
 *   backward   where z < 0:  leaky_relu: dz' = dz * slope, z' = z * (1 / slope);  elu: dz' = dz * (z + 1), z' = log1p(z)
 *              y = (z' - beta) / gamma,  edz = mean(dz'),  eydz = mean(y dz')
 *              dx = (dz' - edz - y eydz) gamma invstd,  dweight = sign(weight) eydz N S,  dbias = edz N S
 *              eval mode: edz = eydz = 0 (as the reference leaves it, functions.py:144-147)
 * Two differences from the reference, both on purpose: the backward reads z and dz and modifies neither (the reference
 * overwrites the saved output with the pre-activation and scales the incoming gradient in place, functions.py:54-60), and a
 * training call with N * S == 1 fails (the reference divides by n - 1 = 0).
 *
 * Two regimes, chosen by cspn_abn_plan from (N, C, S) alone:
 *   CSPN_ABN_SMALL  a channel's N * S elements fit in the LDS slice of one thread group: ONE launch does statistics + apply
 *                   (or reduce + dx) and reads its input once.  Up to N * S = 1024 four channels share a workgroup of 256
 *                   threads (one wavefront each), above that a channel has the whole workgroup.
 *   CSPN_ABN_SPLIT  every channel is cut into `workgroups_per_channel` ranges of `elements_per_workgroup` consecutive elements
 *                   of its (n, s) index space: partials -> finalise (merges the partials of a channel in increasing range
 *                   order, in fp64, and updates the running statistics) -> apply.
 * No atomics anywhere: the result is a function of the values, the shape and the plan, bit for bit, run after run.
 * Loads and stores are 16 bytes wide with a scalar peel per (n, c) plane range (a plane's base is 16-byte aligned only when
 * S % 4 == 0); planes shorter than 32 elements, and tensors whose base pointers do not share one 16-byte phase, are moved
 * element by element: same values, same arithmetic.
 */
#ifndef CSPN_ABN_H_
#define CSPN_ABN_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_ABN_ABI_VERSION 1

enum { CSPN_ABN_ACT_LEAKY_RELU = 0, CSPN_ABN_ACT_ELU = 1, CSPN_ABN_ACT_NONE = 2 };
enum { CSPN_ABN_SMALL = 0, CSPN_ABN_SPLIT = 1 };
/* what a training-mode cspn_abn_forward does: everything, or one half of it (the synchronised variant merges the statistics
 * of the ranks between the two halves) */
enum { CSPN_ABN_FULL = 0, CSPN_ABN_STATS_ONLY = 1, CSPN_ABN_APPLY_ONLY = 2 };

typedef struct cspn_abn_plan_t {
    int regime;                   /* CSPN_ABN_SMALL or CSPN_ABN_SPLIT */
    int channels_per_workgroup;   /* SMALL: 4 or 1;  SPLIT: 1 */
    int workgroups_per_channel;   /* SMALL: 1;  SPLIT: the ranges a channel is cut into */
    int threads;                  /* per workgroup */
    size_t elements_per_workgroup; /* of one channel: N * S (SMALL) or the length of a range (SPLIT, a multiple of 4) */
    size_t small_limit;           /* the largest N * S the SMALL regime takes */
} cspn_abn_plan_t;

/* Callable without a device.  Fails for N, C, S < 1. */
int cspn_abn_plan(int N, int C, int S, cspn_abn_plan_t* plan);

/* Bytes of `work` (16-byte aligned) the entry points below need for this shape; 0 in the SMALL regime (work may be null). */
size_t cspn_abn_workspace_bytes(int N, int C, int S);

/* x [N, C, S] is overwritten with z.  weight / bias: C floats or null.
 *   training == 0: mean / var are not touched; the statistics are running_mean / running_var (not modified); phase must be FULL.
 *   training != 0, FULL:        mean / var [C] are written (keep var for the backward); running_* are updated when non-null.
 *                  STATS_ONLY:  mean / var are written, x and running_* are left alone.
 *                  APPLY_ONLY:  mean / var are read, x is overwritten, running_* are left alone. */
int cspn_abn_forward(void* x, const float* weight, const float* bias, float* running_mean, float* running_var,
                     float* mean, float* var, int N, int C, int S, int training, int phase, float momentum, float eps,
                     int activation, float slope, void* work, cspn_stream_t stream);

/* edz / eydz [C] of (z, dz): the reduction half of a training backward on its own (the synchronised variant averages them over
 * the ranks before cspn_abn_backward). */
int cspn_abn_backward_reduce(const void* z, const void* dz, const float* weight, const float* bias, float* edz, float* eydz,
                             int N, int C, int S, float eps, int activation, float slope, void* work, cspn_stream_t stream);

/* dx [N, C, S] (required), dweight / dbias [C] (may be null; OVERWRITTEN, not accumulated).  var: the statistics the forward
 * normalised with.  edz / eydz: both given -> used as they are; both null and training != 0 -> computed here (SMALL: in the
 * same launch); training == 0 -> 0. */
int cspn_abn_backward(const void* z, const void* dz, const float* var, const float* weight, const float* bias,
                      const float* edz, const float* eydz, void* dx, float* dweight, float* dbias, int N, int C, int S,
                      int training, float eps, int activation, float slope, void* work, cspn_stream_t stream);

/* CSPN_ABN_ABI_VERSION the library was built from */
int cspn_abn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_ABN_H_ */

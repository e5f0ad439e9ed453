/*
 * cspn_max8.h — C ABI of the original CSPN release's propagation (paths relative to the reference repo):
 *   network/libs/post_process/CSPN.py:14-123    AffinityPropagate              (sparse-depth blend)
 *   network/libs/post_process/CSPN.py:126-231   AffinityPropagate_prediction   (no blend)
 * forward and backward, fp32 only (the reference's precision).
 *
 * A header of its own with a version of its own, as cspn_criterion.h: CSPN_ABI_VERSION (cspn_hip.h) does not move.  The
 * conventions are those of cspn_hip.h: 1 on success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects
 * the device, and the library enqueues on the given stream without synchronising.  No kernel waits for another workgroup.
 *
 * The arithmetic.  g_k = |G_k| (k = 0..7), m = sign(s), box(x) = the zero-padded 3x3 sum:
 *     S_k = box(g_k)
 *     d_0 = (1 - m) blur + m s                        (no sparse plane: d_0 = blur, and no blend anywhere)
 *     o_k = box(g_k d_{t-1}) * (1 / S_k)              t = 1..T
 *     e_t = max_k o_k                                 a NaN among the o_k gives NaN (torch.max), 0 * (1 / 0) = NaN = 0 / 0
 *     d_t = (1 - m) e_t + m s
 * A negative sparse value gives m = -1 and d_t = 2 e_t - s, as the reference does.
 *
 * Determinism contract.  Every box sum is formed as (left + centre) + right along a row and then (upper + middle) + lower, a
 * pixel outside the image counting as +0; products and sums are not contracted; 1 / S_k is the correctly rounded quotient.
 * The value of a pixel therefore does not depend on the tile it falls into, on steps_per_launch or on its image's place in the
 * batch: any two calls on the same values give the same bits.
 *
 * Planes.  guidance: fp32, channels 0..7 of image b at guidance + b * batch_stride + k * channel_stride (in elements), each
 * H x W contiguous; channels past 7 are never read.  d0 / sparse / out / grad_out / grad_blur: [B, H, W] contiguous fp32.
 * history: [T, B, H, W] fp32, plane t - 1 = d_t.  mask: [T, B, H, W] uint8, bit k of plane t - 1 set where o_k attains e_t
 * (0 where e_t is NaN) — the backward needs the whole set, not an index: torch.max hands each of two equal operands half of
 * the gradient, so exact ties split along the pairwise tree max(max(max(o0,o1),max(o2,o3)),max(max(o4,o5),max(o6,o7))).
 */
#ifndef CSPN_MAX8_H_
#define CSPN_MAX8_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_MAX8_ABI_VERSION 1

/* the largest steps_per_launch: a launch works on 64 x 48 regions that carry a halo of steps_per_launch pixels */
#define CSPN_MAX8_MAX_STEPS_PER_LAUNCH 16

/* Bytes of `work` (callable without a device; 0 for a bad size).  keep_history = 0: the two ping-pong planes of the forward.
 * keep_history != 0: what the backward needs as well (1 / S_k, the two gradient accumulators of 8 planes each, two planes of
 * the running cotangent): the size cspn_max8_backward asks for. */
size_t cspn_max8_workspace_bytes(int B, int H, int W, int T, int keep_history);

/* ceil(T / S) launches, S = steps_per_launch (0 = the built-in choice, otherwise 1..16; a value above T counts as T), each
 * advancing up to S steps on regions with an S-pixel halo clipped to the image.  sparse_or_null = NULL: the prediction
 * variant.  history_or_null and mask_or_null: both or neither; with them every step also writes d_t and its mask plane.
 * `out` must not alias an input.  work: 16-byte aligned, cspn_max8_workspace_bytes(B, H, W, T, 0) bytes — the two ping-pong
 * planes, with or without history. */
int cspn_max8_forward(const void* guidance, long batch_stride, long channel_stride, const void* d0, const void* sparse_or_null,
                      void* out, void* history_or_null, void* mask_or_null, void* work, int B, int H, int W, int T,
                      int steps_per_launch, cspn_stream_t stream);

/* The reverse sweep, T + 2 launches: with c_T = grad_out and w_k the tree weights of the mask, for t = T..1
 *     a_k = w_k (1 - m) c_t / S_k,   c_{t-1} = sum_k g_k box(a_k),   gbar_k += d_{t-1} box(a_k),   Sbar_k -= a_k e_t
 * then grad_guidance[:, k] = (gbar_k + box(Sbar_k)) sign(G_k) for k < 8 and 0 for 8 <= k < C ([B, C, H, W] contiguous), and
 * grad_blur = (1 - m) c_0.  EVERY element of both gradients is written; the sparse plane gets no gradient.  box is its own
 * adjoint, so every sum is a gather: no atomics.  history / mask: as the forward of the same inputs wrote them.
 * A pixel-step whose maximum is NaN has mask 0 and passes NO gradient (the reference's autograd hands NaN through it, which
 * then spreads over the whole sweep); every other pixel gets the gradient the reference gives a NaN-free input.
 * work: 16-byte aligned, cspn_max8_workspace_bytes(B, H, W, T, 1) bytes. */
int cspn_max8_backward(const void* guidance, long batch_stride, long channel_stride, int C, const void* blur,
                       const void* sparse_or_null, const void* history, const void* mask, const void* grad_out,
                       void* grad_guidance, void* grad_blur, void* work, int B, int H, int W, int T, cspn_stream_t stream);

/* CSPN_MAX8_ABI_VERSION the library was built from */
int cspn_max8_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_MAX8_H_ */

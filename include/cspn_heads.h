/*
 * cspn_heads.h — C ABI of the fused output heads: zero-insertion un-pooling by 2 followed by bias-free 3x3 convolutions (pad 1) of
 * several small heads over the same map, computed straight from the compact map (paths relative to the reference repo):
 *   network/unet_ours.py:194-202      Simple_Gudi_UpConv_Block_Last_Layer (gud_up_proj_layer5: 64 -> 1, gud_up_proj_layer6: 64 -> 8)
 *   network/unet_cspn_nyu.py:203-223  the same block of the config-5 model (64 -> 1, 64 -> 12)
 * forward and both gradients, fp32 only.
 *
 * A header of its own with a version of its own, as cspn_max8.h: CSPN_ABI_VERSION (cspn_hip.h) does not move.  The conventions are
 * those of cspn_hip.h: 1 on success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects the device, and the
 * library enqueues on the given stream without synchronising.  No kernel waits for another workgroup, there are no device-scope
 * flags and no atomics: every call can be captured in a graph.
 *
 * The arithmetic.  x: [N, C, H, W].  u is the un-pooled map cropped to oh x ow (1 <= oh <= 2H, 1 <= ow <= 2W):
 *     u[n, c, 2i, 2j] = x[n, c, i, j]  where 2i < oh and 2j < ow,   0 elsewhere
 * and head h with the filter w_h [O_h, C, 3, 3] gives y_h [N, O_h, oh, ow]:
 *     y_h[n, o, Y, X] = sum_c sum_{ky, kx} w_h[o, c, ky, kx] u[n, c, Y + ky - 1, X + kx - 1]           (outside u: nothing)
 * u is never formed: output pixel (2i + a, 2j + b) reads 1, 2, 2 or 4 pixels of x for (a, b) = (0,0), (0,1), (1,0), (1,1) — 9
 * multiplies per compact pixel, channel and output channel instead of 36.  The gradients:
 *     gx[n, c, i, j]      = sum_h sum_o sum_{ky, kx} w_h[o, c, ky, kx] gy_h[n, o, 2i + 1 - ky, 2j + 1 - kx]    where 2i < oh, 2j < ow
 *                         = 0                                                                                 elsewhere (cropped away)
 *     gw_h[o, c, ky, kx]  = sum_{n, i, j} gy_h[n, o, 2i + 1 - ky, 2j + 1 - kx] x[n, c, i, j]                   over 2i < oh, 2j < ow
 * with gy outside [0, oh) x [0, ow) counting as nothing.
 *
 * Determinism contract.  Forward: every output element is one chain of fused multiply-adds over the channels in ascending order,
 * the taps of a channel in the order of its window from the upper left.  gx: one chain per element over the heads in the order
 * given, their output channels, ky, kx ascending.  Neither depends on the frame's place in the batch or on N.  gw: per-workgroup
 * partial sums in a workspace, added by a second kernel in a fixed order — equal bits run after run for equal arguments.
 *
 * One difference from the reference: a NaN or Inf in x[n, c, i, j] reaches the outputs whose window covers (2i, 2j) only.  The
 * reference's un-pooling multiplies x by 0 at the inserted positions, so there it also reaches the windows that cover the other
 * three positions of its 2 x 2 block.
 *
 * Heads.  1 <= n_heads <= CSPN_HEADS_MAX_HEADS, every O_h >= 1, their sum <= CSPN_HEADS_MAX_OUT_CHANNELS.  weights[h], outs[h],
 * grad_outs[h], grad_weights[h]: host arrays of n_heads device pointers to contiguous fp32 tensors (4-byte aligned; the forward
 * writes 8 bytes per lane where ow is even and the outputs are 8-byte aligned).  N <= 65535.
 */
#ifndef CSPN_HEADS_H_
#define CSPN_HEADS_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_HEADS_ABI_VERSION 1

#define CSPN_HEADS_MAX_HEADS 4
#define CSPN_HEADS_MAX_OUT_CHANNELS 16

/* the `pass` of cspn_heads_workspace_bytes: which call the workspace is for */
#define CSPN_HEADS_FORWARD 0
#define CSPN_HEADS_BACKWARD_INPUT 1
#define CSPN_HEADS_BACKWARD_WEIGHTS 2

/* Bytes of the `work` of one call with `out_channels` output channels over all its heads (callable without a device; 0 for a bad
 * size).  Forward and backward_input: the filters of the call gathered into one buffer; backward_weights: the partial sums.
 * work: 16-byte aligned; its content on entry does not matter, and it may be reused once the call has run. */
size_t cspn_heads_workspace_bytes(int pass, int out_channels, int N, int C, int H, int W, int oh, int ow);

/* outs[h] <- y_h.  Every element of every output is written. */
int cspn_heads_forward(const void* x, const void* const* weights, void* const* outs, const int* out_channels, int n_heads, void* work,
                       int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream);

/* grad_x <- gx, all heads summed in one pass.  Every element is written.  A head whose output has no gradient is left out of the
 * arrays by the caller. */
int cspn_heads_backward_input(const void* const* grad_outs, const void* const* weights, const int* out_channels, int n_heads,
                              void* grad_x, void* work, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream);

/* grad_weights[h] <- gw_h for every head in the arrays. */
int cspn_heads_backward_weights(const void* x, const void* const* grad_outs, void* const* grad_weights, const int* out_channels,
                                int n_heads, void* work, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream);

/* CSPN_HEADS_ABI_VERSION the library was built from */
int cspn_heads_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_HEADS_H_ */

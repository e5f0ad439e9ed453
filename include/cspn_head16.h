/*
 * cspn_head16.h — C ABI of the fused output heads in half precision: the forward of cspn_heads.h (zero-insertion un-pooling by 2
 * followed by the bias-free 3x3 convolutions, pad 1, of several small heads over the same map) on fp16 tensors, on the fp16 matrix
 * cores.  Forward only, fp16 only; the gradients and the fp32 forward stay in cspn_heads.h.
 *
 * A header of its own with a version of its own.  The conventions are those of cspn_hip.h: 1 on success, 0 on failure +
 * cspn_last_error(); the caller owns every buffer, selects the device, and the library enqueues on the given stream without
 * allocating or synchronising.  No kernel waits for another workgroup, there are no atomics and no split sums: every call can be
 * captured in a graph.  Argument checks come before any launch.
 *
 * The arithmetic.  x: [N, C, H, W] fp16.  u is the un-pooled map cropped to oh x ow (1 <= oh <= 2H, 1 <= ow <= 2W):
 *     u[n, c, 2i, 2j] = x[n, c, i, j]  where 2i < oh and 2j < ow,   0 elsewhere
 * and head h with the filter w_h [O_h, C, 3, 3] gives y_h [N, O_h, oh, ow] fp16:
 *     y_h[n, o, Y, X] = sum_c sum_{ky, kx} w_h[o, c, ky, kx] u[n, c, Y + ky - 1, X + kx - 1]           (outside u: nothing)
 * u is never formed.  Output pixel (2i + a, 2j + b) reads
 *     (a, b) = (0, 0): tap (1,1) at (i, j)
 *              (0, 1): tap (1,0) at (i, j),  tap (1,2) at (i, j+1)
 *              (1, 0): tap (0,1) at (i, j),  tap (2,1) at (i+1, j)
 *              (1, 1): taps (0,0), (0,2), (2,0), (2,2) at (i, j), (i, j+1), (i+1, j), (i+1, j+1)
 * and a compact pixel with 2i >= oh or 2j >= ow contributes nothing (it is not read).
 *
 * Precision.  The filters are fp32 or fp16 (weight_dtype).  fp32 filters are rounded to fp16 once, to nearest even; fp16 filters
 * are taken as they are.  fp16 x fp16 products are exact in fp32, the accumulation is in fp32, and the result is rounded once to
 * fp16, to nearest even, a magnitude beyond 65504 + half an ulp becoming +-Inf.
 *
 * Determinism contract.  Every output element is one fixed chain: the channels in blocks of 32 in ascending order (the last block
 * filled with zeros); within a block the taps of the element's phase in the order listed above (the window from its upper left);
 * a (block, tap) step is one v_mfma_f32_16x16x32_f16, which adds the 32 exact products of the step to the fp32 accumulator in the
 * instruction's own fixed order.  A neighbour that the crop removed enters its step as 32 zeros.  The chain does not depend on the
 * element's place in a tile, on the frame's place in the batch or on N: a frame's bits are the same wherever it stands, and runs
 * repeat bit for bit.
 *
 * One difference from the reference, as in cspn_heads.h: a NaN or Inf in x[n, c, i, j] reaches the outputs whose window covers
 * (2i, 2j) only — a 3 x 3 block clipped by the crop.  The reference's un-pooling multiplies x by 0 at the inserted positions, so
 * there it also reaches the windows that cover the other three positions of its 2 x 2 block.
 *
 * Heads.  1 <= n_heads <= CSPN_HEAD16_MAX_HEADS, every O_h >= 1, their sum <= CSPN_HEAD16_MAX_OUT_CHANNELS.  weights[h], outs[h]:
 * host arrays of n_heads device pointers to contiguous tensors, aligned to their element size.  Where ow is even and every
 * output is 4-byte aligned a lane stores two adjacent columns at once; otherwise it stores 2 bytes at a time.  N <= 65535; x and
 * every output hold fewer than 2^31 elements.
 */
#ifndef CSPN_HEAD16_H_
#define CSPN_HEAD16_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_HEAD16_ABI_VERSION 1

#define CSPN_HEAD16_MAX_HEADS 4
#define CSPN_HEAD16_MAX_OUT_CHANNELS 16

/* the compact pixels of one workgroup tile, and the channels of one step of the chain */
#define CSPN_HEAD16_TILE_H 8
#define CSPN_HEAD16_TILE_W 32
#define CSPN_HEAD16_CHANNEL_BLOCK 32

/* Bytes of the `work` of one forward with `out_channels` output channels over all its heads and C input channels: the filters of
 * the call as fp16, [9 taps][16 rows][C rounded up to 32].  Callable without a device; 0 for a bad size.  work: 16-byte aligned;
 * its content on entry does not matter, every byte of it is written, and it may be reused once the call has run. */
size_t cspn_head16_workspace_bytes(int out_channels, int C);

/* outs[h] <- y_h.  Every element of every output is written.  weight_dtype: CSPN_F32 or CSPN_F16, the type of every weights[h]. */
int cspn_head16_forward(const void* x, const void* const* weights, int weight_dtype, void* const* outs, const int* out_channels,
                        int n_heads, void* work, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream);

/* CSPN_HEAD16_ABI_VERSION the library was built from */
int cspn_head16_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_HEAD16_H_ */

/*
 * cspn_convbn.h — C ABI of the encoder's convolutions: a bias-free k x k convolution (k = 1 or 3, pad k / 2, stride 1 or 2) over one
 * map, a per-channel affine map (an eval-mode batch norm), an optional residual and an optional ReLU, in one kernel.  Forward only;
 * fp32 or fp16 (bf16, other kernel sizes, strides, dilation, groups and a bias are out of scope).
 *
 *   Bottleneck   out = relu(bn1(conv1(x)));  out = relu(bn2(conv2(out)));  out = relu(bn3(conv3(out)) + shortcut)
 *   BasicBlock   out = relu(bn1(conv1(x)));  out = relu(bn2(conv2(out)) + shortcut)
 *   shortcut     x, or bn(conv1x1(x)) at the block's stride (no ReLU)
 *   the bridge   bn2(conv2(x)) between encoder and decoder (no ReLU)
 *
 * A header of its own with a version of its own, as cspn_uptail.h, whose conventions hold: 1 on success, 0 on failure +
 * cspn_last_error(); the caller owns every buffer, selects the device, and the library enqueues on the given stream without allocating
 * or synchronising.
 *
 * The arithmetic, for x [N, C, H, W], the filter w [O, C, k, k], stride s and the output [N, O, Ho, Wo] with Ho = (H - 1) / s + 1 and
 * Wo = (W - 1) / s + 1:
 *     acc[n, q, y, x] = sum_{ky, kx} sum_{c < C} w[q, c, ky, kx] x[n, c, s y + ky - k / 2, s x + kx - k / 2]
 *     out = act( fmaf(acc, scale[q], shift[q]) [+ r[n, q, y, x]] )
 * A neighbour outside the frame contributes nothing.  K walks (tap 0 .. k k - 1 row-major, then the channels ascending) in one order
 * whatever the tile.
 *   CSPN_F32  v_mfma_f32_32x32x2_f32: exact products, one fused multiply-add chain over K in fp32.  The epilogue is fmaf(acc, scale,
 *             shift), then + r as an add of its own, then max(y, 0) (NaN stays NaN): the roundings of the stock eval path, whose
 *             convolution may sum in another order.
 *   CSPN_F16  v_mfma_f32_32x32x16_f16: x, r and the packed filter are fp16, products are exact, the sum is kept in fp32 in blocks of
 *             16 channels, and the whole epilogue is fp32.  The result is rounded to fp16 ONCE.  The stock half path rounds after the
 *             convolution, after the batch norm and after the add.
 * For k = 3, s = 1 this is the one-map case of cspn_uptail_forward (Cb = 0): the same K order through the same instructions, the
 * same bits.
 *
 * Determinism contract, as cspn_uptail.h: every output element is ONE chain over K through the same instruction sequence whichever
 * tile it falls into; no split-K, no atomic, no wait for another workgroup.  A frame's bits do not depend on N or on its place in
 * the batch, equal arguments give equal bits run after run, and every call can be captured in a graph.
 *
 * Not part of this family: an instance with a 64-row M tile for the 64-channel convolutions of layer1 (half of every 128-row M tile
 * is padding there), the 7 x 7 stem (its 4 channels would be padded to 32) and the max-pool.
 */
#ifndef CSPN_CONVBN_H_
#define CSPN_CONVBN_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_CONVBN_ABI_VERSION 1

/* Bytes of the packed filter (callable without a device; 0 for a bad size, k or dtype, or a packed form of 2^31 elements or more):
 * k k * roundup(C, 32) * roundup(O, 128) elements of `dtype`.  Per tap a zero-filled matrix of the packed channels by the output
 * channels rounded up to 128 — filter-contiguous for CSPN_F32, channel-contiguous for CSPN_F16. */
size_t cspn_convbn_packed_bytes(int O, int C, int k, int dtype);

/* packed <- w, a contiguous [O, C, kh, kw] tensor of `src_dtype`.  CSPN_F32 -> CSPN_F32 and CSPN_F16 -> CSPN_F16 copy;
 * CSPN_F32 -> CSPN_F16 rounds to nearest even once.  Refused: kh != kw, a k other than 1 or 3, any other pair of dtypes.  packed:
 * 16-byte aligned, cspn_convbn_packed_bytes(O, C, kh, dst_dtype) bytes.  Once per version of the weights. */
int cspn_convbn_pack(const void* w, int O, int C, int kh, int kw, int src_dtype, int dst_dtype, void* packed, cspn_stream_t stream);

/* out <- [N, O, Ho, Wo] (contiguous, `dtype`); x: [N, C, H, W], residual: [N, O, Ho, Wo] or null, all contiguous `dtype`; packed: made
 * for (O, C, k, dtype).  scale, shift: fp32 [O], both or neither.  relu: nonzero for max(y, 0).  Every element of out is written and
 * nothing else; out may not overlap an input.  Refused, before any launch: a null x, packed or out, packed not 16-byte aligned, scale
 * without shift, a k other than 1 or 3, a stride other than 1 or 2, a tensor of 2^31 elements or more, a dtype other than CSPN_F32 /
 * CSPN_F16. */
int cspn_convbn_forward(const void* x, const void* packed, const float* scale, const float* shift, const void* residual, int relu,
                        void* out, int dtype, int N, int C, int O, int H, int W, int k, int stride, cspn_stream_t stream);

/* CSPN_CONVBN_ABI_VERSION the library was built from */
int cspn_convbn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_CONVBN_H_ */

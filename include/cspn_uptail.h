/*
 * cspn_uptail.h — C ABI of the 3x3 tail of the decoder blocks: a bias-free 3x3 convolution (pad 1, stride 1) over the channels of one
 * or two maps taken side by side, a per-channel affine map (an eval-mode batch norm), an optional residual and an optional ReLU, in
 * one kernel.  Forward only; fp32 or fp16 (bf16, other kernel sizes, strides, dilation and a bias are out of scope).
 *
 *   Gudi_UpProj_Block      out = relu(bn2(conv2(out)) + shortcut)
 *   Gudi_UpProj_Block_Cat  out = relu(bn1_1(conv1_1(cat(out, side))));  out = relu(bn2(conv2(out)) + shortcut)
 *
 * A header of its own with a version of its own, as cspn_upconv.h and cspn_uphalf.h, whose conventions hold: 1 on success, 0 on
 * failure + cspn_last_error(); the caller owns every buffer, selects the device, and the library enqueues on the given stream
 * without allocating or synchronising.
 *
 * The arithmetic, for the filter w [O, Ca + Cb, 3, 3] and the maps a [N, Ca, H, W] and b [N, Cb, H, W] (b absent: Cb = 0):
 *     acc[n, q, y, x] = sum_{ky, kx} ( sum_{c < Ca} w[q, c, ky, kx] a[n, c, y + ky - 1, x + kx - 1]
 *                                    + sum_{c < Cb} w[q, Ca + c, ky, kx] b[n, c, y + ky - 1, x + kx - 1] )
 *     out = act( fmaf(acc, scale[q], shift[q]) [+ r[n, q, y, x]] )
 * A neighbour outside the frame contributes nothing.  The concatenation is never formed.  K walks (tap 0 .. 8 row-major, then the
 * channels ascending, a before b) in one order whatever the tile.
 *   CSPN_F32  v_mfma_f32_32x32x2_f32: exact products, one fused multiply-add chain over K in fp32.  The epilogue is fmaf(acc, scale,
 *             shift), then + r as an add of its own, then max(y, 0) (NaN stays NaN): the roundings of the stock eval path, whose
 *             convolution may sum in another order.
 *   CSPN_F16  v_mfma_f32_32x32x16_f16: a, b, r and the packed filter are fp16, products are exact, the sum is kept in fp32 in blocks
 *             of 16 channels, and the whole epilogue is fp32.  The result is rounded to fp16 ONCE.  The stock half path rounds three
 *             times: after the convolution, after the batch norm and after the add.
 *
 * Determinism contract, as cspn_upconv.h: every output element is ONE chain over K through the same instruction sequence whichever
 * tile it falls into; no split-K, no atomic, no wait for another workgroup.  A frame's bits do not depend on N or on its place in
 * the batch, equal arguments give equal bits run after run, and every call can be captured in a graph.
 */
#ifndef CSPN_UPTAIL_H_
#define CSPN_UPTAIL_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_UPTAIL_ABI_VERSION 1

/* Bytes of the packed filter (callable without a device; 0 for a bad size or dtype, or a packed form of 2^31 elements or more):
 * 9 * (roundup(Ca, 32) + roundup(Cb, 32)) * roundup(O, 128) elements of `dtype`.  Per tap a zero-filled matrix of the packed channels
 * by the output channels rounded up to 128 — filter-contiguous for CSPN_F32, channel-contiguous for CSPN_F16 — in which the
 * channels of b start at roundup(Ca, 32): every block of 32 packed channels belongs to one map. */
size_t cspn_uptail_packed_bytes(int O, int Ca, int Cb, int dtype);

/* packed <- w, a contiguous [O, Ca + Cb, kh, kw] tensor of `src_dtype`.  CSPN_F32 -> CSPN_F32 and CSPN_F16 -> CSPN_F16 copy;
 * CSPN_F32 -> CSPN_F16 rounds to nearest even once.  Refused: a filter that is not 3 x 3, any other pair of dtypes.  packed:
 * 16-byte aligned, cspn_uptail_packed_bytes(O, Ca, Cb, dst_dtype) bytes.  Once per version of the weights. */
int cspn_uptail_pack(const void* w, int O, int Ca, int Cb, int kh, int kw, int src_dtype, int dst_dtype, void* packed,
                     cspn_stream_t stream);

/* out <- [N, O, H, W] (contiguous, `dtype`); a: [N, Ca, H, W], b: [N, Cb, H, W] or null with Cb = 0, residual: [N, O, H, W] or null,
 * all contiguous `dtype`; packed: made for (O, Ca, Cb, dtype).  scale, shift: fp32 [O], both or neither.  relu: nonzero for max(y, 0).
 * Every element of out is written and nothing else; out may not overlap an input.  Refused, before any launch: a null a, packed or
 * out, b given with Cb = 0 or missing with Cb > 0, packed not 16-byte aligned, scale without shift, a tensor of 2^31 elements or
 * more, a dtype other than CSPN_F32 / CSPN_F16. */
int cspn_uptail_forward(const void* a, const void* b, const void* packed, const float* scale, const float* shift, const void* residual,
                        int relu, void* out, int dtype, int N, int Ca, int Cb, int O, int H, int W, cspn_stream_t stream);

/* CSPN_UPTAIL_ABI_VERSION the library was built from */
int cspn_uptail_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_UPTAIL_H_ */

/*
 * cspn_uphalf.h — C ABI of the fused decoder-block heads in half precision: the computation of cspn_upconv.h (zero-insertion
 * un-pooling by 2, the one or two bias-free 5x5 convolutions (pad 2) of a decoder block, a per-channel affine map and a ReLU on the
 * leading channels, straight from the compact map) with fp16 activations, fp16 filters and fp16 outputs on the fp16 matrix cores.
 * Forward only.  fp16 only: bf16 is out of scope (it would be a third packed form and a second operand type; nothing in the
 * package runs in bf16).
 *
 * A header of its own with a version of its own, as cspn_upconv.h: neither CSPN_ABI_VERSION (cspn_hip.h) nor CSPN_UPCONV_ABI_VERSION
 * moves, and cspn_upconv_* keeps refusing everything but fp32.  The conventions are those of cspn_upconv.h: 1 on success, 0 on
 * failure + cspn_last_error(); the caller owns every buffer, selects the device, and the library enqueues on the given stream
 * without allocating or synchronising.
 *
 * The arithmetic.  Geometry, phases, taps and the missing-neighbour rule are those of cspn_upconv.h:
 *     acc[n, q, Y, X] = sum_{ky, kx} sum_c w[q, c, ky, kx] u[n, c, Y + ky - 2, X + kx - 2]
 *     y[n, q, Y, X]   = fp16(act_q(fmaf(acc, scale[q], shift[q])))      (scale, shift absent: fp16(act_q(acc)))
 * x and w are fp16; a product of two fp16 values is exact in fp32.  The sum is accumulated in fp32 by
 * v_mfma_f32_32x32x16_f16: K walks (tap, channel) in the packed order — the taps of the phase's window from the upper left, the
 * channels of a tap ascending — in blocks of 16, one instruction per block; the order and the rounding of the 16 additions inside
 * a block are the hardware's.  The epilogue is fp32: one fused multiply-add with scale and shift, then max(y, 0) for q <
 * relu_channels (NaN stays NaN).  After the epilogue there is ONE conversion to fp16, round to nearest even; a magnitude beyond the
 * fp16 range becomes +-Inf, as the conversion defines.
 *
 * Determinism contract.  Every output element is ONE chain over K through the same instruction sequence, whichever tile it falls
 * into (a missing neighbour and the zero padding of the packed filters enter as products with 0).  There is no split-K, no atomic,
 * no wait for another workgroup and no device-scope flag.  So a frame's bits do not depend on N or on its place in the batch, equal
 * arguments give equal bits run after run, and every call can be captured in a graph.
 *
 * The difference from the reference is the one cspn_upconv.h states: a NaN or Inf in x[n, c, i, j] reaches the outputs whose window
 * covers (2i, 2j) only.
 */
#ifndef CSPN_UPHALF_H_
#define CSPN_UPHALF_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_UPHALF_ABI_VERSION 1

#define CSPN_UPHALF_MAX_FILTERS 2

/* Bytes of the packed filters of `out_channels` flat output channels over C input channels (callable without a device; 0 for a bad
 * size, or one whose packed form has 2^31 elements or more): 25 * roundup(C, 32) * roundup(out_channels, 128) * 2.  The packed form
 * holds, for each of the 25 taps in phase-major order, out_channels rounded up to 128 rows of C rounded up to 32 fp16 values,
 * channel-contiguous and zero-filled: 8 consecutive channels of a row are one 16-byte operand fragment. */
size_t cspn_uphalf_packed_bytes(int out_channels, int C);

/* packed <- weights[0 .. n_filters), each a contiguous [out_channels[k], C, kh, kw] tensor of `src_dtype`, in the order the forward
 * walks them.  CSPN_F32 sources are rounded to fp16 once, to nearest even; CSPN_F16 sources are copied.  Once per version of the
 * weights, not once per call.  Refused: n_filters outside [1, CSPN_UPHALF_MAX_FILTERS], a filter that is not 5 x 5, any other
 * src_dtype.  packed: 16-byte aligned, cspn_uphalf_packed_bytes(sum of out_channels, C) bytes. */
int cspn_uphalf_pack(const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, int src_dtype,
                     void* packed, cspn_stream_t stream);

/* outs[k] <- [N, out_channels[k], oh, ow] (contiguous fp16) for the n_outs filters `packed` was made from; x: [N, C, H, W]
 * contiguous fp16.  scale, shift: fp32 [sum of out_channels], both or neither.  relu_channels in [0, sum of out_channels].  Every
 * element of every output is written and nothing else.  Refused, before any launch: oh outside [1, 2H] or ow outside [1, 2W], x or
 * an output of 2^31 elements or more, a null pointer, scale without shift, relu_channels out of range. */
int cspn_uphalf_forward(const void* x, const void* packed, const void* scale, const void* shift, int relu_channels, void* const* outs,
                        const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream);

/* CSPN_UPHALF_ABI_VERSION the library was built from */
int cspn_uphalf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_UPHALF_H_ */

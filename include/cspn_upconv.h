/*
 * cspn_upconv.h — C ABI of the fused decoder-block heads: zero-insertion un-pooling by 2 followed by the one or two bias-free 5x5
 * convolutions (pad 2) every decoder block starts with, a per-channel affine map (the batch norms in eval mode) and a ReLU on the
 * leading channels, computed straight from the compact map (paths relative to the reference repo):
 *   network/unet_ours.py:160-248      UpProj_Block, Simple_Gudi_UpConv_Block, Gudi_UpProj_Block, Gudi_UpProj_Block_Cat
 *   network/unet_cspn_nyu.py:226-300  the same blocks of the config-5 model
 * forward only, fp32 tensors only; the products exact in fp32 or, by the forward's dtype, split into bf16 terms (below).
 *
 * A header of its own with a version of its own, as cspn_heads.h: CSPN_ABI_VERSION (cspn_hip.h) does not move.  The conventions are
 * those of cspn_hip.h: 1 on success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects the device, and the
 * library enqueues on the given stream without allocating or synchronising.  No kernel waits for another workgroup, there is no
 * split-K, no device-scope flag and no atomic: every call can be captured in a graph.
 *
 * The arithmetic.  x: [N, C, H, W].  u is the un-pooled map cropped to oh x ow (1 <= oh <= 2H, 1 <= ow <= 2W):
 *     u[n, c, 2i, 2j] = x[n, c, i, j]  where 2i < oh and 2j < ow,   0 elsewhere
 * The one or two filters w_k [O_k, C, 5, 5] are run as one list of O_1 + O_2 "flat" output channels q:
 *     acc[n, q, Y, X] = sum_{ky, kx} sum_c w[q, c, ky, kx] u[n, c, Y + ky - 2, X + kx - 2]                  (outside u: nothing)
 *     y[n, q, Y, X]   = acc * scale[q] + shift[q]   (scale, shift absent: acc),   then max(y, 0) where q < relu_channels
 * u is never formed.  Output pixel (2i + a, 2j + b) meets x only through the taps with a + ky and b + kx even: compact rows
 * i - 1, i, i + 1 for a = 0 and i, i + 1 for a = 1, likewise the columns — 9, 6, 6 and 4 products per channel for the four phases
 * (a, b), 25 per compact pixel where the un-pooled map costs 100.  A neighbour outside [0, ceil(oh / 2)) x [0, ceil(ow / 2)) is
 * missing (the frame's edge, or a compact pixel the crop removed) and contributes nothing.
 *
 * Each phase is an implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered chain of fused multiply-adds, one
 * rounding per product): M = flat channels, N = the phase's pixels (n, i, j) over the whole batch, K = (tap, channel) — the taps
 * of the phase's window from the upper left, the channels of a tap ascending.
 *
 * Determinism contract.  Every output element is ONE chain over K in that order, whichever tile it falls into (a missing neighbour
 * and the zero padding of the packed filters enter as products with 0).  So a frame's bits do not depend on its place in the
 * batch or on N, and equal arguments give equal bits run after run.
 *
 * One difference from the reference: a NaN or Inf in x[n, c, i, j] reaches the outputs whose window covers (2i, 2j) only.  The
 * reference's un-pooling multiplies x by 0 at the inserted positions, so there it also reaches the windows that cover the other
 * three positions of its 2 x 2 block.
 *
 * The split products (dtype CSPN_UPCONV_F32_BF16X3 of cspn_upconv_forward).  fp32 x, fp32 outputs and the same
 * fp32 pack, but the products run on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16), which gfx950 runs at 16 times the rate of
 * the fp32 instruction.  Every fp32 value v, of x and of the filters, is split in registers into three bf16 terms
 *     v1 = bf16(v),   v2 = bf16(v - v1),   v3 = bf16(v - v1 - v2)        conversions round to nearest even
 * Both subtractions are exact in fp32, and v1 + v2 + v3 == v: three 8-bit significands cover the 24 bits of v.  A product x w is
 * replaced by the six terms x_i w_j with i + j <= 4 — (1,1) (1,2) (2,1) (1,3) (2,2) (3,1) — each of them exact in fp32; the three
 * left out, x_2 w_3 + x_3 w_2 + x_3 w_3, are at most (2^-23 + 2^-32) |x w|.  The terms are summed in fp32 by the matrix
 * instruction.  K = (tap, channel) runs in the packed order in blocks of 16 channels (the channels of a tap rounded up to 32, the
 * padding entering as zeros): per block the six terms in the order above, as (filter term, pixel term), one instruction each;
 * the order of the 16 products inside an instruction is the hardware's and not documented, so an fp32 addition is taken to be
 * faithful (error below one ulp), not correctly rounded.  For an output with A = sum |w x| over its window:
 *     |acc - exact| <= gamma'_n A + (2^-23 + 2^-32) A,     gamma'_n = n u' / (1 - n u'),  u' = 2^-23,  n = 6 taps C
 * The epilogue is the one above — fmaf(acc, scale, shift), the ReLU below relu_channels, a NaN stays a NaN — and so are the
 * geometry, the phases, the missing-neighbour rule and the determinism contract: one chain per output element, no split-K, no
 * atomics, bits independent of N and of the frame's place, runs repeat, the launch can be captured.  Inputs whose products and
 * sums are exact in this form (integers; values with few significant bits) give the bits of the exact kernel.
 * Outside the normal range:
 *   - |v| >= 2^128 - 2^119 (above bf16's largest finite value 2^128 - 2^120 by half a unit or more) rounds to v1 = +-Inf and is
 *     treated as the Inf below, although v is finite in fp32.
 *   - +-Inf in x or in a filter: v1 = +-Inf, v - v1 = NaN, so v2 and v3 are NaN (there is no guard).  Every output whose window
 *     covers the value is NaN, and no other output is touched.  The exact kernel gives +-Inf or NaN at these outputs (and 0 where a
 *     ReLU meets -Inf): every output it makes non-finite is non-finite here too, but an Inf there is a NaN here.  A NaN behaves as
 *     in the exact kernel.
 *   - a term below bf16's normal range (2^-126): v3 is a multiple of ulp(v), so for |v| >= 2^-103 every non-zero term is a normal
 *     bf16 number and the split is exact.  Below that, v2 or v3 may be subnormal; the conversion keeps subnormals but the matrix
 *     cores may flush them, and a product of two small terms may underflow fp32.  The result then loses relative, not absolute,
 *     accuracy: the error added per product is below 2^-103 |w| (|x| below the limit) or 2^-103 |x| (|w| below it).
 */
#ifndef CSPN_UPCONV_H_
#define CSPN_UPCONV_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_UPCONV_ABI_VERSION 1

#define CSPN_UPCONV_MAX_FILTERS 2

/* A `dtype` of cspn_upconv_forward beside CSPN_F32: fp32 tensors, the products split into bf16 terms (see above).  Defined here and
 * not with CSPN_F32 / CSPN_F16 in cspn_hip.h: no other entry point takes it. */
#define CSPN_UPCONV_F32_BF16X3 2

/* Bytes of the packed filters of `out_channels` flat output channels over C input channels (callable without a device; 0 for a bad
 * size, or one whose packed form has 2^31 elements or more).  The packed form holds, for each of the 25 taps in phase-major order,
 * C rounded up to 32 rows of out_channels rounded up to 128 values, zero-filled. */
size_t cspn_upconv_workspace_bytes(int out_channels, int C);

/* packed <- weights[0 .. n_filters), each a contiguous [out_channels[k], C, kh, kw] tensor of `dtype`, in the order the forward walks
 * them.  Once per version of the weights, not once per call.  Refused: n_filters outside [1, CSPN_UPCONV_MAX_FILTERS], a filter
 * that is not 5 x 5, any dtype but CSPN_F32.  packed: 16-byte aligned, cspn_upconv_workspace_bytes(sum of out_channels, C) bytes. */
int cspn_upconv_pack(const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, int dtype, void* packed,
                     cspn_stream_t stream);

/* outs[k] <- [N, out_channels[k], oh, ow] (contiguous, fp32) for the n_outs filters `packed` was made from.  scale, shift:
 * fp32 [sum of out_channels], both or neither.  relu_channels in [0, sum of out_channels].  Every element of every output is
 * written and nothing else.  dtype: CSPN_F32 — exact fp32 products — or CSPN_UPCONV_F32_BF16X3 — the split products, on the same
 * fp32 x, pack and outputs and under the same argument rules.  Refused: any other dtype, oh outside [1, 2H] or ow outside
 * [1, 2W], x or an output of 2^31 elements or more. */
int cspn_upconv_forward(const void* x, int dtype, const void* packed, const void* scale, const void* shift, int relu_channels,
                        void* const* outs, const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow,
                        cspn_stream_t stream);

/* CSPN_UPCONV_ABI_VERSION the library was built from */
int cspn_upconv_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_UPCONV_H_ */

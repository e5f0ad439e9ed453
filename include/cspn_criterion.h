/*
 * cspn_criterion.h — C ABI of the training criteria of libcspn_hip.so (paths relative to the reference repo):
 *   libs/criterion/criteria.py:14-39    MaskedMSELoss / MaskedL1Loss   mean over target > 0 of (t - p)^2 / |t - p|
 *   libs/criterion/criteria.py:91-107   L1_log                         mean over target > 0 of |log t - log p|
 * forward and backward, as kernels without atomics, without a host synchronisation and capturable in a graph (the reference's
 * `diff[valid_mask].mean()` calls nonzero: a device-to-host copy on every step).
 *
 * A header of its own with a version of its own: CSPN_ABI_VERSION (cspn_hip.h) does not move, and neither does the digest of
 * cspn_hip.h that measured HBM traffic of the benchmarked kernels is pinned to.  The conventions are those of cspn_hip.h: 1 on
 * success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects the device, and the library enqueues on the
 * given stream without synchronising.
 *
 * pred / target: n contiguous elements each, aligned to their element size (a 16-byte aligned base is loaded 16 bytes at a time,
 * any other base element by element: same values, same arithmetic, same bits).  A pixel is VALID when target > 0 (a NaN target
 * is not).
 *
 * dtype: CSPN_F32 only; CSPN_F16 fails with a message.  This is on purpose: the criterion is a mean, so the gradient of a valid
 * pixel is g / count — with ~10^6 valid pixels about 1e-6, below the smallest fp16 subnormal (6e-8 is the smallest, 1e-6 keeps
 * four bits).  A half gradient plane would be zeros and noise; cast the prediction to fp32 in front of the criterion instead.
 *
 * Determinism contract.  The state is a function of (pred, target, kind, n) only — not of the shape n was folded from, not of
 * the addresses, not of what ran before:
 *   - the n elements are cut into units of 16 bytes (4 floats), unit u = elements [4u, 4u + 4); S = a function of n slices;
 *   - unit u belongs to slice (u / 256) % S, thread u % 256; a thread adds its units in increasing u, fp32 over a group of 4
 *     units (16 pixels), groups into fp64; the 64 lanes of a wavefront and the 4 wavefronts of a slice are added in a fixed order;
 *   - cspn_criterion_forward's second launch adds the S slices in an order that depends on S only.
 * The backward is element-wise.  The one implementation of this order, for this header and for cspn_losses.h, is
 * csrc/cspn_loss_units.hpp.
 */
#ifndef CSPN_CRITERION_H_
#define CSPN_CRITERION_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_CRITERION_ABI_VERSION 1

/* the per-pixel term that is averaged over the valid pixels */
enum { CSPN_LOSS_L1 = 0, CSPN_LOSS_L2 = 1, CSPN_LOSS_L1_LOG = 2 };

/* The device state one forward leaves for its backward: 32 bytes, 8-byte aligned.
 *   offset  0  float   loss       (float)(sum / count); no valid pixel: 0 / 0 = NaN, the reference's mean over an empty selection
 *   offset  4  float   1 / count  (+inf when count == 0; no pixel uses it then)
 *   offset  8  double  sum        of the kind's term over the valid pixels
 *   offset 16  double  count      of valid pixels
 *   offset 24  reserved (written as 0)                                                                                            */
#define CSPN_CRITERION_STATE_BYTES 32

/* Bytes of `work` for n elements (2 doubles per slice; callable without a device; 0 for n < 1). */
size_t cspn_criterion_workspace_bytes(size_t n);

/* Two launches: per-slice partial sums into `work` (8-byte aligned), then one workgroup that adds them and OVERWRITES `state`.
 * Nothing is read back to the host. */
int cspn_criterion_forward(const void* pred, const void* target, int dtype, int kind, size_t n,
                           void* work, void* state, cspn_stream_t stream);

/* One streaming launch: grad_pred [n] (fp32, every element written) from pred, target, the state of the forward on the same
 * (pred, target, kind) and the DEVICE scalar *grad_loss = g, the incoming gradient of the loss (not always 1: a wrapper may
 * weight the loss):
 *     0                                      where target <= 0 or target is NaN
 *     g / count * -sign(t - p)               CSPN_LOSS_L1       (sign(0) = sign(NaN) = 0, as the backward of abs)
 *     g / count * 2 (p - t)                  CSPN_LOSS_L2
 *     g / count * -sign(log t - log p) / p   CSPN_LOSS_L1_LOG   (p == 0: -inf; p < 0: log p is NaN, sign 0, gradient 0)
 * count == 0 gives all zeros. */
int cspn_criterion_backward(const void* pred, const void* target, int dtype, int kind, size_t n,
                            const void* state, const float* grad_loss, void* grad_pred, cspn_stream_t stream);

/* CSPN_CRITERION_ABI_VERSION the library was built from */
int cspn_criterion_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_CRITERION_H_ */

/*
 * cspn_losses.h — C ABI of the rest of the reference's working criteria in libcspn_hip.so (paths relative to the reference repo):
 *   libs/criterion/criteria.py:42-64    berHuLoss   reverse Huber with the threshold c = 0.2 * max(pred - target)
 *   libs/criterion/criteria.py:79-88    L1          mean |10 r - 10 f|
 *   libs/criterion/criteria.py:145-152  GradLoss    mean |t - p|
 *   libs/criterion/criteria.py:133-142  RMSE        sqrt(mean (10 r - 10 f)^2)
 *   libs/criterion/criteria.py:67-76    RMSE_log    sqrt(mean (log r - log f)^2)
 * forward and backward, as kernels without atomics, without a host synchronisation and capturable in a graph.  BerHu(threshold)
 * (criteria.py:110-130) and NormalLoss (:155-167) are not here: both raise in the reference before they compute anything.
 *
 * A header of its own with a version of its own: neither CSPN_ABI_VERSION (cspn_hip.h) nor CSPN_CRITERION_ABI_VERSION
 * (cspn_criterion.h) moves.  The conventions are those of cspn_criterion.h: 1 on success, 0 on failure + cspn_last_error(); the
 * caller owns every buffer, selects the device, and the library enqueues on the given stream without synchronising; n contiguous
 * fp32 elements per plane, aligned to their element size (a 16-byte aligned base is loaded 16 bytes at a time, any other base
 * element by element: same values, same arithmetic, same bits).  dtype: CSPN_F32 only, CSPN_F16 fails — every loss here is a
 * mean, and g / n is below what fp16 can hold (cspn_criterion.h).
 *
 * Determinism contract: the state is a function of the n values of both planes, the loss and n only.  Sums follow the slice
 * discipline of cspn_criterion.h (units of 16 bytes, unit u -> slice (u / 256) % S, fp32 over 16 pixels, then fp64, fixed orders),
 * through the same code: csrc/cspn_loss_units.hpp.
 * berHu's maximum is combined with a NaN-propagating maximum, whose result does not depend on an order.
 *
 * berHu, every operation in fp32 as written:
 *     e = pred - target over ALL n elements;  m = max e (NaN if any e is NaN);  c = 0.2f * m
 *     valid: target > 0;  d = |target - pred|;  Huber set: valid and d > c  (empty when c is NaN, every valid pixel when c < 0)
 *     loss = (sum_valid d + sum_huber d^2) / (n_valid + n_huber), the sums in fp64;  no valid pixel: 0 / 0 = NaN
 * m, c, d and the comparison are exact fp32 operations, so the Huber set is the reference's set bit for bit.
 */
#ifndef CSPN_LOSSES_H_
#define CSPN_LOSSES_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_LOSSES_ABI_VERSION 1

/* the unmasked means: the loss over all n elements of (fake, real) */
enum { CSPN_MEAN_L1 = 0, CSPN_MEAN_GRAD = 1, CSPN_MEAN_RMSE = 2, CSPN_MEAN_RMSE_LOG = 3 };

/* The device state one forward leaves for its backward: 48 bytes, 8-byte aligned.
 *   offset  0  float   loss
 *   offset  4  float   factor     berHu: 1 / (n_valid + n_huber); L1 / GRAD: 1 / n; RMSE / RMSE_LOG: 1 / (n * loss)
 *   offset  8  float   c          berHu's threshold (0 for the unmasked means)
 *   offset 12  reserved (written as 0)
 *   offset 16  double  sum        berHu: sum_valid d; unmasked: the sum of the kind's term (|x| or x^2)
 *   offset 24  double  sum2       berHu: sum_huber d^2 (else 0)
 *   offset 32  double  n_valid    berHu: valid pixels; unmasked: n
 *   offset 40  double  n_huber    berHu: pixels in the Huber set (else 0)                                                       */
#define CSPN_LOSSES_STATE_BYTES 48

/* Bytes of `work` for n elements, enough for either forward (5 doubles per slice; callable without a device; 0 for n < 1). */
size_t cspn_losses_workspace_bytes(size_t n);

/* Three launches: per slice {max e, sum_valid d, n_valid}; per slice {sum_huber d^2, n_huber}, every workgroup reducing the
 * slice maxima to c itself first; one workgroup that adds the slices and OVERWRITES `state`.  work: 8-byte aligned. */
int cspn_berhu_forward(const void* pred, const void* target, int dtype, size_t n, void* work, void* state, cspn_stream_t stream);

/* One streaming launch: grad_pred [n] (fp32, every element written) from pred, target, the state of the forward on the same
 * planes and the DEVICE scalar *grad_loss = g:
 *     0                                                          where target <= 0 or target is NaN
 *     g * factor * -sign(t - p) * (1 + 2 d [d > c])              elsewhere (sign(0) = sign(NaN) = 0)
 * c is used in a comparison only: no gradient passes through the maximum.  No valid pixel: all zeros. */
int cspn_berhu_backward(const void* pred, const void* target, int dtype, size_t n, const void* state, const float* grad_loss,
                        void* grad_pred, cspn_stream_t stream);

/* Two launches: per-slice sums of the kind's term, then one workgroup that OVERWRITES `state`.
 *     CSPN_MEAN_L1        x = 10 r - 10 f      loss = mean |x|
 *     CSPN_MEAN_GRAD      x = r - f            loss = mean |x|
 *     CSPN_MEAN_RMSE      x = 10 r - 10 f      loss = sqrt(mean x^2)
 *     CSPN_MEAN_RMSE_LOG  x = log r - log f    loss = sqrt(mean x^2)   (an r < 0 anywhere: NaN) */
int cspn_mean_loss_forward(const void* fake, const void* real, int dtype, int kind, size_t n, void* work, void* state,
                           cspn_stream_t stream);

/* One streaming launch: grad_fake [n] (fp32, every element written), s = g * factor:
 *     CSPN_MEAN_L1        -10 sign(x) s        CSPN_MEAN_GRAD      -sign(x) s          (sign(0) = sign(NaN) = 0)
 *     CSPN_MEAN_RMSE      -10 x s              CSPN_MEAN_RMSE_LOG  -x s / f
 * RMSE / RMSE_LOG with loss == 0: s = inf and every element is 0 * inf = NaN, as the reference gives. */
int cspn_mean_loss_backward(const void* fake, const void* real, int dtype, int kind, size_t n, const void* state,
                            const float* grad_loss, void* grad_fake, cspn_stream_t stream);

/* CSPN_LOSSES_ABI_VERSION the library was built from */
int cspn_losses_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_LOSSES_H_ */

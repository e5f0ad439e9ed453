/*
 * cspn_transform.h — C ABI of the NYU train / val transforms of libcspn_hip.so (paths relative to the reference repo):
 *   dataloaders/nyu_dataloader/nyu_dataloader.py:13-44   NYUDataset.train_transform / val_transform
 *   dataloaders/nyu_dataloader/transforms.py             Resize, Rotate, CenterCrop, HorizontalFlip, ColorJitter, adjust_*
 *   dataloaders/nyu_dataloader/dataloader.py:54          ColorJitter(0.4, 0.4, 0.4)
 * for a batch of RAW frames that already sits on the device: uint8 RGB [B, 3, H, W] + fp32 depth [B, 1, H, W] in, the cropped fp32
 * RGB + depth pair out.  No atomics, no wait between workgroups, nothing read back to the host, capturable in a graph; equal bits run
 * after run; a frame's output does not depend on its place in the batch or on the batch size.
 *
 * A header of its own with a version of its own, as cspn_sparsify.h: CSPN_ABI_VERSION (cspn_hip.h) does not move.  The conventions are
 * those of cspn_hip.h: 1 on success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects the device, and the
 * library enqueues on the given stream without synchronising.
 *
 * The reference's geometry is nearest-neighbour throughout, so an output pixel is a COPY of one raw pixel (or a zero), and the
 * outputs can equal the reference's bit for bit.  What has to be reproduced for that (all index arithmetic in fp64, every operation
 * rounded on its own — no fused multiply-add):
 *   Resize(f)      output size (int)(n_in * f); the source index table is Pillow's RUNNING SUM a = n_in / n_out, o = a * 0.5,
 *                  tab[i] = (int)o, o += a — not floor((i + 0.5) * a), which differs at 640 -> 333 and 480 -> 250.  A table is built
 *                  serially by one thread, from index 0.
 *   Rotate(angle)  scipy.ndimage.rotate(order=0, prefilter=False, reshape=False) on the h1 x w1 image: t = angle * (pi / 180),
 *                  M = [[cos t, sin t], [-sin t, cos t]], ctr = (h1/2 - 0.5, w1/2 - 0.5), off = ctr - M ctr; for output (y, x)
 *                  cy = off0 + y*M00, cy += x*M01, cx = off1 + y*M10, cx += x*M11; source (floor(cy + 0.5), floor(cx + 0.5));
 *                  zero-filled unless 0 <= cy <= h1 - 1 and 0 <= cx <= w1 - 1.
 *   CenterCrop     i0 = round((h2 - oh) / 2.), j0 likewise, ties to even.  HorizontalFlip mirrors the cropped columns.
 *   depth          train: depth / (float)s in fp32, then scipy's order-0 sum `t = 0; t += v` — a -0 leaves as +0, every other value
 *                  (Inf, NaN, negative, denormal) as it is; val: the raw 32-bit word.
 *   ColorJitter    on the cropped uint8 RGB, the three ops in the drawn order, each Pillow's blend(degenerate, img, f) with f a C
 *                  float: t = (float)deg + f * (float)(img - deg), two roundings; 0 if t <= 0, 255 if t >= 255, else (uint8)t.
 *                  Degenerates: brightness 0; saturation L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16; contrast the constant
 *                  (int)(sum(L) / n + 0.5) over the WHOLE frame as it stands when contrast is applied (fp64).
 *   output         rgb = (float)((double)v / 255.0).
 *
 * Per-frame parameters: a DEVICE fp64 [B, 8] row per frame,
 *     [0] s   [1] angle in degrees   [2] flip (!= 0)   [3] brightness   [4] contrast   [5] saturation factor
 *     [6] order code 0..5 = the lexicographic permutations of (brightness, contrast, saturation); anything else: no jitter   [7] reserved
 * Precondition: finite values, (int)(h1 * s) >= oh, (int)(w1 * s) >= ow.  Parameters live on the device and cannot be validated on the
 * host: whatever they hold, every table entry and every source coordinate is clamped before it is used as an address (and the second
 * size is capped at CSPN_TRANSFORM_MAX_SECOND, which bounds the serial table loop).  A bad row gives a meaningless frame, never an
 * out-of-range access, and touches no other frame.
 *
 * Launches.  CSPN_TRANSFORM_VAL: tables (the first resize's two tables) + gather.  CSPN_TRANSFORM_TRAIN: tables (the first tables and,
 * per frame, the second tables already cropped and flipped, M, off, the factors as floats) + gather (one thread per output pixel;
 * writes depth; RGB straight out when the frame has no jitter, else the ops in front of contrast, the packed pixel and one integer
 * partial sum of L per workgroup) + finish (adds the frame's partials — integers, any order gives this sum —, forms the contrast
 * constant, applies contrast and what follows it, writes the fp32 planes).
 *
 * Outputs are addressed with strides (in ELEMENTS), so the RGB planes can be channels 0..2 of one [B, 4, oh, ow] tensor:
 *     channel c of frame b      rgb_out + b * rgb_out_batch_stride + c * rgb_out_channel_stride
 *     depth of frame b          depth_out + b * depth_out_batch_stride
 * Every plane is oh * ow contiguous elements; outputs must not overlap an input or each other.
 */
#ifndef CSPN_TRANSFORM_H_
#define CSPN_TRANSFORM_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_TRANSFORM_ABI_VERSION 1

enum { CSPN_TRANSFORM_VAL = 0, CSPN_TRANSFORM_TRAIN = 1 };   /* mode */

#define CSPN_TRANSFORM_PARAMS 8            /* fp64 per frame */
#define CSPN_TRANSFORM_GATHER_PIXELS 256   /* output pixels per workgroup of the gather pass = per partial sum of L */
#define CSPN_TRANSFORM_MAX_SECOND 32768    /* cap of (int)(h1 * s), (int)(w1 * s) */

/* (int)(H * first), (int)(W * first): the size after the first resize (callable without a device).  0 if a size is below 1. */
int cspn_transform_first_size(int H, int W, double first, int* h1, int* w1);

/* Bytes of `work` (callable without a device; 0 for arguments cspn_transform would refuse). */
size_t cspn_transform_workspace_bytes(int mode, int B, int H, int W, double first, int oh, int ow);

/* rgb: uint8 [B, 3, H*W] contiguous; depth: fp32 [B, H*W] contiguous, 4-byte aligned.  B <= 65535, H * W < 2^31, oh * ow < 2^31.
 * params: device fp64 [B, 8], 8-byte aligned, for CSPN_TRANSFORM_TRAIN; NULL for CSPN_TRANSFORM_VAL (which needs oh <= h1, ow <= w1).
 * work: 8-byte aligned, cspn_transform_workspace_bytes(...) bytes. */
int cspn_transform(const unsigned char* rgb, const float* depth, int B, int H, int W, double first, int oh, int ow, int mode,
                   const double* params_or_null, float* rgb_out, long rgb_out_batch_stride, long rgb_out_channel_stride,
                   float* depth_out, long depth_out_batch_stride, void* work, cspn_stream_t stream);

/* Draws the rows of B frames: Philox4x32-10 (Salmon et al., SC'11) with
 *     counter = (slot, 1, frame_id mod 2^32, frame_id >> 32),  key = (seed mod 2^32, seed >> 32),  u = (x0 >> 8) * 2^-24
 * (word 1 = 1 keeps the stream apart from the sampler's, cspn_sparsify.h) and, for the slots 0..6,
 *     s = 1 + 0.5u   angle = -5 + 10u   flip = u < 0.5   brightness, contrast, saturation = 0.6 + 0.8u   order = floor(6u)
 * — the reference's distributions (nyu_dataloader.py:14-17, transforms.py:481-497), not numpy's stream.  frame_ids: DEVICE int64 [B],
 * 8-byte aligned; params: device fp64 [B, 8].  A row depends on (seed, frame id) only. */
int cspn_transform_draw_params(const long long* frame_ids, int B, unsigned long long seed, double* params, cspn_stream_t stream);

/* CSPN_TRANSFORM_ABI_VERSION the library was built from */
int cspn_transform_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_TRANSFORM_H_ */

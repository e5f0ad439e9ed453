/*
 * cspn_visual.h — C ABI of the reference's comparison images in libcspn_hip.so (paths relative to the reference repo):
 *   libs/utils.py:69-75     colored_depthmap          libs/utils.py:139-147   feature_map
 *   libs/utils.py:78-123    merge_into_row, merge_into_row_with_gt, merge_rgb_depth_into_row
 *   libs/utils.py:150-192   merge_features_into_row, save_features
 *   libs/trainers/single_gpu_trainer.py:140-175   the comparison_<iter>.png sheet of trainer.eval
 * as TWO launches without atomics, without "last block" counters, without a host synchronisation and capturable in a graph:
 *   1. range     per frame and per depth plane, the NaN-propagating fp32 minimum and maximum of np.min / np.max, as one partial
 *                pair per chunk of CSPN_VISUAL_RANGE_CHUNK elements, written to the workspace
 *   2. colourise every workgroup folds its frame's partials itself, combines the planes' extrema, and writes interleaved bytes
 *
 * A header of its own with a version of its own: CSPN_ABI_VERSION (cspn_hip.h) does not move.  The conventions are those of
 * cspn_optim.h: 1 on success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects the device, and the library
 * enqueues on the given stream without synchronising.  Depth and feature planes are fp32.
 *
 * Arithmetic, every line ONE separately rounded IEEE fp32 operation (the division is a true one, no reciprocal):
 *     d_min = planes' minima folded in argument order by Python's rule  m = (b < m) ? b : m       (max: b > m)
 *             — a NaN in the FIRST plane stays (the whole row comes out black), a NaN in a later plane is passed over
 *     rel   = (d - d_min) / (d_max - d_min)
 *     x     = rel * 256
 *     i     = NaN -> black (0, 0, 0);  x < 0 -> 0;  x >= 256 -> 255 (x == 256 included);  else trunc(x)
 *     rgb   = table[i]: the 256 x 3 BYTES uint8(255 * jet(i)), truncated in float64 — matplotlib's table, embedded in
 *             cspn_visual.hip and recorded in golden G25 (table[128] is (124, 255, 121): 255 * jet(0.5) is 124.99999…)
 * A constant plane divides 0 by 0: black.  +Inf as the maximum: finite pixels take entry 0, the Inf pixel is black.  -Inf as the
 * minimum: every pixel is black.
 *
 * The RGB panel is uint8(trunc(rgb_scale * v)), the product in fp32: rgb_scale 1 is merge_into_row and merge_rgb_depth_into_row
 * (the reference's `255 *` is commented out there, libs/utils.py:79-80 — reproduced), 255 is merge_into_row_with_gt.  A uint8 RGB
 * input is copied.  DELIBERATE DIFFERENCE: outside [0, 256) and for NaN numpy's astype('uint8') is platform-defined; here the
 * value SATURATES to 0 / 255 and NaN gives 0.
 *
 * Output: interleaved bytes, P panels side by side, a row is P * W * 3 bytes and rows are dense; frame b starts at
 * out + b * out_frame_stride (bytes).  Neither `out` nor the row length need be a multiple of 4: a thread owns 4 consecutive pixels
 * (12 bytes) of a row and writes the dwords that lie on the 4-byte grid as dwords, the ragged head and tail as bytes.  The bytes
 * of a frame do not depend on its place in the batch, on B, or on the launch geometry (min / max are exact, the rest is per pixel).
 */
#ifndef CSPN_VISUAL_H_
#define CSPN_VISUAL_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_VISUAL_ABI_VERSION 1

#define CSPN_VISUAL_RANGE_CHUNK 4096       /* elements per partial (min, max) pair: 256 threads x 4 x 16 bytes */
#define CSPN_VISUAL_MAX_PLANES 3           /* depth planes of a row: sparse input, target, prediction */

#define CSPN_VISUAL_RGB_NONE 0
#define CSPN_VISUAL_RGB_F32 1
#define CSPN_VISUAL_RGB_U8 2

/* The panels of cspn_visual_rows.  Every plane is H x W contiguous elements; strides are in ELEMENTS of the tensor's own type.
 * use_min / use_max != 0: d_min / d_max are taken as given (colored_depthmap(depth, d_min, d_max)) instead of the planes'. */
typedef struct cspn_visual_rows_t {
    const void* rgb;                              /* channel c of frame b at rgb + b * rgb_frame_stride + c * rgb_channel_stride */
    int rgb_kind;                                 /* CSPN_VISUAL_RGB_*; NONE: no RGB panel */
    float rgb_scale;
    long rgb_frame_stride, rgb_channel_stride;
    const void* depth[CSPN_VISUAL_MAX_PLANES];    /* plane k of frame b at depth[k] + b * depth_frame_stride[k], in ARGUMENT order */
    long depth_frame_stride[CSPN_VISUAL_MAX_PLANES];
    int n_depth;                                  /* 1 .. CSPN_VISUAL_MAX_PLANES */
    int use_min, use_max;
    float d_min, d_max;
} cspn_visual_rows_t;

/* Bytes of workspace for B frames of `n_planes` range units of `elements` elements each (rows: n_depth planes of H * W;
 * features: 1 unit of C * H * W).  Callable without a device; 0 + cspn_last_error() on a bad argument. */
size_t cspn_visual_workspace_bytes(int B, int n_planes, size_t elements);

/* B rows of (rgb_kind ? 1 : 0) + n_depth panels of H x W -> out.  With use_min and use_max both set, launch 1 is skipped and
 * `work` may be NULL. */
int cspn_visual_rows(const cspn_visual_rows_t* panels, int B, int H, int W, void* out, size_t out_frame_stride, void* work,
                     cspn_stream_t stream);

/* B feature tensors of C x H x W contiguous fp32 (frame b at features + b * frame_stride elements): ONE range over all C planes —
 * what the reference's np.min(features) / np.max(features) take —, the first n planes as n colour panels, no RGB.  1 <= n <= C. */
int cspn_visual_features(const void* features, long frame_stride, int B, int C, int H, int W, int n, void* out,
                         size_t out_frame_stride, void* work, cspn_stream_t stream);

/* CSPN_VISUAL_ABI_VERSION the library was built from */
int cspn_visual_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_VISUAL_H_ */

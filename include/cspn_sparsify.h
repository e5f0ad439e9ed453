/*
 * cspn_sparsify.h — C ABI of the sparse-depth sampler and the RGB-D assembly of libcspn_hip.so (paths relative to the
 * reference repo):
 *   dataloaders/nyu_dataloader/dense_to_sparse.py:27-52   UniformSampling.dense_to_sparse   ("uar", the default sparsifier)
 *   dataloaders/nyu_dataloader/dataloader.py:85-97        create_sparse_depth / create_rgbd
 * for a batch of frames that already sits on the device: per-frame semantics, two launches, no atomics, no wait between
 * workgroups, nothing read back to the host, capturable in a graph.
 *
 * A header of its own with a version of its own, as cspn_criterion.h: CSPN_ABI_VERSION (cspn_hip.h) does not move.  The
 * conventions are those of cspn_hip.h: 1 on success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects
 * the device, and the library enqueues on the given stream without synchronising.
 *
 * Semantics of frame b (HW = H * W pixels, pixel p = y * W + x), as the reference computes them:
 *     keep(p)   = depth > 0  (a NaN is not kept)  and  depth <= max_depth  (fp32 against fp32, as numpy compares an fp32 array
 *                 with a Python scalar; max_depth = +inf cuts nothing, a NaN max_depth keeps nothing)
 *     n_keep    = the number of kept pixels of THIS frame
 *     prob      = (double)num_samples / (double)n_keep                       (n_keep == 0: nothing is sampled)
 *     mask(p)   = keep(p) and u(p) < prob, compared in fp64                  (u == prob is not sampled; prob >= 1 samples every
 *                                                                             kept pixel; a NaN u samples nothing)
 *     sparse(p) = mask(p) ? depth(p) : +0.0f                                 (a copy or a zero: bit-exact by construction)
 * mode CSPN_SPARSIFY_DENSE is `sparsifier is None` (dataloader.py:86-87): sparse = depth, every bit, mask = 1, one launch.
 *
 * u, the uniform of a pixel:
 *   CSPN_UNIFORM_F32 / CSPN_UNIFORM_F64   given: a [B, HW] contiguous plane, widened exactly.
 *   CSPN_UNIFORM_PHILOX                   generated: Philox4x32-10 (Salmon et al., SC'11) with
 *                                             counter = (p mod 2^32, 0, frame_id mod 2^32, frame_id >> 32),  key = (seed mod 2^32, seed >> 32)
 *                                             u = (x0 >> 8) * 2^-24        x0: the first of the four output words; [0, 1), 24 bits
 *                                         frame_id = frame_ids[b], a DEVICE int64 [B] (a captured loop advances it on the device).
 *                                         The mask of a frame is a function of (seed, frame id, depth, num_samples, max_depth) only:
 *                                         not of b, not of B, not of any tiling.
 *
 * Layout.  A frame is cut into units of 4 pixels, unit q = pixels [4q, 4q + 4) OF THE FRAME; a thread handles whole units.
 * Each plane of each frame is looked at on its own: where its first byte is 16-byte aligned (4-byte for uint8 planes) a full
 * unit moves in one access (two for fp64), anywhere else — HW % 4 != 0 puts every other frame there, and so does a view that
 * starts inside a larger buffer — element by element: the same values in the same registers in front of one copy of the
 * arithmetic, hence the same bits.
 *   count pass   grid (S, B), S = cspn_sparsify_slices(HW) <= 64 slices of 256 threads: work[b * S + s] = kept pixels (uint32)
 *                of the units q with (q / 256) % S == s.
 *   apply pass   every workgroup adds its own frame's S partials (integers: any order gives the same sum; lane l takes
 *                partial l, the 64 lanes are added in a fixed tree), forms prob in fp64 and streams its units.
 * Outputs are addressed with strides (in ELEMENTS of the output), so they can be planes of one [B, 4, H, W] tensor:
 *     sparse plane of frame b          sparse + b * sparse_batch_stride
 *     channel c (0..2) of frame b      rgb_out + b * rgb_out_batch_stride + c * rgb_out_channel_stride
 * Every plane is HW contiguous elements; outputs must not overlap an input or each other.
 *
 * rgb (optional, the fused create_rgbd): [B, 3, HW] contiguous,
 *   CSPN_RGB_F32   copied bit for bit;
 *   CSPN_RGB_U8    converted as the reference's loader does (nyu_dataloader.py:29 `asfarray(rgb) / 255` in fp64, then ToTensor's
 *                  .float()): (float)((double)v / 255.0).
 * mask (optional): [B, HW] contiguous uint8, 1 / 0.
 */
#ifndef CSPN_SPARSIFY_H_
#define CSPN_SPARSIFY_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_SPARSIFY_ABI_VERSION 1

enum { CSPN_SPARSIFY_UAR = 0, CSPN_SPARSIFY_DENSE = 1 };                         /* mode */
enum { CSPN_UNIFORM_PHILOX = 0, CSPN_UNIFORM_F32 = 1, CSPN_UNIFORM_F64 = 2 };    /* uniform_kind */
enum { CSPN_RGB_NONE = 0, CSPN_RGB_F32 = 1, CSPN_RGB_U8 = 2 };                   /* rgb_kind */

/* pixels of a frame one count slice covers before it strides on (256 threads x one unit of 4) */
#define CSPN_SPARSIFY_SLICE_PIXELS 1024
#define CSPN_SPARSIFY_MAX_SLICES 64

/* Slices per frame: ceil(HW / 1024), at least 1, at most 64 — a function of HW only (callable without a device). */
int cspn_sparsify_slices(size_t HW);

/* Bytes of `work`: B * slices * 4 (callable without a device; 0 for B < 1 or HW < 1). */
size_t cspn_sparsify_workspace_bytes(int B, size_t HW);

/* depth: [B, HW] contiguous, dtype CSPN_F32 only (CSPN_F16 fails with a message: a sparse sample is a copy of the measured
 * depth, and the reference's depth is fp32).  B <= 65535, HW < 2^32.
 * uniform: the plane for CSPN_UNIFORM_F32 / _F64, NULL for CSPN_UNIFORM_PHILOX, which reads frame_ids (8-byte aligned) and seed.
 * sparse_or_null / mask_or_null: at least one of them.  rgb_or_null with rgb_kind != CSPN_RGB_NONE needs rgb_out.
 * work: 4-byte aligned, cspn_sparsify_workspace_bytes(B, HW) bytes (not read or written in mode CSPN_SPARSIFY_DENSE, may be NULL there).
 * Launches: count + apply (CSPN_SPARSIFY_UAR), apply alone (CSPN_SPARSIFY_DENSE). */
int cspn_sparsify(const void* depth, int dtype, int B, int H, int W, int mode, long long num_samples, float max_depth,
                  const void* uniform_or_null, int uniform_kind, const long long* frame_ids_or_null, unsigned long long seed,
                  void* sparse_or_null, long sparse_batch_stride,
                  const void* rgb_or_null, int rgb_kind, void* rgb_out_or_null, long rgb_out_batch_stride, long rgb_out_channel_stride,
                  unsigned char* mask_or_null, void* work, cspn_stream_t stream);

/* CSPN_SPARSIFY_ABI_VERSION the library was built from */
int cspn_sparsify_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_SPARSIFY_H_ */

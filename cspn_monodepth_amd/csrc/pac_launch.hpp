// pac_launch.hpp — host-side launch helpers of the pixel-adaptive convolution (pac_conv2d.hip, pac_conv2d_s2.hip): the
// workgroup targets, the channel split, the launch tail and the run-time -> compile-time dispatchers.  No device code.
#pragma once
#include "cspn_common.hpp"

#include <algorithm>
#include <utility>

namespace {

// ------------------------------------------------------------------------------------------------ workgroup targets
// A launch with fewer workgroups than its target splits the channels (or the taps) over more of them until it is reached.
// ANY_WANT_WGS: the any-geometry launches.  Measured on the C = 32 dilated row — 512 / 1024 / 2048 workgroups: forward
// 57 / 47 / 54 us.  The LDS-tiled square kernels share it: every channel chunk re-reads the kernel planes, so only split as far as
// filling the chip needs (~4 x 256 groups).
// GK_ANY_TAPGROUP_WANT_WGS: tap groups of the any-geometry dL/dkernel with a shared kernel.  Same row, 1 / 2 tap groups: 58 / 88 us.
constexpr size_t ANY_WANT_WGS = 1024, GK_ANY_TAPGROUP_WANT_WGS = 256;
constexpr size_t PERCH_WANT_FACTOR = 4;      // tiled forward / dL/dinput with a per-channel kernel: nothing is re-read, split 4 x further
constexpr size_t H8_WANT_WGS = 1024;         // fp16 eight-pixel forward
constexpr size_t GK_WANT_WGS = 4096;         // outer-product dL/dkernel (per-channel kernel: a pure store stream)
constexpr size_t GK_ANY_WANT_WGS = 1024;     // ... of the any-geometry kernel (channel chunks of a per-channel kernel)
constexpr size_t GENERIC_WANT_WGS = 2048;    // generic one-quad kernels: enough workgroups to fill 256 CUs a few times over
constexpr size_t S2_WANT_WGS = 1024;         // stride-2 chunked launches

// Channels per workgroup of a launch that has `have` workgroups before any split and wants `want`: the channels go to
// min(ceil(want / have), ceil(C / granule)) chunks of equal size, rounded up to the granule (the kernel's channel batch).
// A launch that is not split gets C rounded up to the granule — the kernels clamp the chunk's end to C.
inline int split_channels(int C, size_t have, size_t want, int granule) {
    const size_t nchunk = std::min((want + have - 1) / have, (size_t)ceil_div(C, granule));
    return ceil_div(ceil_div(C, (int)std::max<size_t>(nchunk, 1)), granule) * granule;
}

// ------------------------------------------------------------------------------------------------ launch tail
// The poisoned-LDS hook (cspn_common.hpp), the launch, the error check; 1 / 0 as every entry point.
template <typename... P, typename... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... args) {
    CSPN_PRE(st), kernel<<<grid, block, lds, st>>>(std::forward<A>(args)...);
    HIP_OK(hipGetLastError());
    return 1;
}

// ------------------------------------------------------------------------------------------------ dispatchers
// with_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...): run-time flags become template
// arguments inside a generic lambda.  Every combination of the flags is compiled — a lambda whose kernel exists for some of
// them only folds the others onto an existing instance itself (`a.value && b.value`).
template <typename F>
int with_bools(F&& f) { return f(); }
template <typename F, typename... Rest>
int with_bools(F&& f, bool b, Rest... rest) {
    return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
             : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

}  // namespace

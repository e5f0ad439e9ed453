// cspn_upconv.hip — the head of a decoder block fused with its un-pooling (include/cspn_upconv.h).
//
// The entry points of the fp32 family and nothing else: the computation, the decomposition into four phases, the kernels, the fp32
// form of a chunk (the policy F32) and the argument checks are those of cspn_upconv_core.hpp.  fp32 tensors only; the forward's dtype
// CSPN_UPCONV_F32_BF16X3 runs the same pack through the split form (the policy F32X3, f-15).
#include "cspn_upconv_core.hpp"
#include "cspn_upconv.h"

extern "C" {

int cspn_upconv_abi_version(void) { return CSPN_UPCONV_ABI_VERSION; }

size_t cspn_upconv_workspace_bytes(int out_channels, int C) { return packed_elems(out_channels, C) * sizeof(float); }

int cspn_upconv_pack(const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, int dtype, void* packed,
                     cspn_stream_t stream) {
    const char* who = "cspn_upconv_pack";
    if (dtype != CSPN_F32) return fail("%s: fp32 only", who);
    int O0 = 0, M = 0;
    size_t elems = 0;
    if (!check_pack(who, weights, out_channels, n_filters, C, kh, kw, packed, CSPN_UPCONV_MAX_FILTERS, O0, M, elems)) return 0;
    return launch_pack<float, F32>(weights, n_filters, packed, O0, M, C, elems, stream);
}

int cspn_upconv_forward(const void* x, int dtype, const void* packed, const void* scale, const void* shift, int relu_channels,
                        void* const* outs, const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow,
                        cspn_stream_t stream) {
    const char* who = "cspn_upconv_forward";
    // fwd<F32> is named first: the kernels come out in the order they are first used, and the exact kernel keeps its place and labels
    if (dtype == CSPN_F32)
        return forward<F32>(who, x, packed, scale, shift, relu_channels, outs, out_channels, n_outs, N, C, H, W, oh, ow, CSPN_UPCONV_MAX_FILTERS,
                            stream);
    if (dtype == CSPN_UPCONV_F32_BF16X3)      // fp32 tensors and the same pack; only the products differ
        return forward<F32X3>(who, x, packed, scale, shift, relu_channels, outs, out_channels, n_outs, N, C, H, W, oh, ow,
                              CSPN_UPCONV_MAX_FILTERS, stream);
    return fail("%s: fp32 only (CSPN_F32, or CSPN_UPCONV_F32_BF16X3 for the split products)", who);
}

}  // extern "C"

// cspn_uphalf.hip — the head of a decoder block fused with its un-pooling, in half precision (include/cspn_uphalf.h).
//
// The entry points of the fp16 family and nothing else: the computation, the decomposition into four phases, the kernels, the fp16
// form of a chunk (the policy F16) and the argument checks are those of cspn_upconv_core.hpp.  Filters are packed from fp32 or fp16.
#include "cspn_upconv_core.hpp"
#include "cspn_uphalf.h"

extern "C" {

int cspn_uphalf_abi_version(void) { return CSPN_UPHALF_ABI_VERSION; }

size_t cspn_uphalf_packed_bytes(int out_channels, int C) { return packed_elems(out_channels, C) * sizeof(_Float16); }

int cspn_uphalf_pack(const void* const* weights, const int* out_channels, int n_filters, int C, int kh, int kw, int src_dtype,
                     void* packed, cspn_stream_t stream) {
    const char* who = "cspn_uphalf_pack";
    if (src_dtype != CSPN_F32 && src_dtype != CSPN_F16) return fail("%s: the filters must be fp32 or fp16, got dtype %d", who, src_dtype);
    int O0 = 0, M = 0;
    size_t elems = 0;
    if (!check_pack(who, weights, out_channels, n_filters, C, kh, kw, packed, CSPN_UPHALF_MAX_FILTERS, O0, M, elems)) return 0;
    return src_dtype == CSPN_F32 ? launch_pack<float, F16>(weights, n_filters, packed, O0, M, C, elems, stream)
                                 : launch_pack<_Float16, F16>(weights, n_filters, packed, O0, M, C, elems, stream);
}

int cspn_uphalf_forward(const void* x, const void* packed, const void* scale, const void* shift, int relu_channels, void* const* outs,
                        const int* out_channels, int n_outs, int N, int C, int H, int W, int oh, int ow, cspn_stream_t stream) {
    return forward<F16>("cspn_uphalf_forward", x, packed, scale, shift, relu_channels, outs, out_channels, n_outs, N, C, H, W, oh, ow,
                        CSPN_UPHALF_MAX_FILTERS, stream);
}

}  // extern "C"

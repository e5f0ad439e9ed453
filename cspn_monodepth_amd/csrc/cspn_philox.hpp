// cspn_philox.hpp — the one counter-based generator of the data kernels (cspn_sparsify.hip: C1 = 0, cspn_transform.hip: C1 = 1).
#pragma once
#include "cspn_common.hpp"

namespace {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) on the counter
// (c0, C1, c2, c3) with the key (k0, k1); the first output word's upper 24 bits as a uniform in [0, 1).
template <unsigned C1>
__device__ __forceinline__ double philox_uniform(unsigned c0, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    unsigned c1 = C1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (double)(c0 >> 8) * 0x1p-24;
}

}  // namespace

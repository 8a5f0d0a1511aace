// Counter-based Philox4x32-10 and the uniform built from one of its words: shared by the synthetic benchmark env
// (csrc/aux_hooks.hip) and the classic-control tasks (csrc/environment.hip).  Integer arithmetic and two exact fp32 steps, so
// the host and the device give the same bits.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cusrl {

struct Philox {
    uint32_t c[4];
};

__host__ __device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n1 = uint32_t(p1), n2 = uint32_t(p0 >> 32) ^ c3 ^ k1, n3 = uint32_t(p0);
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}

// the top 24 bits at the centre of their cell of [0, 1]: k * 2^-24 + 2^-25.  (The last cell's centre rounds to 1.0f.)
__host__ __device__ __forceinline__ float philox_uniform(uint32_t x) { return float(x >> 8) * 5.9604645e-8f + 2.9802322e-8f; }

}  // namespace cusrl

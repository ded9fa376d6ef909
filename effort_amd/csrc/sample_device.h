// The sampled pick's random source: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), ONE definition
// for the kernel (sample.hip) and for the host (effort_sample_bits in glue.hip: what lets a test without a GPU pin the generator).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EFFORT_HD __host__ __device__
#else
#define EFFORT_HD
#endif

namespace effort {

// counter (pos, stream, 0, 0), key (seed_lo, seed_hi), ten rounds; returns output word 0.  The uniform of a draw is (x0 >> 8) * 2^-24.
EFFORT_HD inline uint32_t philox_x0(uint32_t seedLo, uint32_t seedHi, uint32_t stream, uint32_t pos) {
    uint32_t c0 = pos, c1 = stream, c2 = 0u, c3 = 0u, k0 = seedLo, k1 = seedHi;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

}  // namespace effort

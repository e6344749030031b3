// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator behind
// mlpk_dropout's masks.  Plain C++ with __host__ __device__ under hipcc, so the host build of tests/test_dropout_host.py checks the very code
// the kernel runs against the published known-answer vectors and against tests/philox_ref.py.
#ifndef MLPK_PHILOX_H
#define MLPK_PHILOX_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MLPK_HD __host__ __device__ __forceinline__
#else
#define MLPK_HD inline
#endif

namespace mlpk {

struct philox4 {
    uint32_t v[4];
};

// 10 rounds; the key is bumped by the Weyl increments between rounds
MLPK_HD philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    philox4 out;
    out.v[0] = c0;
    out.v[1] = c1;
    out.v[2] = c2;
    out.v[3] = c3;
    return out;
}

// the four dropout words of logical elements 4 g .. 4 g + 3 (mlpk.h, mlpk_dropout): key = the seed's halves, counter = (g, site, 0)
MLPK_HD philox4 dropout_words(uint64_t seed, uint32_t site, uint64_t g) {
    return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), site, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

}  // namespace mlpk

#endif  // MLPK_PHILOX_H

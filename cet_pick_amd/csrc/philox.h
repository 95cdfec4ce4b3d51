// Counter-based random numbers of the augmentation kernels: Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random
// numbers: as easy as 1, 2, 3", SC'11) and the two maps from a 32-bit word to a uniform draw.  No state: a draw is a pure
// function of (counter, key).
#pragma once
#include "common.h"

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct u32x4 { uint32_t v[4]; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return u32x4{{c0, c1, c2, c3}};
}

// 24 random bits -> [0, 1)
__device__ __forceinline__ float unit_float(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }
// uniform integer in [0, n) (multiply-high; the bias is n / 2^32)
__device__ __forceinline__ int below(uint32_t r, int n) { return (int)__umulhi(r, (uint32_t)n); }

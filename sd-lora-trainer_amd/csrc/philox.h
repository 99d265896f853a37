// The project's counter-based normal generator, shared by the step launch of the stochastic samplers (sampler.hip) and the bootstrap of regional prompts
// (region.hip): Philox4x32-10 and the Box-Muller step that turns its four words into four normals.  A caller chooses the key (an image's seed words)
// and the 128-bit counter; counter word 3 is a tag that keeps one use's draws apart from every other use of the same seed.
//   u_k      = ((word_k >> 9) + 0.5) 2^-23                  23 bits: (2 m + 1) 2^-24 is exact in fp32 and lies strictly inside (0, 1)
//   z_0, z_1 = sqrt(-2 ln u_0) (cos, sin)(2 pi u_1) ;  z_2, z_3 likewise from (u_2, u_3)       (cos, sin)(2 pi u) = sincospif(2 u): 2 u is exact
// Every operation is rounded once (no contraction): the tests compare bits between launches that share these functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr uint32_t NOISE_TAG = 0x53444531u;             // counter word 3 of the stochastic samplers' per-step noise (sampler.hip)
constexpr uint32_t REGION_TAG = 0x52474E31u;            // counter word 3 of the regional prompts' bootstrap noise (region.hip)

// Philox4x32-10 (Salmon et al. 2011, Random123): ten rounds, the key bumped by the Weyl constants between them.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// Four normals from the counter (c0, c1, c2, c3) under the key (k0, k1).
__device__ __forceinline__ void philox_normal4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, float z[4]) {
  uint32_t w[4];
  philox4x32_10(c0, c1, c2, c3, k0, k1, w);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u0 = ((float)(w[2 * h] >> 9) + 0.5f) * 0x1p-23f;
    const float u1 = ((float)(w[2 * h + 1] >> 9) + 0.5f) * 0x1p-23f;
    const float r = sqrtf(-2.f * logf(u0));
    float sn, cs;
    sincospif(2.f * u1, &sn, &cs);
    z[2 * h] = r * cs;
    z[2 * h + 1] = r * sn;
  }
}

}  // namespace

// Counter-based N(0,1) draws on the device: Philox4x32-10 + Box-Muller (the step's eps of
// vae_latent_dec_fwd, vanilla_vae.py:116, and the prior sample of vae_mmd, info_vae.py:220).
#pragma once
#include "vae_common.hpp"

namespace vae {

constexpr uint32_t kStreamEps = 0x5EEDu;        // counter word 2 of the reparameterization noise
constexpr uint32_t kStreamPrior = 0x9A1Du;      // ... of the MMD prior sample (never the eps stream)

// Philox4x32-10 (Salmon et al., SC'11): 4 x 32 random bits per (counter, key)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = uint4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
// four N(0,1) draws for elements 4q..4q+3 of step `step` on `stream` (Box-Muller on word pairs;
// u in (0, 1])
__device__ __forceinline__ f32x4 normal4_stream(uint32_t q, uint32_t step, uint32_t stream, uint64_t seed) {
  const uint4 w = philox4x32_10(uint4{q, step, stream, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
  constexpr float kInv = 2.3283064365386963e-10f;               // 2^-32
  const float u0 = ((float)w.x + 0.5f) * kInv, v0 = (float)w.y * kInv;
  const float u1 = ((float)w.z + 0.5f) * kInv, v1 = (float)w.w * kInv;
  const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u1));
  float s0, c0, s1, c1;
  sincosf(6.283185307179586f * v0, &s0, &c0);
  sincosf(6.283185307179586f * v1, &s1, &c1);
  return f32x4{r0 * c0, r0 * s0, r1 * c1, r1 * s1};
}

}  // namespace vae

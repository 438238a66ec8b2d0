// Standard-normal noise as a pure function of (seed, tag, element index), by Box-Muller on two hashed uniforms: the stochastic kernels of StoSAVi
// (kernel_sample.hip) draw it in the forward, regenerate it in the backward and never store it; tests rebuild it on the host (train.normal_noise).
// u1, u2 lie on the 2^23 midpoints of (0, 1), as sf_gumbel's uniform does, so |eps| <= sqrt(-2 ln 2^-24) = 5.77.
#pragma once
#include "sf_common.h"

// the seed of one stream of draws: `tag` separates the draws a step makes from one seed (StoSAVi: the frame); the pattern of site_seed (dropout_mask.h)
static inline uint32_t sf_normal_seed(unsigned long long seed, uint32_t tag) {
  return sf_mix32((uint32_t)seed ^ sf_mix32((uint32_t)(seed >> 32) + 0x9e3779b9u * (tag + 1u)));
}
// element i (i < 2^31) of the stream: full-precision logf, sqrtf, cosf
__device__ __forceinline__ float sf_normal(uint32_t sseed, uint32_t i) {
  const float u1 = ((float)(sf_mix32((2u * i) ^ sseed) >> 9) + 0.5f) * 1.1920929e-7f;
  const float u2 = ((float)(sf_mix32((2u * i + 1u) ^ sseed) >> 9) + 0.5f) * 1.1920929e-7f;
  return sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
}

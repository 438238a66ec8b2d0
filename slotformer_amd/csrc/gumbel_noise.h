// Gumbel(0, 1) noise as a pure function of (seed, element index): the relaxed one-hot sample of steve_utils.py:26-41 (steve_decoder.hip:
// sf_gumbel_softmax_rows_f32) and the soft rows / sampled ids of the fused token step (slate_step.hip) draw it inside their kernels and never
// store it; tests rebuild it on the host (train.gumbel_noise).
#pragma once
#include "sf_common.h"

// the seed of the stream: what sf_gumbel_softmax_rows_f32 has always derived from its 64-bit seed
static inline uint32_t sf_gumbel_seed(unsigned long long seed) {
  return sf_mix32((uint32_t)seed ^ sf_mix32((uint32_t)(seed >> 32) + 0x9e3779b9u));
}
// Gumbel(0, 1) sample of element idx: -log(E) with E = -log(u) ~ Exp(1), u uniform on the 2^23 midpoints of (0, 1)
__device__ __forceinline__ float sf_gumbel(uint32_t idx, uint32_t sseed) {
  const float u = ((float)(sf_mix32(idx ^ sseed) >> 9) + 0.5f) * 1.1920929e-7f;
  return -logf(-logf(u));
}

// The dropout masks of the training kernels (rollout_train.hip, phyre_readout_train.hip): a pure function of (seed, rollout step, layer, site,
// element index) -- keep = mix32(idx ^ site_seed) >> 8 >= p * 2^24 --, so a backward pass regenerates them and tests rebuild them on the host
// (train.dropout_keep_mask).
#pragma once
#include "sf_common.h"

enum { SITE_ATTN_P = 0, SITE_ATTN_O = 1, SITE_FFN_H = 2, SITE_FFN_O = 3 };
static inline uint32_t site_seed(unsigned long long seed, int step, int layer, int site) {
  const uint32_t tag = (uint32_t)((step * 64 + layer) * 4 + site);
  return sf_mix32((uint32_t)seed ^ sf_mix32((uint32_t)(seed >> 32) + 0x9e3779b9u * (tag + 1u)));
}
__device__ __forceinline__ bool sf_keep(uint32_t sseed, uint32_t idx, uint32_t thresh) {
  return (sf_mix32(idx ^ sseed) >> 8) >= thresh;
}
static inline uint32_t drop_thresh(float p) { return (uint32_t)((double)p * 16777216.0); }

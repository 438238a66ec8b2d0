// The normalisation of a uint8 colour value, (x / 255 - mean_c) / std_c, as ONE multiply-add x * a_c + b_c: the coefficients in float64 on the host,
// rounded once.  Shared by ingest.hip (applied to the resampled value) and clip_train.hip (frames already at the model's resolution), so that the
// two agree bit for bit at equal source and output size.
#pragma once
#include <hip/hip_runtime.h>

inline void sf_ingest_norm_coeffs(const float* mean3, const float* std3, float* a3, float* b3) {
  for (int c = 0; c < 3; ++c) {
    a3[c] = (float)(1.0 / (255.0 * (double)std3[c]));
    b3[c] = (float)(-(double)mean3[c] / (double)std3[c]);
  }
}
__device__ __forceinline__ float sf_ingest_norm(float x, float a, float b) { return x * a + b; }

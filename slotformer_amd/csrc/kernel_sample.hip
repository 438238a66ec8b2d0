// The stochastic kernels of StoSAVi in training (savi.py:337-365; base_slots.fit): sampling, the KL regulariser and their gradient, around one
// counter-based normal generator (normal_noise.h), so a step's noise is a function of (seed, frame) and is never stored.
//   sf_normal_noise_f32        out[i] = eps(seed, tag, i)
//   sf_kernel_sample_fwd_f32   kernels = mu + eps * exp(log_var / 2) from dist = (mu | log_var), and the KL sum against the fixed-variance prior
//   sf_kernel_sample_bwd_f32   d_dist from d_kernels and the gradient at the mean KL term; eps regenerated
#include "../../include/slotformer_hip.h"
#include "sf_common.h"
#include "sf_vec.h"
#include "normal_noise.h"

namespace {

constexpr int KS_NT = 256;        // threads per workgroup
constexpr int KS_MAX_GX = 256;    // workgroups of the forward launch: the last arriver's thread t owns partial t
constexpr size_t KS_HEAD = 16;    // bytes in front of the partials: the arrival counter
constexpr int KS_MAX_D = 1024;

typedef unsigned long long u64;

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

inline int ks_gx(long long n4) {
  const long long g = (n4 + KS_NT - 1) / KS_NT;
  return (int)(g < 1 ? 1 : (g > KS_MAX_GX ? KS_MAX_GX : g));
}

__global__ __launch_bounds__(KS_NT) void normal_noise_kernel(float* __restrict__ out, long long n, uint32_t sseed) {
  const long long i = (long long)blockIdx.x * KS_NT + threadIdx.x;
  if (i < n) out[i] = sf_normal(sseed, (uint32_t)i);
}

// the four noise values of float4 i of a [R, D] tensor: elements 4 i .. 4 i + 3
__device__ __forceinline__ f32x4 ks_eps(const float* __restrict__ noise, uint32_t sseed, long long i) {
  if (noise) return ((const f32x4*)noise)[i];
  const uint32_t e = (uint32_t)(4 * i);
  return f32x4{sf_normal(sseed, e), sf_normal(sseed, e + 1u), sf_normal(sseed, e + 2u), sf_normal(sseed, e + 3u)};
}

// Workgroup x strides over the R * D4 float4s.  The sample is rounded as torch rounds mu + noise * exp(0.5 * log_var) -- the product, then the sum;
// the file is built with -ffp-contract=off -- so a step that samples here and one that samples with torch ops on the same noise see the same
// kernels.  Per element: x = log_var - prior_log_var, KL term 0.5 * (expm1(x) - x) -- the issue's
// 0.5 * (prior - log_var) + exp(log_var) / (2 exp(prior)) - 0.5 with the two halves that cancel near x = 0 taken together -- in float32, summed in
// float64.
__global__ __launch_bounds__(KS_NT) void kernel_sample_fwd_kernel(const float* __restrict__ dist, const float* __restrict__ noise, uint32_t sseed,
                                                                  float prior_log_var, float* __restrict__ kernels, double* kld_sum,
                                                                  unsigned* counter, u64* parts, long long n4, int D4, int gx) {
  __shared__ double s_sum[KS_NT / 64];
  __shared__ int s_last;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double sum = 0.0;
  for (long long i = (long long)blockIdx.x * KS_NT + t; i < n4; i += (long long)gx * KS_NT) {
    const long long r = i / D4;
    const int c4 = (int)(i - r * D4);
    const f32x4 mu = ((const f32x4*)dist)[r * 2 * D4 + c4];
    const f32x4 lv = ((const f32x4*)dist)[r * 2 * D4 + D4 + c4];
    const f32x4 eps = ks_eps(noise, sseed, i);
    f32x4 k, term;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      k[j] = mu[j] + eps[j] * expf(0.5f * lv[j]);
      const float x = lv[j] - prior_log_var;
      term[j] = 0.5f * (expm1f(x) - x);
    }
    ((f32x4*)kernels)[i] = k;
    sum += ((double)term.x + (double)term.y) + ((double)term.z + (double)term.w);
  }
  sum = sf_wave_sum(sum);
  if (lane == 0) s_sum[wave] = sum;
  __syncthreads();
  if (t == 0) {
    const double wg = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    // write-through 8-byte store, drained before the arrival is counted (the pattern of sf_clip_mse_f32)
    __hip_atomic_store(parts + blockIdx.x, __builtin_bit_cast(u64, wg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)gx - 1u);
  }
  __syncthreads();
  if (!s_last) return;
  // The last workgroup to arrive: thread t takes partial t (gx <= 256), then the fixed tree -- a function of the partials' indices only.
  double v = 0.0;
  if (t < gx) v = __builtin_bit_cast(double, __hip_atomic_load(parts + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  v = sf_wave_sum(v);
  __syncthreads();   // (s_sum has been read)
  if (lane == 0) s_sum[wave] = v;
  __syncthreads();
  if (t == 0) {
    *kld_sum += ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
  }
}

// one thread per float4 of [R, D]: d_mu = d_kernels, d_log_var = d_kernels * eps * 0.5 * exp(log_var / 2) + g * 0.5 * expm1(log_var - prior),
// g = d_kld * kld_scale
__global__ __launch_bounds__(KS_NT) void kernel_sample_bwd_kernel(const float* __restrict__ dist, const float* __restrict__ noise, uint32_t sseed,
                                                                  float prior_log_var, const float* __restrict__ d_kernels,
                                                                  const float* __restrict__ d_kld, float kld_scale, float* __restrict__ d_dist,
                                                                  long long n4, int D4) {
  const long long i = (long long)blockIdx.x * KS_NT + threadIdx.x;
  if (i >= n4) return;
  const long long r = i / D4;
  const int c4 = (int)(i - r * D4);
  const f32x4 lv = ((const f32x4*)dist)[r * 2 * D4 + D4 + c4];
  const float g = 0.5f * (d_kld[0] * kld_scale);
  f32x4 dk = f32x4{0.f, 0.f, 0.f, 0.f}, dlv;
  if (d_kernels) {
    dk = ((const f32x4*)d_kernels)[i];
    const f32x4 eps = ks_eps(noise, sseed, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) dlv[j] = (dk[j] * eps[j]) * (0.5f * expf(0.5f * lv[j])) + g * expm1f(lv[j] - prior_log_var);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) dlv[j] = g * expm1f(lv[j] - prior_log_var);
  }
  ((f32x4*)d_dist)[r * 2 * D4 + c4] = dk;
  ((f32x4*)d_dist)[r * 2 * D4 + D4 + c4] = dlv;
}

// what the two kernel_sample entry points share: the shape
inline bool ks_shape_ok(long long R, int D) { return R >= 1 && D >= 4 && D % 4 == 0 && D <= KS_MAX_D && R * (long long)D <= (1LL << 31); }

}   // namespace

extern "C" {

int sf_normal_noise_f32(float* out, long long n, unsigned long long seed, unsigned tag, void* stream) {
  SF_REQUIRE(out, "null pointer (normal noise)");
  SF_REQUIRE(n >= 1 && n <= (1LL << 31), "normal noise: 1 to 2^31 elements");
  hipLaunchKernelGGL(normal_noise_kernel, dim3(cdiv(n, KS_NT)), dim3(KS_NT), 0, (hipStream_t)stream, out, n, sf_normal_seed(seed, tag));
  SF_CHECK_LAUNCH();
  return 0;
}

size_t sf_kernel_sample_workspace_bytes(long long R, int D) {
  if (!ks_shape_ok(R, D)) return 0;
  return KS_HEAD + (size_t)ks_gx(R * (D / 4)) * sizeof(u64);
}

int sf_kernel_sample_fwd_f32(const float* dist, const float* noise, unsigned long long seed, unsigned tag, float prior_log_var, float* kernels,
                             double* kld_sum, long long R, int D, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(dist && kernels && kld_sum && ws, "null pointer (kernel sample)");
  SF_REQUIRE(R >= 1, "kernel sample: R >= 1");
  SF_REQUIRE(D >= 4 && D % 4 == 0 && D <= KS_MAX_D, "kernel sample: D is a multiple of 4, at most 1024");
  SF_REQUIRE(R * (long long)D <= (1LL << 31), "kernel sample: at most 2^31 elements");
  SF_REQUIRE((((uintptr_t)dist | (uintptr_t)noise | (uintptr_t)kernels | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)kld_sum & 7) == 0,
             "kernel sample: dist, noise, kernels and the workspace must be 16-byte aligned");
  SF_REQUIRE(ws_bytes >= sf_kernel_sample_workspace_bytes(R, D), "workspace too small (kernel sample)");
  const long long n4 = R * (D / 4);
  const int gx = ks_gx(n4);
  hipLaunchKernelGGL(kernel_sample_fwd_kernel, dim3(gx), dim3(KS_NT), 0, (hipStream_t)stream, dist, noise, sf_normal_seed(seed, tag), prior_log_var,
                     kernels, kld_sum, (unsigned*)ws, (u64*)((char*)ws + KS_HEAD), n4, D / 4, gx);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_kernel_sample_bwd_f32(const float* dist, const float* noise, unsigned long long seed, unsigned tag, float prior_log_var,
                             const float* d_kernels, const float* d_kld, float kld_scale, float* d_dist, long long R, int D, void* stream) {
  SF_REQUIRE(dist && d_kld && d_dist, "null pointer (kernel sample backward)");
  SF_REQUIRE(R >= 1, "kernel sample backward: R >= 1");
  SF_REQUIRE(D >= 4 && D % 4 == 0 && D <= KS_MAX_D, "kernel sample backward: D is a multiple of 4, at most 1024");
  SF_REQUIRE(R * (long long)D <= (1LL << 31), "kernel sample backward: at most 2^31 elements");
  SF_REQUIRE((((uintptr_t)dist | (uintptr_t)noise | (uintptr_t)d_kernels | (uintptr_t)d_dist) & 15) == 0 && ((uintptr_t)d_kld & 3) == 0,
             "kernel sample backward: dist, noise, d_kernels and d_dist must be 16-byte aligned");
  const long long n4 = R * (D / 4);
  hipLaunchKernelGGL(kernel_sample_bwd_kernel, dim3(cdiv(n4, KS_NT)), dim3(KS_NT), 0, (hipStream_t)stream, dist, noise, sf_normal_seed(seed, tag),
                     prior_log_var, d_kernels, d_kld, kld_scale, d_dist, n4, D / 4);
  SF_CHECK_LAUNCH();
  return 0;
}

}   // extern "C"

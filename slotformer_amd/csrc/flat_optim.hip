// The optimiser step over ONE flat fp32 bucket: plain Adam (sf_adam_flat_f32, at the end of the file) and beyond it
//   sf_grad_clip_coef_f32    global L2 norm of the gradient bucket, torch.nn.utils.clip_grad_norm_'s coefficient and a non-finite
//                            flag, in one launch (base_slots/method.py: backward -> clip_grad -> Adam; clip_grad = 0.05 in the
//                            StoSAVi / SAVi / STEVE configurations)
//   sf_adam_flat_groups_f32  Adam with up to 8 contiguous parameter groups of their own learning rates (STEVE: lr / dec_lr,
//                            base_slots/method.py:237-276) that multiplies every gradient element by a coefficient read from
//                            DEVICE memory -- the clip costs no pass of its own and no host round trip.
// Both stream HBM once (4 and 28 bytes per element), 16 bytes per lane wherever the pointers allow it.
#include "../../include/slotformer_hip.h"
#include "sf_common.h"
#include <limits.h>

namespace {

constexpr int GN_NT = 256;         // threads per workgroup
constexpr int GN_MAX_GRID = 1024;  // 4 workgroups on each of the 256 CUs; beyond it the threads stride over the bucket
constexpr size_t GN_HEAD = 16;     // bytes in front of the partials: the arrival counter

typedef unsigned long long u64;

inline int gn_grid(long long n) {
  const long long g = (n + GN_NT * 4 - 1) / (GN_NT * 4);   // one float4 per thread until the grid is full
  return (int)(g < 1 ? 1 : (g > GN_MAX_GRID ? GN_MAX_GRID : g));
}

__device__ __forceinline__ unsigned gn_bad(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u; }   // NaN or +-Inf

// ws: [0] arrival counter (zero between calls), [GN_HEAD ...) grid x {double sum of squares, u64 non-finite flag}
__global__ __launch_bounds__(GN_NT) void grad_clip_coef_kernel(const float* __restrict__ g, long long n, float max_norm,
                                                               float* __restrict__ out3, unsigned* counter, u64* parts) {
  __shared__ double s_sum[GN_NT / 64];
  __shared__ int s_bad[GN_NT / 64];
  __shared__ int s_last;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int grid = gridDim.x;
  // the 16-byte-aligned body [head, head + 4 nv) as float4, the ragged ends as scalars
  long long head = (long long)(((16 - ((uintptr_t)g & 15)) & 15) >> 2);
  if (head > n) head = n;
  const long long nv = (n - head) >> 2, tail0 = head + 4 * nv;
  const f32x4* gv = (const f32x4*)(g + head);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  unsigned bad = 0;
  const long long stride = (long long)grid * GN_NT;
#pragma unroll 4
  for (long long i = (long long)blockIdx.x * GN_NT + t; i < nv; i += stride) {
    const f32x4 x = gv[i];
    acc += x * x;
    bad |= gn_bad(x.x) | gn_bad(x.y) | gn_bad(x.z) | gn_bad(x.w);
  }
  double sum = ((double)acc.x + (double)acc.y) + ((double)acc.z + (double)acc.w);
  if (blockIdx.x == 0) {   // at most 3 + 3 elements: lanes 0..2 of wave 0 the head, of wave 1 the tail
    const long long e = wave == 0 ? (long long)lane : (wave == 1 ? tail0 + lane : n);
    const long long end = wave == 0 ? head : n;
    if (lane < 3 && e < end) {
      const float x = g[e];
      sum += (double)x * (double)x;
      bad |= gn_bad(x);
    }
  }
  sum = sf_wave_sum(sum);
  const bool wbad = __ballot(bad != 0) != 0;
  if (lane == 0) {
    s_sum[wave] = sum;
    s_bad[wave] = wbad;
  }
  __syncthreads();
  if (t == 0) {
    const double wg = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    const u64 wgbad = (u64)(s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]);
    // write-through 8-byte stores, drained before the arrival is counted: no release fence, no whole-L2 write-back
    __hip_atomic_store(parts + 2 * blockIdx.x, __builtin_bit_cast(u64, wg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(parts + 2 * blockIdx.x + 1, wgbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = (__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(grid - 1));
  }
  __syncthreads();
  if (!s_last) return;
  // The last workgroup to arrive: thread t takes the partials [4t, 4t + 4) in index order, then the same fixed tree as above --
  // a function of the partials' INDICES only, so the bits do not depend on who arrived when.  (One thread adding all 1024 in a
  // chain would take longer than the rest of the launch.)  The loads bypass this CU's L1, like the stores.
  double tot = 0.0;
  u64 anybad = 0;
#pragma unroll
  for (int j = 0; j < GN_MAX_GRID / GN_NT; ++j) {
    const int b = (GN_MAX_GRID / GN_NT) * t + j;
    if (b < grid) {
      tot += __builtin_bit_cast(double, __hip_atomic_load(parts + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      anybad |= __hip_atomic_load(parts + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  tot = sf_wave_sum(tot);
  const bool wbad2 = __ballot(anybad != 0) != 0;
  __syncthreads();   // (s_sum / s_bad of the first round have been read)
  if (lane == 0) {
    s_sum[wave] = tot;
    s_bad[wave] = wbad2;
  }
  __syncthreads();
  if (t == 0) {
    const double total = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    const float norm = (float)sqrt(total);
    // clip_grad_norm_: coef = max_norm / (norm + 1e-6) clamped to 1 -- in fp32 like torch, and a NaN stays a NaN
    const float c = max_norm / (norm + 1e-6f);
    out3[0] = norm;
    out3[1] = (max_norm > 0.f) ? (c > 1.f ? 1.f : c) : 1.f;
    out3[2] = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? 1.f : 0.f;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
  }
}

struct AdamGroups {
  long long begin[SF_ADAM_MAX_GROUPS];   // unused entries: LLONG_MAX
  float lr[SF_ADAM_MAX_GROUPS];
};

__device__ __forceinline__ float group_lr(const AdamGroups& G, long long e) {
  float lr = G.lr[0];
#pragma unroll
  for (int k = 1; k < SF_ADAM_MAX_GROUPS; ++k)
    if (e >= G.begin[k]) lr = G.lr[k];
  return lr;
}

// adam_flat_kernel's update of one element (below): the same expression in the same order.  That kernel compiles
// to separate multiplies and adds (its products are packed in pairs before anything could be fused); four elements per thread
// pack differently, so contraction is switched off here to keep every product and sum rounded on its own, as there
// (tests/test_flat_adam_gpu.py compares the bits).
__device__ __forceinline__ void adam_one(float& p, float gi, float& m, float& v, float lr, float b1, float b2, float eps, float bc1,
                                         float bc2_sqrt) {
#pragma clang fp contract(off)
  const float mi = b1 * m + (1.f - b1) * gi;
  const float vi = b2 * v + (1.f - b2) * gi * gi;
  m = mi;
  v = vi;
  p -= (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
}

// thread j < nv: elements [4j, 4j + 4) as float4 (VEC: all four pointers 16-byte aligned); threads nv ... : one element each
// of the rest [4 nv, n).  SCALED: every gradient element times *scale first.
template <bool SCALED>
__global__ __launch_bounds__(256) void adam_flat_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, long long n, long long nv, AdamGroups G, float b1,
                                                               float b2, float eps, float bc1, float bc2_sqrt,
                                                               const float* __restrict__ scale) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  float s = 1.f;
  if constexpr (SCALED) s = *scale;
  if (j < nv) {
    f32x4 pv = ((const f32x4*)p)[j], mv = ((const f32x4*)m)[j], vv = ((const f32x4*)v)[j];
    const f32x4 gq = ((const f32x4*)g)[j];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float pc = pv[c], mc = mv[c], vc = vv[c], gc = gq[c];
      if constexpr (SCALED) gc = gc * s;
      adam_one(pc, gc, mc, vc, group_lr(G, 4 * j + c), b1, b2, eps, bc1, bc2_sqrt);
      pv[c] = pc, mv[c] = mc, vv[c] = vc;
    }
    ((f32x4*)m)[j] = mv;
    ((f32x4*)v)[j] = vv;
    ((f32x4*)p)[j] = pv;
    return;
  }
  const long long e = 4 * nv + (j - nv);
  if (e >= n) return;
  float pc = p[e], mc = m[e], vc = v[e], gc = g[e];
  if constexpr (SCALED) gc = gc * s;
  adam_one(pc, gc, mc, vc, group_lr(G, e), b1, b2, eps, bc1, bc2_sqrt);
  m[e] = mc;
  v[e] = vc;
  p[e] = pc;
}

}   // namespace

size_t sf_grad_norm_workspace_bytes(long long n) { return n < 0 ? 0 : GN_HEAD + (size_t)gn_grid(n) * 2 * sizeof(u64); }

int sf_grad_clip_coef_f32(const float* grad, long long n, float max_norm, float* out3, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(grad && out3 && ws, "null pointer (gradient norm)");
  SF_REQUIRE(n >= 0, "gradient norm: n >= 0");
  SF_REQUIRE(((uintptr_t)grad & 3) == 0 && ((uintptr_t)ws & 15) == 0, "gradient norm: grad 4-byte, workspace 16-byte aligned");
  SF_REQUIRE(ws_bytes >= sf_grad_norm_workspace_bytes(n), "workspace too small (gradient norm)");
  const int grid = gn_grid(n);
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(grid), dim3(GN_NT), 0, (hipStream_t)stream, grad, n, max_norm, out3, (unsigned*)ws,
                     (u64*)((char*)ws + GN_HEAD));
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_adam_flat_groups_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, int step,
                            const sf_adam_group* groups, int num_groups, float beta1, float beta2, float eps, const float* grad_scale,
                            void* stream) {
  SF_REQUIRE(param && grad && exp_avg && exp_avg_sq && groups && n >= 0 && step >= 1, "bad Adam arguments");
  SF_REQUIRE(num_groups >= 1 && num_groups <= SF_ADAM_MAX_GROUPS, "Adam: 1 to 8 parameter groups");
  SF_REQUIRE(groups[0].begin == 0, "Adam: the first group begins at 0");
  AdamGroups G;
  for (int k = 0; k < SF_ADAM_MAX_GROUPS; ++k) {
    G.begin[k] = LLONG_MAX;
    G.lr[k] = 0.f;
  }
  for (int k = 0; k < num_groups; ++k) {
    SF_REQUIRE(groups[k].begin >= 0 && groups[k].begin <= n, "Adam: group begin outside the bucket");
    SF_REQUIRE(k == 0 || groups[k].begin >= groups[k - 1].begin, "Adam: group begins must ascend");
    G.begin[k] = groups[k].begin;
    G.lr[k] = groups[k].lr;
  }
  if (n == 0) return 0;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  const bool vec = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0;
  const long long nv = vec ? n / 4 : 0, threads = nv + (n - 4 * nv);
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (grad_scale)
    hipLaunchKernelGGL(adam_flat_groups_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, nv, G,
                       beta1, beta2, eps, bc1, sqrtf(bc2), grad_scale);
  else
    hipLaunchKernelGGL(adam_flat_groups_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, nv, G,
                       beta1, beta2, eps, bc1, sqrtf(bc2), grad_scale);
  SF_CHECK_LAUNCH();
  return 0;
}

// torch.optim.Adam (no amsgrad, no weight decay: the reference's optimiser, slotformer_clevrer_params.py:16-19) over ONE flat
// fp32 bucket: p, g, m, v [n]; step = the 1-based step count.  One launch per optimiser step.
extern "C" __global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long long n, float lr, float b1, float b2, float eps,
                                                        float bc1, float bc2_sqrt) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float mi = b1 * m[i] + (1.f - b1) * gi;
  const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  // torch: denom = sqrt(v) / sqrt(bias_correction2) + eps;  p -= (lr / bias_correction1) * m / denom
  p[i] -= (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
}
int sf_adam_flat_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, int step, float lr, float beta1,
                     float beta2, float eps, void* stream) {
  SF_REQUIRE(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1, "bad Adam arguments");
  if (n == 0) return 0;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, lr,
                     beta1, beta2, eps, bc1, sqrtf(bc2));
  SF_CHECK_LAUNCH();
  return 0;
}

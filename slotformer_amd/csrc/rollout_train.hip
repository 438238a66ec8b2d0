// Training of the rollout Transformer: forward with saved activations and the backward pass of
// SlotRollouter.forward (slotformer.py:85-126) with torch's pre-LN nn.TransformerEncoderLayer (slotformer.py:72-80),
// dropout included (the reference trains with the layer's default p = 0.1).
//
// Design (MI355X, 288 GB of HBM): nothing is recomputed and nothing is reduced early.
//   * every activation of every rollout step is kept, stacked over the steps ([S][M][width] per layer and kind), and so
//     is every gradient that feeds a weight gradient;
//   * the backward-through-time loop only runs the data-gradient chain (dX = dY . W on the forward GEMM core against
//     transposed weight copies, LayerNorm / attention / dropout backward kernels);
//   * after the loop each weight gradient is ONE contraction over all S*M rows, bias and LayerNorm-parameter gradients are column sums over the
//     same stacked buffers (train_blocks.hip).
// Gradients are written (not accumulated) into caller-owned buffers (sf_rollouter_grads), which the host lays out as one
// flat bucket for the data-parallel all-reduce.
//
// Dropout masks are a pure function of (seed, rollout step, layer, site, element index): keep = mix32(idx ^ site_seed)
// >> 8 >= p * 2^24, so the backward pass regenerates them and tests can rebuild them on the host.
#include <math.h>
#include <stdlib.h>

#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "rollout_train.h"
#include "train_blocks.h"
#include "sf_arena.h"
#include "dropout_mask.h"   // site_seed / sf_keep / drop_thresh: the mask convention, shared with phyre_readout_train.hip

// y = res + keep(x) / (1 - p)   (res may be NULL); n4 float4 elements
__global__ __launch_bounds__(256) void residual_dropout_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                               float* __restrict__ y, long long n4, uint32_t sseed,
                                                               uint32_t thresh, float inv_keep) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 v = reinterpret_cast<const float4*>(x)[i];
  float4 r = res ? reinterpret_cast<const float4*>(res)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t e = (uint32_t)(4 * i);
  r.x += sf_keep(sseed, e, thresh) ? v.x * inv_keep : 0.f;
  r.y += sf_keep(sseed, e + 1, thresh) ? v.y * inv_keep : 0.f;
  r.z += sf_keep(sseed, e + 2, thresh) ? v.z * inv_keep : 0.f;
  r.w += sf_keep(sseed, e + 3, thresh) ? v.w * inv_keep : 0.f;
  reinterpret_cast<float4*>(y)[i] = r;
}

// ---------------------------------------------------------------------------------------------------------------------
// window assembly:  x0[b, l, :] = tok[s + l / N][b * N + l % N][:] + pe[l]   and its adjoint (dtok += dx)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_assemble_kernel(const float* __restrict__ tok, const float* __restrict__ pe,
                                                              float* __restrict__ x0, int B, int L, int N, int d4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * L * d4;
  if (i >= total) return;
  const int c = (int)(i % d4);
  const int row = (int)(i / d4);
  const int b = row / L, l = row - b * L;
  const int f = l / N, n = l - f * N;
  const float4 t = reinterpret_cast<const float4*>(tok)[((long long)f * B * N + (long long)b * N + n) * d4 + c];
  const float4 p = reinterpret_cast<const float4*>(pe)[(long long)l * d4 + c];
  reinterpret_cast<float4*>(x0)[i] = make_float4(t.x + p.x, t.y + p.y, t.z + p.z, t.w + p.w);
}
__global__ __launch_bounds__(256) void window_scatter_kernel(const float* __restrict__ dx, float* __restrict__ dtok, int B,
                                                             int L, int N, int d4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)B * L * d4;
  if (i >= total) return;
  const int c = (int)(i % d4);
  const int row = (int)(i / d4);
  const int b = row / L, l = row - b * L;
  const int f = l / N, n = l - f * N;
  float4* dst = reinterpret_cast<float4*>(dtok) + ((long long)f * B * N + (long long)b * N + n) * d4 + c;
  const float4 g = reinterpret_cast<const float4*>(dx)[i];
  float4 t = *dst;
  t.x += g.x; t.y += g.y; t.z += g.z; t.w += g.w;
  *dst = t;
}

// adjoint of the "+ pe[l]" of the window assembly: dpe[l, :] += sum_b dx[b, l, :]   (one thread per (l, float4 column), the batch
// in a loop: L * d / 4 <= 8192 threads, each reading B rows d floats apart in the same column -> coalesced across the workgroup)
__global__ __launch_bounds__(256) void pe_grad_kernel(const float* __restrict__ dx, float* __restrict__ dpe, int B, int L, int d4) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L * d4) return;
  float4 a = reinterpret_cast<float4*>(dpe)[i];
  for (int b = 0; b < B; ++b) {
    const float4 g = reinterpret_cast<const float4*>(dx)[(long long)b * L * d4 + i];
    a.x += g.x; a.y += g.y; a.z += g.z; a.w += g.w;
  }
  reinterpret_cast<float4*>(dpe)[i] = a;
}

// y += x  (float4)
__global__ __launch_bounds__(256) void add_inplace_kernel(float* __restrict__ y, const float* __restrict__ x, long long n4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 a = reinterpret_cast<float4*>(y)[i];
  const float4 b = reinterpret_cast<const float4*>(x)[i];
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  reinterpret_cast<float4*>(y)[i] = a;
}

// ---------------------------------------------------------------------------------------------------------------------
// attention with saved-nothing backward: one workgroup per (head, video); L <= 128, head_dim <= 64.
// qkv [B*L, 3d] (q|k|v); ctx / dctx [B*L, d]; dqkv [B*L, 3d].  Dropout acts on the softmax weights (nn.MultiheadAttention).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void attn_probs(const float* qkv, int L, int d, int hd, int b, int h, float scale, float* q,
                                           float* k, float* v, float* P, int hp, int lp) {
  const int tid = threadIdx.x;
  for (int i = tid; i < L * hd; i += 256) {
    const int r = i / hd, c = i - r * hd;
    const float* row = qkv + ((long long)b * L + r) * 3 * d + h * hd + c;
    q[r * hp + c] = row[0] * scale;
    k[r * hp + c] = row[d];
    v[r * hp + c] = row[2 * d];
  }
  __syncthreads();
  for (int i = tid; i < L * L; i += 256) {
    const int r = i / L, c = i - r * L;
    float s = 0.f;
    for (int e = 0; e < hd; ++e) s = fmaf(q[r * hp + e], k[c * hp + e], s);
    P[r * lp + c] = s;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < L; r += 4) {
    const float a0 = lane < L ? P[r * lp + lane] : -INFINITY;
    const float a1 = lane + 64 < L ? P[r * lp + lane + 64] : -INFINITY;
    const float mx = sf_wave_max(fmaxf(a0, a1));
    const float e0 = lane < L ? __expf(a0 - mx) : 0.f;
    const float e1 = lane + 64 < L ? __expf(a1 - mx) : 0.f;
    const float inv = 1.f / sf_wave_sum(e0 + e1);
    if (lane < L) P[r * lp + lane] = e0 * inv;
    if (lane + 64 < L) P[r * lp + lane + 64] = e1 * inv;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void attn_train_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, int L,
                                                             int d, int hd, float scale, uint32_t sseed, uint32_t thresh,
                                                             float inv_keep) {
  extern __shared__ float lds[];
  const int hp = hd + 1, lp = L + 1;
  float* q = lds;
  float* k = q + L * hp;
  float* v = k + L * hp;
  float* P = v + L * hp;
  const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
  attn_probs(qkv, L, d, hd, b, h, scale, q, k, v, P, hp, lp);
  const int tid = threadIdx.x;
  const uint32_t base = (uint32_t)(((long long)b * H + h) * L * L);
  for (int i = tid; i < L * hd; i += 256) {
    const int r = i / hd, c = i - r * hd;
    float s = 0.f;
    for (int j = 0; j < L; ++j) {
      float p = P[r * lp + j];
      if (thresh) p = sf_keep(sseed, base + r * L + j, thresh) ? p * inv_keep : 0.f;
      s = fmaf(p, v[j * hp + c], s);
    }
    ctx[((long long)b * L + r) * d + h * hd + c] = s;
  }
}

__global__ __launch_bounds__(256) void attn_train_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                             float* __restrict__ dqkv, int L, int d, int hd, float scale,
                                                             uint32_t sseed, uint32_t thresh, float inv_keep) {
  extern __shared__ float lds[];
  const int hp = hd + 1, lp = L + 1;
  float* q = lds;
  float* k = q + L * hp;
  float* v = k + L * hp;
  float* g = v + L * hp;
  float* P = g + L * hp;
  float* dS = P + L * lp;
  const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
  const int tid = threadIdx.x;
  for (int i = tid; i < L * hd; i += 256) {
    const int r = i / hd, c = i - r * hd;
    g[r * hp + c] = dctx[((long long)b * L + r) * d + h * hd + c];
  }
  attn_probs(qkv, L, d, hd, b, h, scale, q, k, v, P, hp, lp);   // q holds q * scale
  const uint32_t base = (uint32_t)(((long long)b * H + h) * L * L);
  // dPd[i][j] = g[i] . v[j];  dP = mask * dPd / keep;  stash dP in dS
  for (int i = tid; i < L * L; i += 256) {
    const int r = i / L, c = i - r * L;
    float s = 0.f;
    for (int e = 0; e < hd; ++e) s = fmaf(g[r * hp + e], v[c * hp + e], s);
    if (thresh) s = sf_keep(sseed, base + r * L + c, thresh) ? s * inv_keep : 0.f;
    dS[r * lp + c] = s;
  }
  __syncthreads();
  // dV[j][c] = sum_i Pd[i][j] g[i][c]   (Pd = dropped probabilities)
  for (int i = tid; i < L * hd; i += 256) {
    const int j = i / hd, c = i - j * hd;
    float s = 0.f;
    for (int r = 0; r < L; ++r) {
      float p = P[r * lp + j];
      if (thresh) p = sf_keep(sseed, base + r * L + j, thresh) ? p * inv_keep : 0.f;
      s = fmaf(p, g[r * hp + c], s);
    }
    dqkv[((long long)b * L + j) * 3 * d + 2 * d + h * hd + c] = s;
  }
  __syncthreads();
  // dS = P * (dP - rowsum(dP * P))
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < L; r += 4) {
    const float p0 = lane < L ? P[r * lp + lane] : 0.f, p1 = lane + 64 < L ? P[r * lp + lane + 64] : 0.f;
    const float d0 = lane < L ? dS[r * lp + lane] : 0.f, d1 = lane + 64 < L ? dS[r * lp + lane + 64] : 0.f;
    const float dot = sf_wave_sum(p0 * d0 + p1 * d1);
    if (lane < L) dS[r * lp + lane] = p0 * (d0 - dot);
    if (lane + 64 < L) dS[r * lp + lane + 64] = p1 * (d1 - dot);
  }
  __syncthreads();
  // dq[i][c] = scale * sum_j dS[i][j] k[j][c];  dk[j][c] = sum_i dS[i][j] (q[i][c] * scale)
  for (int i = tid; i < L * hd; i += 256) {
    const int r = i / hd, c = i - r * hd;
    float sq = 0.f, sk = 0.f;
    for (int j = 0; j < L; ++j) {
      sq = fmaf(dS[r * lp + j], k[j * hp + c], sq);
      sk = fmaf(dS[j * lp + r], q[j * hp + c], sk);
    }
    float* o = dqkv + ((long long)b * L + r) * 3 * d + h * hd + c;
    o[0] = sq * scale;
    o[d] = sk;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same two kernels on the exact-f32 matrix pipe (v_mfma_f32_32x32x2_f32) for head_dim 32 / 64 and windows of at most
// 96 tokens: every product (q k^T, P v, g v^T, Pd^T g, dS k, dS^T q) is a set of 32x32 output tiles whose operands are
// read from zero-padded LDS tiles through (row, k) -> address functors, one tile per wave at a time.
// ---------------------------------------------------------------------------------------------------------------------

// load q (scaled), k, v [L, HD] of (video b, head h) into zero-padded [Lp][HD + 1] tiles
template <int HD>
__device__ __forceinline__ void attn_load_qkv(const float* qkv, int L, int Lp, int d, int b, int h, float scale, float* q,
                                              float* k, float* v) {
  constexpr int HP = HD + 1, C4 = HD / 4;
  for (int i = threadIdx.x; i < Lp * C4; i += 256) {
    const int r = i / C4, c = (i - r * C4) * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a, cc = a;
    if (r < L) {
      const float* row = qkv + ((long long)b * L + r) * 3 * d + h * HD + c;
      a = *reinterpret_cast<const float4*>(row);
      bb = *reinterpret_cast<const float4*>(row + d);
      cc = *reinterpret_cast<const float4*>(row + 2 * d);
    }
    float* qo = q + r * HP + c;
    float* ko = k + r * HP + c;
    float* vo = v + r * HP + c;
    qo[0] = a.x * scale; qo[1] = a.y * scale; qo[2] = a.z * scale; qo[3] = a.w * scale;
    ko[0] = bb.x; ko[1] = bb.y; ko[2] = bb.z; ko[3] = bb.w;
    vo[0] = cc.x; vo[1] = cc.y; vo[2] = cc.z; vo[3] = cc.w;
  }
}

// S = q k^T into P (all Lp x Lp tiles), then row softmax.  P <- probabilities (zero outside L x L); if Pd != nullptr it
// receives the dropped probabilities, else (drop_in_place) P itself is dropped.
template <int HD>
__device__ __forceinline__ void attn_probs_mfma(const float* q, const float* k, float* P, float* Pd, bool drop_in_place, int L,
                                                int Lp, uint32_t sseed, uint32_t thresh, float inv_keep, uint32_t base) {
  constexpr int HP = HD + 1;
  const int lp = Lp + 1, nt = Lp / 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = wave; t < nt * nt; t += 4) {
    const int ti = (t / nt) * 32, tj = (t % nt) * 32;
    const f32x16 acc = sf_mm32<false>([&](int i, int kk) { return q[(ti + i) * HP + kk]; },
                            [&](int kk, int j) { return k[(tj + j) * HP + kk]; }, HD, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) P[(ti + MM_ROW(r, lane)) * lp + tj + (lane & 31)] = acc[r];
  }
  __syncthreads();
  for (int r = wave; r < Lp; r += 4) {
    float p0 = 0.f, p1 = 0.f;
    if (r < L) {
      const float a0 = lane < L ? P[r * lp + lane] : -INFINITY;
      const float a1 = lane + 64 < L ? P[r * lp + lane + 64] : -INFINITY;
      const float mx = sf_wave_max(fmaxf(a0, a1));
      const float e0 = lane < L ? __expf(a0 - mx) : 0.f;
      const float e1 = lane + 64 < L ? __expf(a1 - mx) : 0.f;
      const float inv = 1.f / sf_wave_sum(e0 + e1);
      p0 = e0 * inv;
      p1 = e1 * inv;
    }
    float d0 = p0, d1 = p1;
    if (thresh && r < L) {
      d0 = sf_keep(sseed, base + r * L + lane, thresh) ? p0 * inv_keep : 0.f;
      d1 = sf_keep(sseed, base + r * L + lane + 64, thresh) ? p1 * inv_keep : 0.f;
    }
    if (lane < Lp) {
      P[r * lp + lane] = drop_in_place ? d0 : p0;
      if (Pd) Pd[r * lp + lane] = d0;
    }
    if (lane + 64 < Lp) {
      P[r * lp + lane + 64] = drop_in_place ? d1 : p1;
      if (Pd) Pd[r * lp + lane + 64] = d1;
    }
  }
  __syncthreads();
}

template <int HD>
__global__ __launch_bounds__(256) void attn_train_fwd_mfma_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, int L,
                                                                  int Lp, int d, float scale, uint32_t sseed, uint32_t thresh,
                                                                  float inv_keep) {
  extern __shared__ float lds[];
  constexpr int HP = HD + 1;
  const int lp = Lp + 1, nt = Lp / 32;
  float* q = lds;
  float* k = q + Lp * HP;
  float* v = k + Lp * HP;
  float* P = v + Lp * HP;
  const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  attn_load_qkv<HD>(qkv, L, Lp, d, b, h, scale, q, k, v);
  __syncthreads();
  attn_probs_mfma<HD>(q, k, P, nullptr, true, L, Lp, sseed, thresh, inv_keep, (uint32_t)(((long long)b * H + h) * L * L));
  const int Le = (L + 1) & ~1;
  for (int t = wave; t < nt * (HD / 32); t += 4) {
    const int ti = (t / (HD / 32)) * 32, tj = (t % (HD / 32)) * 32;
    const f32x16 acc = sf_mm32<false>([&](int i, int kk) { return P[(ti + i) * lp + kk]; },
                            [&](int kk, int j) { return v[kk * HP + tj + j]; }, Le, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ti + MM_ROW(r, lane);
      if (row < L) ctx[((long long)b * L + row) * d + h * HD + tj + (lane & 31)] = acc[r];
    }
  }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_train_bwd_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                                  float* __restrict__ dqkv, int L, int Lp, int d, float scale,
                                                                  uint32_t sseed, uint32_t thresh, float inv_keep) {
  extern __shared__ float lds[];
  constexpr int HP = HD + 1, C4 = HD / 4, HT = HD / 32;
  const int lp = Lp + 1, nt = Lp / 32;
  float* q = lds;
  float* k = q + Lp * HP;
  float* v = k + Lp * HP;
  float* g = v + Lp * HP;
  float* P = g + Lp * HP;
  float* dS = P + Lp * lp;
  const int h = blockIdx.x, b = blockIdx.y, H = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  attn_load_qkv<HD>(qkv, L, Lp, d, b, h, scale, q, k, v);
  for (int i = threadIdx.x; i < Lp * C4; i += 256) {
    const int r = i / C4, c = (i - r * C4) * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < L) a = *reinterpret_cast<const float4*>(dctx + ((long long)b * L + r) * d + h * HD + c);
    float* go = g + r * HP + c;
    go[0] = a.x; go[1] = a.y; go[2] = a.z; go[3] = a.w;
  }
  __syncthreads();
  // P = softmax, dS buffer = dropped probabilities Pd
  attn_probs_mfma<HD>(q, k, P, dS, false, L, Lp, sseed, thresh, inv_keep, (uint32_t)(((long long)b * H + h) * L * L));
  const int Le = (L + 1) & ~1;
  // dPd = g v^T (kept in registers: at most 3 tiles per wave for Lp = 96)
  f32x16 dp[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    const int t = wave + 4 * n;
    if (t < nt * nt) {
      const int ti = (t / nt) * 32, tj = (t % nt) * 32;
      dp[n] = sf_mm32<false>([&](int i, int kk) { return g[(ti + i) * HP + kk]; }, [&](int kk, int j) { return v[(tj + j) * HP + kk]; }, HD,
                   lane);
    }
  }
  // dV = Pd^T g
  for (int t = wave; t < nt * HT; t += 4) {
    const int ti = (t / HT) * 32, tj = (t % HT) * 32;
    const f32x16 acc = sf_mm32<false>([&](int i, int kk) { return dS[kk * lp + ti + i]; },
                            [&](int kk, int j) { return g[kk * HP + tj + j]; }, Le, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ti + MM_ROW(r, lane);
      if (row < L) dqkv[((long long)b * L + row) * 3 * d + 2 * d + h * HD + tj + (lane & 31)] = acc[r];
    }
  }
  __syncthreads();
  // dP = mask * dPd / keep  (the mask is where Pd is non-zero: softmax weights are strictly positive), over Pd in place
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    const int t = wave + 4 * n;
    if (t < nt * nt) {
      const int ti = (t / nt) * 32, tj = (t % nt) * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* e = &dS[(ti + MM_ROW(r, lane)) * lp + tj + (lane & 31)];
        *e = (thresh == 0 || *e != 0.f) ? dp[n][r] * (thresh ? inv_keep : 1.f) : 0.f;
      }
    }
  }
  __syncthreads();
  // dS = P * (dP - rowsum(dP * P))
  for (int r = wave; r < L; r += 4) {
    const float p0 = lane < L ? P[r * lp + lane] : 0.f, p1 = lane + 64 < L ? P[r * lp + lane + 64] : 0.f;
    const float d0 = lane < L ? dS[r * lp + lane] : 0.f, d1 = lane + 64 < L ? dS[r * lp + lane + 64] : 0.f;
    const float dot = sf_wave_sum(p0 * d0 + p1 * d1);
    if (lane < Lp) dS[r * lp + lane] = p0 * (d0 - dot);
    if (lane + 64 < Lp) dS[r * lp + lane + 64] = p1 * (d1 - dot);
  }
  __syncthreads();
  // dq = scale * dS k (tiles 0 .. nt*HT-1), dk = dS^T (q * scale) (the next nt*HT tiles)
  for (int t = wave; t < 2 * nt * HT; t += 4) {
    const bool isk = t >= nt * HT;
    const int tt = isk ? t - nt * HT : t;
    const int ti = (tt / HT) * 32, tj = (tt % HT) * 32;
    f32x16 acc;
    if (!isk)
      acc = sf_mm32<false>([&](int i, int kk) { return dS[(ti + i) * lp + kk]; }, [&](int kk, int j) { return k[kk * HP + tj + j]; }, Le,
                 lane);
    else
      acc = sf_mm32<false>([&](int i, int kk) { return dS[kk * lp + ti + i]; }, [&](int kk, int j) { return q[kk * HP + tj + j]; }, Le,
                 lane);
    const float sc = isk ? 1.f : scale;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = ti + MM_ROW(r, lane);
      if (row < L) dqkv[((long long)b * L + row) * 3 * d + (isk ? d : 0) + h * HD + tj + (lane & 31)] = acc[r] * sc;
    }
  }
}

// gradient w.r.t. the final layer output: zero except the last N tokens of every video (dxlast [B*N, d]); dfo = the same
// pushed through the top layer's FFN-output dropout
__global__ __launch_bounds__(256) void scatter_last_kernel(const float* __restrict__ dxlast, float* __restrict__ dx,
                                                           float* __restrict__ dfo, int B, int L, int N, int d4,
                                                           uint32_t sseed, uint32_t thresh, float inv_keep) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * L * d4) return;
  const int c = (int)(i % d4);
  const int row = (int)(i / d4);
  const int b = row / L, l = row - b * L;
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (l >= L - N) r = reinterpret_cast<const float4*>(dxlast)[((long long)b * N + (l - (L - N))) * d4 + c];
  reinterpret_cast<float4*>(dx)[i] = r;
  if (thresh) {
    const uint32_t e = (uint32_t)(4 * i);
    r.x = sf_keep(sseed, e, thresh) ? r.x * inv_keep : 0.f;
    r.y = sf_keep(sseed, e + 1, thresh) ? r.y * inv_keep : 0.f;
    r.z = sf_keep(sseed, e + 2, thresh) ? r.z * inv_keep : 0.f;
    r.w = sf_keep(sseed, e + 3, thresh) ? r.w * inv_keep : 0.f;
  }
  reinterpret_cast<float4*>(dfo)[i] = r;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
namespace {

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

struct Dims {
  int B, S, hist, N, C, d, ffn, nl, H, L, M, R, T;   // L, M: the largest window (tokens per video, rows per step)
  int W, single;                                      // window length in frames; growing-window (single-step) rollouter
  // step s sees frames f0(s) .. f0(s) + Lw(s)/N - 1 (single_step_slotformer.py:79-88: the window grows to W frames first)
  int Lw(int s) const { return (single ? (s + 1 < W ? s + 1 : W) : W) * N; }
  int f0(int s) const { return single ? (s + 1 > W ? s + 1 - W : 0) : s; }
  size_t off(int s) const {   // rows of all steps before s in the stacked buffers
    size_t r = 0;
    for (int i = 0; i < s; ++i) r += (size_t)B * Lw(i);
    return r;
  }
};

// workspace carve-up (in floats); identical for forward and backward
struct Ws {
  float *slots_all, *tok_all, *xf, *xlast, *tmp;
  float *xin[16], *a1[16], *qkv[16], *ctx[16], *xmid[16], *a2[16], *hdn[16];
  // backward only
  float *dtok, *dpred, *dx, *dx2, *dctx, *dxlast;
  float *dqkv[16], *dao[16], *dpre[16], *dfo[16], *da1[16], *da2[16];
  float *wt_in[16], *wt_o[16], *wt_1[16], *wt_2[16], *wt_inproj, *wt_outproj;
  float* partial;
  size_t bytes;   // of the carve
};

inline size_t tn_partial_floats(const Dims& D);

constexpr size_t WS_SLACK = 256;   // bytes a caller's workspace holds beyond the carve

Ws carve(const Dims& D, void* ws) {
  Ws w;
  memset(&w, 0, sizeof(w));
  SfArena a(ws);
  const size_t M = D.M, R = D.R, S = D.S, d = D.d, f = D.ffn, Mt = D.off(D.S);
  w.slots_all = a.take((size_t)D.T * R * D.C);
  w.tok_all = a.take((size_t)D.T * R * d);
  w.xf = a.take(Mt * d);
  w.xlast = a.take(S * R * d);
  w.tmp = a.take(M * (f > 3 * d ? f : 3 * d));
  for (int l = 0; l < D.nl; ++l) {
    w.xin[l] = a.take(Mt * d);
    w.a1[l] = a.take(Mt * d);
    w.qkv[l] = a.take(Mt * 3 * d);
    w.ctx[l] = a.take(Mt * d);
    w.xmid[l] = a.take(Mt * d);
    w.a2[l] = a.take(Mt * d);
    w.hdn[l] = a.take(Mt * f);
  }
  w.dtok = a.take((size_t)D.T * R * d);
  w.dpred = a.take(S * R * D.C);
  w.dx = a.take(M * d);
  w.dx2 = a.take(M * d);
  w.dctx = a.take(M * d);
  w.dxlast = a.take(R * d);
  for (int l = 0; l < D.nl; ++l) {
    w.dqkv[l] = a.take(Mt * 3 * d);
    w.dao[l] = a.take(Mt * d);
    w.dpre[l] = a.take(Mt * f);
    w.dfo[l] = a.take(Mt * d);
    w.da1[l] = a.take(Mt * d);
    w.da2[l] = a.take(Mt * d);
    w.wt_in[l] = a.take(3 * d * d);
    w.wt_o[l] = a.take(d * d);
    w.wt_1[l] = a.take(f * d);
    w.wt_2[l] = a.take(f * d);
  }
  w.wt_inproj = a.take((size_t)D.C * d);
  w.wt_outproj = a.take((size_t)D.C * d);
  w.partial = a.take(tn_partial_floats(D));
  w.bytes = a.bytes();
  return w;
}

inline size_t tn_partial_floats(const Dims& D) {
  const long long rows = (long long)D.off(D.S);
  size_t best = 0;
  auto upd = [&](long long r, int N, int K) {
    const size_t n = (size_t)tn_splits(r, N, K) * N * K;
    if (n > best) best = n;
  };
  upd(rows, 3 * D.d, D.d);
  upd(rows, D.d, D.d);
  upd(rows, D.ffn, D.d);
  upd(rows, D.d, D.ffn);
  upd((long long)D.T * D.R, D.d, D.C);
  upd((long long)D.S * D.R, D.C, D.d);
  // column-sum / LayerNorm partials share the buffer (the LayerNorms are d wide: their scratch record fits behind the group records of 3 d)
  const size_t cs = sf_colsum_partial_floats(D.ffn > 3 * D.d ? D.ffn : 3 * D.d, 0);
  return best > cs ? best : cs;
}

inline bool attn_use_mfma(int L, int hd) {
  return (hd == 32 || hd == 64) && L <= 96;
}
// dynamic LDS of the training-attention kernel that launch_attn_fwd / launch_attn_bwd pick for (L, hd): the MFMA kernels
// keep zero-padded tiles of Lp = L rounded up to 32 rows, the scalar ones L rows
size_t attn_lds_bytes(int L, int hd, bool bwd) {
  const size_t l = attn_use_mfma(L, hd) ? (size_t)((L + 31) & ~31) : (size_t)L;
  return ((bwd ? 4 : 3) * l * (hd + 1) + (bwd ? 2 : 1) * l * (l + 1)) * sizeof(float);
}
constexpr size_t kAttnLdsMax = (size_t)160 * 1024;   // the LDS of one CU: the most one workgroup can get
// the (L, head_dim) a training attention accepts: both of its kernels fit the LDS (the backward needs more)
inline bool attn_shape_fits(int L, int hd) {
  return L >= 1 && L <= 128 && hd >= 1 && hd <= 64 && attn_lds_bytes(L, hd, true) <= kAttnLdsMax;
}
int check_model(const sf_rollouter* m, Dims& D, int B, int pred_len) {
  SF_REQUIRE(m && m->layers, "null model");
  SF_REQUIRE(m->norm_first, "training needs norm_first layers (all reference configurations)");
  SF_REQUIRE(B > 0 && pred_len > 0, "bad sizes");
  D.B = B; D.S = pred_len; D.W = m->window_len; D.single = m->single_step ? 1 : 0; D.hist = D.single ? 1 : D.W;
  D.N = m->num_slots; D.C = m->slot_size; D.d = m->d_model;
  D.ffn = m->ffn_dim; D.nl = m->num_layers; D.H = m->num_heads;
  D.L = D.W * D.N; D.M = B * D.L; D.R = B * D.N; D.T = D.hist + pred_len;
  SF_REQUIRE(D.nl >= 1 && D.nl <= 16, "1..16 layers");
  SF_REQUIRE(D.d % 64 == 0 && D.ffn % 64 == 0 && D.C % 64 == 0, "slot_size, d_model and ffn_dim must be multiples of 64");
  SF_REQUIRE(D.d <= 1024, "d_model <= 1024");
  SF_REQUIRE(D.d % D.H == 0 && D.d / D.H <= 64, "head_dim <= 64");
  SF_REQUIRE(D.L <= 128, "window of at most 128 tokens");
  SF_REQUIRE(attn_shape_fits(D.L, D.d / D.H), "attention tile does not fit the 160 KB of LDS");   // (the largest window needs the most)
  return 0;
}

int gemm(const float* A, const float* W, const float* bias, const float* res, float* Cc, int M, int N, int K, int relu,
         hipStream_t st) {
  return sf_linear_ex(A, sf_rows(K), W, bias, nullptr, nullptr, 0.f, res, sf_rows(N), 0, Cc, sf_rows(N), M, N, K, relu, st);
}

template <class Kern>
int set_lds(Kern kern, size_t bytes) {
  if (bytes <= 64 * 1024) return 0;
  return sf_ensure_dyn_lds((const void*)kern, kAttnLdsMax);
}
int launch_attn_fwd(const float* qkv, float* ctx, int B, int H, int L, int d, uint32_t sseed, uint32_t thr, float inv_keep,
                    hipStream_t st) {
  const int hd = d / H;
  const float scale = 1.f / sqrtf((float)hd);
  const size_t bytes = attn_lds_bytes(L, hd, false);
  SF_REQUIRE(bytes <= kAttnLdsMax, "attention tile does not fit the 160 KB of LDS");
  if (attn_use_mfma(L, hd)) {
    const int Lp = (L + 31) & ~31;
    if (hd == 32) {
      SF_TRY(set_lds(attn_train_fwd_mfma_kernel<32>, bytes));
      hipLaunchKernelGGL(attn_train_fwd_mfma_kernel<32>, dim3(H, B), dim3(256), bytes, st, qkv, ctx, L, Lp, d, scale, sseed, thr,
                         inv_keep);
    } else {
      SF_TRY(set_lds(attn_train_fwd_mfma_kernel<64>, bytes));
      hipLaunchKernelGGL(attn_train_fwd_mfma_kernel<64>, dim3(H, B), dim3(256), bytes, st, qkv, ctx, L, Lp, d, scale, sseed, thr,
                         inv_keep);
    }
  } else {
    SF_TRY(set_lds(attn_train_fwd_kernel, bytes));
    hipLaunchKernelGGL(attn_train_fwd_kernel, dim3(H, B), dim3(256), bytes, st, qkv, ctx, L, d, hd, scale, sseed, thr, inv_keep);
  }
  SF_CHECK_LAUNCH();
  return 0;
}
int launch_attn_bwd(const float* qkv, const float* dctx, float* dqkv, int B, int H, int L, int d, uint32_t sseed, uint32_t thr,
                    float inv_keep, hipStream_t st) {
  const int hd = d / H;
  const float scale = 1.f / sqrtf((float)hd);
  const size_t bytes = attn_lds_bytes(L, hd, true);
  SF_REQUIRE(bytes <= kAttnLdsMax, "attention tile does not fit the 160 KB of LDS");
  if (attn_use_mfma(L, hd)) {
    const int Lp = (L + 31) & ~31;
    if (hd == 32) {
      SF_TRY(set_lds(attn_train_bwd_mfma_kernel<32>, bytes));
      hipLaunchKernelGGL(attn_train_bwd_mfma_kernel<32>, dim3(H, B), dim3(256), bytes, st, qkv, dctx, dqkv, L, Lp, d, scale, sseed,
                         thr, inv_keep);
    } else {
      SF_TRY(set_lds(attn_train_bwd_mfma_kernel<64>, bytes));
      hipLaunchKernelGGL(attn_train_bwd_mfma_kernel<64>, dim3(H, B), dim3(256), bytes, st, qkv, dctx, dqkv, L, Lp, d, scale, sseed,
                         thr, inv_keep);
    }
  } else {
    SF_TRY(set_lds(attn_train_bwd_kernel, bytes));
    hipLaunchKernelGGL(attn_train_bwd_kernel, dim3(H, B), dim3(256), bytes, st, qkv, dctx, dqkv, L, d, hd, scale, sseed, thr,
                       inv_keep);
  }
  SF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// The training forward from the point where the burn-in frames lie frame-major in the workspace's slots_all ([hist][B * N][C]): their
// in-projections, then every step.  sf_rollout_train_fwd_f32 copies x there, sf_rollout_train_clips_fwd_f32 (clip_train.hip) reads a slot table.
int sf_rollout_train_steps_ex(const sf_rollouter* m, float* pred, int B, int pred_len, float dropout_p, unsigned long long seed, void* ws,
                              size_t ws_bytes, hipStream_t st) {
  Dims D;
  SF_TRY(check_model(m, D, B, pred_len));
  SF_REQUIRE(pred && ws, "null pointer");
  SF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p in [0, 1)");
  const Ws w = carve(D, ws);
  SF_REQUIRE(w.bytes + WS_SLACK <= ws_bytes, "workspace too small");
  const int d = D.d, f = D.ffn, R = D.R, N = D.N, C = D.C, hd = d / D.H;
  const uint32_t thr = drop_thresh(dropout_p);
  const float inv_keep = 1.f / (1.f - dropout_p);
  const float scale = 1.f / sqrtf((float)hd);

  SF_TRY(gemm(w.slots_all, m->in_proj_w, m->in_proj_b, nullptr, w.tok_all, D.hist * R, d, C, 0, st));

  for (int s = 0; s < D.S; ++s) {
    const size_t so = D.off(s);
    const int L = D.Lw(s), M = B * L;   // this step's window
    if (s > 0) {
      const int fr = D.hist + s - 1;
      SF_TRY(gemm(w.slots_all + (size_t)fr * R * C, m->in_proj_w, m->in_proj_b, nullptr, w.tok_all + (size_t)fr * R * d, R,
                  d, C, 0, st));
    }
    hipLaunchKernelGGL(window_assemble_kernel, dim3(cdiv((long long)M * d / 4, 256)), dim3(256), 0, st,
                       w.tok_all + (size_t)D.f0(s) * R * d, m->pe_tok + (size_t)(D.L - L) * d, w.xin[0] + so * d, B, L, N, d / 4);
    SF_CHECK_LAUNCH();
    for (int l = 0; l < D.nl; ++l) {
      const sf_tfm_layer& ly = m->layers[l];
      float* xin = w.xin[l] + so * d;
      float* a1 = w.a1[l] + so * d;
      float* qkv = w.qkv[l] + so * 3 * d;
      float* ctx = w.ctx[l] + so * d;
      float* xmid = w.xmid[l] + so * d;
      float* a2 = w.a2[l] + so * d;
      float* hdn = w.hdn[l] + so * f;
      float* xnext = (l + 1 < D.nl ? w.xin[l + 1] : w.xf) + so * d;
      SF_TRY(sf_layernorm_ex(xin, sf_rows(d), ly.norm1_g, ly.norm1_b, a1, sf_rows(d), M, d, 1e-5f, st));
      SF_TRY(gemm(a1, ly.in_proj_w, ly.in_proj_b, nullptr, qkv, M, 3 * d, d, 0, st));
      SF_TRY(launch_attn_fwd(qkv, ctx, B, D.H, L, d, site_seed(seed, s, l, SITE_ATTN_P), thr, inv_keep, st));
      SF_TRY(sf_linear_dropout_ex(ctx, ly.out_proj_w, ly.out_proj_b, xin, xmid, M, d, d, 0, site_seed(seed, s, l, SITE_ATTN_O), thr,
                                  inv_keep, st));
      SF_TRY(sf_layernorm_ex(xmid, sf_rows(d), ly.norm2_g, ly.norm2_b, a2, sf_rows(d), M, d, 1e-5f, st));
      SF_TRY(sf_linear_dropout_ex(a2, ly.lin1_w, ly.lin1_b, nullptr, hdn, M, f, d, 1, site_seed(seed, s, l, SITE_FFN_H), thr, inv_keep,
                                  st));
      SF_TRY(sf_linear_dropout_ex(hdn, ly.lin2_w, ly.lin2_b, xmid, xnext, M, d, f, 0, site_seed(seed, s, l, SITE_FFN_O), thr,
                                  inv_keep, st));
    }
    // last N tokens of every video -> xlast[s]; prediction = out_proj(xlast)  (slotformer.py:121)
    SF_TRY(sf_copy_rows_ex(w.xf + so * d, sf_rows_batched(d, N, (long long)L * d, (long long)(L - N) * d),
                           w.xlast + (size_t)s * R * d, sf_rows(d), R, d, st));
    float* fr = w.slots_all + (size_t)(D.hist + s) * R * C;
    SF_TRY(gemm(w.xlast + (size_t)s * R * d, m->out_proj_w, m->out_proj_b, nullptr, fr, R, C, d, 0, st));
    SF_TRY(sf_copy_rows_ex(fr, sf_rows(C), pred, sf_rows_batched(C, N, (long long)D.S * N * C, (long long)s * N * C), R, C,
                           st));
  }
  return 0;
}

// Where the burn-in frames of a training forward go: validates as the forward does and returns slots_all and the burn-in length.
int sf_rollout_train_burnin_ex(const sf_rollouter* m, int B, int pred_len, void* ws, size_t ws_bytes, float** slots_all, int* hist) {
  Dims D;
  SF_TRY(check_model(m, D, B, pred_len));
  SF_REQUIRE(ws, "null pointer");
  const Ws w = carve(D, ws);
  SF_REQUIRE(w.bytes + WS_SLACK <= ws_bytes, "workspace too small");
  *slots_all = w.slots_all;
  *hist = D.hist;
  return 0;
}

extern "C" {

// attention core of nn.MultiheadAttention for training (qkv [B*L, 3d] -> ctx [B*L, d]; dropout on the softmax weights, masks
// a pure function of (seed, element)) and its backward (recomputes the probabilities; nothing saved but qkv)
int sf_mha_train_fwd_f32(const float* qkv, float* ctx, int B, int L, int d_model, int num_heads, float dropout_p,
                         unsigned long long seed, void* stream) {
  SF_REQUIRE(qkv && ctx && B > 0 && L > 0 && L <= 128 && num_heads > 0 && d_model % num_heads == 0 && d_model / num_heads <= 64,
             "bad attention shape");
  SF_REQUIRE(attn_shape_fits(L, d_model / num_heads), "attention tile does not fit the 160 KB of LDS");
  SF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p in [0, 1)");
  return launch_attn_fwd(qkv, ctx, B, num_heads, L, d_model, site_seed(seed, 0, 0, SITE_ATTN_P), drop_thresh(dropout_p),
                         1.f / (1.f - dropout_p), (hipStream_t)stream);
}
int sf_mha_train_bwd_f32(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int d_model, int num_heads,
                         float dropout_p, unsigned long long seed, void* stream) {
  SF_REQUIRE(qkv && d_ctx && d_qkv && B > 0 && L > 0 && L <= 128 && num_heads > 0 && d_model % num_heads == 0 &&
                 d_model / num_heads <= 64, "bad attention shape");
  SF_REQUIRE(attn_shape_fits(L, d_model / num_heads), "attention tile does not fit the 160 KB of LDS");
  return launch_attn_bwd(qkv, d_ctx, d_qkv, B, num_heads, L, d_model, site_seed(seed, 0, 0, SITE_ATTN_P), drop_thresh(dropout_p),
                         1.f / (1.f - dropout_p), (hipStream_t)stream);
}
// y = res + dropout(x) (res may be NULL); the backward of the dropout is the same call on the gradient
int sf_dropout_f32(const float* x, const float* res, float* y, long long n, float dropout_p, unsigned long long seed, void* stream) {
  SF_REQUIRE(x && y && n >= 0 && n % 4 == 0 && n < (1LL << 32), "bad dropout arguments");
  SF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p in [0, 1)");
  if (n == 0) return 0;
  hipLaunchKernelGGL(residual_dropout_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, x, res, y, n / 4,
                     site_seed(seed, 0, 0, SITE_ATTN_O), drop_thresh(dropout_p), 1.f / (1.f - dropout_p));
  SF_CHECK_LAUNCH();
  return 0;
}

size_t sf_rollout_train_workspace_bytes(const sf_rollouter* m, int B, int pred_len) {
  Dims D;
  if (check_model(m, D, B, pred_len) != 0) return 0;
  return carve(D, nullptr).bytes + WS_SLACK;
}

int sf_rollout_train_fwd_f32(const sf_rollouter* m, const float* x, float* pred, int B, int pred_len, float dropout_p,
                             unsigned long long seed, void* ws, size_t ws_bytes, void* stream) {
  float* slots_all = nullptr;
  int hist = 0;
  SF_TRY(sf_rollout_train_burnin_ex(m, B, pred_len, ws, ws_bytes, &slots_all, &hist));
  SF_REQUIRE(x && pred, "null pointer");
  SF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p in [0, 1)");
  hipStream_t st = (hipStream_t)stream;
  const int N = m->num_slots, C = m->slot_size, R = B * N;
  // burn-in frames -> frame-major slots_all
  for (int t = 0; t < hist; ++t)
    SF_TRY(sf_copy_rows_ex(x, sf_rows_batched(C, N, (long long)hist * N * C, (long long)t * N * C), slots_all + (size_t)t * R * C, sf_rows(C), R, C,
                           st));
  return sf_rollout_train_steps_ex(m, pred, B, pred_len, dropout_p, seed, ws, ws_bytes, st);
}

int sf_rollout_train_bwd_f32(const sf_rollouter* m, const float* d_pred, float* d_x, const sf_rollouter_grads* g, int B,
                             int pred_len, float dropout_p, unsigned long long seed, void* ws, size_t ws_bytes,
                             void* stream) {
  Dims D;
  SF_TRY(check_model(m, D, B, pred_len));
  SF_REQUIRE(d_pred && g && g->layers && ws, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const Ws w = carve(D, ws);
  SF_REQUIRE(w.bytes + WS_SLACK <= ws_bytes, "workspace too small");
  const int d = D.d, f = D.ffn, R = D.R, N = D.N, C = D.C, hd = d / D.H;
  const uint32_t thr = drop_thresh(dropout_p);
  const float inv_keep = 1.f / (1.f - dropout_p);
  const float scale = 1.f / sqrtf((float)hd);

  // transposed weight copies: the data-gradient GEMMs run on the forward core (C = A . W^T)
  for (int l = 0; l < D.nl; ++l) {
    const sf_tfm_layer& ly = m->layers[l];
    SF_TRY(sf_transpose_ex(ly.in_proj_w, w.wt_in[l], 3 * d, d, st));   // [3d,d] -> [d,3d]
    SF_TRY(sf_transpose_ex(ly.out_proj_w, w.wt_o[l], d, d, st));
    SF_TRY(sf_transpose_ex(ly.lin1_w, w.wt_1[l], f, d, st));           // [f,d] -> [d,f]
    SF_TRY(sf_transpose_ex(ly.lin2_w, w.wt_2[l], d, f, st));           // [d,f] -> [f,d]
  }
  SF_TRY(sf_transpose_ex(m->in_proj_w, w.wt_inproj, d, C, st));        // [d,C] -> [C,d]
  SF_TRY(sf_transpose_ex(m->out_proj_w, w.wt_outproj, C, d, st));      // [C,d] -> [d,C]

  hipError_t e = hipMemsetAsync(w.dtok, 0, (size_t)D.T * R * d * sizeof(float), st);
  if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  if (g->pe_tok) {
    e = hipMemsetAsync(g->pe_tok, 0, (size_t)D.L * d * sizeof(float), st);
    if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  }
  // d_pred [B,S,N,C] -> step-major dpred [S][R][C]
  for (int s = 0; s < D.S; ++s)
    SF_TRY(sf_copy_rows_ex(d_pred, sf_rows_batched(C, N, (long long)D.S * N * C, (long long)s * N * C),
                           w.dpred + (size_t)s * R * C, sf_rows(C), R, C, st));

  for (int s = D.S - 1; s >= 0; --s) {
    const size_t so = D.off(s);
    const int L = D.Lw(s), M = B * L;   // this step's window
    const long long Md4 = (long long)M * d / 4;
    float* dp = w.dpred + (size_t)s * R * C;
    // feedback through the in-projection of the predicted frame (zero for the last step)
    if (s + 1 < D.S) {
      SF_TRY(gemm(w.dtok + (size_t)(D.hist + s) * R * d, w.wt_inproj, nullptr, dp, dp, R, C, d, 0, st));
    }
    // through out_proj into the last N tokens of the final layer output
    SF_TRY(gemm(dp, w.wt_outproj, nullptr, nullptr, w.dxlast, R, d, C, 0, st));
    hipLaunchKernelGGL(scatter_last_kernel, dim3(cdiv(Md4, 256)), dim3(256), 0, st, w.dxlast, w.dx, w.dfo[D.nl - 1] + so * d, B, L, N,
                       d / 4, site_seed(seed, s, D.nl - 1, SITE_FFN_O), thr, inv_keep);
    SF_CHECK_LAUNCH();
    float* dx = w.dx;     // gradient w.r.t. the current layer's output
    float* dxo = w.dx2;   // gradient w.r.t. the layer's mid-point (after the attention block)
    for (int l = D.nl - 1; l >= 0; --l) {
      const sf_tfm_layer& ly = m->layers[l];
      float* dfo = w.dfo[l] + so * d;     // x2 = xmid + drop(ffn_o): filled by the stage above
      float* dpre = w.dpre[l] + so * f;
      float* da2 = w.da2[l] + so * d;
      float* dao = w.dao[l] + so * d;
      float* dqkv = w.dqkv[l] + so * 3 * d;
      float* da1 = w.da1[l] + so * d;
      // through linear2, the hidden dropout and the ReLU in one GEMM: the saved hidden activation is the mask
      SF_TRY(sf_linear_masked_ex(dfo, w.wt_2[l], w.hdn[l] + so * f, thr ? inv_keep : 1.f, dpre, M, f, d, st));
      SF_TRY(gemm(dpre, w.wt_1[l], nullptr, nullptr, da2, M, d, f, 0, st));
      // xmid = xin + drop(attn_o): dxo = gradient w.r.t. xmid, dao = the same through the attention-output dropout
      SF_TRY(sf_ln_bwd_dropout_ex(w.xmid[l] + so * d, da2, ly.norm2_g, dx, dxo, dao, site_seed(seed, s, l, SITE_ATTN_O), thr, inv_keep, M, d,
                                  1e-5f, st));
      SF_TRY(gemm(dao, w.wt_o[l], nullptr, nullptr, w.dctx, M, d, d, 0, st));
      SF_TRY(launch_attn_bwd(w.qkv[l] + so * 3 * d, w.dctx, dqkv, B, D.H, L, d, site_seed(seed, s, l, SITE_ATTN_P), thr, inv_keep,
                             st));
      SF_TRY(gemm(dqkv, w.wt_in[l], nullptr, nullptr, da1, M, d, 3 * d, 0, st));
      // dx = gradient w.r.t. this layer's input = the output of layer l-1, whose FFN-output dropout is folded in
      SF_TRY(sf_ln_bwd_dropout_ex(w.xin[l] + so * d, da1, ly.norm1_g, dxo, dx, l > 0 ? w.dfo[l - 1] + so * d : (float*)nullptr,
                                  site_seed(seed, s, l > 0 ? l - 1 : 0, SITE_FFN_O), thr, inv_keep, M, d, 1e-5f, st));
    }
    hipLaunchKernelGGL(window_scatter_kernel, dim3(cdiv(Md4, 256)), dim3(256), 0, st, dx, w.dtok + (size_t)D.f0(s) * R * d, B, L,
                       N, d / 4);
    SF_CHECK_LAUNCH();
    if (g->pe_tok) {   // learnable position tables: this step's window used rows D.L - L .. D.L - 1 of the folded table
      hipLaunchKernelGGL(pe_grad_kernel, dim3(cdiv((long long)L * d / 4, 256)), dim3(256), 0, st, dx, g->pe_tok + (size_t)(D.L - L) * d, B,
                         L, d / 4);
      SF_CHECK_LAUNCH();
    }
  }

  // gradient w.r.t. the burn-in slots
  if (d_x) {
    SF_TRY(gemm(w.dtok, w.wt_inproj, nullptr, nullptr, w.tmp, D.hist * R, C, d, 0, st));
    for (int t = 0; t < D.hist; ++t)
      SF_TRY(sf_copy_rows_ex(w.tmp + (size_t)t * R * C, sf_rows(C), d_x,
                             sf_rows_batched(C, N, (long long)D.hist * N * C, (long long)t * N * C), R, C, st));
  }

  // parameter gradients: one contraction per weight over all stacked rows.  The in-projection saw frames 0 .. T-2 (the
  // last predicted frame is never fed back).
  const long long rows = (long long)D.off(D.S);
  const long long in_rows = (long long)(D.T - 1) * R;
  SF_TRY(sf_grad_weight_ex(w.dtok, w.slots_all, g->in_proj_w, in_rows, d, C, w.partial, st));
  SF_TRY(sf_grad_bias_ex(w.dtok, g->in_proj_b, in_rows, d, w.partial, st));
  SF_TRY(sf_grad_weight_ex(w.dpred, w.xlast, g->out_proj_w, (long long)D.S * R, C, d, w.partial, st));
  SF_TRY(sf_grad_bias_ex(w.dpred, g->out_proj_b, (long long)D.S * R, C, w.partial, st));
  for (int l = 0; l < D.nl; ++l) {
    const sf_tfm_layer_grads& gl = g->layers[l];
    SF_TRY(sf_grad_weight_ex(w.dqkv[l], w.a1[l], gl.in_proj_w, rows, 3 * d, d, w.partial, st));
    SF_TRY(sf_grad_bias_ex(w.dqkv[l], gl.in_proj_b, rows, 3 * d, w.partial, st));
    SF_TRY(sf_grad_weight_ex(w.dao[l], w.ctx[l], gl.out_proj_w, rows, d, d, w.partial, st));
    SF_TRY(sf_grad_bias_ex(w.dao[l], gl.out_proj_b, rows, d, w.partial, st));
    SF_TRY(sf_grad_weight_ex(w.dpre[l], w.a2[l], gl.lin1_w, rows, f, d, w.partial, st));
    SF_TRY(sf_grad_bias_ex(w.dpre[l], gl.lin1_b, rows, f, w.partial, st));
    SF_TRY(sf_grad_weight_ex(w.dfo[l], w.hdn[l], gl.lin2_w, rows, d, f, w.partial, st));
    SF_TRY(sf_grad_bias_ex(w.dfo[l], gl.lin2_b, rows, d, w.partial, st));
    SF_TRY(sf_grad_ln_ex(w.xin[l], w.da1[l], gl.norm1_g, gl.norm1_b, rows, d, 1e-5f, w.partial, st));
    SF_TRY(sf_grad_ln_ex(w.xmid[l], w.da2[l], gl.norm2_g, gl.norm2_b, rows, d, 1e-5f, w.partial, st));
  }
  return 0;
}

}  // extern "C"

// The Physion VQA readout (physion_vqa/models/readout.py: PhysionReadout) on rolled-out slots, trained and scored:
//
//   logit[b] = max_t ( w2 . agg_{i<j} ( W1 cat(s_ti, s_tj) + b1 ) + b2 ),   agg in {max, sum, mean} over the N (N - 1) / 2 slot pairs
//
// linear1 of a pair is U_i + V_j with U = S Wa^T + b1, V = S Wb^T, Wa = W1[:, :C], Wb = W1[:, C:]: ONE product [T N, C] x [C, 2F] per video instead of
// a gathered [T, pairs, 2C] tensor and five times the FLOPs.
//
//   pr_fwd_kernel     one workgroup per (video, head).  The video's frames pass through in chunks of 48 / N whole timesteps (48 rows = three 16-row
//                     MFMA tiles; N = 6: eight timesteps): the rows are split into bf16 hi | lo planes in LDS, the eight waves sweep the 2F / 16 column
//                     tiles of U | V (v_mfma_f32_16x16x32_bf16; the head's W1 rows are read as f32 and split on the fly -- they change every training
//                     step, a packed copy would cost a launch per step -- 295 KB per head, L2-resident) and leave U | V as f32 in LDS; then a wave
//                     owns a timestep: lane = feature, pairs in itertools.combinations order, dot with w2 by a wave sum, + b2.  The running
//                     (max, first t) never leaves the wave until the eight meet behind the last barrier.  With pair_star requested the frame t_star
//                     is run once more (same products, same bits) and the first winning pair of every feature is written.
//   pr_route_kernel   backward, one workgroup per video: the relation at t_star again, then per feature the coefficients dL/dU[i], dL/dV[j] of the
//                     frame's N slots (max: the recorded / recomputed winning pair only; sum: (N-1-i) and j times dL/dR; mean: that / pairs) and
//                     the relation itself, into the workspace.
//   pr_wgrad_kernel   dW1[f][:] = sum_b sum_i coef[b][i][f] s[b, t_star_b, i, :]: one workgroup per feature, a thread per column, videos and slots
//                     in ascending order with one fma each -- no atomics, two runs give the same bits.  One more workgroup sums db1, dw2, db2.
//   pr_score_kernel   per head: mean BCE-with-logits, g = dL/dlogit, and the counts of (sigmoid(logit) > thresh) == label per threshold and per
//                     (task, threshold), ADDED to what the int32 buffers hold (one workgroup owns a head's counters: no global atomics).
//
// Arithmetic of U | V: split-bf16 -- every f32 operand is bf16 hi + bf16 lo, three products a_hi.b_lo + a_lo.b_hi + a_hi.b_hi with f32 accumulation --
// WHATEVER sf_set_precision says, as dvae_tokens.hip: a logit has one definition.  The weight gradients are plain f32 fma chains.
// Ties: the FIRST timestep / pair of the maximum.  A NaN in a frame that is read gives unspecified routing.  Frames beyond T and videos that
// video_index does not name are never read.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"

namespace {

constexpr int PR_ROWS = 48;        // slot rows of a chunk: three 16-row MFMA tiles
constexpr int PR_THREADS = 512;    // eight waves: two per SIMD, the only latency hiding a 108 KB workgroup gets
constexpr int PR_WAVES = 8;
constexpr int PR_KS = 8;          // k-steps of 32 at the widest slot (C = 256)
constexpr int PR_MAX_THRESH = 16;  // thresholds of one score launch
constexpr int PR_MAX_TASKS = 64;   // tasks of one score launch
enum { PR_MAX = 0, PR_SUM = 1, PR_MEAN = 2 };

inline bool pr_ok(int N, int C, int F) { return N >= 2 && N <= 16 && C >= 32 && C <= 256 && C % 32 == 0 && F >= 32 && F <= 256 && F % 32 == 0; }
inline int pr_pitch_s(int C) { return (C + 8) * 2; }    // bytes of a row of a bf16 plane
inline int pr_pitch_uv(int F) { return 2 * F + 4; }     // floats of a row of U | V
inline size_t pr_lds_bytes(int C, int F) { return (size_t)PR_ROWS * pr_pitch_s(C) * 2 + (size_t)PR_ROWS * pr_pitch_uv(F) * 4 + 64; }

struct PrLds {
  char *hi, *lo;
  float* uv;
  float* sv;   // [PR_WAVES] the waves' maxima
  int* si;     // [PR_WAVES] and their timesteps
  int ps, puv;
};
__device__ __forceinline__ PrLds pr_lds(char* smem, int C, int F) {
  PrLds l;
  l.ps = (C + 8) * 2;
  l.puv = 2 * F + 4;
  l.hi = smem;
  l.lo = smem + PR_ROWS * l.ps;
  l.uv = reinterpret_cast<float*>(smem + 2 * PR_ROWS * l.ps);
  l.sv = l.uv + PR_ROWS * l.puv;
  l.si = reinterpret_cast<int*>(l.sv + PR_WAVES);
  return l;
}

// rows [0, 16 rt_n) of the planes: row r = slot r % N of frame r / N behind `src` (frame stride in elements; [N][C] contiguous inside a frame);
// a row past nrows is a zero operand, never an address
__device__ __forceinline__ void pr_stage(const float* src, long long stride_t, int nrows, int rt_n, int N, int C, const PrLds& l, int tid) {
  const int c4n = C >> 2;
#pragma unroll 4
  for (int idx = tid; idx < rt_n * 16 * c4n; idx += PR_THREADS) {
    const int r = idx / c4n, c4 = idx - r * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < nrows) {
      const int tl = r / N, i = r - tl * N;
      v = *reinterpret_cast<const f32x4*>(src + (long long)tl * stride_t + i * C + c4 * 4);
    }
    sf_split4(reinterpret_cast<__bf16*>(l.hi + r * l.ps), reinterpret_cast<__bf16*>(l.lo + r * l.ps), c4 * 4, v);
  }
}

// U | V of the staged rows -> l.uv.  Column tile ct of 16: features 16 ct .. of U (ct < F / 16; the accumulators start at b1) or of V.
// A operand: the rows (lane & 15 = row of the tile, k = 8 (lane >> 4) + 0..7); B operand: W1[feature lane & 15][the same k]; accumulator register q of a
// lane = row 4 (lane >> 4) + q, column lane & 15.
// The workgroup's LDS leaves one workgroup on a CU -- two waves on a SIMD -- so little hides a load but the wave itself: a lane requests ALL its W1 operands of the NEXT column
// tile (C / 32 k-steps x 32 bytes) before the products of the current one.
struct PrW {
  f32x4 a[PR_KS], b[PR_KS];
  float bias;
};
__device__ __forceinline__ void pr_wload(PrW& w, const float* __restrict__ W1, const float* __restrict__ b1, int ct, int C, int F, int lane) {
  const int col = ct * 16;
  const bool is_v = col >= F;   // wave-uniform
  const int f = (is_v ? col - F : col) + (lane & 15);
  const float* wrow = W1 + (long long)f * 2 * C + (is_v ? C : 0) + 8 * (lane >> 4);
#pragma unroll
  for (int ks = 0; ks < PR_KS; ++ks)
    if (ks < (C >> 5)) w.a[ks] = *reinterpret_cast<const f32x4*>(wrow + ks * 32), w.b[ks] = *reinterpret_cast<const f32x4*>(wrow + ks * 32 + 4);
  w.bias = is_v ? 0.f : b1[f];
}
__device__ __forceinline__ void pr_gemm(const float* __restrict__ W1, const float* __restrict__ b1, int C, int F, int rt_n, const PrLds& l, int wid,
                                        int lane) {
  const int nct = F >> 3, l15 = lane & 15, q = lane >> 4;
  if (wid >= nct) return;   // (F = 32: four column tiles for eight waves; the barriers are the caller's)
  PrW cur, nxt;
  pr_wload(cur, W1, b1, wid, C, F, lane);
  for (int ct = wid; ct < nct; ct += PR_WAVES) {
    pr_wload(nxt, W1, b1, ct + PR_WAVES < nct ? ct + PR_WAVES : ct, C, F, lane);   // (past the end: the same tile again, never past the matrix)
    __builtin_amdgcn_sched_barrier(0);   // (the requests stay AHEAD of the products)
    const int col = ct * 16;
    f32x4 acc[3];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt) acc[rt] = f32x4{cur.bias, cur.bias, cur.bias, cur.bias};
#pragma unroll
    for (int ks = 0; ks < PR_KS; ++ks)
      if (ks < (C >> 5)) {
        bf16x8 wh, wl;
        sf_split8(cur.a[ks], cur.b[ks], wh, wl);
#pragma unroll
        for (int rt = 0; rt < 3; ++rt)
          if (rt < rt_n) {
            const int o = (rt * 16 + l15) * l.ps + (ks * 32 + 8 * q) * 2;
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(l.hi + o), al = *reinterpret_cast<const bf16x8*>(l.lo + o);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wl, acc[rt], 0, 0, 0);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wh, acc[rt], 0, 0, 0);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wh, acc[rt], 0, 0, 0);
          }
      }
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
      if (rt < rt_n)
#pragma unroll
        for (int e = 0; e < 4; ++e) l.uv[(rt * 16 + q * 4 + e) * l.puv + col + l15] = acc[rt][e];
    cur = nxt;
  }
}

// the relation of feature f over the pairs of the frame whose slot rows start at row0 of l.uv; pair = the first pair of the maximum (max only).
// NT: the slot count at compile time (the frame's 2 NT values are read once, into registers, and the pair loop is unrolled), 0: N at run time.
template <int NT>
__device__ __forceinline__ float pr_agg_n(const PrLds& l, int row0, int f, int F, int N, int agg, float inv_p, int& pair) {
  const float* u = l.uv + row0 * l.puv + f;
  const float* v = u + F;
  pair = 0;
  if constexpr (NT > 0) {
    float uu[NT], vv[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) uu[i] = u[i * l.puv], vv[i] = v[i * l.puv];
    if (agg == PR_MAX) {
      float best = -INFINITY;
      int p = 0;
#pragma unroll
      for (int i = 0; i < NT - 1; ++i)
#pragma unroll
        for (int j = i + 1; j < NT; ++j, ++p) {
          const float s = uu[i] + vv[j];
          if (s > best) best = s, pair = p;
        }
      return best;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NT - 1; ++i)
#pragma unroll
      for (int j = i + 1; j < NT; ++j) s += uu[i] + vv[j];
    return agg == PR_MEAN ? s * inv_p : s;
  } else {
    if (agg == PR_MAX) {
      float best = -INFINITY;
      int p = 0;
      for (int i = 0; i < N - 1; ++i) {
        const float ui = u[i * l.puv];
        for (int j = i + 1; j < N; ++j, ++p) {
          const float s = ui + v[j * l.puv];
          if (s > best) best = s, pair = p;
        }
      }
      return best;
    }
    float s = 0.f;
    for (int i = 0; i < N - 1; ++i) {
      const float ui = u[i * l.puv];
      for (int j = i + 1; j < N; ++j) s += ui + v[j * l.puv];
    }
    return agg == PR_MEAN ? s * inv_p : s;
  }
}
// (the same adds in the same order either way: the reference shape's N = 6 takes the unrolled form)
__device__ __forceinline__ float pr_agg(const PrLds& l, int row0, int f, int F, int N, int agg, float inv_p, int& pair) {
  return N == 6 ? pr_agg_n<6>(l, row0, f, F, N, agg, inv_p, pair) : pr_agg_n<0>(l, row0, f, F, N, agg, inv_p, pair);
}

struct PrFwd {
  const float* slots;
  long long stride_v, stride_t;
  int V;
  const int* video_index;
  const float *W1, *b1, *w2, *b2;
  float* logits;
  int* t_star;
  float* step_logits;
  unsigned char* pair_star;
  int B, T, N, C, F, agg;
};

__global__ __launch_bounds__(PR_THREADS) void pr_fwd_kernel(const PrFwd a) {
  extern __shared__ __attribute__((aligned(16))) char pr_smem[];
  const PrLds l = pr_lds(pr_smem, a.C, a.F);
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x, k = blockIdx.y;
  const int N = a.N, C = a.C, F = a.F, T = a.T;
  const long long kb = (long long)k * a.B + b;
  const int vid = a.video_index ? a.video_index[b] : b;
  if (vid < 0 || vid >= a.V) {   // (workgroup-uniform) a video that does not exist is never an address: NaN out
    if (tid == 0) a.logits[kb] = NAN, a.t_star[kb] = 0;
    if (a.step_logits)
      for (int t = tid; t < T; t += PR_THREADS) a.step_logits[kb * T + t] = NAN;
    if (a.pair_star)
      for (int f = tid; f < F; f += PR_THREADS) a.pair_star[kb * F + f] = 0;
    return;
  }
  const float* base = a.slots + (long long)vid * a.stride_v;
  const float* W1 = a.W1 + (long long)k * F * 2 * C;
  const float* b1 = a.b1 + (long long)k * F;
  const float* w2 = a.w2 + (long long)k * F;
  const float b2 = a.b2[k];
  const float inv_p = 1.f / (float)(N * (N - 1) / 2);
  const int tsc = PR_ROWS / N;
  float best = -INFINITY;
  int bt = 0x7fffffff;
  for (int t0 = 0; t0 < T; t0 += tsc) {
    const int ts = T - t0 < tsc ? T - t0 : tsc, nrows = ts * N, rt_n = (nrows + 15) >> 4;
    pr_stage(base + (long long)t0 * a.stride_t, a.stride_t, nrows, rt_n, N, C, l, tid);
    __syncthreads();
    pr_gemm(W1, b1, C, F, rt_n, l, wid, lane);
    __syncthreads();   // (the next chunk's planes are written behind this barrier, its U | V behind the next one)
    for (int tl = wid; tl < ts; tl += PR_WAVES) {
      float part = 0.f;
      for (int f0 = 0; f0 < F; f0 += 64) {
        const int f = f0 + lane;
        int pair;
        if (f < F) part = fmaf(pr_agg(l, tl * N, f, F, N, a.agg, inv_p, pair), w2[f], part);
      }
      const float s = sf_wave_sum(part) + b2;
      if (a.step_logits && lane == 0) a.step_logits[kb * T + t0 + tl] = s;
      if (s > best) best = s, bt = t0 + tl;   // a wave meets its timesteps in rising order: strict > keeps the first
    }
  }
  if (lane == 0) l.sv[wid] = best, l.si[wid] = bt;
  __syncthreads();
  best = l.sv[0], bt = l.si[0];
#pragma unroll
  for (int w = 1; w < PR_WAVES; ++w)
    if (l.sv[w] > best || (l.sv[w] == best && l.si[w] < bt)) best = l.sv[w], bt = l.si[w];
  const bool found = bt < T;   // false: every step logit was a NaN
  if (tid == 0) a.logits[kb] = found ? best : NAN, a.t_star[kb] = found ? bt : 0;
  if (!a.pair_star) return;
  if (a.agg != PR_MAX || !found) {
    for (int f = tid; f < F; f += PR_THREADS) a.pair_star[kb * F + f] = 0;
    return;
  }
  pr_stage(base + (long long)bt * a.stride_t, a.stride_t, N, 1, N, C, l, tid);
  __syncthreads();
  pr_gemm(W1, b1, C, F, 1, l, wid, lane);
  __syncthreads();
  for (int f = tid; f < F; f += PR_THREADS) {
    int pair;
    pr_agg(l, 0, f, F, N, PR_MAX, inv_p, pair);
    a.pair_star[kb * F + f] = (unsigned char)pair;
  }
}

struct PrBwd {
  const float* slots;
  long long stride_v, stride_t;
  int V;
  const int* video_index;
  const float *W1, *b1, *w2, *g;
  const int* t_star;
  const unsigned char* pair_star;
  float *R, *cu, *cv;   // workspace: [B][F], [B][N][F], [B][N][F]
  float *dW1, *db1, *dw2, *db2;
  int B, T, N, C, F, agg;
};

__global__ __launch_bounds__(PR_THREADS) void pr_route_kernel(const PrBwd a) {
  extern __shared__ __attribute__((aligned(16))) char pr_smem[];
  const PrLds l = pr_lds(pr_smem, a.C, a.F);
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x, N = a.N, C = a.C, F = a.F;
  const int vid = a.video_index ? a.video_index[b] : b, t = a.t_star[b];
  const bool valid = vid >= 0 && vid < a.V && t >= 0 && t < a.T;   // workgroup-uniform
  if (valid) {
    pr_stage(a.slots + (long long)vid * a.stride_v + (long long)t * a.stride_t, a.stride_t, N, 1, N, C, l, tid);
    __syncthreads();
    pr_gemm(a.W1, a.b1, C, F, 1, l, wid, lane);
    __syncthreads();
  }
  const int P = N * (N - 1) / 2;
  const float inv_p = 1.f / (float)P, gb = a.g[b];
  for (int f = tid; f < F; f += PR_THREADS) {
    float* cu = a.cu + (long long)b * N * F + f;
    float* cv = a.cv + (long long)b * N * F + f;
    int pair = 0;
    float R = valid ? pr_agg(l, 0, f, F, N, a.agg, inv_p, pair) : NAN;
    const float dR = valid ? gb * a.w2[f] : NAN;   // (a route that names no frame: NaN gradients, never an address)
    if (a.agg == PR_MAX) {
      if (a.pair_star) pair = a.pair_star[(long long)b * F + f];
      int i = 0, p = pair;
      while (i < N - 1 && p >= N - 1 - i) p -= N - 1 - i, ++i;
      const bool pok = i < N - 1;   // false: a recorded pair >= pairs
      const int j = i + 1 + p;
      if (valid && pok) R = l.uv[i * l.puv + f] + l.uv[j * l.puv + F + f];
      for (int n = 0; n < N; ++n) {
        cu[(long long)n * F] = pok ? (n == i ? dR : 0.f) : NAN;
        cv[(long long)n * F] = pok ? (n == j ? dR : 0.f) : NAN;
      }
    } else {
      const float sc = a.agg == PR_MEAN ? dR * inv_p : dR;
      for (int n = 0; n < N; ++n) {
        cu[(long long)n * F] = (float)(N - 1 - n) * sc;
        cv[(long long)n * F] = (float)n * sc;
      }
    }
    a.R[(long long)b * F + f] = R;
  }
}

// workgroup f < F: row f of dW1 (thread = column c2 of [Wa | Wb]); workgroup F: db1, dw2 (thread = feature) and db2
__global__ __launch_bounds__(PR_THREADS) void pr_wgrad_kernel(const PrBwd a) {
  const int tid = threadIdx.x, N = a.N, C = a.C, F = a.F, B = a.B;
  if ((int)blockIdx.x == F) {
    for (int f = tid; f < F; f += PR_THREADS) {
      float s1 = 0.f, s2 = 0.f;
      for (int b = 0; b < B; ++b) {
        float su = 0.f;
        for (int n = 0; n < N; ++n) su += a.cu[((long long)b * N + n) * F + f];
        s1 += su;
        s2 = fmaf(a.g[b], a.R[(long long)b * F + f], s2);
      }
      a.db1[f] = s1;
      a.dw2[f] = s2;
    }
    if (tid == 0) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s += a.g[b];
      a.db2[0] = s;
    }
    return;
  }
  const int f = blockIdx.x;
  for (int c2 = tid; c2 < 2 * C; c2 += PR_THREADS) {
    const bool is_v = c2 >= C;
    const int c = is_v ? c2 - C : c2;
    const float* coef = (is_v ? a.cv : a.cu) + f;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
      const int vid = a.video_index ? a.video_index[b] : b, t = a.t_star[b];
      if (vid < 0 || vid >= a.V || t < 0 || t >= a.T) {
        acc = NAN;
        continue;
      }
      const float* s = a.slots + (long long)vid * a.stride_v + (long long)t * a.stride_t + c;
      for (int n = 0; n < N; ++n) {
        const float w = coef[((long long)b * N + n) * F];   // workgroup-uniform
        if (w != 0.f) acc = fmaf(w, s[n * C], acc);
      }
    }
    a.dW1[(long long)f * 2 * C + c2] = acc;
  }
}

struct PrThresh {
  float v[PR_MAX_THRESH];
};

__global__ __launch_bounds__(PR_THREADS) void pr_score_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                              const int* __restrict__ task_idx, const PrThresh th, int n_thresh, int n_tasks,
                                                              float* __restrict__ loss, float* __restrict__ g, int* __restrict__ counts,
                                                              int* __restrict__ task_counts, int B) {
  __shared__ double red[PR_THREADS];
  __shared__ int cnt[PR_MAX_THRESH];
  __shared__ int tcnt[PR_MAX_TASKS * PR_MAX_THRESH];
  const int tid = threadIdx.x, k = blockIdx.x;
  for (int i = tid; i < PR_MAX_THRESH; i += PR_THREADS) cnt[i] = 0;
  for (int i = tid; i < PR_MAX_TASKS * PR_MAX_THRESH; i += PR_THREADS) tcnt[i] = 0;
  __syncthreads();
  double part = 0.0;
  const float inv_b = 1.f / (float)B;
  for (int b = tid; b < B; b += PR_THREADS) {
    const float x = logits[(long long)k * B + b], y = labels[b];
    part += (double)(fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))));
    const float p = 1.0f / (1.0f + expf(-x));
    if (g) g[(long long)k * B + b] = (p - y) * inv_b;
    int task = task_idx ? task_idx[b] : -1;
    if (task >= n_tasks) task = -1;   // (a task that does not exist is counted in the totals only)
    for (int i = 0; i < n_thresh; ++i)
      if ((p > th.v[i] ? 1.f : 0.f) == y) {
        atomicAdd(&cnt[i], 1);   // (LDS, integers: the order does not matter)
        if (task >= 0) atomicAdd(&tcnt[task * n_thresh + i], 1);
      }
  }
  red[tid] = part;
  __syncthreads();
  if (tid == 0 && loss) {
    double s = 0.0;
    for (int i = 0; i < PR_THREADS; ++i) s += red[i];
    loss[k] = (float)(s / (double)B);
  }
  if (counts)
    for (int i = tid; i < n_thresh; i += PR_THREADS) counts[(long long)k * n_thresh + i] += cnt[i];
  if (task_counts)
    for (int i = tid; i < n_tasks * n_thresh; i += PR_THREADS) task_counts[(long long)k * n_tasks * n_thresh + i] += tcnt[i];
}

inline bool pr_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define PR_LIMITS "2 <= N <= 16, C and F multiples of 32 in [32, 256]"

extern "C" {

int sf_physion_readout_ok(int N, int C, int F) { return pr_ok(N, C, F) ? 1 : 0; }

size_t sf_physion_readout_bwd_workspace_bytes(int B, int N, int F) {
  if (B < 1 || N < 2 || N > 16 || F < 32 || F > 256 || F % 32) return 0;
  return (size_t)B * F * (1 + 2 * (size_t)N) * sizeof(float);
}

int sf_physion_readout_fwd_f32(const float* slots, long long stride_v, long long stride_t, int V, const int* video_index, const float* W1,
                               const float* b1, const float* w2, const float* b2, float* logits, int* t_star, float* step_logits,
                               unsigned char* pair_star, int K, int B, int T, int N, int C, int F, int agg, void* stream) {
  SF_REQUIRE(slots && W1 && b1 && w2 && b2 && logits && t_star, "sf_physion_readout_fwd_f32: null pointer");
  SF_REQUIRE(pr_ok(N, C, F), "sf_physion_readout_fwd_f32: unsupported shape (" PR_LIMITS ")");
  SF_REQUIRE(T >= 1, "sf_physion_readout_fwd_f32: T >= 1");
  SF_REQUIRE(B >= 1 && K >= 1 && K <= 65535 && V >= 1, "sf_physion_readout_fwd_f32: B >= 1, 1 <= K <= 65535, V >= 1");
  SF_REQUIRE(agg == PR_MAX || agg == PR_SUM || agg == PR_MEAN, "sf_physion_readout_fwd_f32: unknown aggregate (0 max, 1 sum, 2 mean)");
  SF_REQUIRE(stride_t >= (long long)N * C && stride_t % 4 == 0 && stride_v >= 0 && stride_v % 4 == 0,
             "sf_physion_readout_fwd_f32: frame stride >= N * C, strides multiples of 4");
  SF_REQUIRE(video_index || B <= V, "sf_physion_readout_fwd_f32: B > V without a video_index");
  SF_REQUIRE(pr_al16(slots) && pr_al16(W1), "sf_physion_readout_fwd_f32: slots and W1 must be 16-byte aligned");
  const size_t lds = pr_lds_bytes(C, F);
  SF_TRY(sf_ensure_dyn_lds((const void*)pr_fwd_kernel, lds));
  const PrFwd a{slots, stride_v, stride_t, V, video_index, W1, b1, w2, b2, logits, t_star, step_logits, pair_star, B, T, N, C, F, agg};
  hipLaunchKernelGGL(pr_fwd_kernel, dim3((unsigned)B, (unsigned)K), dim3(PR_THREADS), lds, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_physion_readout_bwd_f32(const float* slots, long long stride_v, long long stride_t, int V, const int* video_index, const float* W1,
                               const float* b1, const float* w2, const float* g, const int* t_star, const unsigned char* pair_star, float* dW1,
                               float* db1, float* dw2, float* db2, int B, int T, int N, int C, int F, int agg, void* workspace,
                               size_t workspace_bytes, void* stream) {
  SF_REQUIRE(slots && W1 && b1 && w2 && g && t_star && dW1 && db1 && dw2 && db2 && workspace, "sf_physion_readout_bwd_f32: null pointer");
  SF_REQUIRE(pr_ok(N, C, F), "sf_physion_readout_bwd_f32: unsupported shape (" PR_LIMITS ")");
  SF_REQUIRE(T >= 1, "sf_physion_readout_bwd_f32: T >= 1");
  SF_REQUIRE(B >= 1 && V >= 1, "sf_physion_readout_bwd_f32: B >= 1, V >= 1");
  SF_REQUIRE(agg == PR_MAX || agg == PR_SUM || agg == PR_MEAN, "sf_physion_readout_bwd_f32: unknown aggregate (0 max, 1 sum, 2 mean)");
  SF_REQUIRE(stride_t >= (long long)N * C && stride_t % 4 == 0 && stride_v >= 0 && stride_v % 4 == 0,
             "sf_physion_readout_bwd_f32: frame stride >= N * C, strides multiples of 4");
  SF_REQUIRE(video_index || B <= V, "sf_physion_readout_bwd_f32: B > V without a video_index");
  SF_REQUIRE(pr_al16(slots) && pr_al16(W1) && pr_al16(workspace), "sf_physion_readout_bwd_f32: slots, W1 and the workspace must be 16-byte aligned");
  SF_REQUIRE(workspace_bytes >= sf_physion_readout_bwd_workspace_bytes(B, N, F), "sf_physion_readout_bwd_f32: workspace too small");
  const size_t lds = pr_lds_bytes(C, F);
  SF_TRY(sf_ensure_dyn_lds((const void*)pr_route_kernel, lds));
  float* R = static_cast<float*>(workspace);
  float* cu = R + (size_t)B * F;
  float* cv = cu + (size_t)B * N * F;
  const PrBwd a{slots, stride_v, stride_t, V, video_index, W1, b1, w2, g, t_star, pair_star, R, cu, cv, dW1, db1, dw2, db2, B, T, N, C, F, agg};
  hipLaunchKernelGGL(pr_route_kernel, dim3((unsigned)B), dim3(PR_THREADS), lds, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(pr_wgrad_kernel, dim3((unsigned)F + 1), dim3(PR_THREADS), 0, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_physion_readout_score_f32(const float* logits, const float* labels, const int* task_idx, const float* thresholds, int n_thresh, int n_tasks,
                                 float* loss, float* g, int* counts, int* task_counts, int K, int B, void* stream) {
  SF_REQUIRE(logits && labels, "sf_physion_readout_score_f32: null pointer");
  SF_REQUIRE(K >= 1 && B >= 1, "sf_physion_readout_score_f32: K >= 1, B >= 1");
  SF_REQUIRE(n_thresh >= 0 && n_thresh <= PR_MAX_THRESH, "sf_physion_readout_score_f32: at most 16 thresholds per launch");
  SF_REQUIRE(n_thresh == 0 || thresholds, "sf_physion_readout_score_f32: null pointer (thresholds)");
  SF_REQUIRE(n_tasks >= 0 && n_tasks <= PR_MAX_TASKS, "sf_physion_readout_score_f32: at most 64 tasks per launch");
  SF_REQUIRE(!task_counts || (task_idx && n_tasks >= 1), "sf_physion_readout_score_f32: per-task counts need task_idx and n_tasks >= 1");
  PrThresh th;
  for (int i = 0; i < PR_MAX_THRESH; ++i) th.v[i] = i < n_thresh ? thresholds[i] : 0.f;
  hipLaunchKernelGGL(pr_score_kernel, dim3((unsigned)K), dim3(PR_THREADS), 0, (hipStream_t)stream, logits, labels, task_idx, th, n_thresh,
                     task_counts ? n_tasks : 0, loss, g, counts, task_counts, B);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// The vocabulary head and its cross-entropy in one pass, forward and backward, without the logits [R,V] in memory: the token loss of the Physion
// rollouter (steve_slotformer.py:150-161), which the reference switches off because those logits do not fit.
//
//   hc_fwd_kernel   lse[r] = log sum_v exp(W[v] . x[r]), loss[r] = lse[r] - W[t_r] . x[r] for x [R,K].  D[word][row] on the MFMA's (row, column) axes, as
//                   in dvae_head_argmax_kernel: the sixteen accumulators of a lane belong to ONE row of x, so the running (max, sum) pair and the
//                   target's logit stay in the lane while the vocabulary is swept in blocks of 32 words.  A workgroup owns 64 rows, staged once as
//                   bf16 hi | lo planes in LDS; its four waves sweep every fourth block of the head weight, read in fragment order from the packed
//                   copy (16-byte loads).  The half-waves meet in one exchange, the waves in 3 KB of LDS behind one barrier.  The target's logit is
//                   picked by COMPARING the swept word index with t_r: a target outside [0, V) matches nothing and forms no address.
//   hc_stats_kernel one workgroup adds the tiles' (sum w loss, sum w) partials, in index order, to stats.
//   hc_bwd_kernel   dx[r,:] = c_r (sum_v p[r,v] W[v,:] - W[t_r,:]), p = exp(W[v] . x[r] - lse[r]).  A workgroup owns 32 rows and its four waves split
//                   the vocabulary as in the forward: per block of 32 words a wave recomputes the logits D1[word][row], turns them into p - onehot in
//                   registers, and -- the accumulator of a 32x32 block has its column on the lane and its rows in the registers -- feeds them to the
//                   second product D2[row][feature] += P^T W as its A operand with no lane movement: k-step c of that product contracts the words of
//                   registers 8 c .. 8 c + 7, word(c, kk, j) = 16 c + 8 (j >> 2) + 4 kk + (j & 3), and the SECOND packed copy of W holds its fragments
//                   in exactly that order.  A wave's part of dx (K / 32 accumulator blocks) stays in its registers through the sweep; the four parts
//                   meet once, in a fixed order, through the LDS the rows were staged in, and wave 0 writes 128 contiguous bytes of two rows per store.
//   hc_wgrad_kernel dW[v,:] = sum_r c_r (p[r,v] - [v == t_r]) x[r,:], the gradient of a head that is trained (STEVE): hc_bwd_kernel with the two operands
//                   in each other's place.  A wave owns 32 WORDS: their fragments of packed copy A stay in its registers as the B operand of the
//                   first product and its 32 x K block of dW in K / 32 accumulator blocks, while it sweeps the rows in tiles of 32, staged once per
//                   workgroup (four waves: a slab of 128 words) as bf16 planes in two LDS buffers -- the loads of the next tile are issued before the
//                   products of the current one.  D1[row][word] leaves the lane with ONE word and sixteen rows, whose lse, target and c_r come from
//                   384 bytes of LDS staged with the tile; registers 8 c .. 8 c + 7 of c_r (exp(D1 - lse_r) - [word == t_r]) are the A operand of
//                   k-step c of D3[word][feature] += P x, and x read DOWN the staged rows in the accumulator's row order (pl_rd_tr, kstep 4, second 8)
//                   is its B operand: no second staging, no second packed copy.  The grid is slabs x S row splits; S is a function of (R, V) alone
//                   (hc_wg_splits), capped at 8, so that equal shapes split equally on every device.  Each split writes its [V][K] block to the workspace.
//   hc_wgrad_sum_kernel adds the S blocks in index order into dW.
//
// Arithmetic: split-bf16 -- every f32 operand is bf16 hi + bf16 lo, three products a_hi.b_lo + a_lo.b_hi + a_hi.b_hi with f32 accumulation -- WHATEVER
// sf_set_precision says, as in dvae_tokens.hip: the token loss has one definition.  Every sum has a fixed order, there is no atomic and no
// communication between workgroups: a row's results do not depend on its place in the batch.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "bf16_planes.h"
#include <math.h>

namespace {

constexpr int HC_VB = 32;        // vocabulary words of an MFMA block
constexpr int HC_ROWS = 64;      // rows of a forward workgroup's tile: two MFMA column blocks
constexpr int HC_BWD_ROWS = 32;  // rows of a backward workgroup's tile: one
constexpr int HC_WAVES = 4;      // waves of a workgroup, forward and backward: they share the tile's rows and split the vocabulary
constexpr int HC_MAX_V = 1 << 20;
constexpr int HC_MAX_K = 256;
constexpr long long HC_MAX_R = 1ll << 29;   // (a launch holds fewer than 2^32 threads: 2^24 workgroups of 256)

// f32 -> bf16, round to nearest even, the same on host and device (a NaN stays a NaN)
__host__ __device__ inline unsigned short hc_bf16(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float hc_f32(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }

// Element index of a packed plane -> element index of the [V][K] source.
// Copy A (the logits' A operand): for every block vb of 32 words and every k-step ks of 16 features, lane (r = l & 31, h = l >> 5) holds
// W[32 vb + r][16 ks + 8 h + 0..7].
__host__ __device__ inline long long hc_src_a(long long idx, int K) {
  const int j = (int)(idx & 7), l = (int)((idx >> 3) & 63), KS = K >> 4;
  const long long step = idx >> 9, vb = step / KS;
  const int ks = (int)(step - vb * KS);
  return (vb * HC_VB + (l & 31)) * K + 16 * ks + 8 * (l >> 5) + j;
}
// Copy B (the data gradient's B operand): for every block vb, every half c of its words and every block kfb of 32 features, lane (i = l & 31,
// kk = l >> 5) holds W[32 vb + 16 c + 8 (j >> 2) + 4 kk + (j & 3)][32 kfb + i] in element j = 0..7.
__host__ __device__ inline long long hc_src_b(long long idx, int K) {
  const int j = (int)(idx & 7), l = (int)((idx >> 3) & 63), KB = K >> 5;
  const long long step = idx >> 9, rest = step / KB;
  const int kfb = (int)(step - rest * KB), c = (int)(rest & 1);
  const long long vb = rest >> 1;
  return (vb * HC_VB + 16 * c + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)) * K + 32 * kfb + (l & 31);
}
// planes of the packed buffer, n = V K elements each: A hi | A lo | B hi | B lo
__host__ __device__ inline void hc_pack_one(const float* w, unsigned short* packed, long long idx, long long n, int K) {
  const bool b = idx >= n;
  const long long e = b ? idx - n : idx;
  const float v = w[b ? hc_src_b(e, K) : hc_src_a(e, K)];
  const unsigned short h = hc_bf16(v);
  unsigned short* base = packed + (b ? 2 * n : 0);
  base[e] = h;
  base[n + e] = hc_bf16(v - hc_f32(h));
}

__global__ void hc_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ packed, long long n, int K) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < 2 * n) hc_pack_one(w, packed, idx, n, K);
}

// rows row0 .. row0 + rows - 1 of x as bf16 hi | lo planes in LDS (row pitch 2 K + 16 bytes: the fragment reads of 32 rows fall on distinct banks);
// a row past the end is a zero operand, never an address
__device__ __forceinline__ void hc_stage(char* lds, int loff, int pitch, const float* __restrict__ x, long long ld, long long row0, int rows, long long R,
                                         int K, int tid, int nthreads) {
  const int k8 = K >> 3;
  for (int u = tid; u < rows * k8; u += nthreads) {
    const int row = u / k8, c = u - row * k8;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (row0 + row < R) {
      const float* xp = x + (row0 + row) * ld + 8 * c;
      a = *reinterpret_cast<const f32x4*>(xp);
      b = *reinterpret_cast<const f32x4*>(xp + 4);
    }
    bf16x8 hi, lo;
    sf_split8(a, b, hi, lo);
    *reinterpret_cast<bf16x8*>(lds + row * pitch + c * 16) = hi;
    *reinterpret_cast<bf16x8*>(lds + loff + row * pitch + c * 16) = lo;
  }
}

// the target of row p as an int, -1 (matches no word) when it lies outside [0, V)
__device__ __forceinline__ int hc_target(const long long* t64, const short* t16, long long p, int V) {
  const long long t = t64 ? t64[p] : (long long)t16[p];
  return t >= 0 && t < V ? (int)t : -1;
}
// exp(a - m) for a running maximum a <= m; a pair that has seen no word (a = -inf) brings nothing, whatever m is
__device__ __forceinline__ float hc_scale(float a, float m) { return a == -INFINITY ? 0.f : __expf(a - m); }

__global__ __launch_bounds__(64 * HC_WAVES) void hc_fwd_kernel(const float* __restrict__ x, long long ld, const uint4* __restrict__ wa_hi,
                                                                   const uint4* __restrict__ wa_lo, const long long* __restrict__ t64,
                                                                   const short* __restrict__ t16, const float* __restrict__ group_w, int group,
                                                                   float* __restrict__ lse, float* __restrict__ loss_rows,
                                                                   double* __restrict__ partial, long long R, int V, int K) {
  extern __shared__ __attribute__((aligned(16))) char hc_lds[];
  __shared__ float sm[HC_WAVES][HC_ROWS], ss[HC_WAVES][HC_ROWS], st[HC_WAVES][HC_ROWS];
  const int pitch = 2 * K + 16, loff = HC_ROWS * pitch;
  const long long pt = (long long)blockIdx.x * HC_ROWS;   // < R: the grid is ceil(R / 64)
  hc_stage(hc_lds, loff, pitch, x, ld, pt, HC_ROWS, R, K, threadIdx.x, 64 * HC_WAVES);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  int tgt[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long long p = pt + 32 * s + r;
    tgt[s] = p < R ? hc_target(t64, t16, p, V) : -1;
  }
  float m[2] = {-INFINITY, -INFINITY}, sum[2] = {0.f, 0.f}, tl[2] = {0.f, 0.f};
  const int nvb = V / HC_VB, KS = K >> 4;
  for (int vb = q; vb < nvb; vb += HC_WAVES) {   // wave-uniform
    f32x16 acc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[s][i] = 0.f;
    const long long f0 = (long long)vb * KS * 64 + lane;
    for (int ks = 0; ks < KS; ++ks) {
      PlFrag w;
      w.h = __builtin_bit_cast(bf16x8, wa_hi[f0 + ks * 64]);
      w.l = __builtin_bit_cast(bf16x8, wa_lo[f0 + ks * 64]);
#pragma unroll
      for (int s = 0; s < 2; ++s) pl_mma(acc[s], w, pl_rd(hc_lds, 0, loff, pitch, 32 * s, 16 * ks, lane));
    }
    // register i of the lane: word 32 vb + MM_ROW(i, lane) of row 32 s + r
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float bm = acc[s][0];
#pragma unroll
      for (int i = 1; i < 16; ++i) bm = fmaxf(bm, acc[s][i]);
      const float mn = fmaxf(m[s], bm);
      float add = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) add += __expf(acc[s][i] - mn);
      sum[s] = sum[s] * hc_scale(m[s], mn) + add;
      m[s] = mn;
#pragma unroll
      for (int i = 0; i < 16; ++i) tl[s] += (vb * HC_VB + MM_ROW(i, lane) == tgt[s]) ? acc[s][i] : 0.f;
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float om = __shfl_xor(m[s], 32, 64), os = __shfl_xor(sum[s], 32, 64), ot = __shfl_xor(tl[s], 32, 64);   // the other half-wave, same row
    if (h == 0) {
      const float mn = fmaxf(m[s], om);
      sm[q][32 * s + r] = mn;
      ss[q][32 * s + r] = sum[s] * hc_scale(m[s], mn) + os * hc_scale(om, mn);
      st[q][32 * s + r] = tl[s] + ot;
    }
  }
  __syncthreads();   // every thread of the workgroup reaches it
  if (q != 0) return;
  float mn = sm[0][lane];
#pragma unroll
  for (int w = 1; w < HC_WAVES; ++w) mn = fmaxf(mn, sm[w][lane]);
  float sv = 0.f, tv = 0.f;
#pragma unroll
  for (int w = 0; w < HC_WAVES; ++w) sv += ss[w][lane] * hc_scale(sm[w][lane], mn), tv += st[w][lane];
  const float l = mn + logf(sv);
  const long long p = pt + lane;
  double a = 0., b = 0.;
  if (p < R) {
    const float wgt = group_w ? group_w[p / group] : 1.f;
    lse[p] = l;
    if (loss_rows) loss_rows[p] = l - tv;
    if (wgt != 0.f) a = (double)wgt * (double)(l - tv), b = (double)wgt;
  }
  a = sf_wave_sum(a);
  b = sf_wave_sum(b);
  if (partial && lane == 0) partial[2 * (long long)blockIdx.x] = a, partial[2 * (long long)blockIdx.x + 1] = b;
}

__global__ __launch_bounds__(256) void hc_stats_kernel(const double* __restrict__ partial, long long n, double* __restrict__ stats) {
  __shared__ double sa[256], sb[256];
  double a = 0., b = 0.;
  for (long long i = threadIdx.x; i < n; i += 256) a += partial[2 * i], b += partial[2 * i + 1];
  sa[threadIdx.x] = a, sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sa[threadIdx.x] += sa[threadIdx.x + o], sb[threadIdx.x] += sb[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[0] += sa[0], stats[1] += sb[0];
}

template <int KB>   // K / 32
__global__ __launch_bounds__(64 * HC_WAVES) void hc_bwd_kernel(const float* __restrict__ x, long long ld, const uint4* __restrict__ wa_hi,
                                                               const uint4* __restrict__ wa_lo, const uint4* __restrict__ wb_hi,
                                                               const uint4* __restrict__ wb_lo, const long long* __restrict__ t64,
                                                               const short* __restrict__ t16, const float* __restrict__ group_w, int group,
                                                               const float* __restrict__ lse, const float* __restrict__ g, float* __restrict__ dx,
                                                               long long ldx, long long R, int V) {
  extern __shared__ __attribute__((aligned(16))) char hc_lds[];
  __shared__ float sc[HC_BWD_ROWS];
  constexpr int K = 32 * KB, KS = 2 * KB, pitch = 2 * K + 16, loff = HC_BWD_ROWS * pitch;
  const long long pt = (long long)blockIdx.x * HC_BWD_ROWS;   // < R: the grid is ceil(R / 32)
  hc_stage(hc_lds, loff, pitch, x, ld, pt, HC_BWD_ROWS, R, K, threadIdx.x, 64 * HC_WAVES);
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const long long p = pt + r;
  int tgt = -1;
  float ls = INFINITY, cr = 0.f;   // a row past the end: p = exp(-inf) = 0, nothing stored
  if (p < R) {
    tgt = hc_target(t64, t16, p, V);
    ls = lse[p];
    cr = g[0] * (group_w ? group_w[p / group] : 1.f);
  }
  if (q == 0 && h == 0) sc[r] = cr;
  __syncthreads();
  f32x16 acc2[KB];
#pragma unroll
  for (int kfb = 0; kfb < KB; ++kfb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc2[kfb][i] = 0.f;
  const int nvb = V / HC_VB;
  for (int vb = q; vb < nvb; vb += HC_WAVES) {   // wave-uniform
    f32x16 a1;
#pragma unroll
    for (int i = 0; i < 16; ++i) a1[i] = 0.f;
    const long long f0 = (long long)vb * KS * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      PlFrag w;
      w.h = __builtin_bit_cast(bf16x8, wa_hi[f0 + ks * 64]);
      w.l = __builtin_bit_cast(bf16x8, wa_lo[f0 + ks * 64]);
      pl_mma(a1, w, pl_rd(hc_lds, 0, loff, pitch, 0, 16 * ks, lane));
    }
    // register i: word 32 vb + MM_ROW(i, lane) of the lane's row -> softmax minus one-hot, in place
#pragma unroll
    for (int i = 0; i < 16; ++i) a1[i] = __expf(a1[i] - ls) - ((vb * HC_VB + MM_ROW(i, lane) == tgt) ? 1.f : 0.f);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      PlFrag pf;   // A operand: row r, contraction slots 8 h + 0..7 = registers 8 c + 0..7
      sf_split8(f32x8{a1[8 * c], a1[8 * c + 1], a1[8 * c + 2], a1[8 * c + 3], a1[8 * c + 4], a1[8 * c + 5], a1[8 * c + 6], a1[8 * c + 7]}, pf.h, pf.l);
      const long long f1 = ((long long)vb * 2 + c) * KB * 64 + lane;
#pragma unroll
      for (int kfb = 0; kfb < KB; ++kfb) {
        PlFrag w;
        w.h = __builtin_bit_cast(bf16x8, wb_hi[f1 + kfb * 64]);
        w.l = __builtin_bit_cast(bf16x8, wb_lo[f1 + kfb * 64]);
        pl_mma(acc2[kfb], pf, w);
      }
    }
  }
  // D2 block kfb: the lane holds feature 32 kfb + r and, in register i, row MM_ROW(i, lane).  The four waves' parts meet in wave 0, in the order
  // ((0 + 1) + 2) + 3, through the LDS the rows of x were staged in (32 x K floats fit the two planes); every thread reaches every barrier.
  __syncthreads();   // no wave reads the planes any more
  float* red = reinterpret_cast<float*>(hc_lds);
  for (int w = 1; w < HC_WAVES; ++w) {
    if (q == w) {
#pragma unroll
      for (int kfb = 0; kfb < KB; ++kfb)
#pragma unroll
        for (int i = 0; i < 16; ++i) red[MM_ROW(i, lane) * K + 32 * kfb + r] = acc2[kfb][i];
    }
    __syncthreads();
    if (q == 0) {
#pragma unroll
      for (int kfb = 0; kfb < KB; ++kfb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc2[kfb][i] += red[MM_ROW(i, lane) * K + 32 * kfb + r];
    }
    __syncthreads();
  }
  if (q != 0) return;
  // A dropped row (c_r = 0) is an exact zero.
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = MM_ROW(i, lane);
    const long long pr = pt + row;
    const float c = sc[row];
    if (pr < R) {
#pragma unroll
      for (int kfb = 0; kfb < KB; ++kfb) dx[pr * ldx + 32 * kfb + r] = c != 0.f ? c * acc2[kfb][i] : 0.f;
    }
  }
}

inline bool hc_ok(int V, int K) { return K >= 32 && K <= HC_MAX_K && K % 32 == 0 && V >= HC_VB && V % HC_VB == 0 && V <= HC_MAX_V; }
inline size_t hc_lds_bytes(int K, int rows) { return (size_t)2 * rows * (2 * K + 16); }
inline long long hc_tiles(long long R, int rows = HC_ROWS) { return (R + rows - 1) / rows; }

template <int KB>
int hc_launch_bwd(const float* x, long long ld, const uint4* wp, long long n8, const long long* t64, const short* t16, const float* group_w, int group,
                  const float* lse, const float* g, float* dx, long long ldx, long long R, int V, hipStream_t st) {
  const size_t lds = hc_lds_bytes(32 * KB, HC_BWD_ROWS);   // at most 33 KiB
  hipLaunchKernelGGL(hc_bwd_kernel<KB>, dim3((unsigned)hc_tiles(R, HC_BWD_ROWS)), dim3(64 * HC_WAVES), lds, st, x, ld, wp, wp + n8, wp + 2 * n8, wp + 3 * n8, t64,
                     t16, group_w, group, lse, g, dx, ldx, R, V);
  SF_CHECK_LAUNCH();
  return 0;
}

// ---- the head's own gradient ---------------------------------------------------------------------------------------------------------------------
constexpr int HC_WG_ROWS = 32;       // rows of a tile of the weight gradient's sweep: one MFMA block
constexpr int HC_WG_MAX_SPLIT = 8;   // most row splits of a launch: the workspace is at most this many [V][K] blocks
constexpr int HC_WG_FILL = 256;      // workgroups a launch aims at.  A constant, not the device's CU count: equal shapes split equally everywhere

// Row splits of a launch over R rows and V words: S0 = min(HC_WG_MAX_SPLIT, ceil(HC_WG_FILL / slabs), tiles) runs of ceil(tiles / S0) tiles each, and S
// the number of such runs that hold a tile.  The kernel finds the run length again as ceil(tiles / S).
inline int hc_wg_splits(long long R, int V) {
  const long long tiles = hc_tiles(R, HC_WG_ROWS), slabs = (V + HC_VB * HC_WAVES - 1) / (HC_VB * HC_WAVES);
  long long s0 = (HC_WG_FILL + slabs - 1) / slabs;
  if (s0 > HC_WG_MAX_SPLIT) s0 = HC_WG_MAX_SPLIT;
  if (s0 > tiles) s0 = tiles;
  if (s0 < 1) return 1;
  const long long per = (tiles + s0 - 1) / s0;
  return (int)((tiles + per - 1) / per);
}

template <int KB>   // K / 32
__global__ __launch_bounds__(64 * HC_WAVES) void hc_wgrad_kernel(const float* __restrict__ x, long long ld, const uint4* __restrict__ wa_hi,
                                                                 const uint4* __restrict__ wa_lo, const long long* __restrict__ t64,
                                                                 const short* __restrict__ t16, const float* __restrict__ group_w, int group,
                                                                 const float* __restrict__ lse, const float* __restrict__ g, float* __restrict__ part,
                                                                 long long R, int V) {
  extern __shared__ __attribute__((aligned(16))) char hc_lds[];
  __shared__ __attribute__((aligned(16))) float sl[2][HC_WG_ROWS], sc[2][HC_WG_ROWS];
  __shared__ __attribute__((aligned(16))) int stg[2][HC_WG_ROWS];
  constexpr int K = 32 * KB, KS = 2 * KB, k8 = K / 8, pitch = 2 * K + 16, loff = HC_WG_ROWS * pitch, buf = 2 * loff;
  constexpr int units = HC_WG_ROWS * k8, U = (units + 64 * HC_WAVES - 1) / (64 * HC_WAVES);   // 16-byte column groups of a tile, and a thread's share
  const int tid = threadIdx.x, lane = tid & 63;
  const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nvb = V / HC_VB, vb = (int)blockIdx.x * HC_WAVES + q;   // wave-uniform
  // a wave past the last block works on that block again and stores nothing: it stages its share of every tile and meets every barrier
  const int vbl = vb < nvb ? vb : nvb - 1;
  const long long tiles = (R + HC_WG_ROWS - 1) / HC_WG_ROWS, per = (tiles + gridDim.y - 1) / gridDim.y;
  const long long t0 = (long long)blockIdx.y * per, t1 = t0 + per < tiles ? t0 + per : tiles;
  const float gs = g[0];
  PlFrag wf[KS];   // the wave's 32 words as the B operand of the first product, for the whole sweep
  {
    const long long f0 = (long long)vbl * KS * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      wf[ks].h = __builtin_bit_cast(bf16x8, wa_hi[f0 + ks * 64]);
      wf[ks].l = __builtin_bit_cast(bf16x8, wa_lo[f0 + ks * 64]);
    }
  }
  f32x16 acc[KB];
#pragma unroll
  for (int kfb = 0; kfb < KB; ++kfb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[kfb][i] = 0.f;
  // a thread's share of the next tile on its way from memory to LDS: the loads are issued before the products of the current tile and land behind them
  f32x4 pa[U], pb[U];
  int mt = -1;
  float ml = INFINITY, mc = 0.f;
  auto fetch = [&](long long row0) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int u = tid + 64 * HC_WAVES * j, row = u / k8, c = u - row * k8;
      pa[j] = f32x4{0.f, 0.f, 0.f, 0.f}, pb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < units && row0 + row < R) {   // a row past the end is a zero operand, never an address
        const float* xp = x + (row0 + row) * ld + 8 * c;
        pa[j] = *reinterpret_cast<const f32x4*>(xp);
        pb[j] = *reinterpret_cast<const f32x4*>(xp + 4);
      }
    }
    mt = -1, ml = INFINITY, mc = 0.f;   // a row past the end: c = 0, nothing added
    const long long p = row0 + tid;
    if (tid < HC_WG_ROWS && p < R) {
      mt = hc_target(t64, t16, p, V);
      ml = lse[p];
      mc = gs * (group_w ? group_w[p / group] : 1.f);
    }
  };
  auto put = [&](int b) {
    char* dst = hc_lds + b * buf;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int u = tid + 64 * HC_WAVES * j, row = u / k8, c = u - row * k8;
      if (u < units) {
        bf16x8 hi, lo;
        sf_split8(pa[j], pb[j], hi, lo);
        *reinterpret_cast<bf16x8*>(dst + row * pitch + c * 16) = hi;
        *reinterpret_cast<bf16x8*>(dst + loff + row * pitch + c * 16) = lo;
      }
    }
    if (tid < HC_WG_ROWS) stg[b][tid] = mt, sl[b][tid] = ml, sc[b][tid] = mc;
  };
  if (t0 < t1) {   // uniform over the workgroup
    fetch(t0 * HC_WG_ROWS);
    put(0);
  }
  __syncthreads();
  const int word = vbl * HC_VB + r;
  for (long long t = t0; t < t1; ++t) {
    const int cur = (int)(t - t0) & 1;
    const char* tile = hc_lds + cur * buf;
    if (t + 1 < t1) fetch((t + 1) * HC_WG_ROWS);
    // D1[row][word]: the lane holds its word's logit of row MM_ROW(i, lane) in register i
    f32x16 a1;
#pragma unroll
    for (int i = 0; i < 16; ++i) a1[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) pl_mma(a1, pl_rd(tile, 0, loff, pitch, 0, 16 * ks, lane), wf[ks]);
    // c_r (softmax - onehot), in place; a dropped row (c_r = 0) is an exact zero whatever its lse
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(&sl[cur][8 * qd + 4 * h]);
      const f32x4 c4 = *reinterpret_cast<const f32x4*>(&sc[cur][8 * qd + 4 * h]);
      const int4 t4 = *reinterpret_cast<const int4*>(&stg[cur][8 * qd + 4 * h]);
      const int tt[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * qd + j;
        a1[i] = c4[j] != 0.f ? c4[j] * (__expf(a1[i] - l4[j]) - (word == tt[j] ? 1.f : 0.f)) : 0.f;
      }
    }
    // D3[word][feature] += P x: registers 8 c .. 8 c + 7 are the A operand of k-step c (rows 16 c + 8 (j >> 2) + 4 h + (j & 3)), and x read down the
    // tile's rows in that order is its B operand
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      PlFrag pf;
      sf_split8(f32x8{a1[8 * c], a1[8 * c + 1], a1[8 * c + 2], a1[8 * c + 3], a1[8 * c + 4], a1[8 * c + 5], a1[8 * c + 6], a1[8 * c + 7]}, pf.h, pf.l);
#pragma unroll
      for (int kfb = 0; kfb < KB; ++kfb) pl_mma(acc[kfb], pf, pl_rd_tr(tile, 0, loff, pitch, 16 * c, 32 * kfb, lane, 4, 8));
    }
    if (t + 1 < t1) put(cur ^ 1);   // the other buffer: every wave left it before the barrier that ended the previous tile
    __syncthreads();
  }
  if (vb >= nvb) return;
  // block kfb: the lane holds feature 32 kfb + r and, in register i, word MM_ROW(i, lane) of the wave's 32
  float* out = part + ((long long)blockIdx.y * V + (long long)vb * HC_VB) * K;
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int kfb = 0; kfb < KB; ++kfb) out[MM_ROW(i, lane) * K + 32 * kfb + r] = acc[kfb][i];
}

// dW = the splits' partial blocks, added in index order
__global__ __launch_bounds__(256) void hc_wgrad_sum_kernel(const float* __restrict__ part, int S, float* __restrict__ dW, long long ldw, long long n,
                                                           int K) {
  const long long idx = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;   // n and K are multiples of 4: the four elements share a row
  if (idx >= n) return;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) a += *reinterpret_cast<const f32x4*>(part + s * n + idx);
  const long long v = idx / K;
  float* o = dW + v * ldw + (idx - v * K);
  o[0] = a[0], o[1] = a[1], o[2] = a[2], o[3] = a[3];
}

template <int KB>
int hc_launch_wgrad(const float* x, long long ld, const uint4* wp, long long n8, const long long* t64, const short* t16, const float* group_w, int group,
                    const float* lse, const float* g, float* part, long long R, int V, int S, hipStream_t st) {
  const size_t lds = 2 * hc_lds_bytes(32 * KB, HC_WG_ROWS);   // two buffers: at most 66 KiB
  if (lds > 64 * 1024) SF_TRY(sf_ensure_dyn_lds((const void*)hc_wgrad_kernel<KB>, lds));
  hipLaunchKernelGGL(hc_wgrad_kernel<KB>, dim3((unsigned)((V + HC_VB * HC_WAVES - 1) / (HC_VB * HC_WAVES)), (unsigned)S), dim3(64 * HC_WAVES), lds, st, x,
                     ld, wp, wp + n8, t64, t16, group_w, group, lse, g, part, R, V);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

#define HC_SHAPE_MSG "K must be a multiple of 32 in [32, 256] and V a multiple of 32 in [32, 2^20]"

extern "C" {

int sf_head_ce_ok(int V, int K) { return hc_ok(V, K) ? 1 : 0; }

size_t sf_head_ce_packed_bytes(int V, int K) { return hc_ok(V, K) ? (size_t)V * K * 8 : 0; }

size_t sf_head_ce_workspace_bytes(long long R) { return R >= 0 && R < HC_MAX_R ? (size_t)(hc_tiles(R) > 0 ? hc_tiles(R) : 1) * 16 : 0; }

int sf_head_ce_pack_weights(const float* w, void* packed, int V, int K, void* stream) {
  SF_REQUIRE(w && packed, "sf_head_ce_pack_weights: null pointer");
  SF_REQUIRE(hc_ok(V, K), "sf_head_ce_pack_weights: " HC_SHAPE_MSG);
  const long long n = (long long)V * K;
  hipLaunchKernelGGL(hc_pack_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, static_cast<unsigned short*>(packed), n,
                     K);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_head_ce_pack_weights_host(const float* w, void* packed, int V, int K) {
  SF_REQUIRE(w && packed, "sf_head_ce_pack_weights_host: null pointer");
  SF_REQUIRE(hc_ok(V, K), "sf_head_ce_pack_weights_host: " HC_SHAPE_MSG);
  const long long n = (long long)V * K;
  for (long long idx = 0; idx < 2 * n; ++idx) hc_pack_one(w, static_cast<unsigned short*>(packed), idx, n, K);
  return 0;
}

int sf_head_ce_fwd_f32(const float* x, long long ld, const void* w_packed, const long long* target_i64, const short* target_i16, const float* group_w,
                       int group, float* lse, float* loss_rows, double* stats, long long R, int V, int K, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(x && w_packed && lse, "sf_head_ce_fwd_f32: null pointer");
  SF_REQUIRE((target_i64 != nullptr) != (target_i16 != nullptr), "sf_head_ce_fwd_f32: exactly one of target_i64 and target_i16");
  SF_REQUIRE(hc_ok(V, K), "sf_head_ce_fwd_f32: " HC_SHAPE_MSG);
  SF_REQUIRE(!target_i16 || V <= 32768, "sf_head_ce_fwd_f32: int16 targets need V <= 32768");
  SF_REQUIRE(ld >= K && ld % 4 == 0, "sf_head_ce_fwd_f32: the row stride must be at least K and a multiple of 4");
  SF_REQUIRE(R >= 0 && R < HC_MAX_R, "sf_head_ce_fwd_f32: bad row count");
  SF_REQUIRE(group >= 1 && R % group == 0, "sf_head_ce_fwd_f32: group must be at least 1 and divide R");
  SF_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w_packed & 15) == 0, "sf_head_ce_fwd_f32: x and w_packed must be 16-byte aligned");
  SF_REQUIRE(!stats || (((uintptr_t)stats & 7) == 0 && ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= sf_head_ce_workspace_bytes(R)),
             "sf_head_ce_fwd_f32: stats needs 8-byte alignment and a workspace of sf_head_ce_workspace_bytes(R)");
  if (R == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = hc_lds_bytes(K, HC_ROWS);
  if (lds > 64 * 1024) SF_TRY(sf_ensure_dyn_lds((const void*)hc_fwd_kernel, lds));
  const uint4* wp = static_cast<const uint4*>(w_packed);
  const long long n8 = (long long)V * K / 8, tiles = hc_tiles(R);
  double* partial = stats ? static_cast<double*>(ws) : nullptr;
  hipLaunchKernelGGL(hc_fwd_kernel, dim3((unsigned)tiles), dim3(64 * HC_WAVES), lds, st, x, ld, wp, wp + n8, target_i64, target_i16, group_w, group,
                     lse, loss_rows, partial, R, V, K);
  SF_CHECK_LAUNCH();
  if (stats) {
    hipLaunchKernelGGL(hc_stats_kernel, dim3(1), dim3(256), 0, st, partial, tiles, stats);
    SF_CHECK_LAUNCH();
  }
  return 0;
}

int sf_head_ce_bwd_f32(const float* x, long long ld, const void* w_packed, const long long* target_i64, const short* target_i16, const float* group_w,
                       int group, const float* lse, const float* g, float* dx, long long ldx, long long R, int V, int K, void* stream) {
  SF_REQUIRE(x && w_packed && lse && g && dx, "sf_head_ce_bwd_f32: null pointer");
  SF_REQUIRE((target_i64 != nullptr) != (target_i16 != nullptr), "sf_head_ce_bwd_f32: exactly one of target_i64 and target_i16");
  SF_REQUIRE(hc_ok(V, K), "sf_head_ce_bwd_f32: " HC_SHAPE_MSG);
  SF_REQUIRE(!target_i16 || V <= 32768, "sf_head_ce_bwd_f32: int16 targets need V <= 32768");
  SF_REQUIRE(ld >= K && ld % 4 == 0, "sf_head_ce_bwd_f32: the row stride of x must be at least K and a multiple of 4");
  SF_REQUIRE(ldx >= K, "sf_head_ce_bwd_f32: the row stride of dx must be at least K");
  SF_REQUIRE(R >= 0 && R < HC_MAX_R, "sf_head_ce_bwd_f32: bad row count");
  SF_REQUIRE(group >= 1 && R % group == 0, "sf_head_ce_bwd_f32: group must be at least 1 and divide R");
  SF_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w_packed & 15) == 0, "sf_head_ce_bwd_f32: x and w_packed must be 16-byte aligned");
  if (R == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const uint4* wp = static_cast<const uint4*>(w_packed);
  const long long n8 = (long long)V * K / 8;
#define HC_CASE(KB) \
  case KB:          \
    return hc_launch_bwd<KB>(x, ld, wp, n8, target_i64, target_i16, group_w, group, lse, g, dx, ldx, R, V, st);
  switch (K / 32) {
    HC_CASE(1) HC_CASE(2) HC_CASE(3) HC_CASE(4) HC_CASE(5) HC_CASE(6) HC_CASE(7) HC_CASE(8)
  }
#undef HC_CASE
  return sf_set_err(-1, "invalid argument: sf_head_ce_bwd_f32: " HC_SHAPE_MSG, __FILE__, __LINE__);
}

size_t sf_head_ce_wgrad_workspace_bytes(long long R, int V, int K) {
  return hc_ok(V, K) && R >= 0 && R < HC_MAX_R ? (size_t)hc_wg_splits(R, V) * V * K * sizeof(float) : 0;
}

int sf_head_ce_wgrad_f32(const float* x, long long ld, const void* w_packed, const long long* target_i64, const short* target_i16, const float* group_w,
                         const float* lse, const float* g, float* dW, long long ldw, long long R, int V, int K, int group, void* ws, size_t ws_bytes,
                         void* stream) {
  SF_REQUIRE(x && w_packed && lse && g && dW && ws, "sf_head_ce_wgrad_f32: null pointer");
  SF_REQUIRE((target_i64 != nullptr) != (target_i16 != nullptr), "sf_head_ce_wgrad_f32: exactly one of target_i64 and target_i16");
  SF_REQUIRE(hc_ok(V, K), "sf_head_ce_wgrad_f32: " HC_SHAPE_MSG);
  SF_REQUIRE(!target_i16 || V <= 32768, "sf_head_ce_wgrad_f32: int16 targets need V <= 32768");
  SF_REQUIRE(ld >= K && ld % 4 == 0, "sf_head_ce_wgrad_f32: the row stride of x must be at least K and a multiple of 4");
  SF_REQUIRE(ldw >= K, "sf_head_ce_wgrad_f32: the row stride of dW must be at least K");
  SF_REQUIRE(R >= 0 && R < HC_MAX_R, "sf_head_ce_wgrad_f32: bad row count");
  SF_REQUIRE(group >= 1 && R % group == 0, "sf_head_ce_wgrad_f32: group must be at least 1 and divide R");
  SF_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w_packed & 15) == 0, "sf_head_ce_wgrad_f32: x and w_packed must be 16-byte aligned");
  SF_REQUIRE(((uintptr_t)ws & 15) == 0 && ws_bytes >= sf_head_ce_wgrad_workspace_bytes(R, V, K),
             "sf_head_ce_wgrad_f32: needs a 16-byte aligned workspace of sf_head_ce_wgrad_workspace_bytes(R, V, K)");
  hipStream_t st = (hipStream_t)stream;
  const uint4* wp = static_cast<const uint4*>(w_packed);
  const long long n = (long long)V * K, n8 = n / 8;
  const int S = R > 0 ? hc_wg_splits(R, V) : 0;   // no rows: the sum of no blocks, zeros
  float* part = static_cast<float*>(ws);
  int rc = 0;
#define HC_CASE(KB) \
  case KB:          \
    rc = hc_launch_wgrad<KB>(x, ld, wp, n8, target_i64, target_i16, group_w, group, lse, g, part, R, V, S, st); \
    break;
  if (S > 0) switch (K / 32) { HC_CASE(1) HC_CASE(2) HC_CASE(3) HC_CASE(4) HC_CASE(5) HC_CASE(6) HC_CASE(7) HC_CASE(8) }
#undef HC_CASE
  if (rc != 0) return rc;
  hipLaunchKernelGGL(hc_wgrad_sum_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, part, S, dW, ldw, n, K);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

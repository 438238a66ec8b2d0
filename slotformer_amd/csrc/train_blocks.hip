// The gradient building blocks of train_blocks.h: the kernels every training node launches for its parameter gradients and the LayerNorm / ReLU
// backward, their launchers, and the two entry points that are nothing but those blocks (sf_linear_bwd_f32, sf_layernorm_bwd_f32).
//   * a weight gradient is ONE contraction over all rows: dW = dY^T . X on a split-bf16 MFMA kernel that reads both operands in their natural
//     row-major layout (no transposes), split over row ranges into partial tiles that a second kernel sums in a fixed order (deterministic; no atomics);
//   * bias and LayerNorm-parameter gradients are column sums over the same rows, in the same two stages.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "train_blocks.h"
#include "sf_arena.h"
#include "bf16_planes.h"
#include "dropout_mask.h"   // sf_keep: the mask convention of ln_bwd_kernel's second output

// dpre = hdn > 0 ? dh * inv_keep : 0   (hdn is the saved post-ReLU, post-dropout hidden activation)
__global__ __launch_bounds__(256) void relu_dropout_bwd_kernel(float* __restrict__ dh, const float* __restrict__ hdn,
                                                               long long n4, float inv_keep) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 g = reinterpret_cast<float4*>(dh)[i];
  const float4 h = reinterpret_cast<const float4*>(hdn)[i];
  g.x = h.x > 0.f ? g.x * inv_keep : 0.f;
  g.y = h.y > 0.f ? g.y * inv_keep : 0.f;
  g.z = h.z > 0.f ? g.z * inv_keep : 0.f;
  g.w = h.w > 0.f ? g.w * inv_keep : 0.f;
  reinterpret_cast<float4*>(dh)[i] = g;
}

// out[c][r] = in[r][c]
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int Cn) {
  __shared__ float t[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < R && c0 + tx < Cn) t[i][tx] = in[(long long)(r0 + i) * Cn + c0 + tx];
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < Cn && r0 + tx < R) out[(long long)(c0 + i) * R + r0 + tx] = t[tx][i];
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm backward (one wave per row, D <= 1024, D % 4 == 0):  out = dres + dLN(dy; x, gamma)
// ---------------------------------------------------------------------------------------------------------------------
// out2 (optional): the same gradient pushed through the dropout of the block below it (mask * out / keep), i.e. the
// gradient w.r.t. that block's pre-dropout output -- saves a separate pass over the tensor.
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                     const float* __restrict__ gamma, const float* __restrict__ dres,
                                                     float* __restrict__ out, float* __restrict__ out2, uint32_t sseed2,
                                                     uint32_t thresh, float inv_keep, int rows, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int n4 = D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(x + (long long)row * D);
  const float4* gr = reinterpret_cast<const float4*>(dy + (long long)row * D);
  const float4* gm = reinterpret_cast<const float4*>(gamma);
  float4 xv[4], gv[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    xv[i] = c < n4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (xv[i].x + xv[i].y) + (xv[i].z + xv[i].w);
  }
  const float mean = sf_wave_sum(s) / D;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < n4) {
      xv[i].x -= mean; xv[i].y -= mean; xv[i].z -= mean; xv[i].w -= mean;
      var += (xv[i].x * xv[i].x + xv[i].y * xv[i].y) + (xv[i].z * xv[i].z + xv[i].w * xv[i].w);
    }
  }
  const float rstd = rsqrtf(sf_wave_sum(var) / D + eps);
  float m1 = 0.f, m2 = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < n4) {
      const float4 w = gm[c];
      float4 g = gr[c];
      g.x *= w.x; g.y *= w.y; g.z *= w.z; g.w *= w.w;
      xv[i].x *= rstd; xv[i].y *= rstd; xv[i].z *= rstd; xv[i].w *= rstd;   // x-hat
      gv[i] = g;
      m1 += (g.x + g.y) + (g.z + g.w);
      m2 += (g.x * xv[i].x + g.y * xv[i].y) + (g.z * xv[i].z + g.w * xv[i].w);
    }
  }
  m1 = sf_wave_sum(m1) / D;
  m2 = sf_wave_sum(m2) / D;
  const float4* rr = dres ? reinterpret_cast<const float4*>(dres + (long long)row * D) : nullptr;
  float4* orow = reinterpret_cast<float4*>(out + (long long)row * D);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < n4) {
      float4 r = rr ? rr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      r.x += rstd * (gv[i].x - m1 - xv[i].x * m2);
      r.y += rstd * (gv[i].y - m1 - xv[i].y * m2);
      r.z += rstd * (gv[i].z - m1 - xv[i].z * m2);
      r.w += rstd * (gv[i].w - m1 - xv[i].w * m2);
      orow[c] = r;
      if (out2) {
        if (thresh) {
          const uint32_t e = (uint32_t)(row * D + 4 * c);
          r.x = sf_keep(sseed2, e, thresh) ? r.x * inv_keep : 0.f;
          r.y = sf_keep(sseed2, e + 1, thresh) ? r.y * inv_keep : 0.f;
          r.z = sf_keep(sseed2, e + 2, thresh) ? r.z * inv_keep : 0.f;
          r.w = sf_keep(sseed2, e + 3, thresh) ? r.w * inv_keep : 0.f;
        }
        reinterpret_cast<float4*>(out2 + (long long)row * D)[c] = r;
      }
    }
  }
}

// LayerNorm parameter gradients, stage 1: workgroup g handles rows [g*rpg, (g+1)*rpg); partial[g][0][D] = sum dy*xhat,
// partial[g][1][D] = sum dy.  D <= 1024, D % 4 == 0.
__global__ __launch_bounds__(256) void ln_param_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ partial, long long rows, int rpg, int D,
                                                               float eps) {
  __shared__ float red[3][2][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n4 = D >> 2;
  float4 ag[4], ab[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ag[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const long long r0 = (long long)blockIdx.x * rpg;
  const long long r1 = r0 + rpg < rows ? r0 + rpg : rows;
  for (long long row = r0 + wave; row < r1; row += 4) {
    const float4* xr = reinterpret_cast<const float4*>(x + row * D);
    const float4* gr = reinterpret_cast<const float4*>(dy + row * D);
    float4 xv[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      xv[i] = c < n4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      s += (xv[i].x + xv[i].y) + (xv[i].z + xv[i].w);
    }
    const float mean = sf_wave_sum(s) / D;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < n4) {
        xv[i].x -= mean; xv[i].y -= mean; xv[i].z -= mean; xv[i].w -= mean;
        var += (xv[i].x * xv[i].x + xv[i].y * xv[i].y) + (xv[i].z * xv[i].z + xv[i].w * xv[i].w);
      }
    }
    const float rstd = rsqrtf(sf_wave_sum(var) / D + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < n4) {
        const float4 g = gr[c];
        ag[i].x += g.x * xv[i].x * rstd; ag[i].y += g.y * xv[i].y * rstd;
        ag[i].z += g.z * xv[i].z * rstd; ag[i].w += g.w * xv[i].w * rstd;
        ab[i].x += g.x; ab[i].y += g.y; ab[i].z += g.z; ab[i].w += g.w;
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < n4) {
        reinterpret_cast<float4*>(red[wave - 1][0])[c] = ag[i];
        reinterpret_cast<float4*>(red[wave - 1][1])[c] = ab[i];
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < n4) {
        for (int w = 0; w < 3; ++w) {
          const float4 a = reinterpret_cast<float4*>(red[w][0])[c], b = reinterpret_cast<float4*>(red[w][1])[c];
          ag[i].x += a.x; ag[i].y += a.y; ag[i].z += a.z; ag[i].w += a.w;
          ab[i].x += b.x; ab[i].y += b.y; ab[i].z += b.z; ab[i].w += b.w;
        }
        reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2) * D)[c] = ag[i];
        reinterpret_cast<float4*>(partial + ((long long)blockIdx.x * 2 + 1) * D)[c] = ab[i];
      }
    }
  }
}

// column sums, stage 1: partial[g][n] = sum over rows [g*rpg, (g+1)*rpg) of y[row][n].  The 256 threads of a workgroup
// cover min(n, 256) columns x 256 / that many row lanes (narrow matrices -- conv / head gradients have n = 4 .. 64 and
// millions of rows -- keep every lane busy), four loads in flight per lane, row lanes combined through LDS.
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ y, float* __restrict__ partial,
                                                             long long rows, int rpg, int n) {
  __shared__ float red[256];
  int cols = 1;
  while (cols < n && cols < 256) cols <<= 1;   // columns per workgroup (power of two)
  const int lanes = 256 / cols;
  const int cl = threadIdx.x % cols, rl = threadIdx.x / cols;
  const int c = blockIdx.x * cols + cl;
  const long long r0 = (long long)blockIdx.y * rpg;
  const long long r1 = r0 + rpg < rows ? r0 + rpg : rows;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < n) {
    long long r = r0 + rl;
    for (; r + 3LL * lanes < r1; r += 4LL * lanes) {
      s0 += y[r * n + c];
      s1 += y[(r + lanes) * n + c];
      s2 += y[(r + 2LL * lanes) * n + c];
      s3 += y[(r + 3LL * lanes) * n + c];
    }
    for (; r < r1; r += lanes) s0 += y[r * n + c];
  }
  red[threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (rl == 0 && c < n) {
    float a = red[cl];
    for (int i = 1; i < lanes; ++i) a += red[i * cols + cl];
    partial[(long long)blockIdx.y * n + c] = a;
  }
}

// stage 2 of every split reduction: out[i] = sum_g partial[g][i]  (fixed order: four interleaved chains, then their sum)
// (columns >= n4a go to out2 when it is given: one launch writes d_gamma and d_beta of a LayerNorm)
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                              int G, long long n4, float* __restrict__ out2, long long n4a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4* p = reinterpret_cast<const float4*>(partial) + i;
  float4 a[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  int g = 0;
  for (; g + 4 <= G; g += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 b = p[(long long)(g + u) * n4];
      a[u].x += b.x; a[u].y += b.y; a[u].z += b.z; a[u].w += b.w;
    }
  }
  for (; g < G; ++g) {
    const float4 b = p[(long long)g * n4];
    a[0].x += b.x; a[0].y += b.y; a[0].z += b.z; a[0].w += b.w;
  }
  float4 r;
  r.x = (a[0].x + a[1].x) + (a[2].x + a[3].x);
  r.y = (a[0].y + a[1].y) + (a[2].y + a[3].y);
  r.z = (a[0].z + a[1].z) + (a[2].z + a[3].z);
  r.w = (a[0].w + a[1].w) + (a[2].w + a[3].w);
  if (out2 && i >= n4a) reinterpret_cast<float4*>(out2)[i - n4a] = r;
  else reinterpret_cast<float4*>(out)[i] = r;
}

// the same reduction for few columns and many partials (bias / LayerNorm / 64x64 weight gradients: up to 512 partials of 16
// to 1024 float4 columns, where one thread per column leaves the chip idle behind a handful of long serial chains): a
// workgroup takes 16 columns, its 16 thread rows each sum every 16th partial, LDS combines the rows in a fixed tree.
__global__ __launch_bounds__(256) void reduce_partials_wide_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                                   int G, long long n4, float* __restrict__ out2, long long n4a) {
  const int c = threadIdx.x & 15, q = threadIdx.x >> 4;
  const long long i = (long long)blockIdx.x * 16 + c;
  __shared__ f32x4 sh[16][17];
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  if (i < n4) {
    const f32x4* p = reinterpret_cast<const f32x4*>(partial) + i;
    for (int g = q; g < G; g += 16) a += p[(long long)g * n4];
  }
  sh[q][c] = a;
  __syncthreads();
#pragma unroll
  for (int w = 8; w > 0; w >>= 1) {
    if (q < w) sh[q][c] += sh[q + w][c];
    __syncthreads();
  }
  if (q == 0 && i < n4) {
    if (out2 && i >= n4a) reinterpret_cast<f32x4*>(out2)[i - n4a] = sh[0][c];
    else reinterpret_cast<f32x4*>(out)[i] = sh[0][c];
  }
}
inline void launch_reduce_partials(const float* partial, float* out, int G, long long n4, hipStream_t st, float* out2 = nullptr,
                                   long long n4a = 0) {
  if (G >= 32 && n4 <= 16384)
    hipLaunchKernelGGL(reduce_partials_wide_kernel, dim3((unsigned)((n4 + 15) / 16)), dim3(256), 0, st, partial, out, G, n4, out2, n4a);
  else
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, partial, out, G, n4, out2, n4a);
}

// ---------------------------------------------------------------------------------------------------------------------
// weight-gradient contraction  dW[n][k] = sum_m Y[m][n] * X[m][k]   (Y [rows, N], X [rows, K], both row-major)
// split-bf16 on v_mfma_f32_32x32x16_bf16; 64x64 output tile per workgroup (4 waves, one 32x32 quadrant each), the
// contraction index is the row index: a chunk of 32 rows of both operands is staged in LDS as f32 and every lane reads
// its 8 values per k16 step with a stride of one LDS row (pitch 68: the two half-waves hit disjoint banks).
// grid (N/64 * K/64, splits): split z handles rows [z*rps, (z+1)*rps) and writes partial[z][N][K].
// ---------------------------------------------------------------------------------------------------------------------
// The 32-row chunk of both operands lives in LDS as bf16 hi / lo PLANES (bf16_planes.h; every element split once, where it is staged, instead of once per
// wave that reads it): the contraction index is the tile's ROW index, so the operand fragments come out through ds_read_b64_tr_b16 -- two transposing
// reads per plane and k16 step instead of eight scalar reads + a conversion chain.  Row pitch 192 bytes: the four rows x two 16-column groups a
// half-wave touches per read land on disjoint banks.
#define TN_PB 192
// EDGE: N and K multiples of 4 only -- the tiles of the last tile row / column load zeros past the matrix (a float4 lies inside or outside as a whole) and
// store inside it; the arithmetic of an interior element is that of the plain form.
template <int MODE, bool EDGE = false>   // 0: hi*hi + hi*lo + lo*hi + lo*lo, 1: without lo*lo (split-bf16), 2: hi*hi only (single-pass bf16)
__global__ __launch_bounds__(256) void grad_gemm_tn_kernel(const float* __restrict__ Y, const float* __restrict__ X,
                                                           float* __restrict__ partial, long long rows, int rps, int N,
                                                           int K) {
  constexpr int PT = 32 * TN_PB, YH = 0, YL = PT, XH = 2 * PT, XL = 3 * PT;
  __shared__ __attribute__((aligned(16))) char tsm[4 * PT + 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tk = EDGE ? (K + 63) / 64 : K / 64;
  const int n0 = (blockIdx.x / tk) * 64, k0 = (blockIdx.x % tk) * 64;
  const long long r0 = (long long)blockIdx.y * rps;
  const long long r1 = r0 + rps < rows ? r0 + rps : rows;
  const int wn = (wave >> 1) * 32, wk = (wave & 1) * 32;
  // loader: thread -> (row = tid >> 4 (+16), float4 column = tid & 15)
  const int lr = tid >> 4, lc = (tid & 15) * 4;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int nrows = (int)(r1 - r0);   // <= rps
  const float* Yb = Y + r0 * N + n0 + lc;
  const float* Xb = X + r0 * K + k0 + lc;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool yin = !EDGE || n0 + lc < N, xin = !EDGE || k0 + lc < K;   // (EDGE: this thread's float4 column lies inside the matrix)
  float4 py0 = zero4, py1 = zero4, px0 = zero4, px1 = zero4;
  if (lr < nrows) {
    if (yin) py0 = *reinterpret_cast<const float4*>(Yb + (long long)lr * N);
    if (xin) px0 = *reinterpret_cast<const float4*>(Xb + (long long)lr * K);
  }
  if (lr + 16 < nrows) {
    if (yin) py1 = *reinterpret_cast<const float4*>(Yb + (long long)(lr + 16) * N);
    if (xin) px1 = *reinterpret_cast<const float4*>(Xb + (long long)(lr + 16) * K);
  }
  auto stage = [&](const float4 v, int hoff, int loff, int row) {
    unsigned h0, l0, h1, l1;
    pl_split2(v.x, v.y, h0, l0);
    pl_split2(v.z, v.w, h1, l1);
    *(u32x2*)(tsm + hoff + row * TN_PB + lc * 2) = u32x2{h0, h1};
    if (MODE != 2) *(u32x2*)(tsm + loff + row * TN_PB + lc * 2) = u32x2{l0, l1};
  };
  for (int rb = 0; rb < nrows; rb += 32) {
    __syncthreads();
    stage(py0, YH, YL, lr);
    stage(py1, YH, YL, lr + 16);
    stage(px0, XH, XL, lr);
    stage(px1, XH, XL, lr + 16);
    __syncthreads();
    py0 = py1 = px0 = px1 = zero4;
    const int ra = rb + 32 + lr;
    if (ra < nrows) {
      if (yin) py0 = *reinterpret_cast<const float4*>(Yb + (long long)ra * N);
      if (xin) px0 = *reinterpret_cast<const float4*>(Xb + (long long)ra * K);
    }
    if (ra + 16 < nrows) {
      if (yin) py1 = *reinterpret_cast<const float4*>(Yb + (long long)(ra + 16) * N);
      if (xin) px1 = *reinterpret_cast<const float4*>(Xb + (long long)(ra + 16) * K);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const PlFrag a = pl_rd_tr(tsm, YH, MODE != 2 ? YL : YH, TN_PB, 16 * t, wn, lane);   // lane (n, kk): rows 16 t + 8 kk .. + 7 of column wn + n
      const PlFrag b = pl_rd_tr(tsm, XH, MODE != 2 ? XL : XH, TN_PB, 16 * t, wk, lane);
      if (MODE != 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, acc, 0, 0, 0);
      }
      if (MODE == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.l, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, acc, 0, 0, 0);
    }
  }
  float* out = partial + (long long)blockIdx.y * N * K;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + wn + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (!EDGE || (n < N && k0 + wk + (lane & 31) < K)) out[(long long)n * K + k0 + wk + (lane & 31)] = acc[r];
  }
}
// ---- host side ----
namespace {
inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
// row groups of a two-stage column reduction with at least `min_rows` rows each: G groups of rpg rows
inline int row_groups(long long rows, int min_rows, int& rpg) {
  int G = (int)((rows + min_rows - 1) / min_rows);
  if (G > SF_GRAD_MAX_GROUPS) G = SF_GRAD_MAX_GROUPS;
  rpg = (int)((rows + G - 1) / G);
  return (int)((rows + rpg - 1) / rpg);
}
}  // namespace

size_t sf_grad_partial_floats(long long rows, int N, int K) {
  const size_t a = (size_t)tn_splits(rows, N, K) * N * K;
  const size_t b = sf_colsum_partial_floats(N > K ? N : K);
  return a > b ? a : b;
}
// dW = Y^T X over `rows` rows, written to dW [N, K]
int sf_grad_weight_ex(const float* Y, const float* X, float* dW, long long rows, int N, int K, float* partial, hipStream_t st) {
  SF_REQUIRE(N % 64 == 0 && K % 64 == 0, "weight-gradient contraction needs multiples of 64");
  const int splits = tn_splits(rows, N, K);
  int rps = (int)((rows + splits - 1) / splits);
  rps = (rps + 31) & ~31;
  float* dst = splits == 1 ? dW : partial;
  const dim3 grid((N / 64) * (K / 64), splits);
  if (sf_get_precision() == 0)
    hipLaunchKernelGGL(grad_gemm_tn_kernel<0>, grid, dim3(256), 0, st, Y, X, dst, rows, rps, N, K);
  else if (sf_get_precision() == 1)
    hipLaunchKernelGGL(grad_gemm_tn_kernel<1>, grid, dim3(256), 0, st, Y, X, dst, rows, rps, N, K);
  else
    hipLaunchKernelGGL(grad_gemm_tn_kernel<2>, grid, dim3(256), 0, st, Y, X, dst, rows, rps, N, K);
  SF_CHECK_LAUNCH();
  if (splits > 1) {
    const long long n4 = (long long)N * K / 4;
    launch_reduce_partials(partial, dW, splits, n4, st);
    SF_CHECK_LAUNCH();
  }
  return 0;
}

// The same contraction at N, K multiples of 4 (the Aloe reasoner: 144, 432, 130 ...): the edge-tile form, split-bf16 whatever the process precision;
// the row split and the fixed-order reduction are those of sf_grad_weight_ex.  dW 16-byte aligned when the rows are split.
size_t sf_grad_partial_edge_floats(long long rows, int N, int K) {
  const size_t a = (size_t)tn_splits_edge(rows, N, K) * N * K;
  const size_t b = sf_colsum_partial_floats(N > K ? N : K);
  return a > b ? a : b;
}
int sf_grad_weight_edge_ex(const float* Y, const float* X, float* dW, long long rows, int N, int K, float* partial, hipStream_t st) {
  SF_REQUIRE(N > 0 && K > 0 && N % 4 == 0 && K % 4 == 0, "edge weight-gradient contraction needs multiples of 4");
  const int splits = tn_splits_edge(rows, N, K);
  int rps = (int)((rows + splits - 1) / splits);
  rps = (rps + 31) & ~31;
  float* dst = splits == 1 ? dW : partial;
  const dim3 grid(((N + 63) / 64) * ((K + 63) / 64), splits);
  hipLaunchKernelGGL((grad_gemm_tn_kernel<1, true>), grid, dim3(256), 0, st, Y, X, dst, rows, rps, N, K);
  SF_CHECK_LAUNCH();
  if (splits > 1) {
    launch_reduce_partials(partial, dW, splits, (long long)N * K / 4, st);
    SF_CHECK_LAUNCH();
  }
  return 0;
}

int sf_grad_bias_ex(const float* Y, float* db, long long rows, int n, float* partial, hipStream_t st) {
  int rpg;
  const int G = row_groups(rows, 128, rpg);
  int cols = 1;
  while (cols < n && cols < 256) cols <<= 1;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(cdiv(n, cols), G), dim3(256), 0, st, Y, partial, rows, rpg, n);
  SF_CHECK_LAUNCH();
  launch_reduce_partials(partial, db, G, (long long)n / 4, st);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_grad_ln_ex(const float* x, const float* dy, float* dgamma, float* dbeta, long long rows, int D, float eps, float* partial,
                  hipStream_t st) {
  int rpg;
  const int G = row_groups(rows, 64, rpg);
  hipLaunchKernelGGL(ln_param_partial_kernel, dim3(G), dim3(256), 0, st, x, dy, partial, rows, rpg, D, eps);
  SF_CHECK_LAUNCH();
  // partial is [G][2][D]: one reduction over both rows, the first D columns to d_gamma and the rest to d_beta
  if ((((uintptr_t)dgamma | (uintptr_t)dbeta) & 15) == 0) {
    launch_reduce_partials(partial, dgamma, G, (long long)2 * D / 4, st, dbeta, (long long)D / 4);
    SF_CHECK_LAUNCH();
    return 0;
  }
  // destinations that are not 16-byte aligned (views at odd offsets of a flat bucket): through a [2][D] scratch behind the partials
  float* both = partial + (size_t)G * 2 * D;
  launch_reduce_partials(partial, both, G, (long long)2 * D / 4, st);
  SF_CHECK_LAUNCH();
  hipError_t e = hipMemcpyAsync(dgamma, both, D * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dbeta, both + D, D * sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  return 0;
}
int sf_ln_bwd_dropout_ex(const float* x, const float* dy, const float* gamma, const float* dres, float* out, float* out2, uint32_t sseed2,
                         uint32_t thresh, float inv_keep, long long rows, int D, float eps, hipStream_t st) {
  hipLaunchKernelGGL(ln_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, dy, gamma, dres, out, out2, sseed2, thresh, inv_keep, (int)rows, D,
                     eps);
  SF_CHECK_LAUNCH();
  return 0;
}
int sf_ln_bwd_ex(const float* x, const float* dy, const float* gamma, const float* dres, float* out, long long rows, int D,
                 float eps, hipStream_t st) {
  SF_REQUIRE(D % 4 == 0 && D <= 1024, "LayerNorm width");
  return sf_ln_bwd_dropout_ex(x, dy, gamma, dres, out, nullptr, 0u, 0u, 1.f, rows, D, eps, st);
}
int sf_transpose_ex(const float* in, float* out, int R, int Cn, hipStream_t st) {
  hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(Cn, 32), cdiv(R, 32)), dim3(256), 0, st, in, out, R, Cn);
  SF_CHECK_LAUNCH();
  return 0;
}
int sf_relu_dropout_bwd_ex(float* dh, const float* hdn, long long n, float inv_keep, hipStream_t st) {
  hipLaunchKernelGGL(relu_dropout_bwd_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, st, dh, hdn, n / 4, inv_keep);
  SF_CHECK_LAUNCH();
  return 0;
}
int sf_relu_bwd_ex(float* dh, const float* h, long long n, hipStream_t st) {
  hipLaunchKernelGGL(relu_dropout_bwd_kernel, dim3(cdiv(n / 4, 256)), dim3(256), 0, st, dh, h, n / 4, 1.f);
  SF_CHECK_LAUNCH();
  return 0;
}

// ---- differentiable building blocks for the slot-level layers (predictor, kernel distribution; savi.py:190-200,
// predictor.py:47-73): backward of y = act(x W^T + b) and of LayerNorm, on the same kernels as the big nodes ----
namespace {
constexpr size_t LINEAR_BWD_SLACK = 128 * sizeof(float) + 256, LN_BWD_SLACK = 128 * sizeof(float) + 256;
struct LinearBwdWs { float *partial, *wt; size_t bytes; };   // wt: W^T [K,N]
LinearBwdWs linear_bwd_carve(void* ws, long long M, int N, int K) {
  SfArena a(ws);
  float* partial = a.take(sf_grad_partial_floats(M, N, K));
  return LinearBwdWs{partial, a.take((size_t)N * K), a.bytes()};
}
}  // namespace

extern "C" {

size_t sf_linear_bwd_workspace_bytes(long long M, int N, int K) { return linear_bwd_carve(nullptr, M, N, K).bytes + LINEAR_BWD_SLACK; }
// dy [M,N] is overwritten when relu != 0 (masked by y > 0).  dx [M,K] (may be NULL), dW [N,K], db [N] (may be NULL).
int sf_linear_bwd_f32(const float* x, const float* W, const float* y, float* dy, float* dx, float* dW, float* db, long long M,
                      int N, int K, int relu, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(x && W && dy && dW && ws && M > 0, "null pointer");
  SF_REQUIRE(N % 64 == 0 && K % 64 == 0, "linear backward needs multiples of 64");
  SF_REQUIRE(ws_bytes >= sf_linear_bwd_workspace_bytes(M, N, K), "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const LinearBwdWs w = linear_bwd_carve(ws, M, N, K);
  if (relu) {
    SF_REQUIRE(y != nullptr, "relu backward needs the forward output");
    SF_TRY(sf_relu_bwd_ex(dy, y, M * N, st));
  }
  SF_TRY(sf_grad_weight_ex(dy, x, dW, M, N, K, w.partial, st));
  if (db) SF_TRY(sf_grad_bias_ex(dy, db, M, N, w.partial, st));
  if (dx) {
    SF_TRY(sf_transpose_ex(W, w.wt, N, K, st));   // [N,K] -> [K,N]
    SF_TRY(sf_linear_ex(dy, sf_rows(N), w.wt, nullptr, nullptr, nullptr, 0.f, nullptr, sf_rows(K), 0, dx, sf_rows(K), (int)M, K, N, 0, st));
  }
  return 0;
}

// (one buffer: nothing to carve)
size_t sf_layernorm_bwd_workspace_bytes(int D) { return sf_colsum_partial_floats(D) * sizeof(float) + LN_BWD_SLACK; }
int sf_layernorm_bwd_f32(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta, long long rows,
                         int D, float eps, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(x && dy && gamma && dx && dgamma && dbeta && ws && rows > 0, "null pointer");
  SF_REQUIRE(D > 0 && D % 4 == 0 && D <= 1024, "LayerNorm width");   // (before the parameter-gradient launch, which assumes it too)
  SF_REQUIRE(ws_bytes >= sf_layernorm_bwd_workspace_bytes(D), "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* partial = SfArena(ws).take(sf_colsum_partial_floats(D));
  SF_TRY(sf_grad_ln_ex(x, dy, dgamma, dbeta, rows, D, eps, partial, st));
  return sf_ln_bwd_ex(x, dy, gamma, nullptr, dx, rows, D, eps, st);
}

}  // extern "C"

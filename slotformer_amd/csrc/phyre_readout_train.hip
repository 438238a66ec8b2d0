// Training of the PHYRE task-success readout (phyre_planning/models/readout.py: PHYREReadout under autograd, dropout of nn.TransformerEncoderLayer
// included): a pre-LN layer runs forward as ONE launch and its activation-gradient chain backward as ONE launch.
//
//   forward   ph_embed_kernel (phyre_readout.hip) -> pt_layer_fwd_kernel x num_layers -> pt_head_fwd_kernel
//   backward  pt_transpose_kernel (all dY . W operands of all layers, one launch) -> pt_head_bwd_kernel ->
//             pt_layer_bwd_kernel per layer, last to first (each keeps the left operands of its parameter gradients) -> pt_tok_bwd_kernel
//             (d in_proj, d CLS, d enc_t_pe) -> the parameter gradients of ALL layers as three launches over all B L rows: pt_wgrad_kernel
//             (d W = Y^T X of the 4 x num_layers matrices, with the bias column sums), pt_lnparam_kernel (d gamma, d beta), pt_reduce_kernel
//             (every row split, added in ascending order).  num_layers + 2 launches forward and num_layers + 6 backward, whatever the batch.
//
// Work split: a workgroup (four waves) owns ONE sequence of L = 1 + T N <= 96 tokens and carries it through the whole layer.  The residual stream
// lives in LDS as f32 [L][128]; the operand of a product lives there as bf16 hi | lo planes ([16-row tiles][128], 272-byte rows: the 16 rows of a
// ds_read_b128 group start on 16 distinct 16-byte slots).  Every product of the layer, in both directions, is a sum of [L x 128] . [128 x 128] blocks
// (pt_blk128): wave w owns output columns 32 w .. 32 w + 31 of a block for all row tiles, reads its 16 x 32 weight fragment from global memory as f32
// (the layer's weights are 786 KB, L2-resident), splits it once and uses it for every row tile.  Blocks: q | k | v = 3, out_proj = 1, the hidden
// layer in four 128-wide chunks (lin1 chunk -> ReLU -> dropout -> planes -> lin2 partial accumulated in registers) = 4 + 4; backward the same
// count against transposed copies of the weights that the backward call writes into the workspace itself (they change every optimiser step).
// Arithmetic of the blocks: split-bf16 -- x = hi + lo, hi.lo + lo.hi + hi.hi on v_mfma_f32_16x16x32_bf16 with f32 accumulation -- whatever
// sf_set_precision says.  The attention core of a head (L x L x 16, 0.7 % of the layer's products at L = 17) runs in plain f32 on the vector units,
// ascending index order; LayerNorm, softmax, the head and the loss gradient are f32.  Every sum has a fixed order; no atomics on floats.
//
// What the forward keeps per layer (caller's workspace): the input rows, LN1(x), q|k|v, the attention output, the mid residual, LN2(x2), the hidden
// activation behind ReLU and dropout, and the ReLU gates it took (one byte each) -- the backward reads the gates back instead of re-deciding a sign,
// and recomputes only the attention probabilities (from the saved q, k, with the regenerated masks) and the LayerNorm statistics.
//
// Dropout masks: dropout_mask.h, site_seed(seed, 0, layer, site), element index  site 0: ((b 8 + h) L + i) L + j;  sites 1, 3: (b L + tok) 128 + c;
// site 2: (b L + tok) 512 + j  -- train.dropout_keep_mask restates them.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "train_blocks.h"
#include "sf_arena.h"
#include "split_bf16.h"
#include "dropout_mask.h"

namespace {

constexpr int PT_D = 128, PT_NH = 8, PT_HD = 16, PT_FFN = 512, PT_MAXL = 96, PT_MAXLAYERS = 8;
constexpr int PT_THREADS = 256, PT_WAVES = 4;
constexpr int PT_RT = PT_MAXL / 16;          // row tiles of a workgroup at the longest sequence
constexpr int PT_PITCH = (PT_D + 8) * 2;     // bytes of a row of a bf16 plane
constexpr float PT_EPS = 1e-5f;
constexpr int PT_HEAD_SEQ = 8;               // sequences of a head-forward workgroup
constexpr int PT_HEAD_PITCH = PT_D + 1;
constexpr size_t PT_HEAD_LDS = ((size_t)PT_D * PT_HEAD_PITCH + 2 * (size_t)PT_HEAD_SEQ * PT_D) * sizeof(float);
constexpr int PT_TOK_THREADS = 1024;
constexpr int PT_TOK_U = 8;                 // rows a thread of the token backward's column sums has in flight
constexpr int PT_TOK_J = 8;                 // rows of d in_proj.weight a workgroup of the token backward owns
constexpr int PT_TOK_RS = 16;               // its row splits at most

__host__ __device__ inline int pt_rp(int L) { return (L + 15) & ~15; }
__host__ __device__ inline int pt_planes(int L) { return 2 * pt_rp(L) * PT_PITCH; }                    // bytes of a hi | lo plane pair
__host__ __device__ inline int pt_attn_bytes(int L) { return (3 * L * PT_HD + L * L) * 4; }           // q_h | k_h | v_h | P of a head
__host__ __device__ inline int pt_last(int L) { return pt_planes(L) > pt_attn_bytes(L) ? pt_planes(L) : pt_attn_bytes(L); }
// LDS of a layer workgroup, both directions: f32 rows | planes | (planes or the attention staging)
inline size_t pt_lds(int L) { return (size_t)pt_rp(L) * PT_D * 4 + pt_planes(L) + pt_last(L); }

// acc[rt][c] += A[16 rt + row][k] . W[column][k] over k = 0..127: A in planes (hi, lo), W rows `ldw` floats apart in global memory; wave `wid`
// owns the column tiles 2 wid + c.  A operand: lane & 15 = row of the tile, k = 8 (lane >> 4) + 0..7 of a 32-step; B operand: W[column lane & 15]
// [the same k]; accumulator register e of a lane = row 4 (lane >> 4) + e, column lane & 15.
__device__ __forceinline__ void pt_blk128(const char* hi, const char* lo, int rt_n, const float* __restrict__ W, int ldw, int wid, int lane,
                                          f32x4 (&acc)[PT_RT][2]) {
  const int l15 = lane & 15, q = lane >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float* wrow = W + (long long)((wid * 2 + c) * 16 + l15) * ldw + 8 * q;
#pragma unroll
    for (int ks = 0; ks < PT_D / 32; ++ks) {
      bf16x8 wh, wl;
      sf_split8(*reinterpret_cast<const f32x4*>(wrow + ks * 32), *reinterpret_cast<const f32x4*>(wrow + ks * 32 + 4), wh, wl);
#pragma unroll
      for (int rt = 0; rt < PT_RT; ++rt)
        if (rt < rt_n) {
          const int o = (rt * 16 + l15) * PT_PITCH + (ks * 32 + 8 * q) * 2;
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(hi + o), al = *reinterpret_cast<const bf16x8*>(lo + o);
          acc[rt][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wl, acc[rt][c], 0, 0, 0);
          acc[rt][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wh, acc[rt][c], 0, 0, 0);
          acc[rt][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wh, acc[rt][c], 0, 0, 0);
        }
    }
  }
}
__device__ __forceinline__ void pt_zero(f32x4 (&acc)[PT_RT][2]) {
#pragma unroll
  for (int rt = 0; rt < PT_RT; ++rt) acc[rt][0] = acc[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// one element of a plane pair
__device__ __forceinline__ void pt_put(char* hi, char* lo, int r, int c, float v) {
  const __bf16 h = (__bf16)v;
  reinterpret_cast<__bf16*>(hi + r * PT_PITCH)[c] = h;
  reinterpret_cast<__bf16*>(lo + r * PT_PITCH)[c] = (__bf16)(v - (float)h);
}
// two neighbouring elements (c even) of a plane pair
__device__ __forceinline__ void pt_put2(char* hi, char* lo, int r, int c, float a, float b) {
  unsigned h, l;
  pl_split2(a, b, h, l);
  *reinterpret_cast<unsigned*>(hi + r * PT_PITCH + c * 2) = h;
  *reinterpret_cast<unsigned*>(lo + r * PT_PITCH + c * 2) = l;
}
// rows L .. rp - 1 of a plane pair are zero operands
__device__ __forceinline__ void pt_zero_pad(char* hi, char* lo, int L, int rp, int tid) {
  for (int idx = tid; idx < (rp - L) * (PT_D / 2); idx += PT_THREADS) {
    const int r = L + idx / (PT_D / 2), c = (idx % (PT_D / 2)) * 2;
    *reinterpret_cast<unsigned*>(hi + r * PT_PITCH + c * 2) = 0u;
    *reinterpret_cast<unsigned*>(lo + r * PT_PITCH + c * 2) = 0u;
  }
}
// LayerNorm statistics of a row whose elements 2 lane, 2 lane + 1 a lane holds: the one formula both directions use (equal bits)
__device__ __forceinline__ void pt_ln_stats(float a, float b, float& mean, float& rstd) {
  mean = sf_wave_sum(a + b) * (1.f / PT_D);
  const float da = a - mean, db = b - mean;
  const float var = sf_wave_sum(da * da + db * db) * (1.f / PT_D);
  rstd = 1.f / sqrtf(var + PT_EPS);
}
// LayerNorm of the f32 rows in LDS -> planes (rows past L zero) and the saved copy in global memory; a wave per row
__device__ __forceinline__ void pt_ln_rows(const float* xs, int L, int rp, const float* __restrict__ g, const float* __restrict__ be, char* hi, char* lo,
                                           float* __restrict__ out, int wid, int lane) {
  const float g0 = g[2 * lane], g1 = g[2 * lane + 1], b0 = be[2 * lane], b1 = be[2 * lane + 1];
  for (int r = wid; r < rp; r += PT_WAVES) {
    float y0 = 0.f, y1 = 0.f;
    if (r < L) {
      const float a = xs[r * PT_D + 2 * lane], b = xs[r * PT_D + 2 * lane + 1];
      float mean, rstd;
      pt_ln_stats(a, b, mean, rstd);
      y0 = (a - mean) * rstd * g0 + b0;
      y1 = (b - mean) * rstd * g1 + b1;
      *reinterpret_cast<f32x2*>(out + (long long)r * PT_D + 2 * lane) = f32x2{y0, y1};
    }
    pt_put2(hi, lo, r, 2 * lane, y0, y1);
  }
}
// LayerNorm backward of the rows: ds[r] += d LN(x)[r] / d x . dy[r] (dy: f32 rows in LDS; x: the saved input rows); a wave per row
__device__ __forceinline__ void pt_ln_bwd_row(const float* __restrict__ x, const float* dy, float* ds, int r, const float g0, const float g1, int lane) {
  const f32x2 xv = *reinterpret_cast<const f32x2*>(x + (long long)r * PT_D + 2 * lane);
  float mean, rstd;
  pt_ln_stats(xv[0], xv[1], mean, rstd);
  const float h0 = (xv[0] - mean) * rstd, h1 = (xv[1] - mean) * rstd;
  const float e0 = dy[r * PT_D + 2 * lane] * g0, e1 = dy[r * PT_D + 2 * lane + 1] * g1;
  const float c1 = sf_wave_sum(e0 + e1) * (1.f / PT_D);
  const float c2 = sf_wave_sum(e0 * h0 + e1 * h1) * (1.f / PT_D);
  ds[r * PT_D + 2 * lane] += rstd * (e0 - c1 - h0 * c2);
  ds[r * PT_D + 2 * lane + 1] += rstd * (e1 - c1 - h1 * c2);
}

// Head h of the sequence whose q|k|v rows start at `qkv`: q_h, k_h, v_h [L][16] into LDS and P = softmax(q k^T / 4) into S [L][L] -- with `drop`
// the dropped, rescaled probabilities.  s_ij: fma chain over c = 0..15 from zero, then * 0.25; row maximum and row sum as wave reductions over
// (p_lane + p_{lane + 64}).  Both directions call this, so the backward sees the forward's probabilities bit for bit.
__device__ __forceinline__ void pt_attn_probs(const float* __restrict__ qkv, int L, int h, float* qs, float* ks, float* vs, float* S, bool drop,
                                              uint32_t sseed, uint32_t base, uint32_t thresh, float inv_keep, int tid, int lane, int wid) {
  for (int idx = tid; idx < L * 12; idx += PT_THREADS) {
    const int i = idx / 12, rem = idx - i * 12, part = rem >> 2, c4 = rem & 3;
    const f32x4 v = *reinterpret_cast<const f32x4*>(qkv + (long long)i * (3 * PT_D) + part * PT_D + h * PT_HD + c4 * 4);
    float* dst = part == 0 ? qs : part == 1 ? ks : vs;
    *reinterpret_cast<f32x4*>(dst + i * PT_HD + c4 * 4) = v;
  }
  __syncthreads();
  for (int idx = tid; idx < L * L; idx += PT_THREADS) {
    const int i = idx / L, j = idx - i * L;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < PT_HD; ++c) s = fmaf(qs[i * PT_HD + c], ks[j * PT_HD + c], s);
    S[idx] = s * 0.25f;
  }
  __syncthreads();
  for (int i = wid; i < L; i += PT_WAVES) {
    const int j0 = lane, j1 = lane + 64;
    const float v0 = j0 < L ? S[i * L + j0] : -INFINITY, v1 = j1 < L ? S[i * L + j1] : -INFINITY;
    const float m = sf_wave_max(fmaxf(v0, v1));
    const float e0 = j0 < L ? expf(v0 - m) : 0.f, e1 = j1 < L ? expf(v1 - m) : 0.f;
    const float inv = 1.f / sf_wave_sum(e0 + e1);
    float p0 = e0 * inv, p1 = e1 * inv;
    if (drop) {
      p0 = sf_keep(sseed, base + i * L + j0, thresh) ? p0 * inv_keep : 0.f;
      p1 = sf_keep(sseed, base + i * L + j1, thresh) ? p1 * inv_keep : 0.f;
    }
    if (j0 < L) S[i * L + j0] = p0;
    if (j1 < L) S[i * L + j1] = p1;
  }
  __syncthreads();
}

struct PtLayerW {
  const float *n1g, *n1b, *wqkv, *bqkv, *wo, *bo, *n2g, *n2b, *w1, *b1, *w2, *b2;
};
struct PtFwd {
  PtLayerW w;
  const float* x;                            // [B L][128] the layer's input rows
  float* y;                                  // the layer's output rows
  float *xn1, *qkv, *o, *x2, *xn2, *hact;    // kept for the backward
  unsigned char *gate, *gate_out;            // [B L][512] in the workspace; the caller's copy or NULL
  int L;
  uint32_t s0, s1, s2, s3, thresh;
  float inv_keep;
};

__global__ __launch_bounds__(PT_THREADS) void pt_layer_fwd_kernel(const PtFwd a) {
  extern __shared__ __attribute__((aligned(16))) char pt_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int L = a.L, rp = pt_rp(L), rt_n = rp >> 4, b = blockIdx.x;
  const long long row0 = (long long)b * L;
  float* xs = reinterpret_cast<float*>(pt_smem);
  char* pa_hi = pt_smem + rp * PT_D * 4;
  char* pa_lo = pa_hi + rp * PT_PITCH;
  char* pb_hi = pa_hi + pt_planes(L);
  char* pb_lo = pb_hi + rp * PT_PITCH;
  float* qs = reinterpret_cast<float*>(pb_hi);   // the attention staging lies over the second plane pair
  float* ks = qs + L * PT_HD;
  float* vs = ks + L * PT_HD;
  float* S = vs + L * PT_HD;
  const uint32_t thresh = a.thresh;
  const float inv_keep = a.inv_keep;

  for (int idx = tid; idx < L * (PT_D / 4); idx += PT_THREADS)
    reinterpret_cast<f32x4*>(xs)[idx] = reinterpret_cast<const f32x4*>(a.x + row0 * PT_D)[idx];
  __syncthreads();
  pt_ln_rows(xs, L, rp, a.w.n1g, a.w.n1b, pa_hi, pa_lo, a.xn1 + row0 * PT_D, wid, lane);
  __syncthreads();
  f32x4 acc[PT_RT][2];
  // ---- q | k | v ----
  for (int p = 0; p < 3; ++p) {
    pt_zero(acc);
    pt_blk128(pa_hi, pa_lo, rt_n, a.w.wqkv + (long long)p * PT_D * PT_D, PT_D, wid, lane, acc);
#pragma unroll
    for (int rt = 0; rt < PT_RT; ++rt)
      if (rt < rt_n)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int col = p * PT_D + (wid * 2 + c) * 16 + l15;
          const float bias = a.w.bqkv[col];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = rt * 16 + q * 4 + e;
            if (r < L) a.qkv[(row0 + r) * (3 * PT_D) + col] = acc[rt][c][e] + bias;
          }
        }
  }
  __syncthreads();   // (q|k|v of this sequence are read back below by other waves of this workgroup: workgroup-scope release / acquire)
  // ---- the eight heads: P' V into the first plane pair (its LN1 rows are consumed) ----
  for (int h = 0; h < PT_NH; ++h) {
    pt_attn_probs(a.qkv + row0 * (3 * PT_D), L, h, qs, ks, vs, S, thresh != 0, a.s0, (uint32_t)(((long long)b * PT_NH + h) * L * L), thresh, inv_keep,
                  tid, lane, wid);
    for (int idx = tid; idx < L * PT_HD; idx += PT_THREADS) {
      const int i = idx >> 4, c = idx & 15;
      float o = 0.f;
      for (int j = 0; j < L; ++j) o = fmaf(S[i * L + j], vs[j * PT_HD + c], o);
      a.o[(row0 + i) * PT_D + h * PT_HD + c] = o;
      pt_put(pa_hi, pa_lo, i, h * PT_HD + c, o);
    }
    __syncthreads();
  }
  // ---- out_proj, dropout, + x -> x2 (in place in the f32 rows) ----
  pt_zero(acc);
  pt_blk128(pa_hi, pa_lo, rt_n, a.w.wo, PT_D, wid, lane, acc);
#pragma unroll
  for (int rt = 0; rt < PT_RT; ++rt)
    if (rt < rt_n)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = (wid * 2 + c) * 16 + l15;
        const float bias = a.w.bo[col];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = rt * 16 + q * 4 + e;
          if (r < L) {
            float v = acc[rt][c][e] + bias;
            if (thresh) v = sf_keep(a.s1, (uint32_t)((row0 + r) * PT_D + col), thresh) ? v * inv_keep : 0.f;
            const float x2 = xs[r * PT_D + col] + v;
            xs[r * PT_D + col] = x2;
            a.x2[(row0 + r) * PT_D + col] = x2;
          }
        }
      }
  __syncthreads();
  pt_ln_rows(xs, L, rp, a.w.n2g, a.w.n2b, pa_hi, pa_lo, a.xn2 + row0 * PT_D, wid, lane);
  pt_zero_pad(pb_hi, pb_lo, L, rp, tid);   // (the staging of the heads lay here)
  __syncthreads();
  // ---- the hidden layer in four chunks of 128: lin1 -> ReLU (gate recorded) -> dropout -> planes -> lin2 partial ----
  f32x4 acc2[PT_RT][2];
  pt_zero(acc2);
  for (int ch = 0; ch < PT_FFN / PT_D; ++ch) {
    pt_zero(acc);
    pt_blk128(pa_hi, pa_lo, rt_n, a.w.w1 + (long long)ch * PT_D * PT_D, PT_D, wid, lane, acc);
#pragma unroll
    for (int rt = 0; rt < PT_RT; ++rt)
      if (rt < rt_n)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int lc = (wid * 2 + c) * 16 + l15, col = ch * PT_D + lc;
          const float bias = a.w.b1[col];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = rt * 16 + q * 4 + e;
            if (r < L) {
              const float hv = acc[rt][c][e] + bias;
              const bool gate = hv > 0.f;
              const long long gi = (row0 + r) * PT_FFN + col;
              a.gate[gi] = gate ? 1 : 0;
              if (a.gate_out) a.gate_out[gi] = gate ? 1 : 0;
              float v = gate ? hv : 0.f;
              if (thresh) v = sf_keep(a.s2, (uint32_t)gi, thresh) ? v * inv_keep : 0.f;
              a.hact[gi] = v;
              pt_put(pb_hi, pb_lo, r, lc, v);
            }
          }
        }
    __syncthreads();
    pt_blk128(pb_hi, pb_lo, rt_n, a.w.w2 + ch * PT_D, PT_FFN, wid, lane, acc2);
    __syncthreads();
  }
#pragma unroll
  for (int rt = 0; rt < PT_RT; ++rt)
    if (rt < rt_n)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = (wid * 2 + c) * 16 + l15;
        const float bias = a.w.b2[col];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = rt * 16 + q * 4 + e;
          if (r < L) {
            float v = acc2[rt][c][e] + bias;
            if (thresh) v = sf_keep(a.s3, (uint32_t)((row0 + r) * PT_D + col), thresh) ? v * inv_keep : 0.f;
            a.y[(row0 + r) * PT_D + col] = xs[r * PT_D + col] + v;
          }
        }
      }
}

struct PtBwd {
  const float *n1g, *n2g;
  const float *wqkvT, *woT, *w1T, *w2T;   // [128][384], [128][128], [128][512], [512][128]: W^T of the four matrices
  const float *x, *qkv, *x2;              // the forward's rows
  const unsigned char* gate;
  float* dx;                              // in: d loss / d (layer output); out: d loss / d (layer input), in place
  float *dy2, *dh, *dxn2, *do2, *dqkv, *dxn1;   // the left operands of the weight-gradient contractions
  int L;
  uint32_t s0, s1, s2, s3, thresh;
  float inv_keep;
};

__global__ __launch_bounds__(PT_THREADS) void pt_layer_bwd_kernel(const PtBwd a) {
  extern __shared__ __attribute__((aligned(16))) char pt_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  const int L = a.L, rp = pt_rp(L), rt_n = rp >> 4, b = blockIdx.x;
  const long long row0 = (long long)b * L;
  float* ds = reinterpret_cast<float*>(pt_smem);   // the gradient of the residual stream
  char* pb_hi = pt_smem + rp * PT_D * 4;
  char* pb_lo = pb_hi + rp * PT_PITCH;
  float* ts = reinterpret_cast<float*>(pb_hi);     // f32 rows over the second plane pair when it is idle
  char* pa_hi = pb_hi + pt_planes(L);
  char* pa_lo = pa_hi + rp * PT_PITCH;
  float* qs = reinterpret_cast<float*>(pa_hi);     // the attention staging lies over the first plane pair
  float* ks = qs + L * PT_HD;
  float* vs = ks + L * PT_HD;
  float* S = vs + L * PT_HD;
  const uint32_t thresh = a.thresh;
  const float inv_keep = a.inv_keep;

  // ---- d y2 = dropout'(d out) ----
  for (int idx = tid; idx < L * (PT_D / 4); idx += PT_THREADS) {
    const f32x4 v = reinterpret_cast<const f32x4*>(a.dx + row0 * PT_D)[idx];
    reinterpret_cast<f32x4*>(ds)[idx] = v;
    f32x4 d = v;
    if (thresh) {
      const uint32_t e = (uint32_t)(row0 * PT_D + 4 * idx);
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = sf_keep(a.s3, e + k, thresh) ? v[k] * inv_keep : 0.f;
    }
    reinterpret_cast<f32x4*>(a.dy2 + row0 * PT_D)[idx] = d;
    const int r = idx >> 5, c = (idx & 31) * 4;
    sf_split4(reinterpret_cast<__bf16*>(pa_hi + r * PT_PITCH), reinterpret_cast<__bf16*>(pa_lo + r * PT_PITCH), c, d);
  }
  pt_zero_pad(pa_hi, pa_lo, L, rp, tid);
  pt_zero_pad(pb_hi, pb_lo, L, rp, tid);
  __syncthreads();
  // ---- the hidden layer backwards, chunk by chunk: d h = gate . dropout'(d y2 . W2), d xn2 += d h . W1 ----
  f32x4 acc[PT_RT][2], acc2[PT_RT][2];
  pt_zero(acc2);
  for (int ch = 0; ch < PT_FFN / PT_D; ++ch) {
    pt_zero(acc);
    pt_blk128(pa_hi, pa_lo, rt_n, a.w2T + (long long)ch * PT_D * PT_D, PT_D, wid, lane, acc);
#pragma unroll
    for (int rt = 0; rt < PT_RT; ++rt)
      if (rt < rt_n)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int lc = (wid * 2 + c) * 16 + l15, col = ch * PT_D + lc;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = rt * 16 + q * 4 + e;
            if (r < L) {
              const long long gi = (row0 + r) * PT_FFN + col;
              float v = a.gate[gi] ? acc[rt][c][e] : 0.f;
              if (thresh) v = sf_keep(a.s2, (uint32_t)gi, thresh) ? v * inv_keep : 0.f;
              a.dh[gi] = v;
              pt_put(pb_hi, pb_lo, r, lc, v);
            }
          }
        }
    __syncthreads();
    pt_blk128(pb_hi, pb_lo, rt_n, a.w1T + ch * PT_D, PT_FFN, wid, lane, acc2);
    __syncthreads();
  }
#pragma unroll
  for (int rt = 0; rt < PT_RT; ++rt)
    if (rt < rt_n)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = (wid * 2 + c) * 16 + l15;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = rt * 16 + q * 4 + e;
          if (r < L) {
            a.dxn2[(row0 + r) * PT_D + col] = acc2[rt][c][e];
            ts[r * PT_D + col] = acc2[rt][c][e];
          }
        }
      }
  __syncthreads();
  // ---- LayerNorm 2 backwards into the residual gradient; d (out_proj output) = dropout'(d x2) ----
  {
    const float g0 = a.n2g[2 * lane], g1 = a.n2g[2 * lane + 1];
    for (int r = wid; r < L; r += PT_WAVES) {
      pt_ln_bwd_row(a.x2 + row0 * PT_D, ts, ds, r, g0, g1, lane);
      float d0 = ds[r * PT_D + 2 * lane], d1 = ds[r * PT_D + 2 * lane + 1];
      if (thresh) {
        const uint32_t e = (uint32_t)((row0 + r) * PT_D + 2 * lane);
        d0 = sf_keep(a.s1, e, thresh) ? d0 * inv_keep : 0.f;
        d1 = sf_keep(a.s1, e + 1, thresh) ? d1 * inv_keep : 0.f;
      }
      *reinterpret_cast<f32x2*>(a.do2 + (row0 + r) * PT_D + 2 * lane) = f32x2{d0, d1};
      pt_put2(pa_hi, pa_lo, r, 2 * lane, d0, d1);
    }
  }
  __syncthreads();
  // ---- d (attention output) = d o2 . Wo, as f32 rows ----
  pt_zero(acc);
  pt_blk128(pa_hi, pa_lo, rt_n, a.woT, PT_D, wid, lane, acc);
#pragma unroll
  for (int rt = 0; rt < PT_RT; ++rt)
    if (rt < rt_n)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = (wid * 2 + c) * 16 + l15;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = rt * 16 + q * 4 + e;
          if (r < L) ts[r * PT_D + col] = acc[rt][c][e];
        }
      }
  __syncthreads();
  // ---- the eight heads backwards (plain f32, ascending index order) ----
  float* dqkv = a.dqkv + row0 * (3 * PT_D);
  for (int h = 0; h < PT_NH; ++h) {
    const uint32_t base = (uint32_t)(((long long)b * PT_NH + h) * L * L);
    pt_attn_probs(a.qkv + row0 * (3 * PT_D), L, h, qs, ks, vs, S, false, a.s0, base, thresh, inv_keep, tid, lane, wid);
    // d v_j = sum_i P'_ij d o_i
    for (int idx = tid; idx < L * PT_HD; idx += PT_THREADS) {
      const int j = idx >> 4, c = idx & 15;
      float s = 0.f;
      for (int i = 0; i < L; ++i) {
        float p = S[i * L + j];
        if (thresh) p = sf_keep(a.s0, base + i * L + j, thresh) ? p * inv_keep : 0.f;
        s = fmaf(p, ts[i * PT_D + h * PT_HD + c], s);
      }
      dqkv[(long long)j * (3 * PT_D) + 2 * PT_D + h * PT_HD + c] = s;
    }
    __syncthreads();
    // d S_ij = P_ij (d P_ij - sum_j d P_ij P_ij),  d P = dropout'(d o_i . v_j)   (over P, a wave per row)
    for (int i = wid; i < L; i += PT_WAVES) {
      float dp[2], p[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        dp[k] = p[k] = 0.f;
        if (j < L) {
          float s = 0.f;
#pragma unroll
          for (int c = 0; c < PT_HD; ++c) s = fmaf(ts[i * PT_D + h * PT_HD + c], vs[j * PT_HD + c], s);
          if (thresh) s = sf_keep(a.s0, base + i * L + j, thresh) ? s * inv_keep : 0.f;
          dp[k] = s;
          p[k] = S[i * L + j];
        }
      }
      const float dot = sf_wave_sum(dp[0] * p[0] + dp[1] * p[1]);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int j = lane + 64 * k;
        if (j < L) S[i * L + j] = p[k] * (dp[k] - dot);
      }
    }
    __syncthreads();
    // d q_i = sum_j d S_ij k_j / 4,  d k_j = sum_i d S_ij q_i / 4
    for (int idx = tid; idx < 2 * L * PT_HD; idx += PT_THREADS) {
      const int which = idx >= L * PT_HD, rem = idx - which * L * PT_HD, r = rem >> 4, c = rem & 15;
      float s = 0.f;
      if (!which)
        for (int j = 0; j < L; ++j) s = fmaf(S[r * L + j], ks[j * PT_HD + c], s);
      else
        for (int i = 0; i < L; ++i) s = fmaf(S[i * L + r], qs[i * PT_HD + c], s);
      dqkv[(long long)r * (3 * PT_D) + which * PT_D + h * PT_HD + c] = s * 0.25f;
    }
    __syncthreads();
  }
  // ---- d xn1 = d q . Wq + d k . Wk + d v . Wv: the three parts through the first plane pair (read back from this workgroup's own rows) ----
  pt_zero(acc2);
  for (int p = 0; p < 3; ++p) {
    for (int idx = tid; idx < L * (PT_D / 4); idx += PT_THREADS) {
      const int r = idx >> 5, c = (idx & 31) * 4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(dqkv + (long long)r * (3 * PT_D) + p * PT_D + c);
      sf_split4(reinterpret_cast<__bf16*>(pa_hi + r * PT_PITCH), reinterpret_cast<__bf16*>(pa_lo + r * PT_PITCH), c, v);
    }
    if (p == 0) pt_zero_pad(pa_hi, pa_lo, L, rp, tid);   // (the staging of the heads lay here)
    __syncthreads();
    pt_blk128(pa_hi, pa_lo, rt_n, a.wqkvT + p * PT_D, 3 * PT_D, wid, lane, acc2);
    __syncthreads();
  }
#pragma unroll
  for (int rt = 0; rt < PT_RT; ++rt)
    if (rt < rt_n)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = (wid * 2 + c) * 16 + l15;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = rt * 16 + q * 4 + e;
          if (r < L) {
            a.dxn1[(row0 + r) * PT_D + col] = acc2[rt][c][e];
            ts[r * PT_D + col] = acc2[rt][c][e];
          }
        }
      }
  __syncthreads();
  // ---- LayerNorm 1 backwards; the residual gradient leaves as d loss / d (layer input) ----
  {
    const float g0 = a.n1g[2 * lane], g1 = a.n1g[2 * lane + 1];
    for (int r = wid; r < L; r += PT_WAVES) {
      pt_ln_bwd_row(a.x + row0 * PT_D, ts, ds, r, g0, g1, lane);
      *reinterpret_cast<f32x2*>(a.dx + (row0 + r) * PT_D + 2 * lane) = f32x2{ds[r * PT_D + 2 * lane], ds[r * PT_D + 2 * lane + 1]};
    }
  }
}

// The head on row 0 of every sequence, plain f32.  Summation order: hidden unit j of a sequence is h_j = fma chain over k = 0..127 ascending starting
// from b1[j]; the gate is h_j > 0; p_j = relu(h_j) * w2[j]; the logit is the sum over j taken as (p_lane + p_{lane + 64}) per lane, then
// sf_wave_sum over the 64 lanes, + b2 last (ph_head_kernel's order).  A sequence's logit does not depend on its place in the batch.
__global__ __launch_bounds__(PT_D) void pt_head_fwd_kernel(const float* __restrict__ x, int L, const float* __restrict__ W1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ logits,
                                                           float* __restrict__ hrelu, unsigned char* __restrict__ gate, unsigned char* __restrict__ gate_out,
                                                           int B) {
  extern __shared__ __attribute__((aligned(16))) char pt_smem[];
  float* wt = reinterpret_cast<float*>(pt_smem);   // [k][PT_HEAD_PITCH]: W1^T
  float* xs = wt + PT_D * PT_HEAD_PITCH;           // [PT_HEAD_SEQ][128]
  float* pp = xs + PT_HEAD_SEQ * PT_D;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s0 = blockIdx.x * PT_HEAD_SEQ, ns = B - s0 < PT_HEAD_SEQ ? B - s0 : PT_HEAD_SEQ;
  for (int idx = tid; idx < PT_D * PT_D; idx += PT_D) wt[(idx & 127) * PT_HEAD_PITCH + (idx >> 7)] = W1[idx];
  for (int idx = tid; idx < PT_HEAD_SEQ * PT_D; idx += PT_D) {
    const int s = idx >> 7;
    xs[idx] = s < ns ? x[(long long)(s0 + s) * L * PT_D + (idx & 127)] : 0.f;
  }
  __syncthreads();
  {
    const int j = tid;
    float h[PT_HEAD_SEQ];
    const float bj = b1[j], wj = w2[j];
#pragma unroll
    for (int s = 0; s < PT_HEAD_SEQ; ++s) h[s] = bj;
    for (int k = 0; k < PT_D; ++k) {
      const float w = wt[k * PT_HEAD_PITCH + j];
#pragma unroll
      for (int s = 0; s < PT_HEAD_SEQ; ++s) h[s] = fmaf(w, xs[s * PT_D + k], h[s]);
    }
#pragma unroll
    for (int s = 0; s < PT_HEAD_SEQ; ++s) {
      const bool g = h[s] > 0.f;
      const float r = g ? h[s] : 0.f;
      pp[s * PT_D + j] = r * wj;
      if (s < ns) {
        const long long at = (long long)(s0 + s) * PT_D + j;
        hrelu[at] = r;
        gate[at] = g ? 1 : 0;
        if (gate_out) gate_out[at] = g ? 1 : 0;
      }
    }
  }
  __syncthreads();
  const float bias2 = b2[0];
  for (int s = wid; s < PT_HEAD_SEQ; s += 2) {   // (whole waves: sequences past the end are computed and dropped)
    const float logit = sf_wave_sum(pp[s * PT_D + lane] + pp[s * PT_D + 64 + lane]) + bias2;
    if (lane == 0 && s < ns) logits[s0 + s] = logit;
  }
}

// The head backwards in one launch.  Workgroup j < 128: row j of d W1 (thread k: sum over b ascending of d h[b][j] x[b, 0][k]), d b1[j], d w2[j];
// workgroup 0 also d b2.  Workgroup 128 + b: d x[b, 0][k] = sum over j ascending of d h[b][j] W1[j][k], and zeros for the other rows of sequence b
// (the loss reads row 0 only).  d h[b][j] = gate[b][j] ? g[b] w2[j] : 0.
__global__ __launch_bounds__(PT_D) void pt_head_bwd_kernel(const float* __restrict__ x, int L, const float* __restrict__ W1, const float* __restrict__ w2,
                                                           const float* __restrict__ g, const float* __restrict__ hrelu,
                                                           const unsigned char* __restrict__ gate, float* __restrict__ dW1, float* __restrict__ db1,
                                                           float* __restrict__ dw2, float* __restrict__ db2, float* __restrict__ dx, int B) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < PT_D) {
    const int j = blockIdx.x;
    const float wj = w2[j];
    float s = 0.f, sb = 0.f, sw = 0.f, sg = 0.f;
    for (int b = 0; b < B; ++b) {
      const float gb = g[b], dh = gate[(long long)b * PT_D + j] ? gb * wj : 0.f;
      s = fmaf(dh, x[(long long)b * L * PT_D + tid], s);
      sb += dh;
      sw = fmaf(gb, hrelu[(long long)b * PT_D + j], sw);
      sg += gb;
    }
    dW1[j * PT_D + tid] = s;
    if (tid == 0) {
      db1[j] = sb;
      dw2[j] = sw;
      if (j == 0) db2[0] = sg;
    }
    return;
  }
  const int b = blockIdx.x - PT_D;
  const float gb = g[b];
  float s = 0.f;
  for (int j = 0; j < PT_D; ++j) {
    const float dh = gate[(long long)b * PT_D + j] ? gb * w2[j] : 0.f;
    s = fmaf(dh, W1[j * PT_D + tid], s);
  }
  float* row = dx + (long long)b * L * PT_D;
  row[tid] = s;
  for (int idx = tid; idx < (L - 1) * PT_D; idx += PT_D) row[PT_D + idx] = 0.f;
}

struct PtSel {
  int v[PT_MAXL];
};
struct PtTok {
  const float* slots;
  long long stride_v, stride_t;
  int V;
  const int* video_index;
  const float* dx;                 // [B][L][128] d loss / d (token rows)
  float *dWp, *db, *dcls, *dpe;    // partial [RS][128][C] of d in_proj.weight; [128], [128], [T][128] or NULL
  int B, T, N, C;
};
// The token rows backwards in one launch of 1024-thread workgroups; every sum is taken over strided row groups in ascending order and the groups
// are added in ascending order.  The first 16 RS workgroups give d in_proj.weight: workgroup (jt, rs) owns rows 8 jt .. 8 jt + 7 of the matrix and
// row split rs -- thread (g, c), G = 1024 / C groups, walks the slot rows rs G + g, + RS G, ... (read in place; rows of a frame sel[t] == -1
// contribute nothing), one slot element against eight d x columns per row, and writes partial[rs][128][C], which pt_reduce_kernel adds over rs.
// Then one workgroup each: d in_proj.bias over ALL slot-token rows; d CLS = sum over b of d x[b, 0]; d enc_t_pe[t] = sum over (b, n) of
// d x[b, 1 + t N + n]   (eight groups of 128 threads).
__global__ __launch_bounds__(PT_TOK_THREADS) void pt_tok_bwd_kernel(const PtTok a, const PtSel sel, int RS) {
  __shared__ float red[PT_TOK_J * PT_TOK_THREADS];
  const int tid = threadIdx.x, T = a.T, N = a.N, C = a.C, TN = T * N, L = 1 + TN, B = a.B;
  const long long rows = (long long)B * TN;
  const int ntiles = (PT_D / PT_TOK_J) * RS;
  if ((int)blockIdx.x < ntiles) {
    const int jt = (int)blockIdx.x % (PT_D / PT_TOK_J), rs = (int)blockIdx.x / (PT_D / PT_TOK_J);
    const int G = PT_TOK_THREADS / C, g = tid / C, c = tid - g * C;
    float acc[PT_TOK_J];
#pragma unroll
    for (int k = 0; k < PT_TOK_J; ++k) acc[k] = 0.f;
    if (g < G)
      for (long long r = (long long)rs * G + g; r < rows; r += (long long)RS * G) {
        const int b = (int)(r / TN), rem = (int)(r - (long long)b * TN), t = rem / N, n = rem - t * N;
        const int f = sel.v[t], vid = a.video_index ? a.video_index[b] : b;
        if (f >= 0 && vid >= 0 && vid < a.V) {
          const float sv = a.slots[(long long)vid * a.stride_v + (long long)f * a.stride_t + n * C + c];
          const float* d = a.dx + ((long long)b * L + 1 + rem) * PT_D + jt * PT_TOK_J;
          const f32x4 d0 = *reinterpret_cast<const f32x4*>(d), d1 = *reinterpret_cast<const f32x4*>(d + 4);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            acc[k] = fmaf(d0[k], sv, acc[k]);
            acc[4 + k] = fmaf(d1[k], sv, acc[4 + k]);
          }
        }
      }
#pragma unroll
    for (int k = 0; k < PT_TOK_J; ++k) red[k * PT_TOK_THREADS + tid] = acc[k];
    __syncthreads();
    if (tid < C)
#pragma unroll
      for (int k = 0; k < PT_TOK_J; ++k) {
        float t = red[k * PT_TOK_THREADS + tid];
        for (int q = 1; q < G; ++q) t += red[k * PT_TOK_THREADS + q * C + tid];
        a.dWp[((long long)rs * PT_D + jt * PT_TOK_J + k) * C + tid] = t;
      }
    return;
  }
  const int job = blockIdx.x - ntiles, j = tid & 127, g = tid >> 7;
  float s = 0.f;
  // element i = g, g + 8, ... of the job's list of rows, PT_TOK_U loads in flight, added in list order
  const long long count = job == 0 ? rows : job == 1 ? (long long)B : (long long)B * N;
  for (long long i0 = g; i0 < count; i0 += 8LL * PT_TOK_U) {
    float v[PT_TOK_U];
#pragma unroll
    for (int u = 0; u < PT_TOK_U; ++u) {
      const long long i = i0 + 8LL * u;
      v[u] = 0.f;
      if (i < count) {
        long long row;
        if (job == 0) {
          const long long b = i / TN;
          row = b * L + 1 + (i - b * TN);
        } else if (job == 1) {
          row = i * L;
        } else {
          const long long b = i / N;
          row = b * L + 1 + (long long)(job - 2) * N + (i - b * N);
        }
        v[u] = a.dx[row * PT_D + j];
      }
    }
#pragma unroll
    for (int u = 0; u < PT_TOK_U; ++u) s += v[u];
  }
  red[tid] = s;
  __syncthreads();
  if (tid < PT_D) {
    float t = red[tid];
    for (int k = 1; k < 8; ++k) t += red[k * PT_D + tid];
    float* dst = job == 0 ? a.db : job == 1 ? a.dcls : a.dpe + (long long)(job - 2) * PT_D;
    dst[tid] = t;
  }
}

// ---- the parameter gradients of ALL layers: three launches ------------------------------------------------------------------------------------
// d W = Y^T X over the B L rows for the four matrices of every layer (16 x up to 8 jobs) in ONE launch: blockIdx.z = the job, blockIdx.x = its
// 64 x 64 output tile, blockIdx.y = the row split.  A chunk of 32 rows of both operands is staged TRANSPOSED in LDS as bf16 hi | lo planes
// ([column][row], 80-byte rows), so that a lane's eight consecutive contraction indices are one 16-byte read; a wave owns a 32 x 32 quadrant
// (2 x 2 tiles of v_mfma_f32_16x16x32_bf16, three products each).  Split s handles rows [s rps, (s + 1) rps) in ascending order and writes
// partial[s][N][K]; the workgroups of k-tile 0 also sum their 64 columns of Y over the same rows (plain f32, ascending): the bias gradient.
// pt_reduce_kernel adds the splits in ascending order.  Fixed orders throughout, no atomics.
struct PtWg {
  const float *Y, *X;   // [rows][N], [rows][K]
  int N, K;
  long long poff, boff;   // where this job's [S][N][K] and [S][N] partials start (floats)
};
struct PtWgJobs {
  PtWg j[4 * PT_MAXLAYERS];
};
constexpr int PT_WG_PITCH = 80;   // bytes of a row of a transposed plane: 32 bf16 + 8
__global__ __launch_bounds__(256) void pt_wgrad_kernel(const PtWgJobs jobs, float* __restrict__ partial, long long M, int rps) {
  __shared__ __attribute__((aligned(16))) char sm[4 * 64 * PT_WG_PITCH];
  const PtWg jb = jobs.j[blockIdx.z];
  const int N = jb.N, K = jb.K, tk = K / 64;
  if ((int)blockIdx.x >= (N / 64) * tk) return;
  const int n0 = ((int)blockIdx.x / tk) * 64, k0 = ((int)blockIdx.x % tk) * 64;
  const long long r0 = (long long)blockIdx.y * rps, r1 = r0 + rps < M ? r0 + rps : M;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l15 = lane & 15, q = lane >> 4;
  const int wn = (wid >> 1) * 32, wk = (wid & 1) * 32;
  char *yh = sm, *yl = sm + 64 * PT_WG_PITCH, *xh = sm + 2 * 64 * PT_WG_PITCH, *xl = sm + 3 * 64 * PT_WG_PITCH;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const bool bias = k0 == 0 && tid < 64;
  for (long long rb = r0; rb < r1; rb += 32) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + 256 * u, row = idx >> 4, c = (idx & 15) * 4;
      f32x4 y = {0.f, 0.f, 0.f, 0.f}, x = {0.f, 0.f, 0.f, 0.f};
      if (rb + row < r1) {
        y = *reinterpret_cast<const f32x4*>(jb.Y + (rb + row) * N + n0 + c);
        x = *reinterpret_cast<const f32x4*>(jb.X + (rb + row) * K + k0 + c);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const __bf16 a = (__bf16)y[e], b = (__bf16)x[e];
        reinterpret_cast<__bf16*>(yh + (c + e) * PT_WG_PITCH)[row] = a;
        reinterpret_cast<__bf16*>(yl + (c + e) * PT_WG_PITCH)[row] = (__bf16)(y[e] - (float)a);
        reinterpret_cast<__bf16*>(xh + (c + e) * PT_WG_PITCH)[row] = b;
        reinterpret_cast<__bf16*>(xl + (c + e) * PT_WG_PITCH)[row] = (__bf16)(x[e] - (float)b);
      }
    }
    if (bias)
      for (int m = 0; m < 32 && rb + m < r1; ++m) bsum += jb.Y[(rb + m) * N + n0 + tid];
    __syncthreads();
    bf16x8 ah[2], al[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = (wn + i * 16 + l15) * PT_WG_PITCH + q * 16;
      ah[i] = *reinterpret_cast<const bf16x8*>(yh + o);
      al[i] = *reinterpret_cast<const bf16x8*>(yl + o);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = (wk + j * 16 + l15) * PT_WG_PITCH + q * 16;
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(xh + o), bl = *reinterpret_cast<const bf16x8*>(xl + o);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
      }
    }
  }
  float* dst = partial + jb.poff + (long long)blockIdx.y * N * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[(long long)(n0 + wn + i * 16 + q * 4 + e) * K + k0 + wk + j * 16 + l15] = acc[i][j][e];
  if (bias) partial[jb.boff + (long long)blockIdx.y * N + n0 + tid] = bsum;
}

// d gamma = sum over rows of dy . xhat, d beta = sum over rows of dy, for both LayerNorms of every layer in ONE launch: blockIdx.y = the job,
// blockIdx.x = a group of rpg rows; wave w takes rows w, w + 4, ... of the group (ascending), the four waves are added in order
// -> partial[job][group][gamma | beta][128].  The statistics are pt_ln_stats, the formula of the forward.
struct PtLn {
  const float *x, *dy;
};
struct PtLnJobs {
  PtLn j[2 * PT_MAXLAYERS];
};
__global__ __launch_bounds__(256) void pt_lnparam_kernel(const PtLnJobs jobs, float* __restrict__ partial, long long M, int rpg) {
  __shared__ float red[PT_WAVES][4][64];
  const PtLn jb = jobs.j[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long r0 = (long long)blockIdx.x * rpg, r1 = r0 + rpg < M ? r0 + rpg : M;
  float ag0 = 0.f, ag1 = 0.f, ab0 = 0.f, ab1 = 0.f;
  for (long long r = r0 + wid; r < r1; r += PT_WAVES) {
    const f32x2 xv = *reinterpret_cast<const f32x2*>(jb.x + r * PT_D + 2 * lane), dv = *reinterpret_cast<const f32x2*>(jb.dy + r * PT_D + 2 * lane);
    float mean, rstd;
    pt_ln_stats(xv[0], xv[1], mean, rstd);
    ag0 = fmaf(dv[0], (xv[0] - mean) * rstd, ag0);
    ag1 = fmaf(dv[1], (xv[1] - mean) * rstd, ag1);
    ab0 += dv[0];
    ab1 += dv[1];
  }
  red[wid][0][lane] = ag0; red[wid][1][lane] = ag1; red[wid][2][lane] = ab0; red[wid][3][lane] = ab1;
  __syncthreads();
  if (wid == 0) {
    float* dst = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2 * PT_D;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[(k >> 1) * PT_D + 2 * lane + (k & 1)] = ((red[0][k][lane] + red[1][k][lane]) + red[2][k][lane]) + red[3][k][lane];
  }
}

// dst[i] = sum over s = 0..S-1 (ascending) of src[s stride + i], i < n, for every job (blockIdx.y) in ONE launch
struct PtRed {
  const float* src;
  float* dst;
  long long stride;
  int S, n;
};
struct PtRedJobs {
  PtRed j[12 * PT_MAXLAYERS + 1];
};
__global__ __launch_bounds__(256) void pt_reduce_kernel(const PtRedJobs jobs) {
  const PtRed jb = jobs.j[blockIdx.y];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < jb.n; i += gridDim.x * 256) {
    float s = jb.src[i];
    for (int k = 1; k < jb.S; ++k) s += jb.src[k * jb.stride + i];
    jb.dst[i] = s;
  }
}

// dst [C][R] = src [R][C]^T for up to 4 x 8 matrices in one launch (R, C multiples of 32): blockIdx.y = the matrix, blockIdx.x = its 32 x 32 tile
struct PtTrJob {
  const float* src;
  float* dst;
  int R, C;
};
struct PtTrJobs {
  PtTrJob j[4 * PT_MAXLAYERS];
};
__global__ __launch_bounds__(256) void pt_transpose_kernel(const PtTrJobs jobs) {
  __shared__ float tile[32][33];
  const PtTrJob jb = jobs.j[blockIdx.y];
  const int tc = jb.C / 32, tiles = (jb.R / 32) * tc;
  if ((int)blockIdx.x >= tiles) return;
  const int r0 = ((int)blockIdx.x / tc) * 32, c0 = ((int)blockIdx.x % tc) * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) tile[k][tx] = jb.src[(long long)(r0 + k) * jb.C + c0 + tx];
  __syncthreads();
  for (int k = ty; k < 32; k += 8) jb.dst[(long long)(c0 + k) * jb.R + r0 + tx] = tile[tx][k];
}

inline bool pt_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the workspace, in floats from the caller's (16-byte aligned) ws: offsets, so the arena below only ever counts
struct PtWs {
  size_t X, xn1, qkv, o, x2, xn2, hact, gate, hrelu, hgate, dx, dy2, dh, dxn2, do2, dqkv, dxn1, wT, partial, tokp, total;
  size_t M;   // rows B L
};
constexpr size_t PT_WT = (size_t)4 * PT_D * PT_D + 2 * (size_t)PT_D * PT_FFN;   // floats of a layer's four matrices
constexpr size_t PT_BIAS = 3 * PT_D + PT_D + PT_FFN + PT_D;                      // ... of its four biases
inline int pt_splits(long long M) { const long long s = (M + 511) / 512; return (int)(s < 1 ? 1 : s > 16 ? 16 : s); }        // row splits of d W
inline int pt_ln_groups(long long M) { const long long g = (M + 63) / 64; return (int)(g < 1 ? 1 : g > 64 ? 64 : g); }      // row groups of d gamma
inline PtWs pt_ws(int B, int L, int nl) {
  PtWs w;
  SfArena a(nullptr);
  const size_t M = (size_t)B * L;
  auto take = [&](size_t n) { const size_t at = a.bytes() / sizeof(float); a.take(n); return at; };
  w.M = M;
  w.X = take((size_t)(nl + 1) * M * PT_D);
  w.xn1 = take(nl * M * PT_D);
  w.qkv = take(nl * M * 3 * PT_D);
  w.o = take(nl * M * PT_D);
  w.x2 = take(nl * M * PT_D);
  w.xn2 = take(nl * M * PT_D);
  w.hact = take(nl * M * PT_FFN);
  w.gate = take(nl * M * PT_FFN / 4);   // bytes
  w.hrelu = take((size_t)B * PT_D);
  w.hgate = take((size_t)B * PT_D / 4);   // bytes
  w.dx = take(M * PT_D);
  // the left operands of the parameter-gradient contractions, kept per layer: the contractions of all layers run behind the last layer kernel
  w.dy2 = take(nl * M * PT_D);
  w.dh = take(nl * M * PT_FFN);
  w.dxn2 = take(nl * M * PT_D);
  w.do2 = take(nl * M * PT_D);
  w.dqkv = take(nl * M * 3 * PT_D);
  w.dxn1 = take(nl * M * PT_D);
  w.wT = take(nl * PT_WT);
  w.partial = take((size_t)pt_splits((long long)M) * nl * (PT_WT + PT_BIAS) + (size_t)2 * nl * pt_ln_groups((long long)M) * 2 * PT_D);
  w.tokp = take((size_t)PT_TOK_RS * PT_D * 256);   // d in_proj.weight per row split, at the widest slot
  w.total = a.bytes() / sizeof(float);
  return w;
}
inline int pt_tok_splits(long long rows) { const long long s = rows / 256; return (int)(s < 1 ? 1 : s > PT_TOK_RS ? PT_TOK_RS : s); }

inline bool pt_model_ok(const sf_phyre_readout_model* m, int T) {
  return m && T >= 1 && T <= PT_MAXL && sf_phyre_readout_ok(m->num_slots, m->slot_size, T, m->d_model, m->num_heads, m->ffn_dim, m->num_layers) == 1;
}

#define PT_LIMITS "1 <= num_slots <= 16, slot_size a multiple of 32 in [32, 256], T >= 1, 1 + T * num_slots <= 96, (d_model, heads, ffn) = (128, 8, 512), 1 <= num_layers <= 8"

// everything both calls check, before any launch
int pt_check(const char* who, const sf_phyre_readout_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all,
             const int* video_index, const int* sel, int B, int T, float dropout_p, const void* ws, size_t ws_bytes) {
  static thread_local char msg[256];
  auto fail = [&](const char* what) {
    snprintf(msg, sizeof msg, "invalid argument: %s: %s", who, what);
    return sf_set_err(-1, msg, __FILE__, __LINE__);
  };
  if (!m || !slots || !sel || !ws) return fail("null pointer");
  if (!pt_model_ok(m, T)) return fail("unsupported shape (" PT_LIMITS ")");
  if (!m->in_proj_w || !m->in_proj_b || !m->enc_t_pe || !m->cls || !m->layers || !m->mlp_w1 || !m->mlp_b1 || !m->mlp_w2 || !m->mlp_b2)
    return fail("null pointer in the model");
  if (B < 1 || V < 1 || T_all < 1) return fail("B >= 1, V >= 1, T_all >= 1");
  if ((long long)B * (1 + T * m->num_slots) * PT_FFN >= (1LL << 32)) return fail("batch too large: B * L * 512 must stay below 2^32 (the mask index)");
  const int N = m->num_slots, C = m->slot_size;
  if (!(stride_t >= (long long)N * C && stride_t % 4 == 0 && stride_v >= 0 && stride_v % 4 == 0)) return fail("frame stride >= N * C, strides multiples of 4");
  if (!video_index && B > V) return fail("B > V without a video_index");
  for (int t = 0; t < T; ++t)
    if (sel[t] < -1 || sel[t] >= T_all) return fail("sel[t] must lie in [-1, T_all) (-1: a frame of zeros)");
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail("dropout_p must lie in [0, 1)");
  for (int l = 0; l < m->num_layers; ++l) {
    const sf_tfm_layer& y = m->layers[l];
    if (!y.norm1_g || !y.norm1_b || !y.in_proj_w || !y.in_proj_b || !y.out_proj_w || !y.out_proj_b || !y.norm2_g || !y.norm2_b || !y.lin1_w || !y.lin1_b ||
        !y.lin2_w || !y.lin2_b)
      return fail("null pointer in a layer");
    if (!pt_al16(y.in_proj_w) || !pt_al16(y.out_proj_w) || !pt_al16(y.lin1_w) || !pt_al16(y.lin2_w) || !pt_al16(y.norm1_g) || !pt_al16(y.norm2_g))
      return fail("the layers' matrices must be 16-byte aligned");
  }
  if (!pt_al16(slots) || !pt_al16(m->in_proj_w) || !pt_al16(m->cls) || !pt_al16(ws)) return fail("slots, in_proj_w, cls and the workspace must be 16-byte aligned");
  if (ws_bytes < sf_phyre_readout_train_workspace_bytes(m, B, T)) return fail("workspace too small");
  if (sf_get_precision() != 1) return fail("split-bf16 mode only (the layers have no other form)");
  return 0;
}

}  // namespace

extern "C" {

size_t sf_phyre_readout_train_workspace_bytes(const sf_phyre_readout_model* m, int B, int T) {
  if (!pt_model_ok(m, T) || B < 1) return 0;
  return pt_ws(B, 1 + T * m->num_slots, m->num_layers).total * sizeof(float);
}

int sf_phyre_readout_train_fwd_f32(const sf_phyre_readout_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all,
                                   const int* video_index, const int* sel, int B, int T, float dropout_p, unsigned long long seed, float* logits,
                                   unsigned char* gates, unsigned char* head_gates, void* ws, size_t ws_bytes, void* stream) {
  SF_TRY(pt_check("sf_phyre_readout_train_fwd_f32", m, slots, stride_v, stride_t, V, T_all, video_index, sel, B, T, dropout_p, ws, ws_bytes));
  SF_REQUIRE(logits != nullptr, "sf_phyre_readout_train_fwd_f32: null pointer");
  const int N = m->num_slots, C = m->slot_size, L = 1 + T * N, nl = m->num_layers;
  const PtWs w = pt_ws(B, L, nl);
  float* f = static_cast<float*>(ws);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = pt_lds(L);
  SF_TRY(sf_ensure_dyn_lds((const void*)pt_layer_fwd_kernel, lds));
  SF_TRY(sf_ensure_dyn_lds((const void*)pt_head_fwd_kernel, PT_HEAD_LDS));
  SF_TRY(sf_phyre_embed_ex(slots, stride_v, stride_t, V, video_index, sel, m->in_proj_w, m->in_proj_b, m->enc_t_pe, m->cls, f + w.X, B, T, N, C, st));
  const uint32_t thr = drop_thresh(dropout_p);
  const size_t M = w.M;
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer& y = m->layers[l];
    PtFwd a;
    a.w = PtLayerW{y.norm1_g, y.norm1_b, y.in_proj_w, y.in_proj_b, y.out_proj_w, y.out_proj_b, y.norm2_g, y.norm2_b, y.lin1_w, y.lin1_b, y.lin2_w, y.lin2_b};
    a.x = f + w.X + l * M * PT_D;
    a.y = f + w.X + (l + 1) * M * PT_D;
    a.xn1 = f + w.xn1 + l * M * PT_D;
    a.qkv = f + w.qkv + l * M * 3 * PT_D;
    a.o = f + w.o + l * M * PT_D;
    a.x2 = f + w.x2 + l * M * PT_D;
    a.xn2 = f + w.xn2 + l * M * PT_D;
    a.hact = f + w.hact + l * M * PT_FFN;
    a.gate = reinterpret_cast<unsigned char*>(f + w.gate) + l * M * PT_FFN;
    a.gate_out = gates ? gates + l * M * PT_FFN : nullptr;
    a.L = L;
    a.s0 = site_seed(seed, 0, l, SITE_ATTN_P); a.s1 = site_seed(seed, 0, l, SITE_ATTN_O);
    a.s2 = site_seed(seed, 0, l, SITE_FFN_H); a.s3 = site_seed(seed, 0, l, SITE_FFN_O);
    a.thresh = thr;
    a.inv_keep = 1.f / (1.f - dropout_p);
    hipLaunchKernelGGL(pt_layer_fwd_kernel, dim3((unsigned)B), dim3(PT_THREADS), lds, st, a);
    SF_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(pt_head_fwd_kernel, dim3((unsigned)((B + PT_HEAD_SEQ - 1) / PT_HEAD_SEQ)), dim3(PT_D), PT_HEAD_LDS, st, f + w.X + nl * M * PT_D, L,
                     m->mlp_w1, m->mlp_b1, m->mlp_w2, m->mlp_b2, logits, f + w.hrelu, reinterpret_cast<unsigned char*>(f + w.hgate), head_gates, B);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_phyre_readout_train_bwd_f32(const sf_phyre_readout_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all,
                                   const int* video_index, const int* sel, int B, int T, const float* g, const sf_phyre_readout_grads* grads,
                                   float dropout_p, unsigned long long seed, void* ws, size_t ws_bytes, void* stream) {
  SF_TRY(pt_check("sf_phyre_readout_train_bwd_f32", m, slots, stride_v, stride_t, V, T_all, video_index, sel, B, T, dropout_p, ws, ws_bytes));
  SF_REQUIRE(g && grads && grads->in_proj_w && grads->in_proj_b && grads->cls && grads->layers && grads->mlp_w1 && grads->mlp_b1 && grads->mlp_w2 &&
                 grads->mlp_b2,
             "sf_phyre_readout_train_bwd_f32: null pointer (only grads->enc_t_pe may be NULL: a fixed table)");
  const int N = m->num_slots, C = m->slot_size, L = 1 + T * N, nl = m->num_layers;
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer_grads& d = grads->layers[l];
    float* const leaves[12] = {d.norm1_g, d.norm1_b, d.in_proj_w, d.in_proj_b, d.out_proj_w, d.out_proj_b, d.norm2_g, d.norm2_b, d.lin1_w, d.lin1_b, d.lin2_w, d.lin2_b};
    for (float* p : leaves) SF_REQUIRE(p && pt_al16(p), "sf_phyre_readout_train_bwd_f32: every layer gradient must be a 16-byte aligned buffer");
  }
  const PtWs w = pt_ws(B, L, nl);
  float* f = static_cast<float*>(ws);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = pt_lds(L), M = w.M;
  SF_TRY(sf_ensure_dyn_lds((const void*)pt_layer_bwd_kernel, lds));
  // ---- the transposed copies of this step's weights: [Wqkv^T | Wo^T | W1^T | W2^T] per layer ----
  PtTrJobs jobs;
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer& y = m->layers[l];
    float* t = f + w.wT + l * PT_WT;
    jobs.j[4 * l + 0] = PtTrJob{y.in_proj_w, t, 3 * PT_D, PT_D};
    jobs.j[4 * l + 1] = PtTrJob{y.out_proj_w, t + 3 * PT_D * PT_D, PT_D, PT_D};
    jobs.j[4 * l + 2] = PtTrJob{y.lin1_w, t + 4 * PT_D * PT_D, PT_FFN, PT_D};
    jobs.j[4 * l + 3] = PtTrJob{y.lin2_w, t + 4 * PT_D * PT_D + PT_D * PT_FFN, PT_D, PT_FFN};
  }
  for (int k = 4 * nl; k < 4 * PT_MAXLAYERS; ++k) jobs.j[k] = PtTrJob{nullptr, nullptr, 0, 0};
  hipLaunchKernelGGL(pt_transpose_kernel, dim3((PT_FFN / 32) * (PT_D / 32), (unsigned)(4 * nl)), dim3(256), 0, st, jobs);
  SF_CHECK_LAUNCH();
  float* dx = f + w.dx;
  hipLaunchKernelGGL(pt_head_bwd_kernel, dim3((unsigned)(PT_D + B)), dim3(PT_D), 0, st, f + w.X + nl * M * PT_D, L, m->mlp_w1, m->mlp_w2, g, f + w.hrelu,
                     reinterpret_cast<const unsigned char*>(f + w.hgate), grads->mlp_w1, grads->mlp_b1, grads->mlp_w2, grads->mlp_b2, dx, B);
  SF_CHECK_LAUNCH();
  const uint32_t thr = drop_thresh(dropout_p);
  float* partial = f + w.partial;
  const int S = pt_splits((long long)M), G = pt_ln_groups((long long)M);
  PtWgJobs wg;
  PtLnJobs ln;
  PtRedJobs red;
  float* lnp = partial + (size_t)S * nl * (PT_WT + PT_BIAS);
  size_t poff = 0;
  int nred = 0;
  for (int l = nl - 1; l >= 0; --l) {
    const sf_tfm_layer& y = m->layers[l];
    const sf_tfm_layer_grads& d = grads->layers[l];
    const float* t = f + w.wT + l * PT_WT;
    PtBwd a;
    a.n1g = y.norm1_g; a.n2g = y.norm2_g;
    a.wqkvT = t; a.woT = t + 3 * PT_D * PT_D; a.w1T = t + 4 * PT_D * PT_D; a.w2T = t + 4 * PT_D * PT_D + PT_D * PT_FFN;
    a.x = f + w.X + l * M * PT_D;
    a.qkv = f + w.qkv + l * M * 3 * PT_D;
    a.x2 = f + w.x2 + l * M * PT_D;
    a.gate = reinterpret_cast<const unsigned char*>(f + w.gate) + l * M * PT_FFN;
    a.dx = dx;
    a.dy2 = f + w.dy2 + l * M * PT_D; a.dh = f + w.dh + l * M * PT_FFN; a.dxn2 = f + w.dxn2 + l * M * PT_D;
    a.do2 = f + w.do2 + l * M * PT_D; a.dqkv = f + w.dqkv + l * M * 3 * PT_D; a.dxn1 = f + w.dxn1 + l * M * PT_D;
    a.L = L;
    a.s0 = site_seed(seed, 0, l, SITE_ATTN_P); a.s1 = site_seed(seed, 0, l, SITE_ATTN_O);
    a.s2 = site_seed(seed, 0, l, SITE_FFN_H); a.s3 = site_seed(seed, 0, l, SITE_FFN_O);
    a.thresh = thr;
    a.inv_keep = 1.f / (1.f - dropout_p);
    hipLaunchKernelGGL(pt_layer_bwd_kernel, dim3((unsigned)B), dim3(PT_THREADS), lds, st, a);
    SF_CHECK_LAUNCH();
    // ---- this layer's jobs of the three parameter-gradient launches behind the loop ----
    const float* Ys[4] = {a.dqkv, a.do2, a.dh, a.dy2};
    const float* Xs[4] = {f + w.xn1 + l * M * PT_D, f + w.o + l * M * PT_D, f + w.xn2 + l * M * PT_D, f + w.hact + l * M * PT_FFN};
    const int Ns[4] = {3 * PT_D, PT_D, PT_FFN, PT_D}, Ks[4] = {PT_D, PT_D, PT_D, PT_FFN};
    float* const dWs[4] = {d.in_proj_w, d.out_proj_w, d.lin1_w, d.lin2_w};
    float* const dbs[4] = {d.in_proj_b, d.out_proj_b, d.lin1_b, d.lin2_b};
    for (int k = 0; k < 4; ++k) {
      const size_t nk = (size_t)Ns[k] * Ks[k];
      wg.j[4 * l + k] = PtWg{Ys[k], Xs[k], Ns[k], Ks[k], (long long)poff, (long long)(poff + S * nk)};
      red.j[nred++] = PtRed{partial + poff, dWs[k], (long long)nk, S, (int)nk};
      red.j[nred++] = PtRed{partial + poff + S * nk, dbs[k], (long long)Ns[k], S, Ns[k]};
      poff += S * (nk + Ns[k]);
    }
    ln.j[2 * l] = PtLn{a.x, a.dxn1};
    ln.j[2 * l + 1] = PtLn{a.x2, a.dxn2};
    float* const dgs[2] = {d.norm1_g, d.norm2_g};
    float* const dbe[2] = {d.norm1_b, d.norm2_b};
    for (int k = 0; k < 2; ++k) {
      const float* src = lnp + (size_t)(2 * l + k) * G * 2 * PT_D;
      red.j[nred++] = PtRed{src, dgs[k], 2 * PT_D, G, PT_D};
      red.j[nred++] = PtRed{src + PT_D, dbe[k], 2 * PT_D, G, PT_D};
    }
  }
  for (int k = 4 * nl; k < 4 * PT_MAXLAYERS; ++k) wg.j[k] = PtWg{nullptr, nullptr, 0, 0, 0, 0};
  for (int k = 2 * nl; k < 2 * PT_MAXLAYERS; ++k) ln.j[k] = PtLn{nullptr, nullptr};
  // ---- the token rows backwards; the row splits of d in_proj.weight join the reduction ----
  const int RS = pt_tok_splits((long long)B * T * N);
  PtSel table;
  for (int t = 0; t < PT_MAXL; ++t) table.v[t] = t < T ? sel[t] : -1;
  PtTok k;
  k.slots = slots; k.stride_v = stride_v; k.stride_t = stride_t; k.V = V; k.video_index = video_index;
  k.dx = dx; k.dWp = f + w.tokp; k.db = grads->in_proj_b; k.dcls = grads->cls; k.dpe = grads->enc_t_pe;
  k.B = B; k.T = T; k.N = N; k.C = C;
  hipLaunchKernelGGL(pt_tok_bwd_kernel, dim3((unsigned)((PT_D / PT_TOK_J) * RS + 2 + (grads->enc_t_pe ? T : 0))), dim3(PT_TOK_THREADS), 0, st, k, table, RS);
  SF_CHECK_LAUNCH();
  red.j[nred++] = PtRed{f + w.tokp, grads->in_proj_w, (long long)PT_D * C, RS, PT_D * C};
  for (int q = nred; q < 12 * PT_MAXLAYERS + 1; ++q) red.j[q] = PtRed{nullptr, nullptr, 0, 0, 0};
  const int rps = (int)((((long long)M + S - 1) / S + 31) & ~31LL), rpg = (int)(((long long)M + G - 1) / G);
  hipLaunchKernelGGL(pt_wgrad_kernel, dim3((PT_FFN / 64) * (PT_D / 64), (unsigned)S, (unsigned)(4 * nl)), dim3(256), 0, st, wg, partial, (long long)M, rps);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(pt_lnparam_kernel, dim3((unsigned)G, (unsigned)(2 * nl)), dim3(256), 0, st, ln, lnp, (long long)M, rpg);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(pt_reduce_kernel, dim3(64, (unsigned)nred), dim3(256), 0, st, red);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

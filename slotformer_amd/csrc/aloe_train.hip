// Training of the CLEVRER VQA reasoner (clevrer_vqa/models/transformer.py under autograd, dropout of nn.TransformerEncoderLayer included; the reference's
// clevrer_vqa/method.py step): the launch chain of sf_aloe_fwd_f32 with what a backward needs kept, and that backward.
//
// A batch is ONE pass over B = B1 + Bn sequences, the descriptive questions first, then the choices of the multiple-choice ones; the two kinds differ in
// the type column of q_in_proj (aloe_embed_kernel: sequences b >= B1, positions < question_len) and in the head MLP.
//
//   forward   text table (recomputed: the weights move every step) -> token rows (aloe.hip) -> per layer  LN1 + q|k|v (sf_linear_ex) -> attention
//             (aloe_attn_kernel<true>: row log-sum-exp kept, site-0 dropout on P) -> out_proj + residual -> LN2 + linear1 + ReLU -> linear2 +
//             residual, with the dropout sites 1..3 as elementwise launches when p > 0 (p == 0: the inference chain, no mask evaluated) -> both heads.
//             Kept per layer: x, q|k|v, attention rows, x2, the post-ReLU hidden rows, lse [B][heads][L].  The last layer is NOT row-pruned.
//   backward  heads -> per layer, last to first: the parameter gradients as contractions over all B L rows (sf_grad_weight_edge_ex, sf_grad_bias_ex,
//             sf_grad_ln_ex), dX = dY W through sf_transpose_ex + sf_linear_ex, LayerNorm / ReLU-dropout input gradients (train_blocks.hip), and
//             at_attn_bwd_kernel -> token rows backwards.
//
//   at_attn_bwd_kernel   one workgroup per (sequence, head), L <= 256, head dim even in [4, 32] zero-padded to 32 in LDS only.  P is recomputed from q, k
//                        and lse, the dropout mask regenerated; delta = rowsum(dO . O); dS = P . (mask dP - delta), dP = dO V^T.  Two passes, no sum
//                        across waves, no atomics.  Pass A: a wave owns 16-query tiles -- S^T and dP^T tiles (keys x queries) against K and V as
//                        bf16 hi | lo planes [key][32], dS^T leaves the accumulators IN the A-operand layout of dQ = dS K (K^T planes [dim][key]),
//                        as P does in the forward.  Pass B (LDS restaged: Q scale and dO as row planes and transposed planes): a wave owns 16-key
//                        tiles, recomputes S and dP tiles (queries x keys), dV = (mask P)^T dO and dK = dS^T (Q scale).  All five products are
//                        split-bf16 (hi.lo + lo.hi + hi.hi) on v_mfma_f32_16x16x32_bf16.  LDS: 2 x 40 KB row planes + 2 x 33 KB transposed planes
//                        + 3 KB of row vectors = 149 KB: one workgroup of eight waves per CU.  Padded keys carry a -inf bias: P = 0, so dK = dV = 0 exactly.
//   token rows backwards plain f32, fixed ascending orders: d pos = sum_b dX0[b], d CLS its row 0; d vision_in_proj.weight = [dY^T slots | 0 | d bias]
//                        with the slots read in place; the text side through G[w] = sum of the live text rows whose token is w, by comparison.
//
// Arithmetic: split-bf16 in every product of the layers (the library's GEMM, both attention kernels, the weight-gradient contraction), which is why any
// other process precision is refused; LayerNorm, softmax, heads, loss gradient in f32 / double.  Every sum has a fixed order: equal inputs and seed give
// equal bits.  Dropout masks: dropout_mask.h, site_seed(seed, 0, layer, site), element index site 0: ((b heads + h) L + i) L + j; sites 1, 3:
// (b L + tok) d + c; site 2: (b L + tok) ffn + j -- padded rows included in the numbering (train.dropout_keep_mask restates them).
#include <math.h>

#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "train_blocks.h"
#include "sf_arena.h"
#include "dropout_mask.h"

namespace {

constexpr int AT_THREADS = 256, AT_WAVES = 4;
constexpr int AT_BWD_THREADS = 512, AT_BWD_WAVES = 8;   // the attention backward: two waves a SIMD cover each other's MFMA and exp latencies
constexpr int AT_MAXL = 256, AT_MAXD = 256, AT_MAXH = 1024, AT_MAXA = 1024;
constexpr int AT_KP = 32 + 8;          // bf16 elements of a row of a [row][32] plane (80 B)
constexpr int AT_VP = AT_MAXL + 8;     // ... of a [dim][row] plane
constexpr size_t AT_RM = 2 * (size_t)AT_MAXL * AT_KP * 2;   // bytes of a hi | lo pair of row planes
constexpr size_t AT_TR = 2 * (size_t)32 * AT_VP * 2;        // ... of transposed planes
constexpr size_t AT_BWD_LDS = 2 * AT_RM + 2 * AT_TR + 3 * AT_MAXL * sizeof(float);
constexpr int AT_TOK_THREADS = 1024, AT_TOK_J = 4, AT_TOK_RS = 16;
constexpr float AT_EPS = 1e-5f;

// ---- elementwise: the dropout sites 1..3 and the recorded gates --------------------------------------------------------------------------------------
// out[i] = (res ? res[i] : 0) + (keep(i) ? v[i] * inv_keep : 0), four elements a thread (n4 = n / 4)
__global__ __launch_bounds__(256) void at_drop_kernel(const float* __restrict__ v, const float* __restrict__ res, float* __restrict__ out, long long n4,
                                                      uint32_t sseed, uint32_t thresh, float inv_keep) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 x = reinterpret_cast<const f32x4*>(v)[i];
  const uint32_t e = (uint32_t)(4 * i);
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = sf_keep(sseed, e + k, thresh) ? x[k] * inv_keep : 0.f;
  if (res) x += reinterpret_cast<const f32x4*>(res)[i];
  reinterpret_cast<f32x4*>(out)[i] = x;
}
__global__ __launch_bounds__(256) void at_gate_kernel(const float* __restrict__ h, unsigned char* __restrict__ gate, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) gate[i] = h[i] > 0.f ? 1 : 0;
}

// ---- attention backward ---------------------------------------------------------------------------------------------------------------------------------
// eight consecutive floats of a row (pairs past the head dim are zero), times scale
__device__ __forceinline__ f32x8 at_ld8(const float* p, int c0, int hd, float scale) {
  f32x8 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x2 t = {0.f, 0.f};
    if (c0 + 2 * j < hd) t = *reinterpret_cast<const f32x2*>(p + 2 * j);
    v[2 * j] = t[0] * scale;
    v[2 * j + 1] = t[1] * scale;
  }
  return v;
}
// rows [0, LP) of src (row r at src + r * ld, hd columns) * scale -> row planes rm (hi at rm, lo behind it) and / or transposed planes tr
__device__ __forceinline__ void at_stage(const float* __restrict__ src, int ld, int L, int LP, int hd, float scale, char* rm, char* tr, int tid) {
  __bf16* rh = reinterpret_cast<__bf16*>(rm);
  __bf16* rl = rh + AT_MAXL * AT_KP;
  unsigned short* th = reinterpret_cast<unsigned short*>(tr);
  unsigned short* tl = th + 32 * AT_VP;
  for (int idx = tid; idx < LP * 16; idx += AT_BWD_THREADS) {
    const int r = idx >> 4, c2 = idx & 15;
    f32x2 v = {0.f, 0.f};
    if (r < L && 2 * c2 < hd) v = *reinterpret_cast<const f32x2*>(src + (long long)r * ld + 2 * c2);
    unsigned h, l;
    pl_split2(v[0] * scale, v[1] * scale, h, l);
    if (rm) {
      *reinterpret_cast<unsigned*>(rh + r * AT_KP + 2 * c2) = h;
      *reinterpret_cast<unsigned*>(rl + r * AT_KP + 2 * c2) = l;
    }
    if (tr) {
      th[(2 * c2) * AT_VP + r] = (unsigned short)(h & 0xffffu);
      th[(2 * c2 + 1) * AT_VP + r] = (unsigned short)(h >> 16);
      tl[(2 * c2) * AT_VP + r] = (unsigned short)(l & 0xffffu);
      tl[(2 * c2 + 1) * AT_VP + r] = (unsigned short)(l >> 16);
    }
  }
}
// acc = a . b in split-bf16 from zero
__device__ __forceinline__ f32x4 at_mma3(const bf16x8 ah, const bf16x8 al, const bf16x8 bh, const bf16x8 bl, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
  return acc;
}
// the fragment of a transposed plane pair for contraction step s: row dt 16 + l15, slots 32 s + 4 q + 0..3 and 32 s + 16 + 4 q + 0..3
__device__ __forceinline__ void at_rd_tr(const char* tr, int dt, int s, int l15, int q, bf16x8& h, bf16x8& l) {
  const unsigned short* th = reinterpret_cast<const unsigned short*>(tr);
  const unsigned short* tl = th + 32 * AT_VP;
  const int o = (dt * 16 + l15) * AT_VP + s * 32 + 4 * q;
  const bf16x4 h0 = *reinterpret_cast<const bf16x4*>(th + o), h1 = *reinterpret_cast<const bf16x4*>(th + o + 16);
  const bf16x4 l0 = *reinterpret_cast<const bf16x4*>(tl + o), l1 = *reinterpret_cast<const bf16x4*>(tl + o + 16);
  h = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  l = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void at_rd_rm(const char* rm, int row, int q, bf16x8& h, bf16x8& l) {
  const __bf16* rh = reinterpret_cast<const __bf16*>(rm);
  const __bf16* rl = rh + AT_MAXL * AT_KP;
  const int o = row * AT_KP + 8 * q;
  h = *reinterpret_cast<const bf16x8*>(rh + o);
  l = *reinterpret_cast<const bf16x8*>(rl + o);
}

// qkv [B L][3 d], o / d_o [B L][d] (the attention rows and their gradient), lse [B][heads][L] -> dqkv [B L][3 d] (this head's columns of every row)
__global__ __launch_bounds__(AT_BWD_THREADS) void at_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ o, const float* __restrict__ d_o,
                                                                 const float* __restrict__ lse, const unsigned char* __restrict__ pad,
                                                                 float* __restrict__ dqkv, int L, int text0, int text_len, int d, int hd, float scale,
                                                                 uint32_t sseed, uint32_t thresh, float inv_keep) {
  extern __shared__ __attribute__((aligned(16))) char at_smem[];
  char* R0 = at_smem;             // pass A: K rows          pass B: Q scale rows
  char* R1 = R0 + AT_RM;          //         V rows                  dO rows
  char* T0 = R1 + AT_RM;          //         K^T                     dO^T
  char* T1 = T0 + AT_TR;          //         --                      (Q scale)^T
  float* kbias = reinterpret_cast<float*>(T1 + AT_TR);
  float* lse_s = kbias + AT_MAXL;
  float* delta_s = lse_s + AT_MAXL;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.x, b = blockIdx.y, nh = gridDim.x;
  const int LP = (L + 31) & ~31, nks = LP >> 5;   // contraction steps of 32 keys / queries
  const int l15 = lane & 15, q = lane >> 4;
  const float* base = qkv + (long long)b * L * 3 * d + h * hd;
  const float* obase = o + (long long)b * L * d + h * hd;
  const float* dobase = d_o + (long long)b * L * d + h * hd;
  const float* lrow = lse + ((long long)b * nh + h) * L;
  float* dbase = dqkv + (long long)b * L * 3 * d + h * hd;
  const uint32_t mbase = (uint32_t)(((long long)b * nh + h) * L * L);

  at_stage(base + d, 3 * d, L, LP, hd, 1.f, R0, T0, tid);
  at_stage(base + 2 * d, 3 * d, L, LP, hd, 1.f, R1, nullptr, tid);
  for (int r = tid; r < AT_MAXL; r += AT_BWD_THREADS) {
    bool live = r < L;
    if (live && r >= text0 && r - text0 < text_len) live = pad[(long long)b * text_len + (r - text0)] == 0;
    kbias[r] = live ? 0.f : -INFINITY;
    lse_s[r] = r < L ? lrow[r] : INFINITY;
    delta_s[r] = 0.f;
  }
  __syncthreads();
  // ---- pass A: d q and delta; a lane holds key 16 kt + 4 q + e of query l15 ----
  for (int qt = wid; qt * 16 < L; qt += AT_BWD_WAVES) {
    const int qi = qt * 16 + l15, qrow = qi < L ? qi : L - 1;
    const f32x8 qv = at_ld8(base + (long long)qrow * 3 * d + 8 * q, 8 * q, hd, scale);
    const f32x8 dov = at_ld8(dobase + (long long)qrow * d + 8 * q, 8 * q, hd, 1.f), ov = at_ld8(obase + (long long)qrow * d + 8 * q, 8 * q, hd, 1.f);
    float dl = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dl = fmaf(dov[j], ov[j], dl);
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    if (q == 0 && qi < L) delta_s[qi] = dl;
    bf16x8 qh, ql, doh, dol;
    sf_split8(qv, qh, ql);
    sf_split8(dov, doh, dol);
    const float lq = lse_s[qrow];
    f32x4 dq[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int s = 0; s < nks; ++s) {
      f32x4 ds[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int kt = 2 * s + u;
        bf16x8 kh, kl, vh, vl;
        at_rd_rm(R0, kt * 16 + l15, q, kh, kl);
        at_rd_rm(R1, kt * 16 + l15, q, vh, vl);
        f32x4 st = at_mma3(kh, kl, qh, ql, f32x4{0.f, 0.f, 0.f, 0.f});
        st += *reinterpret_cast<const f32x4*>(kbias + kt * 16 + 4 * q);
        const f32x4 dp = at_mma3(vh, vl, doh, dol, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = __expf(st[e] - lq);
          float x = dp[e];
          if (thresh) x = sf_keep(sseed, mbase + (uint32_t)(qi * L + kt * 16 + 4 * q + e), thresh) ? x * inv_keep : 0.f;
          ds[u][e] = p * (x - dl);
        }
      }
      bf16x8 ah, al;
      sf_split8(ds[0], ds[1], ah, al);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        if (dt * 16 < hd) {
          bf16x8 bh, bl;
          at_rd_tr(T0, dt, s, l15, q, bh, bl);
          dq[dt] = at_mma3(ah, al, bh, bl, dq[dt]);
        }
    }
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = qt * 16 + 4 * q + e, dc = dt * 16 + l15;
        if (row < L && dc < hd) dbase[(long long)row * 3 * d + dc] = dq[dt][e] * scale;
      }
  }
  __syncthreads();
  // ---- pass B: d k and d v; a lane holds query 16 qt + 4 q + e of key l15 ----
  at_stage(base, 3 * d, L, LP, hd, scale, R0, T1, tid);
  at_stage(dobase, d, L, LP, hd, 1.f, R1, T0, tid);
  __syncthreads();
  for (int kt = wid; kt * 16 < L; kt += AT_BWD_WAVES) {
    const int ki = kt * 16 + l15, krow = ki < L ? ki : L - 1;
    bf16x8 kh, kl, vh, vl;
    sf_split8(at_ld8(base + (long long)krow * 3 * d + d + 8 * q, 8 * q, hd, 1.f), kh, kl);
    sf_split8(at_ld8(base + (long long)krow * 3 * d + 2 * d + 8 * q, 8 * q, hd, 1.f), vh, vl);
    const float kb = kbias[krow];
    f32x4 dk[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, dv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int s = 0; s < nks; ++s) {
      f32x4 ds[2], pm[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int qt = 2 * s + u;
        bf16x8 qh, ql, doh, dol;
        at_rd_rm(R0, qt * 16 + l15, q, qh, ql);
        at_rd_rm(R1, qt * 16 + l15, q, doh, dol);
        const f32x4 sc = at_mma3(qh, ql, kh, kl, f32x4{0.f, 0.f, 0.f, 0.f});
        const f32x4 dp = at_mma3(doh, dol, vh, vl, f32x4{0.f, 0.f, 0.f, 0.f});
        const f32x4 lq = *reinterpret_cast<const f32x4*>(lse_s + qt * 16 + 4 * q), dl = *reinterpret_cast<const f32x4*>(delta_s + qt * 16 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = __expf(sc[e] + kb - lq[e]);
          float x = dp[e], pk = p;
          if (thresh) {
            const bool keep = sf_keep(sseed, mbase + (uint32_t)((qt * 16 + 4 * q + e) * L + ki), thresh);
            x = keep ? x * inv_keep : 0.f;
            pk = keep ? p * inv_keep : 0.f;
          }
          ds[u][e] = p * (x - dl[e]);
          pm[u][e] = pk;
        }
      }
      bf16x8 ph, pl, sh, sl;
      sf_split8(pm[0], pm[1], ph, pl);
      sf_split8(ds[0], ds[1], sh, sl);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        if (dt * 16 < hd) {
          bf16x8 bh, bl;
          at_rd_tr(T0, dt, s, l15, q, bh, bl);
          dv[dt] = at_mma3(ph, pl, bh, bl, dv[dt]);
          at_rd_tr(T1, dt, s, l15, q, bh, bl);
          dk[dt] = at_mma3(sh, sl, bh, bl, dk[dt]);
        }
    }
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = kt * 16 + 4 * q + e, dc = dt * 16 + l15;
        if (row < L && dc < hd) {
          dbase[(long long)row * 3 * d + d + dc] = dk[dt][e];
          dbase[(long long)row * 3 * d + 2 * d + dc] = dv[dt][e];
        }
      }
  }
}

// ---- heads ----------------------------------------------------------------------------------------------------------------------------------------------
struct AtHead {
  const float* x;                    // [B][L][d]; row 0 of every sequence
  const float *W1[2], *b1[2], *W2[2], *b2[2];   // [kind]: 0 descriptive (A outputs), 1 multiple choice (1 output)
  float *cls_logits, *mc_logits;     // [B1][A], [Bn]
  float* hrelu;                      // [B][H]
  unsigned char* head_gates;         // [B][H] or NULL
  const int *video_index, *start, *tokens;
  const unsigned char* pad;
  int V, T_all, T, frame_offset, vocab, text_len, B1, L, d, H, A;
};
// The summation order of aloe_head_kernel: hidden unit j = sf_wave_sum over the lanes of (fma chain over k = lane, lane + 64, ...) + b1[j]; an output the
// same over the hidden units + b2.  An entry whose video, frames or live tokens lie outside their tables gets NaN logits.
__global__ __launch_bounds__(AT_THREADS) void at_head_fwd_kernel(const AtHead a) {
  __shared__ float xs[AT_MAXD], hid[AT_MAXH];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x, d = a.d, H = a.H, kind = b >= a.B1 ? 1 : 0, A = kind ? 1 : a.A;
  int bad = 0;
  if (tid == 0) {
    const int vid = a.video_index ? a.video_index[b] : b;
    const long long f0 = a.start ? a.start[b] : 0, f1 = f0 + (long long)(a.T - 1) * a.frame_offset;
    bad = !(vid >= 0 && vid < a.V && f0 >= 0 && f0 < a.T_all && f1 >= 0 && f1 < a.T_all);
  }
  for (int j = tid; j < a.text_len; j += AT_THREADS) {
    const int tok = a.tokens[(long long)b * a.text_len + j];
    if (a.pad[(long long)b * a.text_len + j] == 0 && !(tok >= 0 && tok < a.vocab)) bad = 1;
  }
  bad = __syncthreads_or(bad);
  for (int k = tid; k < d; k += AT_THREADS) xs[k] = a.x[(long long)b * a.L * d + k];
  __syncthreads();
  for (int j = wid; j < H; j += AT_WAVES) {
    const float* w = a.W1[kind] + (long long)j * d;
    float acc = 0.f;
    for (int k = lane; k < d; k += 64) acc = fmaf(w[k], xs[k], acc);
    acc = sf_wave_sum(acc) + a.b1[kind][j];
    if (lane == 0) {
      const float r = fmaxf(acc, 0.f);
      hid[j] = r;
      a.hrelu[(long long)b * H + j] = r;
      if (a.head_gates) a.head_gates[(long long)b * H + j] = r > 0.f ? 1 : 0;
    }
  }
  __syncthreads();
  for (int o = wid; o < A; o += AT_WAVES) {
    const float* w = a.W2[kind] + (long long)o * H;
    float acc = 0.f;
    for (int k = lane; k < H; k += 64) acc = fmaf(w[k], hid[k], acc);
    acc = sf_wave_sum(acc) + a.b2[kind][o];
    if (lane == 0) {
      acc = bad ? NAN : acc;
      if (kind) a.mc_logits[b - a.B1] = acc;
      else a.cls_logits[(long long)b * a.A + o] = acc;
    }
  }
}

struct AtHeadBwd {
  const float *x, *hrelu;
  const float *W1[2], *W2[2];
  const float *g_cls, *g_mc;         // [B1][A], [Bn]
  float *dhid, *dx;                  // [B][H]; [B][L][d]: row 0 written, the other rows zeroed
  float *dW1[2], *db1[2], *dW2[2], *db2[2];
  int B1, B, L, d, H, A;
};
// one workgroup per sequence: d hidden[j] = gate ? sum_a g[a] W2[a][j] : 0 (a ascending), d x[b, 0][c] = sum_j d hidden[j] W1[j][c] (j ascending)
__global__ __launch_bounds__(AT_THREADS) void at_head_bwd_x_kernel(const AtHeadBwd a) {
  __shared__ float gs[AT_MAXA], dhs[AT_MAXH];
  const int tid = threadIdx.x, b = blockIdx.x, d = a.d, H = a.H, kind = b >= a.B1 ? 1 : 0, A = kind ? 1 : a.A;
  for (int o = tid; o < A; o += AT_THREADS) gs[o] = kind ? a.g_mc[b - a.B1] : a.g_cls[(long long)b * a.A + o];
  __syncthreads();
  for (int j = tid; j < H; j += AT_THREADS) {
    float s = 0.f;
    if (a.hrelu[(long long)b * H + j] > 0.f)
      for (int o = 0; o < A; ++o) s = fmaf(gs[o], a.W2[kind][(long long)o * H + j], s);
    dhs[j] = s;
    a.dhid[(long long)b * H + j] = s;
  }
  __syncthreads();
  float* row = a.dx + (long long)b * a.L * d;
  for (int c = tid; c < d; c += AT_THREADS) {
    float s = 0.f;
    for (int j = 0; j < H; ++j) s = fmaf(dhs[j], a.W1[kind][(long long)j * d + c], s);
    row[c] = s;
  }
  for (int idx = tid; idx < (a.L - 1) * d; idx += AT_THREADS) row[d + idx] = 0.f;
}
// the head parameters, one thread per element, blockIdx.y = the kind, every sum over the kind's sequences in ascending order (an empty kind: zeros)
__global__ __launch_bounds__(AT_THREADS) void at_head_bwd_w_kernel(const AtHeadBwd a) {
  const int kind = blockIdx.y, d = a.d, H = a.H, A = kind ? 1 : a.A;
  const int b0 = kind ? a.B1 : 0, b1 = kind ? a.B : a.B1;
  const long long i = (long long)blockIdx.x * AT_THREADS + threadIdx.x;
  const long long n1 = (long long)H * d, n2 = n1 + H, n3 = n2 + (long long)A * H, n4 = n3 + A;
  if (i >= n4) return;
  float s = 0.f;
  if (i < n1) {
    const int j = (int)(i / d), c = (int)(i - (long long)j * d);
    for (int b = b0; b < b1; ++b) s = fmaf(a.dhid[(long long)b * H + j], a.x[(long long)b * a.L * d + c], s);
    a.dW1[kind][i] = s;
  } else if (i < n2) {
    const int j = (int)(i - n1);
    for (int b = b0; b < b1; ++b) s += a.dhid[(long long)b * H + j];
    a.db1[kind][j] = s;
  } else {
    const bool bias = i >= n3;
    const int o = bias ? (int)(i - n3) : (int)((i - n2) / H), j = bias ? 0 : (int)((i - n2) - (long long)o * H);
    for (int b = b0; b < b1; ++b) {
      const float g = kind ? a.g_mc[b - a.B1] : a.g_cls[(long long)b * a.A + o];
      s = bias ? s + g : fmaf(g, a.hrelu[(long long)b * H + j], s);
    }
    if (bias) a.db2[kind][o] = s;
    else a.dW2[kind][(long long)o * H + j] = s;
  }
}

// ---- losses and their gradient: ONE workgroup ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double at_block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int s = AT_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
__global__ __launch_bounds__(AT_THREADS) void at_score_grad_kernel(const float* __restrict__ cls_logits, const int* __restrict__ cls_labels, int B1, int A,
                                                                   const float* __restrict__ mc_logits, const float* __restrict__ mc_labels, int Bn,
                                                                   float w_cls, float w_mc, float* __restrict__ losses, float* __restrict__ g_cls,
                                                                   float* __restrict__ g_mc) {
  __shared__ double red[AT_THREADS];
  const int tid = threadIdx.x;
  double part = 0.0;
  for (int b = tid; b < B1; b += AT_THREADS) {
    const float* x = cls_logits + (long long)b * A;
    const int y = cls_labels[b];
    float mx = x[0];
    for (int o = 1; o < A; ++o) mx = x[o] > mx ? x[o] : mx;
    double s = 0.0;
    for (int o = 0; o < A; ++o) s += exp((double)x[o] - (double)mx);
    const bool ok = y >= 0 && y < A;
    part += ok ? (double)mx + log(s) - (double)x[y] : (double)NAN;   // (a label outside the vocabulary: NaN, never an address)
    if (g_cls)
      for (int o = 0; o < A; ++o) {
        const double sm = exp((double)x[o] - (double)mx) / s;
        g_cls[(long long)b * A + o] = ok ? (float)((double)w_cls * (sm - (o == y ? 1.0 : 0.0)) / B1) : NAN;
      }
  }
  const double tot_cls = at_block_sum(part, red, tid);
  part = 0.0;
  for (int i = tid; i < Bn; i += AT_THREADS) {
    const double x = mc_logits[i], y = mc_labels[i];
    part += fmax(x, 0.0) - x * y + log1p(exp(-fabs(x)));
    if (g_mc) g_mc[i] = (float)((double)w_mc * (1.0 / (1.0 + exp(-x)) - y) / Bn);
  }
  const double tot_mc = at_block_sum(part, red, tid);
  if (tid == 0 && losses) {
    losses[0] = B1 > 0 ? (float)(tot_cls / B1) : 0.f;
    losses[1] = Bn > 0 ? (float)(tot_mc / Bn) : 0.f;
  }
}

// ---- token rows backwards -----------------------------------------------------------------------------------------------------------------------------
// d pos[r][c] = sum over b ascending of d x[b][r][c]; d CLS = its row 0
__global__ __launch_bounds__(256) void at_pos_kernel(const float* __restrict__ dx, float* __restrict__ dpos, float* __restrict__ dcls, int B, int L, int d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L * d) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += dx[(long long)b * L * d + i];
  dpos[i] = s;
  if (i < d) dcls[i] = s;
}
struct AtVis {
  const float* slots;
  long long stride_v, stride_t;
  int V, T_all;
  const int *video_index, *start;
  int frame_offset;
  const float* dx;     // [B][L][d]
  float* dWp;          // partial [RS][d][C]
  int B, T, N, C, L, d;
};
// workgroup (jt, rs): rows 4 jt .. 4 jt + 3 of d vision_in_proj.weight over the slot rows rs G + g, + RS G, ... (G = 1024 / C thread groups, thread
// (g, c) one slot element against four d x columns per row; the slots read in place, a frame or video outside the table contributes nothing); the
// groups are added in ascending order; at_vis_reduce_kernel adds the row splits in ascending order
__global__ __launch_bounds__(AT_TOK_THREADS) void at_vis_wgrad_kernel(const AtVis a, int RS) {
  __shared__ float red[AT_TOK_J * AT_TOK_THREADS];
  const int tid = threadIdx.x, N = a.N, C = a.C, TN = a.T * N, L = a.L, d = a.d, njt = d / AT_TOK_J;
  const int jt = (int)blockIdx.x % njt, rs = (int)blockIdx.x / njt;
  const int G = AT_TOK_THREADS / C, g = tid / C, c = tid - g * C;
  const long long rows = (long long)a.B * TN;
  float acc[AT_TOK_J] = {0.f, 0.f, 0.f, 0.f};
  if (g < G)
    for (long long r = (long long)rs * G + g; r < rows; r += (long long)RS * G) {
      const int b = (int)(r / TN), rem = (int)(r - (long long)b * TN), t = rem / N, n = rem - t * N;
      const int vid = a.video_index ? a.video_index[b] : b;
      const long long f = (long long)(a.start ? a.start[b] : 0) + (long long)t * a.frame_offset;
      if (vid >= 0 && vid < a.V && f >= 0 && f < a.T_all) {
        const float sv = a.slots[(long long)vid * a.stride_v + f * a.stride_t + n * C + c];
        const f32x4 dv = *reinterpret_cast<const f32x4*>(a.dx + ((long long)b * L + 1 + rem) * d + jt * AT_TOK_J);
#pragma unroll
        for (int k = 0; k < AT_TOK_J; ++k) acc[k] = fmaf(dv[k], sv, acc[k]);
      }
    }
#pragma unroll
  for (int k = 0; k < AT_TOK_J; ++k) red[k * AT_TOK_THREADS + tid] = acc[k];
  __syncthreads();
  if (tid < C)
#pragma unroll
    for (int k = 0; k < AT_TOK_J; ++k) {
      float t = red[k * AT_TOK_THREADS + tid];
      for (int u = 1; u < G; ++u) t += red[k * AT_TOK_THREADS + u * C + tid];
      a.dWp[((long long)rs * d + jt * AT_TOK_J + k) * C + tid] = t;
    }
}
// d vision_in_proj.weight [d][C + 2] = [sum of the row splits | 0 | d bias], d bias[j] = sum over r = 1 .. T N ascending of d pos[r][j]
__global__ __launch_bounds__(256) void at_vis_reduce_kernel(const float* __restrict__ dWp, const float* __restrict__ dpos, float* __restrict__ dWv,
                                                            float* __restrict__ dbv, int RS, int d, int C, int TN) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d * (C + 2)) return;
  const int j = i / (C + 2), c = i - j * (C + 2);
  float s = 0.f;
  if (c < C) {
    for (int rs = 0; rs < RS; ++rs) s += dWp[((long long)rs * d + j) * C + c];
  } else if (c == C + 1) {
    for (int r = 1; r <= TN; ++r) s += dpos[(long long)r * d + j];
    dbv[j] = s;
  }
  dWv[i] = s;
}
// G[w][c], w < vocab: the sum of d x over the live text rows whose token is w; G[vocab + t][c]: over the live text rows of type column t (0: the question
// positions of a multiple-choice sequence, 1: every other) -- (b, j) ascending, chosen by comparison, never by address
__global__ __launch_bounds__(256) void at_text_rows_kernel(const float* __restrict__ dx, const int* __restrict__ tokens, const unsigned char* __restrict__ pad,
                                                           float* __restrict__ G, int B, int B1, int L, int text0, int text_len, int question_len, int vocab,
                                                           int d) {
  __shared__ unsigned char hit[1024];   // a chunk of (b, j) entries decided by all threads, then walked by every column's thread
  const int w = blockIdx.x, c = threadIdx.x;
  const long long n = (long long)B * text_len;
  float s = 0.f;
  for (long long at0 = 0; at0 < n; at0 += 1024) {
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += 256) {
      const long long at = at0 + i;
      bool h = false;
      if (at < n && pad[at] == 0) {
        const int b = (int)(at / text_len), j = (int)(at - (long long)b * text_len);
        h = w < vocab ? tokens[at] == w : ((b >= B1 && j < question_len) ? 0 : 1) == w - vocab;
      }
      hit[i] = h ? 1 : 0;
    }
    __syncthreads();
    if (c < d)
      for (int i = 0; i < 1024; ++i)
        if (hit[i]) {
          const long long at = at0 + i;
          const int b = (int)(at / text_len), j = (int)(at - (long long)b * text_len);
          s += dx[((long long)b * L + text0 + j) * d + c];
        }
  }
  if (c < d) G[(long long)w * d + c] = s;
}
// d q_embedding [vocab][E] = G Wq[:, :E]; d q_in_proj.weight [d][E + 4] = [G^T q_embedding | type 0 | type 1 | sum_w G[w] | 0]; d q_in_proj.bias = that sum
__global__ __launch_bounds__(256) void at_text_param_kernel(const float* __restrict__ G, const float* __restrict__ emb, const float* __restrict__ Wq,
                                                            float* __restrict__ demb, float* __restrict__ dWq, float* __restrict__ dbq, int vocab, int E, int d) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, n1 = (long long)vocab * E, n2 = n1 + (long long)d * (E + 4);
  if (i >= n2) return;
  float s = 0.f;
  if (i < n1) {
    const int w = (int)(i / E), e = (int)(i - (long long)w * E);
    for (int c = 0; c < d; ++c) s = fmaf(G[(long long)w * d + c], Wq[(long long)c * (E + 4) + e], s);
    demb[i] = s;
    return;
  }
  const int c = (int)((i - n1) / (E + 4)), e = (int)((i - n1) - (long long)c * (E + 4));
  if (e < E) {
    for (int w = 0; w < vocab; ++w) s = fmaf(G[(long long)w * d + c], emb[(long long)w * E + e], s);
  } else if (e < E + 2) {
    s = G[(long long)(vocab + e - E) * d + c];
  } else if (e == E + 2) {
    for (int w = 0; w < vocab; ++w) s += G[(long long)w * d + c];
    dbq[c] = s;
  }
  dWq[i - n1] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------
inline bool at_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned at_cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
constexpr size_t AT_SLACK = 256;

struct AtWs {
  float *X, *qkv, *att, *x2, *hid, *lse, *table, *hrelu, *dhid;   // the forward's record
  float *dx, *t1, *do2, *dxn, *xn, *dh, *hdrop, *dqkv, *wT, *partial, *G, *tokp;
  size_t bytes;
};
inline size_t at_max(size_t a, size_t b) { return a > b ? a : b; }
AtWs at_carve(void* ws, const sf_aloe_model* m, int B) {
  SfArena a(ws);
  const size_t L = 1 + (size_t)m->T * m->num_slots + m->text_len, M = (size_t)B * L, d = m->d_model, ffn = m->ffn_dim, nl = m->num_layers;
  AtWs w;
  w.X = a.take((nl + 1) * M * d);
  w.qkv = a.take(nl * M * 3 * d);
  w.att = a.take(nl * M * d);
  w.x2 = a.take(nl * M * d);
  w.hid = a.take(nl * M * ffn);
  w.lse = a.take(nl * (size_t)B * m->num_heads * L);
  w.table = a.take((size_t)m->vocab * d);
  w.hrelu = a.take((size_t)B * m->mlp_hidden);
  w.dhid = a.take((size_t)B * m->mlp_hidden);
  w.dx = a.take(M * d);
  w.t1 = a.take(M * d);
  w.do2 = a.take(M * d);
  w.dxn = a.take(M * d);
  w.xn = a.take(M * d);
  w.dh = a.take(M * ffn);
  w.hdrop = a.take(M * ffn);
  w.dqkv = a.take(M * 3 * d);
  w.wT = a.take(at_max(3 * d * d, d * ffn));
  const long long rows = (long long)M;
  w.partial = a.take(at_max(at_max(sf_grad_partial_edge_floats(rows, (int)(3 * d), (int)d), sf_grad_partial_edge_floats(rows, (int)d, (int)d)),
                            at_max(sf_grad_partial_edge_floats(rows, (int)ffn, (int)d), sf_grad_partial_edge_floats(rows, (int)d, (int)ffn))));
  w.G = a.take((size_t)(m->vocab + 2) * d);
  w.tokp = a.take((size_t)AT_TOK_RS * d * m->slot_size);
  w.bytes = a.bytes();
  return w;
}
inline int at_vis_splits(long long rows) { const long long s = rows / 256; return (int)(s < 1 ? 1 : s > AT_TOK_RS ? AT_TOK_RS : s); }

#define AT_LIMITS                                                                                                                                     \
  "1 <= num_slots <= 16, slot_size a multiple of 32 in [32, 256], T >= 1, text_len >= 1, 1 + T * num_slots + text_len <= 256, d_model = heads * "      \
  "head_dim <= 256 and a multiple of 4, head_dim even in [4, 32], ffn a multiple of 64 in [64, 1024], 1 <= num_layers <= 32"

inline bool at_shape_ok(const sf_aloe_model* m) {
  return m && sf_aloe_train_ok(m->num_slots, m->slot_size, m->T, m->text_len, m->d_model, m->num_heads, m->ffn_dim, m->num_layers) == 1 && m->vocab >= 1 &&
         m->emb_dim >= 1 && m->question_len >= 0 && m->mlp_hidden >= 1 && m->mlp_hidden <= AT_MAXH && m->num_answers >= 1 && m->num_answers <= AT_MAXA;
}

// everything both calls check, before any launch
int at_check(const char* who, const sf_aloe_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index,
             const int* tokens, const unsigned char* pad_mask, int B1, int Bn, float dropout_p, const void* ws, size_t ws_bytes) {
  static thread_local char msg[640];
  auto fail = [&](const char* what) {
    snprintf(msg, sizeof msg, "invalid argument: %s: %s", who, what);
    return sf_set_err(-1, msg, __FILE__, __LINE__);
  };
  if (!m || !slots || !tokens || !pad_mask || !ws) return fail("null pointer");
  if (!at_shape_ok(m))
    return fail("unsupported shape (" AT_LIMITS "; vocab >= 1, emb_dim >= 1, question_len >= 0, 1 <= mlp_hidden, num_answers <= 1024)");
  if (!m->cls || !m->pos || !m->vision_w || !m->vision_b || !m->q_embedding || !m->q_in_proj_w || !m->q_in_proj_b || !m->layers || !m->cls_w1 ||
      !m->cls_b1 || !m->cls_w2 || !m->cls_b2 || !m->mc_w1 || !m->mc_b1 || !m->mc_w2 || !m->mc_b2)
    return fail("null pointer in the model");
  if (B1 < 0 || Bn < 0) return fail("B1 >= 0, Bn >= 0");
  const long long B = (long long)B1 + Bn;
  if (B < 1 || B > 65535) return fail("1 <= B1 + Bn <= 65535");
  if (V < 1 || T_all < 1) return fail("V >= 1, T_all >= 1");
  const int N = m->num_slots, C = m->slot_size;
  const long long L = 1 + (long long)m->T * N + m->text_len;
  if (B * L * (3 * m->d_model > m->ffn_dim ? 3 * m->d_model : m->ffn_dim) >= (1LL << 31) || B * m->num_heads * L * L >= (1LL << 32))
    return fail("batch too large for one call: B * L * max(3 d_model, ffn) must stay below 2^31 and B * heads * L * L below 2^32 (the mask index)");
  if (!(stride_t >= (long long)N * C && stride_t % 4 == 0 && stride_v >= 0 && stride_v % 4 == 0)) return fail("frame stride >= N * C, strides multiples of 4");
  if (!video_index && B > V) return fail("B > V without a video_index");
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail("dropout_p must lie in [0, 1)");
  for (int l = 0; l < m->num_layers; ++l) {
    const sf_tfm_layer& y = m->layers[l];
    if (!y.norm1_g || !y.norm1_b || !y.in_proj_w || !y.in_proj_b || !y.out_proj_w || !y.out_proj_b || !y.norm2_g || !y.norm2_b || !y.lin1_w || !y.lin1_b ||
        !y.lin2_w || !y.lin2_b)
      return fail("null pointer in a layer");
    if (!at_al16(y.in_proj_w) || !at_al16(y.out_proj_w) || !at_al16(y.lin1_w) || !at_al16(y.lin2_w) || !at_al16(y.norm1_g) || !at_al16(y.norm2_g) ||
        !at_al16(y.norm1_b) || !at_al16(y.norm2_b))
      return fail("the layers' matrices and LayerNorm parameters must be 16-byte aligned");
  }
  if (!at_al16(slots) || !at_al16(m->vision_w) || !at_al16(ws)) return fail("slots, vision_w and the workspace must be 16-byte aligned");
  if (ws_bytes < sf_aloe_train_workspace_bytes(m, (int)B)) return fail("workspace too small");
  if (sf_get_precision() != 1) return fail("split-bf16 mode only (the layers have no other form)");
  return 0;
}

inline int at_drop(const float* v, const float* res, float* out, long long n, uint32_t sseed, uint32_t thresh, float inv_keep, hipStream_t st) {
  hipLaunchKernelGGL(at_drop_kernel, dim3(at_cdiv(n / 4, 256)), dim3(256), 0, st, v, res, out, n / 4, sseed, thresh, inv_keep);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int sf_aloe_train_ok(int num_slots, int slot_size, int T, int text_len, int d_model, int num_heads, int ffn, int num_layers) {
  return sf_aloe_ok(num_slots, slot_size, T, text_len, d_model, num_heads, ffn, num_layers);
}

size_t sf_aloe_train_workspace_bytes(const sf_aloe_model* m, int B) {
  if (!at_shape_ok(m) || B < 1 || B > 65535) return 0;
  return at_carve(nullptr, m, B).bytes + AT_SLACK;
}

int sf_aloe_train_fwd_f32(const sf_aloe_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index,
                          const int* start, int frame_offset, const int* tokens, const unsigned char* pad_mask, int B1, int Bn, float dropout_p,
                          unsigned long long seed, float* cls_logits, float* mc_logits, unsigned char* gates, unsigned char* head_gates, void* ws,
                          size_t ws_bytes, void* stream) {
  SF_TRY(at_check("sf_aloe_train_fwd_f32", m, slots, stride_v, stride_t, V, T_all, video_index, tokens, pad_mask, B1, Bn, dropout_p, ws, ws_bytes));
  SF_REQUIRE((B1 == 0 || cls_logits) && (Bn == 0 || mc_logits), "sf_aloe_train_fwd_f32: null pointer (a kind with rows needs its logits buffer)");
  const int N = m->num_slots, T = m->T, TL = m->text_len, d = m->d_model, nh = m->num_heads, ffn = m->ffn_dim, nl = m->num_layers, B = B1 + Bn;
  const int L = 1 + T * N + TL, M = B * L;
  const AtWs w = at_carve(ws, m, B);
  hipStream_t st = (hipStream_t)stream;
  SF_TRY(sf_aloe_text_table_f32(m->q_embedding, m->q_in_proj_w, m->q_in_proj_b, w.table, m->vocab, m->emb_dim, d, stream));
  sf_aloe e{};
  e.num_slots = N; e.slot_size = m->slot_size; e.T = T; e.text_len = TL; e.question_len = m->question_len; e.d_model = d; e.num_heads = nh;
  e.ffn_dim = ffn; e.num_layers = nl; e.vocab = m->vocab; e.emb_dim = m->emb_dim; e.cls = m->cls; e.pos = m->pos; e.vision_w = m->vision_w;
  e.vision_b = m->vision_b; e.q_in_proj_w = m->q_in_proj_w; e.text_table = w.table; e.layers = m->layers;
  SF_TRY(sf_aloe_embed_ex(&e, slots, stride_v, stride_t, V, T_all, video_index, start, frame_offset, tokens, B1, w.X, B, st));
  const uint32_t thr = drop_thresh(dropout_p);
  const float inv_keep = 1.f / (1.f - dropout_p);
  const size_t Md = (size_t)M * d;
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer& y = m->layers[l];
    const float* x = w.X + l * Md;
    float* xo = w.X + (l + 1) * Md;
    float* qkv = w.qkv + l * Md * 3;
    float* att = w.att + l * Md;
    float* x2 = w.x2 + l * Md;
    float* hid = w.hid + (size_t)l * M * ffn;
    SF_TRY(sf_linear_ex(x, sf_rows(d), y.in_proj_w, y.in_proj_b, y.norm1_g, y.norm1_b, AT_EPS, nullptr, sf_rows(3 * d), 0, qkv, sf_rows(3 * d), M, 3 * d, d, 0, st));
    SF_TRY(sf_aloe_attn_train_ex(qkv, pad_mask, att, w.lse + (size_t)l * B * nh * L, B, L, 1 + T * N, TL, d, nh, site_seed(seed, 0, l, SITE_ATTN_P), thr,
                                 inv_keep, st));
    if (thr == 0) {
      SF_TRY(sf_linear_ex(att, sf_rows(d), y.out_proj_w, y.out_proj_b, nullptr, nullptr, 0.f, x, sf_rows(d), 0, x2, sf_rows(d), M, d, d, 0, st));
      SF_TRY(sf_linear_ex(x2, sf_rows(d), y.lin1_w, y.lin1_b, y.norm2_g, y.norm2_b, AT_EPS, nullptr, sf_rows(ffn), 0, hid, sf_rows(ffn), M, ffn, d, 1, st));
      SF_TRY(sf_linear_ex(hid, sf_rows(ffn), y.lin2_w, y.lin2_b, nullptr, nullptr, 0.f, x2, sf_rows(d), 0, xo, sf_rows(d), M, d, ffn, 0, st));
    } else {
      SF_TRY(sf_linear_ex(att, sf_rows(d), y.out_proj_w, y.out_proj_b, nullptr, nullptr, 0.f, nullptr, sf_rows(d), 0, w.dxn, sf_rows(d), M, d, d, 0, st));
      SF_TRY(at_drop(w.dxn, x, x2, (long long)Md, site_seed(seed, 0, l, SITE_ATTN_O), thr, inv_keep, st));
      SF_TRY(sf_linear_ex(x2, sf_rows(d), y.lin1_w, y.lin1_b, y.norm2_g, y.norm2_b, AT_EPS, nullptr, sf_rows(ffn), 0, hid, sf_rows(ffn), M, ffn, d, 1, st));
      SF_TRY(at_drop(hid, nullptr, w.hdrop, (long long)M * ffn, site_seed(seed, 0, l, SITE_FFN_H), thr, inv_keep, st));
      SF_TRY(sf_linear_ex(w.hdrop, sf_rows(ffn), y.lin2_w, y.lin2_b, nullptr, nullptr, 0.f, nullptr, sf_rows(d), 0, w.dxn, sf_rows(d), M, d, ffn, 0, st));
      SF_TRY(at_drop(w.dxn, x2, xo, (long long)Md, site_seed(seed, 0, l, SITE_FFN_O), thr, inv_keep, st));
    }
    if (gates) {
      hipLaunchKernelGGL(at_gate_kernel, dim3(at_cdiv((long long)M * ffn, 256)), dim3(256), 0, st, hid, gates + (size_t)l * M * ffn, (long long)M * ffn);
      SF_CHECK_LAUNCH();
    }
  }
  AtHead hp;
  hp.x = w.X + nl * Md;
  hp.W1[0] = m->cls_w1; hp.b1[0] = m->cls_b1; hp.W2[0] = m->cls_w2; hp.b2[0] = m->cls_b2;
  hp.W1[1] = m->mc_w1; hp.b1[1] = m->mc_b1; hp.W2[1] = m->mc_w2; hp.b2[1] = m->mc_b2;
  hp.cls_logits = cls_logits; hp.mc_logits = mc_logits; hp.hrelu = w.hrelu; hp.head_gates = head_gates;
  hp.video_index = video_index; hp.start = start; hp.tokens = tokens; hp.pad = pad_mask; hp.V = V; hp.T_all = T_all; hp.T = T;
  hp.frame_offset = frame_offset; hp.vocab = m->vocab; hp.text_len = TL; hp.B1 = B1; hp.L = L; hp.d = d; hp.H = m->mlp_hidden; hp.A = m->num_answers;
  hipLaunchKernelGGL(at_head_fwd_kernel, dim3((unsigned)B), dim3(AT_THREADS), 0, st, hp);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_aloe_train_bwd_f32(const sf_aloe_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index,
                          const int* start, int frame_offset, const int* tokens, const unsigned char* pad_mask, int B1, int Bn, const float* g_cls,
                          const float* g_mc, const sf_aloe_grads* grads, float dropout_p, unsigned long long seed, void* ws, size_t ws_bytes, void* stream) {
  SF_TRY(at_check("sf_aloe_train_bwd_f32", m, slots, stride_v, stride_t, V, T_all, video_index, tokens, pad_mask, B1, Bn, dropout_p, ws, ws_bytes));
  SF_REQUIRE((B1 == 0 || g_cls) && (Bn == 0 || g_mc), "sf_aloe_train_bwd_f32: null pointer (a kind with rows needs its logit gradient)");
  SF_REQUIRE(grads && grads->cls && grads->pos && grads->vision_w && grads->vision_b && grads->q_embedding && grads->q_in_proj_w && grads->q_in_proj_b &&
                 grads->layers && grads->cls_w1 && grads->cls_b1 && grads->cls_w2 && grads->cls_b2 && grads->mc_w1 && grads->mc_b1 && grads->mc_w2 &&
                 grads->mc_b2,
             "sf_aloe_train_bwd_f32: null pointer in the gradients");
  const int N = m->num_slots, C = m->slot_size, T = m->T, TL = m->text_len, d = m->d_model, nh = m->num_heads, ffn = m->ffn_dim, nl = m->num_layers;
  const int B = B1 + Bn, L = 1 + T * N + TL, M = B * L, hd = d / nh, H = m->mlp_hidden, A = m->num_answers;
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer_grads& g = grads->layers[l];
    float* const aligned[8] = {g.in_proj_w, g.in_proj_b, g.out_proj_w, g.out_proj_b, g.lin1_w, g.lin1_b, g.lin2_w, g.lin2_b};
    for (float* p : aligned) SF_REQUIRE(p && at_al16(p), "sf_aloe_train_bwd_f32: a layer's matrix and bias gradients must be 16-byte aligned buffers");
    SF_REQUIRE(g.norm1_g && g.norm1_b && g.norm2_g && g.norm2_b, "sf_aloe_train_bwd_f32: null pointer in a layer's gradients");
  }
  const AtWs w = at_carve(ws, m, B);
  hipStream_t st = (hipStream_t)stream;
  SF_TRY(sf_ensure_dyn_lds((const void*)at_attn_bwd_kernel, AT_BWD_LDS));
  const size_t Md = (size_t)M * d;
  // ---- the heads ----
  AtHeadBwd hb;
  hb.x = w.X + nl * Md; hb.hrelu = w.hrelu;
  hb.W1[0] = m->cls_w1; hb.W2[0] = m->cls_w2; hb.W1[1] = m->mc_w1; hb.W2[1] = m->mc_w2;
  hb.g_cls = g_cls; hb.g_mc = g_mc; hb.dhid = w.dhid; hb.dx = w.dx;
  hb.dW1[0] = grads->cls_w1; hb.db1[0] = grads->cls_b1; hb.dW2[0] = grads->cls_w2; hb.db2[0] = grads->cls_b2;
  hb.dW1[1] = grads->mc_w1; hb.db1[1] = grads->mc_b1; hb.dW2[1] = grads->mc_w2; hb.db2[1] = grads->mc_b2;
  hb.B1 = B1; hb.B = B; hb.L = L; hb.d = d; hb.H = H; hb.A = A;
  hipLaunchKernelGGL(at_head_bwd_x_kernel, dim3((unsigned)B), dim3(AT_THREADS), 0, st, hb);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(at_head_bwd_w_kernel, dim3(at_cdiv((long long)H * d + H + (long long)A * H + A, AT_THREADS), 2), dim3(AT_THREADS), 0, st, hb);
  SF_CHECK_LAUNCH();
  // ---- the layers, last to first; w.dx holds d loss / d (layer output) and leaves as d loss / d (layer input) ----
  const uint32_t thr = drop_thresh(dropout_p);
  const float inv_keep = 1.f / (1.f - dropout_p), scale = 1.0f / sqrtf((float)hd);
  for (int l = nl - 1; l >= 0; --l) {
    const sf_tfm_layer& y = m->layers[l];
    const sf_tfm_layer_grads& g = grads->layers[l];
    const float* x = w.X + l * Md;
    const float* qkv = w.qkv + l * Md * 3;
    const float* att = w.att + l * Md;
    const float* x2 = w.x2 + l * Md;
    const float* hid = w.hid + (size_t)l * M * ffn;
    // linear2 and its dropout sites
    const float* dy2 = w.dx;
    const float* hdn = hid;
    if (thr) {
      SF_TRY(at_drop(w.dx, nullptr, w.t1, (long long)Md, site_seed(seed, 0, l, SITE_FFN_O), thr, inv_keep, st));
      SF_TRY(at_drop(hid, nullptr, w.hdrop, (long long)M * ffn, site_seed(seed, 0, l, SITE_FFN_H), thr, inv_keep, st));
      dy2 = w.t1;
      hdn = w.hdrop;
    }
    SF_TRY(sf_grad_weight_edge_ex(dy2, hdn, g.lin2_w, M, d, ffn, w.partial, st));
    SF_TRY(sf_grad_bias_ex(dy2, g.lin2_b, M, d, w.partial, st));
    SF_TRY(sf_transpose_ex(y.lin2_w, w.wT, d, ffn, st));   // [d][ffn] -> [ffn][d]
    SF_TRY(sf_linear_ex(dy2, sf_rows(d), w.wT, nullptr, nullptr, nullptr, 0.f, nullptr, sf_rows(ffn), 0, w.dh, sf_rows(ffn), M, ffn, d, 0, st));
    SF_TRY(sf_relu_dropout_bwd_ex(w.dh, hdn, (long long)M * ffn, thr ? inv_keep : 1.f, st));
    // LN2 + linear1
    SF_TRY(sf_layernorm_ex(x2, sf_rows(d), y.norm2_g, y.norm2_b, w.xn, sf_rows(d), M, d, AT_EPS, st));
    SF_TRY(sf_grad_weight_edge_ex(w.dh, w.xn, g.lin1_w, M, ffn, d, w.partial, st));
    SF_TRY(sf_grad_bias_ex(w.dh, g.lin1_b, M, ffn, w.partial, st));
    SF_TRY(sf_transpose_ex(y.lin1_w, w.wT, ffn, d, st));   // [ffn][d] -> [d][ffn]
    SF_TRY(sf_linear_ex(w.dh, sf_rows(ffn), w.wT, nullptr, nullptr, nullptr, 0.f, nullptr, sf_rows(d), 0, w.dxn, sf_rows(d), M, d, ffn, 0, st));
    SF_TRY(sf_grad_ln_ex(x2, w.dxn, g.norm2_g, g.norm2_b, M, d, AT_EPS, w.partial, st));
    // d x2 (in place over d y) and d (out_proj output) = dropout'(d x2)
    SF_TRY(sf_ln_bwd_dropout_ex(x2, w.dxn, y.norm2_g, w.dx, w.dx, thr ? w.do2 : nullptr, site_seed(seed, 0, l, SITE_ATTN_O), thr, inv_keep, M, d, AT_EPS, st));
    const float* do2 = thr ? w.do2 : w.dx;
    SF_TRY(sf_grad_weight_edge_ex(do2, att, g.out_proj_w, M, d, d, w.partial, st));
    SF_TRY(sf_grad_bias_ex(do2, g.out_proj_b, M, d, w.partial, st));
    SF_TRY(sf_transpose_ex(y.out_proj_w, w.wT, d, d, st));
    SF_TRY(sf_linear_ex(do2, sf_rows(d), w.wT, nullptr, nullptr, nullptr, 0.f, nullptr, sf_rows(d), 0, w.t1, sf_rows(d), M, d, d, 0, st));
    // attention
    hipLaunchKernelGGL(at_attn_bwd_kernel, dim3((unsigned)nh, (unsigned)B), dim3(AT_BWD_THREADS), AT_BWD_LDS, st, qkv, att, w.t1,
                       w.lse + (size_t)l * B * nh * L, pad_mask, w.dqkv, L, 1 + T * N, TL, d, hd, scale, site_seed(seed, 0, l, SITE_ATTN_P), thr, inv_keep);
    SF_CHECK_LAUNCH();
    // LN1 + q|k|v
    SF_TRY(sf_layernorm_ex(x, sf_rows(d), y.norm1_g, y.norm1_b, w.xn, sf_rows(d), M, d, AT_EPS, st));
    SF_TRY(sf_grad_weight_edge_ex(w.dqkv, w.xn, g.in_proj_w, M, 3 * d, d, w.partial, st));
    SF_TRY(sf_grad_bias_ex(w.dqkv, g.in_proj_b, M, 3 * d, w.partial, st));
    SF_TRY(sf_transpose_ex(y.in_proj_w, w.wT, 3 * d, d, st));   // [3 d][d] -> [d][3 d]
    SF_TRY(sf_linear_ex(w.dqkv, sf_rows(3 * d), w.wT, nullptr, nullptr, nullptr, 0.f, nullptr, sf_rows(d), 0, w.dxn, sf_rows(d), M, d, 3 * d, 0, st));
    SF_TRY(sf_grad_ln_ex(x, w.dxn, g.norm1_g, g.norm1_b, M, d, AT_EPS, w.partial, st));
    SF_TRY(sf_ln_bwd_dropout_ex(x, w.dxn, y.norm1_g, w.dx, w.dx, nullptr, 0u, 0u, 1.f, M, d, AT_EPS, st));
  }
  // ---- the token rows ----
  hipLaunchKernelGGL(at_pos_kernel, dim3(at_cdiv((long long)L * d, 256)), dim3(256), 0, st, w.dx, grads->pos, grads->cls, B, L, d);
  SF_CHECK_LAUNCH();
  const int RS = at_vis_splits((long long)B * T * N);
  AtVis v;
  v.slots = slots; v.stride_v = stride_v; v.stride_t = stride_t; v.V = V; v.T_all = T_all; v.video_index = video_index; v.start = start;
  v.frame_offset = frame_offset; v.dx = w.dx; v.dWp = w.tokp; v.B = B; v.T = T; v.N = N; v.C = C; v.L = L; v.d = d;
  hipLaunchKernelGGL(at_vis_wgrad_kernel, dim3((unsigned)((d / AT_TOK_J) * RS)), dim3(AT_TOK_THREADS), 0, st, v, RS);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(at_vis_reduce_kernel, dim3(at_cdiv((long long)d * (C + 2), 256)), dim3(256), 0, st, w.tokp, grads->pos, grads->vision_w, grads->vision_b, RS,
                     d, C, T * N);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(at_text_rows_kernel, dim3((unsigned)(m->vocab + 2)), dim3(256), 0, st, w.dx, tokens, pad_mask, w.G, B, B1, L, 1 + T * N, TL, m->question_len,
                     m->vocab, d);
  SF_CHECK_LAUNCH();
  const int E = m->emb_dim;
  hipLaunchKernelGGL(at_text_param_kernel, dim3(at_cdiv((long long)m->vocab * E + (long long)d * (E + 4), 256)), dim3(256), 0, st, w.G, m->q_embedding,
                     m->q_in_proj_w, grads->q_embedding, grads->q_in_proj_w, grads->q_in_proj_b, m->vocab, E, d);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_aloe_score_grad_f32(const float* cls_logits, const int* cls_labels, int B1, int num_answers, const float* mc_logits, const float* mc_labels, int Bn,
                           float w_cls, float w_mc, float* losses, float* g_cls, float* g_mc, void* stream) {
  SF_REQUIRE(B1 >= 0 && Bn >= 0, "sf_aloe_score_grad_f32: B1 >= 0, Bn >= 0");
  SF_REQUIRE(B1 == 0 || (cls_logits && cls_labels && num_answers >= 1), "sf_aloe_score_grad_f32: descriptive logits need labels and num_answers >= 1");
  SF_REQUIRE(Bn == 0 || (mc_logits && mc_labels), "sf_aloe_score_grad_f32: multiple-choice logits need labels");
  hipLaunchKernelGGL(at_score_grad_kernel, dim3(1), dim3(AT_THREADS), 0, (hipStream_t)stream, cls_logits, cls_labels, B1, num_answers, mc_logits, mc_labels, Bn,
                     w_cls, w_mc, losses, g_cls, g_mc);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

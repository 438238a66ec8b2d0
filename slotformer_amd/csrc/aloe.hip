// The CLEVRER VQA reasoner (clevrer_vqa/models/transformer.py: CLEVRERTransformerModel, aloe.py: CLEVRERAloe) at inference:
//
//   tokens[b] = [ CLS ; vision_in_proj([slot(b, t, n) | 0 1])  t-major, slot-minor ; q_in_proj([q_embedding[token] | type pair | 1 0]) ] + pos     L rows of d
//   x         = num_layers pre-LN nn.TransformerEncoderLayer (relu, eps 1e-5) with the padded text positions masked out as keys
//   logits[b] = W2 relu(W1 x[b, 0] + b1) + b2              (cls_answer_mlp: A = answer vocabulary; mc_answer_mlp: A = 1)
//
//   aloe_text_table_kernel  once per weight version: P[w] = Wq[:, :E] q_embedding[w] + Wq[:, E + 2] + bq for every vocabulary word (plain f32 fma chain
//                           over e ascending from the bias term).  q_in_proj over a text token is then P[token] + one of the type columns Wq[:, E], Wq[:, E + 1].
//   aloe_embed_kernel       a workgroup owns 48 vision rows (three 16-row MFMA tiles) of the flattened (b, t, n) space: the slots are read IN PLACE through
//                           (stride_v, stride_t) at video video_index[b], frame start[b] + t * frame_offset, split into bf16 hi | lo planes in LDS, and the
//                           four waves sweep the ceil(d / 16) column tiles of vision_in_proj (v_mfma_f32_16x16x32_bf16; weight rows read as f32, split on the
//                           fly; the id pair [0 1] is the bias column C + 1).  One workgroup per sequence behind the row tiles writes CLS and the text rows.
//                           Every row gets its position row.  A video, frame or token outside its table is a zero operand, never an address; the head kernel
//                           turns such an entry into NaN logits.
//   aloe_attn_kernel        one workgroup per (sequence, head), L <= 256 tokens, head dim <= 32.  K as bf16 hi | lo planes [key][32] (the head dim
//                           zero-padded to the MFMA's K in LDS only) and V transposed, [dim][key]; the wave owns 16-query tiles and computes S^T = K Q^T, so
//                           that a lane holds its query's scores for keys 4 (lane >> 4) + e of every key tile IN the A-operand layout of the second
//                           product -- the contraction slots of P V are assigned to (key tile pair, lane group) accordingly and P never touches LDS.
//                           Softmax in f32 (v_exp_f32), padded text positions and keys past L carry a -inf bias: they are never keys.  Padded rows are
//                           computed as queries like any other; nothing reads them.  In the LAST layer only the CLS row is a query (keys and values
//                           from all rows), and the GEMMs around it run on the B CLS rows.  aloe_attn_kernel<true> is the training form (aloe_train.hip): every
//                           row a query, the row log-sum-exp kept, dropout on P.
//                           LDS per workgroup: K 2 x 256 x 80 B = 40 KB, V^T 2 x 32 x 528 B = 33 KB, key bias 1 KB: 74 KB of the 160 KB of a CU -- two
//                           workgroups (eight waves) share a CU.
//   aloe_head_kernel        one workgroup per sequence, plain f32: row 0 in LDS, a wave per hidden unit (lanes stride over k, sf_wave_sum), a wave per
//                           output; optionally the argmax (first index on ties; A = 1: logit > 0).  Checks the entry's video, frames and live tokens.
//   aloe_score_kernel       ONE workgroup: cross-entropy and BCE-with-logits sums in double, each thread over its rows in ascending order, then a fixed
//                           tree; per question "all its choices right"; the counts of CLEVRERAloe.calc_eval_loss as int32 ADDED to the caller's buffer.
//
// The linear parts (LN1 + q|k|v, out_proj + residual, LN2 + linear1 + ReLU, linear2 + residual at K = d / ffn) are the library's GEMM (sf_linear_ex).
// Arithmetic: split-bf16 -- every f32 operand of a product is bf16 hi + bf16 lo, three products hi.lo + lo.hi + hi.hi with f32 accumulation -- in the
// embedding, the GEMMs and both attention products, which is why the forward refuses every other process precision.  Every sum has a fixed order and there
// are no atomics on floats: equal inputs give equal bits.
#include <math.h>

#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "train_blocks.h"
#include "dropout_mask.h"

namespace {

constexpr int AL_MAXL = 256;       // tokens of a sequence
constexpr int AL_MAXD = 256;       // d_model
constexpr int AL_MAXHD = 32;       // head dim: one K = 32 step of the MFMA
constexpr int AL_THREADS = 256, AL_WAVES = 4;
constexpr int AL_ROWS = 48;        // vision rows of an embed workgroup
constexpr int AL_KS = 8;           // k-steps of 32 at the widest slot (C = 256)
constexpr int AL_KP = AL_MAXHD + 8;    // bf16 elements of a K row in LDS (80 B: ds_read_b128 of 16 consecutive rows is conflict-free)
constexpr int AL_VP = AL_MAXL + 8;     // bf16 elements of a V^T row
constexpr int AL_KT = AL_MAXL / 16;    // key tiles
constexpr size_t AL_ATTN_LDS = 2 * (size_t)AL_MAXL * AL_KP * 2 + 2 * (size_t)AL_MAXHD * AL_VP * 2 + AL_MAXL * sizeof(float);
constexpr int AL_MAXH = 1024, AL_MAXA = 1024;   // hidden units and outputs of a head

inline bool al_ok(int N, int C, int T, int text_len, int d, int nh, int ffn, int nl) {
  if (!(N >= 1 && N <= 16 && C >= 32 && C <= 256 && C % 32 == 0 && T >= 1 && T <= AL_MAXL && text_len >= 1 && text_len <= AL_MAXL)) return false;
  if (1 + T * N + text_len > AL_MAXL) return false;
  if (!(nh >= 1 && d >= 4 && d <= AL_MAXD && d % nh == 0 && d % 4 == 0)) return false;
  const int hd = d / nh;
  return hd >= 4 && hd <= AL_MAXHD && hd % 2 == 0 && ffn >= 64 && ffn <= 1024 && ffn % 64 == 0 && nl >= 1 && nl <= 32;
}
__host__ __device__ inline int al_pitch(int C) { return (C + 8) * 2; }   // bytes of a row of a bf16 plane of slots
inline size_t al_embed_lds(int C) { return (size_t)2 * AL_ROWS * al_pitch(C); }

__global__ __launch_bounds__(AL_THREADS) void aloe_text_table_kernel(const float* __restrict__ emb, const float* __restrict__ Wq, const float* __restrict__ bq,
                                                                     float* __restrict__ table, int vocab, int E, int d) {
  const long long i = (long long)blockIdx.x * AL_THREADS + threadIdx.x;
  if (i >= (long long)vocab * d) return;
  const int w = (int)(i / d), c = (int)(i - (long long)w * d);
  const float* wr = Wq + (long long)c * (E + 4);
  float acc = wr[E + 2] + bq[c];
  for (int e = 0; e < E; ++e) acc = fmaf(wr[e], emb[(long long)w * E + e], acc);
  table[i] = acc;
}

struct AlEmbed {
  const float* slots;
  long long stride_v, stride_t;
  int V, T_all;
  const int *video_index, *start;
  int frame_offset;
  const float *Wv, *bv;        // vision_in_proj [d][C + 2], [d]
  const float *cls, *pos;      // [d], [L][d]
  const float *Wq, *table;     // q_in_proj.weight [d][E + 4] (its type columns E, E + 1), P [vocab][d]
  const int* tokens;           // [B][text_len]
  int vocab, E, question_len, mc_from;   // sequences b >= mc_from are multiple choice
  float* x;                    // [B][L][d]
  int B, T, N, C, text_len, d;
  long long rows;              // B T N
  int ntiles;
};

__device__ __forceinline__ bool al_frame(const AlEmbed& a, int b, int t, int& vid, int& f) {
  vid = a.video_index ? a.video_index[b] : b;
  const long long ff = (long long)(a.start ? a.start[b] : 0) + (long long)t * a.frame_offset;
  f = (int)ff;
  return vid >= 0 && vid < a.V && ff >= 0 && ff < a.T_all;
}

__global__ __launch_bounds__(AL_THREADS) void aloe_embed_kernel(const AlEmbed a) {
  extern __shared__ __attribute__((aligned(16))) char al_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, N = a.N, C = a.C, TN = T * N, d = a.d, L = 1 + TN + a.text_len;
  if ((int)blockIdx.x >= a.ntiles) {   // (workgroup-uniform) CLS and the text rows of one sequence
    const int b = (int)blockIdx.x - a.ntiles;
    float* xb = a.x + (long long)b * L * d;
    for (int c = tid; c < d; c += AL_THREADS) xb[c] = a.cls[c] + a.pos[c];
    for (int idx = tid; idx < a.text_len * d; idx += AL_THREADS) {
      const int j = idx / d, c = idx - j * d, row = 1 + TN + j;
      const int tok = a.tokens[(long long)b * a.text_len + j];
      const int type = (b >= a.mc_from && j < a.question_len) ? 0 : 1;   // cls_token / mc_choice_token = [0 1], mc_question_token = [1 0]
      const float p = (tok >= 0 && tok < a.vocab) ? a.table[(long long)tok * d + c] : 0.f;
      xb[(long long)row * d + c] = (p + a.Wq[(long long)c * (a.E + 4) + a.E + type]) + a.pos[(long long)row * d + c];
    }
    return;
  }
  const int ps = al_pitch(C);
  char* hi = al_smem;
  char* lo = al_smem + AL_ROWS * ps;
  const long long r0 = (long long)blockIdx.x * AL_ROWS;
  const int nrows = a.rows - r0 < AL_ROWS ? (int)(a.rows - r0) : AL_ROWS, rt_n = (nrows + 15) >> 4;
  const int c4n = C >> 2;
  for (int idx = tid; idx < rt_n * 16 * c4n; idx += AL_THREADS) {
    const int r = idx / c4n, c4 = idx - r * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < nrows) {
      const long long gr = r0 + r;
      const int b = (int)(gr / TN), rem = (int)(gr - (long long)b * TN), t = rem / N, n = rem - t * N;
      int vid, f;
      if (al_frame(a, b, t, vid, f))
        v = *reinterpret_cast<const f32x4*>(a.slots + (long long)vid * a.stride_v + (long long)f * a.stride_t + n * C + c4 * 4);
    }
    sf_split4(reinterpret_cast<__bf16*>(hi + r * ps), reinterpret_cast<__bf16*>(lo + r * ps), c4 * 4, v);
  }
  __syncthreads();
  // A operand: the rows (lane & 15 = row of the tile, k = 8 (lane >> 4) + 0..7); B operand: Wv[column lane & 15][the same k]; accumulator register e of
  // a lane = row 4 (lane >> 4) + e, column lane & 15 (phyre_readout.hip).  A column past d reads row d - 1 and is not stored.
  const int l15 = lane & 15, q = lane >> 4, wp = C + 2;
  for (int ct = wid; ct < (d + 15) / 16; ct += AL_WAVES) {
    const int col = ct * 16 + l15, colc = col < d ? col : d - 1;
    const float* wrow = a.Wv + (long long)colc * wp + 8 * q;   // (rows of C + 2 floats: 8-byte aligned)
    f32x4 acc[3];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < AL_KS; ++ks)
      if (ks < (C >> 5)) {
        const f32x2* w2 = reinterpret_cast<const f32x2*>(wrow + ks * 32);
        const f32x2 w0 = w2[0], w1 = w2[1], w2v = w2[2], w3 = w2[3];
        bf16x8 wh, wl;
        sf_split8(f32x4{w0[0], w0[1], w1[0], w1[1]}, f32x4{w2v[0], w2v[1], w3[0], w3[1]}, wh, wl);
#pragma unroll
        for (int rt = 0; rt < 3; ++rt)
          if (rt < rt_n) {
            const int o = (rt * 16 + l15) * ps + (ks * 32 + 8 * q) * 2;
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(hi + o), al = *reinterpret_cast<const bf16x8*>(lo + o);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wl, acc[rt], 0, 0, 0);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wh, acc[rt], 0, 0, 0);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wh, acc[rt], 0, 0, 0);
          }
      }
    if (col < d) {
      const float bias = a.Wv[(long long)col * wp + C + 1] + a.bv[col];   // vision_token = [0 1]: the second id column
#pragma unroll
      for (int rt = 0; rt < 3; ++rt)
        if (rt < rt_n)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = rt * 16 + q * 4 + e;
            if (r < nrows) {
              const long long gr = r0 + r;
              const int b = (int)(gr / TN), rem = (int)(gr - (long long)b * TN);
              a.x[((long long)b * L + 1 + rem) * d + col] = (acc[rt][e] + bias) + a.pos[(long long)(1 + rem) * d + col];
            }
          }
    }
  }
}

// qkv [B L][3 d] (q | k | v, head h at columns h hd ..) -> rows [0, nq) of every sequence of out [B L][d]; pad [B][text_len], 1 = a padded text position (token 1 + TN + j)
// TRAIN (aloe_train.hip): also lse [B][heads][L] = the row's log-sum-exp of the scaled, biased scores, and with thresh != 0 the dropout of
// nn.MultiheadAttention on P before P V: element ((b heads + h) L + query) L + key of the site-0 mask (dropout_mask.h), kept values * inv_keep.
template <bool TRAIN>
__global__ __launch_bounds__(AL_THREADS) void aloe_attn_kernel(const float* __restrict__ qkv, const unsigned char* __restrict__ pad, float* __restrict__ out,
                                                               int L, int nq, int text0, int text_len, int d, int hd, float scale, float* __restrict__ lse,
                                                               uint32_t sseed, uint32_t thresh, float inv_keep) {
  extern __shared__ __attribute__((aligned(16))) char al_smem[];
  __bf16* Kh = reinterpret_cast<__bf16*>(al_smem);
  __bf16* Kl = Kh + AL_MAXL * AL_KP;
  unsigned short* Vh = reinterpret_cast<unsigned short*>(Kl + AL_MAXL * AL_KP);
  unsigned short* Vl = Vh + AL_MAXHD * AL_VP;
  float* kbias = reinterpret_cast<float*>(Vl + AL_MAXHD * AL_VP);
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.x, b = blockIdx.y;
  const int LP = (L + 31) & ~31, nkt = LP >> 4;   // keys rounded up to a K = 32 step of the second product
  const float* base = qkv + (long long)b * L * 3 * d + h * hd;
  for (int idx = tid; idx < LP * 16; idx += AL_THREADS) {
    const int r = idx >> 4, c2 = idx & 15;
    f32x2 kv = {0.f, 0.f}, vv = {0.f, 0.f};
    if (r < L && 2 * c2 < hd) {
      const float* p = base + (long long)r * 3 * d + 2 * c2;
      kv = *reinterpret_cast<const f32x2*>(p + d);
      vv = *reinterpret_cast<const f32x2*>(p + 2 * d);
    }
    unsigned kh, kl, vh, vl;
    pl_split2(kv[0], kv[1], kh, kl);
    pl_split2(vv[0], vv[1], vh, vl);
    *reinterpret_cast<unsigned*>(Kh + r * AL_KP + 2 * c2) = kh;
    *reinterpret_cast<unsigned*>(Kl + r * AL_KP + 2 * c2) = kl;
    Vh[(2 * c2) * AL_VP + r] = (unsigned short)(vh & 0xffffu);
    Vh[(2 * c2 + 1) * AL_VP + r] = (unsigned short)(vh >> 16);
    Vl[(2 * c2) * AL_VP + r] = (unsigned short)(vl & 0xffffu);
    Vl[(2 * c2 + 1) * AL_VP + r] = (unsigned short)(vl >> 16);
  }
  for (int r = tid; r < AL_MAXL; r += AL_THREADS) {
    bool live = r < L;
    if (live && r >= text0 && r - text0 < text_len) live = pad[(long long)b * text_len + (r - text0)] == 0;
    kbias[r] = live ? 0.f : -INFINITY;
  }
  __syncthreads();
  const int l15 = lane & 15, q = lane >> 4;
  for (int qt = wid; qt * 16 < nq; qt += AL_WAVES) {   // (nq = L, or 1: the last layer, whose CLS row alone is read)
    const int qrow = qt * 16 + l15 < L ? qt * 16 + l15 : L - 1;
    bf16x8 qh, ql;
    {
      const float* qp = base + (long long)qrow * 3 * d + 8 * q;
      f32x8 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x2 t = {0.f, 0.f};
        if (8 * q + 2 * j < hd) t = *reinterpret_cast<const f32x2*>(qp + 2 * j);
        v[2 * j] = t[0] * scale;
        v[2 * j + 1] = t[1] * scale;
      }
      sf_split8(v, qh, ql);
    }
    // S^T tiles: acc[kt][e] = score of key 16 kt + 4 q + e for query l15
    f32x4 acc[AL_KT];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < AL_KT; ++kt)
      if (kt < nkt) {
        const int o = (kt * 16 + l15) * AL_KP + 8 * q;
        const bf16x8 kh = *reinterpret_cast<const bf16x8*>(Kh + o), kl = *reinterpret_cast<const bf16x8*>(Kl + o);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh, s, 0, 0, 0);
        s += *reinterpret_cast<const f32x4*>(kbias + kt * 16 + 4 * q);
        acc[kt] = s;
        m = fmaxf(fmaxf(m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));   // (finite: the CLS key is always live)
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < AL_KT; ++kt)
      if (kt < nkt) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = __expf(acc[kt][e] - m);
          acc[kt][e] = p;
          sum += p;
        }
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    if constexpr (TRAIN) {
      const int row = qt * 16 + l15;
      if (q == 0 && row < L) lse[((long long)b * gridDim.x + h) * L + row] = m + logf(sum);
    }
    // P V: contraction slot j of lane group q in step s is key 32 s + 4 q + j (j < 4) or 32 s + 16 + 4 q + j - 4: what the lane already holds
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < AL_KT / 2; ++s)
      if (2 * s < nkt) {
        bf16x8 ph, pl;
        f32x4 p0 = acc[2 * s] * inv, p1 = acc[2 * s + 1] * inv;
        if constexpr (TRAIN) {
          if (thresh) {
            const uint32_t e0 = (uint32_t)((((long long)b * gridDim.x + h) * L + qt * 16 + l15) * L + s * 32 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              p0[e] = sf_keep(sseed, e0 + e, thresh) ? p0[e] * inv_keep : 0.f;
              p1[e] = sf_keep(sseed, e0 + 16 + e, thresh) ? p1[e] * inv_keep : 0.f;
            }
          }
        }
        sf_split8(p0, p1, ph, pl);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          if (dt * 16 < hd) {
            const int vo = (dt * 16 + l15) * AL_VP + s * 32 + 4 * q;
            const bf16x4 h0 = *reinterpret_cast<const bf16x4*>(Vh + vo), h1 = *reinterpret_cast<const bf16x4*>(Vh + vo + 16);
            const bf16x4 l0 = *reinterpret_cast<const bf16x4*>(Vl + vo), l1 = *reinterpret_cast<const bf16x4*>(Vl + vo + 16);
            const bf16x8 vh = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7), vl = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vl, o[dt], 0, 0, 0);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, vh, o[dt], 0, 0, 0);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, vh, o[dt], 0, 0, 0);
          }
      }
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = qt * 16 + 4 * q + e, dc = dt * 16 + l15;
        if (row < nq && dc < hd) out[((long long)b * L + row) * d + h * hd + dc] = o[dt][e];
      }
  }
}

struct AlHead {
  const float* x;              // [B][L][d]; row 0 of every sequence is read
  const float *W1, *b1, *W2, *b2;   // [H][d], [H], [A][H], [A]
  float* logits;               // [B][A]
  int* answers;                // [B] or NULL
  const int *video_index, *start, *tokens;
  const unsigned char* pad;
  int V, T_all, T, frame_offset, vocab, text_len, B, L, d, H, A;
};

// Summation order (plain f32): hidden unit j = sf_wave_sum over the lanes of (fma chain over k = lane, lane + 64, ... ascending from 0) + b1[j]; output a the
// same over the hidden units + b2[a].  A sequence's logits do not depend on its place in the batch.
__global__ __launch_bounds__(AL_THREADS) void aloe_head_kernel(const AlHead a) {
  __shared__ float xs[AL_MAXD], hid[AL_MAXH], lg[AL_MAXA];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x, d = a.d, H = a.H, A = a.A;
  // the entry's video, frames and live tokens: anything outside its table -> NaN logits
  int bad = 0;
  if (tid == 0) {
    const int vid = a.video_index ? a.video_index[b] : b;
    const long long f0 = a.start ? a.start[b] : 0, f1 = f0 + (long long)(a.T - 1) * a.frame_offset;
    bad = !(vid >= 0 && vid < a.V && f0 >= 0 && f0 < a.T_all && f1 >= 0 && f1 < a.T_all);
  }
  for (int j = tid; j < a.text_len; j += AL_THREADS) {
    const int tok = a.tokens[(long long)b * a.text_len + j];
    if (a.pad[(long long)b * a.text_len + j] == 0 && !(tok >= 0 && tok < a.vocab)) bad = 1;
  }
  bad = __syncthreads_or(bad);
  for (int k = tid; k < d; k += AL_THREADS) xs[k] = a.x[(long long)b * a.L * d + k];
  __syncthreads();
  for (int j = wid; j < H; j += AL_WAVES) {
    const float* w = a.W1 + (long long)j * d;
    float acc = 0.f;
    for (int k = lane; k < d; k += 64) acc = fmaf(w[k], xs[k], acc);
    acc = sf_wave_sum(acc) + a.b1[j];
    if (lane == 0) hid[j] = fmaxf(acc, 0.f);
  }
  __syncthreads();
  for (int o = wid; o < A; o += AL_WAVES) {
    const float* w = a.W2 + (long long)o * H;
    float acc = 0.f;
    for (int k = lane; k < H; k += 64) acc = fmaf(w[k], hid[k], acc);
    acc = sf_wave_sum(acc) + a.b2[o];
    if (lane == 0) {
      acc = bad ? NAN : acc;
      lg[o] = acc;
      a.logits[(long long)b * A + o] = acc;
    }
  }
  __syncthreads();
  if (tid == 0 && a.answers) {
    int best = 0;
    if (A == 1) {
      best = lg[0] > 0.f ? 1 : 0;
    } else {
      for (int o = 1; o < A; ++o)
        if (lg[o] > lg[best]) best = o;   // the first index on ties
    }
    a.answers[b] = bad ? -1 : best;
  }
}

// counts: [0] descriptive correct, [1] descriptive questions, [2] multiple-choice questions all of whose choices are right, [3] multiple-choice questions,
// then (right, questions) of the subtypes explanatory 1, predictive 2, counterfactual 3 -- ten int32, ADDED
__device__ __forceinline__ double al_block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int s = AL_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ int al_block_count(int v, int* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int s = AL_THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const int r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(AL_THREADS) void aloe_score_kernel(const float* __restrict__ cls_logits, const int* __restrict__ cls_labels, int B1, int A,
                                                                const float* __restrict__ mc_logits, const float* __restrict__ mc_labels,
                                                                const int* __restrict__ mc_flag, int Bn, const int* __restrict__ mc_subtype, int Q,
                                                                float* __restrict__ losses, int* __restrict__ ques_correct, int* __restrict__ counts) {
  __shared__ double redd[AL_THREADS];
  __shared__ int redi[AL_THREADS];
  const int tid = threadIdx.x;
  {   // descriptive: mean cross-entropy, argmax == label
    double part = 0.0;
    int hit = 0;
    for (int b = tid; b < B1; b += AL_THREADS) {
      const float* x = cls_logits + (long long)b * A;
      const int y = cls_labels[b];
      float mx = x[0];
      int arg = 0;
      for (int o = 1; o < A; ++o)
        if (x[o] > mx) mx = x[o], arg = o;
      double s = 0.0;
      for (int o = 0; o < A; ++o) s += exp((double)x[o] - (double)mx);
      part += (y >= 0 && y < A) ? (double)mx + log(s) - (double)x[y] : (double)NAN;   // (a label outside the vocabulary: NaN, never an address)
      hit += arg == y ? 1 : 0;
    }
    const double tot = al_block_sum(part, redd, tid);
    const int hits = al_block_count(hit, redi, tid);
    if (tid == 0) {
      if (losses) losses[0] = B1 > 0 ? (float)(tot / B1) : 0.f;
      if (counts) counts[0] += hits, counts[1] += B1;
    }
  }
  {   // multiple choice: mean BCE with logits, per question "every choice right"
    for (int qi = tid; qi < Q; qi += AL_THREADS) ques_correct[qi] = 1;   // (torch's .all() of no choice is True)
    __syncthreads();
    double part = 0.0;
    for (int i = tid; i < Bn; i += AL_THREADS) {
      const double x = mc_logits[i], y = mc_labels[i];
      part += fmax(x, 0.0) - x * y + log1p(exp(-fabs(x)));
      const float pred = mc_logits[i] > 0.f ? 1.f : 0.f;
      const int f = mc_flag[i];
      if (pred != mc_labels[i] && f >= 0 && f < Q) ques_correct[f] = 0;   // (every writer stores the same value)
    }
    __threadfence_block();
    const double tot = al_block_sum(part, redd, tid);
    int c[4] = {0, 0, 0, 0}, n[4] = {0, 0, 0, 0};
    for (int qi = tid; qi < Q; qi += AL_THREADS) {
      const int ok = ques_correct[qi], st = mc_subtype ? mc_subtype[qi] : 0;
      c[0] += ok;
      n[0] += 1;
#pragma unroll
      for (int k = 1; k < 4; ++k) c[k] += st == k ? ok : 0, n[k] += st == k ? 1 : 0;
    }
    int cs[4], ns[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cs[k] = al_block_count(c[k], redi, tid), ns[k] = al_block_count(n[k], redi, tid);
    if (tid == 0) {
      if (losses) losses[1] = Bn > 0 ? (float)(tot / Bn) : 0.f;
      if (counts) {
        for (int k = 0; k < 4; ++k) counts[2 + 2 * k] += cs[k], counts[3 + 2 * k] += ns[k];
      }
    }
  }
}

inline bool al_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define AL_LIMITS                                                                                                                                   \
  "1 <= num_slots <= 16, slot_size a multiple of 32 in [32, 256], T >= 1, text_len >= 1, 1 + T * num_slots + text_len <= 256, d_model = heads * "    \
  "head_dim <= 256 and a multiple of 4, head_dim even in [4, 32], ffn a multiple of 64 in [64, 1024], 1 <= num_layers <= 32"

// the token rows [B][L][d] of a batch whose sequences b >= mc_from are multiple choice (arguments validated by the caller)
int sf_aloe_embed_ex(const sf_aloe* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index, const int* start,
                     int frame_offset, const int* tokens, int mc_from, float* x, int B, hipStream_t st) {
  AlEmbed a;
  a.slots = slots; a.stride_v = stride_v; a.stride_t = stride_t; a.V = V; a.T_all = T_all; a.video_index = video_index; a.start = start;
  a.frame_offset = frame_offset; a.Wv = m->vision_w; a.bv = m->vision_b; a.cls = m->cls; a.pos = m->pos; a.Wq = m->q_in_proj_w; a.table = m->text_table;
  a.tokens = tokens; a.vocab = m->vocab; a.E = m->emb_dim; a.question_len = m->question_len; a.mc_from = mc_from; a.x = x;
  a.B = B; a.T = m->T; a.N = m->num_slots; a.C = m->slot_size; a.text_len = m->text_len; a.d = m->d_model;
  a.rows = (long long)B * a.T * a.N;
  a.ntiles = (int)((a.rows + AL_ROWS - 1) / AL_ROWS);
  const size_t lds = al_embed_lds(a.C);
  SF_TRY(sf_ensure_dyn_lds((const void*)aloe_embed_kernel, lds));
  hipLaunchKernelGGL(aloe_embed_kernel, dim3((unsigned)(a.ntiles + B)), dim3(AL_THREADS), lds, st, a);
  SF_CHECK_LAUNCH();
  return 0;
}
// the attention launch of a training layer: every row a query; lse [B][heads][L]; thresh 0: no mask is evaluated
int sf_aloe_attn_train_ex(const float* qkv, const unsigned char* pad, float* out, float* lse, int B, int L, int text0, int text_len, int d, int heads,
                          uint32_t sseed, uint32_t thresh, float inv_keep, hipStream_t st) {
  SF_TRY(sf_ensure_dyn_lds((const void*)aloe_attn_kernel<true>, AL_ATTN_LDS));
  const int hd = d / heads;
  hipLaunchKernelGGL(aloe_attn_kernel<true>, dim3((unsigned)heads, (unsigned)B), dim3(AL_THREADS), AL_ATTN_LDS, st, qkv, pad, out, L, L, text0, text_len, d, hd,
                     1.0f / sqrtf((float)hd), lse, sseed, thresh, inv_keep);
  SF_CHECK_LAUNCH();
  return 0;
}

extern "C" {

int sf_aloe_ok(int num_slots, int slot_size, int T, int text_len, int d_model, int num_heads, int ffn, int num_layers) {
  return al_ok(num_slots, slot_size, T, text_len, d_model, num_heads, ffn, num_layers) ? 1 : 0;
}

size_t sf_aloe_workspace_bytes(int B, int num_slots, int T, int text_len, int d_model, int ffn) {
  if (B < 1 || B > 65535 || d_model < 4 || d_model > AL_MAXD || d_model % 4 != 0 || ffn < 64 || ffn > 1024) return 0;
  if (num_slots < 1 || num_slots > 16 || T < 1 || T > AL_MAXL || text_len < 1 || text_len > AL_MAXL || 1 + T * num_slots + text_len > AL_MAXL) return 0;
  const size_t M = (size_t)B * (1 + (size_t)T * num_slots + text_len);
  return M * ((size_t)6 * d_model + ffn) * sizeof(float);   // x, y, attention rows [M][d]; q|k|v [M][3 d]; hidden [M][ffn]
}

int sf_aloe_text_table_f32(const float* q_embedding, const float* q_in_proj_w, const float* q_in_proj_b, float* table, int vocab, int emb_dim, int d_model,
                           void* stream) {
  SF_REQUIRE(q_embedding && q_in_proj_w && q_in_proj_b && table, "sf_aloe_text_table_f32: null pointer");
  SF_REQUIRE(vocab >= 1 && emb_dim >= 1 && d_model >= 1 && d_model <= AL_MAXD, "sf_aloe_text_table_f32: vocab >= 1, emb_dim >= 1, 1 <= d_model <= 256");
  const long long n = (long long)vocab * d_model;
  SF_REQUIRE(n < (1LL << 31), "sf_aloe_text_table_f32: table too large");
  hipLaunchKernelGGL(aloe_text_table_kernel, dim3((unsigned)((n + AL_THREADS - 1) / AL_THREADS)), dim3(AL_THREADS), 0, (hipStream_t)stream, q_embedding,
                     q_in_proj_w, q_in_proj_b, table, vocab, emb_dim, d_model);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_aloe_fwd_f32(const sf_aloe* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index, const int* start,
                    int frame_offset, const int* tokens, const unsigned char* pad_mask, int multiple_choice, const float* head_w1, const float* head_b1,
                    const float* head_w2, const float* head_b2, int mlp_hidden, int num_outputs, float* logits, int* answers, int B, void* workspace,
                    size_t workspace_bytes, void* stream) {
  SF_REQUIRE(m && slots && tokens && pad_mask && head_w1 && head_b1 && head_w2 && head_b2 && logits && workspace, "sf_aloe_fwd_f32: null pointer");
  SF_REQUIRE(m->cls && m->pos && m->vision_w && m->vision_b && m->q_in_proj_w && m->text_table && m->layers, "sf_aloe_fwd_f32: null pointer in sf_aloe");
  const int N = m->num_slots, C = m->slot_size, T = m->T, TL = m->text_len, d = m->d_model, nh = m->num_heads, ffn = m->ffn_dim, nl = m->num_layers;
  SF_REQUIRE(al_ok(N, C, T, TL, d, nh, ffn, nl), "sf_aloe_fwd_f32: unsupported shape (" AL_LIMITS ")");
  SF_REQUIRE(m->vocab >= 1 && m->emb_dim >= 1 && m->question_len >= 0, "sf_aloe_fwd_f32: vocab >= 1, emb_dim >= 1, question_len >= 0");
  SF_REQUIRE(mlp_hidden >= 1 && mlp_hidden <= AL_MAXH && num_outputs >= 1 && num_outputs <= AL_MAXA, "sf_aloe_fwd_f32: 1 <= mlp_hidden, num_outputs <= 1024");
  SF_REQUIRE(B >= 1 && B <= 65535 && V >= 1 && T_all >= 1, "sf_aloe_fwd_f32: 1 <= B <= 65535, V >= 1, T_all >= 1");
  SF_REQUIRE(stride_t >= (long long)N * C && stride_t % 4 == 0 && stride_v >= 0 && stride_v % 4 == 0,
             "sf_aloe_fwd_f32: frame stride >= N * C, strides multiples of 4");
  SF_REQUIRE(video_index || B <= V, "sf_aloe_fwd_f32: B > V without a video_index");
  SF_REQUIRE(al_al16(slots) && al_al16(m->vision_w) && al_al16(workspace), "sf_aloe_fwd_f32: slots, vision_w and the workspace must be 16-byte aligned");
  SF_REQUIRE(workspace_bytes >= sf_aloe_workspace_bytes(B, N, T, TL, d, ffn), "sf_aloe_fwd_f32: workspace too small");
  SF_REQUIRE(sf_get_precision() == 1, "sf_aloe_fwd_f32: split-bf16 mode only (the attention and embedding products have no other form)");
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer& w = m->layers[l];
    SF_REQUIRE(w.norm1_g && w.norm1_b && w.in_proj_w && w.in_proj_b && w.out_proj_w && w.out_proj_b && w.norm2_g && w.norm2_b && w.lin1_w && w.lin1_b &&
                   w.lin2_w && w.lin2_b,
               "sf_aloe_fwd_f32: null pointer in a layer");
  }
  const int L = 1 + T * N + TL, hd = d / nh;
  const long long Mll = (long long)B * L;
  SF_REQUIRE(Mll * (3 * d > ffn ? 3 * d : ffn) < (1LL << 31), "sf_aloe_fwd_f32: batch too large for one call");
  const int M = (int)Mll;
  float* x = static_cast<float*>(workspace);
  float* y = x + (size_t)M * d;
  float* att = y + (size_t)M * d;
  float* qkv = att + (size_t)M * d;
  float* hid = qkv + (size_t)M * 3 * d;
  hipStream_t st = (hipStream_t)stream;
  SF_TRY(sf_aloe_embed_ex(m, slots, stride_v, stride_t, V, T_all, video_index, start, frame_offset, tokens, multiple_choice ? 0 : B, x, B, st));
  SF_TRY(sf_ensure_dyn_lds((const void*)aloe_attn_kernel<false>, AL_ATTN_LDS));
  const float scale = 1.0f / sqrtf((float)hd);
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer& w = m->layers[l];
    if (l < nl - 1) {
      SF_TRY(sf_linear_ex(x, sf_rows(d), w.in_proj_w, w.in_proj_b, w.norm1_g, w.norm1_b, 1e-5f, nullptr, sf_rows(3 * d), 0, qkv, sf_rows(3 * d), M, 3 * d, d, 0, st));
      hipLaunchKernelGGL(aloe_attn_kernel<false>, dim3((unsigned)nh, (unsigned)B), dim3(AL_THREADS), AL_ATTN_LDS, st, qkv, pad_mask, att, L, L, 1 + T * N, TL, d, hd, scale,
                         (float*)nullptr, 0u, 0u, 1.f);
      SF_CHECK_LAUNCH();
      SF_TRY(sf_linear_ex(att, sf_rows(d), w.out_proj_w, w.out_proj_b, nullptr, nullptr, 0.f, x, sf_rows(d), 0, y, sf_rows(d), M, d, d, 0, st));
      SF_TRY(sf_linear_ex(y, sf_rows(d), w.lin1_w, w.lin1_b, w.norm2_g, w.norm2_b, 1e-5f, nullptr, sf_rows(ffn), 0, hid, sf_rows(ffn), M, ffn, d, 1, st));
      SF_TRY(sf_linear_ex(hid, sf_rows(ffn), w.lin2_w, w.lin2_b, nullptr, nullptr, 0.f, y, sf_rows(d), 0, x, sf_rows(d), M, d, ffn, 0, st));
      continue;
    }
    // the last layer: only its CLS rows are read.  k | v for every row (columns d .. 3 d of q|k|v), q and everything behind the attention for the B
    // CLS rows alone: row b of those GEMMs is row b L of the buffers (a leading dimension of L rows), the hidden rows are compact
    const SfRowMap kv_out = SfRowMap{0, 0, 3 * d, d};
    SF_TRY(sf_linear_ex(x, sf_rows(d), w.in_proj_w + (size_t)d * d, w.in_proj_b + d, w.norm1_g, w.norm1_b, 1e-5f, nullptr, kv_out, 0, qkv, kv_out, M, 2 * d, d, 0, st));
    SF_TRY(sf_linear_ex(x, sf_rows(L * d), w.in_proj_w, w.in_proj_b, w.norm1_g, w.norm1_b, 1e-5f, nullptr, sf_rows(3 * d * L), 0, qkv, sf_rows(3 * d * L), B, d, d, 0, st));
    hipLaunchKernelGGL(aloe_attn_kernel<false>, dim3((unsigned)nh, (unsigned)B), dim3(AL_THREADS), AL_ATTN_LDS, st, qkv, pad_mask, att, L, 1, 1 + T * N, TL, d, hd, scale,
                       (float*)nullptr, 0u, 0u, 1.f);
    SF_CHECK_LAUNCH();
    SF_TRY(sf_linear_ex(att, sf_rows(L * d), w.out_proj_w, w.out_proj_b, nullptr, nullptr, 0.f, x, sf_rows(L * d), 0, y, sf_rows(L * d), B, d, d, 0, st));
    SF_TRY(sf_linear_ex(y, sf_rows(L * d), w.lin1_w, w.lin1_b, w.norm2_g, w.norm2_b, 1e-5f, nullptr, sf_rows(ffn), 0, hid, sf_rows(ffn), B, ffn, d, 1, st));
    SF_TRY(sf_linear_ex(hid, sf_rows(ffn), w.lin2_w, w.lin2_b, nullptr, nullptr, 0.f, y, sf_rows(L * d), 0, x, sf_rows(L * d), B, d, ffn, 0, st));
  }
  AlHead hp;
  hp.x = x; hp.W1 = head_w1; hp.b1 = head_b1; hp.W2 = head_w2; hp.b2 = head_b2; hp.logits = logits; hp.answers = answers;
  hp.video_index = video_index; hp.start = start; hp.tokens = tokens; hp.pad = pad_mask; hp.V = V; hp.T_all = T_all; hp.T = T;
  hp.frame_offset = frame_offset; hp.vocab = m->vocab; hp.text_len = TL; hp.B = B; hp.L = L; hp.d = d; hp.H = mlp_hidden; hp.A = num_outputs;
  hipLaunchKernelGGL(aloe_head_kernel, dim3((unsigned)B), dim3(AL_THREADS), 0, st, hp);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_aloe_score_f32(const float* cls_logits, const int* cls_labels, int B1, int num_answers, const float* mc_logits, const float* mc_labels,
                      const int* mc_flag, int Bn, const int* mc_subtype, int Q, float* losses, int* ques_correct, int* counts, void* stream) {
  SF_REQUIRE(B1 >= 0 && Bn >= 0 && Q >= 0, "sf_aloe_score_f32: B1 >= 0, Bn >= 0, Q >= 0");
  SF_REQUIRE(B1 == 0 || (cls_logits && cls_labels && num_answers >= 1), "sf_aloe_score_f32: descriptive logits need labels and num_answers >= 1");
  SF_REQUIRE(Bn == 0 || (mc_logits && mc_labels && mc_flag), "sf_aloe_score_f32: multiple-choice logits need labels and mc_flag");
  SF_REQUIRE(Q == 0 || ques_correct, "sf_aloe_score_f32: Q > 0 needs ques_correct");
  hipLaunchKernelGGL(aloe_score_kernel, dim3(1), dim3(AL_THREADS), 0, (hipStream_t)stream, cls_logits, cls_labels, B1, num_answers, mc_logits, mc_labels,
                     mc_flag, Bn, mc_subtype, Q, losses, ques_correct, counts);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

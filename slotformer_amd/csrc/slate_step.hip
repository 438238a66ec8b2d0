// One launch per generated token of the STEVE slot-conditioned Transformer decoder (greedy generation,
// steve_transformer.py:305-333): the whole token step -- embedding, every decoder block (self-attention over the K/V
// cache, cross-attention to the slots, FFN), the final LayerNorm, the vocabulary head and the argmax -- in one kernel.
//
// A workgroup owns FR consecutive frames for the whole step and talks to no other workgroup: the only state that
// crosses launches is the K/V cache and the token array, ordered by the stream.  No flags, spins, atomics or
// cooperative launch.  Activations of a frame stay in LDS; the weights (torch layouts, [N][K] row-major) are streamed
// with 16-byte loads, eight lanes per weight row (128 contiguous bytes per row and load), and shared by the FR frames.
// Arithmetic is plain fp32 FMA.
//
// The head's epilogue has two compile-time options (sf_slate_generate_tok_opts_f32), both built on the counter-based Gumbel noise of gumbel_noise.h
// added to a logit while it is still in a register: the soft rows (the Gumbel-softmax relaxation times the first dVAE decoder block, as an online
// softmax over the vocabulary sweep: 64 numbers per token instead of V) and Gumbel-max sampling of the token.  The greedy instantiation is the code
// it was without them.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "gumbel_noise.h"
#include <cmath>

namespace {
constexpr int ST_NT = 1024;          // threads per workgroup
constexpr int ST_NW = ST_NT / 64;    // waves
constexpr int ST_MAXL = 8;           // decoder blocks the kernel argument holds
constexpr int ST_SOFT_C = 64;        // channels of a soft row (the first dVAE decoder block's width): eight per lane of a weight-row group
constexpr int ST_SOFT_REC = ST_SOFT_C + 2;   // a wave's soft record per frame: running max, sum, weighted channels

struct StepBlock {
  const float *ln1_g, *ln1_b, *wqkv, *wo, *ln2_g, *ln2_b, *wq_c, *wo_c, *ln3_g, *ln3_b, *w1, *b1, *w2, *b2;
  const float* memkv;   // [B][N][2d]: cross-attention keys | values of the slots (projected once before the loop)
  float* cache;         // [B][steps][2d]: self-attention keys | values of the tokens generated so far
  int is_first;
};
struct StepArgs {
  StepBlock blk[ST_MAXL];
  const float *tok_emb, *pos_emb, *lnf_g, *lnf_b, *head_w;
  long long* tokens;   // [B][steps]
  float* logits;       // [B][steps][V] or NULL
  int d, H, NL, V, N, B, steps, t;
  // the noise epilogues of the head (SOFT / SAMPLE instantiations only)
  float* soft_rows;       // [B][steps][ST_SOFT_C]
  const float* conv0_t;   // [V][ST_SOFT_C]
  float soft_scale, inv_temperature;
  uint32_t soft_sseed, sample_sseed;
  long long row_base;
};

__device__ __forceinline__ float dot4(const f32x4 w, const f32x4 x, float acc) {
  acc = fmaf(w[0], x[0], acc);
  acc = fmaf(w[1], x[1], acc);
  acc = fmaf(w[2], x[2], acc);
  return fmaf(w[3], x[3], acc);
}

// y[fr][n] = sum_k W[n][k] * xin[fr][k] for n < N, fr < FR; K a multiple of 32.  Eight lanes share a row of W (lane l takes the 16-byte pieces
// l, l + 8, ...), the inputs come from LDS (rows xs floats apart).  epi(fr, n, value) runs on the first lane of each group of eight; with ALL,
// epi(n, values[FR]) runs once per row on all eight lanes instead (sf_sum8 leaves the same bits in each of them).
template <int FR, bool ALL = false, class Epi>
__device__ __forceinline__ void gemv_rows(const float* __restrict__ W, int N, int K, const float* xin, int xs, Epi epi) {
  const int l = threadIdx.x & 7, g = threadIdx.x >> 3;
  const int K4 = K >> 2, KI = K >> 5;
  const f32x4* x4 = (const f32x4*)xin + l;
  const int xs4 = xs >> 2;
  for (int n = g; n < N; n += ST_NT / 8) {
    const f32x4* wr = (const f32x4*)W + (long long)n * K4 + l;
    float acc[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) acc[f] = 0.f;
    int i = 0;
    for (; i + 4 <= KI; i += 4) {
      const f32x4 w0 = wr[i * 8], w1 = wr[i * 8 + 8], w2 = wr[i * 8 + 16], w3 = wr[i * 8 + 24];
#pragma unroll
      for (int f = 0; f < FR; ++f) {
        const f32x4* xr = x4 + f * xs4 + i * 8;
        acc[f] = dot4(w0, xr[0], acc[f]);
        acc[f] = dot4(w1, xr[8], acc[f]);
        acc[f] = dot4(w2, xr[16], acc[f]);
        acc[f] = dot4(w3, xr[24], acc[f]);
      }
    }
    for (; i < KI; ++i) {
      const f32x4 w0 = wr[i * 8];
#pragma unroll
      for (int f = 0; f < FR; ++f) acc[f] = dot4(w0, x4[f * xs4 + i * 8], acc[f]);
    }
#pragma unroll
    for (int f = 0; f < FR; ++f) acc[f] = sf_sum8(acc[f]);
    if constexpr (ALL) {
      epi(n, acc);
    } else {
      if (l == 0) {
#pragma unroll
        for (int f = 0; f < FR; ++f) epi(f, n, acc[f]);
      }
    }
  }
}

// LayerNorm of row f (f < FR) by wave f: y = (x - mean) * rstd * g + b; with also_x the result replaces x too
__device__ __forceinline__ void ln_rows(float* x, float* y, int stride, int FR, const float* __restrict__ g, const float* __restrict__ b, int d,
                                        bool also_x) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (w >= FR) return;
  float* xr = x + w * stride;
  float* yr = y + w * stride;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += xr[c];
  const float mean = sf_wave_sum(s) / (float)d;
  float q = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float v = xr[c] - mean;
    q = fmaf(v, v, q);
  }
  const float rstd = 1.0f / sqrtf(sf_wave_sum(q) / (float)d + 1e-5f);
  for (int c = lane; c < d; c += 64) {
    const float v = (xr[c] - mean) * rstd * g[c] + b[c];
    yr[c] = v;
    if (also_x) xr[c] = v;
  }
}

// One wave's share of softmax(q . k_j) v_j over the keys j = first * 16 + (lane / 4), + stride * 16, ... < nkeys of one head: four lanes per key,
// lane (l & 3) holding the 16-byte pieces (l & 3) + 4 i of the head's HD16 * 16 channels.  q (LDS) is already scaled.  Writes the wave's record
// {running max, sum of weights, weighted values[hd]} to part (LDS); an empty share writes max = -inf.
template <int HD16>
__device__ __forceinline__ void attn_wave(const float* q, const float* __restrict__ kbase, const float* __restrict__ vbase, int ld, int nkeys,
                                          int first, int stride, float* part) {
  const int lane = threadIdx.x & 63, l4 = lane & 3, grp = lane >> 2;
  f32x4 qv[HD16], acc[HD16];
#pragma unroll
  for (int i = 0; i < HD16; ++i) {
    qv[i] = ((const f32x4*)q)[l4 + 4 * i];
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float m = -INFINITY, lsum = 0.f;
  for (int j = first * 16 + grp; j < nkeys; j += stride * 16) {
    const f32x4* kr = (const f32x4*)(kbase + (long long)j * ld) + l4;
    const f32x4* vr = (const f32x4*)(vbase + (long long)j * ld) + l4;
    f32x4 kk[HD16], vv[HD16];
#pragma unroll
    for (int i = 0; i < HD16; ++i) {
      kk[i] = kr[4 * i];
      vv[i] = vr[4 * i];
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < HD16; ++i) s = dot4(qv[i], kk[i], s);
    s = sf_group_sum<4>(s);
    const float mn = fmaxf(m, s);
    const float corr = expf(m - mn), p = expf(s - mn);
    lsum = fmaf(lsum, corr, p);
#pragma unroll
    for (int i = 0; i < HD16; ++i) acc[i] = acc[i] * corr + vv[i] * p;
    m = mn;
  }
  const float M = sf_wave_max(m);
  const float sc = (m == -INFINITY) ? 0.f : expf(m - M);
  lsum *= sc;
#pragma unroll
  for (int o = 4; o < 64; o <<= 1) lsum += __shfl_xor(lsum, o, 64);
#pragma unroll
  for (int i = 0; i < HD16; ++i) {
    f32x4 a = acc[i] * sc;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = a[e];
#pragma unroll
      for (int o = 4; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
      a[e] = v;
    }
    if (grp == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) part[2 + (l4 + 4 * i) * 4 + e] = a[e];
    }
  }
  if (lane == 0) {
    part[0] = M;
    part[1] = lsum;
  }
}

// Attention of one query row per (frame, head) pair over keys in global memory (+ one current key / value in LDS when kcur != NULL):
// the waves of the workgroup split the pairs, or the keys of a pair, then one wave per pair merges the records.  Ends with every att row written
// and the workgroup synchronised.  What a frame's row holds depends on FR (how its keys are split) but not on the other frames of the call.
template <int HD16>
__device__ __forceinline__ void attention(const float* q, int qs, const float* kcur, const float* vcur, const float* __restrict__ kglob,
                                          long long frame_stride, int ld, int voff, int nkeys, int npairs, int pairs_full, int H, int b0,
                                          float* att, float* part) {
  constexpr int hd = HD16 * 16, PS = hd + 2;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // waves per pair from the pairs of a FULL workgroup: a frame's sums are added in the same order in a ragged last workgroup
  const int S = pairs_full >= ST_NW ? 1 : ST_NW / pairs_full;
  if (S == 1) {
    for (int p = w; p < npairs; p += ST_NW) {
      const int f = p / H, h = p - f * H;
      const float* kb = kglob + (long long)(b0 + f) * frame_stride + h * hd;
      attn_wave<HD16>(q + f * qs + h * hd, kb, kb + voff, ld, nkeys, 0, 1, part + p * PS);
    }
  } else {
    const int p = w / S, s = w - p * S;
    if (p < npairs) {
      const int f = p / H, h = p - f * H;
      const float* kb = kglob + (long long)(b0 + f) * frame_stride + h * hd;
      attn_wave<HD16>(q + f * qs + h * hd, kb, kb + voff, ld, nkeys, s, S, part + (p * S + s) * PS);
    }
  }
  __syncthreads();
  for (int p = w; p < npairs; p += ST_NW) {
    const int f = p / H, h = p - f * H;
    const bool on = lane < hd;
    float M = -INFINITY;
    if (kcur) {
      const float v = on ? q[f * qs + h * hd + lane] * kcur[f * qs + h * hd + lane] : 0.f;
      M = sf_wave_sum(v);
    }
    const float st = M;
    for (int s = 0; s < S; ++s) M = fmaxf(M, part[(p * S + s) * PS]);
    float num = 0.f, den = 0.f;
    if (kcur) {
      den = expf(st - M);
      num = on ? den * vcur[f * qs + h * hd + lane] : 0.f;
    }
    for (int s = 0; s < S; ++s) {
      const float* pr = part + (p * S + s) * PS;
      if (pr[0] > -INFINITY) {
        const float e = expf(pr[0] - M);
        den = fmaf(e, pr[1], den);
        if (on) num = fmaf(e, pr[2 + lane], num);
      }
    }
    if (on) att[f * qs + h * hd + lane] = num / den;
  }
  __syncthreads();
}

// The head's epilogue is chosen at compile time.  Neither flag: the greedy step.  SOFT: next to the greedy (or sampled) choice, the soft row
// y[c] = sum_v softmax_v((l_v + G(soft_seed, r V + v)) * soft_scale) * Wt[v][c] of every frame, online over the vocabulary sweep.  SAMPLE: the token
// is argmax_v(l_v * inv_temperature + G(sample_seed, r V + v)) -- Gumbel-max, an exact draw from softmax(l / T).  r = row_base + b * steps + t.
template <int FR, int HD16, bool SOFT, bool SAMPLE>
__global__ __launch_bounds__(ST_NT) void slate_step_kernel(const StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float st_lds[];
  constexpr int hd = HD16 * 16;
  const int d = a.d, H = a.H, V = a.V, t = a.t, tid = threadIdx.x;
  const int b0 = blockIdx.x * FR;
  const int nf = (a.B - b0) < FR ? (a.B - b0) : FR;   // frames of this workgroup that exist; the others touch no global memory
  // LDS: per buffer FR rows
  float* x = st_lds;                // [FR][d]   the residual stream
  float* xn = x + FR * d;           // [FR][d]   LayerNorm output
  float* qkv = xn + FR * d;         // [FR][3d]  q | k | v of the new token (row stride d for q, k at +FR*d, v at +2*FR*d)
  float* att = qkv + 3 * FR * d;    // [FR][d]
  float* hid = att + FR * d;        // [FR][4d]
  float* part = hid + 4 * FR * d;   // attention records
  const int nparts = (FR * H > ST_NW ? FR * H : ST_NW);
  float* bestv = part + nparts * (hd + 2);   // [ST_NW][FR]
  int* besti = (int*)(bestv + ST_NW * FR);   // [ST_NW][FR]
  float* softrec = (float*)(besti + ST_NW * FR);   // SOFT only: [ST_NW][FR][ST_SOFT_REC]
  float* qb = qkv;
  float* kb = qkv + FR * d;
  float* vb = qkv + 2 * FR * d;

  // token t-1 (BOS = id V at t = 0) + position t; rows of absent frames are zero
  for (int i = tid; i < FR * d; i += ST_NT) {
    const int f = i / d, c = i - f * d;
    float v = 0.f;
    if (f < nf) {
      long long tok = V;
      if (t > 0) {
        tok = a.tokens[(long long)(b0 + f) * a.steps + (t - 1)];
        tok = tok < 0 ? 0 : (tok > V ? V : tok);
      }
      v = a.tok_emb[tok * d + c] + a.pos_emb[(long long)t * d + c];
    }
    x[i] = v;
  }
  __syncthreads();
  const float qscale = 1.0f / sqrtf((float)hd);
  for (int L = 0; L < a.NL; ++L) {
    const StepBlock& k = a.blk[L];
    // self-attention
    ln_rows(x, xn, d, FR, k.ln1_g, k.ln1_b, d, k.is_first != 0);
    __syncthreads();
    {
      float* crow = k.cache + ((long long)b0 * a.steps + t) * 2 * d;
      const long long cfs = (long long)a.steps * 2 * d;
      gemv_rows<FR>(k.wqkv, 3 * d, d, xn, d, [&](int f, int n, float v) {
        if (n < d) {
          qb[f * d + n] = v * qscale;
        } else {
          qkv[(n / d) * FR * d + f * d + (n % d)] = v;
          if (f < nf) crow[f * cfs + (n - d)] = v;
        }
      });
    }
    __syncthreads();
    attention<HD16>(qb, d, kb, vb, k.cache, (long long)a.steps * 2 * d, 2 * d, d, t, nf * H, FR * H, H, b0, att, part);
    gemv_rows<FR>(k.wo, d, d, att, d, [&](int f, int n, float v) { x[f * d + n] += v; });
    __syncthreads();
    // cross-attention to the slots
    ln_rows(x, xn, d, FR, k.ln2_g, k.ln2_b, d, false);
    __syncthreads();
    gemv_rows<FR>(k.wq_c, d, d, xn, d, [&](int f, int n, float v) { qb[f * d + n] = v * qscale; });
    __syncthreads();
    attention<HD16>(qb, d, nullptr, nullptr, k.memkv, (long long)a.N * 2 * d, 2 * d, d, a.N, nf * H, FR * H, H, b0, att, part);
    gemv_rows<FR>(k.wo_c, d, d, att, d, [&](int f, int n, float v) { x[f * d + n] += v; });
    __syncthreads();
    // FFN
    ln_rows(x, xn, d, FR, k.ln3_g, k.ln3_b, d, false);
    __syncthreads();
    gemv_rows<FR>(k.w1, 4 * d, d, xn, d, [&](int f, int n, float v) { hid[f * 4 * d + n] = fmaxf(v + k.b1[n], 0.f); });
    __syncthreads();
    gemv_rows<FR>(k.w2, d, 4 * d, hid, 4 * d, [&](int f, int n, float v) { x[f * d + n] += v + k.b2[n]; });
    __syncthreads();
  }
  // final LayerNorm, vocabulary head, argmax (lowest index among equal maxima)
  ln_rows(x, xn, d, FR, a.lnf_g, a.lnf_b, d, false);
  __syncthreads();
  float best[FR];
  int bi[FR];
#pragma unroll
  for (int f = 0; f < FR; ++f) {
    best[f] = -INFINITY;
    bi[f] = 0x7fffffff;
  }
  {
    float* lrow = a.logits ? a.logits + ((long long)b0 * a.steps + t) * V : nullptr;
    const long long lfs = (long long)a.steps * V;
    if constexpr (!SOFT && !SAMPLE) {
      gemv_rows<FR>(a.head_w, V, d, xn, d, [&](int f, int n, float v) {
        if (lrow && f < nf) lrow[f * lfs + n] = v;
        if (v > best[f]) {   // n grows within a lane: the first maximum is kept
          best[f] = v;
          bi[f] = n;
        }
      });
    } else {
      const int l = tid & 7;
      // element index of (frame f, word 0) in the noise streams: below 2^32 for every frame that exists (checked by the host)
      uint32_t nbase[FR];
#pragma unroll
      for (int f = 0; f < FR; ++f) nbase[f] = (uint32_t)((a.row_base + (long long)(b0 + f) * a.steps + t) * V);
      // this lane's share of the soft records: channels 8 l .. 8 l + 7; max and sum are the same in the eight lanes of a group
      float sm[FR], ss[FR];
      f32x4 sa0[FR], sa1[FR];
#pragma unroll
      for (int f = 0; f < FR; ++f) {
        sm[f] = -INFINITY;
        ss[f] = 0.f;
        sa0[f] = sa1[f] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      gemv_rows<FR, true>(a.head_w, V, d, xn, d, [&](int n, const float* v) {
        f32x4 w0, w1;
        if constexpr (SOFT) {
          const f32x4* wt = (const f32x4*)(a.conv0_t + (long long)n * ST_SOFT_C) + 2 * l;
          w0 = wt[0];
          w1 = wt[1];
        }
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          if (l == 0) {
            if (lrow && f < nf) lrow[f * lfs + n] = v[f];
            float score = v[f];
            if constexpr (SAMPLE) score = v[f] * a.inv_temperature + sf_gumbel(nbase[f] + (uint32_t)n, a.sample_sseed);
            if (score > best[f]) {   // n grows within a lane: the first maximum is kept
              best[f] = score;
              bi[f] = n;
            }
          }
          if constexpr (SOFT) {
            const float z = (v[f] + sf_gumbel(nbase[f] + (uint32_t)n, a.soft_sseed)) * a.soft_scale;
            const float mn = fmaxf(sm[f], z);
            const float corr = expf(sm[f] - mn), p = expf(z - mn);   // first entry: exp(-inf) = 0
            ss[f] = fmaf(ss[f], corr, p);
            sa0[f] = sa0[f] * corr + w0 * p;
            sa1[f] = sa1[f] * corr + w1 * p;
            sm[f] = mn;
          }
        }
      });
      if constexpr (SOFT) {
        // merge the eight groups of the wave (lanes l, l + 8, ..., l + 56), then one record per wave and frame to LDS.  A group that saw no word
        // holds max = -inf and weighs 0, whatever its partner holds.
        const int w = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          float m = sm[f], s = ss[f];
          f32x4 c0 = sa0[f], c1 = sa1[f];
#pragma unroll
          for (int o = 8; o < 64; o <<= 1) {
            const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
            f32x4 o0, o1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              o0[e] = __shfl_xor(c0[e], o, 64);
              o1[e] = __shfl_xor(c1[e], o, 64);
            }
            const float M = fmaxf(m, om);
            const float ea = (m == -INFINITY) ? 0.f : expf(m - M), eb = (om == -INFINITY) ? 0.f : expf(om - M);
            // the lower lane's record first in every sum, so that both partners hold the same bits
            const bool lo = (lane & o) == 0;
            const float e1 = lo ? ea : eb, e2 = lo ? eb : ea;
            s = (lo ? s : os) * e1 + (lo ? os : s) * e2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              c0[e] = (lo ? c0[e] : o0[e]) * e1 + (lo ? o0[e] : c0[e]) * e2;
              c1[e] = (lo ? c1[e] : o1[e]) * e1 + (lo ? o1[e] : c1[e]) * e2;
            }
            m = M;
          }
          float* rec = softrec + (w * FR + f) * ST_SOFT_REC;
          if (lane < 8) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              rec[2 + 8 * lane + e] = c0[e];
              rec[2 + 8 * lane + 4 + e] = c1[e];
            }
          }
          if (lane == 0) {
            rec[0] = m;
            rec[1] = s;
          }
        }
      }
    }
  }
  const int w = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int f = 0; f < FR; ++f) {
    float bv = best[f];
    int bx = bi[f];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bx, o, 64);
      if (ob > bv || (ob == bv && oi < bx)) {
        bv = ob;
        bx = oi;
      }
    }
    if (lane == 0) {
      bestv[w * FR + f] = bv;
      besti[w * FR + f] = bx;
    }
  }
  __syncthreads();
  if (tid < nf) {
    float bv = bestv[tid];
    int bx = besti[tid];
    for (int ww = 1; ww < ST_NW; ++ww) {
      const float ob = bestv[ww * FR + tid];
      const int oi = besti[ww * FR + tid];
      if (ob > bv || (ob == bv && oi < bx)) {
        bv = ob;
        bx = oi;
      }
    }
    a.tokens[(long long)(b0 + tid) * a.steps + t] = bx;
  }
  if constexpr (SOFT) {
    // wave f merges the sixteen wave records of frame f in wave order, lane c taking channel c (the __syncthreads above ordered the records)
    if (w < nf) {
      float M = -INFINITY;
      for (int ww = 0; ww < ST_NW; ++ww) M = fmaxf(M, softrec[(ww * FR + w) * ST_SOFT_REC]);
      float num = 0.f, den = 0.f;
      for (int ww = 0; ww < ST_NW; ++ww) {
        const float* rec = softrec + (ww * FR + w) * ST_SOFT_REC;
        if (rec[0] > -INFINITY) {
          const float e = expf(rec[0] - M);
          den = fmaf(e, rec[1], den);
          num = fmaf(e, rec[2 + lane], num);
        }
      }
      a.soft_rows[((long long)(b0 + w) * a.steps + t) * ST_SOFT_C + lane] = num / den;
    }
  }
}

size_t step_lds_bytes(int FR, int d, int H, bool soft) {
  const int hd = d / H, nparts = FR * H > ST_NW ? FR * H : ST_NW;
  return ((size_t)FR * 10 * d + (size_t)nparts * (hd + 2) + 2 * ST_NW * FR + (soft ? (size_t)ST_NW * FR * ST_SOFT_REC : 0)) * sizeof(float);
}

template <int FR, int HD16, bool SOFT, bool SAMPLE>
int step_launch(const StepArgs& a, hipStream_t st) {
  const size_t lds = step_lds_bytes(FR, a.d, a.H, SOFT);
  SF_TRY(sf_ensure_dyn_lds((const void*)slate_step_kernel<FR, HD16, SOFT, SAMPLE>, lds));
  hipLaunchKernelGGL((slate_step_kernel<FR, HD16, SOFT, SAMPLE>), dim3((unsigned)((a.B + FR - 1) / FR)), dim3(ST_NT), lds, st, a);
  SF_CHECK_LAUNCH();
  return 0;
}
template <int FR, int HD16>
int step_launch_mode(const StepArgs& a, bool soft, bool sample, hipStream_t st) {
  if (soft) return sample ? step_launch<FR, HD16, true, true>(a, st) : step_launch<FR, HD16, true, false>(a, st);
  return sample ? step_launch<FR, HD16, false, true>(a, st) : step_launch<FR, HD16, false, false>(a, st);
}
template <int FR>
int step_launch_hd(const StepArgs& a, bool soft, bool sample, hipStream_t st) {
  switch (a.d / a.H) {
    case 16: return step_launch_mode<FR, 1>(a, soft, sample, st);
    case 32: return step_launch_mode<FR, 2>(a, soft, sample, st);
    case 48: return step_launch_mode<FR, 3>(a, soft, sample, st);
    case 64: return step_launch_mode<FR, 4>(a, soft, sample, st);
  }
  return sf_set_err(-1, "invalid argument: slate_step head size", __FILE__, __LINE__);
}

// out[r, :] = table[ids[r], :] (ids outside the table are clamped to its ends: a wrong id never reads out of bounds)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ table, const long long* __restrict__ ids,
                                                          float* __restrict__ out, long long total4, int d4, long long rows) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const long long r = i / d4;
  const int c4 = (int)(i - r * d4);
  long long id = ids[r];
  id = id < 0 ? 0 : (id >= rows ? rows - 1 : id);
  ((f32x4*)out)[i] = ((const f32x4*)table)[id * d4 + c4];
}

constexpr size_t STEP_WS_SLACK = 4096;

// The library's own choice of frames per workgroup for B frames; 0 = the launch chain.  From the table of profiles/steve_render.md (Physion decoder,
// 1024 steps, one MI355X): one frame per workgroup took 0.88 / 0.82 / 0.77 / 0.70 of the chain's time at 1 / 12 / 64 / 192 frames, every one a win
// by more than the 6 % box-to-box spread; two frames per workgroup won by more than that at 1 and 192 frames only and never beat one frame by it;
// four lost.  Beyond 192 frames nothing is measured, so the chain stays.
constexpr int ST_RULE_MAX_FRAMES = 192;
int step_rule(int B) { return B <= ST_RULE_MAX_FRAMES ? 1 : 0; }
}  // namespace

extern "C" {

int sf_slate_step_ok(const sf_slate_decoder* m) {
  if (!m) return 0;
  const int d = m->d_model, H = m->num_heads;
  if (d <= 0 || d > 512 || (d % 32) != 0) return 0;
  if (H <= 0 || H > 16 || (d % H) != 0) return 0;
  const int hd = d / H;
  if (!(hd == 16 || hd == 32 || hd == 48 || hd == 64)) return 0;
  if (m->num_layers < 1 || m->num_layers > ST_MAXL) return 0;
  if (m->vocab_size < 1 || m->num_slots < 1 || m->max_len < 0) return 0;
  return 1;
}

size_t sf_slate_generate_tok_workspace_bytes(const sf_slate_decoder* m, int B, int steps) {
  if (!m || B <= 0 || steps <= 0) return 0;
  const size_t chain = sf_slate_generate_workspace_bytes(m, B, steps);
  if (!sf_slate_step_ok(m)) return chain;
  const size_t fused = sf_slate_gen_carve(nullptr, m, B, steps, (size_t)2 * m->d_model, false).bytes + STEP_WS_SLACK;   // a k|v cache, no row buffers
  return fused > chain ? fused : chain;
}

size_t sf_slate_generate_tok_opts_workspace_bytes(const sf_slate_decoder* m, int B, int steps, const sf_slate_step_opts* opts) {
  // with an option on only the fused step can run: its carve alone (a k|v cache, no row buffers, nothing that grows with the vocabulary)
  if (opts && (opts->soft_rows || opts->sample) && m && B > 0 && steps > 0 && sf_slate_step_ok(m))
    return sf_slate_gen_carve(nullptr, m, B, steps, (size_t)2 * m->d_model, false).bytes + STEP_WS_SLACK;
  return sf_slate_generate_tok_workspace_bytes(m, B, steps);
}

int sf_slate_generate_tok_f32(const sf_slate_decoder* m, const float* slots, int B, int steps, long long* tokens_out, float* logits_out,
                              int frames_per_wg, void* ws, size_t ws_bytes, void* stream, int* frames_per_wg_ran) {
  return sf_slate_generate_tok_opts_f32(m, slots, B, steps, tokens_out, logits_out, frames_per_wg, ws, ws_bytes, stream, frames_per_wg_ran,
                                        nullptr);
}

int sf_slate_generate_tok_opts_f32(const sf_slate_decoder* m, const float* slots, int B, int steps, long long* tokens_out, float* logits_out,
                                   int frames_per_wg, void* ws, size_t ws_bytes, void* stream, int* frames_per_wg_ran,
                                   const sf_slate_step_opts* opts) {
  SF_REQUIRE(m && slots && tokens_out && ws, "sf_slate_generate_tok_f32: null pointer");
  SF_REQUIRE(B >= 1 && steps >= 1 && steps - 1 <= m->max_len, "sf_slate_generate_tok_f32: bad batch / step count");
  SF_REQUIRE(frames_per_wg == 0 || frames_per_wg == 1 || frames_per_wg == 2 || frames_per_wg == 4,
             "sf_slate_generate_tok_f32: frames_per_wg must be 0, 1, 2 or 4");
  const bool soft = opts && opts->soft_rows, sample = opts && opts->sample;
  if (soft) {
    SF_REQUIRE(opts->conv0_t, "sf_slate_generate_tok_opts_f32: soft_rows without the table conv0_t");
    SF_REQUIRE(opts->conv0_width == ST_SOFT_C, "sf_slate_generate_tok_opts_f32: conv0_width must be 64");
    SF_REQUIRE(std::isfinite(opts->soft_scale) && opts->soft_scale > 0.f, "sf_slate_generate_tok_opts_f32: soft_scale must be finite and > 0");
  }
  if (sample)
    SF_REQUIRE(std::isfinite(opts->inv_temperature) && opts->inv_temperature > 0.f,
               "sf_slate_generate_tok_opts_f32: inv_temperature must be finite and > 0");
  if (soft || sample) {
    SF_REQUIRE(opts->row_base >= 0, "sf_slate_generate_tok_opts_f32: negative row_base");
    SF_REQUIRE(m->vocab_size >= 1 && opts->row_base < (1LL << 32) &&
                   (opts->row_base + (long long)B * steps) * (long long)m->vocab_size < (1LL << 32),
               "sf_slate_generate_tok_opts_f32: (row_base + B * steps) * V must stay below 2^32");
    SF_REQUIRE(sf_slate_step_ok(m), "sf_slate_generate_tok_opts_f32: soft rows and sampling need the fused step, which refuses this decoder");
  }
  SF_REQUIRE(ws_bytes >= sf_slate_generate_tok_opts_workspace_bytes(m, B, steps, opts), "sf_slate_generate_tok_f32: workspace too small");
  int FR = 0;
  if (sf_slate_step_ok(m)) FR = frames_per_wg ? frames_per_wg : ((soft || sample) ? 1 : step_rule(B));
  if (frames_per_wg_ran) *frames_per_wg_ran = FR;
  if (FR == 0) return sf_slate_generate_f32(m, slots, B, steps, tokens_out, logits_out, ws, ws_bytes, stream);
  SF_REQUIRE(m->in_proj_w && m->in_proj_b && m->tok_emb && m->pos_emb && m->lnf_g && m->lnf_b && m->head_w && m->blocks,
             "sf_slate_generate_tok_f32: null weight");
  hipStream_t st = (hipStream_t)stream;
  const int d = m->d_model, N = m->num_slots, NL = m->num_layers;
  const float eps = 1e-5f;
  const SfSlateGenWs w = sf_slate_gen_carve(ws, m, B, steps, (size_t)2 * d, false);
  StepArgs a;
  memset(&a, 0, sizeof(a));
  float* mem = w.mem;
  const SfRowMap rd = sf_rows(d);
  // slots -> memory, and every block's cross-attention keys / values (once), as sf_slate_generate_f32 does
  SF_TRY(sf_linear_ex(slots, rd, m->in_proj_w, m->in_proj_b, nullptr, nullptr, eps, nullptr, rd, 0, mem, rd, B * N, d, d, 0, st));
  for (int i = 0; i < NL; ++i) {
    const sf_slate_block& k = m->blocks[i];
    SF_REQUIRE(k.ln1_g && k.ln1_b && k.wqkv && k.wo && k.ln2_g && k.ln2_b && k.wq_c && k.wkv_c && k.wo_c && k.ln3_g && k.ln3_b &&
                   k.w1 && k.b1 && k.w2 && k.b2, "sf_slate_generate_tok_f32: null block weight");
    float* memkv = w.memkv[i];
    SF_TRY(sf_linear_ex(mem, rd, k.wkv_c, nullptr, nullptr, nullptr, eps, nullptr, rd, 0, memkv, sf_rows(2 * d), B * N, 2 * d, d, 0, st));
    StepBlock& s = a.blk[i];
    s.ln1_g = k.ln1_g, s.ln1_b = k.ln1_b, s.wqkv = k.wqkv, s.wo = k.wo;
    s.ln2_g = k.ln2_g, s.ln2_b = k.ln2_b, s.wq_c = k.wq_c, s.wo_c = k.wo_c;
    s.ln3_g = k.ln3_g, s.ln3_b = k.ln3_b, s.w1 = k.w1, s.b1 = k.b1, s.w2 = k.w2, s.b2 = k.b2;
    s.memkv = memkv;
    s.is_first = k.is_first;
  }
  for (int i = 0; i < NL; ++i) a.blk[i].cache = w.cache[i];
  a.tok_emb = m->tok_emb, a.pos_emb = m->pos_emb, a.lnf_g = m->lnf_g, a.lnf_b = m->lnf_b, a.head_w = m->head_w;
  a.tokens = tokens_out, a.logits = logits_out;
  a.d = d, a.H = m->num_heads, a.NL = NL, a.V = m->vocab_size, a.N = N, a.B = B, a.steps = steps;
  if (soft) {
    a.soft_rows = opts->soft_rows, a.conv0_t = opts->conv0_t, a.soft_scale = opts->soft_scale;
    a.soft_sseed = sf_gumbel_seed(opts->soft_seed);
  }
  if (sample) a.inv_temperature = opts->inv_temperature, a.sample_sseed = sf_gumbel_seed(opts->sample_seed);
  if (soft || sample) a.row_base = opts->row_base;
  for (int t = 0; t < steps; ++t) {
    a.t = t;
    if (FR == 1) SF_TRY(step_launch_hd<1>(a, soft, sample, st));
    else if (FR == 2) SF_TRY(step_launch_hd<2>(a, soft, sample, st));
    else SF_TRY(step_launch_hd<4>(a, soft, sample, st));
  }
  return 0;
}

int sf_gather_rows_f32(const float* table, const long long* ids, float* out, long long R, int d, long long table_rows, void* stream) {
  SF_REQUIRE(table && ids && out && R >= 0 && d > 0 && (d % 4) == 0 && table_rows > 0, "sf_gather_rows_f32: bad arguments");
  const long long total4 = R * (d / 4);
  if (total4 == 0) return 0;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table, ids, out, total4,
                     d / 4, table_rows);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

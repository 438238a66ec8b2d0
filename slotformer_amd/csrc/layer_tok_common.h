// What the token-stationary layer kernels (layer_tok.hip: d_model 256; layer_tok128.hip: d_model 128) share: the split-bf16 fragment helpers, the weight
// ring as a wave sees it, the two register-resident products, LayerNorm in accumulator layout, and the kernel that packs a layer's matrices in
// consumption order.  Sizes that differ between the shapes are template parameters deduced from the register arrays.
#pragma once
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"

namespace {
__device__ __forceinline__ bf16x8 cat8(bf16x4 a, bf16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }
__device__ __forceinline__ f32x4 quad(const f32x16& a, int g) { return f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]}; }
// the value of the lane that holds the other half of this token's features / keys (lane ^ 32): one v_permlane32_swap, no LDS.  (The instruction swaps the
// upper half of its first operand with the lower half of its second; whether the compiler gives the two copies of `v` one register or two, the partner's
// value is result 0 in the upper half and result 1 in the lower.)
__device__ __forceinline__ float lt_xother(float v, int h) {
#ifdef LT_SHFL
  return __shfl_xor(v, 32, 64);
#endif
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __builtin_bit_cast(float, h ? r[0] : r[1]);
}
__device__ __forceinline__ float lt_xmax(float v, int h) { return fmaxf(v, lt_xother(v, h)); }
__device__ __forceinline__ float lt_xsum(float v, int h) {
  const float o = lt_xother(v, h);
  return h ? o + v : v + o;   // (lower half's value first in both lanes: the two halves of a token get the same bits)
}

// the ring as one wave sees it during a stage: `rd` = this lane's read address of fragment 0 of the current stage, (`src`, `dst`) = where piece 0 of the
// stage two ahead comes from (per lane) / goes to (wave-uniform); a product issues one piece per fragment group
struct LtRing {
  const char* rd;
  const char* src;
  char* dst;
};
__device__ __forceinline__ void lt_dma_now(const LtRing& R, int f) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(R.src + f * 1024),
                                   (void __attribute__((address_space(3)))*)(R.dst + f * 1024), 16, 0, 0);
}
__device__ __forceinline__ void lt_dma(const LtRing& R, int f) {
#if defined(LT_NODMA) || defined(LT_BURST)
  return;
#endif
#ifndef LT_NOIMMOFF
  // the instruction's immediate offset applies to BOTH addresses: pieces 4 k .. 4 k + 3 share one per-lane source address and one M0 value
  // (354 instead of 365 us per 3-layer launch of 64 workgroups: three instructions less around every piece)
  const void __attribute__((address_space(1)))* s = (const void __attribute__((address_space(1)))*)(R.src + (f >> 2) * 4096);
  void __attribute__((address_space(3)))* d = (void __attribute__((address_space(3)))*)(R.dst + (f >> 2) * 4096);
  switch (f & 3) {
    case 0: __builtin_amdgcn_global_load_lds(s, d, 16, 0, 0); break;
    case 1: __builtin_amdgcn_global_load_lds(s, d, 16, 1024, 0); break;
    case 2: __builtin_amdgcn_global_load_lds(s, d, 16, 2048, 0); break;
    default: __builtin_amdgcn_global_load_lds(s, d, 16, 3072, 0); break;
  }
#else
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(R.src + f * 1024),
                                   (void __attribute__((address_space(3)))*)(R.dst + f * 1024), 16, 0, 0);
#endif
}
#define LT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
// keeps the MFMAs on either side in source order (every other class may cross): the scheduler otherwise groups the MFMAs of one accumulator, and a chain
// of dependent MFMAs issues every ~44 cycles instead of 32
#define LT_PIN() __builtin_amdgcn_sched_barrier(0x7F6)
#define LT_SGB(mask, n) __builtin_amdgcn_sched_group_barrier(mask, n, 0)
struct LtNoSide {
  __device__ __forceinline__ void operator()(int) const {}
};
// the issue pattern of a fragment group: its first MFMA, the four fragment reads of the next group, then the other five MFMAs with up to NV VALU
// instructions of the side work behind each (a wave alone on its SIMD hides about five issue slots under an MFMA)
template <int NV, bool READS>
__device__ __forceinline__ void lt_group_pattern() {
  LT_SGB(0x008, 1);
  if constexpr (READS) LT_SGB(0x100, 4);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if constexpr (NV > 0) LT_SGB(0x002, NV);
    LT_SGB(0x008, 1);
  }
  if constexpr (NV > 0) LT_SGB(0x002, NV);
  __builtin_amdgcn_sched_barrier(0);
}

// D^T[32 features][32 tokens] (SW: D[32 tokens][32 features]) = W block . A^T over the 16 NKS input channels (NKS virtual k-steps): fragment group g = (hi, lo) of the virtual
// k-steps 2 g and 2 g + 1.  Consecutive MFMAs ALTERNATE between two accumulators (even / odd k-steps, summed at the end): anything issued between two
// MFMAs on the SAME accumulator costs ~43 cycles (MI355X_MICROARCH.md), between MFMAs on different ones ~6.  The reads of group g + 1 go behind the first
// MFMA of group g (ffn_tok.hip); side(g) = VALU work of ANOTHER chain (the previous product's conversion, a softmax slice) that the scheduler places
// between this group's MFMAs.
template <bool SW, int NV, int NKS, class Side>
__device__ __forceinline__ void lt_row_product(const LtRing& R, const bf16x8 (&xh)[NKS], const bf16x8 (&xl)[NKS], f32x16& a, Side&& side) {
  constexpr int NG = NKS / 2;
  bf16x8 wb[2][4];
  f32x16 a1;
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = a1[r] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) wb[0][i] = *(const bf16x8*)(R.rd + i * 1024);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int b = g & 1, ks = 2 * g;
    if constexpr (!SW) a = LT_MFMA(wb[b][0], xl[ks], a); else a = LT_MFMA(xl[ks], wb[b][0], a);
#ifndef LT_NOREAD
    if (g + 1 < NG) {
#pragma unroll
      for (int i = 0; i < 4; ++i) wb[b ^ 1][i] = *(const bf16x8*)(R.rd + (4 * (g + 1) + i) * 1024);
    }
#else
    if (g == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) wb[1][i] = *(const bf16x8*)(R.rd + (4 + i) * 1024);
    }
#endif
    lt_dma(R, g);
    LT_PIN();
    if constexpr (!SW) {
      a1 = LT_MFMA(wb[b][2], xl[ks + 1], a1);
      LT_PIN();
      a = LT_MFMA(wb[b][1], xh[ks], a);
      LT_PIN();
      a1 = LT_MFMA(wb[b][3], xh[ks + 1], a1);
      LT_PIN();
      a = LT_MFMA(wb[b][0], xh[ks], a);
      LT_PIN();
      a1 = LT_MFMA(wb[b][2], xh[ks + 1], a1);
    } else {
      a1 = LT_MFMA(xl[ks + 1], wb[b][2], a1);
      LT_PIN();
      a = LT_MFMA(xh[ks], wb[b][1], a);
      LT_PIN();
      a1 = LT_MFMA(xh[ks + 1], wb[b][3], a1);
      LT_PIN();
      a = LT_MFMA(xh[ks], wb[b][0], a);
      LT_PIN();
      a1 = LT_MFMA(xh[ks + 1], wb[b][2], a1);
    }
    LT_PIN();
#ifndef LT_NOSIDE
    side(g);
    if (g + 1 < NG) lt_group_pattern<NV, true>(); else lt_group_pattern<NV, false>();
#else
    if (g + 1 < NG) lt_group_pattern<0, true>(); else lt_group_pattern<0, false>();
#endif
  }
#ifdef LT_NOSIDE
#pragma unroll
  for (int g = 0; g < NG; ++g) side(g);
#endif
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] += a1[r];
}
// Y^T[32 NOB features][32 tokens] += W[:, 32-wide slice] . I^T: fragment group p = the (hi, lo) fragments of the slice's two virtual k-steps for the output
// blocks 2 p and 2 p + 1, whose accumulators alternate (see above)
template <int NV, int NOB, class Side>
__device__ __forceinline__ void lt_kslice_product(const LtRing& R, const bf16x8 (&ih)[2], const bf16x8 (&il)[2], f32x16 (&Y)[NOB], Side&& side) {
  bf16x8 wb[2][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wb[0][i] = *(const bf16x8*)(R.rd + i * 1024);
#pragma unroll
  for (int p = 0; p < NOB / 2; ++p) {
    const int b = p & 1, oa = 2 * p, ob = 2 * p + 1;
    Y[oa] = LT_MFMA(wb[b][0], il[0], Y[oa]);
#ifndef LT_NOREAD
    if (p + 1 < NOB / 2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) wb[b ^ 1][i] = *(const bf16x8*)(R.rd + (8 * (p + 1) + i) * 1024);
    }
#else
    if (p == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) wb[1][i] = *(const bf16x8*)(R.rd + (8 + i) * 1024);
    }
#endif
    lt_dma(R, 2 * p);
    LT_PIN();
    Y[ob] = LT_MFMA(wb[b][4], il[0], Y[ob]);
    LT_PIN();
    Y[oa] = LT_MFMA(wb[b][1], ih[0], Y[oa]);
    LT_PIN();
    Y[ob] = LT_MFMA(wb[b][5], ih[0], Y[ob]);
    LT_PIN();
    Y[oa] = LT_MFMA(wb[b][0], ih[0], Y[oa]);
    LT_PIN();
    Y[ob] = LT_MFMA(wb[b][4], ih[0], Y[ob]);
    lt_dma(R, 2 * p + 1);
    LT_PIN();
    Y[oa] = LT_MFMA(wb[b][2], il[1], Y[oa]);
    LT_PIN();
    Y[ob] = LT_MFMA(wb[b][6], il[1], Y[ob]);
    LT_PIN();
    Y[oa] = LT_MFMA(wb[b][3], ih[1], Y[oa]);
    LT_PIN();
    Y[ob] = LT_MFMA(wb[b][7], ih[1], Y[ob]);
    LT_PIN();
    Y[oa] = LT_MFMA(wb[b][2], ih[1], Y[oa]);
    LT_PIN();
    Y[ob] = LT_MFMA(wb[b][6], ih[1], Y[ob]);
    LT_PIN();
#ifndef LT_NOSIDE
    side(2 * p);
    side(2 * p + 1);
#endif
    // first MFMA, the eight fragment reads of the next pair, then the other eleven MFMAs with the side work between them
    LT_SGB(0x008, 1);
    if (p + 1 < NOB / 2) LT_SGB(0x100, 8);
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      if constexpr (NV > 0) LT_SGB(0x002, NV);
      LT_SGB(0x008, 1);
    }
    if constexpr (NV > 0) LT_SGB(0x002, NV);
    __builtin_amdgcn_sched_barrier(0);
  }
#ifdef LT_NOSIDE
#pragma unroll
  for (int g = 0; g < NOB; ++g) side(g);
#endif
}

// LayerNorm over the 32 NOB features of a token held as X[ob][4 g + q] = feature 32 ob + 8 g + 4 h + q by lanes (token, h = 0 / 1); gamma / beta in LDS at
// float offsets GOFF / BOFF behind pb (= the vector block + 4 h floats, an opaque per-lane base: every read is base + immediate):
// the normalised row as the 2 NOB hi | lo fragments of the virtual k-steps (block ob, s): registers 8 s .. 8 s + 7
template <int GOFF, int BOFF, int NOB>
__device__ __forceinline__ void lt_layernorm(const f32x16 (&X)[NOB], const char* pb, int h, float eps, bf16x8 (&xh)[2 * NOB], bf16x8 (&xl)[2 * NOB]) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
      s0 += X[ob][r];
      s1 += X[ob][r + 1];
      s2 += X[ob][r + 2];
      s3 += X[ob][r + 3];
    }
  const float mu = lt_xsum((s0 + s1) + (s2 + s3), h) * (1.0f / (32 * NOB));
  float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int r = 0; r < 16; r += 4) {
      const float d0 = X[ob][r] - mu, d1 = X[ob][r + 1] - mu, d2 = X[ob][r + 2] - mu, d3 = X[ob][r + 3] - mu;
      q0 += d0 * d0;
      q1 += d1 * d1;
      q2 += d2 * d2;
      q3 += d3 * d3;
    }
  const float rs = 1.0f / sqrtf(lt_xsum((q0 + q1) + (q2 + q3), h) * (1.0f / (32 * NOB)) + eps);
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int s2i = 0; s2i < 2; ++s2i) {
      f32x4 v[2];
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const int g = 2 * s2i + gg, c = 32 * ob + 8 * g;
        v[gg] = (quad(X[ob], g) - mu) * rs * *(const f32x4*)(pb + (GOFF + c) * 4) + *(const f32x4*)(pb + (BOFF + c) * 4);
      }
      sf_split8(v[0], v[1], xh[2 * ob + s2i], xl[2 * ob + s2i]);
      __builtin_amdgcn_sched_barrier(0);   // (left alone the scheduler requests all 64 gamma / beta vectors first: 200 spilled registers)
    }
}
// X[ob][4 g + q] += vec[32 ob + 8 g + 4 h + q]  (vec at float offset OFF behind pb)
template <int OFF, int NOB>
__device__ __forceinline__ void lt_add_vec(f32x16 (&X)[NOB], const char* pb) {
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 bv = *(const f32x4*)(pb + (OFF + 32 * ob + 8 * g) * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) X[ob][4 * g + q] += bv[q];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- weights of one layer -> NST stages x FPS fragments x 64 lanes x 16 B in CONSUMPTION order (the kernels), then the layer's vectors ----------------------
// D = d_model, F = ffn; an attention BLOCK is 32 rows of q / k / v: one head of 32 at d_model 256 (8 blocks), a pair of heads of 16 at d_model 128 (4 blocks);
// NB = D / 32 of them, FPS = D / 8 fragments per stage, NST = 4 NB + 2 (F / 32) stages (96 x 32 KiB at 256 / 1024, 48 x 16 KiB at 128 / 512)
//   attention, stage a:  0 / 1 / 2: q / k / v rows of block 0;  3 + 4 (i - 1) + {0, 1, 2, 3}: q / k / v rows of block i and the out_proj columns of block i - 1
//                        (i = 1..NB - 1);  4 NB - 1: the out_proj columns of block NB - 1     (q rows 32 i, k rows D + 32 i, v rows 2 D + 32 i of in_proj_w [3 D][D])
//   FFN, stage 4 NB + f: f = 0: lin1 rows of hidden block 0;  f = 2 j - 1: lin1 rows of block j,  f = 2 j: lin2 columns of block j - 1  (j = 1..F / 32 - 1);
//                        f = 2 (F / 32) - 1: lin2 columns of the last block
//   row stages:    fragment f = 2 vk + plane, virtual k-step vk = (input block ib, s);  column stages: fragment f = 4 ob + 2 s + plane (output block ob)
//   element j of lane (i, h) of a fragment over columns c0 .. c0 + 31 at k-step s:  W[r0 + i][c0 + 8 (2 s + (j >> 2)) + 4 h + (j & 3)]
//   (the k order of an accumulator: register 8 s + j of lane (token, h) holds feature 8 (2 s + (j >> 2)) + 4 h + (j & 3) of its 32-block)
template <int D, int F>
__global__ void pack_layer_tok_kernel(const float* __restrict__ win, const float* __restrict__ wout, const float* __restrict__ w1,
                                      const float* __restrict__ w2, uint4* __restrict__ out) {
  constexpr int NB = D / 32, FPS = D / 8, NST_ATT = 4 * NB, NFF = 2 * (F / 32), NST = NST_ATT + NFF;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= NST * FPS * 64) return;
  const int lane = idx & 63, f = (idx >> 6) % FPS, st = idx / (64 * FPS);
  const int pl = f & 1, h = lane >> 5, i = lane & 31;
  const float* W;
  int ld, r0 = 0, c0 = 0, s;
  bool slice;
  if (st < NST_ATT) {
    int hd, kind;   // 0 q, 1 k, 2 v, 3 out_proj columns
    if (st < 3) {
      hd = 0; kind = st;
    } else if (st == NST_ATT - 1) {
      hd = NB - 1; kind = 3;
    } else {
      const int tq = st - 3;
      kind = tq & 3;
      hd = 1 + (tq >> 2) - (kind == 3 ? 1 : 0);
    }
    slice = kind == 3;
    ld = D;
    if (!slice) {
      W = win; r0 = kind * D + 32 * hd;
    } else {
      W = wout; c0 = 32 * hd;
    }
  } else {
    const int ff = st - NST_ATT;
    int hb;
    if (ff == 0) {
      slice = false; hb = 0;
    } else if (ff == NFF - 1) {
      slice = true; hb = F / 32 - 1;
    } else if (ff & 1) {
      slice = false; hb = (ff + 1) >> 1;
    } else {
      slice = true; hb = (ff >> 1) - 1;
    }
    if (!slice) {
      W = w1; ld = D; r0 = 32 * hb;
    } else {
      W = w2; ld = F; c0 = 32 * hb;
    }
  }
  if (!slice) {
    const int vk = f >> 1;
    c0 = 32 * (vk >> 1);
    s = vk & 1;
  } else {
    r0 = 32 * (f >> 2);
    s = (f >> 1) & 1;
  }
  const float* src = W + (long long)(r0 + i) * ld + c0 + 4 * h;
  union {
    __bf16 b[8];
    uint4 u;
  } o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = src[8 * (2 * s + (j >> 2)) + (j & 3)];
    const __bf16 hi = (__bf16)v;
    o.b[j] = pl ? (__bf16)(v - (float)hi) : hi;
  }
  out[idx] = o.u;
}
}  // namespace

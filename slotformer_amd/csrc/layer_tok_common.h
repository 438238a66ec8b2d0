// What the token-stationary layer kernels (layer_tok.hip: d_model 256; layer_tok128.hip: d_model 128) share: the split-bf16 fragment helpers, the weight
// ring as a wave sees it, the two register-resident products, LayerNorm in accumulator layout, and the kernel that packs a layer's matrices in
// consumption order.  Sizes that differ between the shapes are template parameters deduced from the register arrays.
// Behind them the same pieces on v_mfma_f32_16x16x32_bf16 (lt16_*: the FFN block of layer_tok.hip; layer_tok128.hip uses none of them): the products over
// 16-token tiles, the in-place swap of the residual stream between the two accumulator layouts, LayerNorm and the vector add in the 16-layout, and the
// packer of the FFN stages in that fragment order.
// Element map of a packed layer (sf_pack_layer_tok_weights at d_model 256): stages 0 .. 4 NB - 1 as pack_layer_tok_kernel documents them (32x32x16 fragments,
// lane = (row i = lane & 31, h = lane >> 5)); stages 4 NB .. as pack_layer_tok_ffn16_kernel does (16x16x32 fragments, lane = (row i = lane & 15, g = lane >> 4));
// in both, a stage is 32 fragments x 64 lanes x 8 bf16, fragment f of plane f & 1 (0: hi = bf16(w), 1: lo = bf16(w - hi)); then the eight vectors in f32.
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

// ================================ the same products on v_mfma_f32_16x16x32_bf16 (layer_tok.hip: the FFN block) ================================
// A wave's 32 tokens are two TILES t of 16; a lane is (token j = lane & 15 of either tile, g = lane >> 4).  A 16 x 16 accumulator holds in register q the
// feature of MFMA row 4 g + q of a 16-feature block; two blocks of one tile read as they lie are the K = 32 B operand of the next product (elements 0..3 of
// a lane: its four rows of the first block, 4..7: of the second), and the packer emits the A fragments in that k order.  Same FLOPs and MFMA cycles as the
// 32x32x16 form (twice the instructions of half the length); the chip holds a higher clock on this shape (profiles/conv_mfma_shape.md).
// The residual stream keeps its registers across the two forms: in the 16-layout register 4 (2 p + t) + q of X[ob] belongs to 16-block 2 ob + p, tile t,
// and MFMA row 4 g + q of a block of the residual stream is feature LT16_FEAT(g) + q of it (what lt16_swap_layout makes of the 32-layout).
#define LT_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define LT16_FEAT(g) (8 * ((g) & 1) + 4 * ((g) >> 1))
// the value of lane ^ 16: one v_permlane16_swap (the odd 16-lane rows of its first operand trade places with the even rows of its second)
__device__ __forceinline__ float lt16_xother(float v, int b4) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __builtin_bit_cast(float, b4 ? r[0] : r[1]);
}
// sum over the four lanes (g = 0..3) of a token; the same bits in all four
__device__ __forceinline__ float lt16_xsum(float v, int g) {
  const float t = v + lt16_xother(v, g & 1);
  return t + lt_xother(t, g >> 1);
}
// 32-layout <-> 16-layout of the residual stream, in place and its own inverse: lane bit 4 is the token's bit 4 in the one and a feature bit in the other.
// One swap per register pair (8 p + q, 8 p + 4 + q): 32-layout registers 4 gg + q = feature 8 gg + 4 h + q of token lane & 31  <->  16-layout register
// 4 (2 p + t) + q = feature 16 p + 8 (g & 1) + 4 (g >> 1) + q of token 16 t + (lane & 15)
template <int NOB>
__device__ __forceinline__ void lt16_swap_layout(f32x16 (&X)[NOB]) {
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // (scalars first: __builtin_bit_cast of a vector ELEMENT reads element 0 of the vector)
        const float a = X[ob][8 * p + q], b = X[ob][8 * p + 4 + q];
        const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b), false, false);
        const unsigned r0 = r[0], r1 = r[1];
        X[ob][8 * p + q] = __builtin_bit_cast(float, r0);
        X[ob][8 * p + 4 + q] = __builtin_bit_cast(float, r1);
      }
}
// the issue pattern of a fragment group of either product below: its first MFMA, the four fragment reads of the next group, then the other eleven MFMAs
// with up to NV VALU instructions of the side work behind each (an MFMA of 16 cycles leaves the vector issue free for about two)
template <int NV, bool READS>
__device__ __forceinline__ void lt16_group_pattern() {
  LT_SGB(0x008, 1);
  if constexpr (READS) LT_SGB(0x100, 4);
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    if constexpr (NV > 0) LT_SGB(0x002, NV);
    LT_SGB(0x008, 1);
  }
  if constexpr (NV > 0) LT_SGB(0x002, NV);
  __builtin_amdgcn_sched_barrier(0);
}
// fragment groups in registers: the reads of group g + LT16_NBUF - 1 go behind the first MFMA of group g (3: two groups ahead -- 1 us of a 350 us launch
// against 2, one group ahead, at 16 more registers)
#ifndef LT16_NBUF
#define LT16_NBUF 3
#endif
// H[r][t] (rows 16 r .. + 15 of a 32-row block of W, tile t) = W block . A^T over the NKS k-steps of 32 input features: fragment group ks = (hi, lo) of
// row half 0, (hi, lo) of row half 1.  xh / xl [NKS t + ks]: the (hi, lo) fragments of tile t.  Twelve MFMAs per group, pass by pass (x_lo w_hi, x_hi w_lo,
// x_hi w_hi) over the FOUR accumulators: an accumulator comes round every fourth MFMA.
template <int NV, int NKS, class Side>
__device__ __forceinline__ void lt16_row_product(const LtRing& R, const bf16x8 (&xh)[2 * NKS], const bf16x8 (&xl)[2 * NKS], f32x4 (&H)[2][2], Side&& side) {
  bf16x8 wb[LT16_NBUF][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int t = 0; t < 2; ++t) H[r][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < LT16_NBUF - 1; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) wb[g][i] = *(const bf16x8*)(R.rd + (4 * g + i) * 1024);
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int b = ks % LT16_NBUF, bn = (ks + LT16_NBUF - 1) % LT16_NBUF;
    H[0][0] = LT_MFMA16(wb[b][0], xl[ks], H[0][0]);
    if (ks + LT16_NBUF - 1 < NKS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) wb[bn][i] = *(const bf16x8*)(R.rd + (4 * (ks + LT16_NBUF - 1) + i) * 1024);
    }
    lt_dma(R, ks);
    LT_PIN();
    H[0][1] = LT_MFMA16(wb[b][0], xl[NKS + ks], H[0][1]);
    LT_PIN();
    H[1][0] = LT_MFMA16(wb[b][2], xl[ks], H[1][0]);
    LT_PIN();
    H[1][1] = LT_MFMA16(wb[b][2], xl[NKS + ks], H[1][1]);
    LT_PIN();
#pragma unroll
    for (int pass = 1; pass < 3; ++pass)   // w_lo, then w_hi, against x_hi
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          H[r][t] = LT_MFMA16(wb[b][2 * r + (pass == 1 ? 1 : 0)], xh[NKS * t + ks], H[r][t]);
          LT_PIN();
        }
    side(ks);
    if (ks + LT16_NBUF - 1 < NKS) lt16_group_pattern<NV, true>(); else lt16_group_pattern<NV, false>();
  }
}
// X (16-layout, all 2 NOB blocks x 2 tiles) += W[:, 32-wide slice] . I^T in ONE K = 32 step: fragment group p = the (hi, lo) fragments of the output blocks
// 2 p and 2 p + 1, which are the sixteen registers of X[p]; ih / il [t]: the slice's (hi, lo) fragments of tile t
template <int NV, int NOB, class Side>
__device__ __forceinline__ void lt16_kslice_product(const LtRing& R, const bf16x8 (&ih)[2], const bf16x8 (&il)[2], f32x16 (&X)[NOB], Side&& side) {
  bf16x8 wb[LT16_NBUF][4];
#pragma unroll
  for (int g = 0; g < LT16_NBUF - 1; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) wb[g][i] = *(const bf16x8*)(R.rd + (4 * g + i) * 1024);
#pragma unroll
  for (int p = 0; p < NOB; ++p) {
    const int b = p % LT16_NBUF, bn = (p + LT16_NBUF - 1) % LT16_NBUF;
    f32x4 c[2][2];   // [block 2 p + bb][tile]
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int t = 0; t < 2; ++t) c[bb][t] = quad(X[p], 2 * bb + t);
    c[0][0] = LT_MFMA16(wb[b][0], il[0], c[0][0]);
    if (p + LT16_NBUF - 1 < NOB) {
#pragma unroll
      for (int i = 0; i < 4; ++i) wb[bn][i] = *(const bf16x8*)(R.rd + (4 * (p + LT16_NBUF - 1) + i) * 1024);
    }
    lt_dma(R, p);
    LT_PIN();
    c[0][1] = LT_MFMA16(wb[b][0], il[1], c[0][1]);
    LT_PIN();
    c[1][0] = LT_MFMA16(wb[b][2], il[0], c[1][0]);
    LT_PIN();
    c[1][1] = LT_MFMA16(wb[b][2], il[1], c[1][1]);
    LT_PIN();
#pragma unroll
    for (int pass = 1; pass < 3; ++pass)
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          c[bb][t] = LT_MFMA16(wb[b][2 * bb + (pass == 1 ? 1 : 0)], ih[t], c[bb][t]);
          LT_PIN();
        }
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) X[p][4 * (2 * bb + t) + q] = c[bb][t][q];
    side(p);
    if (p + LT16_NBUF - 1 < NOB) lt16_group_pattern<NV, true>(); else lt16_group_pattern<NV, false>();
  }
}
// LayerNorm over the 32 NOB features of the tokens of both tiles, X in 16-layout; gamma / beta at float offsets GOFF / BOFF behind px (= the vector block +
// LT16_FEAT(g) floats, an opaque per-lane base): the normalised rows as the NOB hi | lo fragments of each tile, xh / xl [NOB t + ob]
template <int GOFF, int BOFF, int NOB>
__device__ __forceinline__ void lt16_layernorm(const f32x16 (&X)[NOB], const char* px, int g, float eps, bf16x8 (&xh)[2 * NOB], bf16x8 (&xl)[2 * NOB]) {
  float mu[2], rs[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int r = 4 * (2 * p + t);
        s0 += X[ob][r];
        s1 += X[ob][r + 1];
        s2 += X[ob][r + 2];
        s3 += X[ob][r + 3];
      }
    mu[t] = lt16_xsum((s0 + s1) + (s2 + s3), g) * (1.0f / (32 * NOB));
    float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int r = 4 * (2 * p + t);
        const float d0 = X[ob][r] - mu[t], d1 = X[ob][r + 1] - mu[t], d2 = X[ob][r + 2] - mu[t], d3 = X[ob][r + 3] - mu[t];
        q0 += d0 * d0;
        q1 += d1 * d1;
        q2 += d2 * d2;
        q3 += d3 * d3;
      }
    rs[t] = 1.0f / sqrtf(lt16_xsum((q0 + q1) + (q2 + q3), g) * (1.0f / (32 * NOB)) + eps);
  }
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) {
    f32x4 ga[2], be[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      ga[p] = *(const f32x4*)(px + (GOFF + 32 * ob + 16 * p) * 4);
      be[p] = *(const f32x4*)(px + (BOFF + 32 * ob + 16 * p) * 4);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
      sf_split8((quad(X[ob], t) - mu[t]) * rs[t] * ga[0] + be[0], (quad(X[ob], 2 + t) - mu[t]) * rs[t] * ga[1] + be[1], xh[NOB * t + ob], xl[NOB * t + ob]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// X (16-layout) += vec (at float offset OFF behind px)
template <int OFF, int NOB>
__device__ __forceinline__ void lt16_add_vec(f32x16 (&X)[NOB], const char* px) {
#pragma unroll
  for (int ob = 0; ob < NOB; ++ob) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const f32x4 bv = *(const f32x4*)(px + (OFF + 32 * ob + 16 * p) * 4);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) X[ob][4 * (2 * p + t) + q] += bv[q];
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- the FFN stages (4 NB ..) of a layer for the 16x16x32 products: the same stages in the same order as pack_layer_tok_kernel, 32 fragments each ----
//   lane (i = lane & 15, g = lane >> 4), element j of a fragment; hidden block hb, hi plane = bf16(w), lo plane = bf16(w - hi)
//   row stage (lin1 rows of hidden block hb):        fragment f = 4 ks + 2 r + plane (k-step ks, row half r):
//       W1[32 hb + 16 r + i][32 ks + 16 (j >> 2) + LT16_FEAT(g) + (j & 3)]
//   column stage (lin2 columns of hidden block hb):  fragment f = 2 ob + plane (16-row output block ob):
//       W2[16 ob + LT16_FEAT(i >> 2) + (i & 3)][32 hb + 16 (j >> 2) + 4 g + (j & 3)]
//   (a hidden accumulator's MFMA row is its row of W1; a residual accumulator's MFMA row 4 g + q is feature LT16_FEAT(g) + q of its block)
template <int D, int F>
__global__ void pack_layer_tok_ffn16_kernel(const float* __restrict__ w1, const float* __restrict__ w2, uint4* __restrict__ out) {
  constexpr int NB = D / 32, FPS = D / 8, NST_ATT = 4 * NB, NFF = 2 * (F / 32);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= NFF * FPS * 64) return;
  const int lane = idx & 63, f = (idx >> 6) % FPS, ff = idx / (64 * FPS);
  const int pl = f & 1, g = lane >> 4, i = lane & 15;
  bool slice;
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
  const float* src;
  if (!slice)
    src = w1 + (long long)(32 * hb + 16 * ((f >> 1) & 1) + i) * D + 32 * (f >> 2) + LT16_FEAT(g);
  else
    src = w2 + (long long)(16 * (f >> 1) + LT16_FEAT(i >> 2) + (i & 3)) * F + 32 * hb + 4 * g;
  union {
    __bf16 b[8];
    uint4 u;
  } o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = src[16 * (j >> 2) + (j & 3)];
    const __bf16 hi = (__bf16)v;
    o.b[j] = pl ? (__bf16)(v - (float)hi) : hi;
  }
  out[(size_t)NST_ATT * FPS * 64 + idx] = o.u;
}
}  // namespace

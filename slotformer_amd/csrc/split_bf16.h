// The split-bf16 vocabulary of the kernels: an f32 value x travels as hi = bf16(x) and lo = bf16(x - hi), and a product is contracted as
// hi.lo + lo.hi + hi.hi on the bf16 MFMAs.  The splits, the fast gate functions that feed them and the two ways to fetch a fragment of a packed
// weight matrix live here, once.
#pragma once
#include <hip/hip_runtime.h>
#include "sf_vec.h"

// four f32 -> element `off` of a hi and a lo bf16 plane (8-byte stores)
__device__ __forceinline__ void sf_split4(__bf16* hp, __bf16* lp, int off, f32x4 v) {
  const bf16x4 hi = __builtin_convertvector(v, bf16x4);
  const bf16x4 lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x4), bf16x4);
  *(bf16x4*)(hp + off) = hi;
  *(bf16x4*)(lp + off) = lo;
}
// eight f32 -> hi | lo bf16 fragments
__device__ __forceinline__ void sf_split8(const f32x4 a, const f32x4 b, bf16x8& hi, bf16x8& lo) {
  const bf16x4 h0 = __builtin_convertvector(a, bf16x4), h1 = __builtin_convertvector(b, bf16x4);
  const bf16x4 l0 = __builtin_convertvector(a - __builtin_convertvector(h0, f32x4), bf16x4);
  const bf16x4 l1 = __builtin_convertvector(b - __builtin_convertvector(h1, f32x4), bf16x4);
  hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void sf_split8(const f32x8 v, bf16x8& hi, bf16x8& lo) {
  hi = __builtin_convertvector(v, bf16x8);
  lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x8), bf16x8);
}
// two f32 -> packed bf16 hi pair and lo pair
__device__ __forceinline__ void pl_split2(float a, float b, unsigned& hi, unsigned& lo) {
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{a, b}), bf16x2));
  const float fa = __builtin_bit_cast(float, hi << 16), fb = __builtin_bit_cast(float, hi & 0xffff0000u);
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2{a - fa, b - fb}), bf16x2));
}

// sigmoid / tanh on the hardware exponential (v_exp_f32, ~1 ulp): the gate arithmetic of 32 x 128 elements runs on four waves, and
// the libm forms (sf_sigmoid) took 5.6 us of a 20 us kernel; their error is far below the split-bf16 products feeding them
__device__ __forceinline__ float sf_sigmoid_fast(float x) { return __frcp_rn(1.0f + __expf(-x)); }
__device__ __forceinline__ float sf_tanh_fast(float x) { return 1.0f - 2.0f * __frcp_rn(__expf(2.0f * x) + 1.0f); }

// ---- fragment (ks, nb, plane) of a packed [N][K] matrix (pack_linear_kernel, layer_fused.hip): 64 lanes x 16 B, fetched one of two ways ----
// um_frag, an explicitly GLOBAL load: where the body runs inside a non-inlined function -- slot_chain.hip -- the pointer is generic, and a flat
// load counts on lgkmcnt as well: every LDS wait of the update would wait for the weight stream
__device__ __forceinline__ bf16x8 um_frag(const uint4* p, int nblocks, int nb, int ks, int pl, int lane) {
  typedef const uint4 __attribute__((address_space(1))) * gptr;
  return __builtin_bit_cast(bf16x8, ((gptr)p)[((long long)(ks * nblocks + nb) * 2 + pl) * 64 + lane]);
}
// ps_frag, a buffer load: the descriptor and the fragment's offset are wave-uniform -- scalar registers, scalar arithmetic -- and the only
// vector address is lane * 16; with flat 64-bit addresses per fragment the unrolled request loops spilled
__device__ __forceinline__ bf16x8 ps_frag(const uint4* p, int nblocks, int nb, int ks, int pl, int lane) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(p), 0, 0x7fffffff, 0x00020000);
  return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, lane * 16, ((ks * nblocks + nb) * 2 + pl) * 1024, 0));
}

// ---- the product of the 5 x 5 / 64 -> 64 convolutions (conv_ws.hip, conv_rows4.hip, conv_halo.hip): THE definition of its order ----
// One tap over one 32-channel half of the input channels is ONE K = 32 step of v_mfma_f32_16x16x32_bf16 per 16 x 16 tile (16 couts x 16 pixels),
// three passes in this order: x_lo w_hi, x_hi w_lo, x_hi w_hi.  Around it every kernel walks the taps ascending per cin half and adds half 0 + half 1
// last.  The chip holds a higher clock on this shape than on 32x32x16 at equal cycles per FLOP (profiles/conv_mfma_shape.md).
// Operand of a lane: row-or-column (lane & 15) of the tile, channels 8 (lane >> 4) .. + 7 of the half.  Which 16 pixels (couts) make a tile is the
// caller's: all three kernels take the pixels of one parity of a 32-pixel block, 2 (lane & 15) + p, which keeps ds_read_b128 at the 144-byte pixel
// pitch conflict-free (consecutive pixels put lanes 0-3 / 12-15 and 20-27 of a 16-lane read group on the same banks).
// W_IS_A: the weights are the A operand -- accumulator register q of a lane = cout 4 (lane >> 4) + q, pixel lane & 15; else the transpose.
template <bool W_IS_A = true>
__device__ __forceinline__ void sf_conv_tile16(const bf16x8 wh, const bf16x8 wl, const bf16x8 xh, const bf16x8 xl, f32x4& acc) {
  if constexpr (W_IS_A) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, xh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, xh, acc, 0, 0, 0);
  } else {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, wh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wh, acc, 0, 0, 0);
  }
}
// 32 couts (two tiles a; w[a][0] hi, w[a][1] lo) x one 16-pixel tile, and the whole 32-cout x 32-pixel block of a tap (pixel tiles p; acc[a][p])
template <bool W_IS_A = true>
__device__ __forceinline__ void sf_conv_half32(const bf16x8 (&w)[2][2], const bf16x8 xh, const bf16x8 xl, f32x4& acc0, f32x4& acc1) {
  sf_conv_tile16<W_IS_A>(w[0][0], w[0][1], xh, xl, acc0);
  sf_conv_tile16<W_IS_A>(w[1][0], w[1][1], xh, xl, acc1);
}
template <bool W_IS_A = true>
__device__ __forceinline__ void sf_conv_block32(const bf16x8 (&w)[2][2], const bf16x8 (&xh)[2], const bf16x8 (&xl)[2], f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) sf_conv_half32<W_IS_A>(w, xh[p], xl[p], acc[0][p], acc[1][p]);
}

// one 32x32 output tile, C[i][j] = sum_k a(i, k) b(k, j), operands read from LDS through the (row, k) -> value functors; the accumulator's
// register r holds row MM_ROW(r, lane), column lane & 31.
// BF3 = false: exact-f32 MFMA (32x32x2, 64 cycles per 2 k).  BF3 = true (library precision modes 1 / 2): the operands are
// split into bf16 hi + lo on the fly and contracted as hi*hi + hi*lo + lo*hi on the 32x32x16 bf16 MFMA -- 5x less
// matrix-pipe time per k, which is what bounds these kernels (K must then be a multiple of 16).
#define MM_ROW(r, lane) (((r) & 3) + 8 * ((r) >> 2) + 4 * ((lane) >> 5))
template <bool BF3, class FA, class FB>
__device__ __forceinline__ f32x16 sf_mm32(FA a, FB b, int K, int lane) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int i0 = lane & 31, kk = lane >> 5;
  if constexpr (BF3) {
    for (int k = 0; k < K; k += 16) {
      f32x8 av, bv;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        av[j] = a(i0, k + 8 * kk + j);
        bv[j] = b(k + 8 * kk + j, i0);
      }
      const bf16x8 ah = __builtin_convertvector(av, bf16x8), bh = __builtin_convertvector(bv, bf16x8);   // (both hi planes first: sf_split8 per
      const bf16x8 al = __builtin_convertvector(av - __builtin_convertvector(ah, f32x8), bf16x8);         //  operand schedules differently)
      const bf16x8 bl = __builtin_convertvector(bv - __builtin_convertvector(bh, f32x8), bf16x8);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    }
  } else {
    for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a(i0, k + kk), b(k + kk, i0), acc, 0, 0, 0);
  }
  return acc;
}

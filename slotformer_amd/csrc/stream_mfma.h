// Weight-streaming split-bf16 products for kernels that hold a few rows in LDS and pull whole weight matrices through one CU
// (pred_step.hip, pixel_mlp.hip, slot_update_wide.hip): fragment-ordered packed weights (sf_pack_linear_weights) as the MFMA A operand straight from
// memory, a ring of four fragment slots per wave with three chunks in flight.
#pragma once
#include "layer_fused.h"

namespace {

// the fragment ring of a wave: four slots of up to CHMAX k-steps; three chunks are in flight while one is consumed (with two slots of
// 4-6 k-steps -- one chunk in flight, 64 KB per CU -- the kernel ran at 40 GB/s: the stream is bound by latency x bytes in flight).
// PsRing<3> is 96 registers; slot_update_wide.hip, with two accumulators and twelve waves per CU, runs PsRing<2>.
template <int CHMAX>
struct PsRing {
  bf16x8 w[4][CHMAX][2];
};

template <int CH, class Ring>
__device__ __forceinline__ void ps_load(Ring& s, int slot, const uint4* p, int nblocks, int nb, int ks0, int lane) {
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    s.w[slot][k][0] = ps_frag(p, nblocks, nb, ks0 + k, 0, lane);
    s.w[slot][k][1] = ps_frag(p, nblocks, nb, ks0 + k, 1, lane);
  }
}

// chunk size for a product over KS k-steps: a multiple of four chunks of <= 3 k-steps
template <int KS>
struct PsChunk {
  static constexpr int CH = (KS % 3 == 0) ? 3 : (KS % 8 == 0) ? 2 : 1;
  static_assert(KS % CH == 0 && ((KS / CH) % 4) == 0, "a multiple of four chunks");
};

// chunks 0..2 of a product (column block nb of the packed matrix p, from k-step ks0) into slots 0..2: what ps_block expects on entry
template <int CH, class Ring>
__device__ __forceinline__ void ps_prime(Ring& s, const uint4* p, int nblocks, int nb, int ks0, int lane) {
#pragma unroll
  for (int c = 0; c < 3; ++c) ps_load<CH>(s, c, p, nblocks, nb, ks0 + c * CH, lane);
}

// The product every user of the ring runs: NC chunks of CH k-steps, for NRB blocks of 32 tokens on one set of fragment reads,
//   acc[rb][4 g + q] += out[token = 32 rb + (lane & 31)][column 32 nb + 8 g + 4 (lane >> 5) + q]
// over k-steps ks0 .. ks0 + NC CH - 1 of column block nb of the packed matrix p (X planes: k-step 0 at the pointer).  Chunks 0..2 must already be
// in slots S0 .. S0 + 2; every iteration requests the chunk three ahead -- behind the end of this product, chunks 0..2 of the NEXT one (pn,
// nblocksn, nbn, ksn: chunks of CHN k-steps; pn NULL: none), which therefore starts at slot (S0 + NC) & 3.
template <int NC, int CH, int CHN, int S0, int NRB, class Ring>
__device__ __forceinline__ void ps_ring_block(f32x16* acc, Ring& s, const uint4* p, int nblocks, int nb, int ks0, const uint4* pn, int nblocksn,
                                              int nbn, int ksn, const __bf16* Xh, const __bf16* Xl, int stride, int lane) {
  const int ao = (lane & 31) * stride + 8 * (lane >> 5);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c + 3 < NC)
      ps_load<CH>(s, (S0 + c + 3) & 3, p, nblocks, nb, ks0 + (c + 3) * CH, lane);
    else if (pn)
      ps_load<CHN>(s, (S0 + c + 3) & 3, pn, nblocksn, nbn, ksn + (c + 3 - NC) * CHN, lane);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int ks = c * CH + k;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        const bf16x8 xh = *(const bf16x8*)(Xh + ao + rb * 32 * stride + ks * 16), xl = *(const bf16x8*)(Xl + ao + rb * 32 * stride + ks * 16);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s.w[(S0 + c) & 3][k][0], xl, acc[rb], 0, 0, 0);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s.w[(S0 + c) & 3][k][1], xh, acc[rb], 0, 0, 0);
        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(s.w[(S0 + c) & 3][k][0], xh, acc[rb], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);   // the requests stay one ring slot per chunk: hoisted further they spill
  }
}

// a product over KS k-steps from slot 0 (KS / CH is a multiple of four: the next product starts at slot 0 too), one token block / NRB of them
template <int KS, int CHN, class Ring>
__device__ __forceinline__ void ps_block(f32x16& acc, Ring& s, const uint4* p, int nblocks, int nb, int ks0, const uint4* pn, int nblocksn,
                                         int nbn, int ksn, const __bf16* Xh, const __bf16* Xl, int stride, int lane) {
  ps_ring_block<KS / PsChunk<KS>::CH, PsChunk<KS>::CH, CHN, 0, 1>(&acc, s, p, nblocks, nb, ks0, pn, nblocksn, nbn, ksn, Xh, Xl, stride, lane);
}
template <int KS, int CHN, int NRB, class Ring>
__device__ __forceinline__ void ps_blockN(f32x16 (&acc)[NRB], Ring& s, const uint4* p, int nblocks, int nb, int ks0, const uint4* pn,
                                          int nblocksn, int nbn, int ksn, const __bf16* Xh, const __bf16* Xl, int stride, int lane) {
  ps_ring_block<KS / PsChunk<KS>::CH, PsChunk<KS>::CH, CHN, 0, NRB>(acc, s, p, nblocks, nb, ks0, pn, nblocksn, nbn, ksn, Xh, Xl, stride, lane);
}
}  // namespace

// Row and key arithmetic of the q | k | v head projection, shared by its two homes: the row-tile attention form (qkv_rows_body, attn_rows.hip) and the
// FFN launch that runs the NEXT layer's projection on its finished rows (ffn_qkv_tile_kernel, ffn_tile.hip).
#pragma once

// position of key t inside its video's v^T rows: the score accumulators of a 32x32 MFMA hold keys (r & 3) + 8 (r >> 2) + 4 (lane >> 5),
// and eight consecutive registers are one B fragment of the PV product -- bits 2 and 3 of the key index trade places
__device__ __forceinline__ int vpos(int t) { return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1); }

// m / L for 0 <= m < 2^22 (one float multiply and two corrections instead of a 32-bit integer division)
__device__ __forceinline__ int div_rows(int m, int L, float invL) {
  int q = (int)((float)m * invL);
  q -= (q * L > m);
  q += ((q + 1) * L <= m);
  return q;
}

// chunk gc of a wave's weight stream over the packed q|k|v matrix (sf_pack_attn_weights) into its ring slot, gc & 3: chunk gc = group index * 8 +
// (k-step / 2) counted from group g0; buffer loads with scalar fragment offsets.  hpb: byte offset of the head's fragments of group 0.
__device__ __forceinline__ void qh_load_chunk(bf16x8 (&ring)[4][2][2], const __amdgpu_buffer_rsrc_t wrs, unsigned hpb, int g0, int gc, int lane) {
  const int g = g0 + gc / 8, ks0 = (gc % 8) * 2;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
      ring[gc & 3][k][pl] = __builtin_bit_cast(
          bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, (unsigned)(lane * 16), hpb + (unsigned)((g * 16 + ks0 + k) * 2048 + pl * 1024), 0));
}

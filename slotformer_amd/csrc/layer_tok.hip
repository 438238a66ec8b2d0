// One nn.TransformerEncoderLayer (norm_first, relu; d_model 256, 8 heads, ffn 1024) of the rollout Transformer in a TOKEN-STATIONARY form:
//     x2 = x + out_proj(MHA(LN1(x))) + b_o ;   y = x2 + lin2(relu(lin1(LN2(x2))))          (slotformer.py:72-80, torch nn.TransformerEncoderLayer)
// A workgroup owns WHOLE videos -- vpw = 128 / L of them, up to 128 token rows -- and each of its four waves (one per SIMD, up to 512 registers) owns 32
// tokens for the whole layer.  Every linear product runs transposed, D^T[feature][token] = W . A^T, with the wave's activations as the MFMA B operand in
// registers: the accumulator layout of a 32 x 32 block (lane = (token, half h), registers = features 8 g + 4 h + q) IS a B operand of the next product once
// the weight fragments are packed with the matching permuted k order (ffn_tok.hip established this for the FFN pair).  So LN1 -> q|k|v -> scores ->
// softmax -> PV -> out-projection -> LN2 -> FFN1 -> ReLU -> FFN2 is ONE chain of register-resident products per wave:
//   * the residual stream lives in the accumulators the out-projection / FFN2 add into (x + b_o, then x2 + b2, are their initial values);
//   * waves share WEIGHTS, not activations: the layer's 3 MB of split-bf16 fragments, packed in consumption order (sf_pack_layer_tok_weights: 96 stages of
//     32 fragments = one 32-row block of a matrix each), stream global -> LDS through a three-stage ring (global_load_lds, one fragment per
//     wave-instruction, a counted vmcnt wait + ONE barrier per stage);
//   * the only activations that cross waves are a head's keys and values: the owner writes its k accumulators as they lie (they are the A fragments of
//     S^T = K Q^T) and computes v with the MFMA operands swapped, which leaves V^T fragments (lane = dim, registers = keys) in its accumulators --
//     32 KB of LDS per head, handed over by the stage barriers; the scores of a wave's 32 queries against the (at most three) 32-key blocks that hold
//     their videos' tokens stay in registers through the softmax and feed the PV product as its B operand.
//   * the FFN block (LN2, lin1, ReLU, lin2: 3072 of a layer's 4896 MFMAs' worth) runs on v_mfma_f32_16x16x32_bf16 over the wave's two 16-token tiles (the
//     lt16_* helpers of layer_tok_common.h): same MFMA cycles, same 32 KB stages of 32 fragments, and the chip holds a higher clock on that shape when the
//     other half of it is busy (profiles/layer_tok_mfma_shape.md).  The residual stream changes layout in place at the two borders of the block, one
//     v_permlane16_swap per register pair; the attention block, bound by VALU issue, keeps 32x32x16.
// No activation plane, no q|k|v round trip through memory, no per-video attention launch: a layer is one launch of ceil(B / vpw) workgroups
// (43 for a rollout unit of 128 videos at L = 42) instead of 84 FFN + 128 attention workgroups over two launches.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "layer_fused.h"
#include "layer_tok_common.h"
#include <stdlib.h>

namespace {
constexpr int LT_NT = 256, LT_D = 256, LT_F = 1024, LT_NH = 8, LT_TOK = 128, LT_MAXL = 8;
constexpr int LT_STAGE = 32 * 1024, LT_RING = 3;
constexpr int LT_NST_ATT = 4 * LT_NH, LT_NST = LT_NST_ATT + 2 * (LT_F / 32);   // 32 attention + 64 FFN stages per layer
constexpr int LT_KV = LT_RING * LT_STAGE;     // K fragments [s][plane][token block][64 lanes] x 16 B, then V^T fragments [token block][s][plane][64 lanes] x 16 B
constexpr int LT_VT = LT_KV + 16 * 1024;
constexpr int LT_PAR = LT_KV + 32 * 1024;     // the layer's vectors (f32)
constexpr int P_LN1G = 0, P_LN1B = 256, P_BQKV = 512, P_BO = 1280, P_LN2G = 1536, P_LN2B = 1792, P_B1 = 2048, P_B2 = 3072, P_N = 3328;
constexpr size_t LT_LDS = (size_t)LT_PAR + (size_t)P_N * 4;
constexpr size_t LT_BLOB = (size_t)LT_NST * LT_STAGE + (size_t)P_N * 4;   // a layer's fragments + its vectors
static_assert(LT_LDS <= 160 * 1024, "LDS budget");

struct LtArgs {
  const float* x;      // MODE 0: [B * L][256] rows
  const float* ring;   // MODE 1: projection ring [B][RF][N][256] ...
  const float* pe;     //         ... + position table [L][256]
  float* y;            // [B * L][256]
  const char* blob[LT_MAXL];   // sf_pack_layer_tok_weights copies of the layers this launch runs
  float eps;
  int nl, B, L, vpw, RF, N, f0, dbg_ts;
};
}  // namespace

__device__ long long lt_ts[16];   // wall-clock stamps of workgroup 0, wave 0 (SF_DBG=lt; sf_debug_read_ts_layer_tok)
#define LTS(i) do { if (A.dbg_ts && blockIdx.x == 0 && threadIdx.x == 0) lt_ts[i] = wall_clock64(); } while (0)

template <int MODE>
__global__ __launch_bounds__(LT_NT) void layer_tok_kernel(LtArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* P = (float*)(smem + LT_PAR);
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int n = lane & 31, h = lane >> 5;
  const int L = A.L;
  const int v0 = blockIdx.x * A.vpw;
  const int nvalid = min(A.vpw, A.B - v0) * L;   // token rows of this workgroup's videos
  const int tl = wave * 32 + n;
  const int te = min(tl, nvalid - 1);             // (rows past the end repeat the last one: finite values, never stored)
  const int vl = te / L, tok = te - vl * L;
  const long long row = (long long)(v0 + vl) * L + tok;
  LTS(0);
  // ---- the token's row in accumulator layout: X[ob][4 g + q] = x[32 ob + 8 g + 4 h + q] ----
  f32x16 X[8];
  if constexpr (MODE == 0) {
    const float* xr = A.x + row * LT_D + 4 * h;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = *(const f32x4*)(xr + 32 * ob + 8 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) X[ob][4 * g + q] = v[q];
      }
  } else {
    // layer 0 of a rollout step: x = ring[b][(f0 + tok / N) % RF][tok % N] + pe[tok]   (slotformer.py:115-117; the in-projections are cached per frame)
    const int fr = tok / A.N, sl = tok - fr * A.N;
    const float* rr = A.ring + (((long long)(v0 + vl) * A.RF + (A.f0 + fr) % A.RF) * A.N + sl) * LT_D + 4 * h;
    const float* pr = A.pe + (long long)tok * LT_D + 4 * h;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = *(const f32x4*)(rr + 32 * ob + 8 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) X[ob][4 * g + q] = v[q];
      }
    __builtin_amdgcn_sched_barrier(0);   // (the position rows behind the ring rows, a block at a time: 64 vectors in flight at once do not fit)
#pragma unroll
    for (int ob = 0; ob < 8; ++ob) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = *(const f32x4*)(pr + 32 * ob + 8 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) X[ob][4 * g + q] += v[q];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // ---- weight ring: the launch's stages (96 per layer, layer after layer) are ONE stream; stage gs lives in slot gs % 3; this wave copies fragments
  //      8 wave .. 8 wave + 7 of every stage, one per fragment group of the product that runs two stages earlier ----
  const unsigned wlane = (unsigned)(wave * 8 * 1024 + lane * 16);
  char* const wdst = smem + (wave * 8) * 1024;
  // prefetch cursor: the stage two ahead of consumer stage cs of the current layer -- stage cs + 2 of this layer's blob, the first two stages of the next
  // layer's behind the end, and past the end of the launch the last stage again (re-requested into a free slot: every stage issues its eight pieces, one
  // wait count fits all).  Scalar selects only: a branch here would split the stage's basic block (and the side work sinks into the block of its use).
  int cur = 0;   // slot of the next stage to be consumed
  int cs = -2;   // consumer stage inside the current layer (the two calls of the prologue request stages 0 and 1)
  const char* base_cur = A.blob[0];
  const char* base_nxt = A.blob[0];
  bool last_layer = false;
  auto stage_src = [&]() -> const char* {
    const int t2 = cs + 2;
    const bool wrap = t2 >= LT_NST;
    const char* b = wrap ? base_nxt : base_cur;
    const int so = wrap ? (last_layer ? LT_NST - 1 : t2 - LT_NST) : t2;
    ++cs;
    return b + (size_t)so * LT_STAGE + wlane;
  };
  {
    const char* s0 = stage_src();
    const char* s1 = stage_src();
    LtRing R0{nullptr, s0, wdst}, R1{nullptr, s1, wdst + LT_STAGE};
#pragma unroll
    for (int f = 0; f < 8; ++f) lt_dma(R0, f);
#pragma unroll
    for (int f = 0; f < 8; ++f) lt_dma(R1, f);
  }
  // the stage about to be consumed has landed (every wave waits for its own pieces, then the barrier), every wave is done with the previous one
  // (whose slot the pieces of stage gs + 2 go to), LDS writes of the previous stage (keys / values) are visible
#ifdef LT_STAMPS
  long long c_wait = 0, c_bar = 0, c_last = 0, c_work = 0;   // shader cycles (s_memtime) of workgroup 0's wave 0: DMA waits, barrier waits, everything else
#endif
  auto stage_begin = [&]() -> LtRing {
#ifdef LT_STAMPS
    const long long c0 = __builtin_readcyclecounter();
    if (c_last) c_work += c0 - c_last;
#endif
#ifdef LT_NODMA
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
#endif
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#ifdef LT_STAMPS
    const long long c1 = __builtin_readcyclecounter();
#endif
#ifndef LT_NOBAR
    __builtin_amdgcn_s_barrier();
#endif
    asm volatile("" ::: "memory");
#ifdef LT_STAMPS
    c_last = __builtin_readcyclecounter();
    c_wait += c1 - c0;
    c_bar += c_last - c1;
#endif
    const int nb = cur == 0 ? 2 : cur - 1;
    LtRing R{smem + cur * LT_STAGE + lane * 16, stage_src(), wdst + nb * LT_STAGE};
#ifdef LT_BURST
#pragma unroll
    for (int f = 0; f < 8; ++f) lt_dma_now(R, f);
#endif
    cur = cur == 2 ? 0 : cur + 1;
    return R;
  };
  // ---- key blocks this wave's queries need: the tokens of the videos its 32 rows belong to (at most three 32-key blocks, sf_layer_tok_ok); a block
  //      index past the last one is clamped for the READS (finite values), its keys fail the range test of the mask ----
  const int wf = min(wave * 32, nvalid - 1);
  const int kb0 = ((wf / L) * L) >> 5;
  const int d0 = 32 * kb0 + 4 * h - vl * L;   // key index of register (kbi, 4 g + q) minus the video's first key: d0 + 32 kbi + 8 g + q
  const char* pb;   // the vectors as this lane reads them: + 4 h floats; opaque, so that every read is this base + an immediate offset
  {
    unsigned pbo = (unsigned)(LT_PAR + 16 * h);
    asm volatile("" : "+v"(pbo));
    pb = smem + pbo;
  }
  // ... and as the 16x16 tiles of the FFN block read them (g16 = lane >> 4): px + LT16_FEAT(g16) floats for the vectors over the residual stream's
  // features, pg + 4 g16 floats for the lin1 bias (a hidden accumulator's MFMA rows are its hidden units in order)
  const int g16 = lane >> 4;
  const char *px, *pg;
  {
    unsigned pxo = (unsigned)(LT_PAR + 4 * LT16_FEAT(g16)), pgo = (unsigned)(LT_PAR + 16 * g16);
    asm volatile("" : "+v"(pxo), "+v"(pgo));
    px = smem + pxo;
    pg = smem + pgo;
  }
  char* const kwr = smem + LT_KV + wave * 1024 + lane * 16;          // + (s * 2 + plane) * 4096
  char* const vwr = smem + LT_VT + wave * 4096 + lane * 16;          // + (s * 2 + plane) * 1024
  const char* krd[3];
  const char* vrd[3];
#pragma unroll
  for (int kbi = 0; kbi < 3; ++kbi) {
    const int kb = min(kb0 + kbi, 3);
    krd[kbi] = smem + LT_KV + kb * 1024 + lane * 16;                 // + (s * 2 + plane) * 4096
    vrd[kbi] = smem + LT_VT + kb * 4096 + lane * 16;                 // + (s * 2 + plane) * 1024
  }
  const float qscale = 0.2550348616841918f;   // log2(e) / sqrt(32): the scores in the exponent's base
  constexpr float NEG = -3.0e38f;
  LTS(1);

#pragma unroll 1
  for (int l = 0; l < A.nl; ++l) {
    cs = 0;
    base_cur = A.blob[l];
    last_layer = l + 1 >= A.nl;
    base_nxt = A.blob[last_layer ? l : l + 1];
    // ---- the layer's vectors -> LDS (behind the first barrier every wave is done with the previous layer's) ----
    __syncthreads();
    {
      const float* vsrc = (const float*)(A.blob[l] + (size_t)LT_NST * LT_STAGE);
      for (int i = t; i < P_N / 4; i += LT_NT) *(f32x4*)(P + 4 * i) = *(const f32x4*)(vsrc + 4 * i);
    }
    __syncthreads();
    if (l == 0) LTS(2);
    // ================================================= attention block =================================================
    bf16x8 xh[16], xl[16];
    lt_layernorm<P_LN1G, P_LN1B>(X, pb, h, A.eps, xh, xl);
    lt_add_vec<P_BO>(X, pb);   // X = x + b_o: the out-projection slices add into it
    if (l == 0) LTS(3);
    // One head behind: while head i's q / k / v products run, the scores / softmax / PV of head i - 1 are their side work.
    //   D_i [Wq_i]:      S^T(i - 1) = K Q^T;  q(i) product   | mask, max, first exponentials of head i - 1
    //   A_i [Wk_i]:      k(i) product                         | remaining exponentials, sum, P -> hi | lo fragments;   then O(i - 1) = V^T P
    //   B_i [Wv_i]:      v(i) product (operands swapped)      | k(i) -> K fragments in LDS, q(i) -> fragments, O(i - 1) / sum -> fragments
    //   C_i [Wo_{i-1}]:  X += Wo[:, head i - 1] O(i - 1)      | v(i) -> V^T fragments in LDS
    // K / V^T of ONE head live in LDS: K(i) is written behind barrier B_i (the last reader of K(i - 1) is S^T(i - 1) in D_i), V^T(i) behind barrier C_i
    // (the last reader of V^T(i - 1) is the PV product at the end of A_i).
    f32x16 qa, ka, va, S[3], O;
    bf16x8 qh[2], ql[2], ph[3][2], pl[3][2], oh[2], ol[2];
    float mx0 = NEG, mx1 = NEG, mx = 0.f, sm = 0.f, rinv = 0.f;
    auto zero16 = [](f32x16& a) {
#pragma unroll
      for (int r = 0; r < 16; ++r) a[r] = 0.f;
    };
    int hq = 0;   // head whose q / k / v products run (a runtime value inside the loop)
    // -- pieces of side work --
    auto mask_chunk = [&](int c) {   // registers 8 (c & 1) .. + 7 of score block c >> 1: keys of other videos -> NEG; running maxima
      const int kbi = c >> 1;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int r = 8 * (c & 1) + rr;
        const bool ok = (unsigned)(d0 + 32 * kbi + 8 * (r >> 2) + (r & 3)) < (unsigned)L;
        const float v = ok ? S[kbi][r] : NEG;
        S[kbi][r] = v;
        if (rr & 1) mx1 = fmaxf(mx1, v); else mx0 = fmaxf(mx0, v);
      }
    };
    auto exp_chunk = [&](int c) {
      const int kbi = c >> 1;
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int r = 8 * (c & 1) + rr;
#ifdef LT_EXPF
        const float e = __expf((S[kbi][r] - mx) * 0.6931471805599453f);
#else
        const float e = __builtin_amdgcn_exp2f(S[kbi][r] - mx);
#endif
        S[kbi][r] = e;
        if (rr & 1) s1 += e; else s0 += e;
      }
      sm += s0 + s1;
    };
    auto psplit_chunk = [&](int c) { sf_split8(quad(S[c >> 1], 2 * (c & 1)), quad(S[c >> 1], 2 * (c & 1) + 1), ph[c >> 1][c & 1], pl[c >> 1][c & 1]); };
    auto kconv = [&](int s) {
      const float* bk = (const float*)pb + P_BQKV + 256 + 32 * hq;
      bf16x8 fh, fl;
      sf_split8(quad(ka, 2 * s) + *(const f32x4*)(bk + 16 * s), quad(ka, 2 * s + 1) + *(const f32x4*)(bk + 16 * s + 8), fh, fl);
      *(bf16x8*)(kwr + (s * 2) * 4096) = fh;
      *(bf16x8*)(kwr + (s * 2 + 1) * 4096) = fl;
    };
    auto qconv = [&](int s) {
      const float* bq = (const float*)pb + P_BQKV + 32 * hq;
      sf_split8((quad(qa, 2 * s) + *(const f32x4*)(bq + 16 * s)) * qscale, (quad(qa, 2 * s + 1) + *(const f32x4*)(bq + 16 * s + 8)) * qscale, qh[s], ql[s]);
    };
    auto vconv = [&](int s) {
      const float bv = P[P_BQKV + 512 + 32 * hq + n];
      bf16x8 fh, fl;
      sf_split8(quad(va, 2 * s) + bv, quad(va, 2 * s + 1) + bv, fh, fl);
      *(bf16x8*)(vwr + (s * 2) * 1024) = fh;
      *(bf16x8*)(vwr + (s * 2 + 1) * 1024) = fl;
    };
    auto oconv = [&](int s) { sf_split8(quad(O, 2 * s) * rinv, quad(O, 2 * s + 1) * rinv, oh[s], ol[s]); };
    // scores of the previous head: S^T[key][query] = K Q^T for the wave's three key blocks (q fragments of the previous B stage)
    auto scores = [&]() {
      bf16x8 kh[3][2], kl[3][2];
#pragma unroll
      for (int kbi = 0; kbi < 3; ++kbi)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          kh[kbi][s] = *(const bf16x8*)(krd[kbi] + (s * 2) * 4096);
          kl[kbi][s] = *(const bf16x8*)(krd[kbi] + (s * 2 + 1) * 4096);
        }
#pragma unroll
      for (int kbi = 0; kbi < 3; ++kbi) zero16(S[kbi]);
      // (the three blocks' accumulators in turn: no two consecutive MFMAs on one accumulator)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { S[kbi] = LT_MFMA(kh[kbi][s], ql[s], S[kbi]); LT_PIN(); }
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { S[kbi] = LT_MFMA(kl[kbi][s], qh[s], S[kbi]); LT_PIN(); }
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { S[kbi] = LT_MFMA(kh[kbi][s], qh[s], S[kbi]); LT_PIN(); }
      }
      mx0 = mx1 = NEG;
      sm = 0.f;
    };
    auto pv = [&]() {
      f32x16 Op[3];
      bf16x8 vh[3][2], vlo[3][2];
#pragma unroll
      for (int kbi = 0; kbi < 3; ++kbi)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          vh[kbi][s] = *(const bf16x8*)(vrd[kbi] + (s * 2) * 1024);
          vlo[kbi][s] = *(const bf16x8*)(vrd[kbi] + (s * 2 + 1) * 1024);
        }
#pragma unroll
      for (int kbi = 0; kbi < 3; ++kbi) zero16(Op[kbi]);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { Op[kbi] = LT_MFMA(vh[kbi][s], pl[kbi][s], Op[kbi]); LT_PIN(); }
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { Op[kbi] = LT_MFMA(vlo[kbi][s], ph[kbi][s], Op[kbi]); LT_PIN(); }
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { Op[kbi] = LT_MFMA(vh[kbi][s], ph[kbi][s], Op[kbi]); LT_PIN(); }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) O[r] = (Op[0][r] + Op[1][r]) + Op[2][r];
    };
    auto sideD = [&](int g) {
      if (g < 6) mask_chunk(g);
      if (g == 6) mx = lt_xmax(fmaxf(mx0, mx1), h);
      if (g == 7) exp_chunk(0);
    };
    auto sideA = [&](int g) {
      if (g == 0) { exp_chunk(1); exp_chunk(2); }
      if (g == 1) { exp_chunk(3); exp_chunk(4); }
      if (g == 2) { exp_chunk(5); rinv = 1.0f / lt_xsum(sm, h); psplit_chunk(0); }
      if (g == 3) { psplit_chunk(1); psplit_chunk(2); }
      if (g == 4) { psplit_chunk(3); psplit_chunk(4); }
      if (g == 5) psplit_chunk(5);
    };
    // ---- head 0: nothing behind it yet ----
    {
      const LtRing R = stage_begin();   // D_0
      lt_row_product<false, 0>(R, xh, xl, qa, LtNoSide{});
    }
    {
      const LtRing R = stage_begin();   // A_0
      lt_row_product<false, 0>(R, xh, xl, ka, LtNoSide{});
    }
    {
      const LtRing R = stage_begin();   // B_0
      lt_row_product<true, 5>(R, xh, xl, va, [&](int g) {
        if (g < 2) kconv(g);
        else if (g < 4) qconv(g - 2);
      });
      vconv(0);
      vconv(1);
    }
#pragma unroll 1
    for (hq = 1; hq < LT_NH; ++hq) {
      {
        const LtRing R = stage_begin();   // D_i
        scores();
          lt_row_product<false, 6>(R, xh, xl, qa, sideD);
      }
      {
        const LtRing R = stage_begin();   // A_i
          lt_row_product<false, 6>(R, xh, xl, ka, sideA);
        pv();
      }
      {
        const LtRing R = stage_begin();   // B_i
          lt_row_product<true, 5>(R, xh, xl, va, [&](int g) {
          if (g < 2) kconv(g);
          else if (g < 4) qconv(g - 2);
          else if (g < 6) oconv(g - 4);
        });
      }
      {
        const LtRing R = stage_begin();   // C_i
        lt_kslice_product<5>(R, oh, ol, X, [&](int g) {
          if (g < 2) vconv(g);
        });
      }
    }
    // ---- head 7's scores, softmax and PV have no product left to hide under ----
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();   // V^T(7) of every wave is in LDS
    asm volatile("" ::: "memory");
    scores();
#pragma unroll
    for (int g = 0; g < 8; ++g) sideD(g);
#pragma unroll
    for (int g = 0; g < 6; ++g) sideA(g);
    pv();
    oconv(0);
    oconv(1);
    {
      const LtRing R = stage_begin();   // C_8
      lt_kslice_product<0>(R, oh, ol, X, LtNoSide{});
    }
    if (l == 0) LTS(4);
#ifdef LT_STAMPS
    if (l == 0 && blockIdx.x == 0 && threadIdx.x == 0) { lt_ts[8] = c_wait; lt_ts[9] = c_bar; lt_ts[10] = c_work; }
#endif
    // ==================================================== FFN block ====================================================
    // X = x2; LN2 -> fragments; X += b2 becomes the accumulator of the second product.  Stage order W1_0, (W1_j, W2_{j-1}) for j = 1..31, W2_31: block
    // j - 1's bias / ReLU / hi | lo split is the side work of block j's first product.
    // The whole block runs on 16x16x32 MFMAs (layer_tok_common.h): the residual stream moves to the 16-layout here and back behind the last slice, one
    // v_permlane16_swap per register pair each way; a tile t = the wave's tokens 16 t .. 16 t + 15.
    lt16_swap_layout(X);
    lt16_layernorm<P_LN2G, P_LN2B>(X, px, g16, A.eps, xh, xl);
    lt16_add_vec<P_B2>(X, px);
    if (l == 0) LTS(5);
    f32x4 Ha[2][2], Hb[2][2];   // [row half][tile]
    bf16x8 hh[2], hl[2];        // [tile]
    f32x4 b1q[2];   // lin1 bias of the block being converted, requested a stage ahead (a read inside the side work would hold its VALU back)
    auto b1_load = [&](int blk) {
      const float* b1 = (const float*)pg + P_B1 + 32 * blk;
#pragma unroll
      for (int r = 0; r < 2; ++r) b1q[r] = *(const f32x4*)(b1 + 16 * r);
    };
    // bias, ReLU and hi | lo split of a hidden block in EIGHT pieces, one per fragment group of the product they hide under (an MFMA of 16 cycles hides two
    // VALU instructions, a clump of forty stalls the matrix pipe): piece k = packed word k & 3 (row half (k & 3) >> 1) of the fragments of tile k >> 2
    typedef unsigned __attribute__((ext_vector_type(4))) lt_u32x4;
    lt_u32x4 hw[2], lw[2];
    auto hconv_piece = [&](const f32x4 (&Hx)[2][2], int k) {
      const int t16 = k >> 2, w = k & 3, r = w >> 1, e = 2 * (w & 1);
      unsigned hi, lo;
      pl_split2(fmaxf(Hx[r][t16][e] + b1q[r][e], 0.f), fmaxf(Hx[r][t16][e + 1] + b1q[r][e + 1], 0.f), hi, lo);
      hw[t16][w] = hi;
      lw[t16][w] = lo;
    };
    auto hconv_done = [&]() {
#pragma unroll
      for (int t16 = 0; t16 < 2; ++t16) {
        hh[t16] = __builtin_bit_cast(bf16x8, hw[t16]);
        hl[t16] = __builtin_bit_cast(bf16x8, lw[t16]);
      }
    };
    // one step = [W1_j: first product of block j into Hn | bias / ReLU / split of block j - 1 (Hp)] + [W2_{j-1}: second product of block j - 1]
    auto ffn_step = [&](f32x4 (&Hn)[2][2], const f32x4 (&Hp)[2][2], int j) {
      {
        const LtRing R = stage_begin();
        lt16_row_product<2, 8>(R, xh, xl, Hn, [&](int ks) { hconv_piece(Hp, ks); });
        hconv_done();
        asm volatile("" : "+v"(hh[0]), "+v"(hh[1]), "+v"(hl[0]), "+v"(hl[1]));   // (the conversion belongs to THIS stage's MFMA stream)
      }
      {
        const LtRing R = stage_begin();
        b1_load(j);
        lt16_kslice_product<0>(R, hh, hl, X, LtNoSide{});
      }
    };
    {
      const LtRing R = stage_begin();
      b1_load(0);
      lt16_row_product<0, 8>(R, xh, xl, Ha, LtNoSide{});
    }
    ffn_step(Hb, Ha, 1);
#pragma unroll 1
    for (int j = 2; j < LT_F / 32; j += 2) {   // (two steps per trip: the accumulators trade places without a copy)
      ffn_step(Ha, Hb, j);
      ffn_step(Hb, Ha, j + 1);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) hconv_piece(Hb, k);
    hconv_done();
    {
      const LtRing R = stage_begin();
      lt16_kslice_product<0>(R, hh, hl, X, LtNoSide{});
    }
    lt16_swap_layout(X);
    if (l == 0) LTS(6);
#ifdef LT_STAMPS
    if (l == 0 && blockIdx.x == 0 && threadIdx.x == 0) { lt_ts[11] = c_wait; lt_ts[12] = c_bar; lt_ts[13] = c_work; }
#endif
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-requested last stage: no LDS write may be pending when the workgroup leaves
  // ---- finished rows ----
  if (tl < nvalid) {
    float* yr = A.y + row * LT_D + 4 * h;
#pragma unroll
    for (int ob = 0; ob < 8; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g) *(f32x4*)(yr + 32 * ob + 8 * g) = quad(X[ob], g);
  }
  LTS(7);
}

extern "C" int sf_debug_read_ts_layer_tok(long long* out16) {
  hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(lt_ts), sizeof(long long) * 16);
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" size_t sf_layer_tok_packed_bytes(void) { return LT_BLOB; }
// ... of a layer of the given shape: 0 for a shape no token-stationary kernel covers
extern "C" size_t sf_layer_tok_packed_bytes_ex(int d_model, int num_heads, int ffn) {
  if (d_model == LT_D && num_heads == LT_NH && ffn == LT_F) return LT_BLOB;
  return sf_layer_tok128_shape(d_model, num_heads, ffn) ? sf_layer_tok128_packed_bytes() : 0;
}

// the layer's four matrices as fragments in consumption order + its eight vectors (all pointers of `w` device, torch layouts): 96 stages of 32 KB --
// 32 attention stages of 32x32x16 fragments, 64 FFN stages of 16x16x32 fragments (element map: layer_tok_common.h) -- then 3328 floats: norm1 g, b,
// in_proj b, out_proj b, norm2 g, b, lin1 b, lin2 b
extern "C" int sf_pack_layer_tok_weights(const sf_tfm_layer* w, void* packed, int d_model, int num_heads, int ffn, void* stream) {
  SF_REQUIRE(w && packed, "sf_pack_layer_tok_weights: null pointer");
  SF_REQUIRE(w->in_proj_w && w->out_proj_w && w->lin1_w && w->lin2_w && w->norm1_g && w->norm1_b && w->in_proj_b && w->out_proj_b && w->norm2_g &&
                 w->norm2_b && w->lin1_b && w->lin2_b, "sf_pack_layer_tok_weights: null weight");
  hipStream_t st = (hipStream_t)stream;
  if (sf_layer_tok128_shape(d_model, num_heads, ffn)) return sf_pack_layer_tok128(w, packed, st);
  SF_REQUIRE(d_model == LT_D && num_heads == LT_NH && ffn == LT_F, "sf_pack_layer_tok_weights: (d_model, heads, ffn) = (256, 8, 1024) or (128, 8, 512) only");
  // the attention stages in the 32x32x16 fragment order (the grid stops at the first FFN stage), the FFN stages in the 16x16x32 one
  constexpr int n_att = LT_NST_ATT * 32 * 64, n_ffn = (LT_NST - LT_NST_ATT) * 32 * 64;
  static_assert(n_att % 256 == 0 && n_ffn % 256 == 0, "whole blocks");
  hipLaunchKernelGGL((pack_layer_tok_kernel<LT_D, LT_F>), dim3(n_att / 256), dim3(256), 0, st, w->in_proj_w, w->out_proj_w, w->lin1_w, w->lin2_w, (uint4*)packed);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL((pack_layer_tok_ffn16_kernel<LT_D, LT_F>), dim3(n_ffn / 256), dim3(256), 0, st, w->lin1_w, w->lin2_w, (uint4*)packed);
  SF_CHECK_LAUNCH();
  float* vec = (float*)((char*)packed + (size_t)LT_NST * LT_STAGE);
  const struct {
    const float* src;
    int off, n;
  } parts[8] = {{w->norm1_g, P_LN1G, 256}, {w->norm1_b, P_LN1B, 256}, {w->in_proj_b, P_BQKV, 768}, {w->out_proj_b, P_BO, 256},
                {w->norm2_g, P_LN2G, 256}, {w->norm2_b, P_LN2B, 256}, {w->lin1_b, P_B1, 1024},   {w->lin2_b, P_B2, 256}};
  for (const auto& p : parts) {
    const hipError_t e = hipMemcpyAsync(vec + p.off, p.src, (size_t)p.n * 4, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  }
  return 0;
}

// Videos per 128-token workgroup for sequences of L tokens: the largest count of WHOLE videos for which the keys of the videos a wave's 32 rows belong to
// lie inside three 32-key blocks (42 tokens: 3; 50 tokens: 1 -- two would put the keys of wave 1's rows in four blocks; 65..96 tokens, the reference's
// Physion window of 15 frames x 6 slots: 1, the last wave(s) idle); 0: the sequence does not fit a workgroup
int sf_layer_tok_vpw(int L) {
  if (L < 1 || L > 96) return 0;
  for (int vpw = LT_TOK / L; vpw >= 1; --vpw) {
    const int nvalid = vpw * L;
    bool ok = true;
    for (int w = 0; w < 4 && ok; ++w) {
      const int wf = w * 32 < nvalid ? w * 32 : nvalid - 1, wl = w * 32 + 31 < nvalid ? w * 32 + 31 : nvalid - 1;
      const int kb0 = ((wf / L) * L) >> 5, kb1 = (((wl / L) * L) + L - 1) >> 5;
      ok = kb1 - kb0 + 1 <= 3;
    }
    if (ok) return vpw;
  }
  return 0;
}
bool sf_layer_tok_ok(int L) { return sf_layer_tok_vpw(L) > 0; }

// `nl` consecutive layers in ONE launch.  mode 0: xin [B * L][256] rows;  mode 1: the first of them is layer 0 of a rollout step --
// x = ring[b][(f0 + r / nslots) % ring_frames][r % nslots] + pe[r].  y [B * L][256] finished rows of the last of them.
int sf_layer_tok_ex(int mode, const float* xin, const float* ring, int ring_frames, int nslots, int f0, const float* pe, const sf_tfm_layer* layers, int nl,
                    float eps, float* y, int B, int L, hipStream_t st) {
  bool ok = layers && nl >= 1 && nl <= LT_MAXL && sf_layer_tok_ok(L) && B >= 1 && y && (mode == 0 ? xin != nullptr : (ring && pe && nslots >= 1 && ring_frames >= 1));
  for (int l = 0; ok && l < nl; ++l) ok = layers[l].tok_packed != nullptr;
  if (!ok)
    return sf_set_err(-1, "invalid argument: the token-stationary layers need sf_pack_layer_tok_weights fragments, 1..8 layers and 1 <= L <= 96 rows per video", __FILE__, __LINE__);
  static const int dbg = sf_dbg("lt");
  LtArgs A;
  A.x = xin; A.ring = ring; A.pe = pe; A.y = y;
  for (int l = 0; l < LT_MAXL; ++l) A.blob[l] = (const char*)layers[l < nl ? l : nl - 1].tok_packed;
  A.eps = eps; A.nl = nl; A.B = B; A.L = L; A.vpw = sf_layer_tok_vpw(L); A.RF = ring_frames; A.N = nslots; A.f0 = f0; A.dbg_ts = dbg;
  const int nwg = (B + A.vpw - 1) / A.vpw;
  const double flops = nl * ((double)B * L * (2.0 * LT_D * (3 * LT_D + LT_D + 2 * LT_F)) + (double)B * LT_NH * 4.0 * L * L * 32);
  if (mode == 0) {
    SF_TRY(sf_ensure_dyn_lds((const void*)layer_tok_kernel<0>, LT_LDS));
    sf_prof_begin(SF_K_LAYER_TOK, st, flops);
    hipLaunchKernelGGL(layer_tok_kernel<0>, dim3(nwg), dim3(LT_NT), LT_LDS, st, A);
  } else {
    SF_TRY(sf_ensure_dyn_lds((const void*)layer_tok_kernel<1>, LT_LDS));
    sf_prof_begin(SF_K_LAYER_TOK, st, flops);
    hipLaunchKernelGGL(layer_tok_kernel<1>, dim3(nwg), dim3(LT_NT), LT_LDS, st, A);
  }
  sf_prof_end(SF_K_LAYER_TOK, st);
  SF_CHECK_LAUNCH();
  return 0;
}

// Kernel-level entry point (include/slotformer_hip.h): `nl` whole layers (w[0..nl)) on B sequences of L tokens, for tests against a plain reference
extern "C" int sf_layer_tok_block_f32(const sf_tfm_layer* w, int nl, const float* x, float* y, int B, int L, void* stream) {
  SF_REQUIRE(w && x && y && B > 0 && nl >= 1 && nl <= LT_MAXL, "sf_layer_tok_block_f32: null pointer / empty problem / more than 8 layers");
  SF_REQUIRE(sf_get_precision() == 1, "sf_layer_tok_block_f32: split-bf16 mode only");
  return sf_layer_tok_ex(0, x, nullptr, 1, 1, 0, nullptr, w, nl, 1e-5f, y, B, L, (hipStream_t)stream);
}

// ... for either supported shape: the kernel is picked by (d_model, num_heads, ffn), which must be the shape w[].tok_packed was packed for
extern "C" int sf_layer_tok_block_ex_f32(const sf_tfm_layer* w, int nl, int d_model, int num_heads, int ffn, const float* x, float* y, int B, int L,
                                         void* stream) {
  SF_REQUIRE(w && x && y && B > 0 && nl >= 1 && nl <= LT_MAXL, "sf_layer_tok_block_ex_f32: null pointer / empty problem / more than 8 layers");
  SF_REQUIRE(sf_get_precision() == 1, "sf_layer_tok_block_ex_f32: split-bf16 mode only");
  if (sf_layer_tok128_shape(d_model, num_heads, ffn)) return sf_layer_tok128_ex(x, w, nl, 1e-5f, y, B, L, (hipStream_t)stream);
  SF_REQUIRE(d_model == LT_D && num_heads == LT_NH && ffn == LT_F, "sf_layer_tok_block_ex_f32: (d_model, heads, ffn) = (256, 8, 1024) or (128, 8, 512) only");
  return sf_layer_tok_ex(0, x, nullptr, 1, 1, 0, nullptr, w, nl, 1e-5f, y, B, L, (hipStream_t)stream);
}

// The token-stationary layer of layer_tok.hip for the OBJ3D Transformer: d_model 128, 8 heads of 16, ffn 512 (slotformer_obj3d_params.py).
//     x2 = x + out_proj(MHA(LN1(x))) + b_o ;   y = x2 + lin2(relu(lin1(LN2(x2))))
// Same geometry and the same chain of register-resident products (layer_tok_common.h): a workgroup owns whole videos (sf_layer_tok_vpw(L) of them, up
// to 128 token rows), each of its four waves 32 tokens for the whole launch; D^T[feature][token] = W . A^T with the wave's activations as the MFMA B
// operand, split-bf16 (hi | lo operands, three passes, f32 accumulate), LayerNorm and softmax in f32, `nl` layers per launch.  What the shape changes:
//   * An attention BLOCK (32 rows of q / k / v, one stage of the weight stream each) is a PAIR of heads.  Virtual k-step s of a 32-feature accumulator
//     block (registers 8 s .. 8 s + 7) is the features 16 s .. 16 s + 15 of the block = head s of the pair, so the scores of a head are ONE 32x32x16
//     k-step (three passes) of the pair's q fragment s against the pair's K fragment s; the two heads have their own scores, maxima and sums.
//   * P.V runs the 32-row product O^T[32 dims of the PAIR][queries] = V^T . P^T once per head with that head's probabilities and keeps the head's 16
//     rows (registers 8 s .. 8 s + 7; the other 16 are the other head's values against the wrong probabilities: finite, dropped).  Twice the MFMAs of a
//     16x16x32 form, on ~5 % of the layer's FLOPs at 36 tokens; in exchange the V^T fragments are the v accumulators as they lie (operands swapped, as
//     at d 256), the kept halves ARE the 32-wide B operand of the out-projection slice, and no second MFMA shape with its own layouts enters the chain.
//   * Softmax scale 1 / sqrt(16).
// Weight stream: 48 stages of 16 KiB per layer (16 attention: q0 k0 v0, then q k v of pair i and the out_proj columns of pair i - 1, then the columns of
// pair 3; 32 FFN: lin1 rows / lin2 columns of 16 hidden blocks interleaved), 16 fragments of 1 KiB per stage, four per wave (one global_load_lds piece
// behind each fragment group of the product that runs).  A stage here is HALF the MFMA time of a d 256 stage (24 instead of 48 MFMAs of a row product),
// so the ring is FOUR stages deep, requested three ahead: 72 MFMAs (~2,300 cycles at 32 per MFMA) of cover for a piece's flight, where the three-deep ring
// of 32 KiB stages gives 96 and a three-deep ring of these stages would give 48; 64 KiB of LDS instead of 96.  LDS map: ring 4 x 16 KiB | K fragments of the current pair [head s][plane][token block][64 lanes] x 16 B, 16 KiB |
// V^T fragments [token block][key k-step][plane][64 lanes] x 16 B, 16 KiB | the layer's 1664 f32 vectors: 104,960 bytes, one workgroup per CU -- which
// is what its four waves (one per SIMD, the whole register file each) want anyway.  Neither registers nor LDS bind at this shape.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "layer_fused.h"
#include "layer_tok_common.h"

namespace {
constexpr int LS_NT = 256, LS_D = 128, LS_F = 512, LS_NH = 8, LS_NP = LS_D / 32, LS_MAXL = 8;
constexpr int LS_STAGE = 16 * 1024, LS_RING = 4, LS_AHEAD = LS_RING - 1, LS_PIECES = 4;   // pieces of a stage per wave
constexpr int LS_NST_ATT = 4 * LS_NP, LS_NST = LS_NST_ATT + 2 * (LS_F / 32);   // 16 attention + 32 FFN stages per layer
constexpr int LS_KV = LS_RING * LS_STAGE;
constexpr int LS_VT = LS_KV + 16 * 1024;
constexpr int LS_PAR = LS_KV + 32 * 1024;
constexpr int Q_LN1G = 0, Q_LN1B = 128, Q_BQKV = 256, Q_BO = 640, Q_LN2G = 768, Q_LN2B = 896, Q_B1 = 1024, Q_B2 = 1536, Q_N = 1664;
constexpr size_t LS_LDS = (size_t)LS_PAR + (size_t)Q_N * 4;
constexpr size_t LS_BLOB = (size_t)LS_NST * LS_STAGE + (size_t)Q_N * 4;   // a layer's fragments + its vectors
static_assert(LS_LDS <= 160 * 1024, "LDS budget");
static_assert(LS_STAGE == (LS_D / 8) * 1024 && LS_PIECES * 4 == LS_D / 8 && LS_NST > LS_AHEAD, "stage = D / 8 fragments, four waves");

struct LsArgs {
  const float* x;   // [B * L][128] rows
  float* y;         // [B * L][128]
  const char* blob[LS_MAXL];   // sf_pack_layer_tok_weights copies (128 / 8 / 512) of the layers this launch runs
  float eps;
  int nl, B, L, vpw;
};
}  // namespace

__global__ __launch_bounds__(LS_NT) void layer_tok128_kernel(LsArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* P = (float*)(smem + LS_PAR);
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
  // ---- the token's row in accumulator layout: X[ob][4 g + q] = x[32 ob + 8 g + 4 h + q] ----
  f32x16 X[4];
  {
    const float* xr = A.x + row * LS_D + 4 * h;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 v = *(const f32x4*)(xr + 32 * ob + 8 * g);
#pragma unroll
        for (int q = 0; q < 4; ++q) X[ob][4 * g + q] = v[q];
      }
  }
  // ---- weight ring: the launch's stages (48 per layer, layer after layer) are ONE stream; stage gs lives in slot gs % 4; this wave copies fragments
  //      4 wave .. 4 wave + 3 of every stage, one per fragment group of the product that runs three stages earlier ----
  const unsigned wlane = (unsigned)(wave * LS_PIECES * 1024 + lane * 16);
  char* const wdst = smem + (wave * LS_PIECES) * 1024;
  // prefetch cursor (as in layer_tok.hip): the stage LS_AHEAD ahead of consumer stage cs of the current layer -- of this layer's blob, the first stages
  // of the next layer's behind the end, and past the end of the launch the last stage again (re-requested into a free slot: every stage issues its four
  // pieces, one wait count fits all).  Scalar selects only.
  int cur = 0;           // slot of the next stage to be consumed
  int cs = -LS_AHEAD;    // consumer stage inside the current layer (the prologue requests stages 0 .. LS_AHEAD - 1)
  const char* base_cur = A.blob[0];
  const char* base_nxt = A.blob[0];
  bool last_layer = false;
  auto stage_src = [&]() -> const char* {
    const int t2 = cs + LS_AHEAD;
    const bool wrap = t2 >= LS_NST;
    const char* b = wrap ? base_nxt : base_cur;
    const int so = wrap ? (last_layer ? LS_NST - 1 : t2 - LS_NST) : t2;
    ++cs;
    return b + (size_t)so * LS_STAGE + wlane;
  };
#pragma unroll
  for (int a = 0; a < LS_AHEAD; ++a) {
    const LtRing R0{nullptr, stage_src(), wdst + a * LS_STAGE};
#pragma unroll
    for (int f = 0; f < LS_PIECES; ++f) lt_dma(R0, f);
  }
  // the stage about to be consumed has landed (every wave waits for its own pieces -- those of the LS_AHEAD - 1 stages behind it may still fly -- then
  // the barrier), every wave is done with the previous one (whose slot the pieces of stage gs + LS_AHEAD go to), LDS writes of the previous stage
  // (keys / values) are visible
  auto stage_begin = [&]() -> LtRing {
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    static_assert((LS_AHEAD - 1) * LS_PIECES == 8, "the wait count above");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const int nb = cur == 0 ? LS_RING - 1 : cur - 1;
    LtRing R{smem + cur * LS_STAGE + lane * 16, stage_src(), wdst + nb * LS_STAGE};
    cur = cur == LS_RING - 1 ? 0 : cur + 1;
    return R;
  };
  // ---- key blocks this wave's queries need: the tokens of the videos its 32 rows belong to (at most three 32-key blocks, sf_layer_tok_vpw); a block
  //      index past the last one is clamped for the READS (finite values), its keys fail the range test of the mask ----
  const int wf = min(wave * 32, nvalid - 1);
  const int kb0 = ((wf / L) * L) >> 5;
  const int d0 = 32 * kb0 + 4 * h - vl * L;   // key index of register (kbi, 4 g + q) minus the video's first key: d0 + 32 kbi + 8 g + q
  const char* pb;   // the vectors as this lane reads them: + 4 h floats; opaque, so that every read is this base + an immediate offset
  {
    unsigned pbo = (unsigned)(LS_PAR + 16 * h);
    asm volatile("" : "+v"(pbo));
    pb = smem + pbo;
  }
  char* const kwr = smem + LS_KV + wave * 1024 + lane * 16;          // + (s * 2 + plane) * 4096, s = head of the pair
  char* const vwr = smem + LS_VT + wave * 4096 + lane * 16;          // + (s * 2 + plane) * 1024, s = 16-key k-step of the block
  const char* krd[3];
  const char* vrd[3];
#pragma unroll
  for (int kbi = 0; kbi < 3; ++kbi) {
    const int kb = min(kb0 + kbi, 3);
    krd[kbi] = smem + LS_KV + kb * 1024 + lane * 16;
    vrd[kbi] = smem + LS_VT + kb * 4096 + lane * 16;
  }
  const float qscale = 0.36067376022224085f;   // log2(e) / sqrt(16): the scores in the exponent's base
  constexpr float NEG = -3.0e38f;

#pragma unroll 1
  for (int l = 0; l < A.nl; ++l) {
    cs = 0;
    base_cur = A.blob[l];
    last_layer = l + 1 >= A.nl;
    base_nxt = A.blob[last_layer ? l : l + 1];
    // ---- the layer's vectors -> LDS (behind the first barrier every wave is done with the previous layer's) ----
    __syncthreads();
    {
      const float* vsrc = (const float*)(A.blob[l] + (size_t)LS_NST * LS_STAGE);
      for (int i = t; i < Q_N / 4; i += LS_NT) *(f32x4*)(P + 4 * i) = *(const f32x4*)(vsrc + 4 * i);
    }
    __syncthreads();
    // ================================================= attention block =================================================
    bf16x8 xh[8], xl[8];
    lt_layernorm<Q_LN1G, Q_LN1B>(X, pb, h, A.eps, xh, xl);
    lt_add_vec<Q_BO>(X, pb);   // X = x + b_o: the out-projection slices add into it
    // One pair behind, as layer_tok.hip is one head behind: while pair i's q / k / v products run, scores / softmax / PV of pair i - 1 are their side work.
    //   D_i [Wq_i]:      S^T(i - 1) = K Q^T, both heads;  q(i) product   | mask, maxima of pair i - 1
    //   A_i [Wk_i]:      k(i) product                                     | exponentials, sums, P -> hi | lo fragments;   then O(i - 1) = V^T P per head
    //   B_i [Wv_i]:      v(i) product (operands swapped)                  | k(i) -> K fragments in LDS, q(i) -> fragments, O(i - 1) / sums -> fragments
    //   C_i [Wo_{i-1}]:  X += Wo[:, pair i - 1] O(i - 1)                  | v(i) -> V^T fragments in LDS
    // K / V^T of ONE pair live in LDS: K(i) is written behind barrier B_i (the last reader of K(i - 1) is S^T(i - 1) in D_i), V^T(i) behind barrier C_i
    // (the last reader of V^T(i - 1) is the PV product at the end of A_i).
    f32x16 qa, ka, va, S[2][3], O;
    bf16x8 qh[2], ql[2], ph[2][3][2], pl[2][3][2], oh[2], ol[2];
    float mx0[2], mx1[2], mx[2] = {0.f, 0.f}, sm[2], rinv[2] = {0.f, 0.f};
    auto zero16 = [](f32x16& a) {
#pragma unroll
      for (int r = 0; r < 16; ++r) a[r] = 0.f;
    };
    int hp = 0;   // pair whose q / k / v products run (a runtime value inside the loop)
    // -- pieces of side work (s = head of the pair, c = 8-register chunk of its three score blocks) --
    auto mask_chunk = [&](int s, int c) {   // keys of other videos -> NEG; running maxima
      const int kbi = c >> 1;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int r = 8 * (c & 1) + rr;
        const bool ok = (unsigned)(d0 + 32 * kbi + 8 * (r >> 2) + (r & 3)) < (unsigned)L;
        const float v = ok ? S[s][kbi][r] : NEG;
        S[s][kbi][r] = v;
        if (rr & 1) mx1[s] = fmaxf(mx1[s], v); else mx0[s] = fmaxf(mx0[s], v);
      }
    };
    auto exp_chunk = [&](int s, int c) {
      const int kbi = c >> 1;
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int r = 8 * (c & 1) + rr;
        const float e = __builtin_amdgcn_exp2f(S[s][kbi][r] - mx[s]);
        S[s][kbi][r] = e;
        if (rr & 1) s1 += e; else s0 += e;
      }
      sm[s] += s0 + s1;
    };
    auto psplit_chunk = [&](int s, int c) {
      sf_split8(quad(S[s][c >> 1], 2 * (c & 1)), quad(S[s][c >> 1], 2 * (c & 1) + 1), ph[s][c >> 1][c & 1], pl[s][c >> 1][c & 1]);
    };
    auto kconv = [&](int s) {
      const float* bk = (const float*)pb + Q_BQKV + LS_D + 32 * hp;
      bf16x8 fh, fl;
      sf_split8(quad(ka, 2 * s) + *(const f32x4*)(bk + 16 * s), quad(ka, 2 * s + 1) + *(const f32x4*)(bk + 16 * s + 8), fh, fl);
      *(bf16x8*)(kwr + (s * 2) * 4096) = fh;
      *(bf16x8*)(kwr + (s * 2 + 1) * 4096) = fl;
    };
    auto qconv = [&](int s) {
      const float* bq = (const float*)pb + Q_BQKV + 32 * hp;
      sf_split8((quad(qa, 2 * s) + *(const f32x4*)(bq + 16 * s)) * qscale, (quad(qa, 2 * s + 1) + *(const f32x4*)(bq + 16 * s + 8)) * qscale, qh[s], ql[s]);
    };
    auto vconv = [&](int s) {   // lane = dim of the pair, registers 8 s .. 8 s + 7 = keys of the block's k-step s
      const float bv = P[Q_BQKV + 2 * LS_D + 32 * hp + n];
      bf16x8 fh, fl;
      sf_split8(quad(va, 2 * s) + bv, quad(va, 2 * s + 1) + bv, fh, fl);
      *(bf16x8*)(vwr + (s * 2) * 1024) = fh;
      *(bf16x8*)(vwr + (s * 2 + 1) * 1024) = fl;
    };
    // registers 8 s .. 8 s + 7 of O = dims of head s, from the product with head s's probabilities
    auto oconv = [&](int s) { sf_split8(quad(O, 2 * s) * rinv[s], quad(O, 2 * s + 1) * rinv[s], oh[s], ol[s]); };
    // scores of the previous pair: S^T[key][query] = K Q^T per head (ONE k-step: fragment s of K and of q) for the wave's three key blocks
    auto scores = [&]() {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 kh[3], kl[3];
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) {
          kh[kbi] = *(const bf16x8*)(krd[kbi] + (s * 2) * 4096);
          kl[kbi] = *(const bf16x8*)(krd[kbi] + (s * 2 + 1) * 4096);
        }
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) zero16(S[s][kbi]);
        // (the three blocks' accumulators in turn: no two consecutive MFMAs on one accumulator)
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { S[s][kbi] = LT_MFMA(kh[kbi], ql[s], S[s][kbi]); LT_PIN(); }
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { S[s][kbi] = LT_MFMA(kl[kbi], qh[s], S[s][kbi]); LT_PIN(); }
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) { S[s][kbi] = LT_MFMA(kh[kbi], qh[s], S[s][kbi]); LT_PIN(); }
        mx0[s] = mx1[s] = NEG;
        sm[s] = 0.f;
      }
    };
    // O^T[32 dims of the pair][queries] = V^T P^T with head s's probabilities; rows 16 s .. 16 s + 15 (registers 8 s .. 8 s + 7) are head s's output
    auto pv = [&]() {
      bf16x8 vh[3][2], vlo[3][2];
#pragma unroll
      for (int kbi = 0; kbi < 3; ++kbi)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          vh[kbi][ks] = *(const bf16x8*)(vrd[kbi] + (ks * 2) * 1024);
          vlo[kbi][ks] = *(const bf16x8*)(vrd[kbi] + (ks * 2 + 1) * 1024);
        }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f32x16 Op[3];
#pragma unroll
        for (int kbi = 0; kbi < 3; ++kbi) zero16(Op[kbi]);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
          for (int kbi = 0; kbi < 3; ++kbi) { Op[kbi] = LT_MFMA(vh[kbi][ks], pl[s][kbi][ks], Op[kbi]); LT_PIN(); }
#pragma unroll
          for (int kbi = 0; kbi < 3; ++kbi) { Op[kbi] = LT_MFMA(vlo[kbi][ks], ph[s][kbi][ks], Op[kbi]); LT_PIN(); }
#pragma unroll
          for (int kbi = 0; kbi < 3; ++kbi) { Op[kbi] = LT_MFMA(vh[kbi][ks], ph[s][kbi][ks], Op[kbi]); LT_PIN(); }
        }
#pragma unroll
        for (int r = 8 * s; r < 8 * s + 8; ++r) O[r] = (Op[0][r] + Op[1][r]) + Op[2][r];
      }
    };
    // four fragment groups per product: head g >> 1, first / second half of its side work
    auto sideD = [&](int g) {
      const int s = g >> 1;
      if ((g & 1) == 0) {
        mask_chunk(s, 0); mask_chunk(s, 1); mask_chunk(s, 2);
      } else {
        mask_chunk(s, 3); mask_chunk(s, 4); mask_chunk(s, 5);
        mx[s] = lt_xmax(fmaxf(mx0[s], mx1[s]), h);
      }
    };
    auto sideA = [&](int g) {
      const int s = g >> 1;
      if ((g & 1) == 0) {
#pragma unroll
        for (int c = 0; c < 6; ++c) exp_chunk(s, c);
        rinv[s] = 1.0f / lt_xsum(sm[s], h);
      } else {
#pragma unroll
        for (int c = 0; c < 6; ++c) psplit_chunk(s, c);
      }
    };
    // ---- pair 0: nothing behind it yet ----
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
        if (g == 0) { kconv(0); kconv(1); }
        else if (g == 1) { qconv(0); qconv(1); }
      });
      vconv(0);
      vconv(1);
    }
#pragma unroll 1
    for (hp = 1; hp < LS_NP; ++hp) {
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
          if (g == 0) { kconv(0); kconv(1); }
          else if (g == 1) { qconv(0); qconv(1); }
          else oconv(g - 2);
        });
      }
      {
        const LtRing R = stage_begin();   // C_i
        lt_kslice_product<5>(R, oh, ol, X, [&](int g) {
          if (g < 2) vconv(g);
        });
      }
    }
    // ---- the last pair's scores, softmax and PV have no product left to hide under ----
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();   // V^T(3) of every wave is in LDS
    asm volatile("" ::: "memory");
    scores();
#pragma unroll
    for (int g = 0; g < 4; ++g) sideD(g);
#pragma unroll
    for (int g = 0; g < 4; ++g) sideA(g);
    pv();
    oconv(0);
    oconv(1);
    {
      const LtRing R = stage_begin();   // C_4
      lt_kslice_product<0>(R, oh, ol, X, LtNoSide{});
    }
    // ==================================================== FFN block ====================================================
    // X = x2; LN2 -> fragments; X += b2 becomes the accumulator of the second product.  Stage order W1_0, (W1_j, W2_{j-1}) for j = 1..15, W2_15: block
    // j - 1's bias / ReLU / hi | lo split is the side work of block j's first product.
    lt_layernorm<Q_LN2G, Q_LN2B>(X, pb, h, A.eps, xh, xl);
    lt_add_vec<Q_B2>(X, pb);
    f32x16 Ha, Hb;
    bf16x8 hh[2], hl[2];
    f32x4 b1q[4];   // lin1 bias of the block being converted, requested a stage ahead
    auto b1_load = [&](int blk) {
      const float* b1 = (const float*)pb + Q_B1 + 32 * blk;
#pragma unroll
      for (int g = 0; g < 4; ++g) b1q[g] = *(const f32x4*)(b1 + 8 * g);
    };
    auto hconv = [&](const f32x16& Hx, int s) {
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      const f32x4 u0 = __builtin_elementwise_max(quad(Hx, 2 * s) + b1q[2 * s], z4);
      const f32x4 u1 = __builtin_elementwise_max(quad(Hx, 2 * s + 1) + b1q[2 * s + 1], z4);
      sf_split8(u0, u1, hh[s], hl[s]);
    };
    // one step = [W1_j: first product of block j into Hn | bias / ReLU / split of block j - 1 (Hp)] + [W2_{j-1}: second product of block j - 1]
    auto ffn_step = [&](f32x16& Hn, const f32x16& Hp, int j) {
      {
        const LtRing R = stage_begin();
        lt_row_product<false, 4>(R, xh, xl, Hn, [&](int g) {
          if (g >= 1 && g < 3) hconv(Hp, g - 1);
        });
        asm volatile("" : "+v"(hh[0]), "+v"(hh[1]), "+v"(hl[0]), "+v"(hl[1]));   // (the conversion belongs to THIS stage's MFMA stream)
      }
      {
        const LtRing R = stage_begin();
        b1_load(j);
        lt_kslice_product<0>(R, hh, hl, X, LtNoSide{});
      }
    };
    {
      const LtRing R = stage_begin();
      b1_load(0);
      lt_row_product<false, 0>(R, xh, xl, Ha, LtNoSide{});
    }
    ffn_step(Hb, Ha, 1);
#pragma unroll 1
    for (int j = 2; j < LS_F / 32; j += 2) {   // (two steps per trip: the accumulators trade places without a copy)
      ffn_step(Ha, Hb, j);
      ffn_step(Hb, Ha, j + 1);
    }
    hconv(Hb, 0);
    hconv(Hb, 1);
    {
      const LtRing R = stage_begin();
      lt_kslice_product<0>(R, hh, hl, X, LtNoSide{});
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-requested last stage: no LDS write may be pending when the workgroup leaves
  // ---- finished rows ----
  if (tl < nvalid) {
    float* yr = A.y + row * LS_D + 4 * h;
#pragma unroll
    for (int ob = 0; ob < 4; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g) *(f32x4*)(yr + 32 * ob + 8 * g) = quad(X[ob], g);
  }
}

bool sf_layer_tok128_shape(int d_model, int num_heads, int ffn) { return d_model == LS_D && num_heads == LS_NH && ffn == LS_F; }
size_t sf_layer_tok128_packed_bytes() { return LS_BLOB; }

// sf_pack_layer_tok_weights for (128, 8, 512): the four matrices as fragments in this kernel's consumption order + the eight vectors
int sf_pack_layer_tok128(const sf_tfm_layer* w, void* packed, hipStream_t st) {
  const int total = LS_NST * (LS_D / 8) * 64;
  hipLaunchKernelGGL((pack_layer_tok_kernel<LS_D, LS_F>), dim3((total + 255) / 256), dim3(256), 0, st, w->in_proj_w, w->out_proj_w, w->lin1_w, w->lin2_w,
                     (uint4*)packed);
  SF_CHECK_LAUNCH();
  float* vec = (float*)((char*)packed + (size_t)LS_NST * LS_STAGE);
  const struct {
    const float* src;
    int off, n;
  } parts[8] = {{w->norm1_g, Q_LN1G, LS_D}, {w->norm1_b, Q_LN1B, LS_D}, {w->in_proj_b, Q_BQKV, 3 * LS_D}, {w->out_proj_b, Q_BO, LS_D},
                {w->norm2_g, Q_LN2G, LS_D}, {w->norm2_b, Q_LN2B, LS_D}, {w->lin1_b, Q_B1, LS_F},          {w->lin2_b, Q_B2, LS_D}};
  for (const auto& p : parts) {
    const hipError_t e = hipMemcpyAsync(vec + p.off, p.src, (size_t)p.n * 4, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  }
  return 0;
}

// `nl` consecutive layers in ONE launch: xin [B * L][128] rows -> y [B * L][128] finished rows of the last of them.  The window rules are those of the
// 4 waves x 32 tokens geometry (sf_layer_tok_vpw).
int sf_layer_tok128_ex(const float* xin, const sf_tfm_layer* layers, int nl, float eps, float* y, int B, int L, hipStream_t st) {
  bool ok = layers && nl >= 1 && nl <= LS_MAXL && sf_layer_tok_ok(L) && B >= 1 && y && xin;
  for (int l = 0; ok && l < nl; ++l) ok = layers[l].tok_packed != nullptr;
  if (!ok)
    return sf_set_err(-1, "invalid argument: the token-stationary layers need sf_pack_layer_tok_weights fragments, 1..8 layers and 1 <= L <= 96 rows per video", __FILE__, __LINE__);
  LsArgs A;
  A.x = xin; A.y = y;
  for (int l = 0; l < LS_MAXL; ++l) A.blob[l] = (const char*)layers[l < nl ? l : nl - 1].tok_packed;
  A.eps = eps; A.nl = nl; A.B = B; A.L = L; A.vpw = sf_layer_tok_vpw(L);
  const int nwg = (B + A.vpw - 1) / A.vpw;
  const double flops = nl * ((double)B * L * (2.0 * LS_D * (3 * LS_D + LS_D + 2 * LS_F)) + (double)B * LS_NH * 4.0 * L * L * 16);
  SF_TRY(sf_ensure_dyn_lds((const void*)layer_tok128_kernel, LS_LDS));
  sf_prof_begin(SF_K_LAYER_TOK, st, flops);
  hipLaunchKernelGGL(layer_tok128_kernel, dim3(nwg), dim3(LS_NT), LS_LDS, st, A);
  sf_prof_end(SF_K_LAYER_TOK, st);
  SF_CHECK_LAUNCH();
  return 0;
}

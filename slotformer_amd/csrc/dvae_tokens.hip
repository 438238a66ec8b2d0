// dVAE token ids on the device: the two ends of the encoder (base_slots/models/dVAE.py:24-35, 52-77) as kernels of their own, so that a video is
// tokenised without a patchify copy in front and without the vocabulary logits behind.
//
//   dvae_patch_embed_kernel   the first block's bias-free 4x4 / stride-4 convolution, frames [F,3,H,W] f32 (NCHW) -> [F,h,w,64] (NHWC, pre-norm):
//                             D[pixel][cout] = sum_k X[pixel][k] W[cout][k], k = c * 16 + ky * 4 + kx, K = 48 = three k-steps of 32x32x16 bf16 MFMA
//                             (k-step = input channel).  A lane's operand of a step is rows 2 h and 2 h + 1 of its token's 4x4 patch: two 16-byte
//                             loads straight from the frame.  The weight [64][48] is split on the fly (12 KiB: it stays in the caches).  The lane
//                             holds an output CHANNEL, so a store instruction writes two pixels' runs of 128 contiguous bytes.
//   dvae_head_argmax_kernel   ids[r] = argmax_v (W[v] . x[r] + b[v]) for x [R,64]: D[v][pixel] on the MFMA's (row, column) axes, so the sixteen
//                             accumulators of a lane all belong to ONE pixel and the running (max, index) pair never leaves the lane while the
//                             vocabulary is swept in blocks of 32.  A workgroup owns 64 pixels; its four waves each keep the pixels' hi | lo
//                             fragments in registers (four k-steps x two pixel blocks) and sweep every fourth block of the head weight, streamed
//                             in fragment order (sf_dvae_pack_head_weights: 16-byte loads, 1 MiB at V = 4096, L2-resident) one block ahead of its
//                             use; the bias is the accumulators' initial value.  Per block of 32 words and 32 pixels: twelve MFMAs, then compare /
//                             select.  The two half-waves (words 4 h + ...) meet in one exchange, the four waves in 2 KB of LDS behind the only
//                             barrier.  No communication between workgroups: a pixel's id does not depend on its place in the batch.
//
// Arithmetic: split-bf16 -- every f32 operand is bf16 hi + bf16 lo, three products a_hi.b_lo + a_lo.b_hi + a_hi.b_hi with f32 accumulation -- WHATEVER
// sf_set_precision says: token targets have one definition.  Every sum has a fixed order and there is no atomic.
// Ties: the FIRST index of the maximum (sf_argmax_rows_f32); a row holding a NaN is unspecified.
#include "../../include/slotformer_hip.h"
#include "sf_common.h"
#include "bf16_planes.h"

namespace {

constexpr int DT_K = 64;        // features of the head (and output channels of the patch embedding)
constexpr int DT_KP = 48;       // 3 channels x 4 x 4: contraction length of the patch embedding
constexpr int DT_PIX = 64;      // pixels of a wave's tile: two 32-column (head) / 32-row (patch embedding) MFMA blocks
constexpr int DT_VB = 32;       // vocabulary words of an MFMA block
constexpr int DT_WAVES = 4;     // waves of a head workgroup: they share the 64 pixels and split the vocabulary
constexpr int DT_MAX_V = 1 << 20;

// f32 -> bf16, round to nearest even, the same on host and device (a NaN stays a NaN)
__host__ __device__ inline unsigned short dt_bf16(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float dt_f32(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }

// Fragment order of the head weight [V][64]: for every block vb of 32 words and every k-step ks (16 features) the 64 lanes' A operands of
// mfma_f32_32x32x16_bf16 lie one after the other, lane (r = l & 31, h = l >> 5) holding W[32 vb + r][16 ks + 8 h + 0..7].
// element index of a packed plane -> element index of the [V][64] source
__host__ __device__ inline long long dt_pack_src(long long idx) {
  const int j = (int)(idx & 7);
  const int l = (int)((idx >> 3) & 63);
  const long long step = idx >> 9;   // vb * 4 + ks
  const long long vb = step >> 2;
  const int ks = (int)(step & 3);
  return (vb * DT_VB + (l & 31)) * DT_K + 16 * ks + 8 * (l >> 5) + j;
}

__global__ void dt_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ hi, unsigned short* __restrict__ lo, long long n) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float v = w[dt_pack_src(idx)];
  const unsigned short h = dt_bf16(v);
  hi[idx] = h;
  lo[idx] = dt_bf16(v - dt_f32(h));
}

__device__ __forceinline__ PlFrag dt_split(const float4 a, const float4 b) {
  PlFrag f;
  sf_split8(f32x4{a.x, a.y, a.z, a.w}, f32x4{b.x, b.y, b.z, b.w}, f.h, f.l);
  return f;
}

// frames [F,3,H,W] -> y [P = F h w][64].  One wave = 64 pixels x 64 channels, any number of waves per workgroup (no barrier).
__global__ __launch_bounds__(256) void dvae_patch_embed_kernel(const float* __restrict__ img, const float* __restrict__ w, float* __restrict__ y,
                                                               long long P, int H, int W) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  const long long pt = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * DT_PIX;
  if (pt >= P) return;   // wave-uniform
  const int hw_w = W >> 2, hw = (H >> 2) * hw_w;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  f32x16 acc[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[s][t][i] = 0.f;
  long long src[2];   // element offset of row 2 h of the token's patch in channel 0; -1: a pixel past the end (a zero operand, never an address)
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long long p = pt + 32 * s + r;
    src[s] = -1;
    if (p < P) {
      const long long f = p / hw;
      const int rem = (int)(p - f * hw);
      const int py = rem / hw_w, px = rem - py * hw_w;
      src[s] = ((f * 3) * H + 4 * py + 2 * h) * W + 4 * px;
    }
  }
  const long long plane = (long long)H * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    PlFrag xf[2], wf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float4 a = zero, b = zero;
      if (src[s] >= 0) {
        const float* q = img + src[s] + c * plane;
        a = *reinterpret_cast<const float4*>(q);
        b = *reinterpret_cast<const float4*>(q + W);
      }
      xf[s] = dt_split(a, b);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float* q = w + (32 * t + r) * DT_KP + 16 * c + 8 * h;
      wf[t] = dt_split(*reinterpret_cast<const float4*>(q), *reinterpret_cast<const float4*>(q + 4));
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t) pl_mma(acc[s][t], xf[s], wf[t]);
  }
  // D block (s, t): the lane holds channel 32 t + r and, in register i, pixel 32 s + MM_ROW(i, lane)
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long p = pt + 32 * s + MM_ROW(i, lane);
      if (p < P) {
        y[p * DT_K + r] = acc[s][0][i];
        y[p * DT_K + 32 + r] = acc[s][1][i];
      }
    }
}

// (value, -index) order: is (v, i) ahead of (best, bi)?
__device__ __forceinline__ bool dt_ahead(float v, int i, float best, int bi) { return v > best || (v == best && i < bi); }

// x [R][ld] -> ids.  One workgroup = 64 rows; wave q of its four sweeps the blocks q, q + 4, ... of 32 words, so a row's sweep over V is four
// short chains side by side and a call of few rows still has waves on every SIMD.  w_hi / w_lo: the packed planes in 16-byte units.
// The three places where candidates meet, each in (value, -index) order so that the FIRST index of the maximum survives:
//   inside a lane    registers 0..15 of a block are words 8 g + 4 h + e in rising order and the blocks rise too, so a lane meets its indices in
//                    rising order and a strict `>` keeps the first of equals;
//   the half-waves   lanes l and l ^ 32 hold the same pixel and interleaved words (4 h + ...): dt_ahead, one exchange;
//   the four waves   through 2 KB of LDS, wave 0 .. 3 in order: dt_ahead.
template <bool BIAS>
__global__ __launch_bounds__(256) void dvae_head_argmax_kernel(const float* __restrict__ x, long long ld, const uint4* __restrict__ w_hi,
                                                               const uint4* __restrict__ w_lo, const float* __restrict__ bias,
                                                               long long* __restrict__ ids64, short* __restrict__ ids16, long long R, int V) {
  __shared__ float sv[DT_WAVES][DT_PIX];
  __shared__ int si[DT_WAVES][DT_PIX];
  const int lane = threadIdx.x & 63;
  const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (a scalar: the sweep's branches are wave-uniform)
  const int r = lane & 31, h = lane >> 5;
  const long long pt = (long long)blockIdx.x * DT_PIX;   // < R: the grid is ceil(R / 64)
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  PlFrag xf[2][4];   // B operands: lane (r, h) holds features 16 ks + 8 h + 0..7 of pixel 32 s + r
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long long p = pt + 32 * s + r;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      float4 a = zero, b = zero;
      if (p < R) {   // a row past the end is a zero operand, never an address
        const float* xp = x + p * ld + 16 * ks + 8 * h;
        a = *reinterpret_cast<const float4*>(xp);
        b = *reinterpret_cast<const float4*>(xp + 4);
      }
      xf[s][ks] = dt_split(a, b);
    }
  }
  float best[2] = {-INFINITY, -INFINITY};
  int bidx[2] = {0x7fffffff, 0x7fffffff};
  const int nvb = V / DT_VB;
  if (q < nvb) {   // wave-uniform (V = 64: two blocks, waves 2 and 3 bring nothing)
    // two register sets in turn: the fragments and the bias of a wave's next block are requested before the products of the current one
    PlFrag wa[4], wb[4];
    float4 ba[4], bb[4];
    auto fetch = [&](PlFrag* w, float4* bv, int vb) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        w[ks].h = __builtin_bit_cast(bf16x8, w_hi[((long long)vb * 4 + ks) * 64 + lane]);
        w[ks].l = __builtin_bit_cast(bf16x8, w_lo[((long long)vb * 4 + ks) * 64 + lane]);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) bv[g] = BIAS ? *reinterpret_cast<const float4*>(bias + vb * DT_VB + 8 * g + 4 * h) : zero;
    };
    auto sweep = [&](const PlFrag* w, const float4* bv, int vb) {
      // register 4 g + e of the lane: word 32 vb + 8 g + 4 h + e; its bias is the accumulator's initial value
      f32x16 acc[2];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc[s][4 * g] = bv[g].x, acc[s][4 * g + 1] = bv[g].y, acc[s][4 * g + 2] = bv[g].z, acc[s][4 * g + 3] = bv[g].w;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int s = 0; s < 2; ++s) pl_mma(acc[s], w[ks], xf[s][ks]);   // w_hi.x_lo + w_lo.x_hi + w_hi.x_hi
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (acc[s][i] > best[s]) best[s] = acc[s][i], bidx[s] = vb * DT_VB + MM_ROW(i, lane);
    };
    // the wave's last block: a request past it asks for it again, never past the end, and sweeping it a second time changes nothing (equal values
    // are not `>`).  Both halves of the loop body run unconditionally: a request whose only use sits behind a branch is moved behind that branch.
    const int last = q + (nvb - 1 - q) / DT_WAVES * DT_WAVES;
    fetch(wa, ba, q);
    for (int vb = q; vb <= last; vb += 2 * DT_WAVES) {
      const int v1 = vb + DT_WAVES <= last ? vb + DT_WAVES : last, v2 = vb + 2 * DT_WAVES <= last ? vb + 2 * DT_WAVES : last;
      // (the scheduling barriers keep the requests AHEAD of the products: left alone, the scheduler sinks them to their uses to shorten the live ranges)
      fetch(wb, bb, v1);
      __builtin_amdgcn_sched_barrier(0);
      sweep(wa, ba, vb);
      __builtin_amdgcn_sched_barrier(0);
      fetch(wa, ba, v2);
      __builtin_amdgcn_sched_barrier(0);
      sweep(wb, bb, v1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float ov = __shfl_xor(best[s], 32, 64);   // the other half-wave's pair of the same pixel
    const int oi = __shfl_xor(bidx[s], 32, 64);
    if (dt_ahead(ov, oi, best[s], bidx[s])) best[s] = ov, bidx[s] = oi;
    if (h == 0) sv[q][32 * s + r] = best[s], si[q][32 * s + r] = bidx[s];
  }
  __syncthreads();   // the only barrier; every thread of the workgroup reaches it
  if (q != 0) return;
  float bv = sv[0][lane];
  int bi = si[0][lane];
#pragma unroll
  for (int w = 1; w < DT_WAVES; ++w)
    if (dt_ahead(sv[w][lane], si[w][lane], bv, bi)) bv = sv[w][lane], bi = si[w][lane];
  const long long p = pt + lane;
  if (p < R) {
    const int id = bi < V ? bi : 0;   // (a row of NaNs never moved the pair: still a valid id)
    if (ids64) ids64[p] = id;
    if (ids16) ids16[p] = (short)id;
  }
}

inline bool dt_head_ok(int V, int K) { return K == DT_K && V >= DT_VB && V % DT_VB == 0 && V <= DT_MAX_V; }
inline unsigned dt_threads(long long waves) { return waves >= 1024 ? 256u : 64u; }   // few rows: one wave per workgroup, so that they spread over the CUs

}  // namespace

extern "C" {

int sf_dvae_tokens_ok(int V, int K, int C, int H, int W) {
  return dt_head_ok(V, K) && C == 3 && H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0;
}

size_t sf_dvae_head_packed_bytes(int V, int K) { return dt_head_ok(V, K) ? (size_t)V * K * 4 : 0; }

int sf_dvae_pack_head_weights(const float* w, void* packed, int V, int K, void* stream) {
  SF_REQUIRE(w && packed, "sf_dvae_pack_head_weights: null pointer");
  SF_REQUIRE(dt_head_ok(V, K), "sf_dvae_pack_head_weights: K must be 64 and V a multiple of 32 in [32, 2^20]");
  const long long n = (long long)V * K;
  unsigned short* hi = static_cast<unsigned short*>(packed);
  hipLaunchKernelGGL(dt_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, hi, hi + n, n);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_dvae_pack_head_weights_host(const float* w, void* packed, int V, int K) {
  SF_REQUIRE(w && packed, "sf_dvae_pack_head_weights_host: null pointer");
  SF_REQUIRE(dt_head_ok(V, K), "sf_dvae_pack_head_weights_host: K must be 64 and V a multiple of 32 in [32, 2^20]");
  const long long n = (long long)V * K;
  unsigned short* hi = static_cast<unsigned short*>(packed);
  unsigned short* lo = hi + n;
  for (long long idx = 0; idx < n; ++idx) {
    const float v = w[dt_pack_src(idx)];
    hi[idx] = dt_bf16(v);
    lo[idx] = dt_bf16(v - dt_f32(hi[idx]));
  }
  return 0;
}

int sf_dvae_patch_embed_f32(const float* img, const float* w, float* y, int F, int C, int H, int W, void* stream) {
  SF_REQUIRE(img && w && y, "sf_dvae_patch_embed_f32: null pointer");
  SF_REQUIRE(C == 3 && H >= 4 && W >= 4 && H % 4 == 0 && W % 4 == 0, "sf_dvae_patch_embed_f32: 3 channels, H and W multiples of 4");
  SF_REQUIRE(F >= 0 && (long long)F * 3 * H * W < (1ll << 40), "sf_dvae_patch_embed_f32: bad frame count");
  SF_REQUIRE(((uintptr_t)img & 15) == 0 && ((uintptr_t)w & 15) == 0, "sf_dvae_patch_embed_f32: img and w must be 16-byte aligned");
  if (F == 0) return 0;
  const long long P = (long long)F * (H / 4) * (W / 4);
  const long long waves = (P + DT_PIX - 1) / DT_PIX;
  const unsigned threads = dt_threads(waves);
  hipLaunchKernelGGL(dvae_patch_embed_kernel, dim3((unsigned)((waves * 64 + threads - 1) / threads)), dim3(threads), 0, (hipStream_t)stream, img, w, y,
                     P, H, W);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_dvae_head_argmax_f32(const float* x, long long ld, const void* w_packed, const float* bias, long long* ids_i64, short* ids_i16, long long R,
                            int V, int K, void* stream) {
  SF_REQUIRE(x && w_packed, "sf_dvae_head_argmax_f32: null pointer");
  SF_REQUIRE(ids_i64 || ids_i16, "sf_dvae_head_argmax_f32: null pointer (both outputs)");
  SF_REQUIRE(dt_head_ok(V, K), "sf_dvae_head_argmax_f32: K must be 64 and V a multiple of 32 in [32, 2^20]");
  SF_REQUIRE(!ids_i16 || V <= 32768, "sf_dvae_head_argmax_f32: int16 ids need V <= 32768");
  SF_REQUIRE(ld >= K && ld % 4 == 0, "sf_dvae_head_argmax_f32: the row stride must be at least K and a multiple of 4");
  SF_REQUIRE(R >= 0 && R < (1ll << 37), "sf_dvae_head_argmax_f32: bad row count");
  SF_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)w_packed & 15) == 0 && (!bias || ((uintptr_t)bias & 15) == 0),
             "sf_dvae_head_argmax_f32: x, w_packed and bias must be 16-byte aligned");
  if (R == 0) return 0;
  const unsigned tiles = (unsigned)((R + DT_PIX - 1) / DT_PIX);
  const uint4* wp = static_cast<const uint4*>(w_packed);
  const uint4* wl = wp + (long long)V * K / 8;
  if (bias)
    hipLaunchKernelGGL(dvae_head_argmax_kernel<true>, dim3(tiles), dim3(64 * DT_WAVES), 0, (hipStream_t)stream, x, ld, wp, wl, bias, ids_i64, ids_i16, R, V);
  else
    hipLaunchKernelGGL(dvae_head_argmax_kernel<false>, dim3(tiles), dim3(64 * DT_WAVES), 0, (hipStream_t)stream, x, ld, wp, wl, bias, ids_i64, ids_i16, R, V);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

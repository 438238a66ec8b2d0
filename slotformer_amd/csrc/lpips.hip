// LPIPS (VGG16) on the device: the `percept_dist` of the video-prediction evaluation (test_vp.py:21-23, vp_utils.py:109-111) as HIP kernels.
//
//   lp_conv_first_kernel  3 -> 64, plain FMA: the input scaling (x - shift) / scale is applied while loading and the zero padding after it, so the
//                         shift is NOT folded into the bias; bias + ReLU; output written as bf16 hi | lo planes
//   lp_conv3x3_kernel     the other twelve layers (64->64 ... 512->512), one kernel: an implicit GEMM  D[cout][pixel] = sum_k W[cout][k] X[k][pixel]
//                         over k = (tap, cin) on 32x32x16 bf16 MFMA.  Pixels are the flattened (image, y, x) index, so a tile spans frames and the
//                         16 x 16 and 8 x 8 maps of the late stages fill their tiles.  Operand fragments are 16-byte loads straight from global
//                         memory: the weights in fragment order (sf_lpips_pack_conv_weights), the activations channels-last in blocks of eight
//                         channels, [C / 8][pixel][8] (a lane's fragment is one pixel's block; the 32 pixels of a half-wave are mostly neighbours,
//                         so a load is two runs of up to 512 contiguous bytes); a neighbour outside the image, or a pixel past the end of the
//                         batch, is a zero fragment and never an address.  No LDS, no barrier, no communication between waves.  bias + ReLU, then
//                         the result is split ONCE into hi | lo planes, which the next layer loads as MFMA operands without conversion.
//   lp_pool2x2_kernel     nn.MaxPool2d(2, 2) on the planes (floor for odd sizes): the (hi, lo) pair of the largest hi + lo
//   lp_tap_kernel         at the five taps: per pixel n = f / (sqrt(sum_c f^2) + 1e-10) for both images, sum_c w_c (n_x - n_y)^2, summed over the
//                         256 pixels of a workgroup in double -> one partial per (pair, workgroup)
//   lp_finish_kernel      one wave per pair: the partials of every tap in a fixed order, / pixels, summed over the taps -> out[pair]
//   lp_mean_kernel        out [B,T] float -> per-video doubles and their mean over the videos, summed in the order of b
//
// Arithmetic: split-bf16 -- every f32 operand is bf16 hi + bf16 lo, three products x_lo.w_hi + x_hi.w_lo + x_hi.w_hi with f32 accumulation --
// WHATEVER sf_set_precision says: the metric has one definition.  Every sum has a fixed order and there is no floating-point atomic: a pair's
// score does not depend on its place in the batch, on the chunk size or on the other pairs, and equal inputs give exactly 0.
#include <math.h>

#include "../../include/slotformer_hip.h"
#include "sf_common.h"
#include "sf_arena.h"
#include "bf16_planes.h"

namespace {

constexpr int LP_STAGES = 5;
constexpr int LP_LAYERS = 13;
constexpr int LP_MIN_HW = 16;      // five stages: 16 -> 8 -> 4 -> 2 -> 1
constexpr int LP_WAVES = 4;        // waves of a convolution workgroup, each with its own pixel tile
constexpr int LP_PIX = 64;         // pixels of a wave's tile (two 32-column MFMA blocks)
constexpr int LP_CO = 64;          // output channels of a wave's tile (two 32-row MFMA blocks): one workgroup = 256 pixels x 64 channels
constexpr int LP_TAP_PIX = 256;    // pixels of a tap workgroup: one per lane
constexpr int LP_C1 = 64;          // channels of the first layer
constexpr int LP_K1 = 27;          // 3 input channels x 9 taps

const int lp_stage_ch[LP_STAGES] = {64, 128, 256, 512, 512};
const int lp_stage_convs[LP_STAGES] = {2, 2, 3, 3, 3};

static_assert(LP_PIX == 64 && LP_CO == 64, "a wave's tile is 2 x 2 MFMA blocks of 32 x 32");
static_assert((LP_K1 * LP_C1 + LP_C1 + 8) * sizeof(float) <= 16 * 1024, "LDS of the first layer");
static_assert(LP_TAP_PIX == 256, "a tap workgroup is four waves, one pixel per lane");

// f32 -> bf16, round to nearest even, the same on host and device (a NaN stays a NaN)
__host__ __device__ inline unsigned short lp_bf16(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float lp_f32(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }

// Fragment order of a 3x3 weight [Cout][Cin][3][3]: for every block of 32 output channels and every k-step (tap, 16 input channels) the 64 lanes'
// A operands of mfma_f32_32x32x16_bf16 lie one after the other, lane (r = l & 31, h = l >> 5) holding W[32 ct + r][tap][16 cc + 8 h + 0..7].
// element index of the packed plane -> element index of the OIHW source
__host__ __device__ inline long long lp_pack_src(long long idx, int Cin) {
  const int j = (int)(idx & 7);
  const int l = (int)((idx >> 3) & 63);
  const long long step = idx >> 9;          // ct * KS + ks
  const int KC = Cin >> 4, KS = 9 * KC;
  const int ct = (int)(step / KS), ks = (int)(step - (long long)ct * KS);
  const int tap = ks / KC, cc = ks - tap * KC;
  const int co = ct * 32 + (l & 31), ci = cc * 16 + 8 * (l >> 5) + j;
  return ((long long)co * Cin + ci) * 9 + tap;
}

__global__ void lp_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ hi, unsigned short* __restrict__ lo, long long n, int Cin) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const float v = w[lp_pack_src(idx, Cin)];
  const unsigned short h = lp_bf16(v);
  hi[idx] = h;
  lo[idx] = lp_bf16(v - lp_f32(h));
}
// first layer: f32 [27][64], k = ci * 9 + tap
__global__ void lp_pack_first_kernel(const float* __restrict__ w, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= LP_K1 * LP_C1) return;
  const int k = idx / LP_C1, co = idx - k * LP_C1;
  out[idx] = w[co * LP_K1 + k];
}

__device__ __forceinline__ float lp_lo16(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float lp_hi16(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
// eight channels of a pixel from the two planes -> f32 (hi + lo is exact in f32)
__device__ __forceinline__ void lp_unpack8(const uint4 h, const uint4 l, float* f) {
  f[0] = lp_lo16(h.x) + lp_lo16(l.x), f[1] = lp_hi16(h.x) + lp_hi16(l.x);
  f[2] = lp_lo16(h.y) + lp_lo16(l.y), f[3] = lp_hi16(h.y) + lp_hi16(l.y);
  f[4] = lp_lo16(h.z) + lp_lo16(l.z), f[5] = lp_hi16(h.z) + lp_hi16(l.z);
  f[6] = lp_lo16(h.w) + lp_lo16(l.w), f[7] = lp_hi16(h.w) + lp_hi16(l.w);
}

// x, y [c,3,H,W] f32 (NCHW) -> planes of 2c images x 64 channels: image n < c is x[n], image c + n is y[n].  A workgroup takes 64 pixels; a wave
// takes 16 channels of them (lane = pixel: the reads of the frames and the 16-byte stores of a channel block are contiguous over the wave).
__global__ __launch_bounds__(256) void lp_conv_first_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ wk,
                                                            const float* __restrict__ bias, const float* __restrict__ shift,
                                                            const float* __restrict__ scale, uint4* __restrict__ out_hi,
                                                            uint4* __restrict__ out_lo, int c, int H, int W, int normalize) {
  __shared__ __attribute__((aligned(16))) float w[LP_K1][LP_C1];
  __shared__ __attribute__((aligned(16))) float b[LP_C1];
  __shared__ float sc[8];
  for (int i = threadIdx.x; i < LP_K1 * LP_C1; i += 256) (&w[0][0])[i] = wk[i];
  if (threadIdx.x < LP_C1) b[threadIdx.x] = bias[threadIdx.x];
  if (threadIdx.x < 3) sc[threadIdx.x] = shift[threadIdx.x], sc[4 + threadIdx.x] = scale[threadIdx.x];
  __syncthreads();
  const int HW = H * W;
  const long long P = 2ll * c * HW;
  const long long p = (long long)blockIdx.x * 64 + (threadIdx.x & 63);
  const int q = threadIdx.x >> 6;
  if (p >= P) return;   // after the only barrier
  const int n = (int)(p / HW), rem = (int)(p - (long long)n * HW);
  const int py = rem / W, px = rem - py * W;
  const float* src = n < c ? x + (long long)n * 3 * HW : y + (long long)(n - c) * 3 * HW;
  float in[LP_K1];
#pragma unroll
  for (int ci = 0; ci < 3; ++ci)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int iy = py + tap / 3 - 1, ix = px + tap % 3 - 1;
      float v = 0.f;   // the padding is applied to the SCALED input
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        v = src[(long long)ci * HW + iy * W + ix];
        if (normalize) v = 2.f * v - 1.f;
        v = (v - sc[ci]) / sc[4 + ci];
      }
      in[ci * 9 + tap] = v;
    }
  float acc[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = b[16 * q + o];
#pragma unroll
  for (int k = 0; k < LP_K1; ++k)
#pragma unroll
    for (int o4 = 0; o4 < 4; ++o4) {
      const float4 wv = *reinterpret_cast<const float4*>(&w[k][16 * q + 4 * o4]);
      acc[4 * o4] = fmaf(in[k], wv.x, acc[4 * o4]);
      acc[4 * o4 + 1] = fmaf(in[k], wv.y, acc[4 * o4 + 1]);
      acc[4 * o4 + 2] = fmaf(in[k], wv.z, acc[4 * o4 + 2]);
      acc[4 * o4 + 3] = fmaf(in[k], wv.w, acc[4 * o4 + 3]);
    }
  unsigned hi[8], lo[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) pl_split2(fmaxf(acc[2 * o], 0.f), fmaxf(acc[2 * o + 1], 0.f), hi[o], lo[o]);
  out_hi[(2 * q) * P + p] = make_uint4(hi[0], hi[1], hi[2], hi[3]), out_hi[(2 * q + 1) * P + p] = make_uint4(hi[4], hi[5], hi[6], hi[7]);
  out_lo[(2 * q) * P + p] = make_uint4(lo[0], lo[1], lo[2], lo[3]), out_lo[(2 * q + 1) * P + p] = make_uint4(lo[4], lo[5], lo[6], lo[7]);
}

// planes [Cin / 8][P][8] -> planes [Cout / 8][P][8], P = images * H * W flattened pixels.  grid (ceil(P / 256), Cout / 64), 256 threads.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void lp_conv3x3_kernel(const uint4* __restrict__ in_hi, const uint4* __restrict__ in_lo,
                                                         const uint4* __restrict__ w_hi, const uint4* __restrict__ w_lo,
                                                         const float* __restrict__ bias, unsigned short* __restrict__ out_hi,
                                                         unsigned short* __restrict__ out_lo, int P, int H, int W, int Cin, int Cout) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const long long pt = ((long long)blockIdx.x * LP_WAVES + wave) * LP_PIX;
  if (pt >= P) return;   // wave-uniform; the kernel has no barrier
  const int HW = H * W, KC = Cin >> 4, KS = 9 * KC;
  bool valid[2];
  int pc[2], py[2], px[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long long p = pt + 32 * s + r;
    valid[s] = p < P;
    pc[s] = valid[s] ? (int)p : 0;
    const int rem = pc[s] % HW;
    py[s] = rem / W;
    px[s] = rem - py[s] * W;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][s][i] = 0.f;
  const int ct0 = blockIdx.y * 2;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    bool ok[2];
    long long off[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int iy = py[s] + dy, ix = px[s] + dx;
      ok[s] = valid[s] && iy >= 0 && iy < H && ix >= 0 && ix < W;
      // the neighbour lies in the same image, so its flattened index is pc + dy * W + dx; 16-byte units (a pixel's block of eight channels)
      off[s] = ok[s] ? (long long)h * P + (pc[s] + dy * W + dx) : 0;
    }
    const long long wbase = ((long long)ct0 * KS + tap * KC) * 64 + lane;
    for (int cc = 0; cc < KC; ++cc) {
      PlFrag xf[2], wf[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint4 a = zero, b = zero;
        if (ok[s]) {
          a = in_hi[off[s] + (long long)(2 * cc) * P];
          b = in_lo[off[s] + (long long)(2 * cc) * P];
        }
        xf[s].h = __builtin_bit_cast(bf16x8, a);
        xf[s].l = __builtin_bit_cast(bf16x8, b);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const long long wi = wbase + ((long long)t * KS + cc) * 64;
        wf[t].h = __builtin_bit_cast(bf16x8, w_hi[wi]);
        wf[t].l = __builtin_bit_cast(bf16x8, w_lo[wi]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) pl_mma(acc[t][s], wf[t], xf[s]);   // w_hi.x_lo + w_lo.x_hi + w_hi.x_hi
    }
  }
  // D block (t, s): the lane holds pixel 32 s + r and, in registers 4 g .. 4 g + 3, channels 32 t + 8 g + 4 h + 0..3
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (!valid[s]) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co = (ct0 + t) * 32 + 8 * g + 4 * h;
        const float4 bv = *reinterpret_cast<const float4*>(bias + co);
        unsigned h0, l0, h1, l1;
        pl_split2(fmaxf(acc[t][s][4 * g] + bv.x, 0.f), fmaxf(acc[t][s][4 * g + 1] + bv.y, 0.f), h0, l0);
        pl_split2(fmaxf(acc[t][s][4 * g + 2] + bv.z, 0.f), fmaxf(acc[t][s][4 * g + 3] + bv.w, 0.f), h1, l1);
        const long long e = ((long long)(co >> 3) * P + pc[s]) * 8 + 4 * h;   // channel block co / 8, channels 4 h .. 4 h + 3 of it: 8-byte aligned
        *reinterpret_cast<uint2*>(out_hi + e) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(out_lo + e) = make_uint2(l0, l1);
      }
  }
}

// planes [C/8][N * H * W][8] -> [C/8][N * (H/2) * (W/2)][8]; one thread per (channel block, output pixel)
__global__ __launch_bounds__(256) void lp_pool2x2_kernel(const uint4* __restrict__ in_hi, const uint4* __restrict__ in_lo, uint4* __restrict__ out_hi,
                                                         uint4* __restrict__ out_lo, long long total, int H, int W, long long Pi, long long Po) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H >> 1, Wo = W >> 1;
  const long long k = idx / Po;
  const long long po = idx - k * Po;
  const int xo = (int)(po % Wo);
  const long long t = po / Wo;
  const int yo = (int)(t % Ho);
  const long long n = t / Ho;
  unsigned short bh[8], bl[8];
  float best[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long pi = (n * H + 2 * yo + (q >> 1)) * W + 2 * xo + (q & 1);   // inside the image: Ho = floor(H / 2)
    const uint4 hv = in_hi[k * Pi + pi], lv = in_lo[k * Pi + pi];
    float f[8];
    lp_unpack8(hv, lv, f);
    const unsigned hw[4] = {hv.x, hv.y, hv.z, hv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned short hj = (unsigned short)(hw[j >> 1] >> (16 * (j & 1))), lj = (unsigned short)(lw[j >> 1] >> (16 * (j & 1)));
      if (q == 0 || f[j] > best[j]) best[j] = f[j], bh[j] = hj, bl[j] = lj;
    }
  }
  out_hi[idx] = make_uint4(bh[0] | ((unsigned)bh[1] << 16), bh[2] | ((unsigned)bh[3] << 16), bh[4] | ((unsigned)bh[5] << 16), bh[6] | ((unsigned)bh[7] << 16));
  out_lo[idx] = make_uint4(bl[0] | ((unsigned)bl[1] << 16), bl[2] | ((unsigned)bl[3] << 16), bl[4] | ((unsigned)bl[5] << 16), bl[6] | ((unsigned)bl[7] << 16));
}

// planes [C/8][2c * HW][8]: pair i = images i and c + i.  grid (ceil(HW / 256), c).  A thread owns a pixel (the loads of a wave are contiguous):
// first the two norms over the channels, then the weighted squared difference of the normalised features (not expanded: it would cancel).
__global__ __launch_bounds__(256) void lp_tap_kernel(const uint4* __restrict__ f_hi, const uint4* __restrict__ f_lo, const float* __restrict__ lin,
                                                     double* __restrict__ partial, int c, int HW, int C8, long long P, int np_total, int np_off) {
  __shared__ double red[LP_TAP_PIX / 64];
  const int tid = threadIdx.x;
  const int pair = blockIdx.y;
  const int q = blockIdx.x * LP_TAP_PIX + tid;
  const bool live = q < HW;
  float d = 0.f;
  if (live) {
    const long long ex = (long long)pair * HW + q, ey = (long long)(c + pair) * HW + q;
    float sx = 0.f, sy = 0.f;
    for (int k = 0; k < C8; ++k) {
      float fx[8], fy[8];
      lp_unpack8(f_hi[k * P + ex], f_lo[k * P + ex], fx);
      lp_unpack8(f_hi[k * P + ey], f_lo[k * P + ey], fy);
#pragma unroll
      for (int e = 0; e < 8; ++e) sx = fmaf(fx[e], fx[e], sx), sy = fmaf(fy[e], fy[e], sy);
    }
    const float ax = sqrtf(sx) + 1e-10f, ay = sqrtf(sy) + 1e-10f;
    for (int k = 0; k < C8; ++k) {
      float fx[8], fy[8];
      lp_unpack8(f_hi[k * P + ex], f_lo[k * P + ex], fx);
      lp_unpack8(f_hi[k * P + ey], f_lo[k * P + ey], fy);
      const float4 w0 = *reinterpret_cast<const float4*>(lin + 8 * k), w1 = *reinterpret_cast<const float4*>(lin + 8 * k + 4);
      const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float df = fx[e] / ax - fy[e] / ay;
        d = fmaf(wv[e], df * df, d);
      }
    }
  }
  double v = live ? (double)d : 0.;   // the pixels of the workgroup in a fixed tree: lanes, then the four waves
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) partial[(long long)pair * np_total + np_off + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct LpStages {
  int nblk[LP_STAGES];   // tap workgroups (partials) of a pair per stage
  int hw[LP_STAGES];     // pixels of the stage's map
};

__global__ __launch_bounds__(64) void lp_finish_kernel(const double* __restrict__ partial, float* __restrict__ out, int np_total, LpStages st) {
  const long long pair = blockIdx.x;
  const double* p = partial + pair * np_total;
  double total = 0.;
  for (int s = 0; s < LP_STAGES; ++s) {
    double a = 0.;
    for (int i = threadIdx.x; i < st.nblk[s]; i += 64) a += p[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    total += a / (double)st.hw[s];
    p += st.nblk[s];
  }
  if (threadIdx.x == 0) out[pair] = (float)total;
}

__global__ void lp_mean_kernel(const float* __restrict__ scores, double* __restrict__ per_video, double* __restrict__ mean, int B, int T) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  double s = 0.;
  for (int b = 0; b < B; ++b) {
    const double v = (double)scores[(long long)b * T + t];
    if (per_video) per_video[(long long)b * T + t] = v;
    s += v;
  }
  mean[t] = s / (double)B;
}

inline bool lp_shape_ok(int H, int W, int chunk) {
  return H >= LP_MIN_HW && W >= LP_MIN_HW && chunk >= 1 && chunk <= 16384 && 2ll * chunk * H * W < (1ll << 31) / 64;
}
inline LpStages lp_stages(int H, int W, int* np_total) {
  LpStages st;
  int n = 0;
  for (int s = 0; s < LP_STAGES; ++s) {
    st.hw[s] = (H >> s) * (W >> s);
    st.nblk[s] = (st.hw[s] + LP_TAP_PIX - 1) / LP_TAP_PIX;
    n += st.nblk[s];
  }
  *np_total = n;
  return st;
}
struct LpWs {
  char* bufs[2];     // two activation buffers, each both planes of the widest map (stage 1: 2 chunk images x H x W x 64 channels; every later map is smaller)
  double* partial;   // [chunk][np]: the tap kernel's block sums
  size_t bytes;
};
constexpr size_t LP_WS_SLACK = 256;
inline LpWs lp_carve(void* ws, int H, int W, int chunk, int np) {
  SfArena a(ws);
  LpWs w;
  for (char*& b : w.bufs) b = a.take<char>((size_t)2 * chunk * H * W * LP_C1 * 4);
  w.partial = a.take<double>((size_t)chunk * np);
  w.bytes = a.bytes();
  return w;
}
inline bool lp_channels_ok(int Cout, int Cin) {
  if (Cin == 3) return Cout == LP_C1;
  return (Cin == 64 || Cin == 128 || Cin == 256 || Cin == 512) && (Cout == 64 || Cout == 128 || Cout == 256 || Cout == 512);
}

}  // namespace

extern "C" {

int sf_lpips_pack_conv_weights(const float* w_oihw, void* packed, int Cout, int Cin, void* stream) {
  SF_REQUIRE(w_oihw && packed, "sf_lpips_pack_conv_weights: null pointer");
  SF_REQUIRE(lp_channels_ok(Cout, Cin), "sf_lpips_pack_conv_weights: 3 -> 64 or channel counts of 64, 128, 256 or 512");
  hipStream_t st = (hipStream_t)stream;
  if (Cin == 3) {
    hipLaunchKernelGGL(lp_pack_first_kernel, dim3((LP_K1 * LP_C1 + 255) / 256), dim3(256), 0, st, w_oihw, static_cast<float*>(packed));
  } else {
    const long long n = (long long)Cout * Cin * 9;
    unsigned short* hi = static_cast<unsigned short*>(packed);
    hipLaunchKernelGGL(lp_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w_oihw, hi, hi + n, n, Cin);
  }
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_lpips_pack_conv_weights_host(const float* w_oihw, void* packed, int Cout, int Cin) {
  SF_REQUIRE(w_oihw && packed, "sf_lpips_pack_conv_weights_host: null pointer");
  SF_REQUIRE(lp_channels_ok(Cout, Cin), "sf_lpips_pack_conv_weights_host: 3 -> 64 or channel counts of 64, 128, 256 or 512");
  if (Cin == 3) {
    float* out = static_cast<float*>(packed);
    for (int k = 0; k < LP_K1; ++k)
      for (int co = 0; co < LP_C1; ++co) out[k * LP_C1 + co] = w_oihw[co * LP_K1 + k];
    return 0;
  }
  const long long n = (long long)Cout * Cin * 9;
  unsigned short* hi = static_cast<unsigned short*>(packed);
  unsigned short* lo = hi + n;
  for (long long idx = 0; idx < n; ++idx) {
    const float v = w_oihw[lp_pack_src(idx, Cin)];
    hi[idx] = lp_bf16(v);
    lo[idx] = lp_bf16(v - lp_f32(hi[idx]));
  }
  return 0;
}

size_t sf_lpips_workspace_bytes(int H, int W, int chunk) {
  if (!lp_shape_ok(H, W, chunk)) return 0;
  int np = 0;
  lp_stages(H, W, &np);
  return lp_carve(nullptr, H, W, chunk, np).bytes + LP_WS_SLACK;
}

int sf_lpips_f32(const sf_lpips_model* m, const float* x, const float* y, float* out, int F, int H, int W, int chunk, int normalize,
                 void* workspace, size_t workspace_bytes, void* stream) {
  SF_REQUIRE(m && x && y && out && workspace, "sf_lpips_f32: null pointer");
  SF_REQUIRE(H >= LP_MIN_HW && W >= LP_MIN_HW, "sf_lpips_f32: H and W must be at least 16 (five stages of VGG16)");
  SF_REQUIRE(F >= 0 && lp_shape_ok(H, W, chunk), "sf_lpips_f32: bad shape or chunk (2 * chunk * H * W * 64 must stay below 2^31)");
  SF_REQUIRE(workspace_bytes >= sf_lpips_workspace_bytes(H, W, chunk), "sf_lpips_f32: workspace too small (sf_lpips_workspace_bytes)");
  SF_REQUIRE(m->shift && m->scale, "sf_lpips_f32: null pointer in the model");
  for (int i = 0; i < LP_LAYERS; ++i) SF_REQUIRE(m->conv_w[i] && m->conv_b[i], "sf_lpips_f32: null pointer in the model");
  for (int i = 0; i < LP_STAGES; ++i) SF_REQUIRE(m->lin_w[i], "sf_lpips_f32: null pointer in the model");
  if (F == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int np = 0;
  const LpStages stages = lp_stages(H, W, &np);
  const LpWs ws = lp_carve(workspace, H, W, chunk, np);
  char* const* bufs = ws.bufs;
  double* partial = ws.partial;
  for (int f0 = 0; f0 < F; f0 += chunk) {
    const int c = F - f0 < chunk ? F - f0 : chunk;
    const int N = 2 * c;
    int cur = 0, h = H, w = W, ch = LP_C1, layer = 0, np_off = 0;
    // planes of a map of P pixels x C channels in buffer b, each [C / 8][P][8] bf16: hi at its start, lo right behind
    auto hi_of = [&](int b) { return reinterpret_cast<unsigned short*>(bufs[b]); };
    auto lo_of = [&](int b, long long P, int C) { return reinterpret_cast<unsigned short*>(bufs[b]) + P * C; };
    {
      const long long P = (long long)N * h * w;
      hipLaunchKernelGGL(lp_conv_first_kernel, dim3((unsigned)((P + 63) / 64)), dim3(256), 0, st, x + (long long)f0 * 3 * H * W,
                         y + (long long)f0 * 3 * H * W, static_cast<const float*>(m->conv_w[0]), m->conv_b[0], m->shift, m->scale,
                         reinterpret_cast<uint4*>(hi_of(cur)), reinterpret_cast<uint4*>(lo_of(cur, P, ch)), c, h, w, normalize);
      SF_CHECK_LAUNCH();
      layer = 1;
    }
    for (int s = 0; s < LP_STAGES; ++s) {
      const int cs = lp_stage_ch[s];
      if (s > 0) {
        const long long Pi = (long long)N * h * w, Po = (long long)N * (h >> 1) * (w >> 1);
        const long long total = Po * (ch / 8);
        hipLaunchKernelGGL(lp_pool2x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(hi_of(cur)),
                           reinterpret_cast<const uint4*>(lo_of(cur, Pi, ch)), reinterpret_cast<uint4*>(hi_of(cur ^ 1)),
                           reinterpret_cast<uint4*>(lo_of(cur ^ 1, Po, ch)), total, h, w, Pi, Po);
        SF_CHECK_LAUNCH();
        cur ^= 1, h >>= 1, w >>= 1;
      }
      const long long P = (long long)N * h * w;
      for (int k = (s == 0 ? 1 : 0); k < lp_stage_convs[s]; ++k, ++layer) {
        const uint4* wp = static_cast<const uint4*>(m->conv_w[layer]);
        const long long wn = (long long)cs * ch * 9;   // bf16 elements of a plane
        hipLaunchKernelGGL(lp_conv3x3_kernel, dim3((unsigned)((P + LP_WAVES * LP_PIX - 1) / (LP_WAVES * LP_PIX)), cs / LP_CO), dim3(256), 0, st,
                           reinterpret_cast<const uint4*>(hi_of(cur)), reinterpret_cast<const uint4*>(lo_of(cur, P, ch)), wp, wp + wn / 8,
                           m->conv_b[layer], hi_of(cur ^ 1), lo_of(cur ^ 1, P, cs), (int)P, h, w, ch, cs);
        SF_CHECK_LAUNCH();
        cur ^= 1, ch = cs;
      }
      hipLaunchKernelGGL(lp_tap_kernel, dim3(stages.nblk[s], c), dim3(256), 0, st, reinterpret_cast<const uint4*>(hi_of(cur)),
                         reinterpret_cast<const uint4*>(lo_of(cur, P, ch)), m->lin_w[s], partial, c, h * w, ch / 8, P, np, np_off);
      SF_CHECK_LAUNCH();
      np_off += stages.nblk[s];
    }
    hipLaunchKernelGGL(lp_finish_kernel, dim3(c), dim3(64), 0, st, partial, out + f0, np, stages);
    SF_CHECK_LAUNCH();
  }
  return 0;
}

int sf_lpips_mean_over_videos_f32(const float* scores, double* per_video, double* mean, int B, int T, void* stream) {
  SF_REQUIRE(scores && mean, "sf_lpips_mean_over_videos_f32: null pointer");
  SF_REQUIRE(B >= 1 && T >= 1 && (long long)B * T < (1ll << 31), "sf_lpips_mean_over_videos_f32: bad shape");
  hipLaunchKernelGGL(lp_mean_kernel, dim3((T + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, per_video, mean, B, T);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

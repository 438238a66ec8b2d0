// Egress: the way out of the engine for pictures -- float32 frames, slot decompositions, segment ids and boxes -> the uint8 (or [0, 1] float32)
// videos the reference builds on the host (video_prediction/vp_vis.py make_video / draw_bbox, base_slots/method.py _make_video_grid and its
// `(video * 255.).numpy().astype(np.uint8)`), composed and quantised on the device.  The mirror image of ingest.hip.
//
// Arithmetic: the reference's float32 operations in their order, each rounded once.  x * 0.5 + 0.5 is one fma (the product is exact);
// recons * masks + (1 - masks) * scale and v * 255 go through __fmul_rn / __fadd_rn / __fsub_rn, which the compiler does not contract (the file is
// also built with -ffp-contract=off).  Inputs are assumed finite.
//
// Memory: planes are read coalesced (16 bytes per lane where the source is 16-byte aligned and W % 4 == 0).  Everything whose destination is not a
// plain copy of the source's layout (HWC frames, the rows of a grid canvas) is staged through LDS KEEPING THE DESTINATION'S ALIGNMENT (LDS byte i =
// global byte a0 + i, a0 the destination's start rounded down to 16) and leaves with aligned 16-byte stores, the head and the tail of a span that
// share a 16-byte word with bytes that are not ours byte by byte.
#include "sf_internal.h"
#include "../../include/slotformer_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 1024;        // pixels of one frame per workgroup of the HWC kernel
constexpr int kMaxTiles = 32;
constexpr int kMaxBoxes = 256;
constexpr size_t kLdsMax = 64 * 1024;


// v * 255 (one rounding), clamped to [0, 255], cast toward zero or rounded half to even
__device__ __forceinline__ unsigned quant(float v, int nearest) {
  float s = fminf(fmaxf(__fmul_rn(v, 255.f), 0.f), 255.f);
  if (nearest) s = __builtin_rintf(s);
  return (unsigned)(int)s;
}

__device__ __forceinline__ unsigned frame_byte(float x, int rgb, int nearest) { return quant(rgb ? sf_to_rgb(x) : x, nearest); }

// n bytes S[head ..] -> g[0 ..], head = g & 15: aligned 16-byte stores, the ragged ends byte by byte
__device__ __forceinline__ void lds_to_global(const unsigned char* S, unsigned char* g, int n, int tid) {
  const int head = (int)(reinterpret_cast<uintptr_t>(g) & 15);
  const int nvec = (head + n + 15) >> 4;
  for (int i = tid; i < nvec; i += kThreads) {
    const int o = i << 4;
    if (o >= head && o + 16 <= head + n) {
      *reinterpret_cast<uint4*>(g - head + o) = *reinterpret_cast<const uint4*>(S + o);
    } else {
      for (int q = max(o, head); q < min(o + 16, head + n); ++q) g[q - head] = S[q];
    }
  }
}

// ---- (a) frames ------------------------------------------------------------------------------------------------------------------------
// CHW -> CHW is elementwise on the flat tensor: 16 values per lane (four 16-byte loads, one 16-byte store) for the first n16 groups, the rest
// (all of it when either side is not 16-byte aligned) one value per lane
__global__ __launch_bounds__(kThreads) void frames_chw_kernel(const float* __restrict__ in, unsigned char* __restrict__ out, long long n,
                                                              long long n16, int rgb, int nearest) {
  const long long stride = (long long)gridDim.x * kThreads;
  const long long g0 = (long long)blockIdx.x * kThreads + threadIdx.x;
  for (long long i = g0; i < n16; i += stride) {
    const float4* src = reinterpret_cast<const float4*>(in) + i * 4;
    unsigned w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = src[k];
      w[k] = frame_byte(v.x, rgb, nearest) | (frame_byte(v.y, rgb, nearest) << 8) | (frame_byte(v.z, rgb, nearest) << 16) |
             (frame_byte(v.w, rgb, nearest) << 24);
    }
    reinterpret_cast<uint4*>(out)[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (long long i = n16 * 16 + g0; i < n; i += stride) out[i] = (unsigned char)frame_byte(in[i], rgb, nearest);
}

// CHW -> HWC: one workgroup per (frame, chunk of kChunk pixels); the three plane segments are read coalesced, the bytes interleaved in LDS
template <bool VEC>
__global__ __launch_bounds__(kThreads) void frames_hwc_kernel(const float* __restrict__ in, unsigned char* __restrict__ out, long long items,
                                                              int HW, int chunks, int rgb, int nearest) {
  __shared__ __attribute__((aligned(16))) unsigned char S[kChunk * 3 + 32];
  const int tid = threadIdx.x;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const long long f = item / chunks;
    const int p0 = (int)(item - f * chunks) * kChunk;
    const int np = min(kChunk, HW - p0);
    unsigned char* g = out + (f * HW + p0) * 3;
    const int head = (int)(reinterpret_cast<uintptr_t>(g) & 15);
    const float* src = in + f * 3 * HW + p0;
    if (VEC) {   // HW % 4 == 0 and `in` 16-byte aligned: np, p0 and every plane offset are multiples of 4
      const int n4 = np >> 2;
      for (int i = tid; i < 3 * n4; i += kThreads) {
        const int c = i / n4;
        const int q = i - c * n4;
        const float4 v = *reinterpret_cast<const float4*>(src + (long long)c * HW + (q << 2));
        unsigned char* d = S + head + q * 12 + c;
        d[0] = (unsigned char)frame_byte(v.x, rgb, nearest);
        d[3] = (unsigned char)frame_byte(v.y, rgb, nearest);
        d[6] = (unsigned char)frame_byte(v.z, rgb, nearest);
        d[9] = (unsigned char)frame_byte(v.w, rgb, nearest);
      }
    } else {
      for (int i = tid; i < 3 * np; i += kThreads) {
        const int c = i / np;
        const int q = i - c * np;
        S[head + q * 3 + c] = (unsigned char)frame_byte(src[(long long)c * HW + q], rgb, nearest);
      }
    }
    __syncthreads();
    lds_to_global(S, g, np * 3, tid);
    __syncthreads();   // (the next item overwrites S)
  }
}

// ---- (b) grids -------------------------------------------------------------------------------------------------------------------------
struct GridTile {
  const void* a;   // IMG: x [T,3,H,W]; SLOTS: recons [T,N,3,H,W]; IDS: seg [T,H,W]
  const void* b;   // SLOTS: masks [T,N,1,H,W]; IDS: palette [P,3] uint8
  float scale;
  int kind, n, N, P, i64, hist;
};

constexpr int kTileBytes = kMaxTiles * (int)sizeof(GridTile);
static_assert(kTileBytes % 16 == 0, "the row buffers behind the tile table must stay 16-byte aligned");

struct GridArgs {
  GridTile tile[kMaxTiles];
  unsigned char* out;
  int T, K, H, W, xmaps, ymaps, padding, border, CH, CW;
  int mode;      // 0: float32 CHW, 1: uint8 CHW, 2: uint8 HWC
  int seg;       // LDS bytes per channel row (CHW modes), a multiple of 16
  float pad_value;
};

template <int VW>
__device__ __forceinline__ void load_f32(const float* p, float (&v)[VW]) {
  if (VW == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[VW - 1] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int VW>
__device__ __forceinline__ void load_ids(const void* p, int i64, long long at, int P, int (&id)[VW]) {
  if (i64) {
    const long long* s = static_cast<const long long*>(p) + at;
    if (VW == 4) {
      const longlong2 t0 = *reinterpret_cast<const longlong2*>(s);
      const longlong2 t1 = *reinterpret_cast<const longlong2*>(s + 2);
      const long long t[4] = {t0.x, t0.y, t1.x, t1.y};
#pragma unroll
      for (int j = 0; j < VW; ++j) id[j] = (int)min(max(t[j], 0LL), (long long)(P - 1));
    } else {
      id[0] = (int)min(max(s[0], 0LL), (long long)(P - 1));
    }
  } else {
    const unsigned char* s = static_cast<const unsigned char*>(p) + at;
    if (VW == 4) {
      const uchar4 t = *reinterpret_cast<const uchar4*>(s);
      id[0] = min((int)t.x, P - 1); id[1] = min((int)t.y, P - 1); id[2] = min((int)t.z, P - 1); id[VW - 1] = min((int)t.w, P - 1);
    } else {
      id[0] = min((int)s[0], P - 1);
    }
  }
}

// one workgroup per (frame t, canvas row y): the row of all three channels is composed in LDS and leaves with aligned 16-byte stores
template <int VW>
__global__ __launch_bounds__(kThreads) void grid_kernel(GridArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  const int tid = threadIdx.x;
  // the tile table first (lanes index it by column; kept in the dynamic region so that its base stays 16-byte aligned), the row behind it
  GridTile* tiles = reinterpret_cast<GridTile*>(lds_all);
  unsigned char* lds = lds_all + kTileBytes;
  if (tid == 0)
    for (int k = 0; k < p.K; ++k) tiles[k] = p.tile[k];
  const int t = blockIdx.x / p.CH;
  const int y = blockIdx.x - t * p.CH;
  const int mode = p.mode;
  const int esz = mode == 0 ? 4 : 1;
  // destination spans of this row and where their first byte sits in LDS
  unsigned char* g[3];
  int base[3];
  if (mode == 2) {
    g[0] = p.out + ((long long)t * p.CH + y) * p.CW * 3;
    base[0] = (int)(reinterpret_cast<uintptr_t>(g[0]) & 15);
    g[1] = g[2] = g[0];
    base[1] = base[2] = base[0];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g[c] = p.out + (((long long)t * 3 + c) * p.CH + y) * p.CW * esz;
      base[c] = c * p.seg + (int)(reinterpret_cast<uintptr_t>(g[c]) & 15);
    }
  }
  auto put = [&](int c, int x, float v) {
    const int bc = c == 0 ? base[0] : (c == 1 ? base[1] : base[2]);   // (selects: a lane-indexed array would live in scratch)
    if (mode == 0) *reinterpret_cast<float*>(lds + bc + x * 4) = v;
    else if (mode == 1) lds[bc + x] = (unsigned char)quant(v, 0);
    else lds[base[0] + x * 3 + c] = (unsigned char)quant(v, 0);
  };
  for (int i = tid; i < 3 * p.CW; i += kThreads) {
    const int c = i / p.CW;
    put(c, i - c * p.CW, p.pad_value);
  }
  __syncthreads();
  const int TH = p.H + 2 * p.border, TW = p.W + 2 * p.border;
  const int cellH = TH + p.padding, cellW = TW + p.padding;
  const int yy = y - p.padding;
  const int row = yy >= 0 ? yy / cellH : p.ymaps;
  const int ty = yy - row * cellH;
  if (row < p.ymaps && ty < TH) {
    const int k0 = row * p.xmaps;
    const int ncol = min(p.xmaps, p.K - k0);
    const int sy = ty - p.border;
    const bool in_y = sy >= 0 && sy < p.H;
    if (p.border > 0) {   // the frame around every tile of this grid row: written as it is
      const int nb = in_y ? 2 * p.border : TW;
      for (int i = tid; i < ncol * nb; i += kThreads) {
        const int col = i / nb;
        int tx = i - col * nb;
        if (in_y && tx >= p.border) tx += p.W;
        const int x = col * cellW + p.padding + tx;
        const bool green = t < tiles[k0 + col].hist;
        put(0, x, green ? 0.f : 0.7f);
        put(1, x, green ? 0.7f : 0.f);
        put(2, x, 0.f);
      }
    }
    if (in_y) {
      const int WV = p.W / VW;
      for (int i = tid; i < ncol * WV; i += kThreads) {
        const int col = i / WV;
        const int sx = (i - col * WV) * VW;
        const GridTile& tl = tiles[k0 + col];
        const int x = col * cellW + p.padding + p.border + sx;
        const long long px = (long long)sy * p.W + sx;
        const long long HW = (long long)p.H * p.W;
        if (tl.kind == SF_EGRESS_IMG) {
          const float* a = static_cast<const float*>(tl.a) + (long long)t * 3 * HW + px;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float v[VW];
            load_f32<VW>(a + c * HW, v);
#pragma unroll
            for (int j = 0; j < VW; ++j) put(c, x + j, sf_to_rgb(v[j]));
          }
        } else if (tl.kind == SF_EGRESS_SLOTS) {
          const long long tn = (long long)t * tl.N + tl.n;
          const float* a = static_cast<const float*>(tl.a) + tn * 3 * HW + px;
          float m[VW], om[VW];
          load_f32<VW>(static_cast<const float*>(tl.b) + tn * HW + px, m);
#pragma unroll
          for (int j = 0; j < VW; ++j) om[j] = __fmul_rn(__fsub_rn(1.f, m[j]), tl.scale);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float v[VW];
            load_f32<VW>(a + c * HW, v);
#pragma unroll
            for (int j = 0; j < VW; ++j) put(c, x + j, sf_to_rgb(__fadd_rn(__fmul_rn(v[j], m[j]), om[j])));
          }
        } else {
          int id[VW];
          load_ids<VW>(tl.a, tl.i64, (long long)t * HW + px, tl.P, id);
          const unsigned char* pal = static_cast<const unsigned char*>(tl.b);
#pragma unroll
          for (int j = 0; j < VW; ++j) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float col01 = __fdiv_rn((float)pal[id[j] * 3 + c], 255.f);
              put(c, x + j, sf_to_rgb(__fsub_rn(__fmul_rn(col01, 2.f), 1.f)));
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if (mode == 2) {
    lds_to_global(lds, g[0], p.CW * 3, tid);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) lds_to_global(lds + c * p.seg, g[c], p.CW * esz, tid);
  }
}

// ---- (c) boxes -------------------------------------------------------------------------------------------------------------------------
// one workgroup per (frame, 1024 pixel groups); VW pixels of one row per lane.  The kept boxes of the frame, in order, sit in LDS; a pixel takes
// the colour of the LAST box whose outline covers it, and only groups with a covered pixel are read and written back.
template <int VW>
__global__ __launch_bounds__(kThreads) void boxes_kernel(unsigned char* __restrict__ frames, const float* __restrict__ boxes,
                                                         const unsigned char* __restrict__ pres, const unsigned char* __restrict__ palette,
                                                         int P, int M, int H, int W, int width, int blocks_per_frame) {
  __shared__ int bx[kMaxBoxes][4];
  __shared__ unsigned char keep[kMaxBoxes];
  __shared__ int nkept;
  const int tid = threadIdx.x;
  const int f = blockIdx.x / blocks_per_frame;
  const int blk = blockIdx.x - f * blocks_per_frame;
  const float* fb = boxes + (long long)f * M * 4;
  if (tid < M) keep[tid] = (pres == nullptr || pres[(long long)f * M + tid] != 0) && fb[tid * 4] >= 0.f;
  __syncthreads();
  if (tid < M && keep[tid]) {
    int rank = 0;
    for (int j = 0; j < tid; ++j) rank += keep[j];
#pragma unroll
    for (int q = 0; q < 4; ++q) bx[rank][q] = (int)fminf(fmaxf(fb[tid * 4 + q], -1e6f), 1e6f);   // toward zero (far outside is far enough)
  }
  if (tid == 0) {
    int nk = 0;
    for (int j = 0; j < M; ++j) nk += keep[j];
    nkept = nk;
  }
  __syncthreads();
  const int nk = nkept;
  if (nk == 0) return;
  const int WG = W / VW;
  const int total = H * WG;
  const long long HW = (long long)H * W;
  unsigned char* fr = frames + (long long)f * 3 * HW;
  for (int i = blk * (kThreads * 4) + tid; i < min(total, (blk + 1) * (kThreads * 4)); i += kThreads) {
    const int y = i / WG;
    const int x = (i - y * WG) * VW;
    int hit[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) hit[j] = -1;
    bool any = false;
    for (int k = 0; k < nk; ++k) {
      const int x0 = bx[k][0], y0 = bx[k][1], x1 = bx[k][2], y1 = bx[k][3];
      if (y < y0 || y > y1 || x + VW - 1 < x0 || x > x1) continue;
      const bool edge_y = y - y0 < width || y1 - y < width;
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const int xx = x + j;
        if (xx >= x0 && xx <= x1 && (edge_y || xx - x0 < width || x1 - xx < width)) {
          hit[j] = k;
          any = true;
        }
      }
    }
    if (!any) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      unsigned char* d = fr + c * HW + (long long)y * W + x;
      if (VW == 16) {
        union { uint4 v; unsigned char b[16]; } u;
        u.v = *reinterpret_cast<const uint4*>(d);
#pragma unroll
        for (int j = 0; j < VW; ++j)
          if (hit[j] >= 0) u.b[j] = palette[min(hit[j], P - 1) * 3 + c];
        *reinterpret_cast<uint4*>(d) = u.v;
      } else {
        d[0] = palette[min(hit[0], P - 1) * 3 + c];
      }
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int sf_egress_frames_u8(const float* x, unsigned char* out, long long F, int H, int W, int hwc, int to_rgb, int rounding, void* stream) {
  SF_REQUIRE(x && out, "null pointer (egress frames)");
  SF_REQUIRE(F >= 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "egress frames: sizes must be in [1, 16384], F >= 0");
  SF_REQUIRE((hwc == 0 || hwc == 1) && (to_rgb == 0 || to_rgb == 1) && (rounding == SF_EGRESS_TRUNC || rounding == SF_EGRESS_NEAREST_EVEN),
             "egress frames: hwc / to_rgb are 0 or 1, rounding SF_EGRESS_TRUNC or SF_EGRESS_NEAREST_EVEN");
  SF_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "egress frames: x must be 4-byte aligned");
  if (F == 0) return 0;
  const int HW = H * W;
  const int nearest = rounding == SF_EGRESS_NEAREST_EVEN;
  if (!hwc) {
    const long long n = F * 3 * HW;
    const long long n16 = (aligned16(x) && aligned16(out)) ? n / 16 : 0;
    long long blocks = ((n16 ? n16 : n) + kThreads - 1) / kThreads;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(frames_chw_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x, out, n, n16, to_rgb, nearest);
  } else {
    const int chunks = (HW + kChunk - 1) / kChunk;
    const long long items = F * chunks;
    const long long blocks = items < 0x7fffffffLL ? items : 0x7fffffffLL;
    if (HW % 4 == 0 && aligned16(x))
      hipLaunchKernelGGL(frames_hwc_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x, out, items, HW, chunks,
                         to_rgb, nearest);
    else
      hipLaunchKernelGGL(frames_hwc_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x, out, items, HW, chunks,
                         to_rgb, nearest);
  }
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_egress_grid_shape(int K, int H, int W, int nrow, int padding, int border, int* CH, int* CW) {
  SF_REQUIRE(CH && CW, "null pointer (egress grid shape)");
  SF_REQUIRE(K >= 1 && H > 0 && W > 0 && nrow >= 1 && padding >= 0 && border >= 0, "egress grid: K, H, W, nrow >= 1, padding, border >= 0");
  const int TH = H + 2 * border, TW = W + 2 * border;
  if (K == 1) {   // make_grid hands a single image back as it is
    *CH = TH;
    *CW = TW;
    return 0;
  }
  const int xmaps = nrow < K ? nrow : K;
  const int ymaps = (K + xmaps - 1) / xmaps;
  *CH = ymaps * (TH + padding) + padding;
  *CW = xmaps * (TW + padding) + padding;
  return 0;
}

int sf_egress_grid(const sf_egress_tile* tiles, int n_entries, void* out, int out_mode, int T, int H, int W, int nrow, int padding,
                   float pad_value, int border, void* stream) {
  SF_REQUIRE(tiles && out, "null pointer (egress grid)");
  SF_REQUIRE(n_entries >= 1 && T >= 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384 && nrow >= 1 && padding >= 0 && padding <= 1024 &&
                 border >= 0 && border <= 1024,
             "egress grid: sizes must be in [1, 16384], padding and border in [0, 1024]");
  SF_REQUIRE(out_mode >= SF_EGRESS_F32_CHW && out_mode <= SF_EGRESS_U8_HWC, "egress grid: out_mode is SF_EGRESS_F32_CHW, _U8_CHW or _U8_HWC");
  GridArgs p;
  memset(&p, 0, sizeof(p));
  bool vec = W % 4 == 0;
  int K = 0;
  for (int e = 0; e < n_entries; ++e) {
    const sf_egress_tile& s = tiles[e];
    SF_REQUIRE(s.kind >= SF_EGRESS_IMG && s.kind <= SF_EGRESS_IDS, "egress grid: tile kind is SF_EGRESS_IMG, _SLOTS or _IDS");
    SF_REQUIRE(s.a != nullptr && (s.kind == SF_EGRESS_IMG || s.b != nullptr), "null pointer (egress grid tile)");
    const int count = s.kind == SF_EGRESS_SLOTS ? s.N : 1;
    SF_REQUIRE(count >= 1 && K + count <= kMaxTiles, "egress grid: a SLOTS entry has N >= 1 slots; at most 32 tiles per grid");
    SF_REQUIRE(s.kind != SF_EGRESS_IDS || (s.P >= 1 && s.P <= 256), "egress grid: a palette has 1 .. 256 colours");
    vec = vec && aligned16(s.a) && (s.kind != SF_EGRESS_SLOTS || aligned16(s.b));
    for (int n = 0; n < count; ++n) {
      GridTile& d = p.tile[K++];
      d.a = s.a; d.b = s.b; d.scale = s.scale; d.kind = s.kind; d.n = n; d.N = count; d.P = s.P; d.i64 = s.ids_i64 ? 1 : 0;
      d.hist = s.history_len;
    }
  }
  if (T == 0) return 0;
  if (K == 1) padding = 0;
  SF_TRY(sf_egress_grid_shape(K, H, W, nrow, padding, border, &p.CH, &p.CW));
  p.out = static_cast<unsigned char*>(out);
  p.T = T; p.K = K; p.H = H; p.W = W;
  p.xmaps = nrow < K ? nrow : K;
  p.ymaps = (K + p.xmaps - 1) / p.xmaps;
  p.padding = padding; p.border = border; p.mode = out_mode; p.pad_value = pad_value;
  const int esz = out_mode == SF_EGRESS_F32_CHW ? 4 : 1;
  SF_REQUIRE(out_mode != SF_EGRESS_F32_CHW || (reinterpret_cast<uintptr_t>(out) & 3) == 0, "egress grid: a float32 canvas must be 4-byte aligned");
  p.seg = ((p.CW * esz + 15) / 16) * 16 + 16;
  const size_t lds = kTileBytes + (out_mode == SF_EGRESS_U8_HWC ? (size_t)((p.CW * 3 + 15) / 16) * 16 + 16 : (size_t)3 * p.seg);
  SF_REQUIRE(lds <= kLdsMax, "egress grid: one canvas row does not fit 64 KiB of LDS");
  const long long blocks = (long long)T * p.CH;
  SF_REQUIRE(blocks <= 0x7fffffffLL, "egress grid: too many canvas rows for one launch");
  if (vec)
    hipLaunchKernelGGL(grid_kernel<4>, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(grid_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, p);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_egress_draw_boxes(unsigned char* frames, const float* boxes, const unsigned char* pres, const unsigned char* palette, int P, int F, int M,
                         int H, int W, int width, void* stream) {
  SF_REQUIRE(frames && boxes && palette, "null pointer (egress boxes)");
  SF_REQUIRE(F >= 0 && M >= 0 && M <= kMaxBoxes && H > 0 && W > 0 && H <= 16384 && W <= 16384 && width >= 1 && P >= 1 && P <= 256,
             "egress boxes: sizes in [1, 16384], at most 256 boxes per frame, width >= 1, a palette of 1 .. 256 colours");
  if (F == 0 || M == 0) return 0;
  const bool vec = W % 16 == 0 && aligned16(frames);
  const int total = H * (vec ? W / 16 : W);
  const int bpf = (total + kThreads * 4 - 1) / (kThreads * 4);
  const long long blocks = (long long)F * bpf;
  SF_REQUIRE(blocks <= 0x7fffffffLL, "egress boxes: too many frames for one launch");
  if (vec)
    hipLaunchKernelGGL(boxes_kernel<16>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, frames, boxes, pres, palette, P, M, H, W,
                       width, bpf);
  else
    hipLaunchKernelGGL(boxes_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, frames, boxes, pres, palette, P, M, H, W,
                       width, bpf);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// Ingest: the decoder's uint8 frames -> the normalised, resized float32 frames the first convolution reads (the reference's BaseTransforms,
// base_slots/datasets/utils.py:15-43: ToTensor, Normalize, Resize), nearest-neighbour mask resizing (process_mask) and PHYRE's class-index-to-colour
// lookup (datasets/phyre.py:50), on the device.
//
// Source coordinates and weights are TABLES built on the host in float64 (sf_ingest_tables_host), one per (H0, W0, H, W, mode): per output row and
// per output column the first source index, the tap count and float32 weights.  The kernels do no coordinate arithmetic.
//
// sf_ingest_frames_u8: one workgroup per (frame, band of output rows).  The source rows a band needs are ONE contiguous byte span of the HWC frame:
// it is copied into LDS with aligned 16-byte loads (the head and the tail of the span, which share a 16-byte word with bytes that are not ours, byte
// by byte), keeping its alignment (LDS byte i = global byte a0 + i, a0 the span's start rounded down to 16).  Horizontal pass from those bytes into a
// float32 plane [source row][channel][W] in LDS, vertical pass from there, every channel plane written with coalesced (16-byte where W % 4 == 0)
// stores.  Resampling is linear and the taps of an output sum to 1, so the normalisation (x / 255 - mean) / std = x * a_c + b_c is applied once
// per OUTPUT value.
#include "sf_internal.h"
#include "ingest_norm.h"
#include <math.h>

namespace {

constexpr int kHdrWords = 8;
constexpr int kMagic = 0x53464954;   // 'SFIT'
constexpr int kThreads = 256;
constexpr size_t kLdsBudget = 64 * 1024;     // bands are sized to this: two workgroups per CU
constexpr size_t kLdsMax = 160 * 1024;       // a single output row of a wide source may take the whole CU's

// ---- host: the tables ------------------------------------------------------------------------------------------------------------------
inline double tri(double x) {
  x = fabs(x);
  return x < 1.0 ? 1.0 - x : 0.0;
}

// taps of output i along one axis; w may be NULL (count only).  mode 0: bilinear, align_corners=False, negative source coordinates clamped to 0
// (ATen area_pixel_compute_source_index); 1: the separable triangle filter of antialias=True (ATen _compute_indices_weights_aa: support =
// max(scale, 1), weights normalised to sum 1); 2: nearest (ATen nearest_idx, which works with a FLOAT32 scale: floorf(i * (float)in / out),
// = floor(i * in / out) wherever that quotient is not within float rounding of an integer).
void axis_taps(int in, int out, int mode, int i, int* first, int* count, double* w) {
  const double scale = (double)in / (double)out;
  if (mode == 2) {
    long long s;
    if (out == in) s = i;
    else if (out == 2 * in) s = i >> 1;
    else s = (long long)floorf((float)i * ((float)in / (float)out));
    if (s > in - 1) s = in - 1;
    if (s < 0) s = 0;
    *first = (int)s;
    *count = 1;
    if (w) w[0] = 1.0;
    return;
  }
  if (mode == 0) {
    double src = scale * (i + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    const double l = src - i0;
    *first = i0;
    if (i0 < in - 1) {
      *count = 2;
      if (w) { w[0] = 1.0 - l; w[1] = l; }
    } else {
      *count = 1;
      if (w) w[0] = 1.0;
    }
    return;
  }
  const double support = scale >= 1.0 ? scale : 1.0;
  const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
  const double center = scale * (i + 0.5);
  long long xmin = (long long)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  long long xmax = (long long)(center + support + 0.5);
  if (xmax > in) xmax = in;
  if (xmin > in - 1) xmin = in - 1;
  long long n = xmax - xmin;
  if (n < 1) n = 1;
  *first = (int)xmin;
  *count = (int)n;
  if (w) {
    double total = 0.0;
    for (long long j = 0; j < n; ++j) {
      w[j] = tri((j + xmin - center + 0.5) * invscale);
      total += w[j];
    }
    for (long long j = 0; j < n; ++j) w[j] = total != 0.0 ? w[j] / total : (j == 0 ? 1.0 : 0.0);
  }
}

int axis_max_taps(int in, int out, int mode) {
  int m = 1;
  for (int i = 0; i < out; ++i) {
    int f, c;
    axis_taps(in, out, mode, i, &f, &c, nullptr);
    if (c > m) m = c;
  }
  return m;
}

bool sizes_ok(int H0, int W0, int H, int W, int mode) {
  return H0 > 0 && W0 > 0 && H > 0 && W > 0 && H0 <= 16384 && W0 <= 16384 && H <= 16384 && W <= 16384 && mode >= 0 && mode <= 2;
}

struct Layout {   // word offsets into the table blob
  int tapsY, tapsX, ry_first, ry_count, ry_w, cx_first, cx_count, cx_w, words;
};

Layout layout_of(int H0, int W0, int H, int W, int mode) {
  Layout L;
  L.tapsY = axis_max_taps(H0, H, mode);
  L.tapsX = axis_max_taps(W0, W, mode);
  L.ry_first = kHdrWords;
  L.ry_count = L.ry_first + H;
  L.ry_w = L.ry_count + H;
  L.cx_first = L.ry_w + H * L.tapsY;
  L.cx_count = L.cx_first + W;
  L.cx_w = L.cx_count + W;
  L.words = L.cx_w + W * L.tapsX;
  return L;
}

void fill_axis(int in, int out, int mode, int taps, int* first, int* count, float* w) {
  double tmp[64];
  double* buf = taps <= 64 ? tmp : new double[taps];
  for (int i = 0; i < out; ++i) {
    axis_taps(in, out, mode, i, &first[i], &count[i], buf);
    for (int k = 0; k < taps; ++k) w[(size_t)i * taps + k] = k < count[i] ? (float)buf[k] : 0.0f;
  }
  if (buf != tmp) delete[] buf;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------------
struct IngestArgs {
  const unsigned char* src;
  const unsigned char* palette;   // [K, 3] or NULL
  const int* ry_first;
  const int* ry_count;
  const float* ry_w;
  const int* cx_first;
  const int* cx_count;
  const float* cx_w;
  float* out;
  float a[3], b[3];               // out = sum * a_c + b_c
  int K, F, H0, W0, H, W, tapsY, tapsX;
  int BH, nbands, nrmax;          // output rows per band, bands per frame, most source rows a band reads
  int s_off, t_off;               // LDS byte offsets of the source span and of the float plane (multiples of 16)
  int vec4;                       // W % 4 == 0 and `out` 16-byte aligned: float4 stores
};

template <bool PAL>
__global__ __launch_bounds__(kThreads) void ingest_kernel(IngestArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
  const int bpp = PAL ? 1 : 3;
  const long long row_bytes = (long long)p.W0 * bpp;
  unsigned char* S = lds + p.s_off;
  float* T = reinterpret_cast<float*>(lds + p.t_off);
  if (PAL) {
    for (int i = tid; i < p.K * 3; i += kThreads) lds[i] = p.palette[i];
  }
  const long long items = (long long)p.F * p.nbands;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int f = (int)(item / p.nbands);
    const int band = (int)(item - (long long)f * p.nbands);
    const int y0 = band * p.BH;
    const int y1 = min(p.H, y0 + p.BH);
    // source rows of the band (the tables are monotone); clamped so that a table that does not belong to these sizes cannot send a load outside
    int r0 = min(max(p.ry_first[y0], 0), p.H0 - 1);
    int r1 = min(max(p.ry_first[y1 - 1] + p.ry_count[y1 - 1], r0 + 1), p.H0);
    r1 = min(r1, r0 + p.nrmax);
    const int nr = r1 - r0;
    const unsigned char* g = p.src + ((long long)f * p.H0 + r0) * row_bytes;
    const int n = (int)(nr * row_bytes);
    const int head = (int)(reinterpret_cast<uintptr_t>(g) & 15);
    const int nvec = (head + n + 15) >> 4;
    for (int i = tid; i < nvec; i += kThreads) {
      const int o = i << 4;
      if (o >= head && o + 16 <= head + n) {
        *reinterpret_cast<uint4*>(S + o) = *reinterpret_cast<const uint4*>(g - head + o);
      } else {
        for (int q = max(o, head); q < min(o + 16, head + n); ++q) S[q] = g[q - head];
      }
    }
    __syncthreads();
    // horizontal pass: T[(r * 3 + c) * W + x]
    for (int i = tid; i < nr * p.W; i += kThreads) {
      const int r = i / p.W;
      const int x = i - r * p.W;
      const int fx = min(max(p.cx_first[x], 0), p.W0 - 1);
      const int cnt = min(p.cx_count[x], p.tapsX);
      const unsigned char* row = S + head + r * row_bytes;
      const float* w = p.cx_w + (size_t)x * p.tapsX;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int k = 0; k < cnt; ++k) {
        const int sx = min(fx + k, p.W0 - 1);
        const float wk = w[k];
        if (PAL) {
          const int id = min((int)row[sx], p.K - 1) * 3;
          s0 += wk * (float)lds[id];
          s1 += wk * (float)lds[id + 1];
          s2 += wk * (float)lds[id + 2];
        } else {
          s0 += wk * (float)row[sx * 3];
          s1 += wk * (float)row[sx * 3 + 1];
          s2 += wk * (float)row[sx * 3 + 2];
        }
      }
      T[(r * 3 + 0) * p.W + x] = s0;
      T[(r * 3 + 1) * p.W + x] = s1;
      T[(r * 3 + 2) * p.W + x] = s2;
    }
    __syncthreads();
    // vertical pass: out[f][c][y][x]
    const int nyb = y1 - y0;
    if (p.vec4) {
      const int W4 = p.W >> 2;
      for (int i = tid; i < nyb * 3 * W4; i += kThreads) {
        const int x4 = i % W4;
        const int yc = i / W4;
        const int c = yc % 3;
        const int y = y0 + yc / 3;
        const int fy = p.ry_first[y] - r0;
        const int cnt = min(p.ry_count[y], p.tapsY);
        const float* w = p.ry_w + (size_t)y * p.tapsY;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < cnt; ++k) {
          const int r = min(max(fy + k, 0), nr - 1);
          const float4 v = *reinterpret_cast<const float4*>(T + (r * 3 + c) * p.W + (x4 << 2));
          const float wk = w[k];
          acc.x += wk * v.x; acc.y += wk * v.y; acc.z += wk * v.z; acc.w += wk * v.w;
        }
        const float a = p.a[c], b = p.b[c];
        acc.x = sf_ingest_norm(acc.x, a, b); acc.y = sf_ingest_norm(acc.y, a, b); acc.z = sf_ingest_norm(acc.z, a, b); acc.w = sf_ingest_norm(acc.w, a, b);
        *reinterpret_cast<float4*>(p.out + (((long long)f * 3 + c) * p.H + y) * p.W + (x4 << 2)) = acc;
      }
    } else {
      for (int i = tid; i < nyb * 3 * p.W; i += kThreads) {
        const int x = i % p.W;
        const int yc = i / p.W;
        const int c = yc % 3;
        const int y = y0 + yc / 3;
        const int fy = p.ry_first[y] - r0;
        const int cnt = min(p.ry_count[y], p.tapsY);
        const float* w = p.ry_w + (size_t)y * p.tapsY;
        float acc = 0.f;
        for (int k = 0; k < cnt; ++k) {
          const int r = min(max(fy + k, 0), nr - 1);
          acc += w[k] * T[(r * 3 + c) * p.W + x];
        }
        p.out[(((long long)f * 3 + c) * p.H + y) * p.W + x] = sf_ingest_norm(acc, p.a[c], p.b[c]);
      }
    }
    __syncthreads();   // (the next item overwrites S and T)
  }
}

template <typename TI>
__global__ __launch_bounds__(kThreads) void nearest_kernel(const TI* __restrict__ src, long long* __restrict__ out_i64,
                                                           unsigned char* __restrict__ out_u8, const int* __restrict__ ry,
                                                           const int* __restrict__ cx, long long total, int H0, int W0, int H, int W) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int x = (int)(i % W);
    const long long fy = i / W;
    const int y = (int)(fy % H);
    const long long f = fy / H;
    const int sy = min(max(ry[y], 0), H0 - 1);
    const int sx = min(max(cx[x], 0), W0 - 1);
    const TI v = src[(f * H0 + sy) * W0 + sx];
    if (out_i64) out_i64[i] = (long long)v;
    if (out_u8) out_u8[i] = (unsigned char)v;
  }
}

}  // namespace

extern "C" {

size_t sf_ingest_tables_bytes(int H0, int W0, int H, int W, int mode) {
  if (!sizes_ok(H0, W0, H, W, mode)) return 0;
  return (size_t)layout_of(H0, W0, H, W, mode).words * 4;
}

int sf_ingest_tables_host(void* tables, size_t bytes, int H0, int W0, int H, int W, int mode) {
  SF_REQUIRE(tables != nullptr, "null pointer (ingest tables)");
  SF_REQUIRE(sizes_ok(H0, W0, H, W, mode), "ingest tables: sizes must be in [1, 16384], mode 0 (bilinear), 1 (antialias) or 2 (nearest)");
  const Layout L = layout_of(H0, W0, H, W, mode);
  SF_REQUIRE(bytes >= (size_t)L.words * 4, "ingest tables: buffer smaller than sf_ingest_tables_bytes");
  int* wd = static_cast<int*>(tables);
  const int hdr[kHdrWords] = {kMagic, H0, W0, H, W, mode, L.tapsY, L.tapsX};
  memcpy(wd, hdr, sizeof(hdr));
  fill_axis(H0, H, mode, L.tapsY, wd + L.ry_first, wd + L.ry_count, reinterpret_cast<float*>(wd + L.ry_w));
  fill_axis(W0, W, mode, L.tapsX, wd + L.cx_first, wd + L.cx_count, reinterpret_cast<float*>(wd + L.cx_w));
  return 0;
}

int sf_ingest_frames_u8(const unsigned char* src, const unsigned char* palette, int K, const void* tables, const float* mean3,
                        const float* std3, float* out, int F, int H0, int W0, int H, int W, int antialias, int max_blocks, void* stream) {
  SF_REQUIRE(src && tables && mean3 && std3 && out, "null pointer (ingest frames)");
  SF_REQUIRE(F >= 0 && sizes_ok(H0, W0, H, W, 0) && (antialias == 0 || antialias == 1), "ingest frames: bad sizes or mode");
  SF_REQUIRE(palette ? (K >= 1 && K <= 256) : K == 0, "ingest frames: a palette has 1 .. 256 colours, K = 0 without one");
  SF_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "ingest frames: std must not be 0");
  SF_REQUIRE(max_blocks >= 0, "ingest frames: max_blocks < 0");
  if (F == 0) return 0;
  const Layout L = layout_of(H0, W0, H, W, antialias);
  const int bpp = palette ? 1 : 3;
  const size_t row_bytes = (size_t)W0 * bpp;
  const size_t t_row = (size_t)3 * W * 4;
  const int pal_bytes = 768;
  // the band height: the largest whose source span + float plane fit the budget (one row: up to the whole CU's LDS)
  int* rf = new int[2 * H];
  for (int y = 0; y < H; ++y) axis_taps(H0, H, antialias, y, &rf[y], &rf[H + y], nullptr);
  auto rows_of = [&](int bh) {
    int m = 1;
    for (int y0 = 0; y0 < H; y0 += bh) {
      const int y1 = (y0 + bh < H ? y0 + bh : H) - 1;
      const int nr = rf[y1] + rf[H + y1] - rf[y0];
      if (nr > m) m = nr;
    }
    return m;
  };
  auto lds_of = [&](int nr) { return (size_t)pal_bytes + ((nr * row_bytes + 16 + 15) / 16) * 16 + nr * t_row; };
  int bh = H < 32 ? H : 32;
  while (bh > 1 && lds_of(rows_of(bh)) > kLdsBudget) --bh;
  const int nrmax = rows_of(bh);
  delete[] rf;
  const size_t lds = lds_of(nrmax);
  SF_REQUIRE(lds <= kLdsMax, "ingest frames: the source rows of one output row do not fit the LDS of a CU (source too wide for this ratio)");
  IngestArgs p;
  const int* wd = static_cast<const int*>(tables);
  p.src = src;
  p.palette = palette;
  p.ry_first = wd + L.ry_first;
  p.ry_count = wd + L.ry_count;
  p.ry_w = reinterpret_cast<const float*>(wd + L.ry_w);
  p.cx_first = wd + L.cx_first;
  p.cx_count = wd + L.cx_count;
  p.cx_w = reinterpret_cast<const float*>(wd + L.cx_w);
  p.out = out;
  sf_ingest_norm_coeffs(mean3, std3, p.a, p.b);
  p.K = K; p.F = F; p.H0 = H0; p.W0 = W0; p.H = H; p.W = W; p.tapsY = L.tapsY; p.tapsX = L.tapsX;
  p.BH = bh;
  p.nbands = (H + bh - 1) / bh;
  p.nrmax = nrmax;
  p.s_off = pal_bytes;
  p.t_off = (int)(lds - nrmax * t_row);
  p.vec4 = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;
  long long blocks = (long long)F * p.nbands;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  SF_REQUIRE(blocks <= 0x7fffffffLL, "ingest frames: too many frames for one launch");
  const void* kern = palette ? (const void*)ingest_kernel<true> : (const void*)ingest_kernel<false>;
  if (lds > 64 * 1024) SF_TRY(sf_ensure_dyn_lds(kern, lds));
  if (palette)
    hipLaunchKernelGGL(ingest_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(ingest_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, p);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_resize_masks_nearest(const void* src, int src_is_u8, const void* tables, long long* out_i64, unsigned char* out_u8, int F, int H0,
                            int W0, int H, int W, void* stream) {
  SF_REQUIRE(src && tables && (out_i64 || out_u8), "null pointer (resize masks)");
  SF_REQUIRE(F >= 0 && sizes_ok(H0, W0, H, W, 2), "resize masks: bad sizes");
  const long long total = (long long)F * H * W;
  if (total == 0) return 0;
  const Layout L = layout_of(H0, W0, H, W, 2);
  const int* wd = static_cast<const int*>(tables);
  long long blocks = (total + kThreads - 1) / kThreads;
  if (blocks > 65536) blocks = 65536;
  if (src_is_u8)
    hipLaunchKernelGGL(nearest_kernel<unsigned char>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const unsigned char*>(src), out_i64, out_u8, wd + L.ry_first, wd + L.cx_first, total, H0, W0, H, W);
  else
    hipLaunchKernelGGL(nearest_kernel<long long>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream,
                       static_cast<const long long*>(src), out_i64, out_u8, wd + L.ry_first, wd + L.cx_first, total, H0, W0, H, W);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// Video-prediction metrics on the device (vp_utils.py:44-344 as test_vp.py:149-160 calls them): what the paper's tables are made of, scored where
// the decoder leaves its frames.  Two streaming passes and their small finishes:
//
//   image pass  vp_image_tile_kernel   one workgroup per (frame, channel, 16 x 64 tile of the SSIM map): gt and pred through the to_rgb map into
//                                      LDS, the 11-tap Gaussian along x for the five quantities (x, y, xx, yy, xy) into LDS, along y in registers,
//                                      the SSIM map and the squared error summed in double -> one partial record per workgroup
//               vp_image_finish_kernel one wave per frame: the partial records in a fixed order -> MSE, PSNR, SSIM
//   mask pass   vp_mask_count_kernel   one workgroup per frame: the 16 x 16 contingency table and the predicted classes' boxes, counted per wave
//                                      by ballot (no atomics: every wave owns its table), summed over the four waves at the end
//               vp_mask_score_kernel   one wave per frame: ARI, FG-ARI and the Hungarian mIoU in double from the integer table
//               vp_bbox_pr_kernel      one thread per frame: greedy box precision / recall
//   vp_mean_kernel                     [K][B][T] -> [K][T], summed over the videos in order
//
// Every sum has a fixed order (no floating-point atomics): two runs on the same input give the same bits.
#include <limits.h>
#include <math.h>

#include "sf_common.h"
#include "sf_arena.h"

namespace {

constexpr int VP_R = 5;                    // Gaussian radius: int(truncate 3.5 * sigma 1.5 + 0.5)
constexpr int VP_TW = 64, VP_TH = 16;      // SSIM-map tile of a workgroup (49 KB of LDS: three workgroups per CU)
constexpr int VP_IW = VP_TW + 2 * VP_R;    // 74 input columns
constexpr int VP_IH = VP_TH + 2 * VP_R;    // 26 input rows
constexpr int VP_LD = 76;                  // row stride of the raw tiles: a multiple of 4 floats, so that the 16-byte reads are aligned
constexpr int VP_NCLS = 16;                // the decoder's slot limit (DC_NMAX of elementwise.hip)

struct VpTaps {
  float w[VP_R + 1];   // w[k] = weight at distance k from the centre
};

// The SSIM map is cropped by the filter radius on every side (structural_similarity: crop(S, (win_size - 1) // 2)), so a kept map pixel (oy, ox)
// -- crop coordinates -- reads image rows oy .. oy + 10 and columns ox .. ox + 10 only: no tap of a kept pixel crosses the image edge and scipy's
// `reflect` rows never enter the mean.  A tile therefore loads plain image pixels; what lies outside the image (ragged tiles) is loaded as 0 and
// feeds only map pixels that are masked out.
__global__ __launch_bounds__(256) void vp_image_tile_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                            double* __restrict__ partial, int H, int W, int tiles_x, int tiles_y, int to_rgb, VpTaps taps) {
  __shared__ __attribute__((aligned(16))) float raw[2][VP_IH][VP_LD];
  __shared__ __attribute__((aligned(16))) float hq[5][VP_IH][VP_TW];
  __shared__ double red[2][4];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const long long plane = blockIdx.y;   // frame * 3 + channel
  const int ox0 = tx * VP_TW, oy0 = ty * VP_TH;   // the tile's first map pixel = its first image pixel
  const float* g = gt + plane * H * W;
  const float* p = pred + plane * H * W;
  // the squared error of an image pixel is counted by exactly one tile: the one whose map tile covers it, the edge tiles taking the border too
  const int own_x0 = tx == 0 ? 0 : ox0 + VP_R, own_x1 = tx == tiles_x - 1 ? W : ox0 + VP_TW + VP_R;
  const int own_y0 = ty == 0 ? 0 : oy0 + VP_R, own_y1 = ty == tiles_y - 1 ? H : oy0 + VP_TH + VP_R;
  double sse = 0.;
  for (int idx = tid; idx < VP_IH * VP_LD; idx += 256) {
    const int r = idx / VP_LD, c = idx - r * VP_LD;
    const int iy = oy0 + r, ix = ox0 + c;
    float a = 0.f, b = 0.f;
    if (c < VP_IW && iy < H && ix < W) {
      a = g[(long long)iy * W + ix];
      b = p[(long long)iy * W + ix];
      if (to_rgb) a = sf_to_rgb(a), b = sf_to_rgb(b);
      if (iy >= own_y0 && iy < own_y1 && ix >= own_x0 && ix < own_x1) {
        const float d = a - b;
        sse += (double)(d * d);
      }
    }
    raw[0][r][c] = a;
    raw[1][r][c] = b;
  }
  __syncthreads();
  // along x: four neighbouring outputs per thread from 16 floats of each raw row (four 16-byte reads)
  for (int item = tid; item < VP_IH * (VP_TW / 4); item += 256) {
    const int r = item / (VP_TW / 4), c4 = (item - r * (VP_TW / 4)) * 4;
    float xa[16], ya[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 u = *reinterpret_cast<const float4*>(&raw[0][r][c4 + 4 * j]);
      const float4 v = *reinterpret_cast<const float4*>(&raw[1][r][c4 + 4 * j]);
      xa[4 * j] = u.x, xa[4 * j + 1] = u.y, xa[4 * j + 2] = u.z, xa[4 * j + 3] = u.w;
      ya[4 * j] = v.x, ya[4 * j + 1] = v.y, ya[4 * j + 2] = v.z, ya[4 * j + 3] = v.w;
    }
    float o[5][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
      for (int k = 0; k <= 2 * VP_R; ++k) {
        const float w = taps.w[k < VP_R ? VP_R - k : k - VP_R];
        const float x = xa[j + k], y = ya[j + k];
        sx = fmaf(w, x, sx);
        sy = fmaf(w, y, sy);
        sxx = fmaf(w, x * x, sxx);
        syy = fmaf(w, y * y, syy);
        sxy = fmaf(w, x * y, sxy);
      }
      o[0][j] = sx, o[1][j] = sy, o[2][j] = sxx, o[3][j] = syy, o[4][j] = sxy;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) *reinterpret_cast<float4*>(&hq[q][r][c4]) = make_float4(o[q][0], o[q][1], o[q][2], o[q][3]);
  }
  __syncthreads();
  // along y: a thread owns one column and four map rows; the 14 rows it needs of each quantity pass through registers
  constexpr int RPT = VP_TH / 4;
  const int col = tid & 63, r0 = (tid >> 6) * RPT;
  float f[5][RPT];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float v[RPT + 2 * VP_R];
#pragma unroll
    for (int k = 0; k < RPT + 2 * VP_R; ++k) v[k] = hq[q][r0 + k][col];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k <= 2 * VP_R; ++k) s = fmaf(taps.w[k < VP_R ? VP_R - k : k - VP_R], v[j + k], s);
      f[q][j] = s;
    }
  }
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;   // (K1 L)^2, (K2 L)^2 at data range L = 1
  const int mw = W - 2 * VP_R, mh = H - 2 * VP_R;       // the cropped map
  double ssum = 0.;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const float ux = f[0][j], uy = f[1][j];
    const float vx = f[2][j] - ux * ux, vy = f[3][j] - uy * uy, vxy = f[4][j] - ux * uy;
    const float a1 = 2.f * ux * uy + C1, a2 = 2.f * vxy + C2, b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
    const float s = (a1 * a2) / (b1 * b2);
    if (ox0 + col < mw && oy0 + r0 + j < mh) ssum += (double)s;
  }
  sse = sf_wave_sum(sse);
  ssum = sf_wave_sum(ssum);
  if ((tid & 63) == 0) red[0][tid >> 6] = sse, red[1][tid >> 6] = ssum;
  __syncthreads();
  if (tid < 2) partial[(plane * gridDim.x + blockIdx.x) * 2 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// partial [F][3 * tiles][2] -> the three scores of a frame (mse_metric / peak_signal_noise_ratio / structural_similarity, vp_utils.py:72-106)
__global__ __launch_bounds__(64) void vp_image_finish_kernel(const double* __restrict__ partial, double* __restrict__ mse, double* __restrict__ psnr,
                                                             double* __restrict__ ssim, int n, int H, int W) {
  const long long f = blockIdx.x;
  double a = 0., b = 0.;
  for (int i = threadIdx.x; i < n; i += 64) {
    a += partial[(f * n + i) * 2];
    b += partial[(f * n + i) * 2 + 1];
  }
  a = sf_wave_sum(a);
  b = sf_wave_sum(b);
  if (threadIdx.x == 0) {
    mse[f] = a / 3.;                                        // summed over H and W, averaged over the channels
    psnr[f] = 10. * log10(1. / (a / (3. * H * W)));         // data range 1; +inf for equal frames
    ssim[f] = b / (3. * (double)(H - 2 * VP_R) * (double)(W - 2 * VP_R));
  }
}

// Phase one of the mask metrics.  A wave walks 64 consecutive pixels at a time.  Their (gt, pred) pairs take few distinct values, so the wave
// peels them off one value at a time: a ballot of the lanes that hold it gives the count (popcount) and, the pixels being in row-major order, the
// box (first and last lane give the rows; inside one image row the first and last lane give the columns).  All of that is wave-uniform, lane 0
// adds it to the wave's own table in LDS, and no atomic is needed.  gt == nullptr: boxes only (masks_to_boxes), the pair is the predicted id.
template <typename PT>
__global__ __launch_bounds__(256) void vp_mask_count_kernel(const long long* __restrict__ gt, const PT* __restrict__ pm, unsigned* __restrict__ tables,
                                                            float* __restrict__ boxes, unsigned* __restrict__ flag, int HW, int W, int plimit,
                                                            int nboxes) {
  __shared__ unsigned tab[4][VP_NCLS * VP_NCLS];
  __shared__ int box[4][VP_NCLS][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long f = blockIdx.x;
  for (int i = tid; i < 4 * VP_NCLS * VP_NCLS; i += 256) (&tab[0][0])[i] = 0u;
  if (tid < 4 * VP_NCLS) {
    int* b = box[tid >> 4][tid & 15];
    b[0] = INT_MAX, b[1] = INT_MAX, b[2] = -1, b[3] = -1;
  }
  __syncthreads();
  const long long* gf = gt ? gt + f * HW : nullptr;
  const PT* pf = pm + f * HW;
  bool bad = false;
  for (int i0 = wave * 64; i0 < HW; i0 += 256) {
    const int i = i0 + lane;
    int key = -1;
    if (i < HW) {
      const long long pv = (long long)pf[i];
      const long long gv = gf ? gf[i] : 0;
      if (pv >= 0 && pv < plimit && gv >= 0 && gv < VP_NCLS)
        key = (int)gv * VP_NCLS + (int)pv;
      else
        bad = true;
    }
    unsigned long long pending = __ballot(key >= 0);
    while (pending) {
      const int leader = __builtin_ctzll(pending);
      const int k = __builtin_amdgcn_readlane(key, leader);
      const unsigned long long m = __ballot(key == k);
      pending &= ~m;
      const int first = i0 + __builtin_ctzll(m), last = i0 + 63 - __builtin_clzll(m);
      const int y0 = first / W, y1 = last / W;
      int x0, x1;
      if (y0 == y1) {
        x0 = first - y0 * W;
        x1 = last - y0 * W;
      } else {   // the lanes span image rows: row by row
        x0 = INT_MAX, x1 = -1;
        for (int y = y0; y <= y1; ++y) {
          const int lo = max(y * W - i0, 0), hi = min((y + 1) * W - i0, 64);   // lanes [lo, hi) lie in row y
          const unsigned long long rowmask = (hi - lo >= 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull) << lo);
          const unsigned long long mr = m & rowmask;
          if (mr) {
            x0 = min(x0, i0 + __builtin_ctzll(mr) - y * W);
            x1 = max(x1, i0 + 63 - __builtin_clzll(mr) - y * W);
          }
        }
      }
      if (lane == 0) {
        tab[wave][k] += (unsigned)__popcll(m);
        int* b = box[wave][k & (VP_NCLS - 1)];
        b[0] = min(b[0], x0), b[1] = min(b[1], y0), b[2] = max(b[2], x1), b[3] = max(b[3], y1);
      }
    }
  }
  if (flag && __any(bad) && lane == 0) atomicOr(flag, 1u);
  __syncthreads();
  if (tables) tables[f * (VP_NCLS * VP_NCLS) + tid] = (tab[0][tid] + tab[1][tid]) + (tab[2][tid] + tab[3][tid]);
  if (boxes && tid < nboxes) {
    const int x0 = min(min(box[0][tid][0], box[1][tid][0]), min(box[2][tid][0], box[3][tid][0]));
    const int y0 = min(min(box[0][tid][1], box[1][tid][1]), min(box[2][tid][1], box[3][tid][1]));
    const int x1 = max(max(box[0][tid][2], box[1][tid][2]), max(box[2][tid][2], box[3][tid][2]));
    const int y1 = max(max(box[0][tid][3], box[1][tid][3]), max(box[2][tid][3], box[3][tid][3]));
    float4 o = make_float4(-1.f, -1.f, -1.f, -1.f);   // a class without a pixel (masks_to_boxes_w_empty_mask)
    if (x1 >= 0) o = make_float4((float)x0, (float)y0, (float)x1, (float)y1);
    *reinterpret_cast<float4*>(boxes + (f * nboxes + tid) * 4) = o;
  }
}

// adjusted_rand_index (vp_utils.py:114-163) from the integer table, rows row0 .. 15
__device__ double vp_ari(const unsigned* t, int row0) {
  double rindex = 0., aindex = 0., bindex = 0., npts = 0.;
  for (int g = row0; g < VP_NCLS; ++g) {
    double a = 0.;
    for (int p = 0; p < VP_NCLS; ++p) {
      const double n = (double)t[g * VP_NCLS + p];
      rindex += n * (n - 1.);
      a += n;
    }
    aindex += a * (a - 1.);
    npts += a;
  }
  for (int p = 0; p < VP_NCLS; ++p) {
    double b = 0.;
    for (int g = row0; g < VP_NCLS; ++g) b += (double)t[g * VP_NCLS + p];
    bindex += b * (b - 1.);
  }
  const double expected = aindex * bindex / fmax(npts * (npts - 1.), 1.);
  const double max_r = (aindex + bindex) / 2.;
  const double den = max_r - expected;
  return den != 0. ? (rindex - expected) / den : 1.;
}

// Phase two: one wave per frame loads the table; its first lane does the arithmetic, in double on exact integers.
__global__ __launch_bounds__(64) void vp_mask_score_kernel(const unsigned* __restrict__ tables, double* __restrict__ ari, double* __restrict__ fari,
                                                           double* __restrict__ miou) {
  __shared__ unsigned t[VP_NCLS * VP_NCLS];
  __shared__ double iou[VP_NCLS][VP_NCLS + 1];   // rows 1 .. N, columns 1 .. 16 (the assignment below counts from 1)
  __shared__ double u[VP_NCLS + 1], v[VP_NCLS + 1], minv[VP_NCLS + 1];
  __shared__ int match[VP_NCLS + 1], way[VP_NCLS + 1];
  __shared__ int used[VP_NCLS + 1];
  __shared__ double rows[VP_NCLS], cols[VP_NCLS];
  const long long f = blockIdx.x;
  for (int i = threadIdx.x; i < VP_NCLS * VP_NCLS; i += 64) t[i] = tables[f * (VP_NCLS * VP_NCLS) + i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  ari[f] = vp_ari(t, 0);
  fari[f] = vp_ari(t, 1);
  // hungarian_miou (vp_utils.py:225-243): IoU of every foreground ground-truth id 1 .. N (N = the largest id present: the width of the
  // reference's one_hot; an absent id is a zero row) against the 16 predicted ids (absent ones are zero columns, worth what no match is worth)
  int N = 0;
  for (int g = 0; g < VP_NCLS; ++g) {
    double a = 0.;
    for (int p = 0; p < VP_NCLS; ++p) a += (double)t[g * VP_NCLS + p];
    rows[g] = a;
    if (a > 0.) N = g;
  }
  for (int p = 0; p < VP_NCLS; ++p) {
    double b = 0.;
    for (int g = 0; g < VP_NCLS; ++g) b += (double)t[g * VP_NCLS + p];
    cols[p] = b;
  }
  if (N == 0) {   // no foreground pixel: the reference's mean of nothing
    miou[f] = (double)NAN;
    return;
  }
  for (int g = 1; g <= N; ++g)
    for (int p = 0; p < VP_NCLS; ++p) {
      const double inter = (double)t[g * VP_NCLS + p];
      iou[g][p + 1] = inter / ((rows[g] + cols[p] - inter) + 1e-8);
    }
  // maximum-weight assignment of the N <= 15 rows to the 16 columns: the Hungarian method with potentials on the costs -iou (N^2 * 16 steps)
  const int M = VP_NCLS;
  for (int j = 0; j <= M; ++j) v[j] = 0., match[j] = 0;
  for (int i = 0; i <= N; ++i) u[i] = 0.;
  for (int i = 1; i <= N; ++i) {
    match[0] = i;
    int j0 = 0;
    for (int j = 0; j <= M; ++j) minv[j] = INFINITY, used[j] = 0;
    do {
      used[j0] = 1;
      const int i0 = match[j0];
      double delta = INFINITY;
      int j1 = 0;
      for (int j = 1; j <= M; ++j)
        if (!used[j]) {
          const double cur = -iou[i0][j] - u[i0] - v[j];
          if (cur < minv[j]) minv[j] = cur, way[j] = j0;
          if (minv[j] < delta) delta = minv[j], j1 = j;
        }
      for (int j = 0; j <= M; ++j)
        if (used[j])
          u[match[j]] += delta, v[j] -= delta;
        else
          minv[j] -= delta;
      j0 = j1;
    } while (match[j0] != 0);
    do {
      const int j1 = way[j0];
      match[j0] = match[j1];
      j0 = j1;
    } while (j0);
  }
  double s = 0.;
  for (int j = 1; j <= M; ++j)
    if (match[j]) s += iou[match[j]][j];
  miou[f] = s / (double)N;
}

// bbox_precision_recall (vp_utils.py:180-211), one thread per frame: ground-truth boxes in order, each takes the predicted box of largest IoU
// (the first one on ties; a NaN -- two empty boxes -- counts as the largest, as torch's argmax has it, and never reaches the threshold)
__global__ __launch_bounds__(64) void vp_bbox_pr_kernel(const float* __restrict__ gtb, const unsigned char* __restrict__ pres,
                                                        const float* __restrict__ pb, double* __restrict__ ap, double* __restrict__ ar, int F, int N,
                                                        int M, double thresh) {
  const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
  if (f >= F) return;
  const float* g = gtb + f * N * 4;
  const float* p = pb + f * M * 4;
  unsigned long long used = 0ull;
  int n_gt = 0, n_pred = 0, tp = 0;
  for (int j = 0; j < M; ++j) n_pred += p[j * 4] >= 0.f;
  for (int i = 0; i < N; ++i) {
    if (!pres[f * N + i]) continue;
    ++n_gt;
    const double gx0 = g[i * 4], gy0 = g[i * 4 + 1], gx1 = g[i * 4 + 2], gy1 = g[i * 4 + 3];
    const double ga = (gx1 - gx0) * (gy1 - gy0);
    double best = -INFINITY;
    int bj = -1;
    bool best_nan = false;
    for (int j = 0; j < M; ++j) {
      if (!(p[j * 4] >= 0.f)) continue;
      const double px0 = p[j * 4], py0 = p[j * 4 + 1], px1 = p[j * 4 + 2], py1 = p[j * 4 + 3];
      const double w = fmax(fmin(gx1, px1) - fmax(gx0, px0), 0.), h = fmax(fmin(gy1, py1) - fmax(gy0, py0), 0.);
      const double inter = w * h;
      const double v = inter / (ga + (px1 - px0) * (py1 - py0) - inter);
      if (best_nan) continue;
      if (v != v) {
        best_nan = true, bj = j;
      } else if (bj < 0 || v > best) {
        best = v, bj = j;
      }
    }
    if (bj >= 0 && !best_nan && best >= thresh && !((used >> bj) & 1ull)) {
      ++tp;
      used |= 1ull << bj;
    }
  }
  const bool ok = n_gt > 0 && n_pred > 0;   // (the reference divides by zero here)
  ap[f] = ok ? (double)tp / (double)n_pred : (double)NAN;
  ar[f] = ok ? (double)tp / (double)n_gt : (double)NAN;
}

// out [K][T] = mean over b of per_video [K][B][T], summed in the order of b
__global__ void vp_mean_kernel(const double* __restrict__ pv, double* __restrict__ out, int K, int B, int T) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= K * T) return;
  const int k = idx / T, t = idx - k * T;
  double s = 0.;
  for (int b = 0; b < B; ++b) s += pv[((long long)k * B + b) * T + t];
  out[idx] = s / (double)B;
}

inline int vp_tiles_x(int W) { return (W - 2 * VP_R + VP_TW - 1) / VP_TW; }
inline int vp_tiles_y(int H) { return (H - 2 * VP_R + VP_TH - 1) / VP_TH; }
// One workspace serves both metric calls: [contingency tables of the mask metrics | tile partials of the image metrics]
constexpr size_t VP_WS_SLACK = 256;
inline unsigned* vp_take_tables(SfArena& a, int F) { return a.take<unsigned>((size_t)F * VP_NCLS * VP_NCLS); }
inline double* vp_take_partial(SfArena& a, int F, int H, int W) { return a.take<double>((size_t)F * 3 * vp_tiles_x(W) * vp_tiles_y(H) * 2); }

}  // namespace

extern "C" {

size_t sf_vp_metrics_workspace_bytes(int F, int H, int W) {
  if (F < 0 || H < 2 * VP_R + 1 || W < 2 * VP_R + 1) return 0;
  SfArena a(nullptr);
  vp_take_tables(a, F);
  vp_take_partial(a, F, H, W);
  return a.bytes() + VP_WS_SLACK;
}

int sf_vp_image_metrics_f32(const float* gt, const float* pred, double* mse, double* psnr, double* ssim, int F, int H, int W, int to_rgb,
                            void* workspace, size_t workspace_bytes, void* stream) {
  SF_REQUIRE(gt && pred && mse && psnr && ssim && workspace, "null pointer");
  SF_REQUIRE(H >= 2 * VP_R + 1 && W >= 2 * VP_R + 1, "H and W must be at least 11 (the 11-tap SSIM window)");
  SF_REQUIRE(F >= 0 && (long long)H * W < (1ll << 31), "bad image-metric shape");
  SF_REQUIRE(workspace_bytes >= sf_vp_metrics_workspace_bytes(F, H, W), "workspace too small (sf_vp_metrics_workspace_bytes)");
  if (F == 0) return 0;
  VpTaps taps;
  double w[VP_R + 1], sum = 0.;
  for (int k = 0; k <= VP_R; ++k) {
    w[k] = exp(-0.5 * k * k / (1.5 * 1.5));
    sum += k ? 2. * w[k] : w[k];
  }
  for (int k = 0; k <= VP_R; ++k) taps.w[k] = (float)(w[k] / sum);
  const int txn = vp_tiles_x(W), tyn = vp_tiles_y(H);
  SfArena a(workspace);
  vp_take_tables(a, F);
  double* partial = vp_take_partial(a, F, H, W);
  hipStream_t st = (hipStream_t)stream;
  // (frame, channel) planes on grid.y (at most 65535 per launch)
  for (long long p0 = 0; p0 < (long long)F * 3; p0 += 65535) {
    const int np = (int)((long long)F * 3 - p0 < 65535 ? (long long)F * 3 - p0 : 65535);
    hipLaunchKernelGGL(vp_image_tile_kernel, dim3(txn * tyn, np), dim3(256), 0, st, gt + p0 * H * W, pred + p0 * H * W,
                       partial + p0 * txn * tyn * 2, H, W, txn, tyn, to_rgb, taps);
    SF_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(vp_image_finish_kernel, dim3(F), dim3(64), 0, st, partial, mse, psnr, ssim, 3 * txn * tyn, H, W);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_vp_mask_metrics(const long long* gt_mask, const void* pred_mask, int pred_is_u8, unsigned* tables, float* pred_boxes, double* ari,
                       double* fari, double* miou, unsigned* flag, int F, int H, int W, int num_classes, void* workspace, size_t workspace_bytes,
                       void* stream) {
  SF_REQUIRE(gt_mask && pred_mask && ari && fari && miou && flag, "null pointer");
  SF_REQUIRE(num_classes >= 1 && num_classes <= VP_NCLS, "at most 16 classes");
  SF_REQUIRE(F >= 0 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) - 256, "bad mask-metric shape");
  SfArena a(workspace, workspace_bytes);
  unsigned* ws_tab = F > 0 ? vp_take_tables(a, F) : nullptr;
  SF_REQUIRE(tables || (workspace && a.ok), "workspace too small (sf_vp_metrics_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  if (F == 0) return 0;
  unsigned* tab = tables ? tables : ws_tab;
  if (pred_is_u8)
    hipLaunchKernelGGL(vp_mask_count_kernel<unsigned char>, dim3(F), dim3(256), 0, st, gt_mask, static_cast<const unsigned char*>(pred_mask), tab,
                       pred_boxes, flag, H * W, W, num_classes, VP_NCLS);
  else
    hipLaunchKernelGGL(vp_mask_count_kernel<long long>, dim3(F), dim3(256), 0, st, gt_mask, static_cast<const long long*>(pred_mask), tab, pred_boxes,
                       flag, H * W, W, num_classes, VP_NCLS);
  SF_CHECK_LAUNCH();
  hipLaunchKernelGGL(vp_mask_score_kernel, dim3(F), dim3(64), 0, st, tab, ari, fari, miou);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_masks_to_boxes(const void* masks, int is_u8, float* boxes, unsigned* flag, int F, int H, int W, int num_boxes, void* stream) {
  SF_REQUIRE(masks && boxes, "null pointer");
  SF_REQUIRE(num_boxes >= 1 && num_boxes <= VP_NCLS, "at most 16 classes");
  SF_REQUIRE(F >= 0 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) - 256, "bad mask shape");
  hipStream_t st = (hipStream_t)stream;
  if (flag) {
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  }
  if (F == 0) return 0;
  if (is_u8)
    hipLaunchKernelGGL(vp_mask_count_kernel<unsigned char>, dim3(F), dim3(256), 0, st, (const long long*)nullptr,
                       static_cast<const unsigned char*>(masks), (unsigned*)nullptr, boxes, flag, H * W, W, num_boxes, num_boxes);
  else
    hipLaunchKernelGGL(vp_mask_count_kernel<long long>, dim3(F), dim3(256), 0, st, (const long long*)nullptr, static_cast<const long long*>(masks),
                       (unsigned*)nullptr, boxes, flag, H * W, W, num_boxes, num_boxes);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_vp_bbox_pr_f32(const float* gt_bbox, const unsigned char* gt_pres_mask, const float* pred_bbox, double* ap, double* ar, int F, int N, int M,
                      float ovthresh, void* stream) {
  SF_REQUIRE(gt_bbox && gt_pres_mask && pred_bbox && ap && ar, "null pointer");
  SF_REQUIRE(F >= 0 && N >= 1 && N <= 64 && M >= 1 && M <= 64, "between 1 and 64 boxes per frame on either side");
  if (F == 0) return 0;
  hipLaunchKernelGGL(vp_bbox_pr_kernel, dim3((F + 63) / 64), dim3(64), 0, (hipStream_t)stream, gt_bbox, gt_pres_mask, pred_bbox, ap, ar, F, N, M,
                     (double)ovthresh);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_vp_mean_over_videos_f64(const double* per_video, double* out, int K, int B, int T, void* stream) {
  SF_REQUIRE(per_video && out, "null pointer");
  SF_REQUIRE(K >= 1 && B >= 1 && T >= 1 && (long long)K * T < (1ll << 31), "bad mean shape");
  hipLaunchKernelGGL(vp_mean_kernel, dim3((K * T + 255) / 256), dim3(256), 0, (hipStream_t)stream, per_video, out, K, B, T);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// Annotation masks -> the ground truth of the video-prediction evaluation (the reference's CLEVRER dataset with load_mask: anno2mask, process_mask,
// masks_to_boxes_pad, argmax -- base_slots/datasets/clevrer.py:101-125, datasets/utils.py:46-77), straight from the run lengths at the ingest
// resolution: no dense mask at source size is ever built.
//
// The host parses the COCO run lengths (slotformer_amd/annotations.py) and packs them: the CUMULATIVE run ends of every object one after the other,
// the first run of every object, the first object of every frame.  Run j of an object covers the column-major indices [end[j - 1], end[j]); odd j
// is covered.  An output pixel reads its source pixel from the mode-2 (nearest) table of ingest.hip, p = sx * h + sy, and for every object of its
// frame an upper-bound search of p in the object's run ends gives j.
//
// sf_rle_label_maps: one workgroup per frame (looping when the grid is capped).  The frame's run ends are staged in LDS once -- the first kLdsRuns
// of them; an object whose runs do not lie inside that window is searched in global memory -- and every thread walks the frame's pixels in steps of
// the workgroup.  The extents of an object come from its OWN coverage, not from the label map: a wave that covers any pixel of an object reduces
// min / max / count across its lanes and one lane folds them into the workgroup's LDS record with integer atomics, which are order-independent, so
// the result is bit-stable; the record is written with plain stores when the frame is done, so nothing has to be zeroed before the launch.
// Every offset the kernel reads is clamped to the arrays' lengths: unvalidated arrays give wrong labels, never an access outside them.
#include "sf_internal.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kLdsRuns = 8192;     // run ends staged per frame (32 KiB: two workgroups per CU keep their windows)
constexpr int kMaxObjects = 15;    // ground-truth ids 1 .. 15 (the metric kernels count ids in [0, 16))
constexpr int kMaxBoxes = 64;
constexpr int kHdrWords = 8;       // of the ingest table (ingest.hip)

// number of run ends <= p among e[0 .. n): every index read lies in [0, n)
__device__ __forceinline__ int upper_bound(const unsigned* __restrict__ e, int n, unsigned p) {
  int a = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    if (e[a + half] <= p) {
      a += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return a;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

__global__ __launch_bounds__(kThreads) void rle_label_kernel(const unsigned* __restrict__ ends, const int* __restrict__ obj_off,
                                                             const int* __restrict__ frame_off, const int* __restrict__ ry,
                                                             const int* __restrict__ cx, long long* __restrict__ out_i64,
                                                             unsigned char* __restrict__ out_u8, int* __restrict__ extents, int F, int O, int R,
                                                             int h, int w, int H, int W) {
  __shared__ unsigned s_ends[kLdsRuns];
  __shared__ int s_lo[kMaxObjects], s_n[kMaxObjects];
  __shared__ int s_ext[kMaxObjects][5];   // min x, min y, max x, max y, pixels
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int HW = H * W;
  for (int f = blockIdx.x; f < F; f += gridDim.x) {
    const int o0 = min(max(frame_off[f], 0), O);
    const int o1 = min(max(frame_off[f + 1], o0), O);
    const int nobj = min(o1 - o0, kMaxObjects);
    if (tid < kMaxObjects) {
      int lo = 0, n = 0;
      if (tid < nobj) {
        lo = min(max(obj_off[o0 + tid], 0), R);
        n = min(max(obj_off[o0 + tid + 1], lo), R) - lo;
      }
      s_lo[tid] = lo;
      s_n[tid] = n;
      s_ext[tid][0] = INT_MAX;
      s_ext[tid][1] = INT_MAX;
      s_ext[tid][2] = -1;
      s_ext[tid][3] = -1;
      s_ext[tid][4] = 0;
    }
    __syncthreads();
    const int base = s_lo[0];                       // (0 for a frame without objects)
    const int staged = min(kLdsRuns, R - base);     // >= 0: base <= R
    for (int i = tid; i < staged; i += kThreads) s_ends[i] = ends[base + i];
    __syncthreads();
    for (int i0 = 0; i0 < HW; i0 += kThreads) {     // (uniform trip count: the wave reductions below take every lane)
      const int i = i0 + tid;
      const bool valid = i < HW;
      const int y = valid ? i / W : 0;
      const int x = valid ? i - y * W : 0;
      const int sy = min(max(ry[y], 0), h - 1);
      const int sx = min(max(cx[x], 0), w - 1);
      const unsigned p = (unsigned)sx * (unsigned)h + (unsigned)sy;
      int label = 0;
      for (int k = 0; k < nobj; ++k) {
        const int lo = s_lo[k], n = s_n[k];
        // the object's runs lie inside the staged window, or are read where they lie (uniform over the workgroup)
        const bool in_lds = lo >= base && lo - base + n <= staged;
        const int j = in_lds ? upper_bound(s_ends + (lo - base), n, p) : upper_bound(ends + lo, n, p);
        const bool on = valid && (j & 1) && j < n;
        if (__any(on)) {
          const int mnx = wave_min(on ? x : INT_MAX), mny = wave_min(on ? y : INT_MAX);
          const int mxx = wave_max(on ? x : -1), mxy = wave_max(on ? y : -1);
          const int cnt = __popcll(__ballot(on));
          if (lane == 0) {
            atomicMin(&s_ext[k][0], mnx);
            atomicMin(&s_ext[k][1], mny);
            atomicMax(&s_ext[k][2], mxx);
            atomicMax(&s_ext[k][3], mxy);
            atomicAdd(&s_ext[k][4], cnt);
          }
        }
        if (on && label == 0) label = k + 1;
      }
      if (valid) {
        const long long at = (long long)f * HW + i;
        if (out_i64) out_i64[at] = label;
        if (out_u8) out_u8[at] = (unsigned char)label;
      }
    }
    __syncthreads();
    if (tid < kMaxObjects * 5) {
      const int k = tid / 5, c = tid - k * 5;
      const int v = s_ext[k][c];
      extents[((long long)f * kMaxObjects + k) * 5 + c] = (c < 2 && s_ext[k][4] == 0) ? -1 : v;   // no pixel: -1 -1 -1 -1 0
    }
    __syncthreads();   // (the next frame overwrites the records and the window)
  }
}

// one thread per (frame, output row j): the j-th object with a pixel, in order
__global__ __launch_bounds__(kThreads) void rle_boxes_pad_kernel(const int* __restrict__ extents, float* __restrict__ bbox,
                                                                 unsigned char* __restrict__ pres, unsigned* __restrict__ flag, int F, int num) {
  const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long long)F * num) return;
  const int f = (int)(t / num);
  const int j = (int)(t - (long long)f * num);
  const int* e = extents + (long long)f * kMaxObjects * 5;
  int seen = 0, pick = -1;
  for (int k = 0; k < kMaxObjects; ++k) {
    if (e[k * 5 + 4] > 0) {
      if (seen == j) pick = k;
      ++seen;
    }
  }
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pick >= 0) b = make_float4((float)e[pick * 5], (float)e[pick * 5 + 1], (float)e[pick * 5 + 2], (float)e[pick * 5 + 3]);
  float* o = bbox + t * 4;
  o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w;
  pres[t] = pick >= 0 ? 1 : 0;
  if (j == 0 && seen > num) atomicOr(flag, 1u);
}

}  // namespace

extern "C" {

int sf_rle_label_maps(const unsigned* run_ends, const int* object_offsets, const int* frame_offsets, const void* tables, long long* labels_i64,
                      unsigned char* labels_u8, int* extents, int F, int num_objects, int num_runs, int h, int w, int H, int W, void* stream) {
  SF_REQUIRE(run_ends && object_offsets && frame_offsets && tables && extents, "null pointer (rle label maps)");
  SF_REQUIRE(F >= 0 && num_objects >= 0 && num_runs >= 0, "rle label maps: negative counts");
  SF_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0 && h <= 16384 && w <= 16384 && H <= 16384 && W <= 16384, "rle label maps: sizes must be in [1, 16384]");
  if (F == 0) return 0;
  // the mode-2 table has one tap per output: first[H], count[H], weight[H], first[W], ... (ingest.hip layout_of)
  const int* wd = static_cast<const int*>(tables);
  const int* ry = wd + kHdrWords;
  const int* cx = wd + kHdrWords + 3 * H;
  const int blocks = F < 65536 ? F : 65536;
  hipLaunchKernelGGL(rle_label_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, run_ends, object_offsets, frame_offsets, ry,
                     cx, labels_i64, labels_u8, extents, F, num_objects, num_runs, h, w, H, W);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_rle_boxes_pad(const int* extents, float* bbox, unsigned char* pres_mask, unsigned* flag, int F, int num, void* stream) {
  SF_REQUIRE(extents && bbox && pres_mask && flag, "null pointer (rle boxes)");
  SF_REQUIRE(F >= 0 && num >= 1 && num <= kMaxBoxes, "rle boxes: 1 <= num <= 64");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return sf_set_err((int)e, hipGetErrorString(e), __FILE__, __LINE__);
  if (F == 0) return 0;
  const long long blocks = ((long long)F * num + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(rle_boxes_pad_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, extents, bbox, pres_mask, flag, F, num);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

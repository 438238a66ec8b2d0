// SlotFormer training on clips of a device-resident table (video_prediction.fit): a batch is a list of (video, start) pairs, never a gathered copy.
//   sf_rollout_train_clips_fwd_f32  the rollout training forward whose burn-in frames are read from a slot table [V, T_total, N, C] at
//                                   table[clip_video[b], clip_start[b] + j * frame_offset]: ONE indexed-read launch in place of the `hist` row copies
//                                   of sf_rollout_train_fwd_f32, then that function's own code (rollout_train.hip: sf_rollout_train_steps_ex)
//   sf_clip_mse_f32                 the squared-error loss of slotformer.py:289-318 (per-step weights, the vid_len truncation) and its gradient
//                                   in ONE launch, against targets that lie in the table or in a dense tensor
//   sf_clip_frames_f32              the target frames of the image loss from a uint8 table [V, T_total, H, W, 3] -> normalised [B, S, 3, H, W]
// The device index arrays are trusted: they are never read back, so a (video, start) outside the table reads outside it.
#include "../../include/slotformer_hip.h"
#include "sf_common.h"
#include "sf_vec.h"
#include "rollout_train.h"
#include "ingest_norm.h"

namespace {

constexpr int CT_NT = 256;        // threads per workgroup
constexpr int CM_MAX_GX = 256;    // workgroups per step of the loss launch: the last arriver's thread t owns partial t
constexpr int CM_MAX_S = 64;      // steps of one loss launch
constexpr size_t CM_HEAD = 16;    // bytes in front of the partials: the arrival counter

typedef unsigned long long u64;

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

// slots_all[(j * R + b * N + n) * C + c] = table[((clip_video[b] * T_total + clip_start[b] + j * f) * N + n) * C + c], four floats per thread
__global__ __launch_bounds__(CT_NT) void clip_burnin_kernel(const float* __restrict__ table, const int* __restrict__ clip_video,
                                                            const int* __restrict__ clip_start, float* __restrict__ slots_all, long long T_total,
                                                            int frame_offset, int hist, int B, int NC4) {
  const long long i = (long long)blockIdx.x * CT_NT + threadIdx.x;
  if (i >= (long long)hist * B * NC4) return;
  const int e = (int)(i % NC4);
  const long long jb = i / NC4;
  const int b = (int)(jb % B), j = (int)(jb / B);
  const long long frame = (long long)clip_video[b] * T_total + clip_start[b] + (long long)j * frame_offset;
  ((f32x4*)slots_all)[i] = ((const f32x4*)table)[frame * NC4 + e];
}

struct ClipMseArgs {
  const float* pred;        // [B, S, E]
  const float* target;      // element (b, s, e) at ((vid(b) * T_total + start(b) + first_frame + s * frame_step) * E + e
  const int* clip_video;    // [B] or NULL: vid(b) = b
  const int* clip_start;    // [B] or NULL: start(b) = 0
  const float* step_w;      // [S] or NULL: 1
  const int* clip_len;      // [B] or NULL: every step counts
  float* d_pred;            // [B, S, E] or NULL
  double* stats;            // [1 + 2 S]: loss, per-step sums, per-step counts -- all ADDED to
  unsigned* counter;
  u64* parts;               // [S][gx] sums of squares
  long long T_total;
  int first_frame, frame_step, hist, B, S, E4, gx;
  float scale;
};

// steps of clip b that count: hist + s < clip_len[b]
__device__ __forceinline__ int clip_valid_steps(const ClipMseArgs& a, int b) {
  if (!a.clip_len) return a.S;
  const int v = a.clip_len[b] - a.hist;
  return v < 0 ? 0 : (v > a.S ? a.S : v);
}

// grid (gx, S): workgroup (x, s) strides over the B * E4 float4s of step s.  Three float32 roundings per gradient element: the difference, the
// coefficient scale * w_s * 2 / count (float64, rounded once), their product.
__global__ __launch_bounds__(CT_NT) void clip_mse_kernel(ClipMseArgs a) {
  __shared__ double s_sum[CT_NT / 64];
  __shared__ int s_cnt[CT_NT / 64];
  __shared__ int s_last;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int s = blockIdx.y;
  // the number of counted (clip, step) pairs: integers, so every workgroup finds the same value
  int nv = 0;
  for (int b = t; b < a.B; b += CT_NT) nv += clip_valid_steps(a, b);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) nv += __shfl_xor(nv, o, 64);
  if (lane == 0) s_cnt[wave] = nv;
  __syncthreads();
  const long long pairs = (long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  const double count = (double)pairs * 4.0 * (double)a.E4;
  const float w = a.step_w ? a.step_w[s] : 1.f;
  const float coef = pairs > 0 ? (float)((double)a.scale * (double)w * 2.0 / count) : 0.f;

  double sum = 0.0;
  const long long n = (long long)a.B * a.E4;
  for (long long i = (long long)blockIdx.x * CT_NT + t; i < n; i += (long long)a.gx * CT_NT) {
    const int b = (int)(i / a.E4);
    const int e = (int)(i - (long long)b * a.E4);
    const long long po = ((long long)b * a.S + s) * a.E4 + e;
    if (s >= clip_valid_steps(a, b)) {
      if (a.d_pred) ((f32x4*)a.d_pred)[po] = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const long long frame = (long long)(a.clip_video ? a.clip_video[b] : b) * a.T_total + (a.clip_start ? a.clip_start[b] : 0) + a.first_frame +
                            (long long)s * a.frame_step;
    const f32x4 diff = ((const f32x4*)a.pred)[po] - ((const f32x4*)a.target)[frame * a.E4 + e];
    if (a.d_pred) ((f32x4*)a.d_pred)[po] = diff * coef;
    const f32x4 sq = diff * diff;
    sum += ((double)sq.x + (double)sq.y) + ((double)sq.z + (double)sq.w);
  }
  sum = sf_wave_sum(sum);
  if (lane == 0) s_sum[wave] = sum;
  __syncthreads();
  const unsigned total_wgs = (unsigned)a.gx * (unsigned)a.S;
  if (t == 0) {
    const double wg = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    // write-through 8-byte store, drained before the arrival is counted (the pattern of sf_grad_clip_coef_f32)
    __hip_atomic_store(a.parts + (size_t)s * a.gx + blockIdx.x, __builtin_bit_cast(u64, wg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = (__hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == total_wgs - 1);
  }
  __syncthreads();
  if (!s_last) return;
  // The last workgroup to arrive: per step, thread t takes partial t (gx <= 256), then the fixed tree -- a function of the partials' indices only.
  double loss = 0.0;
  for (int q = 0; q < a.S; ++q) {
    double v = 0.0;
    if (t < a.gx) v = __builtin_bit_cast(double, __hip_atomic_load(a.parts + (size_t)q * a.gx + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    v = sf_wave_sum(v);
    int cq = 0;
    for (int b = t; b < a.B; b += CT_NT) cq += (q < clip_valid_steps(a, b)) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cq += __shfl_xor(cq, o, 64);
    __syncthreads();   // (the previous round's s_sum / s_cnt have been read)
    if (lane == 0) {
      s_sum[wave] = v;
      s_cnt[wave] = cq;
    }
    __syncthreads();
    if (t == 0) {
      const double step_sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
      const long long step_pairs = (long long)s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      a.stats[1 + q] += step_sum;
      a.stats[1 + a.S + q] += (double)step_pairs * 4.0 * (double)a.E4;
      loss += (double)(a.step_w ? a.step_w[q] : 1.f) * step_sum;
    }
  }
  if (t == 0) {
    if (pairs > 0) a.stats[0] += (double)a.scale * loss / count;
    __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
  }
}

// one thread per pixel of a target frame: three bytes in, one float into each channel plane
__global__ __launch_bounds__(CT_NT) void clip_frames_kernel(const unsigned char* __restrict__ table, const int* __restrict__ clip_video,
                                                            const int* __restrict__ clip_start, float* __restrict__ out, long long T_total,
                                                            int first_frame, int frame_step, int B, int S, int HW, float a0, float a1, float a2,
                                                            float b0, float b1, float b2) {
  const long long i = (long long)blockIdx.x * CT_NT + threadIdx.x;
  if (i >= (long long)B * S * HW) return;
  const int px = (int)(i % HW);
  const long long bs = i / HW;
  const int s = (int)(bs % S), b = (int)(bs / S);
  const long long frame = (long long)clip_video[b] * T_total + clip_start[b] + first_frame + (long long)s * frame_step;
  const unsigned char* src = table + (frame * HW + px) * 3;
  float* o = out + bs * 3 * HW + px;
  o[0] = sf_ingest_norm((float)src[0], a0, b0);
  o[HW] = sf_ingest_norm((float)src[1], a1, b1);
  o[2 * (long long)HW] = sf_ingest_norm((float)src[2], a2, b2);
}

inline int cm_gx(long long n4) {
  const long long g = (n4 + CT_NT - 1) / CT_NT;
  return (int)(g < 1 ? 1 : (g > CM_MAX_GX ? CM_MAX_GX : g));
}

}   // namespace

extern "C" {

int sf_rollout_train_clips_fwd_f32(const sf_rollouter* m, const float* table, int T_total, const int* clip_video, const int* clip_start,
                                   int frame_offset, float* pred, int B, int pred_len, float dropout_p, unsigned long long seed, void* ws,
                                   size_t ws_bytes, void* stream) {
  SF_REQUIRE(m && table && clip_video && clip_start && pred && ws, "null pointer (clip forward)");
  SF_REQUIRE(frame_offset >= 1, "clip forward: frame_offset >= 1");
  SF_REQUIRE(B >= 1 && pred_len >= 1, "clip forward: B >= 1, pred_len >= 1");
  SF_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p in [0, 1)");
  SF_REQUIRE(((uintptr_t)table & 15) == 0, "clip forward: the table must be 16-byte aligned");
  float* slots_all = nullptr;
  int hist = 0;
  SF_TRY(sf_rollout_train_burnin_ex(m, B, pred_len, ws, ws_bytes, &slots_all, &hist));
  // the host-known bound: a clip (burn-in and targets) starting at frame 0 must fit a video
  SF_REQUIRE((long long)(hist + pred_len - 1) * frame_offset + 1 <= (long long)T_total, "clip forward: a clip does not fit T_total frames");
  hipStream_t st = (hipStream_t)stream;
  const int NC4 = m->num_slots * m->slot_size / 4;   // (slot_size is a multiple of 64)
  hipLaunchKernelGGL(clip_burnin_kernel, dim3(cdiv((long long)hist * B * NC4, CT_NT)), dim3(CT_NT), 0, st, table, clip_video, clip_start, slots_all,
                     (long long)T_total, frame_offset, hist, B, NC4);
  SF_CHECK_LAUNCH();
  return sf_rollout_train_steps_ex(m, pred, B, pred_len, dropout_p, seed, ws, ws_bytes, st);
}

size_t sf_clip_mse_workspace_bytes(int B, int S, long long E) {
  if (B < 1 || S < 1 || S > CM_MAX_S || E < 4 || E % 4 != 0) return 0;
  return CM_HEAD + (size_t)S * cm_gx((long long)B * (E / 4)) * sizeof(u64);
}

int sf_clip_mse_f32(const float* pred, const float* target, const int* clip_video, const int* clip_start, int T_total, int first_frame,
                    int frame_step, const float* step_w, const int* clip_len, int hist, float scale, float* d_pred, double* stats, int B, int S,
                    long long E, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(pred && target && stats && ws, "null pointer (clip mse)");
  SF_REQUIRE(B >= 1, "clip mse: B >= 1");
  SF_REQUIRE(S >= 1 && S <= CM_MAX_S, "clip mse: 1 to 64 steps");
  SF_REQUIRE(E >= 4 && E % 4 == 0 && E / 4 <= 0x7fffffffLL, "clip mse: the row length must be a multiple of 4");
  SF_REQUIRE(first_frame >= 0 && frame_step >= 1 && hist >= 0, "clip mse: first_frame >= 0, frame_step >= 1, hist >= 0");
  SF_REQUIRE((long long)first_frame + (long long)(S - 1) * frame_step < (long long)T_total, "clip mse: the target steps do not fit T_total frames");
  SF_REQUIRE((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)d_pred) & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)stats & 7) == 0,
             "clip mse: pred, target, d_pred and the workspace must be 16-byte aligned");
  SF_REQUIRE(ws_bytes >= sf_clip_mse_workspace_bytes(B, S, E), "workspace too small (clip mse)");
  ClipMseArgs a;
  a.pred = pred; a.target = target; a.clip_video = clip_video; a.clip_start = clip_start; a.step_w = step_w; a.clip_len = clip_len;
  a.d_pred = d_pred; a.stats = stats; a.counter = (unsigned*)ws; a.parts = (u64*)((char*)ws + CM_HEAD);
  a.T_total = T_total; a.first_frame = first_frame; a.frame_step = frame_step; a.hist = hist; a.B = B; a.S = S; a.E4 = (int)(E / 4);
  a.gx = cm_gx((long long)B * a.E4);
  a.scale = scale;
  hipLaunchKernelGGL(clip_mse_kernel, dim3(a.gx, S), dim3(CT_NT), 0, (hipStream_t)stream, a);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_clip_frames_f32(const unsigned char* table, int T_total, const int* clip_video, const int* clip_start, int first_frame, int frame_step,
                       const float* mean3, const float* std3, float* out, int B, int S, int H, int W, void* stream) {
  SF_REQUIRE(table && clip_video && clip_start && mean3 && std3 && out, "null pointer (clip frames)");
  SF_REQUIRE(B >= 1 && S >= 1, "clip frames: B >= 1, S >= 1");
  SF_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= (1 << 26), "clip frames: bad frame size");
  SF_REQUIRE(first_frame >= 0 && frame_step >= 1, "clip frames: first_frame >= 0, frame_step >= 1");
  SF_REQUIRE((long long)first_frame + (long long)(S - 1) * frame_step < (long long)T_total, "clip frames: the target steps do not fit T_total frames");
  SF_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "clip frames: std must not be 0");
  float a[3], b[3];
  sf_ingest_norm_coeffs(mean3, std3, a, b);
  const long long n = (long long)B * S * H * W;
  SF_REQUIRE((n + CT_NT - 1) / CT_NT <= 0x7fffffffLL, "clip frames: too many pixels for one launch");
  hipLaunchKernelGGL(clip_frames_kernel, dim3(cdiv(n, CT_NT)), dim3(CT_NT), 0, (hipStream_t)stream, table, clip_video, clip_start, out,
                     (long long)T_total, first_frame, frame_step, B, S, H * W, a[0], a[1], a[2], b[0], b[1], b[2]);
  SF_CHECK_LAUNCH();
  return 0;
}

}   // extern "C"

// Backward of the attention half of one Slot-Attention iteration (forward: slot_attn.hip,
// reference savi.py:82-94 / steve.py:50-66 under autograd).
//
//   forward, per frame:  l[p,n] = scale k[p].q[n];  a = softmax_n(l);  a' = a + eps;
//                        num[n] = sum_p a'[p,n] v[p];  den[n] = sum_p a'[p,n];  U[n] = num[n] / den[n]
//   backward from dU:    g[n] = dU[n] / den[n];   c[n] = dU[n].U[n] / den[n]
//                        da'[p,n] = g[n].v[p] - c[n];        dv[p] = sum_n a'[p,n] g[n]
//                        dl[p,n]  = a[p,n] (da'[p,n] - sum_m a[p,m] da'[p,m])
//                        dk[p]    = scale sum_n dl[p,n] q[n];   dq[n] = scale sum_p dl[p,n] k[p]
//
// HBM-bound like the forward: one pass that reads K and V and writes (or accumulates into) dK and dV -- 4 D floats per
// pixel against ~70 D flops.  16 lanes share a pixel (lane j owns the float4 channel groups j, j+16, ...: a 16-lane row
// reads whole 256-byte segments), so the 2N dot products per pixel are 4-step DPP row reductions with no LDS or
// cross-row traffic.  The running dq sums live in registers; the scaled queries and g sit in LDS and are read as broadcasts
// (the 16 lanes of a row read 16 consecutive float4, every row the same ones) -- with them in registers too the kernel
// needed 348 VGPRs, one wave per SIMD, and reached 3.3 TB/s; this way two workgroups share a CU.  Every workgroup emits one
// dq partial record, summed in a fixed order by a second kernel (deterministic).
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "sf_arena.h"

#define SAB_NMAX 8      // the first instantiation: every N <= 8, as before the second existed
#define SAB_NMAX16 16   // 9 .. 16 slots (sf_slot_attn_iter_bwd16_f32)
#define SAB_PIX 256   // pixels per workgroup

// g = dU / den, c = dU.U / den per (frame, slot); one wave per (b, n)
__global__ __launch_bounds__(64) void sa_bwd_prep_kernel(const float* __restrict__ part_num, const float* __restrict__ part_den,
                                                        int P, const float* __restrict__ d_updates, float* __restrict__ g,
                                                        float* __restrict__ c, int N, int D) {
  const int n = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  float den = 0.f;
  for (int p = 0; p < P; ++p) den += part_den[((long long)b * P + p) * N + n];
  const float inv = 1.f / den;
  float dot = 0.f;
  for (int ch = lane; ch < D; ch += 64) {
    float num = 0.f;
    for (int p = 0; p < P; ++p) num += part_num[(((long long)b * P + p) * N + n) * D + ch];
    const float du = d_updates[((long long)b * N + n) * D + ch];
    g[((long long)b * N + n) * D + ch] = du * inv;
    dot += du * (num * inv);
  }
  dot = sf_wave_sum(dot);
  if (lane == 0) c[(long long)b * N + n] = dot * inv;
}

// NS: the slot bound of the softmax (all the frame's slots, in registers).  G: which group of 8 slots this launch keeps running dq sums for.
// 16 slots x D / 64 float4 of dq do not fit the registers at D = 256, so the 16-slot form runs as TWO launches that share the softmax (each
// recomputes the 16 logits of a pixel): G = 0 writes dk / dv and the dq partials of slots 0..7 exactly as the 8-slot kernel does, G = 1 reads the
// rows again and emits only the dq partials of slots 8..15.  Every partial is still one workgroup's sum in a fixed order.
template <int D, int NS = SAB_NMAX, int G = 0>
__global__ __launch_bounds__(256, (D <= 128 ? 2 : 1)) void sa_iter_bwd_kernel(const float* __restrict__ k, const float* __restrict__ v, int ld,
                                                          long long batch_stride, const float* __restrict__ q,
                                                          const float* __restrict__ g, const float* __restrict__ c,
                                                          float* __restrict__ dk, float* __restrict__ dv, int accumulate,
                                                          float* __restrict__ dq_part, int HW, int N, float scale, float eps) {
  constexpr int C4 = D / 64;   // float4 groups per lane
  extern __shared__ float red[];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
  const int tid = threadIdx.x, j = tid & 15, grp = tid >> 4;   // 16 pixel groups per workgroup
  // red: [16][D] floats for the final dq reduction, then qs [NMAX][D] (scaled queries) and gg [NMAX][D]
  float* qsl = red + 16 * D;
  float* ggl = qsl + NS * D;
  for (int i = tid; i < NS * D; i += 256) {
    const int n = i / D;
    qsl[i] = n < N ? q[(long long)b * N * D + i] * scale : 0.f;
    ggl[i] = n < N ? g[(long long)b * N * D + i] : 0.f;
  }
  float4 dqa[SAB_NMAX][C4];   // slots 8 G .. 8 G + 7
  float cc[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) cc[n] = n < N ? c[(long long)b * N + n] : 0.f;
#pragma unroll
  for (int n = 0; n < SAB_NMAX; ++n) {
#pragma unroll
    for (int i = 0; i < C4; ++i) dqa[n][i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
#define QS(n, i) (*reinterpret_cast<const float4*>(&qsl[(n) * D + 4 * (j + 16 * (i))]))
#define GG(n, i) (*reinterpret_cast<const float4*>(&ggl[(n) * D + 4 * (j + 16 * (i))]))
  const long long fb = (long long)b * batch_stride;
  const int p0 = chunk * SAB_PIX;
  float4 kk[C4], vv[C4];
  auto row = [&](int p) { return fb + (long long)p * ld + 4 * j; };
  {
    const int p = p0 + grp;
#pragma unroll
    for (int i = 0; i < C4; ++i) {
      kk[i] = p < HW ? *reinterpret_cast<const float4*>(k + row(p) + 64 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
      vv[i] = p < HW ? *reinterpret_cast<const float4*>(v + row(p) + 64 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  for (int step = 0; step < SAB_PIX / 16; ++step) {
    const int p = p0 + step * 16 + grp;
    float4 kc[C4], vc[C4];
#pragma unroll
    for (int i = 0; i < C4; ++i) {
      kc[i] = kk[i];
      vc[i] = vv[i];
    }
    const int pn = p + 16;
    if (step + 1 < SAB_PIX / 16) {
#pragma unroll
      for (int i = 0; i < C4; ++i) {
        kk[i] = pn < HW ? *reinterpret_cast<const float4*>(k + row(pn) + 64 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        vv[i] = pn < HW ? *reinterpret_cast<const float4*>(v + row(pn) + 64 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    float4 ok[C4], ov[C4];
    if (G == 0 && accumulate && p < HW) {
#pragma unroll
      for (int i = 0; i < C4; ++i) {
        ok[i] = *reinterpret_cast<const float4*>(dk + row(p) + 64 * i);
        ov[i] = *reinterpret_cast<const float4*>(dv + row(p) + 64 * i);
      }
    } else {
#pragma unroll
      for (int i = 0; i < C4; ++i) ok[i] = ov[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s[NS], t[NS];
    float mx = -INFINITY;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      float a = 0.f, e = 0.f;
#pragma unroll
      for (int i = 0; i < C4; ++i) {
        const float4 qv = QS(n, i), gv = GG(n, i);
        a += (kc[i].x * qv.x + kc[i].y * qv.y) + (kc[i].z * qv.z + kc[i].w * qv.w);
        e += (vc[i].x * gv.x + vc[i].y * gv.y) + (vc[i].z * gv.z + vc[i].w * gv.w);
      }
      s[n] = n < N ? sf_sum16(a) : -INFINITY;
      t[n] = sf_sum16(e);
      mx = fmaxf(mx, s[n]);
    }
    float sum = 0.f;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      s[n] = n < N ? __expf(s[n] - mx) : 0.f;
      sum += s[n];
    }
    const float inv = 1.f / sum;
    if constexpr (NS != SAB_NMAX) __builtin_amdgcn_sched_barrier(0);   // (16 slots: the dq products are not scheduled into the logits -- registers)
    float dot = 0.f;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      s[n] *= inv;            // a[p,n]
      t[n] -= cc[n];          // da'[p,n]
      dot += s[n] * t[n];
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const float dl = s[n] * (t[n] - dot);
      const float ap = n < N ? s[n] + eps : 0.f;
#pragma unroll
      for (int i = 0; i < C4; ++i) {
        if constexpr (G == 0) {
          const float4 qv = QS(n, i), gv = GG(n, i);
          ok[i].x += dl * qv.x; ok[i].y += dl * qv.y; ok[i].z += dl * qv.z; ok[i].w += dl * qv.w;
          ov[i].x += ap * gv.x; ov[i].y += ap * gv.y; ov[i].z += ap * gv.z; ov[i].w += ap * gv.w;
        }
        if (n >= SAB_NMAX * G && n < SAB_NMAX * (G + 1)) {   // (n is a compile-time constant of the unrolled loop)
          float4& dq4 = dqa[(n - SAB_NMAX * G) & (SAB_NMAX - 1)][i];
          dq4.x += dl * kc[i].x; dq4.y += dl * kc[i].y; dq4.z += dl * kc[i].z; dq4.w += dl * kc[i].w;
        }
      }
    }
    if (G == 0 && p < HW) {
#pragma unroll
      for (int i = 0; i < C4; ++i) {
        *reinterpret_cast<float4*>(dk + row(p) + 64 * i) = ok[i];
        *reinterpret_cast<float4*>(dv + row(p) + 64 * i) = ov[i];
      }
    }
  }
  // dq partial of this workgroup: sum the 16 pixel groups through LDS, slot by slot ([16][D] floats at a time)
  for (int n = SAB_NMAX * G; n < N && n < SAB_NMAX * (G + 1); ++n) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < C4; ++i) {
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int m = 0; m < SAB_NMAX; ++m)
        if (m + SAB_NMAX * G == n) val = dqa[m][i];
      *reinterpret_cast<float4*>(&red[grp * D + 4 * (j + 16 * i)]) = val;
    }
    __syncthreads();
    for (int ch = tid; ch < D; ch += 256) {
      float a = 0.f;
#pragma unroll
      for (int gi = 0; gi < 16; ++gi) a += red[gi * D + ch];
      dq_part[(((long long)b * nchunks + chunk) * N + n) * D + ch] = a;
    }
  }
}

// dq[b][n][:] = scale * sum_chunks partial
__global__ __launch_bounds__(256) void sa_bwd_dq_reduce_kernel(const float* __restrict__ part, float* __restrict__ dq, int nchunks,
                                                               int ND, float scale) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ND) return;
  float a = 0.f;
  for (int ch = 0; ch < nchunks; ++ch) a += part[((long long)b * nchunks + ch) * ND + i];
  dq[(long long)b * ND + i] = a * scale;
}

// The workspace is ONE block off the arena, packed at 16 bytes inside (the pinned size has no room for 256 per buffer): float offsets of
// c [B, N] and the dq partials [B, nchunks, N, D] behind g [B, N, D].  `floats` counts c unpadded; the up to 12 bytes that start the partials
// on a 16-byte boundary come out of the slack, with the base alignment.
struct SabWs { size_t c, part, floats; };
static constexpr size_t SAB_WS_SLACK = 256;
static SabWs sab_layout(int B, int HW, int N, int D) {
  const size_t nchunks = (size_t)(HW + SAB_PIX - 1) / SAB_PIX, bn = (size_t)B * N;
  SabWs w;
  w.c = bn * D;
  w.part = w.c + ((bn + 3) & ~(size_t)3);
  w.floats = w.c + bn + (size_t)B * nchunks * N * D;
  return w;
}
static size_t sab_workspace_bytes(int B, int HW, int N, int D) { return sab_layout(B, HW, N, D).floats * sizeof(float) + SAB_WS_SLACK; }

// both entry points: nmax = 8 (sf_slot_attn_iter_bwd_f32, whose callers rely on 9 slots being refused) or 16 (sf_slot_attn_iter_bwd16_f32)
static int sab_run(const float* k, const float* v, int ld, long long batch_stride, const float* q, const float* part_num,
                   const float* part_den, int P, const float* d_updates, float* dk, float* dv, int accumulate, float* dq, int B, int HW,
                   int N, int D, float scale, float eps, void* ws, size_t ws_bytes, void* stream, int nmax) {
  SF_REQUIRE(k && v && q && part_num && part_den && d_updates && dk && dv && dq && ws, "null pointer");
  SF_REQUIRE(nmax != SAB_NMAX || (N >= 1 && N <= SAB_NMAX), "need 1 <= num_slots <= 8");
  SF_REQUIRE(B >= 0 && HW > 0 && N >= 1 && N <= SAB_NMAX16 && P >= 1, "need 1 <= num_slots <= 16");
  SF_REQUIRE(D == 64 || D == 128 || D == 192 || D == 256, "slot_size must be 64 / 128 / 192 / 256");
  SF_REQUIRE(ld >= D && (ld % 4) == 0 && (batch_stride % 4) == 0, "k/v rows must be 16-byte aligned");
  SF_REQUIRE(ws_bytes >= sab_workspace_bytes(B, HW, N, D), "workspace too small");
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const SabWs w = sab_layout(B, HW, N, D);
  float* g = SfArena(ws).take(w.floats);
  float* c = g + w.c;
  float* part = g + w.part;
  const int nchunks = (HW + SAB_PIX - 1) / SAB_PIX;
  hipLaunchKernelGGL(sa_bwd_prep_kernel, dim3(N, B), dim3(64), 0, st, part_num, part_den, P, d_updates, g, c, N, D);
  SF_CHECK_LAUNCH();
  if (N <= SAB_NMAX) {
    const size_t lds = (size_t)(16 + 2 * SAB_NMAX) * D * sizeof(float);
#define SAB_LAUNCH(DD)                                                                                                       \
  hipLaunchKernelGGL(sa_iter_bwd_kernel<DD>, dim3(nchunks, B), dim3(256), lds, st, k, v, ld, batch_stride, q, g, c, dk, dv, \
                     accumulate, part, HW, N, scale, eps)
    switch (D) {
      case 64: SAB_LAUNCH(64); break;
      case 128: SAB_LAUNCH(128); break;
      case 192: SAB_LAUNCH(192); break;
      default: SAB_LAUNCH(256); break;
    }
#undef SAB_LAUNCH
    SF_CHECK_LAUNCH();
  } else {
    // 9 .. 16 slots: two launches that share the softmax (see sa_iter_bwd_kernel); the second touches neither dk nor dv
    const size_t lds = (size_t)(16 + 2 * SAB_NMAX16) * D * sizeof(float);   // at most 48 KB
#define SAB_LAUNCH16(DD, GG)                                                                                                           \
  do {                                                                                                                                 \
    SF_TRY(sf_ensure_dyn_lds((const void*)sa_iter_bwd_kernel<DD, SAB_NMAX16, GG>, lds));                                               \
    hipLaunchKernelGGL((sa_iter_bwd_kernel<DD, SAB_NMAX16, GG>), dim3(nchunks, B), dim3(256), lds, st, k, v, ld, batch_stride, q, g, c, \
                       dk, dv, accumulate, part, HW, N, scale, eps);                                                                   \
    SF_CHECK_LAUNCH();                                                                                                                 \
  } while (0)
    switch (D) {
      case 64: SAB_LAUNCH16(64, 0); SAB_LAUNCH16(64, 1); break;
      case 128: SAB_LAUNCH16(128, 0); SAB_LAUNCH16(128, 1); break;
      case 192: SAB_LAUNCH16(192, 0); SAB_LAUNCH16(192, 1); break;
      default: SAB_LAUNCH16(256, 0); SAB_LAUNCH16(256, 1); break;
    }
#undef SAB_LAUNCH16
  }
  hipLaunchKernelGGL(sa_bwd_dq_reduce_kernel, dim3((N * D + 255) / 256, B), dim3(256), 0, st, part, dq, nchunks, N * D, scale);
  SF_CHECK_LAUNCH();
  return 0;
}

extern "C" {

size_t sf_slot_attn_iter_bwd_workspace_bytes(int B, int HW, int N, int D) { return sab_workspace_bytes(B, HW, N, D); }

int sf_slot_attn_iter_bwd_f32(const float* k, const float* v, int ld, long long batch_stride, const float* q,
                              const float* part_num, const float* part_den, int P, const float* d_updates, float* dk, float* dv,
                              int accumulate, float* dq, int B, int HW, int N, int D, float scale, float eps, void* ws,
                              size_t ws_bytes, void* stream) {
  return sab_run(k, v, ld, batch_stride, q, part_num, part_den, P, d_updates, dk, dv, accumulate, dq, B, HW, N, D, scale, eps, ws, ws_bytes,
                 stream, SAB_NMAX);
}

// The same backward for 1 <= N <= 16 slots (N <= 8: the kernel of sf_slot_attn_iter_bwd_f32, same bits; 9 .. 16: the two-launch form).
size_t sf_slot_attn_iter_bwd16_workspace_bytes(int B, int HW, int N, int D) { return sab_workspace_bytes(B, HW, N, D); }

int sf_slot_attn_iter_bwd16_f32(const float* k, const float* v, int ld, long long batch_stride, const float* q,
                                const float* part_num, const float* part_den, int P, const float* d_updates, float* dk, float* dv,
                                int accumulate, float* dq, int B, int HW, int N, int D, float scale, float eps, void* ws,
                                size_t ws_bytes, void* stream) {
  return sab_run(k, v, ld, batch_stride, q, part_num, part_den, P, d_updates, dk, dv, accumulate, dq, B, HW, N, D, scale, eps, ws, ws_bytes,
                 stream, SAB_NMAX16);
}

}  // extern "C"

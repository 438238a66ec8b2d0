// The PHYRE task-success readout (phyre_planning/models/readout.py: PHYREReadout) at inference, and the ranking step of AUCCESS
// (phyre_planning/test_phyre_planning.py: collect_results):
//
//   tokens[b] = [ CLS ; in_proj(slots[b, sel[t], n]) + bias + enc_t_pe[t]  for t in 0..T-1, n in 0..N-1 ]        L = 1 + T N rows of 128
//   x         = the num_layers pre-LN Transformer layers on the tokens                                             (layer_tok128.hip, ONE launch)
//   logit[b]  = w2 . relu(W1 x[b, 0] + b1) + b2
//
//   ph_embed_kernel    a workgroup owns 48 token rows (three 16-row MFMA tiles) of the flattened (b, t, n) space: the slot rows are read IN PLACE
//                      through (stride_v, stride_t) -- no gathered [B, T, N, C] tensor --, split into bf16 hi | lo planes in LDS, and the four waves
//                      sweep the eight 16-column tiles of in_proj (v_mfma_f32_16x16x32_bf16; the weight rows are read as f32 and split on the fly,
//                      as physion_readout.hip: 128 x C floats, L2-resident).  A frame sel[t] == -1 is a frame of zeros: its rows are zero operands
//                      and no address.  The position row is chosen by t, the place in sel, not by the frame number.  The workgroups behind the
//                      row tiles write the CLS rows.
//   ph_head_kernel     a workgroup owns 16 sequences: row 0 of each and W1 (transposed, 64.5 KB) in LDS; thread j < 128 computes hidden unit j
//                      of eight sequences, the logit is a wave sum.  Plain f32 (see the summation order at the kernel).  Optionally
//                      conf = sigmoid(logit), optionally scattered into a caller's table at scatter_index[b].
//   ph_auccess_kernel  one workgroup per task, two passes over the row: c* = max conf over the solved actions, then the count of valid actions
//                      with conf > c* (a solved action wins ties).
//
// Arithmetic of the embedding: split-bf16 -- every f32 operand is bf16 hi + bf16 lo, three products a_hi.b_lo + a_lo.b_hi + a_hi.b_hi with f32
// accumulation from zero, then + bias + pe in f32.  The layers are split-bf16 by construction (layer_tok128.hip), which is why the forward refuses
// every other process precision instead of computing the same logit two ways.  Every sum has a fixed order; no atomics on floats anywhere.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "train_blocks.h"
#include "layer_fused.h"

namespace {

constexpr int PH_D = 128, PH_NH = 8, PH_FFN = 512;   // the shape layer_tok128.hip covers
constexpr int PH_MAXL = 96;        // tokens per sequence (sf_layer_tok_vpw)
constexpr int PH_MAXLAYERS = 8;
constexpr int PH_ROWS = 48;        // token rows of an embed workgroup: three 16-row MFMA tiles
constexpr int PH_THREADS = 256;    // four waves, two column tiles of 16 each
constexpr int PH_WAVES = 4;
constexpr int PH_KS = 8;           // k-steps of 32 at the widest slot (C = 256)
constexpr int PH_CLS_PER_WG = 8;   // CLS rows a tail workgroup writes (32 float4 each)
constexpr int PH_HEAD_SEQ = 16;    // sequences of a head workgroup
constexpr int PH_HEAD_PITCH = PH_D + 1;   // floats of a row of W1^T in LDS: thread j reads column j, conflict-free
constexpr size_t PH_HEAD_LDS = ((size_t)PH_D * PH_HEAD_PITCH + 2 * (size_t)PH_HEAD_SEQ * PH_D) * sizeof(float);

inline bool ph_ok(int N, int C, int T, int d, int nh, int ffn, int nl) {
  return N >= 1 && N <= 16 && C >= 32 && C <= 256 && C % 32 == 0 && T >= 1 && T <= PH_MAXL && 1 + T * N <= PH_MAXL && d == PH_D && nh == PH_NH &&
         ffn == PH_FFN && nl >= 1 && nl <= PH_MAXLAYERS && sf_layer_tok_ok(1 + T * N);
}
__host__ __device__ inline int ph_pitch(int C) { return (C + 8) * 2; }   // bytes of a row of a bf16 plane
inline size_t ph_embed_lds(int C) { return (size_t)2 * PH_ROWS * ph_pitch(C); }

struct PhSel {
  int v[PH_MAXL];   // frame of token group t, or -1: a frame of zeros (T <= 95 entries; by value: the table lives on the host)
};

struct PhEmbed {
  const float* slots;
  long long stride_v, stride_t;
  int V;
  const int* video_index;
  const float *W, *bias, *pe, *cls;   // in_proj.weight [128][C], in_proj.bias [128], enc_t_pe [T][128], CLS [128]
  float* x;                           // [B][L][128]
  int B, T, N, C;
  long long rows;                     // B T N
  int ntiles;                         // row-tile workgroups; the CLS workgroups follow
};

__global__ __launch_bounds__(PH_THREADS) void ph_embed_kernel(const PhEmbed a, const PhSel sel) {
  extern __shared__ __attribute__((aligned(16))) char ph_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, N = a.N, C = a.C, TN = T * N, L = 1 + TN;
  if ((int)blockIdx.x >= a.ntiles) {   // (workgroup-uniform) the CLS rows: token 0 of PH_CLS_PER_WG sequences, a float4 per thread
    const int b = ((int)blockIdx.x - a.ntiles) * PH_CLS_PER_WG + (tid >> 5), c4 = tid & 31;
    if (b < a.B) *reinterpret_cast<f32x4*>(a.x + (long long)b * L * PH_D + c4 * 4) = *reinterpret_cast<const f32x4*>(a.cls + c4 * 4);
    return;
  }
  const int ps = ph_pitch(C);
  char* hi = ph_smem;
  char* lo = ph_smem + PH_ROWS * ps;
  const long long r0 = (long long)blockIdx.x * PH_ROWS;
  const int nrows = a.rows - r0 < PH_ROWS ? (int)(a.rows - r0) : PH_ROWS, rt_n = (nrows + 15) >> 4;
  // ---- the rows as bf16 hi | lo planes; a row past the end, of a zero frame or of a video that does not exist is a zero operand, never an address ----
  const int c4n = C >> 2;
  for (int idx = tid; idx < rt_n * 16 * c4n; idx += PH_THREADS) {
    const int r = idx / c4n, c4 = idx - r * c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < nrows) {
      const long long gr = r0 + r;
      const int b = (int)(gr / TN), rem = (int)(gr - (long long)b * TN), t = rem / N, n = rem - t * N;
      const int f = sel.v[t], vid = a.video_index ? a.video_index[b] : b;
      if (f >= 0 && vid >= 0 && vid < a.V)
        v = *reinterpret_cast<const f32x4*>(a.slots + (long long)vid * a.stride_v + (long long)f * a.stride_t + n * C + c4 * 4);
    }
    sf_split4(reinterpret_cast<__bf16*>(hi + r * ps), reinterpret_cast<__bf16*>(lo + r * ps), c4 * 4, v);
  }
  __syncthreads();
  // ---- A operand: the rows (lane & 15 = row of the tile, k = 8 (lane >> 4) + 0..7); B operand: W[column lane & 15][the same k]; accumulator
  //      register e of a lane = row 4 (lane >> 4) + e, column lane & 15 (the layout of physion_readout.hip: pr_gemm) ----
  const int l15 = lane & 15, q = lane >> 4;
  for (int ct = wid; ct < PH_D / 16; ct += PH_WAVES) {
    const int col = ct * 16 + l15;
    const float* wrow = a.W + (long long)col * C + 8 * q;
    f32x4 acc[3];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < PH_KS; ++ks)
      if (ks < (C >> 5)) {
        bf16x8 wh, wl;
        sf_split8(*reinterpret_cast<const f32x4*>(wrow + ks * 32), *reinterpret_cast<const f32x4*>(wrow + ks * 32 + 4), wh, wl);
#pragma unroll
        for (int rt = 0; rt < 3; ++rt)
          if (rt < rt_n) {
            const int o = (rt * 16 + l15) * ps + (ks * 32 + 8 * q) * 2;
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(hi + o), al = *reinterpret_cast<const bf16x8*>(lo + o);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wl, acc[rt], 0, 0, 0);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wh, acc[rt], 0, 0, 0);
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wh, acc[rt], 0, 0, 0);
          }
      }
    const float bias = a.bias[col];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
      if (rt < rt_n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = rt * 16 + q * 4 + e;
          if (r < nrows) {
            const long long gr = r0 + r;
            const int b = (int)(gr / TN), rem = (int)(gr - (long long)b * TN), t = rem / N;
            const int vid = a.video_index ? a.video_index[b] : b;
            const float val = (acc[rt][e] + bias) + a.pe[t * PH_D + col];
            a.x[((long long)b * L + 1 + rem) * PH_D + col] = (vid >= 0 && vid < a.V) ? val : NAN;   // (a video that does not exist: NaN out)
          }
        }
  }
}

// Summation order (plain f32, whatever the process precision): hidden unit j of a sequence is h_j = fma chain over k = 0..127 ascending starting
// from b1[j]; p_j = relu(h_j) * w2[j]; the logit is the sum over j taken as (p_lane + p_{lane + 64}) per lane, then sf_wave_sum over the 64 lanes
// (16-lane rows by DPP, then (row0 + row1) + (row2 + row3)), + b2 last.  A sequence's logit does not depend on its place in the batch.
__global__ __launch_bounds__(PH_THREADS) void ph_head_kernel(const float* __restrict__ x, int L, const float* __restrict__ W1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ logits,
                                                             float* __restrict__ conf, const int* __restrict__ scatter_index,
                                                             float* __restrict__ scatter_table, long long scatter_len, int B) {
  extern __shared__ __attribute__((aligned(16))) char ph_smem[];
  float* wt = reinterpret_cast<float*>(ph_smem);          // [k][PH_HEAD_PITCH]: W1^T
  float* xs = wt + PH_D * PH_HEAD_PITCH;                  // [PH_HEAD_SEQ][128]: row 0 of the sequences
  float* pp = xs + PH_HEAD_SEQ * PH_D;                    // [PH_HEAD_SEQ][128]: relu(h_j) w2[j]
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s0 = blockIdx.x * PH_HEAD_SEQ, ns = B - s0 < PH_HEAD_SEQ ? B - s0 : PH_HEAD_SEQ;
  for (int idx = tid; idx < PH_D * PH_D; idx += PH_THREADS) {
    const int j = idx >> 7, k = idx & 127;
    wt[k * PH_HEAD_PITCH + j] = W1[idx];
  }
  for (int idx = tid; idx < PH_HEAD_SEQ * PH_D; idx += PH_THREADS) {
    const int s = idx >> 7, k = idx & 127;
    xs[idx] = s < ns ? x[(long long)(s0 + s) * L * PH_D + k] : 0.f;
  }
  __syncthreads();
  {
    const int j = tid & 127, sh = (tid >> 7) * (PH_HEAD_SEQ / 2);   // threads 0..127: sequences 0..7, threads 128..255: sequences 8..15
    float h[PH_HEAD_SEQ / 2];
    const float bj = b1[j], wj = w2[j];
#pragma unroll
    for (int s = 0; s < PH_HEAD_SEQ / 2; ++s) h[s] = bj;
    for (int k = 0; k < PH_D; ++k) {
      const float w = wt[k * PH_HEAD_PITCH + j];
#pragma unroll
      for (int s = 0; s < PH_HEAD_SEQ / 2; ++s) h[s] = fmaf(w, xs[(sh + s) * PH_D + k], h[s]);
    }
#pragma unroll
    for (int s = 0; s < PH_HEAD_SEQ / 2; ++s) pp[(sh + s) * PH_D + j] = fmaxf(h[s], 0.f) * wj;
  }
  __syncthreads();
  const float bias2 = b2[0];
  for (int s = wid; s < PH_HEAD_SEQ; s += PH_WAVES) {   // (whole waves: sf_wave_sum needs every lane; sequences past the end are computed and dropped)
    const float logit = sf_wave_sum(pp[s * PH_D + lane] + pp[s * PH_D + 64 + lane]) + bias2;
    if (lane == 0 && s < ns) {
      const int b = s0 + s;
      logits[b] = logit;
      const float c = 1.0f / (1.0f + expf(-logit));
      if (conf) conf[b] = c;
      if (scatter_table) {
        const long long at = scatter_index[b];
        if (at >= 0 && at < scatter_len) scatter_table[at] = c;   // (an index outside the table is skipped, never an address)
      }
    }
  }
}

// first_rank[task] = #{valid actions whose confidence is strictly above the best solved action's}: the 0-based place of the first solved action in
// the ranking by falling confidence, ties resolved in favour of the solved action; `actions` when the task has no solved action.
__global__ __launch_bounds__(PH_THREADS) void ph_auccess_kernel(const float* __restrict__ conf, const int* __restrict__ status, int* __restrict__ first_rank,
                                                                int actions) {
  __shared__ float smax[PH_WAVES];
  __shared__ int sany[PH_WAVES], scnt[PH_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* c = conf + (long long)blockIdx.x * actions;
  const int* s = status + (long long)blockIdx.x * actions;
  float best = -INFINITY;
  int any = 0;
  for (int i = tid; i < actions; i += PH_THREADS)
    if (s[i] > 0) best = fmaxf(best, c[i]), any = 1;
  best = sf_wave_max(best);
  any = __any(any);
  if (lane == 0) smax[wid] = best, sany[wid] = any;
  __syncthreads();
  best = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  any = sany[0] | sany[1] | sany[2] | sany[3];
  int cnt = 0;
  for (int i = tid; i < actions; i += PH_THREADS) cnt += (s[i] != 0 && c[i] > best) ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) scnt[wid] = cnt;
  __syncthreads();
  if (tid == 0) first_rank[blockIdx.x] = any ? scnt[0] + scnt[1] + scnt[2] + scnt[3] : actions;
}

inline bool ph_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// The token rows alone, for the training forward (phyre_readout_train.hip): ph_embed_kernel on arguments its caller has validated as
// sf_phyre_readout_fwd_f32 validates its own (shape, strides, sel in [-1, T_all), 16-byte alignment); x [B][1 + T N][128].
int sf_phyre_embed_ex(const float* slots, long long stride_v, long long stride_t, int V, const int* video_index, const int* sel, const float* in_proj_w,
                      const float* in_proj_b, const float* enc_t_pe, const float* cls, float* x, int B, int T, int N, int C, hipStream_t st) {
  PhSel table;
  for (int t = 0; t < PH_MAXL; ++t) table.v[t] = t < T ? sel[t] : -1;
  PhEmbed a;
  a.slots = slots; a.stride_v = stride_v; a.stride_t = stride_t; a.V = V; a.video_index = video_index;
  a.W = in_proj_w; a.bias = in_proj_b; a.pe = enc_t_pe; a.cls = cls; a.x = x;
  a.B = B; a.T = T; a.N = N; a.C = C;
  a.rows = (long long)B * T * N;
  SF_REQUIRE((a.rows + PH_ROWS - 1) / PH_ROWS + (B + PH_CLS_PER_WG - 1) / PH_CLS_PER_WG < (1LL << 31), "sf_phyre_embed_ex: batch too large for one launch");
  a.ntiles = (int)((a.rows + PH_ROWS - 1) / PH_ROWS);
  const size_t lds = ph_embed_lds(C);
  SF_TRY(sf_ensure_dyn_lds((const void*)ph_embed_kernel, lds));
  hipLaunchKernelGGL(ph_embed_kernel, dim3((unsigned)(a.ntiles + (B + PH_CLS_PER_WG - 1) / PH_CLS_PER_WG)), dim3(PH_THREADS), lds, st, a, table);
  SF_CHECK_LAUNCH();
  return 0;
}

#define PH_LIMITS "1 <= num_slots <= 16, slot_size a multiple of 32 in [32, 256], T >= 1, 1 + T * num_slots <= 96, (d_model, heads, ffn) = (128, 8, 512), 1 <= num_layers <= 8"

extern "C" {

int sf_phyre_readout_ok(int num_slots, int slot_size, int T, int d_model, int num_heads, int ffn, int num_layers) {
  return ph_ok(num_slots, slot_size, T, d_model, num_heads, ffn, num_layers) ? 1 : 0;
}

size_t sf_phyre_readout_workspace_bytes(int B, int num_slots, int T) {
  if (B < 1 || num_slots < 1 || num_slots > 16 || T < 1 || T > PH_MAXL || 1 + T * num_slots > PH_MAXL) return 0;
  return 2 * (size_t)B * (1 + (size_t)T * num_slots) * PH_D * sizeof(float);   // the token rows before and behind the layers
}

int sf_phyre_readout_fwd_f32(const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index, const int* sel,
                             const float* in_proj_w, const float* in_proj_b, const float* enc_t_pe, const float* cls, const sf_tfm_layer* layers,
                             int num_layers, int d_model, int num_heads, int ffn, const float* mlp_w1, const float* mlp_b1, const float* mlp_w2,
                             const float* mlp_b2, float* logits, float* conf, const int* scatter_index, float* scatter_table, long long scatter_len,
                             int B, int T, int N, int C, void* workspace, size_t workspace_bytes, void* stream) {
  SF_REQUIRE(slots && sel && in_proj_w && in_proj_b && enc_t_pe && cls && layers && mlp_w1 && mlp_b1 && mlp_w2 && mlp_b2 && logits && workspace,
             "sf_phyre_readout_fwd_f32: null pointer");
  SF_REQUIRE(ph_ok(N, C, T, d_model, num_heads, ffn, num_layers), "sf_phyre_readout_fwd_f32: unsupported shape (" PH_LIMITS ")");
  SF_REQUIRE(B >= 1 && V >= 1 && T_all >= 1, "sf_phyre_readout_fwd_f32: B >= 1, V >= 1, T_all >= 1");
  SF_REQUIRE(stride_t >= (long long)N * C && stride_t % 4 == 0 && stride_v >= 0 && stride_v % 4 == 0,
             "sf_phyre_readout_fwd_f32: frame stride >= N * C, strides multiples of 4");
  SF_REQUIRE(video_index || B <= V, "sf_phyre_readout_fwd_f32: B > V without a video_index");
  PhSel table;
  for (int t = 0; t < PH_MAXL; ++t) table.v[t] = -1;
  for (int t = 0; t < T; ++t) {
    SF_REQUIRE(sel[t] >= -1 && sel[t] < T_all, "sf_phyre_readout_fwd_f32: sel[t] must lie in [-1, T_all) (-1: a frame of zeros)");
    table.v[t] = sel[t];
  }
  SF_REQUIRE(!scatter_table || (scatter_index && scatter_len >= 1), "sf_phyre_readout_fwd_f32: a scatter table needs scatter_index and scatter_len >= 1");
  SF_REQUIRE(ph_al16(slots) && ph_al16(in_proj_w) && ph_al16(cls) && ph_al16(workspace),
             "sf_phyre_readout_fwd_f32: slots, in_proj_w, cls and the workspace must be 16-byte aligned");
  SF_REQUIRE(workspace_bytes >= sf_phyre_readout_workspace_bytes(B, N, T), "sf_phyre_readout_fwd_f32: workspace too small");
  for (int l = 0; l < num_layers; ++l)
    SF_REQUIRE(layers[l].tok_packed != nullptr, "sf_phyre_readout_fwd_f32: every layer needs its sf_pack_layer_tok_weights copy (tok_packed)");
  SF_REQUIRE(sf_get_precision() == 1, "sf_phyre_readout_fwd_f32: split-bf16 mode only (the layers have no other form)");
  const int L = 1 + T * N;
  float* x = static_cast<float*>(workspace);
  float* y = x + (size_t)B * L * PH_D;
  hipStream_t st = (hipStream_t)stream;
  PhEmbed a;
  a.slots = slots; a.stride_v = stride_v; a.stride_t = stride_t; a.V = V; a.video_index = video_index;
  a.W = in_proj_w; a.bias = in_proj_b; a.pe = enc_t_pe; a.cls = cls; a.x = x;
  a.B = B; a.T = T; a.N = N; a.C = C;
  a.rows = (long long)B * T * N;
  SF_REQUIRE((a.rows + PH_ROWS - 1) / PH_ROWS + (B + PH_CLS_PER_WG - 1) / PH_CLS_PER_WG < (1LL << 31), "sf_phyre_readout_fwd_f32: batch too large for one launch");
  a.ntiles = (int)((a.rows + PH_ROWS - 1) / PH_ROWS);
  const size_t lds = ph_embed_lds(C);
  SF_TRY(sf_ensure_dyn_lds((const void*)ph_embed_kernel, lds));
  SF_TRY(sf_ensure_dyn_lds((const void*)ph_head_kernel, PH_HEAD_LDS));
  hipLaunchKernelGGL(ph_embed_kernel, dim3((unsigned)(a.ntiles + (B + PH_CLS_PER_WG - 1) / PH_CLS_PER_WG)), dim3(PH_THREADS), lds, st, a, table);
  SF_CHECK_LAUNCH();
  SF_TRY(sf_layer_tok128_ex(x, layers, num_layers, 1e-5f, y, B, L, st));
  hipLaunchKernelGGL(ph_head_kernel, dim3((unsigned)((B + PH_HEAD_SEQ - 1) / PH_HEAD_SEQ)), dim3(PH_THREADS), PH_HEAD_LDS, st, y, L, mlp_w1, mlp_b1,
                     mlp_w2, mlp_b2, logits, conf, scatter_index, scatter_table, scatter_len, B);
  SF_CHECK_LAUNCH();
  return 0;
}

int sf_phyre_auccess_f32(const float* conf, const int* status, int* first_rank, int tasks, int actions, void* stream) {
  SF_REQUIRE(conf && status && first_rank, "sf_phyre_auccess_f32: null pointer");
  SF_REQUIRE(tasks >= 1 && actions >= 1, "sf_phyre_auccess_f32: tasks >= 1, actions >= 1");
  hipLaunchKernelGGL(ph_auccess_kernel, dim3((unsigned)tasks), dim3(PH_THREADS), 0, (hipStream_t)stream, conf, status, first_rank, actions);
  SF_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

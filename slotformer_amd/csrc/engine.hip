// Whole-path engines: SAVi/STEVE slot extraction and SlotFormer autoregressive rollout.
// Host-side C++ that sequences the HIP kernels on one stream (hipGraph-capturable: no
// allocation, no synchronisation, no host<->device copies).
//
//   sf_savi_encode_f32 : StoSAVi.encode / STEVE.encode  (savi.py:379-416, steve.py:198-240)
//   sf_rollout_f32     : SlotRollouter.forward / SingleStepSlotRollouter.forward
//                        (slotformer.py:85-126, single_step_slotformer.py:49-90)
//
// The encoder works one time step at a time (all B frames of step t): CNN -> per-pixel MLP ->
// K/V -> Slot-Attention iterations, so every intermediate of a step stays resident in the
// 256 MB Infinity Cache and memory is O(1) in T (the reference's OOM-probing temporal chunking,
// savi.py:431-463, is unnecessary; results are identical for any chunking).
// The rollout keeps all slots in one [B, T_total, N, C] buffer: the Transformer window of step
// s is a strided view of it (no torch.cat, slotformer.py:124), and predictions are written in
// place by the out_proj GEMM epilogue.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "sf_arena.h"
#include <map>
#include <vector>
#include "layer_fused.h"
#include "slot_chain.h"
#include <stdlib.h>

namespace {

// the per-call single-pass modes (sf_rollout_opts.precision 2 / 3): every contraction on the generic GEMM core, which honours them, none
// on the split-bf16-only fused kernels.  A process default of 2 (sf_set_precision, SF_PRECISION=bf16) keeps the fused kernels.
inline bool plain_gemms(const SfThreadOpts& o) { return o.precision == 2 || o.precision == 3; }

struct TfmWs {
  float *x2, *qkv, *att, *hid, *y;
};

bool tfm_ws_take(SfArena& bp, TfmWs& w, int M, int d, int ffn) {
  w.x2 = bp.take((size_t)M * d);
  w.qkv = bp.take((size_t)M * 3 * d);
  w.att = bp.take((size_t)M * d);
  w.hid = bp.take((size_t)M * ffn);
  w.y = bp.take((size_t)M * d);
  return bp.ok;
}

// One nn.TransformerEncoderLayer on x [B*L, d] (in place unless Lq < L).
// Lq < L (norm_first only): only the last Lq rows of every sequence are produced, into ws.y
// ([B*Lq, d]) -- used for the final layer of a rollout step, whose other rows are never read
// (slotformer.py:121).  Returns the output pointer through *out.
// xp / counters non-NULL (pre-LN, d = 256, ffn = 1024, packed FFN weights): the FFN half runs as ONE launch of the fused kernel
// of layer_fused.hip on the finished attention rows (xp [4][B*Lq][d] chunk-partial scratch, counters zeroed by the caller).
int tfm_layer(const sf_tfm_layer& w, float* x, TfmWs& ws, int B, int L, int Lq, int d, int heads, int ffn,
              int norm_first, hipStream_t st, float** out, float* xp = nullptr, int* counters = nullptr) {
  const int M = B * L, Mq = B * Lq;
  const float eps = 1e-5f;
  const SfRowMap rd = sf_rows(d);
  if (norm_first) {
    // split-bf16 mode: LN1 + per-head q|k|v projection + attention in one launch (attn_fused.hip)
    int fused = 1;
    if (sf_get_precision() >= 1 && !plain_gemms(sf_thread_opts()))
      fused = sf_qkv_attn_ex(x, w.norm1_g, w.norm1_b, eps, w.in_proj_w, w.in_proj_b, ws.att, B, L, Lq, d, heads, st);
    if (fused < 0 || fused > 1) return fused;
    if (fused == 1) {
      SF_TRY(sf_linear_ex(x, rd, w.in_proj_w, w.in_proj_b, w.norm1_g, w.norm1_b, eps, nullptr, rd, 0, ws.qkv,
                          sf_rows(3 * d), M, 3 * d, d, 0, st));
      SF_TRY(sf_mha_ex(ws.qkv, ws.att, B, L, Lq, d, heads, st));
    }
    // residual rows: last Lq rows of each sequence of x
    const SfRowMap xr = (Lq == L) ? rd : sf_rows_batched(d, Lq, (long long)L * d, (long long)(L - Lq) * d);
    SF_TRY(sf_linear_ex(ws.att, rd, w.out_proj_w, w.out_proj_b, nullptr, nullptr, eps, x, xr, 0, ws.x2, rd, Mq,
                        d, d, 0, st));
    float* dst = (Lq == L) ? x : ws.y;
    if (xp && counters) {
      SF_TRY(sf_ffn_partial_ex(ws.x2, (long long)Mq * d, w, eps, xp, (long long)Mq * d, dst, counters, Mq, ffn, st, 1));
    } else {
      SF_TRY(sf_linear_ex(ws.x2, rd, w.lin1_w, w.lin1_b, w.norm2_g, w.norm2_b, eps, nullptr, rd, 0, ws.hid,
                          sf_rows(ffn), Mq, ffn, d, 1, st));
      SF_TRY(sf_linear_ex(ws.hid, sf_rows(ffn), w.lin2_w, w.lin2_b, nullptr, nullptr, eps, ws.x2, rd, 0, dst, rd,
                          Mq, d, ffn, 0, st));
    }
    *out = dst;
  } else {
    if (Lq != L) return sf_set_err(-1, "row pruning requires norm_first", __FILE__, __LINE__);
    int fused = 1;
    if (sf_get_precision() >= 1 && !plain_gemms(sf_thread_opts()))
      fused = sf_qkv_attn_ex(x, nullptr, nullptr, eps, w.in_proj_w, w.in_proj_b, ws.att, B, L, L, d, heads, st);
    if (fused < 0 || fused > 1) return fused;
    if (fused == 1) {
      SF_TRY(sf_linear_ex(x, rd, w.in_proj_w, w.in_proj_b, nullptr, nullptr, eps, nullptr, rd, 0, ws.qkv,
                          sf_rows(3 * d), M, 3 * d, d, 0, st));
      SF_TRY(sf_mha_ex(ws.qkv, ws.att, B, L, L, d, heads, st));
    }
    SF_TRY(sf_linear_ex(ws.att, rd, w.out_proj_w, w.out_proj_b, nullptr, nullptr, eps, x, rd, 0, ws.y, rd, M, d,
                        d, 0, st));
    SF_TRY(sf_layernorm_ex(ws.y, rd, w.norm1_g, w.norm1_b, ws.x2, rd, M, d, eps, st));
    SF_TRY(sf_linear_ex(ws.x2, rd, w.lin1_w, w.lin1_b, nullptr, nullptr, eps, nullptr, rd, 0, ws.hid,
                        sf_rows(ffn), M, ffn, d, 1, st));
    SF_TRY(sf_linear_ex(ws.hid, sf_rows(ffn), w.lin2_w, w.lin2_b, nullptr, nullptr, eps, ws.x2, rd, 0, ws.y, rd,
                        M, d, ffn, 0, st));
    SF_TRY(sf_layernorm_ex(ws.y, rd, w.norm2_g, w.norm2_b, x, rd, M, d, eps, st));
    *out = x;
  }
  return 0;
}

int check_layers(const sf_tfm_layer* l, int n) {
  if (n > 0 && !l) return -1;
  for (int i = 0; i < n; ++i) {
    const sf_tfm_layer& w = l[i];
    if (!w.norm1_g || !w.norm1_b || !w.in_proj_w || !w.in_proj_b || !w.out_proj_w || !w.out_proj_b ||
        !w.norm2_g || !w.norm2_b || !w.lin1_w || !w.lin1_b || !w.lin2_w || !w.lin2_b)
      return -1;
  }
  return 0;
}

// frames of the Transformer window of rollout step s (nf) and the first of them (f0)
void step_window(const sf_rollouter* m, int s, int& nf, int& f0) {
  nf = (m->single_step && s + 1 < m->window_len) ? s + 1 : m->window_len;
  f0 = m->single_step ? s + 1 - nf : s;
}

// How sf_rollout_f32 runs a model, chosen once per call from its shape, which packed weight copies it has (their presence only: no
// weight is read, so a plan is made without a GPU), the process defaults and the call's options
struct RolloutPlan {
  // GENERIC: GEMM-core layers (tfm_layer); at d_model 128 / 8 heads / ffn 512 with layer_tok on, the layers before the last as token-stationary
  // launches (layer_tok128.hip) on x = in_proj(window) + PE, the row-pruned last layer still tfm_layer.  LONG_WINDOW (65..128 tokens): tfm_layer on LN1 + q|k|v + attention in one launch
  // (attn_fused.hip), the out-projection GEMM and the fused FFN kernel.  FUSED_*: the two-launch layers of layer_fused.hip on
  // x = in_proj(window) + PE (ROWS), or on the ring of cached in-projections with one launch per step boundary (RING)
  enum Path { GENERIC, LONG_WINDOW, FUSED_ROWS, FUSED_RING } path = GENERIC;
  int tok_layers = 0;   // leading layers run as token-stationary launches (layer_tok.hip, up to eight per launch): 0 or num_layers - 1
  // fused paths, the attention block: head-pair partials (four, summed by the FFN) / one workgroup per video running all 8 heads /
  // q|k|v on 128-row tiles + one core workgroup per video (attn_rows.hip); the last two write finished rows
  enum Attn { HEAD_PAIRS, ALL_HEADS, ROW_TILES } attn = HEAD_PAIRS;
  // ... the FFN block of the layers before the last: four chunk partials the next attention sums / one workgroup per 64-row tile
  // (ffn_tile.hip) / that tile launch fused with LN1 + q|k|v of the next layer (whose attention is then its core launch alone)
  enum Ffn { CHUNK_PARTS, TILE, TILE_QKV } ffn = CHUNK_PARTS;
  // FUSED_RING: the last-layer FFN + boundary of step s and the layer-0 attention of step s + 1 in one grid, on the steps whose next
  // window sf_seam_window_ok allows.  Every workgroup of it must be co-resident, one per CU: 160 fit the whole chip with room for
  // neighbours, a CU-masked caller says how many CUs it has (sf_rollout_opts.cus_available)
  bool seam = false;
  bool fused() const { return path == FUSED_ROWS || path == FUSED_RING; }
};

RolloutPlan plan_rollout(const sf_rollouter* m, int B, const SfThreadOpts& o) {
  RolloutPlan p;
  if (!m || !m->layers) return p;
  const int N = m->num_slots, W = m->window_len, Lmax = W * N, nl = m->num_layers, d = m->d_model;
  bool packed = true, tok_packed = nl >= 2;
  for (int l = 0; l < nl; ++l) {
    const sf_tfm_layer& w = m->layers[l];
    packed = packed && w.lin1_packed && w.lin2_packed && w.attn_in_packed && w.attn_out_packed;
    if (l + 1 < nl) tok_packed = tok_packed && w.tok_packed;
  }
  const int precision = sf_precision(o);
  const bool fusable = packed && !plain_gemms(o) && precision >= 1 && m->norm_first;
  const bool tok_on = tok_packed && sf_layer_tok_on(o);
  if (fusable && sf_layer_fused_ok(d, m->num_heads, m->ffn_dim, Lmax)) {
    p.path = (m->in_proj_packed && m->out_proj_packed && sf_step_boundary_ok(d, m->slot_size)) ? RolloutPlan::FUSED_RING
                                                                                               : RolloutPlan::FUSED_ROWS;
    bool tok = tok_on;
    for (int nf = m->single_step ? 1 : W; nf <= W && tok; ++nf) tok = sf_layer_tok_ok(nf * N);
    p.tok_layers = tok ? nl - 1 : 0;
    // the last layer behind token-stationary launches (finished rows, row-pruned) runs in the row-tile forms
    p.attn = (o.attn_rows == 128 || tok) ? RolloutPlan::ROW_TILES : (o.attn_heads == 8 ? RolloutPlan::ALL_HEADS : RolloutPlan::HEAD_PAIRS);
    if (p.attn != RolloutPlan::HEAD_PAIRS && o.ffn_tile >= 1)
      p.ffn = (p.attn == RolloutPlan::ROW_TILES && o.ffn_tile == 2) ? RolloutPlan::TILE_QKV : RolloutPlan::TILE;
    const int cus = o.cus > 0 && o.cus < 160 ? o.cus : 160;
    p.seam = p.path == RolloutPlan::FUSED_RING && p.attn == RolloutPlan::HEAD_PAIRS &&
             sf_seam_on(o) && sf_seam_blocks(B, N) <= cus;
  } else if (fusable && sf_layer_fused_ok(d, m->num_heads, m->ffn_dim, 1) && Lmax > 64 && sf_ffn_tiles(B * Lmax) <= 1024) {
    p.path = RolloutPlan::LONG_WINDOW;
    if (tok_on && Lmax <= 96 && !m->single_step && sf_layer_tok_ok(Lmax)) p.tok_layers = nl - 1;   // one video per workgroup
  } else if (tok_on && !plain_gemms(o) && precision >= 1 && m->norm_first && sf_layer_tok128_shape(d, m->num_heads, m->ffn_dim) && !m->single_step &&
             sf_layer_tok_ok(Lmax)) {
    // the OBJ3D Transformer: the sliding window has one size (the single-step rollouter has no configuration of this shape and is not taken)
    p.tok_layers = nl - 1;
  }
  return p;
}

// The rollout workspace: one fixed layout for every plan, M = B * window_len * num_slots rows
struct RolloutWs {
  float* x;        // [M][d]: in_proj(window) + PE
  TfmWs tw;        // tfm_layer scratch
  float* apb;      // attention output [8][M][d]: two sets of four head-pair partials (a seam or a parked q|k|v writes the second)
  float* xpb;      // FFN hidden-chunk partials [4][M][d]
  float *xa, *xb2; // layer outputs, alternating
  int* counters;   // tile counters of the FFN launches (1024)
  unsigned* seam_flags;   // per-tile epochs of the seam launches + an error word (1024)
  float* ring;     // cached in-projections [B][window_len + 1][N][d]
  float* planes;   // q / k / v^T fragment planes of the row-tile attention form (sf_attn_rows_plane_bytes)
};

bool rollout_ws_take(SfArena& bp, RolloutWs& w, const sf_rollouter* m, int B) {
  const size_t M = (size_t)B * m->window_len * m->num_slots, d = m->d_model;
  w.x = bp.take(M * d);
  tfm_ws_take(bp, w.tw, (int)M, (int)d, m->ffn_dim);
  w.apb = bp.take(8 * M * d);
  w.xpb = bp.take(4 * M * d);
  w.xa = bp.take(M * d);
  w.xb2 = bp.take(M * d);
  w.counters = (int*)bp.take(1024);
  w.seam_flags = (unsigned*)bp.take(1024);
  w.ring = bp.take((size_t)B * (m->window_len + 1) * m->num_slots * d);
  w.planes = bp.take(sf_attn_rows_plane_bytes(B) / 4);
  return bp.ok;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
size_t sf_rollout_workspace_bytes(const sf_rollouter* m, int B) {
  if (!m || B <= 0) return 0;
  SfArena bp(nullptr);
  RolloutWs w;
  rollout_ws_take(bp, w, m, B);
  return bp.bytes();
}

// a[0..n) = b[0..n) = 0 (n a multiple of 4, both 16-byte aligned)
// One wave kept busy for a given time (wall_clock64: the constant 100 MHz counter).  The pipeline launches two of them on two streams to
// find out whether the streams share a hardware queue (then they run one after the other): pipeline.py _pick_free_streams.
__global__ void spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
extern "C" int sf_debug_spin(int us, void* stream) {
  SF_REQUIRE(us > 0 && us <= 100000, "sf_debug_spin: 1..100000 microseconds");
  hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)us * 100);
  SF_CHECK_LAUNCH();
  return 0;
}

// One wave that measures the shader clock: s_memtime (shader cycles) against the constant 100 MHz counter over `ticks` of the latter; out[0] = cycles,
// out[1] = 10 ns ticks.  tools/clock_probe.py launches it on an idle stream while the pipeline runs: the clock the chip sustains under that load.
__global__ void clock_probe_kernel(long long ticks, long long* out) {
  const long long w0 = wall_clock64(), c0 = __builtin_readcyclecounter();
  long long w1 = w0;
  while (w1 - w0 < ticks) {
    __builtin_amdgcn_s_sleep(8);
    w1 = wall_clock64();
  }
  const long long c1 = __builtin_readcyclecounter();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = w1 - w0;
  }
}
extern "C" int sf_debug_clock_probe(int us, long long* out2, void* stream) {
  SF_REQUIRE(us > 0 && us <= 100000 && out2, "sf_debug_clock_probe: 1..100000 microseconds, a device buffer of two int64");
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)us * 100, out2);
  SF_CHECK_LAUNCH();
  return 0;
}

// clears a[0..n) and b[0..n): float4 stores where both pointers are 16-byte aligned and four elements remain, scalars otherwise
// (launch with ceil(n / 4) threads)
__global__ void zero_f32_kernel(float* a, float* b, long long n) {
  const long long i = 4 * ((long long)blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const bool vec = i + 4 <= n && ((((unsigned long long)(a + i)) | ((unsigned long long)(b + i))) & 15ull) == 0;
  if (vec) {
    *(float4*)(a + i) = float4{0.f, 0.f, 0.f, 0.f};
    *(float4*)(b + i) = float4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (long long j = i; j < n && j < i + 4; ++j) {
      a[j] = 0.f;
      b[j] = 0.f;
    }
  }
}

// block 0 clears a[0..1023], block 1 clears b[0..1023] (b may be NULL)
__global__ void zero_words_kernel(unsigned* a, unsigned* b) {
  unsigned* p = blockIdx.x == 0 ? a : b;
  if (p) p[threadIdx.x] = 0u;
}

// float4 i of the staged window [B][nf * N][C] of virtual videos v = b * f + p: frame j of v is frame (f0 + j) * f + p of video b
// (fe = N * C elements per frame, a multiple of 4; n4 float4 in all)
__global__ void gather_phase_window_kernel(const float* __restrict__ slots, long long bs, int f, long long fe, int f0, int nf,
                                           float* __restrict__ dst, long long n4) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const long long e = 4 * i, pv = (long long)nf * fe, v = e / pv, r = e - v * pv, j = r / fe, o = r - j * fe;
  const long long b = v / f, p = v - b * f;
  *(float4*)(dst + e) = *(const float4*)(slots + b * bs + ((f0 + j) * f + p) * fe + o);
}

}  // extern "C"

namespace {
// The rollout of sf_rollout_f32 (f == 1, first == 0) and of sf_rollout_phases_f32 on B * f VIRTUAL videos v = b * f + p, phase p of
// video b: frame u of v is frame first + u * f + p of video b.  The burn-in is frames 0 .. n_in-1 of every virtual video, step s
// writes its frame n_in + s.  Everything between the in-projection and the out-projection -- the plan, the workspace, every layer
// launch -- sees B * f videos and nothing else; `slots` is touched by the step boundary / ring initialisation (layer_fused.hip: the
// frames the f phases of a video write in one step are consecutive, one group of f * N rows) and by the two row maps of the paths
// without a ring.  Of those the out-projection's is the same group of f * N rows; the window's rows lie f frames apart, which a row
// map cannot say, so for f > 1 the window is staged into contiguous rows first (one small copy launch per step, into workspace the
// path leaves idle) -- the row map, and with it every GEMM kernel of the library, stays as it is.
int rollout_run(const sf_rollouter* m, float* slots, int Bvid, int T_total, int first, int f, int pred_len, void* ws,
                size_t ws_bytes, void* stream) {
  SF_REQUIRE(m && slots && ws, "null pointer");
  SF_REQUIRE(Bvid >= 1 && pred_len >= 0 && f >= 1 && first >= 0, "bad batch / pred_len");
  SF_REQUIRE(m->num_slots >= 1 && m->slot_size > 0 && (m->slot_size % 4) == 0 && m->d_model > 0 &&
                 (m->d_model % 4) == 0 && m->ffn_dim > 0 && (m->ffn_dim % 4) == 0 && m->num_layers >= 1 &&
                 m->window_len >= 1, "bad rollouter shape");
  SF_REQUIRE(m->in_proj_w && m->in_proj_b && m->out_proj_w && m->out_proj_b && m->pe_tok, "null weight");
  SF_REQUIRE(check_layers(m->layers, m->num_layers) == 0, "null transformer-layer weight");
  const int n_in = m->single_step ? 1 : m->window_len;
  SF_REQUIRE(!(m->single_step && f > 1), "sf_rollout_phases_f32: a single-step rollouter takes frame_offset 1 only");
  SF_REQUIRE((long long)T_total >= first + (long long)(n_in + pred_len) * f, "slots buffer shorter than burn-in + pred_len");
  SF_REQUIRE((long long)Bvid * f <= 0x7fffffffLL / ((long long)m->window_len * m->num_slots), "batch too large");
  const int B = Bvid * f;   // virtual videos
  SF_REQUIRE(ws_bytes >= sf_rollout_workspace_bytes(m, B), "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int N = m->num_slots, C = m->slot_size, d = m->d_model, W = m->window_len, nl = m->num_layers;
  const float eps = 1e-5f;
  SfArena bp(ws, ws_bytes);
  RolloutWs w;
  if (!rollout_ws_take(bp, w, m, B)) return sf_set_err(-1, "workspace too small", __FILE__, __LINE__);
  const RolloutPlan p = plan_rollout(m, B, sf_thread_opts());
  const bool ring_in = p.path == RolloutPlan::FUSED_RING;   // layer 0 reads the projection ring + PE, not x = in_proj(window) + PE
  const bool long_ffn = p.path == RolloutPlan::LONG_WINDOW;
  const int np = p.attn == RolloutPlan::HEAD_PAIRS ? 4 : 1;   // attention partials the FFN sums
  const int RF = W + 1;   // frames in the projection ring: the window being read + the frame being written
  const long long bs = (long long)T_total * N * C;
  slots += (long long)first * N * C;   // frame 0 of the virtual videos
  // f > 1 without a ring: where the window is staged -- the attention partials on the paths that run no fused layer, else the ring
  float* stage = nullptr;
  if (f > 1 && !ring_in) {
    const bool in_apb = !p.fused();
    stage = in_apb ? w.apb : w.ring;
    SF_REQUIRE(in_apb ? C <= 8 * d : (long long)W * C <= (long long)(W + 1) * d,
               "sf_rollout_phases_f32: slot_size too wide for this model's idle workspace (the staged window)");
  }
  if (ring_in) {
    // in-projection (without PE) of the burn-in frames -> ring slots 0 .. n_in-1
    SF_TRY(sf_ring_init_ex(m->out_proj_packed, m->out_proj_b, m->in_proj_packed, m->in_proj_b, slots, bs, n_in, w.ring, RF, N, B, st, f));
  }
  if (p.fused() || long_ffn) {
    SF_REQUIRE(sf_ffn_tiles(B * W * N) <= 1024, "batch too large for the fused-layer tile counters");
    // zeroed by a KERNEL, not hipMemsetAsync: the rollout is captured into hipGraphs, and the memset nodes of a graph were seen
    // to stop clearing these words after an OLDER graph exec had been destroyed (stale seam epochs -> consumers read ring rows
    // before they were written; found by tests/test_pipeline_gpu.py when a second pipeline followed a first in one process)
    hipLaunchKernelGGL(zero_words_kernel, dim3(2), dim3(1024), 0, st, (unsigned*)w.counters, p.seam ? w.seam_flags : nullptr);
    SF_CHECK_LAUNCH();
    if (p.attn == RolloutPlan::ROW_TILES) {
      // key positions >= L of the v^T planes meet probability 0 in the PV product: they must hold finite values
      const long long nfl = (long long)(sf_attn_rows_plane_bytes(B) / 4), half = nfl / 2;
      hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)(((half + 3) / 4 + 255) / 256)), dim3(256), 0, st, w.planes, w.planes + half, half);
      SF_CHECK_LAUNCH();
    }
  }
  float* apb2 = w.apb + (size_t)4 * B * W * N * d;   // second set of head-pair partials
  float* ap0 = w.apb;        // where the layer-0 attention of the current step put its partials
  bool attn0_done = false;   // ... and whether it already ran (inside the previous step's seam launch)
  for (int s = 0; s < pred_len; ++s) {
    int nf, f0;
    step_window(m, s, nf, f0);
    const int L = nf * N, pe_off = (W - nf) * N;
    const float* pe = m->pe_tok + (long long)pe_off * d;
    float* cin = nullptr;   // the current layer's input rows (NULL: the ring, four chunk partials in xpb or rows parked with the planes)
    if (!ring_in) {
      // x = in_proj(window) + pe   (slotformer.py:115-117; single_step_slotformer.py:79-81)
      SfRowMap pmap = sf_rows(d);
      pmap.base = (long long)pe_off * d;
      if (stage) {
        const long long n4 = (long long)B * L * C / 4;
        hipLaunchKernelGGL(gather_phase_window_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, slots, bs, f, (long long)N * C, f0, nf,
                           stage, n4);
        SF_CHECK_LAUNCH();
      }
      SF_TRY(sf_linear_ex(stage ? stage : slots, stage ? sf_rows(C) : sf_rows_batched(C, L, bs, (long long)f0 * N * C), m->in_proj_w, m->in_proj_b,
                          nullptr, nullptr, 0.f, m->pe_tok, pmap, L, w.x, sf_rows(d), B * L, d, C, 0, st));
      cin = w.x;
    }
    // the leading layers as token-stationary launches of up to eight layers each (the rows stay in registers between them)
    int l = 0;
    while (l < p.tok_layers) {
      const int nlt = (p.tok_layers - l) < 8 ? (p.tok_layers - l) : 8;
      float* xo = (cin == w.xa) ? w.xb2 : w.xa;
      if (ring_in)
        SF_TRY(sf_layer_tok_ex(l == 0 ? 1 : 0, cin, w.ring, RF, N, f0, pe, m->layers + l, nlt, eps, xo, B, L, st));
      else if (sf_layer_tok128_shape(d, m->num_heads, m->ffn_dim))   // (the kernel follows the MODEL's shape: its tok_packed blobs are that shape's)
        SF_TRY(sf_layer_tok128_ex(cin, m->layers + l, nlt, eps, xo, B, L, st));
      else
        SF_TRY(sf_layer_tok_ex(0, cin, nullptr, 1, 1, 0, nullptr, m->layers + l, nlt, eps, xo, B, L, st));
      cin = xo;
      l += nlt;
    }
    if (!p.fused()) {
      int Lc = L;
      for (; l < nl; ++l) {
        const int Lq = (l == nl - 1 && m->norm_first) ? N : Lc;
        SF_TRY(tfm_layer(m->layers[l], cin, w.tw, B, Lc, Lq, d, m->num_heads, m->ffn_dim, m->norm_first, st, &cin,
                         long_ffn ? w.xpb : nullptr, long_ffn ? w.counters : nullptr));
        Lc = Lq;
      }
      // pred = out_proj(x[:, -N:]) written straight into frame n_in + s   (slotformer.py:121-124): the f phases of a video write f
      // consecutive frames, f * N rows
      const SfRowMap lastmap = (Lc == N) ? sf_rows(d) : sf_rows_batched(d, N, (long long)Lc * d, (long long)(Lc - N) * d);
      SF_TRY(sf_linear_ex(cin, lastmap, m->out_proj_w, m->out_proj_b, nullptr, nullptr, 0.f, nullptr, sf_rows(C), 0,
                          slots, sf_rows_batched(C, f * N, bs, (long long)(n_in + s) * f * N * C), B * N, C, d, 0, st));
      continue;
    }
    // every other layer is two launches: the attention block, then the FFN block (which also finishes the sums)
    bool parts_in = false;     // the current layer's input is the previous layer's four FFN chunk partials in xpb
    float* parked = nullptr;   // TILE_QKV: where the previous layer's launch parked this layer's residual rows (planes written)
    for (; l < nl; ++l) {
      const sf_tfm_layer& lw = m->layers[l];
      const bool lastl = (l == nl - 1);
      const int Lq = lastl ? N : L;   // last layer: only the newest frame's rows are read (slotformer.py:121)
      const long long pst = (long long)B * Lq * d;
      float* xo = (cin == w.xa) ? w.xb2 : w.xa;
      float* ap = (l == 0) ? ap0 : w.apb;   // the attention block's output
      if (parked) {
        ap = parked;
        SF_TRY(sf_attn_core_ex(lw, ap, w.planes, B, L, Lq, st));
      } else if (p.attn == RolloutPlan::ROW_TILES) {
        if (l == 0 && ring_in)
          SF_TRY(sf_attn_rows_ex(2, w.ring, (long long)RF * N * d, 0, pe, f0, RF, N, lw, eps, ap, w.planes, B, L, Lq, st));
        else if (parts_in)
          SF_TRY(sf_attn_rows_ex(1, w.xpb, (long long)L * d, (long long)B * L * d, nullptr, 0, 1, 1, lw, eps, ap, w.planes, B, L, Lq, st));
        else
          SF_TRY(sf_attn_rows_ex(0, cin, (long long)L * d, 0, nullptr, 0, 1, 1, lw, eps, ap, w.planes, B, L, Lq, st));
      } else if (p.attn == RolloutPlan::ALL_HEADS) {
        if (l == 0 && ring_in)
          SF_TRY(sf_attn_all_ring_ex(w.ring, RF, N, f0, pe, lw, eps, ap, B, L, Lq, st));
        else if (parts_in)
          SF_TRY(sf_attn_all_parts_ex(w.xpb, (long long)B * L * d, lw, eps, ap, B, L, Lq, st));
        else
          SF_TRY(sf_attn_all_ex(cin, lw, eps, ap, B, L, Lq, st));
      } else if (l == 0 && ring_in) {
        if (!attn0_done) SF_TRY(sf_attn_oproj_ring_ex(w.ring, RF, N, f0, pe, lw, eps, ap, pst, B, L, Lq, st));
      } else if (parts_in) {
        SF_TRY(sf_attn_oproj_parts_ex(w.xpb, (long long)B * L * d, lw, eps, ap, pst, B, L, Lq, st));
      } else {
        SF_TRY(sf_attn_oproj_ex(cin, lw, eps, ap, pst, B, L, Lq, st));
      }
      if (!lastl) {
        if (p.ffn == RolloutPlan::TILE_QKV) {
          float* park = (ap == w.apb) ? apb2 : w.apb;
          SF_TRY(sf_ffn_qkv_tile_ex(ap, lw, m->layers[l + 1], eps, park, w.planes, B, L, (l + 1 == nl - 1) ? N : L, m->ffn_dim, st));
          parked = park;
          cin = nullptr;
        } else if (p.ffn == RolloutPlan::TILE) {
          SF_TRY(sf_ffn_tile_ex(ap, lw, eps, xo, B * Lq, m->ffn_dim, st));
          cin = xo;
        } else {
          // the chunk partials are the layer output: the next attention sums them
          SF_TRY(sf_ffn_parts_ex(ap, pst, lw, eps, w.xpb, pst, B * Lq, m->ffn_dim, st, np));
          cin = nullptr;
        }
        parts_in = p.ffn == RolloutPlan::CHUNK_PARTS;
      } else if (ring_in) {
        // last layer: FFN + step boundary in one launch.  pred = out_proj(last rows) -> frame n_in + s; its
        // in-projection -> the ring   (slotformer.py:121-124, :115)
        int nf1 = 0, f01 = 0;
        if (s + 1 < pred_len) step_window(m, s + 1, nf1, f01);
        if (p.seam && s + 1 < pred_len && sf_seam_window_ok(nf1 * N, N)) {
          // ... and the layer-0 attention of step s + 1 in the same grid
          const int L1 = nf1 * N, Lq1 = (nl == 1) ? N : L1;
          float* ap_next = (ap == w.apb) ? apb2 : w.apb;
          SF_TRY(sf_seam_ex(ap, pst, lw, eps, w.xpb, pst, w.counters, m->ffn_dim, m->out_proj_packed, m->out_proj_b,
                            m->in_proj_packed, m->in_proj_b, slots, bs, n_in + s, w.ring, RF, N, B, m->layers[0], f01,
                            m->pe_tok + (long long)((W - nf1) * N) * d, ap_next, (long long)B * Lq1 * d, L1, Lq1, w.seam_flags,
                            (unsigned)(s + 1), st, f));
          ap0 = ap_next;
          attn0_done = true;
        } else {
          SF_TRY(sf_ffn_boundary_ex(ap, pst, lw, eps, w.xpb, pst, w.counters, m->ffn_dim, m->out_proj_packed, m->out_proj_b,
                                    m->in_proj_packed, m->in_proj_b, slots, bs, n_in + s, w.ring, RF, N, B, st, np, f));
          ap0 = w.apb;
          attn0_done = false;
        }
      } else {
        // last layer: FFN into finished rows, then pred = out_proj(them) written straight into frame n_in + s
        SF_TRY(sf_ffn_partial_ex(ap, pst, lw, eps, w.xpb, pst, xo, w.counters, B * Lq, m->ffn_dim, st, np));
        SF_TRY(sf_linear_ex(xo, sf_rows(d), m->out_proj_w, m->out_proj_b, nullptr, nullptr, 0.f, nullptr, sf_rows(C), 0,
                            slots, sf_rows_batched(C, f * N, bs, (long long)(n_in + s) * f * N * C), B * N, C, d, 0, st));
      }
    }
  }
  return 0;
}
}  // namespace

extern "C" {

int sf_rollout_f32(const sf_rollouter* m, float* slots, int B, int T_total, int pred_len, void* ws,
                   size_t ws_bytes, void* stream) {
  return rollout_run(m, slots, B, T_total, 0, 1, pred_len, ws, ws_bytes, stream);
}

namespace {
// the calling thread's options for the duration of one engine call
struct OptsScope {
  SfThreadOpts saved;
  explicit OptsScope(const SfThreadOpts& o) : saved(sf_thread_opts()) { sf_thread_opts() = o; }
  ~OptsScope() { sf_thread_opts() = saved; }
};

// the thread options a rollout with per-call options `opts` runs under (NULL: the calling thread's own)
SfThreadOpts rollout_thread_opts(const sf_rollout_opts* opts) {
  SfThreadOpts o = sf_thread_opts();
  if (!opts) return o;
  if (opts->precision >= 0) o.precision = opts->precision;
  if (opts->seam_fused >= 0) o.seam = opts->seam_fused ? 1 : 0;
  if (opts->ffn_rows > 0) o.ffn_rows = opts->ffn_rows;
  if (opts->attn_heads_per_wg > 0) o.attn_heads = opts->attn_heads_per_wg;
  if (opts->attn_qkv_rows > 0) o.attn_rows = opts->attn_qkv_rows;
  if (opts->ffn_tile > 0) o.ffn_tile = opts->ffn_tile;
  if (opts->cus_available > 0) o.cus = opts->cus_available;
  if (opts->layer_tok != 0) o.layer_tok = opts->layer_tok > 0 ? 1 : -1;
  return o;
}

int check_rollout_opts(const sf_rollout_opts* opts) {
  SF_REQUIRE(opts->precision >= -1 && opts->precision <= 3, "sf_rollout_opts: precision must be -1 (default), 0, 1, 2 or 3");
  SF_REQUIRE(opts->ffn_rows == 0 || opts->ffn_rows == 32 || opts->ffn_rows == 64 || opts->ffn_rows == 128,
             "sf_rollout_opts: ffn_rows must be 0 (default), 32, 64 or 128");
  SF_REQUIRE(opts->attn_heads_per_wg == 0 || opts->attn_heads_per_wg == 2 || opts->attn_heads_per_wg == 8,
             "sf_rollout_opts: attn_heads_per_wg must be 0 (default), 2 or 8");
  SF_REQUIRE(opts->attn_qkv_rows == 0 || opts->attn_qkv_rows == 128, "sf_rollout_opts: attn_qkv_rows must be 0 (off) or 128");
  SF_REQUIRE(opts->ffn_tile >= 0 && opts->ffn_tile <= 2, "sf_rollout_opts: ffn_tile must be 0, 1 or 2");
  SF_REQUIRE(opts->cus_available >= 0 && opts->cus_available <= 256, "sf_rollout_opts: cus_available must be 0 (whole chip) .. 256");
  return 0;
}
}  // namespace

// sf_rollout_f32 with per-call options (include/slotformer_hip.h, sf_rollout_opts): arithmetic mode, seam launches, rows
// per FFN workgroup, videos per attention workgroup.  The options live in thread-local state for the duration of the call,
// so concurrent calls from other host threads (one per GPU in the reference's drivers, extract_slots.py:128) keep theirs.
int sf_rollout_opts_f32(const sf_rollouter* m, float* slots, int B, int T_total, int pred_len, void* ws, size_t ws_bytes,
                        void* stream, const sf_rollout_opts* opts) {
  if (!opts) return sf_rollout_f32(m, slots, B, T_total, pred_len, ws, ws_bytes, stream);
  SF_TRY(check_rollout_opts(opts));
  OptsScope scope(rollout_thread_opts(opts));
  return sf_rollout_f32(m, slots, B, T_total, pred_len, ws, ws_bytes, stream);
}

// Every phase of a video rolled forward at a frame offset in ONE call (rollout_clevrer_slots.py:20-65, rollout_physion_slots.py:22-63, which
// call the model frame_offset times): phase p < f burns in on frames first + p + j * f (j < hist, first = obs - hist * f) and writes
// frame obs + p + s * f at step s < S = ceil(pred_len / f) -- as B * f virtual videos through the plan, the workspace and the
// launches of a rollout of that many videos (rollout_run)
size_t sf_rollout_phases_workspace_bytes(const sf_rollouter* m, int B, int frame_offset) {
  if (!m || B <= 0 || frame_offset <= 0 || (long long)B * frame_offset > 0x7fffffffLL) return 0;
  return sf_rollout_workspace_bytes(m, B * frame_offset);
}

int sf_rollout_phases_f32(const sf_rollouter* m, float* slots, int B, int T_total, int obs, int frame_offset, int pred_len, void* ws,
                          size_t ws_bytes, void* stream, const sf_rollout_opts* opts) {
  SF_REQUIRE(m && slots && ws, "null pointer");
  SF_REQUIRE(B >= 1 && pred_len >= 0, "bad batch / pred_len");
  SF_REQUIRE(frame_offset >= 1, "sf_rollout_phases_f32: frame_offset >= 1");
  SF_REQUIRE(!(m->single_step && frame_offset > 1), "sf_rollout_phases_f32: a single-step rollouter takes frame_offset 1 only");
  SF_REQUIRE(m->window_len >= 1, "bad rollouter shape");
  const int f = frame_offset, hist = m->single_step ? 1 : m->window_len;
  SF_REQUIRE((long long)obs >= (long long)hist * f, "sf_rollout_phases_f32: fewer observed frames than burn-in * frame_offset");
  const long long S = ((long long)pred_len + f - 1) / f;
  SF_REQUIRE((long long)T_total >= obs + S * f, "slots buffer shorter than obs + ceil(pred_len / frame_offset) * frame_offset");
  const int first = obs - hist * f;
  if (!opts) return rollout_run(m, slots, B, T_total, first, f, (int)S, ws, ws_bytes, stream);
  SF_TRY(check_rollout_opts(opts));
  OptsScope scope(rollout_thread_opts(opts));
  return rollout_run(m, slots, B, T_total, first, f, (int)S, ws, ws_bytes, stream);
}

// 1 when sf_rollout_f32 runs this model's layers as the two fused launches of layer_fused.hip (per-video / per-row kernels whose
// results do not depend on how videos are grouped into batches); 0: the generic GEMM path, whose tile / split-K choice -- and
// with it the summation order -- follows the batch size
int sf_rollout_is_fused(const sf_rollouter* m) { return plan_rollout(m, 1, sf_thread_opts()).fused(); }

// 1 when sf_rollout_f32 can run this model's layers before the last as token-stationary launches (sf_rollout_opts.layer_tok): the
// fused-layer path with layer_tok on takes them
int sf_rollout_tok_ok(const sf_rollouter* m) {
  SfThreadOpts o = sf_thread_opts();
  o.layer_tok = 1;
  const RolloutPlan p = plan_rollout(m, 1, o);
  return p.fused() && p.tok_layers > 0;
}

// How many leading layers sf_rollout_f32 with these options (NULL: the thread's defaults) runs as token-stationary launches, on whatever path: 0 or
// num_layers - 1
int sf_rollout_tok_layers(const sf_rollouter* m, int B, const sf_rollout_opts* opts) {
  if (B <= 0) return 0;
  return plan_rollout(m, B, rollout_thread_opts(opts)).tok_layers;
}

// 1 when sf_rollout_f32 with these options may launch seams for this model / batch (a caller that wants to verify
// sf_seam_timeouts() after the call only needs to when this is non-zero)
int sf_rollout_uses_seam_opts(const sf_rollouter* m, int B, const sf_rollout_opts* opts) {
  if (B <= 0 || !plan_rollout(m, B, rollout_thread_opts(opts)).seam) return 0;
  // the seam launch at the end of step s runs in the window of step s + 1
  for (int s = 1; s <= m->window_len; ++s) {
    int nf, f0;
    step_window(m, s, nf, f0);
    if (sf_seam_window_ok(nf * m->num_slots, m->num_slots)) return 1;
  }
  return 0;
}
int sf_rollout_uses_seam(const sf_rollouter* m, int B) { return sf_rollout_uses_seam_opts(m, B, nullptr); }

// SURVEY.md 8(b2) `sf_rollout_bf16`: the same rollout with every matrix product in SINGLE-PASS bf16 (operands rounded to
// 8 mantissa bits, f32 accumulation; f32 storage, LayerNorm, softmax) -- the arithmetic of the reference's `--fp16` AMP
// (scripts/train.py:84,105) and of BASELINE.json's literal "bf16".  Measured on the 6+50 path of config C2 against the
// reference fixture: ~8e-3 relative (tools/precision_probe.py, tests/test_engine_gpu.py), i.e. OUTSIDE the 1e-3 parity bar --
// which is why sf_rollout_f32 (split-bf16, 1e-5) is the default and the product path.  Same arguments as sf_rollout_f32.
int sf_rollout_bf16(const sf_rollouter* m, float* slots, int B, int T_total, int pred_len, void* ws, size_t ws_bytes,
                    void* stream) {
  sf_rollout_opts o = {2, -1, 0, 0};
  return sf_rollout_opts_f32(m, slots, B, T_total, pred_len, ws, ws_bytes, stream, &o);
}

// ---------------------------------------------------------------------------------------------
}  // extern "C"

// StoSAVi.encode / STEVE.encode
namespace {
int enc_chunk(int B) { return B < 32 ? B : 32; }
// the forked form keeps the Slot-Attention inputs of up to ENC_FORK_AHEAD time steps (the feature branch runs that far ahead of the slot branch)
constexpr int ENC_FORK_AHEAD = 4;
int enc_fork_steps(int T) { return T < 2 ? 2 : (T < ENC_FORK_AHEAD ? T : ENC_FORK_AHEAD); }
constexpr int ENC_HW = 64 * 64;   // pixels of the encoder's feature maps (savi.py:226)

// channels of the widest CNN layer output
int enc_cmax(const sf_savi_encoder* m) {
  int cmax = 0;
  for (int i = 1; i <= m->enc_layers && i < 9; ++i) cmax = m->enc_channels[i] > cmax ? m->enc_channels[i] : cmax;
  return cmax;
}
// n CNN activation buffers of `frames` frames each
void enc_cnn_take(SfArena& bp, float** buf, int n, const sf_savi_encoder* m, size_t frames) {
  for (int i = 0; i < n; ++i) buf[i] = bp.take(frames * ENC_HW * enc_cmax(m));
}

// the slot branch's four [rows][D] buffers: ping-pong slots, the predictor's latents, q (the video-stationary launch's row buffers too)
struct SlotRows { float *a, *b, *lat, *q; };
void slot_rows_take(SfArena& bp, SlotRows& r, size_t rows, int D) {
  for (float** f : {&r.a, &r.b, &r.lat, &r.q}) *f = bp.take(rows * D);
}

// How sf_savi_encode_fork_f32 runs a call, chosen once from the encoder's shape, which weights and packed copies it has (their presence only: no
// weight is read, so a plan is made without a GPU), the process defaults and the size of the caller's workspace
struct EncodePlan {
  bool fork = false;   // two branches: the features on `stream`, the slot branch one step behind on `side_stream`
  int KV = 2;          // resident Slot-Attention inputs: a ring of KV time steps
  // the CNN features of step t: precomputed (t < n_pre), from the convolutions of all T steps as one launch per layer (batched), or per step
  int n_pre = 0;
  bool batched = false;
  // Slot-Attention inputs, which also fix the iteration's form.  KV_*: k|v rows of 2 D, by three GEMMs or sf_pixel_mlp_kv_ex where that applies.
  // FOLD_*: k / v folded into project_q and the GRU input matrix (include/slotformer_hip.h, sa_fold_*), keys == values = the normalised features
  // as f32 rows (192: the 192-wide chain as one launch) or as bf16 hi | lo rows of 512 B (sa_attn_planes_kernel)
  enum Feat { KV_GEMMS, KV_FUSED, FOLD_ROWS, FOLD_192, FOLD_PLANES } feat = KV_GEMMS;
  // project_q and GRU input weights of that form
  const float *q_w = nullptr, *q_w_t = nullptr, *gru_ih_t = nullptr;
  const void *q_w_p = nullptr, *gru_ih_p = nullptr;
  // slot update on the matrix cores from packed copies (slot size 128: slot_update_mfma.hip; 192: slot_update_wide.hip), else the VALU kernel.
  // p_step 2: the update reads every second partial record (the one-pass iteration kernels leave the others zero -- eight, one round of requests)
  enum Update { VALU, WIDE, MFMA } update = VALU;
  int p_step = 1;
  bool pred_step = false;     // the Transformer predictor (+ LSTM) tried as one launch (pred_step.hip)
  bool prologue = false;      // the one-launch slot prologue (CLEVRER configuration: residual-MLP predictor, one-Linear kernel distribution)
  bool fuse_next = false;     // ... of step t + 1 at the tail of step t's last slot update (slot_update_mfma.hip, NEXT form)
  bool chain_model = false;   // the model runs the video-stationary slot branch (slot_chain.hip)
  bool chain = false;         // ... and this call does: batched, sf_set_slot_chain(1), room for the feature planes
  bool fold() const { return feat >= FOLD_ROWS; }
};

// The encode workspace of a plan (over a NULL base: its size)
struct EncodeWs {
  float* feat[2];         // CNN activations of up to 32 frames, ping-pong
  float *h1, *h2;         // encoder_out_layer rows of the three-GEMM k|v
  float* kv;              // the Slot-Attention inputs of KV time steps, B * 64 * 64 * 2 D floats each
  SlotRows rows;
  float *lnbuf, *px;      // predictor rows
  float *kdist, *kdtmp;   // kernel distribution rows
  float *pnum, *pden;     // partial records of an iteration
  TfmWs tw;               // Transformer predictor
  float* gates;           // LSTM gates
  float* big[3];          // batched: CNN activations of all B * T frames
  float* planes;          // chain: their Slot-Attention inputs as bf16 hi | lo rows of 512 B
};

bool enc_ws_take(SfArena& bp, EncodeWs& w, const sf_savi_encoder* m, int B, int T, const EncodePlan& p) {
  const int N = m->num_slots, D = m->slot_size, Ce = m->enc_out_channels, P = sf_sa_pick_partials(ENC_HW);
  const size_t R = (size_t)B * N, Bc = enc_chunk(B), HW = ENC_HW;
  enc_cnn_take(bp, w.feat, 2, m, Bc);
  w.h1 = bp.take(Bc * HW * Ce);
  w.h2 = bp.take(Bc * HW * Ce);
  w.kv = bp.take((size_t)p.KV * B * HW * 2 * D);
  slot_rows_take(bp, w.rows, R, D);
  w.lnbuf = bp.take(R * D);
  w.px = bp.take(R * D);
  w.kdist = bp.take(R * 2 * D);
  w.kdtmp = bp.take(R * 2 * D);
  w.pnum = bp.take((size_t)B * P * N * D);
  w.pden = bp.take((size_t)B * P * N);
  tfm_ws_take(bp, w.tw, (int)R, D, m->pred_ffn_dim > 2 * D ? m->pred_ffn_dim : 2 * D);
  w.gates = bp.take(R * 4 * (m->pred_hidden > 0 ? m->pred_hidden : 1));
  if (p.batched) enc_cnn_take(bp, w.big, 3, m, (size_t)B * T);
  if (p.chain) w.planes = bp.take((size_t)B * T * HW * 128);
  return bp.ok;
}

size_t enc_ws_bytes(const sf_savi_encoder* m, int B, int T, const EncodePlan& p) {
  SfArena bp(nullptr);
  EncodeWs w;
  enc_ws_take(bp, w, m, B, T, p);
  return bp.bytes() + 8192;
}

bool enc_batched_ok(const sf_savi_encoder* m, int B, int T, int precision) {
  // (at most 384 frames per call: 1.2 GB of activations + 0.8 GB of feature rows; longer clips keep the per-step order)
  if (T < 2 || B > enc_chunk(B) || (long long)B * T > 384 || m->enc_layers < 2 || precision != 1) return false;
  for (int i = 1; i < m->enc_layers; ++i)
    if (!m->conv_w_frag[i] || m->enc_channels[i] != 64 || m->enc_channels[i + 1] != 64) return false;
  return true;
}

EncodePlan plan_encode(const sf_savi_encoder* m, int B, int T, int n_pre, bool fork, size_t ws_bytes) {
  EncodePlan p;
  p.fork = fork;
  p.KV = fork ? enc_fork_steps(T) : 2;
  p.n_pre = n_pre;
  if (!m || m->enc_layers < 1 || m->enc_layers > 8) return p;
  const int precision = sf_get_precision();
  const int HW = ENC_HW, N = m->num_slots, D = m->slot_size, Ce = m->enc_out_channels, Hm = m->slot_mlp_size, P = sf_sa_pick_partials(HW);
  const int Cl = m->enc_channels[m->enc_layers];
  const bool feat192 = Cl == 64 && Ce == 192 && m->enc_fc1_p && m->enc_fc2_p;
  const bool fold = precision >= 1 && m->sa_fold_q_w && m->sa_fold_q_w_t && m->sa_fold_gru_ih_t && Ce == D && (sf_pixel_mlp_feat_ok(Cl, Ce) || feat192);
  const bool planes = fold && !feat192 && sf_switch(SF_SW_SLOT_ATTN_PLANES) && sf_slot_attn_planes_ok(HW, D, N) && Cl == 64 && P == HW / 256;
  p.feat = fold ? (feat192 ? EncodePlan::FOLD_192 : planes ? EncodePlan::FOLD_PLANES : EncodePlan::FOLD_ROWS)
                : (precision >= 1 ? EncodePlan::KV_FUSED : EncodePlan::KV_GEMMS);
  p.q_w = fold ? m->sa_fold_q_w : m->sa_q_w;
  p.q_w_t = fold ? m->sa_fold_q_w_t : m->sa_q_w_t;
  p.gru_ih_t = fold ? m->sa_fold_gru_ih_t : m->gru_w_ih;
  p.q_w_p = fold ? m->sa_fold_q_w_p : m->sa_q_w_p;
  p.gru_ih_p = fold ? m->sa_fold_gru_ih_p : m->sa_gru_ih_p;
  const bool su_packed = precision >= 1 && p.gru_ih_p && m->sa_gru_hh_p && m->sa_mlp_w1_p && m->sa_mlp_w2_p && p.q_w_p;
  p.update = !su_packed ? EncodePlan::VALU : sf_slot_update_mfma_ok(D, Hm, P) ? EncodePlan::MFMA
            : sf_slot_update_wide_ok(D, Hm, P) ? EncodePlan::WIDE : EncodePlan::VALU;
  // (the folded iterations read keys == values)
  if (fold && P == HW / 256 && (planes || sf_slot_attn_sparse_records_n(nullptr, nullptr, HW, D, N))) p.p_step = 2;
  p.pred_step = m->pred_type == 1 && m->pred_packed && precision >= 1;
  p.prologue = m->pred_type == 0 && !m->pred_rnn && m->kd_mode == 1 && m->pm_w0_t && m->pm_w2_t && m->kd_w0_t && p.q_w_t;
  p.fuse_next = p.prologue && p.update == EncodePlan::MFMA && m->pm_w0_p && m->pm_w2_p && m->kd_w0_p && m->pm_ln_g && m->pm_ln_b && m->pm_b0 &&
                m->pm_b2 && m->kd_b0 && sf_switch(SF_SW_ENCODE_FUSE_NEXT);
  // (the CLEVRER shape of StoSAVi: savi.py:76-100, 393-402)
  p.chain_model = precision == 1 && fold && p.feat != EncodePlan::FOLD_192 && p.update == EncodePlan::MFMA && p.fuse_next &&
                  sf_slot_chain_ok(D, Hm, HW, N) && m->init_latents && m->enc_fc1_w && m->enc_fc2_w;
  p.batched = !fork && n_pre == 0 && enc_batched_ok(m, B, T, precision);
  p.chain = p.batched && p.chain_model && sf_switch(SF_SW_SLOT_CHAIN);
  // without room for the feature planes: the per-iteration launches; without room for the batched activations: the per-step convolutions
  if (p.chain && ws_bytes < enc_ws_bytes(m, B, T, p)) p.chain = false;
  if (p.batched && ws_bytes < enc_ws_bytes(m, B, T, p)) p.batched = false;
  return p;
}

// CNN stack (savi.py:231-244: convs + soft position embedding) for `nb` frames: frame i at src + i*frame_stride;
// the last conv writes into `dst` (NHWC [nb,64,64,C_last]); featA/featB are ping-pong scratch.
// layers [i0, i1) of the stack
int run_cnn_layers(const sf_savi_encoder* m, const float* src, long long frame_stride, int nb, float* dst, float* featA, float* featB,
                   int i0, int i1, hipStream_t st) {
  const int res = m->resolution;
  for (int i = i0; i < i1; ++i) {
    const bool lastc = (i == m->enc_layers - 1);
    const int cin = m->enc_channels[i], cout = m->enc_channels[i + 1];
    const float* add = lastc ? m->pos_table : nullptr;
    float* out = lastc ? dst : ((i & 1) ? featB : featA);
    const float* cur = i == 0 ? nullptr : (((i - 1) & 1) ? featB : featA);   // the previous layer's output
    if (i == 0) {
      SF_TRY(sf_conv2d_nchw_in_f32(src, frame_stride, m->conv_w[0], m->conv_b[0], add, out, nb, cin, res, res, cout,
                                   m->enc_ks, res == 128 ? 2 : 1, lastc ? 0 : 1, st));
    } else {
      // 64 -> 64 channels with a fragment-ordered weight copy: 4-row tiles, weights streamed as MFMA fragments (conv_rows4.hip)
      int rc = 1;
      // (weights stationary in registers where the launch gives every CU of the stream its rows: conv_ws.hip -- the same bits)
      if (rc == 1 && m->conv_w_frag[i])
        rc = sf_conv5x5_ws_ex(cur, m->conv_w_frag[i], m->conv_b[i], add, out, nb, 64, 64, cin, cout, m->enc_ks, lastc ? 0 : 1, 0, st);
      if (rc == 1 && m->conv_w_frag[i])
        rc = sf_conv5x5_rows4_ex(cur, m->conv_w_frag[i], m->conv_b[i], add, out, nb, 64, 64, cin, cout, m->enc_ks, lastc ? 0 : 1, st);
      if (rc < 0 || rc > 1) return rc;
      if (rc == 1)
        SF_TRY(sf_conv2d_nhwc_f32(cur, m->conv_w[i], m->conv_b[i], add, out, nb, 64, 64, cin, cout, m->enc_ks, lastc ? 0 : 1, st));
    }
  }
  return 0;
}

// The CNN of all B x T frames, every layer as one launch (the first per time step where its grouped kernel does not apply: the frames of one step lie
// T frames apart) -> big[2] [T][B][64 * 64][C_last]; big[0] / big[1] are ping-pong scratch
int enc_cnn_all_steps(const sf_savi_encoder* m, const float* img, int B, int T, float* const* big, hipStream_t st) {
  const int res = m->resolution, c1 = m->enc_channels[1];
  const long long frame_elems = (long long)3 * res * res;
  const int rc = sf_conv_first_grouped_ex(img, (long long)T * frame_elems, B, frame_elems, m->conv_w[0], m->conv_b[0], nullptr, big[0], B * T,
                                          m->enc_channels[0], res, res, c1, m->enc_ks, res == 128 ? 2 : 1, 1, st);
  if (rc < 0 || rc > 1) return rc;
  for (int t = 0; t < T && rc == 1; ++t)
    SF_TRY(sf_conv2d_nchw_in_f32(img + (long long)t * frame_elems, (long long)T * frame_elems, m->conv_w[0], m->conv_b[0], nullptr,
                                 big[0] + (long long)t * B * ENC_HW * c1, B, m->enc_channels[0], res, res, c1, m->enc_ks, res == 128 ? 2 : 1, 1, st));
  return run_cnn_layers(m, nullptr, 0, B * T, big[2], big[0], big[1], 1, m->enc_layers, st);
}

// ---- the encode in two halves (round 6): image features of a batch as bf16 hi | lo rows, and the slot branch of a GROUP of batches as one
//      video-stationary launch (slot_chain.hip).  The batch pipeline runs the first on its encode lane and the second in front of the group's rollout, on
//      the rollout stream: the slot branch is 32 workgroups of ~0.5 ms per batch that would leave the other 96 CUs of the lane idle. ----
// CNN + encoder_out_layer + SlotAttention.norm_inputs of all B x T frames -> planes (big: enc_cnn_all_steps scratch)
int enc_feature_planes(const sf_savi_encoder* m, const float* img, int B, int T, float* const* big, void* planes, hipStream_t st) {
  SF_TRY(enc_cnn_all_steps(m, img, B, T, big, st));
  return sf_pixel_mlp_feat_planes_ex(big[2], m->enc_ln_g, m->enc_ln_b, m->enc_fc1_w, m->enc_fc1_b, m->enc_fc2_w, m->enc_fc2_b, m->sa_norm_in_g, m->sa_norm_in_b,
                                     planes, B * T * ENC_HW, 1e-5f, st);
}
// prologue of step 0 + the chain, for NB batches of B videos; the row buffers hold NB * B * N rows each
int enc_slots_chain(const sf_savi_encoder* m, const void* planes, const float* noise, const float* prev, float* post, long long post_bs, float* kernel_dist,
                    float* attn, int NB, int B, int T, const SlotRows& r, hipStream_t st) {
  const int N = m->num_slots, D = m->slot_size;
  const float ln_eps = 1e-5f;
  const int pr = sf_slot_prologue_ex(prev, m->init_latents, m->pm_ln_g, m->pm_ln_b, m->pm_w0_t, m->pm_b0, m->pm_w2_t, m->pm_b2, m->pred_norm_first, m->kd_w0_t,
                                     m->kd_b0, noise, (long long)T * N * D, kernel_dist, (long long)T * N * 2 * D, m->sa_q_ln_g, m->sa_q_ln_b, m->sa_fold_q_w_t,
                                     r.a, r.q, NB * B, N, D, ln_eps, st);
  if (pr != 0) return pr < 0 ? pr : sf_set_err(-1, "the one-launch slot prologue does not apply to this model", __FILE__, __LINE__);
  SfChainWeights cw;
  cw.gru_ih_p = m->sa_fold_gru_ih_p; cw.gru_hh_p = m->sa_gru_hh_p; cw.gru_b_ih = m->gru_b_ih; cw.gru_b_hh = m->gru_b_hh; cw.ln_g = m->mlp_ln_g; cw.ln_b = m->mlp_ln_b;
  cw.w1_p = m->sa_mlp_w1_p; cw.b1 = m->mlp_b1; cw.w2_p = m->sa_mlp_w2_p; cw.b2 = m->mlp_b2; cw.q_ln_g = m->sa_q_ln_g; cw.q_ln_b = m->sa_q_ln_b; cw.q_w_p = m->sa_fold_q_w_p;
  cw.pm_ln_g = m->pm_ln_g; cw.pm_ln_b = m->pm_ln_b; cw.pm_w0_p = m->pm_w0_p; cw.pm_b0 = m->pm_b0; cw.pm_w2_p = m->pm_w2_p; cw.pm_b2 = m->pm_b2;
  cw.pm_norm_first = m->pred_norm_first; cw.kd_w_p = m->kd_w0_p; cw.kd_b = m->kd_b0;
  return sf_slot_chain_ex(planes, NB, B, T, ENC_HW, N, m->num_iterations, 1.0f / sqrtf((float)D), m->sa_eps, ln_eps, r.a, r.b, r.lat, r.q, post, post_bs, attn,
                          noise, kernel_dist, &cw, st);
}

// fork / join events of the forked encode, per host thread (created on first use, kept for the life of the thread: the library's
// only host-side objects; no device memory)
hipEvent_t enc_fork_event(int i) {
  // keyed by the CURRENT device: an event belongs to the device it was created on, and one host thread may drive several GPUs (engine.py keeps its
  // side streams per device); recording a device-0 event on a device-1 stream is hipErrorInvalidHandle
  thread_local std::map<int, std::vector<hipEvent_t>> per_dev;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::vector<hipEvent_t>& ev = per_dev[dev];
  while ((int)ev.size() <= i) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    ev.push_back(e);
  }
  return ev[i];
}
// fork event i of the forked encode: recorded on stream s / waited for on stream s
int enc_fork_record(int i, hipStream_t s) {
  const hipEvent_t e = enc_fork_event(i);
  SF_REQUIRE(e != nullptr, "hipEventCreate failed");
  return hipEventRecord(e, s) == hipSuccess ? 0 : sf_set_err((int)hipGetLastError(), "hipEventRecord", __FILE__, __LINE__);
}
int enc_fork_wait(int i, hipStream_t s) {
  return hipStreamWaitEvent(s, enc_fork_event(i), 0) == hipSuccess ? 0 : sf_set_err((int)hipGetLastError(), "hipStreamWaitEvent", __FILE__, __LINE__);
}

// the arguments of one encode call that its steps read
struct EncodeArgs {
  const sf_savi_encoder* m;
  const float *img, *feat_pre, *noise;
  float *lstm_h, *lstm_c, *post, *kernel_dist, *attn;
  int B, T;
};

// ---- the image features of step t: CNN (or its precomputed / batched output) -> encoder_out_layer (LN -> Linear -> ReLU -> Linear, savi.py:245-250)
//      -> the Slot-Attention inputs (savi.py:66-70) at kv, per chunk of up to 32 frames ----
int enc_step_features(const EncodeArgs& a, const EncodePlan& p, const EncodeWs& w, int t, float* kv, hipStream_t st) {
  const sf_savi_encoder* m = a.m;
  const int HW = ENC_HW, B = a.B, Bc = enc_chunk(B), Cl = m->enc_channels[m->enc_layers], Ce = m->enc_out_channels, D = m->slot_size;
  const long long frame_elems = (long long)3 * m->resolution * m->resolution;
  const float ln_eps = 1e-5f;
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int nb = (B - b0 < Bc) ? (B - b0) : Bc, Mp = nb * HW;
    const float* cur;
    if (t < p.n_pre) {
      cur = a.feat_pre + ((long long)t * B + b0) * HW * Cl;
    } else if (p.batched) {
      cur = w.big[2] + ((long long)t * B + b0) * HW * Cl;
    } else {
      float* dstf = (m->enc_layers & 1) ? w.feat[0] : w.feat[1];   // the buffer the last conv does not read
      SF_TRY(run_cnn_layers(m, a.img + ((long long)b0 * a.T + t) * frame_elems, (long long)a.T * frame_elems, nb, dstf, w.feat[0], w.feat[1], 0,
                            m->enc_layers, st));
      cur = dstf;
    }
    if (p.feat == EncodePlan::FOLD_192) {
      SF_TRY(sf_pixel_mlp_feat192_ex(cur, m->enc_ln_g, m->enc_ln_b, m->enc_fc1_p, m->enc_fc1_b, m->enc_fc2_p, m->enc_fc2_b,
                                     m->sa_norm_in_g, m->sa_norm_in_b, kv + (long long)b0 * HW * Ce, Mp, ln_eps, st));
    } else if (p.feat == EncodePlan::FOLD_PLANES) {
      SF_TRY(sf_pixel_mlp_feat_planes_ex(cur, m->enc_ln_g, m->enc_ln_b, m->enc_fc1_w, m->enc_fc1_b, m->enc_fc2_w, m->enc_fc2_b, m->sa_norm_in_g, m->sa_norm_in_b,
                                         (char*)kv + (size_t)b0 * HW * 512, Mp, ln_eps, st));
    } else if (p.feat == EncodePlan::FOLD_ROWS) {
      SF_TRY(sf_pixel_mlp_feat_ex(cur, m->enc_ln_g, m->enc_ln_b, m->enc_fc1_w, m->enc_fc1_b, m->enc_fc2_w, m->enc_fc2_b,
                                  m->sa_norm_in_g, m->sa_norm_in_b, kv + (long long)b0 * HW * Ce, Mp, ln_eps, st));
    } else {
      float* kv_dst = kv + (long long)b0 * HW * 2 * D;
      int rc = 1;
      if (p.feat == EncodePlan::KV_FUSED)   // one kernel per 128-pixel tile (pixel_mlp.hip)
        rc = sf_pixel_mlp_kv_ex(cur, m->enc_ln_g, m->enc_ln_b, m->enc_fc1_w, m->enc_fc1_b, m->enc_fc2_w, m->enc_fc2_b, m->sa_norm_in_g, m->sa_norm_in_b,
                                m->sa_kv_w, kv_dst, Mp, Cl, Ce, 2 * D, ln_eps, st);
      if (rc < 0 || rc > 1) return rc;
      if (rc == 1) {
        SF_TRY(sf_linear_ex(cur, sf_rows(Cl), m->enc_fc1_w, m->enc_fc1_b, m->enc_ln_g, m->enc_ln_b, ln_eps, nullptr,
                            sf_rows(Ce), 0, w.h1, sf_rows(Ce), Mp, Ce, Cl, 1, st));
        SF_TRY(sf_linear_ex(w.h1, sf_rows(Ce), m->enc_fc2_w, m->enc_fc2_b, nullptr, nullptr, ln_eps, nullptr,
                            sf_rows(Ce), 0, w.h2, sf_rows(Ce), Mp, Ce, Ce, 0, st));
        SF_TRY(sf_linear_ex(w.h2, sf_rows(Ce), m->sa_kv_w, nullptr, m->sa_norm_in_g, m->sa_norm_in_b, ln_eps, nullptr,
                            sf_rows(2 * D), 0, kv_dst, sf_rows(2 * D), Mp, 2 * D, Ce, 0, st));
      }
    }
  }
  return 0;
}

// ---- the prior of a step's slots: init_latents without previous slots, else predictor(prev) (savi.py:393-398) -> *lat ----
int enc_predict(const EncodeArgs& a, const EncodePlan& p, const EncodeWs& w, const float* prev, hipStream_t st, const float** lat) {
  const sf_savi_encoder* m = a.m;
  const int N = m->num_slots, D = m->slot_size, R = a.B * N;
  const float ln_eps = 1e-5f;
  *lat = w.rows.lat;
  if (prev == nullptr) return sf_copy_rows_ex(m->init_latents, sf_rows_batched(D, N, 0, 0), w.rows.lat, sf_rows(D), R, D, st);
  int rc = 1;
  if (p.pred_step)   // Transformer predictor (+ LSTM wrapper) in one launch (pred_step.hip)
    rc = sf_pred_step_ex(prev, m->pred_layers, m->pred_num_layers, m->pred_num_heads, m->pred_ffn_dim, m->pred_norm_first, m->pred_packed, m->lstm_b_ih,
                         m->lstm_b_hh, m->proj_b, m->pred_hidden, m->pred_rnn ? a.lstm_h : nullptr, m->pred_rnn ? a.lstm_c : nullptr, w.rows.lat, a.B, N, D,
                         ln_eps, st);
  if (rc != 1) return rc;
  const float* pout;
  if (m->pred_type == 0) {
    // ResidualMLPPredictor (predictor.py:65-73)
    SF_TRY(sf_layernorm_ex(prev, sf_rows(D), m->pm_ln_g, m->pm_ln_b, w.lnbuf, sf_rows(D), R, D, ln_eps, st));
    SF_TRY(sf_linear_ex(w.lnbuf, sf_rows(D), m->pm_w0, m->pm_b0, nullptr, nullptr, ln_eps, nullptr, sf_rows(D), 0,
                        w.tw.hid, sf_rows(2 * D), R, 2 * D, D, 1, st));
    SF_TRY(sf_linear_ex(w.tw.hid, sf_rows(2 * D), m->pm_w2, m->pm_b2, nullptr, nullptr, ln_eps,
                        m->pred_norm_first ? w.lnbuf : prev, sf_rows(D), 0, w.px, sf_rows(D), R, D, 2 * D, 0, st));
    pout = w.px;
  } else {
    // TransformerPredictor over the N slots (predictor.py:20-44)
    SF_TRY(sf_copy_rows_ex(prev, sf_rows(D), w.px, sf_rows(D), R, D, st));
    float* cur = w.px;
    TfmWs tw = w.tw;
    for (int l = 0; l < m->pred_num_layers; ++l)
      SF_TRY(tfm_layer(m->pred_layers[l], cur, tw, a.B, N, N, D, m->pred_num_heads, m->pred_ffn_dim, m->pred_norm_first, st, &cur));
    pout = cur;
  }
  *lat = m->pred_rnn ? w.rows.lat : pout;
  if (!m->pred_rnn) return 0;
  // nn.LSTM, seq len 1, batch B*N (predictor.py:113-120)
  const int Hh = m->pred_hidden;
  SF_TRY(sf_linear_ex(pout, sf_rows(D), m->lstm_w_ih, m->lstm_b_ih, nullptr, nullptr, ln_eps, nullptr,
                      sf_rows(4 * Hh), 0, w.gates, sf_rows(4 * Hh), R, 4 * Hh, D, 0, st));
  SF_TRY(sf_linear_ex(a.lstm_h, sf_rows(Hh), m->lstm_w_hh, m->lstm_b_hh, nullptr, nullptr, ln_eps, w.gates,
                      sf_rows(4 * Hh), 0, w.gates, sf_rows(4 * Hh), R, 4 * Hh, Hh, 0, st));
  SF_TRY(sf_lstm_pointwise_ex(w.gates, a.lstm_c, a.lstm_h, a.lstm_c, R, Hh, st));
  return sf_linear_ex(a.lstm_h, sf_rows(Hh), m->proj_w, m->proj_b, nullptr, nullptr, ln_eps, nullptr,
                      sf_rows(D), 0, w.rows.lat, sf_rows(D), R, D, Hh, 0, st);
}

// ---- the slots of step t before its first iteration -> rows.a, their q -> rows.q: the one-launch slot prologue where it applies (*one_launch; predictor
//      -> kernel_dist -> sampling -> q, slot_attn.hip), else the prior, the kernel distribution + sampling (savi.py:401-402) and q as an LN-fused GEMM ----
int enc_slot_init(const EncodeArgs& a, const EncodePlan& p, const EncodeWs& w, const float* prev, int t, hipStream_t st, bool* one_launch) {
  const sf_savi_encoder* m = a.m;
  const int N = m->num_slots, D = m->slot_size, R = a.B * N, T = a.T;
  const float ln_eps = 1e-5f;
  int rc = 1;
  if (p.prologue)
    rc = sf_slot_prologue_ex(prev, m->init_latents, m->pm_ln_g, m->pm_ln_b, m->pm_w0_t, m->pm_b0, m->pm_w2_t, m->pm_b2, m->pred_norm_first, m->kd_w0_t,
                             m->kd_b0, a.noise ? a.noise + (long long)t * N * D : nullptr, (long long)T * N * D,
                             a.kernel_dist ? a.kernel_dist + (long long)t * N * 2 * D : nullptr, (long long)T * N * 2 * D, m->sa_q_ln_g, m->sa_q_ln_b,
                             p.q_w_t, w.rows.a, w.rows.q, a.B, N, D, ln_eps, st);
  *one_launch = rc == 0;
  if (rc != 1) return rc;
  const float* lat;
  SF_TRY(enc_predict(a, p, w, prev, st, &lat));
  if (m->kd_mode == 0) {
    SF_TRY(sf_copy_rows_ex(lat, sf_rows(D), w.rows.a, sf_rows(D), R, D, st));
  } else {
    SF_TRY(sf_linear_ex(lat, sf_rows(D), m->kd_w0, m->kd_b0, nullptr, nullptr, ln_eps, nullptr, sf_rows(2 * D), 0,
                        m->kd_mode == 1 ? w.kdist : w.kdtmp, sf_rows(2 * D), R, 2 * D, D, 0, st));
    if (m->kd_mode == 2)   // Linear -> LayerNorm -> ReLU -> Linear
      SF_TRY(sf_linear_ex(w.kdtmp, sf_rows(2 * D), m->kd_w3, m->kd_b3, m->kd_ln_g, m->kd_ln_b, ln_eps, nullptr,
                          sf_rows(2 * D), 0, w.kdist, sf_rows(2 * D), R, 2 * D, 2 * D, 0, st, /*ln_relu=*/1));
    const SfRowMap nmap = sf_rows_batched(D, N, (long long)T * N * D, (long long)t * N * D);
    SF_TRY(sf_sample_dist_ex(w.kdist, a.noise, nmap, w.rows.a, R, D, st));
    if (a.kernel_dist)
      SF_TRY(sf_copy_rows_ex(w.kdist, sf_rows(2 * D), a.kernel_dist, sf_rows_batched(2 * D, N, (long long)T * N * 2 * D, (long long)t * N * 2 * D), R,
                             2 * D, st));
  }
  // q of the first iteration; every later q comes out of the slot-update kernel
  return sf_linear_ex(w.rows.a, sf_rows(D), p.q_w, nullptr, m->sa_q_ln_g, m->sa_q_ln_b, ln_eps, nullptr, sf_rows(D), 0, w.rows.q, sf_rows(D), R, D, D, 0, st);
}

// ---- the Slot-Attention iterations of step t (savi.py:76-100) on the inputs at kv, from rows.a and its q; the last slot update writes post[:, t]
//      (next: and the slot prologue of step t + 1 into rows.a / rows.q, NEXT form).  *out: the buffer that holds step t's slots afterwards ----
int enc_iterations(const EncodeArgs& a, const EncodePlan& p, const EncodeWs& w, const float* kv, int t, bool next, hipStream_t st, const float** out) {
  const sf_savi_encoder* m = a.m;
  const int HW = ENC_HW, N = m->num_slots, D = m->slot_size, Hm = m->slot_mlp_size, Ce = m->enc_out_channels, T = a.T, B = a.B, P = sf_sa_pick_partials(HW);
  const float ln_eps = 1e-5f, scale = 1.0f / sqrtf((float)D);
  const long long attn_bs = (long long)T * N * HW, post_bs = (long long)T * N * D;
  float *s_in = w.rows.a, *s_out = w.rows.b;
  for (int it = 0; it < m->num_iterations; ++it) {
    const bool last_it = (it == m->num_iterations - 1), nx_on = next && last_it;
    float* aout = (a.attn && last_it) ? a.attn + (long long)t * N * HW : nullptr;
    float* post = last_it ? a.post + (long long)t * N * D : nullptr;
    if (p.feat == EncodePlan::FOLD_PLANES)
      SF_TRY(sf_slot_attn_planes_ex(kv, HW, w.rows.q, w.pnum, w.pden, aout, attn_bs, B, HW, N, scale, m->sa_eps, st));
    else if (p.fold())   // keys = values = the normalised features (q is Wk^T q here, the GRU input matrix is W_ih Wv)
      SF_TRY(sf_slot_attn_iter_ex(kv, kv, Ce, (long long)HW * Ce, w.rows.q, w.pnum, w.pden, aout, attn_bs, B, HW, N, D, scale, m->sa_eps, st));
    else
      SF_TRY(sf_slot_attn_iter_ex(kv, kv + D, 2 * D, (long long)HW * 2 * D, w.rows.q, w.pnum, w.pden, aout, attn_bs, B, HW, N, D, scale, m->sa_eps, st));
    if (p.update == EncodePlan::MFMA) {
      SfNextStep nx;   // (read in the NEXT form only)
      nx.pm_ln_g = m->pm_ln_g; nx.pm_ln_b = m->pm_ln_b; nx.pm_w0_p = m->pm_w0_p; nx.pm_b0 = m->pm_b0; nx.pm_w2_p = m->pm_w2_p; nx.pm_b2 = m->pm_b2;
      nx.norm_first = m->pred_norm_first; nx.kd_w_p = m->kd_w0_p; nx.kd_b = m->kd_b0;
      nx.noise = a.noise ? a.noise + (long long)(t + 1) * N * D : nullptr; nx.noise_bs = (long long)T * N * D;
      nx.kdist_out = a.kernel_dist ? a.kernel_dist + (long long)(t + 1) * N * 2 * D : nullptr; nx.kdist_bs = (long long)T * N * 2 * D;
      nx.slots = w.rows.a;   // where the next step's iterations start
      // (NEXT form: the finished rows of step t go to post[:, t]; their ping-pong copy is not read again, and must not alias the sampled slots)
      SF_TRY(sf_slot_update_mfma_ex(w.pnum, w.pden, P, s_in, p.gru_ih_p, m->sa_gru_hh_p, m->gru_b_ih, m->gru_b_hh, m->mlp_ln_g, m->mlp_ln_b,
                                    m->sa_mlp_w1_p, m->mlp_b1, m->sa_mlp_w2_p, m->mlp_b2, (nx_on && s_out == w.rows.a) ? w.rows.lat : s_out, post, post_bs,
                                    m->sa_q_ln_g, m->sa_q_ln_b, p.q_w_p, (last_it && !nx_on) ? nullptr : w.rows.q, B, N, ln_eps, st, nx_on ? &nx : nullptr,
                                    p.p_step));
    } else if (p.update == EncodePlan::WIDE) {
      SF_TRY(sf_slot_update_wide_ex(w.pnum, w.pden, P, s_in, p.gru_ih_p, m->sa_gru_hh_p, m->gru_b_ih, m->gru_b_hh, m->mlp_ln_g, m->mlp_ln_b,
                                    m->sa_mlp_w1_p, m->mlp_b1, m->sa_mlp_w2_p, m->mlp_b2, s_out, post, post_bs, m->sa_q_ln_g, m->sa_q_ln_b,
                                    p.q_w_p, last_it ? nullptr : w.rows.q, B, N, ln_eps, st));
    } else {
      SF_TRY(sf_slot_update_ex(w.pnum, w.pden, P, s_in, p.gru_ih_t, m->gru_w_hh, m->gru_b_ih, m->gru_b_hh, m->mlp_ln_g, m->mlp_ln_b, m->mlp_w1,
                               m->mlp_b1, m->mlp_w2, m->mlp_b2, s_out, post, post_bs, m->sa_q_ln_g, m->sa_q_ln_b, p.q_w_t,
                               (last_it || !p.q_w_t) ? nullptr : w.rows.q, B, N, D, Hm, ln_eps, st));
      if (!last_it && !p.q_w_t)   // no transposed copy of project_q given: the LN-fused GEMM produces q
        SF_TRY(sf_linear_ex(s_out, sf_rows(D), p.q_w, nullptr, m->sa_q_ln_g, m->sa_q_ln_b, ln_eps, nullptr, sf_rows(D), 0, w.rows.q,
                            sf_rows(D), B * N, D, D, 0, st));
    }
    std::swap(s_in, s_out);
  }
  *out = s_in;
  return 0;
}
}  // namespace

extern "C" {

size_t sf_savi_encode_workspace_bytes(const sf_savi_encoder* m, int B) {
  return (m && B > 0) ? enc_ws_bytes(m, B, 1, plan_encode(m, B, 1, 0, false, 0)) : 0;
}
size_t sf_savi_encode_fork_workspace_bytes(const sf_savi_encoder* m, int B, int T) {
  return (m && B > 0 && T >= 1) ? enc_ws_bytes(m, B, T, plan_encode(m, B, T, 0, true, 0)) : 0;
}
// One-stream encode with the convolutions of ALL T time steps as one launch per layer (the weights-stationary kernel of conv_ws.hip pays its 410 KB of
// weights per workgroup once per launch: 81 instead of 99 us per time step and layer on a 128-CU partition): the activations of B * T frames in three
// buffers on top of sf_savi_encode_workspace_bytes, and under sf_set_slot_chain(1) the feature planes of the video-stationary slot branch.
// sf_savi_encode_fork_f32 (side_stream NULL) takes this form when it is handed that much workspace.
size_t sf_savi_encode_batched_workspace_bytes(const sf_savi_encoder* m, int B, int T) {
  return (m && B > 0 && T > 0) ? enc_ws_bytes(m, B, T, plan_encode(m, B, T, 0, false, ~(size_t)0)) : 0;
}

size_t sf_savi_cnn_workspace_bytes(const sf_savi_encoder* m, int B) {
  if (!m || B <= 0) return 0;
  SfArena bp(nullptr);
  float* feat[2];
  enc_cnn_take(bp, feat, 2, m, enc_chunk(B));
  return bp.bytes() + 4096;
}

// CNN features of time steps [t0, t1) of every video: feat [t1-t0][B][64*64][C_last].  Independent of the slots, so a
// caller may compute them ahead of sf_savi_encode_pre_f32 on another stream (bench.py runs part of the NEXT batch's
// convolutions on the rollout stream's CUs while that stream would otherwise idle).
int sf_savi_cnn_f32(const sf_savi_encoder* m, const float* img, int B, int T, int t0, int t1, float* feat, void* ws,
                    size_t ws_bytes, void* stream) {
  SF_REQUIRE(m && img && feat && ws, "null pointer");
  SF_REQUIRE(B >= 1 && T >= 1 && t0 >= 0 && t1 >= t0 && t1 <= T, "bad batch / time range");
  SF_REQUIRE(m->resolution == 64 || m->resolution == 128, "resolution must be 64 or 128 (savi.py:226,236)");
  SF_REQUIRE(m->enc_layers >= 1 && m->enc_layers <= 8 && m->pos_table, "bad CNN config");
  SF_REQUIRE(ws_bytes >= sf_savi_cnn_workspace_bytes(m, B), "workspace too small");
  for (int i = 0; i < m->enc_layers; ++i) SF_REQUIRE(m->conv_w[i] != nullptr, "null conv weight");
  const int Bc = enc_chunk(B), HW = ENC_HW, Cl = m->enc_channels[m->enc_layers];
  SfArena bp(ws, ws_bytes);
  float* fb[2];
  enc_cnn_take(bp, fb, 2, m, Bc);
  if (!bp.ok) return sf_set_err(-1, "workspace too small", __FILE__, __LINE__);
  const long long frame_elems = (long long)3 * m->resolution * m->resolution;
  // these launches usually run on another stream / CU partition than the encode: keep them out of the per-class
  // HIP-event timer so that bench.py's live conv figure stays "launches of the encode stream"
  sf_prof_suppress(1);
  int rc = 0;
  for (int t = t0; t < t1 && rc == 0; ++t)
    for (int b0 = 0; b0 < B && rc == 0; b0 += Bc) {
      const int nb = (B - b0 < Bc) ? (B - b0) : Bc;
      rc = run_cnn_layers(m, img + ((long long)b0 * T + t) * frame_elems, (long long)T * frame_elems, nb,
                          feat + ((long long)(t - t0) * B + b0) * HW * Cl, fb[0], fb[1], 0, m->enc_layers, (hipStream_t)stream);
    }
  sf_prof_suppress(0);
  return rc;
}

int sf_savi_chain_ok(const sf_savi_encoder* m, int B, int T) {
  const EncodePlan p = plan_encode(m, B, T, 0, false, ~(size_t)0);   // (the conditions of a batched encode that runs the chain)
  return (p.batched && p.chain_model) ? 1 : 0;
}
size_t sf_savi_planes_bytes(const sf_savi_encoder* m, int B, int T) { return (m && B > 0 && T > 0) ? (size_t)B * T * ENC_HW * 512 : 0; }
size_t sf_savi_features_workspace_bytes(const sf_savi_encoder* m, int B, int T) {
  if (!m || B <= 0 || T <= 0) return 0;
  SfArena bp(nullptr);
  float* big[3];
  enc_cnn_take(bp, big, 3, m, (size_t)B * T);
  return bp.bytes() + 4096;
}
// Image features of B videos x T frames as the Slot-Attention inputs of the video-stationary slot branch: CNN (savi.py:231-244), encoder_out_layer
// (:245-250) and SlotAttention.norm_inputs (:66) -> planes [T][B][64 * 64] rows of 512 B (bf16 hi 128 | lo 128).  Independent of any slots.
int sf_savi_features_planes_f32(const sf_savi_encoder* m, const float* img, int B, int T, void* planes, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(m && img && planes && ws, "sf_savi_features_planes_f32: null pointer");
  SF_REQUIRE(B >= 1 && T >= 1 && sf_savi_chain_ok(m, B, T), "sf_savi_features_planes_f32: the video-stationary slot branch does not apply (sf_savi_chain_ok)");
  SF_REQUIRE(ws_bytes >= sf_savi_features_workspace_bytes(m, B, T), "workspace too small");
  SfArena bp(ws, ws_bytes);
  float* big[3];
  enc_cnn_take(bp, big, 3, m, (size_t)B * T);
  if (!bp.ok) return sf_set_err(-1, "workspace too small", __FILE__, __LINE__);
  return enc_feature_planes(m, img, B, T, big, planes, (hipStream_t)stream);
}
size_t sf_savi_slots_chain_workspace_bytes(const sf_savi_encoder* m, int videos) {
  if (!m || videos <= 0) return 0;
  SfArena bp(nullptr);
  SlotRows r;
  slot_rows_take(bp, r, (size_t)videos * m->num_slots, m->slot_size);
  return bp.bytes() + 4096;
}
// The slot branch of NB batches of B videos over their T frames (StoSAVi.encode's per-step chain, savi.py:393-416, and the Slot-Attention iterations,
// :76-100) from sf_savi_features_planes_f32 rows: planes [NB][T][B][64 * 64][256 bf16]; noise NULL or [NB * B][T][N][D]; prev_slots NULL or [NB * B][N][D];
// video v's slots of step t -> post + v * post_bs + t * N * D; kernel_dist NULL or [NB * B][T][N][2 D]; attn NULL or [NB * B][T][N][64 * 64].
int sf_savi_slots_chain_f32(const sf_savi_encoder* m, const void* planes, const float* noise, const float* prev_slots, float* post, long long post_bs,
                            float* kernel_dist, float* attn, int NB, int B, int T, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(m && planes && post && ws, "sf_savi_slots_chain_f32: null pointer");
  SF_REQUIRE(NB >= 1 && B >= 1 && T >= 1 && plan_encode(m, B, T, 0, false, 0).chain_model,
             "sf_savi_slots_chain_f32: the video-stationary slot branch does not apply (sf_savi_chain_ok)");
  SF_REQUIRE(noise == nullptr || m->kd_mode != 0, "noise given but the model has no kernel_dist layer");
  SF_REQUIRE(ws_bytes >= sf_savi_slots_chain_workspace_bytes(m, NB * B), "workspace too small");
  SfArena bp(ws, ws_bytes);
  SlotRows r;
  slot_rows_take(bp, r, (size_t)NB * B * m->num_slots, m->slot_size);
  if (!bp.ok) return sf_set_err(-1, "workspace too small", __FILE__, __LINE__);
  return enc_slots_chain(m, planes, noise, prev_slots, post, post_bs, kernel_dist, attn, NB, B, T, r, (hipStream_t)stream);
}

int sf_savi_encode_f32(const sf_savi_encoder* m, const float* img, const float* noise, const float* prev_slots,
                       float* lstm_h, float* lstm_c, int state_valid, float* post_slots, float* kernel_dist,
                       float* attn, int B, int T, void* ws, size_t ws_bytes, void* stream) {
  return sf_savi_encode_pre_f32(m, img, nullptr, 0, noise, prev_slots, lstm_h, lstm_c, state_valid, post_slots, kernel_dist,
                                attn, B, T, ws, ws_bytes, stream);
}

// As sf_savi_encode_f32, with the CNN features of the first n_pre time steps already computed by sf_savi_cnn_f32
// (feat_pre [n_pre][B][64*64][C_last]; NULL / 0: compute everything here).
int sf_savi_encode_pre_f32(const sf_savi_encoder* m, const float* img, const float* feat_pre, int n_pre, const float* noise,
                           const float* prev_slots, float* lstm_h, float* lstm_c, int state_valid, float* post_slots,
                           float* kernel_dist, float* attn, int B, int T, void* ws, size_t ws_bytes, void* stream) {
  return sf_savi_encode_fork_f32(m, img, feat_pre, n_pre, noise, prev_slots, lstm_h, lstm_c, state_valid, post_slots, kernel_dist, attn,
                                 B, T, ws, ws_bytes, stream, nullptr);
}


// The encode as TWO branches (side_stream != NULL).  The image features of a time step (CNN + per-pixel chain: ~420 us of dense
// launches per step at C2) do not depend on the slots; the slot branch of a step (prologue, Slot-Attention iterations, slot updates:
// ~140 us, half of it in seven-workgroup launches that leave the chip idle) needs only that step's features.  `stream` runs the
// features of all T steps back to back; `side_stream` follows one step behind with the slot branches, ordered by events (fork after
// the features of step t, join at the end: `stream` waits for the last slot update).
// Captured into a hipGraph the two become parallel branches of the graph.  Same kernels, same arguments, same bits.  Workspace:
// sf_savi_encode_fork_workspace_bytes(m, B, T).
int sf_savi_encode_fork_f32(const sf_savi_encoder* m, const float* img, const float* feat_pre, int n_pre, const float* noise,
                            const float* prev_slots, float* lstm_h, float* lstm_c, int state_valid, float* post_slots,
                            float* kernel_dist, float* attn, int B, int T, void* ws, size_t ws_bytes, void* stream, void* side_stream) {
  SF_REQUIRE(m && img && post_slots && ws, "null pointer");
  SF_REQUIRE(n_pre >= 0 && n_pre <= T && (n_pre == 0 || feat_pre != nullptr), "bad precomputed-feature arguments");
  SF_REQUIRE(B >= 1 && T >= 1, "bad batch / clip length");
  SF_REQUIRE(m->resolution == 64 || m->resolution == 128, "resolution must be 64 or 128 (savi.py:226,236)");
  SF_REQUIRE(m->enc_layers >= 1 && m->enc_layers <= 8 && m->enc_channels[0] > 0 && (m->enc_ks & 1), "bad CNN config");
  SF_REQUIRE(m->num_slots >= 1 && m->num_slots <= 16 && m->num_iterations >= 1, "bad slot config (1 <= num_slots <= 16)");
  SF_REQUIRE(m->pos_table && m->enc_ln_g && m->enc_ln_b && m->enc_fc1_w && m->enc_fc1_b && m->enc_fc2_w &&
                 m->enc_fc2_b && m->sa_norm_in_g && m->sa_norm_in_b && m->sa_q_ln_g && m->sa_q_ln_b &&
                 m->sa_q_w && m->sa_kv_w && m->init_latents, "null encoder weight");
  SF_REQUIRE(m->kd_mode >= 0 && m->kd_mode <= 2, "bad kd_mode");
  SF_REQUIRE(m->kd_mode == 0 || (m->kd_w0 && m->kd_b0), "null kernel_dist weight");
  SF_REQUIRE(m->kd_mode != 2 || (m->kd_ln_g && m->kd_ln_b && m->kd_w3 && m->kd_b3), "null kernel_dist weight");
  SF_REQUIRE(noise == nullptr || m->kd_mode != 0, "noise given but the model has no kernel_dist layer");
  if (m->pred_type == 0)
    SF_REQUIRE(m->pm_ln_g && m->pm_ln_b && m->pm_w0 && m->pm_b0 && m->pm_w2 && m->pm_b2, "null predictor weight");
  else
    SF_REQUIRE(check_layers(m->pred_layers, m->pred_num_layers) == 0, "null predictor weight");
  if (m->pred_rnn)
    SF_REQUIRE(lstm_h && lstm_c && m->pred_hidden > 0 && m->lstm_w_ih && m->lstm_w_hh && m->lstm_b_ih &&
                   m->lstm_b_hh && m->proj_w && m->proj_b, "null LSTM state / weight");
  const EncodePlan p = plan_encode(m, B, T, n_pre, side_stream != nullptr && side_stream != stream, ws_bytes);
  for (int i = 0; i < m->enc_layers; ++i) SF_REQUIRE(m->conv_w[i] != nullptr, "null conv weight");
  SfArena bp(ws, ws_bytes);
  EncodeWs w;
  SF_REQUIRE(ws_bytes >= enc_ws_bytes(m, B, T, p) && enc_ws_take(bp, w, m, B, T, p), "workspace too small");
  const hipStream_t st_main = (hipStream_t)stream, st = p.fork ? (hipStream_t)side_stream : st_main;   // st: the slot branch
  const EncodeArgs a{m, img, feat_pre, noise, lstm_h, lstm_c, post_slots, kernel_dist, attn, B, T};
  const int N = m->num_slots, D = m->slot_size;
  const float* prev = prev_slots;
  if (m->pred_rnn && (prev == nullptr || !state_valid)) {
    // RNNPredictorWrapper.reset(): hidden_state = None -> zeros on first use (predictor.py:132-135)
    // (a KERNEL, not hipMemsetAsync: the encode may be captured into a hipGraph, and memset nodes were seen to stop clearing
    //  after an older graph exec had been destroyed -- see zero_words_kernel above; pipeline encode graphs hit it at once)
    const long long nz = (long long)B * N * m->pred_hidden;
    hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)(((nz + 3) / 4 + 255) / 256)), dim3(256), 0, st_main, lstm_h, lstm_c, nz);
    SF_CHECK_LAUNCH();
  }
  if (p.chain) {   // the slot branch of all T steps as ONE video-stationary launch behind the features of the B * T frames as bf16 hi | lo rows
    SF_TRY(enc_feature_planes(m, img, B, T, w.big, w.planes, st_main));
    return enc_slots_chain(m, w.planes, noise, prev, post_slots, (long long)T * N * D, kernel_dist, attn, 1, B, T, w.rows, st_main);
  }
  // (the per-pixel chain stays per time step: as ONE launch for the B * T frames it takes 333 instead of 6 x 65 us on the lane, but the Slot-Attention
  //  iterations then read their rows from HBM instead of the cache the launch in front of them left warm: 18.9 -> 20.8 us each -- no gain, probes r06)
  if (p.batched) SF_TRY(enc_cnn_all_steps(m, img, B, T, w.big, st_main));
  bool next_done = false;   // the slot prologue of step t ran at the tail of step t - 1's last slot update
  for (int t = 0; t < T; ++t) {
    float* kv = w.kv + (size_t)(t % p.KV) * B * ENC_HW * 2 * D;
    if (p.fork && t >= p.KV) SF_TRY(enc_fork_wait(T + 1 + (t - p.KV), st_main));   // the ring slot, once the slot branch of step t - KV has read it
    SF_TRY(enc_step_features(a, p, w, t, kv, st_main));
    if (p.fork) {   // the slot branch of step t behind its features
      SF_TRY(enc_fork_record(t, st_main));
      SF_TRY(enc_fork_wait(t, st));
    }
    bool one_launch = next_done;
    if (!next_done) SF_TRY(enc_slot_init(a, p, w, prev, t, st, &one_launch));
    next_done = p.fuse_next && one_launch && t + 1 < T;
    SF_TRY(enc_iterations(a, p, w, kv, t, next_done, st, &prev));
    if (p.fork && t + p.KV < T) SF_TRY(enc_fork_record(T + 1 + t, st));
  }
  if (p.fork) {   // join: the calling stream continues behind the last slot update
    SF_TRY(enc_fork_record(T, st));
    SF_TRY(enc_fork_wait(T, st_main));
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// StoSAVi.decode (savi.py:504-525)
// floats of the largest activation map of ONE slot image: max over the layers of size_i^2 x channels_i (the broadcast input, every layer output)
static size_t dec_maxact(const sf_savi_decoder* m) {
  size_t best = (size_t)m->dec_res * m->dec_res * m->dec_channels[0];
  int size = m->dec_res;
  for (int i = 0; i < m->dec_layers && i < 8; ++i) {
    size *= m->dec_strides[i] > 0 ? m->dec_strides[i] : 1;
    const size_t a = (size_t)size * size * m->dec_channels[i + 1];
    best = a > best ? a : best;
  }
  const size_t tab = (size_t)25 * m->dec_channels[1];   // the first layer's class table
  return best > tab ? best : tab;
}
// frames per chunk: one activation buffer <= 1 GiB (7 slots at 128 x 128 x 64: 36 frames = 252 slot images per launch -- one round of
// 16-pixel-wide tiles, four of 32-wide, sixteen of 64-wide; chunks of 4 frames, the round-1 size, left most of the chip idle in the small layers)
static int dec_chunk(const sf_savi_decoder* m, int F) {
  const double per_frame = (double)m->num_slots * (double)dec_maxact(m);
  int fc = (int)(256.0 * 1024 * 1024 / per_frame);
  if (fc < 1) fc = 1;
  return fc < F ? fc : F;
}

struct DecodeWs {
  float *bufA, *bufB, *dec;
  unsigned* slot_max;
};
static DecodeWs dec_ws_take(SfArena& bp, const sf_savi_decoder* m, int F) {
  const size_t R = (size_t)dec_chunk(m, F) * m->num_slots, HW = (size_t)m->resolution * m->resolution;
  float *a = bp.take(R * dec_maxact(m)), *b = bp.take(R * dec_maxact(m)), *dec = bp.take(R * HW * 4);
  return DecodeWs{a, b, dec, bp.take<unsigned>(R)};
}
size_t sf_savi_decode_workspace_bytes(const sf_savi_decoder* m, int F) {
  if (!m || F <= 0) return 0;
  SfArena bp(nullptr);
  dec_ws_take(bp, m, F);
  return bp.bytes() + 4096;
}

int sf_savi_decode_f32(const sf_savi_decoder* m, const float* slots, float* recon_combined, float* recons,
                       float* masks, int F, void* ws, size_t ws_bytes, void* stream) {
  return sf_savi_decode_seg_f32(m, slots, recon_combined, recons, masks, nullptr, nullptr, 0.5f, F, ws, ws_bytes, stream);
}

int sf_savi_decode_seg_f32(const sf_savi_decoder* m, const float* slots, float* recon_combined, float* recons, float* masks,
                           long long* seg_i64, unsigned char* seg_u8, float fg_thre, int F, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(m && slots && recon_combined && ws, "null pointer");
  SF_REQUIRE(F >= 1 && m->dec_layers >= 1 && m->dec_layers <= 8 && m->num_slots >= 1 && m->dec_res >= 1 && (m->dec_ks & 1),
             "bad decoder config");
  SF_REQUIRE(m->dec_channels[0] == m->slot_size && (m->slot_size % 4) == 0, "dec_channels[0] must equal slot_size");
  SF_REQUIRE(m->pos_table && m->out_w && m->out_b, "null decoder weight");
  int size = m->dec_res;
  for (int i = 0; i < m->dec_layers; ++i) {
    SF_REQUIRE(m->deconv_w[i] != nullptr && m->dec_strides[i] >= 1 && (m->dec_channels[i + 1] % 4) == 0, "bad deconv layer");
    size *= m->dec_strides[i];
  }
  SF_REQUIRE(size == m->resolution, "decoder output size does not match the resolution (savi.py:279-284)");
  SF_REQUIRE(ws_bytes >= sf_savi_decode_workspace_bytes(m, F), "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int N = m->num_slots, D = m->slot_size, res = m->resolution, HW = res * res;
  const int Fc = dec_chunk(m, F);
  SfArena bp(ws, ws_bytes);
  const DecodeWs dw = dec_ws_take(bp, m, F);
  float *bufA = dw.bufA, *bufB = dw.bufB, *dec = dw.dec;
  unsigned* slot_max = dw.slot_max;
  if (!bp.ok) return sf_set_err(-1, "workspace too small", __FILE__, __LINE__);
  const bool bf3 = sf_get_precision() == 1;
  const int nl = m->dec_layers, Cl = m->dec_channels[nl];
  for (int f0 = 0; f0 < F; f0 += Fc) {
    const int nf = (F - f0 < Fc) ? (F - f0) : Fc, R = nf * N;
    float* cur = bufA;
    float* nxt = bufB;
    int hin = m->dec_res;
    bool head_done = false;
    for (int i = 0; i < nl; ++i) {
      const int Ci = m->dec_channels[i], Co = m->dec_channels[i + 1], sd = m->dec_strides[i];
      const bool last = i == nl - 1;
      int rc = 1;
      if (i == 0) {
        if (m->l0_weff && m->l0_posterm && sd == 2 && m->dec_ks == 5 && hin >= 2) {
          // the first layer on its broadcast input: table [R][25 Co] = slots . l0_weff^T, then the expansion (include/slotformer_hip.h)
          SF_TRY(sf_linear_ex(slots + (long long)f0 * N * D, sf_rows(D), m->l0_weff, nullptr, nullptr, nullptr, 0.f, nullptr, sf_rows(25 * Co), 0,
                              nxt, sf_rows(25 * Co), R, 25 * Co, D, 0, st));
          SF_TRY(sf_decode_l0_expand_f32(nxt, m->l0_posterm, cur, R, hin, Co, st));
          hin *= sd;
          continue;
        }
        SF_TRY(sf_slot_broadcast_f32(slots + (long long)f0 * N * D, m->pos_table, cur, R, m->dec_res * m->dec_res, D, st));
      }
      if (bf3 && sd == 2 && m->deconv_w_frag[i]) {
        // parity-class kernel with streamed weight fragments; on the last layer with the 1x1 head in its epilogue (deconv_s2.hip)
        const bool head = last && hin == 64 && Cl == 64;
        rc = sf_deconv5x5s2_ex(cur, m->deconv_w_frag[i], m->deconv_b[i], head ? m->out_w : nullptr, head ? m->out_b : nullptr,
                               head ? dec : nxt, R, hin, hin, Ci, Co, m->dec_ks, sd, 1, st);
        if (rc < 0 || rc > 1) return rc;
        if (rc == 0 && head) head_done = true;
      }
      if (rc == 1 && bf3 && sd == 1 && last && m->deconv_w_frag[i] && hin == 64) {
        // stride-1 last layer (the 64 x 64 configurations): the encoder's 4-row-tile convolution on the flipped kernel, 1x1 head in the epilogue
        rc = sf_conv5x5_rows4_head_ex(cur, m->deconv_w_frag[i], m->deconv_b[i], m->out_w, m->out_b, dec, R, hin, hin, Ci, Co, m->dec_ks, st);
        if (rc < 0 || rc > 1) return rc;
        if (rc == 0) head_done = true;
      }
      if (rc == 1) {
        if (sd == 1 && m->deconv_w_flipped[i])   // = convolution with the flipped kernel (halo-resident 5x5 path)
          SF_TRY(sf_conv2d_nhwc_f32(cur, m->deconv_w_flipped[i], m->deconv_b[i], nullptr, nxt, R, hin, hin, Ci, Co, m->dec_ks, 1, st));
        else
          SF_TRY(sf_conv_transpose2d_nhwc_f32(cur, m->deconv_w[i], m->deconv_b[i], nxt, R, hin, hin, Ci, Co, m->dec_ks, sd, 1, st));
      }
      hin *= sd;
      float* tmp = cur;
      cur = nxt;
      nxt = tmp;
    }
    if (!head_done)
      SF_TRY(sf_linear_ex(cur, sf_rows(Cl), m->out_w, m->out_b, nullptr, nullptr, 0.f, nullptr, sf_rows(4), 0, dec,
                          sf_rows(4), R * HW, 4, Cl, 0, st));
    SF_TRY(sf_decode_combine_seg_f32(dec, recon_combined + (long long)f0 * 3 * HW,
                                     recons ? recons + (long long)f0 * N * 3 * HW : nullptr,
                                     masks ? masks + (long long)f0 * N * HW : nullptr, seg_i64 ? seg_i64 + (long long)f0 * HW : nullptr,
                                     seg_u8 ? seg_u8 + (long long)f0 * HW : nullptr, fg_thre, slot_max, nf, N, HW, st));
  }
  return 0;
}

}  // extern "C"

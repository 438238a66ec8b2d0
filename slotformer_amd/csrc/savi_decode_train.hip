// The SAVi spatial-broadcast decoder under autograd, data gradient only: what the image term of
// SlotFormer's training loss (slotformer.py:313-326, `use_img_recon_loss`) back-propagates through -- the decoder is
// frozen there (slotformer.py:203-210), so no weight gradients are needed.
//
//   forward  (savi.py:504-525): broadcast slots over the dec_res x dec_res grid + position table -> ConvTranspose2d+ReLU
//            stack -> 1x1 head -> masks = softmax over slots, recon = sum_n rgb_n * mask_n.  Every layer output is kept.
//   backward: head / recombination adjoint (one kernel), then per layer ReLU mask + the adjoint of the transposed
//            convolution, which is a plain strided convolution of the gradient with the same weights
//            (sf_conv2d_nhwc_strided_ex on the GEMM core's im2col loader), then the sum over the broadcast grid.
#include "../../include/slotformer_hip.h"
#include "sf_internal.h"
#include "train_blocks.h"
#include "sf_arena.h"

// d_dec [F*N, HW, 4] from d_recon [F, 3, HW]:  d_rgb_n = m_n d_recon;  d_alpha_n = m_n (rgb_n.d_recon - sum_k m_k rgb_k.d_recon)
__global__ __launch_bounds__(256) void decode_combine_bwd_kernel(const float* __restrict__ dec, const float* __restrict__ d_recon,
                                                                 float* __restrict__ d_dec, int F, int N, int HW) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)F * HW) return;
  const int pix = idx % HW;
  const long long f = idx / HW;
  float g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) g[c] = d_recon[(f * 3 + c) * HW + pix];
  float mx = -INFINITY;
  for (int n = 0; n < N; ++n) mx = fmaxf(mx, dec[((f * N + n) * HW + pix) * 4 + 3]);
  float sum = 0.f, dot = 0.f;
  for (int n = 0; n < N; ++n) {
    const f32x4 v = *(const f32x4*)(dec + ((f * N + n) * HW + pix) * 4);
    const float e = expf(v[3] - mx);
    sum += e;
    dot += e * (v[0] * g[0] + v[1] * g[1] + v[2] * g[2]);
  }
  const float inv = 1.f / sum;
  dot *= inv;
  for (int n = 0; n < N; ++n) {
    const f32x4 v = *(const f32x4*)(dec + ((f * N + n) * HW + pix) * 4);
    const float m = expf(v[3] - mx) * inv;
    f32x4 o;
    o[0] = m * g[0]; o[1] = m * g[1]; o[2] = m * g[2];
    o[3] = m * ((v[0] * g[0] + v[1] * g[1] + v[2] * g[2]) - dot);
    *(f32x4*)(d_dec + ((f * N + n) * HW + pix) * 4) = o;
  }
}

// d_slots[r][c] = sum_p d_x[r][p][c]   (adjoint of the spatial broadcast; the position table is a constant)
__global__ __launch_bounds__(256) void broadcast_bwd_kernel(const float* __restrict__ dx, float* __restrict__ d_slots, int P, int D) {
  const int r = blockIdx.x;
  for (int c = threadIdx.x; c < D; c += 256) {
    float a = 0.f;
    for (int p = 0; p < P; ++p) a += dx[((long long)r * P + p) * D + c];
    d_slots[(long long)r * D + c] = a;
  }
}

// head weight gradient: part[g][j][c] = sum over the rows of chunk g of d_dec[m][j] * act[m][c]   (j < 4, c < Cl <= 64)
__global__ __launch_bounds__(256) void head_grad_partial_kernel(const float* __restrict__ d_dec, const float* __restrict__ act,
                                                                float* __restrict__ part, long long rows, int rpg, int Cl) {
  __shared__ float red[4][4][64];
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * rpg, r1 = r0 + rpg < rows ? r0 + rpg : rows;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < Cl)
    for (long long r = r0 + rl; r < r1; r += 4) {
      const f32x4 d = *(const f32x4*)(d_dec + r * 4);
      const float x = act[r * Cl + c];
      a[0] += d[0] * x; a[1] += d[1] * x; a[2] += d[2] * x; a[3] += d[3] * x;
    }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[rl][j][c] = a[j];
  __syncthreads();
  if (rl == 0 && c < Cl)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      part[((long long)blockIdx.x * 4 + j) * Cl + c] = (red[0][j][c] + red[1][j][c]) + (red[2][j][c] + red[3][j][c]);
}
__global__ __launch_bounds__(256) void head_grad_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int G, int n) {
  const int i = threadIdx.x;
  if (i >= n) return;
  float a = 0.f;
  for (int g = 0; g < G; ++g) a += part[(long long)g * n + i];
  out[i] = a;
}

// The head block of the backward: d_recon [F,3,HW] -> d_dec [F*N,HW,4] (recombination + softmax adjoint), the 1x1 head's weight [4,Cl] and bias [4]
// gradients (optional), and d_act [F*N*HW,Cl] = d_dec . W_out gated by act > 0 (the ReLU of the last transposed conv; the GEMM core wants the
// transpose of W_out [4,Cl] as its weight operand).  wout_t [4*Cl], partial [HEAD_PARTIAL_FLOATS]: scratch.
static constexpr size_t HEAD_PARTIAL_FLOATS = sf_colsum_partial_floats(256);   // bias column sums, head partials
static int head_bwd(const float* dec, const float* d_recon, const float* act, const float* out_w, float* d_dec, float* d_act, float* d_out_w,
                    float* d_out_b, int F, int N, int HW, int Cl, float* wout_t, float* partial, hipStream_t st) {
  const long long rows = (long long)F * N * HW;
  {
    const long long total = (long long)F * HW;
    hipLaunchKernelGGL(decode_combine_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dec, d_recon, d_dec, F, N, HW);
    SF_CHECK_LAUNCH();
  }
  if (d_out_w) {
    int G = SF_GRAD_MAX_GROUPS;
    const int rpg = (int)((rows + G - 1) / G);
    G = (int)((rows + rpg - 1) / rpg);
    hipLaunchKernelGGL(head_grad_partial_kernel, dim3(G), dim3(256), 0, st, d_dec, act, partial, rows, rpg, Cl);
    SF_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_grad_reduce_kernel, dim3(1), dim3(256), 0, st, partial, d_out_w, G, 4 * Cl);
    SF_CHECK_LAUNCH();
  }
  if (d_out_b) SF_TRY(sf_grad_bias_ex(d_dec, d_out_b, rows, 4, partial, st));
  SF_TRY(sf_transpose_ex(out_w, wout_t, 4, Cl, st));
  return sf_linear_masked_ex(d_dec, wout_t, act, 1.f, d_act, rows, Cl, 4, st);
}

namespace {
struct DecWs {
  float* act[9];   // act[0]: broadcast input, act[l+1]: output of transposed conv l (post-ReLU)
  float *dec, *ga, *gb, *wout_t, *partial, *dtab;
  float* wf;       // fragment-ordered copy of a stride-1 64 -> 64 layer's weights (forward, then backward-data) for conv_rows4.hip
  size_t bytes;
};
constexpr size_t WS_SLACK = 256;   // bytes a caller's workspace holds beyond either carve of this file

DecWs carve(const sf_savi_decoder* m, int F, void* ws) {
  DecWs w;
  memset(&w, 0, sizeof(w));
  SfArena ar(ws);
  const size_t R = (size_t)F * m->num_slots;
  int h = m->dec_res;
  size_t gmax = R * h * h * m->dec_channels[0];
  w.act[0] = ar.take(gmax);
  for (int l = 0; l < m->dec_layers; ++l) {
    h *= m->dec_strides[l];
    const size_t n = R * h * h * m->dec_channels[l + 1];
    w.act[l + 1] = ar.take(n);
    gmax = n > gmax ? n : gmax;
  }
  w.dec = ar.take(R * h * h * 4);
  w.ga = ar.take(gmax);
  w.gb = ar.take(gmax);
  w.wout_t = ar.take((size_t)4 * m->dec_channels[m->dec_layers]);
  {
    size_t pf = HEAD_PARTIAL_FLOATS;
    for (int l = 0; l < m->dec_layers; ++l) {
      const size_t a = sf_conv_wgrad_partial_floats(m->dec_channels[l], m->dec_ks);
      pf = a > pf ? a : pf;
    }
    w.partial = ar.take(pf);
  }
  w.dtab = ar.take((size_t)m->dec_res * m->dec_res * m->slot_size);
  w.wf = ar.take((sf_conv_frag_bytes(64, 64, 5) + 3) / 4);
  w.bytes = ar.bytes();
  return w;
}

// the scratch of the head backward alone (sf_savi_decode_head_bwd_f32)
struct HeadWs { float *wout_t, *partial; size_t bytes; };
HeadWs head_carve(int Cl, void* ws) {
  SfArena ar(ws);
  float* wout_t = ar.take((size_t)4 * Cl);
  return HeadWs{wout_t, ar.take(HEAD_PARTIAL_FLOATS), ar.bytes()};
}

int check(const sf_savi_decoder* m, int F) {
  SF_REQUIRE(m, "null model");
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
  return 0;
}
}  // namespace

extern "C" {

size_t sf_savi_decode_train_workspace_bytes(const sf_savi_decoder* m, int F) {
  if (check(m, F) != 0) return 0;
  return carve(m, F, nullptr).bytes + WS_SLACK;
}

int sf_savi_decode_train_fwd_f32(const sf_savi_decoder* m, const float* slots, float* recon_combined, float* recons, float* masks,
                                 int F, void* ws, size_t ws_bytes, void* stream) {
  SF_TRY(check(m, F));
  SF_REQUIRE(slots && recon_combined && ws, "null pointer");
  const DecWs w = carve(m, F, ws);
  SF_REQUIRE(w.bytes + WS_SLACK <= ws_bytes, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int N = m->num_slots, D = m->slot_size, R = F * N, HW = m->resolution * m->resolution;
  SF_TRY(sf_slot_broadcast_f32(slots, m->pos_table, w.act[0], R, m->dec_res * m->dec_res, D, st));
  int hin = m->dec_res;
  for (int l = 0; l < m->dec_layers; ++l) {
    if (m->dec_strides[l] == 1 && m->deconv_w_flipped[l]) {   // = convolution with the flipped kernel (4-row-tile / halo-resident 5x5 paths)
      // the 4-row-tile kernel on a fragment-ordered copy of the OHWI weights where it applies (conv_rows4.hip: the same products in the same order)
      int rc = sf_conv5x5_rows4_ohwi_ex(w.act[l], m->deconv_w_flipped[l], w.wf, m->deconv_b[l], nullptr, w.act[l + 1], R, hin, hin,
                                        m->dec_channels[l], m->dec_channels[l + 1], m->dec_ks, 1, st);
      if (rc == 1)
        rc = sf_conv2d_nhwc_f32(w.act[l], m->deconv_w_flipped[l], m->deconv_b[l], nullptr, w.act[l + 1], R, hin, hin, m->dec_channels[l],
                                m->dec_channels[l + 1], m->dec_ks, 1, st);
      SF_TRY(rc);
    } else
      SF_TRY(sf_conv_transpose2d_nhwc_f32(w.act[l], m->deconv_w[l], m->deconv_b[l], w.act[l + 1], R, hin, hin, m->dec_channels[l],
                                          m->dec_channels[l + 1], m->dec_ks, m->dec_strides[l], 1, st));
    hin *= m->dec_strides[l];
  }
  const int Cl = m->dec_channels[m->dec_layers];
  SF_TRY(sf_linear_ex(w.act[m->dec_layers], sf_rows(Cl), m->out_w, m->out_b, nullptr, nullptr, 0.f, nullptr, sf_rows(4), 0, w.dec,
                      sf_rows(4), R * HW, 4, Cl, 0, st));
  return sf_decode_combine_f32(w.dec, recon_combined, recons, masks, F, N, HW, st);
}

int sf_savi_decode_train_bwd_f32(const sf_savi_decoder* m, const float* const* deconv_w_bwd, const float* d_recon, float* d_slots,
                                 const float* pos_grid, const sf_savi_decoder_grads* g_out, int F, void* ws, size_t ws_bytes,
                                 void* stream) {
  SF_TRY(check(m, F));
  SF_REQUIRE(deconv_w_bwd && d_recon && d_slots && ws, "null pointer");
  SF_REQUIRE(g_out == nullptr || pos_grid != nullptr, "weight gradients need the position grid");
  if (g_out)
    for (int l = 0; l < m->dec_layers; ++l)
      SF_REQUIRE(m->dec_channels[l + 1] == 64 && m->dec_channels[l] % 64 == 0 && m->dec_channels[m->dec_layers] <= 64,
                 "decoder weight gradients need 64-channel layers (the reference decoder)");
  const DecWs w = carve(m, F, ws);
  SF_REQUIRE(w.bytes + WS_SLACK <= ws_bytes, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int N = m->num_slots, D = m->slot_size, R = F * N, HW = m->resolution * m->resolution, L = m->dec_layers;
  const int Cl = m->dec_channels[L];
  // head / recombination adjoint: w.gb = d_dec, w.ga = the gradient w.r.t. the pre-activation output of the last transposed conv
  SF_TRY(head_bwd(w.dec, d_recon, w.act[L], m->out_w, w.gb, w.ga, g_out ? g_out->out_w : nullptr, g_out ? g_out->out_b : nullptr, F, N, HW, Cl,
                  w.wout_t, w.partial, st));
  float* g = w.ga;   // gradient w.r.t. the pre-activation output of layer l
  float* o = w.gb;
  int h = m->resolution;
  for (int l = L - 1; l >= 0; --l) {
    SF_REQUIRE(deconv_w_bwd[l] != nullptr, "null backward weight");
    if (g_out) {   // transposed-conv weight [C_l, C_{l+1}, k, k] and bias: A = the layer input, X = this gradient on the finer grid
      const int hin = h / m->dec_strides[l];
      SF_TRY(sf_grad_bias_ex(g, g_out->deconv_b[l], (long long)R * h * h, m->dec_channels[l + 1], w.partial, st));
      SF_TRY(sf_conv_wgrad_ex(w.act[l], m->dec_channels[l], hin, hin, g, h, h, m->dec_strides[l], m->dec_ks, (long long)R * hin * hin,
                              g_out->deconv_w[l], w.partial, st));
    }
    // adjoint of the transposed conv = strided conv of the gradient; its output is gated by the ReLU of the layer below
    // (act[0] is the broadcast input: no ReLU there)
    int rc = 1;
    if (m->dec_strides[l] == 1 && l >= 1)
      rc = sf_conv5x5_rows4_ohwi_ex(g, deconv_w_bwd[l], w.wf, nullptr, w.act[l], o, R, h, h, m->dec_channels[l + 1], m->dec_channels[l], m->dec_ks, 2,
                                    st);
    if (rc == 1)
      rc = sf_conv2d_nhwc_strided_ex(g, deconv_w_bwd[l], nullptr, o, R, h, h, m->dec_channels[l + 1], m->dec_channels[l], m->dec_ks,
                                     m->dec_strides[l], 0, st, l >= 1 ? w.act[l] : nullptr);
    SF_TRY(rc);
    h /= m->dec_strides[l];
    float* t = g;
    g = o;
    o = t;
  }
  if (g_out) SF_TRY(sf_pos_dense_grad_ex(g, R, m->dec_res * m->dec_res, D, pos_grid, g_out->pos_w, g_out->pos_b, w.dtab, st));
  hipLaunchKernelGGL(broadcast_bwd_kernel, dim3(R), dim3(256), 0, st, g, d_slots, m->dec_res * m->dec_res, D);
  SF_CHECK_LAUNCH();
  return 0;
}

size_t sf_savi_decode_head_bwd_workspace_bytes(int Cl) {
  if (Cl < 4 || Cl > 64 || Cl % 4) return 0;
  return head_carve(Cl, nullptr).bytes + WS_SLACK;
}

int sf_savi_decode_head_bwd_f32(const float* dec, const float* d_recon, const float* act, const float* out_w, float* d_dec, float* d_act,
                                float* d_out_w, float* d_out_b, int F, int N, int HW, int Cl, void* ws, size_t ws_bytes, void* stream) {
  SF_REQUIRE(dec && d_recon && act && out_w && d_dec && d_act && ws, "sf_savi_decode_head_bwd_f32: null pointer");
  SF_REQUIRE(Cl >= 4 && Cl <= 64 && Cl % 4 == 0, "sf_savi_decode_head_bwd_f32: Cl must be a multiple of 4, at most 64");
  SF_REQUIRE(F >= 1 && N >= 1 && HW >= 1 && (long long)F * N * HW < (1LL << 31), "sf_savi_decode_head_bwd_f32: bad shape");
  SF_REQUIRE(((uintptr_t)dec & 15) == 0 && ((uintptr_t)d_dec & 15) == 0 && ((uintptr_t)act & 15) == 0,
             "sf_savi_decode_head_bwd_f32: dec, d_dec and act must be 16-byte aligned");
  SF_REQUIRE(sf_savi_decode_head_bwd_workspace_bytes(Cl) <= ws_bytes, "sf_savi_decode_head_bwd_f32: workspace too small");
  const HeadWs w = head_carve(Cl, ws);
  return head_bwd(dec, d_recon, act, out_w, d_dec, d_act, d_out_w, d_out_b, F, N, HW, Cl, w.wout_t, w.partial, (hipStream_t)stream);
}

}  // extern "C"

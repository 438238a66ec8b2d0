// Gradient building blocks every training node shares (train_blocks.hip unless noted): weight gradients as one contraction over all rows, bias and
// LayerNorm-parameter gradients as two-stage column sums, LayerNorm / ReLU backward, transposes.  Each takes the caller's `partial` scratch.
#pragma once
#include "../../include/slotformer_hip.h"
#include "sf_common.h"

// The two-stage reductions split their rows over at most this many groups; stage 1 writes one [2][width] record per group (column sums use half).
constexpr int SF_GRAD_MAX_GROUPS = 512;
// Column-sum / LayerNorm partial floats at width w: the group records, and (ln_scratch = 1) one more [2][w] record behind them, which
// sf_grad_ln_ex reduces into when its destinations are not 16-byte aligned.
constexpr size_t sf_colsum_partial_floats(size_t w, int ln_scratch = 1) { return (size_t)(SF_GRAD_MAX_GROUPS + ln_scratch) * 2 * w; }
// number of row splits of a weight-gradient contraction: enough workgroups to fill the chip a few times over
inline int tn_splits(long long rows, int N, int K) {
  const long long tiles = (long long)(N / 64) * (K / 64);
  long long s = (SF_GRAD_MAX_GROUPS + tiles - 1) / tiles;
  const long long max_s = (rows + 63) / 64;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  return (int)s;
}
// ... of the edge-tile form (N, K multiples of 4): tiles counted rounding up
inline int tn_splits_edge(long long rows, int N, int K) {
  const long long tiles = (long long)((N + 63) / 64) * ((K + 63) / 64);
  long long s = (SF_GRAD_MAX_GROUPS + tiles - 1) / tiles;
  const long long max_s = (rows + 63) / 64;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  return (int)s;
}
// floats of `partial` that serve sf_grad_weight_ex at (rows, N, K) and the column-sum / LayerNorm blocks up to width max(N, K)
size_t sf_grad_partial_floats(long long rows, int N, int K);
int sf_grad_weight_ex(const float* Y, const float* X, float* dW, long long rows, int N, int K, float* partial, hipStream_t st);
size_t sf_grad_partial_edge_floats(long long rows, int N, int K);
int sf_grad_weight_edge_ex(const float* Y, const float* X, float* dW, long long rows, int N, int K, float* partial, hipStream_t st);
int sf_grad_bias_ex(const float* Y, float* db, long long rows, int n, float* partial, hipStream_t st);
int sf_grad_ln_ex(const float* x, const float* dy, float* dgamma, float* dbeta, long long rows, int D, float eps, float* partial,
                  hipStream_t st);
int sf_ln_bwd_ex(const float* x, const float* dy, const float* gamma, const float* dres, float* out, long long rows, int D,
                 float eps, hipStream_t st);
// the same with out2 (may be NULL) = out pushed through the dropout of the block below it (mask of site seed sseed2; thresh 0: a plain copy)
int sf_ln_bwd_dropout_ex(const float* x, const float* dy, const float* gamma, const float* dres, float* out, float* out2, uint32_t sseed2,
                         uint32_t thresh, float inv_keep, long long rows, int D, float eps, hipStream_t st);
int sf_transpose_ex(const float* in, float* out, int R, int Cn, hipStream_t st);
int sf_relu_bwd_ex(float* dh, const float* h, long long n, hipStream_t st);
// dh = hdn > 0 ? dh * inv_keep : 0 (hdn: the hidden rows behind ReLU and dropout)
int sf_relu_dropout_bwd_ex(float* dh, const float* hdn, long long n, float inv_keep, hipStream_t st);

// blocks that live with the kernels they wrap
// savi_features_train.hip:
int sf_conv_wgrad_ex(const float* A, int CA, int H, int W, const float* X, int Hx, int Wx, int s, int ks, long long rows,
                     float* out_oihw, float* partial, hipStream_t st);
int sf_pos_dense_grad_ex(const float* d, int F, int HW, int C, const float* grid, float* dw, float* db, float* dtab, hipStream_t st);
// gemm.hip:
int sf_conv2d_nhwc_strided_ex(const float* in, const float* w_packed, const float* bias, float* out, int F, int Hin, int Win,
                              int Cin, int Cout, int ks, int stride, int relu, hipStream_t stream, const float* relu_mask = nullptr);
int sf_linear_masked_ex(const float* A, const float* W, const float* mask, float scale, float* C, long long M, int N, int K,
                        hipStream_t stream);
// the token rows of the PHYRE readout (phyre_readout.hip: ph_embed_kernel) for its training forward; arguments validated by the caller
int sf_phyre_embed_ex(const float* slots, long long stride_v, long long stride_t, int V, const int* video_index, const int* sel, const float* in_proj_w,
                      const float* in_proj_b, const float* enc_t_pe, const float* cls, float* x, int B, int T, int N, int C, hipStream_t st);
// aloe.hip: the token rows of the Aloe reasoner (sequences b >= mc_from are multiple choice) and the attention launch of a training layer (every row a
// query; lse [B][heads][L]; site-0 dropout on P when thresh != 0); arguments validated by the caller
int sf_aloe_embed_ex(const sf_aloe* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index, const int* start,
                     int frame_offset, const int* tokens, int mc_from, float* x, int B, hipStream_t st);
int sf_aloe_attn_train_ex(const float* qkv, const unsigned char* pad, float* out, float* lse, int B, int L, int text0, int text_len, int d, int heads,
                          uint32_t sseed, uint32_t thresh, float inv_keep, hipStream_t st);
// steve_decoder.hip:
int sf_slate_flash_train_ex(const float* q, const float* k, const float* v, float* out, float* lse, int ldq, int ldk, int ldv, int ldo,
                            long long q_bs, long long k_bs, long long v_bs, long long o_bs, int B, int L, int num_heads, int head_dim,
                            unsigned drop_seed, unsigned drop_thresh, float drop_scale, hipStream_t st);

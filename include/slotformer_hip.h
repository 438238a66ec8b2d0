/* slotformer_hip.h -- C ABI of libslotformer_hip.so (gfx950 / MI355X only).
 *
 * The reference (pairlab/SlotFormer) has NO native/FFI boundary: its hot path is Python
 * nn.Modules calling ATen/cuDNN.  This header is therefore the boundary a maintainer would
 * bind (ctypes); every entry point cites the reference call site whose
 * arithmetic it replaces (file:line under the reference tree).
 *
 * Conventions: extern "C"; int return (0 = ok, <0 = argument error, >0 = hipError_t);
 * sf_last_error_string() describes the last failure on the calling thread; every pointer is a
 * DEVICE pointer to row-major contiguous fp32 unless stated; the caller owns every buffer
 * (inputs, outputs, workspace -- query *_workspace_bytes()); `stream` is a hipStream_t passed
 * as void*; calls are asynchronous on that stream, re-entrant, never synchronise, and never
 * allocate device memory.
 */
#ifndef SLOTFORMER_HIP_H
#define SLOTFORMER_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

int sf_version(void);
const char* sf_last_error_string(void);

/* Matrix-arithmetic mode of every GEMM/conv kernel: 1 (default) = split-bf16 ("bf16x3": each f32 operand
 * = hi + lo bf16, hi*hi + hi*lo + lo*hi on bf16 MFMA with f32 accumulation, ~2^-17 relative per operand);
 * 0 = exact f32 MFMA (bitwise an fmaf chain); 2 = single-pass bf16 (hi*hi only, f32 accumulation, fp32 storage and master
 * weights) in the GEMM / convolution / weight-gradient cores -- the AMP-bf16 policy of the training path (row N1); kernels
 * without a single-pass variant keep mode 1.  Environment SF_PRECISION=f32 | bf16 selects 0 | 2 at load time. */
int sf_get_precision(void);
int sf_set_precision(int mode);

/* Optional per-kernel-class HIP-event timer (bench.py roofline): events bracket every launch of a
 * class on the launch stream while enabled (never during hipGraph capture).  Classes: 0 conv
 * NHWC implicit GEMM, 1 first conv, 2 linear, 3 slot-attention iteration, 4 slot update, 5 attention (incl. the fused
 * attention + out-proj kernel), 6 fused FFN, 7 seam launch, 8 the decoder's fragment-weight transposed convolutions / head-fused last layer.
 * sf_profile_read sums elapsed ms, launches and algorithmic work (FLOP, or bytes for class 3)
 * since the last read. */
int sf_profile_enable(int class_mask); /* bit c enables class c; 0 disables */
/* Seam launches of the rollout (last FFN + step boundary of step s and the first attention of step s+1 in one grid): on by
 * default (SF_SEAM_FUSED=0 in the environment: off).  They shorten the critical path of ONE rollout; when several rollouts
 * share the same CUs (pipeline partition 'pair') the spinning consumers waste CU time and the graphs are captured with it off. */
int sf_set_seam_fused(int on);
int sf_get_seam_fused(void);
/* 64 rows per workgroup in the chunk-partial FFN launches of the rollout (two 32-row tiles against one load of the weight
 * chunk: 40 % less CU time per launch, a slightly longer launch).  Off by default; the 'pair' pipeline, whose rollout CUs are
 * shared by two rollouts and therefore throughput-bound, captures its graphs with it on.  Bit-identical results either way. */
int sf_set_ffn_rows64(int on);
int sf_get_ffn_rows64(void);
int sf_profile_sample(int every);      /* bracket every `every`-th launch of an enabled class only (default 1: all) */
int sf_profile_read(int kernel_class, double* total_ms, long long* launches, double* work);

/* ---- building blocks ------------------------------------------------------------------ */

/* C[M,N] = act( LN?(A)[M,K] @ W[N,K]^T + bias ) + residual.   nn.Linear / F.layer_norm call
 * sites: savi.py:66-70,80,245-250; predictor.py:58-73; slotformer.py:115,121; torch
 * TransformerEncoderLayer linears.  W is the torch weight as stored ([out,in]).  ln_gamma/
 * ln_beta (both or neither) fuse a LayerNorm over K into the A load; residual may be NULL. */
int sf_linear_f32(const float* A, int lda, const float* W, const float* bias, const float* ln_gamma,
                  const float* ln_beta, float ln_eps, const float* residual, int ldr, float* C, int ldc,
                  int M, int N, int K, int relu, void* stream);
/* Which tile configuration of csrc/gemm.hip (the ids of launch_by_id) sf_linear_f32 launches for a shape: the host rule and nothing else, no
 * device work.  precision 0, 1 or 2 is taken as given (ids < 100: exact-f32 tiles, ids >= 100: split-bf16 tiles, which mode 2 shares); -1 = the
 * calling thread's current precision (sf_get_precision).  The rule's id whatever SF_DBG=gemmcfg forces.  < 0: bad arguments (M < 0, N <= 0,
 * K <= 0, K % 4 != 0, any other precision).  For tests and tools that have to know which kernel a shape runs. */
int sf_linear_config(int M, int N, int K, int precision);

/* nn.LayerNorm over the last dim (savi.py:41,50,66; predictor.py:57). */
int sf_layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int rows, int D,
                     float eps, void* stream);

/* First encoder conv (savi.py:231-239, i == 0): NCHW image, frame f at img + f*frame_stride
 * floats; weight [Cout,Cin,ks,ks]; padding ks/2; output NHWC [F,Ho,Wo,Cout]; optional `add`
 * table [Ho*Wo,Cout] added after the activation. */
int sf_conv2d_nchw_in_f32(const float* img, long long frame_stride, const float* weight, const float* bias,
                          const float* add, float* out, int F, int Cin, int Hin, int Win, int Cout, int ks,
                          int stride, int relu, void* stream);
/* The same convolution with the frames in groups, as the batched encode launches it for all time steps of a [B][T] clip at once: output frame i reads
 * the image at img + (i % fgroup) * frame_stride + (i / fgroup) * group_stride floats.  Only the shapes of the persistent kernel (csrc/conv_first.hip:
 * 3 -> 64 channels, 5 x 5, 64 x 64 at stride 1 or 128 x 128 at stride 2; split-bf16 mode); anything else is an error, there is no generic grouped
 * path.  The kernel walks its tiles on 2 * sf_stream_cus(stream) workgroups. */
int sf_conv2d_nchw_in_grouped_f32(const float* img, long long frame_stride, int fgroup, long long group_stride, const float* weight,
                                  const float* bias, const float* add, float* out, int F, int Cin, int Hin, int Win, int Cout, int ks,
                                  int stride, int relu, void* stream);

/* Encoder convs i > 0 (savi.py:231-239): stride 1, padding ks/2, NHWC in -> NHWC out,
 * w_packed [Cout,ks,ks,Cin] (sf_pack_conv_weight_f32); `add` as above (used for the soft
 * position embedding, utils.py:60-63 / savi.py:370).
 * relu: 0 none, 1 ReLU, 2 = the backward-data form of training: `add` [F,H,W,Cout] is then laid out like `out` (one mask PER FRAME, not a table) and
 * gates it, out = add > 0 ? conv + bias : +0.0.  The same three values hold for sf_conv5x5_frag_f32 below. */
int sf_conv2d_nhwc_f32(const float* in, const float* w_packed, const float* bias, const float* add, float* out,
                       int F, int H, int W, int Cin, int Cout, int ks, int relu, void* stream);
int sf_pack_conv_weight_f32(const float* w_oihw, float* w_ohwi, int Cout, int Cin, int ks, void* stream);
/* 64 -> 64 channel 5 x 5 convolutions on a 64-pixel-wide grid: w_ohwi (above) -> split-bf16 copy in MFMA-fragment order,
 * sf_conv_frag_bytes(64, 64, 5) bytes; sf_conv5x5_frag_f32 is sf_conv2d_nhwc_f32 for that shape on the fragment copy (H % 4 == 0,
 * split-bf16 mode; csrc/conv_rows4.hip).  relu / add as sf_conv2d_nhwc_f32.  The first 409,600 bytes are the A operands of v_mfma_f32_16x16x32_bf16:
 * 16-byte piece ((((tap * 2 + kh) * 2 + cb) * 2 + a) * 2 + plane) * 64 + lane = w[cb * 32 + 16 a + (lane & 15)][tap][kh * 32 + 8 (lane >> 4) + 0 .. 7],
 * plane 0 bf16(w), plane 1 bf16(w - plane 0); behind them the single-fp16 copy of the opt-in arithmetic below. */
/* Per-pixel chain of the SAVi encoder up to the normalised Slot-Attention inputs (64 -> 128 -> 128 channels; savi.py:245-250, 66-70):
 * feat [M][128] = LN(fc2(relu(fc1(LN(x))))), x [M][64]; torch-layout weights w1 [128][64], w2 [128][128].  form 0: one 128-pixel tile per
 * workgroup, weights through LDS; form 1: weights resident in registers, four tiles per workgroup; form 2 (the one the encode uses): the same on
 * 64-pixel tiles with 256 threads, two workgroups per CU (csrc/pixel_mlp.hip).  Same bits.  form 3: the pixel-stationary kernel (sf_set_pixel_tok
 * below; another summation order), on at most sf_stream_cus(stream) workgroups.  form 4: `feat` is M rows of 512 bytes instead, bf16 hi | bf16 lo of
 * the 128 channels (hi = bf16(y), lo = bf16(y - hi), round to nearest even), written by the launch the encode uses for them: form 3's kernel under
 * sf_set_pixel_tok(1), form 2's under sf_set_pixel_tok(0). */
int sf_pixel_feat_f32(const float* x, const float* ln0_g, const float* ln0_b, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* ln1_g, const float* ln1_b, float* feat, int M, float eps, int form, void* stream);
size_t sf_conv_frag_bytes(int Cout, int Cin, int ks);
/* Opt-in arithmetic of the fragment-weight convolution (process-wide; default 0 = split-bf16, three MFMAs per product, like every other bf16x3
 * kernel): 1 = activations as two fp16 terms x weights rounded to ONE fp16 (2^-12 per weight), two MFMAs per product and half the weight stream.
 * A measured trade (profiles/r03_probes.txt section 14), not the path the parity numbers are quoted on.  Also SF_CONV_FP16X2=1. */
int sf_set_conv_fp16x2(int on);
int sf_get_conv_fp16x2(void);
int sf_pack_conv_frag_weights(const float* w_ohwi, void* frag, int Cout, int Cin, int ks, void* stream);
int sf_conv5x5_frag_f32(const float* in, const void* w_frag, const float* bias, const float* add, float* out, int F, int H, int W,
                        int relu, void* stream);
/* The same convolution on the same fragment copy with the WEIGHTS STATIONARY IN REGISTERS (csrc/conv_ws.hip): one four-wave workgroup per CU keeps the
 * layer's 410 KB of split-bf16 fragments in its register file and walks its share of the F * H output rows through a ring of six halo rows in LDS --
 * what the encode launches for layers i > 0 when a launch gives every CU of its stream at least four rows (savi.py:231-239).  Bit-identical to
 * sf_conv5x5_frag_f32.  Any H >= 1; relu 0 / 1; n_workgroups 0 = one per CU of the stream (sf_stream_create_cu_mask streams: their CUs), else
 * that many (any split of the rows gives the same bits). */
int sf_conv5x5_ws_f32(const float* in, const void* w_frag, const float* bias, const float* add, float* out, int F, int H, int W,
                      int relu, int n_workgroups, void* stream);

/* 64 -> 64 channel 5 x 5 stride-2 transposed convolutions (padding 2, output_padding 1: H x W -> 2H x 2W; the decoder layers of savi.py:252-293):
 * w_ohwi (sf_pack_deconv_weight_f32) -> split-bf16 copy in the kernel's consumption order, sf_deconv_frag_bytes(64, 64, 5, 2) bytes;
 * sf_deconv5x5s2_frag_f32: in [R][H][W][64] -> out [R][2H][2W][64] (+ bias, relu 0 / 1), W in {16, 32, 64}, H % (256 / W) == 0;
 * sf_deconv5x5s2_head_frag_f32 (W == 64): dec [R][2H * 2W][4] = head_w [4][64] . relu(deconv(in) + bias) + head_b [4] -- the last decoder layer with
 * the 1x1 output convolution (savi.py:286-289) in its epilogue.  Split-bf16 mode only (csrc/deconv_s2.hip). */
size_t sf_deconv_frag_bytes(int Cout, int Cin, int ks, int stride);
int sf_pack_deconv_frag_weights(const float* w_ohwi, void* frag, int Cout, int Cin, int ks, int stride, void* stream);
int sf_deconv5x5s2_frag_f32(const float* in, const void* w_frag, const float* bias, float* out, int R, int H, int W, int relu, void* stream);
int sf_deconv5x5s2_head_frag_f32(const float* in, const void* w_frag, const float* bias, const float* head_w, const float* head_b, float* dec,
                                 int R, int H, int W, void* stream);
/* First decoder layer on its broadcast input (sf_savi_decoder.l0_weff / l0_posterm): out [R][2 res][2 res][C1] = relu(table[r][class(p)] + posterm[p]),
 * table [R][25 * C1]. */
int sf_decode_l0_expand_f32(const float* table, const float* posterm, float* out, int R, int res, int C1, void* stream);

/* Decoder building blocks (savi.py:252-293,504-525).  ConvTranspose2d(k, stride, padding=k/2,
 * output_padding=stride-1) as a gather implicit GEMM: NHWC in [F,Hin,Win,Cin] -> [F,Hin*s,Win*s,Cout];
 * w_packed [Cout,ks,ks,Cin] from the torch weight [Cin,Cout,ks,ks] (sf_pack_deconv_weight_f32). */
int sf_conv_transpose2d_nhwc_f32(const float* in, const float* w_packed, const float* bias, float* out, int F,
                                 int Hin, int Win, int Cin, int Cout, int ks, int stride, int relu, void* stream);
int sf_pack_deconv_weight_f32(const float* w_iohw, float* w_ohwi, int Cin, int Cout, int ks, void* stream);
/* out[R,P,D] = slots[R,D] (broadcast over the P = r*r positions) + table[P,D]  (savi.py:512-517). */
int sf_slot_broadcast_f32(const float* slots, const float* table, float* out, int R, int P, int D, void* stream);
/* dec [F*N,HW,4] (rgb + mask logit per slot) -> masks = softmax over slots [F,N,1,H,W], recons [F,N,3,H,W],
 * recon_combined = sum_n recons*masks [F,3,H,W]  (savi.py:519-525); recons / masks may be NULL. */
int sf_decode_combine_f32(const float* dec, float* recon_combined, float* recons, float* masks, int F, int N, int HW,
                          void* stream);
/* ... followed by postproc_mask (vp_utils.py:20-41) on those masks: seg [F,H,W] = the slot with the smallest peak mask value over the frame
 * (the background) where the best mask value is below fg_thre, else the argmax over slots; as int64 (the reference's dtype) and / or
 * uint8, either may be NULL.  (The reference sets the background's score to 1 and takes the argmax, first index on ties: with fg_thre > 1 a
 * slot at 1 or above still wins, and so it does here.)  slot_max: [F * N] words of scratch.  recon_combined is always written; recons /
 * masks may be NULL. */
int sf_decode_combine_seg_f32(const float* dec, float* recon_combined, float* recons, float* masks, long long* seg_i64,
                              unsigned char* seg_u8, float fg_thre, unsigned* slot_max, int F, int N, int HW, void* stream);
/* postproc_mask (vp_utils.py:20-41) on given masks [F,N,HW] (any float values) -> seg [F,HW] int64 and / or uint8; slot_max: [F * N] words. */
int sf_postproc_mask_f32(const float* masks, long long* seg_i64, unsigned char* seg_u8, float fg_thre, unsigned* slot_max, int F, int N,
                         int HW, void* stream);

/* ---- video-prediction metrics (vp_utils.py:44-344 as test_vp.py:149-160 calls them; csrc/vp_metrics.hip) ---------------------------------
 * F = B * T frames, frame (b, t) at index b * T + t.  Every score is a double; every sum has a fixed order, so equal inputs give equal bits.
 * Bytes of workspace for the calls below on F frames of H x W (0 for a shape they reject). */
size_t sf_vp_metrics_workspace_bytes(int F, int H, int W);
/* MSE / PSNR / SSIM per frame in one pass over both clips (vp_utils.py:72-106, 323-333).  gt, pred [F,3,H,W] float32; to_rgb = 1: in the model's
 * [-1, 1] range, to_rgb_from_tensor (x * 0.5 + 0.5, clamped to [0, 1]) is applied on load; to_rgb = 0: already in [0, 1], taken as they are.  mse [F]: squared error summed over H and W, averaged over the channels.
 * psnr [F]: peak_signal_noise_ratio at data range 1 (+inf for equal frames).  ssim [F]: structural_similarity(channel_axis=0, gaussian_weights=True,
 * sigma=1.5, use_sample_covariance=False) -- 11 normalised Gaussian taps, K1 0.01, K2 0.03, the map cropped by 5 pixels and averaged over crop and
 * channels -- evaluated at data range 1, which is the same function as the reference's data range 255 on the x 255 images.  The crop equals the
 * filter radius, so no kept map pixel reads across the image edge.  Any H, W >= 11. */
int sf_vp_image_metrics_f32(const float* gt, const float* pred, double* mse, double* psnr, double* ssim, int F, int H, int W, int to_rgb,
                            void* workspace, size_t workspace_bytes, void* stream);
/* ARI / FG-ARI / mIoU per frame (vp_utils.py:114-177, 225-255).  gt_mask [F,H*W] int64; pred_mask [F,H*W] int64, or uint8 with pred_is_u8 = 1; ids
 * in [0, num_classes) for pred_mask and [0, 16) for gt_mask, num_classes <= 16.  A pixel with an id outside is left out and sets *flag to 1 (flag: one
 * device word, zeroed by the call).  tables [F,16,16] uint32 (ground truth x predicted counts; NULL: kept in the workspace), pred_boxes [F,16,4]
 * float32 or NULL (as sf_masks_to_boxes).  ari / fari [F]: adjusted_rand_index without / with ignore_background, 1 where the denominator is 0;
 * miou [F]: the maximum-weight assignment over intersect / (union + 1e-8) of the ground-truth ids 1 .. N against the predicted ids, divided by
 * N = the largest ground-truth id of the frame; NaN without a foreground pixel. */
int sf_vp_mask_metrics(const long long* gt_mask, const void* pred_mask, int pred_is_u8, unsigned* tables, float* pred_boxes, double* ari,
                       double* fari, double* miou, unsigned* flag, int F, int H, int W, int num_classes, void* workspace, size_t workspace_bytes,
                       void* stream);
/* bbox_precision_recall per frame at IoU >= ovthresh (vp_utils.py:180-222).  gt_bbox [F,N,4], pred_bbox [F,M,4] float32 as [x1,y1,x2,y2];
 * gt_pres_mask [F,N] bytes (torch.bool) selects the ground-truth rows, predicted rows count where x1 >= 0; N, M <= 64.  Greedy in ground-truth order,
 * first maximum on ties, each predicted box used once; box IoU = inter / (area_a + area_b - inter), areas (x2 - x1)(y2 - y1), in double.  ap [F] =
 * tp / predicted boxes, ar [F] = tp / present boxes; NaN for a frame without a present or without a predicted box (the reference divides by zero). */
int sf_vp_bbox_pr_f32(const float* gt_bbox, const unsigned char* gt_pres_mask, const float* pred_bbox, double* ap, double* ar, int F, int N, int M,
                      float ovthresh, void* stream);
/* masks_to_boxes (vp_utils.py:44-69): masks [F,H*W] int64 (or uint8 with is_u8 = 1) -> boxes [F,num_boxes,4] float32 [min x, min y, max x, max y] of
 * every id below num_boxes <= 16, -1 for an id without a pixel.  flag (may be NULL): set to 1 by an id outside [0, num_boxes). */
int sf_masks_to_boxes(const void* masks, int is_u8, float* boxes, unsigned* flag, int F, int H, int W, int num_boxes, void* stream);
/* out [K,T] = the mean over the B videos of per_video [K,B,T] (np.mean over the batch, vp_utils.py:88,106,222,255), summed in order. */
int sf_vp_mean_over_videos_f64(const double* per_video, double* out, int K, int B, int T, void* stream);

/* ---- LPIPS, VGG16 (the `percept_dist` of test_vp.py:21-23, 149-160: lpips.LPIPS(net='vgg'); csrc/lpips.hip) ----------------------------------
 * Thirteen 3x3 convolutions (stride 1, zero padding 1, bias, ReLU), four 2x2 max pools, and at the five taps (after relu1_2, relu2_2, relu3_3,
 * relu4_3, relu5_3) the channel-normalised squared difference under the tap's 1x1 weights, averaged over the pixels and summed over the taps.
 * Arithmetic: the first layer (3 -> 64) in f32 FMA; the other twelve on bf16 MFMA with split-bf16 operands (every f32 value = bf16 hi + bf16 lo,
 * x_lo.w_hi + x_hi.w_lo + x_hi.w_hi, f32 accumulation).  This is the same WHATEVER sf_set_precision says: the metric has one definition.
 * Every sum has a fixed order: a pair's score does not depend on its place in the batch, on `chunk` or on the other pairs; equal images give 0.
 *
 * The model: device pointers.  conv_w[0]: the first layer as f32 [27][64] (k = cin * 9 + tap); conv_w[1..12]: fragment order, a bf16 hi plane of
 * Cout * Cin * 9 elements followed by the lo plane -- both written by sf_lpips_pack_conv_weights, Cout * Cin * 9 * 4 bytes either way.  conv_b[i]:
 * the bias [Cout].  lin_w[s]: the tap's weights [C_s], C = 64, 128, 256, 512, 512.  shift, scale: [3], the input is (x - shift) / scale. */
typedef struct {
  const void* conv_w[13];
  const float* conv_b[13];
  const float* lin_w[5];
  const float* shift;
  const float* scale;
} sf_lpips_model;
/* w_oihw [Cout,Cin,3,3] f32 (torch's layout) -> packed.  Cin = 3 (Cout = 64): f32 [27][64].  Otherwise Cin, Cout in {64, 128, 256, 512}: for every
 * block ct of 32 output channels and every k-step ks = tap * (Cin / 16) + cc, 64 lanes x 8 bf16, lane l holding W[32 ct + (l & 31)][16 cc + 8 (l >> 5)
 * + 0..7][tap] -- element ((ct * 9 * Cin / 16 + ks) * 64 + l) * 8 + j of the hi plane, the lo plane (bf16 of the remainder) behind it.  The _host
 * twin takes and fills HOST memory with the same bytes. */
int sf_lpips_pack_conv_weights(const float* w_oihw, void* packed, int Cout, int Cin, void* stream);
int sf_lpips_pack_conv_weights_host(const float* w_oihw, void* packed, int Cout, int Cin);
/* Bytes of workspace for frames of H x W scored `chunk` pairs at a time (two activation buffers of 2 * chunk images at the first stage's width
 * and the tap partials); 0 for H or W below 16, chunk outside [1, 16384], or 2 * chunk * H * W * 64 >= 2^31. */
size_t sf_lpips_workspace_bytes(int H, int W, int chunk);
/* x, y [F,3,H,W] f32 -> out [F] f32, the distance of every pair.  normalize = 1 first maps [0, 1] to [-1, 1] (2 v - 1).  The frames go through
 * the network `chunk` pairs at a time, x and y of a chunk as one batch (a layer's weights are read once for both). */
int sf_lpips_f32(const sf_lpips_model* m, const float* x, const float* y, float* out, int F, int H, int W, int chunk, int normalize,
                 void* workspace, size_t workspace_bytes, void* stream);
/* scores [B,T] f32 (the out of sf_lpips_f32 on B videos of T steps) -> per_video [B,T] doubles (may be NULL) and mean [T], the mean over the videos
 * of every step, summed in the order of b. */
int sf_lpips_mean_over_videos_f32(const float* scores, double* per_video, double* mean, int B, int T, void* stream);

/* ---- ingest: the decoder's uint8 frames -> the encoder's input (base_slots/datasets/utils.py:15-43 BaseTransforms; csrc/ingest.hip) -------------
 * Source coordinates and weights are tables built on the HOST in float64, one per (H0, W0, H, W, mode): per output row and per output column the
 * first source index, the tap count and float32 weights (the kernels do no coordinate arithmetic, so they carry no float32 coordinate rounding).
 * mode 0: bilinear, align_corners=False, edge-clamped (what the reference's pinned torchvision does to a tensor); 1: the separable triangle filter of
 * F.interpolate(..., antialias=True), support max(in / out, 1) per axis; 2: nearest as F.interpolate(mode='nearest') picks it: floor(dst * in / out)
 * clamped to in - 1, evaluated like ATen with a float32 ratio.  Sizes in [1, 16384].
 * sf_ingest_tables_bytes: bytes of the table (0 for sizes or a mode it rejects).  sf_ingest_tables_host fills `tables` (HOST memory, `bytes` long);
 * the caller uploads it once and passes the device copy to the two kernels below.  Layout (32-bit words): 8 header words {magic, H0, W0, H, W, mode,
 * tapsY, tapsX}, then first[H], count[H], weight[H][tapsY] of the rows and first[W], count[W], weight[W][tapsX] of the columns (weights beyond
 * count are 0; the taps of an output sum to 1 to float32 rounding). */
size_t sf_ingest_tables_bytes(int H0, int W0, int H, int W, int mode);
int sf_ingest_tables_host(void* tables, size_t bytes, int H0, int W0, int H, int W, int mode);
/* src [F,H0,W0,3] uint8 (HWC, as decoded; any byte alignment) -> out [F,3,H,W] float32 = resize((x / 255 - mean_c) / std_c), antialias 0 / 1 = table
 * modes 0 / 1.  With a palette [K,3] uint8 (device; 1 <= K <= 256) src is [F,H0,W0] uint8 colour indices instead (datasets/phyre.py:50); an index
 * >= K takes colour K - 1.  palette NULL: K = 0.  tables: the DEVICE copy of the table for these sizes and this mode.  mean3 / std3: three HOST
 * floats each.  max_blocks: 0 = one workgroup per (frame, band of output rows); > 0 caps the grid (the workgroups loop). */
int sf_ingest_frames_u8(const unsigned char* src, const unsigned char* palette, int K, const void* tables, const float* mean3,
                        const float* std3, float* out, int F, int H0, int W0, int H, int W, int antialias, int max_blocks, void* stream);
/* BaseTransforms.process_mask: src [F,H0,W0] int64 (or uint8 with src_is_u8 = 1) -> [F,H,W] as int64 and / or uint8 (either may be NULL; ids are
 * copied, uint8 output keeps the low byte).  tables: the DEVICE copy of the mode-2 table for these sizes. */
int sf_resize_masks_nearest(const void* src, int src_is_u8, const void* tables, long long* out_i64, unsigned char* out_u8, int F, int H0,
                            int W0, int H, int W, void* stream);

/* ---- annotation masks -> ground truth (base_slots/datasets/clevrer.py:101-125 _read_masks, datasets/utils.py:46-77; csrc/rle_masks.hip) ---------
 * The run-length masks of F frames, parsed and packed on the host (slotformer_amd/annotations.py): run_ends [num_runs] uint32, the CUMULATIVE run
 * ends of every object one after the other -- run j of an object covers the column-major source indices [end[j-1], end[j]) (index x * h + y), odd j
 * is covered --; object_offsets [num_objects + 1], the first run of every object; frame_offsets [F + 1], the first object of every frame (a
 * pointer INTO a longer array selects a range of frames: the offsets are absolute).  A frame's objects beyond the 15th are ignored.  tables: the
 * DEVICE copy of the mode-2 (nearest) table of (h, w) -> (H, W), the one sf_resize_masks_nearest takes.
 * labels [F,H,W] as int64 and / or uint8 (either may be NULL): 1 + the first object of the frame, in order, that covers the pixel's source pixel, 0
 * where none does = argmax(0) over [not any(objects), objects...].  extents [F,15,5] int32: {min x, min y, max x, max y, pixels} of every object's
 * OWN resized mask (an object hidden behind an earlier one has no label pixel but keeps its extents); {-1,-1,-1,-1,0} without a pixel.  Integer
 * results, equal bits on every run.  Every offset read is clamped to num_objects / num_runs and every table entry to the source size:
 * unvalidated arrays give wrong labels, never an access outside the arrays.  One launch, nothing to zero beforehand. */
int sf_rle_label_maps(const unsigned* run_ends, const int* object_offsets, const int* frame_offsets, const void* tables, long long* labels_i64,
                      unsigned char* labels_u8, int* extents, int F, int num_objects, int num_runs, int h, int w, int H, int W, void* stream);
/* masks_to_boxes_pad (datasets/utils.py:59-77) on the extents of sf_rle_label_maps: bbox [F,num,4] float32 [min x, min y, max x, max y] and
 * pres_mask [F,num] bytes (torch.bool): the objects with a pixel AFTER the resize, compacted in order, padded with zeros; pres_mask is 1 for the
 * first k.  (The label ids of sf_rle_label_maps are not compacted: the asymmetry is the reference's.)  num <= 64.  flag: one device word, zeroed by
 * the call, set to 1 when a frame has more objects with a pixel than num (the reference fails with a shape error there); such a frame keeps its
 * first num boxes. */
int sf_rle_boxes_pad(const int* extents, float* bbox, unsigned char* pres_mask, unsigned* flag, int F, int num, void* stream);

/* ---- egress: decoded frames, slot decompositions, segment ids and boxes -> the videos a writer takes (video_prediction/vp_vis.py make_video /
 * draw_bbox, base_slots/method.py _make_video_grid, the `(video * 255.).astype(np.uint8)` of _save_video; csrc/egress.hip) -----------------------
 * The float work is the reference's float32 operations in their order, each rounded once (nothing is contracted into an fma except x * 0.5 + 0.5,
 * whose product is exact), so the results are held to EXACT equality with the same torch operations on the CPU.  Inputs are assumed FINITE (a NaN
 * or an infinity gives an unspecified byte).  All pointers are device pointers unless stated; float32 tensors 4-byte aligned, contiguous. */
enum { SF_EGRESS_TRUNC = 0, SF_EGRESS_NEAREST_EVEN = 1 };               /* rounding of v * 255: toward zero (_save_video) / torch.round (draw_bbox) */
enum { SF_EGRESS_F32_CHW = 0, SF_EGRESS_U8_CHW = 1, SF_EGRESS_U8_HWC = 2 };   /* what a grid is written as */
enum { SF_EGRESS_IMG = 0, SF_EGRESS_SLOTS = 1, SF_EGRESS_IDS = 2 };     /* tile kinds */
/* x [F,3,H,W] float32 -> out uint8 [F,3,H,W] (hwc = 0) or [F,H,W,3] (hwc = 1).  to_rgb = 1: v = clamp(x * 0.5 + 0.5, 0, 1) first (x in [-1, 1]);
 * 0: v = x (in [0, 1]).  out = rounding(clamp(v * 255.f, 0, 255)), so nothing wraps.  `x` and `out` may sit at any (4-byte / 1-byte) offset and W
 * need not be a multiple of 4: 16-byte loads and stores where the alignment allows them, a scalar path otherwise. */
int sf_egress_frames_u8(const float* x, unsigned char* out, long long F, int H, int W, int hwc, int to_rgb, int rounding, void* stream);
/* One entry of a grid's tile list (HOST memory, read during the call).  IMG: a = x [T,3,H,W] float32 in [-1, 1] -> to_rgb(x).  SLOTS: a = recons
 * [T,N,3,H,W], b = masks [T,N,1,H,W] float32 -> N consecutive tiles to_rgb(recons * masks + (1 - masks) * scale).  IDS: a = segment ids [T,H,W]
 * uint8 (ids_i64 = 0) or int64 (1), b = palette [P,3] uint8, 1 <= P <= 256 -> to_rgb(palette[id] / 255 * 2 - 1); an id >= P takes colour P - 1.
 * history_len: with a border, frames t < history_len get the green frame (0, 0.7, 0), the others the red one (0.7, 0, 0). */
typedef struct {
  int kind;
  int N;
  const void* a;
  const void* b;
  float scale;
  int ids_i64;
  int P;
  int history_len;
} sf_egress_tile;
/* The canvas of K tiles of H x W as torchvision.utils.make_grid(tiles, nrow, padding) lays them, each tile grown by `border` pixels on every side
 * first: xmaps = min(nrow, K), ymaps = ceil(K / xmaps), CH = ymaps * (H + 2 border + padding) + padding, CW likewise; tile k at row k / xmaps,
 * column k % xmaps.  K == 1: the tile itself, no padding. */
int sf_egress_grid_shape(int K, int H, int W, int nrow, int padding, int border, int* CH, int* CW);
/* One video of grids per launch: out [T,3,CH,CW] float32 in [0, 1] (SF_EGRESS_F32_CHW, what the reference's functions return), uint8 [T,3,CH,CW] or
 * uint8 [T,CH,CW,3] (TRUNC rounding).  The tiles of all entries in order (at most 32); pad_value and the border colours are written as they are,
 * not passed through to_rgb.  One canvas row must fit 64 KiB of LDS. */
int sf_egress_grid(const sf_egress_tile* tiles, int n_entries, void* out, int out_mode, int T, int H, int W, int nrow, int padding,
                   float pad_value, int border, void* stream);
/* Rectangle outlines IN PLACE on frames [F,3,H,W] uint8.  boxes [F,M,4] float32 (x0, y0, x1, y1), pres [F,M] uint8 or NULL, palette [P,3] uint8,
 * M <= 256.  Per frame: keep the boxes that are present and have x0 >= 0, truncate their coordinates toward zero; the k-th KEPT box takes colour
 * min(k, P - 1) (vp_vis.py:60-65: colors=PALETTE[:N] zipped with the surviving boxes -- not the slot index).  A pixel belongs to an outline iff it
 * lies inside the inclusive box and within `width` pixels of one of its four sides; outlines are clipped to the image, later boxes overwrite
 * earlier ones.  This is PIL's ImageDraw.rectangle(outline=, width=) for every box with both sides >= 2 * width; for thinner boxes PIL draws
 * outside the box, which is not followed -- the one difference. */
int sf_egress_draw_boxes(unsigned char* frames, const float* boxes, const unsigned char* pres, const unsigned char* palette, int P, int F, int M,
                         int H, int W, int width, void* stream);

/* table[HW,C] = dense(grid) (SoftPositionEmbed, utils.py:52-63; grid [HW,4]). */
int sf_pos_embed_table_f32(const float* grid, const float* dense_w, const float* dense_b, float* table, int HW,
                           int C, void* stream);

/* One Slot-Attention iteration, attention half (savi.py:82-89 / steve.py:50-60): logits,
 * softmax over slots, +eps, and the per-slot sums over pixels as P partial records per batch.
 * k,v rows have leading dimension ld and batch_stride floats between batches. */
int sf_slot_attn_num_partials(int HW);
int sf_slot_attn_iter_f32(const float* k, const float* v, int ld, long long batch_stride, const float* q,
                          float* part_num, float* part_den, float* attn_out, int B, int HW, int N, int D,
                          float scale, float eps, void* stream);
/* The same iteration on keys == values kept as rows of 512 bytes (bf16 hi | lo of 128 channels: sf_pixel_feat_f32 form 4), the default of the encode
 * (sa_attn_planes_kernel, csrc/slot_chain.hip; sf_set_slot_attn_planes below).  Frame b starts batch_stride_rows rows behind frame b - 1; slot size 128,
 * HW a multiple of 512, 1 <= N <= 8.  P = HW / 256 records per frame: record 2c holds the sums over pixels 512 c .. 512 c + 511, the odd records are
 * zero.  attn_out NULL or [B][N][HW] with attn_batch_stride floats between frames. */
int sf_slot_attn_iter_planes_f32(const void* planes, long long batch_stride_rows, const float* q, float* part_num, float* part_den,
                                 float* attn_out, long long attn_batch_stride, int B, int HW, int N, float scale, float eps, void* stream);
/* The slots of a time step before its first iteration, as one launch (sa_slot_prologue_kernel, csrc/slot_attn.hip; savi.py:393-402, predictor.py:65-73,
 * project_q): lat = prev NULL ? init[row % N] : ResidualMLPPredictor(prev); kernel_dist = Linear(lat) [2D]; slots = mu (+ noise * exp(logvar / 2));
 * q = project_q(slots).  Exact f32.  Matrices TRANSPOSED ([in][out]): pm_w0_t [D][2D], pm_w2_t [2D][D], kd_w_t [D][2D], q_w_t [D][D].  noise row (b, n)
 * at noise + b * noise_bs + n * D, kdist_out row (b, n) at kdist_out + b * kdist_bs + n * 2D (either may be NULL).  D a multiple of 64, at most 384. */
int sf_slot_prologue_f32(const float* prev, const float* init, const float* pm_ln_g, const float* pm_ln_b, const float* pm_w0_t,
                         const float* pm_b0, const float* pm_w2_t, const float* pm_b2, int norm_first, const float* kd_w_t,
                         const float* kd_b, const float* noise, long long noise_bs, float* kdist_out, long long kdist_bs,
                         const float* q_ln_g, const float* q_ln_b, const float* q_w_t, float* slots_out, float* q_out, int B, int N,
                         int D, float ln_eps, void* stream);

/* bf16-STORAGE variant (SURVEY.md 8(b2) `sf_slot_attn_iter_bf16`): k, v are bf16 rows (ld / batch_stride in elements), half the
 * bytes of this HBM-bound kernel; logits, softmax, the weighted sums and every output stay f32.  Rounding K/V to bf16 costs
 * ~2e-3 relative on the updates (tests/test_kernels_gpu.py) -- outside the encode path's 5e-5, hence an option only. */
int sf_slot_attn_iter_bf16(const void* k, const void* v, int ld, long long batch_stride, const float* q, float* part_num,
                           float* part_den, float* attn_out, int B, int HW, int N, int D, float scale, float eps, void* stream);
/* Both take 1 <= N <= 16 slots.  N <= 8 runs the 8-slot instantiation of the iteration kernel, 9 .. 16 the 16-slot one (same
 * three forms: VALU, two-pass MFMA, one-pass tile for keys == values at slot_size 128).  At 9 .. 16 slots the one-pass form
 * holds 84,480 B of LDS -- one workgroup per CU; sf_set_slot_attn_tile16(0) sends those shapes to the two-pass form instead
 * (process-wide, default 1; profiles/slots16.md). */
int sf_set_slot_attn_tile16(int on);
int sf_get_slot_attn_tile16(void);

/* Backward of sf_slot_attn_iter_f32 (row N1: savi.py:82-94 under autograd).  Inputs of the forward call (k, v, q, the
 * partial records it produced) plus d_updates [B,N,D], the gradient w.r.t. updates = sum(num) / sum(den).  Writes
 * dq [B,N,D] and dk / dv (same row layout as k / v); accumulate != 0 adds into dk / dv instead (the iterations of one
 * frame share k and v).  slot_size 64 / 128 / 192 / 256, at most 8 slots (9 .. 16: sf_slot_attn_iter_bwd16_f32 below). */
size_t sf_slot_attn_iter_bwd_workspace_bytes(int B, int HW, int N, int D);
int sf_slot_attn_iter_bwd_f32(const float* k, const float* v, int ld, long long batch_stride, const float* q,
                              const float* part_num, const float* part_den, int P, const float* d_updates, float* dk,
                              float* dv, int accumulate, float* dq, int B, int HW, int N, int D, float scale, float eps,
                              void* ws, size_t ws_bytes, void* stream);
/* The same backward for 1 <= N <= 16 slots, same arguments and workspace layout.  N <= 8 runs the kernel above (same bits);
 * 9 .. 16 slots run it as two launches that share the softmax over all the slots: the first writes dk / dv and the dq partials
 * of slots 0..7, the second reads the rows again for the dq partials of slots 8..15 (16 slots of running dq sums do not fit
 * the registers at slot_size 256).  dq stays a fixed-order sum of per-workgroup partials. */
size_t sf_slot_attn_iter_bwd16_workspace_bytes(int B, int HW, int N, int D);
int sf_slot_attn_iter_bwd16_f32(const float* k, const float* v, int ld, long long batch_stride, const float* q,
                                const float* part_num, const float* part_den, int P, const float* d_updates, float* dk,
                                float* dv, int accumulate, float* dq, int B, int HW, int N, int D, float scale, float eps,
                                void* ws, size_t ws_bytes, void* stream);

/* Slot update (savi.py:95-100): updates = sum(num)/sum(den); GRUCell (r,z,n); slots + MLP(LN(slots)).
 * The four weight MATRICES are passed transposed ([in,out] = torch weight.t().contiguous()):
 * gru_w_ih [D,3D], gru_w_hh [D,3D], mlp_w1 [D,H], mlp_w2 [H,D]; biases / LN vectors as in torch. */
int sf_slot_update_f32(const float* part_num, const float* part_den, int P, const float* slots_prev,
                       const float* gru_w_ih, const float* gru_w_hh, const float* gru_b_ih,
                       const float* gru_b_hh, const float* ln_g, const float* ln_b, const float* mlp_w1,
                       const float* mlp_b1, const float* mlp_w2, const float* mlp_b2, float* slots_out, int B,
                       int N, int D, int H, float ln_eps, void* stream);

/* The same slot update on the matrix cores (split-bf16 products; slot size D = 128 with slot MLP size H = 256, or D = 192 with H = 384), plus the
 * next iteration's q = project_q(slots_out) (savi.py:45-48,79) when q_out is not NULL.  The five matrices are
 * sf_pack_linear_weights copies of the TORCH-layout weights: GRUCell weight_ih / weight_hh [3D, D], mlp[1].weight [H, D],
 * mlp[3].weight [D, H], project_q[1].weight [D, D]. */
int sf_slot_update_packed_f32(const float* part_num, const float* part_den, int P, const float* slots_prev,
                              const void* gru_ih_packed, const void* gru_hh_packed, const float* gru_b_ih,
                              const float* gru_b_hh, const float* ln_g, const float* ln_b, const void* mlp_w1_packed,
                              const float* mlp_b1, const void* mlp_w2_packed, const float* mlp_b2, float* slots_out,
                              const float* q_ln_g, const float* q_ln_b, const void* q_w_packed, float* q_out, int B, int N,
                              int D, int H, float ln_eps, void* stream);
/* The same (D = 128, H = 256 only) the way the encode launches a time step's last iteration: out2 NULL or a second copy of the rows, row (b, n) at
 * out2 + b * out2_bs + n * D; p_step 1 or 2: only every p_step-th partial record is read (2: the even ones, what sf_slot_attn_iter_planes_f32 fills);
 * and, next_slots not NULL, the NEXT form: behind the update the same workgroups run the slot prologue of the following step on the updated rows --
 * ResidualMLPPredictor (pm_*, norm_first), kernel_dist Linear (kd_*), sampling with noise (row (b, n) at noise + b * noise_bs + n * D, or NULL) -> next_slots
 * [B * N][D] (not slots_out), kdist_out (row (b, n) at kdist_out + b * kdist_bs + n * 2D, or NULL), and q_out = project_q(next_slots) instead of
 * project_q(slots_out).  pm_w0_packed / pm_w2_packed / kd_w_packed: sf_pack_linear_weights copies of the torch-layout [2D][D], [D][2D], [2D][D]. */
int sf_slot_update_packed_next_f32(const float* part_num, const float* part_den, int P, const float* slots_prev,
                                   const void* gru_ih_packed, const void* gru_hh_packed, const float* gru_b_ih,
                                   const float* gru_b_hh, const float* ln_g, const float* ln_b, const void* mlp_w1_packed,
                                   const float* mlp_b1, const void* mlp_w2_packed, const float* mlp_b2, float* slots_out,
                                   const float* q_ln_g, const float* q_ln_b, const void* q_w_packed, float* q_out, int B, int N,
                                   int D, int H, float ln_eps, float* out2, long long out2_bs, int p_step, const float* pm_ln_g,
                                   const float* pm_ln_b, const void* pm_w0_packed, const float* pm_b0, const void* pm_w2_packed,
                                   const float* pm_b2, int norm_first, const void* kd_w_packed, const float* kd_b, const float* noise,
                                   long long noise_bs, float* kdist_out, long long kdist_bs, float* next_slots, void* stream);

/* nn.MultiheadAttention core for short sequences: qkv [B*L,3d] (q|k|v), out [B*Lq,d]; queries
 * are the last Lq rows of each sequence (Lq == L: all). */
int sf_mha_f32(const float* qkv, float* out, int B, int L, int Lq, int d_model, int num_heads, void* stream);

/* Fused self-attention block of one TransformerEncoderLayer (split-bf16 MFMA projection, f32 attention):
 * att[B*Lq,d] = MHA(LN?(x)) before out_proj; x [B*L,d]; in_proj_w [3d,d], in_proj_b [3d] (torch packed q|k|v);
 * ln_gamma/ln_beta may both be NULL.  Needs L <= 64, d % 64 == 0, head_dim in {16,32,48,64}. */
int sf_qkv_attention_f32(const float* x, const float* ln_gamma, const float* ln_beta, float ln_eps,
                         const float* in_proj_w, const float* in_proj_b, float* out, int B, int L, int Lq, int d_model,
                         int num_heads, void* stream);

/* nn.LSTM single step pointwise part (predictor.py:116-117), gates [R,4H] (i,f,g,o) pre-summed. */
int sf_lstm_pointwise_f32(const float* gates, const float* c_prev, float* h_out, float* c_out, int R, int H,
                          void* stream);

/* StoSAVi._sample_dist (savi.py:355-365): out = mu (+ noise*exp(logvar/2)); noise may be NULL. */
int sf_sample_dist_f32(const float* dist, const float* noise, float* out, int R, int D, void* stream);

/* F.interpolate(bilinear, align_corners=False) on R planes (steve.py:230-238). */
int sf_bilinear_resize_f32(const float* in, float* out, long long R, int Hi, int Wi, int Ho, int Wo,
                           void* stream);

/* ---- STEVE image side (row N2, second half): dVAE blocks -------------------------------------- */
/* Conv2dBlock's normalisation (steve_utils.py:124-126): F.group_norm(x, 1, gamma, beta, eps) over (C,H,W) per
 * sample, then ReLU when `relu`; NHWC x [F,H,W,C].  pixel_shuffle == 2 also applies the nn.PixelShuffle(2) that
 * follows the block in dVAE.py:44,49 (y [F,2H,2W,C/4]); 1 = none. */
size_t sf_groupnorm1_workspace_bytes(int F);
int sf_groupnorm1_nhwc_f32(const float* x, const float* gamma, const float* beta, float* y, int F, int H, int W, int C,
                           float eps, int relu, int pixel_shuffle, void* ws, size_t ws_bytes, void* stream);
/* Adjoint of the call above (row N1: the dVAE under autograd, dVAE.py:113-139).  x is the INPUT of the forward call (the
 * statistics and the ReLU gate are recomputed from it), dy the gradient of its output ([F,H,W,C], or [F,2H,2W,C/4] with
 * pixel_shuffle 2); writes dx [F,H,W,C], dgamma [C], dbeta [C]. */
size_t sf_groupnorm1_bwd_workspace_bytes(int F, int H, int W, int C);
int sf_groupnorm1_nhwc_bwd_f32(const float* x, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma,
                               float* dbeta, int F, int H, int W, int C, float eps, int relu, int pixel_shuffle, void* ws,
                               size_t ws_bytes, void* stream);

/* STEVE's slot-conditioned Transformer decoder (steve_transformer.py): attention core (bias-free projections are
 * plain sf_linear_f32 calls), token + position embedding, greedy token pick, token cross-entropy. */
int sf_slate_attention_f32(const float* q, const float* k, const float* v, float* out, int ldq, int ldk, int ldv, int ldo,
                           int B, int Lq, int Lk, int num_heads, int head_dim, int causal, void* stream);
/* Adjoint of sf_slate_attention_strided_f32 (row N1: the STEVE decoder's causal self-attention and slot cross-attention
 * under autograd, steve_transformer.py:61-116), flash style: `out` is the forward result, d_out its gradient; dq / dk / dv
 * have the layouts of q / k / v.  dq is cleared here and accumulated with float atomics.  head_dim even, <= 64; causal
 * needs Lq == Lk. */
size_t sf_slate_attention_bwd_workspace_bytes(int B, int Lq, int num_heads);
/* The same pair with dropout on the attention WEIGHTS (the nn.Dropout inside steve_transformer.py's MultiHeadAttention, active
 * in train() mode): masks are a pure function of (seed, sequence, head, query, key).  The forward also returns the row
 * log-sum-exp lse [B][H][Lq], which the backward takes instead of recomputing it (lse == NULL: recompute).
 * sf_slate_attention_train_bwd_f32 takes head_dim = every multiple of 4 up to 64 (the forward every even one) and reads q and
 * d_out with 16-byte loads: q, d_out, ldq, ldo, q_bs and o_bs must be multiples of 16 bytes (4 floats), or the call is refused
 * before anything is launched.  k and v may sit anywhere: the 48-wide split-bf16 kernel (32 < head_dim <= 48) is chosen only when
 * k, v, ldk, ldv, k_bs and v_bs are multiples of 16 bytes too, otherwise the generic kernel reads them float by float.  dq is
 * cleared over the head columns of its Lq rows per sequence only: columns and rows next to them are not written. */
int sf_slate_attention_train_fwd_f32(const float* q, const float* k, const float* v, float* out, float* lse, int ldq, int ldk,
                                     int ldv, int ldo, long long q_bs, long long k_bs, long long v_bs, long long o_bs, int B,
                                     int Lq, int Lk, int num_heads, int head_dim, int causal, float dropout_p,
                                     unsigned long long seed, void* stream);
int sf_slate_attention_train_bwd_f32(const float* q, const float* k, const float* v, const float* out, const float* d_out,
                                     const float* lse, float* dq, float* dk, float* dv, int ldq, int ldk, int ldv, int ldo,
                                     long long q_bs, long long k_bs, long long v_bs, long long o_bs, int B, int Lq, int Lk,
                                     int num_heads, int head_dim, int causal, float dropout_p, unsigned long long seed, void* ws,
                                     size_t ws_bytes, void* stream);
int sf_slate_attention_bwd_f32(const float* q, const float* k, const float* v, const float* out, const float* d_out, float* dq,
                               float* dk, float* dv, int ldq, int ldk, int ldv, int ldo, long long q_bs, long long k_bs,
                               long long v_bs, long long o_bs, int B, int Lq, int Lk, int num_heads, int head_dim, int causal,
                               void* ws, size_t ws_bytes, void* stream);
/* the same with explicit batch strides (floats), so that k/v may be a partially filled K/V cache */
int sf_slate_attention_strided_f32(const float* q, const float* k, const float* v, float* out, int ldq, int ldk, int ldv,
                                   int ldo, long long q_bs, long long k_bs, long long v_bs, long long o_bs, int B, int Lq,
                                   int Lk, int num_heads, int head_dim, int causal, void* stream);
int sf_embed_tokens_f32(const long long* idx, const float* tok_emb, const float* pos, float* out, int B, int L, int d,
                        void* stream);
int sf_argmax_rows_f32(const float* x, long long ld, long long* out, long long R, int V, void* stream);
int sf_cross_entropy_f32(const float* x, const long long* target, float* loss_rows, float* mean_out, long long R, int V,
                         void* stream);
/* y = softmax((x + add) * scale) per row (add may be NULL): the Gumbel-softmax relaxation of steve_utils.py:26-41 with
 * add = Gumbel noise, scale = 1/tau (steve_slotformer.py:97-98). */
int sf_softmax_rows_f32(const float* x, const float* add, float scale, float* y, long long R, int V, void* stream);
/* Backward of sf_cross_entropy_f32's mean loss w.r.t. the logits: dx = (softmax(x) - onehot(target)) * g[0] / R, with g the
 * upstream gradient as a DEVICE scalar (no host read); V <= 16384 (steve.py:341-344 under autograd). */
int sf_cross_entropy_bwd_f32(const float* x, const long long* target, const float* g, float* dx, long long R, int V, void* stream);
/* y = log_softmax(x) per row (the z_logits of dVAE.py:127). */
int sf_log_softmax_rows_f32(const float* x, float* y, long long R, int V, void* stream);
/* y[r, :] = softmax((x[r, :] + g[r, :]) * scale), g ~ Gumbel(0, 1) generated inside the kernel as a pure function of
 * (seed, r * V + j) -- g = -log(-log(u)), u = ((mix32(idx ^ s) >> 9) + 0.5) * 2^-23 -- so the noise of
 * steve_utils.py:30-35 never travels through memory (training only; R * V < 2^32). */
int sf_gumbel_softmax_rows_f32(const float* x, unsigned long long seed, float scale, float* y, long long R, int V, void* stream);
/* Adjoint of sf_softmax_rows_f32 w.r.t. x (and add) given its output y: dx = scale * y * (dy - sum(y * dy)) per row -- the
 * Gumbel-softmax relaxation of steve_utils.py:26-41 under autograd. */
int sf_softmax_rows_bwd_f32(const float* y, const float* dy, float scale, float* dx, long long R, int V, void* stream);

/* K/V-cached greedy generation of the dVAE token grid (STEVETransformerDecoder.generate, sample=False,
 * steve_transformer.py:305-333; used by STEVESlotFormer.decode, steve_slotformer.py:92-93).  One token per step; the
 * arithmetic of a step equals the reference's forward on the prefix.  All pointers device, torch layouts; wqkv =
 * cat(proj_q, proj_k, proj_v).weight [3d,d], wkv_c = cat(proj_k, proj_v).weight of the cross-attention [2d,d]. */
typedef struct {
  const float *ln1_g, *ln1_b, *wqkv, *wo;          /* self-attention */
  const float *ln2_g, *ln2_b, *wq_c, *wkv_c, *wo_c; /* encoder_decoder_attn (keys / values = the slots) */
  const float *ln3_g, *ln3_b, *w1, *b1, *w2, *b2;   /* FFN */
  int is_first;                                     /* first block: input normalised in place (steve_transformer.py:186) */
} sf_slate_block;

typedef struct {
  int d_model, num_heads, num_layers, vocab_size, num_slots, max_len;
  const float *in_proj_w, *in_proj_b, *tok_emb /*[V+1,d]*/, *pos_emb /*[max_len+1,d]*/, *lnf_g, *lnf_b, *head_w /*[V,d]*/;
  const sf_slate_block* blocks; /* HOST array [num_layers] */
} sf_slate_decoder;

size_t sf_slate_generate_workspace_bytes(const sf_slate_decoder* m, int B, int steps);
/* slots [B,N,d] -> tokens_out int64 [B,steps]; logits_out [B,steps,V] or NULL. */
int sf_slate_generate_f32(const sf_slate_decoder* m, const float* slots, int B, int steps, long long* tokens_out,
                          float* logits_out, void* ws, size_t ws_bytes, void* stream);

/* The same generation with one launch per token (slate_step.hip): a workgroup owns frames_per_wg consecutive frames for a whole
 * token step -- embedding, every block, final LayerNorm, vocabulary head, argmax -- and talks to no other workgroup; the K/V
 * cache and the token array are the only state between launches.  Exact fp32 FMA.
 * sf_slate_step_ok reads shapes only (never a weight) and returns 1 where the fused step applies.  It refuses:
 *   d_model <= 0, d_model > 512 or d_model % 32 != 0;  num_heads < 1, > 16 or not dividing d_model;
 *   a head size other than 16, 32, 48 or 64;  num_layers < 1 or > 8;  vocab_size < 1;  num_slots < 1;  max_len < 0. */
int sf_slate_step_ok(const sf_slate_decoder* m);
/* enough for either form (0 for a NULL model, B <= 0 or steps <= 0) */
size_t sf_slate_generate_tok_workspace_bytes(const sf_slate_decoder* m, int B, int steps);
/* slots [B,N,d] -> tokens_out int64 [B,steps]; logits_out [B,steps,V] on the device, or NULL (then no logits are written).
 * frames_per_wg: 1, 2 or 4 asks for the fused step with that many frames per workgroup; 0 is the library's choice.
 * Where sf_slate_step_ok is 0 -- whatever frames_per_wg says -- or the library's choice for this B is the launch chain,
 * sf_slate_generate_f32 runs.  *frames_per_wg_ran (may be NULL) receives the form that ran: 0 = the launch chain, else the
 * frames per workgroup of the fused step.
 * The library's choice (profiles/steve_render.md; the fused step is chosen only where it beat the chain by more than the 6 %
 * box-to-box spread; measured at the Physion decoder, 1024 steps, on one MI355X): up to 192 frames the fused step
 * with one frame per workgroup (0.88 / 0.82 / 0.77 / 0.70 of the chain's time at 1 / 12 / 64 / 192 frames; two frames per
 * workgroup never beat one by more than the spread, four lost to the chain from 12 frames on); beyond 192 frames, where nothing
 * is measured, the launch chain. */
int sf_slate_generate_tok_f32(const sf_slate_decoder* m, const float* slots, int B, int steps, long long* tokens_out,
                              float* logits_out, int frames_per_wg, void* ws, size_t ws_bytes, void* stream,
                              int* frames_per_wg_ran);
/* Two things the fused step can do inside its vocabulary sweep, each logit still in a register (csrc/slate_step.hip); both add the library's
 * counter-based Gumbel noise G(seed, i) = -log(-log(u)), u = ((mix32(i ^ s) >> 9) + 0.5) * 2^-23 with s derived from the 64-bit seed as
 * sf_gumbel_softmax_rows_f32 derives it.  Row r = row_base + b * steps + t, element i = r * V + v (uint32): with row_base = 0 the noise is what
 * sf_gumbel_softmax_rows_f32 adds to logits viewed as [B * steps, V]; a caller that renders a sequence in several calls passes the rows before a
 * call as row_base and gets the bits of one call.
 *   soft_rows (device [B][steps][64], or NULL = off): soft_rows[b, t, c] = sum_v z_v * conv0_t[v, c], z = softmax_v((l_v + G(soft_seed, i)) *
 *     soft_scale) -- the first dVAE decoder block (a bias-free 1x1 convolution V -> 64) applied to the Gumbel-softmax relaxation of
 *     steve_slotformer.py:97-98, computed online (running max, sum, 64 weighted accumulators; partial records merged in a fixed order), so neither
 *     the logits nor the relaxation [B, steps, V] need exist.  conv0_t: device [V][64], the transposed weight; conv0_width must be 64.  A frame's row
 *     does not depend on the other frames of the call.  Tokens and logits are bit-identical to a call without soft_rows.
 *   sample != 0: token[b, t] = argmax_v(l_v * inv_temperature + G(sample_seed, i)) (fp32; ties to the lowest index) -- Gumbel-max, an exact draw
 *     from softmax(l / T) -- and the drawn token feeds the next step.  Soft rows are computed from the raw logits either way.
 * With an option on the fused step always runs: frames_per_wg = 0 then means ONE frame per workgroup at any batch size (beyond 192 frames that
 * form is unmeasured, profiles/steve_render.md), and a decoder sf_slate_step_ok refuses is an error (negative code, nothing launched).
 * Argument errors -- soft_rows without conv0_t, conv0_width != 64, a non-finite or non-positive soft_scale (with soft_rows) or inv_temperature (with
 * sample), row_base < 0, (row_base + B * steps) * V >= 2^32 -- are reported before any device work. */
typedef struct {
  float* soft_rows;
  const float* conv0_t;
  int conv0_width;
  float soft_scale;
  unsigned long long soft_seed;
  int sample;
  float inv_temperature;
  unsigned long long sample_seed;
  long long row_base;
} sf_slate_step_opts;
/* With an option on (and a decoder the fused step takes): the fused step's own scratch -- the K/V cache [B, steps, 2 d] per block and the
 * projected slots, nothing that grows with the vocabulary; it is at most sf_slate_generate_tok_workspace_bytes, which must also fit the launch chain.
 * Otherwise that query's value. */
size_t sf_slate_generate_tok_opts_workspace_bytes(const sf_slate_decoder* m, int B, int steps, const sf_slate_step_opts* opts);
/* sf_slate_generate_tok_f32 with options; opts NULL, or soft_rows NULL and sample 0, behaves exactly as sf_slate_generate_tok_f32 does. */
int sf_slate_generate_tok_opts_f32(const sf_slate_decoder* m, const float* slots, int B, int steps, long long* tokens_out,
                                   float* logits_out, int frames_per_wg, void* ws, size_t ws_bytes, void* stream,
                                   int* frames_per_wg_ran, const sf_slate_step_opts* opts);
/* out[r, :] = table[ids[r], :], ids int64 [R], table [table_rows, d], d % 4 == 0 (the first 1x1 convolution of the dVAE decoder
 * on a one-hot token map).  An id outside the table is clamped to its ends, so a wrong id never reads out of bounds. */
int sf_gather_rows_f32(const float* table, const long long* ids, float* out, long long R, int d, long long table_rows,
                       void* stream);

/* ---- dVAE token ids without the logits (base_slots/tokenize_images.py, dVAE.py:24-35, 52-77; csrc/dvae_tokens.hip) --------------------------------
 * The two ends of the dVAE encoder as kernels of their own: the 4x4 / stride-4 patch embedding read straight from NCHW frames, and the vocabulary
 * head with the argmax inside (the logits live in MFMA accumulators only).  Between them the six 1x1 blocks run on sf_linear_f32 /
 * sf_groupnorm1_nhwc_f32 as before.  Arithmetic of both: split-bf16 (every f32 operand = bf16 hi + bf16 lo, three products, f32 accumulation)
 * WHATEVER sf_set_precision says -- token targets have one definition -- every sum in a fixed order, no atomics: a pixel's id does not depend on
 * its place in the batch.  No workspace.
 *
 * sf_dvae_tokens_ok reads shapes only: 1 exactly when K == 64 (features of the head), C == 3, H >= 4 and W >= 4 are multiples of 4, and V is a
 * multiple of 32 (the MFMA block) with 32 <= V <= 2^20; 0 otherwise. */
int sf_dvae_tokens_ok(int V, int K, int C, int H, int W);
/* Bytes of the packed head weight: V * K * 4 (a bf16 hi plane of V * K elements and the lo plane behind it); 0 unless K == 64 and V as above. */
size_t sf_dvae_head_packed_bytes(int V, int K);
/* w [V,K] f32 (the head's 1x1 convolution, torch's layout) -> packed, in fragment order: for every block vb of 32 words and every k-step ks of 16
 * features, 64 lanes x 8 bf16, lane l holding W[32 vb + (l & 31)][16 ks + 8 (l >> 5) + 0..7] -- element ((vb * 4 + ks) * 64 + l) * 8 + j of the hi
 * plane (bf16 of the value, round to nearest even), the lo plane (bf16 of the remainder) behind it.  The _host twin takes and fills HOST memory with
 * the same bytes. */
int sf_dvae_pack_head_weights(const float* w, void* packed, int V, int K, void* stream);
int sf_dvae_pack_head_weights_host(const float* w, void* packed, int V, int K);
/* img [F,C,H,W] f32 (NCHW, C == 3, H and W multiples of 4), w [64,C,4,4] -> y [F,H/4,W/4,64] (NHWC): the bias-free 4x4 / stride-4 convolution of
 * the first encoder block, before its GroupNorm.  img and w 16-byte aligned. */
int sf_dvae_patch_embed_f32(const float* img, const float* w, float* y, int F, int C, int H, int W, void* stream);
/* ids[r] = the FIRST index of the maximum over v of (W[v] . x[r] + bias[v]); x [R,K] f32 with row stride ld >= K (a multiple of 4), w_packed from
 * sf_dvae_pack_head_weights, bias [V] or NULL.  ids_i64 [R] and ids_i16 [R]: either may be NULL, not both; int16 (the dtype of the token files)
 * is refused when V > 32768.  A row holding a NaN gives an unspecified (valid) id.  x, w_packed and bias 16-byte aligned. */
int sf_dvae_head_argmax_f32(const float* x, long long ld, const void* w_packed, const float* bias, long long* ids_i64, short* ids_i16, long long R,
                            int V, int K, void* stream);

/* ---- the vocabulary head and its cross-entropy without the logits (steve_slotformer.py:150-161; csrc/head_ce.hip) --------------------------------
 * The token loss of a frozen decoder head W [V,K] (nn.Linear without bias) on rows x [R,K] against token ids t [R], forward and backward, with the
 * logits [R,V] in MFMA accumulators only:
 *   lse[r] = log sum_v exp(W[v] . x[r]),  loss[r] = lse[r] - W[t_r] . x[r],  dx[r,:] = c_r (sum_v exp(W[v] . x[r] - lse[r]) W[v,:] - W[t_r,:]).
 * The target's logit (forward) and the one-hot (backward) are picked by comparing the swept word index with t_r, never by an address formed from
 * it: a target outside [0, V) matches no word -- loss[r] = lse[r], dx[r,:] = c_r sum_v p W[v,:] -- and reads nothing.  The gradient of W is a launch
 * of its own, sf_head_ce_wgrad_f32.
 * Arithmetic: split-bf16 (every f32 operand = bf16 hi + bf16 lo, three products, f32 accumulation) WHATEVER sf_set_precision says, as for the dVAE
 * tokens; the exponentials are summed against the running maximum; every sum in a fixed order, no atomics, no communication between workgroups: two
 * calls give the same bits, and a row's results do not depend on its place in the batch.
 *
 * sf_head_ce_ok reads shapes only: 1 exactly when K is a multiple of 32 with 32 <= K <= 256 and V a multiple of 32 with 32 <= V <= 2^20. */
int sf_head_ce_ok(int V, int K);
/* Bytes of the packed head weight: V * K * 8 (two fragment-ordered copies, each a bf16 hi plane of V * K elements and its lo plane); 0 unless
 * sf_head_ce_ok.  Bytes of the forward's workspace for R rows (one pair of float64 per tile of 64 rows; needs no initial value); 0 for a bad R. */
size_t sf_head_ce_packed_bytes(int V, int K);
size_t sf_head_ce_workspace_bytes(long long R);
/* w [V,K] f32 (torch's layout) -> packed: four planes of n = V * K bf16 elements, A hi | A lo | B hi | B lo; hi = bf16 of the value (round to
 * nearest even), lo = bf16 of the remainder (value - hi).  Both copies are sequences of fragments of 64 lanes x 8 elements, element (f * 64 + l) * 8 + j
 * of a plane being lane l's element j of fragment f:
 *   copy A, fragment f = vb * (K / 16) + ks (block vb of 32 words, k-step ks of 16 features):  W[32 vb + (l & 31)][16 ks + 8 (l >> 5) + j];
 *   copy B, fragment f = (vb * 2 + c) * (K / 32) + kfb (half c of block vb, block kfb of 32 features):
 *                                                   W[32 vb + 16 c + 8 (j >> 2) + 4 (l >> 5) + (j & 3)][32 kfb + (l & 31)].
 * The _host twin takes and fills HOST memory with the same bytes. */
int sf_head_ce_pack_weights(const float* w, void* packed, int V, int K, void* stream);
int sf_head_ce_pack_weights_host(const float* w, void* packed, int V, int K);
/* Forward.  x [R,K] f32 with row stride ld >= K (a multiple of 4); targets as int64 (target_i64) or int16 (target_i16, the dtype of the token files,
 * refused when V > 32768): exactly one of the two.  group_w [R / group] or NULL (all 1): the weight w of each run of `group` consecutive rows (a
 * frame's tokens); R % group == 0.  lse [R] is written; loss_rows [R] (the unweighted loss[r]; may be NULL) too.  stats (may be NULL) is float64 [2] and has
 * sum_r w(r) loss[r] and sum_r w(r) ADDED to it (rows of weight 0 add nothing, whatever their loss), the tiles' partial sums combined in index order by
 * a one-workgroup launch; it needs ws of sf_head_ce_workspace_bytes(R), 8-byte aligned.  x and w_packed 16-byte aligned. */
int sf_head_ce_fwd_f32(const float* x, long long ld, const void* w_packed, const long long* target_i64, const short* target_i16,
                       const float* group_w, int group, float* lse, float* loss_rows, double* stats, long long R, int V, int K, void* ws,
                       size_t ws_bytes, void* stream);
/* Backward.  x, ld, w_packed, targets, group_w, group as in the forward, lse [R] from it; g: ONE float on the device (no host read),
 * c_r = g[0] * w(r).  dx [R,K] with row stride ldx >= K is written; a row of weight 0 receives exact zeros. */
int sf_head_ce_bwd_f32(const float* x, long long ld, const void* w_packed, const long long* target_i64, const short* target_i16,
                       const float* group_w, int group, const float* lse, const float* g, float* dx, long long ldx, long long R, int V, int K,
                       void* stream);
/* The head's own gradient, for a head that is trained (STEVE):  dW[v,:] = sum_r c_r (exp(W[v] . x[r] - lse[r]) - [v == t_r]) x[r,:], again without
 * the logits.  x, ld, w_packed, targets, group_w, group, lse, g as in the backward; dW [V,K] with row stride ldw >= K is OVERWRITTEN (R == 0: with
 * zeros).  A launch of (slabs of 128 words) x (S row splits) workgroups keeps a wave's 32 words x K block of dW in accumulators over its split's
 * rows and writes it to ws; a second launch adds the S blocks in index order.  S depends on (R, V) alone -- min(8, ceil(256 / slabs), tiles of 32
 * rows), then the fewest splits of that run length -- never on the device, so equal inputs give equal bits everywhere.  ws: 16-byte aligned,
 * sf_head_ce_wgrad_workspace_bytes(R, V, K) = S * V * K * 4 bytes (at most 8 blocks of dW whatever R is; needs no initial value); 0 for a shape
 * sf_head_ce_ok refuses or an R outside [0, 2^29). */
size_t sf_head_ce_wgrad_workspace_bytes(long long R, int V, int K);
int sf_head_ce_wgrad_f32(const float* x, long long ld, const void* w_packed, const long long* target_i64, const short* target_i16,
                         const float* group_w, const float* lse, const float* g, float* dW, long long ldw, long long R, int V, int K, int group,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- Physion VQA readout on rolled-out slots (physion_vqa/models/readout.py; csrc/physion_readout.hip) -------------------------------------------
 * logit[k][b] = max_t ( w2_k . agg_{i<j} ( W1_k cat(s_ti, s_tj) + b1_k ) + b2_k ) for a stack of K heads, agg = 0 max / 1 sum / 2 mean over the
 * N (N - 1) / 2 slot pairs in itertools.combinations order.  linear1 of a pair is U_i + V_j (U = S W1[:, :C]^T + b1, V = S W1[:, C:]^T): one product
 * per slot, no gathered pair tensor.  U | V are split-bf16 products (every f32 operand = bf16 hi + bf16 lo, three products, f32 accumulation) WHATEVER
 * sf_set_precision says; every sum has a fixed order and no floating-point atomic is used: equal inputs give equal bits, and a video's results do not
 * depend on its place in the batch.  Ties: the FIRST timestep / pair of the maximum.
 *
 * slots: video v, frame t, slot n at slots + v * stride_v + t * stride_t + n * C (strides in elements, multiples of 4; stride_t >= N * C), V videos;
 * batch entry b reads video video_index[b] (int32, any order, repeats allowed) or video b when video_index is NULL.  Only frames [0, T) of the
 * named videos are read; an index outside [0, V) gives NaN results, never an access.  slots and W1 16-byte aligned.
 * Shapes (sf_physion_readout_ok, shapes only): 2 <= N <= 16, C and F multiples of 32 in [32, 256]; T >= 1, B >= 1, 1 <= K <= 65535. */
int sf_physion_readout_ok(int N, int C, int F);
/* W1 [K,F,2C], b1 [K,F], w2 [K,F], b2 [K] -> logits [K,B], t_star [K,B] (int32), and when not NULL step_logits [K,B,T] and pair_star [K,B,F]
 * (uint8: per feature the winning pair at t_star for agg = max; zeros for sum / mean). */
int sf_physion_readout_fwd_f32(const float* slots, long long stride_v, long long stride_t, int V, const int* video_index, const float* W1,
                               const float* b1, const float* w2, const float* b2, float* logits, int* t_star, float* step_logits,
                               unsigned char* pair_star, int K, int B, int T, int N, int C, int F, int agg, void* stream);
/* Backward of ONE head: g [B] = dL/dlogit, t_star [B] from the forward, pair_star [B,F] from the forward or NULL (max: the winning pairs are then
 * found again) -> dW1 [F,2C], db1 [F], dw2 [F], db2 [1], overwritten.  The gradient reaches frame t_star of each video only (max: the one pair of each
 * feature); the slots are frozen inputs.  Two launches: the relation at t_star per video, then per feature a sum over the videos in ascending order.
 * A t_star outside [0, T) or a recorded pair >= N (N - 1) / 2 gives NaN gradients, never an access.  workspace: 16-byte aligned,
 * sf_physion_readout_bwd_workspace_bytes(B, N, F) bytes (0 for unsupported arguments). */
size_t sf_physion_readout_bwd_workspace_bytes(int B, int N, int F);
int sf_physion_readout_bwd_f32(const float* slots, long long stride_v, long long stride_t, int V, const int* video_index, const float* W1,
                               const float* b1, const float* w2, const float* g, const int* t_star, const unsigned char* pair_star, float* dW1,
                               float* db1, float* dw2, float* db2, int B, int T, int N, int C, int F, int agg, void* workspace,
                               size_t workspace_bytes, void* stream);
/* One launch: logits [K,B], labels [B] (f32, 0 / 1), task_idx [B] (int32) or NULL, thresholds: n_thresh <= 16 floats in HOST memory ->
 * loss [K] = mean_b BCE-with-logits, g [K,B] = dloss/dlogit, and counts [K,n_thresh], task_counts [K,n_tasks,n_thresh] (int32; n_tasks <= 64) of
 * (sigmoid(logit) > thresh) == label, ADDED to what the buffers hold, so that batches accumulate.  Every output may be NULL. */
int sf_physion_readout_score_f32(const float* logits, const float* labels, const int* task_idx, const float* thresholds, int n_thresh, int n_tasks,
                                 float* loss, float* g, int* counts, int* task_counts, int K, int B, void* stream);

/* ---- whole-path engines ------------------------------------------------------------------ */

/* One nn.TransformerEncoderLayer (relu, batch_first); all pointers device, torch layouts. */
typedef struct {
  const float *norm1_g, *norm1_b, *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;
  const float *norm2_g, *norm2_b, *lin1_w, *lin1_b, *lin2_w, *lin2_b;
  /* optional (NULL = absent): sf_pack_ffn_weights() copies of lin1_w / lin2_w.  When every layer of a rollouter
   * has them (d_model 256, 8 heads, ffn 1024, norm_first, split-bf16 mode) sf_rollout_f32 runs each layer as two
   * launches (attention + out-proj partials; FFN1 + FFN2) instead of four. */
  const void *lin1_packed, *lin2_packed;
  /* optional, same rule: sf_pack_attn_weights() copies of in_proj_w / out_proj_w */
  const void *attn_in_packed, *attn_out_packed;
  /* optional: sf_pack_layer_tok_weights() copy of all four matrices (the layer's fragments in consumption order) -- with it the rollout runs the layers
   * before the last as ONE token-stationary launch each (csrc/layer_tok.hip, csrc/layer_tok128.hip; sf_rollout_opts.layer_tok).  A blob belongs to
   * the (d_model, heads, ffn) it was packed for: (256, 8, 1024) or (128, 8, 512) */
  const void* tok_packed;
} sf_tfm_layer;

/* Pre-split attention weights (d_model 256, 8 heads) in MFMA-fragment order: in_packed needs
 * sf_attn_packed_bytes(d, 0) bytes, out_packed sf_attn_packed_bytes(d, 1). */
size_t sf_attn_packed_bytes(int d_model, int which);
int sf_pack_attn_weights(const float* in_proj_w, const float* out_proj_w, void* in_packed, void* out_packed, int d_model,
                         int num_heads, void* stream);

/* Pre-split (bf16 hi/lo) FFN weights in MFMA-fragment order; each output needs sf_ffn_packed_bytes() bytes. */
size_t sf_ffn_packed_bytes(int d_model, int ffn);
int sf_pack_ffn_weights(const float* lin1_w, const float* lin2_w, void* lin1_packed, void* lin2_packed, int d_model,
                        int ffn, void* stream);

/* FFN half of a pre-LN nn.TransformerEncoderLayer (d_model 256, ffn 1024; slotformer.py:72-80) on M rows whose input arrives
 * as 4 partial sums ap [4][M][256] (ap_stride floats apart; the head-pair partials of the layer's attention launch):
 *   x2 = ((ap0 + ap1) + ap2) + ap3;   y = x2 + lin2(relu(lin1(LN2(x2))))
 * written as the four hidden-chunk partials xp [4][M][256] with y = ((xp0 + xp1) + xp2) + xp3 (the next layer's attention
 * launch sums them while loading).  rows_per_wg: 32 / 64 / 128 rows per workgroup (0 = default); every choice gives the
 * same bits.  Needs w->lin1_packed / lin2_packed. */
int sf_ffn_chunk_partials_f32(const sf_tfm_layer* w, const float* ap, long long ap_stride, float* xp, long long xp_stride, int M,
                              int ffn, int rows_per_wg, void* stream);

/* Attention half of the same layer on B sequences of L <= 64 tokens, x [B][L][256]: the last Lq rows of every sequence of
 *   x2 = x + out_proj(MHA(LN1(x))) + b_o        (8 heads of 32)
 * heads_per_wg = 8: one workgroup per sequence runs all heads, out [2][B*Lq][256]: out[0] = x2, out[1] scratch;  heads_per_wg = 2: one workgroup per
 * (head pair, sequence), out [4][B*Lq][256] = the four head-pair partials with x2 = ((p0 + p1) + p2) + p3 -- the input format
 * of sf_ffn_chunk_partials_f32.  Both forms give the same bits.  Needs w->attn_in_packed / attn_out_packed. */
int sf_attn_block_f32(const sf_tfm_layer* w, const float* x, float* out, int B, int L, int Lq, int heads_per_wg, void* stream);
/* The same block in its row-tile form (sf_rollout_opts.attn_qkv_rows = 128; csrc/attn_rows.hip): LN1 + q|k|v on 128-row tiles of the
 * whole batch, then one workgroup per sequence (wave = head) + out-projection.  out [B*Lq][256] = x2;  planes: scratch of
 * sf_attn_rows_planes_bytes(B) bytes (q, k, v^T of every (sequence, head) as split-bf16 MFMA-fragment planes; cleared by the call). */
/* The FFN block y = x2 + lin2(relu(lin1(LN2(x2)))) on finished rows x2 [M][256] in its row-tile form (sf_rollout_opts.ffn_tile). */
int sf_ffn_block_rows_f32(const sf_tfm_layer* w, const float* x2, float* y, int M, int ffn, void* stream);
/* Whole pre-LN layers  y = x2 + lin2(relu(lin1(LN2(x2)))),  x2 = x + out_proj(MHA(LN1(x))) + b_o  on B sequences of L <= 96 tokens, x, y [B][L][256],
 * in the token-stationary form (csrc/layer_tok.hip): a 128-token workgroup owns whole sequences (as many as keep the keys of a wave's rows inside three
 * 32-key blocks: three of 42 tokens, one of 50 or of 65..96), a wave 32 tokens; every product of a layer keeps its
 * activations in registers (the accumulator layout of one product is the B operand of the next), the weight fragments stream global -> LDS once per
 * workgroup, only a head's keys / values cross waves; `nl` (1..8) consecutive layers w[0..nl) run in ONE launch (the rows never leave the registers
 * between them).  tok_packed: sf_pack_layer_tok_weights copy of a layer (sf_layer_tok_packed_bytes() bytes: its four matrices as fragments in consumption
 * order + its eight vectors).  A sequence's result does not depend on the other sequences of the call; it may differ in the last bits with its position
 * modulo the sequences per workgroup.
 * Two shapes (d_model, heads, ffn) are covered: (256, 8, 1024) and (128, 8, 512) -- the OBJ3D Transformer, heads of 16, x, y [B][L][128]
 * (csrc/layer_tok128.hip: the same workgroup / wave geometry and window rules; an attention stage carries a PAIR of heads).  sf_pack_layer_tok_weights
 * takes either and refuses every other shape; the blob it writes (sf_layer_tok_packed_bytes_ex(d_model, heads, ffn) bytes; 0 = shape not covered;
 * sf_layer_tok_packed_bytes() is the (256, 8, 1024) size) is only valid for the kernel of that shape.  sf_layer_tok_block_f32 is the (256, 8, 1024)
 * entry; sf_layer_tok_block_ex_f32 names the shape w[].tok_packed was packed for and runs that shape's kernel.  Both return an argument error without a
 * launch for L > 96, nl outside 1..8, an uncovered shape or a process precision other than split-bf16. */
size_t sf_layer_tok_packed_bytes(void);
size_t sf_layer_tok_packed_bytes_ex(int d_model, int num_heads, int ffn);
int sf_pack_layer_tok_weights(const sf_tfm_layer* w, void* packed, int d_model, int num_heads, int ffn, void* stream);
int sf_layer_tok_block_f32(const sf_tfm_layer* w, int nl, const float* x, float* y, int B, int L, void* stream);
int sf_layer_tok_block_ex_f32(const sf_tfm_layer* w, int nl, int d_model, int num_heads, int ffn, const float* x, float* y, int B, int L, void* stream);
int sf_debug_read_ts_layer_tok(long long* out16);   /* wall-clock stamps (10 ns) of workgroup 0 with SF_DBG=lt */
size_t sf_attn_rows_planes_bytes(int B);
int sf_attn_block_rows_f32(const sf_tfm_layer* w, const float* x, float* out, void* planes, int B, int L, int Lq, void* stream);

/* ---- PHYRE task-success readout and AUCCESS ranks (phyre_planning/models/readout.py, test_phyre_planning.py; csrc/phyre_readout.hip) -------------
 * Inference only.  logit[b] = cls_mlp( TransformerEncoder( [CLS ; in_proj(slots[b, sel[t], n]) + enc_t_pe[t]] )[0] ): three launches -- the token
 * rows x [B][1 + T N][128] (t-major, slot-minor; split-bf16 product on MFMA, f32 accumulation), the num_layers pre-LN layers as ONE token-stationary
 * launch (layers[l].tok_packed: sf_pack_layer_tok_weights copies for (128, 8, 512); eps 1e-5), and the head Linear(128,128) - ReLU - Linear(128,1)
 * on row 0 in plain f32.  Fixed summation orders, no floating-point atomics: equal inputs give equal bits.
 *
 * slots: video v, frame f, slot n at slots + v * stride_v + f * stride_t + n * C (strides in elements, multiples of 4; stride_t >= N * C), V videos
 * of T_all frames, read in place; batch entry b reads video video_index[b] (int32, device; any order, repeats allowed) or video b when NULL; an index
 * outside [0, V) gives NaN logits, never an access.  sel: T int32 in HOST memory, sel[t] in [-1, T_all): the frame of token group t; -1 is a frame of
 * zeros (tokens = bias + enc_t_pe[t], nothing is read).  The position row is chosen by t, the place in sel.  in_proj_w [128][C], in_proj_b [128],
 * enc_t_pe [T][128], cls [128], layers: HOST array [num_layers], mlp_w1 [128][128], mlp_b1 [128], mlp_w2 [128], mlp_b2 [1] -> logits [B];
 * conf [B] = sigmoid(logit) when not NULL; scatter_table[scatter_index[b]] = conf[b] when scatter_table is not NULL (scatter_index [B] int32, device;
 * an index outside [0, scatter_len) is skipped).  workspace: 16-byte aligned, sf_phyre_readout_workspace_bytes(B, N, T) bytes (0 for unsupported
 * arguments).  Limits (sf_phyre_readout_ok, shapes only): 1 <= N <= 16, C a multiple of 32 in [32, 256], T >= 1, 1 + T N <= 96,
 * (d_model, heads, ffn) = (128, 8, 512), 1 <= num_layers <= 8.  Every violation -- and a process precision other than split-bf16, which the layers
 * need -- is a negative return code before any launch. */
int sf_phyre_readout_ok(int num_slots, int slot_size, int T, int d_model, int num_heads, int ffn, int num_layers);
size_t sf_phyre_readout_workspace_bytes(int B, int num_slots, int T);
int sf_phyre_readout_fwd_f32(const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index, const int* sel,
                             const float* in_proj_w, const float* in_proj_b, const float* enc_t_pe, const float* cls, const sf_tfm_layer* layers,
                             int num_layers, int d_model, int num_heads, int ffn, const float* mlp_w1, const float* mlp_b1, const float* mlp_w2,
                             const float* mlp_b2, float* logits, float* conf, const int* scatter_index, float* scatter_table, long long scatter_len,
                             int B, int T, int N, int C, void* workspace, size_t workspace_bytes, void* stream);
/* conf [tasks][actions] f32, status [tasks][actions] int32 (phyre's SimulationStatus: 0 invalid input, -1 not solved, > 0 solved) ->
 * first_rank [tasks] int32 = #{status != 0 and conf > c*}, c* = max conf over {status > 0}: the 0-based place of the first solved action when the
 * valid actions are ranked by falling confidence and a solved action wins ties; `actions` when the task has no solved action.  One workgroup per
 * task, two passes over its row. */
int sf_phyre_auccess_f32(const float* conf, const int* status, int* first_rank, int tasks, int actions, void* stream);

/* ---- CLEVRER VQA: the Aloe reasoner (clevrer_vqa/models/transformer.py, aloe.py; csrc/aloe.hip) ---------------------------------------------------
 * The forward (training: sf_aloe_train_fwd_f32 below).  tokens[b] = [CLS ; vision_in_proj([slot | 0 1]) for (t, n) t-major ; q_in_proj([q_embedding[token] | type pair | 1 0])] + pos,
 * L = 1 + T N + text_len rows of d_model; num_layers pre-LN nn.TransformerEncoderLayer (relu, eps 1e-5) with the padded text positions masked out as
 * keys; logits[b] = W2 relu(W1 x[b, 0] + b1) + b2.  Launches: the token rows (split-bf16 on MFMA), per layer LN1 + q|k|v, the masked attention
 * (split-bf16 on MFMA, f32 softmax), out_proj + residual, LN2 + linear1 + ReLU, linear2 + residual (the library's GEMM), and a plain-f32 head.  The
 * last layer computes k | v for every row and everything else for the CLS rows only.  Fixed summation orders, no floating-point atomics: equal inputs
 * give equal bits.
 * Limits (sf_aloe_ok, shapes only): 1 <= N <= 16 slots, C a multiple of 32 in [32, 256], T >= 1, text_len >= 1, 1 + T N + text_len <= 256,
 * d_model = heads * head_dim <= 256 and a multiple of 4 (the GEMM's K), head_dim even in [4, 32], ffn a multiple of 64 in [64, 1024],
 * 1 <= layers <= 32; pre-LN only.  Every violation -- and a process precision other than split-bf16 -- is a negative return code with a message before
 * any launch. */
typedef struct {
  int num_slots, slot_size, T, text_len;   /* N, C, frames per question, text positions (question + choice) */
  int question_len;                        /* multiple choice: text positions < question_len carry the question id pair [1 0], the others [0 1] */
  int d_model, num_heads, ffn_dim, num_layers;
  int vocab, emb_dim;                      /* rows of text_table; E = width of q_embedding (q_in_proj takes E + 4 inputs: E | type pair | text id pair) */
  const float* cls;                        /* [d_model] */
  const float* pos;                        /* [L][d_model]: added to every row, CLS included */
  const float *vision_w, *vision_b;        /* vision_in_proj [d_model][C + 2] (column C + 1 is the vision id [0 1]), [d_model]; 16-byte aligned */
  const float* q_in_proj_w;                /* [d_model][E + 4]: only its type columns E and E + 1 are read */
  const float* text_table;                 /* [vocab][d_model] from sf_aloe_text_table_f32 */
  const sf_tfm_layer* layers;              /* HOST array [num_layers]; the torch-layout pointers only */
} sf_aloe;
int sf_aloe_ok(int num_slots, int slot_size, int T, int text_len, int d_model, int num_heads, int ffn, int num_layers);
/* bytes of the forward's workspace (token rows twice, attention rows, q|k|v, hidden rows); 0 for unsupported arguments or B outside [1, 65535] */
size_t sf_aloe_workspace_bytes(int B, int num_slots, int T, int text_len, int d_model, int ffn);
/* Once per weight version: q_embedding [vocab][E], q_in_proj_w [d_model][E + 4], q_in_proj_b [d_model] ->
 * table[w] = q_in_proj_w[:, :E] q_embedding[w] + q_in_proj_w[:, E + 2] + q_in_proj_b  ([vocab][d_model]; text_token = [1 0] selects column E + 2). */
int sf_aloe_text_table_f32(const float* q_embedding, const float* q_in_proj_w, const float* q_in_proj_b, float* table, int vocab, int emb_dim, int d_model,
                           void* stream);
/* slots: video v, frame f, slot n at slots + v * stride_v + f * stride_t + n * C (strides in elements, multiples of 4; stride_t >= N * C), V videos of
 * T_all frames, read in place.  Batch entry b reads video video_index[b] (int32, device; any order, repeats allowed; NULL: video b) at frames
 * start[b] + t * frame_offset, t < T (start: int32, device; NULL: 0).  tokens [B][text_len] int32 and pad_mask [B][text_len] bytes (1 = padded, never a
 * key) on the device.  multiple_choice: 0 = every text position carries the id pair [0 1]; 1 = see question_len.  head_w1 [mlp_hidden][d_model],
 * head_b1 [mlp_hidden], head_w2 [num_outputs][mlp_hidden], head_b2 [num_outputs] (both <= 1024) -> logits [B][num_outputs]; answers [B] int32 when not
 * NULL: the argmax (first index on ties), for num_outputs == 1 logit > 0.  A video, a frame or the token of an unpadded position outside its table
 * gives NaN logits (answer -1) for that entry, never an access.  workspace: 16-byte aligned, sf_aloe_workspace_bytes(...) bytes. */
int sf_aloe_fwd_f32(const sf_aloe* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index, const int* start,
                    int frame_offset, const int* tokens, const unsigned char* pad_mask, int multiple_choice, const float* head_w1, const float* head_b1,
                    const float* head_w2, const float* head_b2, int mlp_hidden, int num_outputs, float* logits, int* answers, int B, void* workspace,
                    size_t workspace_bytes, void* stream);
/* One launch of one workgroup.  cls_logits [B1][num_answers] with cls_labels [B1] (int32); mc_logits [Bn] with mc_labels [Bn] (f32, 0 / 1), mc_flag [Bn]
 * (int32: the question of every choice, non-decreasing runs) and mc_subtype [Q] (int32; explanatory 1, predictive 2, counterfactual 3; NULL: none).
 * Either kind may be empty (B1 = 0 / Bn = 0, its pointers NULL).  -> losses [2] = mean cross-entropy, mean BCE-with-logits (0 for an empty kind);
 * ques_correct [Q] int32 = every choice of the question has (logit > 0) == label; counts [10] int32, ADDED to what the buffer holds so that batches
 * accumulate: descriptive (right, questions), multiple choice (right, questions), then the same for subtypes 1, 2, 3.  losses and counts may be NULL.
 * A label outside [0, num_answers) gives a NaN loss, an mc_flag outside [0, Q) is skipped: never an access. */
int sf_aloe_score_f32(const float* cls_logits, const int* cls_labels, int B1, int num_answers, const float* mc_logits, const float* mc_labels,
                      const int* mc_flag, int Bn, const int* mc_subtype, int Q, float* losses, int* ques_correct, int* counts, void* stream);

/* SlotRollouter / SingleStepSlotRollouter (slotformer.py:48-134, single_step_slotformer.py:6-90). */
typedef struct {
  int num_slots, slot_size, d_model, num_layers, num_heads, ffn_dim, norm_first;
  int window_len;   /* history_len (sliding window) or cond_len (single-step growing window) */
  int single_step;  /* 0: SlotRollouter, 1: SingleStepSlotRollouter */
  const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;
  const float* pe_tok;          /* [window_len*num_slots, d_model]: enc_t_pe per slot (+ enc_slots_pe) */
  const sf_tfm_layer* layers;   /* HOST array [num_layers] */
  /* optional (NULL = absent): sf_pack_linear_weights() copies of in_proj_w [d_model, slot_size] and out_proj_w
   * [slot_size, d_model].  With them (slot_size 128, d_model 256, packed FFN weights in every layer) a rollout step
   * projects only the newly predicted frame (the in-projections of older frames are cached in the workspace) and
   * out-proj + in-proj run as one launch. */
  const void *in_proj_packed, *out_proj_packed;
} sf_rollouter;

/* nn.Linear weight W [N, K] -> split-bf16 copy in MFMA-fragment order (N % 32 == 0, K % 16 == 0);
 * sf_packed_linear_bytes(N, K) bytes. */
size_t sf_packed_linear_bytes(int N, int K);
int sf_pack_linear_weights(const float* w, void* packed, int N, int K, void* stream);

size_t sf_rollout_workspace_bytes(const sf_rollouter* m, int B);
/* slots: [B, T_total, N, C]; the first n_in frames hold the burn-in slots (n_in = window_len, or 1
 * for single_step); frames n_in .. n_in+pred_len-1 are written.  T_total >= n_in + pred_len. */
int sf_rollout_f32(const sf_rollouter* m, float* slots, int B, int T_total, int pred_len, void* ws,
                   size_t ws_bytes, void* stream);

/* Per-call options of a rollout: they apply to THIS call on the calling thread only (thread-local inside the library; the
 * reference drives forward() from one host thread per GPU, base_slots/extract_slots.py:128), whereas sf_set_precision /
 * sf_set_seam_fused / sf_set_ffn_rows64 set process-wide DEFAULTS.  Every choice is bit-identical except `precision` and `layer_tok` (see there).
 * A process-wide switch is read when a call plans its launches.  A hipGraph captured earlier keeps the form it was captured with. */
typedef struct {
  int precision;    /* -1: default; 0 exact f32, 1 split-bf16, 2 single-pass bf16 (= sf_rollout_bf16), 3 single-pass fp16 (a
                     * measurement probe: the linear layers on one fp16 MFMA per product, profiles/r03_probes.txt) */
  int seam_fused;   /* -1: default; 0 / 1: seam launches off / on */
  int ffn_rows;     /* 0: default; 32 / 64 / 128 rows per workgroup of the chunk-partial FFN launches */
  int attn_heads_per_wg; /* 0: default (2: one workgroup per head pair and video, four partial outputs summed by the FFN launch);
                          * 8: one workgroup per video runs all heads and writes finished rows -- fewer, longer workgroups with
                          * a third of the bytes through a CU: the throughput form (the same bits as the default) */
  int attn_qkv_rows; /* 0: default (off); 128: the attention block as TWO launches -- LN1 + q|k|v on 128-row tiles of the whole
                      * batch (no padding of a video to 64 rows, one weight load per 128 rows), then one workgroup per video
                      * whose eight waves run the eight heads side by side + the out-projection: finished rows like
                      * attn_heads_per_wg = 8, the same bits, less CU time per row (csrc/attn_rows.hip) */
  int ffn_tile;      /* 0: default (off); 1: behind an attention block that writes finished rows (attn_heads_per_wg = 8 or attn_qkv_rows),
                      * the FFN block of the layers before the last as ONE workgroup per 64-row tile that runs all four hidden chunks
                      * on one ingest / LayerNorm with streamed weight fragments and writes finished rows (csrc/ffn_tile.hip) instead of
                      * one workgroup per (tile, hidden chunk) and four partial tensors: the same bits, half the CU time;
                      * 2 (with attn_qkv_rows): that launch also runs LN1 + q|k|v of the NEXT layer on its tile -- the rows never leave
                      * the workgroup, the next attention block is its core launch alone (one launch less per layer, the same bits) */
  int cus_available; /* 0: the whole chip; else the number of CUs the call's stream may use (its CU mask).  Seam launches hand rows over inside
                      * a grid and need every workgroup of it resident at once: they are used only when the grid fits min(160, cus_available) */
  int layer_tok;     /* 0: the process default (sf_set_layer_tok / SF_LAYER_TOK=1; OFF unless set); 1 / -1: on / off.  On (and every layer before the last has tok_packed, windows
                      * of <= 96 tokens; 65..96 -- the reference's Physion window of 15 frames x 6 slots -- outside the pipeline's units): those layers run as ONE token-stationary launch each (csrc/layer_tok.hip) -- a 128-token workgroup owns whole
                      * videos, every product of the layer keeps its activations in registers -- instead of an attention-core launch per video plus an
                      * FFN + q|k|v launch per 64-row tile; the row-pruned last layer keeps the row-tile forms.  Not bit-identical to the other forms
                      * (one accumulator per output block instead of per-chunk partial sums): 1e-6-level differences per layer.
                      * A rollouter of d_model 128, 8 heads, ffn 512 (OBJ3D; the generic GEMM path) takes the same option: with tok_packed on the layers
                      * before the last, norm_first, split-bf16 mode and a sliding window of <= 96 tokens those layers run as ONE launch of
                      * csrc/layer_tok128.hip per step, the last layer stays on the GEMM core (sf_rollout_tok_layers tells which).  Measured
                      * (profiles/layer_tok_d128.md, 6 + 10 frames): FASTER than the GEMM path from 64 videos up (1.43 x at 192, 2.5 x at 512), SLOWER at 32
                      * (188 against 175 us per step: the launch costs about the same whatever it holds) -- pick per batch size */
} sf_rollout_opts;
int sf_set_layer_tok(int on);   /* process default of sf_rollout_opts.layer_tok == 0 */
int sf_get_layer_tok(void);
int sf_rollout_opts_f32(const sf_rollouter* m, float* slots, int B, int T_total, int pred_len, void* ws, size_t ws_bytes,
                        void* stream, const sf_rollout_opts* opts); /* opts == NULL: sf_rollout_f32 */
/* Rollout at a frame offset, every phase of a video in ONE call (rollout_clevrer_slots.py:20-65 with frame_offset 2,
 * rollout_physion_slots.py:22-63 with 3: the reference rolls a video forward frame_offset times, once per phase, and interleaves).
 * slots [B, T_total, N, C]; f = frame_offset >= 1, hist = window_len (1 for a single-step rollouter, which takes f == 1 only),
 * first = obs - hist * f >= 0.  Phase p < f burns in on frames first + p + j * f (j < hist) and writes frame obs + p + s * f at
 * step s; all phases run S = ceil(pred_len / f) steps, so frames obs .. obs + S * f - 1 are written -- every one of them, there is
 * no masked write: T_total >= obs + S * f, and a caller who wants exactly pred_len frames pads the buffer and slices.  Frames
 * before `first`, the burn-in frames and frames from obs + S * f on are never written.
 * A phase is a VIRTUAL VIDEO v = b * f + p: the call is planned, and runs the launches, of a rollout of B * f videos (whatever
 * path that is: fused ring with or without seams, row tiles, long window, generic GEMMs, token-stationary layers), and its
 * workspace is that of B * f videos.  Where sf_rollout_is_fused promises batch-independent bits, the result equals, bit for bit,
 * sf_rollout_opts_f32 run once per phase on gathered copies; with f == 1 and obs == hist it IS sf_rollout_opts_f32.
 * An argument error before any launch: f < 1, a single-step rollouter with f > 1, first < 0, a buffer that is too short, null pointers.
 * opts == NULL: the thread's defaults. */
size_t sf_rollout_phases_workspace_bytes(const sf_rollouter* m, int B, int frame_offset);
int sf_rollout_phases_f32(const sf_rollouter* m, float* slots, int B, int T_total, int obs, int frame_offset, int pred_len, void* ws,
                          size_t ws_bytes, void* stream, const sf_rollout_opts* opts);
/* 1 when sf_rollout_f32 runs this model's Transformer layers as the fused per-video / per-row launches (d_model 256, 8 heads,
 * ffn 1024, window <= 64 tokens, packed weights, split-bf16 mode): a video's result then does not depend on the batch it is in -- bit for bit in the
 * row-tile / latency forms; with layer_tok on, to ~1e-6 per layer (a video's last bits depend on its position modulo the videos of a workgroup) */
int sf_rollout_is_fused(const sf_rollouter* m);
/* 1 when the layers before the last can run as token-stationary launches (sf_rollout_opts.layer_tok): fused-layer path, tok_packed on those layers,
 * every window of the rollout within the kernel's limits (whether layer_tok is on is not asked) */
int sf_rollout_tok_ok(const sf_rollouter* m);
/* How many leading layers a rollout of B videos with these options (NULL: the process defaults) runs as token-stationary launches, on whatever path:
 * 0 or num_layers - 1.  Unlike sf_rollout_tok_ok it asks whether layer_tok is ON for the call and counts every path that takes the launches: the
 * fused-layer path, the long-window path (65..96 tokens) and the generic path at (128, 8, 512), for which sf_rollout_tok_ok and sf_rollout_is_fused
 * stay 0.  Reads no weight and needs no GPU. */
int sf_rollout_tok_layers(const sf_rollouter* m, int B, const sf_rollout_opts* opts);
/* 1 when sf_rollout_f32 may run seam launches for this model / batch with the calling thread's defaults: the fused-layer path with
 * packed in/out projections in split-bf16 mode, seams on, head-pair attention (attn_heads_per_wg 8, attn_qkv_rows and the
 * token-stationary layers take other forms), a grid that fits the CUs, and a window of some step after the first that a seam launch
 * accepts; 0 when none can run */
int sf_rollout_uses_seam(const sf_rollouter* m, int B);
/* ... with the options of the call in question (NULL: the thread's defaults), precision included: a caller on a CU-masked stream passes
 * its cus_available */
int sf_rollout_uses_seam_opts(const sf_rollouter* m, int B, const sf_rollout_opts* opts);

/* ---- differentiable building blocks for the slot-level layers --------------------------------
 * (predictor, kernel distribution: savi.py:190-200, predictor.py:47-73).  Backward of y = act(x W^T + b): dW [N,K],
 * db [N] (or NULL), dx [M,K] (or NULL); with relu != 0, dy is first masked in place by y > 0.  N, K multiples of 64. */
size_t sf_linear_bwd_workspace_bytes(long long M, int N, int K);
int sf_linear_bwd_f32(const float* x, const float* W, const float* y, float* dy, float* dx, float* dW, float* db, long long M,
                      int N, int K, int relu, void* ws, size_t ws_bytes, void* stream);
/* Attention core of nn.MultiheadAttention under autograd (predictor.py:33-38 in train mode): qkv [B*L, 3d] (q|k|v) -> ctx
 * [B*L, d]; dropout on the softmax weights with masks that are a pure function of (seed, element); the backward call
 * recomputes the probabilities.  Accepted: L <= 128 and head_dim <= 64 where the backward kernel's tile fits the 160 KB of
 * LDS, the same range for both calls.  Head dim 32 / 64 with L <= 96 runs on the MFMA kernels, whose tiles pad L to Lp (a
 * multiple of 32): 4 Lp (hd + 1) + 2 Lp (Lp + 1) floats; every other shape on the scalar kernels, 4 L (hd + 1) + 2 L (L + 1)
 * floats.  So head dim 64 stops at L = 64 and head dim 32 at L = 113; head dim 16 reaches L = 126, head dim 48 L = 101.
 * Other shapes return an argument error before any launch. */
int sf_mha_train_fwd_f32(const float* qkv, float* ctx, int B, int L, int d_model, int num_heads, float dropout_p,
                         unsigned long long seed, void* stream);
int sf_mha_train_bwd_f32(const float* qkv, const float* d_ctx, float* d_qkv, int B, int L, int d_model, int num_heads,
                         float dropout_p, unsigned long long seed, void* stream);
/* y = res + dropout(x) (nn.Dropout in train mode; res may be NULL; n % 4 == 0).  Its backward is the same call on dy. */
int sf_dropout_f32(const float* x, const float* res, float* y, long long n, float dropout_p, unsigned long long seed,
                   void* stream);
/* torch.optim.Adam (the reference's optimiser: slotformer_clevrer_params.py:16-19, stosavi_clevrer_params.py:14-17; no
 * weight decay, no amsgrad) over one flat fp32 bucket of n elements; step is the 1-based step count. */
int sf_adam_flat_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, int step, float lr,
                     float beta1, float beta2, float eps, void* stream);
/* Gradient clipping by global norm on the flat bucket (torch.nn.utils.clip_grad_norm_; clip_grad = 0.05 in the StoSAVi,
 * SAVi and STEVE configurations, base_slots/method.py).  ONE launch, nothing read back: out3 (device, 3 floats) receives
 * the L2 norm of grad[0..n), the coefficient min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0) and 1.0 / 0.0 for
 * "some element is NaN or +-Inf".  Elements are accumulated in fp32 per thread and in double from the wave on; the result
 * is bit-identical from call to call.  ws: the workspace query's bytes, 16-byte aligned, ZERO-FILLED before its first use;
 * every call leaves its arrival counter (the first 4 bytes) at zero again, so one workspace serves any later n it is large enough for. */
size_t sf_grad_norm_workspace_bytes(long long n);
int sf_grad_clip_coef_f32(const float* grad, long long n, float max_norm, float* out3, void* ws, size_t ws_bytes,
                          void* stream);
/* Adam as above with parameter groups (torch.optim.Adam's param_groups; STEVE's lr / dec_lr, base_slots/method.py:237-276):
 * group k owns the elements from groups[k].begin up to the next group's begin (the last one up to n) and steps at groups[k].lr.
 * groups: HOST array, begins ascending, groups[0].begin == 0, at most SF_ADAM_MAX_GROUPS of them.  grad_scale: NULL, or a
 * DEVICE pointer to one float that every gradient element is multiplied by before it enters the moments -- the coefficient
 * written by the clip call above (out3 + 1), so clipping costs no pass and no host round trip; grad itself is not modified.
 * With one group and grad_scale == NULL the result equals the plain entry point's bit for bit. */
#define SF_ADAM_MAX_GROUPS 8
typedef struct {
  long long begin;
  float lr;
} sf_adam_group;
int sf_adam_flat_groups_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, int step,
                            const sf_adam_group* groups, int num_groups, float beta1, float beta2, float eps,
                            const float* grad_scale, void* stream);
/* Backward of nn.LayerNorm over the last dimension (D <= 1024, D % 4 == 0). */
size_t sf_layernorm_bwd_workspace_bytes(int D);
int sf_layernorm_bwd_f32(const float* x, const float* dy, const float* gamma, float* dx, float* dgamma, float* dbeta,
                         long long rows, int D, float eps, void* ws, size_t ws_bytes, void* stream);

/* ---- the SAVi image encoder under autograd ------------------------------------------------
 * conv stack + soft position embedding + per-pixel MLP (savi.py:220-250, 367-377; utils.py:52-63) with all weight
 * gradients.  Parameters in TORCH layouts (conv weights [Cout,Cin,5,5] for every layer; the node packs what its kernels
 * need into the workspace on every call, because an optimizer step changes them).  The reference encoder only: 64
 * channels, 5x5 kernels, a 64x64 feature map (first conv stride 2 at 128x128 input). */
typedef struct {
  int resolution, layers, channels, ks, hidden, out_channels;
  const float* conv_w[8];
  const float* conv_b[8];
  const float *pos_grid, *pos_w, *pos_b;   /* SoftPositionEmbed: grid [64*64, 4] (buffer), dense.weight [C,4], dense.bias [C] */
  const float *ln_g, *ln_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;   /* encoder_out_layer */
} sf_savi_features;

typedef struct {
  float* conv_w[8];
  float* conv_b[8];
  float *pos_w, *pos_b, *ln_g, *ln_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} sf_savi_features_grads;

size_t sf_savi_features_train_workspace_bytes(const sf_savi_features* m, int F);
/* frame f (NCHW [3,H,W]) at img + f*frame_stride floats -> out [F, 64*64, out_channels] */
int sf_savi_features_train_fwd_f32(const sf_savi_features* m, const float* img, long long frame_stride, int F, float* out,
                                   void* ws, size_t ws_bytes, void* stream);
int sf_savi_features_train_bwd_f32(const sf_savi_features* m, const float* img, long long frame_stride, const float* d_out,
                                   const sf_savi_features_grads* g, int F, void* ws, size_t ws_bytes, void* stream);

/* ---- training of the Slot-Attention module ------------------------------------------------
 * SlotAttention (savi.py:36-102) under autograd: parameters in torch layouts, gradients with the same shapes (written,
 * not accumulated).  The forward keeps its activations in the caller's workspace for the backward call.
 * slot_size 64 / 128 / 192 / 256, in_features and mlp_hidden multiples of 64, at most 16 slots and 8 iterations. */
typedef struct {
  int in_features, slot_size, mlp_hidden, num_slots;
  const float *norm_in_g, *norm_in_b, *wk, *wv;                  /* norm_inputs, project_k / project_v [D, in] */
  const float *q_ln_g, *q_ln_b, *wq;                             /* project_q = LayerNorm + Linear [D, D] */
  const float *gru_w_ih, *gru_w_hh, *gru_b_ih, *gru_b_hh;        /* nn.GRUCell [3D, D] x2, [3D] x2 */
  const float *mlp_ln_g, *mlp_ln_b, *mlp_w1, *mlp_b1, *mlp_w2, *mlp_b2;
  float eps;
} sf_slot_attention;

typedef struct {
  float *norm_in_g, *norm_in_b, *wk, *wv, *q_ln_g, *q_ln_b, *wq, *gru_w_ih, *gru_w_hh, *gru_b_ih, *gru_b_hh;
  float *mlp_ln_g, *mlp_ln_b, *mlp_w1, *mlp_b1, *mlp_w2, *mlp_b2;
} sf_slot_attention_grads;

size_t sf_slot_attention_train_workspace_bytes(const sf_slot_attention* m, int B, int HW, int iters);
/* inputs [B, HW, in_features], slots_in [B, N, D] -> slots_out [B, N, D] after `iters` iterations */
int sf_slot_attention_train_fwd_f32(const sf_slot_attention* m, const float* inputs, const float* slots_in, int B, int HW,
                                    int iters, float* slots_out, void* ws, size_t ws_bytes, void* stream);
/* d_slots_out [B, N, D] -> d_slots_in, parameter gradients and (if d_inputs != NULL) d_inputs [B, HW, in_features] */
int sf_slot_attention_train_bwd_f32(const sf_slot_attention* m, const float* inputs, const float* d_slots_out, float* d_inputs,
                                    float* d_slots_in, const sf_slot_attention_grads* g, int B, int HW, int iters, void* ws,
                                    size_t ws_bytes, void* stream);

/* ---- training of the rollout Transformer ------------------------------------
 * SlotFormer.forward in train mode (slotformer.py:263-282) -> SlotRollouter.forward (:85-126) under autograd, i.e. what
 * `loss.backward()` of calc_train_loss (:284-318) differentiates.  The forward keeps every activation of every rollout
 * step in the caller's workspace; the backward pass reads them, so the workspace must stay untouched in between.
 * Gradient buffers mirror the parameter leaves of sf_tfm_layer / sf_rollouter (same shapes) and are WRITTEN, not
 * accumulated.  Dropout (nn.TransformerEncoderLayer default p = 0.1 in train mode): masks are a pure function of
 * (seed, step, layer, site, element); pass the same dropout_p / seed to both calls.  Both rollouters (x holds
 * history_len burn-in frames, or ONE frame for single_step), norm_first layers, slot_size / d_model / ffn_dim multiples of 64, window of at most 128 tokens. */
typedef struct {
  float *norm1_g, *norm1_b, *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;
  float *norm2_g, *norm2_b, *lin1_w, *lin1_b, *lin2_w, *lin2_b;
} sf_tfm_layer_grads;

typedef struct {
  float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;
  const sf_tfm_layer_grads* layers; /* HOST array [num_layers] */
  float* pe_tok; /* [window_len * num_slots, d_model] gradient of the folded position table sf_rollouter.pe_tok (the caller sums it
                    over slots / frames into enc_t_pe / enc_slots_pe, slotformer.py:103-109), or NULL: tables are fixed ('sin') */
} sf_rollouter_grads;

size_t sf_rollout_train_workspace_bytes(const sf_rollouter* m, int B, int pred_len);
/* x [B, history_len, N, C] burn-in slots -> pred [B, pred_len, N, C] */
int sf_rollout_train_fwd_f32(const sf_rollouter* m, const float* x, float* pred, int B, int pred_len, float dropout_p,
                             unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
/* d_pred [B, pred_len, N, C] -> parameter gradients in *g and (if d_x != NULL) d_x [B, history_len, N, C] */
int sf_rollout_train_bwd_f32(const sf_rollouter* m, const float* d_pred, float* d_x, const sf_rollouter_grads* g, int B,
                             int pred_len, float dropout_p, unsigned long long seed, void* ws, size_t ws_bytes,
                             void* stream);

/* ---- Training of the PHYRE task-success readout (csrc/phyre_readout_train.hip; phyre_planning.fit) ------------------------------------------
 * PHYREReadout.forward in train mode + the gradient of its logits: tokens as sf_phyre_readout_fwd_f32 builds them (slots read in place through
 * (stride_v, stride_t), batch entry b = video video_index[b] or b, sel [T] HOST frame numbers, -1 = a frame of zeros), then ONE launch per layer
 * in each direction and one for the head.  Limits: sf_phyre_readout_ok.  Split-bf16 products whatever sf_set_precision says -- any other process
 * precision is refused.  All parameter pointers are DEVICE memory in torch layouts (`layers`: a HOST array, the torch-layout leaves only; the
 * packed copies are not read); the calls split / transpose what their kernels need into the workspace themselves, every call, so the weights may
 * change between steps.  Dropout (p of nn.TransformerEncoderLayer; 0: no mask is evaluated): a pure function of (seed, layer, site, element) --
 * csrc/dropout_mask.h, train.dropout_keep_mask; pass the same dropout_p / seed / slot arguments to both calls and leave the workspace (16-byte
 * aligned, sf_phyre_readout_train_workspace_bytes; 0 for unsupported arguments) untouched in between.
 * video_index is TRUSTED, as the index arrays of sf_rollout_train_clips_fwd_f32: it is not read back; an entry outside [0, V) gives NaN logits and
 * contributes nothing to d in_proj_w, never an address -- validate it on the host once (phyre_planning.fit does).
 * Every argument error (shape, NULL, alignment, workspace too small, sel outside [-1, T_all), process precision) is a negative return code before
 * any launch.  No allocation and no synchronisation inside the calls; equal inputs give equal bits (fixed summation orders, no float atomics). */
typedef struct {
  int num_slots, slot_size, d_model, num_heads, ffn_dim, num_layers;
  const float *in_proj_w, *in_proj_b; /* [d_model, slot_size], [d_model] */
  const float *enc_t_pe, *cls;        /* [T, d_model], [d_model] */
  const sf_tfm_layer* layers;         /* HOST array [num_layers] */
  const float *mlp_w1, *mlp_b1, *mlp_w2, *mlp_b2; /* cls_mlp: [d_model, d_model], [d_model], [d_model], [1] */
} sf_phyre_readout_model;

/* The same leaves; gradients are WRITTEN, not accumulated (slices of a flat optimiser bucket are fine; the layer leaves 16-byte aligned). */
typedef struct {
  float *in_proj_w, *in_proj_b;
  float *enc_t_pe, *cls;              /* enc_t_pe: NULL for a fixed ('sin') table */
  const sf_tfm_layer_grads* layers;   /* HOST array [num_layers] */
  float *mlp_w1, *mlp_b1, *mlp_w2, *mlp_b2;
} sf_phyre_readout_grads;

size_t sf_phyre_readout_train_workspace_bytes(const sf_phyre_readout_model* m, int B, int T);
/* -> logits [B].  gates (or NULL): [num_layers][B * L][ffn_dim] bytes, the ReLU decisions of the layers (1: passed); head_gates (or NULL):
 * [B][d_model] bytes, those of the head.  The backward reads the decisions the forward kept in the workspace, it never re-decides a sign. */
int sf_phyre_readout_train_fwd_f32(const sf_phyre_readout_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all,
                                   const int* video_index, const int* sel, int B, int T, float dropout_p, unsigned long long seed, float* logits,
                                   unsigned char* gates, unsigned char* head_gates, void* ws, size_t ws_bytes, void* stream);
/* g [B] = d loss / d logit -> every parameter gradient in *grads (the slots are frozen inputs and get none) */
int sf_phyre_readout_train_bwd_f32(const sf_phyre_readout_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all,
                                   const int* video_index, const int* sel, int B, int T, const float* g, const sf_phyre_readout_grads* grads,
                                   float dropout_p, unsigned long long seed, void* ws, size_t ws_bytes, void* stream);

/* ---- Training of the Aloe reasoner (csrc/aloe_train.hip; clevrer_vqa.fit, train.aloe_with_grad) ---------------------------------------------------
 * CLEVRERTransformerModel.forward in train mode + the gradient of its logits, as the reference's clevrer_vqa/method.py step differentiates it.  A
 * batch is ONE pass over B = B1 + Bn sequences: the B1 descriptive questions first, then the Bn choices of the multiple-choice questions (the order
 * the dataset collates); slots, video_index, start, frame_offset, tokens [B][text_len], pad_mask [B][text_len] as sf_aloe_fwd_f32 takes them.  The
 * launch chain is that of sf_aloe_fwd_f32 (no row-pruned last layer) with the text table recomputed every call and the four dropout sites of
 * nn.TransformerEncoderLayer (dropout_p == 0: no mask is evaluated): masks are a pure function of (seed, layer, site, element) -- csrc/dropout_mask.h,
 * train.dropout_keep_mask; element index site 0: ((b heads + h) L + i) L + j, sites 1 and 3: (b L + token) d_model + c, site 2: (b L + token) ffn + j.
 * Pass the same batch / dropout_p / seed to both calls and leave the workspace (16-byte aligned, sf_aloe_train_workspace_bytes; 0 for unsupported
 * arguments or B outside [1, 65535]) untouched in between.  All parameter pointers are DEVICE memory in torch layouts (`layers`: a HOST array, the
 * torch-layout leaves only), read every call, so they may move between steps; gradients are WRITTEN, not accumulated.  Aligned to 16 bytes: slots,
 * vision_w, every layer's matrices and LayerNorm parameters, and the gradients of every layer's matrices and biases; every other leaf may stand at
 * an odd offset of a flat bucket.  Limits: sf_aloe_train_ok == sf_aloe_ok; B heads L^2 < 2^32.  Split-bf16 products whatever sf_set_precision says:
 * any other process precision is refused.  Every argument error (shape, NULL, alignment, workspace too small, precision, B) is a negative return
 * code with a message before any launch.  video_index / start / tokens are TRUSTED as in sf_aloe_fwd_f32: an entry outside its table is never an
 * address -- it is a zero operand and gives NaN logits for its sequence; a loss over them is NaN and so is every gradient of that step (validate
 * the indices on the host once: clevrer_vqa.fit does).  No allocation, no synchronisation; fixed summation orders, no float atomics. */
typedef struct {
  int num_slots, slot_size, T, text_len, question_len;
  int d_model, num_heads, ffn_dim, num_layers;
  int vocab, emb_dim;                      /* q_embedding [vocab][emb_dim] */
  int mlp_hidden, num_answers;             /* both answer MLPs: d_model -> mlp_hidden -> num_answers (cls) / 1 (mc) */
  const float* cls;                        /* [d_model] */
  const float* pos;                        /* [L][d_model] */
  const float *vision_w, *vision_b;        /* [d_model][C + 2], [d_model] */
  const float* q_embedding;
  const float *q_in_proj_w, *q_in_proj_b;  /* [d_model][emb_dim + 4], [d_model] */
  const sf_tfm_layer* layers;              /* HOST array [num_layers] */
  const float *cls_w1, *cls_b1, *cls_w2, *cls_b2;
  const float *mc_w1, *mc_b1, *mc_w2, *mc_b2;
} sf_aloe_model;

/* The same leaves (d vision_w column C is 0, d q_in_proj_w column emb_dim + 3 is 0: their inputs are 0). */
typedef struct {
  float *cls, *pos, *vision_w, *vision_b, *q_embedding, *q_in_proj_w, *q_in_proj_b;
  const sf_tfm_layer_grads* layers;        /* HOST array [num_layers] */
  float *cls_w1, *cls_b1, *cls_w2, *cls_b2;
  float *mc_w1, *mc_b1, *mc_w2, *mc_b2;
} sf_aloe_grads;

int sf_aloe_train_ok(int num_slots, int slot_size, int T, int text_len, int d_model, int num_heads, int ffn, int num_layers);
size_t sf_aloe_train_workspace_bytes(const sf_aloe_model* m, int B);
/* -> cls_logits [B1][num_answers], mc_logits [Bn] (NULL for an empty kind).  gates (or NULL): [num_layers][B * L][ffn] bytes, the ReLU decisions of
 * the layers (1: passed); head_gates (or NULL): [B][mlp_hidden] bytes, those of each sequence's head. */
int sf_aloe_train_fwd_f32(const sf_aloe_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index,
                          const int* start, int frame_offset, const int* tokens, const unsigned char* pad_mask, int B1, int Bn, float dropout_p,
                          unsigned long long seed, float* cls_logits, float* mc_logits, unsigned char* gates, unsigned char* head_gates, void* ws,
                          size_t ws_bytes, void* stream);
/* g_cls [B1][num_answers], g_mc [Bn] = d loss / d logits -> every parameter gradient in *grads; a kind without rows leaves zeros in its head. */
int sf_aloe_train_bwd_f32(const sf_aloe_model* m, const float* slots, long long stride_v, long long stride_t, int V, int T_all, const int* video_index,
                          const int* start, int frame_offset, const int* tokens, const unsigned char* pad_mask, int B1, int Bn, const float* g_cls,
                          const float* g_mc, const sf_aloe_grads* grads, float dropout_p, unsigned long long seed, void* ws, size_t ws_bytes, void* stream);
/* One launch of one workgroup: losses [2] as sf_aloe_score_f32 computes them (mean cross-entropy, mean BCE-with-logits, in double; 0 for an empty
 * kind) and the gradient of w_cls * losses[0] + w_mc * losses[1]: g_cls [B1][num_answers] = w_cls (softmax - onehot) / B1, g_mc [Bn] =
 * w_mc (sigmoid - label) / Bn.  losses, g_cls, g_mc may be NULL. */
int sf_aloe_score_grad_f32(const float* cls_logits, const int* cls_labels, int B1, int num_answers, const float* mc_logits, const float* mc_labels, int Bn,
                           float w_cls, float w_mc, float* losses, float* g_cls, float* g_mc, void* stream);

/* ---- SlotFormer training on clips of a device-resident table (csrc/clip_train.hip; video_prediction.fit) ----------------------------------
 * A batch is B (video, start) pairs in two int32 DEVICE arrays, never a gathered copy.  The index arrays are TRUSTED: they are not read back,
 * so a pair outside the table reads outside it -- validate them on the host once, before the loop (video_prediction.fit does).  What the host
 * does know is checked: a clip of (burn-in + pred_len) frames at this frame_offset must fit T_total.
 *
 * sf_rollout_train_fwd_f32 whose burn-in frame j of clip b is table[clip_video[b], clip_start[b] + j * frame_offset]; table [V, T_total, N, C]
 * float32, 16-byte aligned.  The burn-in is window_len frames, ONE frame for a single-step rollouter.  Workspace: the layout of
 * sf_rollout_train_workspace_bytes, so sf_rollout_train_bwd_f32 follows as it is. */
int sf_rollout_train_clips_fwd_f32(const sf_rollouter* m, const float* table, int T_total, const int* clip_video, const int* clip_start,
                                   int frame_offset, float* pred, int B, int pred_len, float dropout_p, unsigned long long seed, void* ws,
                                   size_t ws_bytes, void* stream);
/* The squared-error loss of a rollout and its gradient in ONE launch (slotformer.py:289-318).  pred [B, S, E] dense; target element (b, s, e) at
 * target[((vid(b) * T_total + start(b) + first_frame + s * frame_step) * E + e], vid(b) = clip_video[b] (NULL: b), start(b) = clip_start[b] (NULL: 0).
 * Targets in the slot table: T_total, first_frame = burn-in * frame_offset, frame_step = frame_offset, E = N * C.  Dense targets [B, S, E]: both
 * index arrays NULL, T_total = S, first_frame = 0, frame_step = 1.  step_w [S] device weights or NULL (1).  clip_len [B] int32 or NULL: step s of
 * clip b counts iff hist + s < clip_len[b] (the reference's vid_len rule); count = counted elements.
 *   d_pred [B, S, E] (may be NULL) = scale * w_s * 2 * (pred - target) / count, 0 where not counted (three float32 roundings per element)
 *   stats [1 + 2 S] float64, every entry ADDED to: the weighted loss scale * sum_s w_s * sum (pred - target)^2 / count; the UNWEIGHTED sum of
 *   squares of each step; the counted elements of each step.  With count == 0 the loss entry is left alone and d_pred is 0.
 * float32 squares accumulated in float64, per-workgroup partials combined in index order by the last workgroup to arrive: bit-identical from call to
 * call.  ws: the workspace query's bytes, 16-byte aligned, ZERO-FILLED before its first use; every call leaves its arrival counter at zero.
 * E % 4 == 0, S <= 64; pred, target, d_pred 16-byte aligned. */
size_t sf_clip_mse_workspace_bytes(int B, int S, long long E);
int sf_clip_mse_f32(const float* pred, const float* target, const int* clip_video, const int* clip_start, int T_total, int first_frame,
                    int frame_step, const float* step_w, const int* clip_len, int hist, float scale, float* d_pred, double* stats, int B, int S,
                    long long E, void* ws, size_t ws_bytes, void* stream);
/* Target frames of the image loss: table [V, T_total, H, W, 3] uint8, already at the model's resolution -> out [B, S, 3, H, W] float32, frame
 * (b, s) = table[clip_video[b], clip_start[b] + first_frame + s * frame_step], normalised (x / 255 - mean_c) / std_c with the arithmetic of
 * sf_ingest_frames_u8 at equal source and output size (the same bits).  mean3 / std3: three HOST floats each. */
int sf_clip_frames_f32(const unsigned char* table, int T_total, const int* clip_video, const int* clip_start, int first_frame, int frame_step,
                       const float* mean3, const float* std3, float* out, int B, int S, int H, int W, void* stream);

/* ---- The stochastic kernels of StoSAVi in training (csrc/kernel_sample.hip, csrc/normal_noise.h; base_slots.fit) ------------------------------
 * Standard-normal noise as a pure function of (seed, tag, element index): out[i] = eps(seed, tag, i), n <= 2^31 elements.
 *   s   = mix32((u32)seed ^ mix32((u32)(seed >> 32) + 0x9e3779b9 * (tag + 1)))           (mix32: the dropout masks' finaliser)
 *   u1  = ((mix32((2 i) ^ s) >> 9) + 0.5) * 2^-23,  u2 the same from 2 i + 1               (exact in float32)
 *   eps = sqrtf(-2 logf(u1)) * cosf(6.2831855f * u2)                                      (full-precision functions; |eps| <= 5.77)
 * The two entry points below call the same device function, so a seed gives them these bits; train.normal_noise restates it on the host. */
int sf_normal_noise_f32(float* out, long long n, unsigned long long seed, unsigned tag, void* stream);
/* dist [R, 2 D] = (mu | log_var) -> kernels [R, D] = mu + eps * exp(0.5 * log_var) (savi.py:355-365).  eps = noise [R, D] when given, else
 * eps(seed, tag, r * D + c), generated in registers.  *kld_sum, a DEVICE double, is ADDED to: the sum over rows and channels of
 * 0.5 * (prior_log_var - log_var) + exp(log_var) / (2 exp(prior_log_var)) - 0.5 -- savi.py:337-353 with the prior at the posterior's mean, before
 * its mean over rows -- evaluated per element in float32 as 0.5 * (expm1f(x) - x), x = log_var - prior_log_var (the same value without the
 * cancellation near x = 0), accumulated in float64, per-workgroup partials combined in index order by the last workgroup to arrive: bit-identical
 * from call to call.  ws: the workspace query's bytes, 16-byte aligned, ZERO-FILLED before its first use; every call leaves its arrival counter at
 * zero.  D % 4 == 0, D <= 1024, R >= 1, R * D <= 2^31; dist, noise, kernels 16-byte aligned.  The query returns 0 for a refused shape. */
size_t sf_kernel_sample_workspace_bytes(long long R, int D);
int sf_kernel_sample_fwd_f32(const float* dist, const float* noise, unsigned long long seed, unsigned tag, float prior_log_var, float* kernels,
                             double* kld_sum, long long R, int D, void* ws, size_t ws_bytes, void* stream);
/* Its gradient; eps is the same tensor or is regenerated from (seed, tag), never stored.  d_kernels [R, D] (NULL: zero); d_kld a DEVICE float, the
 * gradient arriving at the mean KL term; kld_scale a host float, 1 / rows of that mean.  d_dist [R, 2 D] = (d_mu | d_log_var):
 *   d_mu      = d_kernels
 *   d_log_var = d_kernels * eps * 0.5 * exp(0.5 * log_var) + d_kld * kld_scale * 0.5 * (exp(log_var - prior_log_var) - 1) */
int sf_kernel_sample_bwd_f32(const float* dist, const float* noise, unsigned long long seed, unsigned tag, float prior_log_var,
                             const float* d_kernels, const float* d_kld, float kld_scale, float* d_dist, long long R, int D, void* stream);

/* StoSAVi / STEVE encoder side (savi.py:177-250,295-322,367-416; steve.py:198-240). */
typedef struct {
  int resolution;      /* input H == W (64 or 128) */
  int enc_layers;      /* number of convs (<= 8) */
  int enc_channels[9]; /* enc_channels[0] = 3 */
  int enc_ks;
  int enc_out_channels, num_slots, slot_size, slot_mlp_size, num_iterations;
  const float* conv_w[8]; /* [0]: torch [C1,3,ks,ks]; [i>0]: packed [Cout,ks,ks,Cin] */
  const float* conv_b[8]; /* may be NULL */
  const float* pos_table; /* [64*64, C_last] */
  const float *enc_ln_g, *enc_ln_b, *enc_fc1_w, *enc_fc1_b, *enc_fc2_w, *enc_fc2_b;
  const float *sa_norm_in_g, *sa_norm_in_b, *sa_q_ln_g, *sa_q_ln_b, *sa_q_w;
  const float* sa_kv_w; /* [2*slot_size, enc_out_channels] = cat(project_k.weight, project_v.weight) */
  const float *gru_w_ih, *gru_w_hh, *gru_b_ih, *gru_b_hh; /* matrices transposed: [D,3D] */
  const float *mlp_ln_g, *mlp_ln_b, *mlp_w1, *mlp_b1, *mlp_w2, *mlp_b2; /* mlp_w1 [D,H], mlp_w2 [H,D] (transposed) */
  const float* init_latents; /* [N, D] */
  int kd_mode;               /* 0: none (STEVE), 1: Linear, 2: Linear-LN-ReLU-Linear (kernel_mlp) */
  const float *kd_w0, *kd_b0, *kd_ln_g, *kd_ln_b, *kd_w3, *kd_b3;
  int pred_type;             /* 0: ResidualMLPPredictor, 1: TransformerPredictor */
  int pred_rnn, pred_norm_first, pred_num_layers, pred_num_heads, pred_ffn_dim, pred_hidden;
  const float *pm_ln_g, *pm_ln_b, *pm_w0, *pm_b0, *pm_w2, *pm_b2;
  const sf_tfm_layer* pred_layers; /* HOST array */
  const float *lstm_w_ih, *lstm_w_hh, *lstm_b_ih, *lstm_b_hh, *proj_w, *proj_b;
  float sa_eps;
  const float* sa_q_w_t; /* optional: project_q weight transposed [in, out] (coalesced reads for the slot-update kernel, which
                          * then also emits the next iteration's q); NULL: q comes from a separate LN-fused GEMM launch */
  /* optional transposed ([in, out]) copies of the ResidualMLPPredictor weights and of the single-Linear kernel_dist layer:
   * with them (and sa_q_w_t) the per-frame slot prologue -- predictor, kernel distribution, sampling, q projection -- is ONE
   * launch (pred_type 0, no LSTM, kd_mode 1); NULL: separate LayerNorm / GEMM / sampling launches */
  const float *pm_w0_t, *pm_w2_t, *kd_w0_t;
  /* optional (slot size 128, slot MLP 256): sf_pack_linear_weights copies of the torch-layout GRUCell weight_ih / weight_hh
   * [3D, D], Slot-Attention mlp[1].weight [H, D], mlp[3].weight [D, H] and project_q[1].weight [D, D]; with all five the slot
   * update after every Slot-Attention iteration runs on the matrix cores (split-bf16, like the other bf16x3 kernels) */
  const void *sa_gru_ih_p, *sa_gru_hh_p, *sa_mlp_w1_p, *sa_mlp_w2_p, *sa_q_w_p;
  /* optional: Slot Attention with the key / value projections FOLDED away (project_k / project_v are bias-free Linears,
   * savi.py:44-45, so  k.q = x.(Wk^T q)  and  sum_p a v = Wv (sum_p a x)):  the attention runs on the normalised pixel features x
   * themselves -- half the bytes of k|v, and the [Wk;Wv] GEMM disappears -- with
   *   sa_fold_q_w   = Wk^T Wq   [C, D]  in place of project_q[1].weight  (its transposed [D, C] and packed copies beside it)
   *   sa_fold_gru_ih = W_ih Wv  [3D, C] in place of GRUCell.weight_ih    (transposed [C, 3D] and packed copies)
   * Used when all are given, enc_out_channels == slot_size == 128 (or 192 with enc_fc1_p / enc_fc2_p) and the split-bf16 mode is on. */
  const float *sa_fold_q_w, *sa_fold_q_w_t, *sa_fold_gru_ih_t;
  const void *sa_fold_q_w_p, *sa_fold_gru_ih_p;
  /* optional (pred_type 1, pre-LN, 4 heads, N <= 8; slot size / ffn / LSTM hidden 128 / 512 / 256 or 64 / 128 / 128):
   * HOST array of sf_pack_linear_weights copies -- [4 l + 0..3] = predictor layer l's in_proj_weight [3D, D], out_proj.weight
   * [D, D], linear1.weight [F, D], linear2.weight [D, F]; then, with the LSTM wrapper, weight_ih_l0 [4H, D], weight_hh_l0 [4H, H],
   * out_projector.weight [D, H].  With it the predictor step of a frame (predictor.py:20-44,76-135) is ONE launch instead of
   * 8 + 4 (split-bf16, like the other bf16x3 kernels); NULL: the unfused chain. */
  const void** pred_packed;
  /* optional (encoder_out_layer 64 -> 192 -> 192, i.e. STEVE on Physion): sf_pack_linear_weights copies of enc_fc1_w [192, 64] and
   * enc_fc2_w [192, 192]; with them and the sa_fold_* copies the per-pixel chain up to the normalised Slot-Attention inputs is one
   * launch (pixel_mlp.hip) and Slot Attention runs folded at width 192 as well */
  const void *enc_fc1_p, *enc_fc2_p;
  /* optional (NULL = absent), per conv i > 0 with 64 -> 64 channels, 5 x 5, on the 64 x 64 grid: sf_pack_conv_frag_weights copies of
   * conv_w[i].  With one, the conv runs on 4-row tiles with its weights streamed as MFMA fragments (csrc/conv_rows4.hip; split-bf16
   * mode) instead of the 2-row tile kernel that passes every tap's weights through LDS -- the same products in the same order. */
  const void* conv_w_frag[8];
  /* optional (slot size 128; pred_type 0 without LSTM, kd_mode 1): sf_pack_linear_weights copies of the ResidualMLPPredictor's mlp[0].weight
   * [2D, D] and mlp[2].weight [D, 2D] and of the kernel_dist Linear [2D, D].  With them and the matrix-core slot update (sa_*_p above), the slot
   * prologue of time step t + 1 -- predictor, kernel distribution, sampling, first q (savi.py:393-402) -- runs at the tail of step t's last slot
   * update instead of as its own launch (split-bf16 products, like the update's). */
  const void *pm_w0_p, *pm_w2_p, *kd_w0_p;
} sf_savi_encoder;

size_t sf_savi_encode_workspace_bytes(const sf_savi_encoder* m, int B);
/* img [B,T,3,H,W]; noise [B,T,N,D] or NULL (deterministic / STEVE); prev_slots [B,N,D] or NULL
 * (NULL: frame 0 starts from init_latents and the LSTM state is reset, savi.py:474-475);
 * lstm_h/lstm_c [B*N, pred_hidden] in/out (used iff pred_rnn; state_valid == 0: zeros);
 * outputs: post_slots [B,T,N,D], kernel_dist [B,T,N,2D] or NULL, attn [B,T,N,64*64] or NULL. */
int sf_savi_encode_f32(const sf_savi_encoder* m, const float* img, const float* noise, const float* prev_slots,
                       float* lstm_h, float* lstm_c, int state_valid, float* post_slots, float* kernel_dist,
                       float* attn, int B, int T, void* ws, size_t ws_bytes, void* stream);

/* The CNN stack alone (savi.py:231-244,367-371: convs + soft position embedding) for time steps [t0, t1) of every
 * video: feat [t1-t0][B][64*64][C_last] channels-last.  It does not depend on the slots, so it may run ahead of the
 * encode on another stream; sf_savi_encode_pre_f32 is sf_savi_encode_f32 with the features of the first n_pre time
 * steps taken from feat_pre (bench.py computes part of the NEXT batch's convolutions on the rollout stream's CUs while
 * that stream would otherwise idle). */
size_t sf_savi_cnn_workspace_bytes(const sf_savi_encoder* m, int B);
int sf_savi_cnn_f32(const sf_savi_encoder* m, const float* img, int B, int T, int t0, int t1, float* feat, void* ws,
                    size_t ws_bytes, void* stream);
int sf_savi_encode_pre_f32(const sf_savi_encoder* m, const float* img, const float* feat_pre, int n_pre, const float* noise,
                           const float* prev_slots, float* lstm_h, float* lstm_c, int state_valid, float* post_slots,
                           float* kernel_dist, float* attn, int B, int T, void* ws, size_t ws_bytes, void* stream);
/* The same as TWO branches: `stream` runs the image features (CNN + per-pixel chain) of all T steps back to back, `side_stream` follows one
 * step behind with the slot branches (prologue, Slot-Attention iterations, slot updates), ordered by events; `stream` continues behind the
 * last slot update.  Captured into a hipGraph the two are parallel branches.  side_stream NULL = sf_savi_encode_pre_f32.  Same bits.
 * Workspace: sf_savi_encode_fork_workspace_bytes(m, B, T) (the Slot-Attention inputs of all T steps stay resident). */
size_t sf_savi_encode_fork_workspace_bytes(const sf_savi_encoder* m, int B, int T);
/* Workspace of the one-stream encode (side_stream NULL) that runs the 64 -> 64 convolutions of ALL T time steps as one launch per layer (three
 * buffers of B * T frames on top of sf_savi_encode_workspace_bytes): sf_savi_encode_fork_f32 takes that form when it is handed this much and the
 * encoder has fragment weights on every layer behind the first (B <= 32, T >= 2, split-bf16); the same bits as the step-by-step order.  Only while
 * sf_set_slot_chain(1) is on and sf_savi_chain_ok holds does it also hold the feature planes of the video-stationary slot branch (below). */
size_t sf_savi_encode_batched_workspace_bytes(const sf_savi_encoder* m, int B, int T);
/* Where the slot prologue of time step t + 1 runs (process-wide; default 1).  1: with the packed predictor / kernel-distribution
 * copies of sf_savi_encoder (pm_w0_p, pm_w2_p, kd_w0_p) and the matrix-core slot update, at the tail of step t's last slot update -- one launch fewer per
 * time step, its products on the split-bf16 matrix path like the update's; 0: as its own launch on every step (fp32 thread-per-output products).  The
 * two agree to split-bf16 rounding (~1e-6 relative), not bit for bit; step 0 of a call always takes the stand-alone launch. */
int sf_set_encode_fuse_next(int on);
int sf_get_encode_fuse_next(void);
/* The slot branch of a batched encode (all T steps' convolutions per launch, sf_savi_encode_batched_workspace_bytes queried while on) as ONE video-stationary launch
 * (csrc/slot_chain.hip; savi.py:76-100, 393-402): one workgroup per video walks the T steps x num_iterations Slot-Attention iterations, their slot
 * updates and the per-step prologues on feature rows kept as bf16 hi | lo -- 7 launches per encode instead of ~60.  OPT-IN: process default 0
 * (sf_set_slot_chain(1)).  Measured (profiles/r06_probes.txt): 0.80 ms per batch of 32 videos x 6 frames on 32 CUs against 0.58 ms for
 * the per-iteration launches on the whole chip and 1.2 ms on a 128-CU partition -- fewer CU-ms, more latency; the default keeps the per-iteration launches.  Applies to the CLEVRER shape of the slot branch (slot size 128, slot MLP 256,
 * residual-MLP predictor, single-Linear kernel distribution, folded Slot Attention, up to 8 slots, HW a multiple of 256); everything else keeps the
 * per-iteration launches.  The two forms agree to split-bf16 rounding (the attention products are split-bf16 here, exact f32 there). */
int sf_set_slot_chain(int on);
int sf_get_slot_chain(void);
/* The Slot-Attention iterations of sf_savi_encode_* (folded form, slot size 128, 4096 pixels) on feature rows kept as bf16 hi | lo: logits and weighted sums as
 * split-bf16 v_mfma_f32_16x16x32_bf16 products (sa_attn_planes_kernel, csrc/slot_chain.hip) instead of exact-f32 16x16x4 MFMAs on f32 rows
 * (sa_attn_tile_kernel) -- a third of the matrix-pipe time, the same records, split-bf16 rounding apart.  That rounding grows with the logit scale: measured against float64 on N(0, 1)
 * rows, the attention is ~5e-6 off at logits of std 1, 4e-5 at std 8 and 1.5e-4 at std 32 (near one-hot softmax; the f32 rows: 5e-7 / 3e-6 / 8e-6), the
 * updates within 8e-6 at every scale (tests/test_encode_kernels_gpu.py, profiles/encode_kernel_tests.md).  Process default 1; 0: the f32 rows. */
int sf_set_slot_attn_planes(int on);
int sf_get_slot_attn_planes(void);
/* The per-pixel chain of the encoder (encoder_out_layer + SlotAttention.norm_inputs, savi.py:245-250, 66; 64 -> 128 -> 128 channels) in its pixel-stationary
 * form (pixel_feat_tok_kernel, csrc/pixel_mlp.hip: a wave owns 32 pixels for the whole chain, activations in registers, weights as fragments in LDS, no
 * barrier behind the prologue).  Process default 1; 0: the tile kernels.  The two agree to split-bf16 rounding (different summation order). */
int sf_set_pixel_tok(int on);
int sf_get_pixel_tok(void);
/* The encode in two halves, for callers that overlap them (the batch pipeline: features on the encode lane, the slot branch of a whole rollout unit in
 * front of its rollout).  sf_savi_chain_ok: 1 when both apply to this model at B videos x T frames (the conditions of sf_set_slot_chain above).
 *   sf_savi_features_planes_f32: CNN + encoder_out_layer + SlotAttention.norm_inputs (savi.py:231-250, 66) of B x T frames -> planes [T][B][64 * 64] rows
 *     of 512 B (bf16 hi | lo of the 128 channels; sf_savi_planes_bytes); workspace sf_savi_features_workspace_bytes.
 *   sf_savi_slots_chain_f32: the per-step chain of StoSAVi.encode (savi.py:393-416) with its Slot-Attention iterations (:76-100) for NB batches of B
 *     videos from planes [NB][T][B][64 * 64][512 B]: noise NULL or [NB * B][T][N][D], prev_slots NULL or [NB * B][N][D]; video v's slots of step t ->
 *     post + v * post_bs + t * N * D (post_bs in floats: a [NB * B][T + H][N][D] rollout buffer takes them in place); kernel_dist NULL or
 *     [NB * B][T][N][2 D]; attn NULL or [NB * B][T][N][64 * 64]; workspace sf_savi_slots_chain_workspace_bytes(m, NB * B).
 * The two in sequence give the bits of a batched sf_savi_encode_f32 under sf_set_slot_chain(1); the default (0) differs by split-bf16 rounding. */
int sf_savi_chain_ok(const sf_savi_encoder* m, int B, int T);
size_t sf_savi_planes_bytes(const sf_savi_encoder* m, int B, int T);
size_t sf_savi_features_workspace_bytes(const sf_savi_encoder* m, int B, int T);
int sf_savi_features_planes_f32(const sf_savi_encoder* m, const float* img, int B, int T, void* planes, void* ws, size_t ws_bytes, void* stream);
size_t sf_savi_slots_chain_workspace_bytes(const sf_savi_encoder* m, int videos);
int sf_savi_slots_chain_f32(const sf_savi_encoder* m, const void* planes, const float* noise, const float* prev_slots, float* post, long long post_bs,
                            float* kernel_dist, float* attn, int NB, int B, int T, void* ws, size_t ws_bytes, void* stream);
int sf_savi_encode_fork_f32(const sf_savi_encoder* m, const float* img, const float* feat_pre, int n_pre, const float* noise,
                            const float* prev_slots, float* lstm_h, float* lstm_c, int state_valid, float* post_slots,
                            float* kernel_dist, float* attn, int B, int T, void* ws, size_t ws_bytes, void* stream, void* side_stream);

/* StoSAVi.decode (savi.py:504-525): spatial broadcast + position embedding -> transposed-conv stack -> 1x1 conv
 * -> softmax-over-slots recombination. */
typedef struct {
  int resolution;      /* output H == W */
  int dec_layers;      /* number of transposed convs (<= 8) */
  int dec_channels[9]; /* dec_channels[0] == slot_size */
  int dec_strides[8];
  int dec_ks, dec_res; /* kernel size; broadcast resolution (square) */
  int num_slots, slot_size;
  const float* deconv_w[8]; /* packed [Cout,ks,ks,Cin] */
  const float* deconv_b[8]; /* may be NULL */
  const float *out_w, *out_b; /* final 1x1 conv: [4, C_last], [4] */
  const float* pos_table;     /* [dec_res*dec_res, slot_size] */
  /* optional (NULL = absent), stride-1 layers only: deconv_w spatially flipped ([Cout][ks-1-ky][ks-1-kx][Cin]).  A
   * stride-1 transposed convolution is an ordinary convolution with the flipped kernel, which lets those layers run on
   * the encoder's halo-resident 5x5 kernel (64 -> 64 channels, 64 pixels wide). */
  const float* deconv_w_flipped[8];
  /* optional (NULL = absent), per 64 -> 64 channel 5 x 5 stride-2 layer: sf_pack_deconv_frag_weights copies of deconv_w[i] (split-bf16,
   * consumption order) for the parity-class kernel with streamed weights (csrc/deconv_s2.hip; split-bf16 mode, input 16 / 32 / 64 wide).
   * On the last layer that kernel also applies the 1x1 head, and the [F*N, H, W, 64] activation never reaches memory. */
  const void* deconv_w_frag[8];
  /* optional (NULL = absent): the FIRST layer (5 x 5, stride 2) on its broadcast input.  Its input is slot + pos_table[p] (savi.py:512-517),
   * so  out[r, p] = relu( (sum of the taps valid at p) . slot[r] + const[p] ):  l0_weff [25 * C1, slot_size] holds the tap sums of the 5 x 5
   * border / parity classes of an output pixel (class of a coordinate o = 2 o2 + par: par 0 -> {0: o2 == 0, 1: interior, 2: o2 == res - 1},
   * par 1 -> {3: o2 < res - 1, 4: o2 == res - 1}; row (vy * 5 + vx) * C1 + co), l0_posterm [(2 dec_res)^2, C1] the transposed convolution of
   * the position table + bias.  One [F*N, D] x [D, 25 C1] product and an expansion replace 98 % of the layer's multiplications. */
  const float* l0_weff;
  const float* l0_posterm;
} sf_savi_decoder;

size_t sf_savi_decode_workspace_bytes(const sf_savi_decoder* m, int F);
/* slots [F,N,D] -> recon_combined [F,3,H,W], recons [F,N,3,H,W] (or NULL), masks [F,N,1,H,W] (or NULL). */
int sf_savi_decode_f32(const sf_savi_decoder* m, const float* slots, float* recon_combined, float* recons,
                       float* masks, int F, void* ws, size_t ws_bytes, void* stream);
/* The same + the segmentation test_vp.py scores (postproc_mask of the decoded masks, video_prediction/test_vp.py:55-63 -> vp_utils.py:20-41):
 * seg_i64 / seg_u8 [F,H,W] (either or both NULL); recons / masks may be NULL -- a caller that only scores frames and segmentations never
 * materialises the per-slot tensors.  Workspace as sf_savi_decode_f32. */
int sf_savi_decode_seg_f32(const sf_savi_decoder* m, const float* slots, float* recon_combined, float* recons, float* masks,
                           long long* seg_i64, unsigned char* seg_u8, float fg_thre, int F, void* ws, size_t ws_bytes, void* stream);

/* Row N1: the same decoder under autograd, data gradient only (the image term of SlotFormer's training loss,
 * slotformer.py:313-326; the decoder is frozen there).  The forward keeps every layer output in the workspace; the
 * backward maps d_recon_combined [F,3,H,W] to d_slots [F,N,D].  deconv_w_bwd: HOST array [dec_layers] of device pointers
 * to sf_pack_conv_weight_f32(torch ConvTranspose2d weight [Cin,Cout,k,k]) = [Cin][k][k][Cout]: the adjoint of a
 * transposed convolution is a strided convolution with the same weights. */
typedef struct { /* gradients in torch layouts: ConvTranspose2d weight [Cin,Cout,k,k], head Conv2d [4,C,1,1], dense [D,4] */
  float* deconv_w[8];
  float* deconv_b[8];
  float *out_w, *out_b, *pos_w, *pos_b;
} sf_savi_decoder_grads;

size_t sf_savi_decode_train_workspace_bytes(const sf_savi_decoder* m, int F);
int sf_savi_decode_train_fwd_f32(const sf_savi_decoder* m, const float* slots, float* recon_combined, float* recons,
                                 float* masks, int F, void* ws, size_t ws_bytes, void* stream);
/* g != NULL (SAVi's own training, savi.py:527-538): also the decoder's parameter gradients; pos_grid [dec_res^2, 4] is
 * decoder_pos_embedding.grid.  Needs the reference decoder widths (64 channels after the first layer). */
int sf_savi_decode_train_bwd_f32(const sf_savi_decoder* m, const float* const* deconv_w_bwd, const float* d_recon,
                                 float* d_slots, const float* pos_grid, const sf_savi_decoder_grads* g, int F, void* ws,
                                 size_t ws_bytes, void* stream);

/* Kernel-level entry points of the two training paths above (sf_savi_features_train_bwd_f32, sf_savi_decode_train_bwd_f32), one launch group at a
 * time, for tests against plain references.  Each is the block the module path itself calls; none adds arithmetic.
 *
 * Weight gradient of a 5 x 5 "same" convolution (s = 1: A = dY, X = the layer input) or of a transposed convolution of stride s (A = the layer
 * input, X = dY on the s times finer grid):  dW[n][k][ky][kx] = sum over (f, y, x) of A[f, y, x, n] * X[f, y*s + ky - 2, x*s + kx - 2, k], zero
 * outside the X grid.  A [rows, CA] NHWC on an H x W grid, X [F, Hx, Wx, 64] NHWC, dW [CA, 64, 5, 5] (the torch layout of either weight).
 * partial: scratch of `partial_floats` floats, at most sf_conv_wgrad_partial_floats(CA, ks); every float of it that the reduction reads is written
 * first.  Refused before any launch: ks != 5, CA % 64 != 0, rows != F * H * W, Hx != H * s or Wx != W * s, a partial buffer smaller than the call's
 * row splits need, and an A, X or partial that is not 16-byte aligned (the kernels load four floats at a time). */
size_t sf_conv_wgrad_partial_floats(int CA, int ks);
int sf_conv_wgrad_f32(const float* A, int CA, int F, int H, int W, const float* X, int Hx, int Wx, int s, int ks, long long rows, float* dW,
                      float* partial, size_t partial_floats, void* stream);
/* Backward-data pass of a convolution layer: Conv2d(ks, stride, padding ks/2) of the gradient `in` [F,Hin,Win,Cin] NHWC with w_packed
 * [Cout][ks][ks][Cin] -> out [F,Hin/stride,Win/stride,Cout], no bias; relu_mask (optional, laid out like out): out = relu_mask > 0 ? conv : 0.
 * With w_packed = sf_pack_conv_weight_f32(ConvTranspose2d weight) this is the adjoint of sf_conv_transpose2d_nhwc_f32; with
 * sf_pack_conv_bwd_weight_f32(Conv2d weight) and stride 1 the adjoint of sf_conv2d_nhwc_f32 (= that function with relu = 2). */
int sf_conv2d_nhwc_bwd_data_f32(const float* in, const float* w_packed, const float* relu_mask, float* out, int F, int Hin, int Win, int Cin,
                                int Cout, int ks, int stride, void* stream);
/* w_bwd[ci][ky][kx][co] = w_oihw[co][ci][ks-1-ky][ks-1-kx]: the packed weight of the backward-data pass of a "same" Conv2d. */
int sf_pack_conv_bwd_weight_f32(const float* w_oihw, float* w_bwd, int Cout, int Cin, int ks, void* stream);
/* conv0's weight gradient dW [64,3,5,5] from the NCHW image (frame f at img + f * frame_stride floats; 64 x 64 at stride 1 or 128 x 128 at stride
 * 2) and dY [F*4096, 64]: im2col with K = 75 padded to 128, the TN contraction of sf_linear_bwd_f32, the 75 live columns. */
size_t sf_conv_first_wgrad_workspace_bytes(int F);
int sf_conv_first_wgrad_f32(const float* img, long long frame_stride, int resolution, const float* dY, int F, float* dW, void* ws,
                            size_t ws_bytes, void* stream);
/* SoftPositionEmbed gradients from d [F,HW,C] (the table grid W^T + b is added to every frame): dw [C,4], db [C]; grid [HW,4]; dtab: scratch
 * [HW*C], holds the frame sum of d on return. */
int sf_pos_dense_grad_f32(const float* d, int F, int HW, int C, const float* grid, float* dw, float* db, float* dtab, void* stream);
/* Head block of the decoder backward: dec [F*N,HW,4] (rgb | mask logit), d_recon [F,3,HW], act [F*N*HW,Cl] (post-ReLU output of the last
 * transposed conv), out_w [4,Cl] -> d_dec [F*N,HW,4], d_act [F*N*HW,Cl] = act > 0 ? d_dec . out_w : 0, and d_out_w [4,Cl] / d_out_b [4] (either
 * may be NULL).  Cl a multiple of 4, at most 64; dec, d_dec, act 16-byte aligned. */
size_t sf_savi_decode_head_bwd_workspace_bytes(int Cl);
int sf_savi_decode_head_bwd_f32(const float* dec, const float* d_recon, const float* act, const float* out_w, float* d_dec, float* d_act,
                                float* d_out_w, float* d_out_b, int F, int N, int HW, int Cl, void* ws, size_t ws_bytes, void* stream);


/* ---- K/V producer (SURVEY.md 8(b2) sf_kv_producer_*) ---------------------------------------- */
/* encoder_out_layer (savi.py:245-250: LN -> Linear -> ReLU -> Linear) followed by Slot Attention's
 * norm_inputs + project_k / project_v (savi.py:66-70): feat [M,C0] channels-last CNN features (position
 * embedding already added, savi.py:371-375) -> kv [M,2D] = (k | v).  kv_w = cat(project_k.weight,
 * project_v.weight) [2D,C1].  One fused kernel in split-bf16 mode at (C0,C1,2D) = (64,128,256); otherwise
 * three GEMMs through ws (sf_kv_producer_workspace_bytes). */
size_t sf_kv_producer_workspace_bytes(int M, int C1);
int sf_kv_producer_f32(const float* feat, const float* ln0_g, const float* ln0_b, const float* fc1_w,
                       const float* fc1_b, const float* fc2_w, const float* fc2_b, const float* ln1_g,
                       const float* ln1_b, const float* kv_w, float* kv, int M, int C0, int C1, int D, float ln_eps,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- device-memory helpers and host-buffer twins (SURVEY.md 8(b2) "_host twin") -------------- */
/* For callers without a HIP binding of their own (plain C, ctypes + numpy): place the weights on the GPU
 * once with sf_device_alloc / sf_device_upload, fill the model structs with those device pointers, and call
 * the *_host twins, whose DATA buffers (everything that is not inside a model struct) are host pointers.
 * A twin has its device counterpart's signature; ws == NULL means "allocate the workspace for this call".
 * Twins are synchronous (the results are in host memory on return) and allocate/free staging memory. */
int sf_device_alloc(void** dev_out, size_t bytes);
int sf_device_free(void* dev);
int sf_device_upload(void* dev, const void* host, size_t bytes);
int sf_device_download(void* host, const void* dev, size_t bytes);
int sf_device_synchronize(void);
/* A HIP stream restricted to a subset of the CUs (hipExtStreamCreateWithCUMask; bit i of cu_mask = CU i,
 * n_words 32-bit words): partitions the GPU between the encode of batch i+1 and the rollout of batch i. */
int sf_stream_create_cu_mask(void** stream_out, const unsigned int* cu_mask, int n_words);
/* CUs a launch on `stream` may occupy: the popcount of the mask of a stream made by sf_stream_create_cu_mask, else the device's CU count.  The
 * persistent kernels (csrc/conv_ws.hip) launch one workgroup per CU of their stream. */
int sf_stream_cus(void* stream);
/* The CU count the library is to assume for launches issued on `stream` (cus <= 0: forget): for a stream that captures a graph which will be replayed
 * on a CU-masked stream. */
int sf_stream_set_cus(void* stream, int cus);
int sf_stream_destroy(void* stream);
/* One wave busy for `us` microseconds on `stream` (1..100000): two of them on two streams tell whether the streams share a hardware queue. */
int sf_debug_spin(int us, void* stream);
/* One wave that counts shader cycles (out2[0]) over `us` microseconds of the constant 100 MHz counter (out2[1] ticks): the clock the chip sustains
 * under whatever else is running (tools/clock_probe.py); out2: device buffer of two int64. */
int sf_debug_clock_probe(int us, long long* out2, void* stream);
int sf_slot_attn_iter_f32_host(const float* k_host, const float* v_host, int ld, long long batch_stride,
                               const float* q_host, float* part_num_host, float* part_den_host, float* attn_out_host,
                               int B, int HW, int N, int D, float scale, float eps, void* stream);
int sf_rollout_f32_host(const sf_rollouter* m, float* slots_host, int B, int T_total, int pred_len, void* ws,
                        size_t ws_bytes, void* stream);
/* Health check of the rollout's seam launches (the last FFN + step boundary of step s and the first attention of step s+1 run
 * in one grid and hand 7 rows per video over through memory, slotformer.py:121-124 -> :115): number of hand-offs that gave up
 * waiting since the library was loaded (synchronises the device).  Must be 0; SF_SEAM_FUSED=0 disables the seam launches. */
int sf_seam_timeouts(void);

/* Single-pass bf16 variant of sf_rollout_f32 (SURVEY.md 8(b2) `sf_rollout_bf16`; the reference's `--fp16` AMP,
 * scripts/train.py:84,105, and BASELINE.json's literal "bf16"): same arguments and storage (f32), every matrix product with
 * operands rounded to bf16 and f32 accumulation.  ~8e-3 relative on the 6+50 path of config C2 -- outside the 1e-3 parity
 * bar, so it is an option, never the default. */
int sf_rollout_bf16(const sf_rollouter* m, float* slots, int B, int T_total, int pred_len, void* ws, size_t ws_bytes,
                    void* stream);
int sf_rollout_bf16_host(const sf_rollouter* m, float* slots_host, int B, int T_total, int pred_len, void* ws,
                         size_t ws_bytes, void* stream);
/* host twins of the slot update (savi.py:95-100) and of the K/V producer (savi.py:245-250,66-70): data buffers on the host,
 * weights on the device */
int sf_slot_update_f32_host(const float* part_num_host, const float* part_den_host, int P, const float* slots_prev_host,
                            const float* gru_w_ih, const float* gru_w_hh, const float* gru_b_ih, const float* gru_b_hh,
                            const float* ln_g, const float* ln_b, const float* mlp_w1, const float* mlp_b1,
                            const float* mlp_w2, const float* mlp_b2, float* slots_out_host, int B, int N, int D, int H,
                            float ln_eps, void* stream);
int sf_kv_producer_f32_host(const float* feat_host, const float* ln0_g, const float* ln0_b, const float* fc1_w,
                            const float* fc1_b, const float* fc2_w, const float* fc2_b, const float* ln1_g,
                            const float* ln1_b, const float* kv_w, float* kv_host, int M, int C0, int C1, int D, float ln_eps,
                            void* ws, size_t ws_bytes, void* stream);
int sf_savi_encode_f32_host(const sf_savi_encoder* m, const float* img_host, const float* noise_host,
                            const float* prev_slots_host, float* lstm_h_host, float* lstm_c_host, int state_valid,
                            float* post_slots_host, float* kernel_dist_host, float* attn_host, int B, int T, void* ws,
                            size_t ws_bytes, void* stream);
int sf_savi_decode_f32_host(const sf_savi_decoder* m, const float* slots_host, float* recon_combined_host,
                            float* recons_host, float* masks_host, int F, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

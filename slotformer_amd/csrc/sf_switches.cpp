// The table of process-wide switches (sf_switches.h) and the twenty exported setters / getters over it (include/slotformer_hip.h describes each).
#include <stdlib.h>
#include <atomic>

#include "../../include/slotformer_hip.h"
#include "sf_internal.h"

namespace {
// how a variable's text becomes a value.  FLAG: a switch that defaults off turns on only when the first character is '1', one that defaults on turns
// off only when it is '0'.  PRECISION: a first character of 'f' or '0' selects 0, the exact string "bf16" 2, anything else 1.
enum Parse { NO_ENV, FLAG, PRECISION };
struct Row {
  const char* env;
  int def;
  Parse parse;
};
constexpr Row ROWS[SF_SW_NUM] = {
    // 0: exact f32 MFMA everywhere; 1: split-bf16 MFMA (default); 2: single-pass bf16 MFMA with f32 accumulation in the GEMM / conv
    // / weight-gradient cores (the "AMP-bf16" policy of the training path: fp32 storage and master weights, one bf16 rounding of
    // each operand; kernels without a single-pass variant keep mode 1).  SF_PRECISION=f32 | bf16 selects 0 | 2.
    /* SF_SW_PRECISION */ {"SF_PRECISION", 1, PRECISION},
    // Process default of the token-stationary layer launches (sf_rollout_opts.layer_tok == 0): OFF unless SF_LAYER_TOK=1 / sf_set_layer_tok(1).
    // The pipeline passes its own choice per unit; a direct call at 32 videos of the OBJ3D shape is slower with it (profiles/layer_tok_d128.md).
    /* SF_SW_LAYER_TOK */ {"SF_LAYER_TOK", 0, FLAG},
    // Seam launches on / off (default: on unless SF_SEAM_FUSED=0).  A seam launch saves a kernel boundary on the critical path of
    // ONE rollout chain; its 128 consumer workgroups spin until the 28 producers are done, which is CU time a second chain running
    // on the same CUs could use -- the 'pair' pipeline captures its graphs with the seam off.
    /* SF_SW_SEAM_FUSED */ {"SF_SEAM_FUSED", 1, FLAG},
    // 64 instead of 32 rows per workgroup of the chunk-partial FFN launches (sf_ffn_rows, sf_internal.h; layer_fused.hip): the same bits
    /* SF_SW_FFN_ROWS64 */ {nullptr, 0, NO_ENV},
    // opt-in arithmetic of the 4-row-tile convolution (conv_rows4.hip): 0 (default) split-bf16, three products; 1 activations as two fp16 terms x
    // weights as ONE fp16, two products
    /* SF_SW_CONV_FP16X2 */ {"SF_CONV_FP16X2", 0, FLAG},
    // 9 .. 16 slots, keys == values: the one-pass tile kernel (default; at 84,480 B of LDS ONE workgroup per CU) or, 0, the two-pass kernel
    // (slot_attn.hip).  profiles/slots16.md has the measurement behind the default.
    /* SF_SW_SLOT_ATTN_TILE16 */ {nullptr, 1, NO_ENV},
    // the slot prologue of step t + 1 at the tail of step t's last slot update (slot_update_mfma.hip, NEXT form): on by default where it applies;
    // 0: the prologue as its own launch (sa_slot_prologue_kernel) on every step
    /* SF_SW_ENCODE_FUSE_NEXT */ {nullptr, 1, NO_ENV},
    // the slot branch of a batched encode as one video-stationary launch (slot_chain.hip): OPT-IN; the default keeps the per-iteration launches
    // (Slot-Attention iteration over the batch + slot update), which are faster for a batch alone on its CUs
    /* SF_SW_SLOT_CHAIN */ {nullptr, 0, NO_ENV},
    // the Slot-Attention iterations of the per-step encode on feature rows kept as bf16 hi | lo (sa_attn_planes_kernel, slot_chain.hip: split-bf16
    // 16x16x32 MFMAs) instead of f32 rows and the exact-f32 tile kernel
    /* SF_SW_SLOT_ATTN_PLANES */ {nullptr, 1, NO_ENV},
    // the per-pixel chain in its pixel-stationary form (pixel_feat_tok_kernel, pixel_mlp.hip); 0: the tile kernels
    /* SF_SW_PIXEL_TOK */ {nullptr, 1, NO_ENV},
    // 0: the 4-row-tile convolution everywhere; default: the weights-stationary kernel on streams with CUs of their own (conv_ws.hip; the same bits)
    /* SF_SW_CONV_WS */ {"SF_CONV_WS", 1, FLAG},
};

// value + 1; 0 (what static storage starts as): not yet read
std::atomic<int> g_slot[SF_SW_NUM];

int initial(const Row& r) {
  const char* e = r.env ? getenv(r.env) : nullptr;
  if (!e) return r.def;
  if (r.parse == PRECISION) return (e[0] == 'f' || e[0] == '0') ? 0 : (strcmp(e, "bf16") == 0 ? 2 : 1);
  return r.def ? e[0] != '0' : e[0] == '1';
}
}  // namespace

int sf_switch(SfSwitch s) {
  int v = g_slot[s].load(std::memory_order_relaxed);
  if (v == 0) {
    v = initial(ROWS[s]) + 1;
    int seen = 0;   // a setter that got in between keeps its value
    if (!g_slot[s].compare_exchange_strong(seen, v, std::memory_order_relaxed)) v = seen;
  }
  return v - 1;
}

int sf_switch_set(SfSwitch s, int v) {
  g_slot[s].store(v + 1, std::memory_order_relaxed);
  return 0;
}

extern "C" {
int sf_get_precision(void) { return sf_precision(sf_thread_opts()); }
int sf_set_precision(int mode) {
  if (mode < 0 || mode > 2) return sf_set_err(-1, "invalid argument: precision mode must be 0 (f32), 1 (bf16x3) or 2 (bf16)", __FILE__, __LINE__);   // (3 = single-pass fp16 exists per call only: sf_rollout_opts.precision, a measurement probe)
  return sf_switch_set(SF_SW_PRECISION, mode);
}
int sf_get_layer_tok(void) { return sf_switch(SF_SW_LAYER_TOK); }
int sf_set_layer_tok(int on) { return sf_switch_set(SF_SW_LAYER_TOK, on != 0); }
int sf_get_seam_fused(void) { return sf_switch(SF_SW_SEAM_FUSED); }
int sf_set_seam_fused(int on) { return sf_switch_set(SF_SW_SEAM_FUSED, on != 0); }
int sf_get_ffn_rows64(void) { return sf_switch(SF_SW_FFN_ROWS64); }
int sf_set_ffn_rows64(int on) { return sf_switch_set(SF_SW_FFN_ROWS64, on != 0); }
int sf_get_conv_fp16x2(void) { return sf_switch(SF_SW_CONV_FP16X2); }
int sf_set_conv_fp16x2(int on) { return sf_switch_set(SF_SW_CONV_FP16X2, on != 0); }
int sf_get_slot_attn_tile16(void) { return sf_switch(SF_SW_SLOT_ATTN_TILE16); }
int sf_set_slot_attn_tile16(int on) { return sf_switch_set(SF_SW_SLOT_ATTN_TILE16, on != 0); }
int sf_get_encode_fuse_next(void) { return sf_switch(SF_SW_ENCODE_FUSE_NEXT); }
int sf_set_encode_fuse_next(int on) { return sf_switch_set(SF_SW_ENCODE_FUSE_NEXT, on != 0); }
int sf_get_slot_chain(void) { return sf_switch(SF_SW_SLOT_CHAIN); }
int sf_set_slot_chain(int on) { return sf_switch_set(SF_SW_SLOT_CHAIN, on != 0); }
int sf_get_slot_attn_planes(void) { return sf_switch(SF_SW_SLOT_ATTN_PLANES); }
int sf_set_slot_attn_planes(int on) { return sf_switch_set(SF_SW_SLOT_ATTN_PLANES, on != 0); }
int sf_get_pixel_tok(void) { return sf_switch(SF_SW_PIXEL_TOK); }
int sf_set_pixel_tok(int on) { return sf_switch_set(SF_SW_PIXEL_TOK, on != 0); }
}

// The process-wide switches of libslotformer_hip.so: one table (sf_switches.cpp), one read and one write.
//
// How a switch gets its value, stated once: the table's default; the switch's environment variable, where it has one, read ONCE on the first read;
// a setter called before that wins and the variable is then never read; a per-call option of the calling thread (SfThreadOpts, sf_internal.h) wins
// over all of it for that call -- the sf_*_on / sf_precision / sf_ffn_rows functions beside SfThreadOpts resolve that last step.
// A switch is read when a call plans its launches: a hipGraph captured earlier keeps the form it was captured with.
// The slots are relaxed atomics: the library is driven from one host thread per GPU and a switch orders nothing else.
#pragma once

enum SfSwitch {
  SF_SW_PRECISION,          // sf_set_precision / SF_PRECISION
  SF_SW_LAYER_TOK,          // sf_set_layer_tok / SF_LAYER_TOK
  SF_SW_SEAM_FUSED,         // sf_set_seam_fused / SF_SEAM_FUSED
  SF_SW_FFN_ROWS64,         // sf_set_ffn_rows64
  SF_SW_CONV_FP16X2,        // sf_set_conv_fp16x2 / SF_CONV_FP16X2
  SF_SW_SLOT_ATTN_TILE16,   // sf_set_slot_attn_tile16
  SF_SW_ENCODE_FUSE_NEXT,   // sf_set_encode_fuse_next
  SF_SW_SLOT_CHAIN,         // sf_set_slot_chain
  SF_SW_SLOT_ATTN_PLANES,   // sf_set_slot_attn_planes
  SF_SW_PIXEL_TOK,          // sf_set_pixel_tok
  SF_SW_CONV_WS,            // SF_CONV_WS only: no setter
  SF_SW_NUM
};

int sf_switch(SfSwitch s);              // the process value
int sf_switch_set(SfSwitch s, int v);   // returns 0

// the matrix-arithmetic mode of the calling thread: its per-call precision while one is set, else the process value (sf_switches.cpp)
extern "C" int sf_get_precision(void);

// Stand-alone ThreadSanitizer check of the switch table (csrc/sf_switches.cpp): host code only, no GPU is opened, nothing of it is loaded into Python.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=thread -x hip tools/switches_tsan.cpp slotformer_amd/csrc/sf_switches.cpp \
//         -o switches_tsan && ./switches_tsan && ./switches_tsan - 1 && ./switches_tsan 01 0 && ./switches_tsan 10 1
//
// The two things the table needs from sf_runtime.cpp are defined here.  Eight threads read and write every switch through the table's two functions
// and through the exported wrappers while the first reads of the environment are still outstanding; then one thread checks the values the rules give
// (the SF_CONV_WS rule too, which no exported getter reaches).  Exit status 0 and no ThreadSanitizer report: clean.
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <vector>

#include "../include/slotformer_hip.h"
#include "../slotformer_amd/csrc/sf_internal.h"

thread_local char sf_err_buf[512] = "";
SfThreadOpts& sf_thread_opts() {
  static thread_local SfThreadOpts o;
  return o;
}

#define CHECK(c)                                           \
  do {                                                     \
    if (!(c)) {                                            \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);      \
      return 1;                                            \
    }                                                      \
  } while (0)

int main(int argc, char** argv) {
  // switches_tsan [<value of SF_CONV_WS, or - for unset> <the switch's value then>]
  const char* ws = argc == 3 ? argv[1] : "0";
  const int ws_value = argc == 3 ? atoi(argv[2]) : 0;
  setenv("SF_PRECISION", "bf16", 1);
  setenv("SF_LAYER_TOK", "1", 1);
  setenv("SF_SEAM_FUSED", "0", 1);
  setenv("SF_CONV_FP16X2", "1x", 1);
  if (ws[0] == '-') unsetenv("SF_CONV_WS");
  else setenv("SF_CONV_WS", ws, 1);
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([t] {
      long sum = 0;
      for (int i = 0; i < 20000; ++i) {
        const SfSwitch s = (SfSwitch)((i + t) % SF_SW_NUM);
        sum += sf_switch(s);
        if (t >= 4 && s != SF_SW_PRECISION && s != SF_SW_CONV_WS) sf_switch_set(s, (i >> 4) & 1);
        sum += sf_get_precision() + sf_get_layer_tok() + sf_get_pixel_tok();
        if (t == 7) {
          sf_set_precision(i % 3);
          sf_set_precision(7);   // rejected: writes this thread's error text only
          sf_set_slot_chain(i & 1);
          sf_thread_opts().precision = (i & 1) ? 3 : -1;   // this thread's per-call option
        }
      }
      if (sum < 0) abort();
    });
  for (auto& x : th) x.join();

  // a per-call option of the thread wins; the process value underneath is one of what thread 7 wrote
  CHECK(sf_get_precision() >= 0 && sf_get_precision() <= 2);
  sf_thread_opts().precision = 3;
  CHECK(sf_get_precision() == 3 && sf_precision(sf_thread_opts()) == 3);
  sf_thread_opts().precision = -1;
  CHECK(sf_set_precision(1) == 0 && sf_get_precision() == 1);
  CHECK(sf_set_precision(3) < 0 && sf_get_precision() == 1);
  // SF_CONV_WS: off only when the first character is '0' (no thread wrote it: this is the first read's value)
  CHECK(sf_switch(SF_SW_CONV_WS) == ws_value);
  // the resolved values: option, else switch
  SfThreadOpts o;
  sf_switch_set(SF_SW_SEAM_FUSED, 1);
  sf_switch_set(SF_SW_LAYER_TOK, 0);
  sf_switch_set(SF_SW_FFN_ROWS64, 0);
  CHECK(sf_seam_on(o) && !sf_layer_tok_on(o) && sf_ffn_rows(o) == 32 && sf_precision(o) == 1);
  sf_switch_set(SF_SW_SEAM_FUSED, 0);
  sf_switch_set(SF_SW_LAYER_TOK, 1);
  sf_switch_set(SF_SW_FFN_ROWS64, 1);
  CHECK(!sf_seam_on(o) && sf_layer_tok_on(o) && sf_ffn_rows(o) == 64);
  o.seam = 1, o.layer_tok = -1, o.ffn_rows = 128, o.precision = 0;
  CHECK(sf_seam_on(o) && !sf_layer_tok_on(o) && sf_ffn_rows(o) == 128 && sf_precision(o) == 0);
  o.seam = 0, o.layer_tok = 1;
  sf_switch_set(SF_SW_SEAM_FUSED, 1);
  sf_switch_set(SF_SW_LAYER_TOK, 0);
  CHECK(!sf_seam_on(o) && sf_layer_tok_on(o));
  printf("switches_tsan: ok\n");
  return 0;
}

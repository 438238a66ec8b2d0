// The rollout training forward (rollout_train.hip) in two halves, for entry points that place the burn-in frames themselves (clip_train.hip).
#pragma once
#include "../../include/slotformer_hip.h"
#include "sf_common.h"

// Validates (m, B, pred_len, workspace) as sf_rollout_train_fwd_f32 does; *slots_all: where the frame-major burn-in [hist][B * N][C] goes in the
// workspace, *hist: its length in frames (1 for a single-step rollouter).
int sf_rollout_train_burnin_ex(const sf_rollouter* m, int B, int pred_len, void* ws, size_t ws_bytes, float** slots_all, int* hist);
// The in-projections of the burn-in frames and every step from there: all of sf_rollout_train_fwd_f32 after its copy of x.
int sf_rollout_train_steps_ex(const sf_rollouter* m, float* pred, int B, int pred_len, float dropout_p, unsigned long long seed, void* ws,
                              size_t ws_bytes, hipStream_t st);

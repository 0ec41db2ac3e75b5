// train_step.h -- the record a dfa_<model>_forward_train leaves for its dfa_<model>_backward: what the backward must know about
// its forward.  One rule for all four models: the record describes the LATEST forward_train call on the model's slot and is live
// only if that call returned DFA_OK.  forward_train clears `live` at entry, fills a local record and commits it as its last
// statement; dfa_<model>_set_params clears `live`; a backward, refused or completed, leaves the record as it was.
// Host only, plain structs: match_step is what tests/host/train_step_match.cpp walks.
#pragma once
#include "rng.h"

namespace dfa {

struct TrainStep {
  bool live = false;
  int B = 0, T = 0, F = 0;     // DeepfakeDetector: T = T_max, F = in_ch
  int prec = -1, x_dtype = -1;
  int ragged = 0;              // the forward was dfa_cnn1d_forward_train_ragged (its table sits behind the plan in the workspace)
  double frames = 0.0;         // frames BatchNorm1d counted (CNN1D: B T, or the sum of the lengths)
  bool synced = false;         // the SyncBN hook (dfa_ctx_set_bn_sync) was armed
  DropCfg drop{};
  AugCfg aug{};                // the forward's one-shot augmentation (the backward re-reads x through it)
  // which kernel forms ran, so what the backward finds in the workspace and in the per-step weight images
  int c1_fused = 0;            // CNN2D: XX / Xs left behind for the one-pass block-1 backward
  int c1_mfma = 0;             // CNN2D, auto-encoder: the block-1 passes ran on train_conv1_mfma.hip
  int dgrad_m16 = 0;           // CNN2D, auto-encoder: data-gradient images in the 16x16x32 order of conv_split.hip
  int enc4_wide = 0;           // auto-encoder: 128-input-channel block-4 images
  int x3 = 0;                  // CNN1D: the context's cnn1d_train_x3 (which wx3 images were packed, how many terms)
  // Options a backward reads from the context at its own call, each harmless late: wgrad_variant, train_conv_variant and
  // cae_dgrad_mfma pick between kernels that read the same saved tensors and images; cae_bwd_fold picks how many passes the
  // backward itself makes over dz; conv1_mfma can only turn c1_mfma off, and the vector kernels read the same statistics and XX / Xs.
};

// a backward call as it came, and the hook's state at that call
struct StepCall {
  int B, T, F, x_dtype, ragged;
  bool synced;
};

enum StepVerdict { STEP_SAME = 0, STEP_OTHER_BATCH, STEP_HOOK_CHANGED };

// Is `c` the backward of the forward `s` describes?  f32_only: the model refuses any x_dtype but float32 with a text of its own,
// so x_dtype is not compared here.  Another batch outranks a changed hook.
inline StepVerdict match_step(const TrainStep& s, const StepCall& c, bool f32_only) {
  if (!s.live || s.B != c.B || s.T != c.T || s.F != c.F || s.ragged != c.ragged || (!f32_only && s.x_dtype != c.x_dtype))
    return STEP_OTHER_BATCH;
  return s.synced != c.synced ? STEP_HOOK_CHANGED : STEP_SAME;
}

}  // namespace dfa

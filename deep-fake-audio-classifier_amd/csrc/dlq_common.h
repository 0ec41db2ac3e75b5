// dlq_common.h -- what the DeepfakeDetector kernels share (dlq.hip: the layer kernel and the eval finish; dlq_train.hip: the training
// step's other kernels): the tile constants, GELU and its derivative, the per-element dropout scale.  The three-term split (split3_pair) and the MFMA wrapper
// (mma32) come from dfa_device.h; nothing of the 3x3 convolution header is used here.
#pragma once
#include "dfa_internal.h"
#include "dfa_device.h"

namespace dfa {
namespace dlq {
constexpr int NF = DFA_DLQ_TILE_FRAMES;   // frames per tile
constexpr int HID = 256;
constexpr int PIXB = 6 * HID;             // bytes per split pixel: three bf16 terms of 256 channels
constexpr int PIXC = PIXB / 16;           // 16-byte chunks per pixel (term t: chunks [32 t, 32 t + 32))
constexpr int SLOTS = NF + 4;             // widest halo: 2 frames each side (layer 1, k = 5)
constexpr int LDS_BYTES = SLOTS * PIXB;   // 104448: one workgroup per CU; the layer-3 epilogue reuses it as float [256][NF + 1] (66560)
constexpr int NTH = 256;
static_assert(HID * (NF + 1) * 4 <= LDS_BYTES, "layer-3 epilogue tile does not fit");
}  // namespace dlq

__device__ __forceinline__ float dlq_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// d/dv GELU(v), erf form
__device__ __forceinline__ float dlq_dgelu(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}
// the keep-scale factor drop_scale8 gives element idx (the same draw, one element of its group of 8)
// (drop1 of train_cnn1d.hip is the same value picked by an indexed array read; this one is a select chain, the two compile differently)
__device__ __forceinline__ float drop_scale1(const DropCfg& d, uint64_t idx) {
  if (d.thresh == 0) return 1.f;
  float f[8];
  drop_scale8(d, idx & ~(uint64_t)7, f);
  float r = f[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) r = ((int)(idx & 7) == j) ? f[j] : r;
  return r;
}

}  // namespace dfa

// cnn1d_x3_common.h -- what the CNN1D eval forward (cnn1d_fused_x3.hip, cnn1d_x3_body.h) and the training step's layer kernel
// (conv1d_x3.hip) share: the workgroup shape, the k-step count, the fragment order of their A-fragment images and the tap mask.
#pragma once
#include "dfa_internal.h"

namespace dfa {
namespace c1x {
constexpr int TW = 32, NW = 8, NTH = 64 * NW, MAXT1 = 2;   // 8 waves = two per SIMD (one wave's VALU / LDS work under the other's MFMAs); layer 1: tiles w, w + 8
}

// k-steps of 16 input channels; layer 1 (the only layer with cin != 32, 64) runs its slabs two per loop trip: padded to an even count
__host__ __device__ inline int cnn1d_x3_nks(int cin) { const int n = (cin + 15) / 16; return (cin == 32 || cin == 64) ? n : (n + 1) & ~1; }

// where fragment (channel tile m, tap, k-step ks) sits in an A-fragment image, in fragments: [m][tap][ks], or -- five taps, the
// layer-1 image of the k = (5, 3, 3) variant, which its kernels stream one k-step per trip -- k-step-major [m][ks][tap], a
// k-step's taps contiguous
__device__ __forceinline__ int cnn1d_x3_frag_slot(int m, int tap, int ks, int taps, int nks) {
  return taps == 5 ? (m * nks + ks) * taps + tap : (m * taps + tap) * nks + ks;
}

__device__ __forceinline__ uint4 and4(unsigned m, const uint4& v) { return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m); }   // (a select here became an exec branch)

}  // namespace dfa

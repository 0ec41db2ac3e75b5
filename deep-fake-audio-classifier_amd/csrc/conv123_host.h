// conv123_host.h -- the host side of the CNN2D blocks 1-3 kernels (conv123_*.hip), shared with the dispatcher in cnn2d_api.hip: the
// kernel arguments, the entry of each form, and the plan that says which form runs.  The kernel bodies are conv123_body.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch_views.h"

namespace dfa {

namespace c123 { constexpr int SW = 30; }   // output columns of a unit = an (utterance, strip) pair
struct Conv123Args {
  const void* x;            // features (bf16 or fp32: the x_dtype of the launch), element strides below (any layout)
  long long sxb, sxt, sxf;
  const uint4* c1pack;      // [4][64] block-1 A operands (pack_conv1_mfma_kernel)
  const float* c1bias;      // [32]  0.5 * folded bias
  const uint4* wpack2;      // block 2 image [2][9][2][64] (pool factor folded)
  const float* bias2;       // [64]
  const uint4* wpack3;      // block 3 image in the 16x16x32 order [4][9][2][2][64]
  const float* bias3;       // [128]
  float* emb;               // [B][128][F] fp32 time mean
  float inv_h;
  int B, T, F, H1, H2, nstrips;
  int chunk_iters;          // canonical chunks of the time mean (conv3_m16.hip)
  long long* clock_stamps;  // held-clock probe (ConvArgs::clock_stamps), null = off
  // conv123_cls.hip alone (appended: the offsets above are those of the four older kernels); set by the dispatcher, null / 0 elsewhere
  const float* cls_w;       // [K] classifier weights, 16-byte aligned
  const float* cls_b;       // [1]
  float* logits;            // [B]
  int cls_K;                // 128 * F
};
static inline Conv123Args c123_args(const FeatView& v, const uint4* c1pack, const float* c1bias, const uint4* wpack2, const float* bias2,
                                    const uint4* wpack3, const float* bias3, float* emb, int chunk_iters, long long* clock_stamps) {
  const int T = v.T, F = v.F;
  Conv123Args a{};
  a.x = v.x; a.sxb = v.sb; a.sxt = v.st; a.sxf = v.sf;
  a.c1pack = c1pack; a.c1bias = c1bias; a.wpack2 = wpack2; a.bias2 = bias2; a.wpack3 = wpack3; a.bias3 = bias3; a.emb = emb;
  a.B = v.B; a.T = T; a.F = F; a.H1 = T / 2; a.H2 = a.H1 / 2; a.nstrips = (F + c123::SW - 1) / c123::SW;
  a.inv_h = 1.0f / (float)a.H2;
  a.chunk_iters = chunk_iters;
  a.clock_stamps = clock_stamps;
  return a;
}
// one entry per form: per unit (conv123_fused.hip), persistent (conv123_persist.hip), persistent with carried a1 columns
// (conv123_carry.hip), the carry form de-phased (conv123_phase.hip).  Each takes grid and LDS bytes from conv123_plan and
// returns hipErrorInvalidValue where the plan does not allow its form.
hipError_t launch_conv123_fused(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe);
hipError_t launch_conv123_persist(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe);
hipError_t launch_conv123_carry(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe);
hipError_t launch_conv123_phase(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe);
// the phase form with, where conv123_cls_in_kernel() answers 1 (the shipped build), the classifier head at the end of every
// workgroup: a.cls_w, a.cls_b, a.logits, a.cls_K must be set, cls_w
// and emb 16-byte aligned, and the caller launches no linear1_kernel behind it (conv123_cls.hip)
hipError_t launch_conv123_cls(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe);
int conv123_cls_in_kernel();
// which form runs for these dimensions and options: form = DFA_CONV123_*, phase = the de-phased build of the carry form, grid
// workgroups of 512 threads, lds bytes of dynamic LDS.  (Defined in conv123_carry.hip: the LDS layout constants it needs are
// conv123_body.h's, which only the kernel files may include.)
struct Conv123Plan { int form, phase, grid; size_t lds; };
Conv123Plan conv123_plan(int B, int T, int F, int num_cus, int persist123, int carry_a1, int phase123);

}  // namespace dfa

// conv123_fused.hip -- CNN2D blocks 1, 2 and 3 + mean over T in ONE kernel (bf16 mode, large batches):
//   conv12_fused's unit (block 1 on the matrix cores into an a1 ring, block 2 + ReLU + pool) in waves 0-3 ("producers")
//   and conv3_m16's unit (block 3 on v_mfma_f32_16x16x32_bf16, running column sums, canonical-chunk time mean) in waves
//   4-7 ("consumers") of one 512-thread workgroup per (utterance, 30-column strip), one workgroup per CU.
//
// Why.  conv12_fused is bound by vector-instruction issue with a half-idle matrix pipe; conv3_m16 by the matrix pipe with
// spare issue slots.  Two waves of the same kind per SIMD cannot trade those; one producer + one consumer per
// SIMD can.  On the way, the a2 activation [B][T/4][F][64] (471 MB stored + ~490 MB re-read per step at the headline
// shape) no longer goes through HBM: producers write each pooled a2 row with ds_write_b128 straight into the consumers'
// LDS ring, in block 3's layout (128 B per pixel slot, 16-byte chunk c at c ^ (slot & 6)).
//
// Columns.  Block 3 of strip f0 reads a2 columns f0-1 .. f0+30 (ring slots 0..31), so the producers' 32-pixel block-2
// tile computes exactly those: it needs a1 columns f0-2 .. f0+31 (ring slots 0..33) and feature columns f0-3 .. f0+32.
// a1 slots 0..31 are the block-1 tile of conv12_fused shifted by one column; slots 32 and 33 come from a second block-1
// tile through the same MFMAs (lanes 0, 1 of it are live).  MFMA output columns are independent, so every a1 / a2 value
// is bit-identical to the one conv12_fused computes, and block 3 sees exactly the bf16 a2 that conv3_m16 reads from HBM.
// Out-of-image a2 slots (column -1, columns >= F, rows >= H2, row -1) hold explicit zeros, chosen by select.
//
// Schedule.  One s_barrier per step serves both roles.  Producer iteration p (= step p) writes a2 rows 2p, 2p+1 at the
// end of its unit; consumer iteration it needs rows 2it-1 .. 2it+2 and runs in step it + 2.  Consumer ring block j holds
// a2 rows 2j-1, 2j in slot j % 4: at step s the consumers read blocks s-2, s-1 while the producers write blocks s, s+1
// (after the step's barrier), so four blocks are enough.  Steps: niter3 + 2 (producers idle in the last two, consumers
// in the first two).
//
// The two role bodies live in conv123_body.h, shared with the persistent form of this kernel (conv123_persist.hip).
#define DFA_CONV123_BODY_SCOPE
#include "conv123_body.h"

namespace dfa {

// PIPE = false is the compiler-scheduled twin (plain LDS loads and stores, same arithmetic): bit-identical output
template <typename TX, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv123_fused_kernel(Conv123Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  c123_workgroup<TX, PIPE, false>(a, smem);
}

hipError_t launch_conv123_fused(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe) {
  return c123_launch(DFA_C123_KERNEL(conv123_fused_kernel, x_dtype, pipe), DFA_CONV123_PER_UNIT, "conv123", a, num_cus, s);
}

}  // namespace dfa

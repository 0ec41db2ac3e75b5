// conv123_persist.hip -- the CNN2D blocks 1-3 kernel of conv123_fused.hip as ONE workgroup per CU that walks a contiguous
// range of (utterance, 30-column strip) units (context option "persist123", the default where the dispatcher fuses blocks 1-3).
//
// Why.  conv123_fused runs one 512-thread workgroup per CU (254 VGPRs x 8 waves), so a CU works its units strictly one
// after the other, and with one workgroup per unit each of them pays, with the whole matrix pipe of the CU idle: the weight
// images from L2 into registers (58 uint4 per lane), the LDS fills, three dependent feature-load round trips before the
// first block-2 step, the store of the time mean, and the retire / dispatch turn-around of the workgroup.  Here a workgroup
// pays them once; between two of its units the producers stage the next unit while the consumers finish this one.
//
// Ranges.  grid = min(units, CUs); workgroup w (after the blockIdx -> XCD remap of conv123_fused: neighbouring ranges on
// one XCD) owns units [w q + min(w, rem), ...) of q or q + 1 units, q = units / grid, rem = units % grid, in the per-unit
// kernel's `logical` order: the strips of an utterance back to back.  Static: no flag, no atomic, no wait on another
// workgroup; the result does not depend on which workgroups are resident together or in which order they run.
//
// Unit boundary (conv123_body.h, PERSIST).  Barriers are workgroup-wide; both roles execute the same sequence:
//
//     producers (waves 0-3)                                   consumers (waves 4-7)
//     step niter3 - 1 of unit v (last a2 rows)                iteration niter3 - 3
//     zero row 2 niter3; x_load(0), x_load(1) of unit v + 1   iteration niter3 - 2, first reads
//   T1 ------------------------------------------------------------------------------ (idle step niter3 of unit v)
//     x_store(0); x_load(2); x_store(1)                       iteration niter3 - 2 / iteration niter3 - 1, first reads
//   T2 ------------------------------------------------------------------------------ (idle step niter3 + 1)
//     produce_now(0), produce_now(1): a1 ring blocks 0, 1     iteration niter3 - 1 (a2 ring blocks niter3 - 1, niter3)
//   N1 ------------------------------------------------------------------------------ (the one boundary barrier)
//     x_store(0) of feature block 2; step 0 of unit v + 1     zero a2 row -1; time mean of unit v -> emb; totals = 0
//
// so a unit after the first of its workgroup has niter3 + 3 barriers (N1, niter3 steps, two idle steps) where the first
// has niter3 + 6.  LDS ownership across the boundary:
//   * feature windows, a1 ring: written and read by the producers only, but every producer wave reads all of them.  The last
//     reads of unit v (c1_issue and the ring fragment reads of step niter3 - 1) are counted and drained before T1; the window
//     stores follow T1, the a1 ring stores T2; the third window store follows N1, behind produce_now's window reads.
//   * a2 ring: the consumers' last two iterations read blocks (niter3 - 2 .. niter3) mod 4 and are finished at N1.  The
//     consumers then zero row -1 (block 0, row 0); the producers' first a2 rows of unit v + 1 (rows 0, 1 = block 0 row 1,
//     block 1 row 0) are stored behind the barrier of step 0, i.e. after N1 too, to different rows.  The zero row 2 niter3 of
//     unit v (block niter3 mod 4, row 1) is written before T1, as in the per-unit kernel, and unit v + 1 writes that row
//     again (a pooled row, behind N1) before it reads it.  This holds for every residue of niter3 mod 4: nothing above
//     depends on which block number coincides with block 0.
//   * running totals: 16 LDS words per consumer lane that no other lane touches; read out, then zeroed, in program order.
//   * bias2 / bias3 in LDS, window pads (slots 34, 35 and bytes 6, 7 of a slot: x_store rewrites every other byte of both
//     window buffers for each feature block, out-of-image entries as zeros): written once, before the first barrier.
#define DFA_CONV123_BODY_SCOPE
#include "conv123_body.h"

namespace dfa {

// PIPE = false is the compiler-scheduled twin, as in conv123_fused.hip
template <typename TX, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv123_persist_kernel(Conv123Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  c123_workgroup<TX, PIPE, true>(a, smem);
}

hipError_t launch_conv123_persist(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe) {
  return c123_launch(DFA_C123_KERNEL(conv123_persist_kernel, x_dtype, pipe), DFA_CONV123_PERSIST, "conv123 persist", a, num_cus, s);
}

}  // namespace dfa

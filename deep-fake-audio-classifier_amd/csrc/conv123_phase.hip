// conv123_phase.hip -- conv123_carry.hip with the two roles' step edges moved apart (context option "phase123", the default
// where the carry form runs: cnn2d_api.hip).  Same arguments, same launch conditions, same LDS layout, same arithmetic instruction
// for instruction; the two differences are where the consumers' step barrier stands in their fragment-read stream
// (DFA_C123_CBAR = 35 instead of 4) and that the consumer waves run at s_setprio 1 (DFA_C123_PRIO = 1).
//
// Why.  In a paired step each role runs an MFMA-free edge (drain of its last MFMAs, ReLU / time-mean or a2 hand-off, bias
// and first fragment reads), then five fragment reads, the barrier, then its MFMA stream.  With both barriers behind read 4
// the two edges of a SIMD's wave pair end at the same barrier.  Behind read 35 the consumers' edge lies three quarters into a
// barrier interval, under the producers' stream, and the producers' edge under the consumers'.  Alone that position is
// slower than the parent's: the matrix pipe serves the producers first, and the consumers' 2304 of a step's 3584 pipe cycles
// bound the step.  With the consumers' MFMAs given issue priority it is the fastest of the sweep: a paired step 4505
// instead of 4819 cycles, part of it paid back in held clock ("de-phased step edges": every variant measured
// is listed there).
//
// Ownership of the a2 ring.  Barrier #k is the k-th step barrier of a unit.
//   Producers.  Iteration k holds #k.  It writes a2 row 2k -> ring block k row 1 and row 2k + 1 -> block k + 1 row 0 behind its
//   MFMA stream, i.e. in the interval [#k, #k+1); the stores have completed before the wave reaches #(k+1) (in-order LDS,
//   counted wait in front of that barrier).
//   Consumers.  Iteration `it` holds #(it+2): the two idle barriers of a unit are #0, #1.  Its 48 fragment reads:
//     reads  0 .. 23   block it (rows 2it - 1, 2it)           written in [#it, #it+1) at the latest    legal anywhere behind #(it+1)
//     reads 24 .. 35   block it+1 row 0 (row 2it + 1)         written in [#it, #it+1)                   legal anywhere behind #(it+1)
//     reads 36 .. 47   block it+1 row 1 (row 2it + 2)         written in [#it+1, #it+2)                 must stand behind #(it+2)
//   #(it+1) is the barrier of the iteration before, or the second idle barrier for it = 0.  Hence CBAR <= 35 (static_assert
//   in conv123_body.h), and 35 is the last position: every read that may precede the barrier does.
//   Write after read.  In [#k, #k+1) the consumers read block k-1 and, as reads 24 .. CBAR of iteration k-1, block k row 0
//   (the reads of iteration k-2 behind its barrier are blocks k-2 and k-1).  In the same interval the producers write block k
//   row 1 and block k+1 = k-3 (mod 4) row 0: other rows.  The next writer of any slot is four steps away.
//   Unit boundary.  Nothing changes: the producers' zero row 2 niter3 (written before T1 into a row whose last reader had
//   finished before the barrier that opens that interval), T1 / T2 / N1, the consumers' zeroing of row -1 behind N1, the
//   side buffer (producer waves only, no barrier: conv123_carry.hip).  The consumers merely arrive at N1 with fewer reads
//   behind their last step barrier.
// The counted lgkmcnt waits of the consumers count reads only and are those of the carry form: the barrier is no LDS
// operation.  tests/test_phase123_cpu.py walks both roles interval by interval for niter3 = 1 .. 48 and every CBAR = 0 .. 35,
// and shows that 36 races.
#define DFA_CONV123_BODY_SCOPE
#define DFA_C123_CARRY 1
#define DFA_C123_CBAR 35
#define DFA_C123_PRIO 1
#include "conv123_body.h"

namespace dfa {

// PIPE = false is the compiler-scheduled twin, as in conv123_fused.hip; arguments, conditions and LDS bytes are the carry form's
// (one plan: conv123_plan in conv123_carry.hip)
template <typename TX, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv123_phase_kernel(Conv123Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  c123_workgroup<TX, PIPE, true>(a, smem);
}

hipError_t launch_conv123_phase(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe) {
  return c123_launch(DFA_C123_KERNEL(conv123_phase_kernel, x_dtype, pipe), DFA_CONV123_CARRY, "conv123 phase", a, num_cus, s);
}

}  // namespace dfa

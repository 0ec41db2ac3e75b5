// conv123_cls.hip -- conv123_phase.hip with the classifier head inside the kernel, and, as a build option, the time-mean stores
// moved off the producers' step 0: two pieces of work on the critical path outside the paired steps (context
// option "cls123", the default wherever the phase form runs: cnn2d_api.hip).  Same launch conditions, same LDS layout, same
// arithmetic in the paired steps; the embedding is written as before and logits and embedding are the same bits.
//
// 1. Late EMIT (DFA_C123_LATE_EMIT; NOT in the shipped kernel: as a part of its own it was within noise of the parent, DESIGN
//    3.4b.  The code and its barrier model stay as a build option, -DDFA_C123_LATE_EMIT=1).  In the phase form the consumers, behind the boundary barrier N1, zero ring row -1, store
//    the time mean of the finished unit (16 scattered stores per lane), zero their totals and only then pass the two idle
//    barriers of the next unit.  The first of those is the barrier of the producers' step 0, a lone step on the critical
//    path: the producers stand there until the stores have been issued.  Here, for every unit but the last of the range:
//        N1, zero ring row -1          (as before)
//        idle barrier 0
//        EMIT of the finished unit, with its b and f0; zero `tot`; advance u, b, f0
//        idle barrier 1
//    The last unit of the range is unchanged.  Ownership:
//      - `tot` words are lane-private: read by EMIT, zeroed behind it, first written again by the flush that follows an
//        iteration of the new unit, all by the same lane in program order.
//      - The zeroing of ring row -1 is still separated from its first reader (the consumers' iteration 0) by both idle
//        barriers, and from the producers' first write of block 0 (behind their step-0 barrier = idle barrier 0) as before.
//      - EMIT touches no LDS another wave reads: it reads the lane's `tot` words and writes global memory.
//    Both roles still execute niter3 + 3 barriers per unit after the first; tests/test_cls123_cpu.py walks them.
//    Variant DFA_C123_EMIT_PRIO0 (the consumers drop to s_setprio 0 around EMIT, which now runs beside the producers' step
//    0): DESIGN 3.4b says which of the two ships.
//
// 2. Classifier in the kernel (DFA_C123_CLS).  A workgroup of the carry form owns whole utterances.  Behind the last unit's
//    EMIT its four consumer waves -- 256 threads, linear1_kernel's block -- run that kernel's operation sequence over emb[b]
//    for each of their utterances (c123_classifier in conv123_body.h: visibility, barriers and the LDS words it uses are
//    argued there).  No cross-workgroup reduction, no atomics; the producers execute the same trailing barriers and return.
//    The dispatcher then launches no linear1_kernel.
//
// Both macros can be set to 0 on the command line: scratch builds that measure each part alone (conv123_cls_in_kernel tells
// the dispatcher whether the head ran).
#define DFA_CONV123_BODY_SCOPE
#define DFA_C123_CARRY 1
#define DFA_C123_CBAR 35
#define DFA_C123_PRIO 1
#ifndef DFA_C123_LATE_EMIT
#define DFA_C123_LATE_EMIT 0   // measured alone: not faster in every pair, so the shipped kernel leaves it out
#endif
#ifndef DFA_C123_CLS
#define DFA_C123_CLS 1
#endif
#include "conv123_body.h"

namespace dfa {

// PIPE = false is the compiler-scheduled twin, as in conv123_fused.hip; conditions and LDS bytes are the carry form's
template <typename TX, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv123_cls_kernel(Conv123Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  c123_workgroup<TX, PIPE, true>(a, smem);
}

int conv123_cls_in_kernel() { return DFA_C123_CLS; }

hipError_t launch_conv123_cls(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe) {
  if (DFA_C123_CLS && (!a.cls_w || !a.cls_b || !a.logits || a.cls_K != 128 * a.F || (((uintptr_t)a.cls_w | (uintptr_t)a.emb) & 15) != 0))
    return hipErrorInvalidValue;
  return c123_launch(DFA_C123_KERNEL(conv123_cls_kernel, x_dtype, pipe), DFA_CONV123_CARRY, "conv123 cls", a, num_cus, s);
}

}  // namespace dfa

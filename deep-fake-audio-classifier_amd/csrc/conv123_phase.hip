// conv123_phase.hip -- conv123_carry.hip with the two roles' step edges moved apart (context option "phase123", the default
// where the carry form runs: api.hip).  Same arguments, same launch conditions, same LDS layout, same arithmetic instruction
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

// PIPE = false is the compiler-scheduled twin, as in conv123_fused.hip
template <typename TX, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv123_phase_kernel(Conv123Args a) {
  using namespace c123;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = bid & 7, xi = bid >> 3;
  const int lw = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + xi;
  const int uq = (a.B * a.nstrips) / nwg;                  // the launcher: no remainder, a multiple of nstrips
  const int u0 = lw * uq, u1 = u0 + uq;
  const int b = u0 / a.nstrips, strip = u0 - b * a.nstrips;    // strip = 0
  const int f0 = strip * SW;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int niter3 = (a.H2 + 1) / 2;
  if (wave < 4) c123_producer<TX, PIPE, true>(a, smem, lds0, tid, wave, b, f0, niter3, u0, u1);
  else c123_consumer<PIPE, true>(a, smem, lds0, tid - 256, wave - 4, b, f0, niter3, u0, u1);
}

template <typename TX, bool PIPE>
static hipError_t launch_conv123_phase_t(const Conv123Args& a, int num_cus, hipStream_t s) {
  const int nunits = a.B * a.nstrips;
  const size_t lds = conv123_carry_lds_bytes(a.T);     // the carry form's layout, side buffer included
  // (the carry form's conditions, checked again: a range that began inside an utterance would read an entry nobody wrote)
  if (nunits < num_cus || nunits % num_cus != 0 || (nunits / num_cus) % a.nstrips != 0 || lds > 160 * 1024) return hipErrorInvalidValue;
  auto kern = conv123_phase_kernel<TX, PIPE>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;       // (per device: set on every launch, it is cheap)
  hipLaunchKernelGGL(kern, dim3(num_cus), dim3(512), lds, s, a);
#ifdef DFA_STAMPS
  {
    static int calls = 0;      // seconds of back-to-back launches: the clock has settled (tools/gpu_stamps.py)
    if (++calls == 4000) c123_print_stamps("conv123 phase", num_cus);
  }
#endif
  return hipGetLastError();
}

hipError_t launch_conv123_phase(const void* x, int x_dtype, int64_t sb, int64_t st, int64_t sf, const uint4* c1pack,
                                const float* c1bias, const uint4* wpack2, const float* bias2, const uint4* wpack3,
                                const float* bias3, float* emb, int B, int T, int F, int chunk_iters, long long* clock_stamps,
                                int num_cus, hipStream_t s, int pipe) {
  if (num_cus < 1) return hipErrorInvalidValue;
  const Conv123Args a = c123_args(x, sb, st, sf, c1pack, c1bias, wpack2, bias2, wpack3, bias3, emb, B, T, F, chunk_iters, clock_stamps);
  if (x_dtype == DFA_DTYPE_BF16) return pipe ? launch_conv123_phase_t<bf16_t, true>(a, num_cus, s) : launch_conv123_phase_t<bf16_t, false>(a, num_cus, s);
  return pipe ? launch_conv123_phase_t<float, true>(a, num_cus, s) : launch_conv123_phase_t<float, false>(a, num_cus, s);
}

}  // namespace dfa

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
  using namespace c123;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = bid & 7, xi = bid >> 3;
  const int lw = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + xi;
  const int nunits = a.B * a.nstrips;
  const int uq = nunits / nwg, urem = nunits - uq * nwg;
  const int u0 = lw * uq + min(lw, urem), u1 = u0 + uq + (lw < urem ? 1 : 0);   // nwg <= nunits: never empty
  const int b = u0 / a.nstrips, strip = u0 - b * a.nstrips;
  const int f0 = strip * SW;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int niter3 = (a.H2 + 1) / 2;
  if (wave < 4) c123_producer<TX, PIPE, true>(a, smem, lds0, tid, wave, b, f0, niter3, u0, u1);
  else c123_consumer<PIPE, true>(a, smem, lds0, tid - 256, wave - 4, b, f0, niter3, u0, u1);
}

template <typename TX, bool PIPE>
static hipError_t launch_conv123_persist_t(const Conv123Args& a, int num_cus, hipStream_t s) {
  auto kern = conv123_persist_kernel<TX, PIPE>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, c123::LDS_BYTES);
  if (e != hipSuccess) return e;       // (per device: set on every launch, it is cheap)
  const int nunits = a.B * a.nstrips;
  hipLaunchKernelGGL(kern, dim3(nunits < num_cus ? nunits : num_cus), dim3(512), c123::LDS_BYTES, s, a);
#ifdef DFA_STAMPS
  {
    static int calls = 0;      // seconds of back-to-back launches: the clock has settled (tools/gpu_stamps.py)
    if (++calls == 4000) c123_print_stamps("conv123 persist", nunits < num_cus ? nunits : num_cus);
  }
#endif
  return hipGetLastError();
}

hipError_t launch_conv123_persist(const void* x, int x_dtype, int64_t sb, int64_t st, int64_t sf, const uint4* c1pack,
                                  const float* c1bias, const uint4* wpack2, const float* bias2, const uint4* wpack3,
                                  const float* bias3, float* emb, int B, int T, int F, int chunk_iters, long long* clock_stamps,
                                  int num_cus, hipStream_t s, int pipe) {
  if (num_cus < 1) return hipErrorInvalidValue;
  const Conv123Args a = c123_args(x, sb, st, sf, c1pack, c1bias, wpack2, bias2, wpack3, bias3, emb, B, T, F, chunk_iters, clock_stamps);
  if (x_dtype == DFA_DTYPE_BF16) return pipe ? launch_conv123_persist_t<bf16_t, true>(a, num_cus, s) : launch_conv123_persist_t<bf16_t, false>(a, num_cus, s);
  return pipe ? launch_conv123_persist_t<float, true>(a, num_cus, s) : launch_conv123_persist_t<float, false>(a, num_cus, s);
}

}  // namespace dfa

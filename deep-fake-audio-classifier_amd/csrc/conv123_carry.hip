// conv123_carry.hip -- conv123_persist.hip with the two a1 halo columns on the left of a strip carried over from the strip
// before it instead of computed again (context option "carry_a1", the default where its conditions hold: api.hip; with
// option "phase123" at its default the dispatcher runs this form as built by conv123_phase.hip, with 0 this file's kernel).
//
// Why.  A strip owns 30 output columns, f0 .. f0 + 29.  Block 2 needs the a1 columns f0 - 2 .. f0 + 31 = ring slots 0 .. 33,
// and block 1 makes them with 32-column MFMA tiles: in the two older kernels tile 0 = slots 0 .. 31 and tile 1 = slots 32, 33,
// a whole tile (4 of a step's 44 MFMAs, a quarter of its vector instructions) for two live columns.  But slots 0, 1 of strip
// k + 1 are the a1 columns f0 + 28, f0 + 29 that strip k has just computed as its slots 30, 31, the persistent kernel walks
// the strips of an utterance back to back in one workgroup, and the columns of an MFMA result do not depend on one another:
// the values are the same bits.  So here tile 0 is slots 2 .. 33 (lane r owns slot 2 + r, column f0 + r), there is no tile
// 1, and slots 0, 1 come from the previous unit -- or are zeros for the first strip of an utterance, whose columns -2, -1
// lie off the image.  The launcher's condition: every workgroup's range starts at the first strip of an utterance.
//
// Side buffer.  LDS behind the producer region (c123::SIDE_OFF): one 128-byte entry per a1 row a unit produces, i.e. four
// per ring block j = 0 .. niter3 + 1, entry 4 j + m for ring row m.  An entry is the image of ring slots 0, 1 of that row:
// 2 slots x 64 B, 16-byte chunks at (chunk ^ lds_swz(slot)) = chunk, packed bf16 as the ring holds them.
//
// Per-row sequence.  Ring row m of every block is produced by producer wave m (c1_m) and by no other.  When that wave has
// the tile-0 values of row (j, m), it issues, in this program order:
//   1. reads of entry (j, m): what the previous unit left there (all lanes; lanes 28, 29, 60, 61 use them)
//   2. the tile-0 stores into ring slots 2 .. 33
//   3. lanes 28, 29, 60, 61: stores of their own chunks (slots 30, 31 of this row) over entry (j, m)
//   4. once the reads have landed: lanes 28, 29, 60, 61 store them -- zeros instead where this unit is the first strip of
//      its utterance, by a select, so that neither stale LDS nor another utterance's NaN can reach a sum -- into ring
//      slots 0, 1.
// Every access to an entry comes from one wave (even from one lane per chunk), and the LDS operations of a wave complete in
// the order it issued them: read 1 returns the previous unit's bytes although store 3 follows it at once, and store 3 of
// unit v is in LDS long before read 1 of unit v + 1.  So the side buffer needs no barrier and takes part in none.  The ring
// stores 2 and 4 go to disjoint slots of a ring row that block 2 reads behind the same barriers as before: the ownership
// argument at the top of conv123_persist.hip holds word for word for everything else -- windows, a1 ring, a2 ring, totals.
// In the main loop (conv123_body.h, CARRY) 1 - 3 follow consume step C_STORE and 4 consume step C_CARRY = C_STORE + 4; the
// counted lgkmcnt of the steps between them includes all six and the two of step 4.
//
// The feature staging is the persistent kernel's: window columns f0 - 3, f0 - 2 are staged and not read.
#define DFA_CONV123_BODY_SCOPE
#define DFA_C123_CARRY 1
#include "conv123_body.h"

namespace dfa {

// PIPE = false is the compiler-scheduled twin, as in conv123_fused.hip
template <typename TX, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv123_carry_kernel(Conv123Args a) {
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

// dynamic LDS of the kernel for T frames; the dispatcher compares it with the CU's 160 KiB
size_t conv123_carry_lds_bytes(int T) {
  const int niter3 = (T / 2 / 2 + 1) / 2;
  return (size_t)c123::LDS_BYTES + (size_t)c123::side_bytes(niter3);
}

template <typename TX, bool PIPE>
static hipError_t launch_conv123_carry_t(const Conv123Args& a, int num_cus, hipStream_t s) {
  const int nunits = a.B * a.nstrips;
  const size_t lds = conv123_carry_lds_bytes(a.T);
  // (the dispatcher's conditions, checked again: a range that began inside an utterance would read an entry nobody wrote)
  if (nunits < num_cus || nunits % num_cus != 0 || (nunits / num_cus) % a.nstrips != 0 || lds > 160 * 1024) return hipErrorInvalidValue;
  auto kern = conv123_carry_kernel<TX, PIPE>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;       // (per device: set on every launch, it is cheap)
  hipLaunchKernelGGL(kern, dim3(num_cus), dim3(512), lds, s, a);
#ifdef DFA_STAMPS
  {
    static int calls = 0;      // seconds of back-to-back launches: the clock has settled (tools/gpu_stamps.py)
    if (++calls == 4000) c123_print_stamps("conv123 carry", num_cus);
  }
#endif
  return hipGetLastError();
}

hipError_t launch_conv123_carry(const void* x, int x_dtype, int64_t sb, int64_t st, int64_t sf, const uint4* c1pack,
                                const float* c1bias, const uint4* wpack2, const float* bias2, const uint4* wpack3,
                                const float* bias3, float* emb, int B, int T, int F, int chunk_iters, long long* clock_stamps,
                                int num_cus, hipStream_t s, int pipe) {
  if (num_cus < 1) return hipErrorInvalidValue;
  const Conv123Args a = c123_args(x, sb, st, sf, c1pack, c1bias, wpack2, bias2, wpack3, bias3, emb, B, T, F, chunk_iters, clock_stamps);
  if (x_dtype == DFA_DTYPE_BF16) return pipe ? launch_conv123_carry_t<bf16_t, true>(a, num_cus, s) : launch_conv123_carry_t<bf16_t, false>(a, num_cus, s);
  return pipe ? launch_conv123_carry_t<float, true>(a, num_cus, s) : launch_conv123_carry_t<float, false>(a, num_cus, s);
}

}  // namespace dfa

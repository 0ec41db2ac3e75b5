// conv123_carry.hip -- conv123_persist.hip with the two a1 halo columns on the left of a strip carried over from the strip
// before it instead of computed again (context option "carry_a1", the default where its conditions hold: conv123_plan below; with
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
  extern __shared__ __attribute__((aligned(16))) char smem[];
  c123_workgroup<TX, PIPE, true>(a, smem);
}

hipError_t launch_conv123_carry(const Conv123Args& a, int x_dtype, int num_cus, hipStream_t s, int pipe) {
  return c123_launch(DFA_C123_KERNEL(conv123_carry_kernel, x_dtype, pipe), DFA_CONV123_CARRY, "conv123 carry", a, num_cus, s);
}

// Which form runs blocks 1-3, for a shape the dispatcher fuses (cnn2d_api.hip) and the three options, and with what grid and dynamic
// LDS bytes: the one statement of the grid rule and of the carry form's conditions, asked by the dispatcher and by every entry.
Conv123Plan conv123_plan(int B, int T, int F, int num_cus, int persist123, int carry_a1, int phase123) {
  const int nstrips = (F + c123::SW - 1) / c123::SW, nunits = B * nstrips, niter3 = (T / 2 / 2 + 1) / 2;
  if (!persist123) return {DFA_CONV123_PER_UNIT, 0, nunits, (size_t)c123::LDS_BYTES};
  const int grid = std::min(nunits, num_cus);      // one workgroup per CU, or per unit where there are fewer (< 1: the entry refuses)
  // carry: every range is a whole number of utterances (it starts at strip 0), and the side buffer fits the CU's 160 KiB
  const size_t lds_carry = (size_t)c123::LDS_BYTES + (size_t)c123::side_bytes(niter3);
  if (!carry_a1 || grid < 1 || nunits % grid != 0 || (nunits / grid) % nstrips != 0 || lds_carry > (size_t)160 * 1024)
    return {DFA_CONV123_PERSIST, 0, grid, (size_t)c123::LDS_BYTES};
  return {DFA_CONV123_CARRY, phase123 != 0, grid, lds_carry};
}

}  // namespace dfa

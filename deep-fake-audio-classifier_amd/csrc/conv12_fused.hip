// conv12_fused.hip -- CNN2D blocks 1 and 2 in ONE kernel (bf16 mode; fp32 features are rounded to bf16 as they are loaded):
//   Conv2d(1,32,3,p=1)+BN+ReLU+AvgPool(2,1)  ->  Conv2d(32,64,3,p=1)+BN+ReLU+AvgPool(2,1)      (src/model.py:15-25)
// The block-1 activation a1 [B,160,180,32] (1.84 MB per utterance, written and re-read through HBM by the two-kernel
// path: 0.94 GB per step at B = 256) never leaves the chip: the workgroup that consumes a ring block of a1 rows
// produces it, from the raw features, straight into the LDS ring of conv3x3_mfma's block-2 main loop.
//
// Block 1 on the matrix cores.  One v_mfma_f32_32x32x16_bf16 has K = 16 = 4 feature rows x (3 taps + 1 zero): for the
// pooled a1 row q, the B operand of a 32-pixel tile holds x[2q-1 .. 2q+2][f-1 .. f+1] and serves BOTH conv rows of the
// pool pair -- the even row 2q through an A operand with weights on feature rows 0..2, the odd row 2q+1 through one
// with weights on rows 1..3.  The folded fp32 weights are split into bf16 hi + lo parts (w = hi + lo to 2^-17), one MFMA
// each: products of bf16 inputs are exact in the fp32 accumulator, so block 1 keeps fp32-level accuracy on bf16 input.
// Cost: 4 MFMAs per a1 tile against the 36 of the block-2 work that consumes it.
//
// Strips are 30 output columns wide: with the two halo columns a ring row has exactly 32 live slots = ONE block-1 MFMA
// tile per a1 row, one tile per wave per iteration (180 = 6 x 30: the block-2 MFMAs still compute 6 x 32 columns, the
// same count the 32-wide strips of the unfused kernel spend on their ragged last strip).
//
// LDS: [block-2 ring 3 x 4 rows x 36 slots x 64 B][bias2][2 x feature-window tiles 10 rows x 36 slots x 8 B].
// A window entry is {x[f-1], x[f], x[f+1], 0} (4 bf16), i.e. one half of a lane's B operand: the lane reads two of them
// (ds_read_b64 x 2).  Pipeline per iteration `it` (one __syncthreads each, like the unfused kernel):
//   global-load the features of ring block it+3 -> registers;  block-2 MFMA unit on ring blocks it, it+1 with the wave's
//   block-1 tile of ring block it+2 (window buffer it&1 -> ring slot (it+2)%3) and the register -> window buffer
//   (it+3)&1 stores threaded through its MFMA stream, so the block-1 VALU work hides in the MFMA shadow.
#include <stdlib.h>

#include "dfa_internal.h"

namespace dfa {

struct Conv12Args {
  const void* x;            // features (bf16 or fp32: template argument TX), element strides below (any layout)
  long long sxb, sxt, sxf;
  const uint4* c1pack;      // [4][64] A operands: even-hi, even-lo, odd-hi, odd-lo (pack.hip: pack_conv1_mfma_kernel)
  const float* c1bias;      // [32]  0.5 * folded bias
  const uint4* wpack;       // block 2 image [2][9][2][64] (pool factor folded)
  const float* bias;        // [64]
  bf16_t* out;              // a2 [B][H1/2][F][64]
  int B, T, F, H1, nstrips;
  int seg_iters;            // time-axis split for small batches: blockIdx.y walks seg_iters iterations (multiple of 6), 0 = all
};

namespace c12 {
constexpr int PB = 64, SP = 36, ROWB = SP * PB, BR = 4, NKG = 2, PF = 4, SW = 30;   // SW: output columns per strip
constexpr int RING_BYTES = 3 * BR * ROWB;
constexpr int BIAS2_OFF = RING_BYTES, XW_OFF = BIAS2_OFF + 64 * 4;
constexpr int XROWS = 10, XW_ROWB = SP * 8, XW_BYTES = XROWS * XW_ROWB;
constexpr int DUMMY_OFF = XW_OFF + 2 * XW_BYTES;   // sink for the window stores of out-of-tile taps (keeps them branch-free)
constexpr int LDS_BYTES = DUMMY_OFF + 16;
constexpr int XCOLS = 34;                 // feature columns per ring block: 32 slots + 1 more each side
constexpr int NX = XROWS * XCOLS;
constexpr int NXLD = (NX + 255) / 256;
}  // namespace c12

#ifdef DFA_STAMPS
static __device__ long long g_diag12[2048 * 4 * 8];
#endif

// PIPE = false is the compiler-scheduled twin (plain LDS loads, same arithmetic): the GPU tests require bit-identical output
// RAGGED = true: variable-length batch (dfa_cnn2d_forward_ragged).  The workgroup's utterance comes from the dispatch order
// of the ragged table and its own length T_b sets H, the trip count, the row masks and the segment range; a.T / a.H1 are
// the batch maximum and only fix the a2 row pitch.  Rows t >= T_b of x are never read.

#define DFA_KERNEL_BODY_SCOPE   // the kernel bodies below include conv12_body.h
template <typename TX, bool PIPE>
__global__ __launch_bounds__(256, 2) void conv12_fused_kernel(Conv12Args a) {
  constexpr bool RAGGED = false;
  const RaggedTab rt{};
#include "conv12_body.h"
}

template <typename TX, bool PIPE>
__global__ __launch_bounds__(256, 2) void conv12_ragged_kernel(Conv12Args a, RaggedTab rt) {
  constexpr bool RAGGED = true;
#include "conv12_body.h"
}
#undef DFA_KERNEL_BODY_SCOPE

// A operands of the block-1 MFMAs.  Lane (ch = lane&31, hh = lane>>5), element j: k = 8*hh + j, feature row dyy = k/4,
// tap dx = k%4 (dx = 3 is the zero pad).  even conv row: weight (dyy, dx) for dyy <= 2; odd: weight (dyy-1, dx), dyy >= 1.
__global__ void pack_conv1_mfma_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                       uint4* __restrict__ c1pack, float* __restrict__ c1bias) {
  const int i = threadIdx.x;   // 256 threads: (operand k = i / 64, lane = i % 64)
  if (i < 32) c1bias[i] = 0.5f * b1[i];   // 16-byte aligned rows of 4: read as float4 by the kernel
  const int op = i >> 6, lane = i & 63, ch = lane & 31, hh = lane >> 5;
  const bool odd = op >= 2, lo = op & 1;
  bf16_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * hh + j, dyy = k >> 2, dx = k & 3;
    const int dy = odd ? dyy - 1 : dyy;
    float wv = 0.f;
    if (dx < 3 && dy >= 0 && dy <= 2) wv = 0.5f * w1[ch * 9 + dy * 3 + dx];
    const bf16_t hi = float_to_bf16(wv);
    v[j] = lo ? float_to_bf16(wv - bf16_to_float(hi)) : hi;
  }
  c1pack[i] = *reinterpret_cast<const uint4*>(v);
}

hipError_t launch_pack_conv1_mfma(const float* w1, const float* b1, uint4* c1pack, float* c1bias, hipStream_t s) {
  hipLaunchKernelGGL(pack_conv1_mfma_kernel, dim3(1), dim3(256), 0, s, w1, b1, c1pack, c1bias);
  return hipGetLastError();
}

template <typename TX, bool PIPE>
static hipError_t launch_conv12_t(const Conv12Args& a, int B, hipStream_t s) {
  auto kern = conv12_fused_kernel<TX, PIPE>;
#ifdef DFA_STAMPS
  // diagnostic build only: DFA_C12_LDS_PAD=<bytes> pads the dynamic LDS request (e.g. 60000 -> one workgroup per CU, one wave per SIMD)
  static const int lds_bytes = c12::LDS_BYTES + (getenv("DFA_C12_LDS_PAD") ? atoi(getenv("DFA_C12_LDS_PAD")) : 0);
#else
  constexpr int lds_bytes = c12::LDS_BYTES;
#endif
  const int niter = (a.H1 + c12::BR - 1) / c12::BR;
  const int nseg = a.seg_iters ? (niter + a.seg_iters - 1) / a.seg_iters : 1;
  return launch_lds(kern, dim3(B * a.nstrips, nseg), dim3(256), lds_bytes, s, a);
}

template <typename TX, bool PIPE>
static hipError_t launch_conv12_ragged_t(const Conv12Args& a, const RaggedTab& rt, int B, hipStream_t s) {
  auto kern = conv12_ragged_kernel<TX, PIPE>;
  const int niter = (a.H1 + c12::BR - 1) / c12::BR;      // of the longest utterance; shorter ones leave their late segments at once
  const int nseg = a.seg_iters ? (niter + a.seg_iters - 1) / a.seg_iters : 1;
  return launch_lds(kern, dim3(B * a.nstrips, nseg), dim3(256), c12::LDS_BYTES, s, a, rt);
}

// ragged batch: x is [B, T_max, F] (strided), a2 is [B][T_max/4][F][64] with utterance b's rows 0 .. T_b/4 - 1 written
hipError_t launch_conv12_ragged(const FeatView& v, const uint4* c1pack, const float* c1bias, const uint4* wpack2, const float* bias2, void* a2,
                                const int* tab, hipStream_t s, int pipe, int seg_iters) {
  const int B = v.B;
  Conv12Args a{};
  a.seg_iters = seg_iters;
  a.x = v.x; a.sxb = v.sb; a.sxt = v.st; a.sxf = v.sf;
  a.c1pack = c1pack; a.c1bias = c1bias; a.wpack = wpack2; a.bias = bias2; a.out = (bf16_t*)a2;
  a.B = B; a.T = v.T; a.F = v.F; a.H1 = v.T / 2; a.nstrips = (v.F + c12::SW - 1) / c12::SW;
  const RaggedTab rt{tab, B};
  if (v.dtype == DFA_DTYPE_BF16) return pipe ? launch_conv12_ragged_t<bf16_t, true>(a, rt, B, s) : launch_conv12_ragged_t<bf16_t, false>(a, rt, B, s);
  return pipe ? launch_conv12_ragged_t<float, true>(a, rt, B, s) : launch_conv12_ragged_t<float, false>(a, rt, B, s);
}

hipError_t launch_conv12_fused(const FeatView& v, const uint4* c1pack, const float* c1bias, const uint4* wpack2, const float* bias2, void* a2,
                               hipStream_t s, int pipe, int seg_iters) {
  const int B = v.B;
  Conv12Args a{};
  a.seg_iters = seg_iters;
  a.x = v.x; a.sxb = v.sb; a.sxt = v.st; a.sxf = v.sf;
  a.c1pack = c1pack; a.c1bias = c1bias; a.wpack = wpack2; a.bias = bias2; a.out = (bf16_t*)a2;
  a.B = B; a.T = v.T; a.F = v.F; a.H1 = v.T / 2; a.nstrips = (v.F + c12::SW - 1) / c12::SW;
  hipError_t le;
  if (v.dtype == DFA_DTYPE_BF16) le = pipe ? launch_conv12_t<bf16_t, true>(a, B, s) : launch_conv12_t<bf16_t, false>(a, B, s);
  else le = pipe ? launch_conv12_t<float, true>(a, B, s) : launch_conv12_t<float, false>(a, B, s);
  if (le != hipSuccess) return le;
#ifdef DFA_STAMPS
  {
    static int calls = 0;
    if (++calls == 4000) {        // seconds of back-to-back launches: the clock has settled
      static long long hbuf[2048 * 4 * 8];
      hipDeviceSynchronize();
      hipMemcpyFromSymbol(hbuf, HIP_SYMBOL(g_diag12), sizeof(hbuf));
      const int nw = (B * a.nstrips < 2048 ? B * a.nstrips : 2048) * 4;
      double m[8] = {0};
      for (int i = 0; i < nw; ++i) { for (int k = 0; k < 6; ++k) m[k] += hbuf[i * 8 + k]; m[6] += hbuf[i * 8 + 7] - hbuf[i * 8 + 6]; }
      fprintf(stderr, "[stamps conv12] in-kernel clock %.3f GHz (shader cycles / 100 MHz real-time ticks, mean over waves)\n", m[6] / (m[4] * 10.0));
      fprintf(stderr, "[stamps conv12] waves %d  mean cycles/wave: x_load %.0f  mfma_stream %.0f  epilogue %.0f  barrier %.0f  prologue %.0f  lifetime %.0f\n",
              nw, m[0] / nw, m[1] / nw, m[2] / nw, m[3] / nw, m[5] / nw, m[6] / nw);
    }
  }
#endif
  return hipGetLastError();
}

}  // namespace dfa

// conv3x3_mfma.h -- 3x3 / pad 1 convolution as an implicit GEMM on the gfx950 matrix cores, with the
// BatchNorm(eval, folded) + ReLU + pooling / time-mean epilogue fused in.
//
// Replaces, per launch, one "Conv2d -> BatchNorm2d -> ReLU [-> AvgPool2d]" group of the reference:
//   src/model.py:21-25 (block 2), :27-29 + :37 (block 3 + mean over T),
//   src/model_cae.py:40-55 (encoder blocks 2-4); in train mode (EPI_PLAIN) it stores the pre-BatchNorm output
//   and serves as the data-gradient convolution of loss.backward() (src/train.py:75).
//
// Data layout (HBM): activations are channels-last  act[b][t][f][c]  so that one tap of one pixel is
// CIN contiguous elements; weights are pre-packed by pack.hip in the exact register order the MFMA
// operand wants:  wpack[cout/32][tap][kgroup][lane] (16 bytes each).
//
// Work decomposition
//   workgroup  = (utterance b, strip of 32 feature columns, chunk of 32*NSL output channels); it walks
//                DOWN the time axis keeping a ring of input rows in LDS, so every input element is read from
//                HBM once per strip (+2 halo columns) and there is no vertical halo re-read.
//   wave       = (N-slice nsl of 32 output channels, M-group mg).  The wave keeps its full 9 x CIN x 32 weight
//                slice in VGPRs for the whole kernel, and streams activation fragments from the LDS ring.
//   iteration  = 2*RP output rows (RP row pairs).  A "unit" is one pair of 32-pixel tiles (rows t, t+1; same
//                32 columns): both accumulators share the fragments of the two input rows they have in
//                common, so a unit issues 12*NKG ds_read_b128 for 18*NKG k-groups of MFMA work.
//   staging    = ring block j holds input rows [2RP*j-1, 2RP*(j+1)-1).  Iteration `it` computes from
//                blocks it, it+1 while block it+2 is fetched (through registers, or by LDS-DMA), one
//                __syncthreads() per iteration.
//
// Instruction economy (rocprofv3 showed ~5 VALU per MFMA in the first version; the matrix pipe shares issue slots
// with the VALU):
//   * LDS image: pixel slot s of ring row q owns PB = CIN*sizeof(T) bytes at (q*SP + s)*PB; 16-byte chunk c sits at
//     physical chunk c ^ swz(s).  The swizzle depends on the COLUMN only and SP*PB is a multiple of 256 bytes, so
//     (a) the 16 lanes of every ds_read_b128 lane group (consecutive columns, same logical chunk) hit 16 distinct
//     bank slots, and (b) a lane's byte offset inside a row is loop-invariant: it is computed once, the k-group is
//     one XOR with an immediate, and -- the iteration loop being unrolled over the ring period 3 -- the row offset
//     is an instruction immediate.
//   * staging addresses are per-thread constants plus a per-iteration scalar.
//   * MFMA operands are swapped: weights are the A operand, activations the B operand, so the accumulator holds
//     pixel = lane&31 and channels (i&3)+8*(i>>2)+4*(lane>>5) in its 16 registers.  Bias is the accumulator's initial
//     value; every lane owns 4 consecutive channels x 4 groups of its pixel, which become 16-byte stores (bf16: after
//     one v_permlane32_swap per dword, the T21 idiom of the CDNA guide); the time-mean epilogue writes whole rows of
//     the embedding with no transpose.
//   * average pooling's 1/2 (1/4) is folded into the packed weights and bias (relu(s*x) = s*relu(x), s > 0, exact).
//
// MFMA: bf16 -> v_mfma_f32_32x32x16_bf16 (8 bf16 per lane = one 16-byte chunk);
//       f32  -> v_mfma_f32_32x32x2_f32  (exact fp32 fma chain; one 16-byte chunk feeds 4 MFMAs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>
#include <utility>

#include "dfa_device.h"
#include "launch_views.h"
#include "rng.h"

namespace dfa {

enum { EPI_POOL_H2 = 0, EPI_POOL_2X2 = 1, EPI_MEAN_T = 2, EPI_PLAIN = 3, EPI_RAW = 4 };

struct ConvArgs {
  const void* in;      // [B][H][W][CIN] T
  const uint4* wpack;  // [COUT/32][9][CIN/KG][64] x 16 bytes
  const float* bias;   // [COUT] folded bias
  void* out;           // POOL_H2: [B][H/2][W][COUT]; POOL_2X2: [B][H/2][W/2][COUT]; PLAIN: [B][H][W][COUT]
  float* emb;          // MEAN_T: [B][COUT][W] fp32 (= mean over H)
  int B, H, W, COUT;
  int nstrips;
  float inv_h;
  int relu;            // PLAIN only: apply ReLU (1) or not (0)
  // K-split support (Cin larger than one launch can keep in registers, e.g. fp32 Cin = 128): a launch may read a
  // CIN-channel window of wider pixels, start from previously stored partial sums and/or store raw partial sums.
  int in_pix_bytes;    // bytes between consecutive input pixels (0 = CIN*sizeof(T), i.e. dense)
  int in_ch_off_bytes; // byte offset of this launch's first input channel inside a pixel
  const float* acc_in; // ACCIN: [B][H][W][COUT] fp32 partial sums to start from (they already contain the bias)
  float* raw_out;      // EPI_RAW: [B][H][W][COUT] fp32 partial sums (bias included, no activation)
  // train-mode BatchNorm statistics (EPI_PLAIN only): per-workgroup partial sums of the stored values v and v*v
  // per output channel, partial[(blockIdx.x * COUT + channel) * 2 + {0,1}]; reduced in a fixed order by bn_finalize.
  float* stats_partial;
  const void* zero_page;  // DMA staging: >= 16 zero bytes in device memory (source of out-of-image chunks)
  // time-axis split for small batches (conv3_m16.hip, conv_split.hip): blockIdx.z = segment, a segment walks seg_iters
  // iterations (0 = the whole axis).  The time mean is ALWAYS summed in canonical chunks of chunk_iters iterations (a
  // multiple of 6 that depends on H only), the chunk sums added in chunk order: an unsplit workgroup keeps the running total
  // in LDS, a split one writes every chunk sum (unscaled) to emb + chunk * emb_seg_stride floats and the classifier kernel
  // adds them in the same order -- so logits do not depend on the batch size or on the split, bit for bit.
  int seg_iters, chunk_iters;
  size_t emb_seg_stride;
  // conv_split.hip PLAIN_BF16 (data gradient of block 2): thresh != 0 zeroes the elements the forward's dropout layer dropped
  // (same Philox draw, element index = output index) -- the keep mask of the pooled a1 applied where da1 is produced
  DropCfg drop;
  // held-clock probe (conv3_m16.hip eval form; context option "clock_probe"): when non-null, lane 0 of the first 1024 workgroups
  // (blockIdx.y = z = 0) writes {delta s_memtime (shader cycles), delta s_memrealtime (100 MHz ticks)} around its main loop to
  // clock_stamps[2 * blockIdx.x ..]; never read by any kernel.  Null (the default): two scalar compares per workgroup.
  long long* clock_stamps;
};

// Variable-length batches (dfa_cnn2d_forward_ragged): a device table of 4 * B int32 words, copied from the host with each
// call.  [0, B): length T_b of utterance b; [B, 2B): dispatch order, workgroup slot u -> utterance (longest first);
// [2B, 3B): 1 / H2_b as float bits; [3B, 4B): number of canonical time-mean chunks of block 3.  A ragged kernel reads its
// utterance's words once per workgroup (wave-uniform).  dfa_cae_score_ragged uses the same first 2 * B words; its [2B, 3B)
// hold 1 / (T_b F) as float bits and its [3B, 4B) the utterance's decoder tile count.
struct RaggedTab {
  const int* tab;
  int B;
};

// chunk swizzle as a function of the pixel slot (column) only
template <int PB>
__device__ __forceinline__ int lds_swz(int slot) {
  if (PB == 64) return (slot >> 2) & 3;
  if (PB == 128) return (slot >> 1) & 7;
  return slot & 15;  // 256, 512, 1024
}

// acc += W(A operand: 32 channels x K) . X(B operand: K x 32 pixels)
template <typename T>
struct Mma;
template <>
struct Mma<bf16_t> {
  static __device__ __forceinline__ f32x16_t run(const uint4& w, const uint4& x, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w), __builtin_bit_cast(bf16x8_t, x), c,
                                                   0, 0, 0);
  }
};
template <>
struct Mma<float> {
  static __device__ __forceinline__ f32x16_t run(const uint4& w, const uint4& x, f32x16_t c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.x), __uint_as_float(x.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.y), __uint_as_float(x.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.z), __uint_as_float(x.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.w), __uint_as_float(x.w), c, 0, 0, 0);
    return c;
  }
};

// ---- explicit LDS fragment pipeline.  hipcc schedules "ds_read_b128 -> s_waitcnt lgkmcnt(0) -> MFMA" with ONE fragment
// buffer (every MFMA pair eats the full LDS latency), so the fragment reads are issued through inline asm PFD reads
// ahead of their use and retired with counted waits.  LDS operations complete in order, so "lgkmcnt(N)" guarantees
// everything older than the N youngest reads has landed; reads the compiler adds on its own only make a wait stricter.
template <int OFF, bool PIPE>
__device__ __forceinline__ u32x4_t lds_frag(unsigned addr) {
  u32x4_t v;
  if constexpr (PIPE) {
    constexpr int LO = OFF & 0xFFFF, HI = OFF - LO;   // the DS offset field is 16 bits
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr + HI), "n"(LO));
  } else {   // compiler-scheduled read (it places its own s_waitcnt)
    v = *(const u32x4_t*)((const __attribute__((address_space(3))) char*)(size_t)(addr + OFF));
  }
  return v;
}
template <int N>
__device__ __forceinline__ void lds_wait(u32x4_t& v) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N));
}
template <int N>
__device__ __forceinline__ void lds_wait4(u32x4_t& a, u32x4_t& b, u32x4_t& c, u32x4_t& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
template <int... Is, typename F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}

template <typename T, int CIN, int NSL, int MG, int RP, int EPI>
struct ConvCfg {
  static constexpr int ES = sizeof(T);
  static constexpr int KG = 32 / ES;       // input channels per k-group (two 16-byte chunks)
  static constexpr int NKG = CIN / KG;
  static constexpr int PB = CIN * ES;      // bytes per pixel
  static constexpr int CPP = PB / 16;      // 16-byte chunks per pixel
  static constexpr int SLOTS = 34;         // 32 columns + 2 halo
  static constexpr int SPA = (PB >= 256) ? 1 : 256 / PB;          // row pitch must make SP*PB a multiple of 256 B
  static constexpr int SP = (SLOTS + SPA - 1) / SPA * SPA;
  static constexpr int BR = 2 * RP;        // rows per ring block
  static constexpr int NT = 64 * NSL * MG;
  static constexpr int NCH = BR * SP * CPP;  // physical chunks per ring block
  static constexpr int NLD = (NCH + NT - 1) / NT;
  static constexpr int UPW = RP / MG;      // units per wave per iteration
  static constexpr int ROW_BYTES = SP * PB;
  static constexpr int RING_BYTES = 3 * BR * ROW_BYTES;
  static constexpr int BIAS_BYTES = NSL * 32 * 4;
  static constexpr int STAT_BYTES = (EPI == EPI_PLAIN) ? MG * NSL * 32 * 2 * 4 : 0;
  static constexpr int LDS_BYTES = RING_BYTES + BIAS_BYTES + STAT_BYTES;
  static_assert(RP % MG == 0, "row pairs must split evenly over the M groups");
  static_assert((BR & (BR - 1)) == 0, "rows per block must be a power of two");
  static_assert(EPI != EPI_MEAN_T || MG == 1, "time-mean epilogue keeps column sums per wave: MG must be 1");
  static_assert(CIN % KG == 0, "CIN must be a multiple of the k-group");
};

#ifdef DFA_STAMPS
static __device__ long long g_diag[2048 * 4 * 8];
#endif
#define DFA_KERNEL_BODY_SCOPE   // the two kernels below include conv3x3_body.h
template <typename T, int CIN, int NSL, int MG, int RP, int MT, int EPI, int MINW, bool ACCIN = false, bool DMA = false,
          bool STATS = false, int PFD = -1>
__global__ __launch_bounds__(64 * NSL * MG, MINW) void conv3x3_mfma_kernel(ConvArgs a) {
  constexpr bool RAGGED = false;
  constexpr int hshift = 0;
  const RaggedTab rt{};
#include "conv3x3_body.h"
}

// Ragged form (dfa_cae_score_ragged): the same body; the workgroup's utterance comes from the dispatch order of the table and its
// height at this layer is T_b >> hshift.  A function of its own name, so no uniform instantiation is renamed.
template <typename T, int CIN, int NSL, int MG, int RP, int MT, int EPI, int MINW, bool ACCIN = false, bool DMA = false,
          bool STATS = false, int PFD = -1>
__global__ __launch_bounds__(64 * NSL * MG, MINW) void conv3x3_mfma_ragged_kernel(ConvArgs a, RaggedTab rt, int hshift) {
  constexpr bool RAGGED = true;
#include "conv3x3_body.h"
}
#undef DFA_KERNEL_BODY_SCOPE

// host-side launcher
template <typename T, int CIN, int NSL, int MG, int RP, int MT, int EPI, int MINW, bool ACCIN = false, bool DMA = false,
          bool STATS = false, int PFD = -1>
hipError_t launch_conv3x3(const ConvArgs& a0, hipStream_t stream) {
  using C = ConvCfg<T, CIN, NSL, MG, RP, EPI>;
  ConvArgs a = a0;
  a.nstrips = (a.W + 31) / 32;
  if (STATS && a.relu) return hipErrorInvalidValue;     // the statistics forms store pre-BatchNorm outputs
  auto kern = conv3x3_mfma_kernel<T, CIN, NSL, MG, RP, MT, EPI, MINW, ACCIN, DMA, STATS, PFD>;
  dim3 grid(a.B * a.nstrips, a.COUT / (NSL * 32), 1), block(C::NT, 1, 1);
  const hipError_t e = launch_lds(kern, grid, block, C::LDS_BYTES, stream, a);
#ifdef DFA_STAMPS
  if ((EPI == EPI_MEAN_T || STATS) && sizeof(T) == 2) {
    static int calls = 0;
    if (++calls == 30) {
      static long long hbuf[2048 * 4 * 8];
      hipDeviceSynchronize();
      hipMemcpyFromSymbol(hbuf, HIP_SYMBOL(g_diag), sizeof(hbuf));
      const int nw = (grid.x < 2048 ? grid.x : 2048) * 4;
      double m[8] = {0}; long long tmin = hbuf[6], tmax = hbuf[7];
      for (int i = 0; i < nw; ++i) { for (int k = 0; k < 6; ++k) m[k] += hbuf[i * 8 + k]; m[6] += hbuf[i * 8 + 7] - hbuf[i * 8 + 6];
        if (hbuf[i * 8 + 6] < tmin) tmin = hbuf[i * 8 + 6]; if (hbuf[i * 8 + 7] > tmax) tmax = hbuf[i * 8 + 7]; }
      fprintf(stderr, "[stamps conv3x3<cin %d, epi %d, stats %d>] waves %d  mean cycles/wave: stage_issue %.0f  mfma_loop %.0f  epilogue %.0f  vmcnt_wait %.0f  barrier %.0f  prologue %.0f  lifetime %.0f  kernel span %lld\n",
              CIN, EPI, (int)STATS, nw, m[0] / nw, m[1] / nw, m[2] / nw, m[3] / nw, m[4] / nw, m[5] / nw, m[6] / nw, tmax - tmin);
    }
  }
#endif
  return e;
}

// ragged batch: a.H = the height of the longest utterance at this layer (row pitch of a.in and a.out), hshift = log2 of
// T / a.H (1, 2, 3 for the auto-encoder's encoder blocks 2, 3, 4); rt = the device table
template <typename T, int CIN, int NSL, int MG, int RP, int MT, int EPI, int MINW, bool ACCIN = false, bool DMA = false,
          bool STATS = false, int PFD = -1>
hipError_t launch_conv3x3_ragged(const ConvArgs& a0, const RaggedTab& rt, int hshift, hipStream_t stream) {
  using C = ConvCfg<T, CIN, NSL, MG, RP, EPI>;
  ConvArgs a = a0;
  a.nstrips = (a.W + 31) / 32;
  auto kern = conv3x3_mfma_ragged_kernel<T, CIN, NSL, MG, RP, MT, EPI, MINW, ACCIN, DMA, STATS, PFD>;
  dim3 grid(a.B * a.nstrips, a.COUT / (NSL * 32), 1), block(C::NT, 1, 1);
  return launch_lds(kern, grid, block, C::LDS_BYTES, stream, a, rt, hshift);
}

}  // namespace dfa

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
#include "dfa_internal.h"

#ifndef DFA_C123_PRIO
#define DFA_C123_PRIO 0   // s_setprio 1 on one role: 0 = neither, 1 = consumers, 2 = producers
#endif

namespace dfa {

typedef __attribute__((ext_vector_type(4))) float f32x4_t;

struct Conv123Args {
  const void* x;            // features (bf16 or fp32: template argument TX), element strides below (any layout)
  long long sxb, sxt, sxf;
  const uint4* c1pack;      // [4][64] block-1 A operands (pack_conv1_mfma_kernel)
  const float* c1bias;      // [32]  0.5 * folded bias
  const uint4* wpack2;      // block 2 image [2][9][2][64] (pool factor folded)
  const float* bias2;       // [64]
  const uint4* wpack3;      // block 3 image in the 16x16x32 order [4][9][2][2][64]
  const float* bias3;       // [128]
  float* emb;               // [B][128][F] fp32 time mean
  float inv_h;
  int B, T, F, H1, H2, nstrips;
  int chunk_iters;          // canonical chunks of the time mean (conv3_m16.hip)
  long long* clock_stamps;  // held-clock probe (ConvArgs::clock_stamps), null = off
};

namespace c123 {
// consumer region (LDS offset 0): a2 ring 4 blocks x 2 rows x 32 slots x 128 B, block-3 bias, running time-mean totals
constexpr int CPB = 128, CSP = 32, CROWB = CSP * CPB, CBR = 2, CNB = 4, NT = 256;
constexpr int CRING_BYTES = CNB * CBR * CROWB;
constexpr int CBIAS_OFF = CRING_BYTES, TOT_OFF = CBIAS_OFF + 128 * 4, TOT_BYTES = NT * 64;
// producer region: a1 ring 3 blocks x 4 rows x 36 slots x 64 B, block-2 bias, 2 feature-window buffers, store sink
constexpr int P_OFF = TOT_OFF + TOT_BYTES;
constexpr int PB = 64, SP = 36, ROWB = SP * PB, BR = 4, NKG = 2, PF = 4, SW = 30;
constexpr int RING_BYTES = 3 * BR * ROWB;
constexpr int BIAS2_OFF = RING_BYTES, XW_OFF = BIAS2_OFF + 64 * 4;
constexpr int XROWS = 10, XW_ROWB = SP * 8, XW_BYTES = XROWS * XW_ROWB;
constexpr int DUMMY_OFF = XW_OFF + 2 * XW_BYTES;
constexpr int P_BYTES = DUMMY_OFF + 16;
constexpr int LDS_BYTES = P_OFF + P_BYTES;
constexpr int XCOLS = 36;                 // feature columns per ring block: f0-3 .. f0+32
constexpr int NSLOT = 34;                 // live a1 slots: f0-2 .. f0+31
constexpr int NX = XROWS * XCOLS;
constexpr int NXLD = (NX + 255) / 256;
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
static_assert(P_OFF + RING_BYTES < 65536 + P_OFF, "");
}  // namespace c123

__device__ __forceinline__ float ld_as_float123(const float* p) { return *p; }
__device__ __forceinline__ float ld_as_float123(const bf16_t* p) { return bf16_to_float(*p); }
__device__ __forceinline__ f32x4_t mma16_123(const uint4& w, const uint4& x, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w), __builtin_bit_cast(bf16x8_t, x), c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------- producers
// conv12_fused_kernel's main loop (same pipeline, same consume-step schedule), 256 threads, columns shifted by one, plus
// the second block-1 tile and the a2 hand-off.  Barrier count: niter3 (one per unit) + 4 (prologue) + 2 (idle steps).
template <typename TX, bool PIPE>
__device__ __forceinline__ void c123_producer(const Conv123Args& a, char* smem, unsigned lds0, int tid, int wave, int b, int f0,
                                              int niter3) {
  using namespace c123;
  const int lane = tid & 63;
  const int nsl = wave & 1, mg = wave >> 1;
  const int r = lane & 31, h = lane >> 5;
  const int H = a.H1, W = a.F, T = a.T;
  const unsigned plds = lds0 + P_OFF;
  char* const psm = smem + P_OFF;
  const float rlim = relu_limit();
  if (DFA_C123_PRIO == 2) __builtin_amdgcn_s_setprio(1);

  uint4 w[9][NKG];
  {
    const uint4* wp = a.wpack2 + (size_t)nsl * 9 * NKG * 64 + lane;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kg = 0; kg < NKG; ++kg) w[tap][kg] = wp[(tap * NKG + kg) * 64];
  }
  uint4 c1w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) c1w[k] = a.c1pack[k * 64 + lane];

  float* bias2_lds = (float*)(psm + BIAS2_OFF);
  if (tid < 64) bias2_lds[tid] = a.bias2[tid];
  for (int i = tid; i < 2 * XW_BYTES / 8; i += 256) *(uint2*)(psm + XW_OFF + i * 8) = make_uint2(0u, 0u);
  f32x16_t bias1;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 bv = *(const float4*)(a.c1bias + 8 * g + 4 * h);
    bias1[4 * g] = bv.x; bias1[4 * g + 1] = bv.y; bias1[4 * g + 2] = bv.z; bias1[4 * g + 3] = bv.w;
  }

  int xa[3];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int slot = r + dx, s = lds_swz<PB>(slot);
    xa[dx] = slot * PB + (((h ^ (s & 1)) << 4) | ((s >> 1) << 5));
  }

  // ---- feature staging: element e of a ring block = (local row, column c); x column f0 - 3 + c, x row 8j - 3 + row
  const bool t_fast = (a.sxt == 1);
  int xrow[NXLD], xcol[NXLD];
#pragma unroll
  for (int k = 0; k < NXLD; ++k) {
    const int e = k * 256 + tid;
    xrow[k] = t_fast ? e % XROWS : e / XCOLS;
    xcol[k] = t_fast ? e / XROWS : e % XCOLS;
  }
  const TX* xb = (const TX*)a.x + (long long)b * a.sxb;
  unsigned short xreg[NXLD];
  bool xok[NXLD];
  long long xoff[NXLD];
  bool xfok[NXLD];
#pragma unroll
  for (int k = 0; k < NXLD; ++k) {
    const int f = f0 - 3 + xcol[k];
    xfok[k] = (k * 256 + tid < NX) && f >= 0 && f < W;
    xoff[k] = (long long)(xrow[k] - 3) * a.sxt + (long long)(xfok[k] ? f : 0) * a.sxf;
  }
  auto x_load = [&](int j) {
    const long long jo = (long long)(8 * j) * a.sxt;
#pragma unroll
    for (int k = 0; k < NXLD; ++k) {
      const int t = 8 * j - 3 + xrow[k];
      xok[k] = xfok[k] && (unsigned)t < (unsigned)T;
      const TX* src = xb + (xok[k] ? xoff[k] + jo : 0);
      if constexpr (sizeof(TX) == 2) xreg[k] = *(const unsigned short*)src;
      else xreg[k] = cvt_out<bf16_t>(ld_as_float123(src)).v;
    }
  };
  auto x_store = [&](int buf) {   // element (row, c) is tap e of the windows of slots c - e, e = 0..2
#pragma unroll
    for (int k = 0; k < NXLD; ++k) {
      const int base = XW_OFF + buf * XW_BYTES + xrow[k] * XW_ROWB;
      const unsigned short v = xok[k] ? xreg[k] : (unsigned short)0;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int s = xcol[k] - e;
        const bool ok = (k * 256 + tid < NX) && s >= 0 && s < NSLOT;
        const int off = ok ? base + s * 8 + e * 2 : DUMMY_OFF;
        if constexpr (PIPE) {
          asm volatile("ds_write_b16 %0, %1" : : "v"(plds + off), "v"((unsigned)v) : "memory");
        } else {
          *(unsigned short*)(psm + off) = v;
        }
      }
    }
  };

  // ---- block 1: a1 row m = wave of ring block j; tile 0 = slots 0..31, tile 1 = slots 32, 33 (lanes r = 0, 1)
  const int c1_m = wave;
  const unsigned c1_win0 = plds + XW_OFF + ((2 * c1_m + 2 * h) * SP + r) * 8;
  const unsigned c1_win1 = plds + XW_OFF + ((2 * c1_m + 2 * h) * SP + 32 + (r & 1)) * 8;
  const int c1_f0 = f0 - 2 + r, c1_f1 = f0 + 30 + (r & 1);
  const bool c1_fok0 = c1_f0 >= 0 && c1_f0 < W, c1_fok1 = c1_f1 < W;
  const int c1_dst0 = (c1_m * SP + r) * PB, c1_dst1 = (c1_m * SP + 32 + (r & 1)) * PB;
  const int c1_sw0 = lds_swz<PB>(r), c1_sw1 = lds_swz<PB>(32 + (r & 1));
  const bool c1_live1 = r < 2;
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  struct C1State { u32x2_t w0, w1, w2, w3; f32x16_t e, o; float v[16]; };
  auto c1_issue = [&](C1State& st, int j) {       // four window reads (asm: they join the counted LDS pipeline)
    const unsigned a0 = c1_win0 + (j & 1) * XW_BYTES, a1 = c1_win1 + (j & 1) * XW_BYTES;
    if constexpr (PIPE) {
      asm volatile("ds_read_b64 %0, %1" : "=v"(st.w0) : "v"(a0));
      asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(st.w1) : "v"(a0), "n"(XW_ROWB));
      asm volatile("ds_read_b64 %0, %1" : "=v"(st.w2) : "v"(a1));
      asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(st.w3) : "v"(a1), "n"(XW_ROWB));
    } else {
      st.w0 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)a0);
      st.w1 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)(a0 + XW_ROWB));
      st.w2 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)a1);
      st.w3 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)(a1 + XW_ROWB));
    }
  };
  auto c1_mfma = [&](C1State& st, auto t_c) {
    constexpr int TL = decltype(t_c)::value;
    if constexpr (PIPE) asm volatile("" : "+v"(st.w0), "+v"(st.w1), "+v"(st.w2), "+v"(st.w3));
    const uint4 xv = TL == 0 ? make_uint4(st.w0[0], st.w0[1], st.w1[0], st.w1[1]) : make_uint4(st.w2[0], st.w2[1], st.w3[0], st.w3[1]);
    st.e = Mma<bf16_t>::run(c1w[0], xv, bias1);
    st.o = Mma<bf16_t>::run(c1w[2], xv, bias1);
    st.e = Mma<bf16_t>::run(c1w[1], xv, st.e);
    st.o = Mma<bf16_t>::run(c1w[3], xv, st.o);
  };
  auto c1_relu = [&](C1State& st, int j, auto t_c) {
    constexpr int TL = decltype(t_c)::value;
    const int q = BR * j - 1 + c1_m;
    const float lim = (q >= 0 && q < H && (TL == 0 ? c1_fok0 : c1_fok1)) ? __builtin_inff() : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      st.v[i] = __builtin_amdgcn_fmed3f(st.e[i], 0.f, lim) + __builtin_amdgcn_fmed3f(st.o[i], 0.f, lim);
  };
  auto c1_store = [&](C1State& st, int ringblk, auto t_c) {
    constexpr int TL = decltype(t_c)::value;
    const int dst = ringblk * (BR * ROWB) + (TL == 0 ? c1_dst0 : c1_dst1);
    const int sw = TL == 0 ? c1_sw0 : c1_sw1;
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const unsigned a0 = pack_bf16x2(st.v[4 * g], st.v[4 * g + 1]), a1 = pack_bf16x2(st.v[4 * g + 2], st.v[4 * g + 3]);
      const unsigned b0 = pack_bf16x2(st.v[4 * g + 4], st.v[4 * g + 5]), b1 = pack_bf16x2(st.v[4 * g + 6], st.v[4 * g + 7]);
      const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      const unsigned addr = plds + dst + (((g + h) ^ sw) << 4);
      const u32x4_t pk = {s0[0], s1[0], s0[1], s1[1]};
      if (TL == 0 || c1_live1) {   // tile 1: lanes 0, 1, 32, 33 (never an empty exec mask: the store always issues)
        if constexpr (PIPE) asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(pk) : "memory");
        else *(u32x4_t*)((__attribute__((address_space(3))) char*)(size_t)addr) = pk;
      }
    }
  };
  auto produce_now = [&](int j, int ringblk) {
    C1State st;
    c1_issue(st, j);
    if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(st.w0), "+v"(st.w1), "+v"(st.w2), "+v"(st.w3));
    c1_mfma(st, std::integral_constant<int, 0>{});
    c1_relu(st, j, std::integral_constant<int, 0>{});
    c1_store(st, ringblk, std::integral_constant<int, 0>{});
    c1_mfma(st, std::integral_constant<int, 1>{});
    c1_relu(st, j, std::integral_constant<int, 1>{});
    c1_store(st, ringblk, std::integral_constant<int, 1>{});
  };

  // a2 hand-off: pixel r = column f0 - 1 + r = consumer ring slot r; lanes own channels 32 nsl + 8h + 16g .. + 7 after the swap
  const int col = f0 - 1 + r;
  const bool col_ok = col >= 0 && col < W;
  const int a2_dst = r * CPB;
  const int a2_sw = r & 6;
  auto lds_drain = [&]() { if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
  auto barrier = [&]() { lds_drain(); __syncthreads(); };

  barrier();                 // window pads / biases / consumer ring row -1 written
  x_load(0); x_store(0);
  x_load(1); x_store(1);
  barrier();
  produce_now(0, 0);
  produce_now(1, 1);
  barrier();
  x_load(2); x_store(0);
  barrier();

  auto unit = [&](auto ph_c, auto rp_c, int it) {
    constexpr int PH = decltype(ph_c)::value, RPI = decltype(rp_c)::value;
    f32x16_t acc0, acc1;
    constexpr int NR = 12 * NKG;
    constexpr int S_RELU0 = 9 * NKG + 2;
    constexpr int S_BAR = 4;
    // consume steps of the block-1 pieces (tile 0, then tile 1 in the same registers) and of the window stores
    constexpr int C_MFMA = 5, C_XLOAD = 7, C_RELU = 10, C_MFMA1 = 11, C_STORE = 13, C_RELU1 = 17, C_XSTORE = 19, C_STORE1 = 21;
    constexpr int NWR = 4;   // window reads issued behind fragment read S_BAR
    u32x4_t xbuf[PF];
    C1State c1;
    auto step = [&](auto s_c) {
      constexpr int s = decltype(s_c)::value;
      if constexpr (s < NR) {
        constexpr int i = s / (3 * NKG), dx = (s / NKG) % 3, kg = s % NKG;
        constexpr int ringrow = (BR * PH + 2 * RPI + i) % (3 * BR);
        xbuf[s % PF] = lds_frag<ringrow * ROWB, PIPE>(plds + (xa[dx] ^ (kg << 5)));
        if constexpr (s == S_BAR) {
          if constexpr (PIPE) asm volatile("s_barrier" ::: "memory");
          else __syncthreads();
          c1_issue(c1, it + 2);
        }
      }
      if constexpr (s >= PF - 1) {
        constexpr int c = s - (PF - 1);
        constexpr int i = c / (3 * NKG), dx = (c / NKG) % 3, kg = c % NKG;
        // outstanding LDS operations younger than read c (in order): younger reads, ring stores behind C_STORE / C_STORE1,
        // window stores behind C_XSTORE, window reads behind S_BAR
        constexpr int young_r = (NR - 1 - c) < (PF - 1) ? (NR - 1 - c) : (PF - 1);
        constexpr int young = young_r + ((c > C_STORE && c <= C_STORE + PF - 1 && c < NR) ? 2 : 0) +
                              ((c > C_STORE1 && c <= C_STORE1 + PF - 1 && c < NR) ? 2 : 0) +
                              ((c > C_XSTORE && c <= C_XSTORE + PF - 1 && c < NR) ? 3 * NXLD : 0) +
                              ((c > S_BAR - PF && c <= S_BAR) ? NWR : 0);
        if constexpr (PIPE) lds_wait<young>(xbuf[c % PF]);
        const uint4 xv = __builtin_bit_cast(uint4, xbuf[c % PF]);
        if constexpr (i <= 2) acc0 = Mma<bf16_t>::run(w[i * 3 + dx][kg], xv, acc0);
        if constexpr (i >= 1) acc1 = Mma<bf16_t>::run(w[(i - 1) * 3 + dx][kg], xv, acc1);
        if constexpr (c == C_MFMA) c1_mfma(c1, std::integral_constant<int, 0>{});
        if constexpr (c == C_XLOAD) x_load(it + 3);
        if constexpr (c == C_RELU) c1_relu(c1, it + 2, std::integral_constant<int, 0>{});
        if constexpr (c == C_MFMA1) c1_mfma(c1, std::integral_constant<int, 1>{});
        if constexpr (c == C_STORE) c1_store(c1, (PH + 2) % 3, std::integral_constant<int, 0>{});
        if constexpr (c == C_RELU1) c1_relu(c1, it + 2, std::integral_constant<int, 1>{});
        if constexpr (c == C_XSTORE) x_store((it + 3) & 1);
        if constexpr (c == C_STORE1) c1_store(c1, (PH + 2) % 3, std::integral_constant<int, 1>{});
        if constexpr (c == S_RELU0) {
#pragma unroll
          for (int e = 0; e < 16; ++e) acc0[e] = relu1(acc0[e], rlim);
        }
      }
    };
    {
      const unsigned ba = plds + BIAS2_OFF + (nsl * 32 + 4 * h) * 4;
      u32x4_t b0 = lds_frag<0, PIPE>(ba), b1 = lds_frag<32, PIPE>(ba), b2 = lds_frag<64, PIPE>(ba), b3 = lds_frag<96, PIPE>(ba);
      static_for(std::make_integer_sequence<int, PF - 1>{}, step);
      if constexpr (PIPE) lds_wait4<PF - 1>(b0, b1, b2, b3);
      const u32x4_t bq[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc0[4 * g + e] = acc1[4 * g + e] = __uint_as_float(bq[g][e]);
    }
    static_for(std::make_integer_sequence<int, NR>{}, [&](auto s_c) {
      step(std::integral_constant<int, decltype(s_c)::value + PF - 1>{});
    });
    // AvgPool2d((2,1)) over the row pair (the 1/2 is in the weights) -> a2 row 2 it + RPI, straight into the consumer ring
    const int to = 2 * it + RPI;
    const bool ok = col_ok && to < a.H2;
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = acc0[i] + relu1(acc1[i], rlim);
    // a2 row 2p -> block p, row 1;  row 2p + 1 -> block p + 1, row 0
    const unsigned dst = lds0 + ((it + RPI) & (CNB - 1)) * (CBR * CROWB) + (1 - RPI) * CROWB + a2_dst;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      unsigned pq0 = pack_bf16x2(v[8 * g], v[8 * g + 1]), pq1 = pack_bf16x2(v[8 * g + 2], v[8 * g + 3]);
      unsigned pq2 = pack_bf16x2(v[8 * g + 4], v[8 * g + 5]), pq3 = pack_bf16x2(v[8 * g + 6], v[8 * g + 7]);
      pq0 = ok ? pq0 : 0u; pq1 = ok ? pq1 : 0u; pq2 = ok ? pq2 : 0u; pq3 = ok ? pq3 : 0u;
      const auto s0 = __builtin_amdgcn_permlane32_swap(pq0, pq2, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(pq1, pq3, false, false);
      const int chunk = 4 * nsl + h + 2 * g;
      const unsigned addr = dst + ((chunk ^ a2_sw) << 4);
      if constexpr (PIPE) {
        const u32x4_t pk = {s0[0], s1[0], s0[1], s1[1]};
        asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(pk) : "memory");
      } else {
        *(uint4*)((__attribute__((address_space(3))) char*)(size_t)addr) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
      }
    }
  };
  auto iteration = [&](auto ph_c, int it) {
    if (mg == 0) unit(ph_c, std::integral_constant<int, 0>{}, it);
    else unit(ph_c, std::integral_constant<int, 1>{}, it);
  };
  for (int it = 0; it < niter3; it += 3) {
    iteration(std::integral_constant<int, 0>{}, it);
    if (it + 1 < niter3) iteration(std::integral_constant<int, 1>{}, it + 1);
    if (it + 2 < niter3) iteration(std::integral_constant<int, 2>{}, it + 2);
  }
  // idle step niter3: a2 row 2 niter3 (>= H2: zero padding of the consumers' last iteration) = block niter3, row 1
  {
    char* zr = smem + (niter3 & (CNB - 1)) * (CBR * CROWB) + CROWB;
    *(uint4*)(zr + tid * 16) = make_uint4(0u, 0u, 0u, 0u);
  }
  barrier();
  barrier();                 // idle step niter3 + 1
}

// ---------------------------------------------------------------------------------------------------------- consumers
// conv3_m16_meant_kernel's eval unit on the 4-block ring the producers fill.  Barrier count: 4 (prologue) + 2 (idle steps)
// + niter3 (one per unit).
template <bool PIPE>
__device__ __forceinline__ void c123_consumer(const Conv123Args& a, char* smem, unsigned lds0, int ctid, int nsl, int b, int f0,
                                              int niter) {
  using namespace c123;
  constexpr int PF3 = 4;
  const int lane = ctid & 63;
  const int p = lane & 15, q = lane >> 4;
  const int H = a.H2, W = a.F, COUT = 128;
  const float rlim = relu_limit();
  if (DFA_C123_PRIO == 1) __builtin_amdgcn_s_setprio(1);

  uint4 w[9][2][2];
  {
    const uint4* wp = a.wpack3 + (size_t)nsl * 9 * 2 * 2 * 64 + lane;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int ca = 0; ca < 2; ++ca) w[tap][kk][ca] = wp[((tap * 2 + kk) * 2 + ca) * 64];
  }
  float* bias_lds = (float*)(smem + CBIAS_OFF);
  if (ctid < 128) bias_lds[ctid] = a.bias3[ctid];
  *(uint4*)(smem + ctid * 16) = make_uint4(0u, 0u, 0u, 0u);    // ring block 0, row 0 = a2 row -1 (zero padding)

  int xa[3];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int slot = p + dx;
    xa[dx] = slot * CPB + ((q ^ (slot & 6)) << 4);
  }

  f32x4_t cs[2][2];
#pragma unroll
  for (int ca = 0; ca < 2; ++ca)
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) cs[ca][pb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  f32x4_t* const tot = (f32x4_t*)(smem + TOT_OFF) + ctid;
#pragma unroll
  for (int k = 0; k < 4; ++k) tot[k * NT] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto unit = [&](auto ph_c, int it) {
    constexpr int PH = decltype(ph_c)::value;
    const int t0 = CBR * it;
    f32x4_t acc0[2][2], acc1[2][2];
    constexpr int NR = 4 * 3 * 2 * 2;
    constexpr int C_RELU0 = 36 + 3;
    constexpr int S_BAR = 4;
    u32x4_t xbuf[PF3];
    auto step = [&](auto s_c) {
      constexpr int s = decltype(s_c)::value;
      if constexpr (s < NR) {
        constexpr int i = s / 12, dx = (s / 4) % 3, kk = (s / 2) % 2, pb = s % 2;
        constexpr int ringrow = (CBR * PH + i) % (CNB * CBR);
        xbuf[s % PF3] = lds_frag<ringrow * CROWB + pb * 16 * CPB, PIPE>(lds0 + (xa[dx] ^ (kk << 6)));
        if constexpr (s == S_BAR) {
          // behind it: the rows of block it+1 (second half of the stream), written by the producers in the previous step
          if constexpr (PIPE) asm volatile("s_barrier" ::: "memory");
          else __syncthreads();
        }
      }
      if constexpr (s >= PF3 - 1) {
        constexpr int c = s - (PF3 - 1);
        constexpr int i = c / 12, dx = (c / 4) % 3, kk = (c / 2) % 2, pb = c % 2;
        constexpr int young = (NR - 1 - c) < (PF3 - 1) ? (NR - 1 - c) : (PF3 - 1);
        if constexpr (PIPE) lds_wait<young>(xbuf[c % PF3]);
        const uint4 xv = __builtin_bit_cast(uint4, xbuf[c % PF3]);
#pragma unroll
        for (int ca = 0; ca < 2; ++ca) {
          if constexpr (i <= 2) acc0[ca][pb] = mma16_123(w[i * 3 + dx][kk][ca], xv, acc0[ca][pb]);
          if constexpr (i >= 1) acc1[ca][pb] = mma16_123(w[(i - 1) * 3 + dx][kk][ca], xv, acc1[ca][pb]);
        }
        if constexpr (c == C_RELU0) {
#pragma unroll
          for (int ca = 0; ca < 2; ++ca)
#pragma unroll
            for (int pb2 = 0; pb2 < 2; ++pb2)
#pragma unroll
              for (int e = 0; e < 4; ++e) acc0[ca][pb2][e] = relu1(acc0[ca][pb2][e], rlim);
        }
      }
    };
    {
      const unsigned ba = lds0 + CBIAS_OFF + (nsl * 32 + 4 * q) * 4;
      u32x4_t b0 = lds_frag<0, PIPE>(ba), b1 = lds_frag<64, PIPE>(ba);
      static_for(std::make_integer_sequence<int, PF3 - 1>{}, step);
      if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(b0), "+v"(b1) : "n"(PF3 - 1));
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        acc0[0][pb] = acc1[0][pb] = __builtin_bit_cast(f32x4_t, b0);
        acc0[1][pb] = acc1[1][pb] = __builtin_bit_cast(f32x4_t, b1);
      }
    }
    static_for(std::make_integer_sequence<int, NR>{}, [&](auto s_c) {
      step(std::integral_constant<int, decltype(s_c)::value + PF3 - 1>{});
    });
    if (t0 + 1 < H) {   // wave-uniform
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int e = 0; e < 4; ++e) cs[ca][pb][e] += acc0[ca][pb][e] + relu1(acc1[ca][pb][e], rlim);
    } else if (t0 < H) {
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int e = 0; e < 4; ++e) cs[ca][pb][e] += acc0[ca][pb][e];
    }
  };

  auto barrier = [&]() { if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __syncthreads(); };
  barrier(); barrier(); barrier(); barrier();   // the producers' prologue
  barrier(); barrier();                         // idle steps 0, 1

  // canonical chunks of the time mean (conv3_m16.hip): a chunk's sum is added to the total after its last iteration
  const int chunk = a.chunk_iters > 0 ? a.chunk_iters : niter + 3;
  int next_flush = min(niter, chunk);
  long long st_c = 0, st_r = 0;
  const bool probe = a.clock_stamps != nullptr;
  if (probe) {
    st_c = __builtin_amdgcn_s_memtime();
    st_r = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xc07f);
  }
  auto citer = [&](auto ph_c, int it) {
    unit(ph_c, it);
    if (it + 1 == next_flush) {   // wave-uniform, outside the MFMA stream
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
          tot[(ca * 2 + pb) * NT] += cs[ca][pb];
          cs[ca][pb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
      next_flush = min(niter, next_flush + chunk);
    }
  };
  for (int it = 0; it < niter; it += 4) {
    citer(std::integral_constant<int, 0>{}, it);
    if (it + 1 < niter) citer(std::integral_constant<int, 1>{}, it + 1);
    if (it + 2 < niter) citer(std::integral_constant<int, 2>{}, it + 2);
    if (it + 3 < niter) citer(std::integral_constant<int, 3>{}, it + 3);
  }
  const int bid = blockIdx.x;
  if (probe && ctid == 0 && bid < 1024) {
    a.clock_stamps[2 * bid] = __builtin_amdgcn_s_memtime() - st_c;
    a.clock_stamps[2 * bid + 1] = __builtin_amdgcn_s_memrealtime() - st_r;
  }
#pragma unroll
  for (int ca = 0; ca < 2; ++ca)
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const int col = f0 + 16 * pb + p;
      const f32x4_t tv = tot[(ca * 2 + pb) * NT];
      if (16 * pb + p < SW && col < W) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = nsl * 32 + 16 * ca + 4 * q + e;
          a.emb[((size_t)b * COUT + c) * W + col] = tv[e] * a.inv_h;
        }
      }
    }
}

// PIPE = false is the compiler-scheduled twin (plain LDS loads and stores, same arithmetic): bit-identical output
template <typename TX, bool PIPE>
__global__ __launch_bounds__(512, 1) void conv123_fused_kernel(Conv123Args a) {
  using namespace c123;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = bid & 7, xi = bid >> 3;
  const int logical = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + xi;
  const int b = logical / a.nstrips, strip = logical - b * a.nstrips;
  const int f0 = strip * SW;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int niter3 = (a.H2 + 1) / 2;
  // roles by wave number (not parity): waves 0-3 and 4-7 land one of each on every SIMD
  if (wave < 4) c123_producer<TX, PIPE>(a, smem, lds0, tid, wave, b, f0, niter3);
  else c123_consumer<PIPE>(a, smem, lds0, tid - 256, wave - 4, b, f0, niter3);
}

template <typename TX, bool PIPE>
static hipError_t launch_conv123_t(const Conv123Args& a, hipStream_t s) {
  auto kern = conv123_fused_kernel<TX, PIPE>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, c123::LDS_BYTES);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3(a.B * a.nstrips), dim3(512), c123::LDS_BYTES, s, a);
  return hipGetLastError();
}

hipError_t launch_conv123_fused(const void* x, int x_dtype, int64_t sb, int64_t st, int64_t sf, const uint4* c1pack,
                                const float* c1bias, const uint4* wpack2, const float* bias2, const uint4* wpack3,
                                const float* bias3, float* emb, int B, int T, int F, int chunk_iters, long long* clock_stamps,
                                hipStream_t s, int pipe) {
  Conv123Args a{};
  a.x = x; a.sxb = sb; a.sxt = st; a.sxf = sf;
  a.c1pack = c1pack; a.c1bias = c1bias; a.wpack2 = wpack2; a.bias2 = bias2; a.wpack3 = wpack3; a.bias3 = bias3; a.emb = emb;
  a.B = B; a.T = T; a.F = F; a.H1 = T / 2; a.H2 = a.H1 / 2; a.nstrips = (F + c123::SW - 1) / c123::SW;
  a.inv_h = 1.0f / (float)a.H2;
  a.chunk_iters = chunk_iters;
  a.clock_stamps = clock_stamps;
  if (x_dtype == DFA_DTYPE_BF16) return pipe ? launch_conv123_t<bf16_t, true>(a, s) : launch_conv123_t<bf16_t, false>(a, s);
  return pipe ? launch_conv123_t<float, true>(a, s) : launch_conv123_t<float, false>(a, s);
}

}  // namespace dfa

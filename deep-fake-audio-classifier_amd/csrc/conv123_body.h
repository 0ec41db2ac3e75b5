// conv123_body.h -- the producer and consumer units of the CNN2D blocks 1-3 kernels, one text for four kernels:
//   conv123_fused.hip    one workgroup per (utterance, 30-column strip) unit            (PERSIST = false)
//   conv123_persist.hip  one workgroup per CU walking a contiguous range of units        (PERSIST = true)
//   conv123_carry.hip    the persistent form, two a1 columns carried from strip to strip (PERSIST = true, CARRY = true)
//   conv123_phase.hip    the carry form, consumers' step barrier behind read 35, consumers at s_setprio 1 (DFA_C123_CBAR / _PRIO)
//   conv123_cls.hip      the phase form, classifier head at the end of the workgroup (DFA_C123_CLS; build option
//                        DFA_C123_LATE_EMIT: time mean stored under the next unit's step 0)
// The roles, the column bookkeeping and the per-step schedule are described at the top of conv123_fused.hip; the unit
// boundary of the persistent form at the top of conv123_persist.hip, the carried columns at the top of conv123_carry.hip.
// With PERSIST = false every `if constexpr (PERSIST)` below drops out and the functions are the per-unit kernel's bodies;
// with CARRY = false every `CARRY` term is a constant and the producers are those of the two older kernels.
#ifndef DFA_CONV123_BODY_SCOPE
#error "conv123_body.h holds kernel bodies: include it only from the conv123_*.hip kernel files"
#endif
#ifndef DFA_CONV123_BODY_H
#define DFA_CONV123_BODY_H
#include "dfa_internal.h"
#ifdef DFA_STAMPS
#include <algorithm>
#include <climits>
#include <cstdio>
#include <vector>
#endif

#ifndef DFA_C123_PRIO
#define DFA_C123_PRIO 0   // s_setprio 1 on one role: 0 = neither, 1 = consumers, 2 = producers
#endif
// The fragment-read index behind which the CONSUMERS' step barrier stands (the producers' stays behind their read 4).  Consumer
// iteration `it` holds barrier #(it + 2) of its unit.  Its reads 0 .. 35 are ring block it and row 0 of block it + 1 = a2 rows
// 2 it - 1 .. 2 it + 1, which the producers wrote before #(it + 1): legal on either side of #(it + 2).  Reads 36 .. 47 are row
// 1 of block it + 1 = a2 row 2 it + 2, written in [#(it + 1), #(it + 2)): they must stay behind the barrier.  Hence <= 35
// (tests/test_phase123_cpu.py walks every value).
#ifndef DFA_C123_CBAR
#define DFA_C123_CBAR 4
#endif
// CARRY, set by conv123_carry.hip and conv123_phase.hip alone.  A macro behind the constant: what only the carry form needs (lane constants, lambdas)
// is not declared at all in the two older kernels, whose instruction streams an unused lambda already disturbs.
#ifndef DFA_C123_CARRY
#define DFA_C123_CARRY 0
#endif
// Set by conv123_cls.hip alone (PERSIST consumers; the argument for both stands at the top of that file).
// LATE_EMIT: the time-mean stores of a unit follow the first idle barrier of the next unit instead of preceding it, so that
// the producers' step 0 does not wait for them.  EMIT_PRIO0: those stores run at s_setprio 0 (a measured variant).
// CLS (CARRY only: a workgroup owns whole utterances): after its last unit the workgroup's consumer waves compute the
// classifier head of its utterances from the emb rows they have just stored, as linear1_kernel (linear.hip) would.
#ifndef DFA_C123_LATE_EMIT
#define DFA_C123_LATE_EMIT 0
#endif
#ifndef DFA_C123_EMIT_PRIO0
#define DFA_C123_EMIT_PRIO0 0
#endif
#ifndef DFA_C123_CLS
#define DFA_C123_CLS 0
#endif
#if DFA_C123_CLS && !DFA_C123_CARRY
#error "DFA_C123_CLS needs the carry form: a workgroup's range must be whole utterances"
#endif

namespace dfa {

namespace c123 {
// consumer region (LDS offset 0): a2 ring 4 blocks x 2 rows x 32 slots x 128 B, block-3 bias, running time-mean totals
constexpr int CPB = 128, CSP = 32, CROWB = CSP * CPB, CBR = 2, CNB = 4, NT = 256;
constexpr int CRING_BYTES = CNB * CBR * CROWB;
constexpr int CBIAS_OFF = CRING_BYTES, TOT_OFF = CBIAS_OFF + 128 * 4, TOT_BYTES = NT * 64;
// producer region: a1 ring 3 blocks x 4 rows x 36 slots x 64 B, block-2 bias, 2 feature-window buffers, store sink
constexpr int P_OFF = TOT_OFF + TOT_BYTES;
constexpr int PB = 64, SP = 36, ROWB = SP * PB, BR = 4, NKG = 2, PF = 4;   // (SW, the strip width: conv123_host.h)
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
// CARRY: the side buffer behind the producer region, one entry (ring slots 0 and 1 of an a1 row, as the ring holds them) per
// a1 row of a unit = BR entries per ring block, ring blocks 0 .. niter3 + 1
constexpr bool CARRY = DFA_C123_CARRY != 0;
constexpr int CS = CARRY ? 2 : 0;          // slot of tile-0 lane 0
constexpr int CY = 2, SIDE_OFF = P_OFF + P_BYTES, SIDE_ROWB = CY * PB, SIDE_BLKB = BR * SIDE_ROWB;
constexpr int side_bytes(int niter3) { return (niter3 + 2) * SIDE_BLKB; }
static_assert(SIDE_OFF % 16 == 0, "");
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
static_assert(P_OFF + RING_BYTES < 65536 + P_OFF, "");
}  // namespace c123

// The persistent kernel's main loops are as tight on registers as the per-unit kernel's (254 of 256), and whatever the code
// between two units computes from loop-invariant lane numbers alone the compiler computes before the loop over units and
// keeps (spills) across the main loop.  So that code takes its lane number, and its zeros, from here: behind an empty asm
// nothing is loop-invariant, and the lane number costs no register that lives across the main loop.
__device__ __forceinline__ int c123_fresh_lane() {
  unsigned m = ~0u;
  asm volatile("" : "+s"(m));
  return (int)__builtin_amdgcn_mbcnt_hi(m, __builtin_amdgcn_mbcnt_lo(m, 0u));
}
template <bool ON>
__device__ __forceinline__ unsigned c123_zero() {        // ON = false: the constant
  unsigned z = 0u;
  if constexpr (ON) asm volatile("" : "+s"(z));
  return z;
}

#ifdef DFA_STAMPS
// Diagnostic build (make stamps; never loaded by the product): per wave, shader cycles (s_memtime) spent in
//   0 prologue (entry, or the end of the previous unit's last working step, -> first working step)
//   1 fill (producers: steps 0, 1; consumers: the two idle barriers)      2 paired steps
//   3 drain (producers: the two idle barriers; consumers: their last two iterations)      4 epilogue (time mean -> emb)
// summed over the units of the workgroup, then: units, lifetime cycles, entry / exit in 100 MHz ticks (s_memrealtime) and
// the CU the wave ran on (HW_ID cu / sh / se bits, XCC_ID), from which the launcher takes the idle gap between two
// workgroups on one CU.  Own buffer; nothing the kernel computes depends on a stamp.
constexpr int C123_STAMP_WGS = 2048, C123_STAMP_WORDS = 12;
static __device__ long long g_diag123[C123_STAMP_WGS * 8 * C123_STAMP_WORDS];
struct C123Stamps {
  long long seg[5] = {0, 0, 0, 0, 0};
  long long t_prev, t_begin, r_begin;
  __device__ __forceinline__ C123Stamps() { t_prev = t_begin = __builtin_amdgcn_s_memtime(); r_begin = __builtin_amdgcn_s_memrealtime(); }
  __device__ __forceinline__ void operator()(int k) { const long long t = __builtin_amdgcn_s_memtime(); seg[k] += t - t_prev; t_prev = t; }
  __device__ __forceinline__ void write(int wave8, int lane, int units) {
    if (lane == 0 && blockIdx.x < C123_STAMP_WGS) {
      long long* dd = g_diag123 + ((size_t)blockIdx.x * 8 + wave8) * C123_STAMP_WORDS;
      for (int k = 0; k < 5; ++k) dd[k] = seg[k];
      dd[5] = units;
      dd[6] = __builtin_amdgcn_s_memtime() - t_begin;
      dd[7] = r_begin;
      dd[8] = __builtin_amdgcn_s_memrealtime();
      const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_ID, XCC_ID
      dd[9] = (long long)(((xcc & 15u) << 16) | (hw & 0xff00u));
    }
  }
};
static void c123_print_stamps(const char* tag, int nwg) {
  static long long hbuf[C123_STAMP_WGS * 8 * C123_STAMP_WORDS];
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(hbuf, HIP_SYMBOL(g_diag123), sizeof(hbuf));
  if (nwg > C123_STAMP_WGS) nwg = C123_STAMP_WGS;
  const char* role[2] = {"producers", "consumers"};
  double units = 0;
  for (int rl = 0; rl < 2; ++rl) {
    double m[7] = {0}, ticks = 0;
    for (int g = 0; g < nwg; ++g)
      for (int w = 4 * rl; w < 4 * rl + 4; ++w) {
        const long long* dd = hbuf + ((size_t)g * 8 + w) * C123_STAMP_WORDS;
        for (int k = 0; k < 7; ++k) m[k] += (double)dd[k];
        ticks += (double)(dd[8] - dd[7]);
      }
    const double nw = 4.0 * nwg;
    units = m[5] / nw;
    fprintf(stderr, "[stamps %s] %s: waves %d units/wave %.2f clock %.3f GHz  mean cycles per wave and UNIT: prologue %.0f  fill %.0f  paired %.0f  "
            "drain %.0f  epilogue %.0f  | lifetime per wave %.0f\n", tag, role[rl], (int)nw, units, m[6] / (ticks * 10.0),
            m[0] / m[5], m[1] / m[5], m[2] / m[5], m[3] / m[5], m[4] / m[5], m[6] / nw);
  }
  // idle gap on a CU between the exit of one workgroup (last wave) and the entry of the next (first wave)
  struct Wg { long long key, in, out; };
  std::vector<Wg> v;
  for (int g = 0; g < nwg; ++g) {
    Wg x{hbuf[(size_t)g * 8 * C123_STAMP_WORDS + 9], LLONG_MAX, 0};
    for (int w = 0; w < 8; ++w) {
      const long long* dd = hbuf + ((size_t)g * 8 + w) * C123_STAMP_WORDS;
      x.in = std::min(x.in, dd[7]); x.out = std::max(x.out, dd[8]);
    }
    v.push_back(x);
  }
  std::sort(v.begin(), v.end(), [](const Wg& p, const Wg& q) { return p.key != q.key ? p.key < q.key : p.in < q.in; });
  double gap = 0, span = 0; int ngap = 0, ncu = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    if (i == 0 || v[i].key != v[i - 1].key) { ++ncu; continue; }
    gap += (double)(v[i].in - v[i - 1].out); ++ngap;
  }
  long long lo = LLONG_MAX, hi = 0;
  for (auto& x : v) { lo = std::min(lo, x.in); hi = std::max(hi, x.out); }
  span = (double)(hi - lo);
  fprintf(stderr, "[stamps %s] workgroups %d on %d CUs; turn-around gap on a CU: %d gaps, mean %.0f ns; first entry -> last exit %.1f us\n",
          tag, nwg, ncu, ngap, ngap ? gap * 10.0 / ngap : 0.0, span / 100.0);
}
#define C123_STAMP(k) stamps(k)
#else
#define C123_STAMP(k)
#endif

// ---------------------------------------------------------------------------------------------------------- producers
// conv12_fused_kernel's main loop (same pipeline, same consume-step schedule), 256 threads, columns shifted by one, plus
// the second block-1 tile and the a2 hand-off.  Barrier count: niter3 (one per unit) + 4 (prologue) + 2 (idle steps).
// PERSIST: (b, f0) is unit u, the first of the workgroup's range [u, u_end); every later unit of the range executes
// niter3 + 3 barriers (one boundary barrier instead of the four of the prologue: conv123_persist.hip), in both roles.
// CARRY (PERSIST only; every range starts at the first strip of an utterance): no second tile.  Tile 0 is slots 2 .. 33, and
// slots 0, 1 of a row are the previous strip's slots 30, 31 of that row, kept in the side buffer (conv123_carry.hip).
template <typename TX, bool PIPE, bool PERSIST>
__device__ __forceinline__ void c123_producer(const Conv123Args& a, char* smem, unsigned lds0, int tid, int wave, int b, int f0,
                                              int niter3, int u, int u_end) {
  using namespace c123;
  static_assert(PERSIST || !CARRY, "the carried columns come from the previous unit of the workgroup");
  const int lane = tid & 63;
  const int nsl = wave & 1, mg = wave >> 1;
  const int r = lane & 31, h = lane >> 5;
  const int H = a.H1, W = a.F, T = a.T;
  const unsigned plds = lds0 + P_OFF;
  char* const psm = smem + P_OFF;
  const float rlim = relu_limit();
  if (DFA_C123_PRIO == 2) __builtin_amdgcn_s_setprio(1);
#ifdef DFA_STAMPS
  C123Stamps stamps;
  const int stamp_u0 = u;
#endif
#if DFA_C123_CLS
  const int cls_u0 = u;
#endif

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
  const TX* xb = (const TX*)a.x + (long long)b * a.sxb;   // (per unit: re-pointed by next_unit below)
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
      else xreg[k] = cvt_out<bf16_t>(ld1(src)).v;
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
  const unsigned c1_win0 = plds + XW_OFF + ((2 * c1_m + 2 * h) * SP + CS + r) * 8;
  const unsigned c1_win1 = plds + XW_OFF + ((2 * c1_m + 2 * h) * SP + 32 + (r & 1)) * 8;
  const int c1_f0 = f0 - 2 + CS + r, c1_f1 = f0 + 30 + (r & 1);
  bool c1_fok0 = c1_f0 >= 0 && c1_f0 < W, c1_fok1 = c1_f1 < W;       // (per unit)
  const int c1_dst0 = (c1_m * SP + CS + r) * PB, c1_dst1 = (c1_m * SP + 32 + (r & 1)) * PB;
  const int c1_sw0 = lds_swz<PB>(CS + r), c1_sw1 = lds_swz<PB>(32 + (r & 1));
  const bool c1_live1 = r < 2;
#if DFA_C123_CARRY
  // CARRY: lanes r = SW - 2, SW - 1 hold slots 30, 31 = the next strip's slots 0, 1; each of the four keeps its two 16-byte
  // chunks of the row's side entry and, one unit later, moves them into the ring (chunk swizzle of slots 0, 1: none)
  static_assert(PB == 64 && CY <= 4 && (SW - CY) % 2 == 0, "lds_swz<64> of slots 0 .. 3 is 0");
  const bool cy_lane = (r >> 1) == (SW - CY) / 2;
  const unsigned cy_side = lds0 + SIDE_OFF + c1_m * SIDE_ROWB + (r & 1) * PB + (h << 4);
  const int cy_dst = (c1_m * SP + (r & 1)) * PB + (h << 4);
  bool cy_on = f0 != 0;                                               // (per unit) false: the carried columns are off the image
#endif
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  struct C1State { u32x2_t w0, w1, w2, w3; f32x16_t e, o; float v[16]; };
  auto c1_issue = [&](C1State& st, int j) {       // four window reads (asm: they join the counted LDS pipeline)
    const unsigned a0 = c1_win0 + (j & 1) * XW_BYTES, a1 = c1_win1 + (j & 1) * XW_BYTES;
    if constexpr (PIPE) {
      asm volatile("ds_read_b64 %0, %1" : "=v"(st.w0) : "v"(a0));
      asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(st.w1) : "v"(a0), "n"(XW_ROWB));
      if constexpr (!CARRY) {
        asm volatile("ds_read_b64 %0, %1" : "=v"(st.w2) : "v"(a1));
        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(st.w3) : "v"(a1), "n"(XW_ROWB));
      }
    } else {
      st.w0 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)a0);
      st.w1 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)(a0 + XW_ROWB));
      if constexpr (!CARRY) {
        st.w2 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)a1);
        st.w3 = *(const u32x2_t*)((const __attribute__((address_space(3))) char*)(size_t)(a1 + XW_ROWB));
      }
    }
  };
  auto c1_mfma = [&](C1State& st, auto t_c) {
    constexpr int TL = decltype(t_c)::value;
    if constexpr (PIPE && CARRY) asm volatile("" : "+v"(st.w0), "+v"(st.w1));
    else if constexpr (PIPE) asm volatile("" : "+v"(st.w0), "+v"(st.w1), "+v"(st.w2), "+v"(st.w3));
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
#if DFA_C123_CARRY
  // ---- CARRY.  Per a1 row (ring block j, row c1_m), in this program order and all by wave c1_m:
  //   cy_issue   read the row's side entry (the previous unit's slots 30, 31)
  //   c1_store_cy  tile 0 into ring slots 2 .. 33, then slots 30, 31 (lanes cy_lane) over the side entry
  //   cy_store   (the reads landed) ring slots 0, 1 = the entry, or zeros where the unit is the first strip of its utterance
  // `side` / `dst` / `live` are cy_side / cy_dst / cy_lane, or the same values from a fresh lane number between two units.
  auto cy_issue = [&](u32x4_t& c0, u32x4_t& c2, int j, unsigned side) {
    const unsigned sa = side + j * SIDE_BLKB;
    if constexpr (PIPE) {
      asm volatile("ds_read_b128 %0, %1" : "=v"(c0) : "v"(sa));
      asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(c2) : "v"(sa));
    } else {
      c0 = *(const u32x4_t*)((const __attribute__((address_space(3))) char*)(size_t)sa);
      c2 = *(const u32x4_t*)((const __attribute__((address_space(3))) char*)(size_t)(sa + 32));
    }
  };
  auto c1_store_cy = [&](C1State& st, int ringblk, int j, int dst0, int sw, int hh, unsigned side, bool live) {
    u32x4_t pk[2];
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const unsigned a0 = pack_bf16x2(st.v[4 * g], st.v[4 * g + 1]), a1 = pack_bf16x2(st.v[4 * g + 2], st.v[4 * g + 3]);
      const unsigned b0 = pack_bf16x2(st.v[4 * g + 4], st.v[4 * g + 5]), b1 = pack_bf16x2(st.v[4 * g + 6], st.v[4 * g + 7]);
      const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      const unsigned addr = plds + ringblk * (BR * ROWB) + dst0 + (((g + hh) ^ sw) << 4);
      pk[g / 2] = u32x4_t{s0[0], s1[0], s0[1], s1[1]};
      if constexpr (PIPE) asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(pk[g / 2]) : "memory");
      else *(u32x4_t*)((__attribute__((address_space(3))) char*)(size_t)addr) = pk[g / 2];
    }
    const unsigned sa = side + j * SIDE_BLKB;
    if (live) {                    // lanes 28, 29, 60, 61: chunks hh and 2 + hh of slot r - 28
      if constexpr (PIPE) {
        asm volatile("ds_write_b128 %0, %1" : : "v"(sa), "v"(pk[0]) : "memory");
        asm volatile("ds_write_b128 %0, %1 offset:32" : : "v"(sa), "v"(pk[1]) : "memory");
      } else {
        *(u32x4_t*)((__attribute__((address_space(3))) char*)(size_t)sa) = pk[0];
        *(u32x4_t*)((__attribute__((address_space(3))) char*)(size_t)(sa + 32)) = pk[1];
      }
    }
  };
  auto cy_store = [&](u32x4_t& c0, u32x4_t& c2, int ringblk, int dst, bool live) {
    if constexpr (PIPE) asm volatile("" : "+v"(c0), "+v"(c2));
#pragma unroll
    for (int e = 0; e < 4; ++e) { c0[e] = cy_on ? c0[e] : 0u; c2[e] = cy_on ? c2[e] : 0u; }   // a select: stale LDS never multiplies
    const unsigned addr = plds + ringblk * (BR * ROWB) + dst;
    if (live) {
      if constexpr (PIPE) {
        asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(c0) : "memory");
        asm volatile("ds_write_b128 %0, %1 offset:32" : : "v"(addr), "v"(c2) : "memory");
      } else {
        *(u32x4_t*)((__attribute__((address_space(3))) char*)(size_t)addr) = c0;
        *(u32x4_t*)((__attribute__((address_space(3))) char*)(size_t)(addr + 32)) = c2;
      }
    }
  };
  // one a1 row outside the main loop (prologue: FRESH = false; between two units: lane constants from a fresh lane number)
  auto produce_cy = [&](int j, int ringblk, auto fresh_c) {
    constexpr bool FRESH = decltype(fresh_c)::value;
    C1State st;
    u32x4_t c0, c2;
    c1_issue(st, j);
    if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(st.w0), "+v"(st.w1));
    c1_mfma(st, std::integral_constant<int, 0>{});
    c1_relu(st, j, std::integral_constant<int, 0>{});
    const int fl = FRESH ? c123_fresh_lane() : lane, fr = fl & 31, fh = fl >> 5;
    const unsigned side = lds0 + SIDE_OFF + c1_m * SIDE_ROWB + (fr & 1) * PB + (fh << 4);
    const bool live = (fr >> 1) == (SW - CY) / 2;
    cy_issue(c0, c2, j, side);
    c1_store_cy(st, ringblk, j, (c1_m * SP + CS + fr) * PB, lds_swz<PB>(CS + fr), fh, side, live);
    if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(c0), "+v"(c2) : : "memory");
    cy_store(c0, c2, ringblk, (c1_m * SP + (fr & 1)) * PB + (fh << 4), live);
  };
#endif
  // c1_store between two units of the persistent kernel: the same stores, their lane constants from a fresh lane number
  // (c123_fresh_lane; as a mode of c1_store itself the per-unit kernel compiled to other registers)
  auto c1_store_fresh = [&](C1State& st, int ringblk, auto t_c) {
    constexpr int TL = decltype(t_c)::value;
    const int fl = c123_fresh_lane(), fh = fl >> 5, fslot = TL == 0 ? (fl & 31) : 32 + (fl & 1);
    const int dst = ringblk * (BR * ROWB) + (c1_m * SP + fslot) * PB;
    const int sw = lds_swz<PB>(fslot);
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      const unsigned a0 = pack_bf16x2(st.v[4 * g], st.v[4 * g + 1]), a1 = pack_bf16x2(st.v[4 * g + 2], st.v[4 * g + 3]);
      const unsigned b0 = pack_bf16x2(st.v[4 * g + 4], st.v[4 * g + 5]), b1 = pack_bf16x2(st.v[4 * g + 6], st.v[4 * g + 7]);
      const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      const unsigned addr = plds + dst + (((g + fh) ^ sw) << 4);
      const u32x4_t pk = {s0[0], s1[0], s0[1], s1[1]};
      if (TL == 0 || (fl & 31) < 2) {
        if constexpr (PIPE) asm volatile("ds_write_b128 %0, %1" : : "v"(addr), "v"(pk) : "memory");
        else *(u32x4_t*)((__attribute__((address_space(3))) char*)(size_t)addr) = pk;
      }
    }
  };
  auto produce_now = [&](int j, int ringblk) {
#if DFA_C123_CARRY
    produce_cy(j, ringblk, std::false_type{});
    return;
#endif
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
  auto produce_fresh = [&](int j, int ringblk) {     // produce_now between two units of the persistent kernel
#if DFA_C123_CARRY
    produce_cy(j, ringblk, std::true_type{});
    return;
#endif
    C1State st;
    c1_issue(st, j);
    if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(st.w0), "+v"(st.w1), "+v"(st.w2), "+v"(st.w3));
    c1_mfma(st, std::integral_constant<int, 0>{});
    c1_relu(st, j, std::integral_constant<int, 0>{});
    c1_store_fresh(st, ringblk, std::integral_constant<int, 0>{});
    c1_mfma(st, std::integral_constant<int, 1>{});
    c1_relu(st, j, std::integral_constant<int, 1>{});
    c1_store_fresh(st, ringblk, std::integral_constant<int, 1>{});
  };

  // a2 hand-off: pixel r = column f0 - 1 + r = consumer ring slot r; lanes own channels 32 nsl + 8h + 16g .. + 7 after the swap
  const int col = f0 - 1 + r;
  bool col_ok = col >= 0 && col < W;                                 // (per unit)
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
    constexpr int NWR = CARRY ? 2 : 4;   // window reads issued behind fragment read S_BAR
    // CARRY: behind C_STORE two side reads, two ring stores, two side stores; the reads have landed four consume steps on
    // (fragment read C_STORE + PF, issued behind them, is retired there), where C_CARRY puts them into ring slots 0, 1
    constexpr int N_STORE = CARRY ? 6 : 2, C_CARRY = C_STORE + PF;
    static_assert(C_CARRY == C_RELU1 && C_CARRY + PF - 1 < C_STORE1 + PF - 1 && C_CARRY < NR, "");
    u32x4_t xbuf[PF];
    C1State c1;
#if DFA_C123_CARRY
    u32x4_t cy0, cy2;
#endif
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
        constexpr int C_ST2 = CARRY ? C_CARRY : C_STORE1;   // the second pair of ring stores
        constexpr int young = young_r + ((c > C_STORE && c <= C_STORE + PF - 1 && c < NR) ? N_STORE : 0) +
                              ((c > C_ST2 && c <= C_ST2 + PF - 1 && c < NR) ? 2 : 0) +
                              ((c > C_XSTORE && c <= C_XSTORE + PF - 1 && c < NR) ? 3 * NXLD : 0) +
                              ((c > S_BAR - PF && c <= S_BAR) ? NWR : 0);
        if constexpr (PIPE) lds_wait<young>(xbuf[c % PF]);
        const uint4 xv = __builtin_bit_cast(uint4, xbuf[c % PF]);
        if constexpr (i <= 2) acc0 = Mma<bf16_t>::run(w[i * 3 + dx][kg], xv, acc0);
        if constexpr (i >= 1) acc1 = Mma<bf16_t>::run(w[(i - 1) * 3 + dx][kg], xv, acc1);
        if constexpr (c == C_MFMA) c1_mfma(c1, std::integral_constant<int, 0>{});
        if constexpr (c == C_XLOAD) x_load(it + 3);
        if constexpr (c == C_RELU) c1_relu(c1, it + 2, std::integral_constant<int, 0>{});
        if constexpr (c == C_MFMA1 && !CARRY) c1_mfma(c1, std::integral_constant<int, 1>{});
        if constexpr (c == C_STORE && !CARRY) c1_store(c1, (PH + 2) % 3, std::integral_constant<int, 0>{});
#if DFA_C123_CARRY
        if constexpr (c == C_STORE) {
          cy_issue(cy0, cy2, it + 2, cy_side);
          c1_store_cy(c1, (PH + 2) % 3, it + 2, c1_dst0, c1_sw0, h, cy_side, cy_lane);
        }
        if constexpr (c == C_CARRY) cy_store(cy0, cy2, (PH + 2) % 3, cy_dst, cy_lane);
#endif
        if constexpr (c == C_RELU1 && !CARRY) c1_relu(c1, it + 2, std::integral_constant<int, 1>{});
        if constexpr (c == C_XSTORE) x_store((it + 3) & 1);
        if constexpr (c == C_STORE1 && !CARRY) c1_store(c1, (PH + 2) % 3, std::integral_constant<int, 1>{});
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
    C123_STAMP(it < 2 ? 1 : 2);
  };
  C123_STAMP(0);
  // the per-unit values of unit v: feature offsets / column masks of the staging, block-1 and a2 column masks
  auto next_unit = [&](int v) {
    const int vb = v / a.nstrips, vf0 = (v - vb * a.nstrips) * SW;
    xb = (const TX*)a.x + (long long)vb * a.sxb;
    const int tid = wave * 64 + c123_fresh_lane(), r = tid & 31;    // (shadow the outer ones: see c123_fresh_lane)
#pragma unroll
    for (int k = 0; k < NXLD; ++k) {
      const int e = k * 256 + tid;
      const int row = t_fast ? e % XROWS : e / XCOLS, f = vf0 - 3 + (t_fast ? e / XROWS : e % XCOLS);
      xfok[k] = (e < NX) && f >= 0 && f < W;
      xoff[k] = (long long)(row - 3) * a.sxt + (long long)(xfok[k] ? f : 0) * a.sxf;
    }
    const int vf = vf0 - 2 + CS + r;
    c1_fok0 = vf >= 0 && vf < W;
    c1_fok1 = vf0 + 30 + (r & 1) < W;
#if DFA_C123_CARRY
    cy_on = vf0 != 0;
#endif
    const int vcol = vf0 - 1 + r;
    col_ok = vcol >= 0 && vcol < W;
  };
  // the niter3 working steps of a unit, then (idle step niter3) a2 row 2 niter3 (>= H2: zero padding of the consumers' last
  // iteration) = block niter3, row 1.  A macro, not a lambda: as a lambda the per-unit kernel compiled to other registers.
#define DFA_C123_PRODUCER_STEPS()                                                           \
  for (int it = 0; it < niter3; it += 3) {                                                  \
    iteration(std::integral_constant<int, 0>{}, it);                                        \
    if (it + 1 < niter3) iteration(std::integral_constant<int, 1>{}, it + 1);               \
    if (it + 2 < niter3) iteration(std::integral_constant<int, 2>{}, it + 2);               \
  }                                                                                         \
  {                                                                                         \
    char* zr = smem + (niter3 & (CNB - 1)) * (CBR * CROWB) + CROWB;                         \
    const unsigned zz = c123_zero<PERSIST>();                                               \
    *(uint4*)(zr + (PERSIST ? wave * 64 + c123_fresh_lane() : tid) * 16) = make_uint4(zz, zz, zz, zz); \
  }
  if constexpr (!PERSIST) {
    DFA_C123_PRODUCER_STEPS()
    barrier();
    barrier();                 // idle step niter3 + 1
    C123_STAMP(3);
  } else {
    // Unit boundary: the prologue of the next unit in the two idle steps of this one, while the consumers finish it.
    // LDS ownership (the argument in full: conv123_persist.hip).  Windows and a1 ring are read by all four producer waves
    // and by nobody else: every c1_issue and ring read of this unit has completed (counted, then drained) before barrier
    // T1, so the x_store pairs may follow T1 and the ring writes of produce_now T2.  The consumers still read a2 ring
    // blocks niter3 - 2 .. niter3 until they reach N1; the first a2 write of the next unit is behind its step-0 barrier.
    // (The block / buffer numbers go through `opq`: as compile-time constants each call would have its own set of lane
    // address constants, hoisted out of the loop over units and alive across the main loop, which has no register to spare.)
    auto opq = [](int v) { asm volatile("" : "+s"(v)); return v; };
    for (;;) {
      DFA_C123_PRODUCER_STEPS()
      if (++u >= u_end) break;
      next_unit(u);
      unsigned short xr0[NXLD], xr1[NXLD];
      bool xk0[NXLD], xk1[NXLD];
      x_load(opq(0));                     // both round trips in flight before T1 (registers are free between two units)
#pragma unroll
      for (int k = 0; k < NXLD; ++k) { xr0[k] = xreg[k]; xk0[k] = xok[k]; }
      x_load(opq(1));
#pragma unroll
      for (int k = 0; k < NXLD; ++k) { xr1[k] = xreg[k]; xk1[k] = xok[k]; }
      barrier();                          // T1 = idle step niter3
#pragma unroll
      for (int k = 0; k < NXLD; ++k) { xreg[k] = xr0[k]; xok[k] = xk0[k]; }
      x_store(opq(0));
      x_load(opq(2));
#pragma unroll
      for (int k = 0; k < NXLD; ++k) { xr0[k] = xreg[k]; xk0[k] = xok[k]; xreg[k] = xr1[k]; xok[k] = xk1[k]; }
      x_store(opq(1));
      barrier();                          // T2 = idle step niter3 + 1
      C123_STAMP(3);
      produce_fresh(opq(0), opq(0));
      produce_fresh(opq(1), opq(1));
      barrier();                          // N1: the only barrier in place of the prologue's four
#pragma unroll
      for (int k = 0; k < NXLD; ++k) { xreg[k] = xr0[k]; xok[k] = xk0[k]; }
      x_store(opq(0));                    // (window buffer 0 was last read by produce_now(0, .) above, before N1)
      C123_STAMP(0);
    }
    barrier();
    barrier();                 // idle step niter3 + 1 of the last unit
    C123_STAMP(3);
#if DFA_C123_CLS
    // the consumers' classifier barriers (c123_classifier): one, then one per utterance of the range
    for (int k = (u_end - cls_u0) / a.nstrips; k >= 0; --k) __syncthreads();
#endif
  }
#ifdef DFA_STAMPS
  stamps.write(wave, lane, (PERSIST ? u_end : stamp_u0 + 1) - stamp_u0);
#endif
#undef DFA_C123_PRODUCER_STEPS
}

#if DFA_C123_CLS
// ---------------------------------------------------------------------------------------------------------- classifier
// logits[bb] for the utterances [b0, b1) of the workgroup, by its four consumer waves, behind the last time-mean stores of the
// last unit: linear1_kernel's operation sequence (linear.hip) with the consumer thread number in the role of its thread
// number -- one fmaf chain per thread over the float4 words ctid + 256 k (x, y, z, w in that order), the same shuffle tree,
// the same ((p0 + p1) + (p2 + p3)) + bias -- so the logits are the bits the separate launch gives.  The launcher takes this
// kernel only where emb rows and weights are 16-byte aligned (K = 128 F is a multiple of 4: no scalar tail).
// Visibility.  The emb rows were stored by these four waves, each lane its own words, and are read across waves: every wave
// waits for its stores (release at workgroup scope = vmcnt(0); the waves of a workgroup share the CU's vector L1, which
// the stores write through), all meet at a workgroup barrier, then acquire.  No other workgroup reads or writes these rows.
// Barriers: 1 + (b1 - b0), all eight waves (the producers execute the same number before they return: c123_producer).
// The partial sums alternate between two sets of four words of the block-3 bias area (read by the consumers alone, last in
// front of their last step barrier): the writers of utterance i + 2 have passed the barrier of utterance i + 1, which thread
// 0 reaches only after it has read the words of utterance i.
// The lane number is a fresh one (c123_fresh_lane): no address below is computed before the loop over units.
__device__ __forceinline__ void c123_classifier(const Conv123Args& a, char* smem, int cwave, int b0, int b1) {
  using namespace c123;
  constexpr int NB = 8;                            // float4 pairs in flight per thread
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // the time-mean stores of the last unit (and every LDS read)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const int clane = c123_fresh_lane(), ctid = cwave * 64 + clane;
  float* const part = (float*)(smem + CBIAS_OFF);
  const int K4 = a.cls_K >> 2;
  const float4* const w4 = reinterpret_cast<const float4*>(a.cls_w);
  for (int bb = b0; bb < b1; ++bb) {
    const float4* const e4 = reinterpret_cast<const float4*>(a.emb + (size_t)bb * a.cls_K);
    float acc = 0.f;
    for (int j0 = ctid; j0 < K4; j0 += 256 * NB) {
      float4 ev[NB], wv[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const int j = j0 + 256 * k, jc = j < K4 ? j : j0;      // (past the end: a word this thread owns anyway, not used)
        ev[k] = e4[jc];
        wv[k] = w4[jc];
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        float t = acc;
        t = fmaf(ev[k].x, wv[k].x, t);
        t = fmaf(ev[k].y, wv[k].y, t);
        t = fmaf(ev[k].z, wv[k].z, t);
        t = fmaf(ev[k].w, wv[k].w, t);
        acc = (j0 + 256 * k < K4) ? t : acc;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    float* const pp = part + 4 * ((bb - b0) & 1);
    if (clane == 0) pp[cwave] = acc;
    __syncthreads();
    if (ctid == 0) a.logits[bb] = ((pp[0] + pp[1]) + (pp[2] + pp[3])) + a.cls_b[0];
  }
}
#endif

// ---------------------------------------------------------------------------------------------------------- consumers
// conv3_m16_meant_kernel's eval unit on the 4-block ring the producers fill.  Barrier count: 4 (prologue) + 2 (idle steps)
// + niter3 (one per unit).  PERSIST: as the producers, niter3 + 3 for every unit of [u, u_end) after the first.
template <bool PIPE, bool PERSIST>
__device__ __forceinline__ void c123_consumer(const Conv123Args& a, char* smem, unsigned lds0, int ctid, int nsl, int b, int f0,
                                              int niter, int u, int u_end) {
  using namespace c123;
  constexpr int PF3 = 4;
  const int lane = ctid & 63;
  const int p = lane & 15, q = lane >> 4;
  const int H = a.H2, W = a.F, COUT = 128;
  const float rlim = relu_limit();
  if (DFA_C123_PRIO == 1) __builtin_amdgcn_s_setprio(1);
#ifdef DFA_STAMPS
  C123Stamps stamps;
  const int stamp_u0 = u;
#endif

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
    constexpr int S_BAR = DFA_C123_CBAR;
    static_assert(0 <= S_BAR && S_BAR <= 35, "reads 36 .. 47 are the a2 row the producers write in the interval this barrier ends");
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
          if constexpr (i <= 2) acc0[ca][pb] = mma16(w[i * 3 + dx][kk][ca], xv, acc0[ca][pb]);
          if constexpr (i >= 1) acc1[ca][pb] = mma16(w[(i - 1) * 3 + dx][kk][ca], xv, acc1[ca][pb]);
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
  C123_STAMP(0);
  if constexpr (!PERSIST) { barrier(); barrier(); }   // idle steps 0, 1 (PERSIST: per unit, below)
  if constexpr (!PERSIST) { C123_STAMP(1); }

  // canonical chunks of the time mean (conv3_m16.hip): a chunk's sum is added to the total after its last iteration
  const int chunk = a.chunk_iters > 0 ? a.chunk_iters : niter + 3;
  int next_flush = min(niter, chunk);
  long long st_c = 0, st_r = 0;
  const bool probe = a.clock_stamps != nullptr;
  if constexpr (!PERSIST) {
    if (probe) {
      st_c = __builtin_amdgcn_s_memtime();
      st_r = __builtin_amdgcn_s_memrealtime();
      __builtin_amdgcn_s_waitcnt(0xc07f);
    }
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
    C123_STAMP(it + 2 < niter ? 2 : 3);
  };
  // (macros for the reason given in the producers)
#define DFA_C123_CONSUMER_STEPS()                                                           \
  for (int it = 0; it < niter; it += 4) {                                                   \
    citer(std::integral_constant<int, 0>{}, it);                                            \
    if (it + 1 < niter) citer(std::integral_constant<int, 1>{}, it + 1);                    \
    if (it + 2 < niter) citer(std::integral_constant<int, 2>{}, it + 2);                    \
    if (it + 3 < niter) citer(std::integral_constant<int, 3>{}, it + 3);                    \
  }
  // the time mean of unit (b, f0): this lane's totals -> emb; P, Q = the lane's pixel and channel-group numbers
#define DFA_C123_EMIT(P, Q)                                                                 \
  _Pragma("unroll") for (int ca = 0; ca < 2; ++ca)                                          \
    _Pragma("unroll") for (int pb = 0; pb < 2; ++pb) {                                      \
      const int col = f0 + 16 * pb + (P);                                                   \
      const f32x4_t tv = tot[(ca * 2 + pb) * NT];                                           \
      if (16 * pb + (P) < SW && col < W) {                                                  \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                     \
          const int c = nsl * 32 + 16 * ca + 4 * (Q) + e;                                   \
          a.emb[((size_t)b * COUT + c) * W + col] = tv[e] * a.inv_h;                        \
        }                                                                                   \
      }                                                                                     \
    }
  if constexpr (!PERSIST) {
    DFA_C123_CONSUMER_STEPS()
    const int bid = blockIdx.x;
    if (probe && ctid == 0 && bid < 1024) {
      a.clock_stamps[2 * bid] = __builtin_amdgcn_s_memtime() - st_c;
      a.clock_stamps[2 * bid + 1] = __builtin_amdgcn_s_memrealtime() - st_r;
    }
    DFA_C123_EMIT(p, q)
    C123_STAMP(4);
  } else {
    const int bid = blockIdx.x;
#if DFA_C123_LATE_EMIT || DFA_C123_CLS
    const int u_first = u;
#endif
    long long sum_c = 0, sum_r = 0;               // the probe reports the main loops of all units of the workgroup
    for (;;) {
#if DFA_C123_LATE_EMIT
      // The time mean of the unit before this one goes out between the two idle barriers, under the producers' step 0 (which
      // stands behind the first of them), and the totals are zeroed behind it: this lane's own LDS words, long before the
      // first flush of this unit.  Ring row -1 was zeroed behind N1, both idle barriers before its first reader.
      barrier();                                  // idle step 0
      if (u != u_first) {
        C123_STAMP(1);
        int pl = p, ql = q;
        asm volatile("" : "+v"(pl), "+v"(ql));
        if (DFA_C123_EMIT_PRIO0 && DFA_C123_PRIO == 1) __builtin_amdgcn_s_setprio(0);
        DFA_C123_EMIT(pl, ql)
        if (DFA_C123_EMIT_PRIO0 && DFA_C123_PRIO == 1) __builtin_amdgcn_s_setprio(1);
        C123_STAMP(4);
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[k * NT] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        b = u / a.nstrips;
        f0 = (u - b * a.nstrips) * SW;
      }
      barrier();                                  // idle step 1
#else
      barrier(); barrier();                       // idle steps 0, 1
#endif
      C123_STAMP(1);
      next_flush = min(niter, chunk);
      if (probe) {
        st_c = __builtin_amdgcn_s_memtime();
        st_r = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0xc07f);
      }
      DFA_C123_CONSUMER_STEPS()
      if (probe) {
        sum_c += __builtin_amdgcn_s_memtime() - st_c;
        sum_r += __builtin_amdgcn_s_memrealtime() - st_r;
      }
      const bool last = u + 1 >= u_end;
      // Unit boundary.  N1: all four consumer waves have read the last a2 rows of this unit, so row -1 of the next one
      // (ring block 0, row 0) may be zeroed; the producers write rows 0, 1 behind the barrier of their step 0, and the
      // consumers' first read of block 0 is two barriers further on.  The totals are this lane's own LDS words: read
      // out, then zeroed, in program order.  The stores of the time mean run under the producers' fill steps.
      if (!last) {
        barrier();
        *(uint4*)(smem + ctid * 16) = make_uint4(0u, 0u, 0u, 0u);
#if DFA_C123_LATE_EMIT
        C123_STAMP(4);
        ++u;                                      // (b, f0) stay the finished unit's until its time mean is out: loop top
        continue;
#endif
      }
      // the time mean of unit (b, f0) -> emb.  (The lane numbers go through an empty asm so that no address of these
      // stores is computed before the loop over units and kept across the main loop, which has no register to spare.)
      int pl = p, ql = q;
      asm volatile("" : "+v"(pl), "+v"(ql));
      DFA_C123_EMIT(pl, ql)
      C123_STAMP(4);
      if (last) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) tot[k * NT] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      ++u;
      b = u / a.nstrips;
      f0 = (u - b * a.nstrips) * SW;
    }
    if (probe && ctid == 0 && bid < 1024) {
      a.clock_stamps[2 * bid] = sum_c;
      a.clock_stamps[2 * bid + 1] = sum_r;
    }
#if DFA_C123_CLS
    c123_classifier(a, smem, nsl, u_first / a.nstrips, u_end / a.nstrips);
    C123_STAMP(4);
#endif
  }
#undef DFA_C123_CONSUMER_STEPS
#undef DFA_C123_EMIT
#ifdef DFA_STAMPS
  stamps.write(4 + nsl, lane, (PERSIST ? u_end : stamp_u0 + 1) - stamp_u0);
#endif
}

// ---------------------------------------------------------------------------------------------------------- the frame
// What a workgroup of each of the four kernels does around the two roles: blockIdx -> XCD -> logical workgroup lw, its unit
// range [u0, u1) in the per-unit kernel's order (the strips of an utterance back to back), the first unit's (b, f0), and the
// roles by wave number (not parity): waves 0-3 and 4-7 land one of each on every SIMD.  Ranges: !PERSIST the one unit lw;
// PERSIST q or q + 1 units, q = units / grid, the first units % grid workgroups one more (conv123_persist.hip); CARRY q
// units, because conv123_plan lets that form run only where nothing remains and q is a multiple of nstrips (strip = 0).
template <typename TX, bool PIPE, bool PERSIST>
__device__ __forceinline__ void c123_workgroup(const Conv123Args& a, char* smem) {
  using namespace c123;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lw = xcd_logical_workgroup();
  int u0 = lw, u1 = lw + 1;
  if constexpr (PERSIST && CARRY) {
    const int uq = (a.B * a.nstrips) / (int)gridDim.x;
    u0 = lw * uq; u1 = u0 + uq;
  } else if constexpr (PERSIST) {
    const int nwg = gridDim.x, nunits = a.B * a.nstrips;
    const int uq = nunits / nwg, urem = nunits - uq * nwg;
    u0 = lw * uq + min(lw, urem); u1 = u0 + uq + (lw < urem ? 1 : 0);   // nwg <= nunits: never empty
  }
  const int b = u0 / a.nstrips, strip = u0 - b * a.nstrips;
  const int f0 = strip * SW;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int niter3 = (a.H2 + 1) / 2;
  if (wave < 4) c123_producer<TX, PIPE, PERSIST>(a, smem, lds0, tid, wave, b, f0, niter3, u0, u1);
  else c123_consumer<PIPE, PERSIST>(a, smem, lds0, tid - 256, wave - 4, b, f0, niter3, u0, u1);
}

// ---------------------------------------------------------------------------------------------------------- host
// the instantiation of a form's kernel K for the feature type and the pipelined / compiler-scheduled build
typedef void (*C123Kernel)(Conv123Args);
#define DFA_C123_KERNEL(K, x_dtype, pipe)                                                                           \
  ((x_dtype) == DFA_DTYPE_BF16 ? ((pipe) ? (C123Kernel)K<bf16_t, true> : (C123Kernel)K<bf16_t, false>)             \
                               : ((pipe) ? (C123Kernel)K<float, true> : (C123Kernel)K<float, false>))
// The launch of every form: grid and dynamic LDS bytes from conv123_plan, asked for this form alone.  Where the plan answers
// another form, this one's conditions do not hold (for the carry form: a range that began inside an utterance would read a
// side-buffer entry nobody wrote) and nothing is launched.
static hipError_t c123_launch(C123Kernel kern, int form, const char* tag, const Conv123Args& a, int num_cus, hipStream_t s) {
  const Conv123Plan p = conv123_plan(a.B, a.T, a.F, num_cus, form != DFA_CONV123_PER_UNIT, form == DFA_CONV123_CARRY, 0);
  if (p.form != form || p.grid < 1) return hipErrorInvalidValue;
  const hipError_t e = launch_lds(kern, dim3(p.grid), dim3(512), p.lds, s, a);
#ifdef DFA_STAMPS
  {
    static int calls = 0;      // seconds of back-to-back launches: the clock has settled (tools/gpu_stamps.py)
    if (++calls == 4000) c123_print_stamps(tag, p.grid);
  }
#endif
  return e;
}

}  // namespace dfa
#endif  // DFA_CONV123_BODY_H

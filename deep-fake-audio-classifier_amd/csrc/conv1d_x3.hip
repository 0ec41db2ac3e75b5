// conv1d_x3.hip -- one Conv1d(k = 3, pad 1) layer of the CNN1D TRAINING step on the matrix cores (src/train.py:71-76 through
// src/model_cnn1d.py:17-34): z[b][co][t] = bias[co] + sum_{ci, k} W[co][ci][k] in[b][ci][t + k - 1], channel-major fp32 in and
// out, no BatchNorm / ReLU (train mode: batch statistics come first).  It serves the three forward convolutions and -- on the
// flipped / transposed weight image of pack_conv1d_train_all_kernel -- the two data gradients.  Layer 1 of the eval kernel
// (cnn1d_fused_x3.hip), generalised: a workgroup = (utterance, MT tiles of 32 output channels); 16-channel slabs of the input go
// through LDS as they are (contiguous 16 T floats, 16-byte loads, two slabs ahead), the lane that owns frame t splits
// x[c][t-1..t+1] of its 8 channels into bf16 B fragments ONCE per slab and tap and feeds them to every channel tile; this layer's
// A fragments sit in LDS.
// TERMS = 3 (default): every fp32 operand = hi + lo + lo2, three bf16 terms (split8n<3>, dfa_device.h: the operand exactly), six MFMAs per product
// (all term pairs of order <= 2; the dropped ones are below 2^-24 of a product): fp32-grade sums.  TERMS = 2: the bf16x3
// construction of the eval kernel (16-bit operands, three MFMAs, ~1e-5) -- fine for inference's 1e-4 bar, but in a training step
// a 1e-5 perturbation of a pre-activation flips ~1e-5 of the ReLU masks and every flip moves a gradient by a whole element:
// relative L2 error ~ sqrt(1e-5) = 3e-3 against 3e-4 for fp32 arithmetic (tools/gpu_cnn1d_x3_probe.py), so it is opt-in.
// The fp32 VALU kernel this replaces (conv1d.hip) needs 97 us per call at [256, *, 321].
// K = 5 (layer 1 of the k = (5, 3, 3) variant: Conv1d(k = 5, pad 2), F -> 32, one channel tile) is the same kernel with its
// weights streamed; the kernel's comment has what that changes.
#include "cnn1d_x3_common.h"

namespace dfa {

struct Conv1dX3Args {
  const float* x;              // [B] x [Cin][T] contiguous per utterance, utterance stride sb floats, 16-byte aligned
  int64_t sb;
  const uint4* w;              // pack_conv1d_train_all_kernel image [Cout / 32][3][nks][TERMS][64]; five taps: [nks][5][TERMS][64]
  const float* bias;           // [Cout]
  float* z;                    // [B][Cout][T]
  int T, Cin, Cout, NT, nks, slab_floats, offW;
  AugCfg aug;                  // AUG instantiation (training layer 1): x is read through the armed train-time augmentation (rng.h)
  const int* lens;             // RAGGED instantiation (training layer 1 of a ragged batch): device [B], utterance b owns frames [0, lens[b]) of T
};

// A-fragment images with TERMS bf16 terms per weight: wx[m][tap][ks][term][lane] (pack_conv1d_train_all_kernel writes them)
size_t conv1d_terms_pack_bytes(int cin, int cout, int terms, int taps) { return (size_t)(cout / 32) * taps * cnn1d_x3_nks(cin) * terms * 64 * 16; }

// The five images of a training step (forward layers 1-3, data gradients 3 -> 2 and 2 -> 1) in ONE launch, the data-gradient ones read
// straight from the layer's own weight: W'[c][o][k'] = W[o][c][2 - k'] (a Conv1d with Cin' = Cout, Cout' = Cin) -- seven launches
// (five packs + two transposes) of ~4.5 us each otherwise, in a step of 0.6 ms.
struct Conv1dPackAll {
  const float* w[5];     // the layer's weight [Cout][Cin][3] (for a flipped entry: the FORWARD layer's weight)
  uint4* dst[5];
  int cin[5], cout[5], nks[5], flip[5], begin[6];   // cin / cout of the convolution the image serves; fragment range [begin[i], begin[i+1])
  int taps[5];           // 3; 5 for entry 0 of the k = (5, 3, 3) variant, whose image is k-step-major (cnn1d_x3_frag_slot)
  int terms;
  float* zero_bias;      // [256] zeroed here (the data gradients' bias)
};
__global__ void pack_conv1d_train_all_kernel(Conv1dPackAll a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 256) a.zero_bias[i] = 0.f;
  if (i >= a.begin[5]) return;
  int e = 0;
#pragma unroll
  for (int q = 1; q < 5; ++q) e += (i >= a.begin[q]) ? 1 : 0;
  const int li = i - a.begin[e], cin = a.cin[e], cout = a.cout[e], nks = a.nks[e];
  const int lane = li & 63;
  int rest = li >> 6;
  const int ks = rest % nks; rest /= nks;
  const int taps = a.taps[e];
  const int tap = rest % taps, m = rest / taps;
  const int co = 32 * m + (lane & 31), hh = lane >> 5;
  const float* w = a.w[e];
  bf16_t t0[8], t1[8], t2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = 16 * ks + 8 * hh + j;
    float v = 0.f;
    if (ci < cin) v = a.flip[e] ? w[((size_t)ci * cout + co) * 3 + (2 - tap)]      // forward weight [o = ci'][c = co'][2 - k'], its Cin = cout'
                                : w[((size_t)co * cin + ci) * taps + tap];
    t0[j] = float_to_bf16(v);
    const float r1 = v - bf16_to_float(t0[j]);
    t1[j] = float_to_bf16(r1);
    t2[j] = float_to_bf16(r1 - bf16_to_float(t1[j]));
  }
  uint4* dst = a.dst[e] + ((size_t)cnn1d_x3_frag_slot(m, tap, ks, taps, nks) * a.terms) * 64 + lane;
  dst[0] = *reinterpret_cast<const uint4*>(t0);
  dst[64] = *reinterpret_cast<const uint4*>(t1);
  if (a.terms == 3) dst[128] = *reinterpret_cast<const uint4*>(t2);
}
// w1, w2, w3: the three Conv1d weights [32][F][k1], [64][32][3], [128][64][3]; dst[0..4]: forward 1-3, data gradients 3 -> 2, 2 -> 1
hipError_t launch_pack_conv1d_train_all(const float* w1, const float* w2, const float* w3, void* const* dst, int F, int terms, float* zero_bias,
                                        hipStream_t s, int k1) {
  Conv1dPackAll a{};
  const float* w[5] = {w1, w2, w3, w3, w2};
  const int cin[5] = {F, 32, 64, 128, 64}, cout[5] = {32, 64, 128, 64, 32}, flip[5] = {0, 0, 0, 1, 1};
  a.begin[0] = 0;
  for (int i = 0; i < 5; ++i) {
    a.w[i] = w[i]; a.dst[i] = (uint4*)dst[i]; a.cin[i] = cin[i]; a.cout[i] = cout[i]; a.flip[i] = flip[i];
    a.nks[i] = cnn1d_x3_nks(cin[i]);
    a.taps[i] = i == 0 ? k1 : 3;
    a.begin[i + 1] = a.begin[i] + (cout[i] / 32) * a.taps[i] * a.nks[i] * 64;
  }
  a.terms = terms; a.zero_bias = zero_bias;
  const int total = a.begin[5] > 256 ? a.begin[5] : 256;
  hipLaunchKernelGGL(pack_conv1d_train_all_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

// K = taps (padding K / 2).  What five taps change: the image -- 5 taps x nks x TERMS KB, 180 KB at F = 180 with three terms -- has
// no resident form, so it is STREAMED as in the eval kernel (cnn1d_x3_body.h, C1X_K1 = 5): packed k-step-major, one k-step's
// [5 taps][TERMS][64 lanes] fragments (15 KB / 10 KB) pass through two LDS buffers -- k-step s + 1 is parked while k-step s is
// computed, k-step s + 2 is in flight in two registers -- on the slabs' own barrier; and the lane reads x[c][t - 2 .. t + 2] per
// tap inside the tap loop (16 values live instead of 80), where three taps read theirs up front.  Each tap ends in a
// sched_barrier, so the two forms of the read are different schedules: they stay two.
template <int MT, int TERMS, bool AUG = false, bool RAGGED = false, int K = 3>
__global__ __launch_bounds__(512) void conv1d_x3_kernel(Conv1dX3Args a) {
  static_assert(K == 3 || (K == 5 && MT == 1 && !RAGGED), "five taps: one channel tile (Cout = 32), uniform batches");
  using namespace c1x;
  constexpr int WKS = K * TERMS * 64;                      // K = 5: uint4 of one k-step's fragments, 960 (three terms) or 640
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int b = blockIdx.x, m0 = K == 5 ? 0 : blockIdx.y * MT;
  const int T = a.T, NT = a.NT, nks = a.nks;
  float* const slab0 = (float*)smem;                      // two slabs of slab_floats floats: [4 pad][16 x T][4 pad]
  char* const wS = smem + a.offW;                         // this workgroup's A fragments [MT][3][nks][TERMS][64] x 16 B; K = 5: W[0], W[1], one k-step each
  f32x16_t acc[MT][MAXT1];
  const float4* xg = (const float4*)(a.x + (size_t)b * a.sb);
  const int SL = a.slab_floats;
  constexpr int NLD = 3;                                   // 16 T / 4 float4 per slab <= 1536 = 3 x 512
  float4 xrA[NLD], xrB[NLD];
  const int nreal = (a.Cin + 15) / 16;                     // slabs that exist (nks may be one more: a zero slab)
  auto slab_n4 = [&](int s) { return max(0, min(16, a.Cin - 16 * s)) * T / 4; };
  auto slab_load = [&](int s, float4 (&xr)[NLD]) {         // unconditional, clamped (see the fused kernel)
    const int sc = min(s, nreal - 1), n4 = slab_n4(sc);
    if constexpr (AUG) {
      // element (channel = feature dim f, frame t) of the augmented batch: the source frame is rolled, so the slab is gathered
      // element by element (4 dword loads per float4 slot) and finished by aug_apply -- the value dfa_augment_batch would write
      const float* xf = a.x + (size_t)b * a.sb;
#pragma unroll
      for (int k = 0; k < NLD; ++k) {
        const int i = min(k * NTH + tid, n4 - 1);
        float e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int flat = 4 * i + u, c = flat / T, t = flat - c * T, f = 16 * sc + c;
          e[u] = aug_apply(a.aug, xf[(size_t)f * T + aug_src_t(a.aug, t)], b, t, f);
        }
        xr[k] = make_float4(e[0], e[1], e[2], e[3]);
      }
    } else if constexpr (RAGGED) {
      // the same 16-byte loads; the padding frames t >= lens[b] of every channel row are cleared bit-wise (they may hold NaN / Inf):
      // the slab is 16 rows of T floats back to back, so element `flat` is frame flat mod T
      const float4* src = xg + (size_t)4 * sc * T;
      const int Tb = a.lens[b];
#pragma unroll
      for (int k = 0; k < NLD; ++k) {
        const int i = min(k * NTH + tid, n4 - 1);
        const float4 v = src[i];
        const int flat = 4 * i, t0 = flat - (flat / T) * T;
        unsigned q[4] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          int t = t0 + u;
          t = t >= T ? t - T : t;                              // T >= 3: at most one wrap into the next row
          q[u] = t < Tb ? q[u] : 0u;
        }
        xr[k] = make_float4(__uint_as_float(q[0]), __uint_as_float(q[1]), __uint_as_float(q[2]), __uint_as_float(q[3]));
      }
    } else {
      const float4* src = xg + (size_t)4 * sc * T;
#pragma unroll
      for (int k = 0; k < NLD; ++k) xr[k] = src[min(k * NTH + tid, n4 - 1)];
    }
  };
  auto slab_store = [&](int s, const float4 (&xr)[NLD]) {
    float* dst = slab0 + (s & 1) * SL + 4;
    const int n4 = slab_n4(s);
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int i = k * NTH + tid;
      const unsigned m = i < n4 ? 0xffffffffu : 0u;
      const float4 v = xr[k];
      if (i < 4 * T)
        *(uint4*)(dst + 4 * i) = make_uint4(__float_as_uint(v.x) & m, __float_as_uint(v.y) & m, __float_as_uint(v.z) & m, __float_as_uint(v.w) & m);
    }
  };
  // K = 5, the weight stream
  uint4 wr0, wr1;                                          // k-step in flight (two scalars: an array of two was kept in scratch)
  auto w_load = [&](int s) {                               // unconditional, clamped: past the last k-step the last one again
    const uint4* src = a.w + (size_t)min(s, nks - 1) * WKS;
    wr0 = src[tid];
    wr1 = src[min(NTH + tid, WKS - 1)];
  };
  auto w_park = [&](int s) {                               // registers -> W[s & 1]
    char* dst = wS + (s & 1) * (WKS * 16);
    *(uint4*)(dst + (size_t)tid * 16) = wr0;
    if (tid < WKS - NTH) *(uint4*)(dst + (size_t)(NTH + tid) * 16) = wr1;
  };
  if constexpr (K == 5) w_load(0);
  slab_load(0, xrA);
  slab_load(1, xrB);
  if constexpr (K == 5) {
    w_park(0);
    w_load(1);
  } else {                                                 // the whole image, resident
    const int n = MT * 3 * nks * TERMS * 64;
    const uint4* wsrc = a.w + (size_t)m0 * 3 * nks * TERMS * 64;
    for (int i = tid; i < n; i += NTH) *(uint4*)(wS + (size_t)i * 16) = wsrc[i];
  }
  if (tid < 16) {
    const int sbuf = tid >> 3, e = tid & 7;
    slab0[sbuf * SL + (e < 4 ? e : 16 * T + e)] = 0.f;
  }
  slab_store(0, xrA);
  __syncthreads();

  const int nmine = (NT - wave + NW - 1) / NW;
  unsigned tin[MAXT1][K];                                  // all-ones where tap k of this lane's frame exists (t - K / 2 + k in [0, T)), else 0
  int tl[MAXT1];
#pragma unroll
  for (int j = 0; j < MAXT1; ++j) {
    const int t = TW * (wave + NW * j) + col;
    tl[j] = t;
#pragma unroll
    for (int k = 0; k < K; ++k) tin[j][k] = ((j < nmine) && t < T && t - K / 2 + k >= 0 && t - K / 2 + k < T) ? 0xffffffffu : 0u;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;
  }
  // one slab = one k-step of 16 channels: trip s computes slab s from buffer s & 1, requests slab s + 2 and parks slab s + 1
  // (requested a trip ago) in the other buffer; one barrier per trip.  Inside a trip the TAP is the outer loop: its MT x TERMS
  // weight fragments are read from LDS once and serve both of the wave's frame tiles.  K = 5: the fragments are those of
  // W[s & 1]; the trip also parks k-step s + 1 in W[(s + 1) & 1] (last read in trip s - 1, behind that trip's barrier) and
  // requests k-step s + 2.
  auto trip = [&](int s, float4 (&xr_next)[NLD], float4 (&xr_far)[NLD], bool load) {
    if (load) slab_load(s + 2, xr_far);
    const float* sl = slab0 + (s & 1) * SL + 4 + 8 * h * T - K / 2;   // this lane half's 8 channels, frame index - K / 2
    [[maybe_unused]] float v3[MAXT1][3][8];
    if constexpr (K == 3) {
#pragma unroll
      for (int j = 0; j < MAXT1; ++j)
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
          for (int k = 0; k < 3; ++k) v3[j][k][c] = sl[c * T + tl[j] + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uint4 w[MT][TERMS];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int p = 0; p < TERMS; ++p) {
          const int f = K == 5 ? ((s & 1) * K + k) * TERMS + p : ((m * 3 + k) * nks + s) * TERMS + p;
          w[m][p] = *(const uint4*)(wS + ((size_t)(f * 64 + lane)) * 16);
        }
#pragma unroll
      for (int j = 0; j < MAXT1; ++j) {
        uint4 xs[TERMS];
        if constexpr (K == 5) {
          float v[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) v[c] = sl[c * T + tl[j] + k];
          split8n<TERMS>(v, xs);
        } else {
          split8n<TERMS>(v3[j][k], xs);
        }
#pragma unroll
        for (int p = 0; p < TERMS; ++p) xs[p] = and4(tin[j][k], xs[p]);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if constexpr (TERMS == 3) {                      // smallest terms first
            acc[m][j] = mma32(w[m][2], xs[0], acc[m][j]);
            acc[m][j] = mma32(w[m][0], xs[2], acc[m][j]);
            acc[m][j] = mma32(w[m][1], xs[1], acc[m][j]);
          }
          acc[m][j] = mma32(w[m][1], xs[0], acc[m][j]);
          acc[m][j] = mma32(w[m][0], xs[1], acc[m][j]);
          acc[m][j] = mma32(w[m][0], xs[0], acc[m][j]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (K == 5) {
      w_park(s + 1);
      w_load(s + 2);
    }
    slab_store(s + 1, xr_next);
    __syncthreads();
  };
  int s = 0;
  for (; s + 2 < nks; s += 2) {                              // nks is even
    trip(s, xrB, xrA, true);
    trip(s + 1, xrA, xrB, true);
  }
  trip(s, xrB, xrA, false);
  trip(s + 1, xrA, xrB, false);

  // ---- + bias, channel-major store: register r = channel (r&3) + 8 (r>>2) + 4 h of frame t = lane: 32 lanes write 128 contiguous bytes
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int cb = 32 * (m0 + m) + 4 * h;
    float bv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) bv[r] = a.bias[cb + (r & 3) + 8 * (r >> 2)];
#pragma unroll
    for (int j = 0; j < MAXT1; ++j) {
      const int t = tl[j];
      if (j < nmine && t < T) {
        float* zr = a.z + ((size_t)b * a.Cout + cb) * T + t;
#pragma unroll
        for (int r = 0; r < 16; ++r) zr[(size_t)((r & 3) + 8 * (r >> 2)) * T] = acc[m][j][r] + bv[r];
      }
    }
  }
}

// taps = 5: two k-steps of the streamed image instead of the resident one
static void conv1d_x3_layout(int T, int cin, int mt, int terms, int* offW, int* total, int* slab_floats, int taps = 3) {
  const int sl = 16 * T + 8;
  *slab_floats = sl;
  *offW = (2 * sl * 4 + 255) & ~255;
  *total = *offW + (taps == 5 ? 2 * 5 : mt * 3 * cnn1d_x3_nks(cin)) * terms * 64 * 16;
}
// channel tiles per workgroup: two when the layer has them and their fragments fit beside the slabs; mode 2 (diagnostic) forces one
static int conv1d_x3_mt(int T, int cin, int cout, int terms, int mode) {
  if (mode == 2 || cout % 64 != 0) return 1;
  int offW, total, sl;
  conv1d_x3_layout(T, cin, 2, terms, &offW, &total, &sl);
  return total <= 160 * 1024 ? 2 : 1;
}

// taps = 5 (layer 1 of the k = (5, 3, 3) variant): Cout = 32 only
bool conv1d_x3_supports(const float* x, int64_t sb, int64_t sc, int64_t st, const float* z, int T, int Cin, int Cout, int terms, int taps) {
  if (taps != 3 && (taps != 5 || Cout != 32)) return false;
  if (T < 3 || T > 384 || (T + 31) / 32 > c1x::NW * c1x::MAXT1 || Cin < 1 || (Cin & 3) || Cout < 32 || (Cout & 31)) return false;
  if (st != 1 || sc != T || (sb & 3) || ((uintptr_t)x & 15) || ((uintptr_t)z & 3)) return false;
  if ((cnn1d_x3_nks(Cin) & 1) || (terms != 2 && terms != 3)) return false;
  int offW, total, sl;
  conv1d_x3_layout(T, Cin, 1, terms, &offW, &total, &sl, taps);
  return total <= 160 * 1024;
}

// taps = 5: wx is the k-step-major five-tap image of launch_pack_conv1d_train_all(..., k1 = 5); Cout = 32, no lens
hipError_t launch_conv1d_x3(const float* x, int64_t sb, const void* wx, const float* bias, float* z, int B, int Cin, int Cout, int T,
                            int terms, hipStream_t s, int mode, const AugCfg* aug, const int* lens, int taps) {
  if (taps != 3 && (taps != 5 || Cout != 32 || lens)) return hipErrorInvalidValue;
  Conv1dX3Args a{};
  if (aug && aug->on) a.aug = *aug;
  a.lens = lens;
  a.x = x; a.sb = sb; a.w = (const uint4*)wx; a.bias = bias; a.z = z; a.T = T; a.Cin = Cin; a.Cout = Cout;
  a.NT = (T + 31) / 32; a.nks = cnn1d_x3_nks(Cin);
  const int mt = conv1d_x3_mt(T, Cin, Cout, terms, mode);           // (one at Cout = 32)
  int total;
  conv1d_x3_layout(T, Cin, mt, terms, &a.offW, &total, &a.slab_floats, taps);
  auto go = [&](auto kern) { return launch_lds(kern, dim3(B, Cout / (32 * mt)), dim3(c1x::NTH), total, s, a); };
  if (lens) {                     // ragged layer 1 (one channel tile), never with an augmentation
    if (mt != 1 || a.aug.on) return hipErrorInvalidValue;
    return terms == 3 ? go(conv1d_x3_kernel<1, 3, false, true>) : go(conv1d_x3_kernel<1, 2, false, true>);
  }
  if (a.aug.on) {                 // layer 1 only (one channel tile)
    if (mt != 1) return hipErrorInvalidValue;
    if (taps == 5) return terms == 3 ? go(conv1d_x3_kernel<1, 3, true, false, 5>) : go(conv1d_x3_kernel<1, 2, true, false, 5>);
    return terms == 3 ? go(conv1d_x3_kernel<1, 3, true>) : go(conv1d_x3_kernel<1, 2, true>);
  }
  if (taps == 5) return terms == 3 ? go(conv1d_x3_kernel<1, 3, false, false, 5>) : go(conv1d_x3_kernel<1, 2, false, false, 5>);
  if (terms == 3) return mt == 2 ? go(conv1d_x3_kernel<2, 3>) : go(conv1d_x3_kernel<1, 3>);
  return mt == 2 ? go(conv1d_x3_kernel<2, 2>) : go(conv1d_x3_kernel<1, 2>);
}

}  // namespace dfa

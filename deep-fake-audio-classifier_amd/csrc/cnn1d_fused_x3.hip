// cnn1d_fused_x3.hip -- the CNN1D eval forward (src/model_cnn1d.py:37-46) as ONE kernel on the bf16 matrix cores at fp32-grade
// accuracy: every weight and activation is carried as hi + lo bf16 (16 significant bits), every product is three
// v_mfma_f32_32x32x16_bf16 (hi*hi + lo*hi + hi*lo, fp32 accumulate; the dropped lo*lo term is 2^-18 of a product) -- the
// DFA_PREC_BF16X3 construction of conv_split.hip.  The exact-fp32 form (cnn1d_fused.hip, v_mfma_f32_32x32x2_f32) is held at
// ~80 cycles per 2048 MACs by the fp32 matrix pipe (2172 MFMAs = 174 k cycles per utterance, 85 us per 256 utterances); the same
// MACs cost 3 x 32 cycles per 16384 here, so the kernel is bound by moving and splitting x instead.
//   * workgroup = one utterance, 8 waves (two per SIMD); x is read ONCE with aligned 16-byte loads: the reference stores [F][T] contiguously
//     (src/dataset.py:52), so 16 input channels = one contiguous, 16-byte aligned slab of 16 T floats; a slab passes through LDS as
//     it is (fp32, [channel][frame]) and is split ONCE into a pixel image [frame + 1][hi 16 ch | lo 16 ch] (bf16, 64 bytes per frame,
//     swizzled, zero halo): the lane that owns frame t reads the B fragments of its three taps as two ds_read_b128 each (the layer-1
//     comment in the kernel has the pipeline);
//   * its weights (72 KB of A fragments) sit in LDS for the layer;
//   * h1 [T][32] and h2 [T][64] live in LDS channels-last as [hi: C bf16][lo: C bf16] pixels with the chunk swizzle of
//     conv3x3_mfma.h, written from the accumulator layout as 8-byte stores (4 consecutive channels of one frame per lane),
//     read as ds_read_b128 fragments at frame t + tap - 1; layers 2 and 3 keep their hi / lo A fragments in registers;
//   * frame mean and the 128 -> 1 classifier in the epilogue, as in cnn1d_fused.hip: logits[b] is the only global write.
// LDS: two fp32 slabs + two split images + layer-1 weights during layer 1 (156.5 KB at T = 321), then h1 and h2 over the same space.
// Takes the reference's storage only (x[b][f][t] contiguous, 16-byte aligned, F % 4 == 0, 3 <= T <= 347 at F = 180: the LDS budget); anything else runs
// cnn1d_fused.hip / the three-launch path (cnn1d_api.hip).
// A variable-length batch padded to its longest utterance runs cnn1d_ragged_x3_kernel (dfa_cnn1d_forward_ragged): the same body
// (cnn1d_x3_body.h) with the utterance's own length from a device table, rows read at the batch's pitch, and utterances longer
// than one LDS window walked in time segments inside their workgroup.
// This file is the eval forward only; the training step's layer kernel, layer 1 of this one generalised, is conv1d_x3.hip, and
// what the two share is cnn1d_x3_common.h.
#include "cnn1d_x3_common.h"

namespace dfa {

// A-fragment images: wx[m][tap][ks][part][lane] (uint4), part 0 = hi, 1 = lo; lane: co = 32 m + (lane & 31), element j <-> input
// channel 16 ks + 8 (lane >> 5) + j (zero beyond cin).  wf = BN-folded fp32 weights [cout][cin][taps].  taps = 5 (layer 1 of the
// k = (5, 3, 3) variant, whose image is streamed one k-step per trip): k-step-major, wx[m][ks][tap][part][lane] (cnn1d_x3_frag_slot).
__global__ void pack_cnn1d_x3_kernel(const float* __restrict__ wf, uint4* __restrict__ wx, int cin, int cout, int nks, int taps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int total = (cout / 32) * taps * nks * 64;
  if (i >= total) return;
  const int lane = i & 63;
  int rest = i >> 6;
  const int ks = rest % nks; rest /= nks;
  const int tap = rest % taps, m = rest / taps;
  const int co = 32 * m + (lane & 31), hh = lane >> 5;
  bf16_t hi[8], lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = 16 * ks + 8 * hh + j;
    const float w = ci < cin ? wf[((size_t)co * cin + ci) * taps + tap] : 0.f;
    hi[j] = float_to_bf16(w);
    lo[j] = float_to_bf16(w - bf16_to_float(hi[j]));
  }
  uint4* dst = wx + ((size_t)cnn1d_x3_frag_slot(m, tap, ks, taps, nks) * 2) * 64 + lane;
  dst[0] = *reinterpret_cast<const uint4*>(hi);
  dst[64] = *reinterpret_cast<const uint4*>(lo);
}

size_t cnn1d_x3_pack_bytes(int cin, int cout, int taps) { return (size_t)(cout / 32) * taps * cnn1d_x3_nks(cin) * 2 * 64 * 16; }
// taps = 5 (layer 1 of the k = (5, 3, 3) variant) packs the k-step-major image the five-tap kernels stream
hipError_t launch_pack_cnn1d_x3(const float* wf, void* wx, int cin, int cout, hipStream_t s, int taps) {
  const int total = (cout / 32) * taps * cnn1d_x3_nks(cin) * 64;
  hipLaunchKernelGGL(pack_cnn1d_x3_kernel, dim3((total + 255) / 256), dim3(256), 0, s, wf, (uint4*)wx, cin, cout, cnn1d_x3_nks(cin), taps);
  return hipGetLastError();
}

struct Cnn1dX3Args {
  const float* x;              // [B][F][T] contiguous, 16-byte aligned
  const uint4 *w1, *w2, *w3;   // hi / lo A-fragment images of the three layers
  const float *b1, *b2, *b3, *cw, *cb;
  float* logits;
  int T, F, NT, nks1;          // NT = ceil(T / 32), nks1 = ceil(F / 16)
  int offA_h1, offB;           // LDS byte offsets: [0, offS) two fp32 slabs, [offS, offB) two split images, [offB, ...) layer-1 weights;
  int offS, offH2;             // after layer 1: h1 at 0, h2 at offH2
  int slab_floats;             // 16 T + 8
  long long* stamps;
};

// one 32-frame tile of a layer whose input lives in LDS as split pixels: acc = sum over (tap, ks) of the three split products.
// PB = pixel bytes (4 * CIN), NKS = CIN / 16; lane reads pixel slot t + tap, chunks 2 ks + h (hi) and CIN / 8 + 2 ks + h (lo).
// The fragment reads run PD steps ahead of their MFMAs through a rotating register queue and `side(i)` -- a slice of the PREVIOUS
// tile's epilogue -- is issued in the shadow of step i's three MFMAs; sched_barrier pins that order (left alone, hipcc puts each
// ds_read_b128 directly in front of its MFMA and the whole epilogue between two tiles: stamps showed layers 2 / 3 at 3.6x / 2.1x
// their matrix-pipe time).
template <int CIN, typename Side>
__device__ __forceinline__ void split_gemm(const uint4 (&wh)[3 * (CIN / 16)], const uint4 (&wl)[3 * (CIN / 16)], const char* img, int t0,
                                           int col, int h, f32x16_t& acc, Side side) {
  constexpr int PB = 4 * CIN, NKS = CIN / 16, NS = 3 * NKS, PD = CIN >= 64 ? 2 : 3;   // (layer 3 holds 96 weight registers: a shorter queue)
  const char* px[3];
  int sw[3];
#pragma unroll
  for (int tap = 0; tap < 3; ++tap) {
    const int slot = t0 + col + tap;
    sw[tap] = lds_swz<PB>(slot);
    px[tap] = img + slot * PB;
  }
  uint4 qh[PD], ql[PD];
  auto rd = [&](int i, uint4& xh, uint4& xl) {
    const int tap = i / NKS, ks = i % NKS;
    xh = *(const uint4*)(px[tap] + (((2 * ks + h) ^ sw[tap]) << 4));
    xl = *(const uint4*)(px[tap] + (((CIN / 8 + 2 * ks + h) ^ sw[tap]) << 4));
  };
#pragma unroll
  for (int i = 0; i < PD; ++i) rd(i, qh[i], ql[i]);
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const uint4 xh = qh[i % PD], xl = ql[i % PD];
    if (i + PD < NS) rd(i + PD, qh[i % PD], ql[i % PD]);
    acc = mma32(wh[i], xh, acc);
    acc = mma32(wl[i], xh, acc);
    acc = mma32(wh[i], xl, acc);
    side(i);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// bias + ReLU + hi / lo split of one accumulator -> the split image of the next layer (COUT channels per pixel); frames >= T are
// stored as zeros (the next layer's right-hand padding); lane = frame, registers 4 g .. 4 g + 3 = channels co0 + 8 g + 4 h + (0..3)
template <int COUT>
__device__ __forceinline__ void store_split_g(const f32x16_t& acc, const float* bias, int co0, char* img, int t, int T, int h, int g) {
  constexpr int PB = 4 * COUT;
  const int slot = t + 1, sw = lds_swz<PB>(slot);
  char* px = img + slot * PB;
  const int co = co0 + 8 * g + 4 * h;
  const float4 bv = *(const float4*)(bias + co);
  float v[4] = {fmaxf(acc[4 * g] + bv.x, 0.f), fmaxf(acc[4 * g + 1] + bv.y, 0.f), fmaxf(acc[4 * g + 2] + bv.z, 0.f), fmaxf(acc[4 * g + 3] + bv.w, 0.f)};
  if (t >= T) v[0] = v[1] = v[2] = v[3] = 0.f;
  const unsigned h0 = pack_bf16x2(v[0], v[1]), h1 = pack_bf16x2(v[2], v[3]);
  const unsigned l0 = pack_bf16x2(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xffff0000u));
  const unsigned l1 = pack_bf16x2(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xffff0000u));
  const int c = co >> 3;
  *(uint2*)(px + ((c ^ sw) << 4) + 8 * h) = make_uint2(h0, h1);
  *(uint2*)(px + (((COUT / 8 + c) ^ sw) << 4) + 8 * h) = make_uint2(l0, l1);
}
template <int COUT>
__device__ __forceinline__ void store_split(const f32x16_t& acc, const float* bias, int co0, char* img, int t, int T, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g) store_split_g<COUT>(acc, bias, co0, img, t, T, h, g);
}

// LDS layout of one utterance (uniform kernel) or one time window (ragged kernel) of T frames.  ragged: a slab's rows sit at a
// pitch of T rounded up to 4 floats (rows of the padded batch are loaded 16 bytes at a time), otherwise at T (contiguous slab).
// Host and device: the ragged kernel asks it per segment, its launch for the largest window.
// k1 = taps of layer 1.  3: its whole A-fragment image sits behind the split images.  5 (the k = (5, 3, 3) variant): the image
// (120 KB at F = 180) does not fit beside the slabs, so only TWO k-steps of it (5 taps x 2 parts x 1 KB each) are resident and the
// kernel streams the rest with the slabs; the split images carry a two-frame halo.
__host__ __device__ inline void cnn1d_x3_layout(int T, int F, int ragged, int* offB, int* total, int* slab_floats, int* offS = nullptr,
                                                int* offH2 = nullptr, int k1 = 3) {
  const int NT = (T + 31) / 32, nslots = 32 * NT + 2, nks1 = cnn1d_x3_nks(F);
  const int SL = 16 * (ragged ? (T + 3) & ~3 : T) + 8;
  const int oS = (2 * SL * 4 + 255) / 256 * 256;                       // two fp32 slabs
  const int oB = (oS + 2 * (nslots + (k1 == 5 ? 2 : 0)) * 64 + 255) / 256 * 256;             // two split images
  const int oH2 = (nslots * 128 + 255) / 256 * 256;                    // h1, then h2
  const int l1 = oB + (k1 == 5 ? 2 * 5 : 3 * nks1) * 2 * 64 * 16, l23 = oH2 + nslots * 256 + 64;
  *offB = oB;
  *total = l1 > l23 ? l1 : l23;
  *slab_floats = SL;
  if (offS) *offS = oS;
  if (offH2) *offH2 = oH2;
}

// ---- the segment plan of the ragged kernel: a function of the utterance's length T, the feature count F (through wcap and
// seg_step) and nothing else, so an utterance's logit does not depend on its batch.
//   wcap     = the longest window whose layout fits the 160 KiB of a workgroup (cnn1d_ragged_wcap);
//   seg_step = the frames a segment owns when T > wcap: the largest multiple of 4 with seg_step + 7 <= wcap.
// T <= wcap: one segment, window = owned = [0, T) -- the uniform kernel's work.  Otherwise segment i owns
// [i seg_step, min(T, (i + 1) seg_step)) and its window runs from 4 frames before (a multiple of 4: the 16-byte row loads stay
// aligned; layer 3 needs 3) to 3 frames behind the owned range, both clipped to [0, T).
__host__ __device__ inline int cnn1d_ragged_nseg(int T, int seg_step, int wcap) { return T <= wcap ? 1 : (T + seg_step - 1) / seg_step; }
// -> window start w0 and length W in the utterance, owned frames [olo, ohi) in WINDOW coordinates
// back = the frames a window runs on behind its owned range: 3 (three-tap layers: 1 + 1 + 1), 4 with a five-tap layer 1 (2 + 1 + 1)
__host__ __device__ inline void cnn1d_ragged_segment(int T, int seg_step, int wcap, int seg, int* w0, int* W, int* olo, int* ohi, int back = 3) {
  if (T <= wcap) { *w0 = 0; *W = T; *olo = 0; *ohi = T; return; }
  const int lo = seg * seg_step, hi = lo + seg_step < T ? lo + seg_step : T;
  const int ws = lo >= 4 ? lo - 4 : 0, we = hi + back < T ? hi + back : T;
  *w0 = ws; *W = we - ws; *olo = lo - ws; *ohi = hi - ws;
}
// the longest T whose layout fits the 160 KiB of a workgroup (0: none)
static int cnn1d_x3_longest_t(int F, int ragged, int k1) {
  int best = 0;
  for (int T = 3; T <= 384 && (T + 31) / 32 <= c1x::NW * c1x::MAXT1; ++T) {   // (a slab's 16 rows of ceil(T / 4) float4 fit the 3 x 512 loads of a trip)
    int offB, total, sl;
    cnn1d_x3_layout(T, F, ragged, &offB, &total, &sl, nullptr, nullptr, k1);
    if (total <= 160 * 1024) best = T;   // (the layout grows with T)
  }
  return best;
}
int cnn1d_ragged_wcap(int F, int k1) { return cnn1d_x3_longest_t(F, 1, k1); }
int cnn1d_ragged_seg_step(int F, int k1) { return (cnn1d_ragged_wcap(F, k1) - (k1 == 5 ? 8 : 7)) & ~3; }

// what the ragged form takes beside Cnn1dX3Args (whose x is then the padded batch and whose T / NT / LDS offsets are unused)
struct Cnn1dRaggedArgs {
  RaggedTab rt;                // [0, B): lengths, [B, 2B): dispatch order (conv3x3_mfma.h)
  long long stride_b;          // floats between utterances (a multiple of 4)
  int stride_f;                // floats between the rows of an utterance (a multiple of 4, >= T_max)
  int seg_step, wcap;          // the segment plan's two constants (functions of F)
};

#define DFA_KERNEL_BODY_SCOPE   // the kernel bodies below include cnn1d_x3_body.h
// C1X_K1 = taps of layer 1.  With 3 the body must stay, token for token, what it was before the five-tap form existed -- the two
// kernels below are held to the same instructions -- so everything five taps add sits under `#if C1X_K1 == 5`,
// and the one name both forms share, `nslots1` (slots of a split image), is a #define of `nslots` in the three-tap body rather
// than a second variable: an `int nslots1 = nslots` changed the order of hipcc's scalar address arithmetic.  Keep it a macro.
#define C1X_K1 3
__global__ __launch_bounds__(512) void cnn1d_fused_x3_kernel(Cnn1dX3Args a) {
#define C1X_RAGGED 0
#include "cnn1d_x3_body.h"
#undef C1X_RAGGED
}

// Variable-length batch (dfa_cnn1d_forward_ragged): workgroup i scores utterance order[i] of the ragged table, of its own
// length T_b, from rows at the pitch of the batch padded to T_max.  The arithmetic is the uniform kernel's; an utterance that
// fits one window takes exactly its path, a longer one is walked in segments (cnn1d_x3_body.h).
__global__ __launch_bounds__(512) void cnn1d_ragged_x3_kernel(Cnn1dX3Args a, Cnn1dRaggedArgs rg) {
#define C1X_RAGGED 1
#include "cnn1d_x3_body.h"
#undef C1X_RAGGED
}
#undef C1X_K1

// The k = (5, 3, 3) variant (the reference's src/compare_kernels.py:38-67): layer 1 has five taps and padding 2, layers 2 and 3
// are the three-tap ones.  Same body; what C1X_K1 = 5 changes is layer 1 alone -- a two-frame halo in the split images, five
// fragment pairs per frame tile, and the A fragments STREAMED: the k-step-major image (pack_cnn1d_x3_kernel, taps = 5) passes
// through two 10 KB LDS buffers, k-step s + 1 parked while k-step s is computed, k-step s + 2 in flight in registers -- the
// slabs' own pipeline, one barrier per trip as before.  a.w1 = that image, a.nks1 k-steps of 640 uint4.
#define C1X_K1 5
__global__ __launch_bounds__(512) void cnn1d_fused_x3_k5_kernel(Cnn1dX3Args a) {
#define C1X_RAGGED 0
#include "cnn1d_x3_body.h"
#undef C1X_RAGGED
}
__global__ __launch_bounds__(512) void cnn1d_ragged_x3_k5_kernel(Cnn1dX3Args a, Cnn1dRaggedArgs rg) {
#define C1X_RAGGED 1
#include "cnn1d_x3_body.h"
#undef C1X_RAGGED
}
#undef C1X_K1
#undef DFA_KERNEL_BODY_SCOPE


// x must be the contiguous [B][F][T] storage (element (b, t, f) at b F T + f T + t), 16-byte aligned
bool cnn1d_fused_x3_supports(const FeatView& v, int k1) {
  const int T = v.T, F = v.F;
  // (a slab of 16 channels = 4 T float4 must fit the 3 x 512 loads of a trip: T <= 384)
  if (T < 3 || T > 384 || (T + 31) / 32 > c1x::NW * c1x::MAXT1 || F < 1 || (F & 3)) return false;
  if (v.st != 1 || v.sf != T || v.sb != (int64_t)F * T || ((uintptr_t)v.x & 15)) return false;
  int offB, total, sl;
  cnn1d_x3_layout(T, F, 0, &offB, &total, &sl, nullptr, nullptr, k1);
  return total <= 160 * 1024;
}
// the longest utterance the one-kernel form takes at F features (0: none), the bound cnn1d_fused_x3_supports applies
int cnn1d_fused_x3_max_t(int F, int k1) { return cnn1d_x3_longest_t(F, 0, k1); }

hipError_t launch_cnn1d_fused_x3(const float* x, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                                 const float* b3, const float* cw, const float* cb, float* logits, int B, int T, int F, hipStream_t s,
                                 long long* stamps, int k1) {
  Cnn1dX3Args a{};
  a.x = x; a.w1 = (const uint4*)w1; a.w2 = (const uint4*)w2; a.w3 = (const uint4*)w3; a.b1 = b1; a.b2 = b2; a.b3 = b3; a.cw = cw; a.cb = cb;
  a.logits = logits; a.T = T; a.F = F; a.NT = (T + 31) / 32; a.nks1 = cnn1d_x3_nks(F); a.stamps = stamps;
  int total;
  cnn1d_x3_layout(T, F, 0, &a.offB, &total, &a.slab_floats, &a.offS, &a.offH2, k1);
  if (k1 == 5) return launch_lds(cnn1d_fused_x3_k5_kernel, dim3(B), dim3(c1x::NTH), total, s, a);
  return launch_lds(cnn1d_fused_x3_kernel, dim3(B), dim3(c1x::NTH), total, s, a);
}

// ---- ragged launch: x = the padded batch (element (b, f, t) at b stride_b + f stride_f + t), tab = the device table
size_t cnn1d_ragged_lds_bytes(int T_max, int F, int k1) {
  int offB, total, sl;
  cnn1d_x3_layout(std::min(T_max, cnn1d_ragged_wcap(F, k1)), F, 1, &offB, &total, &sl, nullptr, nullptr, k1);
  return (size_t)total;
}
// the plan as the kernel walks it (tests, tools): fills up to cap entries, returns the number of segments
int cnn1d_ragged_segments(int T, int F, int* starts, int* lens, int* owned_lo, int* owned_hi, int cap, int k1) {
  const int wcap = cnn1d_ragged_wcap(F, k1), step = cnn1d_ragged_seg_step(F, k1);
  if (T < 3 || wcap < 11 || step < 4) return 0;
  const int n = cnn1d_ragged_nseg(T, step, wcap);
  for (int i = 0; i < n && i < cap; ++i) {
    int w0, W, lo, hi;
    cnn1d_ragged_segment(T, step, wcap, i, &w0, &W, &lo, &hi, k1 == 5 ? 4 : 3);
    if (starts) starts[i] = w0;
    if (lens) lens[i] = W;
    if (owned_lo) owned_lo[i] = w0 + lo;
    if (owned_hi) owned_hi[i] = w0 + hi;
  }
  return n;
}
hipError_t launch_cnn1d_ragged_x3(const float* x, int64_t stride_b, int64_t stride_f, const int* tab, const void* w1, const float* b1,
                                  const void* w2, const float* b2, const void* w3, const float* b3, const float* cw, const float* cb,
                                  float* logits, int B, int T_max, int F, hipStream_t s, long long* stamps, int k1) {
  Cnn1dX3Args a{};
  a.x = x; a.w1 = (const uint4*)w1; a.w2 = (const uint4*)w2; a.w3 = (const uint4*)w3; a.b1 = b1; a.b2 = b2; a.b3 = b3; a.cw = cw; a.cb = cb;
  a.logits = logits; a.F = F; a.nks1 = cnn1d_x3_nks(F); a.stamps = stamps;
  Cnn1dRaggedArgs rg{};
  rg.rt = RaggedTab{tab, B};
  rg.stride_b = stride_b; rg.stride_f = (int)stride_f;
  rg.wcap = cnn1d_ragged_wcap(F, k1); rg.seg_step = cnn1d_ragged_seg_step(F, k1);
  if (rg.wcap < 11 || rg.seg_step < 4) return hipErrorInvalidValue;
  const size_t total = cnn1d_ragged_lds_bytes(T_max, F, k1);
  if (k1 == 5) return launch_lds(cnn1d_ragged_x3_k5_kernel, dim3(B), dim3(c1x::NTH), total, s, a, rg);
  return launch_lds(cnn1d_ragged_x3_kernel, dim3(B), dim3(c1x::NTH), total, s, a, rg);
}

}  // namespace dfa

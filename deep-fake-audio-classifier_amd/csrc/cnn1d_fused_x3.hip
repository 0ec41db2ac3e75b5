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
#include "dfa_internal.h"
#include "conv3x3_mfma.h"
#include "rng.h"

namespace dfa {
namespace c1x {
constexpr int TW = 32, NW = 8, NTH = 64 * NW, MAXT1 = 2;   // 8 waves = two per SIMD (one wave's VALU / LDS work under the other's MFMAs); layer 1: tiles w, w + 8
}

// A-fragment images: wx[m][tap][ks][part][lane] (uint4), part 0 = hi, 1 = lo; lane: co = 32 m + (lane & 31), element j <-> input
// channel 16 ks + 8 (lane >> 5) + j (zero beyond cin).  wf = BN-folded fp32 weights [cout][cin][taps].  ksmajor (the five-tap
// layer 1, whose image is streamed one k-step per trip): wx[m][ks][tap][part][lane], a k-step's taps contiguous.
__global__ void pack_cnn1d_x3_kernel(const float* __restrict__ wf, uint4* __restrict__ wx, int cin, int cout, int nks, int taps, int ksmajor) {
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
  uint4* dst = wx + ((size_t)(ksmajor ? (m * nks + ks) * taps + tap : (m * taps + tap) * nks + ks) * 2) * 64 + lane;
  dst[0] = *reinterpret_cast<const uint4*>(hi);
  dst[64] = *reinterpret_cast<const uint4*>(lo);
}

// k-steps of 16 input channels; layer 1 (the only layer with cin != 32, 64) runs its slabs two per loop trip: padded to an even count
int cnn1d_x3_nks(int cin) { const int n = (cin + 15) / 16; return (cin == 32 || cin == 64) ? n : (n + 1) & ~1; }
size_t cnn1d_x3_pack_bytes(int cin, int cout, int taps) { return (size_t)(cout / 32) * taps * cnn1d_x3_nks(cin) * 2 * 64 * 16; }
// taps = 5 (layer 1 of the k = (5, 3, 3) variant) packs the k-step-major image the five-tap kernels stream
hipError_t launch_pack_cnn1d_x3(const float* wf, void* wx, int cin, int cout, hipStream_t s, int taps) {
  const int total = (cout / 32) * taps * cnn1d_x3_nks(cin) * 64;
  hipLaunchKernelGGL(pack_cnn1d_x3_kernel, dim3((total + 255) / 256), dim3(256), 0, s, wf, (uint4*)wx, cin, cout, cnn1d_x3_nks(cin), taps,
                     taps == 5 ? 1 : 0);
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

__device__ __forceinline__ uint4 and4(unsigned m, const uint4& v) { return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m); }   // (a select here became an exec branch)

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
__host__ __device__ inline int cnn1d_x3_nks_hd(int cin) { const int n = (cin + 15) / 16; return (cin == 32 || cin == 64) ? n : (n + 1) & ~1; }
// k1 = taps of layer 1.  3: its whole A-fragment image sits behind the split images.  5 (the k = (5, 3, 3) variant): the image
// (120 KB at F = 180) does not fit beside the slabs, so only TWO k-steps of it (5 taps x 2 parts x 1 KB each) are resident and the
// kernel streams the rest with the slabs; the split images carry a two-frame halo.
__host__ __device__ inline void cnn1d_x3_layout(int T, int F, int ragged, int* offB, int* total, int* slab_floats, int* offS = nullptr,
                                                int* offH2 = nullptr, int k1 = 3) {
  const int NT = (T + 31) / 32, nslots = 32 * NT + 2, nks1 = cnn1d_x3_nks_hd(F);
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
int cnn1d_ragged_wcap(int F, int k1) {
  int w = 0;
  for (int T = 3; T <= 384 && (T + 31) / 32 <= c1x::NW * c1x::MAXT1; ++T) {   // (a slab's 16 rows of ceil(T / 4) float4 fit the 3 x 512 loads of a trip)
    int offB, total, sl;
    cnn1d_x3_layout(T, F, 1, &offB, &total, &sl, nullptr, nullptr, k1);
    if (total <= 160 * 1024) w = T;      // (the layout grows with T)
  }
  return w;
}
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
// fragment pairs per frame tile, and the A fragments STREAMED: the k-step-major image (pack_cnn1d_x3_kernel, ksmajor) passes
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
// ---- one Conv1d(k = 3, pad 1) layer of the TRAINING step on the matrix cores (src/train.py:71-76 through
// src/model_cnn1d.py:17-34): z[b][co][t] = bias[co] + sum_{ci, k} W[co][ci][k] in[b][ci][t + k - 1], channel-major fp32 in and
// out, no BatchNorm / ReLU (train mode: batch statistics come first).  It serves the three forward convolutions and -- on the
// flipped / transposed weight image of conv1d_dgrad_pack_kernel -- the two data gradients.  Layer 1 of the fused kernel above,
// generalised: a workgroup = (utterance, MT tiles of 32 output channels); 16-channel slabs of the input go through LDS as they are
// (contiguous 16 T floats, 16-byte loads, two slabs ahead), the lane that owns frame t splits x[c][t-1..t+1] of its 8 channels
// into bf16 B fragments ONCE per slab and tap and feeds them to every channel tile; this layer's A fragments sit in LDS.
// TERMS = 3 (default): every fp32 operand = hi + lo + lo2, three bf16 terms (split8n<3>, dfa_device.h: the operand exactly), six MFMAs per product
// (all term pairs of order <= 2; the dropped ones are below 2^-24 of a product): fp32-grade sums.  TERMS = 2: the bf16x3
// construction of the eval kernel (16-bit operands, three MFMAs, ~1e-5) -- fine for inference's 1e-4 bar, but in a training step
// a 1e-5 perturbation of a pre-activation flips ~1e-5 of the ReLU masks and every flip moves a gradient by a whole element:
// relative L2 error ~ sqrt(1e-5) = 3e-3 against 3e-4 for fp32 arithmetic (tools/gpu_cnn1d_x3_probe.py), so it is opt-in.
// The fp32 VALU kernel this replaces (conv1d.hip) needs 97 us per call at [256, *, 321].
struct Conv1dX3Args {
  const float* x;              // [B] x [Cin][T] contiguous per utterance, utterance stride sb floats, 16-byte aligned
  int64_t sb;
  const uint4* w;              // pack_conv1d_train_all_kernel image [Cout / 32][3][nks][TERMS][64]
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
  int taps[5];           // 3; 5 for entry 0 of the k = (5, 3, 3) variant, whose image is k-step-major: [ks][tap][term][lane] (conv1d_x3_k5_kernel)
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
  uint4* dst = a.dst[e] + ((size_t)(taps == 5 ? (m * nks + ks) * taps + tap : (m * 3 + tap) * nks + ks) * a.terms) * 64 + lane;
  dst[0] = *reinterpret_cast<const uint4*>(t0);
  dst[64] = *reinterpret_cast<const uint4*>(t1);
  if (a.terms == 3) dst[128] = *reinterpret_cast<const uint4*>(t2);
}
// w1, w2, w3: the three Conv1d weights [32][F][3], [64][32][3], [128][64][3]; dst[0..4]: forward 1-3, data gradients 3 -> 2, 2 -> 1
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

template <int MT, int TERMS, bool AUG = false, bool RAGGED = false>
__global__ __launch_bounds__(512) void conv1d_x3_kernel(Conv1dX3Args a) {
  using namespace c1x;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int b = blockIdx.x, m0 = blockIdx.y * MT;
  const int T = a.T, NT = a.NT, nks = a.nks;
  float* const slab0 = (float*)smem;                      // two slabs of slab_floats floats: [4 pad][16 x T][4 pad]
  char* const wS = smem + a.offW;                         // this workgroup's A fragments [MT][3][nks][TERMS][64] x 16 B
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
  slab_load(0, xrA);
  slab_load(1, xrB);
  {
    const int n = MT * 3 * nks * TERMS * 64;
    const uint4* wsrc = a.w + (size_t)m0 * 3 * nks * TERMS * 64;
    for (int i = tid; i < n; i += NTH) *(uint4*)(wS + (size_t)i * 16) = wsrc[i];
    if (tid < 16) {
      const int sbuf = tid >> 3, e = tid & 7;
      slab0[sbuf * SL + (e < 4 ? e : 16 * T + e)] = 0.f;
    }
  }
  slab_store(0, xrA);
  __syncthreads();

  const int nmine = (NT - wave + NW - 1) / NW;
  unsigned tin[MAXT1][3];                                  // all-ones where tap k of this lane's frame exists, else 0
  int tl[MAXT1];
#pragma unroll
  for (int j = 0; j < MAXT1; ++j) {
    const int t = TW * (wave + NW * j) + col;
    tl[j] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) tin[j][k] = ((j < nmine) && t < T && t - 1 + k >= 0 && t - 1 + k < T) ? 0xffffffffu : 0u;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][j][r] = 0.f;
  }
  // one slab = one k-step of 16 channels: trip s computes slab s from buffer s & 1, requests slab s + 2 and parks slab s + 1
  // (requested a trip ago) in the other buffer; one barrier per trip.  Inside a trip the TAP is the outer loop: its MT x TERMS
  // weight fragments are read from LDS once and serve both of the wave's frame tiles.
  auto trip = [&](int s, float4 (&xr_next)[NLD], float4 (&xr_far)[NLD], bool load) {
    if (load) slab_load(s + 2, xr_far);
    const float* sl = slab0 + (s & 1) * SL + 4 + 8 * h * T - 1;       // this lane half's 8 channels, frame index - 1
    float v[MAXT1][3][8];
#pragma unroll
    for (int j = 0; j < MAXT1; ++j)
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[j][k][c] = sl[c * T + tl[j] + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      uint4 w[MT][TERMS];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int p = 0; p < TERMS; ++p) w[m][p] = *(const uint4*)(wS + ((size_t)((((m * 3 + k) * nks + s) * TERMS + p) * 64 + lane)) * 16);
#pragma unroll
      for (int j = 0; j < MAXT1; ++j) {
        uint4 xs[TERMS];
        split8n<TERMS>(v[j][k], xs);
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

static void conv1d_x3_layout(int T, int cin, int mt, int terms, int* offW, int* total, int* slab_floats) {
  const int sl = 16 * T + 8;
  *slab_floats = sl;
  *offW = (2 * sl * 4 + 255) & ~255;
  *total = *offW + mt * 3 * cnn1d_x3_nks(cin) * terms * 64 * 16;
}
// channel tiles per workgroup: two when the layer has them and their fragments fit beside the slabs; mode 2 (diagnostic) forces one
static int conv1d_x3_mt(int T, int cin, int cout, int terms, int mode) {
  if (mode == 2 || cout % 64 != 0) return 1;
  int offW, total, sl;
  conv1d_x3_layout(T, cin, 2, terms, &offW, &total, &sl);
  return total <= 160 * 1024 ? 2 : 1;
}

bool conv1d_x3_supports(const float* x, int64_t sb, int64_t sc, int64_t st, const float* z, int T, int Cin, int Cout, int terms) {
  if (T < 3 || T > 384 || (T + 31) / 32 > c1x::NW * c1x::MAXT1 || Cin < 1 || (Cin & 3) || Cout < 32 || (Cout & 31)) return false;
  if (st != 1 || sc != T || (sb & 3) || ((uintptr_t)x & 15) || ((uintptr_t)z & 3)) return false;
  if ((cnn1d_x3_nks(Cin) & 1) || (terms != 2 && terms != 3)) return false;
  int offW, total, sl;
  conv1d_x3_layout(T, Cin, 1, terms, &offW, &total, &sl);
  return total <= 160 * 1024;
}

hipError_t launch_conv1d_x3(const float* x, int64_t sb, const void* wx, const float* bias, float* z, int B, int Cin, int Cout, int T,
                            int terms, hipStream_t s, int mode, const AugCfg* aug, const int* lens) {
  Conv1dX3Args a{};
  if (aug && aug->on) a.aug = *aug;
  a.lens = lens;
  a.x = x; a.sb = sb; a.w = (const uint4*)wx; a.bias = bias; a.z = z; a.T = T; a.Cin = Cin; a.Cout = Cout;
  a.NT = (T + 31) / 32; a.nks = cnn1d_x3_nks(Cin);
  const int mt = conv1d_x3_mt(T, Cin, Cout, terms, mode);
  int total;
  conv1d_x3_layout(T, Cin, mt, terms, &a.offW, &total, &a.slab_floats);
  auto go = [&](auto kern) { return launch_lds(kern, dim3(B, Cout / (32 * mt)), dim3(c1x::NTH), total, s, a); };
  if (lens) {                     // ragged layer 1 (one channel tile), never with an augmentation
    if (mt != 1 || a.aug.on) return hipErrorInvalidValue;
    return terms == 3 ? go(conv1d_x3_kernel<1, 3, false, true>) : go(conv1d_x3_kernel<1, 2, false, true>);
  }
  if (a.aug.on) {                 // layer 1 only (one channel tile)
    if (mt != 1) return hipErrorInvalidValue;
    return terms == 3 ? go(conv1d_x3_kernel<1, 3, true>) : go(conv1d_x3_kernel<1, 2, true>);
  }
  if (terms == 3) return mt == 2 ? go(conv1d_x3_kernel<2, 3>) : go(conv1d_x3_kernel<1, 3>);
  return mt == 2 ? go(conv1d_x3_kernel<2, 2>) : go(conv1d_x3_kernel<1, 2>);
}


// ---- layer 1 of the k = (5, 3, 3) variant's training step: Conv1d(k = 5, pad 2), F -> 32, the kernel above with five taps and
// one channel tile.  Its image -- 5 taps x nks x TERMS KB, 180 KB at F = 180 with three terms -- has no resident form, so it is
// STREAMED as in the eval kernel (cnn1d_x3_body.h, C1X_K1 = 5): packed k-step-major (pack_conv1d_train_all_kernel, ksmajor), one
// k-step's [5 taps][TERMS][64 lanes] fragments (15 KB / 10 KB) pass through two LDS buffers -- k-step s + 1 is parked while k-step s
// is computed, k-step s + 2 is in flight in two registers -- on the slabs' own barrier.  A function of its own, so that the
// three-tap instantiations above keep their text.  The lane splits x[c][t - 2 .. t + 2] per tap inside the tap loop (16 values live
// instead of 80).
template <int TERMS, bool AUG>
__global__ __launch_bounds__(512) void conv1d_x3_k5_kernel(Conv1dX3Args a) {
  using namespace c1x;
  constexpr int K = 5, WKS = K * TERMS * 64;               // uint4 of one k-step's fragments: 960 (three terms) or 640
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int b = blockIdx.x;
  const int T = a.T, NT = a.NT, nks = a.nks;
  float* const slab0 = (float*)smem;                      // two slabs of slab_floats floats: [4 pad][16 x T][4 pad]
  char* const wS = smem + a.offW;                         // W[0], W[1]: one k-step each, [5][TERMS][64] x 16 B
  f32x16_t acc[MAXT1];
  const float4* xg = (const float4*)(a.x + (size_t)b * a.sb);
  const int SL = a.slab_floats;
  constexpr int NLD = 3;
  float4 xrA[NLD], xrB[NLD];
  const int nreal = (a.Cin + 15) / 16;
  auto slab_n4 = [&](int s) { return max(0, min(16, a.Cin - 16 * s)) * T / 4; };
  auto slab_load = [&](int s, float4 (&xr)[NLD]) {         // unconditional, clamped (as conv1d_x3_kernel)
    const int sc = min(s, nreal - 1), n4 = slab_n4(sc);
    if constexpr (AUG) {
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
  w_load(0);
  slab_load(0, xrA);
  slab_load(1, xrB);
  w_park(0);
  w_load(1);
  if (tid < 16) {
    const int sbuf = tid >> 3, e = tid & 7;
    slab0[sbuf * SL + (e < 4 ? e : 16 * T + e)] = 0.f;
  }
  slab_store(0, xrA);
  __syncthreads();

  const int nmine = (NT - wave + NW - 1) / NW;
  unsigned tin[MAXT1][K];                                  // all-ones where tap k of this lane's frame exists (t - 2 + k in [0, T)), else 0
  int tl[MAXT1];
#pragma unroll
  for (int j = 0; j < MAXT1; ++j) {
    const int t = TW * (wave + NW * j) + col;
    tl[j] = t;
#pragma unroll
    for (int k = 0; k < K; ++k) tin[j][k] = ((j < nmine) && t < T && t - 2 + k >= 0 && t - 2 + k < T) ? 0xffffffffu : 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  }
  // trip s: compute k-step s from slab buffer s & 1 and W[s & 1]; request slab s + 2; park k-step s + 1 in W[(s + 1) & 1] (last read
  // in trip s - 1, behind that trip's barrier) and request k-step s + 2; park slab s + 1; one barrier
  auto trip = [&](int s, float4 (&xr_next)[NLD], float4 (&xr_far)[NLD], bool load) {
    if (load) slab_load(s + 2, xr_far);
    const float* sl = slab0 + (s & 1) * SL + 4 + 8 * h * T - 2;       // this lane half's 8 channels, frame index - 2
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uint4 w[TERMS];
#pragma unroll
      for (int p = 0; p < TERMS; ++p) w[p] = *(const uint4*)(wS + ((size_t)((((s & 1) * K + k) * TERMS + p) * 64 + lane)) * 16);
#pragma unroll
      for (int j = 0; j < MAXT1; ++j) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = sl[c * T + tl[j] + k];
        uint4 xs[TERMS];
        split8n<TERMS>(v, xs);
#pragma unroll
        for (int p = 0; p < TERMS; ++p) xs[p] = and4(tin[j][k], xs[p]);
        if constexpr (TERMS == 3) {                        // smallest terms first
          acc[j] = mma32(w[2], xs[0], acc[j]);
          acc[j] = mma32(w[0], xs[2], acc[j]);
          acc[j] = mma32(w[1], xs[1], acc[j]);
        }
        acc[j] = mma32(w[1], xs[0], acc[j]);
        acc[j] = mma32(w[0], xs[1], acc[j]);
        acc[j] = mma32(w[0], xs[0], acc[j]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    w_park(s + 1);
    w_load(s + 2);
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

  // ---- + bias, channel-major store (as conv1d_x3_kernel, channel tile 0)
  const int cb = 4 * h;
  float bv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bv[r] = a.bias[cb + (r & 3) + 8 * (r >> 2)];
#pragma unroll
  for (int j = 0; j < MAXT1; ++j) {
    const int t = tl[j];
    if (j < nmine && t < T) {
      float* zr = a.z + ((size_t)b * a.Cout + cb) * T + t;
#pragma unroll
      for (int r = 0; r < 16; ++r) zr[(size_t)((r & 3) + 8 * (r >> 2)) * T] = acc[j][r] + bv[r];
    }
  }
}

static void conv1d_x3_k5_layout(int T, int terms, int* offW, int* total, int* slab_floats) {
  const int sl = 16 * T + 8;
  *slab_floats = sl;
  *offW = (2 * sl * 4 + 255) & ~255;
  *total = *offW + 2 * 5 * terms * 64 * 16;
}
bool conv1d_x3_k5_supports(const float* x, int64_t sb, int64_t sc, int64_t st, const float* z, int T, int Cin, int Cout, int terms) {
  if (T < 3 || T > 384 || (T + 31) / 32 > c1x::NW * c1x::MAXT1 || Cin < 1 || (Cin & 3) || Cout != 32) return false;
  if (st != 1 || sc != T || (sb & 3) || ((uintptr_t)x & 15) || ((uintptr_t)z & 3)) return false;
  if ((cnn1d_x3_nks(Cin) & 1) || (terms != 2 && terms != 3)) return false;
  int offW, total, sl;
  conv1d_x3_k5_layout(T, terms, &offW, &total, &sl);
  return total <= 160 * 1024;
}
// wx: the k-step-major five-tap image of launch_pack_conv1d_train_all(..., k1 = 5)
hipError_t launch_conv1d_x3_k5(const float* x, int64_t sb, const void* wx, const float* bias, float* z, int B, int Cin, int T, int terms,
                               hipStream_t s, const AugCfg* aug) {
  Conv1dX3Args a{};
  if (aug && aug->on) a.aug = *aug;
  a.x = x; a.sb = sb; a.w = (const uint4*)wx; a.bias = bias; a.z = z; a.T = T; a.Cin = Cin; a.Cout = 32;
  a.NT = (T + 31) / 32; a.nks = cnn1d_x3_nks(Cin);
  int total;
  conv1d_x3_k5_layout(T, terms, &a.offW, &total, &a.slab_floats);
  auto go = [&](auto kern) { return launch_lds(kern, dim3(B), dim3(c1x::NTH), total, s, a); };
  if (a.aug.on) return terms == 3 ? go(conv1d_x3_k5_kernel<3, true>) : go(conv1d_x3_k5_kernel<2, true>);
  return terms == 3 ? go(conv1d_x3_k5_kernel<3, false>) : go(conv1d_x3_k5_kernel<2, false>);
}

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
int cnn1d_fused_x3_max_t(int F, int k1) {
  int best = 0;
  for (int T = 3; T <= 384 && (T + 31) / 32 <= c1x::NW * c1x::MAXT1; ++T) {
    int offB, total, sl;
    cnn1d_x3_layout(T, F, 0, &offB, &total, &sl, nullptr, nullptr, k1);
    if (total <= 160 * 1024) best = T;
  }
  return best;
}

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

// cae_dec_fused.hip -- the auto-encoder's whole decoder + reconstruction error as ONE kernel (bf16 storage mode):
//   ConvT 256->128 + BN + ReLU -> ConvT 128->64 (output_padding (0,1)) + BN + ReLU -> ConvT 64->32 + BN + ReLU -> ConvT 32->1
//   -> zero-pad T -> per-sample mean((recon - x)^2)        (src/model_cae.py:57-80,107-125; src/evaluation_cae.py:52-53).
//
// ConvTranspose2d(kernel 2, stride 2) never overlaps: a latent pixel owns its 2x2 -> 4x4 -> 8x8 -> 16x16 patch, so the three
// intermediates (d1, d2, d3: 3.2 MB per utterance written and re-read by the four-launch path, 0.55 ms of its 1.25 ms) need never
// leave the CU.  A workgroup takes 32 consecutive latent pixels of one utterance (16 KB, contiguous: channels-last) and runs the
// chain with the activations in LDS:
//   phase A  d1[128 px][128] = relu(W1 . lat)     M = 512 (q, co) x N = 32  x K = 256    256 MFMAs
//   phase B  d2[512 px][64]  = relu(W2 . d1)      M = 256         x N = 128 x K = 128    256 MFMAs
//   phase C  d3 = relu(W3 . d2) in REGISTERS      M = 128         x N = 512 x K = 64     256 MFMAs, then the 32 -> 1 layer as 64 FMAs
//            per lane on its 16 channels + one half-wave exchange, the z-scored x read through the caller's strides, and the
//            squared error -- no d3, no reconstruction in memory (recon is written only when the caller asks for it).
// v_mfma_f32_32x32x16_bf16 with the WEIGHTS as the A operand (the packed images of convt2x2_mfma.h serve unchanged: the register
// image of a B-operand column block is that of an A-operand row block) and pixels as columns: a lane then holds 4 consecutive
// channels x 4 groups of one pixel, so outputs leave as 8-byte LDS stores (the four-launch kernels store single bf16 elements).
// Pixel order is the quadtree order (child = 4 * parent + q): only phase C maps a pixel back to (t, f).  Rounding points are those
// of the four-launch path (d1, d2, d3 rounded to bf16, fp32 accumulation), so the emulated-oracle tests apply unchanged.
// The output_padding column of block 2 is a per-channel constant, and so is everything grown from it: reconstruction columns
// 16 W4 .. 16 W4 + 3 are a 4 x 4 pattern of constants (row mod 4, column) computed once at prepare time (cae_opad_consts_kernel);
// the last workgroup of an utterance adds their error and that of the zero rows t >= 16 H4.
#include "dfa_internal.h"
#include "convt2x2_mfma.h"

namespace dfa {

struct CaeDecFusedArgs {
  const bf16_t* lat;               // [B][H4*W4][256]
  const uint4 *wp1, *wp2, *wp3;    // [4*COUT/32][CIN/16][64] x 16 bytes (launch_fold_pack_convt2x2, bf16)
  const float *b1, *b2, *b3;       // folded biases [128], [64], [32]
  const float *w4, *b4;            // ConvTranspose2d(32 -> 1) weight [32][4], bias [1] (raw, fp32)
  const uint4* w4pack;             // the same weights as MFMA A operands [2 k-steps][hi, lo][64] (pack_cae_dec4_kernel)
  const float* cst;                // [16] reconstruction constants of the output_padding columns: cst[(t & 3) * 4 + (f - 16 W4)]
  const void* x;
  int x_bf16;
  int64_t sb, st, sf;
  const float *mu, *sigma;         // fused FeatureNormalizer z-score, or null
  float* recon;                    // [B][T][F] or null
  float* partial;                  // [B][ntile] squared-error sums
  int H4, W4, T, F, ntile;
  long long* stamps;               // diagnostic (context option "clock_probe"): s_memtime at the phase boundaries, workgroups (tile, b < 18)
};

namespace cdf {
#ifndef DFA_CDF_NP
#define DFA_CDF_NP 64
#endif
constexpr int NP = DFA_CDF_NP;               // latent pixels per workgroup (32 or 64)
constexpr int LAT_B = NP * 512, D1_B = 4 * NP * 256;
constexpr int B2_OFF = LAT_B + D1_B;         // [64] float: block 2's folded bias (read per unit; global loads there would serialise)
constexpr int W3_OFF = B2_OFF + 256;         // [4 q3][4 k-steps][64 lanes] x 16 B: block 3's fragments in the permuted channel order
constexpr int RED_OFF = W3_OFF + 16384;      // [8] float
constexpr int ZS_OFF = RED_OFF + 64;          // [F <= 1024][2] float: 1 / sigma, -mu / sigma (z-score table of the NORM instantiations)
constexpr int ZS_MAXF = 1024;
constexpr int LDS_BYTES = ZS_OFF + 2 * ZS_MAXF * 4;
}  // namespace cdf

__device__ __forceinline__ float cdf_ldx(const CaeDecFusedArgs& a, int b, int t, int f) {
  const int64_t off = (int64_t)b * a.sb + (int64_t)t * a.st + (int64_t)f * a.sf;
  float v = a.x_bf16 ? bf16_to_float(((const bf16_t*)a.x)[off]) : ((const float*)a.x)[off];
  if (a.mu) v = (v - a.mu[f]) / a.sigma[f];
  return v;
}

// raw x element (no branches: XBF is a template parameter, so eight of these issue back to back)
template <bool XBF>
__device__ __forceinline__ float cdf_ldraw(const void* xu, unsigned off) {   // xu = the utterance's base (uniform), off in elements
  if constexpr (XBF) return bf16_to_float(((const bf16_t*)xu)[off]);
  else return ((const float*)xu)[off];
}

// RAGGED = true (dfa_cae_score_ragged): grid = (tiles of the longest utterance, B); utterance b keeps the tile partition it has
// alone (cae_dec_fused_tiles(T_b / 16, W4) tiles of NP consecutive latent pixels), so its partial sums are those of the uniform
// call on x[b:b+1, :T_b]; they land at partial[b * a.ntile + tile].  Rows t >= T_b of x are never read.
#define DFA_KERNEL_BODY_SCOPE   // the kernel bodies below include cae_dec_fused_body.h
template <bool XBF, bool NORM>
__global__ __launch_bounds__(512, 1) void cae_dec_fused_kernel(CaeDecFusedArgs a) {
  constexpr bool RAGGED = false;
  const RaggedTab rt{};
#include "cae_dec_fused_body.h"
}

template <bool XBF, bool NORM>
__global__ __launch_bounds__(512, 1) void cae_dec_fused_ragged_kernel(CaeDecFusedArgs a, RaggedTab rt) {
  constexpr bool RAGGED = true;
#include "cae_dec_fused_body.h"
}
#undef DFA_KERNEL_BODY_SCOPE

// Reconstruction values of the columns grown from block 2's output_padding column (a per-channel constant):
//   c2[ci] = bf16(relu(b2[ci]));  c3[q3][co] = bf16(relu(b3[co] + sum_ci W3[ci][q3, co] c2[ci]))  (W3 = the bf16 MFMA image);
//   cst[(2 a3 + a4) * 4 + 2 c3 + c4] = b4 + sum_co c3[(a3, c3)][co] * W4[co][(a4, c4)].
__global__ __launch_bounds__(128) void cae_opad_consts_kernel(const float* __restrict__ b2, const uint4* __restrict__ wp3,
                                                              const float* __restrict__ b3, const float* __restrict__ w4,
                                                              const float* __restrict__ b4, float* __restrict__ cst) {
  __shared__ float c2[64], c3[4][32];
  const int tid = threadIdx.x;
  if (tid < 64) c2[tid] = bf16_to_float(float_to_bf16(fmaxf(b2[tid], 0.f)));
  __syncthreads();
  {
    const int q3 = tid >> 5, co = tid & 31;
    float s = b3[co];
    for (int ci = 0; ci < 64; ++ci) {
      const int kg = ci >> 4, hh = (ci >> 3) & 1, j = ci & 7;
      const unsigned short* frag = (const unsigned short*)(wp3 + (size_t)(q3 * 4 + kg) * 64 + co + 32 * hh);
      bf16_t w;
      w.v = frag[j];
      s = fmaf(bf16_to_float(w), c2[ci], s);
    }
    c3[q3][co] = bf16_to_float(float_to_bf16(fmaxf(s, 0.f)));
  }
  __syncthreads();
  if (tid < 16) {
    const int q3 = tid >> 2, q4 = tid & 3;
    float s = b4[0];
    for (int co = 0; co < 32; ++co) s = fmaf(c3[q3][co], w4[co * 4 + q4], s);
    const int trow = 2 * (q3 >> 1) + (q4 >> 1), fcol = 2 * (q3 & 1) + (q4 & 1);
    cst[trow * 4 + fcol] = s;
  }
}

// W4 [32 ch][4] as the A operand of v_mfma_f32_32x32x16_bf16 for "accumulator tile as the next operand": rows 0, 1 = outputs
// q4 = 0, 1 and rows 4, 5 = outputs 2, 3 (so that lane half h finds its patch row a4 = h in accumulator registers 0, 1), zero
// elsewhere; k-step s, lane half hh, element j <-> channel 16 s + 8 (j >> 2) + 4 hh + (j & 3) -- the order in which registers
// 8 s .. 8 s + 7 of a 32 x 32 accumulator hold their rows (cdna_hip_programming.md section 3).  pack[2 s + part][lane], part 0 = hi.
__global__ void pack_cae_dec4_kernel(const float* __restrict__ w4, uint4* __restrict__ pack) {
  const int i = threadIdx.x;                     // 256 = [s][part][lane]
  const int lane = i & 63, part = (i >> 6) & 1, s = i >> 7;
  const int row = lane & 31, hh = lane >> 5;
  const int q4 = row == 0 ? 0 : row == 1 ? 1 : row == 4 ? 2 : row == 5 ? 3 : -1;
  bf16_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3);
    const float w = q4 >= 0 ? w4[c * 4 + q4] : 0.f;
    const bf16_t hi = float_to_bf16(w);
    v[j] = part ? float_to_bf16(w - bf16_to_float(hi)) : hi;
  }
  pack[i] = *reinterpret_cast<const uint4*>(v);
}
hipError_t launch_pack_cae_dec4(const float* w4, uint4* pack, hipStream_t s) {
  hipLaunchKernelGGL(pack_cae_dec4_kernel, dim3(1), dim3(256), 0, s, w4, pack);
  return hipGetLastError();
}

hipError_t launch_cae_opad_consts(const float* b2, const uint4* wp3, const float* b3, const float* w4, const float* b4, float* cst,
                                  hipStream_t s) {
  hipLaunchKernelGGL(cae_opad_consts_kernel, dim3(1), dim3(128), 0, s, b2, wp3, b3, w4, b4, cst);
  return hipGetLastError();
}

// the kernel addresses x inside one utterance with unsigned 32-bit element offsets
bool cae_dec_fused_supports(const FeatView& v) {
  return v.st >= 0 && v.sf >= 0 && v.F <= cdf::ZS_MAXF && (int64_t)(v.T - 1) * v.st + (int64_t)(v.F - 1) * v.sf < ((int64_t)1 << 31);
}
// what both launches below fill alike: the packed decoder blocks, block 4, the features and their z-score
static CaeDecFusedArgs cae_dec_fused_args(const void* lat, const PackedConv* dec, const HeadParams& head, const uint4* w4pack, const float* cst,
                                          const FeatView& v, const float* mu, const float* sigma, float* partial, int H4, int W4) {
  CaeDecFusedArgs a{};
  a.w4pack = w4pack;
  a.lat = (const bf16_t*)lat; a.wp1 = dec[0].wpack; a.wp2 = dec[1].wpack; a.wp3 = dec[2].wpack;
  a.b1 = dec[0].bias; a.b2 = dec[1].bias; a.b3 = dec[2].bias; a.w4 = head.w; a.b4 = head.b; a.cst = cst;
  a.x = v.x; a.x_bf16 = v.dtype == DFA_DTYPE_BF16 ? 1 : 0; a.sb = v.sb; a.st = v.st; a.sf = v.sf; a.mu = mu; a.sigma = sigma;
  a.partial = partial; a.H4 = H4; a.W4 = W4; a.T = v.T; a.F = v.F; a.ntile = cae_dec_fused_tiles(H4, W4);
  return a;
}

int cae_dec_fused_tiles(int H4, int W4) { return (H4 * W4 + cdf::NP - 1) / cdf::NP; }

hipError_t launch_cae_dec_fused(const void* lat, const PackedConv* dec, const HeadParams& head, const uint4* w4pack, const float* cst,
                                const FeatView& v, const float* mu, const float* sigma, float* recon, float* partial, int H4, int W4,
                                hipStream_t s, long long* stamps) {
  const int B = v.B;
  CaeDecFusedArgs a = cae_dec_fused_args(lat, dec, head, w4pack, cst, v, mu, sigma, partial, H4, W4);
  a.stamps = stamps;
  a.recon = recon;
  auto go = [&](auto kern) { return launch_lds(kern, dim3(a.ntile, B), dim3(512), cdf::LDS_BYTES, s, a); };
  if (a.x_bf16) return mu ? go(cae_dec_fused_kernel<true, true>) : go(cae_dec_fused_kernel<true, false>);
  return mu ? go(cae_dec_fused_kernel<false, true>) : go(cae_dec_fused_kernel<false, false>);
}

// ragged batch, score only: H4 / T = those of the padded batch (pitches and grid extent); tab = the device table, [0, B) the lengths
hipError_t launch_cae_dec_fused_ragged(const void* lat, const PackedConv* dec, const HeadParams& head, const uint4* w4pack, const float* cst,
                                       const FeatView& v, const float* mu, const float* sigma, float* partial, int H4, int W4, const int* tab,
                                       hipStream_t s) {
  const int B = v.B;
  const CaeDecFusedArgs a = cae_dec_fused_args(lat, dec, head, w4pack, cst, v, mu, sigma, partial, H4, W4);
  const RaggedTab rt{tab, B};
  auto go = [&](auto kern) { return launch_lds(kern, dim3(a.ntile, B), dim3(512), cdf::LDS_BYTES, s, a, rt); };
  if (a.x_bf16) return mu ? go(cae_dec_fused_ragged_kernel<true, true>) : go(cae_dec_fused_ragged_kernel<true, false>);
  return mu ? go(cae_dec_fused_ragged_kernel<false, true>) : go(cae_dec_fused_ragged_kernel<false, false>);
}

}  // namespace dfa

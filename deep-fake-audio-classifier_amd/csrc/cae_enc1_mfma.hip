// cae_enc1_mfma.hip -- auto-encoder block 1 on the matrix cores (bf16 storage mode):
//   Conv2d(1, 32, 3, pad 1) + BatchNorm (folded) + ReLU + AvgPool2d(2)   (src/model_cae.py:34-37), FeatureNormalizer z-score fused
//   into the loads (src/dataset_cae.py:37-41).
// The vector-ALU kernel (cae.hip) spends 36 FMAs + 4 ReLUs per pooled output element: 4.2 G FMAs per 256 utterances, 0.157 ms at
// 35 % of the VALU peak, for 236 MB of output.  Here the 9-tap convolution is ONE K = 16 matrix product per pooled row and
// 32-column tile, the construction of conv12_fused.hip: K = 4 feature rows x (3 taps + a zero), the B operand of a lane is its
// column's window x[2q-1 .. 2q+2][f-1 .. f+1], and two A operands (weights on rows 0..2 / 1..3) give the even and the odd
// convolution row of the pool pair.  The features reach this kernel in fp32 (z-scored) and e1 is STORED in bf16: a product error
// of 2^-17 (two-term operands) moved 0.4 % of the stored e1 elements to the neighbouring bf16 value and 6 % of the latent
// (measured against the rounding-faithful oracle; the fp32 vector kernel: 2 %), so both operands are carried as THREE bf16 terms
// (hi + lo + lo2 = 24 bits) and a product is the six MFMAs whose weight is above 2^-25: every partial product is exact in the
// fp32 accumulator and only the accumulation rounds, as in the vector kernel -- 12 MFMAs per tile, still a fraction of its time.
// Epilogue in the accumulator layout (lane = column, 16 channels in registers): ReLU, vertical pair add (the pool's 1/2 rides on
// the packed weights), horizontal pair add with the neighbouring lane, bf16 pack, half-wave exchange -> every lane stores ONE
// 16-byte chunk of the pooled pixel (even columns the chunk of channels 8h.., odd columns the chunk 16 + 8h..).
// Workgroup = (utterance, 16 pooled rows, all columns): the 34 x (F + 2) feature rows go to LDS once (lanes along the
// contiguous axis of x, row pitch = 1 mod 32 floats: conflict-free stores either way); 4 waves share the 16 x ceil(F / 32) tiles.
#include "dfa_internal.h"
#include "conv3x3_mfma.h"
#include <stdlib.h>

namespace dfa {
namespace e1m {
constexpr int QG = 16, XR = 2 * QG + 2;      // pooled rows per workgroup; feature rows in LDS
}

// A operands [6][64]: even-{hi, lo, lo2}, odd-{hi, lo, lo2}; lane (channel lane & 31, half lane >> 5), element j <-> k = 8 h + j =
// 4 * (window row) + tap (tap 3 = zero); the even convolution row uses window rows 0..2, the odd one rows 1..3; the 2 x 2 pool's
// 1/4 is folded in (relu(s y) = s relu(y)).  w1 / b1: BatchNorm-folded fp32 weights [32][9] / bias [32].
__global__ void pack_cae_enc1_mfma_kernel(const float* __restrict__ w1, const float* __restrict__ b1, uint4* __restrict__ pack,
                                          float* __restrict__ bias) {
  const int i = threadIdx.x;                 // 384 threads: (operand i / 64, lane i % 64)
  if (i < 32) bias[i] = 0.25f * b1[i];
  const int op = i >> 6, lane = i & 63, ch = lane & 31, hh = lane >> 5;
  const bool odd = op >= 3;
  const int term = op % 3;
  bf16_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 8 * hh + j, dyy = k >> 2, dx = k & 3;
    const int dy = odd ? dyy - 1 : dyy;
    float wv = 0.f;
    if (dx < 3 && dy >= 0 && dy <= 2) wv = 0.25f * w1[ch * 9 + dy * 3 + dx];
    const bf16_t t0 = float_to_bf16(wv);
    const float r1 = wv - bf16_to_float(t0);
    const bf16_t t1 = float_to_bf16(r1);
    const bf16_t t2 = float_to_bf16(r1 - bf16_to_float(t1));
    v[j] = term == 0 ? t0 : (term == 1 ? t1 : t2);
  }
  pack[i] = *reinterpret_cast<const uint4*>(v);
}
hipError_t launch_pack_cae_enc1_mfma(const float* w1, const float* b1, uint4* pack, float* bias, hipStream_t s) {
  hipLaunchKernelGGL(pack_cae_enc1_mfma_kernel, dim3(1), dim3(384), 0, s, w1, b1, pack, bias);
  return hipGetLastError();
}

// RAGGED = true (dfa_cae_score_ragged): x is the batch padded to T frames, utterance b spans its first rt.tab[b] of them; rows
// t >= T_b of x are never read, pooled rows q < T_b / 2 are written at the row pitch Ho = T / 2 of the padded batch.
#define DFA_KERNEL_BODY_SCOPE   // the kernel bodies below include cae_enc1_mfma_body.h
template <typename TX>
__global__ __launch_bounds__(256) void cae_enc1_mfma_kernel(const TX* __restrict__ x, int64_t sb, int64_t st, int64_t sf,
                                                            const float* __restrict__ mu, const float* __restrict__ sigma,
                                                            const uint4* __restrict__ c1pack, const float* __restrict__ c1bias,
                                                            bf16_t* __restrict__ out, int T, int F, int Ho, int Wo, int pitch, int dbg) {
  constexpr bool RAGGED = false;
  const RaggedTab rt{};
#include "cae_enc1_mfma_body.h"
}

template <typename TX>
__global__ __launch_bounds__(256) void cae_enc1_mfma_ragged_kernel(const TX* __restrict__ x, int64_t sb, int64_t st, int64_t sf,
                                                            const float* __restrict__ mu, const float* __restrict__ sigma,
                                                            const uint4* __restrict__ c1pack, const float* __restrict__ c1bias,
                                                            bf16_t* __restrict__ out, int T, int F, int Ho, int Wo, int pitch, int dbg, RaggedTab rt) {
  constexpr bool RAGGED = true;
#include "cae_enc1_mfma_body.h"
}
#undef DFA_KERNEL_BODY_SCOPE

int cae_enc1_mfma_pitch(int F) { return (F + 2 + 31) / 32 * 32 + 1; }
size_t cae_enc1_mfma_lds(int F) { return ((size_t)e1m::XR * cae_enc1_mfma_pitch(F) + 2 * (size_t)F) * sizeof(float); }   // x rows + the z-score table

hipError_t launch_cae_enc1_mfma(const FeatView& v, const float* mu, const float* sigma, const uint4* c1pack, const float* c1bias, void* out,
                                hipStream_t s) {
  const void* x = v.x;
  const int x_dtype = v.dtype, B = v.B, T = v.T, F = v.F;
  const int64_t sb = v.sb, st = v.st, sf = v.sf;
  const int Ho = T / 2, Wo = F / 2, pitch = cae_enc1_mfma_pitch(F);
#ifdef DFA_STAMPS
  static const int dbg = getenv("DFA_E1_DBG") ? atoi(getenv("DFA_E1_DBG")) : 0;   // diagnostic build only: phase skipping (timing only)
#else
  constexpr int dbg = 0;
#endif
  const size_t lds = cae_enc1_mfma_lds(F);
  dim3 grid((Ho + e1m::QG - 1) / e1m::QG, B), block(256);
  if (x_dtype == DFA_DTYPE_BF16)
    return launch_lds(cae_enc1_mfma_kernel<bf16_t>, grid, block, lds, s, (const bf16_t*)x, sb, st, sf, mu, sigma, c1pack, c1bias, (bf16_t*)out, T, F, Ho, Wo, pitch, dbg);
  return launch_lds(cae_enc1_mfma_kernel<float>, grid, block, lds, s, (const float*)x, sb, st, sf, mu, sigma, c1pack, c1bias, (bf16_t*)out, T, F, Ho, Wo, pitch, dbg);
}

// ragged batch: T = the padded length (grid extent, output row pitch); tab = the device table, [0, B) the lengths
hipError_t launch_cae_enc1_mfma_ragged(const FeatView& v, const float* mu, const float* sigma, const uint4* c1pack, const float* c1bias,
                                       void* out, const int* tab, hipStream_t s) {
  const void* x = v.x;
  const int x_dtype = v.dtype, B = v.B, T = v.T, F = v.F;
  const int64_t sb = v.sb, st = v.st, sf = v.sf;
  const int Ho = T / 2, Wo = F / 2, pitch = cae_enc1_mfma_pitch(F);
  const size_t lds = cae_enc1_mfma_lds(F);
  const RaggedTab rt{tab, B};
  dim3 grid((Ho + e1m::QG - 1) / e1m::QG, B), block(256);
  if (x_dtype == DFA_DTYPE_BF16)
    return launch_lds(cae_enc1_mfma_ragged_kernel<bf16_t>, grid, block, lds, s, (const bf16_t*)x, sb, st, sf, mu, sigma, c1pack, c1bias, (bf16_t*)out, T, F, Ho, Wo, pitch, 0, rt);
  return launch_lds(cae_enc1_mfma_ragged_kernel<float>, grid, block, lds, s, (const float*)x, sb, st, sf, mu, sigma, c1pack, c1bias, (bf16_t*)out, T, F, Ho, Wo, pitch, 0, rt);
}

}  // namespace dfa

// train_cnn1d.hip -- training step of the 1-D CNN (src/train.py:71-76 over src/model_cnn1d.py:15-46): train-mode
// forward (Conv1d -> BatchNorm1d(batch statistics) -> ReLU -> Dropout, x3; mean over T; Linear) and its backward.
// Everything is channel-major [B][C][T] fp32 (the stored feature layout).  The whole network is 30.8 MFLOP/utt
// (about 0.3 % of the 2-D CNN): these are LDS-tiled fp32 VALU kernels bound by reading the 231 KB input, not matrix-core
// kernels.  Reductions are two-stage with a fixed order (deterministic).
#include "dfa_internal.h"
#include "bn_device.h"
#include "rng.h"

namespace dfa {

// ---- The channel-major kernels are templates on RAGGED (dfa_cnn1d_forward_train_ragged / dfa_cnn1d_backward_ragged run the
// <true> instantiations): the batch is padded to T frames, utterance b owns frames [0, lens[b]) (lens = the device table the
// forward staged; nullptr and unread in the uniform instantiation).  Sums and the time mean run over an utterance's own frames in
// the uniform loops' order, the element-wise kernels write an exact zero at every padding frame (the next convolution / weight
// gradient reads it as that utterance's zero padding).  The BatchNorm element math is bn_device.h's one-channel form.

// ---- per-channel sum / sum of squares of z[B][C][T]: one block per (channel, batch chunk) -> partial[chunk][C][2]
// shifted: the sums are those of z - k, k = the channel's first sample z[0][c][0] (the same for every chunk; bn_finalize_kernel adds
// it back to the mean).  E[z^2] - mean^2 from fp32 sums loses mean^2 / var of its 24 bits -- a channel fed by activations of large
// mean and small spread had mean^2 / var = 3000 and an invstd off by 1e-4; with the shift the ratio is that of one sample's
// distance from the mean.  Off under synchronised BatchNorm: the ranks' first samples differ and the hook carries plain sums.
template <bool RAGGED>
__global__ __launch_bounds__(256) void cm_stats_kernel(const float* __restrict__ z, float* __restrict__ partial, int B, int C, int T, int bchunk, const int* __restrict__ lens, int shifted) {
  __shared__ float r1[256], r2[256];
  const int c = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
  const int b0 = ch * bchunk, b1 = min(B, b0 + bchunk);
  const float k = shifted ? z[(size_t)c * T] : 0.f;
  float s1 = 0.f, s2 = 0.f;
  for (int b = b0; b < b1; ++b) {
    const float* row = z + ((size_t)b * C + c) * T;
    const int Tb = RAGGED ? lens[b] : T;
    for (int t = tid; t < Tb; t += 256) { const float v = row[t] - k; s1 += v; s2 = fmaf(v, v, s2); }
  }
  r1[tid] = s1; r2[tid] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { r1[tid] += r1[tid + off]; r2[tid] += r2[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) { partial[((size_t)ch * C + c) * 2] = r1[0]; partial[((size_t)ch * C + c) * 2 + 1] = r2[0]; }
}

// (drop_scale1 of dlq_common.h is the same value picked by a select chain; this one reads an indexed array, the two compile differently)
__device__ __forceinline__ float drop1(const DropCfg& dc, uint64_t idx) {
  if (dc.thresh == 0) return 1.f;
  float f[8];
  drop_scale8(dc, idx & ~(uint64_t)7, f);
  return f[idx & 7];
}

// ---- forward: h = dropout(relu(bn(z)))  (elementwise, [B][C][T])
template <bool RAGGED>
__global__ void cm_bn_relu_drop_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ h, int C, int T, size_t n, DropCfg dc, const int* __restrict__ lens) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)((i / T) % C);
  if constexpr (RAGGED) {
    const size_t bc = i / T;
    if ((int)(i - bc * T) >= lens[bc / C]) { h[i] = 0.f; return; }
  }
  const float y = bn_y(bn_xhat(z[i], mean[c], invstd[c]), gamma[c], beta[c]);
  h[i] = fmaxf(y, 0.f) * drop1(dc, i);
}

// ---- forward: pooled[b][c] = mean_t relu(bn(z[b][c][t]))   (one wave per (b, c) row)
template <bool RAGGED>
__global__ __launch_bounds__(256) void cm_bn_relu_meant_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ pooled, int C, int T, int rows, const int* __restrict__ lens) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int c = row % C;
  const BnFwd1 bn = bn_fwd1(mean[c], invstd[c], gamma[c], beta[c]);
  float s = 0.f;
  const int Tb = RAGGED ? lens[row / C] : T;
  for (int t = lane; t < Tb; t += 64) s += bn_relu(z[(size_t)row * T + t], bn.sc, bn.sh);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) pooled[row] = s / (float)Tb;
}

// ---- BatchNorm1d backward, channel-major.  Upstream gradient g of the ReLU output:
//   SRC 0 (mean over T then Linear): dpooled[b][c] / T_b;   SRC 1 (dropout): dropscale * dh[b][c][t]
template <int SRC, bool RAGGED>
__global__ __launch_bounds__(256) void cm_bn_bwd_reduce_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ up, float* __restrict__ partial, int B, int C, int T, int bchunk, DropCfg dc, const int* __restrict__ lens) {
  __shared__ float r1[256], r2[256];
  const int c = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
  const int b0 = ch * bchunk, b1 = min(B, b0 + bchunk);
  const float mu = mean[c], is = invstd[c], gm = gamma[c], bt = beta[c];
  float s1 = 0.f, s2 = 0.f;
  for (int b = b0; b < b1; ++b) {
    const size_t base = ((size_t)b * C + c) * T;
    const int Tb = RAGGED ? lens[b] : T;
    for (int t = tid; t < Tb; t += 256) {
      const float xh = bn_xhat(z[base + t], mu, is);
      const float g = (SRC == 0) ? up[(size_t)b * C + c] / (float)Tb : up[base + t] * drop1(dc, base + t);
      bn_accum(bn_gate(xh, gm, bt, g), xh, s1, s2);
    }
  }
  r1[tid] = s1; r2[tid] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { r1[tid] += r1[tid + off]; r2[tid] += r2[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) { partial[((size_t)ch * C + c) * 2] = r1[0]; partial[((size_t)ch * C + c) * 2 + 1] = r2[0]; }
}

template <int SRC, bool RAGGED>
__global__ void cm_bn_bwd_apply_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ sums, const float* __restrict__ up, float* __restrict__ dz, int C, int T, size_t n, float inv_n, DropCfg dc, const int* __restrict__ lens) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)((i / T) % C);
  const size_t bc = i / T;
  int Tb = T;
  if constexpr (RAGGED) {
    Tb = lens[bc / C];
    if ((int)(i - bc * T) >= Tb) { dz[i] = 0.f; return; }      // an exact zero: the padding frame is no frame of the batch
  }
  const float xh = bn_xhat(z[i], mean[c], invstd[c]);
  const float g = (SRC == 0) ? up[bc] / (float)Tb : up[i] * drop1(dc, i);
  const float dy = bn_gate(xh, gamma[c], beta[c], g);
  // bn_dz's terms, but the last one associated (xh * S2) * inv_n where bn_dz forms xh * (S2 * inv_n): one rounding apart, and this
  // kernel's results are pinned bit for bit, so it keeps the order it has always had
  dz[i] = gamma[c] * invstd[c] * (dy - sums[2 * c] * inv_n - xh * sums[2 * c + 1] * inv_n);
}

// ---- Conv1d weight gradient: dW[o][c][k] = sum_{b,t} dz[b][o][t] * h[b][c][t+k-1],  db[o] = sum dz, in slabs of W1D_TT frames;
// partial[chunk][Cout][Cin][3] (+ [Cout] for db).  Both kernels take 32 output channels per block (dfa_cnn1d_set_params admits
// base_channels = 32 only, so Cout is 32, 64 or 128).
// RAGGED (layer 1 of a ragged batch): h = x padded to T frames, utterance b owns [0, lens[b]); a padding frame is never loaded
// (it may hold NaN / Inf, and dz = 0 there would not clear it) -- another bound in the load, in a branch of its own so that the
// uniform and AUG instantiations keep their code.
constexpr int W1D_TT = 64;

// ---- on the fp32 matrix cores: three GEMMs [32 o x t] . [t x 32 c] (one per tap) sharing the dz
// operand; both operands are channel-major with t contiguous, i.e. K-contiguous rows, so v_mfma_f32_32x32x2_f32 takes
// them straight from LDS tiles (lane = channel, k = frame parity).  One wave per (o tile, c tile, utterance chunk):
// 96 MFMAs per 64-frame slab.
// AUG (layer 1 only): h = x read through the armed train-time augmentation, as the forward read it (conv1d.hip)
// K = taps (padding K / 2): 3, or 5 for layer 1 of the k = (5, 3, 3) variant -- record [Cout][Cin][K] + [Cout], a window of 64 + K - 1
// frames per slab (K = 5: two more extra frames per channel, rh3)
template <bool AUG, bool RAGGED = false, int K = 3>
__global__ __launch_bounds__(64) void conv1d_wgrad_mfma_kernel(const float* __restrict__ dz, const float* __restrict__ h,
                                                               int64_t hsb, int64_t hsc, int64_t hst,
                                                               float* __restrict__ partial, int B, int Cin, int Cout, int T,
                                                               int bchunk, AugCfg aug, const int* __restrict__ lens = nullptr) {
  __shared__ float dzs[32][W1D_TT + 1];
  __shared__ float hs[32][W1D_TT + K];
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int o0 = blockIdx.x * 32, c0 = blockIdx.y * 32, ch = blockIdx.z;
  const int b0 = ch * bchunk, b1 = min(B, b0 + bchunk);
  f32x16_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[k][i] = 0.f;
  float ab = 0.f;
  // slab = (utterance, 64 frames); the next slab's 66 values per lane are fetched into registers while the MFMAs of the
  // current one run (all loads of a slab are issued back to back: one latency per slab, not one per row)
  const int nslab_t = (T + W1D_TT - 1) / W1D_TT;
  const int nslab = (b1 - b0) * nslab_t;
  float rdz[32], rh[32], rh2 = 0.f;
  [[maybe_unused]] float rh3 = 0.f;
  auto fetch = [&](int sl) {
    const int b = b0 + sl / nslab_t, t0 = (sl % nslab_t) * W1D_TT;
#pragma unroll
    for (int oo = 0; oo < 32; ++oo)
      rdz[oo] = (t0 + lane < T) ? dz[((size_t)b * Cout + o0 + oo) * T + t0 + lane] : 0.f;
    const int t = t0 - K / 2 + lane;
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) {
      const int ci = c0 + cc;
      if constexpr (AUG)
        rh[cc] = (ci < Cin && t >= 0 && t < T) ? aug_apply(aug, h[(int64_t)b * hsb + (int64_t)ci * hsc + (int64_t)aug_src_t(aug, t) * hst], b, t, ci) : 0.f;
      else if constexpr (RAGGED)
        rh[cc] = (ci < Cin && t >= 0 && t < lens[b]) ? h[(int64_t)b * hsb + (int64_t)ci * hsc + (int64_t)t * hst] : 0.f;
      else
        rh[cc] = (ci < Cin && t >= 0 && t < T) ? h[(int64_t)b * hsb + (int64_t)ci * hsc + (int64_t)t * hst] : 0.f;
    }
    // the two extra frames of the 66-frame window: lane = (channel, which frame)
    const int ci2 = c0 + (lane & 31), t2 = t0 + 64 - K / 2 + (lane >> 5);
    if constexpr (AUG)
      rh2 = (ci2 < Cin && t2 < T) ? aug_apply(aug, h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)aug_src_t(aug, t2) * hst], b, t2, ci2) : 0.f;
    else if constexpr (RAGGED)
      rh2 = (ci2 < Cin && t2 < lens[b]) ? h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)t2 * hst] : 0.f;
    else
      rh2 = (ci2 < Cin && t2 < T) ? h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)t2 * hst] : 0.f;
    if constexpr (K == 5) {      // frames 66, 67 of the window (uniform batches only: never RAGGED)
      const int t3 = t2 + 2;
      if constexpr (AUG)
        rh3 = (ci2 < Cin && t3 < T) ? aug_apply(aug, h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)aug_src_t(aug, t3) * hst], b, t3, ci2) : 0.f;
      else
        rh3 = (ci2 < Cin && t3 < T) ? h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)t3 * hst] : 0.f;
    }
  };
  if (nslab > 0) fetch(0);
  for (int sl = 0; sl < nslab; ++sl) {
    __syncthreads();
#pragma unroll
    for (int oo = 0; oo < 32; ++oo) dzs[oo][lane] = rdz[oo];
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) hs[cc][lane] = rh[cc];
    hs[lane & 31][64 + (lane >> 5)] = rh2;
    if constexpr (K == 5) hs[lane & 31][66 + (lane >> 5)] = rh3;
    __syncthreads();
    if (sl + 1 < nslab) fetch(sl + 1);
#pragma unroll 8
    for (int tt = 0; tt < W1D_TT; tt += 2) {
      const float a = dzs[r][tt + hh];
      ab += a;
#pragma unroll
      for (int k = 0; k < K; ++k)
        acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, hs[r][tt + hh + k], acc[k], 0, 0, 0);
    }
  }
  float* rec = partial + (size_t)ch * ((size_t)Cout * Cin * K + Cout);
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = o0 + (i & 3) + 8 * (i >> 2) + 4 * hh, c = c0 + r;
      if (c < Cin) rec[((size_t)o * Cin + c) * K + k] = acc[k][i];
    }
  ab += __shfl_xor(ab, 32, 64);
  if (blockIdx.y == 0 && hh == 0) rec[(size_t)Cout * Cin * K + o0 + r] = ab;
}

// ---- the same weight gradient on the bf16 matrix cores at fp32 grade: every fp32 operand is carried as three bf16 terms
// (split8n<3>; dfa_device.h has why three terms are the operand exactly) and every product is six v_mfma_f32_32x32x16_bf16 (all term pairs of order <= 2),
// as the training convolutions of conv1d_x3.hip do.  The fp32 matrix pipe issues one 32x32x2 MFMA per ~80 cycles: 24 of them
// per 16 frames and tap triple = 1920 cycles; the same products cost 18 x 32 = 576 matrix-pipe cycles here plus the splits.
// Same decomposition and slab pipeline as the kernel above; the LDS tiles are laid out for aligned 16-byte fragment reads (row
// pitch 68 floats: the 16 lanes of a ds_read_b128 group fall on distinct banks): a lane reads its row's 8 dz frames (two reads)
// and 12 h frames (three reads: frames t-1 .. t+10) per 16-frame k-step, the three taps are register windows [k, k + 8) of
// those 12 values.

// K = 5 (layer 1 of the k = (5, 3, 3) variant): the five taps are the windows [k, k + 8) of the same 12 values, now frames
// t - 2 .. t + 9, and the slab's window is all 68 frames of a row
template <bool AUG, bool RAGGED = false, int K = 3>
__global__ __launch_bounds__(64) void conv1d_wgrad_x3_kernel(const float* __restrict__ dz, const float* __restrict__ h,
                                                             int64_t hsb, int64_t hsc, int64_t hst,
                                                             float* __restrict__ partial, int B, int Cin, int Cout, int T,
                                                             int bchunk, AugCfg aug, const int* __restrict__ lens = nullptr) {
  constexpr int PITCH = 68;
  __shared__ __attribute__((aligned(16))) float dzs[32][PITCH];
  __shared__ __attribute__((aligned(16))) float hs[32][PITCH];      // hs[c][i] = frame t0 - 1 + i, i < 66 (67 = zero); K = 5: frame t0 - 2 + i, i < 68
  const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
  const int o0 = blockIdx.x * 32, c0 = blockIdx.y * 32, ch = blockIdx.z;
  const int b0 = ch * bchunk, b1 = min(B, b0 + bchunk);
  f32x16_t acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[k][i] = 0.f;
  float ab = 0.f;
  const int nslab_t = (T + W1D_TT - 1) / W1D_TT;
  const int nslab = (b1 - b0) * nslab_t;
  float rdz[32], rh[32], rh2 = 0.f;
  [[maybe_unused]] float rh3 = 0.f;
  auto fetch = [&](int sl) {
    const int b = b0 + sl / nslab_t, t0 = (sl % nslab_t) * W1D_TT;
#pragma unroll
    for (int oo = 0; oo < 32; ++oo)
      rdz[oo] = (t0 + lane < T) ? dz[((size_t)b * Cout + o0 + oo) * T + t0 + lane] : 0.f;
    const int t = t0 - K / 2 + lane;
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) {
      const int ci = c0 + cc;
      if constexpr (AUG)
        rh[cc] = (ci < Cin && t >= 0 && t < T) ? aug_apply(aug, h[(int64_t)b * hsb + (int64_t)ci * hsc + (int64_t)aug_src_t(aug, t) * hst], b, t, ci) : 0.f;
      else if constexpr (RAGGED)
        rh[cc] = (ci < Cin && t >= 0 && t < lens[b]) ? h[(int64_t)b * hsb + (int64_t)ci * hsc + (int64_t)t * hst] : 0.f;
      else
        rh[cc] = (ci < Cin && t >= 0 && t < T) ? h[(int64_t)b * hsb + (int64_t)ci * hsc + (int64_t)t * hst] : 0.f;
    }
    const int ci2 = c0 + (lane & 31), t2 = t0 + 64 - K / 2 + (lane >> 5);
    if constexpr (AUG)
      rh2 = (ci2 < Cin && t2 < T) ? aug_apply(aug, h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)aug_src_t(aug, t2) * hst], b, t2, ci2) : 0.f;
    else if constexpr (RAGGED)
      rh2 = (ci2 < Cin && t2 < lens[b]) ? h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)t2 * hst] : 0.f;
    else
      rh2 = (ci2 < Cin && t2 < T) ? h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)t2 * hst] : 0.f;
    if constexpr (K == 5) {      // frames 66, 67 of the window (uniform batches only: never RAGGED)
      const int t3 = t2 + 2;
      if constexpr (AUG)
        rh3 = (ci2 < Cin && t3 < T) ? aug_apply(aug, h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)aug_src_t(aug, t3) * hst], b, t3, ci2) : 0.f;
      else
        rh3 = (ci2 < Cin && t3 < T) ? h[(int64_t)b * hsb + (int64_t)ci2 * hsc + (int64_t)t3 * hst] : 0.f;
    }
  };
  if (lane < 32) { hs[lane][66] = 0.f; hs[lane][67] = 0.f; }      // the tail of the 12-frame window of the last k-step
  if (nslab > 0) fetch(0);
  for (int sl = 0; sl < nslab; ++sl) {
    __syncthreads();
#pragma unroll
    for (int oo = 0; oo < 32; ++oo) dzs[oo][lane] = rdz[oo];
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) hs[cc][lane] = rh[cc];
    hs[lane & 31][64 + (lane >> 5)] = rh2;
    if constexpr (K == 5) hs[lane & 31][66 + (lane >> 5)] = rh3;
    __syncthreads();
    if (sl + 1 < nslab) fetch(sl + 1);
#pragma unroll
    for (int ks = 0; ks < W1D_TT / 16; ++ks) {
      float dv[8], hv[12];
      *(float4*)&dv[0] = *(const float4*)&dzs[r][16 * ks + 8 * hh];
      *(float4*)&dv[4] = *(const float4*)&dzs[r][16 * ks + 8 * hh + 4];
      *(float4*)&hv[0] = *(const float4*)&hs[r][16 * ks + 8 * hh];
      *(float4*)&hv[4] = *(const float4*)&hs[r][16 * ks + 8 * hh + 4];
      *(float4*)&hv[8] = *(const float4*)&hs[r][16 * ks + 8 * hh + 8];
#pragma unroll
      for (int j = 0; j < 8; ++j) ab += dv[j];
      uint4 a[3];
      split8n<3>(dv, a);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float win[8] = {hv[k], hv[k + 1], hv[k + 2], hv[k + 3], hv[k + 4], hv[k + 5], hv[k + 6], hv[k + 7]};
        uint4 bq[3];
        split8n<3>(win, bq);
        acc[k] = mma32(a[2], bq[0], acc[k]);          // smallest terms first
        acc[k] = mma32(a[0], bq[2], acc[k]);
        acc[k] = mma32(a[1], bq[1], acc[k]);
        acc[k] = mma32(a[1], bq[0], acc[k]);
        acc[k] = mma32(a[0], bq[1], acc[k]);
        acc[k] = mma32(a[0], bq[0], acc[k]);
      }
    }
  }
  float* rec = partial + (size_t)ch * ((size_t)Cout * Cin * K + Cout);
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = o0 + (i & 3) + 8 * (i >> 2) + 4 * hh, c = c0 + r;
      if (c < Cin) rec[((size_t)o * Cin + c) * K + k] = acc[k][i];
    }
  ab += __shfl_xor(ab, 32, 64);
  if (blockIdx.y == 0 && hh == 0) rec[(size_t)Cout * Cin * K + o0 + r] = ab;
}

// data-gradient weights of Conv1d: W'[c][o][k'] = W[o][c][2-k']  (a Conv1d with Cin' = Cout, Cout' = Cin)
__global__ void conv1d_dgrad_pack_kernel(const float* __restrict__ w, float* __restrict__ wt, float* __restrict__ zero_bias,
                                         int cin, int cout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cin) zero_bias[i] = 0.f;
  if (i >= cin * cout * 3) return;
  const int k = i % 3, o = (i / 3) % cout, c = i / (3 * cout);
  wt[i] = w[((size_t)o * cin + c) * 3 + (2 - k)];
}

// whole partial record in one launch: elements [0, n0) -> out0, [n0, n0 + n1) -> out1; 64 elements x 4 record groups per
// block, fp64 sums combined in a fixed order (as reduce_wgrad_record_kernel of train_elem.hip)
__global__ __launch_bounds__(256) void reduce_record2_kernel(const float* __restrict__ partial, int nparts, int stride, int n0,
                                                             float* __restrict__ out0, int n1, float* __restrict__ out1) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, pg = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane, total = n0 + n1;
  double s = 0.0;
  if (e < total) {
    const int k0 = (int)((long)pg * nparts / 4), k1 = (int)((long)(pg + 1) * nparts / 4);
    const float* p = partial + (size_t)k0 * stride + e;
#pragma unroll 8
    for (int k = k0; k < k1; ++k, p += stride) s += (double)*p;
  }
  red[pg][lane] = s;
  __syncthreads();
  if (pg != 0 || e >= total) return;
  const float v = (float)((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]));
  if (e < n0) out0[e] = v; else out1[e - n0] = v;
}

// ================================================================================================ launchers
constexpr int kCmChunks = 64;   // batch chunks of the channel-major reductions: 16 left the 32->64 weight gradient at 128 blocks on 256 CUs
int cm_chunks(int B) { return B < kCmChunks ? B : kCmChunks; }

hipError_t launch_cm_stats(const float* z, float* partial, int B, int C, int T, hipStream_t s, const int* lens, bool shifted) {
  const int nch = cm_chunks(B), bchunk = (B + nch - 1) / nch;
  hipLaunchKernelGGL(lens ? cm_stats_kernel<true> : cm_stats_kernel<false>, dim3(C, nch), dim3(256), 0, s, z, partial, B, C, T, bchunk, lens, (int)shifted);
  return hipGetLastError();
}
hipError_t launch_cm_bn_relu_drop(const float* z, const BnApply& bn, float* h, int B, int C, int T, const DropCfg& dc, hipStream_t s,
                                  const int* lens) {
  const size_t n = (size_t)B * C * T;
  hipLaunchKernelGGL(lens ? cm_bn_relu_drop_kernel<true> : cm_bn_relu_drop_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z,
                     bn.mean, bn.invstd, bn.gamma, bn.beta, h, C, T, n, dc, lens);
  return hipGetLastError();
}
hipError_t launch_cm_bn_relu_meant(const float* z, const BnApply& bn, float* pooled, int B, int C, int T, hipStream_t s, const int* lens) {
  const int rows = B * C;
  hipLaunchKernelGGL(lens ? cm_bn_relu_meant_kernel<true> : cm_bn_relu_meant_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, s, z, bn.mean,
                     bn.invstd, bn.gamma, bn.beta, pooled, C, T, rows, lens);
  return hipGetLastError();
}
// lens != null: the ragged instantiations, n_valid = the batch's frame count (sum of the lengths)
hipError_t launch_cm_bn_bwd(int src, const float* z, const BnApply& bn, const float* up, float* partial, float* sums, float* dz, int B, int C,
                            int T, const DropCfg& dc, hipStream_t s, const BnSync* sync, const int* lens, double n_valid) {
  const int nch = cm_chunks(B), bchunk = (B + nch - 1) / nch;
  const size_t n = (size_t)B * C * T;
  const auto reduce = src == 0 ? (lens ? cm_bn_bwd_reduce_kernel<0, true> : cm_bn_bwd_reduce_kernel<0, false>)
                               : (lens ? cm_bn_bwd_reduce_kernel<1, true> : cm_bn_bwd_reduce_kernel<1, false>);
  const auto apply = src == 0 ? (lens ? cm_bn_bwd_apply_kernel<0, true> : cm_bn_bwd_apply_kernel<0, false>)
                              : (lens ? cm_bn_bwd_apply_kernel<1, true> : cm_bn_bwd_apply_kernel<1, false>);
  hipLaunchKernelGGL(reduce, dim3(C, nch), dim3(256), 0, s, z, bn.mean, bn.invstd, bn.gamma, bn.beta, up, partial, B, C, T, bchunk, dc, lens);
  const float* sums_a;
  float inv_n = (float)(1.0 / (lens ? n_valid : (double)B * T));
  const hipError_t e = bn_bwd_sums(partial, nch, C, sums, nullptr, sync, s, &sums_a, &inv_n);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, bn.mean, bn.invstd, bn.gamma, bn.beta, sums_a, up, dz, C, T, n,
                     inv_n, dc, lens);
  return hipGetLastError();
}
// partial: conv1d_wgrad_chunks(B) * (Cout*Cin*taps + Cout) floats
int conv1d_wgrad_chunks(int B) { return B < 256 ? B : 256; }
hipError_t launch_conv1d_wgrad(const float* dz, const float* h, int64_t hsb, int64_t hsc, int64_t hst, float* partial,
                               float* dw, float* db, int B, int Cin, int Cout, int T, hipStream_t s, const AugCfg* aug, int x3, const int* lens,
                               int taps) {
  const int nch = conv1d_wgrad_chunks(B), bchunk = (B + nch - 1) / nch;
  const bool aug_on = aug && aug->on;
  if (Cout % 32 != 0) return hipErrorInvalidValue;     // both kernels tile 32 output channels
  if (lens && aug_on) return hipErrorInvalidValue;     // a time roll has no per-utterance meaning
  // x3: the three-term bf16 matrix-core form (fp32-grade sums), else the fp32 matrix cores; lens: ragged layer 1, h = the padded x,
  // bounded per utterance in the loads
  if (taps != 3 && (taps != 5 || lens)) return hipErrorInvalidValue;   // five taps: layer 1 of the variant, uniform batches
  const auto kern =
      taps == 5 ? (x3 ? (aug_on ? conv1d_wgrad_x3_kernel<true, false, 5> : conv1d_wgrad_x3_kernel<false, false, 5>)
                      : (aug_on ? conv1d_wgrad_mfma_kernel<true, false, 5> : conv1d_wgrad_mfma_kernel<false, false, 5>))
      : x3      ? (lens ? conv1d_wgrad_x3_kernel<false, true> : aug_on ? conv1d_wgrad_x3_kernel<true> : conv1d_wgrad_x3_kernel<false>)
                : (lens ? conv1d_wgrad_mfma_kernel<false, true> : aug_on ? conv1d_wgrad_mfma_kernel<true> : conv1d_wgrad_mfma_kernel<false>);
  hipLaunchKernelGGL(kern, dim3(Cout / 32, (Cin + 31) / 32, nch), dim3(64), 0, s, dz, h, hsb, hsc, hst, partial, B, Cin, Cout, T, bchunk,
                     aug_on ? *aug : AugCfg{}, lens);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int n = Cout * Cin * taps;
  hipLaunchKernelGGL(reduce_record2_kernel, dim3((n + Cout + 63) / 64), dim3(256), 0, s, partial, nch, n + Cout, n, dw, Cout, db);
  return hipGetLastError();
}
hipError_t launch_conv1d_dgrad_pack(const float* w, float* wt, float* zero_bias, int cin, int cout, hipStream_t s) {
  const int n = cin * cout * 3;
  hipLaunchKernelGGL(conv1d_dgrad_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w, wt, zero_bias, cin, cout);
  return hipGetLastError();
}

}  // namespace dfa

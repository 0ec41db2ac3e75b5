// bn_device.h -- the train-mode BatchNorm + ReLU element math of the training steps, stated once (train_elem.hip: channels-last,
// 8 channels per lane; train_cnn1d.hip: channel-major, one channel per thread).  With xh = (z - mean) * invstd:
//   forward   relu(fma(z, sc, sh)),  sc = gamma * invstd,  sh = beta - mean * sc
//   backward  dy = fma(gamma, xh, beta) > 0 ? g : 0   (g = the upstream gradient of the ReLU output)
//             S1 = sum dy (= dbeta),  S2 = sum dy * xh (= dgamma)
//             dz = gamma * invstd * (dy - S1 / n - xh * S2 / n)
// Every reduce pass masks as its apply pass does, and the sums bn_relu_meant_kernel saves carry the mask bn_bwd_apply_meant_kernel
// applies, because all of them call bn_xhat / bn_gate below; the 8-wide forms are loops over the one-channel forms.
// Accumulators and data stay local arrays of the kernel and come in by pointer: held in a struct they cost the row-pair reduction
// 26 VGPRs.  Only the read-only per-channel terms are structs.
#pragma once
#include <hip/hip_runtime.h>

namespace dfa {

// ---- one channel
__device__ __forceinline__ float bn_xhat(float z, float mu, float is) { return (z - mu) * is; }
__device__ __forceinline__ float bn_y(float xh, float gm, float bt) { return fmaf(gm, xh, bt); }
__device__ __forceinline__ float bn_gate(float xh, float gm, float bt, float g) { return bn_y(xh, gm, bt) > 0.f ? g : 0.f; }
__device__ __forceinline__ void bn_accum(float dy, float xh, float& s1, float& s2) {
  s1 += dy;
  s2 = fmaf(dy, xh, s2);
}
// k0 = gamma * invstd, k1 = S1 / n, k2 = S2 / n
__device__ __forceinline__ float bn_dz(float dy, float xh, float k0, float k1, float k2) { return k0 * (dy - k1 - xh * k2); }
struct BnFwd1 { float sc, sh; };
__device__ __forceinline__ BnFwd1 bn_fwd1(float mu, float is, float gm, float bt) {
  const float sc = gm * is;
  return {sc, bt - mu * sc};
}
__device__ __forceinline__ float bn_relu(float z, float sc, float sh) { return fmaxf(fmaf(z, sc, sh), 0.f); }

// ---- 8 consecutive channels from c0 = 8 * cg
struct Bn8 {
  float mu[8], is[8], gm[8], bt[8];
  __device__ __forceinline__ float xhat(int j, float z) const { return bn_xhat(z, mu[j], is[j]); }
  __device__ __forceinline__ float gate(int j, float xh, float g) const { return bn_gate(xh, gm[j], bt[j], g); }
};
struct BnFwd8 {
  float sc[8], sh[8];
  __device__ __forceinline__ float relu(int j, float z) const { return bn_relu(z, sc[j], sh[j]); }
};
struct BnCoef8 {
  float k0[8], k1[8], k2[8];
  __device__ __forceinline__ float dz(int j, float dy, float xh) const { return bn_dz(dy, xh, k0[j], k1[j], k2[j]); }
};

__device__ __forceinline__ Bn8 bn_load8(const float* __restrict__ mean, const float* __restrict__ invstd,
                                        const float* __restrict__ gamma, const float* __restrict__ beta, int c0) {
  Bn8 t;
#pragma unroll
  for (int j = 0; j < 8; ++j) { t.mu[j] = mean[c0 + j]; t.is[j] = invstd[c0 + j]; t.gm[j] = gamma[c0 + j]; t.bt[j] = beta[c0 + j]; }
  return t;
}
__device__ __forceinline__ BnFwd8 bn_fwd8(const Bn8& t) {
  BnFwd8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const BnFwd1 f1 = bn_fwd1(t.mu[j], t.is[j], t.gm[j], t.bt[j]);
    f.sc[j] = f1.sc; f.sh[j] = f1.sh;
  }
  return f;
}
// the terms and, on top of them, the apply pass's coefficients; sums: [C][2] (S1, S2).  (One loop, channel by channel: loading the
// four term arrays first and the sums after them schedules the row-pair apply pass differently.)
__device__ __forceinline__ void bn_load8(const float* __restrict__ mean, const float* __restrict__ invstd,
                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                         const float* __restrict__ sums, int c0, float inv_n, Bn8& t, BnCoef8& k) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    t.mu[j] = mean[c]; t.is[j] = invstd[c]; t.gm[j] = gamma[c]; t.bt[j] = beta[c];
    k.k0[j] = t.gm[j] * t.is[j];
    k.k1[j] = sums[2 * c] * inv_n;
    k.k2[j] = sums[2 * c + 1] * inv_n;
  }
}
// one pixel: (s1, s2) += (dy, dy * xh)
__device__ __forceinline__ void bn_bwd_accum8(const Bn8& t, const float* z, const float* g, float* s1, float* s2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xh = t.xhat(j, z[j]);
    bn_accum(t.gate(j, xh, g[j]), xh, s1[j], s2[j]);
  }
}
// one pixel: z, g -> dz
__device__ __forceinline__ void bn_bwd_dz8(const Bn8& t, const BnCoef8& k, const float* z, const float* g, float* dz) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float xh = t.xhat(j, z[j]);
    dz[j] = k.dz(j, t.gate(j, xh, g[j]), xh);
  }
}

// ---- thread map of the blocked channels-last passes: thread = (channel octet cg, item lane pl) of a 256-thread block, item lanes
// stride PL; the block takes items [p0, p1) of n (pixels, row pairs or positions)
struct BnLane { int PL, cg, pl; };
__device__ __forceinline__ BnLane bn_lane(int C) {
  const int CG = C >> 3, tid = threadIdx.x;
  return {256 / CG, tid % CG, tid / CG};
}
struct BnRange { size_t p0, p1; };
__device__ __forceinline__ BnRange bn_range(size_t n, int per_block) {
  const size_t p0 = (size_t)blockIdx.x * per_block;
  return {p0, (p0 + per_block < n) ? p0 + per_block : n};
}

// ---- block epilogue: per-thread sums -> red[PL][C][2] (or red[PL][C]) in LDS -> one record rec[block][C][N], the
// item lanes added in the order q = 0 .. PL-1: fixed, so the record is deterministic
__device__ __forceinline__ void bn_lds_put2(float* red, const BnLane& ln, int C, const float* s1, const float* s2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) { red[(ln.pl * C + ln.cg * 8 + j) * 2] = s1[j]; red[(ln.pl * C + ln.cg * 8 + j) * 2 + 1] = s2[j]; }
}
__device__ __forceinline__ void bn_lds_put1(float* red, const BnLane& ln, int C, const float* s) {
#pragma unroll
  for (int j = 0; j < 8; ++j) red[ln.pl * C + ln.cg * 8 + j] = s[j];
}
template <int N>      // floats per channel: 2 or 1
__device__ __forceinline__ void bn_lds_to_record(const float* red, int PL, int C, float* __restrict__ rec) {
  __syncthreads();
  for (int e = threadIdx.x; e < C * N; e += 256) {
    float s = 0.f;
    for (int q = 0; q < PL; ++q) s += red[q * C * N + e];
    rec[(size_t)blockIdx.x * C * N + e] = s;
  }
}

}  // namespace dfa

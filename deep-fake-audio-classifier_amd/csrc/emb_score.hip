// emb_score.hip -- anomaly scoring of CNN2D embeddings on the GPU (src/embedding_anomaly.py:129-163: StandardScaler, then
// OneClassSVM.decision_function, and PCA + GaussianMixture.score_samples).  One GEMM frame on the exact-fp32 matrix cores
// (v_mfma_f32_32x32x2_f32) serves the three products; the scaler is applied as the embedding rows are staged, so no scaled copy
// of the batch exists in HBM.
//
//   emb_gemm_kernel      C[z][n][m] = sum_d f(A[n][d]) B[m][d],  f(a) = (a - sub[d]) mul[d] - sub2[d]  (null mul / sub2: left out)
//                          z = a split of the reduction over D (OC-SVM: B = support vectors; PCA: B = components), or
//                          z = a mixture component (A = z, sub = its mean, B = its transposed precision factor)
//   emb_ocsvm_finish     one workgroup per row: |x~|^2, the splits summed in their order, the RBF terms, their sum
//   emb_z_reduce         the PCA splits summed in their order -> z[N][P_pad]
//   emb_gmm_finish       one workgroup per row: |y_k|^2 per component, log-sum-exp
//   emb_rownorm / emb_pack_gmm   the bind-time image: |sv_i|^2, and prec_chol transposed + the means, zero-padded to P_pad
//
// No atomics anywhere: every sum has one owner and a fixed order that depends on D, M and K alone, so a row's score is bit for bit
// a function of that row (the split of D is chosen from D and M, never from N; a row's MFMA accumulator chain is the same in every
// tile position).  Every LDS word and every workspace word that is read has been written by the same call.
#include "dfa_device.h"
#include "dfa_internal.h"

namespace dfa {

namespace {

constexpr int TN = 128, TM = 128, TK = 32;   // workgroup tile: 128 rows x 128 columns, 32 of the reduction per stage
constexpr int LDP = TK + 1;                  // LDS row pitch in floats: rows r and r + 1 one bank apart (ds_read_b32: bank = word % 32)
constexpr int CHAIN = 8;                     // stages per fmaf chain: 256 products, then the chain is added to the running total

struct EmbGemmArgs {
  const float* A; int64_t lda;               // [N][lda]
  const float *sub, *mul, *sub2;             // [D] each; mul, sub2 may be null
  const float* B; int64_t ldb;               // [Brows][ldb]
  float* C;                                  // [gridDim.z][N][M]
  int N, M, Brows, D;
  int kstep;                                 // reduction range of z: [z kstep, min(D, z kstep + klen))
  int klen;
  int64_t b_zstride;                         // B of z = B + z b_zstride
  int sub_zstride;                           // sub of z = sub + z sub_zstride
};

__device__ __forceinline__ float4 stage_a(const float4 x, const float4 s, const float4 m, const float4 p, bool has_mul, bool has_sub2) {
  float v[4] = {__fsub_rn(x.x, s.x), __fsub_rn(x.y, s.y), __fsub_rn(x.z, s.z), __fsub_rn(x.w, s.w)};
  const float mm[4] = {m.x, m.y, m.z, m.w}, pp[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (has_mul) v[j] = __fmul_rn(v[j], mm[j]);
    if (has_sub2) v[j] = __fsub_rn(v[j], pp[j]);
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

// 256 threads = 4 waves as 2 x 2, each wave a 64 x 64 part of the tile (2 x 2 MFMA tiles of 32 x 32).  D, klen, kstep are
// multiples of 32; A, B, sub, mul, sub2 16-byte aligned with lda, ldb multiples of 4 (the entry points check).
__global__ __launch_bounds__(256, 2) void emb_gemm_kernel(const EmbGemmArgs a) {
  __shared__ float As[TN * LDP];
  __shared__ float Bs[TM * LDP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n0 = blockIdx.y * TN, m0 = blockIdx.x * TM, z = blockIdx.z;
  const int kbeg = z * a.kstep, kend = min(a.D, kbeg + a.klen);
  const float* Bz = a.B + (int64_t)z * a.b_zstride;
  const float* subz = a.sub + (int64_t)z * a.sub_zstride;
  const bool has_mul = a.mul != nullptr, has_sub2 = a.sub2 != nullptr;
  const int c4 = (t & 7) * 4, r0 = t >> 3;   // the thread's float4 column of a stage and its first row (rows r0 + 32 i)
  const int wn = (wave >> 1) * 64, wm = (wave & 1) * 64, r = lane & 31, h = lane >> 5;

  float4 ra[4], rb[4];
  auto load = [&](int k0) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 s = *(const float4*)(subz + k0 + c4);
    float4 m = zero, p = zero;
    if (has_mul) m = *(const float4*)(a.mul + k0 + c4);
    if (has_sub2) p = *(const float4*)(a.sub2 + k0 + c4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + r0 + 32 * i, mrow = m0 + r0 + 32 * i;
      ra[i] = zero;
      rb[i] = zero;
      if (n < a.N) ra[i] = stage_a(*(const float4*)(a.A + (int64_t)n * a.lda + k0 + c4), s, m, p, has_mul, has_sub2);
      if (mrow < a.Brows) rb[i] = *(const float4*)(Bz + (int64_t)mrow * a.ldb + k0 + c4);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* pa = As + (r0 + 32 * i) * LDP + c4;
      float* pb = Bs + (r0 + 32 * i) * LDP + c4;
      pa[0] = ra[i].x; pa[1] = ra[i].y; pa[2] = ra[i].z; pa[3] = ra[i].w;
      pb[0] = rb[i].x; pb[1] = rb[i].y; pb[2] = rb[i].z; pb[3] = rb[i].w;
    }
  };

  f32x16_t acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.f; tot[i][j][e] = 0.f; }

  load(kbeg);
  int stage = 0;
  for (int k0 = kbeg; k0 < kend; k0 += TK) {
    __syncthreads();                       // the previous stage's reads are done
    store();
    __syncthreads();
    if (k0 + TK < kend) load(k0 + TK);     // the next stage's loads fly under this stage's MFMAs
#pragma unroll
    for (int k = 0; k < TK; k += 2) {
      const float a0 = As[(wn + r) * LDP + k + h], a1 = As[(wn + 32 + r) * LDP + k + h];
      const float b0 = Bs[(wm + r) * LDP + k + h], b1 = Bs[(wm + 32 + r) * LDP + k + h];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (++stage == CHAIN || k0 + TK >= kend) {   // a chain of at most 256 products joins the total: the sum's error stays that of short chains
      stage = 0;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) { tot[i][j][e] += acc[i][j][e]; acc[i][j][e] = 0.f; }
    }
  }

  float* Cz = a.C + (size_t)z * a.N * a.M;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = n0 + wn + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h, m = m0 + wm + 32 * j + r;
        if (n < a.N && m < a.M) Cz[(size_t)n * a.M + m] = tot[i][j][e];
      }
}

// the workgroup's 256 values summed in one fixed tree; every thread returns the sum
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int t = threadIdx.x;
  __syncthreads();                         // red is free again
  red[t] = v;
  for (int s = 128; s > 0; s >>= 1) {
    __syncthreads();
    if (t < s) red[t] += red[t + s];
  }
  __syncthreads();
  return red[0];
}

// |f(row)|^2 of one row by the workgroup: thread t owns d = t, t + 256, ...
__device__ __forceinline__ float row_sqnorm(const float* row, const float* sub, const float* mul, int D, float* red) {
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) {
    float v = row[d];
    if (sub) v = __fmul_rn(__fsub_rn(v, sub[d]), mul[d]);
    s = fmaf(v, v, s);
  }
  return block_sum(s, red);
}

__global__ __launch_bounds__(256) void emb_rownorm_kernel(const float* x, int64_t ld, int D, float* out) {
  __shared__ float red[256];
  const float s = row_sqnorm(x + (int64_t)blockIdx.x * ld, nullptr, nullptr, D, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// out[n] = sum_i coef[i] exp(-gamma (|x~_n|^2 + |sv_i|^2 - 2 x~_n . sv_i)) + intercept
__global__ __launch_bounds__(256) void emb_ocsvm_finish_kernel(const float* emb, int64_t ld, const float* mean, const float* inv_scale, int D,
                                                               const float* part, int nsplit, int N, int M, const float* svn, const float* coef,
                                                               float gamma, float intercept, float* out) {
  __shared__ float red[256];
  const int n = blockIdx.x;
  const float xn = row_sqnorm(emb + (int64_t)n * ld, mean, inv_scale, D, red);
  float s = 0.f;
  for (int m = threadIdx.x; m < M; m += 256) {
    float dot = 0.f;
    for (int q = 0; q < nsplit; ++q) dot += part[((size_t)q * N + n) * M + m];
    const float d2 = __fsub_rn(__fadd_rn(xn, svn[m]), __fmul_rn(2.f, dot));
    s = fmaf(coef[m], expf(-gamma * d2), s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[n] = s + intercept;
}

__global__ __launch_bounds__(256) void emb_z_reduce_kernel(const float* part, int nsplit, int N, int P, int Ppad, float* z) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)N * Ppad) return;
  const int n = (int)(i / Ppad), p = (int)(i % Ppad);
  float s = 0.f;
  if (p < P)
    for (int q = 0; q < nsplit; ++q) s += part[((size_t)q * N + n) * P + p];
  z[i] = s;
}

// out[n] = logsumexp_k (-|y_k|^2 / 2 + log_const[k]); wave w owns components w, w + 4, ...
__global__ __launch_bounds__(256) void emb_gmm_finish_kernel(const float* y, int N, int P, int K, const float* log_const, float* out) {
  __shared__ float lp[64];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < K; k += 4) {
    const float* yk = y + ((size_t)k * N + n) * P;
    float q = 0.f;
    for (int j = lane; j < P; j += 64) q = fmaf(yk[j], yk[j], q);
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (lane == 0) lp[k] = -0.5f * q + log_const[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mx = lp[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, lp[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(lp[k] - mx);
    out[n] = mx + logf(s);
  }
}

// LT[k][j][p] = prec_chol[k][p][j] and mpad[k][p] = means[k][p] inside P, +0 in the padding up to Ppad
__global__ __launch_bounds__(256) void emb_pack_gmm_kernel(const float* prec_chol, const float* means, int P, int Ppad, int K, float* LT, float* mpad) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)Ppad * Ppad;
  if (i >= per * K) return;
  const int k = (int)(i / per), j = (int)(i % per / Ppad), p = (int)(i % Ppad);
  LT[i] = (j < P && p < P) ? prec_chol[((size_t)k * P + p) * P + j] : 0.f;
  if (j == 0) mpad[(size_t)k * Ppad + p] = p < P ? means[(size_t)k * P + p] : 0.f;
}

hipError_t launch_gemm(const EmbGemmArgs& a, int nz, hipStream_t s) {
  hipLaunchKernelGGL(emb_gemm_kernel, dim3((a.M + TM - 1) / TM, (a.N + TN - 1) / TN, nz), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

EmbSplit emb_split(int D, int M) {
  const int mtiles = (M + TM - 1) / TM;
  const int want = std::min(32, std::max(1, (256 + mtiles - 1) / mtiles));
  EmbSplit sp;
  sp.klen = std::max(256, ((D + want - 1) / want + TK - 1) / TK * TK);
  sp.nsplit = (D + sp.klen - 1) / sp.klen;
  return sp;
}

hipError_t launch_emb_rownorm(const float* x, int64_t ld, int rows, int D, float* out, hipStream_t s) {
  hipLaunchKernelGGL(emb_rownorm_kernel, dim3(rows), dim3(256), 0, s, x, ld, D, out);
  return hipGetLastError();
}

hipError_t launch_emb_pack_gmm(const float* prec_chol, const float* means, int P, int K, float* LT, float* mpad, hipStream_t s) {
  const int Ppad = emb_ppad(P);
  const size_t n = (size_t)K * Ppad * Ppad;
  hipLaunchKernelGGL(emb_pack_gmm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, prec_chol, means, P, Ppad, K, LT, mpad);
  return hipGetLastError();
}

hipError_t launch_emb_ocsvm(const EmbOcsvm& d, const float* emb, int N, int64_t ld, float* part, float* out, hipStream_t s) {
  const EmbSplit sp = emb_split(d.D, d.n_sv);
  EmbGemmArgs a{};
  a.A = emb; a.lda = ld; a.sub = d.mean; a.mul = d.inv_scale; a.sub2 = nullptr;
  a.B = d.sv; a.ldb = d.D; a.C = part; a.N = N; a.M = d.n_sv; a.Brows = d.n_sv; a.D = d.D;
  a.kstep = sp.klen; a.klen = sp.klen; a.b_zstride = 0; a.sub_zstride = 0;
  hipError_t e = launch_gemm(a, sp.nsplit, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(emb_ocsvm_finish_kernel, dim3(N), dim3(256), 0, s, emb, ld, d.mean, d.inv_scale, d.D, (const float*)part, sp.nsplit, N, d.n_sv,
                     (const float*)d.svn, d.coef, d.gamma, d.intercept, out);
  return hipGetLastError();
}

hipError_t launch_emb_gmm(const EmbGmm& d, const float* emb, int N, int64_t ld, float* zpart, float* z, float* y, float* out, hipStream_t s) {
  const EmbSplit sp = emb_split(d.D, d.P);
  const int Ppad = emb_ppad(d.P);
  EmbGemmArgs a{};
  a.A = emb; a.lda = ld; a.sub = d.mean; a.mul = d.inv_scale; a.sub2 = d.pca_mean;
  a.B = d.comp; a.ldb = d.D; a.C = zpart; a.N = N; a.M = d.P; a.Brows = d.P; a.D = d.D;
  a.kstep = sp.klen; a.klen = sp.klen; a.b_zstride = 0; a.sub_zstride = 0;
  hipError_t e = launch_gemm(a, sp.nsplit, s);
  if (e != hipSuccess) return e;
  const size_t nz = (size_t)N * Ppad;
  hipLaunchKernelGGL(emb_z_reduce_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, s, (const float*)zpart, sp.nsplit, N, d.P, Ppad, z);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  EmbGemmArgs g{};
  g.A = z; g.lda = Ppad; g.sub = d.mpad; g.mul = nullptr; g.sub2 = nullptr;
  g.B = d.LT; g.ldb = Ppad; g.C = y; g.N = N; g.M = d.P; g.Brows = Ppad; g.D = Ppad;
  g.kstep = 0; g.klen = Ppad; g.b_zstride = (int64_t)Ppad * Ppad; g.sub_zstride = Ppad;
  if ((e = launch_gemm(g, d.K, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(emb_gmm_finish_kernel, dim3(N), dim3(256), 0, s, (const float*)y, N, d.P, d.K, d.log_const, out);
  return hipGetLastError();
}

}  // namespace dfa

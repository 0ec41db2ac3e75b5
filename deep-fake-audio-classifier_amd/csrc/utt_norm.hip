// utt_norm.hip -- per-utterance cepstral mean (CMN) and mean-and-variance (CVMN) normalisation of a float32 feature batch
// (include/dfa_hip.h: dfa_utt_norm, dfa_utt_norm_packed; src/compare_normalization.py:53-62).
//
// For utterance b, feature row c and its own n = len_b frames:
//   mean = (1/n) sum_t x[t];  cmn: y = x - mean;  cvmn: y = (x - mean) / max(sqrt(sum_t (x - mean)^2 / (n - 1)), 1e-8)
//   y[t] = +0.0f for n <= t (a select: x there is never used)
// Two-pass statistics in float64 (the mean, then the centred sum of squares: the StatsPool's rule), the
// quotient formed in float64 and rounded once.  No atomics: every sum has a fixed order that depends on n alone, so within one
// layout form a row's output is a function of its n values, n and the mode.  y == x (same strides) is allowed: every element is
// written by the thread that read it, after the last statistics read of its row.
//
// Time fastest (stride_t == 1): one wave per row, 16-byte pieces, lane l owns pieces l, l + 64, ...  A row of at most
// kHeldFrames frames stays in registers between the statistics and the write (one read and one write of the batch); a longer
// row is read again per pass.  Both add in the same order.
// Feature fastest (stride_c == 1): a workgroup owns 64 consecutive features of one utterance, lanes run over the features, wave w
// of kFeatWaves walks the frames w, w + kFeatWaves, ...; the waves' sums are merged through LDS in wave order.
#include "dfa_internal.h"

namespace dfa {

namespace {

constexpr int kTimeThreads = 256;                         // 4 waves = 4 rows per workgroup
constexpr int kHeldPieces = 4;                            // 16-byte pieces a lane keeps in registers (8: 106 VGPRs, 4 waves per SIMD, 1.3x slower)
constexpr int kHeldFrames = 64 * kHeldPieces * 4;         // = DFA_UTT_NORM_HELD_FRAMES
static_assert(kHeldFrames == DFA_UTT_NORM_HELD_FRAMES, "the row cap the header documents");
constexpr int kFeatWaves = 8;
constexpr int kFeatThreads = 64 * kFeatWaves;
constexpr double kStdFloor = 1e-8;                        // .clamp(min=1e-8)

// the sum of v over the 64 lanes, the same bits in every lane (a butterfly: each step adds the same two values in both lanes)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the floats of piece p (frames 4p .. 4p + 3) that lie behind n, as +0.0f
__device__ __forceinline__ float4 keep_front(float4 v, int p, int n) {
  const int t0 = 4 * p;
  v.x = t0 + 0 < n ? v.x : 0.f;
  v.y = t0 + 1 < n ? v.y : 0.f;
  v.z = t0 + 2 < n ? v.z : 0.f;
  v.w = t0 + 3 < n ? v.w : 0.f;
  return v;
}

__device__ __forceinline__ double sum4(double s, float4 v) {
  s += (double)v.x;
  s += (double)v.y;
  s += (double)v.z;
  s += (double)v.w;
  return s;
}

// the centred squares of the piece's frames in front of n
__device__ __forceinline__ double css4(double q, float4 v, int p, int n, double mean) {
  const int t0 = 4 * p;
  const double d0 = (double)v.x - mean, d1 = (double)v.y - mean, d2 = (double)v.z - mean, d3 = (double)v.w - mean;
  q += t0 + 0 < n ? d0 * d0 : 0.0;
  q += t0 + 1 < n ? d1 * d1 : 0.0;
  q += t0 + 2 < n ? d2 * d2 : 0.0;
  q += t0 + 3 < n ? d3 * d3 : 0.0;
  return q;
}

__device__ __forceinline__ float4 norm4(float4 v, int p, int n, double mean, double inv) {
  float4 o;
  o.x = (float)(((double)v.x - mean) * inv);
  o.y = (float)(((double)v.y - mean) * inv);
  o.z = (float)(((double)v.z - mean) * inv);
  o.w = (float)(((double)v.w - mean) * inv);
  return keep_front(o, p, n);
}

// 1 / max(sqrt(q / (n - 1)), 1e-8) for cvmn, 1 for cmn
__device__ __forceinline__ double inv_std(double q, int n) {
  const double sd = sqrt(q / (double)(n - 1));
  return 1.0 / (sd > kStdFloor ? sd : kStdFloor);
}

// One wave per row.  tab == nullptr: every row spans T_max frames.  packed == 0: row (b, c) at b stride_b + c stride_c, tab =
// [0, B) lengths, and the ceil(T_max / 4) pieces of y's row are written.  packed != 0: utterance b is C rows of pitch
// ceil(len_b / 4) * 4 from the float offset in tab[2B + 2b] (low word) and tab[2B + 2b + 1] (high word); its pitch is written.
__global__ __launch_bounds__(kTimeThreads) void utt_norm_time_kernel(const float* x, float* y,
                                                                      const int* __restrict__ tab, int mode, int B, int C, int T_max,
                                                                      int64_t stride_b, int64_t stride_c, int packed) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kTimeThreads / 64) + (threadIdx.x >> 6);
  if (row >= (int64_t)B * C) return;                      // (no barrier in this kernel)
  const int b = (int)(row / C), c = (int)(row - (int64_t)b * C);
  const int n = tab ? tab[b] : T_max;
  const int np = (n + 3) >> 2;                            // pieces read
  int64_t base;
  int wp;                                                 // pieces written
  if (packed) {
    const int64_t off = (int64_t)(((uint64_t)(uint32_t)tab[2 * B + 2 * b]) | ((uint64_t)(uint32_t)tab[2 * B + 2 * b + 1] << 32));
    base = off + (int64_t)c * (4 * (int64_t)np);
    wp = np;
  } else {
    base = (int64_t)b * stride_b + (int64_t)c * stride_c;
    wp = (T_max + 3) >> 2;
  }
  const float4* xr = reinterpret_cast<const float4*>(x + base);
  float4* yr = reinterpret_cast<float4*>(y + base);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);

  if (np <= 64 * kHeldPieces) {
    float4 v[kHeldPieces];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kHeldPieces; ++k) {
      const int p = lane + 64 * k;
      v[k] = zero;
      if (p < np) v[k] = keep_front(xr[p], p, n);
    }
#pragma unroll
    for (int k = 0; k < kHeldPieces; ++k)
      if (64 * k < np) s = sum4(s, v[k]);                 // (a piece past np holds zeros: lanes of one round add alike)
    const double mean = wave_sum(s) / (double)n;
    double inv = 1.0;
    if (mode == DFA_NORM_CVMN) {
      double q = 0.0;
#pragma unroll
      for (int k = 0; k < kHeldPieces; ++k)
        if (64 * k < np) q = css4(q, v[k], lane + 64 * k, n, mean);
      inv = inv_std(wave_sum(q), n);
    }
#pragma unroll
    for (int k = 0; k < kHeldPieces; ++k) {
      const int p = lane + 64 * k;
      if (p < np) yr[p] = norm4(v[k], p, n, mean, inv);
    }
  } else {
    double s = 0.0;
    for (int p0 = 0; p0 < np; p0 += 64) {
      const int p = p0 + lane;
      s = sum4(s, p < np ? keep_front(xr[p], p, n) : zero);
    }
    const double mean = wave_sum(s) / (double)n;
    double inv = 1.0;
    if (mode == DFA_NORM_CVMN) {
      double q = 0.0;
      for (int p0 = 0; p0 < np; p0 += 64) {
        const int p = p0 + lane;
        q = css4(q, p < np ? keep_front(xr[p], p, n) : zero, p, n, mean);
      }
      inv = inv_std(wave_sum(q), n);
    }
    for (int p = lane; p < np; p += 64) yr[p] = norm4(xr[p], p, n, mean, inv);
  }
  for (int p = np + lane; p < wp; p += 64) yr[p] = zero;
}

// Workgroup b * groups + g: features [64 g, 64 g + 64) of utterance b; element (b, t, c) at b stride_b + t stride_t + c.
__global__ __launch_bounds__(kFeatThreads) void utt_norm_feat_kernel(const float* x, float* y,
                                                                      const int* __restrict__ tab, int mode, int C, int T_max,
                                                                      int64_t stride_b, int64_t stride_t, int groups) {
  __shared__ double part[2][kFeatWaves][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x / groups;
  const int c = (blockIdx.x - b * groups) * 64 + lane;
  const bool live = c < C;
  const int n = tab ? tab[b] : T_max;
  const float* xc = x + (int64_t)b * stride_b + c;
  float* yc = y + (int64_t)b * stride_b + c;

  // four frames in flight per lane; the four sums are added as (s0 + s1) + (s2 + s3): an order of n alone
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (live) {
    int t = w;
    for (; t + 3 * kFeatWaves < n; t += 4 * kFeatWaves) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = xc[(int64_t)(t + j * kFeatWaves) * stride_t];
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += (double)v[j];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)                           // at most three frames are left
      if (t + j * kFeatWaves < n) s[j] += (double)xc[(int64_t)(t + j * kFeatWaves) * stride_t];
  }
  part[0][w][lane] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  double mean = 0.0;
#pragma unroll
  for (int k = 0; k < kFeatWaves; ++k) mean += part[0][k][lane];
  mean /= (double)n;

  double inv = 1.0;
  if (mode == DFA_NORM_CVMN) {                            // (uniform over the grid)
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
      int t = w;
      for (; t + 3 * kFeatWaves < n; t += 4 * kFeatWaves) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = xc[(int64_t)(t + j * kFeatWaves) * stride_t];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d = (double)v[j] - mean;
          q[j] += d * d;
        }
      }
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (t + j * kFeatWaves < n) {
          const double d = (double)xc[(int64_t)(t + j * kFeatWaves) * stride_t] - mean;
          q[j] += d * d;
        }
    }
    part[1][w][lane] = (q[0] + q[1]) + (q[2] + q[3]);
    __syncthreads();
    double qq = 0.0;
#pragma unroll
    for (int k = 0; k < kFeatWaves; ++k) qq += part[1][k][lane];
    inv = inv_std(qq, n);
  }
  if (!live) return;                                      // (behind the last barrier)
  for (int t = w; t < n; t += kFeatWaves) {
    const int64_t o = (int64_t)t * stride_t;
    yc[o] = (float)(((double)xc[o] - mean) * inv);
  }
  for (int t = n + w; t < T_max; t += kFeatWaves) yc[(int64_t)t * stride_t] = 0.f;
}

}  // namespace

hipError_t launch_utt_norm_time(const float* x, float* y, const int* tab, int mode, int B, int C, int T_max, int64_t stride_b,
                                int64_t stride_c, bool packed, hipStream_t s) {
  const int64_t rows = (int64_t)B * C, per = kTimeThreads / 64;
  hipLaunchKernelGGL(utt_norm_time_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(kTimeThreads), 0, s, x, y, tab, mode, B, C, T_max,
                     stride_b, stride_c, packed ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_utt_norm_feat(const float* x, float* y, const int* tab, int mode, int B, int C, int T_max, int64_t stride_b,
                                int64_t stride_t, hipStream_t s) {
  const int groups = (C + 63) / 64;
  hipLaunchKernelGGL(utt_norm_feat_kernel, dim3((unsigned)((int64_t)B * groups)), dim3(kFeatThreads), 0, s, x, y, tab, mode, C, T_max,
                     stride_b, stride_t, groups);
  return hipGetLastError();
}

}  // namespace dfa

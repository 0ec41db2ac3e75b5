// dlq.hip -- eval forward of the reference's DeepfakeDetector (src/dlqueen_model.py:115-173: three Conv1d + BatchNorm1d + GELU
// layers of 256 channels, masked mean / std pooling, a 512 -> 256 -> 1 head) on a variable-length batch.
//   * every convolution is an implicit GEMM on v_mfma_f32_32x32x16_bf16 at fp32 grade: each fp32 operand is carried as THREE bf16 terms
//     (t0 + t1 + t2 = its 24-bit mantissa: dfa_device.h, the term split) and every product is the six MFMAs of order <= 2 (w0 x0, w1 x0, w0 x1, w2 x0, w0 x2, w1 x1; fp32
//     accumulate) -- the construction of the CNN1D training kernels (train_cnn1d.hip).  Two terms (hi + lo, three MFMAs: bf16x3) carry 16
//     bits: 2^-17 per operand, which a float64 emulation of this network put at 4.6e-6 of the largest logit before any cancellation in
//     the head -- no margin under the 2^-17 parity bound;
//   * a workgroup (4 waves) owns one tile of NF = 64 frames of one utterance and all 256 output channels: wave w owns channels
//     [64 w, 64 w + 64) as two 32-row A tiles times two 32-frame B tiles (64 accumulator registers);
//   * the input tile (NF frames + the taps' halo) sits in LDS as split pixels [t0 256 bf16 | t1 256 bf16 | t2 256 bf16] (1.5 KB per frame,
//     16-byte chunk c of slot s at chunk c ^ (s & 15), the swizzle of conv3x3_mfma.h for 1 KB pixels) and is shared by the four waves; the
//     weights are NOT shared -- each wave owns its output channels -- so they go from L2 straight to registers in fragment order, one
//     k-step ahead (3.7 MB of images for the three layers, 1.4 MB for the largest: resident in L2, 24 KB per k-step per workgroup);
//   * between layers the activations live in the workspace frame-major in the same pixel form; only the frames that exist for an
//     utterance are written, and only those are read (everything else is the convolution's zero padding):
//        h1 on frames < min(T_max, len + 2), h2 on frames < min(T_max, len + 1), h3 on frames < len -- the padded-batch rule
//        (the reference's encoder is not masked, only its pool is);
//   * layer 1 reads x[b][c][t] (fp32, time fastest) with 16-byte row loads, frames >= len taken as zero without using what was loaded;
//   * layer 3 never stores h3: its epilogue leaves per tile and channel (mean, M2) over the tile's valid frames (two passes over the
//     tile in LDS, frame order), and dlq_finish_kernel merges an utterance's tiles in tile order (Chan's formula), clamps, takes the
//     square root and runs the head in fp32.  No atomics anywhere: a logit is a fixed-order function of its utterance.
// Tiles are dispatched from a table the host builds from the lengths (longest utterance first): a short utterance costs few tiles.
#include "dfa_internal.h"
#include "dlq_common.h"

namespace dfa {

// ---- weight preparation: BatchNorm folded into the convolution (float64), three-term bf16 A-fragment images ------------------------
// wp[k][wave][m][term][lane] (uint4), k = tap * nks + ks, term 0 .. 2; lane: co = 64 wave + 32 m + (lane & 31), element j <->
// input channel 16 ks + 8 (lane >> 5) + j (zero beyond cin).  bias[co] = (b - mean) * scale + beta.
__global__ void dlq_pack_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ g,
                                const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
                                uint4* __restrict__ wp, float* __restrict__ bias, int cin, int taps, int nks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int total = taps * nks * 8 * 64;
  if (i < dlq::HID) {
    const double sc = (double)g[i] / sqrt((double)var[i] + (double)kBnEps);
    bias[i] = (float)(((double)b[i] - (double)mean[i]) * sc + (double)beta[i]);
  }
  if (i >= total) return;
  const int lane = i & 63, m = (i >> 6) & 1, wave = (i >> 7) & 3, k = i >> 9;
  const int tap = k / nks, ks = k % nks;
  const int co = 64 * wave + 32 * m + (lane & 31), hh = lane >> 5;
  const double sc = (double)g[co] / sqrt((double)var[co] + (double)kBnEps);
  bf16_t t0[8], t1[8], t2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = 16 * ks + 8 * hh + j;
    const float wf = ci < cin ? (float)((double)w[((size_t)co * cin + ci) * taps + tap] * sc) : 0.f;
    t0[j] = float_to_bf16(wf);
    const float r1 = wf - bf16_to_float(t0[j]);
    t1[j] = float_to_bf16(r1);
    t2[j] = float_to_bf16(r1 - bf16_to_float(t1[j]));
  }
  uint4* dst = wp + ((size_t)(k * 4 + wave) * 6 + m * 3) * 64 + lane;
  dst[0] = *reinterpret_cast<const uint4*>(t0);
  dst[64] = *reinterpret_cast<const uint4*>(t1);
  dst[128] = *reinterpret_cast<const uint4*>(t2);
}

int dlq_nks(int cin) { return (cin + 15) / 16; }
size_t dlq_pack_bytes(int cin, int taps) { return (size_t)taps * dlq_nks(cin) * 4 * 6 * 64 * 16; }
hipError_t launch_dlq_pack(const LayerParams& lp, int cin, int taps, void* wp, float* bias, hipStream_t s) {
  const int total = taps * dlq_nks(cin) * 8 * 64;
  hipLaunchKernelGGL(dlq_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, s, lp.w, lp.b, lp.gamma, lp.beta, lp.rmean, lp.rvar, (uint4*)wp, bias,
                     cin, taps, dlq_nks(cin));
  return hipGetLastError();
}

// ---- one layer ---------------------------------------------------------------------------------------------------------------------

// dispatch position of workgroup `blk`: the last i with first[i] <= blk
__device__ __forceinline__ int dlq_find(const int* first, int B, int blk) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// MODE 0: the eval forward described above.  The training step (dlq_train.hip) runs the same loop DENSE -- every
// utterance owns ceil(T_max / NF) tiles at every layer, workgroup = b * tpu + tile -- with its own epilogues:
//   MODE 1 (train forward): z = conv + bias in fp32 frame-major [B][T_max][256] and the tile's per-channel (mean, M2) over its frames;
//   MODE 2 (data gradient, LAYER 2's shape on the data-gradient image with dz as input): dh of the layer below, turned into
//          dy = dh * keep / (1 - p) * GELU'(gamma zhat + beta) there (fp32 frame-major) with the tile's per-channel (sum dy, sum dy zhat).
template <int LAYER, int MODE>
__global__ __launch_bounds__(dlq::NTH) void dlq_layer_kernel(const DlqLayerArgs a) {
  using namespace dlq;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int TAPS = LAYER == 1 ? 5 : 3, HALO = TAPS / 2, EXT = LAYER == 1 ? 2 : (LAYER == 2 ? 1 : 0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
  const int blk = blockIdx.x, B = a.B;
  int b, tile;
  if (MODE == 0) {
    const int pos = dlq_find(a.tab + 3 * B, B, blk);
    b = a.tab[2 * B + pos];
    tile = blk - a.tab[3 * B + pos];
  } else {
    b = blk / a.tpu;
    tile = blk - b * a.tpu;
  }
  const int len = a.tab[b];
  const int t0 = tile * NF;
  const int e_out = MODE == 0 ? min(a.T_max, len + EXT) : a.T_max;   // frames of this layer's output that exist
  if (t0 >= e_out) return;                         // (the tile list is layer 1's; the later layers have fewer frames)
  const int nact = e_out - t0 > 32 ? 2 : 1;        // 32-frame B tiles that hold an existing frame

  // ---- stage the input tile: slot s <-> frame t0 - HALO + s, zero where the input does not exist
  uint4* lds4 = reinterpret_cast<uint4*>(lds);
  if (LAYER == 1) {
    // x rows in groups of 4 frames (16-byte loads, aligned: t0 % 4 == 0), two channels per item -> one 32-bit word per term and frame
    constexpr int NG = NF / 4 + 2;                 // frame groups [t0 - 4, t0 + NF + 4)
    const int npair = 8 * a.nks;
    const float* xb = a.x + (size_t)b * a.sb;
    for (int i = tid; i < npair * NG; i += NTH) {
      const int p = i / NG, g = i - p * NG;
      const int f4 = t0 - 4 + 4 * g, c = 2 * p;
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
      if (f4 >= 0 && f4 < len && c < a.C) {        // (f4 + 3 < sc: rows are whole 16-byte groups)
        v0 = *reinterpret_cast<const float4*>(xb + (size_t)c * a.sc + f4);
        v1 = *reinterpret_cast<const float4*>(xb + (size_t)(c + 1) * a.sc + f4);
      }
      const float r0[4] = {v0.x, v0.y, v0.z, v0.w}, r1[4] = {v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int f = f4 + j, s = f - (t0 - HALO);
        if (s < 0 || s >= NF + 2 * HALO) continue;
        const bool in = f < len;                   // a select, never a product: the padding may hold NaN
        const float u0 = in ? r0[j] : 0.f, u1 = in ? r1[j] : 0.f;
        unsigned w0, w1, w2;
        split3_pair(u0, u1, w0, w1, w2);
        const int ch = p >> 2, sw = s & 15;        // chunk of 8 channels = 4 pairs
        unsigned* px = reinterpret_cast<unsigned*>(lds + s * PIXB);
        px[((ch ^ sw) << 2) + (p & 3)] = w0;
        px[(((32 + ch) ^ sw) << 2) + (p & 3)] = w1;
        px[(((64 + ch) ^ sw) << 2) + (p & 3)] = w2;
      }
    }
  } else {
    const int e_in = MODE == 0 ? min(a.T_max, len + EXT + 1) : a.T_max;  // frames of the previous layer's output that exist
    const uint4* src = a.hin + (size_t)b * a.T_max * PIXC;
    for (int i = tid; i < (NF + 2 * HALO) * PIXC; i += NTH) {
      const int s = i / PIXC, ch = i - s * PIXC, f = t0 - HALO + s;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (f >= 0 && f < e_in) v = src[(size_t)f * PIXC + ch];
      lds4[s * PIXC + (ch ^ (s & 15))] = v;
    }
  }
  __syncthreads();

  // ---- the GEMM: k-steps of 16 input channels of one tap; A fragments one step ahead in registers
  f32x16_t acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
  const int nks = a.nks, nk = TAPS * nks;
  const uint4* wp = a.w + (size_t)wave * 6 * 64 + lane;
  uint4 af[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) af[q] = wp[q * 64];
  int tap = 0, ks = 0;
  for (int k = 0; k < nk; ++k) {
    uint4 an[6];
    if (k + 1 < nk) {
      const uint4* wn = wp + (size_t)(k + 1) * 24 * 64;
#pragma unroll
      for (int q = 0; q < 6; ++q) an[q] = wn[q * 64];
    } else {
#pragma unroll
      for (int q = 0; q < 6; ++q) an[q] = af[q];
    }
    uint4 xf[2][3];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int s = n * 32 + col + tap, sw = s & 15;
#pragma unroll
      for (int t = 0; t < 3; ++t) xf[n][t] = lds4[s * PIXC + ((32 * t + 2 * ks + h) ^ sw)];
    }
    // the six products of order <= 2, smallest first
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if (n >= nact) continue;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const uint4 *w3 = af + 3 * m;
        acc[m][n] = mma32(w3[1], xf[n][1], acc[m][n]);
        acc[m][n] = mma32(w3[2], xf[n][0], acc[m][n]);
        acc[m][n] = mma32(w3[0], xf[n][2], acc[m][n]);
        acc[m][n] = mma32(w3[1], xf[n][0], acc[m][n]);
        acc[m][n] = mma32(w3[0], xf[n][1], acc[m][n]);
        acc[m][n] = mma32(w3[0], xf[n][0], acc[m][n]);
      }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) af[q] = an[q];
    if (++ks == nks) { ks = 0; ++tap; }
  }

  // ---- epilogue: lane = frame, registers 4 g .. 4 g + 3 = channels co0 + 8 g + 4 h + (0 .. 3)
  if (MODE != 0) {
    // the tile through LDS as float [channel][NF + 1]; then thread = channel walks the tile's frames in order (coalesced over channels)
    __syncthreads();                               // every wave is done with the input tile
    float* tile_f = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if (n >= nact) continue;
      const int fc = n * 32 + col;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = 64 * wave + 32 * m + 8 * g + 4 * h;
          float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
          if (MODE == 1) bv = *reinterpret_cast<const float4*>(a.bias + co);
          tile_f[(co + 0) * (NF + 1) + fc] = acc[m][n][4 * g] + bv.x;
          tile_f[(co + 1) * (NF + 1) + fc] = acc[m][n][4 * g + 1] + bv.y;
          tile_f[(co + 2) * (NF + 1) + fc] = acc[m][n][4 * g + 2] + bv.z;
          tile_f[(co + 3) * (NF + 1) + fc] = acc[m][n][4 * g + 3] + bv.w;
        }
    }
    __syncthreads();
    const int cnt = min(NF, a.T_max - t0);         // >= 1, and <= 32 when nact == 1
    const float* row = tile_f + tid * (NF + 1);
    const size_t fr0 = (size_t)b * a.T_max + t0;   // the tile's first frame in the batch
    float* out = a.zout + fr0 * HID + tid;
    float* rec = a.rec + (size_t)blk * 2 * HID;
    if (MODE == 1) {
      float sum = 0.f;
      for (int f = 0; f < cnt; ++f) {
        sum += row[f];
        out[(size_t)f * HID] = row[f];
      }
      const float mean = sum / (float)cnt;
      float m2 = 0.f;
      for (int f = 0; f < cnt; ++f) {
        const float d = row[f] - mean;
        m2 += d * d;
      }
      rec[tid] = mean;
      rec[HID + tid] = m2;
    } else {
      const float mu = a.st_mean[tid], is = a.st_invstd[tid], ga = a.gamma[tid], be = a.beta[tid];
      const float* zp = a.zprev + fr0 * HID + tid;
      float s1 = 0.f, s2 = 0.f;
      for (int f = 0; f < cnt; ++f) {
        const float zh = (zp[(size_t)f * HID] - mu) * is;
        const float dy = row[f] * drop_scale1(a.drop, (fr0 + f) * HID + tid) * dlq_dgelu(ga * zh + be);
        out[(size_t)f * HID] = dy;
        s1 += dy;
        s2 += dy * zh;
      }
      rec[2 * tid] = s1;                           // [channel][2]: the record form of launch_reduce_partials / launch_split_sums
      rec[2 * tid + 1] = s2;
    }
  } else if (LAYER != 3) {
    char* dst = reinterpret_cast<char*>(a.hout + (size_t)b * a.T_max * PIXC);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int f = t0 + n * 32 + col;
      if (n >= nact || f >= e_out) continue;
      char* px = dst + (size_t)f * PIXB;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = 64 * wave + 32 * m + 8 * g + 4 * h;
          const float4 bv = *reinterpret_cast<const float4*>(a.bias + co);
          const float v0 = dlq_gelu(acc[m][n][4 * g] + bv.x), v1 = dlq_gelu(acc[m][n][4 * g + 1] + bv.y);
          const float v2 = dlq_gelu(acc[m][n][4 * g + 2] + bv.z), v3 = dlq_gelu(acc[m][n][4 * g + 3] + bv.w);
          unsigned p0, p1, p2, q0, q1, q2;
          split3_pair(v0, v1, p0, p1, p2);
          split3_pair(v2, v3, q0, q1, q2);
          *reinterpret_cast<uint2*>(px + 2 * co) = make_uint2(p0, q0);
          *reinterpret_cast<uint2*>(px + 2 * HID + 2 * co) = make_uint2(p1, q1);
          *reinterpret_cast<uint2*>(px + 4 * HID + 2 * co) = make_uint2(p2, q2);
        }
    }
  } else {
    // pool statistics of the tile: h3 through LDS as float [channel][NF + 1], then thread = channel walks its valid frames in order
    __syncthreads();                               // every wave is done with the input tile
    float* tile_f = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if (n >= nact) continue;
      const int fc = n * 32 + col;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = 64 * wave + 32 * m + 8 * g + 4 * h;
          const float4 bv = *reinterpret_cast<const float4*>(a.bias + co);
          tile_f[(co + 0) * (NF + 1) + fc] = dlq_gelu(acc[m][n][4 * g] + bv.x);
          tile_f[(co + 1) * (NF + 1) + fc] = dlq_gelu(acc[m][n][4 * g + 1] + bv.y);
          tile_f[(co + 2) * (NF + 1) + fc] = dlq_gelu(acc[m][n][4 * g + 2] + bv.z);
          tile_f[(co + 3) * (NF + 1) + fc] = dlq_gelu(acc[m][n][4 * g + 3] + bv.w);
        }
    }
    __syncthreads();
    const int cnt = min(NF, len - t0);             // >= 1, and <= 32 when nact == 1
    const float* row = tile_f + tid * (NF + 1);
    float sum = 0.f;
    for (int f = 0; f < cnt; ++f) sum += row[f];
    const float mean = sum / (float)cnt;
    float m2 = 0.f;
    for (int f = 0; f < cnt; ++f) {
      const float d = row[f] - mean;
      m2 += d * d;
    }
    float* out = a.part + (size_t)blk * 2 * HID;
    out[tid] = mean;
    out[HID + tid] = m2;
  }
}

hipError_t launch_dlq_layer(int layer, const DlqLayerArgs& a, int ntiles, hipStream_t s) {
  void (*const kerns[])(DlqLayerArgs) = {dlq_layer_kernel<1, 0>, dlq_layer_kernel<2, 0>, dlq_layer_kernel<3, 0>};
  return launch_lds(kerns[layer == 1 ? 0 : layer == 2 ? 1 : 2], dim3(ntiles), dim3(dlq::NTH), dlq::LDS_BYTES, s, a);
}

// mode 1: the train forward of `layer`; mode 2: the data gradient (layer 2's shape).  ntiles = B * a.tpu
hipError_t launch_dlq_layer_train(int layer, int mode, const DlqLayerArgs& a, int ntiles, hipStream_t s) {
  void (*const kerns[])(DlqLayerArgs) = {dlq_layer_kernel<2, 2>, dlq_layer_kernel<1, 1>, dlq_layer_kernel<2, 1>, dlq_layer_kernel<3, 1>};
  return launch_lds(kerns[mode == 2 ? 0 : layer == 1 ? 1 : layer == 2 ? 2 : 3], dim3(ntiles), dim3(dlq::NTH), dlq::LDS_BYTES, s, a);
}

// ---- pool + head: workgroup = dispatch position, thread = channel ------------------------------------------------------------------
__global__ __launch_bounds__(256) void dlq_finish_kernel(const float* __restrict__ part, const int* __restrict__ tab, const float* __restrict__ w0,
                                                         const float* __restrict__ b0, const float* __restrict__ w3, const float* __restrict__ b3,
                                                         float* __restrict__ logits, float* __restrict__ pooled, int B) {
  using namespace dlq;
  __shared__ float z[2 * HID];
  __shared__ float hb[HID];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pos = blockIdx.x, b = tab[2 * B + pos], len = tab[b], first = tab[3 * B + pos];
  const int ntile = (len + NF - 1) / NF;
  // tiles in order: (n, mean, M2) <- merge with (n_t, mean_t, M2_t)
  float n = 0.f, mean = 0.f, m2 = 0.f;
  for (int t = 0; t < ntile; ++t) {
    const float* p = part + (size_t)(first + t) * 2 * HID;
    const float nt = (float)min(NF, len - t * NF), mt = p[tid], qt = p[HID + tid];
    if (t == 0) { n = nt; mean = mt; m2 = qt; continue; }
    const float tot = n + nt, d = mt - mean;
    mean = mean + d * (nt / tot);
    m2 = m2 + qt + d * d * (n * nt / tot);
    n = tot;
  }
  const float var = m2 / (float)len;
  // (float) of the float64 root is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits); the fp32 intrinsics compile to a bare
  // v_sqrt_f32, which is one ulp off at 1e-6: len = 1 must give fl(1e-3) as torch.sqrt(var.clamp(1e-6)) does
  const float sd = (float)sqrt((double)fmaxf(var, 1e-6f));
  z[tid] = mean;
  z[HID + tid] = sd;
  if (pooled) {
    pooled[(size_t)b * 2 * HID + tid] = mean;
    pooled[(size_t)b * 2 * HID + HID + tid] = sd;
  }
  __syncthreads();
  // Linear(512 -> 256) + GELU: a wave per row, lanes along k (coalesced), a fixed xor tree
  for (int r = 0; r < 64; ++r) {
    const int row = wave * 64 + r;
    const float* wr = w0 + (size_t)row * 2 * HID;
    float sacc = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) sacc += wr[q * 64 + lane] * z[q * 64 + lane];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sacc += __shfl_xor(sacc, o, 64);
    if (lane == 0) hb[row] = dlq_gelu(sacc + b0[row]);
  }
  __syncthreads();
  // Linear(256 -> 1): a fixed tree in LDS
  z[tid] = hb[tid] * w3[tid];
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) z[tid] += z[tid + o];
    __syncthreads();
  }
  if (tid == 0) logits[b] = z[0] + b3[0];
}

hipError_t launch_dlq_finish(const float* part, const int* tab, const float* w0, const float* b0, const float* w3, const float* b3, float* logits,
                             float* pooled, int B, hipStream_t s) {
  hipLaunchKernelGGL(dlq_finish_kernel, dim3(B), dim3(256), 0, s, part, tab, w0, b0, w3, b3, logits, pooled, B);
  return hipGetLastError();
}

}  // namespace dfa

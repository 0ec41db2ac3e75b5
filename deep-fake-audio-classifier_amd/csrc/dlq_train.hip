// dlq_train.hip -- the DeepfakeDetector training step's kernels besides the layer kernel (dlq.hip, MODE 1 / 2): the reference's step
// (src/dlqueen_model.py:115-173 in train mode, 255-330) without AMP, DENSE over the padded batch -- BatchNorm1d counts all
// N = B T_max frames, padding included, as the reference's unmasked encoder does; only the pool is masked.
//   * weight images: one launch packs the three forward images (dlq.hip's A-fragment layout, no BatchNorm folded) and the two
//     data-gradient images W'[c][o][k'] = W[o][c][2 - k'] of layers 3 and 2;
//   * BatchNorm statistics: the layer kernel leaves (mean, M2) per tile and channel; dlq_bn_finalize_kernel merges them in tile order
//     (Chan's formula, float64) -- no shift is needed, a tile's M2 is already centred;
//   * BN + GELU + dropout of layers 1, 2 in one pass z -> split pixels; layer 3's inside the pool (thread = channel, frame order, two
//     passes), followed by the head in the same workgroup;
//   * backward: head (two small kernels), pool backward + layer-3 dy, then per layer the (sum dy, sum dy zhat) reduction, the dz pass
//     (split pixels, the form the data gradient and the weight gradient read, plus the conv-bias records), the weight gradient (a
//     three-term MFMA GEMM over frame chunks with K = B T_max, operands transposed through LDS) and the data gradient (dlq.hip MODE 2);
//   * the keep factor of an element is a pure function of (seed, offset, layer, index): regenerated, never stored.
// No atomics: every reduction is per-workgroup records plus a fixed-order second stage.
#include "dlq_common.h"

namespace dfa {

using namespace dlq;

// ---- weight images ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dlq_train_pack_kernel(const DlqPackJobs jobs) {
  int job = 0;
  while (job < 4 && (int)blockIdx.x >= jobs.first[job + 1]) ++job;
  const int cin = jobs.cin[job], taps = jobs.taps[job], nks = (cin + 15) / 16, dg = jobs.dgrad[job];
  const int i = ((int)blockIdx.x - jobs.first[job]) * 256 + threadIdx.x;
  if (i >= taps * nks * 8 * 64) return;
  const float* __restrict__ w = jobs.w[job];
  const int lane = i & 63, m = (i >> 6) & 1, wave = (i >> 7) & 3, k = i >> 9;
  const int tap = k / nks, ks = k % nks;
  const int co = 64 * wave + 32 * m + (lane & 31), hh = lane >> 5;
  bf16_t t0[8], t1[8], t2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ci = 16 * ks + 8 * hh + j;
    float wf = 0.f;
    if (ci < cin) wf = dg ? w[((size_t)ci * HID + co) * 3 + (2 - tap)] : w[((size_t)co * cin + ci) * taps + tap];
    t0[j] = float_to_bf16(wf);
    const float r1 = wf - bf16_to_float(t0[j]);
    t1[j] = float_to_bf16(r1);
    t2[j] = float_to_bf16(r1 - bf16_to_float(t1[j]));
  }
  uint4* dst = jobs.dst[job] + ((size_t)(k * 4 + wave) * 6 + m * 3) * 64 + lane;
  dst[0] = *reinterpret_cast<const uint4*>(t0);
  dst[64] = *reinterpret_cast<const uint4*>(t1);
  dst[128] = *reinterpret_cast<const uint4*>(t2);
}

hipError_t launch_dlq_train_pack(const float* w1, const float* w2, const float* w3, void* const* dst, int in_ch, hipStream_t s) {
  DlqPackJobs j{};
  const float* w[5] = {w1, w2, w3, w3, w2};
  const int cin[5] = {in_ch, HID, HID, HID, HID}, taps[5] = {5, 3, 3, 3, 3}, dg[5] = {0, 0, 0, 1, 1};
  int nb = 0;
  for (int q = 0; q < 5; ++q) {
    j.w[q] = w[q]; j.dst[q] = (uint4*)dst[q]; j.cin[q] = cin[q]; j.taps[q] = taps[q]; j.dgrad[q] = dg[q];
    j.first[q] = nb;
    nb += (taps[q] * dlq_nks(cin[q]) * 8 * 64 + 255) / 256;
  }
  j.first[5] = nb;
  hipLaunchKernelGGL(dlq_train_pack_kernel, dim3(nb), dim3(256), 0, s, j);
  return hipGetLastError();
}

// ---- BatchNorm statistics from the tile records --------------------------------------------------------------------------------------
// block = 32 channels x 8 tile lanes: lane q merges tiles q, q + 8, ... in order, then lane 0 merges the eight in order
__global__ __launch_bounds__(256) void dlq_bn_finalize_kernel(const float* __restrict__ rec, int ntiles, int tpu, int T_max, float* __restrict__ mean,
                                                              float* __restrict__ var, float* __restrict__ invstd, float* __restrict__ rm,
                                                              float* __restrict__ rv, float momentum) {
  __shared__ double sn[8][32], sm[8][32], sq[8][32];
  const int cl = threadIdx.x & 31, q = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
  double n = 0.0, mu = 0.0, m2 = 0.0;
  for (int t = q; t < ntiles; t += 8) {
    const double nt = (double)min(NF, T_max - (t % tpu) * NF), mt = (double)rec[(size_t)t * 2 * HID + c], qt = (double)rec[(size_t)t * 2 * HID + HID + c];
    const double tot = n + nt, d = mt - mu;
    mu += d * (nt / tot);
    m2 += qt + d * d * (n * nt / tot);
    n = tot;
  }
  sn[q][cl] = n; sm[q][cl] = mu; sq[q][cl] = m2;
  __syncthreads();
  if (q != 0) return;
  for (int r = 1; r < 8; ++r) {
    const double nt = sn[r][cl];
    if (nt == 0.0) continue;
    const double tot = n + nt, d = sm[r][cl] - mu;
    mu += d * (nt / tot);
    m2 += sq[r][cl] + d * d * (n * nt / tot);
    n = tot;
  }
  const double v = m2 / n;
  mean[c] = (float)mu;
  var[c] = (float)v;
  invstd[c] = (float)(1.0 / sqrt(v + (double)kBnEps));
  if (rm) {
    rm[c] = (float)((1.0 - momentum) * (double)rm[c] + momentum * mu);
    rv[c] = (float)((1.0 - momentum) * (double)rv[c] + momentum * (v * n / (n - 1.0)));      // n >= 2: checked by the entry point
  }
}

hipError_t launch_dlq_bn_finalize(const float* rec, int ntiles, int tpu, int T_max, float* mean, float* var, float* invstd, float* rm, float* rv,
                                  float momentum, hipStream_t s) {
  hipLaunchKernelGGL(dlq_bn_finalize_kernel, dim3(HID / 32), dim3(256), 0, s, rec, ntiles, tpu, T_max, mean, var, invstd, rm, rv, momentum);
  return hipGetLastError();
}

// ---- BN + GELU + dropout, z -> split pixels (layers 1, 2): thread = one frame's 8 channels (one Philox call) --------------------------
__device__ __forceinline__ void dlq_store_pixel8(uint4* px, int g, const float* v) {
  unsigned a[4], b[4], c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) split3_pair(v[2 * j], v[2 * j + 1], a[j], b[j], c[j]);
  px[g] = make_uint4(a[0], a[1], a[2], a[3]);
  px[32 + g] = make_uint4(b[0], b[1], b[2], b[3]);
  px[64 + g] = make_uint4(c[0], c[1], c[2], c[3]);
}

__global__ __launch_bounds__(256) void dlq_bn_act_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, uint4* __restrict__ h,
                                                         unsigned char* __restrict__ keep_out, long long N, DropCfg dc) {
  const int g = threadIdx.x & 31;
  const long long n = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (n >= N) return;
  const float* zp = z + (size_t)n * HID + 8 * g;
  const float4 z0 = *reinterpret_cast<const float4*>(zp), z1 = *reinterpret_cast<const float4*>(zp + 4);
  const float zv[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
  float kf[8], v[8];
  drop_scale8(dc, (uint64_t)n * HID + 8 * g, kf);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * g + j;
    v[j] = kf[j] * dlq_gelu(gamma[c] * ((zv[j] - mean[c]) * invstd[c]) + beta[c]);
  }
  dlq_store_pixel8(h + (size_t)n * PIXC, g, v);
  if (keep_out) {
#pragma unroll
    for (int j = 0; j < 8; ++j) keep_out[(size_t)n * HID + 8 * g + j] = kf[j] != 0.f;
  }
}

hipError_t launch_dlq_bn_act(const float* z, const BnApply& bn, void* h, unsigned char* keep_out, long long N, const DropCfg& dc, hipStream_t s) {
  hipLaunchKernelGGL(dlq_bn_act_kernel, dim3((unsigned)((N + 7) / 8)), dim3(256), 0, s, z, bn.mean, bn.invstd, bn.gamma, bn.beta, (uint4*)h, keep_out,
                     N, dc);
  return hipGetLastError();
}

// ---- layer 3's BN + GELU + dropout, the pool and the head: workgroup = utterance, thread = channel ------------------------------------
__global__ __launch_bounds__(256) void dlq_pool_head_kernel(const DlqHeadArgs a) {
  __shared__ float zs[2 * HID];
  __shared__ float hb[HID];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, T = a.T_max, len = a.lens[b];
  const float mu = a.mean[tid], is = a.invstd[tid], ga = a.gamma[tid], be = a.beta[tid];
  const float* zp = a.z3 + (size_t)b * T * HID + tid;
  const uint64_t i0 = (uint64_t)b * T * HID + tid;
  float sum = 0.f;
  for (int t = 0; t < len; ++t) sum += drop_scale1(a.drop, i0 + (uint64_t)t * HID) * dlq_gelu(ga * ((zp[(size_t)t * HID] - mu) * is) + be);
  const float pm = sum / (float)len;
  float m2 = 0.f;
  for (int t = 0; t < len; ++t) {
    const float d = drop_scale1(a.drop, i0 + (uint64_t)t * HID) * dlq_gelu(ga * ((zp[(size_t)t * HID] - mu) * is) + be) - pm;
    m2 += d * d;
  }
  const float var = m2 / (float)len;
  const float sd = (float)sqrt((double)fmaxf(var, 1e-6f));      // correctly rounded, as dlq_finish_kernel's
  zs[tid] = pm;
  zs[HID + tid] = sd;
  a.pooled[(size_t)b * 2 * HID + tid] = pm;
  a.pooled[(size_t)b * 2 * HID + HID + tid] = sd;
  a.pvar[(size_t)b * HID + tid] = var;
  if (a.keep3)       // the test hook shows the draw of every frame; the pool used those of frames < len
    for (int t = 0; t < T; ++t) a.keep3[i0 + (uint64_t)t * HID] = drop_scale1(a.drop, i0 + (uint64_t)t * HID) != 0.f;
  __syncthreads();
  for (int r = 0; r < 64; ++r) {
    const int row = wave * 64 + r;
    const float* wr = a.w0 + (size_t)row * 2 * HID;
    float sacc = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) sacc += wr[q * 64 + lane] * zs[q * 64 + lane];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sacc += __shfl_xor(sacc, o, 64);
    if (lane == 0) hb[row] = sacc + a.b0[row];
  }
  __syncthreads();
  DropCfg dh = a.drop;
  dh.layer = 4;
  const float u = hb[tid], kf = drop_scale1(dh, (uint64_t)b * HID + tid);
  a.u[(size_t)b * HID + tid] = u;
  if (a.keep4) a.keep4[(size_t)b * HID + tid] = kf != 0.f;
  __syncthreads();
  zs[tid] = kf * dlq_gelu(u) * a.w3[tid];
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) zs[tid] += zs[tid + o];
    __syncthreads();
  }
  if (tid == 0) a.logits[b] = zs[0] + a.b3[0];
}

hipError_t launch_dlq_pool_head(const DlqHeadArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(dlq_pool_head_kernel, dim3(B), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- loss: BCEWithLogitsLoss(pos_weight), mean over the batch, and its gradient -------------------------------------------------------
__global__ __launch_bounds__(256) void dlq_bce_pw_kernel(const float* __restrict__ logits, const float* __restrict__ y, float pw, int B,
                                                         float* __restrict__ loss, float* __restrict__ dlogits) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int b = tid; b < B; b += 256) {
    const float l = logits[b], yy = y[b];
    const float sp = log1pf(expf(-fabsf(l)));
    const float ls_pos = fminf(l, 0.f) - sp, ls_neg = fminf(-l, 0.f) - sp;      // log sigmoid(l), log sigmoid(-l)
    acc += -(double)(pw * yy * ls_pos + (1.f - yy) * ls_neg);
    const float sg = 1.f / (1.f + expf(-l));
    if (dlogits) dlogits[b] = (sg * (1.f + (pw - 1.f) * yy) - pw * yy) / (float)B;
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0 && loss) loss[0] = (float)(red[0] / (double)B);
}

hipError_t launch_bce_pos_weight(const float* logits, const float* labels, float pw, int B, float* loss, float* dlogits, hipStream_t s) {
  hipLaunchKernelGGL(dlq_bce_pw_kernel, dim3(1), dim3(256), 0, s, logits, labels, pw, B, loss, dlogits);
  return hipGetLastError();
}

// ---- head backward --------------------------------------------------------------------------------------------------------------------
// workgroup = utterance: du = dlogit w3 keep / (1 - p) GELU'(u), then dpooled = du W0 (thread = pooled column, rows in order)
__global__ __launch_bounds__(256) void dlq_head_bwd_a_kernel(const DlqHeadArgs a) {
  __shared__ float dus[HID];
  const int tid = threadIdx.x, b = blockIdx.x;
  DropCfg dh = a.drop;
  dh.layer = 4;
  const float du = a.dlogits[b] * a.w3[tid] * drop_scale1(dh, (uint64_t)b * HID + tid) * dlq_dgelu(a.u[(size_t)b * HID + tid]);
  dus[tid] = du;
  a.du[(size_t)b * HID + tid] = du;
  __syncthreads();
  for (int i = tid; i < 2 * HID; i += 256) {
    float acc = 0.f;
    for (int j = 0; j < HID; ++j) acc += dus[j] * a.w0[(size_t)j * 2 * HID + i];
    a.dpooled[(size_t)b * 2 * HID + i] = acc;
  }
}
// workgroup = head row j: dW0[j][:], db0[j], dW3[j] (and db3 in row 0), the batch in order
__global__ __launch_bounds__(256) void dlq_head_bwd_w_kernel(const DlqHeadArgs a, int B, float* __restrict__ dw0, float* __restrict__ db0,
                                                             float* __restrict__ dw3, float* __restrict__ db3) {
  const int tid = threadIdx.x, j = blockIdx.x;
  for (int i = tid; i < 2 * HID; i += 256) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += a.du[(size_t)b * HID + j] * a.pooled[(size_t)b * 2 * HID + i];
    dw0[(size_t)j * 2 * HID + i] = acc;
  }
  if (tid == 0) {
    DropCfg dh = a.drop;
    dh.layer = 4;
    float s0 = 0.f, s3 = 0.f, sl = 0.f;
    for (int b = 0; b < B; ++b) {
      s0 += a.du[(size_t)b * HID + j];
      s3 += a.dlogits[b] * drop_scale1(dh, (uint64_t)b * HID + j) * dlq_gelu(a.u[(size_t)b * HID + j]);
      sl += a.dlogits[b];
    }
    db0[j] = s0;
    dw3[j] = s3;
    if (j == 0) db3[0] = sl;
  }
}

hipError_t launch_dlq_head_bwd(const DlqHeadArgs& a, int B, float* dw0, float* db0, float* dw3, float* db3, hipStream_t s) {
  hipLaunchKernelGGL(dlq_head_bwd_a_kernel, dim3(B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(dlq_head_bwd_w_kernel, dim3(HID), dim3(256), 0, s, a, B, dw0, db0, dw3, db3);
  return hipGetLastError();
}

// ---- pool backward + layer 3's dy: workgroup = tile, thread = channel -----------------------------------------------------------------
// dh3[t < len] = dmean / len + dstd (h - mean) / (len std), the dstd term dropped where var < 1e-6 (the clamp's gradient); zero on padding
__global__ __launch_bounds__(256) void dlq_dy3_kernel(const DlqHeadArgs a, int tpu, float* __restrict__ dy, float* __restrict__ rec) {
  const int tid = threadIdx.x, blk = blockIdx.x, b = blk / tpu, t0 = (blk - b * tpu) * NF, T = a.T_max, len = a.lens[b];
  const int cnt = min(NF, T - t0);
  const float mu = a.mean[tid], is = a.invstd[tid], ga = a.gamma[tid], be = a.beta[tid];
  const float pm = a.pooled[(size_t)b * 2 * HID + tid], sd = a.pooled[(size_t)b * 2 * HID + HID + tid], var = a.pvar[(size_t)b * HID + tid];
  const float dm = a.dpooled[(size_t)b * 2 * HID + tid] / (float)len;
  const float ds = var < 1e-6f ? 0.f : a.dpooled[(size_t)b * 2 * HID + HID + tid] / ((float)len * sd);
  const size_t i0 = ((size_t)b * T + t0) * HID + tid;
  float s1 = 0.f, s2 = 0.f;
  for (int f = 0; f < cnt; ++f) {
    const size_t i = i0 + (size_t)f * HID;
    float d = 0.f, zh = 0.f;
    if (t0 + f < len) {
      zh = (a.z3[i] - mu) * is;
      const float v = ga * zh + be, kf = drop_scale1(a.drop, i);
      d = (dm + ds * (kf * dlq_gelu(v) - pm)) * kf * dlq_dgelu(v);
    }
    dy[i] = d;
    s1 += d;
    s2 += d * zh;
  }
  rec[(size_t)blk * 2 * HID + 2 * tid] = s1;
  rec[(size_t)blk * 2 * HID + 2 * tid + 1] = s2;
}

hipError_t launch_dlq_dy3(const DlqHeadArgs& a, int B, int tpu, float* dy, float* rec, hipStream_t s) {
  hipLaunchKernelGGL(dlq_dy3_kernel, dim3(B * tpu), dim3(256), 0, s, a, tpu, dy, rec);
  return hipGetLastError();
}

// ---- BatchNorm backward, the dz pass: dz = gamma invstd (dy - mean(dy) - zhat mean(dy zhat)) on every frame ---------------------------
// workgroup = 64 frames, thread = (frame lane 0 .. 7, 8 channels); writes dz as split pixels and the workgroup's per-channel sums of dz
__global__ __launch_bounds__(256) void dlq_dz_kernel(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ sums,
                                                     uint4* __restrict__ dz, float* __restrict__ dbrec, long long N) {
  __shared__ float red[8][HID];
  const int g = threadIdx.x & 31, fl = threadIdx.x >> 5;
  const float inv_n = 1.0f / (float)N;
  float mu[8], is[8], gi[8], m1[8], m2[8], acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * g + j;
    mu[j] = mean[c]; is[j] = invstd[c]; gi[j] = gamma[c] * is[j];
    m1[j] = sums[2 * c] * inv_n; m2[j] = sums[2 * c + 1] * inv_n;
    acc[j] = 0.f;
  }
  for (int it = 0; it < 8; ++it) {
    const long long n = (long long)blockIdx.x * 64 + it * 8 + fl;
    if (n >= N) break;
    const float* dp = dy + (size_t)n * HID + 8 * g;
    const float* zp = z + (size_t)n * HID + 8 * g;
    const float4 d0 = *reinterpret_cast<const float4*>(dp), d1 = *reinterpret_cast<const float4*>(dp + 4);
    const float4 z0 = *reinterpret_cast<const float4*>(zp), z1 = *reinterpret_cast<const float4*>(zp + 4);
    const float dv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w}, zv[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = gi[j] * (dv[j] - m1[j] - (zv[j] - mu[j]) * is[j] * m2[j]);
      acc[j] += v[j];
    }
    dlq_store_pixel8(dz + (size_t)n * PIXC, g, v);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[fl][8 * g + j] = acc[j];
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 8; ++r) s += red[r][threadIdx.x];
  dbrec[(size_t)blockIdx.x * HID + threadIdx.x] = s;
}

int dlq_dz_blocks(long long N) { return (int)((N + 63) / 64); }
hipError_t launch_dlq_dz(const float* dy, const float* z, const BnApply& bn, const float* sums, void* dz, float* dbrec, long long N, hipStream_t s) {
  hipLaunchKernelGGL(dlq_dz_kernel, dim3(dlq_dz_blocks(N)), dim3(256), 0, s, dy, z, bn.mean, bn.invstd, bn.gamma, sums, (uint4*)dz, dbrec, N);
  return hipGetLastError();
}

// ---- weight gradient: dW[o][c][k] = sum over frames n = (b, t) of dz[n][o] src[b][t + k - pad][c] --------------------------------------
// A GEMM with K = N = B T_max frames, the slow axis of both operands: a workgroup owns (frame chunk, 64 output channels, tap) and
// stages 32 frames at a time into LDS TRANSPOSED -- [term][channel][frame] bf16, rows of 40 so that a lane's 8 consecutive frames are
// one aligned 16-byte read and channels spread over the banks -- with the tap's shift applied at staging: a frame whose shifted source
// falls outside its own utterance's [0, T_max) is the convolution's zero padding, never the neighbouring utterance.  Wave w owns source
// channels [64 w, 64 w + 64).  SRCX: the source is x[b][c][t] itself (fp32, time fastest: K-contiguous), taken as zero at t >= len_b by a
// select and split into its three terms here; else the previous layer's split pixels.  Each workgroup writes its partial
// [chunk][tap][o][c]; dlq_wgrad_reduce_kernel adds the chunks in order.
constexpr int WG_ROW = 40;                                     // bf16 per LDS row: 32 frames + 8 of padding (80 bytes, a multiple of 16)
constexpr int WG_LDS = 3 * (64 + HID) * WG_ROW * 2;            // 76800 bytes

template <int SRCX>
__global__ __launch_bounds__(256) void dlq_wgrad_kernel(const DlqWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  unsigned short* As = reinterpret_cast<unsigned short*>(lds);                 // [3][64][WG_ROW]
  unsigned short* Bs = As + 3 * 64 * WG_ROW;                                   // [3][256][WG_ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
  const int chunk = blockIdx.x, ob = blockIdx.y * 64, tap = blockIdx.z, shift = tap - a.taps / 2, T = a.T_max;
  const long long N = a.N, nbeg = (long long)chunk * a.CH, nend = min(N, nbeg + a.CH);
  const int Cr = SRCX ? (a.C + 31) / 32 * 32 : HID;                            // source channel rows staged
  const int ntile = min(2, max(0, (Cr - 64 * wave + 31) / 32));                // this wave's 32-channel tiles that exist
  f32x16_t acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  for (long long n0 = nbeg; n0 < nend; n0 += 32) {
    // dz: 32 frames x 3 terms x 8 chunks of 8 channels
    for (int i = tid; i < 32 * 24; i += 256) {
      const int fl = i / 24, r = i - fl * 24, t = r >> 3, q = r & 7;
      const long long n = n0 + fl;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (n < nend) v = a.dz[(size_t)n * PIXC + 32 * t + (ob >> 3) + q];
      const unsigned wv[4] = {v.x, v.y, v.z, v.w};
      unsigned short* dst = As + (t * 64 + 8 * q) * WG_ROW + fl;
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j * WG_ROW] = (unsigned short)(wv[j >> 1] >> (16 * (j & 1)));
    }
    if (SRCX) {
      for (int i = tid; i < Cr * 32; i += 256) {
        const int c = i >> 5, fl = i & 31;
        const long long n = n0 + fl;
        const int b = (int)(n / T), ts = (int)(n - (long long)b * T) + shift;
        float v = 0.f;
        if (n < nend && c < a.C && ts >= 0 && ts < a.lens[b]) v = a.x[(size_t)b * a.sb + (size_t)c * a.sc + ts];
        const bf16_t t0 = float_to_bf16(v);
        const float r1 = v - bf16_to_float(t0);
        const bf16_t t1 = float_to_bf16(r1);
        const bf16_t t2 = float_to_bf16(r1 - bf16_to_float(t1));
        Bs[(0 * HID + c) * WG_ROW + fl] = t0.v;
        Bs[(1 * HID + c) * WG_ROW + fl] = t1.v;
        Bs[(2 * HID + c) * WG_ROW + fl] = t2.v;
      }
    } else {
      for (int i = tid; i < 32 * 96; i += 256) {
        const int fl = i / 96, r = i - fl * 96, t = r >> 5, q = r & 31;
        const long long n = n0 + fl;
        const int ts = (int)(n % T) + shift;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (n < nend && ts >= 0 && ts < T) v = a.h[(size_t)(n + shift) * PIXC + r];
        const unsigned wv[4] = {v.x, v.y, v.z, v.w};
        unsigned short* dst = Bs + (t * HID + 8 * q) * WG_ROW + fl;
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j * WG_ROW] = (unsigned short)(wv[j >> 1] >> (16 * (j & 1)));
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 af[2][3], bf[2][3];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 3; ++t) af[m][t] = *reinterpret_cast<const uint4*>(As + (t * 64 + 32 * m + col) * WG_ROW + 16 * ks + 8 * h);
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if (n >= ntile) continue;
#pragma unroll
        for (int t = 0; t < 3; ++t) bf[n][t] = *reinterpret_cast<const uint4*>(Bs + (t * HID + 64 * wave + 32 * n + col) * WG_ROW + 16 * ks + 8 * h);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          acc[m][n] = mma32(af[m][1], bf[n][1], acc[m][n]);
          acc[m][n] = mma32(af[m][2], bf[n][0], acc[m][n]);
          acc[m][n] = mma32(af[m][0], bf[n][2], acc[m][n]);
          acc[m][n] = mma32(af[m][1], bf[n][0], acc[m][n]);
          acc[m][n] = mma32(af[m][0], bf[n][1], acc[m][n]);
          acc[m][n] = mma32(af[m][0], bf[n][0], acc[m][n]);
        }
      }
    }
    __syncthreads();
  }
  // lane = source channel, registers 4 g .. 4 g + 3 = output channels ob + 32 m + 8 g + 4 h + (0 .. 3)
  float* out = a.partial + ((size_t)chunk * a.taps + tap) * HID * a.C;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int c = 64 * wave + 32 * n + col;
    if (n >= ntile || c >= a.C) continue;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) out[(size_t)(ob + 32 * m + 8 * (r >> 2) + 4 * h + (r & 3)) * a.C + c] = acc[m][n][r];
  }
}

// dW[o][c][k] = sum over chunks, in order (float64 accumulate); thread = (k, o, c), c fastest
__global__ __launch_bounds__(256) void dlq_wgrad_reduce_kernel(const float* __restrict__ partial, int nch, int C, int taps, float* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x, per = taps * HID * C;
  if (i >= per) return;
  double s = 0.0;
  for (int q = 0; q < nch; ++q) s += (double)partial[(size_t)q * per + i];
  const int c = i % C, o = (i / C) % HID, k = i / (C * HID);
  dw[((size_t)o * C + c) * taps + k] = (float)s;
}

// frames per chunk (a multiple of 32) and the chunk count for N frames
void dlq_wgrad_chunks(long long N, int* CH, int* nch) {
  const long long want = std::min<long long>(48, (N + 255) / 256);
  const long long ch = 32 * ((N + 32 * want - 1) / (32 * want));
  *CH = (int)ch;
  *nch = (int)((N + ch - 1) / ch);
}

hipError_t launch_dlq_wgrad(const DlqWgradArgs& a0, float* dw, hipStream_t s) {
  DlqWgradArgs a = a0;
  int nch;
  dlq_wgrad_chunks(a.N, &a.CH, &nch);
  auto kern = a.x ? dlq_wgrad_kernel<1> : dlq_wgrad_kernel<0>;
  hipError_t e = launch_lds(kern, dim3(nch, HID / 64, a.taps), dim3(256), WG_LDS, s, a);
  if (e != hipSuccess) return e;
  const int per = a.taps * HID * a.C;
  hipLaunchKernelGGL(dlq_wgrad_reduce_kernel, dim3((per + 255) / 256), dim3(256), 0, s, a.partial, nch, a.C, a.taps, dw);
  return hipGetLastError();
}

// ---- gradient clipping: two-stage fixed-order L2 norm, then grad *= min(1, max_norm / (norm + 1e-6)) -----------------------------------
constexpr int kClipBlocks = 256;
__global__ __launch_bounds__(256) void dlq_sumsq_kernel(const float* __restrict__ g, size_t n, double* __restrict__ partial) {
  __shared__ double red[256];
  const size_t per = (n + kClipBlocks - 1) / kClipBlocks, lo = (size_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double acc = 0.0;
  for (size_t i = lo + threadIdx.x; i < hi; i += 256) acc += (double)g[i] * (double)g[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void dlq_clip_scale_kernel(float* __restrict__ g, size_t n, const double* __restrict__ partial, float max_norm,
                                                             float* __restrict__ norm_out) {
  __shared__ double red[256];
  red[threadIdx.x] = partial[threadIdx.x];
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float norm = (float)sqrt(red[0]);
  const float coef = fminf(1.f, max_norm / (norm + 1e-6f));
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) norm_out[0] = norm;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) g[i] *= coef;
}

hipError_t launch_clip_grad_norm(float* g, size_t n, float max_norm, float* norm_out, double* partial, hipStream_t s) {
  hipLaunchKernelGGL(dlq_sumsq_kernel, dim3(kClipBlocks), dim3(256), 0, s, g, n, partial);
  hipLaunchKernelGGL(dlq_clip_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, n, partial, max_norm, norm_out);
  return hipGetLastError();
}

}  // namespace dfa

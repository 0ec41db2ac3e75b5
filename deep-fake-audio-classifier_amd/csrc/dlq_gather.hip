// dlq_gather.hip -- one training or dev batch of the DeepfakeDetector assembled on the device from the packed resident set
// (include/dfa_hip.h: dfa_dlq_gather_batch).  One kernel of pure data movement and its entry point.
//
// The set: utterance i of [C][T_i], time fastest, as C rows of pitch_i = ceil(T_i / 4) * 4 floats from float offset off_i
// (a multiple of 4).  The batch: x[B][C][T_pad], T_pad = ceil(T_max / 4) * 4, the layout the step and the eval forward read in
// place.  Element (b, c, t) is the set's when t < len_b and neither t lies in a time span of b nor c in a channel span of b,
// else +0.0f: a SELECT, so NaN or Inf in a masked span, behind len_b or in a row's padding floats never reaches x.  All T_pad
// columns of every row are written (the batch buffer needs no memset), nothing else is.
#include <vector>

#include "dfa_checks.h"
#include "trace.h"

using namespace dfa;

namespace {

constexpr int kThreads = 256;
constexpr int kSlotsPerThread = 4;                       // 4-frame slots of one thread, kThreads apart: 4 x 16 bytes in flight
constexpr int kSlotsPerWg = kThreads * kSlotsPerThread;
constexpr int kMaxSpans = 16;
constexpr int kTimingSlot = 14;

// table words: [0, B) lengths | [B, 2B) dispatch order (unused here) | [2B, 4B) source offsets, low word then high word |
// [4B, 4B + B * nsp * 2) spans (start, width): n_t time spans, then n_f channel spans
inline size_t table_words(int B, int nsp) { return (size_t)4 * B + (size_t)2 * B * nsp; }

// A workgroup stays inside one utterance: b, its length, offset and spans are wave-uniform words read once.  The C * S slots
// of an utterance (S = T_pad / 4 per row) are numbered row-major, so consecutive lanes store consecutive 16-byte pieces of x.
__global__ __launch_bounds__(kThreads) void dlq_gather_kernel(const float* __restrict__ set, const int* __restrict__ tab, float* __restrict__ x,
                                                              int64_t stride_b, int64_t stride_c, int B, int C, int S, int wg_per_utt,
                                                              int n_t, int n_f) {
  const int b = blockIdx.x / wg_per_utt;
  const int first = (blockIdx.x - b * wg_per_utt) * kSlotsPerWg + threadIdx.x;
  const int len = tab[b];
  const int64_t off = (int64_t)(((uint64_t)(uint32_t)tab[2 * B + 2 * b]) | ((uint64_t)(uint32_t)tab[2 * B + 2 * b + 1] << 32));
  const int pitch = (len + 3) & ~3;
  const int* sp = tab + 4 * (size_t)B + (size_t)b * 2 * (n_t + n_f);
  const float* src = set + off;
  float* dst = x + (int64_t)b * stride_b;
  const int total = C * S;

  float4 v[kSlotsPerThread];
  int cc[kSlotsPerThread], tt[kSlotsPerThread];
#pragma unroll
  for (int k = 0; k < kSlotsPerThread; ++k) {
    const int i = first + k * kThreads;
    const int c = i / S;
    const int t0 = (i - c * S) * 4;
    cc[k] = c;
    tt[k] = t0;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    // a slot that straddles len ends inside the row's pitch; slots at or past the pitch belong to the next row or utterance
    if (i < total && t0 < pitch) v[k] = *reinterpret_cast<const float4*>(src + (int64_t)c * pitch + t0);
  }
  // (the slots outermost.  With the spans outermost and sixteen keep flags per thread the compiler holds the flags as lane masks
  // in scalar registers and spills them; measured no faster: DESIGN.md section 3.15b)
#pragma unroll
  for (int k = 0; k < kSlotsPerThread; ++k) {
    if (first + k * kThreads >= total) continue;
    const int c = cc[k], t0 = tt[k];
    bool row_off = false;
    for (int j = 0; j < n_f; ++j) {
      const int s0 = sp[2 * (n_t + j)], w = sp[2 * (n_t + j) + 1];
      row_off |= (c >= s0) & (c < s0 + w);
    }
    bool keep[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) keep[e] = !row_off & (t0 + e < len);
    for (int j = 0; j < n_t; ++j) {
      const int s0 = sp[2 * j], w = sp[2 * j + 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) keep[e] &= !((t0 + e >= s0) & (t0 + e < s0 + w));
    }
    float4 o;
    o.x = keep[0] ? v[k].x : 0.f;
    o.y = keep[1] ? v[k].y : 0.f;
    o.z = keep[2] ? v[k].z : 0.f;
    o.w = keep[3] ? v[k].w : 0.f;
    *reinterpret_cast<float4*>(dst + (int64_t)c * stride_c + t0) = o;
  }
}

}  // namespace

extern "C" {

size_t dfa_dlq_gather_workspace_bytes(int B, int n_tmask, int n_fmask) {
  if (B < 1 || n_tmask < 0 || n_fmask < 0 || n_tmask + n_fmask > kMaxSpans) return 0;
  return align_up(table_words(B, n_tmask + n_fmask) * sizeof(int32_t), 256);
}

int dfa_dlq_gather_batch(dfa_ctx* ctx, const float* set, int64_t set_floats, const int64_t* src_off, const int32_t* lengths,
                         const int32_t* spans, int n_tmask, int n_fmask, int B, int T_max, int C, float* x, int64_t stride_b,
                         int64_t stride_c, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_dlq_gather_batch");
  if (!ctx) return DFA_E_NULL_PTR;
  if (!set || !src_off || !lengths || !x || !workspace)
    return fail(ctx, DFA_E_NULL_PTR, "set, src_off, lengths, x and workspace must be non-null");
  if (n_tmask < 0 || n_fmask < 0) return fail(ctx, DFA_E_BAD_SHAPE, "n_tmask=%d and n_fmask=%d must be >= 0", n_tmask, n_fmask);
  const int nsp = n_tmask + n_fmask;
  if (nsp > kMaxSpans)
    return fail(ctx, DFA_E_UNSUPPORTED, "n_tmask + n_fmask = %d spans per utterance (limit %d)", nsp, kMaxSpans);
  if (nsp > 0 && !spans) return fail(ctx, DFA_E_NULL_PTR, "spans must be non-null when n_tmask + n_fmask > 0");
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "batch must be >= 1 (got %d)", B);
  if (C < 1) return fail(ctx, DFA_E_BAD_SHAPE, "C must be >= 1 (got %d)", C);
  if (T_max < 1) return fail(ctx, DFA_E_BAD_SHAPE, "T_max must be >= 1 (got %d)", T_max);
  DFA_TRY(check_lengths(ctx, lengths, B, 1, T_max));
  const int64_t T_pad = ((int64_t)T_max + 3) / 4 * 4;
  for (int b = 0; b < B; ++b) {
    const int64_t pitch = ((int64_t)lengths[b] + 3) / 4 * 4;
    if (src_off[b] < 0 || (src_off[b] & 3) != 0 || src_off[b] > set_floats || C * pitch > set_floats - src_off[b])
      return fail(ctx, DFA_E_BAD_SHAPE, "src_off[%d]=%lld: needs a non-negative multiple of 4 with %d rows of %lld floats inside set_floats=%lld",
                  b, (long long)src_off[b], C, (long long)pitch, (long long)set_floats);
    for (int j = 0; j < nsp; ++j) {
      const int64_t s0 = spans[((size_t)b * nsp + j) * 2], w = spans[((size_t)b * nsp + j) * 2 + 1];
      const bool time = j < n_tmask;
      const int64_t dim = time ? lengths[b] : C;
      if (s0 < 0 || w < 0 || s0 + w > dim)
        return fail(ctx, DFA_E_BAD_SHAPE, "%s span %d of utterance %d, (start=%lld, width=%lld), leaves [0, %lld]", time ? "time" : "channel",
                    time ? j : j - n_tmask, b, (long long)s0, (long long)w, (long long)dim);
    }
  }
  if (((uintptr_t)x & 15) != 0) return fail(ctx, DFA_E_BAD_SHAPE, "x must be 16-byte aligned (got %p)", (void*)x);
  if ((stride_c & 3) != 0 || stride_c < T_pad)
    return fail(ctx, DFA_E_BAD_SHAPE, "stride_c=%lld: needs a multiple of 4 >= T_pad=%lld", (long long)stride_c, (long long)T_pad);
  if ((stride_b & 3) != 0 || stride_b < 0 || (B > 1 && stride_b < (C - 1) * stride_c + T_pad))
    return fail(ctx, DFA_E_BAD_SHAPE, "stride_b=%lld: needs a multiple of 4 that keeps the utterances apart, >= (C - 1) * stride_c + T_pad = %lld",
                (long long)stride_b, (long long)((C - 1) * stride_c + T_pad));
  const int64_t S = T_pad / 4;
  const int64_t wg_per_utt = (C * S + kSlotsPerWg - 1) / kSlotsPerWg;
  if (C * S >= ((int64_t)1 << 30) || wg_per_utt * B >= ((int64_t)1 << 31))
    return fail(ctx, DFA_E_UNSUPPORTED, "the batch needs %lld workgroups of %lld slots per utterance (limits 2^31 - 1, 2^30)",
                (long long)(wg_per_utt * B), (long long)(C * S));
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, dfa_dlq_gather_workspace_bytes(B, n_tmask, n_fmask)));
  DFA_TRY(refuse_capture(ctx, "batch gather"));

  std::vector<int32_t> extra((size_t)2 * B + (size_t)2 * B * nsp);
  for (int b = 0; b < B; ++b) {
    extra[2 * b] = (int32_t)(uint32_t)((uint64_t)src_off[b] & 0xFFFFFFFFu);
    extra[2 * b + 1] = (int32_t)(uint32_t)((uint64_t)src_off[b] >> 32);
  }
  for (size_t i = 0; i < (size_t)2 * B * nsp; ++i) extra[(size_t)2 * B + i] = spans[i];
  DFA_TRY(stage_ragged_lengths_extra(ctx, lengths, B, extra.data(), extra.size(), workspace));
  {
    ScopedSlot ts(ctx, kTimingSlot);
    hipLaunchKernelGGL(dlq_gather_kernel, dim3((unsigned)(wg_per_utt * B)), dim3(kThreads), 0, ctx->stream, set, (const int*)workspace, x,
                       stride_b, stride_c, B, C, (int)S, (int)wg_per_utt, n_tmask, n_fmask);
    DFA_HIP_CHECK(ctx, hipGetLastError());
  }
  return DFA_OK;
}

}  // extern "C"

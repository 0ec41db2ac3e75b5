// utt_norm_api.hip -- C ABI of the per-utterance CMN / CVMN normalisation (include/dfa_hip.h: dfa_utt_norm, dfa_utt_norm_packed;
// kernels in utt_norm.hip): the argument checks, the per-call table and the one launch.
#include <limits.h>

#include <vector>

#include "dfa_checks.h"
#include "trace.h"

using namespace dfa;

namespace {

constexpr int kTimingSlot = 15;

// table words: [0, B) lengths | [B, 2B) dispatch order (unused here) | packed: [2B, 4B) float offsets, low word then high word
inline size_t table_bytes(int B) { return align_up((size_t)4 * B * sizeof(int32_t), 256); }

int check_mode(dfa_ctx* ctx, int mode) {
  if (mode != DFA_NORM_CMN && mode != DFA_NORM_CVMN)
    return fail(ctx, DFA_E_UNSUPPORTED, "unknown normalisation mode %d (DFA_NORM_CMN = %d, DFA_NORM_CVMN = %d)", mode, DFA_NORM_CMN, DFA_NORM_CVMN);
  return DFA_OK;
}

// the unbiased standard deviation needs two frames (the reference returns NaN for one)
int check_cvmn_lengths(dfa_ctx* ctx, int mode, const int32_t* lengths, int B) {
  if (mode != DFA_NORM_CVMN) return DFA_OK;
  for (int b = 0; b < B; ++b)
    if (lengths[b] < 2) return fail(ctx, DFA_E_BAD_SHAPE, "lengths[%d]=%d: cvmn needs at least 2 frames per utterance", b, (int)lengths[b]);
  return DFA_OK;
}

}  // namespace

extern "C" {

size_t dfa_utt_norm_workspace_bytes(int B) { return B < 1 ? 0 : table_bytes(B); }

int dfa_utt_norm(dfa_ctx* ctx, int mode, const float* x, float* y, int B, int T_max, int C, int64_t stride_b, int64_t stride_t,
                 int64_t stride_c, const int32_t* lengths, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_utt_norm");
  if (!ctx) return DFA_E_NULL_PTR;
  if (!x || !y || !workspace) return fail(ctx, DFA_E_NULL_PTR, "x, y and workspace must be non-null");
  DFA_TRY(check_mode(ctx, mode));
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "batch must be >= 1 (got %d)", B);
  if (C < 1) return fail(ctx, DFA_E_BAD_SHAPE, "C must be >= 1 (got %d)", C);
  if (T_max < 1) return fail(ctx, DFA_E_BAD_SHAPE, "T_max must be >= 1 (got %d)", T_max);
  if (lengths) {
    DFA_TRY(check_lengths(ctx, lengths, B, 1, T_max));
    DFA_TRY(check_cvmn_lengths(ctx, mode, lengths, B));
  } else if (mode == DFA_NORM_CVMN && T_max < 2) {
    return fail(ctx, DFA_E_BAD_SHAPE, "T_max=%d: cvmn needs at least 2 frames per utterance", T_max);
  }
  const bool time_fast = stride_t == 1;
  if (!time_fast && stride_c != 1)
    return fail(ctx, DFA_E_UNSUPPORTED, "the normalisation needs stride_t == 1 or stride_c == 1 (got stride_t=%lld, stride_c=%lld)",
                (long long)stride_t, (long long)stride_c);
  if (time_fast) {
    DFA_TRY(check_channel_major(ctx, "time-fastest normalisation", "stride_c", x, stride_b, stride_c, T_max));
    if (((uintptr_t)y & 15) != 0) return fail(ctx, DFA_E_UNSUPPORTED, "the time-fastest normalisation needs y 16-byte aligned (got %p)", (void*)y);
  } else {
    if (stride_t < C || stride_b < 0)
      return fail(ctx, DFA_E_UNSUPPORTED, "the feature-fastest normalisation needs stride_t >= C=%d and stride_b >= 0 (got stride_t=%lld, stride_b=%lld)",
                  C, (long long)stride_t, (long long)stride_b);
    if ((((uintptr_t)x | (uintptr_t)y) & 3) != 0) return fail(ctx, DFA_E_UNSUPPORTED, "x and y must be 4-byte aligned (got %p, %p)", (const void*)x, (void*)y);
  }
  const int64_t wgs = time_fast ? ((int64_t)B * C + 3) / 4 : (int64_t)B * ((C + 63) / 64);
  if (wgs >= ((int64_t)1 << 31)) return fail(ctx, DFA_E_UNSUPPORTED, "the batch needs %lld workgroups (limit 2^31 - 1)", (long long)wgs);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, table_bytes(B)));
  const int* tab = nullptr;
  if (lengths) {
    DFA_TRY(refuse_capture(ctx, "normalisation"));
    DFA_TRY(stage_ragged_lengths(ctx, lengths, B, workspace));
    tab = (const int*)workspace;
  }
  ScopedSlot ts(ctx, kTimingSlot);
  if (time_fast) DFA_HIP_CHECK(ctx, launch_utt_norm_time(x, y, tab, mode, B, C, T_max, stride_b, stride_c, false, ctx->stream));
  else DFA_HIP_CHECK(ctx, launch_utt_norm_feat(x, y, tab, mode, B, C, T_max, stride_b, stride_t, ctx->stream));
  return DFA_OK;
}

int dfa_utt_norm_packed(dfa_ctx* ctx, int mode, float* set, int64_t set_floats, const int64_t* offsets, const int32_t* lengths, int N,
                        int C, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_utt_norm_packed");
  if (!ctx) return DFA_E_NULL_PTR;
  if (!set || !offsets || !lengths || !workspace) return fail(ctx, DFA_E_NULL_PTR, "set, offsets, lengths and workspace must be non-null");
  DFA_TRY(check_mode(ctx, mode));
  if (N < 1) return fail(ctx, DFA_E_BAD_SHAPE, "N must be >= 1 (got %d)", N);
  if (C < 1) return fail(ctx, DFA_E_BAD_SHAPE, "C must be >= 1 (got %d)", C);
  if (N > DFA_UTT_NORM_MAX_PACKED)
    return fail(ctx, DFA_E_UNSUPPORTED, "N=%d utterances in one call (limit %d: walk the set in chunks)", N, DFA_UTT_NORM_MAX_PACKED);
  DFA_TRY(check_lengths(ctx, lengths, N, 1, INT_MAX - 3));
  DFA_TRY(check_cvmn_lengths(ctx, mode, lengths, N));
  for (int i = 0; i < N; ++i) {
    const int64_t pitch = ((int64_t)lengths[i] + 3) / 4 * 4;
    if (offsets[i] < 0 || (offsets[i] & 3) != 0 || offsets[i] > set_floats || C * pitch > set_floats - offsets[i])
      return fail(ctx, DFA_E_BAD_SHAPE, "offsets[%d]=%lld: needs a non-negative multiple of 4 with %d rows of %lld floats inside set_floats=%lld", i,
                  (long long)offsets[i], C, (long long)pitch, (long long)set_floats);
  }
  if (((int64_t)N * C + 3) / 4 >= ((int64_t)1 << 31))
    return fail(ctx, DFA_E_UNSUPPORTED, "the set needs %lld workgroups (limit 2^31 - 1)", (long long)(((int64_t)N * C + 3) / 4));
  if (((uintptr_t)set & 15) != 0) return fail(ctx, DFA_E_UNSUPPORTED, "the packed set must be 16-byte aligned (got %p)", (void*)set);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, table_bytes(N)));
  DFA_TRY(refuse_capture(ctx, "normalisation"));
  std::vector<int32_t> extra((size_t)2 * N);
  for (int i = 0; i < N; ++i) {
    extra[2 * i] = (int32_t)(uint32_t)((uint64_t)offsets[i] & 0xFFFFFFFFu);
    extra[2 * i + 1] = (int32_t)(uint32_t)((uint64_t)offsets[i] >> 32);
  }
  DFA_TRY(stage_ragged_lengths_extra(ctx, lengths, N, extra.data(), extra.size(), workspace));
  ScopedSlot ts(ctx, kTimingSlot);
  DFA_HIP_CHECK(ctx, launch_utt_norm_time(set, set, (const int*)workspace, mode, N, C, 0, 0, 0, true, ctx->stream));
  return DFA_OK;
}

}  // extern "C"

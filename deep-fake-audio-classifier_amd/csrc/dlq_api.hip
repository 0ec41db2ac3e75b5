// dlq_api.hip -- C ABI of the DeepfakeDetector eval forward (include/dfa_hip.h, kernels in dlq.hip): parameter binding, weight
// preparation, the workspace plan and the four launches of a variable-length batch.
#include <algorithm>
#include <vector>

#include "dfa_checks.h"
#include "trace.h"

using namespace dfa;

namespace {

constexpr int NF = DFA_DLQ_TILE_FRAMES;

// workspace: [table: 4 B + 1 words] [h1: B T_max pixels of 1.5 KB] [h2: the same] [per-tile pool records: B ceil(T_max / NF) x 512 floats]
struct DlqPlan {
  size_t tab_words, h1_off, h2_off, part_off, total;
};
DlqPlan plan_dlq(int B, int T_max) {
  DlqPlan p;
  p.tab_words = (size_t)4 * B + 1;
  size_t off = align_up(p.tab_words * 4, 256);
  p.h1_off = off;
  off = align_up(off + (size_t)B * T_max * 1536, 256);
  p.h2_off = off;
  off = align_up(off + (size_t)B * T_max * 1536, 256);
  p.part_off = off;
  off = align_up(off + (size_t)B * ((T_max + NF - 1) / NF) * 512 * sizeof(float), 256);
  p.total = off;
  return p;
}

}  // namespace

extern "C" {

int dfa_dlq_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int in_ch, int hidden) {
  DFA_TRY(set_params_core(ctx, &dfa_ctx::dlq, "DeepfakeDetector", device_params, n, [&]() -> int {
    if (hidden != 256) return fail(ctx, DFA_E_UNSUPPORTED, "the DeepfakeDetector HIP path is built for hidden=256 (got %d)", hidden);
    if (in_ch < 4 || in_ch > 256 || (in_ch & 3) != 0)
      return fail(ctx, DFA_E_UNSUPPORTED, "the DeepfakeDetector HIP path needs in_ch %% 4 == 0 and 4 <= in_ch <= 256 (got in_ch=%d)", in_ch);
    return DFA_OK;
  }));
  ctx->dlq.in_ch = in_ch;
  ctx->dlq.prepared = false;
  return DFA_OK;
}

int dfa_dlq_prepare(dfa_ctx* ctx) {
  if (!ctx) return DFA_E_NULL_PTR;
  DlqState& m = ctx->dlq;
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_dlq_set_params has not been called");
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int cin[3] = {m.in_ch, 256, 256}, taps[3] = {5, 3, 3};
  size_t woff[3], boff[3], total = 0;
  for (int l = 0; l < 3; ++l) { woff[l] = total; total = align_up(total + dlq_pack_bytes(cin[l], taps[l]), 256); }
  for (int l = 0; l < 3; ++l) { boff[l] = total; total = align_up(total + 256 * sizeof(float), 256); }
  if (m.packed) { DFA_HIP_CHECK(ctx, hipFree(m.packed)); m.packed = nullptr; }
  DFA_HIP_CHECK(ctx, hipMalloc(&m.packed, total));
  for (int l = 0; l < 3; ++l) {
    m.w[l] = (char*)m.packed + woff[l];
    m.b[l] = (float*)((char*)m.packed + boff[l]);
    DFA_HIP_CHECK(ctx, launch_dlq_pack(layer_params(m.p, l), cin[l], taps[l], m.w[l], m.b[l], ctx->stream));
  }
  m.prepared = true;
  return DFA_OK;
}

size_t dfa_dlq_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int in_ch) {
  (void)ctx; (void)in_ch;
  if (B < 1 || T_max < 1) return 0;
  return plan_dlq(B, T_max).total;
}

int dfa_dlq_forward(dfa_ctx* ctx, const void* x, int B, int T_max, int in_ch, int64_t stride_b, int64_t stride_c, const int32_t* lengths,
                    float* logits, float* pooled, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_dlq_forward");
  if (!ctx) return DFA_E_NULL_PTR;
  DlqState& m = ctx->dlq;
  if (!m.prepared) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_dlq_prepare has not been called since the last set_params");
  if (!x || !logits || !workspace || !lengths) return fail(ctx, DFA_E_NULL_PTR, "x, lengths, logits and workspace must be non-null");
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "batch must be >= 1 (got %d)", B);
  if (T_max < 1) return fail(ctx, DFA_E_BAD_SHAPE, "T_max must be >= 1 (got %d)", T_max);
  if (in_ch != m.in_ch)
    return fail(ctx, DFA_E_BAD_SHAPE, "channel dim %d does not match in_ch=%d of the first Conv1d (src/dlqueen_model.py:136)", in_ch, m.in_ch);
  DFA_TRY(check_lengths(ctx, lengths, B, 1, T_max));
  DFA_TRY(check_channel_major(ctx, "DeepfakeDetector forward", "stride_c", x, stride_b, stride_c, T_max));
  DFA_TRY(refuse_capture(ctx, "forward"));
  const DlqPlan pl = plan_dlq(B, T_max);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total));

  // the tile list: utterances longest first (ties in batch order); position i owns tiles [first[i], first[i + 1]) of NF frames
  // over the frames layer 1 produces, min(T_max, len + 2)
  std::vector<int32_t> extra((size_t)2 * B + 1);
  int32_t* order = extra.data();
  int32_t* first = extra.data() + B;
  for (int b = 0; b < B; ++b) order[b] = b;
  std::stable_sort(order, order + B, [&](int i, int j) { return lengths[i] > lengths[j]; });
  long long ntiles = 0;
  for (int i = 0; i < B; ++i) {
    first[i] = (int32_t)ntiles;
    ntiles += (std::min(T_max, lengths[order[i]] + 2) + NF - 1) / NF;
  }
  first[B] = (int32_t)ntiles;
  if (ntiles >= ((long long)1 << 31)) return fail(ctx, DFA_E_UNSUPPORTED, "the batch needs %lld tiles (limit 2^31 - 1)", ntiles);
  DFA_TRY(stage_ragged_lengths_extra(ctx, lengths, B, extra.data(), extra.size(), workspace));
  char* ws = (char*)workspace;
  DlqLayerArgs a{};
  a.x = (const float*)x;
  a.sb = stride_b;
  a.sc = stride_c;
  a.tab = (const int*)workspace;
  a.part = (float*)(ws + pl.part_off);
  a.B = B;
  a.T_max = T_max;
  hipStream_t s = ctx->stream;
  {
    ScopedSlot ts(ctx, 4);
    a.hin = nullptr; a.hout = (uint4*)(ws + pl.h1_off); a.w = (const uint4*)m.w[0]; a.bias = m.b[0]; a.C = in_ch; a.nks = dlq_nks(in_ch);
    DFA_HIP_CHECK(ctx, launch_dlq_layer(1, a, (int)ntiles, s));
  }
  {
    ScopedSlot ts(ctx, 5);
    a.hin = (const uint4*)(ws + pl.h1_off); a.hout = (uint4*)(ws + pl.h2_off); a.w = (const uint4*)m.w[1]; a.bias = m.b[1]; a.C = 256; a.nks = 16;
    DFA_HIP_CHECK(ctx, launch_dlq_layer(2, a, (int)ntiles, s));
  }
  {
    ScopedSlot ts(ctx, 6);
    a.hin = (const uint4*)(ws + pl.h2_off); a.hout = nullptr; a.w = (const uint4*)m.w[2]; a.bias = m.b[2];
    DFA_HIP_CHECK(ctx, launch_dlq_layer(3, a, (int)ntiles, s));
  }
  {
    ScopedSlot ts(ctx, 7);
    const HeadParams h0 = head_params(m.p, kDlqLayers, 0), h3 = head_params(m.p, kDlqLayers, 1);
    DFA_HIP_CHECK(ctx, launch_dlq_finish(a.part, a.tab, h0.w, h0.b, h3.w, h3.b, logits, pooled, B, s));
  }
  return DFA_OK;
}

}  // extern "C"

// cnn1d_api.hip -- C ABI of the CNN1D eval forward, uniform and ragged (include/dfa_hip.h; the reference's src/model_cnn1d.py):
// parameter binding, weight preparation, the workspace plan and the dispatch between the one-kernel forms (cnn1d_fused_x3.hip,
// cnn1d_fused.hip) and the three-launch path (conv1d.hip + linear.hip).
#include "dfa_checks.h"
#include "trace.h"

using namespace dfa;

namespace {

struct Cnn1dPlan { size_t h1_off, h2_off, pooled_off, total; };

Cnn1dPlan plan_cnn1d(int B, int T) {
  Cnn1dPlan p;
  size_t off = 0;
  p.h1_off = off;
  off = align_up(off + (size_t)B * 32 * T * sizeof(float), 256);
  p.h2_off = off;
  off = align_up(off + (size_t)B * 64 * T * sizeof(float), 256);
  p.pooled_off = off;
  off = align_up(off + (size_t)B * 128 * sizeof(float), 256);
  p.total = off;
  return p;
}

// the checks dfa_cnn1d_forward and dfa_cnn1d_forward_ragged make first, in this order (have_ptrs: no required pointer is null)
int cnn1d_forward_front(dfa_ctx* ctx, bool ragged, bool have_ptrs, int x_dtype, int B, int T, int F) {
  const Cnn1dState& m = ctx->cnn1d;
  if (!m.prepared) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cnn1d_prepare has not been called since the last set_params");
  if (!have_ptrs) return fail(ctx, DFA_E_NULL_PTR, "x, %slogits and workspace must be non-null", ragged ? "lengths, " : "");
  if (x_dtype != DFA_DTYPE_F32) return fail(ctx, DFA_E_BAD_DTYPE, "cnn1d takes float32 input (got dtype %d)", x_dtype);
  if (ragged) {
    if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "batch must be >= 1 (got %d)", B);
  } else if (B < 1 || T < 1) {
    return fail(ctx, DFA_E_BAD_SHAPE, "B and T must be >= 1 (got %d, %d)", B, T);
  }
  if (F != m.in_features)
    return fail(ctx, DFA_E_BAD_SHAPE, "feature dim %d does not match in_features=%d of the first Conv1d (src/model_cnn1d.py:17)", F, m.in_features);
  return DFA_OK;
}

}  // namespace

// Uniform: the h1 / h2 / pooled regions of the three-launch path.  Ragged: the per-call table alone (2 * B words: lengths and
// dispatch order) -- the one ragged kernel keeps every activation in LDS.
size_t dfa::cnn1d_workspace_bytes(int B, int T, bool ragged) { return ragged ? align_up((size_t)2 * B * 4, 256) : plan_cnn1d(B, T).total; }

extern "C" {

int dfa_cnn1d_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int in_features, int base_channels) {
  DFA_TRY(set_params_core(ctx, &dfa_ctx::cnn1d, "cnn1d", device_params, n, [&]() -> int {
    if (base_channels != 32) return fail(ctx, DFA_E_UNSUPPORTED, "cnn1d HIP path is built for base_channels=32 (got %d)", base_channels);
    if (in_features < 1) return fail(ctx, DFA_E_BAD_SHAPE, "in_features must be positive (got %d)", in_features);
    return DFA_OK;
  }));
  ctx->cnn1d.in_features = in_features;
  ctx->cnn1d.prepared = false;
  return DFA_OK;
}

// The kernel sizes of the three Conv1d layers the NEXT dfa_cnn1d_set_params / dfa_cnn1d_prepare bind: (3, 3, 3), or (5, 3, 3) --
// the reference's CNN1D_Variant (src/compare_kernels.py:38-67), whose conv.0.weight is [32][F][5].  Sticky on the context.
int dfa_cnn1d_set_kernels(dfa_ctx* ctx, int k1, int k2, int k3) {
  if (!ctx) return DFA_E_NULL_PTR;
  if (!((k1 == 3 || k1 == 5) && k2 == 3 && k3 == 3))
    return fail(ctx, DFA_E_UNSUPPORTED, "cnn1d kernels (%d, %d, %d): the HIP path is built for (3, 3, 3) and (5, 3, 3)", k1, k2, k3);
  Cnn1dState& m = ctx->cnn1d;
  if (k1 != m.k1) m.have_params = false;   // the bound conv.0.weight has the other shape: set_params again (never read past it)
  m.k1 = k1;
  m.prepared = false;                  // as dfa_cnn1d_set_params: the folded / packed weights go
  m.train.step.live = false;           // and a batch in flight is over
  return DFA_OK;
}

int dfa_cnn1d_prepare(dfa_ctx* ctx) {
  if (!ctx) return DFA_E_NULL_PTR;
  Cnn1dState& m = ctx->cnn1d;
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cnn1d_set_params has not been called");
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int cin[3] = {m.in_features, 32, 64}, cout[3] = {32, 64, 128}, taps[3] = {m.k1, 3, 3};
  size_t off[3], boff[3], total = 0;
  for (int l = 0; l < 3; ++l) { off[l] = total; total = align_up(total + (size_t)cout[l] * cin[l] * taps[l] * 4, 256); }
  for (int l = 0; l < 3; ++l) { boff[l] = total; total = align_up(total + (size_t)cout[l] * 4, 256); }
  size_t poff[3], xoff[3];
  for (int l = 0; l < 3; ++l) { poff[l] = total; total = align_up(total + cnn1d_fused_pack_floats(cin[l], cout[l], l) * 4, 256); }
  for (int l = 0; l < 3; ++l) { xoff[l] = total; total = align_up(total + cnn1d_x3_pack_bytes(cin[l], cout[l], taps[l]), 256); }
  if (m.packed) { DFA_HIP_CHECK(ctx, hipFree(m.packed)); m.packed = nullptr; }
  DFA_HIP_CHECK(ctx, hipMalloc(&m.packed, total));
  for (int l = 0; l < 3; ++l) {
    m.w[l] = (float*)((char*)m.packed + off[l]);
    m.b[l] = (float*)((char*)m.packed + boff[l]);
    DFA_HIP_CHECK(ctx, launch_fold_conv1d(layer_params(m.p, l), m.w[l], m.b[l], cin[l], cout[l], ctx->stream, taps[l]));
    m.wp[l] = (float*)((char*)m.packed + poff[l]);
    if (taps[l] == 3)     // (the exact-fp32 one-kernel form is three-tap only: a five-tap model never runs it, its image stays unwritten)
      DFA_HIP_CHECK(ctx, launch_pack_cnn1d_fused(m.w[l], m.wp[l], cin[l], cout[l], l, ctx->stream));
    m.wx[l] = (char*)m.packed + xoff[l];
    DFA_HIP_CHECK(ctx, launch_pack_cnn1d_x3(m.w[l], m.wx[l], cin[l], cout[l], ctx->stream, taps[l]));
  }
  m.prepared = true;
  return DFA_OK;
}

int dfa_cnn1d_forward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                      int64_t stride_f, float* logits, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn1d_forward");
  if (!ctx) return DFA_E_NULL_PTR;
  Cnn1dState& m = ctx->cnn1d;
  DFA_TRY(cnn1d_forward_front(ctx, false, x && logits && workspace, x_dtype, B, T, F));
  const Cnn1dPlan pl = plan_cnn1d(B, T);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total, false));   // (this entry point never asked for the alignment)
  char* ws = (char*)workspace;
  float *h1 = (float*)(ws + pl.h1_off), *h2 = (float*)(ws + pl.h2_off), *pooled = (float*)(ws + pl.pooled_off);
  hipStream_t s = ctx->stream;
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T, F};
  const HeadParams head = head_params(m.p, kCnn1dLayers, 0);
  // (the fused kernel addresses an utterance's elements with 32-bit offsets)
  const bool off32 = stride_t >= 0 && stride_f >= 0 && (int64_t)(F - 1) * stride_f + (int64_t)(T - 1) * stride_t < ((int64_t)1 << 31);
  if (ctx->cnn1d_fused == 1 && cnn1d_fused_x3_supports(v, m.k1)) {   // split-bf16 matrix cores (slot 4)
    ScopedSlot ts(ctx, 4);
    DFA_HIP_CHECK(ctx, launch_cnn1d_fused_x3((const float*)x, m.wx[0], m.b[0], m.wx[1], m.b[1], m.wx[2], m.b[2], head.w, head.b, logits, B, T, F,
                                             s, ctx->clock_probe ? ctx->clock_buf : nullptr, m.k1));
    return DFA_OK;
  }
  // (five taps: the exact-fp32 one-kernel form does not take them -- what the split-bf16 kernel refuses runs the three launches)
  if (m.k1 == 3 && ctx->cnn1d_fused && cnn1d_fused_supports(T) && off32) {   // one kernel, one global write per utterance (timing slot 4)
    ScopedSlot ts(ctx, 4);
    DFA_HIP_CHECK(ctx, launch_cnn1d_fused(v, m.wp[0], m.b[0], m.wp[1], m.b[1], m.wp[2], m.b[2], head.w, head.b, logits, s,
                                          ctx->clock_probe ? ctx->clock_buf : nullptr));
    return DFA_OK;
  }
  { ScopedSlot ts(ctx, 4);
    DFA_HIP_CHECK(ctx, launch_conv1d((const float*)x, stride_b, stride_f, stride_t, m.w[0], m.b[0], h1, B, F, 32, T, false, s, true, nullptr,
                                     nullptr, m.k1)); }
  { ScopedSlot ts(ctx, 5);
    DFA_HIP_CHECK(ctx, launch_conv1d(h1, (int64_t)32 * T, T, 1, m.w[1], m.b[1], h2, B, 32, 64, T, false, s)); }
  { ScopedSlot ts(ctx, 6);
    DFA_HIP_CHECK(ctx, launch_conv1d(h2, (int64_t)64 * T, T, 1, m.w[2], m.b[2], pooled, B, 64, 128, T, true, s)); }
  { ScopedSlot ts(ctx, 7);
    DFA_HIP_CHECK(ctx, launch_linear(pooled, head.w, head.b, logits, B, 128, s)); }
  return DFA_OK;
}

// Ragged CNN1D batch: ONE launch of cnn1d_ragged_x3_kernel (cnn1d_fused_x3.hip), workgroup i = utterance order[i] of the
// table.  No activation ever leaves LDS, so the workspace is the table alone; an utterance longer than one LDS window is
// walked in time segments inside its workgroup, so lengths[b] has no upper bound but T_max.
int dfa_cnn1d_forward_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b, int64_t stride_t,
                             int64_t stride_f, const int32_t* lengths, float* logits, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn1d_forward_ragged");
  if (!ctx) return DFA_E_NULL_PTR;
  Cnn1dState& m = ctx->cnn1d;
  DFA_TRY(cnn1d_forward_front(ctx, true, x && logits && workspace && lengths, x_dtype, B, T_max, F));
  if (T_max < 3) return fail(ctx, DFA_E_BAD_SHAPE, "T_max=%d is too short: the ragged cnn1d kernel needs T >= 3", T_max);
  DFA_TRY(check_lengths(ctx, lengths, B, 3, T_max));
  // layout: the stored channel-major batch [B][F][T_pad] seen as [B, T_max, F] -- frames contiguous, 16-byte aligned rows
  if (stride_t != 1)
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d forward takes the channel-major storage only: stride_t=%lld, needs 1", (long long)stride_t);
  if ((F & 3) != 0) return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d forward needs F %% 4 == 0 (got F=%d)", F);
  DFA_TRY(check_channel_major(ctx, "ragged cnn1d forward", "stride_f", x, stride_b, stride_f, T_max));
  if ((int64_t)F * stride_f >= ((int64_t)1 << 31))   // (the kernel addresses an utterance's elements with 32-bit offsets)
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d forward needs F * stride_f < 2^31 (got %d * %lld)", F, (long long)stride_f);
  if (ctx->cnn1d_fused != 1)   // the uniform forward would run other kernels: no bit-identity promise there
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d forward needs the default option cnn1d_fused=1 (got %d)", ctx->cnn1d_fused);
  if (cnn1d_ragged_segments(3, F, nullptr, nullptr, nullptr, nullptr, 0, m.k1) < 1)
    return fail(ctx, DFA_E_UNSUPPORTED, "F=%d: the layer-1 weights leave no LDS for a time window", F);
  DFA_TRY(refuse_capture(ctx, "forward"));
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, cnn1d_workspace_bytes(B, T_max, true)));
  DFA_TRY(stage_ragged_lengths(ctx, lengths, B, workspace));
  ScopedSlot ts(ctx, 4);
  const HeadParams head = head_params(m.p, kCnn1dLayers, 0);
  DFA_HIP_CHECK(ctx, launch_cnn1d_ragged_x3((const float*)x, stride_b, stride_f, (const int*)workspace, m.wx[0], m.b[0], m.wx[1], m.b[1], m.wx[2],
                                            m.b[2], head.w, head.b, logits, B, T_max, F, ctx->stream,
                                            ctx->clock_probe ? ctx->clock_buf : nullptr, m.k1));
  return DFA_OK;
}

// the time segments the ragged cnn1d kernel walks for an utterance of T frames (a function of T and F only): window
// [starts[i], starts[i] + lens[i]) and the layer-3 frames [owned_lo[i], owned_hi[i]) it adds to the mean; fills up to cap
// entries of each non-null array and returns the number of segments (0: T < 3, or F leaves no LDS for a window)
int dfa_cnn1d_ragged_segments(int T, int F, int* starts, int* lens, int* owned_lo, int* owned_hi, int cap) {
  return cnn1d_ragged_segments(T, F, starts, lens, owned_lo, owned_hi, cap);
}
// dynamic LDS of the ragged cnn1d launch for a batch padded to T_max (the layout of the largest window)
size_t dfa_cnn1d_ragged_lds_bytes(int T_max, int F) {
  if (T_max < 3 || cnn1d_ragged_segments(3, F, nullptr, nullptr, nullptr, nullptr, 0) < 1) return 0;
  return cnn1d_ragged_lds_bytes(T_max, F);
}
// The same two for a model whose layer 1 has k1 taps (3: exactly the pair above; 5: the k = (5, 3, 3) variant, whose windows run
// 4 frames to either side of their owned frames, or to the utterance's end); 0 for any other k1.
int dfa_cnn1d_ragged_segments_k(int T, int F, int k1, int* starts, int* lens, int* owned_lo, int* owned_hi, int cap) {
  if (k1 != 3 && k1 != 5) return 0;
  return cnn1d_ragged_segments(T, F, starts, lens, owned_lo, owned_hi, cap, k1);
}
size_t dfa_cnn1d_ragged_lds_bytes_k(int T_max, int F, int k1) {
  if ((k1 != 3 && k1 != 5) || T_max < 3 || cnn1d_ragged_segments(3, F, nullptr, nullptr, nullptr, nullptr, 0, k1) < 1) return 0;
  return cnn1d_ragged_lds_bytes(T_max, F, k1);
}
// the longest utterance the one-launch uniform forward takes at F features with k1 taps in layer 1 (the contiguous [B][F][T] storage;
// anything longer runs the three-launch path); 0 for an unsupported k1
int dfa_cnn1d_fused_max_t(int F, int k1) {
  if ((k1 != 3 && k1 != 5) || F < 1 || (F & 3)) return 0;
  return cnn1d_fused_x3_max_t(F, k1);
}

}  // extern "C"

// dfa_checks.h -- the argument checks the C ABI's entry points share (api.hip, cnn2d_api.hip, cnn1d_api.hip, cae_api.hip, dlq_api.hip,
// emb_api.hip, utt_norm_api.hip, train_api.hip, cnn1d_train_api.hip, cae_train_api.hip, dlq_train_api.hip).
// Host code only.  Every helper returns DFA_OK or the code it left, with its text, in the context (dfa::fail); an entry point
// wraps it in DFA_TRY.  The wording belongs to the entry points: where it differs between them it comes in as an argument.
#pragma once
#include "dfa_internal.h"

#define DFA_TRY(expr)                        \
  do {                                       \
    const int rc__ = (expr);                 \
    if (rc__ != DFA_OK) return rc__;         \
  } while (0)

namespace dfa {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// per-utterance frame counts of a ragged batch (host): each in [lo, T_max]
inline int check_lengths(dfa_ctx* ctx, const int32_t* lengths, int B, int lo, int T_max) {
  for (int b = 0; b < B; ++b)
    if (lengths[b] < lo || lengths[b] > T_max)
      return fail(ctx, DFA_E_BAD_SHAPE, "lengths[%d]=%d is outside [%d, T_max=%d]", b, (int)lengths[b], lo, T_max);
  return DFA_OK;
}

// a ragged call copies its lengths per call: a captured copy would replay this call's lengths forever.  what: "forward", "score", ...
inline int refuse_capture(dfa_ctx* ctx, const char* what) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  DFA_HIP_CHECK(ctx, hipStreamIsCapturing(ctx->stream, &cap));
  if (cap != hipStreamCaptureStatusNone)
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged %s cannot be captured into a graph: its lengths are copied per call", what);
  return DFA_OK;
}

// the caller's workspace against the plan's byte count; aligned: also the 256-byte alignment the plans' offsets assume (the
// entry points that never asked for it pass false).  what: "" or "train ", the entry point's wording
inline int check_workspace(dfa_ctx* ctx, const void* workspace, size_t have, size_t need, bool aligned = true, const char* what = "") {
  if (have < need) return fail(ctx, DFA_E_WORKSPACE, "%sworkspace too small: %zu < %zu bytes", what, have, need);
  if (aligned && ((uintptr_t)workspace & 255) != 0) return fail(ctx, DFA_E_WORKSPACE, "workspace must be 256-byte aligned");
  return DFA_OK;
}

// x as the stored channel-major batch [B][C][T_pad]: rows (stride_c, named `cname` in the text) and utterances a multiple of 4
// floats apart, rows at least T_max long, a 16-byte aligned base.  who: "ragged cnn1d forward", "DeepfakeDetector forward"
inline int check_channel_major(dfa_ctx* ctx, const char* who, const char* cname, const void* x, int64_t stride_b, int64_t stride_c, int T_max) {
  if ((stride_c & 3) != 0 || stride_c < T_max)
    return fail(ctx, DFA_E_UNSUPPORTED, "the %s needs %s %% 4 == 0 and %s >= T_max=%d (got %s=%lld)", who, cname, cname, T_max, cname,
                (long long)stride_c);
  if ((stride_b & 3) != 0 || stride_b < 0)
    return fail(ctx, DFA_E_UNSUPPORTED, "the %s needs a non-negative stride_b %% 4 == 0 (got stride_b=%lld)", who, (long long)stride_b);
  if (((uintptr_t)x & 15) != 0) return fail(ctx, DFA_E_UNSUPPORTED, "the %s needs x 16-byte aligned (got %p)", who, x);
  return DFA_OK;
}

// dfa_<model>_backward: the model's step record matches the call (train_step.h: match_step), no null pointer, [float32 x], the
// gradient count, no null gradient, the workspace's size (`need`, a callable that forms the plan: only once the shape is known to
// be the forward's), the model's own later checks (`late`, a callable returning a code), the SyncBN hook as the forward found it
struct BackwardNames {
  const char* bwd;        // "dfa_cnn2d_backward"
  const char* fwd;        // "dfa_cnn2d_forward_train"
  const char* model;      // "cnn2d", "the auto-encoder": the subject of the count's and the dtype's sentence
  int nparams;
  const char* upstream;   // "dlogits"; nullptr where the upstream gradient may be null
  bool f32_only;          // x must be float32 (x_dtype is not looked at otherwise)
};
template <typename Need, typename Late>
int check_backward(dfa_ctx* ctx, const BackwardNames& w, const TrainStep& step, int B, int T, int F, int ragged, const void* x, int x_dtype,
                   const void* upstream, float* const* grads, int ngrads, const void* workspace, size_t have, Need need, Late late) {
  const StepVerdict verdict = match_step(step, {B, T, F, x_dtype, ragged, ctx->bn_sync.fn != nullptr}, w.f32_only);
  if (verdict == STEP_OTHER_BATCH) return fail(ctx, DFA_E_NOT_PREPARED, "%s must follow %s on the same batch", w.bwd, w.fwd);
  if (w.upstream) {
    if (!x || !upstream || !grads || !workspace) return fail(ctx, DFA_E_NULL_PTR, "x, %s, grads and workspace must be non-null", w.upstream);
  } else if (!x || !grads || !workspace) {
    return fail(ctx, DFA_E_NULL_PTR, "x, grads and workspace must be non-null");
  }
  if (w.f32_only && x_dtype != DFA_DTYPE_F32) return fail(ctx, DFA_E_BAD_DTYPE, "%s takes float32 input", w.model);
  if (ngrads != w.nparams) return fail(ctx, DFA_E_BAD_SHAPE, "%s has %d parameters, got %d gradient pointers", w.model, w.nparams, ngrads);
  for (int i = 0; i < w.nparams; ++i)
    if (!grads[i]) return fail(ctx, DFA_E_NULL_PTR, "gradient pointer %d is null", i);
  if (have < need()) return fail(ctx, DFA_E_WORKSPACE, "train workspace too small");
  DFA_TRY(late());
  if (verdict == STEP_HOOK_CHANGED)
    return fail(ctx, DFA_E_UNSUPPORTED, "the SyncBN hook changed between %s and %s: dfa_ctx_set_bn_sync was %s since the forward", w.fwd, w.bwd,
                step.synced ? "cleared" : "armed");
  return DFA_OK;
}
inline int no_late_checks() { return DFA_OK; }

// dfa_<model>_set_params: null context / array, the pointer count, the model's own dimension rules (`dims`, a callable returning
// a code, run at their place between the two), no null pointer; then the pointers are bound to the model's slot `state`
template <typename State, typename Dims>
int set_params_core(dfa_ctx* ctx, State dfa_ctx::*state, const char* name, const float* const* device_params, int n, Dims dims) {
  if (!ctx || !device_params) return DFA_E_NULL_PTR;
  State& m = ctx->*state;
  constexpr int N = (int)(sizeof(m.p) / sizeof(m.p[0]));
  if (n != N) return fail(ctx, DFA_E_BAD_SHAPE, "%s expects %d parameter pointers, got %d", name, N, n);
  DFA_TRY(dims());
  for (int i = 0; i < n; ++i)
    if (!device_params[i]) return fail(ctx, DFA_E_NULL_PTR, "%s parameter %d is null", name, i);
  for (int i = 0; i < n; ++i) m.p[i] = device_params[i];
  m.have_params = true;
  m.train.step.live = false;      // a backward never runs with other weights than its forward's
  return DFA_OK;
}

}  // namespace dfa

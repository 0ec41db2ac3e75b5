// cnn1d_train_api.hip -- C ABI of the CNN1D training step, uniform and ragged (src/model_cnn1d.py in train mode, src/train.py:71-76):
// dfa_cnn1d_forward_train[_ragged] (Conv1d -> BatchNorm1d on batch statistics -> ReLU -> Dropout twice, Conv1d -> BN -> ReLU -> mean_T
// -> Linear) and dfa_cnn1d_backward[_ragged] (14 gradients from dlogits).  Arming, SyncBN hook, loss, optimiser: train_api.hip.
#include "train_host.h"
#include "trace.h"

using namespace dfa;

namespace {

struct Train1dPlan {
  size_t z[3], h[2], pooled, dpooled, dz[3], dh[2], stats, sums, partial, partial_bytes, total;
};

// k1 = taps of layer 1 (Cnn1dState::k1): sizes the weight-gradient records [32][F][k1] + [32]
Train1dPlan plan_train1d(int B, int T, int F, int k1) {
  Train1dPlan p;
  Bump take;
  const int C[3] = {32, 64, 128};
  for (int l = 0; l < 3; ++l) p.z[l] = take((size_t)B * C[l] * T * 4);
  for (int l = 0; l < 2; ++l) p.h[l] = take((size_t)B * C[l] * T * 4);
  p.pooled = take((size_t)B * 128 * 4);
  p.dpooled = take((size_t)B * 128 * 4);
  for (int l = 0; l < 3; ++l) p.dz[l] = take((size_t)B * C[l] * T * 4);
  for (int l = 0; l < 2; ++l) p.dh[l] = take((size_t)B * C[l] * T * 4);
  p.stats = take((32 + 64 + 128) * 3 * 4);
  p.sums = take((32 + 64 + 128) * 2 * 4);
  const size_t nch = (size_t)cm_chunks(B);
  size_t pb = nch * 128 * 2 * 4;
  const size_t wch = (size_t)conv1d_wgrad_chunks(B);
  pb = std::max(pb, wch * ((size_t)32 * F * k1 + 32) * 4);
  pb = std::max(pb, wch * ((size_t)128 * 64 * 3 + 128) * 4);
  p.partial_bytes = pb;
  p.partial = take(pb);
  p.total = take.off;
  return p;
}

// the shape a step refuses (what cnn1d_forward_train_impl and dfa_cnn1d_train_plan both answer, word for word)
int check_shape1d(dfa_ctx* ctx, int B, int T, bool ragged) {
  if (B < 1 || T < 1) return fail(ctx, DFA_E_BAD_SHAPE, "B and T must be >= 1 (got %d, %d)", B, T);
  if (ragged && T < 3) return fail(ctx, DFA_E_BAD_SHAPE, "T_max=%d is too short: a ragged cnn1d batch needs T_max >= 3", T);
  return DFA_OK;
}

const int kBnOff[3] = {0, 32, 96}, kBnC[3] = {32, 64, 128};     // BN layer order in the stats / sums blocks: layers 1-3
BnStats st1d(char* ws, const Train1dPlan& pl, int l) { return bn_stats(ws + pl.stats, kBnOff[l], kBnC[l]); }
float* sums1d(char* ws, const Train1dPlan& pl, int l) { return bn_sums(ws + pl.sums, kBnOff[l]); }

// A ragged batch (dfa_cnn1d_forward_train_ragged): x is padded to T = T_max frames, utterance b is x[b, :lengths[b], :].  The step
// is the reference model's on the utterances concatenated along time: each Conv1d zero-pads an utterance at
// its own two ends, BatchNorm1d's statistics run over the N = sum lengths[b] valid frames, the time mean of utterance b over its own.
// It is reached with the UNIFORM convolution / weight-gradient / data-gradient kernels on the padded batch, because three things
// hold at every padding frame t >= lengths[b]: x reads as zero (a bound in the loads of the kernels that read x), every activation
// h is written as an exact zero, and so is every dz.  The table ([0, B) lengths, [B, 2B) the staging's dispatch order, unused here)
// sits behind the uniform plan in the workspace; the backward reads it from there.
size_t ragged1d_tab_bytes(int B) { return align_up((size_t)2 * B * sizeof(int32_t), 256); }

// lengths == nullptr: the uniform step.  v: the entry point's arguments as they came, checked here
int cnn1d_forward_train_impl(dfa_ctx* ctx, const FeatView& v, const int32_t* lengths, float p_drop, uint64_t seed, uint64_t offset,
                             float momentum, int update_running_stats, float* logits, void* workspace, size_t workspace_bytes) {
  Cnn1dState& m = ctx->cnn1d;
  const float* x = (const float*)v.x;       // (float32: refused below otherwise)
  const int x_dtype = v.dtype, B = v.B, T = v.T, F = v.F;
  Cnn1dTrain& tr = m.train;
  const AugCfg armed = tr.aug_armed;    // one-shot: consumed here, also by a call that fails its checks below
  tr.aug_armed = AugCfg{};
  tr.step.live = false;                 // and the batch that was in flight is over, whatever this call returns
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cnn1d_set_params has not been called");
  if (m.k1 != 3 && lengths)    // the five-tap layer-1 kernels have no per-utterance bound in their loads
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d training step is built for kernels (3, 3, 3): dfa_cnn1d_set_kernels bound (%d, 3, 3), "
                                        "which trains on uniform batches only", m.k1);
  if (!x || !logits || !workspace) return fail(ctx, DFA_E_NULL_PTR, "x, logits and workspace must be non-null");
  if (x_dtype != DFA_DTYPE_F32) return fail(ctx, DFA_E_BAD_DTYPE, "cnn1d takes float32 input (got dtype %d)", x_dtype);
  DFA_TRY(check_shape1d(ctx, B, T, lengths != nullptr));
  if (F != m.in_features) return fail(ctx, DFA_E_BAD_SHAPE, "feature dim %d does not match in_features=%d", F, m.in_features);
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(ctx, DFA_E_BAD_SHAPE, "dropout p must be in [0, 1)");
  double frames = (double)B * T;             // frames BatchNorm1d counts
  if (lengths) {
    DFA_TRY(check_lengths(ctx, lengths, B, 3, T));
    frames = 0.0;
    for (int b = 0; b < B; ++b) frames += (double)lengths[b];
  }
  const Train1dPlan pl = plan_train1d(B, T, F, m.k1);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total + (lengths ? ragged1d_tab_bytes(B) : 0), false, "train "));
  if (armed.on && (armed.T != T || armed.F != F))
    return fail(ctx, DFA_E_BAD_SHAPE, "armed augmentation is for [T=%d, F=%d], the batch is [T=%d, F=%d]", armed.T, armed.F, T, F);
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int* lens = nullptr;                 // device table of a ragged batch
  if (lengths) {
    if (armed.on)
      return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d training step takes no train augmentation (dfa_cnn1d_set_train_augment was armed): "
                                          "a time roll has no per-utterance meaning yet");
    if (ctx->bn_sync.fn)
      return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d training step cannot run under synchronised BatchNorm (dfa_ctx_set_bn_sync is armed): "
                                          "the ranks' frame counts differ and the hook carries sums only");
    DFA_TRY(refuse_capture(ctx, "training step"));
    DFA_TRY(stage_ragged_lengths(ctx, lengths, B, (char*)workspace + pl.total));
    lens = (const int*)((char*)workspace + pl.total);
  }
  TrainStep step;                              // this call's record: committed to tr.step by the last statement
  step.B = B; step.T = T; step.F = F; step.x_dtype = x_dtype; step.ragged = lengths ? 1 : 0; step.frames = frames;
  step.synced = ctx->bn_sync.fn != nullptr; step.aug = armed;
  const AugCfg* aug = step.aug.on ? &step.aug : nullptr;
  if (!tr.train_packed) {
    Bump take;
    const size_t wt0 = take((size_t)64 * 32 * 3 * 4), wt1 = take((size_t)128 * 64 * 3 * 4), zb = take(256 * 4);
    DFA_HIP_CHECK(ctx, hipMalloc(&tr.train_packed, take.off));
    char* base = (char*)tr.train_packed;
    tr.wt[0] = (float*)(base + wt0); tr.wt[1] = (float*)(base + wt1); tr.zero_bias = (float*)(base + zb);
  }
  // bf16x3 A-fragment images of this step's weights (they change every step): forward layers 1-3, data gradients 3->2, 2->1
  const int xcin[5] = {F, 32, 64, 128, 64}, xcout[5] = {32, 64, 128, 64, 32};
  if (!tr.wx3[0] || tr.wx3_F != F || tr.wx3_k1 != m.k1) {
    if (tr.wx3[0]) { DFA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); DFA_HIP_CHECK(ctx, hipFree(tr.wx3[0])); tr.wx3[0] = nullptr; }
    Bump take;
    size_t off[5];
    for (int i = 0; i < 5; ++i) off[i] = take(conv1d_terms_pack_bytes(xcin[i], xcout[i], 3, i == 0 ? m.k1 : 3));
    char* base = nullptr;
    DFA_HIP_CHECK(ctx, hipMalloc((void**)&base, take.off));
    for (int i = 0; i < 5; ++i) tr.wx3[i] = base + off[i];
    tr.wx3_F = F; tr.wx3_k1 = m.k1;
  }
  const LayerParams layer[3] = {layer_params(m.p, 0), layer_params(m.p, 1), layer_params(m.p, 2)};
  const HeadParams head = head_params(m.p, kCnn1dLayers, 0);
  hipStream_t s = ctx->stream;
  const int x3 = ctx->cnn1d_train_x3, terms = (x3 == 3) ? 2 : 3;
  // the fp32 data-gradient images are only read by the vector-ALU fallback (T > 384, option 0)
  const bool dgrad_x3 = x3 && conv1d_x3_supports((const float*)workspace, (int64_t)128 * T, T, 1, (const float*)workspace, T, 128, 64, terms) &&
                        conv1d_x3_supports((const float*)workspace, (int64_t)64 * T, T, 1, (const float*)workspace, T, 64, 32, terms);
  if (!dgrad_x3) {
    DFA_HIP_CHECK(ctx, launch_conv1d_dgrad_pack(layer[1].w, tr.wt[0], tr.zero_bias, 32, 64, s));
    DFA_HIP_CHECK(ctx, launch_conv1d_dgrad_pack(layer[2].w, tr.wt[1], tr.zero_bias, 64, 128, s));
  }
  if (x3) DFA_HIP_CHECK(ctx, launch_pack_conv1d_train_all(layer[0].w, layer[1].w, layer[2].w, tr.wx3, F, terms, tr.zero_bias, s, m.k1));   // all five images, one launch
  step.x3 = x3;
  DropCfg dc = drop_cfg(p_drop, seed, offset);
  step.drop = dc;
  char* ws = (char*)workspace;
  float* partial = (float*)(ws + pl.partial);
  const int C[3] = {32, 64, 128}, Cin[3] = {F, 32, 64};
  const int nch = cm_chunks(B);
  for (int l = 0; l < 3; ++l) {
    float* z = (float*)(ws + pl.z[l]);
    const LayerParams& q = layer[l];
    if (l == 0) {
      // m.k1 taps (five: uniform batches only, refused above otherwise): the matrix-core kernel, else the tap-templated fp32
      // kernel; the armed augmentation or the ragged batch's bound is folded into the loads of either
      if (x3 && conv1d_x3_supports(x, v.sb, v.sf, v.st, z, T, F, 32, terms, m.k1))
        DFA_HIP_CHECK(ctx, launch_conv1d_x3(x, v.sb, tr.wx3[0], q.b, z, B, F, 32, T, terms, s, x3, aug, lens, m.k1));
      else
        DFA_HIP_CHECK(ctx, launch_conv1d(x, v.sb, v.sf, v.st, q.w, q.b, z, B, F, 32, T, false, s, false, aug, lens, m.k1));
    } else {
      const float* hin = (const float*)(ws + pl.h[l - 1]);
      if (x3 && conv1d_x3_supports(hin, (int64_t)Cin[l] * T, T, 1, z, T, Cin[l], C[l], terms))
        DFA_HIP_CHECK(ctx, launch_conv1d_x3(hin, (int64_t)Cin[l] * T, tr.wx3[l], q.b, z, B, Cin[l], C[l], T, terms, s, x3));
      else
        DFA_HIP_CHECK(ctx, launch_conv1d(hin, (int64_t)Cin[l] * T, T, 1, q.w, q.b, z, B, Cin[l], C[l], T, false, s, false));
    }
    BnStats st = st1d(ws, pl, l);
    const bool shifted = !step.synced;             // sums of z - z[0][c][0]: see cm_stats_body
    DFA_HIP_CHECK(ctx, launch_cm_stats(z, partial, B, C[l], T, s, lens, shifted));
    DFA_TRY(finalize_bn_stats(ctx, partial, nch, C[l], frames, st, running_stats(q, update_running_stats), momentum, nullptr, shifted ? z : nullptr, T));
    if (l < 2) {
      dc.layer = 1 + l;
      DFA_HIP_CHECK(ctx, launch_cm_bn_relu_drop(z, bn_apply(st, q), (float*)(ws + pl.h[l]), B, C[l], T, dc, s, lens));
    } else {
      DFA_HIP_CHECK(ctx, launch_cm_bn_relu_meant(z, bn_apply(st, q), (float*)(ws + pl.pooled), B, 128, T, s, lens));
    }
  }
  DFA_HIP_CHECK(ctx, launch_linear((const float*)(ws + pl.pooled), head.w, head.b, logits, B, 128, s));
  step.live = true;
  tr.step = step;
  return DFA_OK;
}

// ragged = which of the two entry points this is: it must be the one whose forward is in flight
int cnn1d_backward_impl(dfa_ctx* ctx, int ragged, const FeatView& v, const float* dlogits, float* const* grads, int ngrads, void* workspace,
                        size_t workspace_bytes) {
  const Cnn1dState& m = ctx->cnn1d;
  const Cnn1dTrain& tr = m.train;
  const TrainStep& step = tr.step;
  const int B = v.B, T = v.T, F = v.F;
  Train1dPlan pl;
  DFA_TRY(check_backward(
      ctx, {ragged ? "dfa_cnn1d_backward_ragged" : "dfa_cnn1d_backward", ragged ? "dfa_cnn1d_forward_train_ragged" : "dfa_cnn1d_forward_train",
            "cnn1d", kCnn1dGrads, "dlogits", true},
      step, B, T, F, ragged, v.x, v.dtype, dlogits, grads, ngrads, workspace, workspace_bytes,
      [&] { return (pl = plan_train1d(B, T, F, m.k1)).total + (ragged ? ragged1d_tab_bytes(B) : 0); },
      [&] {
        return !(ragged && ctx->bn_sync.fn) ? DFA_OK : fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d training step cannot run under synchronised "
                                                                                     "BatchNorm (dfa_ctx_set_bn_sync is armed)");
      }));
  char* ws = (char*)workspace;
  const int* lens = ragged ? (const int*)(ws + pl.total) : nullptr;     // the table the forward left behind the plan
  float* partial = (float*)(ws + pl.partial);
  const HeadGrads gh = head_grads(grads, kCnn1dLayers, 0);
  hipStream_t s = ctx->stream;
  DropCfg dc = step.drop;
  const int C[3] = {32, 64, 128}, Cin[3] = {F, 32, 64};
  float* dpooled = (float*)(ws + pl.dpooled);
  DFA_HIP_CHECK(ctx, launch_linear_bwd(dlogits, head_params(m.p, kCnn1dLayers, 0).w, (const float*)(ws + pl.pooled), dpooled, gh.dw, gh.db, B, 128, s));
  for (int l = 2; l >= 0; --l) {
    const LayerGrads g = layer_grads(grads, l);
    BnStats st = st1d(ws, pl, l);
    float* sm = sums1d(ws, pl, l);
    float* dz = (float*)(ws + pl.dz[l]);
    const float* up = (l == 2) ? dpooled : (const float*)(ws + pl.dh[l]);
    dc.layer = 1 + l;
    DFA_HIP_CHECK(ctx, launch_cm_bn_bwd(l == 2 ? 0 : 1, (const float*)(ws + pl.z[l]), bn_apply(st, layer_params(m.p, l)), up, partial, sm, dz,
                                        B, C[l], T, dc, s, step.synced ? &ctx->bn_sync : nullptr, lens, step.frames));
    DFA_HIP_CHECK(ctx, launch_split_sums(sm, g.dgamma, g.dbeta, C[l], s));
    if (l == 0) {
      DFA_HIP_CHECK(ctx, launch_conv1d_wgrad(dz, (const float*)v.x, v.sb, v.sf, v.st, partial, g.dw, g.db, B, F, 32, T, s,
                                             step.aug.on ? &step.aug : nullptr, step.x3, lens, m.k1));
    } else {
      DFA_HIP_CHECK(ctx, launch_conv1d_wgrad(dz, (const float*)(ws + pl.h[l - 1]), (int64_t)Cin[l] * T, T, 1, partial, g.dw,
                                             g.db, B, Cin[l], C[l], T, s, nullptr, step.x3));
      // data gradient: dh[l-1] = conv1d(dz; W'[Cin][Cout][3]) -- a Conv1d with Cout input channels, Cin output channels
      float* dh = (float*)(ws + pl.dh[l - 1]);
      const int terms = (step.x3 == 3) ? 2 : 3;
      if (step.x3 && conv1d_x3_supports(dz, (int64_t)C[l] * T, T, 1, dh, T, C[l], Cin[l], terms))
        DFA_HIP_CHECK(ctx, launch_conv1d_x3(dz, (int64_t)C[l] * T, tr.wx3[l == 2 ? 3 : 4], tr.zero_bias, dh, B, C[l], Cin[l], T, terms, s, step.x3));
      else
        DFA_HIP_CHECK(ctx, launch_conv1d(dz, (int64_t)C[l] * T, T, 1, tr.wt[l - 1], tr.zero_bias, dh, B, C[l], Cin[l], T, false, s, false));
    }
  }
  return DFA_OK;
}

}  // namespace

extern "C" {

size_t dfa_cnn1d_train_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F) {
  if (B < 1 || T < 1 || F < 1) return 0;
  return plan_train1d(B, T, F, ctx ? ctx->cnn1d.k1 : 3).total;
}

int dfa_cnn1d_train_plan(dfa_ctx* ctx, int B, int T, int F, int ragged, long long* fields, int cap) {
  DFA_TRY(check_shape1d(ctx, B, T, ragged != 0));
  if (F < 1) return fail(ctx, DFA_E_BAD_SHAPE, "feature dim %d: need F >= 1", F);
  if (ragged && ctx && ctx->cnn1d.k1 != 3)
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged cnn1d training step is built for kernels (3, 3, 3): dfa_cnn1d_set_kernels bound (%d, 3, 3)",
                ctx->cnn1d.k1);
  const Train1dPlan pl = plan_train1d(B, T, F, ctx ? ctx->cnn1d.k1 : 3);
  const long long v[] = {(long long)pl.z[0], (long long)pl.z[1], (long long)pl.z[2], (long long)pl.h[0], (long long)pl.h[1],
                         (long long)pl.pooled, (long long)pl.dpooled, (long long)pl.dz[0], (long long)pl.dz[1], (long long)pl.dz[2],
                         (long long)pl.dh[0], (long long)pl.dh[1], (long long)pl.stats, (long long)pl.sums, (long long)pl.partial,
                         (long long)pl.partial_bytes, ragged ? (long long)pl.total : -1LL,
                         (long long)(pl.total + (ragged ? ragged1d_tab_bytes(B) : 0))};
  static_assert(sizeof(v) / sizeof(v[0]) == DFA_CNN1D_TRAIN_PLAN_FIELDS, "field table of dfa_cnn1d_train_plan");
  for (int i = 0; fields && i < cap && i < DFA_CNN1D_TRAIN_PLAN_FIELDS; ++i) fields[i] = v[i];
  return DFA_CNN1D_TRAIN_PLAN_FIELDS;
}

int dfa_cnn1d_forward_train(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                            int64_t stride_t, int64_t stride_f, float p_drop, uint64_t seed, uint64_t offset,
                            float momentum, int update_running_stats, float* logits, void* workspace,
                            size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn1d_forward_train");
  if (!ctx) return DFA_E_NULL_PTR;
  return cnn1d_forward_train_impl(ctx, FeatView{x, x_dtype, stride_b, stride_t, stride_f, B, T, F}, nullptr, p_drop, seed, offset, momentum,
                                  update_running_stats, logits, workspace, workspace_bytes);
}

int dfa_cnn1d_backward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                       int64_t stride_f, const float* dlogits, float* const* grads, int ngrads, void* workspace,
                       size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn1d_backward");
  if (!ctx) return DFA_E_NULL_PTR;
  return cnn1d_backward_impl(ctx, 0, FeatView{x, x_dtype, stride_b, stride_t, stride_f, B, T, F}, dlogits, grads, ngrads, workspace, workspace_bytes);
}

size_t dfa_cnn1d_train_ragged_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int F) {
  if (B < 1 || T_max < 3 || F < 1 || (ctx && ctx->cnn1d.k1 != 3)) return 0;     // (no ragged step with five taps)
  return plan_train1d(B, T_max, F, 3).total + ragged1d_tab_bytes(B);
}

int dfa_cnn1d_forward_train_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b,
                                   int64_t stride_t, int64_t stride_f, const int32_t* lengths, float p_drop, uint64_t seed,
                                   uint64_t offset, float momentum, int update_running_stats, float* logits, void* workspace,
                                   size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn1d_forward_train_ragged");
  if (!ctx) return DFA_E_NULL_PTR;
  if (!lengths) {
    ctx->cnn1d.train.aug_armed = AugCfg{};      // one-shot, as in every forward_train; and the batch in flight is over
    ctx->cnn1d.train.step.live = false;
    return fail(ctx, DFA_E_NULL_PTR, "lengths must be non-null");
  }
  return cnn1d_forward_train_impl(ctx, FeatView{x, x_dtype, stride_b, stride_t, stride_f, B, T_max, F}, lengths, p_drop, seed, offset, momentum,
                                  update_running_stats, logits, workspace, workspace_bytes);
}

int dfa_cnn1d_backward_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b, int64_t stride_t,
                              int64_t stride_f, const float* dlogits, float* const* grads, int ngrads, void* workspace,
                              size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn1d_backward_ragged");
  if (!ctx) return DFA_E_NULL_PTR;
  return cnn1d_backward_impl(ctx, 1, FeatView{x, x_dtype, stride_b, stride_t, stride_f, B, T_max, F}, dlogits, grads, ngrads, workspace,
                             workspace_bytes);
}

}  // extern "C"

// dlq_train_api.hip -- C ABI of the DeepfakeDetector training step (include/dfa_hip.h; kernels in dlq.hip MODE 1 / 2 and dlq_train.hip):
// dfa_dlq_forward_train, dfa_dlq_backward, the pos_weight BCE and the gradient clip.  The step is DENSE over the padded batch: it
// depends on the batch's composition and on T_max, as the reference's does.
#include "train_host.h"
#include "trace.h"

using namespace dfa;

namespace {

constexpr int NF = DFA_DLQ_TILE_FRAMES;
constexpr int HID = 256;

struct DlqTrainPlan {
  int tpu, ntiles, nch;
  size_t tab, z[3], h[2], dy, dz, stats, rec, sums, pooled, pvar, u, du, dpooled, dbrec, scratch, partial, total;
};
DlqTrainPlan plan_dlq_train(int B, int T_max, int in_ch) {
  DlqTrainPlan p;
  Bump take;
  const size_t N = (size_t)B * T_max;
  p.tpu = (T_max + NF - 1) / NF;
  p.ntiles = B * p.tpu;
  int CH;
  dlq_wgrad_chunks((long long)N, &CH, &p.nch);
  p.tab = take((size_t)2 * B * 4);
  for (int l = 0; l < 3; ++l) p.z[l] = take(N * HID * 4);
  for (int l = 0; l < 2; ++l) p.h[l] = take(N * 1536);
  p.dy = take(N * HID * 4);
  p.dz = take(N * 1536);
  p.stats = take(3 * 3 * HID * 4);
  p.rec = take((size_t)p.ntiles * 2 * HID * 4);
  p.sums = take(2 * HID * 4);
  p.pooled = take((size_t)B * 2 * HID * 4);
  p.pvar = take((size_t)B * HID * 4);
  p.u = take((size_t)B * HID * 4);
  p.du = take((size_t)B * HID * 4);
  p.dpooled = take((size_t)B * 2 * HID * 4);
  p.dbrec = take((size_t)dlq_dz_blocks((long long)N) * HID * 4);
  p.scratch = take((size_t)64 * 2 * HID * 4);
  p.partial = take((size_t)p.nch * HID * std::max(3 * HID, 5 * in_ch) * 4);
  p.total = take.off;
  return p;
}

BnStats st_dlq(char* ws, const DlqTrainPlan& pl, int l) { return bn_stats(ws + pl.stats, HID * l, HID); }

// what launch_dlq_pool_head, launch_dlq_head_bwd and launch_dlq_dy3 share: layer 3's terms, the head's two pairs, the pool's buffers
DlqHeadArgs head_args(const DlqState& m, char* ws, const DlqTrainPlan& pl) {
  DlqHeadArgs h{};
  const BnApply bn = bn_apply(st_dlq(ws, pl, 2), layer_params(m.p, 2));
  const HeadParams h0 = head_params(m.p, kDlqLayers, 0), h3 = head_params(m.p, kDlqLayers, 1);
  h.z3 = (const float*)(ws + pl.z[2]); h.mean = bn.mean; h.invstd = bn.invstd; h.gamma = bn.gamma; h.beta = bn.beta;
  h.w0 = h0.w; h.b0 = h0.b; h.w3 = h3.w; h.b3 = h3.b;
  h.pooled = (float*)(ws + pl.pooled); h.pvar = (float*)(ws + pl.pvar); h.u = (float*)(ws + pl.u);
  return h;
}

int check_dlq_shape(dfa_ctx* ctx, int B, int T_max, int in_ch) {
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "batch must be >= 1 (got B=%d)", B);
  if (T_max < 1) return fail(ctx, DFA_E_BAD_SHAPE, "T_max must be >= 1 (got %d)", T_max);
  if ((long long)B * T_max < 2)
    return fail(ctx, DFA_E_BAD_SHAPE, "BatchNorm1d in train mode needs more than one value per channel: B * T_max = %lld (B=%d, T_max=%d)",
                (long long)B * T_max, B, T_max);
  if ((long long)B * T_max * HID >= ((long long)1 << 31))
    return fail(ctx, DFA_E_UNSUPPORTED, "B * T_max = %lld frames exceed the training step's limit of 2^23 - 1", (long long)B * T_max);
  if (in_ch != ctx->dlq.in_ch)
    return fail(ctx, DFA_E_BAD_SHAPE, "channel dim in_ch=%d does not match in_ch=%d of the first Conv1d (src/dlqueen_model.py:136)", in_ch, ctx->dlq.in_ch);
  return DFA_OK;
}

}  // namespace

extern "C" {

size_t dfa_dlq_train_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int in_ch) {
  (void)ctx;
  if (B < 1 || T_max < 1 || (long long)B * T_max < 2 || in_ch < 1 || (long long)B * T_max * HID >= ((long long)1 << 31)) return 0;
  return plan_dlq_train(B, T_max, in_ch).total;
}

int dfa_dlq_forward_train(dfa_ctx* ctx, const void* x, int B, int T_max, int in_ch, int64_t stride_b, int64_t stride_c, const int32_t* lengths,
                          float p_drop, uint64_t seed, uint64_t offset, float momentum, int update_running_stats, float* logits,
                          uint8_t* keep_out, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_dlq_forward_train");
  if (!ctx) return DFA_E_NULL_PTR;
  DlqState& m = ctx->dlq;
  DlqTrain& tr = m.train;
  tr.step.live = false;                          // a refused forward leaves none in flight
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_dlq_set_params has not been called");
  if (!x || !logits || !workspace || !lengths) return fail(ctx, DFA_E_NULL_PTR, "x, lengths, logits and workspace must be non-null");
  DFA_TRY(check_dlq_shape(ctx, B, T_max, in_ch));
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(ctx, DFA_E_BAD_SHAPE, "dropout p_drop must be in [0, 1)");
  DFA_TRY(check_lengths(ctx, lengths, B, 1, T_max));
  DFA_TRY(check_channel_major(ctx, "DeepfakeDetector training step", "stride_c", x, stride_b, stride_c, T_max));
  const DlqTrainPlan pl = plan_dlq_train(B, T_max, in_ch);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total, true, "train "));
  if (ctx->bn_sync.fn)
    return fail(ctx, DFA_E_UNSUPPORTED, "the DeepfakeDetector training step is single-rank in this version: it cannot run under synchronised "
                                        "BatchNorm (dfa_ctx_set_bn_sync is armed)");
  DFA_TRY(refuse_capture(ctx, "training step"));
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!tr.train_packed || tr.tw_in_ch != in_ch) {
    if (tr.train_packed) { DFA_HIP_CHECK(ctx, hipStreamSynchronize(s)); DFA_HIP_CHECK(ctx, hipFree(tr.train_packed)); tr.train_packed = nullptr; }
    Bump take;
    size_t off[5];
    off[0] = take(dlq_pack_bytes(in_ch, 5));
    for (int q = 1; q < 5; ++q) off[q] = take(dlq_pack_bytes(HID, 3));
    DFA_HIP_CHECK(ctx, hipMalloc(&tr.train_packed, take.off));
    for (int q = 0; q < 5; ++q) tr.tw[q] = (char*)tr.train_packed + off[q];
    tr.tw_in_ch = in_ch;
  }
  DFA_TRY(stage_ragged_lengths(ctx, lengths, B, workspace));
  char* ws = (char*)workspace;
  const long long N = (long long)B * T_max;
  {
    ScopedSlot ts(ctx, 8);
    DFA_HIP_CHECK(ctx, launch_dlq_train_pack(layer_params(m.p, 0).w, layer_params(m.p, 1).w, layer_params(m.p, 2).w, tr.tw, in_ch, s));
  }
  DropCfg dc = drop_cfg(p_drop, seed, offset);
  DlqLayerArgs a{};
  a.x = (const float*)x; a.sb = stride_b; a.sc = stride_c;
  a.tab = (const int*)(ws + pl.tab);
  a.B = B; a.T_max = T_max; a.tpu = pl.tpu;
  a.rec = (float*)(ws + pl.rec);
  for (int l = 0; l < 3; ++l) {
    const LayerParams q = layer_params(m.p, l);
    BnStats st = st_dlq(ws, pl, l);
    const RunningStats run = running_stats(q, update_running_stats);
    {
      ScopedSlot ts(ctx, 9);
      a.hin = l ? (const uint4*)(ws + pl.h[l - 1]) : nullptr;
      a.w = (const uint4*)tr.tw[l]; a.bias = q.b;
      a.C = l ? HID : in_ch; a.nks = dlq_nks(a.C);
      a.zout = (float*)(ws + pl.z[l]);
      DFA_HIP_CHECK(ctx, launch_dlq_layer_train(l + 1, 1, a, pl.ntiles, s));
    }
    ScopedSlot ts(ctx, 10);
    DFA_HIP_CHECK(ctx, launch_dlq_bn_finalize(a.rec, pl.ntiles, pl.tpu, T_max, st.mean, st.var, st.invstd, run.mean, run.var, momentum, s));
    if (l < 2) {
      dc.layer = 1 + l;
      DFA_HIP_CHECK(ctx, launch_dlq_bn_act(a.zout, bn_apply(st, q), ws + pl.h[l], keep_out ? keep_out + (size_t)l * N * HID : nullptr, N, dc, s));
    }
  }
  {
    ScopedSlot ts(ctx, 10);
    DlqHeadArgs h = head_args(m, ws, pl);
    h.lens = a.tab; h.logits = logits;
    h.keep3 = keep_out ? keep_out + (size_t)2 * N * HID : nullptr;
    h.keep4 = keep_out ? keep_out + (size_t)3 * N * HID : nullptr;
    h.T_max = T_max;
    dc.layer = 3;
    h.drop = dc;
    DFA_HIP_CHECK(ctx, launch_dlq_pool_head(h, B, s));
  }
  TrainStep step;                                  // committed last: live only once every launch above went out
  step.B = B; step.T = T_max; step.F = in_ch; step.x_dtype = DFA_DTYPE_F32; step.drop = dc;
  step.live = true;
  tr.step = step;
  return DFA_OK;
}

int dfa_dlq_backward(dfa_ctx* ctx, const void* x, int B, int T_max, int in_ch, int64_t stride_b, int64_t stride_c, const float* dlogits,
                     float* const* grads, int ngrads, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_dlq_backward");
  if (!ctx) return DFA_E_NULL_PTR;
  const DlqState& m = ctx->dlq;
  const DlqTrain& tr = m.train;
  DlqTrainPlan pl;
  DFA_TRY(check_backward(
      ctx, {"dfa_dlq_backward", "dfa_dlq_forward_train", "the DeepfakeDetector", kDlqGrads, "dlogits", false}, tr.step, B, T_max, in_ch, 0, x,
      DFA_DTYPE_F32, dlogits, grads, ngrads, workspace, workspace_bytes, [&] { return (pl = plan_dlq_train(B, T_max, in_ch)).total; },
      [&] {
        DFA_TRY(check_channel_major(ctx, "DeepfakeDetector training step", "stride_c", x, stride_b, stride_c, T_max));
        return !ctx->bn_sync.fn ? DFA_OK : fail(ctx, DFA_E_UNSUPPORTED, "the DeepfakeDetector training step is single-rank in this version: it cannot "
                                                                        "run under synchronised BatchNorm (dfa_ctx_set_bn_sync is armed)");
      }));
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  char* ws = (char*)workspace;
  const long long N = (long long)B * T_max;
  const int* lens = (const int*)(ws + pl.tab);       // the table the forward left
  float* rec = (float*)(ws + pl.rec);
  float* sums = (float*)(ws + pl.sums);
  float* scratch = (float*)(ws + pl.scratch);
  float* dy = (float*)(ws + pl.dy);
  float* dbrec = (float*)(ws + pl.dbrec);
  DropCfg dc = tr.step.drop;
  {
    ScopedSlot ts(ctx, 11);
    const HeadGrads g0 = head_grads(grads, kDlqLayers, 0), g3 = head_grads(grads, kDlqLayers, 1);
    DlqHeadArgs h = head_args(m, ws, pl);
    h.lens = lens;
    h.dlogits = dlogits; h.du = (float*)(ws + pl.du); h.dpooled = (float*)(ws + pl.dpooled);
    h.T_max = T_max;
    dc.layer = 3;
    h.drop = dc;
    DFA_HIP_CHECK(ctx, launch_dlq_head_bwd(h, B, g0.dw, g0.db, g3.dw, g3.db, s));
    DFA_HIP_CHECK(ctx, launch_dlq_dy3(h, B, pl.tpu, dy, rec, s));
  }
  for (int l = 2; l >= 0; --l) {
    const BnApply bn = bn_apply(st_dlq(ws, pl, l), layer_params(m.p, l));
    const LayerGrads g = layer_grads(grads, l);
    {
      ScopedSlot ts(ctx, 11);
      DFA_HIP_CHECK(ctx, launch_reduce_partials(rec, pl.ntiles, 2 * HID, 1.0f, sums, s, scratch));
      DFA_HIP_CHECK(ctx, launch_split_sums(sums, g.dgamma, g.dbeta, HID, s));
      DFA_HIP_CHECK(ctx, launch_dlq_dz(dy, (const float*)(ws + pl.z[l]), bn, sums, ws + pl.dz, dbrec, N, s));
      DFA_HIP_CHECK(ctx, launch_reduce_partials(dbrec, dlq_dz_blocks(N), HID, 1.0f, g.db, s, scratch));
    }
    {
      ScopedSlot ts(ctx, 13);
      DlqWgradArgs w{};
      w.dz = (const uint4*)(ws + pl.dz);
      w.lens = lens; w.partial = (float*)(ws + pl.partial); w.N = N; w.T_max = T_max;
      if (l == 0) { w.x = (const float*)x; w.sb = stride_b; w.sc = stride_c; w.C = in_ch; w.taps = 5; }
      else { w.h = (const uint4*)(ws + pl.h[l - 1]); w.C = HID; w.taps = 3; }
      DFA_HIP_CHECK(ctx, launch_dlq_wgrad(w, g.dw, s));
    }
    if (l > 0) {        // dy of the layer below: the 256 -> 256 k3 layer kernel on the data-gradient image, dz as its input
      ScopedSlot ts(ctx, 12);
      const BnApply below = bn_apply(st_dlq(ws, pl, l - 1), layer_params(m.p, l - 1));
      DlqLayerArgs a{};
      a.tab = lens; a.B = B; a.T_max = T_max; a.tpu = pl.tpu; a.C = HID; a.nks = 16;
      a.hin = (const uint4*)(ws + pl.dz); a.w = (const uint4*)tr.tw[l == 2 ? 3 : 4];
      a.zout = dy; a.rec = rec;
      a.zprev = (const float*)(ws + pl.z[l - 1]); a.st_mean = below.mean; a.st_invstd = below.invstd; a.gamma = below.gamma; a.beta = below.beta;
      dc.layer = l;
      a.drop = dc;
      DFA_HIP_CHECK(ctx, launch_dlq_layer_train(2, 2, a, pl.ntiles, s));
    }
  }
  return DFA_OK;
}

int dfa_bce_pos_weight_fwd_bwd(dfa_ctx* ctx, const float* logits, const float* labels, float pos_weight, int B, float* loss, float* dlogits) {
  if (!ctx) return DFA_E_NULL_PTR;
  if (!logits || !labels) return fail(ctx, DFA_E_NULL_PTR, "logits and labels must be non-null");
  if (!(pos_weight > 0.f)) return fail(ctx, DFA_E_BAD_SHAPE, "pos_weight must be > 0 (got %g)", (double)pos_weight);
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "B must be >= 1 (got %d)", B);
  DFA_HIP_CHECK(ctx, launch_bce_pos_weight(logits, labels, pos_weight, B, loss, dlogits, ctx->stream));
  return DFA_OK;
}

int dfa_clip_grad_norm(dfa_ctx* ctx, float* grad, size_t n, float max_norm, float* norm_out) {
  if (!ctx) return DFA_E_NULL_PTR;
  if (!grad) return fail(ctx, DFA_E_NULL_PTR, "grad must be non-null");
  if (!(max_norm > 0.f)) return fail(ctx, DFA_E_BAD_SHAPE, "max_norm must be > 0 (got %g)", (double)max_norm);
  if (n == 0) return DFA_OK;
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!ctx->clip_partial) DFA_HIP_CHECK(ctx, hipMalloc((void**)&ctx->clip_partial, 256 * sizeof(double)));
  DFA_HIP_CHECK(ctx, launch_clip_grad_norm(grad, n, max_norm, norm_out, ctx->clip_partial, ctx->stream));
  return DFA_OK;
}

}  // extern "C"

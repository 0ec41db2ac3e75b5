// train_api.hip -- C ABI of the CNN2D training step (replaces, for src/train.py:71-76, what torch autograd does
// with src/model.py:13-39 in train mode):
//   dfa_cnn2d_forward_train : conv -> BatchNorm(batch statistics, running-stat update) -> ReLU -> AvgPool -> Dropout x2,
//                             conv -> BN -> ReLU -> mean_T -> Linear, keeping what backward needs in the workspace
//   dfa_cnn2d_backward      : gradients of all 14 parameters from dlogits (in parameters() order)
//   dfa_bce_smooth_fwd_bwd  : BCEWithLogitsLoss(mean) on smoothed labels + dlogits      (src/train.py:311-320)
//   dfa_adamw_step          : torch.optim.AdamW update of one flat fp32 buffer           (src/train.py:326-328)
#include "train_host.h"
#include "trace.h"

using namespace dfa;

namespace {

struct TrainPlan {
  int H1, H2;
  size_t a1, z2, a2, z3, emb, demb, msum, dz3, da2, dz2, da1, raw, stats, sums, partial, partial_bytes, total;
};

TrainPlan plan_train(int B, int T, int F, int prec) {
  TrainPlan p;
  const size_t es = (prec == DFA_PREC_BF16) ? 2 : 4;
  p.H1 = T / 2;
  p.H2 = p.H1 / 2;
  Bump take;
  p.a1 = take((size_t)B * p.H1 * F * 32 * es);
  p.z2 = take((size_t)B * p.H1 * F * 64 * es);
  p.a2 = take((size_t)B * p.H2 * F * 64 * es);
  p.z3 = take((size_t)B * p.H2 * F * 128 * es);
  p.emb = take((size_t)B * 128 * F * 4);
  p.demb = take((size_t)B * 128 * F * 4);
  p.msum = take((size_t)B * 128 * F * 2 * 4);        // block 3: per (b, f, c) mask count and mask*xhat sum over t (bn_relu_meant)
  p.dz3 = take((size_t)B * p.H2 * F * 128 * es);
  p.da2 = take((size_t)B * p.H2 * F * 64 * es);
  p.dz2 = take((size_t)B * p.H1 * F * 64 * es);
  p.da1 = take((size_t)B * p.H1 * F * 32 * es);
  p.raw = take((size_t)B * p.H2 * F * 64 * 4);
  p.stats = take((32 + 64 + 128) * 3 * 4);          // mean | var | invstd per layer
  p.sums = take((32 + 64 + 128) * 2 * 4 + 352 * 4 + 96 * 4);  // (S1,S2) per layer + conv1 backward record [32][11] + XX[9][9] | Xs[9]
  const int nstrips = (F + 29) / 30;                                         // (the 30-column strips of conv3_m16: >= the 32-column count)
  size_t pb = (size_t)B * nstrips * 128 * 2 * 4;                              // conv stats partials
  pb = std::max(pb, ((size_t)conv1_train_blocks(B, T, F) + 64) * 352 * 4);   // conv1 passes + 2nd-level scratch
  int ppb;
  pb = std::max(pb, ((size_t)bn_bwd_blocks(B, p.H1, F, &ppb) + 64) * 128 * 2 * 4);  // BN backward partials + 2nd-level scratch
  pb = std::max(pb, (size_t)kWgradWGs * ((size_t)128 * 64 * 9 + 256) * 4);   // weight-gradient partials
  pb = std::max(pb, ((size_t)B * F / 128 + 1) * 128 * 2 * 4);                // saved-sum BN reduction partials (8 * 16 positions per block)
  p.partial_bytes = pb;
  p.partial = take(pb);
  p.total = take.off;
  return p;
}

const int kBnOff[3] = {0, 32, 96}, kBnC[3] = {32, 64, 128};     // BN layer order in the stats / sums blocks: blocks 1-3
BnStats stat_ptrs(char* ws, const TrainPlan& pl, int layer) { return bn_stats(ws + pl.stats, kBnOff[layer], kBnC[layer]); }
float* sums_ptr(char* ws, const TrainPlan& pl, int layer) { return bn_sums(ws + pl.sums, kBnOff[layer]); }

// block 1 of a step: what conv1_train_stats (forward) and conv1_train_backward (backward, da = da1) take
Conv1Train conv1_block(const Cnn2dState& m, const TrainStep& step, const FeatView& v, char* ws, const TrainPlan& pl, const DropCfg& dc) {
  float* c1rec = (float*)(ws + pl.sums) + 2 * (32 + 64 + 128);      // [32][11] record, then XX[9][9] | Xs[9]
  Conv1Train c{};
  c.v = v; c.prec = step.prec; c.poolw = 1;
  c.drop = dc; c.aug = step.aug.on ? &step.aug : nullptr; c.p = layer_params(m.p, 0); c.fw = m.train.tw1; c.fb = m.train.tb1;
  c.partial = (float*)(ws + pl.partial); c.stats_scratch = true; c.xxs = c1rec + 352; c.c1rec = c1rec;
  c.sums = sums_ptr(ws, pl, 0); c.stats = stat_ptrs(ws, pl, 0); c.da = ws + pl.da1;
  return c;
}

// the plan of a step, or the refusal of its precision or shape (what dfa_cnn2d_forward_train and dfa_cnn2d_train_plan both answer);
// armed: the forward's one-shot augmentation, refused between the two where it was drawn for another shape
int checked_plan(dfa_ctx* ctx, int B, int T, int F, int precision, const AugCfg* armed, TrainPlan* pl) {
  if (precision != DFA_PREC_F32 && precision != DFA_PREC_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "unknown precision %d", precision);
  if (armed && armed->on && (armed->T != T || armed->F != F))
    return fail(ctx, DFA_E_BAD_SHAPE, "the armed augmentation was drawn for [T=%d, F=%d], the batch is [T=%d, F=%d]", armed->T, armed->F, T, F);
  if (B < 1 || T < 4) return fail(ctx, DFA_E_BAD_SHAPE, "need B >= 1 and T >= 4 (got %d, %d)", B, T);
  if (F < 1) return fail(ctx, DFA_E_BAD_SHAPE, "feature dim %d: need F >= 1", F);
  *pl = plan_train(B, T, F, precision);
  return DFA_OK;
}

}  // namespace

extern "C" {

size_t dfa_cnn2d_train_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F, int precision) {
  (void)ctx;
  if (B < 1 || T < 4 || F < 1) return 0;
  return plan_train(B, T, F, precision).total;
}

int dfa_cnn2d_train_plan(dfa_ctx* ctx, int B, int T, int F, int precision, long long* fields, int cap) {
  TrainPlan pl;
  DFA_TRY(checked_plan(ctx, B, T, F, precision, nullptr, &pl));
  const long long v[] = {pl.H1, pl.H2, precision == DFA_PREC_BF16 ? 2 : 4,
                         (long long)pl.a1, (long long)pl.z2, (long long)pl.a2, (long long)pl.z3, (long long)pl.emb, (long long)pl.demb,
                         (long long)pl.msum, (long long)pl.dz3, (long long)pl.da2, (long long)pl.dz2, (long long)pl.da1, (long long)pl.raw,
                         (long long)pl.stats, (long long)pl.sums, (long long)pl.partial, (long long)pl.partial_bytes, (long long)pl.total};
  static_assert(sizeof(v) / sizeof(v[0]) == DFA_CNN2D_TRAIN_PLAN_FIELDS, "field table of dfa_cnn2d_train_plan");
  for (int i = 0; fields && i < cap && i < DFA_CNN2D_TRAIN_PLAN_FIELDS; ++i) fields[i] = v[i];
  return DFA_CNN2D_TRAIN_PLAN_FIELDS;
}

int dfa_cnn2d_forward_train(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                            int64_t stride_t, int64_t stride_f, int precision, float p_drop, uint64_t seed,
                            uint64_t offset, float momentum, int update_running_stats, float* logits, float* embedding,
                            void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn2d_forward_train");
  if (!ctx) return DFA_E_NULL_PTR;
  Cnn2dState& m = ctx->cnn2d;
  Cnn2dTrain& tr = m.train;
  // The augmentation armed by dfa_cnn2d_set_train_augment is one-shot and belongs to THIS call: it is taken (and the arm cleared)
  // before any check can return, so a failed forward never leaves it armed for an unrelated later batch.  The step record
  // likewise: whatever this call returns, the batch that was in flight is over.
  const AugCfg armed = tr.aug_armed;
  tr.aug_armed = AugCfg{};
  tr.step.live = false;
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cnn2d_set_params has not been called");
  if (!x || !logits || !workspace) return fail(ctx, DFA_E_NULL_PTR, "x, logits and workspace must be non-null");
  if (x_dtype != DFA_DTYPE_F32 && x_dtype != DFA_DTYPE_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "x dtype %d not supported", x_dtype);
  TrainPlan pl;
  DFA_TRY(checked_plan(ctx, B, T, F, precision, &armed, &pl));
  if (F != m.in_features) return fail(ctx, DFA_E_BAD_SHAPE, "feature dim %d does not match in_features=%d", F, m.in_features);
  if (!(p_drop >= 0.f && p_drop < 1.f)) return fail(ctx, DFA_E_BAD_SHAPE, "dropout p must be in [0, 1)");
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total, true, "train "));
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // train-mode weight images: raw convs (BN is its own pass) + data-gradient images; rebuilt every step (weights move)
  if (!tr.train_packed) {
    const size_t w2 = (size_t)64 * 32 * 9 * 4, w3 = (size_t)128 * 64 * 9 * 4;
    Bump take;
    const size_t small = take((288 + 32 + 64 + 128 + 32 + 64) * 4), t2 = take(w2), t3 = take(w3), d2 = take(w2), d3 = take(w3);
    DFA_HIP_CHECK(ctx, hipMalloc(&tr.train_packed, take.off));
    char* base = (char*)tr.train_packed;
    tr.tw1 = (float*)(base + small); tr.tb1 = tr.tw1 + 288;
    tr.t2.bias = tr.tb1 + 32; tr.t3.bias = tr.t2.bias + 64;
    tr.d2.bias = tr.t3.bias + 128; tr.d3.bias = tr.d2.bias + 32;
    tr.t2.wpack = (uint4*)(base + t2); tr.t3.wpack = (uint4*)(base + t3);
    tr.d2.wpack = (uint4*)(base + d2); tr.d3.wpack = (uint4*)(base + d3);
  }
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T, F};
  const LayerParams l2 = layer_params(m.p, 1), l3 = layer_params(m.p, 2);
  const HeadParams head = head_params(m.p, kCnn2dLayers, 0);
  hipStream_t s = ctx->stream;
  const int prec = precision;
  DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(raw_conv(l2), 32, 0, 32, 64, prec, tr.t2.wpack, tr.t2.bias, s));
  DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(raw_conv(l3), 64, 0, 64, 128, prec, tr.t3.wpack, tr.t3.bias, s));
  // bf16: the 16x16x32 image of the same raw weights, in the unused second half of the (fp32-sized) t3 buffer
  uint4* t3_m16 = (uint4*)((char*)tr.t3.wpack + (size_t)128 * 64 * 9 * 2);
  const bool fwd3_m16 = prec == DFA_PREC_BF16 && ctx->train_conv_variant != 1;   // 2: pipelined, 0: its compiler-scheduled twin
  if (fwd3_m16)
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3_m16(raw_conv(l3), 64, 128, t3_m16, s));
  TrainStep step;              // this call's record: committed to tr.step by the last statement
  step.B = B; step.T = T; step.F = F; step.prec = prec; step.x_dtype = x_dtype; step.synced = ctx->bn_sync.fn != nullptr;
  step.dgrad_m16 = (prec == DFA_PREC_BF16 && ctx->dgrad_m16) ? 1 : 0;
  DFA_TRY(pack_dgrad_images(ctx, l2.w, l3.w, prec, step.dgrad_m16, tr.d2, tr.d3));
  char* ws = (char*)workspace;
  float* partial = (float*)(ws + pl.partial);
  DropCfg dc = drop_cfg(p_drop, seed, offset);
  step.drop = dc;
  // ---- block 1
  // augmentation armed by dfa_cnn2d_set_train_augment: one-shot, folded into the three kernels that read x
  step.aug = armed;
  const AugCfg* aug = step.aug.on ? &step.aug : nullptr;
  // synchronised BatchNorm needs the layer's (sum dy, sum dy*xhat) BEFORE the weight gradient is formed: block 1 then takes the
  // two-pass vector path (reduce -> hook -> weight gradient), not the one-pass moment algebra
  step.c1_fused = (ctx->conv1_bwd_fused && !step.synced) ? 1 : 0;
  // matrix-core passes: bf16 mode on bf16 features without a folded augmentation (its noise makes x non-bf16), fused backward
  // (the backward reads da1 with the dropout keep mask already applied by the 16x16x32 data-gradient kernel)
  step.c1_mfma = (ctx->conv1_mfma && step.c1_fused && prec == DFA_PREC_BF16 && x_dtype == DFA_DTYPE_BF16 && !aug && F <= 224 &&
                (dc.thresh == 0 || step.dgrad_m16)) ? 1 : 0;
  DFA_TRY(conv1_train_stats(ctx, conv1_block(m, step, v, ws, pl, dc), step.c1_mfma, step.c1_fused, update_running_stats != 0, momentum));
  dc.layer = 1;
  if (step.c1_mfma)
    DFA_HIP_CHECK(ctx, launch_conv1_mfma(C1X_FWD, v, tr.tw1, tr.tb1, ws + pl.a1, nullptr, nullptr, dc, 1, s));
  else
    DFA_HIP_CHECK(ctx, launch_conv1(v, tr.tw1, tr.tb1, ws + pl.a1, prec, s, &dc, aug));
  // ---- block 2
  const int nstrips = (F + 31) / 32;
  {
    ConvArgs a = conv_args(ws + pl.a1, tr.t2, ws + pl.z2, B, pl.H1, F, 64, ctx);
    a.stats_partial = partial;
    DFA_HIP_CHECK(ctx, launch_train_fwd2(prec, a, s, ctx->train_conv_variant));
  }
  BnStats s2 = stat_ptrs(ws, pl, 1);
  DFA_TRY(finalize_bn_stats(ctx, partial, B * nstrips, 64, (double)B * pl.H1 * F, s2, running_stats(l2, update_running_stats), momentum, partial + (size_t)B * nstrips * 128));
  dc.layer = 2;
  DFA_HIP_CHECK(ctx, launch_bn_relu_pool_drop(prec, ws + pl.z2, bn_apply(s2, l2), ws + pl.a2, B, pl.H1, F, 64, dc, s));
  // ---- block 3
  {
    ConvArgs a = conv_args(ws + pl.a2, tr.t3, ws + pl.z3, B, pl.H2, F, 128, ctx);
    a.stats_partial = partial;
    if (fwd3_m16) {
      a.wpack = t3_m16;
      DFA_HIP_CHECK(ctx, launch_train_fwd3_m16(a, s, ctx->train_conv_variant == 2));
    } else {
      DFA_HIP_CHECK(ctx, launch_train_fwd3(prec, a, s));
    }
  }
  BnStats s3 = stat_ptrs(ws, pl, 2);
  const int np3 = B * (fwd3_m16 ? (F + 29) / 30 : nstrips);   // conv3_m16 owns 30 columns per strip
  DFA_TRY(finalize_bn_stats(ctx, partial, np3, 128, (double)B * pl.H2 * F, s3, running_stats(l3, update_running_stats), momentum, partial + (size_t)np3 * 256));
  float* emb = (float*)(ws + pl.emb);
  DFA_HIP_CHECK(ctx, launch_bn_relu_meant(prec, ws + pl.z3, bn_apply(s3, l3), emb, B, pl.H2, F, 128, s, (float*)(ws + pl.msum)));
  if (embedding) DFA_HIP_CHECK(ctx, hipMemcpyAsync(embedding, emb, (size_t)B * 128 * F * 4, hipMemcpyDeviceToDevice, s));
  DFA_HIP_CHECK(ctx, launch_linear(emb, head.w, head.b, logits, B, 128 * F, s));
  step.live = true;
  tr.step = step;
  return DFA_OK;
}

int dfa_cnn2d_backward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                       int64_t stride_f, const float* dlogits, float* const* grads, int ngrads, void* workspace,
                       size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn2d_backward");
  if (!ctx) return DFA_E_NULL_PTR;
  const Cnn2dState& m = ctx->cnn2d;
  const Cnn2dTrain& tr = m.train;
  const TrainStep& step = tr.step;
  const int prec = step.prec;
  TrainPlan pl;
  DFA_TRY(check_backward(ctx, {"dfa_cnn2d_backward", "dfa_cnn2d_forward_train", "cnn2d", kCnn2dGrads, "dlogits", false}, step, B, T, F, 0, x, x_dtype,
                         dlogits, grads, ngrads, workspace, workspace_bytes, [&] { return (pl = plan_train(B, T, F, prec)).total; }, no_late_checks));
  char* ws = (char*)workspace;
  float* partial = (float*)(ws + pl.partial);
  const LayerParams l2 = layer_params(m.p, 1), l3 = layer_params(m.p, 2);
  const LayerGrads g2 = layer_grads(grads, 1), g3 = layer_grads(grads, 2);
  const HeadGrads gh = head_grads(grads, kCnn2dLayers, 0);
  hipStream_t s = ctx->stream;
  DropCfg dc = step.drop;
  BnStats s2 = stat_ptrs(ws, pl, 1), s3 = stat_ptrs(ws, pl, 2);
  float *sm2 = sums_ptr(ws, pl, 1), *sm3 = sums_ptr(ws, pl, 2);
  float* demb = (float*)(ws + pl.demb);
  const dfa::BnSync* sync = step.synced ? &ctx->bn_sync : nullptr;           // synchronised BatchNorm (dfa_ctx_set_bn_sync)
  // classifier
  DFA_HIP_CHECK(ctx, launch_linear_bwd(dlogits, head_params(m.p, kCnn2dLayers, 0).w, (const float*)(ws + pl.emb), demb, gh.dw, gh.db, B, 128 * F, s, 128, F));
  // block 3: BN backward (upstream = mean_T then Linear), weight gradient, data gradient
  DFA_HIP_CHECK(ctx, launch_bn_bwd_meant_saved(prec, ws + pl.z3, bn_apply(s3, l3), demb, (const float*)(ws + pl.msum), partial,
                                               sm3, ws + pl.dz3, B, pl.H2, F, 128, s, sync));
  DFA_HIP_CHECK(ctx, launch_split_sums(sm3, g3.dgamma, g3.dbeta, 128, s));
  DFA_HIP_CHECK(ctx, launch_wgrad3x3(prec, 64, 128, ws + pl.dz3, ws + pl.a2, partial, g3.dw, g3.db, B, pl.H2, F, kWgradWGs, s, ctx->wgrad_variant));
  DFA_HIP_CHECK(ctx, launch_dgrad3(step.dgrad_m16, prec, conv_args(ws + pl.dz3, tr.d3, ws + pl.da2, B, pl.H2, F, 64, ctx), (float*)(ws + pl.raw), s, ctx->train_conv_variant));
  // block 2
  dc.layer = 2;
  {
    int ppb_;
    float* scratch2 = partial + (size_t)bn_bwd_blocks(B, pl.H1, F, &ppb_) * 64 * 2;
    DFA_HIP_CHECK(ctx, launch_bn_bwd(prec, SRC_POOL, ws + pl.z2, bn_apply(s2, l2), ws + pl.da2, partial, sm2, ws + pl.dz2,
                                     B, pl.H1, F, 64, dc, s, scratch2, sync));
  }
  DFA_HIP_CHECK(ctx, launch_split_sums(sm2, g2.dgamma, g2.dbeta, 64, s));
  DFA_HIP_CHECK(ctx, launch_wgrad3x3(prec, 32, 64, ws + pl.dz2, ws + pl.a1, partial, g2.dw, g2.db, B, pl.H1, F, kWgradWGs, s, ctx->wgrad_variant));
  {
    ConvArgs a = conv_args(ws + pl.dz2, tr.d2, ws + pl.da1, B, pl.H1, F, 32, ctx);
    if (step.c1_mfma) { a.drop = dc; a.drop.layer = 1; }   // keep mask of a1's dropout where da1 is produced (idempotent for the vector kernel)
    DFA_HIP_CHECK(ctx, launch_dgrad2(step.dgrad_m16, prec, a, s, ctx->train_conv_variant));
  }
  // block 1 (z1 recomputed from x; conv1_mfma may be cleared between forward and backward: the vector kernel reads the same state)
  dc.layer = 1;
  return conv1_train_backward(ctx, conv1_block(m, step, FeatView{x, x_dtype, stride_b, stride_t, stride_f, B, T, F}, ws, pl, dc),
                              step.c1_mfma && ctx->conv1_mfma, step.c1_fused, sync, layer_grads(grads, 0));
}

// shared by the CNN2D and CNN1D entry points: validate, copy the keep mask into the context's double buffer, fill `armed`
static int arm_train_augment(dfa_ctx* ctx, AugCfg& armed, int enable, int T, int F, int shift, const float* keep_f, int tmask_start,
                             int tmask_len, int fmask_start, int fmask_len, float jitter_std, uint64_t seed, uint64_t offset) {
  armed = AugCfg{};
  if (!enable) return DFA_OK;
  if (T < 1 || F < 1) return fail(ctx, DFA_E_BAD_SHAPE, "bad augmentation shape [T=%d, F=%d]", T, F);
  if (tmask_len < 0 || fmask_len < 0 || tmask_start < 0 || fmask_start < 0 || tmask_start + tmask_len > T ||
      fmask_start + fmask_len > F)
    return fail(ctx, DFA_E_BAD_SHAPE, "mask span outside the batch");
  if (!(jitter_std >= 0.f)) return fail(ctx, DFA_E_BAD_SHAPE, "jitter std must be >= 0");
  // The keep mask is COPIED (stream-ordered) into one of two context-owned buffers, alternating per call: the caller's tensor may
  // be freed as soon as this returns (a temporary FusedAugment did exactly that in a test and the backward read recycled memory),
  // and arming batch n+1 cannot disturb the backward of batch n.
  const float* keep_dev = nullptr;
  if (keep_f) {
    DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->aug_keep_cap < F) {
      if (ctx->aug_keep) { DFA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); DFA_HIP_CHECK(ctx, hipFree(ctx->aug_keep)); ctx->aug_keep = nullptr; }
      const int cap = F < 1024 ? 1024 : F;
      DFA_HIP_CHECK(ctx, hipMalloc((void**)&ctx->aug_keep, (size_t)2 * cap * sizeof(float)));
      ctx->aug_keep_cap = cap;
    }
    ctx->aug_keep_slot ^= 1;
    float* dst = ctx->aug_keep + (size_t)ctx->aug_keep_slot * ctx->aug_keep_cap;
    DFA_HIP_CHECK(ctx, hipMemcpyAsync(dst, keep_f, (size_t)F * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    keep_dev = dst;
  }
  AugCfg a{};
  a.on = 1; a.T = T; a.F = F; a.shift = ((shift % T) + T) % T; a.keep = keep_dev;
  a.tm_start = tmask_start; a.tm_len = tmask_len; a.fm_start = fmask_start; a.fm_len = fmask_len;
  a.std = jitter_std; a.seed = seed; a.offset = offset;
  armed = a;
  return DFA_OK;
}

int dfa_cnn2d_set_train_augment(dfa_ctx* ctx, int enable, int T, int F, int shift, const float* keep_f, int tmask_start,
                                int tmask_len, int fmask_start, int fmask_len, float jitter_std, uint64_t seed,
                                uint64_t offset) {
  if (!ctx) return DFA_E_NULL_PTR;
  return arm_train_augment(ctx, ctx->cnn2d.train.aug_armed, enable, T, F, shift, keep_f, tmask_start, tmask_len, fmask_start, fmask_len,
                           jitter_std, seed, offset);
}

int dfa_cnn1d_set_train_augment(dfa_ctx* ctx, int enable, int T, int F, int shift, const float* keep_f, int tmask_start,
                                int tmask_len, int fmask_start, int fmask_len, float jitter_std, uint64_t seed,
                                uint64_t offset) {
  if (!ctx) return DFA_E_NULL_PTR;
  return arm_train_augment(ctx, ctx->cnn1d.train.aug_armed, enable, T, F, shift, keep_f, tmask_start, tmask_len, fmask_start, fmask_len,
                           jitter_std, seed, offset);
}

int dfa_ctx_set_bn_sync(dfa_ctx* ctx, dfa_bn_sync_fn fn, void* user, int world, float* buf, int capacity) {
  if (!ctx) return DFA_E_NULL_PTR;
  ctx->bn_sync = dfa::BnSync{};
  if (!fn) return DFA_OK;
  if (world < 1) return fail(ctx, DFA_E_BAD_SHAPE, "world must be >= 1 (got %d)", world);
  if (!buf || capacity < 512) return fail(ctx, DFA_E_NULL_PTR, "the synchronisation buffer must hold at least 512 floats");
  ctx->bn_sync.fn = fn; ctx->bn_sync.user = user; ctx->bn_sync.world = world; ctx->bn_sync.buf = buf;
  return DFA_OK;
}

int dfa_bce_smooth_fwd_bwd(dfa_ctx* ctx, const float* logits, const float* labels, float label_smoothing, int B,
                           float* loss, float* dlogits) {
  if (!ctx) return DFA_E_NULL_PTR;
  if (!logits || !labels) return fail(ctx, DFA_E_NULL_PTR, "logits and labels must be non-null");
  if (!(label_smoothing >= 0.f && label_smoothing < 0.5f))
    return fail(ctx, DFA_E_BAD_SHAPE, "--label-smoothing must be in [0, 0.5)");   /* src/train.py:308-309 */
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "B must be >= 1");
  DFA_HIP_CHECK(ctx, launch_bce_smooth(logits, labels, label_smoothing, B, loss, dlogits, ctx->stream));
  return DFA_OK;
}

int dfa_adamw_step(dfa_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale) {
  TraceRange trace_("dfa_adamw_step");
  if (!ctx) return DFA_E_NULL_PTR;
  if (!param || !grad || !exp_avg || !exp_avg_sq) return fail(ctx, DFA_E_NULL_PTR, "adamw buffers must be non-null");
  if (step < 1) return fail(ctx, DFA_E_BAD_SHAPE, "step is 1-based (got %d)", step);
  if (n == 0) return DFA_OK;
  DFA_HIP_CHECK(ctx, launch_adamw(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, ctx->stream));
  return DFA_OK;
}

}  // extern "C"

// train_host.h -- what the training steps of the C ABI share on the host (train_api.hip, cnn1d_train_api.hip, cae_train_api.hip,
// dlq_train_api.hip): the bump that carves plans and allocations, the BatchNorm accessors and finalize, the ConvArgs / DropCfg fills,
// the data-gradient images and launches, the block-1 passes of the CNN2D and the auto-encoder.  Features, a layer's parameters and
// gradients, running statistics and BatchNorm terms travel as the views of launch_views.h; what a backward must know about its
// forward is the model's TrainStep (train_step.h), matched by check_backward (dfa_checks.h).  Host only; int-returning helpers go
// in DFA_TRY.
#pragma once
#include "dfa_checks.h"

namespace dfa {

constexpr int kWgradWGs = 256;     // workgroups of a 3x3 weight-gradient launch (the plans size its partials)

// take(bytes) = offset of the next 256-byte aligned region, take.off = their total: the workspace plans and the train_packed allocations
struct Bump {
  size_t off = 0;
  size_t operator()(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
};

// mean | var | invstd of one BatchNorm layer inside a model's statistics block ([3 C] per layer, layers in the model's order),
// and the layer's (S1, S2) record inside its sums block; ch_off = the channels of the layers before it
inline BnStats bn_stats(void* stats_block, int ch_off, int C) {
  float* b = (float*)stats_block + 3 * ch_off;
  return {b, b + C, b + 2 * C};
}
inline float* bn_sums(void* sums_block, int ch_off) { return (float*)sums_block + 2 * ch_off; }

// BatchNorm batch statistics from the per-workgroup records partial[nparts][C][2].  Synchronised BatchNorm (dfa_ctx_set_bn_sync):
// the records are first reduced to one [C][2] record in the caller's buffer (scratch: a second reduction level), summed over the
// ranks by the caller's hook, and the statistics come from those sums and the global count: every rank ends with the same ones.
// shift: the records are sums of z - shift[c * shift_stride]; never given under synchronised BatchNorm.
inline int finalize_bn_stats(dfa_ctx* ctx, const float* partial, int nparts, int C, double n, const BnStats& st, const RunningStats& run,
                             float momentum, float* scratch = nullptr, const float* shift = nullptr, int shift_stride = 0) {
  const BnSync& sy = ctx->bn_sync;
  hipStream_t s = ctx->stream;
  if (!sy.fn) {
    DFA_HIP_CHECK(ctx, launch_bn_finalize(partial, nparts, C, n, st.mean, st.var, st.invstd, run.mean, run.var, momentum, s, shift, shift_stride));
    return DFA_OK;
  }
  DFA_HIP_CHECK(ctx, launch_reduce_partials(partial, nparts, C * 2, 1.0f, sy.buf, s, scratch));
  if (sy.fn(sy.user, sy.buf, C * 2) != 0) return fail(ctx, DFA_E_HIP, "the BatchNorm synchronisation hook failed (forward statistics, %d channels)", C);
  DFA_HIP_CHECK(ctx, launch_bn_finalize(sy.buf, 1, C, n * (double)sy.world, st.mean, st.var, st.invstd, run.mean, run.var, momentum, s));
  return DFA_OK;
}

inline DropCfg drop_cfg(float p_drop, uint64_t seed, uint64_t offset) {
  DropCfg dc{};
  dc.thresh = (p_drop > 0.f) ? (unsigned)((double)p_drop * 4294967296.0) : 0u;
  dc.scale = 1.0f / (1.0f - p_drop);
  dc.seed = seed; dc.offset = offset;
  return dc;
}

// a plain 3x3 convolution launch (no ReLU); the caller adds stats_partial / drop where it wants them
inline ConvArgs conv_args(const void* in, const PackedConv& w, void* out, int B, int H, int W, int COUT, const dfa_ctx* ctx) {
  ConvArgs a{};
  a.in = in; a.wpack = w.wpack; a.bias = w.bias; a.out = out;
  a.B = B; a.H = H; a.W = W; a.COUT = COUT; a.relu = 0; a.zero_page = ctx->zero_page;
  return a;
}

// data-gradient images of the 32 -> 64 (w2) and 64 -> 128 (w3) convolutions: m16 = the 16x16x32 order of conv_split.hip, else the
// 32x32x16 order with the second as two 64-output-channel halves (see launch_train_dgrad3)
inline int pack_dgrad_images(dfa_ctx* ctx, const float* w2, const float* w3, int prec, int m16, const PackedConv& d2, const PackedConv& d3) {
  hipStream_t s = ctx->stream;
  if (m16) {
    DFA_HIP_CHECK(ctx, launch_pack_conv3x3_dgrad_m16(w2, 32, 64, d2.wpack, d2.bias, s));
    DFA_HIP_CHECK(ctx, launch_pack_conv3x3_dgrad_m16(w3, 64, 128, d3.wpack, d3.bias, s));
    return DFA_OK;
  }
  const int nkg = (prec == DFA_PREC_BF16) ? 4 : 8;
  DFA_HIP_CHECK(ctx, launch_pack_conv3x3_dgrad(w2, 32, 64, 0, 64, prec, d2.wpack, d2.bias, s));
  for (int hlf = 0; hlf < 2; ++hlf)
    DFA_HIP_CHECK(ctx, launch_pack_conv3x3_dgrad(w3, 64, 128, 64 * hlf, 64, prec, d3.wpack + (size_t)hlf * (64 / 32) * 9 * nkg * 64, d3.bias, s));
  return DFA_OK;
}
// variant = the context's train_conv_variant (0: the compiler-scheduled twins)
inline hipError_t launch_dgrad2(int m16, int prec, const ConvArgs& a, hipStream_t s, int variant) {
  return m16 ? launch_train_dgrad2_m16(a, s, variant != 0) : launch_train_dgrad2(prec, a, s);
}
inline hipError_t launch_dgrad3(int m16, int prec, const ConvArgs& a, float* raw_tmp, hipStream_t s, int variant) {
  return m16 ? launch_train_dgrad3_m16(a, s, variant != 0) : launch_train_dgrad3(prec, a, raw_tmp, s, variant);
}

// ---- block 1 of the CNN2D and the auto-encoder: conv 1 -> 32 whose pre-BN output is recomputed from x in every pass -------------
struct Conv1Train {
  FeatView v;
  int prec;
  int poolw;                 // width of the pool behind the block: 1 (CNN2D, AvgPool (2, 1)) or 2 (auto-encoder, 2 x 2)
  DropCfg drop;
  const AugCfg* aug;
  LayerParams p;             // the block's layer
  float *fw, *fb;            // the weights folded with this batch's statistics (the forward's image; the matrix-core backward's ReLU mask)
  float* partial;            // per-workgroup records
  bool stats_scratch;        // synchronised statistics: reduce the records in two levels, the second behind them
  float* xxs;                // XX[9][9] | Xs[9]: left by the statistics pass for the one-pass backwards
  float* c1rec;              // the backward's reduced record ([32][11] one-pass, [32][10] two-pass)
  float* sums;               // the layer's (S1, S2)
  BnStats stats;
  const void* da;            // upstream gradient at the pooled activation
};

// statistics pass (mfma: on the matrix cores; xx: also the tap moments XX / Xs), batch statistics, fold into fw / fb
inline int conv1_train_stats(dfa_ctx* ctx, const Conv1Train& c, bool mfma, bool xx, bool update_running, float momentum) {
  hipStream_t s = ctx->stream;
  const FeatView& v = c.v;
  const int nb = mfma ? conv1_mfma_blocks(v.B, v.T, v.F) : conv1_train_blocks(v.B, v.T, v.F);
  if (mfma)
    DFA_HIP_CHECK(ctx, launch_conv1_mfma(C1X_STATS, v, c.p.w, c.p.b, nullptr, nullptr, c.partial, c.drop, 1, s));
  else
    DFA_HIP_CHECK(ctx, launch_conv1_train(xx ? C1M_STATS_XX : C1M_STATS, v, c.p.w, c.p.b, BnApply{}, nullptr, nullptr, c.prec, c.partial, c.drop,
                                          1, c.aug, 1.0f, s));
  DFA_TRY(finalize_bn_stats(ctx, c.partial, nb, 32, (double)v.B * v.T * v.F, c.stats, running_stats(c.p, update_running), momentum,
                            c.stats_scratch ? c.partial + (size_t)nb * 352 : nullptr));
  if (xx)   // block records of 96 floats behind the [32][2] records
    DFA_HIP_CHECK(ctx, launch_reduce_partials(c.partial + (size_t)nb * 64, nb, 96, 1.0f, c.xxs, s, c.partial + (size_t)nb * 160));
  DFA_HIP_CHECK(ctx, launch_fold_conv1({c.p.w, c.p.b, c.p.gamma, c.p.beta, c.stats.mean, c.stats.var}, c.fw, c.fb, 32, s));   // batch statistics
  return DFA_OK;
}

// backward into the block's gradients g.  mfma / fused: one pass over da (matrix cores / vector ALU) + the moment algebra of
// train_conv1.hip; else a reduce pass, the synchronisation of (S1, S2) where armed, and the weight-gradient pass
inline int conv1_train_backward(dfa_ctx* ctx, const Conv1Train& c, bool mfma, bool fused, const BnSync* sync, const LayerGrads& g) {
  hipStream_t s = ctx->stream;
  const FeatView& v = c.v;
  const LayerParams& p = c.p;
  const BnApply bn = bn_apply(c.stats, p);
  const double n = (double)v.B * v.T * v.F;
  const int nb1 = conv1_train_blocks(v.B, v.T, v.F);
  if (mfma || fused) {
    const int nb = mfma ? conv1_mfma_blocks(v.B, v.T, v.F) : nb1;
    if (mfma)   // the ReLU mask comes from the forward's own folded image; S2 is derived in the finalize
      DFA_HIP_CHECK(ctx, launch_conv1_mfma(C1X_BWD, v, c.fw, c.fb, nullptr, c.da, c.partial, c.drop, c.poolw, s));
    else
      DFA_HIP_CHECK(ctx, launch_conv1_train(C1M_BWD_FUSED, v, p.w, p.b, bn, nullptr, c.da, c.prec, c.partial, c.drop, c.poolw, c.aug, 1.0f, s));
    DFA_HIP_CHECK(ctx, launch_reduce_partials(c.partial, nb, 352, 1.0f, c.c1rec, s, c.partial + (size_t)nb * 352));
    DFA_HIP_CHECK(ctx, launch_conv1_bwd_finalize(c.c1rec, c.xxs, p, bn, n, g, s, mfma ? 1 : 0));
    return DFA_OK;
  }
  float* scratch = c.partial + (size_t)nb1 * 320;
  DFA_HIP_CHECK(ctx, launch_conv1_train(C1M_BWD_REDUCE, v, p.w, p.b, bn, nullptr, c.da, c.prec, c.partial, c.drop, c.poolw, c.aug, 1.0f, s));
  DFA_HIP_CHECK(ctx, launch_reduce_partials(c.partial, nb1, 64, 1.0f, c.sums, s, scratch));
  DFA_HIP_CHECK(ctx, launch_split_sums(c.sums, g.dgamma, g.dbeta, 32, s));      // this rank's own sums
  const float* sums_a;
  float isc;
  DFA_HIP_CHECK(ctx, bn_sync_sums(sync, c.sums, 64, s, &sums_a, &isc));         // dz1 is formed from the global ones
  DFA_HIP_CHECK(ctx, launch_conv1_train(C1M_WGRAD, v, p.w, p.b, bn, sums_a, c.da, c.prec, c.partial, c.drop, c.poolw, c.aug, isc, s));
  DFA_HIP_CHECK(ctx, launch_reduce_partials(c.partial, nb1, 320, 1.0f, c.c1rec, s, scratch));
  DFA_HIP_CHECK(ctx, launch_split_c1(c.c1rec, g.dw, g.db, s));
  return DFA_OK;
}

}  // namespace dfa

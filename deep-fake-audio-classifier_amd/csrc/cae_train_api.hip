// cae_train_api.hip -- C ABI of the ConvAutoencoder training step (replaces, for src/train_cae.py:58-82, torch autograd
// over src/model_cae.py:32-125):  dfa_cae_forward_train (BatchNorm with batch statistics, running-stat update, keeps
// what backward needs in the workspace) and dfa_cae_backward (gradients of the 30 parameters from d(loss)/d(recon)).
#include "train_host.h"
#include "trace.h"
#include "convt2x2_mfma.h"

using namespace dfa;

namespace {

constexpr int kGemmSplit = 64;
const int kEC[4] = {32, 64, 128, 256};     // encoder block output channels
const int kDC[3] = {128, 64, 32};          // decoder block 1-3 output channels
const int kDCin[3] = {256, 128, 64};

struct CaeTrainPlan {
  int H[5], W[5], Hd[4], Wd[4];
  bool ok;
  size_t e[4], z[4], zd[3], d[3], dd[3], dzd[3], de[4], dz[4], zp, xf, raw, stats, sums, wq, dwq, rec, partial, partial_bytes, total;
};

CaeTrainPlan plan_cae_train(int B, int T, int F, int prec) {
  CaeTrainPlan p;
  const size_t es = (prec == DFA_PREC_BF16) ? 2 : 4;
  p.H[0] = T; p.W[0] = F;
  for (int l = 1; l <= 4; ++l) { p.H[l] = p.H[l - 1] / 2; p.W[l] = p.W[l - 1] / 2; }
  p.Hd[0] = 2 * p.H[4]; p.Wd[0] = 2 * p.W[4];
  p.Hd[1] = 2 * p.Hd[0]; p.Wd[1] = 2 * p.Wd[0] + 1;
  p.Hd[2] = 2 * p.Hd[1]; p.Wd[2] = 2 * p.Wd[1];
  p.Hd[3] = 2 * p.Hd[2]; p.Wd[3] = 2 * p.Wd[2];
  p.ok = (p.H[4] >= 1 && p.W[4] >= 1 && p.Wd[3] == F);
  Bump take;
  for (int l = 0; l < 4; ++l) p.e[l] = take((size_t)B * p.H[l + 1] * p.W[l + 1] * kEC[l] * es);
  p.z[0] = 0;  // block 1's pre-BN output is recomputed, never stored
  for (int l = 1; l < 4; ++l) p.z[l] = take((size_t)B * p.H[l] * p.W[l] * kEC[l] * es);
  for (int l = 0; l < 3; ++l) p.zd[l] = take((size_t)B * p.Hd[l] * p.Wd[l] * kDC[l] * es);
  for (int l = 0; l < 3; ++l) p.d[l] = take((size_t)B * p.Hd[l] * p.Wd[l] * kDC[l] * es);
  for (int l = 0; l < 3; ++l) p.dd[l] = take((size_t)B * p.Hd[l] * p.Wd[l] * kDC[l] * es);
  for (int l = 0; l < 3; ++l) p.dzd[l] = take((size_t)B * p.Hd[l] * p.Wd[l] * kDC[l] * es);
  for (int l = 0; l < 4; ++l) p.de[l] = take((size_t)B * p.H[l + 1] * p.W[l + 1] * kEC[l] * es);
  p.dz[0] = 0;
  for (int l = 1; l < 4; ++l) p.dz[l] = take((size_t)B * p.H[l] * p.W[l] * kEC[l] * es);
  size_t zp = 0, xf = 0;
  for (int l = 0; l < 3; ++l) {
    const size_t P = (size_t)B * (p.Hd[l] / 2) * (l == 1 ? (p.Wd[l] - 1) / 2 : p.Wd[l] / 2);
    zp = std::max(zp, P * 4 * kDC[l] * es);
    xf = std::max(xf, P * kDCin[l] * 4);
  }
  p.zp = take(zp);
  p.xf = take(xf);
  size_t raw = (size_t)B * p.H[3] * p.W[3] * 256 * 4;                    // enc4 forward split
  raw = std::max(raw, (size_t)B * p.H[2] * p.W[2] * 64 * 4);             // dgrad3
  p.raw = take(raw);
  p.stats = take(704 * 3 * 4);
  p.sums = take(704 * 2 * 4 + 1024 * 4);
  p.wq = take((size_t)256 * 512 * 4);
  p.dwq = take((size_t)256 * 512 * 4);
  p.rec = take(1024 * 4);
  size_t pb = (size_t)kWgradWGs * ((size_t)128 * 64 * 9 + 256) * 4;
  pb = std::max(pb, (size_t)kGemmSplit * 256 * 512 * 4);
  pb = std::max(pb, ((size_t)conv1_train_blocks(B, T, F) + 64) * 352 * 4);   // [32][11] records + the second reduction level (as train_api.hip)
  int ppb;
  pb = std::max(pb, (size_t)cl_stats_blocks((size_t)B * T * F, &ppb) * 256 * 2 * 4);
  pb = std::max(pb, (size_t)cae_dec4_bwd_blocks() * 132 * 4);
  // channel-sum records of the decoder's folded BatchNorm-backward apply pass (cae_bwd_fold): one [C] record per 16 * (256 / (C / 8)) pixels
  for (int l = 0; l < 3; ++l) {
    const size_t npix = (size_t)B * p.Hd[l] * p.Wd[l], ppb2 = 16 * (256 / (kDC[l] / 8));
    pb = std::max(pb, 2 * ((npix + ppb2 - 1) / ppb2 + 64) * kDC[l] * 4);
  }
  // statistics records of the convolution epilogues (cae_conv_stats): the lower half holds the records, the upper half the second
  // reduction level of the synchronised form
  for (int l = 1; l < 4; ++l) pb = std::max(pb, 2 * ((size_t)B * ((p.W[l] + 31) / 32) + 64) * kEC[l] * 2 * 4);
  for (int l = 0; l < 3; ++l) {
    const long P = (long)B * (p.Hd[l] / 2) * (l == 1 ? (p.Wd[l] - 1) / 2 : p.Wd[l] / 2);
    pb = std::max(pb, 2 * ((size_t)cae_dec_stats_records(prec, kDCin[l], P) + 64) * kDC[l] * 2 * 4);
  }
  p.partial = take(pb);
  p.partial_bytes = pb;
  p.total = take.off;
  return p;
}

// BN layer order in the stats / sums blocks: enc1..enc4 (32, 64, 128, 256), dec1..dec3 (128, 64, 32)
const int kBnOff[7] = {0, 32, 96, 224, 480, 608, 672};
BnStats stat_of(char* ws, const CaeTrainPlan& pl, int layer, int C) { return bn_stats(ws + pl.stats, kBnOff[layer], C); }
float* sums_of(char* ws, const CaeTrainPlan& pl, int layer) { return bn_sums(ws + pl.sums, kBnOff[layer]); }

// statistics of a stored pre-BN output in a pass of their own
int finalize_stats(dfa_ctx* ctx, int prec, const void* z, size_t npix, int C, const BnStats& st, float* partial, const RunningStats& run,
                   float momentum) {
  int ppb;
  const int nblk = cl_stats_blocks(npix, &ppb);
  DFA_HIP_CHECK(ctx, launch_cl_stats(prec, z, partial, npix, C, ctx->stream));
  return finalize_bn_stats(ctx, partial, nblk, C, (double)npix, st, run, momentum);
}

// encoder block 1 of a step: what conv1_train_stats (forward) and conv1_train_backward (backward, da = de[0]) take.  The matrix-core
// passes keep XX | Xs and their [32][11] record behind the decoder-block-4 record in pl.rec; the two-pass record is pl.rec itself
Conv1Train conv1_block(const CaeState& m, const TrainStep& step, const FeatView& v, char* ws, const CaeTrainPlan& pl, bool mfma) {
  float* rec = (float*)(ws + pl.rec);
  Conv1Train c{};             // (no dropout, no augmentation, single-level synchronised statistics)
  c.v = v; c.prec = step.prec; c.poolw = 2;
  c.p = layer_params(m.p, 0); c.fw = m.train.tw1; c.fb = m.train.tb1; c.partial = (float*)(ws + pl.partial); c.xxs = rec + 512; c.c1rec = mfma ? rec + 640 : rec;
  c.sums = sums_of(ws, pl, 0); c.stats = stat_of(ws, pl, 0, 32); c.da = ws + pl.de[0];
  return c;
}

// the plan of a step, or the refusal of its precision or shape (what dfa_cae_forward_train and dfa_cae_train_plan both answer)
int checked_plan(dfa_ctx* ctx, int B, int T, int F, int precision, CaeTrainPlan* pl) {
  if (precision != DFA_PREC_F32 && precision != DFA_PREC_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "unknown precision %d", precision);
  if (B < 1 || T < 16) return fail(ctx, DFA_E_BAD_SHAPE, "need B >= 1 and T >= 16 (got %d, %d)", B, T);
  *pl = plan_cae_train(B, T, F, precision);
  if (!pl->ok) return fail(ctx, DFA_E_BAD_SHAPE, "F=%d: decoder would rebuild %d columns (needs F = 16*(F/16)+4)", F, pl->Wd[3]);
  return DFA_OK;
}

}  // namespace

extern "C" {

int dfa_cae_train_plan(dfa_ctx* ctx, int B, int T, int F, int precision, long long* fields, int cap) {
  CaeTrainPlan pl;
  DFA_TRY(checked_plan(ctx, B, T, F, precision, &pl));
  long long v[DFA_CAE_TRAIN_PLAN_FIELDS];
  int n = 0;
  auto put = [&](long long x) { v[n++] = x; };
  for (int l = 0; l < 5; ++l) put(pl.H[l]);
  for (int l = 0; l < 5; ++l) put(pl.W[l]);
  for (int l = 0; l < 4; ++l) put(pl.Hd[l]);
  for (int l = 0; l < 4; ++l) put(pl.Wd[l]);
  for (int l = 0; l < 4; ++l) put((long long)pl.e[l]);
  for (int l = 0; l < 4; ++l) put(l ? (long long)pl.z[l] : -1);      // block 1's pre-BN output is never stored
  for (int l = 0; l < 3; ++l) put((long long)pl.zd[l]);
  for (int l = 0; l < 3; ++l) put((long long)pl.d[l]);
  for (int l = 0; l < 3; ++l) put((long long)pl.dd[l]);
  for (int l = 0; l < 3; ++l) put((long long)pl.dzd[l]);
  for (int l = 0; l < 4; ++l) put((long long)pl.de[l]);
  for (int l = 0; l < 4; ++l) put(l ? (long long)pl.dz[l] : -1);
  for (size_t off : {pl.zp, pl.xf, pl.raw, pl.stats, pl.sums, pl.wq, pl.dwq, pl.rec, pl.partial, pl.partial_bytes, pl.total}) put((long long)off);
  put(precision == DFA_PREC_BF16 ? 2 : 4);
  for (int l = 0; l < 7; ++l) put(l < 4 ? kEC[l] : kDC[l - 4]);
  for (int k = 0; k < 3; ++k)       // mean, biased variance, inverse standard deviation: where bn_stats puts them
    for (int l = 0; l < 7; ++l) {
      const int C = l < 4 ? kEC[l] : kDC[l - 4];
      put((long long)(pl.stats + ((size_t)3 * kBnOff[l] + (size_t)k * C) * sizeof(float)));
    }
  static_assert(DFA_CAE_TRAIN_PLAN_FIELDS == 18 + 28 + 11 + 1 + 7 + 21, "field table of dfa_cae_train_plan");
  for (int i = 0; fields && i < cap && i < DFA_CAE_TRAIN_PLAN_FIELDS; ++i) fields[i] = v[i];
  return DFA_CAE_TRAIN_PLAN_FIELDS;
}

size_t dfa_cae_train_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F, int precision) {
  (void)ctx;
  if (B < 1 || T < 16 || F < 16) return 0;
  const CaeTrainPlan pl = plan_cae_train(B, T, F, precision);
  return pl.ok ? pl.total : 0;
}

int dfa_cae_forward_train(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                          int64_t stride_f, int precision, float momentum, int update_running_stats, float* recon,
                          float* latent, float* mse, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_cae_forward_train");
  if (!ctx) return DFA_E_NULL_PTR;
  CaeState& m = ctx->cae;
  CaeTrain& tr = m.train;
  tr.step.live = false;     // whatever this call returns, the batch that was in flight is over
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cae_set_params has not been called");
  if (!x || !workspace) return fail(ctx, DFA_E_NULL_PTR, "x and workspace must be non-null");
  if (!recon && !mse) return fail(ctx, DFA_E_NULL_PTR, "give recon, mse or both (the decoder's last kernel needs an output)");
  if (x_dtype != DFA_DTYPE_F32 && x_dtype != DFA_DTYPE_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "x dtype %d not supported", x_dtype);
  CaeTrainPlan pl;
  DFA_TRY(checked_plan(ctx, B, T, F, precision, &pl));
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total, false, "train "));
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int prec = precision;
  if (!tr.train_packed) {  // raw conv images enc2-4 (+ their dgrad images), raw convT images, conv1 fold target, biases
    Bump take;
    size_t eb[3], db[3], ew[3], dgw[3], dw[3];
    const size_t c1 = take((288 + 32) * 4);
    for (int l = 0; l < 3; ++l) eb[l] = take(kEC[l + 1] * 4);
    for (int l = 0; l < 3; ++l) db[l] = take(kDC[l] * 4);
    const size_t dgb = take(256 * 4);
    for (int l = 0; l < 3; ++l) ew[l] = take((size_t)kEC[l + 1] * kEC[l] * 9 * 4);
    for (int l = 0; l < 3; ++l) dgw[l] = take((size_t)kEC[l + 1] * kEC[l] * 9 * 4);
    for (int l = 0; l < 3; ++l) dw[l] = take((size_t)kDC[l] * kDCin[l] * 4 * 4);
    DFA_HIP_CHECK(ctx, hipMalloc(&tr.train_packed, take.off));
    char* b = (char*)tr.train_packed;
    tr.tw1 = (float*)(b + c1); tr.tb1 = tr.tw1 + 288;
    for (int l = 0; l < 3; ++l) {
      tr.tenc[l].bias = (float*)(b + eb[l]); tr.tenc[l].wpack = (uint4*)(b + ew[l]);
      tr.tdg[l].bias = (float*)(b + dgb); tr.tdg[l].wpack = (uint4*)(b + dgw[l]);
      tr.tdec[l].bias = (float*)(b + db[l]); tr.tdec[l].wpack = (uint4*)(b + dw[l]);
    }
  }
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T, F};
  const LayerParams e2 = layer_params(m.p, 1), e3 = layer_params(m.p, 2), e4 = layer_params(m.p, 3);
  hipStream_t s = ctx->stream;
  char* ws = (char*)workspace;
  float* partial = (float*)(ws + pl.partial);
  const int nkg = (prec == DFA_PREC_BF16) ? 4 : 8;
  // ---- weight images (weights move every step)
  DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(raw_conv(e2), 32, 0, 32, 64, prec, tr.tenc[0].wpack, tr.tenc[0].bias, s));
  DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(raw_conv(e3), 64, 0, 64, 128, prec, tr.tenc[1].wpack, tr.tenc[1].bias, s));
  TrainStep step;             // this call's record: committed to tr.step by the last statement
  step.B = B; step.T = T; step.F = F; step.prec = prec; step.x_dtype = x_dtype; step.synced = ctx->bn_sync.fn != nullptr;
  step.enc4_wide = (prec == DFA_PREC_BF16 && ctx->cae_enc4_wide) ? 1 : 0;
  if (step.enc4_wide) {   // one 128-input-channel image (the eval forward's layout)
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(raw_conv(e4), 128, 0, 128, 256, prec, tr.tenc[2].wpack, tr.tenc[2].bias, s));
  } else {
  for (int hlf = 0; hlf < 2; ++hlf)
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(raw_conv(e4), 128, 64 * hlf, 64, 256, prec,
                                                tr.tenc[2].wpack + (size_t)hlf * (256 / 32) * 9 * nkg * 64, tr.tenc[2].bias, s));
  }
  // bf16 mode: the 64 -> 32 and 128 -> 64 data gradients on the 16x16x32 kernels of conv_split.hip, one launch each (as the CNN2D's;
  // the 32x32x16 forms ran the first with one channel slice per workgroup -- 0.31 ms -- and the second as two launches chained
  // through fp32 partial sums)
  step.dgrad_m16 = (prec == DFA_PREC_BF16 && ctx->dgrad_m16) ? 1 : 0;
  DFA_TRY(pack_dgrad_images(ctx, e2.w, e3.w, prec, step.dgrad_m16, tr.tdg[0], tr.tdg[1]));
  if (step.enc4_wide) {
    for (int c = 0; c < 2; ++c)
      DFA_HIP_CHECK(ctx, launch_pack_conv3x3_dgrad(e4.w, 128, 256, 128 * c, 128, prec, tr.tdg[2].wpack + (size_t)c * (128 / 32) * 9 * 8 * 64, tr.tdg[2].bias, s));
  } else {
  for (int c = 0; c < 4; ++c)
    DFA_HIP_CHECK(ctx, launch_pack_conv3x3_dgrad(e4.w, 128, 256, 64 * c, 64, prec, tr.tdg[2].wpack + (size_t)c * (128 / 32) * 9 * nkg * 64, tr.tdg[2].bias, s));
  }
  for (int l = 0; l < 3; ++l)
    DFA_HIP_CHECK(ctx, launch_fold_pack_convt2x2(raw_conv(layer_params(m.p, kCaeDec0 + l)), kDCin[l], kDC[l], prec, tr.tdec[l].wpack, tr.tdec[l].bias, s));
  const bool upd = update_running_stats != 0;
  // ---- encoder block 1 (pre-BN output recomputed from x: statistics pass, fold, fused eval kernel)
  {
    // bf16 mode on bf16 features (F even): the statistics pass (with the 9 x 9 tap moments the fused backward algebra needs) and
    // the backward pass on the matrix cores (train_conv1_mfma.hip, as the CNN2D's block 1), the forward on cae_enc1_mfma.hip
    // (synchronised BatchNorm: the backward needs the layer's sums before the weight gradient is formed -> the two-pass vector path)
    step.c1_mfma = (ctx->conv1_mfma && !step.synced && prec == DFA_PREC_BF16 && x_dtype == DFA_DTYPE_BF16 && F <= 224 && !(F & 1) && T >= 4) ? 1 : 0;
    DFA_TRY(conv1_train_stats(ctx, conv1_block(m, step, v, ws, pl, step.c1_mfma), step.c1_mfma, step.c1_mfma, upd, momentum));
    if (step.c1_mfma && ctx->cae_enc1_mfma) {
      uint4* tpack = (uint4*)(ws + pl.wq);                // this step's three-term A operands (pl.wq is free until the decoder's backward)
      float* tbias = (float*)(ws + pl.wq) + 6 * 64 * 4;
      DFA_HIP_CHECK(ctx, launch_pack_cae_enc1_mfma(tr.tw1, tr.tb1, tpack, tbias, s));
      DFA_HIP_CHECK(ctx, launch_cae_enc1_mfma(v, nullptr, nullptr, tpack, tbias, ws + pl.e[0], s));
    } else {
      DFA_HIP_CHECK(ctx, launch_cae_enc1(v, nullptr, nullptr, tr.tw1, tr.tb1, ws + pl.e[0], prec, s));
    }
  }
  // ---- encoder blocks 2-4
  for (int l = 1; l < 4; ++l) {
    const LayerParams q = layer_params(m.p, l);
    ConvArgs a = conv_args(ws + pl.e[l - 1], tr.tenc[l - 1], ws + pl.z[l], B, pl.H[l], pl.W[l], kEC[l], ctx);
    const bool epi_stats = ctx->cae_conv_stats && l < 3;         // (block 4: conv3x3_inst_cae_train.hip)
    a.stats_partial = epi_stats ? partial : nullptr;             // one [COUT][2] record per (sample, 32-column strip)
    DFA_HIP_CHECK(ctx, launch_cae_train_fwd(prec, kEC[l - 1], a, (float*)(ws + pl.raw), s, step.enc4_wide, ctx->train_conv_variant));
    BnStats st = stat_of(ws, pl, l, kEC[l]);
    const size_t npix = (size_t)B * pl.H[l] * pl.W[l];
    const RunningStats run = running_stats(q, upd);
    int rc = epi_stats ? finalize_bn_stats(ctx, partial, B * ((pl.W[l] + 31) / 32), kEC[l], (double)npix, st, run, momentum)
                                 : finalize_stats(ctx, prec, ws + pl.z[l], npix, kEC[l], st, partial, run, momentum);
    if (rc != DFA_OK) return rc;
    DFA_HIP_CHECK(ctx, launch_bn_relu_pool(prec, 2, ws + pl.z[l], bn_apply(st, q), ws + pl.e[l], B, pl.H[l], pl.W[l], kEC[l], s));
  }
  if (latent) DFA_HIP_CHECK(ctx, launch_cae_latent_export(ws + pl.e[3], prec, latent, B, pl.H[4] * pl.W[4], 256, s));
  // ---- decoder blocks 1-3: raw ConvTranspose2d -> statistics -> BN + ReLU
  for (int l = 0; l < 3; ++l) {
    const LayerParams q = layer_params(m.p, kCaeDec0 + l);
    ConvTArgs a{};
    a.in = (l == 0) ? ws + pl.e[3] : ws + pl.d[l - 1];
    a.wpack = tr.tdec[l].wpack; a.bias = tr.tdec[l].bias; a.out = ws + pl.zd[l];
    a.B = B; a.H = pl.Hd[l] / 2; a.W = (l == 1) ? (pl.Wd[l] - 1) / 2 : pl.Wd[l] / 2;
    a.COUT = kDC[l]; a.opad_w = (l == 1) ? 1 : 0; a.no_relu = 1;
    a.stats_partial = ctx->cae_conv_stats ? partial : nullptr;   // one [COUT][2] record per workgroup (the padding column's share in record 0)
    DFA_HIP_CHECK(ctx, launch_cae_dec(prec, kDCin[l], a, s));
    if (l == 1) DFA_HIP_CHECK(ctx, launch_cae_opad_col(ws + pl.zd[1], tr.tdec[1].bias, prec, B * pl.Hd[1], pl.Wd[1], 64, s, 1));
    BnStats st = stat_of(ws, pl, kCaeDec0 + l, kDC[l]);
    const size_t npix = (size_t)B * pl.Hd[l] * pl.Wd[l];
    const RunningStats run = running_stats(q, upd);
    int rc = ctx->cae_conv_stats ? finalize_bn_stats(ctx, partial, cae_dec_stats_records(prec, kDCin[l], (long)B * a.H * a.W), kDC[l], (double)npix, st,
                                                    run, momentum, partial + pl.partial_bytes / 8)
                                 : finalize_stats(ctx, prec, ws + pl.zd[l], npix, kDC[l], st, partial, run, momentum);
    if (rc != DFA_OK) return rc;
    DFA_HIP_CHECK(ctx, launch_bn_relu_pool(prec, 1, ws + pl.zd[l], bn_apply(st, q), ws + pl.d[l], B, pl.Hd[l], pl.Wd[l], kDC[l], s));
  }
  // ---- decoder block 4 + zero time padding (+ per-sample MSE)
  DFA_HIP_CHECK(ctx, launch_cae_dec4_mse(ws + pl.d[2], prec, head_params(m.p, kCaeLayers, 0), v, nullptr, nullptr, recon, partial, mse, pl.Hd[2],
                                         pl.Wd[2], s));
  step.live = true;
  tr.step = step;
  return DFA_OK;
}

int dfa_cae_backward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                     int64_t stride_f, const float* drecon, float* const* grads, int ngrads, void* workspace,
                     size_t workspace_bytes) {
  TraceRange trace_("dfa_cae_backward");
  if (!ctx) return DFA_E_NULL_PTR;
  const CaeState& m = ctx->cae;
  const CaeTrain& tr = m.train;
  const TrainStep& step = tr.step;
  const int prec = step.prec;
  CaeTrainPlan pl;
  DFA_TRY(check_backward(ctx, {"dfa_cae_backward", "dfa_cae_forward_train", "the auto-encoder", kCaeGrads, nullptr, false}, step, B, T, F, 0, x, x_dtype,
                         drecon, grads, ngrads, workspace, workspace_bytes, [&] { return (pl = plan_cae_train(B, T, F, prec)).total; }, no_late_checks));
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T, F};
  const HeadParams head = head_params(m.p, kCaeLayers, 0);
  const HeadGrads gh = head_grads(grads, kCaeLayers, 0);
  hipStream_t s = ctx->stream;
  char* ws = (char*)workspace;
  float* partial = (float*)(ws + pl.partial);
  float* rec = (float*)(ws + pl.rec);
  float* scratch_c = (float*)(ws + pl.sums) + 2 * 704;   // 1024 floats of scratch behind the sums block
  // second-level scratch of the block-record reductions (64 x C x 2 floats): the upper half of the partial buffer -- the records
  // of the BatchNorm / statistics passes (<= 3600 x 512 floats) use a fraction of the lower half (sized for the weight gradients)
  float* scratch2 = partial + pl.partial_bytes / 8;
  const dfa::BnSync* sync = step.synced ? &ctx->bn_sync : nullptr;           // synchronised BatchNorm (dfa_ctx_set_bn_sync)
  const int bf = (prec == DFA_PREC_BF16) ? 1 : 0;
  DropCfg nodrop{};
  // ---- decoder block 4
  // drecon == NULL: the loss is MSELoss(recon, x) (src/train_cae.py:67-68) and its gradient 2 (recon - x) / (B T F) is formed inside
  // the kernel from the saved d3 and x -- neither recon nor drecon has to exist in memory
  MseArgs ma{v, head.b};
  DFA_HIP_CHECK(ctx, launch_cae_dec4_bwd(prec, ws + pl.d[2], head.w, drecon, ws + pl.dd[2], partial, B, pl.Hd[2], pl.Wd[2], T, F, s, drecon ? nullptr : &ma));
  DFA_HIP_CHECK(ctx, launch_reduce_partials(partial, cae_dec4_bwd_blocks(), 132, 1.0f, rec, s, nullptr));
  DFA_HIP_CHECK(ctx, hipMemcpyAsync(gh.dw, rec, 128 * 4, hipMemcpyDeviceToDevice, s));
  DFA_HIP_CHECK(ctx, hipMemcpyAsync(gh.db, rec + 128, 4, hipMemcpyDeviceToDevice, s));
  // ---- decoder blocks 3, 2, 1
  for (int l = 2; l >= 0; --l) {
    const LayerParams q = layer_params(m.p, kCaeDec0 + l);
    const LayerGrads g = layer_grads(grads, kCaeDec0 + l);
    const int Hin = pl.Hd[l] / 2, Win = (l == 1) ? (pl.Wd[l] - 1) / 2 : pl.Wd[l] / 2;
    const int Cin = kDCin[l], Cout = kDC[l];
    const long P = (long)B * Hin * Win;
    BnStats st = stat_of(ws, pl, kCaeDec0 + l, Cout);
    float* sm = sums_of(ws, pl, kCaeDec0 + l);
    const BnApply bn = bn_apply(st, q);
    if (ctx->cae_bwd_fold) {
      // one apply pass writes dz patch-major (what the two gradient GEMMs read) and leaves the records of its channel sums = the
      // ConvTranspose2d bias gradient (over ALL output pixels, the output_padding column included): dzd itself is never stored
      dfa::BnBwdFold fold{ws + pl.zp, Win, partial, 0};
      DFA_HIP_CHECK(ctx, launch_bn_bwd(prec, SRC_DIRECT, ws + pl.zd[l], bn, ws + pl.dd[l], partial, sm, nullptr, B, pl.Hd[l], pl.Wd[l],
                                       Cout, nodrop, s, scratch2, sync, &fold));
      DFA_HIP_CHECK(ctx, launch_split_sums(sm, g.dgamma, g.dbeta, Cout, s));
      DFA_HIP_CHECK(ctx, launch_reduce_partials(partial, fold.nrec, Cout, 1.0f, g.db, s, scratch2));
    } else {
    DFA_HIP_CHECK(ctx, launch_bn_bwd(prec, SRC_DIRECT, ws + pl.zd[l], bn, ws + pl.dd[l], partial, sm, ws + pl.dzd[l], B, pl.Hd[l],
                                     pl.Wd[l], Cout, nodrop, s, scratch2, sync));
    DFA_HIP_CHECK(ctx, launch_split_sums(sm, g.dgamma, g.dbeta, Cout, s));
    {  // ConvTranspose2d bias gradient = channel sums of dz over ALL output pixels (the output_padding column included)
      int ppb;
      const size_t npix = (size_t)B * pl.Hd[l] * pl.Wd[l];
      const int nblk = cl_stats_blocks(npix, &ppb);
      DFA_HIP_CHECK(ctx, launch_cl_stats(prec, ws + pl.dzd[l], partial, npix, Cout, s));
      DFA_HIP_CHECK(ctx, launch_reduce_partials(partial, nblk, Cout * 2, 1.0f, scratch_c, s, scratch2));
      DFA_HIP_CHECK(ctx, launch_split_sums(scratch_c, scratch_c + 512, g.db, Cout, s));
    }
    DFA_HIP_CHECK(ctx, launch_pixel_unshuffle(prec, ws + pl.dzd[l], ws + pl.zp, B, Hin, Win, pl.Wd[l], Cout, s));
    }
    float* wq = (float*)(ws + pl.wq);
    DFA_HIP_CHECK(ctx, launch_convt_w_to_q(q.w, wq, Cin, Cout, s));
    // data gradient: dX[P x Cin] = Zp[P x 4Cout] . Wq^T
    float* xf = (float*)(ws + pl.xf);
    void* dx = (l == 0) ? ws + pl.de[3] : ws + pl.dd[l - 1];
    if (bf && ctx->cae_dgrad_mfma && convt_dgrad_bf16_supports(Cin, Cout)) {   // bf16 matrix cores, bf16 result in place
      // the bf16 weight fragments (Cin * 4 Cout * 2 bytes, at most half of pl.dwq) go to pl.dwq, which is free until this layer's
      // weight gradient below.  (pl.xf holds P * Cin floats: on a small batch the fragments would run past it, over raw, the
      // BatchNorm statistics and the head of wq, which the pack kernel is still reading.)
      DFA_HIP_CHECK(ctx, launch_convt_dgrad_bf16(ws + pl.zp, wq, ws + pl.dwq, dx, P, Cin, Cout, s));
    } else {
      DFA_HIP_CHECK(ctx, launch_gemm_f32(bf, ws + pl.zp, 4 * Cout, 1, 0, wq, 1, 4 * Cout, xf, (int)P, Cin, 4 * Cout, 1, s));
      DFA_HIP_CHECK(ctx, launch_cast_from_f32(prec, xf, dx, (size_t)P * Cin, s));
    }
    // weight gradient: dWq[Cin x 4Cout] = X^T . Zp   (K = P, split over workgroups)
    const void* xin = (l == 0) ? ws + pl.e[3] : ws + pl.d[l - 1];
    float* dwq = (float*)(ws + pl.dwq);
    int nparts = kGemmSplit;
    if (bf) {   // bf16 mode: transposed-read bf16 MFMA GEMM (gemm_tn_bf16.hip)
      DFA_HIP_CHECK(ctx, launch_gemm_tn_bf16(xin, ws + pl.zp, partial, pl.partial_bytes / sizeof(float), Cin, 4 * Cout, (int)P, &nparts, s));
    } else {
      DFA_HIP_CHECK(ctx, launch_gemm_f32(bf, xin, 1, Cin, bf, ws + pl.zp, 4 * Cout, 1, partial, Cin, 4 * Cout, (int)P, kGemmSplit, s));
    }
    DFA_HIP_CHECK(ctx, launch_reduce_partials(partial, nparts, Cin * 4 * Cout, 1.0f, dwq, s, nullptr));
    DFA_HIP_CHECK(ctx, launch_convt_q_to_w(dwq, g.dw, Cin, Cout, s));
  }
  // ---- encoder blocks 4, 3, 2
  for (int l = 3; l >= 1; --l) {
    BnStats st = stat_of(ws, pl, l, kEC[l]);
    float* sm = sums_of(ws, pl, l);
    const LayerGrads g = layer_grads(grads, l);
    DFA_HIP_CHECK(ctx, launch_bn_bwd(prec, SRC_POOL22, ws + pl.z[l], bn_apply(st, layer_params(m.p, l)), ws + pl.de[l], partial, sm,
                                     ws + pl.dz[l], B, pl.H[l], pl.W[l], kEC[l], nodrop, s, scratch2, sync));
    DFA_HIP_CHECK(ctx, launch_split_sums(sm, g.dgamma, g.dbeta, kEC[l], s));
    if (l == 3) {
      for (int co = 0; co < 2; ++co)
        for (int ci = 0; ci < 2; ++ci)
          DFA_HIP_CHECK(ctx, launch_wgrad3x3_window(prec, 64, 128, 128, 256, 64 * ci, 128 * co, ws + pl.dz[3], ws + pl.e[2], partial, g.dw,
                                                    ci == 0 ? g.db : nullptr, B, pl.H[3], pl.W[3], kWgradWGs, s, ctx->wgrad_variant));
    } else {
      DFA_HIP_CHECK(ctx, launch_wgrad3x3(prec, kEC[l - 1], kEC[l], ws + pl.dz[l], ws + pl.e[l - 1], partial, g.dw, g.db, B,
                                         pl.H[l], pl.W[l], kWgradWGs, s, ctx->wgrad_variant));
    }
    const ConvArgs a = conv_args(ws + pl.dz[l], tr.tdg[l - 1], ws + pl.de[l - 1], B, pl.H[l], pl.W[l], kEC[l - 1], ctx);
    DFA_HIP_CHECK(ctx, (l == 3)   ? launch_cae_dgrad4(prec, a, (float*)(ws + pl.raw), s, step.enc4_wide)
                       : (l == 2) ? launch_dgrad3(step.dgrad_m16, prec, a, (float*)(ws + pl.raw), s, ctx->train_conv_variant)
                                  : launch_dgrad2(step.dgrad_m16, prec, a, s, ctx->train_conv_variant));
  }
  // ---- encoder block 1 (z1 recomputed from x; upstream through the 2x2 average pool): matrix-core pass + algebra, or two vector passes
  const bool c1_mfma = step.c1_mfma && ctx->conv1_mfma;
  return conv1_train_backward(ctx, conv1_block(m, step, v, ws, pl, c1_mfma), c1_mfma, false, sync, layer_grads(grads, 0));
}

int dfa_mse_fwd_bwd(dfa_ctx* ctx, const float* recon, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                    int64_t stride_t, int64_t stride_f, float* loss, float* drecon) {
  TraceRange trace_("dfa_mse_fwd_bwd");
  if (!ctx) return DFA_E_NULL_PTR;
  if (!recon || !x) return fail(ctx, DFA_E_NULL_PTR, "recon and x must be non-null");
  if (!loss && !drecon) return fail(ctx, DFA_E_NULL_PTR, "give loss, drecon or both");
  if (x_dtype != DFA_DTYPE_F32 && x_dtype != DFA_DTYPE_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "x dtype %d not supported", x_dtype);
  if (B < 1 || T < 1 || F < 1) return fail(ctx, DFA_E_BAD_SHAPE, "need B, T, F >= 1 (got %d, %d, %d)", B, T, F);
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!ctx->mse_partial) DFA_HIP_CHECK(ctx, hipMalloc((void**)&ctx->mse_partial, kMseBlocks * sizeof(float)));
  DFA_HIP_CHECK(ctx, launch_mse_fwd_bwd(recon, FeatView{x, x_dtype, stride_b, stride_t, stride_f, B, T, F}, ctx->mse_partial, loss, drecon,
                                        ctx->stream));
  return DFA_OK;
}

}  // extern "C"

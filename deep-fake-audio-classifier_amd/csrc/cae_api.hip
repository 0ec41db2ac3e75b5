// cae_api.hip -- C ABI of the auto-encoder's eval forward and ragged scoring (include/dfa_hip.h; the reference's
// src/model_cae.py): parameter binding, weight preparation, the workspace plan, and the launches -- encoder block 1, encoder
// blocks 2-4 (conv3x3_inst_cae.hip), then the decoder + squared error as one kernel (cae_dec_fused.hip) or as four launches.
#include "dfa_checks.h"
#include "trace.h"
#include "convt2x2_mfma.h"

using namespace dfa;

namespace {

struct CaePlan {
  int H[5], W[5];        // H[0]=T, W[0]=F, then after each 2x2 pool
  int Hd[4], Wd[4];      // decoder outputs d1, d2, d3 and recon rows/cols
  size_t e_off[4], raw_off, d_off[3], part_off, total;
  int nblk;
  bool ok;
};

CaePlan plan_cae(int B, int T, int F, int prec) {
  CaePlan p;
  const size_t es = (prec == DFA_PREC_BF16) ? 2 : 4;
  p.H[0] = T; p.W[0] = F;
  for (int l = 1; l <= 4; ++l) { p.H[l] = p.H[l - 1] / 2; p.W[l] = p.W[l - 1] / 2; }
  p.Hd[0] = 2 * p.H[4]; p.Wd[0] = 2 * p.W[4];
  p.Hd[1] = 2 * p.Hd[0]; p.Wd[1] = 2 * p.Wd[0] + 1;   // output_padding = (0, 1)
  p.Hd[2] = 2 * p.Hd[1]; p.Wd[2] = 2 * p.Wd[1];
  p.Hd[3] = 2 * p.Hd[2]; p.Wd[3] = 2 * p.Wd[2];
  p.ok = (p.H[4] >= 1 && p.W[4] >= 1 && p.Wd[3] == F);
  const int ch[4] = {32, 64, 128, 256};
  size_t off = 0;
  for (int l = 0; l < 4; ++l) { p.e_off[l] = off; off = align_up(off + (size_t)B * p.H[l + 1] * p.W[l + 1] * ch[l] * es, 256); }
  p.raw_off = off;
  if (prec == DFA_PREC_F32) off = align_up(off + (size_t)B * p.H[3] * p.W[3] * 256 * 4, 256);
  const int dch[3] = {128, 64, 32};
  for (int l = 0; l < 3; ++l) { p.d_off[l] = off; off = align_up(off + (size_t)B * p.Hd[l] * p.Wd[l] * dch[l] * es, 256); }
  p.nblk = cae_dec4_blocks(T, p.Wd[2]);
  p.part_off = off;
  off = align_up(off + (size_t)B * p.nblk * sizeof(float), 256);
  p.total = off;
  return p;
}

// the plan's activation regions in a caller's workspace: encoder outputs e1..e4, decoder outputs d1..d3
struct CaeBuffers { void* e[4]; void* d[3]; };
CaeBuffers cae_buffers(char* ws, const CaePlan& pl) {
  return {{ws + pl.e_off[0], ws + pl.e_off[1], ws + pl.e_off[2], ws + pl.e_off[3]}, {ws + pl.d_off[0], ws + pl.d_off[1], ws + pl.d_off[2]}};
}
// the arguments of encoder block l + 2 (l = 0, 1, 2): e[l] -> e[l + 1]
ConvArgs cae_enc_args(const dfa_ctx* ctx, const CaePlan& pl, const CaeBuffers& bf, int l, int B) {
  const CaeState& m = ctx->cae;
  const int ecout[3] = {64, 128, 256};
  ConvArgs a{};
  a.in = bf.e[l]; a.wpack = m.enc[l].wpack; a.bias = m.enc[l].bias; a.out = bf.e[l + 1];
  a.B = B; a.H = pl.H[l + 1]; a.W = pl.W[l + 1]; a.COUT = ecout[l]; a.relu = 1; a.zero_page = ctx->zero_page;
  return a;
}

// the checks dfa_cae_forward and dfa_cae_score_ragged make first, in this order (have_ptrs: no required pointer is null)
int cae_forward_front(dfa_ctx* ctx, bool ragged, bool have_ptrs, const float* mu, const float* sigma, int x_dtype, int B, int T) {
  if (ctx->cae.prepared_prec < 0) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cae_prepare has not been called since the last set_params");
  if (!have_ptrs) return fail(ctx, DFA_E_NULL_PTR, ragged ? "x, lengths, mse and workspace must be non-null" : "x and workspace must be non-null");
  if ((mu == nullptr) != (sigma == nullptr)) return fail(ctx, DFA_E_NULL_PTR, "mu and sigma must both be given or both be NULL");
  if (x_dtype != DFA_DTYPE_F32 && x_dtype != DFA_DTYPE_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "x dtype %d not supported", x_dtype);
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "batch must be >= 1 (got %d)", B);
  if (T < 16) return fail(ctx, DFA_E_BAD_SHAPE, "%s=%d is too short: four 2x2 average pools need T >= 16", ragged ? "T_max" : "T", T);
  return DFA_OK;
}
int cae_refuse_F(dfa_ctx* ctx, int F, const CaePlan& pl) {
  return fail(ctx, DFA_E_BAD_SHAPE, "F=%d: decoder would rebuild %d columns (needs F = 16*(F/16)+4, e.g. 180; src/model_cae.py:68-69)", F, pl.Wd[3]);
}

}  // namespace

size_t dfa::cae_workspace_bytes(int B, int T, int F, int prec) { return plan_cae(B, T, F, prec).total; }

extern "C" {

int dfa_cae_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int base_channels) {
  DFA_TRY(set_params_core(ctx, &dfa_ctx::cae, "cae", device_params, n, [&]() -> int {
    if (base_channels != 32) return fail(ctx, DFA_E_UNSUPPORTED, "cae HIP path is built for base_channels=32 (got %d)", base_channels);
    return DFA_OK;
  }));
  ctx->cae.prepared_prec = -1;
  return DFA_OK;
}

int dfa_cae_prepare(dfa_ctx* ctx, int precision) {
  if (!ctx) return DFA_E_NULL_PTR;
  CaeState& m = ctx->cae;
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cae_set_params has not been called");
  if (precision != DFA_PREC_F32 && precision != DFA_PREC_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "unknown precision %d", precision);
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int ecin[3] = {32, 64, 128}, ecout[3] = {64, 128, 256};
  const int dcin[3] = {256, 128, 64}, dcout[3] = {128, 64, 32};
  size_t off = align_up((288 + 32) * sizeof(float), 256);
  size_t eb[3], ew[3], db[3], dw[3];
  for (int l = 0; l < 3; ++l) { eb[l] = off; off = align_up(off + ecout[l] * 4, 256); }
  for (int l = 0; l < 3; ++l) { db[l] = off; off = align_up(off + dcout[l] * 4, 256); }
  for (int l = 0; l < 3; ++l) { ew[l] = off; off = align_up(off + (size_t)ecout[l] * ecin[l] * 9 * 4, 256); }
  for (int l = 0; l < 3; ++l) { dw[l] = off; off = align_up(off + (size_t)dcout[l] * dcin[l] * 4 * 4, 256); }
  const size_t cst_off = off;
  off = align_up(off + 16 * sizeof(float), 256);
  const size_t c1p_off = off;
  off = align_up(off + 6 * 64 * 16 + 256, 256);
  const size_t d4p_off = off;
  off = align_up(off + 4 * 64 * 16, 256);
  if (!m.packed) DFA_HIP_CHECK(ctx, hipMalloc(&m.packed, off));
  char* base = (char*)m.packed;
  m.w1 = (float*)base;
  m.b1 = m.w1 + 288;
  for (int l = 0; l < 3; ++l) {
    m.enc[l].bias = (float*)(base + eb[l]); m.enc[l].wpack = (uint4*)(base + ew[l]);
    m.dec[l].bias = (float*)(base + db[l]); m.dec[l].wpack = (uint4*)(base + dw[l]);
  }
  const HeadParams head = head_params(m.p, kCaeLayers, 0);
  hipStream_t s = ctx->stream;
  DFA_HIP_CHECK(ctx, launch_fold_conv1(layer_params(m.p, 0), m.w1, m.b1, 32, s));
  for (int l = 0; l < 2; ++l)
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(layer_params(m.p, l + 1), ecin[l], 0, ecin[l], ecout[l], precision, m.enc[l].wpack, m.enc[l].bias, s, 0.25f));
  const LayerParams e4 = layer_params(m.p, 3);
  if (precision == DFA_PREC_BF16) {
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(e4, 128, 0, 128, 256, precision, m.enc[2].wpack, m.enc[2].bias, s, 0.25f));
  } else {  // two Cin halves, see conv3x3_inst_cae.hip
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(e4, 128, 0, 64, 256, precision, m.enc[2].wpack, m.enc[2].bias, s, 0.25f));
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(e4, 128, 64, 64, 256, precision, m.enc[2].wpack + (size_t)(256 / 32) * 9 * 8 * 64, m.enc[2].bias, s, 0.25f));
  }
  for (int l = 0; l < 3; ++l)
    DFA_HIP_CHECK(ctx, launch_fold_pack_convt2x2(layer_params(m.p, kCaeDec0 + l), dcin[l], dcout[l], precision, m.dec[l].wpack, m.dec[l].bias, s));
  m.opad_cst = (float*)(base + cst_off);
  m.c1pack = (uint4*)(base + c1p_off);
  m.c1bias = (float*)(base + c1p_off + 6 * 64 * 16);
  DFA_HIP_CHECK(ctx, launch_pack_cae_enc1_mfma(m.w1, m.b1, m.c1pack, m.c1bias, s));
  m.dec4pack = (uint4*)(base + d4p_off);
  DFA_HIP_CHECK(ctx, launch_pack_cae_dec4(head.w, m.dec4pack, s));
  if (precision == DFA_PREC_BF16)   // the constants the fused decoder uses for the columns grown from block 2's output_padding column
    DFA_HIP_CHECK(ctx, launch_cae_opad_consts(m.dec[1].bias, m.dec[2].wpack, m.dec[2].bias, head.w, head.b, m.opad_cst, s));
  m.prepared_prec = precision;
  return DFA_OK;
}

int dfa_cae_forward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                    int64_t stride_f, const float* mu, const float* sigma, float* recon, float* latent, float* mse,
                    void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_cae_forward");
  if (!ctx) return DFA_E_NULL_PTR;
  CaeState& m = ctx->cae;
  DFA_TRY(cae_forward_front(ctx, false, x && workspace, mu, sigma, x_dtype, B, T));
  const int prec = m.prepared_prec;
  const CaePlan pl = plan_cae(B, T, F, prec);
  if (!pl.ok) return cae_refuse_F(ctx, F, pl);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total));
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T, F};
  const HeadParams head = head_params(m.p, kCaeLayers, 0);
  char* ws = (char*)workspace;
  const CaeBuffers bf = cae_buffers(ws, pl);
  void* const* e = bf.e;
  void* const* d = bf.d;
  hipStream_t s = ctx->stream;
  { ScopedSlot ts(ctx, 8);
    if (prec == DFA_PREC_BF16 && ctx->cae_enc1_mfma && F <= 1022)    // block 1 on the matrix cores (hi + lo bf16 operands)
      DFA_HIP_CHECK(ctx, launch_cae_enc1_mfma(v, mu, sigma, m.c1pack, m.c1bias, e[0], s));
    else
      DFA_HIP_CHECK(ctx, launch_cae_enc1(v, mu, sigma, m.w1, m.b1, e[0], prec, s)); }
  for (int l = 0; l < 3; ++l) {
    ScopedSlot ts(ctx, 9 + l);
    const ConvArgs a = cae_enc_args(ctx, pl, bf, l, B);
    const int dma = ctx->cae_enc_dma;
    hipError_t err = (l == 0) ? launch_cae_enc2(prec, a, s, ctx->lds_pipe, dma) : (l == 1) ? launch_cae_enc3(prec, a, s, ctx->lds_pipe, dma)
                                                                             : launch_cae_enc4(prec, a, (float*)(ws + pl.raw_off), s, dma, ctx->train_conv_variant);
    DFA_HIP_CHECK(ctx, err);
  }
  if (latent) DFA_HIP_CHECK(ctx, launch_cae_latent_export(e[3], prec, latent, B, pl.H[4] * pl.W[4], 256, s));
  if (prec == DFA_PREC_BF16 && ctx->cae_dec_fused && cae_dec_fused_supports(v)) {   // decoder + squared error in one kernel: d1, d2, d3 never leave the CU (slot 12)
    if (recon || mse) {
      ScopedSlot ts(ctx, 12);
      float* partial = (float*)(ws + pl.part_off);
      DFA_HIP_CHECK(ctx, launch_cae_dec_fused(e[3], m.dec, head, m.dec4pack, m.opad_cst, v, mu, sigma, recon, partial, pl.H[4], pl.W[4], s,
                                              ctx->clock_probe ? ctx->clock_buf : nullptr));
      if (mse) DFA_HIP_CHECK(ctx, launch_cae_mse_finalize(partial, cae_dec_fused_tiles(pl.H[4], pl.W[4]), 1.0f / ((float)T * (float)F), mse, B, s));
    }
    return DFA_OK;
  }
  const int dcin[3] = {256, 128, 64}, dcout[3] = {128, 64, 32};
  for (int l = 0; l < 3; ++l) {
    ScopedSlot ts(ctx, 12 + l);
    ConvTArgs a{};
    a.in = (l == 0) ? e[3] : d[l - 1];
    a.wpack = m.dec[l].wpack; a.bias = m.dec[l].bias; a.out = d[l];
    a.B = B; a.H = (l == 0) ? pl.H[4] : pl.Hd[l - 1]; a.W = (l == 0) ? pl.W[4] : pl.Wd[l - 1];
    a.COUT = dcout[l]; a.opad_w = (l == 1) ? 1 : 0;
    DFA_HIP_CHECK(ctx, launch_cae_dec(prec, dcin[l], a, s));
    if (l == 1) DFA_HIP_CHECK(ctx, launch_cae_opad_col(d[1], m.dec[1].bias, prec, B * pl.Hd[1], pl.Wd[1], 64, s));
  }
  if (recon || mse) {
    ScopedSlot ts(ctx, 15);
    DFA_HIP_CHECK(ctx, launch_cae_dec4_mse(d[2], prec, head, v, mu, sigma, recon, (float*)(ws + pl.part_off), mse, pl.Hd[2], pl.Wd[2], s));
  }
  return DFA_OK;
}

// Ragged auto-encoder scoring.  Workspace: the uniform plan at T_max with the table (4 * B words) behind it.  Table words
// [0, B) lengths, [B, 2B) dispatch order, [2B, 3B) 1 / (T_b F) as float bits, [3B, 4B) the utterance's decoder tile count.
// A planner of its own: dfa_ragged_workspace_bytes(DFA_MODEL_CAE) keeps its historical 0 (include/dfa_hip.h).
size_t dfa_cae_ragged_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int F, int precision) {
  (void)ctx;
  if (B < 1 || T_max < 1 || F < 1) return 0;
  return plan_cae(B, T_max, F, precision).total + align_up((size_t)4 * B * 4, 256);
}

int dfa_cae_score_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b, int64_t stride_t,
                         int64_t stride_f, const int32_t* lengths, const float* mu, const float* sigma, float* mse, void* workspace,
                         size_t workspace_bytes) {
  TraceRange trace_("dfa_cae_score_ragged");
  if (!ctx) return DFA_E_NULL_PTR;
  CaeState& m = ctx->cae;
  DFA_TRY(cae_forward_front(ctx, true, x && workspace && lengths && mse, mu, sigma, x_dtype, B, T_max));
  DFA_TRY(check_lengths(ctx, lengths, B, 16, T_max));
  const int prec = m.prepared_prec;
  if (prec != DFA_PREC_BF16)
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged auto-encoder score has kernels for precision bf16 only (prepared: %d)", prec);
  const CaePlan pl = plan_cae(B, T_max, F, prec);
  if (!pl.ok) return cae_refuse_F(ctx, F, pl);
  if (!ctx->cae_dec_fused || !ctx->cae_enc1_mfma || !ctx->cae_enc_dma || !ctx->lds_pipe)   // the uniform forward would run other kernels
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged auto-encoder score needs the default options cae_dec_fused=1, cae_enc1_mfma=1, "
                "cae_enc_dma=1 and lds_pipe=1");
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T_max, F};
  if (F > 1022 || !cae_dec_fused_supports(v))
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged auto-encoder score needs F <= 1022, non-negative strides and 32-bit element "
                "offsets inside an utterance (F=%d, stride_t=%lld, stride_f=%lld)", F, (long long)stride_t, (long long)stride_f);
  DFA_TRY(refuse_capture(ctx, "score"));
  const size_t tab_off = pl.total;
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total + align_up((size_t)4 * B * 4, 256)));
  char* ws = (char*)workspace;
  const int* dtab = (const int*)(ws + tab_off);
  hipStream_t s = ctx->stream;
  std::vector<int32_t> extra((size_t)2 * B);   // the model's half of the table
  for (int b = 0; b < B; ++b) {
    const float inv_n = 1.0f / ((float)lengths[b] * (float)F);     // as the uniform call forms it
    memcpy(&extra[b], &inv_n, 4);
    extra[B + b] = cae_dec_fused_tiles(lengths[b] / 16, pl.W[4]);
  }
  DFA_TRY(stage_ragged_lengths_extra(ctx, lengths, B, extra.data(), extra.size(), ws + tab_off));
  const RaggedTab rt{dtab, B};
  const CaeBuffers bf = cae_buffers(ws, pl);
  { ScopedSlot ts(ctx, 8);
    DFA_HIP_CHECK(ctx, launch_cae_enc1_mfma_ragged(v, mu, sigma, m.c1pack, m.c1bias, bf.e[0], dtab, s)); }
  for (int l = 0; l < 3; ++l) {
    ScopedSlot ts(ctx, 9 + l);
    DFA_HIP_CHECK(ctx, launch_cae_enc_ragged(l, cae_enc_args(ctx, pl, bf, l, B), rt, s));
  }
  {
    ScopedSlot ts(ctx, 12);
    float* partial = (float*)(ws + pl.part_off);
    DFA_HIP_CHECK(ctx, launch_cae_dec_fused_ragged(bf.e[3], m.dec, head_params(m.p, kCaeLayers, 0), m.dec4pack, m.opad_cst, v, mu, sigma, partial,
                                                   pl.H[4], pl.W[4], dtab, s));
    DFA_HIP_CHECK(ctx, launch_cae_mse_finalize_ragged(partial, cae_dec_fused_tiles(pl.H[4], pl.W[4]), dtab, mse, B, s));
  }
  return DFA_OK;
}

}  // extern "C"

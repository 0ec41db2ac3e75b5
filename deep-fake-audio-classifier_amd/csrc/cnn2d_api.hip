// cnn2d_api.hip -- C ABI of the CNN2D eval forward, uniform and ragged (include/dfa_hip.h; the reference's src/model.py:33-42):
// parameter binding, weight preparation, and the ONE plan every caller reads (cnn2d_forward_plan below; dfa_cnn2d_forward_plan
// reports it): which kernels a forward runs, how it segments the time axis, where things live in the workspace.  The paths:
//   conv123 (blocks 1-3 + time mean in one kernel, conv123_*.hip)                                            ->  linear
//           (conv123_cls.hip, where the phase form runs: the linear head inside that kernel, no launch behind it)
//   conv12 (blocks 1+2, conv12_fused.hip)  ->  block 3 (+BN+ReLU+mean_T)                   [->  emb_reduce]  ->  linear
//   conv1 (+BN+ReLU+pool)  ->  block 2 MFMA conv (+BN+ReLU+pool)  ->  block 3 MFMA conv    [->  emb_reduce]  ->  linear
#include <algorithm>

#include "dfa_checks.h"
#include "trace.h"

using namespace dfa;

namespace {

constexpr int kMaxSeg = 4;   // at most this many time segments per strip, and chunk slabs of block 3's time mean

// Small batches (B * strips below the chip's resident-workgroup count; the reference's predict.py default is batch 32): every
// workgroup would walk the whole time axis alone, so the axis is split into segments that separate workgroups walk (blocks 1+2:
// disjoint output rows; block 3: partial means per segment, added up by emb_reduce_kernel).  The resident-workgroup counts the
// automatic split fills, per kernel:
constexpr int kSlots = 512;         // conv12_fused and conv3_m16; also where blocks 1-3 fuse, and the planner's slab rule
constexpr int kSlotsSplit2 = 768;   // bf16x3 block 2 (conv_split.hip)
constexpr int kSlotsSplit3 = 256;   // bf16x3 block 3 (conv_split.hip)
// ... and the columns a workgroup's strip owns:
constexpr int kStripCols = c123::SW;   // 30: conv12_fused, conv3_m16, conv_split, conv123 -- the kernels that split
constexpr int kStripColsMfma = 32;     // conv3x3_mfma (never splits); the width the slab rule counts strips in

// iterations per time-axis segment for a kernel that walks `niter` iterations with `nwg` workgroups and `slots` resident
// workgroup slots on the chip: 0 = do not split.  A multiple of `period` (ring / window-buffer phase of the kernel).
int seg_iters_for(int niter, int nwg, int slots, int period, int forced) {
  if (forced == 0 || niter <= period) return 0;
  int seg;
  if (forced > 0) seg = (niter + forced - 1) / forced;
  else {
    if (nwg >= slots) return 0;
    seg = (int)(((long long)niter * nwg + slots - 1) / slots);
  }
  seg = (seg + period - 1) / period * period;
  if (seg >= niter) return 0;
  if ((niter + seg - 1) / seg > kMaxSeg) seg = ((niter + kMaxSeg - 1) / kMaxSeg + period - 1) / period * period;
  return seg >= niter ? 0 : seg;
}

// canonical chunk of block 3's time mean (iterations of 2 rows, a multiple of 6): depends on H2 only, <= kMaxSeg chunks
int chunk3_for(int niter3) { return 6 * std::max(2, (niter3 + 6 * kMaxSeg - 1) / (6 * kMaxSeg)); }

// the context options the plan reads (a null context: the defaults of dfa_ctx, so time_split = -1)
struct Cnn2dOptions { int time_split, fuse_conv1, block3_m16, fuse_blocks123, persist123, carry_a1, phase123; };
Cnn2dOptions options_of(const dfa_ctx& c) {
  return {c.time_split, c.fuse_conv1, c.block3_m16, c.fuse_blocks123, c.persist123, c.carry_a1, c.phase123};
}

struct Cnn2dForwardPlan {
  int H1, H2;                        // rows after pool 1 / pool 2
  size_t a1_off, a2_off, emb_off;    // workspace regions; the embedding region holds `slabs` slabs of B * 128 * F floats
  int slabs;                         // 1, or kMaxSeg + 1: slab 0 the reduced embedding, slabs 1.. one chunk of block 3's time mean each
  size_t tab_off, tab_words, total;  // ragged: the per-call table (RaggedTab, 4 * B words) behind the regions; total includes it
  int path;                          // DFA_CNN2D_PATH_*
  Conv123Plan p123;                  // DFA_CNN2D_PATH_CONV123: form, phase, grid and LDS bytes (conv123_plan); zeros otherwise
  int seg12;                         // iterations per segment of conv12 (of block 2 in bf16x3 mode), 0 = no split
  int seg3, chunk3, nseg3;           // block 3: iterations per segment (0 = no split), canonical chunk (0: the kernel has none), chunks in use
  bool split3;                       // ragged: block 3 runs one workgroup per chunk and writes the chunk slabs
};

// Uniform: B utterances of T frames.  Ragged: B utterances padded to T = T_max; the ragged forward has the conv12 + block 3
// kernels only (it refuses other precisions and options), its seg3 is the 0 / 1 switch its kernel takes, and chunk3 / nseg3 are
// those of an utterance of T_max frames (each utterance's own chunk is per-call data: the table).
Cnn2dForwardPlan cnn2d_forward_plan(int B, int T, int F, int prec, bool ragged, const Cnn2dOptions& o, int num_cus) {
  Cnn2dForwardPlan p{};
  const int ts = o.time_split;
  p.H1 = T / 2;
  p.H2 = p.H1 / 2;
  const int nwg = B * ((F + kStripCols - 1) / kStripCols);
  const int niter12 = (p.H1 + 3) / 4, niter3 = (p.H2 + 1) / 2;
  const int chunk3 = chunk3_for(niter3);   // canonical chunks: depend on T only (12 iterations = 24 rows for T = 321), <= kMaxSeg of them
  // The embedding region.  Split implies slabs: block 3 splits (seg3 != 0, or split3) only where time_split > 0 -- the first term
  // below -- or where time_split < 0 and B * ceil(F / kStripCols) < kSlots or kSlotsSplit3 (seg_iters_for answers 0 for nwg >=
  // slots and for time_split == 0); both counts are <= kSlots and ceil(F / 32) <= ceil(F / 30), so then B * ceil(F / 32) < kSlots:
  // the second term.  And never more than kMaxSeg chunks: chunk3_for(n) >= ceil(n / kMaxSeg).  (time_split == 0 never splits
  // but keeps the slabs of a small batch: the historical plan.)
  p.slabs = (ts > 0 || (size_t)B * ((F + kStripColsMfma - 1) / kStripColsMfma) < (size_t)kSlots) ? kMaxSeg + 1 : 1;
  if (ragged) {
    p.path = DFA_CNN2D_PATH_CONV12;
    p.seg12 = seg_iters_for(niter12, nwg, kSlots, 6, ts);   // segments of the longest utterance's trip count, the shorter ones leave their late ones
    p.split3 = p.slabs > 1 && ts != 0;                      // split as the uniform plan would, and whenever it could (its chunk slabs exist then)
    p.seg3 = p.split3 ? 1 : 0;
    p.chunk3 = chunk3;
    p.nseg3 = std::max(1, (niter3 + chunk3 - 1) / chunk3);
  } else {
    // bf16 mode: blocks 1 and 2 run as one kernel and a1 stays on chip; fp32 features are rounded to bf16 as the kernel loads
    // them (bf16 storage mode), exactly like a caller-side .to(bfloat16)
    const bool fused12 = prec == DFA_PREC_BF16 && o.fuse_conv1;
    const bool chunked3 = prec == DFA_PREC_BF16X3 || (prec == DFA_PREC_BF16 && o.block3_m16);   // conv_split / conv3_m16 (conv3x3_mfma: no chunks, no split)
    // Blocks 1-3 + time mean as ONE kernel wherever no kernel of the two-kernel path could split the time axis (no forced split,
    // B * strips >= kSlots -- also where a short T would not split: small batches keep the two-kernel path and its a2 in the
    // workspace): same chunked time mean, bit-identical logits and embeddings.  In the form conv123_plan chooses.
    const bool fused123 = fused12 && o.block3_m16 && o.fuse_blocks123 && ts <= 0 && nwg >= kSlots;
    p.path = fused123 ? DFA_CNN2D_PATH_CONV123 : fused12 ? DFA_CNN2D_PATH_CONV12 : DFA_CNN2D_PATH_CONV1;
    if (fused123) p.p123 = conv123_plan(B, T, F, num_cus, o.persist123, o.carry_a1, o.phase123);
    else if (fused12) p.seg12 = seg_iters_for(niter12, nwg, kSlots, 6, ts);
    else if (prec == DFA_PREC_BF16X3) p.seg12 = seg_iters_for((p.H1 + 1) / 2, nwg, kSlotsSplit2, 3, ts);
    if (chunked3) p.chunk3 = chunk3;
    if (chunked3 && !fused123) p.seg3 = seg_iters_for(niter3, nwg, prec == DFA_PREC_BF16X3 ? kSlotsSplit3 : kSlots, chunk3, ts);
    p.nseg3 = p.seg3 ? (niter3 + chunk3 - 1) / chunk3 : 1;   // one slab of (unscaled) sums per canonical chunk
  }
  const size_t es = (prec == DFA_PREC_BF16) ? 2 : 4;   // fp32, or a hi + lo bf16 pair (DFA_PREC_BF16X3)
  size_t off = 0;
  p.a1_off = off;
  off = align_up(off + (size_t)B * p.H1 * F * 32 * es, 256);
  p.a2_off = off;
  off = align_up(off + (size_t)B * p.H2 * F * 64 * es, 256);
  p.emb_off = off;
  off = align_up(off + (size_t)p.slabs * B * 128 * F * sizeof(float), 256);
  p.tab_off = off;
  p.tab_words = ragged ? (size_t)4 * B : 0;
  p.total = off + align_up(p.tab_words * 4, 256);
  return p;
}

Cnn2dForwardPlan plan_for(const dfa_ctx* ctx, int B, int T, int F, int prec, bool ragged) {
  return ctx ? cnn2d_forward_plan(B, T, F, prec, ragged, options_of(*ctx), ctx->num_cus)
             : cnn2d_forward_plan(B, T, F, prec, ragged, options_of(dfa_ctx{}), 0);
}

// the checks dfa_cnn2d_forward and dfa_cnn2d_forward_ragged make first, in this order (have_ptrs: no required pointer is null)
int cnn2d_forward_front(dfa_ctx* ctx, bool ragged, bool have_ptrs, int x_dtype, int B, int T, int F) {
  const Cnn2dState& m = ctx->cnn2d;
  if (m.prepared_prec < 0) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cnn2d_prepare has not been called since the last set_params");
  if (!have_ptrs) return fail(ctx, DFA_E_NULL_PTR, "x, %slogits and workspace must be non-null", ragged ? "lengths, " : "");
  if (x_dtype != DFA_DTYPE_F32 && x_dtype != DFA_DTYPE_BF16) return fail(ctx, DFA_E_BAD_DTYPE, "x dtype %d not supported", x_dtype);
  if (B < 1) return fail(ctx, DFA_E_BAD_SHAPE, "batch must be >= 1 (got %d)", B);
  if (F != m.in_features)
    return fail(ctx, DFA_E_BAD_SHAPE, "feature dim %d does not match in_features=%d of the classifier (src/model.py:31)", F, m.in_features);
  if (T < 4) return fail(ctx, DFA_E_BAD_SHAPE, "%s=%d is too short: two (2,1) average pools need T >= 4", ragged ? "T_max" : "T", T);
  return DFA_OK;
}
// ... and last: the workspace, and the embedding (emb_reduce_kernel / the block-3 epilogues store 16 bytes at a time)
int cnn2d_forward_buffers(dfa_ctx* ctx, const void* workspace, size_t workspace_bytes, size_t need, const float* embedding) {
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, need));
  if (embedding && ((uintptr_t)embedding & 15) != 0)
    return fail(ctx, DFA_E_BAD_SHAPE, "embedding must be 16-byte aligned (got %p)", (void*)embedding);
  return DFA_OK;
}

}  // namespace

size_t dfa::cnn2d_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F, int prec, bool ragged) {
  return plan_for(ctx, B, T, F, prec, ragged).total;
}

extern "C" {

int dfa_cnn2d_forward_plan(const dfa_ctx* ctx, int B, int T, int F, int precision, int ragged, const int* options, int num_cus,
                           long long* fields, int cap) {
  if (B < 1 || T < 1 || F < 1) return 0;
  const Cnn2dOptions o = ctx       ? options_of(*ctx)
                         : options ? Cnn2dOptions{options[0], options[1], options[2], options[3], options[4], options[5], options[6]}
                                   : options_of(dfa_ctx{});
  const Cnn2dForwardPlan p = cnn2d_forward_plan(B, T, F, precision, ragged != 0, o, ctx ? ctx->num_cus : num_cus);
  const long long v[DFA_CNN2D_PLAN_FIELDS] = {
      p.H1, p.H2, (long long)p.a1_off, (long long)p.a2_off, (long long)p.emb_off, p.slabs, (long long)p.tab_off, (long long)p.tab_words,
      (long long)p.total, p.path, p.p123.form, p.p123.phase, p.p123.grid, (long long)p.p123.lds, p.seg12, p.seg3, p.chunk3, p.nseg3,
      p.split3 ? 1 : 0};
  for (int i = 0; fields && i < cap && i < DFA_CNN2D_PLAN_FIELDS; ++i) fields[i] = v[i];
  return DFA_CNN2D_PLAN_FIELDS;
}

int dfa_cnn2d_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int in_features, int base_channels) {
  DFA_TRY(set_params_core(ctx, &dfa_ctx::cnn2d, "cnn2d", device_params, n, [&]() -> int {
    if (base_channels != 32) return fail(ctx, DFA_E_UNSUPPORTED, "cnn2d HIP path is built for base_channels=32 (got %d)", base_channels);
    if (in_features < 1) return fail(ctx, DFA_E_BAD_SHAPE, "in_features must be positive (got %d)", in_features);
    return DFA_OK;
  }));
  ctx->cnn2d.in_features = in_features;
  ctx->cnn2d.prepared_prec = -1;
  return DFA_OK;
}

int dfa_cnn2d_prepare(dfa_ctx* ctx, int precision) {
  if (!ctx) return DFA_E_NULL_PTR;
  Cnn2dState& m = ctx->cnn2d;
  if (!m.have_params) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_cnn2d_set_params has not been called");
  if (precision != DFA_PREC_F32 && precision != DFA_PREC_BF16 && precision != DFA_PREC_BF16X3)
    return fail(ctx, DFA_E_BAD_DTYPE, "unknown precision %d", precision);
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // one allocation: w1[288] b1[32] | bias2[64] bias3[128] | wpack2 | wpack3   (sized for fp32, the larger mode)
  const size_t w2_bytes = (size_t)64 * 32 * 9 * 4, w3_bytes = (size_t)128 * 64 * 9 * 4;
  const size_t m16_bytes = (size_t)128 * 64 * 9 * 2;   // block-3 image for the 16x16x32 kernel (bf16)
  const size_t c1_bytes = 4 * 64 * 16 + 256 + m16_bytes;   // block-1 MFMA operands + bias of the fused kernel
  const size_t need = align_up((288 + 32 + 64 + 128) * sizeof(float), 256) + w2_bytes + w3_bytes + c1_bytes;
  if (!m.packed) {
    DFA_HIP_CHECK(ctx, hipMalloc(&m.packed, need));
    m.packed_bytes = need;
  }
  char* base = (char*)m.packed;
  m.w1 = (float*)base;
  m.b1 = m.w1 + 288;
  m.c2.bias = m.b1 + 32;
  m.c3.bias = m.c2.bias + 64;
  char* wp = base + align_up((288 + 32 + 64 + 128) * sizeof(float), 256);
  m.c2.wpack = (uint4*)wp;
  m.c3.wpack = (uint4*)(wp + w2_bytes);
  m.c1pack = (uint4*)(wp + w2_bytes + w3_bytes);
  m.c1bias = (float*)(wp + w2_bytes + w3_bytes + 4 * 64 * 16);
  m.c3_m16 = (uint4*)(wp + w2_bytes + w3_bytes + 4 * 64 * 16 + 256);
  const LayerParams l1 = layer_params(m.p, 0), l2 = layer_params(m.p, 1), l3 = layer_params(m.p, 2);
  DFA_HIP_CHECK(ctx, launch_fold_conv1(l1, m.w1, m.b1, 32, ctx->stream));
  DFA_HIP_CHECK(ctx, launch_pack_conv1_mfma(m.w1, m.b1, m.c1pack, m.c1bias, ctx->stream));
  if (precision == DFA_PREC_BF16X3) {
    // hi/lo split images (conv_split.hip): the same byte counts as the fp32 images, so they live in the same regions
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3_split(l2, 32, 64, m.c2.wpack, m.c2.bias, 0.5f, ctx->stream));
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3_split(l3, 64, 128, m.c3.wpack, m.c3.bias, 1.0f, ctx->stream));
    m.prepared_prec = precision;
    return DFA_OK;
  }
  DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(l2, 32, 0, 32, 64, precision, m.c2.wpack, m.c2.bias, ctx->stream, 0.5f));
  DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3(l3, 64, 0, 64, 128, precision, m.c3.wpack, m.c3.bias, ctx->stream));
  if (precision == DFA_PREC_BF16)
    DFA_HIP_CHECK(ctx, launch_fold_pack_conv3x3_m16(l3, 64, 128, m.c3_m16, ctx->stream));
  m.prepared_prec = precision;
  return DFA_OK;
}

// Timing slots: 0 = conv1, 1 = conv12 / block 2, 2 = block 3 / conv123 (slot 1 then reports nothing), 3 = emb_reduce + linear.
int dfa_cnn2d_forward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                      int64_t stride_f, float* logits, float* embedding, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn2d_forward");
  if (!ctx) return DFA_E_NULL_PTR;
  Cnn2dState& m = ctx->cnn2d;
  ctx->last_conv123_cls = 0;     // (also where a check below refuses the call)
  DFA_TRY(cnn2d_forward_front(ctx, false, x && logits && workspace, x_dtype, B, T, F));
  const int prec = m.prepared_prec;
  const Cnn2dForwardPlan pl = plan_for(ctx, B, T, F, prec, false);
  DFA_TRY(cnn2d_forward_buffers(ctx, workspace, workspace_bytes, pl.total, embedding));
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T, F};
  const HeadParams head = head_params(m.p, kCnn2dLayers, 0);
  char* ws = (char*)workspace;
  void* a1 = ws + pl.a1_off;
  void* a2 = ws + pl.a2_off;
  float* emb = embedding ? embedding : (float*)(ws + pl.emb_off);
  hipStream_t s = ctx->stream;
  // (the de-phased build is the carry form with the roles' step edges moved apart: bit-identical results, the value reported stays CARRY)
  ctx->last_conv123_form = pl.p123.form;
  ctx->last_conv123_phase = pl.p123.phase;
  // The phase form with the classifier head inside (conv123_cls.hip): wherever the phase form runs, unless linear1_kernel would
  // take its scalar path (weights or embedding not 16-byte aligned), which the kernel does not reproduce.  Same plan, same
  // form and phase reported; the head runs in the kernel where that build has it (conv123_cls_in_kernel: the shipped one does).
  const bool cls123 = pl.path == DFA_CNN2D_PATH_CONV123 && pl.p123.phase && ctx->cls123 && (((uintptr_t)head.w | (uintptr_t)emb) & 15) == 0;
  bool head_done = false;
  if (pl.path == DFA_CNN2D_PATH_CONV123) {
    ScopedSlot ts(ctx, 2);
    Conv123Args a = c123_args(v, m.c1pack, m.c1bias, m.c2.wpack, m.c2.bias, m.c3_m16, m.c3.bias, emb, pl.chunk3,
                              ctx->clock_probe ? ctx->clock_buf : nullptr);
    if (cls123) { a.cls_w = head.w; a.cls_b = head.b; a.logits = logits; a.cls_K = 128 * F; }
    const auto launch = cls123 ? launch_conv123_cls : pl.p123.phase ? launch_conv123_phase : pl.p123.form == DFA_CONV123_CARRY ? launch_conv123_carry :
                        pl.p123.form == DFA_CONV123_PERSIST ? launch_conv123_persist : launch_conv123_fused;
    DFA_HIP_CHECK(ctx, launch(a, x_dtype, ctx->num_cus, s, ctx->lds_pipe));
    head_done = cls123 && conv123_cls_in_kernel();
    ctx->last_conv123_cls = head_done ? 1 : 0;
  } else if (pl.path == DFA_CNN2D_PATH_CONV12) {
    ScopedSlot ts(ctx, 1);
    DFA_HIP_CHECK(ctx, launch_conv12_fused(v, m.c1pack, m.c1bias, m.c2.wpack, m.c2.bias, a2, s, ctx->lds_pipe, pl.seg12));
  } else {
    { ScopedSlot ts(ctx, 0);
      DFA_HIP_CHECK(ctx, launch_conv1(v, m.w1, m.b1, a1, prec, s)); }
    ScopedSlot ts(ctx, 1);
    ConvArgs a{};
    a.in = a1; a.wpack = m.c2.wpack; a.bias = m.c2.bias; a.out = a2; a.emb = nullptr;
    a.B = B; a.H = pl.H1; a.W = F; a.COUT = 64; a.inv_h = 0.f; a.relu = 1; a.zero_page = ctx->zero_page;
    a.seg_iters = pl.seg12;
    if (prec == DFA_PREC_BF16X3) DFA_HIP_CHECK(ctx, launch_cnn2d_block2_split(a, s, ctx->lds_pipe));
    else DFA_HIP_CHECK(ctx, launch_cnn2d_block2(prec, a, s, ctx->conv_dma, ctx->lds_pipe));
  }
  if (pl.path != DFA_CNN2D_PATH_CONV123) {
    ScopedSlot ts(ctx, 2);
    ConvArgs a{};
    a.in = a2; a.wpack = m.c3.wpack; a.bias = m.c3.bias; a.out = nullptr; a.emb = emb;
    a.B = B; a.H = pl.H2; a.W = F; a.COUT = 128; a.inv_h = 1.0f / (float)pl.H2; a.relu = 1; a.zero_page = ctx->zero_page;
    a.chunk_iters = pl.chunk3;
    a.seg_iters = pl.seg3;
    if (pl.seg3) {               // one slab of (unscaled) sums per canonical chunk in the workspace; emb_reduce_kernel adds them
      a.emb_seg_stride = (size_t)B * 128 * F;
      a.emb = (float*)(ws + pl.emb_off) + a.emb_seg_stride;     // slab 0 of the region is the reduced embedding
    }
    if (prec == DFA_PREC_BF16X3) {
      DFA_HIP_CHECK(ctx, launch_cnn2d_block3_split(a, s, ctx->lds_pipe));
    } else if (prec == DFA_PREC_BF16 && ctx->block3_m16) {
      a.wpack = m.c3_m16;
      a.clock_stamps = ctx->clock_probe ? ctx->clock_buf : nullptr;
      DFA_HIP_CHECK(ctx, launch_cnn2d_block3_m16(a, s, ctx->lds_pipe));
    } else {
      DFA_HIP_CHECK(ctx, launch_cnn2d_block3(prec, a, s, ctx->conv_dma, ctx->lds_pipe));
    }
  }
  {
    ScopedSlot ts(ctx, 3);      // one record per forward, also where the head ran inside the blocks 1-3 kernel: then of 0 ms
    if (head_done) { ts.nothing_launched(); return DFA_OK; }
    if (pl.nseg3 > 1) {   // chunk slabs 1 .. nseg3 of the workspace region -> the embedding (slab 0 of the region, or the caller's buffer)
      const size_t n = (size_t)B * 128 * F;
      DFA_HIP_CHECK(ctx, launch_emb_reduce((const float*)(ws + pl.emb_off) + n, pl.nseg3, n, n, 1.0f / (float)pl.H2, emb, s));
    }
    DFA_HIP_CHECK(ctx, launch_linear(emb, head.w, head.b, logits, B, 128 * F, s));
  }
  return DFA_OK;
}

// Ragged batch: the uniform plan at T_max plus the ragged table (conv3x3_mfma.h: RaggedTab, 4 * B int32 words) behind it.
// Table words [0, B) lengths, [B, 2B) dispatch order, [2B, 3B) 1 / H2_b as float bits, [3B, 4B) the utterance's canonical chunk.
int dfa_cnn2d_forward_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b, int64_t stride_t,
                             int64_t stride_f, const int32_t* lengths, float* logits, float* embedding, void* workspace,
                             size_t workspace_bytes) {
  TraceRange trace_("dfa_cnn2d_forward_ragged");
  if (!ctx) return DFA_E_NULL_PTR;
  Cnn2dState& m = ctx->cnn2d;
  DFA_TRY(cnn2d_forward_front(ctx, true, x && logits && workspace && lengths, x_dtype, B, T_max, F));
  DFA_TRY(check_lengths(ctx, lengths, B, 4, T_max));
  const int prec = m.prepared_prec;
  if (prec != DFA_PREC_BF16)
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged forward has kernels for precision bf16 only (prepared: %d)", prec);
  if (!ctx->fuse_conv1 || !ctx->block3_m16)   // the uniform forward would run other kernels: no bit-identity promise there
    return fail(ctx, DFA_E_UNSUPPORTED, "the ragged forward needs the default options fuse_conv1=1 and block3_m16=1");
  DFA_TRY(refuse_capture(ctx, "forward"));
  const Cnn2dForwardPlan pl = plan_for(ctx, B, T_max, F, prec, true);
  DFA_TRY(cnn2d_forward_buffers(ctx, workspace, workspace_bytes, pl.total, embedding));
  const FeatView v{x, x_dtype, stride_b, stride_t, stride_f, B, T_max, F};
  const HeadParams head = head_params(m.p, kCnn2dLayers, 0);
  char* ws = (char*)workspace;
  const int* dtab = (const int*)(ws + pl.tab_off);
  hipStream_t s = ctx->stream;
  // the model's half of the table, and the most chunks any utterance of this batch has (per-call data, not dispatch)
  int nseg3 = 1;
  std::vector<int32_t> extra((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    const int h2 = lengths[b] / 4, niter3 = (h2 + 1) / 2, chunk = chunk3_for(niter3);
    const float inv_h = 1.0f / (float)h2;
    memcpy(&extra[b], &inv_h, 4);
    extra[B + b] = chunk;
    nseg3 = std::max(nseg3, (niter3 + chunk - 1) / chunk);
  }
  DFA_TRY(stage_ragged_lengths_extra(ctx, lengths, B, extra.data(), extra.size(), ws + pl.tab_off));
  const RaggedTab rt{dtab, B};
  void* a2 = ws + pl.a2_off;
  float* emb = embedding ? embedding : (float*)(ws + pl.emb_off);
  {   // blocks 1 + 2 (timing slot 1)
    ScopedSlot ts(ctx, 1);
    DFA_HIP_CHECK(ctx, launch_conv12_ragged(v, m.c1pack, m.c1bias, m.c2.wpack, m.c2.bias, a2, dtab, s, ctx->lds_pipe, pl.seg12));
  }
  {   // block 3 + time mean (slot 2): split = one workgroup per chunk
    ScopedSlot ts(ctx, 2);
    ConvArgs a{};
    a.in = a2; a.wpack = m.c3_m16; a.bias = m.c3.bias; a.out = nullptr; a.emb = emb;
    a.B = B; a.H = pl.H2; a.W = F; a.COUT = 128; a.relu = 1; a.zero_page = ctx->zero_page;
    a.chunk_iters = 1;                 // (the kernel takes each utterance's own chunk from the table)
    if (pl.split3) {
      a.seg_iters = pl.seg3;
      a.emb_seg_stride = (size_t)B * 128 * F;
      a.emb = (float*)(ws + pl.emb_off) + a.emb_seg_stride;
    }
    DFA_HIP_CHECK(ctx, launch_cnn2d_block3_m16_ragged(a, rt, nseg3, s, ctx->lds_pipe));
  }
  {
    ScopedSlot ts(ctx, 3);
    if (pl.split3) {
      const size_t n = (size_t)B * 128 * F;
      DFA_HIP_CHECK(ctx, launch_emb_reduce_ragged((const float*)(ws + pl.emb_off) + n, n, 128 * F, dtab, B, emb, s));
    }
    DFA_HIP_CHECK(ctx, launch_linear(emb, head.w, head.b, logits, B, 128 * F, s));
  }
  return DFA_OK;
}

}  // extern "C"

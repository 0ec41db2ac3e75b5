// dfa_internal.h -- context object and internal launch prototypes of libdfa_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/dfa_hip.h"
#include "conv3x3_mfma.h"
#include "conv123_host.h"
#include "launch_views.h"
#include "rng.h"
#include "train_step.h"

namespace dfa {

constexpr float kBnEps = 1e-5f;  // torch.nn.BatchNorm default (src/model.py:16)

// ---- kernel timing slots (HIP events on the context's stream) -----------------------------------
constexpr int kMaxSlots = 16;
constexpr int kEventsPerSlot = 256;

struct SlotTimer {
  std::vector<hipEvent_t> start, stop;
  std::vector<char> empty;   // 1 = the record stands for a stage that launched nothing: it counts, with zero duration (ScopedSlot::nothing_launched)
  int used = 0;
};

struct PackedConv {
  uint4* wpack = nullptr;  // [COUT/32][9][CIN/KG][64]
  float* bias = nullptr;   // [COUT]
};

// Every model's parameter array p is `layers` conv + BatchNorm layers of six pointers, then the head's (w, b) pairs; its gradient array
// four per layer, then the head's (launch_views.h: layer_params, layer_grads, head_params, head_grads -- the only indexing of either).
// CNN2D, CNN1D: three blocks + the linear head.  Auto-encoder: encoder blocks 1-4 = layers 0-3, decoder blocks 1-3 = layers 4-6, decoder
// block 4 (no BatchNorm) = the head.  DeepfakeDetector: three layers + head.0 and head.3
constexpr int kCnn2dLayers = 3, kCnn1dLayers = 3, kCaeLayers = 7, kCaeDec0 = 4, kDlqLayers = 3;
constexpr int kCnn2dGrads = n_grads(kCnn2dLayers, 1), kCnn1dGrads = n_grads(kCnn1dLayers, 1), kCaeGrads = n_grads(kCaeLayers, 1),
              kDlqGrads = n_grads(kDlqLayers, 2);
static_assert(DFA_CNN2D_NPARAMS == n_params(kCnn2dLayers, 1) && DFA_CNN1D_NPARAMS == n_params(kCnn1dLayers, 1) &&
              DFA_CAE_NPARAMS == n_params(kCaeLayers, 1) && DFA_DLQ_NPARAMS == n_params(kDlqLayers, 2), "parameter arrays: 6 per layer + the head");
static_assert(kCnn2dGrads == 14 && kCnn1dGrads == 14 && kCaeGrads == 30 && kDlqGrads == 16, "gradient arrays (dfa_hip.h): 4 per layer + the head");

// A model's slot in the context: the bound parameters, the eval part (folded images, dfa_<model>_prepare) and the train part (the
// per-step weight images of forward_train / backward and the step record, train_step.h).  release() frees the train part's allocations.
struct Cnn2dEval {
  int prepared_prec = -1;
  void* packed = nullptr;  // one device allocation holding everything below
  size_t packed_bytes = 0;
  float* w1 = nullptr;     // [32][9] folded
  float* b1 = nullptr;     // [32]
  uint4* c1pack = nullptr; // [4][64] bf16 hi/lo A operands of the fused block 1+2 kernel (conv12_fused.hip)
  float* c1bias = nullptr; // [32]
  uint4* c3_m16 = nullptr; // block 3 weights in the 16x16x32 operand order (conv3_m16.hip), bf16 mode only
  PackedConv c2, c3;
};
struct Cnn2dTrain {          // train_api.hip
  void* train_packed = nullptr;
  float *tw1 = nullptr, *tb1 = nullptr;   // conv1 folded with the current batch statistics
  PackedConv t2, t3, d2, d3;              // raw forward images and data-gradient images
  AugCfg aug_armed{};                     // dfa_cnn2d_set_train_augment: consumed by the next forward_train
  TrainStep step;
  void release() { if (train_packed) (void)hipFree(train_packed); train_packed = nullptr; }
};
struct Cnn2dState : Cnn2dEval {
  const float* p[DFA_CNN2D_NPARAMS] = {nullptr};
  bool have_params = false;
  int in_features = 0;
  Cnn2dTrain train;
};

// Synchronised BatchNorm for data-parallel training ("SyncBN via two small all-reduces per layer -- makes
// N GPUs x B equal to one GPU x N*B up to summation order"): between a layer's statistics reduction and its use the library copies
// the per-channel sums into `buf` and calls fn(user, buf, count) on the host thread; the callee enqueues an in-place SUM all-reduce
// of buf[0 .. count) ordered after the work already on the context's stream (torch.distributed does) and returns 0.
struct BnSync {
  int (*fn)(void* user, float* buf, int count) = nullptr;
  void* user = nullptr;
  int world = 1;
  float* buf = nullptr;   // caller-owned device buffer, >= 512 floats (2 x the widest layer's channels)
};
// local sums -> the sums the apply / finalize stage uses (buf after the all-reduce, or `sums` itself when not synchronising) and
// the factor that turns 1 / n_local into 1 / n_global
hipError_t bn_sync_sums(const BnSync* sy, const float* sums, int count, hipStream_t s, const float** sums_apply, float* inv_scale);
// second stage of a BatchNorm backward (after its reduce kernel's launch): block records partial[nrec][C][2] -> sums[C][2] in a fixed
// order -> bn_sync_sums; *inv_n (in: 1 / n_local) leaves as 1 / n_global
hipError_t bn_bwd_sums(const float* partial, int nrec, int C, float* sums, float* scratch, const BnSync* sync, hipStream_t s,
                       const float** sums_apply, float* inv_n);

struct Cnn1dEval {
  bool prepared = false;
  void* packed = nullptr;
  float *w[3] = {nullptr, nullptr, nullptr}, *b[3] = {nullptr, nullptr, nullptr};
  float* wp[3] = {nullptr, nullptr, nullptr};   // MFMA A-fragment images of the folded weights (cnn1d_fused.hip)
  void* wx[3] = {nullptr, nullptr, nullptr};    // hi / lo bf16 A-fragment images (cnn1d_fused_x3.hip)
};
struct Cnn1dTrain {          // cnn1d_train_api.hip
  void* train_packed = nullptr;   // data-gradient weight images of conv layers 2 and 3 (+ a zero bias)
  float *wt[2] = {nullptr, nullptr}, *zero_bias = nullptr;
  int wx3_F = 0, wx3_k1 = 3;      // what the wx3 allocation was sized for
  void* wx3[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // per-step bf16x3 A-fragment images: forward layers 1-3, data gradients 3->2, 2->1 (conv1d_x3_kernel); wx3[0] = their one allocation
  AugCfg aug_armed{};             // dfa_cnn1d_set_train_augment: consumed by the next forward_train
  TrainStep step;
  void release() {
    if (train_packed) (void)hipFree(train_packed);
    if (wx3[0]) (void)hipFree(wx3[0]);
    train_packed = wx3[0] = nullptr;
  }
};
struct Cnn1dState : Cnn1dEval {
  const float* p[DFA_CNN1D_NPARAMS] = {nullptr};
  bool have_params = false;
  int in_features = 0;
  int k1 = 3;                  // taps of layer 1: 3, or 5 for the k = (5, 3, 3) variant (dfa_cnn1d_set_kernels; sticky)
  Cnn1dTrain train;
};

struct CaeEval {
  int prepared_prec = -1;
  void* packed = nullptr;
  float *w1 = nullptr, *b1 = nullptr;
  PackedConv enc[3];   // encoder blocks 2-4
  PackedConv dec[3];   // decoder blocks 1-3 (ConvTranspose2d images)
  uint4* c1pack = nullptr;     // block-1 MFMA A operands [6][64]: three bf16 terms of the folded weights, even / odd row (cae_enc1_mfma.hip)
  float* c1bias = nullptr;     // [32] 0.5 * folded bias
  uint4* dec4pack = nullptr;   // decoder block 4 as MFMA A operands [4][64] (cae_dec_fused.hip)
  float* opad_cst = nullptr;   // [16] reconstruction constants of the output_padding columns (cae_dec_fused.hip)
};
struct CaeTrain {            // cae_train_api.hip: raw forward images, data-gradient images, raw ConvTranspose2d images
  void* train_packed = nullptr;
  float *tw1 = nullptr, *tb1 = nullptr;
  PackedConv tenc[3], tdg[3], tdec[3];
  TrainStep step;
  void release() { if (train_packed) (void)hipFree(train_packed); train_packed = nullptr; }
};
struct CaeState : CaeEval {
  const float* p[DFA_CAE_NPARAMS] = {nullptr};
  bool have_params = false;
  CaeTrain train;
};

// DeepfakeDetector (dlq.hip, dlq_api.hip)
struct DlqEval {
  bool prepared = false;
  void* packed = nullptr;                       // one device allocation: the three A-fragment images, then the folded biases
  void* w[3] = {nullptr, nullptr, nullptr};     // three-term bf16 A-fragment images, BatchNorm folded
  float* b[3] = {nullptr, nullptr, nullptr};    // folded biases [256]
};
struct DlqTrain {            // dlq_train_api.hip: this step's raw weight images -- forward layers 1-3, data gradients 3 -> 2 and 2 -> 1
  void* train_packed = nullptr;
  void* tw[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int tw_in_ch = 0;
  TrainStep step;
  void release() { if (train_packed) (void)hipFree(train_packed); train_packed = nullptr; }
};
struct DlqState : DlqEval {
  const float* p[DFA_DLQ_NPARAMS] = {nullptr};
  bool have_params = false;
  int in_ch = 0;
  DlqTrain train;
};

// Embedding anomaly detectors (emb_score.hip, emb_api.hip): the caller's arrays as bound (remembered, not copied) and the image the
// context owns beside them -- |sv_i|^2; prec_chol transposed and the mixture means, both zero-padded to P_pad
struct EmbOcsvm {
  bool bound = false;
  int D = 0, n_sv = 0;
  const float *mean = nullptr, *inv_scale = nullptr, *sv = nullptr, *coef = nullptr;
  float gamma = 0.f, intercept = 0.f;
  float* svn = nullptr;      // [n_sv], the image
};
struct EmbGmm {
  bool bound = false;
  int D = 0, P = 0, K = 0;
  const float *mean = nullptr, *inv_scale = nullptr, *pca_mean = nullptr, *comp = nullptr, *log_const = nullptr;
  void* image = nullptr;     // one allocation: LT, then mpad
  float *LT = nullptr, *mpad = nullptr;   // [K][P_pad][P_pad], [K][P_pad]
};

}  // namespace dfa

struct dfa_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  char err[512] = {0};
  void* zero_page = nullptr;   // 256 zero bytes: source of out-of-image chunks for LDS-DMA staging
  dfa::BnSync bn_sync;         // dfa_ctx_set_bn_sync: synchronised BatchNorm statistics in the three models' forward_train / backward
  int block3_m16 = 1;          // bf16 block 3 on v_mfma_f32_16x16x32_bf16 (conv3_m16.hip); 0 = the 32x32x16 kernel
  int fuse_conv1 = 1;          // bf16 mode: blocks 1 and 2 in one kernel (conv12_fused.hip; fp32 features are rounded to bf16 on load); 0 = two kernels
  int fuse_blocks123 = 1;      // bf16 mode, fuse_conv1 && block3_m16, no time split: blocks 1-3 + time mean in one kernel (conv123_fused.hip)
  int persist123 = 1;          // where blocks 1-3 are fused: 1 = one workgroup per CU over a contiguous range of units (conv123_persist.hip), 0 = one workgroup per unit
  int carry_a1 = 1;            // where persist123 applies and every workgroup's range is a whole number of utterances: the two left a1 halo columns of a strip come from the strip before it (conv123_carry.hip), 0 = conv123_persist.hip
  int phase123 = 1;            // where the carry form runs: its de-phased build (consumers' step barrier behind fragment read 35, consumers at s_setprio 1: conv123_phase.hip), 0 = conv123_carry.hip
  int cls123 = 1;              // where the phase form runs: conv123_cls.hip (classifier head inside the kernel, no linear1_kernel launch), 0 = conv123_phase.hip + linear1_kernel.  Not a plan option: the plan's values do not depend on it
  int last_conv123_cls = 0;    // 1 = the last dfa_cnn2d_forward computed the logits inside the blocks 1-3 kernel (dfa_ctx_last_conv123_cls)
  int last_conv123_phase = 0;  // 1 = the last dfa_cnn2d_forward ran conv123_phase.hip (dfa_ctx_last_conv123_phase)
  int last_conv123_form = 0;   // blocks 1-3 of the last dfa_cnn2d_forward: DFA_CONV123_* (dfa_ctx_last_conv123_form)
  int num_cus = 0;             // hipDeviceAttributeMultiprocessorCount of `device`, asked once in dfa_ctx_create (grid of the persistent kernel)
  int lds_pipe = 1;            // 1 = asm-pipelined LDS fragment reads where instantiated, 0 = compiler-scheduled twins (test hook)
  int time_split = -1;         // eval forward, small batches: -1 = automatic time-axis split, 0 = off, n > 0 = force n segments
  int conv1_bwd_fused = 1;     // CNN2D training: block-1 backward as ONE pass over da1 (train_conv1.hip BWD_FUSED); 0 = reduce pass + weight-gradient pass
  int conv1_mfma = 1;          // bf16 training, bf16 features, no folded augmentation: block-1 passes on the matrix cores (train_conv1_mfma.hip); 0 = vector-ALU kernels
  int dgrad_m16 = 1;           // bf16 training: data-gradient convolutions on the 16x16x32 kernel (conv_split.hip), one launch each; 0 = the 32x32x16 kernels
  int cae_enc1_mfma = 1;       // auto-encoder eval forward, bf16 mode: block 1 on the matrix cores (cae_enc1_mfma.hip); 0 = the vector-ALU kernel
  int cae_enc_dma = 1;         // auto-encoder eval forward, bf16 mode: encoder blocks 2-4 stage their input rows by LDS-DMA; 0 = through registers
  int cae_dgrad_mfma = 1;      // auto-encoder training, bf16 mode: ConvTranspose2d data gradients on the bf16 matrix cores writing bf16
                               // (convt_dgrad_bf16.hip); 0 = the fp32-MFMA GEMM + cast pass of round 2
  int cae_conv_stats = 1;      // auto-encoder training: encoder blocks 2-3 and decoder blocks 1-3 take their BatchNorm statistics in the convolution's epilogue (0 = separate pass over z)
  int cae_bwd_fold = 1;        // auto-encoder training: the decoder's BatchNorm-backward apply pass writes dz patch-major and sums the ConvTranspose2d bias gradient (0 = three passes)
  int cae_enc4_wide = 1;       // auto-encoder training, bf16 mode: encoder block 4 forward in ONE 128-input-channel launch, its data gradient in two (0 = 64-channel launches chained through fp32 partial sums)
  int cae_dec_fused = 1;       // auto-encoder eval forward, bf16 mode: decoder + squared error as ONE kernel (cae_dec_fused.hip); 0 = four launches
  int cnn1d_train_x3 = 1;      // CNN1D training convolutions (3 forward, 2 data gradients) on the matrix-core layer kernel (conv1d_x3_kernel) where
                               // its layout rules hold: 1 = three bf16 terms per operand (fp32-grade), 3 = two terms (bf16x3, ~1e-5: opt-in),
                               // 0 = the fp32 VALU kernel (conv1d.hip); 2 = diagnostic: as 1 with one channel tile per workgroup
  int cnn1d_fused = 1;         // CNN1D eval forward as ONE kernel when T <= 384: 1 = split-bf16 kernel (cnn1d_fused_x3.hip) for the reference's
                               // storage layout, the exact-fp32 one (cnn1d_fused.hip) otherwise; 2 = always the exact-fp32 one; 0 = the three-launch path
  int wgrad_variant = 3;       // bf16 3x3 weight gradients (wgrad_mfma.hip): 3 = the asm-pipelined v3 kernels, 30 = their compiler-scheduled twins, 2 = the v2 kernels (test hook)
  int train_conv_variant = 2;  // bf16 training convolutions (conv3x3_inst_train.hip): 2 = asm-pipelined LDS reads, 0 = their compiler-scheduled twins, 1 = the one-wave-per-SIMD
                               // instantiations; 7 / 8 = diagnostic fp32 ACCIN forms (test hook)
  int clock_probe = 0;         // 1 = the bf16 block-3 kernel stamps its main loop (s_memtime / s_memrealtime) into clock_buf: dfa_ctx_clock_read
  long long* clock_buf = nullptr;   // device, 1024 x {cycles, 100 MHz ticks}
  float* aug_keep = nullptr;        // device copy of the armed augmentation's keep mask (dfa_cnn2d_set_train_augment copies keep_f)
  int aug_keep_cap = 0, aug_keep_slot = 0;
  float* mse_partial = nullptr;     // device, kMseBlocks floats: block sums of dfa_mse_fwd_bwd (allocated on first use)
  double* clip_partial = nullptr;   // device, 256 doubles: block sums of dfa_clip_grad_norm (allocated on first use)
  // ragged forwards: pinned host staging of the per-call table (RaggedTab), kRaggedSlots slots used in turn; a slot is rewritten
  // only after the event recorded behind its last copy has completed
  static constexpr int kRaggedSlots = 4;
  int32_t* ragged_host = nullptr;   // kRaggedSlots x ragged_cap words
  size_t ragged_cap = 0;
  int ragged_slot = 0;
  hipEvent_t ragged_done[kRaggedSlots] = {};
  int conv_dma = -1;           // conv input staging: 1 = global_load_lds (LDS-DMA), 0 = through registers, -1 = per-kernel default
  dfa::Cnn2dState cnn2d;
  dfa::Cnn1dState cnn1d;
  dfa::CaeState cae;
  dfa::DlqState dlq;
  dfa::EmbOcsvm emb_ocsvm;
  dfa::EmbGmm emb_gmm;
  unsigned timing = 0;         // bit s set: record HIP events around the launches of timing slot s
  dfa::SlotTimer slots[dfa::kMaxSlots];
};

namespace dfa {

inline int fail(dfa_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int fail(dfa_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define DFA_HIP_CHECK(ctx, expr)                                                                  \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess)                                                                        \
      return dfa::fail(ctx, DFA_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

// RAII-less helper: record start/stop events around a launch when ctx->timing is on
struct ScopedSlot {
  dfa_ctx* ctx;
  int slot;
  int idx;
  ScopedSlot(dfa_ctx* c, int s) : ctx(c), slot(s), idx(-1) {
    if (!((ctx->timing >> slot) & 1u)) return;
    SlotTimer& t = ctx->slots[slot];
    if (t.used >= kEventsPerSlot) return;
    if ((int)t.start.size() <= t.used) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      t.start.push_back(a);
      t.stop.push_back(b);
      t.empty.push_back(0);
    }
    idx = t.used++;
    t.empty[idx] = 0;
    (void)hipEventRecord(t.start[idx], ctx->stream);
  }
  ~ScopedSlot() {
    if (idx >= 0) (void)hipEventRecord(ctx->slots[slot].stop[idx], ctx->stream);
  }
  // the stage this slot times ran inside another kernel and launched nothing of its own: callers still find one record per
  // call in the slot, and dfa_ctx_timing_read adds exactly 0 ms for it
  void nothing_launched() { if (idx >= 0) ctx->slots[slot].empty[idx] = 1; }
};

// ---- launch prototypes (one translation unit each, see Makefile) ---------------------------------
// The caller's features come as a FeatView, a layer's six parameters as a LayerParams (raw_conv(layer): its convolution alone, no
// BatchNorm folded), a BatchNorm layer's mean / invstd / gamma / beta as a BnApply: launch_views.h.  A launcher unpacks them into
// its kernel's own arguments; the channel-major launchers of the CNN1D training path and the DeepfakeDetector keep their strides.
// pack.hip
hipError_t launch_fold_conv1(const LayerParams& lp, float* w1, float* b1, int cout, hipStream_t s);
hipError_t launch_fold_pack_conv3x3(const LayerParams& lp, int cin_total, int cin_off, int cin, int cout, int prec, uint4* wpack,
                                    float* bias, hipStream_t s, float post_scale = 1.0f);
hipError_t launch_pack_conv3x3_dgrad(const float* w, int cin, int cout, int co_off, int co_n, int prec, uint4* wpack,
                                     float* bias, hipStream_t s);
hipError_t launch_fold_pack_convt2x2(const LayerParams& lp, int cin, int cout, int prec, uint4* wpack, float* bias, hipStream_t s);
// gemm_f32.hip
hipError_t launch_gemm_tn_bf16(const void* X, const void* Z, float* partial, size_t partial_floats, int M, int N, int K,
                               int* nparts, hipStream_t s);
hipError_t launch_gemm_f32(int a_bf16, const void* A, int64_t sam, int64_t sak, int b_bf16, const void* Bm, int64_t sbk,
                           int64_t sbn, float* C, int M, int N, int K, int ksplit, hipStream_t s);
// conv1.hip
hipError_t launch_conv1(const FeatView& v, const float* w1, const float* b1, void* out, int out_prec, hipStream_t s,
                        const DropCfg* drop = nullptr, const AugCfg* aug = nullptr);
// linear.hip
hipError_t launch_linear(const float* emb, const float* w, const float* bias, float* logits, int B, int K,
                         hipStream_t s);
hipError_t launch_emb_reduce(const float* parts, int nparts, size_t stride, size_t n, float inv_h, float* out, hipStream_t s);
hipError_t launch_emb_reduce_ragged(const float* parts, size_t stride, int per_b, const int* tab, int B, float* out, hipStream_t s);
// conv1d.hip
hipError_t launch_fold_conv1d(const LayerParams& lp, float* wf, float* bf, int cin, int cout, hipStream_t s, int taps = 3);
// cae_enc1_mfma.hip: auto-encoder block 1 (conv 1 -> 32 + ReLU + 2 x 2 pool) on the matrix cores, bf16 mode
hipError_t launch_cae_enc1_mfma(const FeatView& v, const float* mu, const float* sigma, const uint4* c1pack, const float* c1bias, void* out,
                                hipStream_t s);
hipError_t launch_cae_enc1_mfma_ragged(const FeatView& v, const float* mu, const float* sigma, const uint4* c1pack, const float* c1bias,
                                       void* out, const int* tab, hipStream_t s);
hipError_t launch_pack_cae_enc1_mfma(const float* w1, const float* b1, uint4* pack, float* bias, hipStream_t s);
// cae_dec_fused.hip: the auto-encoder's decoder + per-sample squared error as one kernel (bf16 mode)
int cae_dec_fused_tiles(int H4, int W4);
hipError_t launch_cae_opad_consts(const float* b2, const uint4* wp3, const float* b3, const float* w4, const float* b4, float* cst,
                                  hipStream_t s);
// dec = the three packed decoder blocks (CaeState::dec), head = decoder block 4
hipError_t launch_cae_dec_fused(const void* lat, const PackedConv* dec, const HeadParams& head, const uint4* w4pack, const float* cst,
                                const FeatView& v, const float* mu, const float* sigma, float* recon, float* partial, int H4, int W4,
                                hipStream_t s, long long* stamps = nullptr);
hipError_t launch_cae_dec_fused_ragged(const void* lat, const PackedConv* dec, const HeadParams& head, const uint4* w4pack, const float* cst,
                                       const FeatView& v, const float* mu, const float* sigma, float* partial, int H4, int W4, const int* tab,
                                       hipStream_t s);
bool cae_dec_fused_supports(const FeatView& v);
hipError_t launch_pack_cae_dec4(const float* w4, uint4* pack, hipStream_t s);
hipError_t launch_cae_mse_finalize(const float* partial, int nblk, float inv_n, float* mse, int B, hipStream_t s);
hipError_t launch_cae_mse_finalize_ragged(const float* partial, int nblk, const int* tab, float* mse, int B, hipStream_t s);
// cnn1d_fused.hip: the whole CNN1D eval forward as one kernel (fp32 matrix cores, activations in LDS)
int cnn1d_fused_ncp_pad(int cin, int layer);
size_t cnn1d_fused_pack_floats(int cin, int cout, int layer);
bool cnn1d_fused_supports(int T);
hipError_t launch_pack_cnn1d_fused(const float* wf, float* wp, int cin, int cout, int layer, hipStream_t s);
hipError_t launch_cnn1d_fused(const FeatView& v, const float* wp1, const float* b1, const float* wp2, const float* b2, const float* wp3,
                              const float* b3, const float* cw, const float* cb, float* logits, hipStream_t s, long long* stamps = nullptr);
// cnn1d_fused_x3.hip: the same forward on the bf16 matrix cores with hi + lo bf16 operands (fp32-grade accuracy)
// k1 / taps: the taps of layer 1, 3 or 5 (the k = (5, 3, 3) variant: five-tap kernels, a k-step-major layer-1 image)
size_t cnn1d_x3_pack_bytes(int cin, int cout, int taps = 3);
hipError_t launch_pack_cnn1d_x3(const float* wf, void* wx, int cin, int cout, hipStream_t s, int taps = 3);
bool cnn1d_fused_x3_supports(const FeatView& v, int k1 = 3);
int cnn1d_fused_x3_max_t(int F, int k1);
// ragged form (cnn1d_ragged_x3_kernel): x = the batch padded to T_max, element (b, f, t) at b stride_b + f stride_f + t;
// tab = device table, [0, B) lengths, [B, 2B) dispatch order
hipError_t launch_cnn1d_ragged_x3(const float* x, int64_t stride_b, int64_t stride_f, const int* tab, const void* w1, const float* b1,
                                  const void* w2, const float* b2, const void* w3, const float* b3, const float* cw, const float* cb,
                                  float* logits, int B, int T_max, int F, hipStream_t s, long long* stamps, int k1 = 3);
size_t cnn1d_ragged_lds_bytes(int T_max, int F, int k1 = 3);
int cnn1d_ragged_segments(int T, int F, int* starts, int* lens, int* owned_lo, int* owned_hi, int cap, int k1 = 3);
hipError_t launch_cnn1d_fused_x3(const float* x, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                                 const float* b3, const float* cw, const float* cb, float* logits, int B, int T, int F, hipStream_t s,
                                 long long* stamps = nullptr, int k1 = 3);
hipError_t launch_conv1d(const float* x, int64_t sb, int64_t sc, int64_t st, const float* w, const float* bias,
                         float* out, int B, int Cin, int Cout, int T, bool mean, hipStream_t s, bool relu = true,
                         const AugCfg* aug = nullptr, const int* lens = nullptr, int taps = 3);
// api.hip: the per-call table of a ragged batch ([0, B) lengths, [B, 2B) dispatch order: 2 B words) through the next pinned staging
// slot to `dst` (device) on the context's stream
int stage_ragged_lengths(dfa_ctx* ctx, const int32_t* lengths, int B, void* dst);
// the same with `extra` words the caller supplies behind them: [2B, 2B + extra) (words = 2 B + extra)
int stage_ragged_lengths_extra(dfa_ctx* ctx, const int32_t* lengths, int B, const int32_t* extra, size_t n_extra, void* dst);
// utt_norm.hip: per-utterance CMN / CVMN (dfa_utt_norm).  tab: device table ([0, B) lengths; packed: [2B, 4B) float offsets, low
// word then high word) or null (every row spans T_max)
hipError_t launch_utt_norm_time(const float* x, float* y, const int* tab, int mode, int B, int C, int T_max, int64_t stride_b,
                                int64_t stride_c, bool packed, hipStream_t s);
hipError_t launch_utt_norm_feat(const float* x, float* y, const int* tab, int mode, int B, int C, int T_max, int64_t stride_b,
                                int64_t stride_t, hipStream_t s);
// cnn2d_api.hip, cnn1d_api.hip, cae_api.hip: the models' planners behind dfa_workspace_bytes and dfa_ragged_workspace_bytes
// (api.hip), for B, T, F >= 1.  ctx may be null (CNN2D: the plan of the default options); ragged: T = T_max, the table included
size_t cnn2d_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F, int prec, bool ragged);
size_t cnn1d_workspace_bytes(int B, int T, bool ragged);
size_t cae_workspace_bytes(int B, int T, int F, int prec);
// dlq.hip: the DeepfakeDetector layers (one launch each over the tile list) and the pool + head kernel
struct DlqLayerArgs {
  const float* x;        // layer 1: element (b, c, t) at b sb + c sc + t
  int64_t sb, sc;
  const uint4* hin;      // layers 2, 3: [B][T_max] split pixels (three bf16 terms of 256 channels, 1536 bytes)
  uint4* hout;           // layers 1, 2
  const uint4* w;
  const float* bias;
  const int* tab;        // [0, B) lengths; [2B, 3B) dispatch order; [3B, 4B] first tile of each dispatch position
  float* part;           // layer 3: [tile][mean 256 | M2 256]
  int B, T_max, C, nks;
  // the training step's dense launches (launch_dlq_layer_train; tab = the lengths alone)
  int tpu;               // tiles per utterance, ceil(T_max / NF)
  float* zout;           // mode 1: z of this layer, mode 2: dy of the layer below; fp32 [B][T_max][256]
  float* rec;            // per tile: mode 1 [mean 256 | M2 256], mode 2 [256][sum dy, sum dy zhat]
  const float *zprev, *st_mean, *st_invstd, *gamma, *beta;   // mode 2: z, batch statistics and affine of the layer below
  DropCfg drop;          // mode 2: the layer below's dropout (drop.layer set)
};
int dlq_nks(int cin);
size_t dlq_pack_bytes(int cin, int taps);
hipError_t launch_dlq_pack(const LayerParams& lp, int cin, int taps, void* wp, float* bias, hipStream_t s);
hipError_t launch_dlq_layer(int layer, const DlqLayerArgs& a, int ntiles, hipStream_t s);
hipError_t launch_dlq_layer_train(int layer, int mode, const DlqLayerArgs& a, int ntiles, hipStream_t s);
hipError_t launch_dlq_finish(const float* part, const int* tab, const float* w0, const float* b0, const float* w3, const float* b3, float* logits,
                             float* pooled, int B, hipStream_t s);
// dlq_train.hip: the DeepfakeDetector training step besides the layer kernel
struct DlqPackJobs {
  const float* w[5]; uint4* dst[5];
  int cin[5], taps[5], dgrad[5], first[6];   // first[q]: the job's first workgroup
};
hipError_t launch_dlq_train_pack(const float* w1, const float* w2, const float* w3, void* const* dst, int in_ch, hipStream_t s);
hipError_t launch_dlq_bn_finalize(const float* rec, int ntiles, int tpu, int T_max, float* mean, float* var, float* invstd, float* rm, float* rv,
                                  float momentum, hipStream_t s);
hipError_t launch_dlq_bn_act(const float* z, const BnApply& bn, void* h, unsigned char* keep_out, long long N, const DropCfg& dc, hipStream_t s);
struct DlqHeadArgs {       // layer 3's BN + GELU + dropout, the pool, the head; forward and backward
  const float *z3, *mean, *invstd, *gamma, *beta;   // layer 3
  const int* lens;
  const float *w0, *b0, *w3, *b3;                   // head.0, head.3
  float *pooled, *pvar, *u, *logits;                // [B][512] mean | std, [B][256] variance, [B][256] head.0's output
  unsigned char *keep3, *keep4;                     // test hook or null
  const float* dlogits;
  float *du, *dpooled;                              // [B][256], [B][512]
  int T_max;
  DropCfg drop;                                     // layer = 3; the head's dropout is layer 4
};
hipError_t launch_dlq_pool_head(const DlqHeadArgs& a, int B, hipStream_t s);
hipError_t launch_dlq_head_bwd(const DlqHeadArgs& a, int B, float* dw0, float* db0, float* dw3, float* db3, hipStream_t s);
hipError_t launch_dlq_dy3(const DlqHeadArgs& a, int B, int tpu, float* dy, float* rec, hipStream_t s);
int dlq_dz_blocks(long long N);
hipError_t launch_dlq_dz(const float* dy, const float* z, const BnApply& bn, const float* sums, void* dz, float* dbrec, long long N, hipStream_t s);
struct DlqWgradArgs {
  const uint4* dz;       // [N] split pixels
  const uint4* h;        // the source as split pixels, or
  const float* x;        // x itself (layer 1): element (b, c, t) at b sb + c sc + t, zero at t >= lens[b]
  int64_t sb, sc;
  const int* lens;
  float* partial;        // [chunks][taps][256][C]
  long long N;           // B T_max
  int T_max, C, taps, CH;
};
void dlq_wgrad_chunks(long long N, int* CH, int* nch);
hipError_t launch_dlq_wgrad(const DlqWgradArgs& a, float* dw, hipStream_t s);
hipError_t launch_bce_pos_weight(const float* logits, const float* labels, float pw, int B, float* loss, float* dlogits, hipStream_t s);
hipError_t launch_clip_grad_norm(float* g, size_t n, float max_norm, float* norm_out, double* partial, hipStream_t s);
// train_cnn1d.hip
int cm_chunks(int B);
int conv1d_wgrad_chunks(int B);
// lens (device, [B]) != null selects the ragged twins: utterance b owns frames [0, lens[b]) of the T the batch is padded to
hipError_t launch_cm_stats(const float* z, float* partial, int B, int C, int T, hipStream_t s, const int* lens = nullptr, bool shifted = false);
hipError_t launch_cm_bn_relu_drop(const float* z, const BnApply& bn, float* h, int B, int C, int T, const DropCfg& dc, hipStream_t s,
                                  const int* lens = nullptr);
hipError_t launch_cm_bn_relu_meant(const float* z, const BnApply& bn, float* pooled, int B, int C, int T, hipStream_t s, const int* lens = nullptr);
hipError_t launch_cm_bn_bwd(int src, const float* z, const BnApply& bn, const float* up, float* partial, float* sums, float* dz, int B, int C,
                            int T, const DropCfg& dc, hipStream_t s, const BnSync* sync = nullptr, const int* lens = nullptr, double n_valid = 0.0);
// conv1d_x3.hip: the matrix-core layer kernel of the training step.  taps = 5: layer 1 of the k = (5, 3, 3) variant (Cout = 32, no
// lens; weights streamed from the k-step-major image of launch_pack_conv1d_train_all, k1 = 5)
bool conv1d_x3_supports(const float* x, int64_t sb, int64_t sc, int64_t st, const float* z, int T, int Cin, int Cout, int terms, int taps = 3);
hipError_t launch_conv1d_x3(const float* x, int64_t sb, const void* wx, const float* bias, float* z, int B, int Cin, int Cout, int T,
                            int terms, hipStream_t s, int mode = 1, const AugCfg* aug = nullptr, const int* lens = nullptr, int taps = 3);
size_t conv1d_terms_pack_bytes(int cin, int cout, int terms, int taps = 3);
hipError_t launch_pack_conv1d_train_all(const float* w1, const float* w2, const float* w3, void* const* dst, int F, int terms, float* zero_bias,
                                        hipStream_t s, int k1 = 3);
// taps = 5: layer 1 of the k = (5, 3, 3) variant (uniform batches; record [Cout][Cin][5] + [Cout])
hipError_t launch_conv1d_wgrad(const float* dz, const float* h, int64_t hsb, int64_t hsc, int64_t hst, float* partial,
                               float* dw, float* db, int B, int Cin, int Cout, int T, hipStream_t s, const AugCfg* aug = nullptr, int x3 = 0, const int* lens = nullptr,
                               int taps = 3);
hipError_t launch_conv1d_dgrad_pack(const float* w, float* wt, float* zero_bias, int cin, int cout, hipStream_t s);
// cae.hip
hipError_t launch_cae_enc1(const FeatView& v, const float* mu, const float* sigma, const float* w1, const float* b1, void* out, int prec,
                           hipStream_t s);
hipError_t launch_cae_opad_col(void* out, const float* bias, int prec, int rows, int Wo, int C, hipStream_t s,
                               int no_relu = 0);
int cae_dec4_blocks(int T, int W3);
hipError_t launch_cae_dec4_mse(const void* d3, int prec, const HeadParams& head, const FeatView& v, const float* mu, const float* sigma,
                               float* recon, float* partial, float* mse, int H3, int W3, hipStream_t s);
hipError_t launch_cae_latent_export(const void* lat, int prec, float* out, int B, int HW, int C, hipStream_t s);
// train_elem.hip / train_conv1.hip / wgrad_mfma.hip
// the `mode` of launch_conv1_train and the `src` of launch_bn_bwd (described at their kernels)
enum { C1M_STATS = 0, C1M_BWD_REDUCE = 1, C1M_WGRAD = 2, C1M_BWD_FUSED = 3, C1M_STATS_XX = 4 };
enum { SRC_POOL = 1, SRC_DIRECT = 2, SRC_POOL22 = 3 };
hipError_t launch_bn_finalize(const float* partial, int nparts, int C, double n, float* mean, float* var, float* invstd,
                              float* running_mean, float* running_var, float momentum, hipStream_t s,
                              const float* shift = nullptr, int shift_stride = 0);   // sums of z - shift[c * shift_stride]
hipError_t launch_reduce_partials(const float* partial, int nparts, int n, float scale, float* out, hipStream_t s,
                                  float* scratch = nullptr);
hipError_t launch_bn_relu_pool_drop(int prec, const void* z, const BnApply& bn, void* out, int B, int H, int W, int C, const DropCfg& dc,
                                    hipStream_t s);
int cl_stats_blocks(size_t npix, int* pix_per_block);
hipError_t launch_cl_stats(int prec, const void* z, float* partial, size_t npix, int C, hipStream_t s);
hipError_t launch_bn_relu_pool(int prec, int pool, const void* z, const BnApply& bn, void* out, int B, int H, int W, int C, hipStream_t s);
hipError_t launch_bn_relu_meant(int prec, const void* z, const BnApply& bn, float* emb, int B, int H, int W, int C, hipStream_t s,
                                float* msum = nullptr);
hipError_t launch_bn_bwd_meant_saved(int prec, const void* z, const BnApply& bn, const float* demb, const float* msum, float* partial,
                                     float* sums, void* dz, int B, int H, int W, int C, hipStream_t s, const BnSync* sync = nullptr);
hipError_t launch_linear_bwd(const float* dlogits, const float* w, const float* emb, float* demb, float* dw, float* db,
                             int B, int K, hipStream_t s, int tc = 0, int tw = 0);
int bn_bwd_blocks(int B, int H, int W, int* pix_per_block);
// SRC_DIRECT apply pass that writes dz patch-major (the pixel-unshuffled operand of a ConvTranspose2d(k2, s2) layer's gradient GEMMs,
// Wh input columns) and leaves [nrec][C] records of its channel sums in bias_partial (train_elem.hip bn_bwd_apply_unshuffle_kernel)
struct BnBwdFold { void* zp; int Wh; float* bias_partial; int nrec; };
hipError_t launch_bn_bwd(int prec, int src, const void* z, const BnApply& bn, const void* da, float* partial, float* sums, void* dz, int B,
                         int H, int W, int C, const DropCfg& dc, hipStream_t s, float* scratch = nullptr, const BnSync* sync = nullptr,
                         BnBwdFold* fold = nullptr);
// sums[C][2] -> dbeta = S1, dgamma = S2 (C <= 256); the conv1 weight-gradient record [32][10] -> dW1[32][9], db1[32]
hipError_t launch_split_sums(const float* sums, float* dgamma, float* dbeta, int C, hipStream_t s);
hipError_t launch_split_c1(const float* rec, float* dw, float* db, hipStream_t s);
hipError_t launch_bce_smooth(const float* logits, const float* labels, float eps, int B, float* loss, float* dlogits,
                             hipStream_t s);
hipError_t launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps,
                        float wd, int step, float grad_scale, hipStream_t s);
int conv1_train_blocks(int B, int T, int F);
// train_conv1_mfma.hip: the block-1 train passes on the matrix cores (bf16 features, no folded augmentation)
enum { C1X_STATS = 0, C1X_FWD = 1, C1X_BWD = 2 };
int conv1_mfma_blocks(int B, int T, int F);
// (v: bf16 features.)  The passes of one block 1 (train_host.h: Conv1Train); poolw = the pool behind the block, 1 in the statistics passes
hipError_t launch_conv1_mfma(int mode, const FeatView& v, const float* w, const float* bias, void* a1, const void* da1, float* partial,
                             const DropCfg& dc, int poolw, hipStream_t s);
// bn: null terms in the statistics passes.  sums, inv_n_scale: the (S1, S2) C1M_WGRAD forms dz1 from, and 1 / world where they are the
// synchronised ones (1 otherwise)
hipError_t launch_conv1_train(int mode, const FeatView& v, const float* w, const float* bconv, const BnApply& bn, const float* sums,
                              const void* da1, int prec, float* partial, const DropCfg& dc, int poolw, const AugCfg* aug, float inv_n_scale,
                              hipStream_t s);
hipError_t launch_conv1_bwd_finalize(const float* rec, const float* xxs, const LayerParams& lp, const BnApply& bn, double n, const LayerGrads& g,
                                     hipStream_t s, int derive_s2 = 0);
// cae_train.hip
hipError_t launch_pixel_unshuffle(int prec, const void* dz, void* zp, int B, int H, int W, int Wo, int C, hipStream_t s);
hipError_t launch_convt_w_to_q(const float* w, float* wq, int cin, int cout, hipStream_t s);
hipError_t launch_convt_q_to_w(const float* dwq, float* dw, int cin, int cout, hipStream_t s);
int cae_dec4_bwd_blocks();
// MSE form of the decoder-block-4 backward (drecon == nullptr): the upstream gradient 2 (recon - x) / (B T F) is formed in the kernel
struct MseArgs {
  FeatView v;              // x
  const float* b4_dev;
};
hipError_t launch_cae_dec4_bwd(int prec, const void* d3, const float* w4, const float* drecon, void* dd3, float* partial,
                               int B, int H3, int W3, int T, int F, hipStream_t s, const MseArgs* mse_args = nullptr);
// loss = mean((recon - x)^2), drecon = 2 (recon - x) / n  (src/train_cae.py:67-68,203); partial: >= kMseBlocks floats of scratch
constexpr int kMseBlocks = 1024;
hipError_t launch_mse_fwd_bwd(const float* recon, const FeatView& v, float* partial, float* loss, float* drecon, hipStream_t s);
bool convt_dgrad_bf16_supports(int Cin, int Cout);
hipError_t launch_convt_dgrad_bf16(const void* zp, const float* wq, void* wfrag, void* dx, long P, int Cin, int Cout, hipStream_t s);
hipError_t launch_cast_from_f32(int prec, const float* src, void* dst, size_t n, hipStream_t s);
// wgrad_mfma.hip; variant = the context's wgrad_variant
hipError_t launch_wgrad3x3_window(int prec, int cin, int cout, int cin_total, int cout_total, int ci_off, int co_off,
                                  const void* dz, const void* a, float* partial, float* dw, float* db, int B, int H,
                                  int W, int nwg, hipStream_t s, int variant);
hipError_t launch_wgrad3x3(int prec, int cin, int cout, const void* dz, const void* a, float* partial, float* dw,
                           float* db, int B, int H, int W, int nwg, hipStream_t s, int variant);
// conv3x3_inst_*.hip; variant = the context's train_conv_variant
hipError_t launch_fold_pack_conv3x3_m16(const LayerParams& lp, int cin, int cout, uint4* wpack, hipStream_t s);
hipError_t launch_train_fwd2(int prec, const ConvArgs& a, hipStream_t s, int variant);
hipError_t launch_train_fwd3(int prec, const ConvArgs& a, hipStream_t s);
hipError_t launch_train_dgrad3(int prec, const ConvArgs& a, float* raw_tmp, hipStream_t s, int variant);
hipError_t launch_train_dgrad2(int prec, const ConvArgs& a, hipStream_t s);
hipError_t launch_cae_train_fwd(int prec, int cin, const ConvArgs& a, float* raw_tmp, hipStream_t s, int wide, int variant);
hipError_t launch_cae_dgrad4(int prec, const ConvArgs& a, float* raw_tmp, hipStream_t s, int wide);
hipError_t launch_train_fwd3_m16(const ConvArgs& a, hipStream_t s, int pipe = 1);
// conv_split.hip (DFA_PREC_BF16X3)
hipError_t launch_fold_pack_conv3x3_split(const LayerParams& lp, int cin, int cout, uint4* wpack, float* bias, float post_scale, hipStream_t s);
hipError_t launch_cnn2d_block2_split(const ConvArgs& a, hipStream_t s, int pipe = 1);
hipError_t launch_cnn2d_block3_split(const ConvArgs& a, hipStream_t s, int pipe = 1);
hipError_t launch_pack_conv3x3_dgrad_m16(const float* w, int cin, int cout, uint4* wpack, float* bias, hipStream_t s);
hipError_t launch_train_dgrad3_m16(const ConvArgs& a, hipStream_t s, int pipe = 1);
hipError_t launch_train_dgrad2_m16(const ConvArgs& a, hipStream_t s, int pipe = 1);
hipError_t launch_cnn2d_block3_m16(const ConvArgs& a, hipStream_t s, int pipe = 1);
hipError_t launch_cnn2d_block3_m16_ragged(const ConvArgs& a, const RaggedTab& rt, int nseg, hipStream_t s, int pipe = 1);
hipError_t launch_reduce_wgrad_record(const float* partial, int nparts, int stride, int cin, int cout, int cin_total,
                                      int ci_off, int co_off, float* dw, float* db, hipStream_t s, int perm = 0);
hipError_t launch_pack_conv1_mfma(const float* w1, const float* b1, uint4* c1pack, float* c1bias, hipStream_t s);
hipError_t launch_conv12_fused(const FeatView& v, const uint4* c1pack, const float* c1bias, const uint4* wpack2, const float* bias2, void* a2,
                               hipStream_t s, int pipe = 1, int seg_iters = 0);
hipError_t launch_conv12_ragged(const FeatView& v, const uint4* c1pack, const float* c1bias, const uint4* wpack2, const float* bias2, void* a2,
                                const int* tab, hipStream_t s, int pipe = 1, int seg_iters = 0);
// (blocks 1-3 in one kernel, conv123_*.hip: conv123_host.h)
hipError_t launch_cnn2d_block2(int prec, const ConvArgs& a, hipStream_t s, int dma = -1, int pipe = 1);
hipError_t launch_cnn2d_block3(int prec, const ConvArgs& a, hipStream_t s, int dma = -1, int pipe = 1);
struct ConvTArgs;
hipError_t launch_cae_enc2(int prec, const ConvArgs& a, hipStream_t s, int pipe = 1, int dma = 0);
hipError_t launch_cae_enc3(int prec, const ConvArgs& a, hipStream_t s, int pipe = 1, int dma = 0);
hipError_t launch_cae_enc4(int prec, const ConvArgs& a, float* raw_tmp, hipStream_t s, int dma, int variant);
hipError_t launch_cae_enc_ragged(int layer, const ConvArgs& a, const RaggedTab& rt, hipStream_t s);
hipError_t launch_cae_dec(int prec, int cin, const ConvTArgs& a, hipStream_t s);
int cae_dec_stats_records(int prec, int cin, long P);
// emb_score.hip: the split of the reduction over D (a function of D and the column count M alone: a row's score does not depend on
// the batch it is scored in), P rounded up to the GEMM frame's stage, and the launches of the two detectors
struct EmbSplit { int klen, nsplit; };
EmbSplit emb_split(int D, int M);
inline int emb_ppad(int P) { return (P + 31) / 32 * 32; }
hipError_t launch_emb_rownorm(const float* x, int64_t ld, int rows, int D, float* out, hipStream_t s);
hipError_t launch_emb_pack_gmm(const float* prec_chol, const float* means, int P, int K, float* LT, float* mpad, hipStream_t s);
// part: [nsplit][N][n_sv] floats
hipError_t launch_emb_ocsvm(const EmbOcsvm& d, const float* emb, int N, int64_t ld, float* part, float* out, hipStream_t s);
// zpart: [nsplit][N][P], z: [N][P_pad], y: [K][N][P] floats
hipError_t launch_emb_gmm(const EmbGmm& d, const float* emb, int N, int64_t ld, float* zpart, float* z, float* y, float* out, hipStream_t s);

}  // namespace dfa

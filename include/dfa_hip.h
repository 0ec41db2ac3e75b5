/*
 * dfa_hip.h -- C ABI of libdfa_hip.so: the MI355X (gfx950) implementation of the LFCC-classifier
 * hot path of kingdomseed/Deep-Fake-Audio-Classifier.
 *
 * The reference has no FFI of its own: its boundary for this path is the nn.Module surface of
 * src/model.py:5-42 (CNN2D), src/model_cnn1d.py:5-46 (CNN1D), src/model_cae.py:20-125
 * (ConvAutoencoder) plus the loss/optimiser calls of src/train.py:71-76,311-330.  Each entry point
 * below names the reference code it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C types only; every pointer named "device" is a HIP device pointer owned by the caller
 *     (PyTorch-ROCm tensors are used for storage only);
 *   - every function returns 0 (DFA_OK) or a negative DFA_E_* code; dfa_last_error() gives the text;
 *   - a context is bound to one device and one HIP stream; calls enqueue work on that stream and
 *     return without synchronising; a context is not thread-safe; one process per GPU for data parallel;
 *   - no allocation on the hot path: activations live in a caller-provided workspace
 *     (dfa_workspace_bytes), the library owns only the packed (BN-folded, MFMA-ordered) weights.
 */
#ifndef DFA_HIP_H
#define DFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFA_VERSION 100 /* 0.1.0 */

/* error codes */
#define DFA_OK 0
#define DFA_E_BAD_SHAPE (-1)
#define DFA_E_BAD_DTYPE (-2)
#define DFA_E_NULL_PTR (-3)
#define DFA_E_NOT_PREPARED (-4)
#define DFA_E_HIP (-5)
#define DFA_E_WORKSPACE (-6)
#define DFA_E_UNSUPPORTED (-7)

/* element types of the input tensor x */
#define DFA_DTYPE_F32 0
#define DFA_DTYPE_BF16 1

/* arithmetic mode of the convolution stack (chosen at prepare time)
 *   DFA_PREC_F32  : fp32 storage, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) -- parity mode, logits within 1e-4
 *   DFA_PREC_BF16 : bf16 storage of weights/activations, fp32 accumulate (v_mfma_f32_32x32x16_bf16) -- throughput mode
 *   DFA_PREC_BF16X3 : CNN2D only.  Every weight and activation is carried as hi + lo bf16 (16 significant bits) and every
 *                   product is three bf16 MFMAs (hi*hi + lo*hi + hi*lo) accumulated in fp32 -- parity-grade (logits within
 *                   1e-4 of the reference like DFA_PREC_F32) at 3/16 of the fp32-MFMA cost */
#define DFA_PREC_F32 0
#define DFA_PREC_BF16 1
#define DFA_PREC_BF16X3 2

/* model ids for dfa_workspace_bytes */
#define DFA_MODEL_CNN2D 0
#define DFA_MODEL_CNN1D 1
#define DFA_MODEL_CAE 2

typedef struct dfa_ctx dfa_ctx;

/* ---- lifecycle ------------------------------------------------------------------------------ */
int dfa_version(void);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for the default stream */
int dfa_ctx_create(int device_id, void* hip_stream, dfa_ctx** out);
int dfa_ctx_destroy(dfa_ctx* ctx);
int dfa_ctx_set_stream(dfa_ctx* ctx, void* hip_stream);
/* tuning / test switches (all default to the fastest verified path; the alternatives exist so the tests can compare):
 *   "conv_dma"      1 = stage the MFMA convolutions' input rows with LDS-DMA (global_load_lds), 0 = through registers,
 *                   -1 (default) = per-kernel choice (also: environment variable DFA_CONV_DMA=0|1 before dfa_ctx_create)
 *   "lds_pipe"      1 (default) = asm-pipelined LDS fragment reads in the bf16 kernels that have them, 0 = their
 *                   compiler-scheduled twins (bit-identical results)
 *   "fuse_conv1"    1 (default) = CNN2D bf16 mode on bf16 features runs blocks 1+2 as one kernel, 0 = two kernels
 *   "block3_m16"    1 (default) = CNN2D bf16 block 3 on v_mfma_f32_16x16x32_bf16, 0 = the 32x32x16 kernel
 *   "fuse_blocks123" 1 (default) = CNN2D bf16 eval forward with fuse_conv1 and block3_m16 set runs blocks 1-3 + the time
 *                   mean as ONE kernel (a2 stays in LDS) wherever neither old kernel would split the time axis (B * strips >= 512,
 *                   no forced time_split); 0 = the two-kernel path.  Bit-identical results either way
 *   "persist123"    1 (default) = where fuse_blocks123 applies, the fused kernel runs as one persistent workgroup per CU that
 *                   walks a contiguous range of (utterance, strip) units and stages the next unit under the tail of the current
 *                   one (static ranges, no communication between workgroups); 0 = one workgroup per unit.  Bit-identical results
 *   "carry_a1"      1 (default) = where persist123 applies, every workgroup's range is a whole number of utterances (B * strips
 *                   a multiple of the CU count, the quotient a multiple of the strips per utterance) and T is short enough for
 *                   the side buffer to fit LDS, a strip takes its two left a1 halo columns from the strip before it instead of
 *                   computing them again; 0 = the persist123 kernel everywhere.  Bit-identical results
 *   "phase123"      1 (default) = where carry_a1 applies, the build of that kernel whose consumer waves hold their step barrier
 *                   late in their operand reads and run at raised issue priority, so that the MFMA-free parts of the two
 *                   roles' steps do not coincide; 0 = the carry_a1 kernel as it was.  Bit-identical results
 *   "cls123"        1 (default) = where phase123 applies and the classifier weights and the embedding are 16-byte aligned, the
 *                   build of that kernel which computes the
 *                   logits at the end of each workgroup, from the embedding rows it has just written: no linear1_kernel launch
 *                   (timing slot 3 keeps its one record per forward, of exactly 0 ms: no launch in it).  0 = the phase123 kernel and the separate classifier launch.  Bit-identical
 *                   logits and embeddings.  Not one of the plan's options: dfa_cnn2d_forward_plan answers the same either way
 *   "time_split"    -1 (default) = CNN2D eval forward splits the time axis over workgroups when the batch alone cannot fill
 *                   the chip (B * strips below the resident-workgroup count, e.g. the reference's predict batch of 32), 0 =
 *                   never, n > 0 = force n segments (at most 4).  Logits and embeddings are bit-identical for every setting and
 *                   batch size: the time mean is always summed in the same canonical chunks
 *   "conv1_mfma"    1 (default) = bf16 training on bf16 features without a folded augmentation: the block-1 statistics,
 *                   forward and fused backward passes run on the matrix cores (train_conv1_mfma.hip); 0 = vector-ALU kernels.
 *                   May be cleared between dfa_cnn2d_forward_train and dfa_cnn2d_backward (both backward kernels read the
 *                   same forward state; used by the twin test).  The auto-encoder's training step (bf16 mode, bf16 features, even F)
 *                   obeys the same option: statistics + fused backward (2 x 2-pool form) on the same kernels, forward on
 *                   cae_enc1_mfma.hip; 0 = a statistics pass, the eval kernel and two vector-ALU backward passes
 *   "conv1_bwd_fused" 1 (default) = block-1 backward as one pass over da1 + algebra, 0 = reduce pass + weight-gradient pass
 *   "dgrad_m16"     1 (default) = bf16 training: each data-gradient convolution is ONE launch of the 16x16x32 kernel
 *                   (conv_split.hip), 0 = the 32x32x16 kernels (block 3 as two Cin-half launches through fp32 partial sums)
 *   "wgrad_variant" 3 (default) = pipelined bf16 weight-gradient kernel, 30 = its compiler-scheduled twin, 2 = the
 *                   earlier 4-wave kernel.  Held by the context, like every option: it selects kernels for this context's calls only
 *   "train_conv_variant" 2 (default) = pipelined two-wave bf16 training convolutions where they fit, 0 = their
 *                   compiler-scheduled twins, 1 = the one-wave-per-SIMD instantiations.  Per context as well
 *   "cae_enc1_mfma" 1 (default) = auto-encoder eval forward in bf16 mode: block 1 (conv 1 -> 32 + ReLU + 2 x 2 pool) on the matrix
 *                   cores with hi + lo bf16 operands; 0 = the vector-ALU kernel
 *   "cae_enc_dma"   1 (default) = auto-encoder eval forward in bf16 mode: encoder blocks 2-4 stage their input rows by LDS-DMA;
 *                   0 = through registers (bit-identical)
 *   "cae_dgrad_mfma" 1 (default) = auto-encoder training step in bf16 mode: the three ConvTranspose2d data gradients on the bf16
 *                   matrix cores, bf16 result written in place (convt_dgrad_bf16.hip); 0 = fp32-MFMA GEMM + cast pass
 *   "cae_conv_stats" 1 (default) = auto-encoder training step: encoder blocks 2-3 and decoder blocks 1-3 take their BatchNorm batch statistics in the
 *                   convolution's epilogue (fp32 sums of the outputs before they are rounded for storage, as the CNN2D's blocks 2 / 3);
 *                   0 = a separate statistics pass over the stored output
 *   "cae_bwd_fold"  1 (default) = auto-encoder training step: the BatchNorm-backward apply pass of decoder blocks 1-3 writes dz in the
 *                   patch-major order the ConvTranspose2d gradient GEMMs read and sums the bias gradient on the way; 0 = apply pass,
 *                   channel-sum pass and pixel-unshuffle pass (same values)
 *   "cae_enc4_wide" 1 (default) = auto-encoder training step in bf16 mode: encoder block 4 (128 -> 256) forward as ONE launch over all 128
 *                   input channels and its data gradient as two 128-channel launches; 0 = two / four 64-channel launches chained
 *                   through fp32 partial sums (same products, other summation order)
 *   "cae_dec_fused" 1 (default) = auto-encoder eval forward in bf16 mode: the four decoder blocks, the zero time padding and the
 *                   per-sample squared error run as ONE kernel with the intermediates in LDS / registers; 0 = four launches
 *   "cnn1d_fused"   1 (default) = CNN1D eval forward as ONE kernel for T <= 384 (all three Conv1d layers on the matrix cores with the
 *                   activations in LDS, the frame mean and the classifier in its epilogue): hi + lo bf16 operands, three bf16 MFMAs
 *                   per product (fp32-grade: logits within 1e-4 of the reference) when x is the reference's contiguous [B,F,T]
 *                   storage, the exact-fp32 matrix-core kernel for any other strides; 2 = always the exact-fp32 kernel; 0 = the
 *                   three-launch path
 *   "cnn1d_train_x3" 1 (default) = the five convolutions of a CNN1D training step (3 forward, 2 data gradients) on the matrix cores
 *                   (conv1d_x3_kernel, conv1d_x3.hip) when the tensors are in the stored [B,F,T] layout, T <= 384, F % 4 == 0:
 *                   every fp32 operand as three bf16 terms (its 24-bit mantissa exactly), six MFMAs per product -- sums of fp32 grade; a folded
 *                   augmentation (dfa_cnn1d_set_train_augment) is applied as the input slabs are staged.  3 = two terms, three
 *                   MFMAs (bf16x3, ~1e-5 per product: gradients then carry ReLU-flip noise of ~3e-3 relative L2; opt-in);
 *                   0 = the fp32 vector-ALU kernels; 2 = diagnostic (as 1, one channel tile per workgroup)
 *   "clock_probe"   1 = the dominant kernel of the bf16 eval forward (CNN2D block 3) brackets its main loop with s_memtime /
 *                   s_memrealtime stamps (lane 0 of the first 1024 workgroups, into a buffer no kernel reads); dfa_ctx_clock_read
 *                   returns the shader clock the chip held inside that kernel.  0 (default) = two scalar compares per workgroup
 *   "poison_lds"    (action, test hook) fills all 160 KB of LDS of every CU with the 16-bit pattern `value` (0xffff / 0x7fc0 =
 *                   NaN, 0x7f80 = +Inf) on the context's stream.  LDS is not cleared between workgroups; the stale-LDS tests
 *                   (tests/test_lds_poison_gpu.py) run every path after this and require bit-identical results
 * unknown names return DFA_E_UNSUPPORTED */
int dfa_ctx_set_option(dfa_ctx* ctx, const char* name, int value);
/* the value this context holds for an option: *value = what dfa_ctx_set_option stored (a switch set to any non-zero value reads 1),
 * or the default above.  "poison_lds" is an action and holds no value: DFA_E_UNSUPPORTED, as for unknown names */
int dfa_ctx_get_option(const dfa_ctx* ctx, const char* name, int* value);
const char* dfa_last_error(const dfa_ctx* ctx);
const char* dfa_error_name(int code);

/* ---- CNN2D (replaces CNN2D.__init__/forward, src/model.py:12-42) -------------------------------- */
/* params: 20 device pointers (fp32) in state_dict order without num_batches_tracked:
 *   conv.0.{weight,bias}, conv.1.{weight,bias,running_mean,running_var},
 *   conv.5.{weight,bias}, conv.6.{weight,bias,running_mean,running_var},
 *   conv.10.{weight,bias}, conv.11.{weight,bias,running_mean,running_var},
 *   classifier.{weight,bias}
 * The pointers are remembered (not copied); base_channels must be 32. */
#define DFA_CNN2D_NPARAMS 20
int dfa_cnn2d_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int in_features,
                         int base_channels);
/* (re)build the BN-folded, MFMA-ordered weight images for eval-mode forward; call after any weight
 * change (load_state_dict, optimiser step) or precision switch. */
int dfa_cnn2d_prepare(dfa_ctx* ctx, int precision);
/* eval-mode forward: logits[b] = classifier(flatten(mean_T(conv(x[b]))))   (src/model.py:33-42)
 *   x: device, element (b,t,f) at x + b*stride_b + t*stride_t + f*stride_f (strides in elements; the
 *      reference harness passes the transposed view of the stored [B,F,T] tensor, src/predict.py:105);
 *   logits: device float[B]; embedding: device float[B*128*F] in c*F+f order, or NULL
 *      (src/model.py:40-41, src/embedding_anomaly.py:61);
 *   workspace: device, >= dfa_workspace_bytes(ctx, DFA_MODEL_CNN2D, B, T, F, precision) bytes. */
int dfa_cnn2d_forward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                      int64_t stride_t, int64_t stride_f, float* logits, float* embedding,
                      void* workspace, size_t workspace_bytes);
/* eval-mode forward of a variable-length (ragged) batch: utterance b is x[b, :lengths[b], :] and gets exactly the logit
 * (and embedding) dfa_cnn2d_forward gives x[b:b+1, :lengths[b], :] alone, bit for bit.  Replaces scoring a file of
 * uncropped utterances one at a time (src/predict.py:97-110 at --batch-size 1; src/dataloaders.py:63-75).
 *   x: the padded [B, T_max, F] strided view as above; rows t >= lengths[b] are never read (may be uninitialised);
 *   lengths: HOST int32[B], 4 <= lengths[b] <= T_max (else DFA_E_BAD_SHAPE naming the index); validated here and copied
 *      into the workspace on the context's stream;
 *   workspace: device, >= dfa_ragged_workspace_bytes(ctx, DFA_MODEL_CNN2D, B, T_max, F, precision) bytes.
 * Precision bf16 only in this version (blocks 1+2 and block 3 + time mean as two kernels, then the classifier).  A context
 * prepared for fp32 or bf16x3, one with fuse_conv1 = 0 or block3_m16 = 0, or a capturing stream returns DFA_E_UNSUPPORTED
 * (the lengths are copied per call, so the forward cannot be replayed from a graph). */
int dfa_cnn2d_forward_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b,
                             int64_t stride_t, int64_t stride_f, const int32_t* lengths, float* logits,
                             float* embedding, void* workspace, size_t workspace_bytes);

/* eval-mode CNN1D forward of a variable-length (ragged) batch in ONE kernel launch: utterance b is x[b, :lengths[b], :].
 *   x: float32, the padded batch in the stored channel-major layout -- [B][F][T_pad] storage seen as [B, T_max, F]:
 *      stride_t == 1, stride_f % 4 == 0, stride_f >= T_max, stride_b % 4 == 0, base 16-byte aligned, F % 4 == 0
 *      (what dataloaders.RaggedBatcher yields); any other layout or a bf16 x returns DFA_E_UNSUPPORTED / DFA_E_BAD_DTYPE.
 *      Of row f of utterance b only the floats [0, 4 * ceil(lengths[b] / 4)) are read, and those at t >= lengths[b] are
 *      masked before use: padding may be uninitialised, NaN or Inf;
 *   lengths: HOST int32[B], 3 <= lengths[b] <= T_max (else DFA_E_BAD_SHAPE naming the index), no other upper bound:
 *      an utterance longer than one LDS window (348 frames at F = 180) is walked in time segments by its workgroup;
 *   logits: device float[B];
 *   workspace: device, 256-byte aligned, >= dfa_ragged_workspace_bytes(ctx, DFA_MODEL_CNN1D, B, T_max, F, DFA_PREC_F32)
 *      bytes: the per-call table only, no activation leaves the chip.
 * The arithmetic is that of the split-bf16 kernel of dfa_cnn1d_forward (fp32-grade, 1e-4 of the fp32 reference).  An
 * utterance that fits one window gets, bit for bit, the logit dfa_cnn1d_forward gives its own contiguous [F][T_b] tensor;
 * for every length the logit depends on the utterance alone, not on its batch, its position in it or T_max.
 * Option cnn1d_fused != 1 or a capturing stream returns DFA_E_UNSUPPORTED (the lengths are copied per call). */
int dfa_cnn1d_forward_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b,
                             int64_t stride_t, int64_t stride_f, const int32_t* lengths, float* logits,
                             void* workspace, size_t workspace_bytes);
/* the time segments dfa_cnn1d_forward_ragged walks for an utterance of T frames, a function of T and F only: segment i loads
 * the window [starts[i], starts[i] + lens[i]) and adds the layer-3 frames [owned_lo[i], owned_hi[i]) to the frame mean.
 * Fills up to cap entries of each non-NULL array; returns the number of segments (0 when T < 3). */
int dfa_cnn1d_ragged_segments(int T, int F, int* starts, int* lens, int* owned_lo, int* owned_hi, int cap);
/* dynamic LDS bytes of the ragged CNN1D launch for a batch padded to T_max (<= 160 KiB) */
size_t dfa_cnn1d_ragged_lds_bytes(int T_max, int F);
/* The same two for a model whose first Conv1d has k1 taps (dfa_cnn1d_set_kernels).  k1 = 3: exactly the pair above.  k1 = 5:
 * the windows of the k = (5, 3, 3) variant -- owned frames plus 4 frames to either side (3 + 1 for the wider layer 1), or up
 * to the utterance's end; one window spans up to 384 frames at F = 180.  Any other k1: 0. */
int dfa_cnn1d_ragged_segments_k(int T, int F, int k1, int* starts, int* lens, int* owned_lo, int* owned_hi, int cap);
size_t dfa_cnn1d_ragged_lds_bytes_k(int T_max, int F, int k1);
/* the largest T at which dfa_cnn1d_forward runs as ONE launch for the contiguous [B][F][T] storage with k1 taps in layer 1
 * (349 at F = 180, k1 = 3; 384 at k1 = 5, whose layer-1 weights are streamed); 0 for an F or k1 the one-kernel form does not take */
int dfa_cnn1d_fused_max_t(int F, int k1);

/* ---- CNN2D training step (replaces, for src/train.py:71-76, torch autograd over src/model.py:13-39) ------------ */
size_t dfa_cnn2d_train_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F, int precision);
/* The workspace layout of a training step of [B, T, F] in `precision`: the very plan dfa_cnn2d_forward_train, dfa_cnn2d_backward and
 * dfa_cnn2d_train_workspace_bytes read, reported.  Pure host arithmetic; ctx may be NULL (it only receives the refusal's text).
 * Activations are channels-last, [B][H][F][C], of `elem` bytes per element (bf16 or fp32); offsets are bytes from the workspace's
 * start, each 256-byte aligned, in the order below.  After one forward_train + backward every region but raw and partial still
 * holds what the step stored in it.  Fills the first min(cap, DFA_CNN2D_TRAIN_PLAN_FIELDS) of
 *    0 H1, 1 H2    rows of a1 / z2 (T / 2) and of a2 / z3 (H1 / 2)
 *    2 elem        bytes per stored activation element (2 or 4)
 *    3 a1          block 1's pooled (and dropped-out) output            [B][H1][F][32]
 *    4 z2          conv 32 -> 64 pre-BatchNorm output                   [B][H1][F][64]
 *    5 a2          block 2's pooled (and dropped-out) output            [B][H2][F][64]
 *    6 z3          conv 64 -> 128 pre-BatchNorm output                  [B][H2][F][128]
 *    7 emb         mean over time of ReLU(BatchNorm(z3)), the classifier's input      float [B][128][F]
 *    8 demb        its gradient, transposed for the BatchNorm backward               float [B][F][128]
 *    9 msum        per (b, f, c) the two time sums block 3's BatchNorm backward reduces from: n = sum_t mask and
 *                  sx = sum_t mask * xhat, mask = (gamma * xhat + beta > 0), xhat = (z3 - mean) * invstd     float [B][F][128][2]
 *   10 dz3, 11 da2, 12 dz2, 13 da1   gradients, shaped as z3, a2, z2, a1
 *   14 raw         fp32 scratch of the two-launch 64 <- 128 data gradient (written only with option dgrad_m16 = 0 or in fp32)
 *   15 stats       float: per BatchNorm layer mean[C] | biased variance[C] | invstd[C]; the layers (C = 32, 64, 128) follow each
 *                  other, so layer l's block starts 3 * {0, 32, 96}[l] floats in
 *   16 sums        float: per layer the backward's [C][2] records (S1 = sum dy = dbeta, S2 = sum dy * xhat = dgamma) at
 *                  2 * {0, 32, 96}[l] floats (layer 1's only on the two-pass block-1 backward, conv1_bwd_fused = 0 or
 *                  synchronised BatchNorm); at float 448 block 1's backward record: [32][11] = per channel A[9] = sum dy * x_tap,
 *                  S1, S2 on the one-pass paths (the matrix-core pass leaves S2 = 0 and derives it), [32][10] = dW[9], db on the
 *                  two-pass path; at float 800 the tap moments XX[9][9] | Xs[9] of x (one-pass paths only)
 *   17 partial, 18 partial_bytes   the per-workgroup records of every reduction
 *   19 total       = dfa_cnn2d_train_workspace_bytes
 * of `fields` (may be NULL: validate only) and returns DFA_CNN2D_TRAIN_PLAN_FIELDS.  A precision or shape the step refuses returns
 * the step's own error code (negative) and leaves its message in ctx. */
#define DFA_CNN2D_TRAIN_PLAN_FIELDS 20
int dfa_cnn2d_train_plan(dfa_ctx* ctx, int B, int T, int F, int precision, long long* fields, int cap);
/* train-mode forward: BatchNorm uses batch statistics (and updates running_mean/var in place through the pointers
 * given to dfa_cnn2d_set_params when update_running_stats != 0, momentum 0.1 in the reference); Dropout(p_drop) after
 * pools 1 and 2 with a Philox mask keyed by (seed, offset).  Uses the raw parameters directly (no prepare needed).
 * The workspace keeps what dfa_cnn2d_backward needs; it must stay untouched until then. */
int dfa_cnn2d_forward_train(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                            int64_t stride_t, int64_t stride_f, int precision, float p_drop, uint64_t seed,
                            uint64_t offset, float momentum, int update_running_stats, float* logits,
                            float* embedding, void* workspace, size_t workspace_bytes);
/* gradients of the 14 parameters w.r.t. sum_b dlogits[b]*logit[b], written (not accumulated) to grads[0..13] in
 * parameters() order: conv.0.{weight,bias}, conv.1.{weight,bias}, conv.5.*, conv.6.*, conv.10.*, conv.11.*,
 * classifier.{weight,bias}.  Pointing grads[] into ONE flat buffer gives the single all-reduce payload of data-parallel
 * training (464,644 bytes).
 * The rule of all four pairs (CNN2D, CNN1D uniform and ragged, auto-encoder, DeepfakeDetector): dfa_<model>_backward must follow
 * its own forward on the same workspace and shape (else DFA_E_NOT_PREPARED) -- B, T, F (T_max, in_ch), x_dtype and the ragged or
 * uniform form are the forward's.  The forward it follows is the model's LATEST dfa_<model>_forward_train call, and only if that
 * call returned DFA_OK: a forward refused by an argument check, or one that failed, ends the batch that was in flight, and so
 * does dfa_<model>_set_params.  A backward, refused or completed, ends nothing: it may be called again.  The SyncBN hook must be
 * what the forward found: a dfa_ctx_set_bn_sync that armed or cleared it between the two calls is DFA_E_UNSUPPORTED. */
int dfa_cnn2d_backward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                       int64_t stride_t, int64_t stride_f, const float* dlogits, float* const* grads, int ngrads,
                       void* workspace, size_t workspace_bytes);
/* loss = mean(BCEWithLogits(logits, y*(1-eps)+eps/2)), dlogits = dloss/dlogits   (src/train.py:311-320); device ptrs;
 * loss and dlogits may be NULL. */
int dfa_bce_smooth_fwd_bwd(dfa_ctx* ctx, const float* logits, const float* labels, float label_smoothing, int B,
                           float* loss, float* dlogits);
/* train-time feature augmentation in one pass (replaces the torch-op chain of src/augmentation.py:5-186 as composed by
 * src/train.py:68-69 / 271-289): out[b][t][f] = keep_f[f] * mask(x[b][(t - shift) mod T][f]) + jitter_std * N(0,1).
 * The caller draws the per-batch parameters exactly as the reference does (Python `random` spans and shift, torch
 * generator keep mask); mask spans refer to the frames / feature dims BEFORE the shift (the reference's op order:
 * time mask, feature mask, roll, channel drop, jitter); len = 0 disables a mask, keep_f = NULL and jitter_std = 0 disable
 * the other two; the noise is the library's Philox stream keyed by (seed, offset + (b*T + t)*F + f).  Out of place; any strides. */
int dfa_augment_batch(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                      int64_t stride_f, void* out, int out_dtype, int64_t out_stride_b, int64_t out_stride_t,
                      int64_t out_stride_f, int shift, const float* keep_f, int tmask_start, int tmask_len,
                      int fmask_start, int fmask_len, float jitter_std, uint64_t seed, uint64_t offset);
/* The same augmentation FOLDED INTO THE LOADS of the training step (src/train.py:68-69 applies the
 * augmentation to the batch and hands the result to the model): arms the parameters for the NEXT dfa_cnn2d_forward_train /
 * dfa_cnn2d_backward pair, whose three kernels that read x (statistics pass, block 1, block-1 backward) then read
 * keep_f[f] * mask(x[b][(t - shift) mod T][f]) + jitter_std * N(0,1) instead of x -- no augmented copy of the batch is
 * written or re-read.  One-shot: consumed by that forward (also by one that fails its argument checks); enable = 0 disarms.
 * keep_f (device float[F] or NULL) is copied into a context-owned buffer on the stream: the caller's tensor may be released at
 * once.  The element formula, noise stream included, is the one of dfa_augment_batch. */
int dfa_cnn2d_set_train_augment(dfa_ctx* ctx, int enable, int T, int F, int shift, const float* keep_f, int tmask_start,
                                int tmask_len, int fmask_start, int fmask_len, float jitter_std, uint64_t seed,
                                uint64_t offset);
/* The same for the CNN1D (src/train.py:68-69 feeds both classifiers): arms the augmentation for the NEXT dfa_cnn1d_forward_train /
 * dfa_cnn1d_backward pair, whose two kernels that read x (layer-1 convolution, layer-1 weight gradient) read it through the same
 * element formula -- the stand-alone dfa_augment_batch pass (one read + one write of the batch) disappears.  Same one-shot and
 * keep_f rules as dfa_cnn2d_set_train_augment. */
int dfa_cnn1d_set_train_augment(dfa_ctx* ctx, int enable, int T, int F, int shift, const float* keep_f, int tmask_start,
                                int tmask_len, int fmask_start, int fmask_len, float jitter_std, uint64_t seed,
                                uint64_t offset);
/* Synchronised BatchNorm for data-parallel training of all three models (the optional `dfa_bn_stats_{get,set}` pair, as
 * ONE hook): the reference trains on one GPU with plain BatchNorm2d (src/model.py:16,22,28); N ranks x B utterances reproduce one
 * rank x N*B -- statistics, running statistics and gradients, up to summation order -- when every BatchNorm layer's per-channel sums
 * are added over the ranks between their reduction and their use: (sum x, sum x^2) in the forward, (sum dy, sum dy*xhat) in the
 * backward, 2*C floats each, six exchanges per step for the classifiers, fourteen for the auto-encoder.  With a hook set, the
 * forward_train / backward entry points copy those sums into `buf` (caller-owned DEVICE memory, >= 512 floats) and call fn(user, buf, count) on the calling thread; fn enqueues an in-place
 * SUM all-reduce of buf[0 .. count) ordered after the work already on the context's stream (torch.distributed.all_reduce on the
 * tensor that owns buf does) and returns 0.  dgamma / dbeta stay the rank's own sums: the flat-gradient all-reduce adds them.
 * Block 1 of the CNN2D / auto-encoder then runs the two-pass vector backward (the one-pass moment algebra needs the sums too late).
 * fn = NULL: local statistics (torch DistributedDataParallel's default; what dfa_amd.train / train_cae use unless --sync-bn is given).
 * Set it before a forward_train; it stays in force until changed, and a backward whose forward ran under another setting is
 * refused (DFA_E_UNSUPPORTED). */
typedef int (*dfa_bn_sync_fn)(void* user, float* buf, int count);
int dfa_ctx_set_bn_sync(dfa_ctx* ctx, dfa_bn_sync_fn fn, void* user, int world, float* buf, int capacity);
/* one torch.optim.AdamW step over a flat fp32 buffer: p *= 1-lr*wd; m,v update; p -= lr/bc1 * m/(sqrt(v)/sqrt(bc2)+eps).
 * grad_scale multiplies the gradient first (1/world after a sum all-reduce).  step is 1-based. */
int dfa_adamw_step(dfa_ctx* ctx, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale);

/* ---- CNN1D (replaces CNN1D.forward, src/model_cnn1d.py:37-46) -------------------------------------- */
/* params: 20 device pointers (fp32) in state_dict order without num_batches_tracked:
 *   conv.0.{weight,bias}, conv.1.{weight,bias,running_mean,running_var}, conv.4.*, conv.5.*, conv.8.*, conv.9.*,
 *   classifier.{weight,bias}.   base_channels must be 32; in_features is the Conv1d input-channel count. */
#define DFA_CNN1D_NPARAMS 20
int dfa_cnn1d_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int in_features,
                         int base_channels);
int dfa_cnn1d_prepare(dfa_ctx* ctx);
/* Kernel sizes of the three Conv1d layers that the NEXT dfa_cnn1d_set_params binds: (3, 3, 3) -- the default, src/model_cnn1d.py --
 * or (5, 3, 3), the reference's CNN1D_Variant (src/compare_kernels.py:38-67: conv.0.weight is [32][in_features][5], padding 2).
 * Sticky on the context.  Like dfa_cnn1d_set_params it ends a training batch in flight and clears what dfa_cnn1d_prepare built;
 * a call that CHANGES k1 also unbinds the parameters (conv.0.weight has the other shape): call dfa_cnn1d_set_params again.
 * Anything but the two sets returns DFA_E_UNSUPPORTED with a message and changes nothing.
 * CAUTION: dfa_cnn1d_set_params cannot see the shape of the tensors it is given.  The caller must have set the kernels the bound
 * conv.0.weight has -- binding a [32][F][3] weight on a context left at (5, 3, 3) makes dfa_cnn1d_prepare and the training step
 * read past its end.  Call dfa_cnn1d_set_kernels in front of every dfa_cnn1d_set_params when one context serves both models.
 * With (5, 3, 3): dfa_cnn1d_forward and dfa_cnn1d_forward_ragged work as documented (one launch for the layouts the three-tap
 * model takes in one launch); dfa_cnn1d_forward_train / dfa_cnn1d_backward run the uniform step (layer 1: a five-tap
 * convolution and a [32][F][5] weight gradient, on the matrix cores or the fp32 kernels as cnn1d_train_x3 says), and
 * dfa_cnn1d_train_workspace_bytes / dfa_cnn1d_train_plan size `partial` for it; dfa_cnn1d_forward_train_ragged and
 * dfa_cnn1d_train_plan(ragged) return DFA_E_UNSUPPORTED with a message before anything is launched, and
 * dfa_cnn1d_train_ragged_workspace_bytes returns 0. */
int dfa_cnn1d_set_kernels(dfa_ctx* ctx, int k1, int k2, int k3);
/* eval-mode forward, fp32 arithmetic.  x as in dfa_cnn2d_forward (fp32 only); logits: device float[B]. */
int dfa_cnn1d_forward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                      int64_t stride_t, int64_t stride_f, float* logits, void* workspace,
                      size_t workspace_bytes);

/* CNN1D training step (fp32): same contract as the CNN2D pair above; dropout follows ReLU in blocks 1 and 2
 * (src/model_cnn1d.py:20,26); grads[0..13] in parameters() order conv.0.*, conv.1.*, conv.4.*, conv.5.*, conv.8.*, conv.9.*,
 * classifier.*. */
size_t dfa_cnn1d_train_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F);
int dfa_cnn1d_forward_train(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                            int64_t stride_t, int64_t stride_f, float p_drop, uint64_t seed, uint64_t offset,
                            float momentum, int update_running_stats, float* logits, void* workspace,
                            size_t workspace_bytes);
int dfa_cnn1d_backward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                       int64_t stride_t, int64_t stride_f, const float* dlogits, float* const* grads, int ngrads,
                       void* workspace, size_t workspace_bytes);

/* CNN1D training step on a variable-length (ragged) batch: x is the batch padded to T_max frames, utterance b is
 * x[b, :lengths[b], :] with 3 <= lengths[b] <= T_max (lengths: HOST int32[B], validated here: DFA_E_BAD_SHAPE names the index).
 * The step is the reference model's on the utterances concatenated along time: every Conv1d zero-pads an utterance at its own two
 * ends, each BatchNorm1d takes its batch statistics over the N = sum lengths[b] valid frames (biased variance to normalise, the
 * N / (N - 1) correction in the running variance, momentum as above), the time mean of utterance b runs over its own frames.
 * Frames t >= lengths[b] of x are never used: they may hold anything, NaN and Inf included.  With every length equal to T_max the
 * pair computes the uniform pair's results bit for bit.
 *   workspace: dfa_cnn1d_train_ragged_workspace_bytes (the uniform plan at T_max plus the per-call table).  The backward reads the
 *   table the forward left there, so it takes no lengths; the pairs do not mix: dfa_cnn1d_backward after a ragged forward, and
 *   dfa_cnn1d_backward_ragged after a uniform one, return DFA_E_NOT_PREPARED.
 *   DFA_E_UNSUPPORTED: a capturing stream (the lengths are copied per call), an armed dfa_cnn1d_set_train_augment (a time roll has no
 *   per-utterance meaning), an armed dfa_ctx_set_bn_sync (the ranks' frame counts differ, the hook carries sums only).
 * Everything else -- dtype (float32), strides, option cnn1d_train_x3, dropout, running statistics, gradients -- as in the
 * uniform pair. */
size_t dfa_cnn1d_train_ragged_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int F);
/* The workspace layout of a CNN1D training step of [B, T, F] (ragged != 0: of a ragged batch padded to T = T_max): the very plan
 * the forward_train / backward pairs and the two *_workspace_bytes functions read, reported.  Pure host arithmetic; ctx may be NULL
 * (it only receives the refusal's text).  Everything is float, channel-major [B][C][T] with C = 32, 64, 128 for layers 1-3; offsets
 * are bytes from the workspace's start, each 256-byte aligned, in the order below.  After one forward_train + backward every region
 * but partial still holds what the step stored in it.  Fills the first min(cap, DFA_CNN1D_TRAIN_PLAN_FIELDS) of
 *    0-2  z[3]      the Conv1d outputs in front of BatchNorm                        [B][C_l][T]
 *    3-4  h[2]      dropout(ReLU(BatchNorm(z))) of layers 1 and 2                    [B][C_l][T]
 *    5    pooled    the time mean of ReLU(BatchNorm(z[2])), the classifier's input   [B][128]
 *    6    dpooled   its gradient                                                    [B][128]
 *    7-9  dz[3]     the gradients of z                                              [B][C_l][T]
 *   10-11 dh[2]     the gradients of h                                              [B][C_l][T]
 *   12    stats     per BatchNorm layer mean[C] | biased variance[C] | invstd[C]; layer l's block starts 3 * {0, 32, 96}[l] floats in
 *   13    sums      per layer the backward's [C][2] records (S1 = sum dy = dbeta, S2 = sum dy * xhat = dgamma) at 2 * {0, 32, 96}[l]
 *   14 partial, 15 partial_bytes   the per-chunk records of every reduction
 *   16    lengths   where the forward leaves the ragged batch's table (int32[B] lengths, then int32[B] unused); -1 when ragged == 0
 *   17    total     = dfa_cnn1d_train_workspace_bytes, or dfa_cnn1d_train_ragged_workspace_bytes when ragged != 0
 * of `fields` (may be NULL: validate only) and returns DFA_CNN1D_TRAIN_PLAN_FIELDS.  At a padding frame t >= lengths[b] of a ragged
 * batch h and dz hold exact zeros; z and dh hold whatever the uniform convolution makes of its zero-padded neighbours (finite, read
 * by nothing).  A shape the step refuses returns the step's own error code (negative) and leaves its message in ctx. */
#define DFA_CNN1D_TRAIN_PLAN_FIELDS 18
int dfa_cnn1d_train_plan(dfa_ctx* ctx, int B, int T, int F, int ragged, long long* fields, int cap);
int dfa_cnn1d_forward_train_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b,
                                   int64_t stride_t, int64_t stride_f, const int32_t* lengths, float p_drop, uint64_t seed,
                                   uint64_t offset, float momentum, int update_running_stats, float* logits, void* workspace,
                                   size_t workspace_bytes);
int dfa_cnn1d_backward_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b,
                              int64_t stride_t, int64_t stride_f, const float* dlogits, float* const* grads, int ngrads,
                              void* workspace, size_t workspace_bytes);

/* ---- ConvAutoencoder (replaces ConvAutoencoder.forward, src/model_cae.py:83-125, and the per-sample MSE of
 *      src/evaluation_cae.py:52-53 / src/hybrid_ensemble.py:55) ------------------------------------------------ */
/* params: 44 device pointers (fp32) in state_dict order without num_batches_tracked:
 *   encoder.{0,4,8,12}.{weight,bias} each followed by encoder.{1,5,9,13}.{weight,bias,running_mean,running_var};
 *   decoder.{0,3,6}.{weight,bias} each followed by decoder.{1,4,7}.{weight,bias,running_mean,running_var};
 *   decoder.9.{weight,bias}.   ConvTranspose2d weights keep torch's (Cin, Cout, 2, 2) layout.  base_channels = 32. */
#define DFA_CAE_NPARAMS 44
int dfa_cae_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int base_channels);
int dfa_cae_prepare(dfa_ctx* ctx, int precision);
/* eval-mode forward.  x as in dfa_cnn2d_forward; T >= 16; F must satisfy F == 16*(F/16) + 4 (180 does), because
 * the decoder's output_padding=(0,1) is fixed (src/model_cae.py:68-69).
 *   mu, sigma: device float[F] or both NULL.  When given, the FeatureNormalizer z-score (x - mu[f]) / sigma[f]
 *              (src/dataset_cae.py:37-41) is fused into every read of x, i.e. x is the RAW feature tensor;
 *   recon:  device float[B*T*F] or NULL  -- reconstruction, rows >= 16*(T/16) are zero (model_cae.py:116-119);
 *   latent: device float[B*256*(T/16)*(F/16)] (NCHW) or NULL;
 *   mse:    device float[B] or NULL      -- mean over T*F of (recon - x_normalised)^2. */
int dfa_cae_forward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                    int64_t stride_t, int64_t stride_f, const float* mu, const float* sigma, float* recon,
                    float* latent, float* mse, void* workspace, size_t workspace_bytes);

/* ConvAutoencoder training step (replaces, for src/train_cae.py:58-82, torch autograd over src/model_cae.py:32-125).
 * forward_train: x is the (already z-scored) input; BatchNorm uses batch statistics and updates the running statistics
 * in place when update_running_stats != 0; recon, latent and mse may each be NULL (at least one of recon / mse is required;
 * mean_b mse[b] is MSELoss(recon, x) of src/train_cae.py:67-68, every sample having T*F elements).
 * backward: drecon = d(loss)/d(reconstruction), device float[B*T*F] -- or NULL for the reference's own loss,
 * MSELoss(recon, x) (src/train_cae.py:67-68,203): its gradient 2*(recon-x)/(B*T*F) is then formed INSIDE the decoder's last
 * backward kernel from the saved activations and x, so neither the reconstruction nor its gradient has to exist in memory.
 * Gradients of the 30 parameters are written to grads[] in parameters() order: encoder.{0,1,4,5,8,9,12,13}.{weight,bias},
 * decoder.{0,1,3,4,6,7}.{weight,bias}, decoder.9.{weight,bias}; pointing grads[] into ONE flat buffer gives the single
 * all-reduce payload of data-parallel training (2,246,532 bytes). */
size_t dfa_cae_train_workspace_bytes(const dfa_ctx* ctx, int B, int T, int F, int precision);
int dfa_cae_forward_train(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                          int64_t stride_t, int64_t stride_f, int precision, float momentum,
                          int update_running_stats, float* recon, float* latent, float* mse, void* workspace,
                          size_t workspace_bytes);
int dfa_cae_backward(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b, int64_t stride_t,
                     int64_t stride_f, const float* drecon, float* const* grads, int ngrads, void* workspace,
                     size_t workspace_bytes);
/* The workspace layout of a training step of [B, T, F] in `precision`: the very plan dfa_cae_forward_train, dfa_cae_backward and
 * dfa_cae_train_workspace_bytes read, reported.  Pure host arithmetic; ctx may be NULL (it only receives the refusal's text).
 * Every activation is channels-last, [B][H][W][C], of `elem` bytes per element (bf16 or fp32); offsets are bytes from the
 * workspace's start.  After one forward_train + backward every region below still holds what the step stored in it.
 * Fills the first min(cap, DFA_CAE_TRAIN_PLAN_FIELDS) of
 *    0-4   H[0..4]      rows of x and of the pooled encoder outputs e[0..3] (H[l+1] = H[l] / 2)
 *    5-9   W[0..4]      their columns
 *   10-13  Hd[0..3]     rows of the decoder outputs d[0..2] and of the uncropped reconstruction
 *   14-17  Wd[0..3]     their columns (Wd[1] includes the output_padding column)
 *   18-21  e[0..3]      pooled encoder outputs                         [B][H[l+1]][W[l+1]][32 << l]
 *   22-25  z[0..3]      encoder pre-BatchNorm outputs, z[0] = -1 (block 1's is recomputed, never stored)   [B][H[l]][W[l]][32 << l]
 *   26-28  zd[0..2]     decoder pre-BatchNorm outputs                  [B][Hd[l]][Wd[l]][128 >> l]
 *   29-31  d[0..2]      decoder block outputs                          as zd
 *   32-34  dd[0..2]     gradients of d                                 as zd
 *   35-37  dzd[0..2]    gradients of zd (written only with option cae_bwd_fold = 0)   as zd
 *   38-41  de[0..3]     gradients of e                                 as e
 *   42-45  dz[0..3]     gradients of z, dz[0] = -1                     as z
 *   46 zp               the ConvTranspose2d gradient GEMMs' patch-major dzd: [B * Hd[l]/2 * Win][2][2][Cout], rewritten per layer
 *   47 xf, 48 raw       fp32 scratch of the fp32 GEMM path / of the split convolutions
 *   49 stats, 50 sums   the BatchNorm statistics block and the backward's (sum dy, sum dy * xhat) block
 *   51 wq, 52 dwq       ConvTranspose2d weights / weight gradients as [Cin][4 Cout] matrices
 *   53 rec              decoder block 4's and encoder block 1's gradient records
 *   54 partial, 55 partial_bytes   the per-workgroup records of every reduction
 *   56 total            = dfa_cae_train_workspace_bytes
 *   57 elem             bytes per stored activation element (2 or 4)
 *   58-64  C[0..6]      channels of the seven BatchNorm layers in the order encoder.{1,5,9,13}, decoder.{1,4,7}
 *   65-71  mean[0..6]   byte offset of each layer's float[C] batch mean
 *   72-78  var[0..6]    ... of its biased batch variance
 *   79-85  invstd[0..6] ... of its 1 / sqrt(var + 1e-5)
 * of `fields` (may be NULL) and returns DFA_CAE_TRAIN_PLAN_FIELDS.  A precision or shape the step refuses returns the step's own
 * error code (negative) and leaves its message in ctx. */
#define DFA_CAE_TRAIN_PLAN_FIELDS 86
int dfa_cae_train_plan(dfa_ctx* ctx, int B, int T, int F, int precision, long long* fields, int cap);

/* anomaly scores of a variable-length (ragged) batch in five launches: utterance b is x[b, :lengths[b], :] and mse[b] is, bit for
 * bit, the mse dfa_cae_forward gives x[b:b+1, :lengths[b], :] alone (layer heights T_b/2, T_b/4, T_b/8, T_b/16, zero
 * reconstruction rows t >= 16 (T_b/16), divisor T_b * F; src/model_cae.py:107-125, src/evaluation_cae.py:52-53) -- whatever
 * B, T_max, the utterance's position in the batch or the dispatch order.  Replaces one dfa_cae_forward per uncropped utterance.
 *   x: the padded [B, T_max, F] strided view, float32 or bf16; rows t >= lengths[b] are never read (may hold NaN);
 *   lengths: HOST int32[B], 16 <= lengths[b] <= T_max (else DFA_E_BAD_SHAPE naming the index); copied into the workspace on the
 *      context's stream;
 *   mu, sigma: the fused z-score as in dfa_cae_forward, or both NULL;  mse: device float[B];
 *   workspace: device, 256-byte aligned, >= dfa_cae_ragged_workspace_bytes(ctx, B, T_max, F, DFA_PREC_BF16) bytes; rows past an
 *      utterance's own height are never read in any activation, so it may hold stale data.
 * Score only: no reconstruction, no latent export, no train mode.  Precision bf16 with the default kernel options only:
 * a context prepared for fp32, one with cae_dec_fused = 0, cae_enc1_mfma = 0, cae_enc_dma = 0 or lds_pipe = 0 (the uniform
 * forward would run other kernels), an input the fused decoder does not take (32-bit offsets inside an utterance,
 * non-negative strides) or F > 1022, or a capturing stream returns DFA_E_UNSUPPORTED. */
int dfa_cae_score_ragged(dfa_ctx* ctx, const void* x, int x_dtype, int B, int T_max, int F, int64_t stride_b, int64_t stride_t,
                         int64_t stride_f, const int32_t* lengths, const float* mu, const float* sigma, float* mse,
                         void* workspace, size_t workspace_bytes);

/* MSELoss(recon, x) forward + backward in one pass (replaces nn.MSELoss + its autograd node, src/train_cae.py:67-68,203):
 * loss[0] = mean((recon - x)^2) over B*T*F elements (fixed-order two-stage reduction), drecon = 2*(recon - x)/(B*T*F).
 * recon: device float[B*T*F] contiguous; x: as in dfa_cae_forward (dtype + element strides); loss / drecon: device, either may be
 * NULL.  For callers that keep an explicit reconstruction; the native trainer uses dfa_cae_backward(drecon = NULL) instead. */
int dfa_mse_fwd_bwd(dfa_ctx* ctx, const float* recon, const void* x, int x_dtype, int B, int T, int F, int64_t stride_b,
                    int64_t stride_t, int64_t stride_f, float* loss, float* drecon);

/* ---- DeepfakeDetector (replaces DeepfakeDetector.forward in eval mode, src/dlqueen_model.py:115-173) ------------------------
 * Conv1d(C -> 256, k5) + BN + GELU, 2 x (Conv1d(256 -> 256, k3) + BN + GELU), masked mean / std pool over each utterance's own
 * frames, Linear(512 -> 256) + GELU + Linear(256 -> 1).  Variable-length batches only (the model takes `lengths` by definition).
 * params: 22 device pointers (fp32) in state_dict order without num_batches_tracked:
 *   enc.net.0.{weight,bias}, enc.net.1.{weight,bias,running_mean,running_var}, enc.net.4.*, enc.net.5.*, enc.net.8.*, enc.net.9.*,
 *   head.0.{weight,bias}, head.3.{weight,bias}.
 * hidden must be 256, in_ch a multiple of 4 in [4, 256]: anything else returns DFA_E_UNSUPPORTED. */
#define DFA_DLQ_NPARAMS 22
#define DFA_DLQ_TILE_FRAMES 64 /* frames of one utterance a workgroup owns */
int dfa_dlq_set_params(dfa_ctx* ctx, const float* const* device_params, int n, int in_ch, int hidden);
/* folds every BatchNorm into its convolution and packs hi + lo bf16 matrix-core images (once per weight set) */
int dfa_dlq_prepare(dfa_ctx* ctx);
/* bytes of workspace for B utterances padded to T_max frames (a multiple of 256; 0 for B < 1 or T_max < 1) */
size_t dfa_dlq_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int in_ch);
/* x: device float32, element (b, c, t) at x + b stride_b + c stride_c + t (time fastest: the stored [C, T] layout of a features.pkl
 *    row, padded to the batch's longest utterance); x 16-byte aligned, stride_c % 4 == 0, stride_c >= T_max, stride_b % 4 == 0,
 *    every row readable up to T_max rounded up to 4 frames (else DFA_E_UNSUPPORTED).
 * lengths: HOST int32[B], 1 <= lengths[b] <= T_max (else DFA_E_BAD_SHAPE naming the index).
 * The padded-batch rule: the reference's encoder is not masked, only its pool is.  Frames t >= lengths[b] of x are taken as zero
 * and never used (they may hold NaN); layer 1's output exists on frames < min(T_max, len + 2), layer 2's on frames
 * < min(T_max, len + 1), layer 3's on frames < len; everything past those is the convolution's zero padding.  logits[b] is, bit for
 * bit, a function of (x[b, :, :len], len, min(T_max - len, 2)): not of B, the position in the batch, the other utterances, the
 * memory behind the padding or the workspace's previous contents.
 * logits: device float[B]; pooled: device float[B * 512] ([mean 256 | std 256]) or NULL.
 * workspace: device, 256-byte aligned, >= dfa_dlq_workspace_bytes bytes.  A capturing stream returns DFA_E_UNSUPPORTED (the
 * lengths are copied per call).  Timing slots: 4, 5, 6 = layers 1-3, 7 = pool + head. */
int dfa_dlq_forward(dfa_ctx* ctx, const void* x, int B, int T_max, int in_ch, int64_t stride_b, int64_t stride_c,
                    const int32_t* lengths, float* logits, float* pooled, void* workspace, size_t workspace_bytes);

/* ---- DeepfakeDetector training step (src/dlqueen_model.py:255-330 without AMP: everything is fp32-grade, GradScaler / autocast have
 * no counterpart).  The step is DENSE over the padded batch, as the reference's is: the encoder runs on all T_max frames of every
 * utterance (x at t >= lengths[b] taken as zero by a select, never used), BatchNorm1d's batch statistics count all N = B * T_max
 * frames, padding included, and only the pool is masked.  The step therefore DEPENDS on the batch's composition and on T_max; the
 * "function of the utterance alone" promise of dfa_dlq_forward is an eval promise only.  Dropout (p_drop) follows each encoder GELU
 * and the head's; the keep factor of an element is a function of (seed, offset, layer, index) and is regenerated by the backward.
 * Raw parameters from dfa_dlq_set_params are used (no prepare); running statistics are updated in place (momentum, unbiased
 * variance N / (N - 1)) when update_running_stats != 0; num_batches_tracked is the caller's.
 * x, strides, lengths, workspace alignment: as dfa_dlq_forward.  B * T_max < 2 returns DFA_E_BAD_SHAPE (one value per channel).
 * keep_out: test hook, NULL in production: device uint8[3 * B * 256 * T_max + B * 256], the keep bits the kernels applied, layers
 *   1-3 as [B][T_max][256], then the head's [B][256] (layer 3's are drawn for every frame; the pool uses those of frames < len).
 * An armed dfa_ctx_set_bn_sync hook returns DFA_E_UNSUPPORTED (single rank in this version), a capturing stream too.
 * dfa_dlq_backward must follow its own forward on the same workspace and shape (else DFA_E_NOT_PREPARED); it WRITES the 16
 *   gradients in parameters() order: enc.net.{0,1,4,5,8,9}.{weight,bias}, head.{0,3}.{weight,bias}.  The conv-bias gradients in
 *   front of a BatchNorm are mathematically zero: the rounding noise of the sums is returned.
 * No atomics: every reduction is per-workgroup records and a fixed-order second stage, so a step is bit-reproducible.
 * Timing slots: 8 = weight images, 9 = forward convolutions, 10 = BatchNorm statistics / activation passes / pool + head,
 *   11 = backward head, pool and BatchNorm passes, 12 = data gradients, 13 = weight gradients. */
size_t dfa_dlq_train_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int in_ch);
int dfa_dlq_forward_train(dfa_ctx* ctx, const void* x, int B, int T_max, int in_ch, int64_t stride_b, int64_t stride_c,
                          const int32_t* lengths, float p_drop, uint64_t seed, uint64_t offset, float momentum,
                          int update_running_stats, float* logits, uint8_t* keep_out, void* workspace, size_t workspace_bytes);
int dfa_dlq_backward(dfa_ctx* ctx, const void* x, int B, int T_max, int in_ch, int64_t stride_b, int64_t stride_c,
                     const float* dlogits, float* const* grads, int ngrads /* 16 */, void* workspace, size_t workspace_bytes);
/* ---- DeepfakeDetector batches from a resident set.  The whole training or dev set lives in ONE device
 * float32 buffer `set` of set_floats floats: utterance i of [C][T_i], time fastest, is C rows of pitch_i = ceil(T_i / 4) * 4 floats
 * from float offset off_i, a multiple of 4 (a 16-byte aligned base makes every row 16-byte aligned).  The floats T_i .. pitch_i of a
 * row are unspecified.  One launch assembles the batch x[B][C][T_pad], T_pad = ceil(T_max / 4) * 4, element (b, c, t) at
 * x + b stride_b + c stride_c + t, from B utterances of the set, optionally SpecAugmented:
 *   x[b][c][t] = (t < lengths[b] and t in no time span of b and c in no channel span of b) ? set[src_off[b] + c pitch_b + t] : +0.0f
 * for every t < T_pad.  It is a select, never a multiply: NaN or Inf inside a masked span, behind lengths[b] or in a row's padding
 * floats gives an exact +0.0.  Every float of [b][c][0, T_pad) is written (no memset needed), no other float of x is.
 * src_off: HOST int64[B]; lengths: HOST int32[B], each in [1, T_max]; spans: HOST int32[B][n_tmask + n_fmask][2] = (start, width),
 *   the n_tmask time spans of an utterance first, then its n_fmask channel spans, half-open [start, start + width), width 0 masks
 *   nothing; NULL when both counts are 0.  At most 16 spans per utterance (else DFA_E_UNSUPPORTED).
 * DFA_E_BAD_SHAPE, naming the index: B, C or T_max < 1; lengths[b] outside [1, T_max]; src_off[b] negative, not a multiple of 4 or
 *   with src_off[b] + C pitch_b > set_floats; a time span with start < 0, width < 0 or start + width > lengths[b]; a channel span
 *   that leaves [0, C]; x not 16-byte aligned; stride_c or stride_b not a multiple of 4, stride_c < T_pad, or (B > 1) stride_b <
 *   (C - 1) stride_c + T_pad.
 * workspace: device, 256-byte aligned, >= the bytes the planner below returns (the per-call table; 0 for B < 1 or more than 16
 *   spans), else DFA_E_WORKSPACE.  The table goes through the context's pinned staging slots; the launch is on the context's
 *   stream.  A capturing stream returns DFA_E_UNSUPPORTED (the table is per-call data).  Timing slot: 14. */
size_t dfa_dlq_gather_workspace_bytes(int B, int n_tmask, int n_fmask);
int dfa_dlq_gather_batch(dfa_ctx* ctx, const float* set, int64_t set_floats, const int64_t* src_off, const int32_t* lengths,
                         const int32_t* spans, int n_tmask, int n_fmask, int B, int T_max, int C, float* x, int64_t stride_b,
                         int64_t stride_c, void* workspace, size_t workspace_bytes);
/* loss = mean_b -[pos_weight y log sigmoid(l) + (1 - y) log sigmoid(-l)] (BCEWithLogitsLoss(pos_weight), mean reduction);
 * dlogits = (sigmoid(l) (1 + (pos_weight - 1) y) - pos_weight y) / B.  loss: device float[1] or NULL; dlogits: device float[B] or NULL */
int dfa_bce_pos_weight_fwd_bwd(dfa_ctx* ctx, const float* logits, const float* labels, float pos_weight, int B, float* loss,
                               float* dlogits);
/* torch.nn.utils.clip_grad_norm_ on one flat buffer, on the device with no host synchronisation: a two-stage fixed-order L2 norm,
 * then grad *= min(1, max_norm / (norm + 1e-6)).  norm_out: device float[1] (the norm before clipping) or NULL. */
int dfa_clip_grad_norm(dfa_ctx* ctx, float* grad, size_t n, float max_norm, float* norm_out);

/* ---- per-utterance feature normalisation (src/compare_normalization.py:53-62, src/compare_kernels.py:83-90; DESIGN.md section
 * 3.17).  For utterance b, feature row c and its own n = lengths[b] frames (n = T_max for every b when lengths is NULL):
 *   mean = (1/n) sum_{t<n} x[b][c][t]
 *   DFA_NORM_CMN :  y = x - mean
 *   DFA_NORM_CVMN:  y = (x - mean) / max(sqrt(sum_{t<n} (x - mean)^2 / (n - 1)), 1e-8)        (torch.std: unbiased)
 *   y[b][c][t] = +0.0f for n <= t < T_max: a select, x there (NaN included) is never used.
 * x, y: device float32 with the SAME strides, element (b, t, c) at b stride_b + t stride_t + c stride_c; y == x is allowed, any
 * other overlap is the caller's error.  Two layout forms:
 *   time fastest (stride_t == 1): the stored [B][C][T_pad] batch.  x and y 16-byte aligned, stride_c % 4 == 0, stride_c >= T_max,
 *     stride_b % 4 == 0, stride_b >= 0.  The whole 16-byte pieces of a row are read and written: floats [0, ceil(T_max / 4) * 4) of
 *     every row of y are written (those behind n as +0.0f).  A row of at most DFA_UTT_NORM_HELD_FRAMES frames is read once.
 *   feature fastest (stride_c == 1, stride_t != 1): a [B, T, F] tensor.  stride_t >= C, stride_b >= 0; frames [0, T_max) of the C
 *     features are written, nothing else.
 * The statistics are two-pass float64 sums in a fixed order that depends on n alone (no atomics): within one layout form a row's
 * output is bit for bit a function of its n values, n and the mode -- not of B, b, T_max, the strides, its companions, what lies
 * behind n, or whether the call is in place.
 * lengths: HOST int32[B] or NULL.  With lengths the table goes through the context's pinned staging slots, so a capturing stream
 *   returns DFA_E_UNSUPPORTED; with NULL nothing is copied and the call may be captured.
 * workspace: device, 256-byte aligned, >= dfa_utt_norm_workspace_bytes(B) (0 for B < 1), else DFA_E_WORKSPACE.
 * Refusals, in this order, each with a message and before anything is launched: unknown mode DFA_E_UNSUPPORTED; B, C or T_max < 1
 *   DFA_E_BAD_SHAPE; a length outside [1, T_max], or < 2 with DFA_NORM_CVMN (T_max < 2 without lengths), DFA_E_BAD_SHAPE; neither
 *   stride_t == 1 nor stride_c == 1, or a misaligned base or pitch, DFA_E_UNSUPPORTED; the workspace.  Timing slot: 15.
 *
 * dfa_utt_norm_packed: the same, in place, on a packed resident set (dfa_dlq_gather_batch above: utterance i = C rows of pitch_i =
 *   ceil(T_i / 4) * 4 floats from float offset offsets[i]); the floats T_i .. pitch_i of a row become +0.0f.  offsets: HOST
 *   int64[N], lengths: HOST int32[N] (both required), checked as dfa_dlq_gather_batch checks src_off.  At most
 *   DFA_UTT_NORM_MAX_PACKED utterances per call (else DFA_E_UNSUPPORTED): callers walk a larger set in chunks.  Bit for bit the
 *   time-fastest form of dfa_utt_norm on the same utterance.  workspace: >= dfa_utt_norm_workspace_bytes(N). */
#define DFA_NORM_CMN 1
#define DFA_NORM_CVMN 2
#define DFA_UTT_NORM_HELD_FRAMES 1024
#define DFA_UTT_NORM_MAX_PACKED 65536
size_t dfa_utt_norm_workspace_bytes(int B);
int dfa_utt_norm(dfa_ctx* ctx, int mode, const float* x, float* y, int B, int T_max, int C, int64_t stride_b, int64_t stride_t,
                 int64_t stride_c, const int32_t* lengths, void* workspace, size_t workspace_bytes);
int dfa_utt_norm_packed(dfa_ctx* ctx, int mode, float* set, int64_t set_floats, const int64_t* offsets, const int32_t* lengths, int N,
                        int C, void* workspace, size_t workspace_bytes);

/* ---- embedding anomaly detectors (replace the scoring half of src/embedding_anomaly.py:129-163) ---------
 * The reference fits a StandardScaler, a OneClassSVM and a PCA + GaussianMixture on the bonafide CNN2D embeddings with sklearn
 * (a one-off on the host: dfa_amd/embedding_anomaly.py does the same) and scores with decision_function / score_samples.
 * Here a fitted detector is plain fp32 device arrays, and the scores are computed from the embedding rows where
 * dfa_cnn2d_forward[_ragged] left them: emb[n] = emb + n stride_n, D = 128 * F floats each.  The scaler is applied as the rows are
 * staged (x~ = (x - mean) inv_scale, inv_scale = 1 / scale_ with sklearn's scale_ = 1 on a zero-variance column); every product
 * runs on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32).  No atomics: the reduction over D is split by a rule of D and the
 * column count alone and summed in that order, so out[n] is bit for bit a function of row n -- the same scored alone, in any
 * batch, at any position, in any run.
 *
 * dfa_emb_ocsvm_bind (OneClassSVM(kernel="rbf").decision_function, :136-140): sv[n_sv][D] = support_vectors_ (already scaled),
 *   dual_coef[n_sv] = dual_coef_[0], gamma = _gamma, intercept = intercept_[0];
 *   out[n] = sum_i dual_coef[i] exp(-gamma |x~_n - sv_i|^2) + intercept, the distance as |x~|^2 + |sv|^2 - 2 x~ . sv.
 * dfa_emb_gmm_bind (PCA.transform + GaussianMixture("full").score_samples, :147-161): pca_mean[D] = mean_, components[P][D] =
 *   components_, means[K][P] = means_, prec_chol[K][P][P] = precisions_cholesky_, log_const[K] = sum log diag(prec_chol[k]) +
 *   log weights_[k] - P log(2 pi) / 2;
 *   z = (x~ - pca_mean) components^T, y_k = (z - means[k]) prec_chol[k], out[n] = logsumexp_k(-|y_k|^2 / 2 + log_const[k]).
 * Both remember the pointers (not copied) and build an image the context owns (|sv_i|^2; prec_chol transposed and the means,
 * zero-padded) on the context's stream: bind again when an array moves or changes; dfa_ctx_destroy frees the images.  One
 * detector of each kind per context.  DFA_E_BAD_SHAPE: D not 128 * F with F >= 1, n_sv < 1, P outside [1, DFA_EMB_MAX_P], K
 * outside [1, DFA_EMB_MAX_K]; DFA_E_NULL_PTR names the array; DFA_E_UNSUPPORTED: gamma <= 0, mean / inv_scale / sv / dual_coef /
 * pca_mean / components not 16-byte aligned, a capturing stream (the image is allocated).  A refused bind leaves that detector
 * unbound.
 *
 * dfa_emb_ocsvm_score / dfa_emb_gmm_score: emb device fp32, 16-byte aligned, stride_n >= D and a multiple of 4; out device
 * float[N]; workspace device, 256-byte aligned, >= dfa_emb_workspace_bytes(detector, N, D, M, K) with M = n_sv (K ignored) or
 * M = P (the planner returns 0 for a shape the calls refuse).  Nothing is copied per call: both may be captured.  Two launches
 * (OC-SVM), four (GMM: one product for all K components).  DFA_E_NOT_PREPARED: no successful bind; DFA_E_BAD_SHAPE: N < 1, D not
 * the bound D, stride_n < D; DFA_E_WORKSPACE: a short or misaligned workspace; DFA_E_NULL_PTR names emb, out or workspace. */
#define DFA_EMB_OCSVM 0
#define DFA_EMB_GMM 1
#define DFA_EMB_MAX_P 256
#define DFA_EMB_MAX_K 64
int dfa_emb_ocsvm_bind(dfa_ctx* ctx, int D, int n_sv, const float* mean, const float* inv_scale, const float* sv, const float* dual_coef,
                       float gamma, float intercept);
int dfa_emb_gmm_bind(dfa_ctx* ctx, int D, int P, int K, const float* mean, const float* inv_scale, const float* pca_mean,
                     const float* components, const float* means, const float* prec_chol, const float* log_const);
size_t dfa_emb_workspace_bytes(int detector, int N, int D, int M, int K);
int dfa_emb_ocsvm_score(dfa_ctx* ctx, const float* emb, int N, int D, int64_t stride_n, float* out, void* workspace,
                        size_t workspace_bytes);
int dfa_emb_gmm_score(dfa_ctx* ctx, const float* emb, int N, int D, int64_t stride_n, float* out, void* workspace,
                      size_t workspace_bytes);

/* ---- shared ------------------------------------------------------------------------------------ */
size_t dfa_workspace_bytes(const dfa_ctx* ctx, int model, int B, int T, int F, int precision);
/* workspace of dfa_cnn2d_forward_ragged / dfa_cnn1d_forward_ragged for B utterances padded to T_max frames (0 for a model
 * without a ragged forward) */
size_t dfa_ragged_workspace_bytes(const dfa_ctx* ctx, int model, int B, int T_max, int F, int precision);
/* workspace of dfa_cae_score_ragged: the uniform plan at T_max plus the per-call table (4 * B int32 words), a multiple of
 * 256; 0 for B < 1.  The auto-encoder has a planner of its own because dfa_ragged_workspace_bytes(DFA_MODEL_CAE) returned 0
 * ("no ragged forward") before this entry point existed and callers test for that value: it keeps returning 0. */
size_t dfa_cae_ragged_workspace_bytes(const dfa_ctx* ctx, int B, int T_max, int F, int precision);
/* names of the device kernels a forward launches, for profile post-processing ("" when unknown) */
const char* dfa_dominant_kernel(int model, int precision);
/* ---- per-kernel timing (HIP events recorded on the context's stream around every launch) -------------
 * slots for CNN2D: 0 = conv1, 1 = block 2 (MFMA), 2 = block 3 (MFMA, the dominant kernel), 3 = linear;
 * CNN1D: 4 = the fused forward (three-launch path: 4, 5, 6 = conv blocks, 7 = linear);  CAE: 8 = enc1, 9-11 = enc2-4 (MFMA), 12 = fused decoder + MSE (bf16 mode; four-launch path: 12-14 = dec1-3, 15 = dec4+MSE).
 * enable: 0 = off, 1 = all slots, any other value = bit mask of slots (e.g. 1<<2 = block 3 only).
 * Enable, run forwards, then read (read synchronises on the recorded events; call it outside timed regions).
 * At most 256 launches per slot are recorded between resets. */
int dfa_ctx_timing_enable(dfa_ctx* ctx, int enable);
int dfa_ctx_timing_reset(dfa_ctx* ctx);
int dfa_ctx_timing_read(dfa_ctx* ctx, int slot, float* total_ms, int* count);
/* The shader clock (GHz) the chip held inside the LAST bf16 CNN2D block-3 launch made with option "clock_probe" = 1: per
 * workgroup delta s_memtime / (delta s_memrealtime * 10 ns), median / min / max over the workgroups that stamped (at most
 * 1024).  Synchronises on the context's stream.  The MFMA peak is quoted at 2.4 GHz; under MFMA load the chip holds less
 * (MI355X_MICROARCH.md, DVFS give-back), so roofline fractions are reported both against the nominal peak and at this clock.
 * ghz_min / ghz_max may be NULL. */
int dfa_ctx_clock_read(dfa_ctx* ctx, double* ghz_median, double* ghz_min, double* ghz_max, int* workgroups);
/* Which kernel ran blocks 1-3 of the LAST dfa_cnn2d_forward of this context (read-only; ctx NULL: DFA_E_NULL_PTR):
 * DFA_CONV123_NONE = separate kernels, _PER_UNIT = conv123_fused, _PERSIST = conv123_persist, _CARRY = conv123_carry. */
#define DFA_CONV123_NONE 0
#define DFA_CONV123_PER_UNIT 1
#define DFA_CONV123_PERSIST 2
#define DFA_CONV123_CARRY 3
int dfa_ctx_last_conv123_form(const dfa_ctx* ctx);
/* 1 if blocks 1-3 of the LAST dfa_cnn2d_forward ran the "phase123" build of the carry form (the form above is then
 * DFA_CONV123_CARRY: it is that form), else 0; ctx NULL: DFA_E_NULL_PTR. */
int dfa_ctx_last_conv123_phase(const dfa_ctx* ctx);
/* 1 if the LAST dfa_cnn2d_forward computed the logits inside the blocks 1-3 kernel (option "cls123"; form and phase above
 * read DFA_CONV123_CARRY and 1: it is that kernel with the classifier head at its end), 0 if linear1_kernel was launched or
 * the call was refused; ctx NULL: DFA_E_NULL_PTR. */
int dfa_ctx_last_conv123_cls(const dfa_ctx* ctx);
/* The plan of a CNN2D eval forward of [B, T, F] in `precision` (ragged != 0: of dfa_cnn2d_forward_ragged at T = T_max): the
 * very function dfa_cnn2d_forward[_ragged] and the two workspace planners read, reported.  Pure host arithmetic.  With a
 * context: for its options and its device's CU count (`options` and `num_cus` are not read).  Without one: for the seven
 * values options[] = {time_split, fuse_conv1, block3_m16, fuse_blocks123, persist123, carry_a1, phase123} (NULL = the
 * defaults -1, 1, 1, 1, 1, 1, 1) and `num_cus` compute units.  Fills the first min(cap, DFA_CNN2D_PLAN_FIELDS) of
 *    0 H1, 1 H2                      rows after pool 1 / pool 2
 *    2 a1_off, 3 a2_off, 4 emb_off   workspace regions (bytes)
 *    5 slabs                         slabs of B * 128 * F floats in the embedding region: 1, or 5 (the reduced embedding and
 *                                    four chunk slabs of a split block 3)
 *    6 tab_off, 7 tab_words          ragged: the per-call table behind the regions (4 * B words; uniform: 0 words)
 *    8 total                         = dfa_workspace_bytes / dfa_ragged_workspace_bytes
 *    9 path                          DFA_CNN2D_PATH_*
 *   10 form, 11 phase, 12 grid, 13 lds   path CONV123: DFA_CONV123_*, the de-phased build, workgroups, dynamic LDS bytes; else 0
 *   14 seg12                         iterations per time segment of the blocks 1+2 kernel (bf16x3 mode: of block 2), 0 = no split
 *   15 seg3, 16 chunk3, 17 nseg3     block 3: iterations per segment (0 = no split), iterations per canonical chunk of the time
 *                                    mean (0: the kernel has none), chunk slabs in use (1 = none).  Ragged: seg3 is the kernel's
 *                                    0 / 1 switch, chunk3 / nseg3 those of an utterance of T_max frames
 *   18 split3                        ragged: block 3 writes chunk slabs
 * of `fields` (may be NULL) and returns DFA_CNN2D_PLAN_FIELDS; 0 for B, T or F < 1. */
#define DFA_CNN2D_PATH_CONV1 0   /* conv1, block 2, block 3 */
#define DFA_CNN2D_PATH_CONV12 1  /* blocks 1+2 in one kernel, block 3 */
#define DFA_CNN2D_PATH_CONV123 2 /* blocks 1-3 in one kernel */
#define DFA_CNN2D_PLAN_FIELDS 19
int dfa_cnn2d_forward_plan(const dfa_ctx* ctx, int B, int T, int F, int precision, int ragged, const int* options, int num_cus,
                           long long* fields, int cap);
/* Raw copy of the first n (<= 2048) 64-bit words of the probe buffer the "clock_probe" kernels stamp (diagnostics: the fused CNN1D
 * kernel writes, per workgroup b < 128, words 8b..8b+3 = s_memtime at start / after layer 1 / after layer 2 / at the end and
 * 8b+5, 8b+6 = s_memrealtime at start / end).  Synchronises on the context's stream. */
int dfa_ctx_debug_read(dfa_ctx* ctx, long long* host_words, int n);

#ifdef __cplusplus
}
#endif
#endif /* DFA_HIP_H */

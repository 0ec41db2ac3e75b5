// api.hip -- what the C ABI of libdfa_hip.so (include/dfa_hip.h) has besides its models: version and error names, the context
// (create / destroy / set_stream, the option table, timing slots, clock and debug reads, the LDS poison hook), the staging of a
// ragged batch's per-call table, and the two shared workspace planners, which dispatch to the models'.  The models' entry points:
// cnn2d_api.hip, cnn1d_api.hip, cae_api.hip, dlq_api.hip (eval) and *_train_api.hip (training).
#include <stdlib.h>

#include <algorithm>

#include "dfa_checks.h"

using namespace dfa;

// The per-call table of a ragged forward, staged and sent: takes the next of the context's pinned slots (waiting for the copy
// that last read it; the staging grows when a batch needs more words), fills [0, B) with the lengths and [B, 2B) with the
// dispatch order, lets `fill_rest` write the model's own words behind them, and copies `words` words to `dst` (device) on the
// context's stream.  Dispatch order: the kernels' XCD remap gives each of the 8 XCDs one contiguous range of workgroup slots,
// so the utterances, sorted longest first, are dealt round-robin over 8 contiguous groups (sorted rank k -> group k % 8, place
// k / 8 in it).  Every XCD then gets about the same work, and inside its range the long utterances start first.
template <typename Fill>
static int stage_ragged_table(dfa_ctx* ctx, const int32_t* lengths, int B, size_t words, void* dst, Fill fill_rest) {
  if (words > ctx->ragged_cap) {
    for (auto& e : ctx->ragged_done)
      if (e) DFA_HIP_CHECK(ctx, hipEventSynchronize(e));
    if (ctx->ragged_host) DFA_HIP_CHECK(ctx, hipHostFree(ctx->ragged_host));
    ctx->ragged_host = nullptr;
    ctx->ragged_cap = 0;
    const size_t cap = std::max(words, (size_t)4 * 256);
    DFA_HIP_CHECK(ctx, hipHostMalloc((void**)&ctx->ragged_host, dfa_ctx::kRaggedSlots * cap * sizeof(int32_t), hipHostMallocDefault));
    ctx->ragged_cap = cap;
  }
  const int slot = ctx->ragged_slot;
  ctx->ragged_slot = (slot + 1) % dfa_ctx::kRaggedSlots;
  if (!ctx->ragged_done[slot]) DFA_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ragged_done[slot], hipEventDisableTiming));
  else DFA_HIP_CHECK(ctx, hipEventSynchronize(ctx->ragged_done[slot]));   // its previous copy has been read
  int32_t* tab = ctx->ragged_host + slot * ctx->ragged_cap;
  for (int b = 0; b < B; ++b) tab[b] = lengths[b];
  fill_rest(tab);
  std::vector<int> sorted(B);
  for (int b = 0; b < B; ++b) sorted[b] = b;
  std::stable_sort(sorted.begin(), sorted.end(), [&](int i, int j) { return lengths[i] > lengths[j]; });
  {
    int group_start[9] = {0};
    for (int g = 0; g < 8; ++g) group_start[g + 1] = group_start[g] + (B - g + 7) / 8;   // ranks k < B with k % 8 == g
    for (int k = 0; k < B; ++k) tab[B + group_start[k % 8] + k / 8] = sorted[k];
  }
  DFA_HIP_CHECK(ctx, hipMemcpyAsync(dst, tab, words * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  DFA_HIP_CHECK(ctx, hipEventRecord(ctx->ragged_done[slot], ctx->stream));
  return DFA_OK;
}

int dfa::stage_ragged_lengths(dfa_ctx* ctx, const int32_t* lengths, int B, void* dst) {
  return stage_ragged_table(ctx, lengths, B, (size_t)2 * B, dst, [](int32_t*) {});
}

int dfa::stage_ragged_lengths_extra(dfa_ctx* ctx, const int32_t* lengths, int B, const int32_t* extra, size_t n_extra, void* dst) {
  return stage_ragged_table(ctx, lengths, B, (size_t)2 * B + n_extra, dst, [&](int32_t* tab) {
    for (size_t i = 0; i < n_extra; ++i) tab[2 * B + i] = extra[i];
  });
}

extern "C" {

int dfa_version(void) { return DFA_VERSION; }

const char* dfa_error_name(int code) {
  switch (code) {
    case DFA_OK: return "DFA_OK";
    case DFA_E_BAD_SHAPE: return "DFA_E_BAD_SHAPE";
    case DFA_E_BAD_DTYPE: return "DFA_E_BAD_DTYPE";
    case DFA_E_NULL_PTR: return "DFA_E_NULL_PTR";
    case DFA_E_NOT_PREPARED: return "DFA_E_NOT_PREPARED";
    case DFA_E_HIP: return "DFA_E_HIP";
    case DFA_E_WORKSPACE: return "DFA_E_WORKSPACE";
    case DFA_E_UNSUPPORTED: return "DFA_E_UNSUPPORTED";
    default: return "DFA_E_UNKNOWN";
  }
}

int dfa_ctx_create(int device_id, void* hip_stream, dfa_ctx** out) {
  if (!out) return DFA_E_NULL_PTR;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return DFA_E_HIP;
  if (hipSetDevice(device_id) != hipSuccess) return DFA_E_HIP;
  dfa_ctx* c = new dfa_ctx();
  c->device = device_id;
  c->stream = (hipStream_t)hip_stream;
  if (hipMalloc(&c->zero_page, 256) != hipSuccess || hipMemset(c->zero_page, 0, 256) != hipSuccess) {
    delete c;
    return DFA_E_HIP;
  }
  // the persistent CNN2D kernel sizes its grid by the CU count: asked once here, so a forward (a captured one too) asks nothing
  if (hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || c->num_cus < 1) {
    (void)hipFree(c->zero_page);
    delete c;
    return DFA_E_HIP;
  }
  const char* dma = getenv("DFA_CONV_DMA");   // unset = per-kernel choice measured on MI355X (see launch_cnn2d_block*)
  c->conv_dma = (dma && (dma[0] == '0' || dma[0] == '1')) ? dma[0] - '0' : -1;
  *out = c;
  return DFA_OK;
}

int dfa_ctx_destroy(dfa_ctx* ctx) {
  if (!ctx) return DFA_E_NULL_PTR;
  (void)hipSetDevice(ctx->device);
  for (void* p : {ctx->cnn2d.packed, ctx->cnn1d.packed, ctx->cae.packed, ctx->dlq.packed, (void*)ctx->emb_ocsvm.svn, ctx->emb_gmm.image})
    if (p) (void)hipFree(p);
  ctx->cnn2d.train.release(); ctx->cnn1d.train.release(); ctx->cae.train.release(); ctx->dlq.train.release();
  if (ctx->clip_partial) (void)hipFree(ctx->clip_partial);
  if (ctx->zero_page) (void)hipFree(ctx->zero_page);
  if (ctx->clock_buf) (void)hipFree(ctx->clock_buf);
  if (ctx->mse_partial) (void)hipFree(ctx->mse_partial);
  if (ctx->aug_keep) (void)hipFree(ctx->aug_keep);
  for (auto e : ctx->ragged_done)
    if (e) (void)hipEventSynchronize(e), (void)hipEventDestroy(e);
  if (ctx->ragged_host) (void)hipHostFree(ctx->ragged_host);
  for (auto& t : ctx->slots) {
    for (auto e : t.start) (void)hipEventDestroy(e);
    for (auto e : t.stop) (void)hipEventDestroy(e);
  }
  delete ctx;
  return DFA_OK;
}

int dfa_ctx_set_stream(dfa_ctx* ctx, void* hip_stream) {
  if (!ctx) return DFA_E_NULL_PTR;
  ctx->stream = (hipStream_t)hip_stream;
  return DFA_OK;
}

const char* dfa_last_error(const dfa_ctx* ctx) { return ctx ? ctx->err : "null context"; }

namespace {
// Test hook ("poison_lds"): fills the whole 160 KB of LDS of every CU with a 16-bit pattern (0x7fc0 = bf16 NaN, 0xffff = NaN in
// either width).  LDS is not cleared between workgroups, so a kernel that lets bytes it never wrote reach a result shows up in the
// parity tests that run after this instead of once in a few thousand launches.
__global__ __launch_bounds__(256) void poison_lds_kernel(unsigned pattern, unsigned* sink) {
  extern __shared__ unsigned lds_words[];
  constexpr int N = 160 * 1024 / 4;
  for (int i = threadIdx.x; i < N; i += 256) lds_words[i] = pattern;
  __syncthreads();
  __builtin_amdgcn_s_sleep(127);
  if (lds_words[(threadIdx.x * 97 + blockIdx.x) % N] != pattern) sink[0] = 1;   // keeps the stores; never true
}
hipError_t launch_poison_lds(dfa_ctx* ctx, unsigned half) {
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return e;
  half &= 0xffffu;
  return launch_lds(poison_lds_kernel, dim3(2048), dim3(256), 160 * 1024, ctx->stream, half | (half << 16), (unsigned*)ctx->zero_page);
}
}  // namespace

namespace {
// the options that are one int of the context: a 0/1 switch (any non-zero value = 1) or the value as given.  dfa_ctx_get_option
// reads every row; dfa_ctx_set_option stores the last four itself (a range, an allocation) before it comes to the table
enum OptionKind { OPT_FLAG, OPT_INT };
struct Option { const char* name; int dfa_ctx::*field; OptionKind kind; };
const Option kOptions[] = {
    {"time_split", &dfa_ctx::time_split, OPT_INT},
    {"conv1_bwd_fused", &dfa_ctx::conv1_bwd_fused, OPT_FLAG}, {"dgrad_m16", &dfa_ctx::dgrad_m16, OPT_FLAG},
    {"conv1_mfma", &dfa_ctx::conv1_mfma, OPT_FLAG}, {"cae_enc1_mfma", &dfa_ctx::cae_enc1_mfma, OPT_FLAG},
    {"cae_enc_dma", &dfa_ctx::cae_enc_dma, OPT_FLAG}, {"cae_dgrad_mfma", &dfa_ctx::cae_dgrad_mfma, OPT_FLAG},
    {"cae_conv_stats", &dfa_ctx::cae_conv_stats, OPT_FLAG}, {"cae_bwd_fold", &dfa_ctx::cae_bwd_fold, OPT_FLAG},
    {"cae_enc4_wide", &dfa_ctx::cae_enc4_wide, OPT_FLAG}, {"cae_dec_fused", &dfa_ctx::cae_dec_fused, OPT_FLAG},
    {"block3_m16", &dfa_ctx::block3_m16, OPT_FLAG}, {"fuse_conv1", &dfa_ctx::fuse_conv1, OPT_FLAG},
    {"fuse_blocks123", &dfa_ctx::fuse_blocks123, OPT_FLAG}, {"persist123", &dfa_ctx::persist123, OPT_FLAG},
    {"lds_pipe", &dfa_ctx::lds_pipe, OPT_FLAG}, {"carry_a1", &dfa_ctx::carry_a1, OPT_FLAG},
    {"phase123", &dfa_ctx::phase123, OPT_FLAG}, {"cls123", &dfa_ctx::cls123, OPT_FLAG},
    {"wgrad_variant", &dfa_ctx::wgrad_variant, OPT_INT}, {"train_conv_variant", &dfa_ctx::train_conv_variant, OPT_INT},
    {"cnn1d_train_x3", &dfa_ctx::cnn1d_train_x3, OPT_INT}, {"cnn1d_fused", &dfa_ctx::cnn1d_fused, OPT_INT},
    {"conv_dma", &dfa_ctx::conv_dma, OPT_INT}, {"clock_probe", &dfa_ctx::clock_probe, OPT_INT},
};
}  // namespace

int dfa_ctx_set_option(dfa_ctx* ctx, const char* name, int value) {
  if (!ctx || !name) return DFA_E_NULL_PTR;
  if (strcmp(name, "poison_lds") == 0) {
    hipError_t e = launch_poison_lds(ctx, (unsigned)value);
    return e == hipSuccess ? DFA_OK : fail(ctx, DFA_E_HIP, "poison_lds: %s", hipGetErrorString(e));
  }
  if (strcmp(name, "clock_probe") == 0) {
    if (value && !ctx->clock_buf) {
      DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
      DFA_HIP_CHECK(ctx, hipMalloc((void**)&ctx->clock_buf, 1024 * 2 * sizeof(long long)));
    }
    if (value) DFA_HIP_CHECK(ctx, hipMemsetAsync(ctx->clock_buf, 0, 1024 * 2 * sizeof(long long), ctx->stream));
    ctx->clock_probe = value ? 1 : 0;
    return DFA_OK;
  }
  if (strcmp(name, "cnn1d_train_x3") == 0) { ctx->cnn1d_train_x3 = (value < 0 || value > 3) ? 1 : value; return DFA_OK; }
  if (strcmp(name, "cnn1d_fused") == 0) { ctx->cnn1d_fused = value < 0 ? 0 : (value > 2 ? 1 : value); return DFA_OK; }
  if (strcmp(name, "conv_dma") == 0) { ctx->conv_dma = value < 0 ? -1 : value; return DFA_OK; }
  for (const Option& o : kOptions)
    if (strcmp(name, o.name) == 0) { ctx->*o.field = (o.kind == OPT_FLAG) ? (value ? 1 : 0) : value; return DFA_OK; }
  return fail(ctx, DFA_E_UNSUPPORTED, "unknown option '%s'", name);
}

int dfa_ctx_get_option(const dfa_ctx* ctx, const char* name, int* value) {
  if (!ctx || !name || !value) return DFA_E_NULL_PTR;
  for (const Option& o : kOptions)
    if (strcmp(name, o.name) == 0) { *value = ctx->*o.field; return DFA_OK; }
  return DFA_E_UNSUPPORTED;   // unknown, or the action "poison_lds"
}

int dfa_ctx_timing_enable(dfa_ctx* ctx, int enable) {
  if (!ctx) return DFA_E_NULL_PTR;
  ctx->timing = (enable == 1) ? 0xffffffffu : (unsigned)enable;   // 1 = all slots, otherwise a bit mask of slots
  return DFA_OK;
}

int dfa_ctx_timing_reset(dfa_ctx* ctx) {
  if (!ctx) return DFA_E_NULL_PTR;
  for (auto& t : ctx->slots) t.used = 0;
  return DFA_OK;
}

int dfa_ctx_timing_read(dfa_ctx* ctx, int slot, float* total_ms, int* count) {
  if (!ctx || !total_ms || !count) return DFA_E_NULL_PTR;
  if (slot < 0 || slot >= kMaxSlots) return fail(ctx, DFA_E_BAD_SHAPE, "timing slot %d out of range", slot);
  SlotTimer& t = ctx->slots[slot];
  float sum = 0.f;
  for (int i = 0; i < t.used; ++i) {
    DFA_HIP_CHECK(ctx, hipEventSynchronize(t.stop[i]));
    if (t.empty[i]) continue;   // a stage that launched nothing: the record counts, its duration is 0
    float ms = 0.f;
    DFA_HIP_CHECK(ctx, hipEventElapsedTime(&ms, t.start[i], t.stop[i]));
    sum += ms;
  }
  *total_ms = sum;
  *count = t.used;
  return DFA_OK;
}

int dfa_ctx_clock_read(dfa_ctx* ctx, double* ghz_median, double* ghz_min, double* ghz_max, int* workgroups) {
  if (!ctx || !ghz_median || !workgroups) return DFA_E_NULL_PTR;
  *ghz_median = 0.0; *workgroups = 0;
  if (ghz_min) *ghz_min = 0.0;
  if (ghz_max) *ghz_max = 0.0;
  if (!ctx->clock_buf) return fail(ctx, DFA_E_NOT_PREPARED, "set the context option clock_probe = 1 and run a bf16 CNN2D forward first");
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DFA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  static thread_local long long h[1024 * 2];
  DFA_HIP_CHECK(ctx, hipMemcpy(h, ctx->clock_buf, sizeof(h), hipMemcpyDeviceToHost));
  double g[1024];
  int n = 0;
  for (int i = 0; i < 1024; ++i)
    if (h[2 * i + 1] > 0 && h[2 * i] > 0) g[n++] = (double)h[2 * i] / ((double)h[2 * i + 1] * 10.0);   // cycles / (ticks * 10 ns) = GHz
  if (n == 0) return DFA_OK;
  std::sort(g, g + n);
  *ghz_median = g[n / 2];
  if (ghz_min) *ghz_min = g[0];
  if (ghz_max) *ghz_max = g[n - 1];
  *workgroups = n;
  return DFA_OK;
}

int dfa_ctx_last_conv123_form(const dfa_ctx* ctx) { return ctx ? ctx->last_conv123_form : DFA_E_NULL_PTR; }
int dfa_ctx_last_conv123_phase(const dfa_ctx* ctx) { return ctx ? ctx->last_conv123_phase : DFA_E_NULL_PTR; }
int dfa_ctx_last_conv123_cls(const dfa_ctx* ctx) { return ctx ? ctx->last_conv123_cls : DFA_E_NULL_PTR; }

int dfa_ctx_debug_read(dfa_ctx* ctx, long long* host_words, int n) {
  if (!ctx || !host_words) return DFA_E_NULL_PTR;
  if (n < 0 || n > 2048) return fail(ctx, DFA_E_BAD_SHAPE, "the probe buffer holds 2048 words (got %d)", n);
  if (!ctx->clock_buf) return fail(ctx, DFA_E_NOT_PREPARED, "set the context option clock_probe = 1 first");
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  DFA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  DFA_HIP_CHECK(ctx, hipMemcpy(host_words, ctx->clock_buf, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost));
  return DFA_OK;
}

const char* dfa_dominant_kernel(int model, int precision) {
  if (model == DFA_MODEL_CNN2D)
    return precision == DFA_PREC_BF16 ? "conv3_m16_meant_kernel" : precision == DFA_PREC_BF16X3 ? "conv_split_kernel" : "conv3x3_mfma_kernel";
  return "";
}

size_t dfa_workspace_bytes(const dfa_ctx* ctx, int model, int B, int T, int F, int precision) {
  if (B < 1 || T < 1 || F < 1) return 0;
  if (model == DFA_MODEL_CNN2D) return cnn2d_workspace_bytes(ctx, B, T, F, precision, false);
  if (model == DFA_MODEL_CNN1D) return cnn1d_workspace_bytes(B, T, false);
  if (model == DFA_MODEL_CAE) return cae_workspace_bytes(B, T, F, precision);
  return 0;
}

// (the auto-encoder's ragged plan: dfa_cae_ragged_workspace_bytes in cae_api.hip; here it keeps its historical 0)
size_t dfa_ragged_workspace_bytes(const dfa_ctx* ctx, int model, int B, int T_max, int F, int precision) {
  if (B < 1 || T_max < 1 || F < 1) return 0;
  if (model == DFA_MODEL_CNN2D) return cnn2d_workspace_bytes(ctx, B, T_max, F, precision, true);
  if (model == DFA_MODEL_CNN1D) return cnn1d_workspace_bytes(B, T_max, true);
  return 0;
}

}  // extern "C"

// emb_api.hip -- C ABI of the embedding anomaly detectors (include/dfa_hip.h, kernels in emb_score.hip): binding a fitted
// One-Class SVM / PCA + GMM, the workspace plan, and the two scoring calls on embedding rows where the CNN2D forward left them.
#include "dfa_checks.h"
#include "trace.h"

using namespace dfa;

namespace {

constexpr int kMaxRows = 65535 * 128;   // the GEMM frame's grid: 128 rows per workgroup along gridDim.y

struct Named { const char* name; const void* p; };

// no null pointer, every array 16-byte aligned (the frame stages float4)
template <size_t N>
int check_arrays(dfa_ctx* ctx, const Named (&a)[N]) {
  for (const Named& e : a)
    if (!e.p) return fail(ctx, DFA_E_NULL_PTR, "%s must be non-null", e.name);
  for (const Named& e : a)
    if (((uintptr_t)e.p & 15) != 0) return fail(ctx, DFA_E_UNSUPPORTED, "%s must be 16-byte aligned (got %p)", e.name, e.p);
  return DFA_OK;
}

int check_D(dfa_ctx* ctx, int D) {
  if (D < 128 || D % 128 != 0)
    return fail(ctx, DFA_E_BAD_SHAPE, "D must be 128 * F, the CNN2D embedding width, for an F >= 1 (got D=%d)", D);
  return DFA_OK;
}

int no_capture(dfa_ctx* ctx, const char* what) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  DFA_HIP_CHECK(ctx, hipStreamIsCapturing(ctx->stream, &cap));
  if (cap != hipStreamCaptureStatusNone) return fail(ctx, DFA_E_UNSUPPORTED, "%s allocates the detector's image: it cannot be captured into a graph", what);
  return DFA_OK;
}

// workspace regions in bytes, each 256-byte aligned.  OC-SVM: the split products.  GMM: the split products of z, z, y
struct EmbPlan { size_t part_off, z_off, y_off, total; };
EmbPlan plan_emb(int detector, int N, int D, int M, int K) {
  EmbPlan p{};
  const EmbSplit sp = emb_split(D, M);
  size_t off = align_up((size_t)sp.nsplit * N * M * sizeof(float), 256);
  if (detector == DFA_EMB_GMM) {
    p.z_off = off;
    off = align_up(off + (size_t)N * emb_ppad(M) * sizeof(float), 256);
    p.y_off = off;
    off = align_up(off + (size_t)K * N * M * sizeof(float), 256);
  }
  p.total = off;
  return p;
}

int check_rows(dfa_ctx* ctx, const float* emb, int N, int D, int bound_D, int64_t stride_n, const float* out, const void* workspace) {
  if (!emb) return fail(ctx, DFA_E_NULL_PTR, "emb must be non-null");
  if (!out) return fail(ctx, DFA_E_NULL_PTR, "out must be non-null");
  if (!workspace) return fail(ctx, DFA_E_NULL_PTR, "workspace must be non-null");
  if (N < 1) return fail(ctx, DFA_E_BAD_SHAPE, "N must be >= 1 (got N=%d)", N);
  if (N > kMaxRows) return fail(ctx, DFA_E_UNSUPPORTED, "N must be <= %d rows per call (got N=%d)", kMaxRows, N);
  DFA_TRY(check_D(ctx, D));
  if (D != bound_D) return fail(ctx, DFA_E_BAD_SHAPE, "D=%d does not match the bound detector's D=%d", D, bound_D);
  if (stride_n < D) return fail(ctx, DFA_E_BAD_SHAPE, "stride_n must be >= D=%d: rows may not overlap (got stride_n=%lld)", D, (long long)stride_n);
  if ((stride_n & 3) != 0 || ((uintptr_t)emb & 15) != 0)
    return fail(ctx, DFA_E_UNSUPPORTED, "emb must be 16-byte aligned with stride_n %% 4 == 0 (got emb=%p, stride_n=%lld)", (const void*)emb,
                (long long)stride_n);
  return DFA_OK;
}

}  // namespace

extern "C" {

int dfa_emb_ocsvm_bind(dfa_ctx* ctx, int D, int n_sv, const float* mean, const float* inv_scale, const float* sv, const float* dual_coef,
                       float gamma, float intercept) {
  if (!ctx) return DFA_E_NULL_PTR;
  EmbOcsvm& d = ctx->emb_ocsvm;
  d.bound = false;
  DFA_TRY(check_D(ctx, D));
  if (n_sv < 1) return fail(ctx, DFA_E_BAD_SHAPE, "n_sv must be >= 1 (got n_sv=%d)", n_sv);
  if (!(gamma > 0.f)) return fail(ctx, DFA_E_UNSUPPORTED, "gamma must be positive: the RBF kernel is the only one (got gamma=%g)", (double)gamma);
  const Named arrays[] = {{"mean", mean}, {"inv_scale", inv_scale}, {"sv", sv}, {"dual_coef", dual_coef}};
  DFA_TRY(check_arrays(ctx, arrays));
  DFA_TRY(no_capture(ctx, "dfa_emb_ocsvm_bind"));
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (d.svn) { DFA_HIP_CHECK(ctx, hipFree(d.svn)); d.svn = nullptr; }
  DFA_HIP_CHECK(ctx, hipMalloc((void**)&d.svn, align_up((size_t)n_sv * sizeof(float), 256)));
  DFA_HIP_CHECK(ctx, launch_emb_rownorm(sv, D, n_sv, D, d.svn, ctx->stream));
  d.D = D; d.n_sv = n_sv; d.mean = mean; d.inv_scale = inv_scale; d.sv = sv; d.coef = dual_coef; d.gamma = gamma; d.intercept = intercept;
  d.bound = true;
  return DFA_OK;
}

int dfa_emb_gmm_bind(dfa_ctx* ctx, int D, int P, int K, const float* mean, const float* inv_scale, const float* pca_mean, const float* components,
                     const float* means, const float* prec_chol, const float* log_const) {
  if (!ctx) return DFA_E_NULL_PTR;
  EmbGmm& d = ctx->emb_gmm;
  d.bound = false;
  DFA_TRY(check_D(ctx, D));
  if (P < 1 || P > DFA_EMB_MAX_P) return fail(ctx, DFA_E_BAD_SHAPE, "P must be in [1, %d] (got P=%d)", DFA_EMB_MAX_P, P);
  if (K < 1 || K > DFA_EMB_MAX_K) return fail(ctx, DFA_E_BAD_SHAPE, "K must be in [1, %d] (got K=%d)", DFA_EMB_MAX_K, K);
  const Named arrays[] = {{"mean", mean}, {"inv_scale", inv_scale}, {"pca_mean", pca_mean}, {"components", components}};
  DFA_TRY(check_arrays(ctx, arrays));
  for (const Named& e : {Named{"means", means}, Named{"prec_chol", prec_chol}, Named{"log_const", log_const}})   // read by scalar loads: any alignment
    if (!e.p) return fail(ctx, DFA_E_NULL_PTR, "%s must be non-null", e.name);
  DFA_TRY(no_capture(ctx, "dfa_emb_gmm_bind"));
  DFA_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int Ppad = emb_ppad(P);
  const size_t lt_bytes = align_up((size_t)K * Ppad * Ppad * sizeof(float), 256), m_bytes = align_up((size_t)K * Ppad * sizeof(float), 256);
  if (d.image) { DFA_HIP_CHECK(ctx, hipFree(d.image)); d.image = nullptr; }
  DFA_HIP_CHECK(ctx, hipMalloc(&d.image, lt_bytes + m_bytes));
  d.LT = (float*)d.image;
  d.mpad = (float*)((char*)d.image + lt_bytes);
  DFA_HIP_CHECK(ctx, launch_emb_pack_gmm(prec_chol, means, P, K, d.LT, d.mpad, ctx->stream));
  d.D = D; d.P = P; d.K = K; d.mean = mean; d.inv_scale = inv_scale; d.pca_mean = pca_mean; d.comp = components; d.log_const = log_const;
  d.bound = true;
  return DFA_OK;
}

size_t dfa_emb_workspace_bytes(int detector, int N, int D, int M, int K) {
  if (N < 1 || N > kMaxRows || D < 128 || D % 128 != 0 || M < 1) return 0;
  if (detector == DFA_EMB_OCSVM) return plan_emb(detector, N, D, M, 0).total;
  if (detector != DFA_EMB_GMM || M > DFA_EMB_MAX_P || K < 1 || K > DFA_EMB_MAX_K) return 0;
  return plan_emb(detector, N, D, M, K).total;
}

int dfa_emb_ocsvm_score(dfa_ctx* ctx, const float* emb, int N, int D, int64_t stride_n, float* out, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_emb_ocsvm_score");
  if (!ctx) return DFA_E_NULL_PTR;
  const EmbOcsvm& d = ctx->emb_ocsvm;
  if (!d.bound) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_emb_ocsvm_bind has not been called (or its last call was refused)");
  DFA_TRY(check_rows(ctx, emb, N, D, d.D, stride_n, out, workspace));
  const EmbPlan pl = plan_emb(DFA_EMB_OCSVM, N, D, d.n_sv, 0);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total));
  DFA_HIP_CHECK(ctx, launch_emb_ocsvm(d, emb, N, stride_n, (float*)workspace, out, ctx->stream));
  return DFA_OK;
}

int dfa_emb_gmm_score(dfa_ctx* ctx, const float* emb, int N, int D, int64_t stride_n, float* out, void* workspace, size_t workspace_bytes) {
  TraceRange trace_("dfa_emb_gmm_score");
  if (!ctx) return DFA_E_NULL_PTR;
  const EmbGmm& d = ctx->emb_gmm;
  if (!d.bound) return fail(ctx, DFA_E_NOT_PREPARED, "dfa_emb_gmm_bind has not been called (or its last call was refused)");
  DFA_TRY(check_rows(ctx, emb, N, D, d.D, stride_n, out, workspace));
  const EmbPlan pl = plan_emb(DFA_EMB_GMM, N, D, d.P, d.K);
  DFA_TRY(check_workspace(ctx, workspace, workspace_bytes, pl.total));
  char* ws = (char*)workspace;
  DFA_HIP_CHECK(ctx, launch_emb_gmm(d, emb, N, stride_n, (float*)ws, (float*)(ws + pl.z_off), (float*)(ws + pl.y_off), out, ctx->stream));
  return DFA_OK;
}

}  // extern "C"

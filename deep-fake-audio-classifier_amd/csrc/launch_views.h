// launch_views.h -- the typed views the host launch layer passes between the C ABI's entry points and the launchers: the feature
// tensor, one layer's parameters / gradients, one BatchNorm layer's apply terms; and launch_lds, the launch of a kernel with dynamic
// LDS.  Host only: no view appears in a kernel signature or in a struct passed to a kernel; a launcher unpacks it into the kernel's
// own arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dfa {

// THE launch of a kernel with dynamic LDS: every such launch of the library goes through here, and nothing else touches a kernel's
// attributes.  The limit on a kernel's dynamic LDS is an attribute per device (and several kernels are launched with more than one
// byte count), so it is set on the current device with every launch: nothing is remembered per process, and two contexts on two
// GPUs, or two host threads, need no agreement.  Returns the attribute's error, or the launch's.
template <typename... Params, typename... Args>
inline hipError_t launch_lds(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args&... args) {
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
  return hipGetLastError();
}

// the caller's feature tensor [B, T, F] (T = T_max of a ragged batch): element (b, t, f) at x[b sb + t st + f sf], dtype = DFA_DTYPE_*.
// An extern "C" entry point builds it once, behind its argument checks, from its own arguments in this order; no other function takes
// the three strides side by side
struct FeatView { const void* x; int dtype; int64_t sb, st, sf; int B, T, F; };

// THE layout rule of every model's parameter array (CNN2D, CNN1D, auto-encoder, DeepfakeDetector; each model's _abi_tensors() writes it): six
// pointers per conv + BatchNorm layer in this order, then the head's (w, b) pairs.  Gradients: four per layer, then the head's.
// The auto-encoder's decoder blocks 1-3 are layers 4-6 of the same numbering; its decoder block 4 is its head.
struct LayerParams { const float *w, *b, *gamma, *beta, *rmean, *rvar; };
struct LayerGrads { float *dw, *db, *dgamma, *dbeta; };
struct HeadParams { const float *w, *b; };
struct HeadGrads { float *dw, *db; };
constexpr int n_params(int layers, int head_pairs) { return 6 * layers + 2 * head_pairs; }
constexpr int n_grads(int layers, int head_pairs) { return 4 * layers + 2 * head_pairs; }
inline LayerParams layer_params(const float* const* p, int l) {
  const float* const* q = p + 6 * l;
  return {q[0], q[1], q[2], q[3], q[4], q[5]};
}
inline LayerGrads layer_grads(float* const* grads, int l) {
  float* const* g = grads + 4 * l;
  return {g[0], g[1], g[2], g[3]};
}
// pair `k` of the head behind `layers` layers
inline HeadParams head_params(const float* const* p, int layers, int k) {
  const float* const* q = p + n_params(layers, k);
  return {q[0], q[1]};
}
inline HeadGrads head_grads(float* const* grads, int layers, int k) {
  float* const* g = grads + n_grads(layers, k);
  return {g[0], g[1]};
}
// the layer's convolution alone (train mode: BatchNorm runs on batch statistics as a pass of its own): what a fold / pack launcher
// takes in place of the layer to leave the weights unscaled and the bias as it is.  folds(lp) is how the launcher tells
inline LayerParams raw_conv(const LayerParams& lp) { return {lp.w, lp.b, nullptr, nullptr, nullptr, nullptr}; }
inline bool folds(const LayerParams& lp) { return lp.gamma != nullptr; }

// the running statistics a train-mode forward updates (the one place the parameter array is written through): null = leave them
struct RunningStats { float *mean, *var; };
inline RunningStats running_stats(const LayerParams& lp, bool update) {
  return update ? RunningStats{const_cast<float*>(lp.rmean), const_cast<float*>(lp.rvar)} : RunningStats{nullptr, nullptr};
}

// mean | var | invstd of one BatchNorm layer in a model's statistics block (train_host.h: bn_stats), and the four terms its apply
// and backward passes read
struct BnStats { float *mean, *var, *invstd; };
struct BnApply { const float *mean, *invstd, *gamma, *beta; };
inline BnApply bn_apply(const BnStats& st, const LayerParams& lp) { return {st.mean, st.invstd, lp.gamma, lp.beta}; }

}  // namespace dfa

// cae_mse_finalize_body.h -- the body of cae_mse_finalize_kernel / cae_mse_finalize_ragged_kernel (cae.hip), included INSIDE each
// __global__ function with partial, nblk, inv_n, tab, mse, B and RAGGED (compile-time bool) in scope: an utterance's per-tile
// squared-error sums are added in tile order in double, in both forms.
#ifndef DFA_KERNEL_BODY_SCOPE
#error "cae_mse_finalize_body.h is a kernel body: include it only inside the __global__ functions of cae.hip"
#endif
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = RAGGED ? tab[3 * B + b] : nblk;
  const float scale = RAGGED ? __int_as_float(tab[2 * B + b]) : inv_n;
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += (double)partial[(size_t)b * nblk + k];
  mse[b] = (float)(s * (double)scale);

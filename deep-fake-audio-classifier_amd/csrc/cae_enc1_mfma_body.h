// cae_enc1_mfma_body.h -- the body of cae_enc1_mfma_kernel / cae_enc1_mfma_ragged_kernel (cae_enc1_mfma.hip), included INSIDE
// each __global__ function with TX, the kernel's arguments, RAGGED (compile-time bool) and `rt` (RaggedTab) in scope: one
// source for the uniform and the ragged form.
#ifndef DFA_KERNEL_BODY_SCOPE
#error "cae_enc1_mfma_body.h is a kernel body: include it only inside the __global__ functions of cae_enc1_mfma.hip"
#endif
  static_assert(std::is_same<decltype(RAGGED), const bool>::value, "the including kernel defines constexpr bool RAGGED");
  using namespace e1m;
  extern __shared__ __attribute__((aligned(16))) float xs[];      // [XR][pitch]: column c <-> feature f = c - 1
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int b = blockIdx.y, q0 = blockIdx.x * QG;
  // RAGGED: the utterance's own length sets the row masks and the pooled height; T / Ho (the batch maximum) remain the grid's
  // extent and the row pitch of the output.  Row groups past the utterance's end leave before they read anything.
  const int Tb = RAGGED ? __builtin_amdgcn_readfirstlane(rt.tab[b]) : T;
  const int Hob = RAGGED ? Tb >> 1 : Ho;
  if constexpr (RAGGED) {
    if (q0 >= Hob) return;
  }
  const TX* xb = x + (int64_t)b * sb;
  const int t_base = 2 * q0 - 1;
  const bool t_fast = (st == 1);
  const int ncol = F + 2;
  float* const zs = xs + XR * pitch;                  // [F][2]: 1 / sigma, -mu / sigma (z-score table, only when mu != null)
  if (mu) {
    for (int f = tid; f < F; f += 256) {
      const float rs = __builtin_amdgcn_rcpf(sigma[f]);
      zs[2 * f] = rs;
      zs[2 * f + 1] = -mu[f] * rs;
    }
    __syncthreads();
  }
  // Eight loads in flight per thread and trip (a one-load-per-trip loop pays the memory latency 25 times per workgroup: the
  // vector kernel it replaces does, and so did the first version of this one -- 0.158 ms for 0.06 ms of arithmetic).
  constexpr int NE = 8;
  const int nel = XR * ncol;
  for (int e0 = 0; e0 < nel; e0 += 256 * NE) {
    float v[NE];
    int dst[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      const int e = e0 + k * 256 + tid;
      int rr, cc;
      if (t_fast) { cc = e / XR; rr = e - cc * XR; } else { rr = e / ncol; cc = e - rr * ncol; }
      const int t = t_base + rr, f = cc - 1;
      const bool ok = e < nel && t >= 0 && t < Tb && f >= 0 && f < F && !(dbg & 2);
      const TX* p = xb + (ok ? (int64_t)t * st + (int64_t)f * sf : 0);      // clamped address, branch-free
      float xv;
      if constexpr (sizeof(TX) == 2) xv = bf16_to_float(*p); else xv = *p;
      // z-score as x * (1 / sigma) - mu / sigma from a per-column table in LDS (built once per workgroup): one LDS read pair + one FMA
      // per element instead of two more global loads and an IEEE division (this loop is bound by its memory instructions); the 1-2
      // ulp difference disappears in the bf16 rounding of the operand (bf16 mode only: the fp32 parity path keeps the division)
      if (mu) { const int fc = ok ? f : 0; xv = fmaf(xv, zs[2 * fc], zs[2 * fc + 1]); }
      v[k] = ok ? xv : 0.f;                     // the convolution's zero padding applies to the NORMALISED input
      dst[k] = e < nel ? rr * pitch + cc : -1;
    }
#pragma unroll
    for (int k = 0; k < NE; ++k)
      if (dst[k] >= 0) xs[dst[k]] = v[k];
  }
  // A operands (even-hi, even-lo, odd-hi, odd-lo; conv12_fused.hip's pack: the vertical pool's 1/2 is folded in) and the bias as
  // the accumulators' initial value: channel (r & 3) + 8 (r >> 2) + 4 h <-> register r
  uint4 cw[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) cw[k] = c1pack[k * 64 + lane];
  f32x16_t bias;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 bv = *(const float4*)(c1bias + 8 * g + 4 * h);
    bias[4 * g] = bv.x; bias[4 * g + 1] = bv.y; bias[4 * g + 2] = bv.z; bias[4 * g + 3] = bv.w;
  }
  __syncthreads();

  const float rlim = relu_limit();
  const int ntile = (F + 31) / 32;
  const int nunit = min(QG, Hob - q0) * ntile;
  for (int u = wave; u < ((dbg & 4) ? 0 : nunit); u += 4) {
    const int qq = u / ntile, tile = u - qq * ntile;
    const int f = 32 * tile + col;
    // this lane's window rows 2 qq + 2 h, + 1 (of the 4-row window of pooled row q0 + qq), columns f - 1 .. f + 1 (zero beyond F:
    // the tile's columns past the image read the zeroed right-hand pad or the next row's pad -- clamp to the pad column)
    const int cc = min(f, F + 1 - 2);
    const float* r0 = xs + (2 * qq + 2 * h) * pitch + cc;
    float v[8];
    const bool inimg = f < F;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
#pragma unroll
      for (int k = 0; k < 3; ++k) v[4 * rr + k] = inimg ? r0[rr * pitch + k] : 0.f;
      v[4 * rr + 3] = 0.f;
    }
    unsigned hh[4], ll[4], l2[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      hh[p] = pack_bf16x2(v[2 * p], v[2 * p + 1]);
      const float ra = v[2 * p] - __uint_as_float(hh[p] << 16), rb = v[2 * p + 1] - __uint_as_float(hh[p] & 0xffff0000u);
      ll[p] = pack_bf16x2(ra, rb);
      l2[p] = pack_bf16x2(ra - __uint_as_float(ll[p] << 16), rb - __uint_as_float(ll[p] & 0xffff0000u));
    }
    const uint4 xh = make_uint4(hh[0], hh[1], hh[2], hh[3]), xl = make_uint4(ll[0], ll[1], ll[2], ll[3]),
                x2 = make_uint4(l2[0], l2[1], l2[2], l2[3]);
    // smallest terms first into the accumulator that starts from the bias
    f32x16_t e = Mma<bf16_t>::run(cw[0], x2, bias);
    f32x16_t o = Mma<bf16_t>::run(cw[3], x2, bias);
    e = Mma<bf16_t>::run(cw[2], xh, e);
    o = Mma<bf16_t>::run(cw[5], xh, o);
    e = Mma<bf16_t>::run(cw[1], xl, e);
    o = Mma<bf16_t>::run(cw[4], xl, o);
    e = Mma<bf16_t>::run(cw[0], xl, e);
    o = Mma<bf16_t>::run(cw[3], xl, o);
    e = Mma<bf16_t>::run(cw[1], xh, e);
    o = Mma<bf16_t>::run(cw[4], xh, o);
    e = Mma<bf16_t>::run(cw[0], xh, e);
    o = Mma<bf16_t>::run(cw[3], xh, o);
    // ReLU + 2 x 2 average: vertical pair in this lane (factor 1/2 in the weights), horizontal pair with the lane of column f ^ 1
    unsigned pk[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      float s0 = relu1(e[2 * p], rlim) + relu1(o[2 * p], rlim);
      float s1 = relu1(e[2 * p + 1], rlim) + relu1(o[2 * p + 1], rlim);
      // neighbouring column = neighbouring lane: a DPP quad_perm [1,0,3,2] move, not an LDS permute
      s0 += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s0), 0xB1, 0xF, 0xF, true));
      s1 += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s1), 0xB1, 0xF, 0xF, true));
      pk[p] = pack_bf16x2(s0, s1);                             // (both pool factors ride on the packed weights and bias)
    }
    // half-wave exchange: lanes < 32 get channels 8 g .. 8 g + 7, lanes >= 32 channels 8 g + 8 .. 8 g + 15 (g = 0, 2)
    const auto a0 = __builtin_amdgcn_permlane32_swap(pk[0], pk[2], false, false);
    const auto a1 = __builtin_amdgcn_permlane32_swap(pk[1], pk[3], false, false);
    const auto b0 = __builtin_amdgcn_permlane32_swap(pk[4], pk[6], false, false);
    const auto b1 = __builtin_amdgcn_permlane32_swap(pk[5], pk[7], false, false);
    const int q = q0 + qq, j = f >> 1;
    const bool oddc = col & 1;                                 // even column: chunk g = 0 (+ h), odd column: chunk g = 2 (+ h)
    // (element-wise selects: indexing a two-element register array with the lane's parity sent it through scratch memory)
    const uint4 val = make_uint4(oddc ? b0[0] : a0[0], oddc ? b1[0] : a1[0], oddc ? b0[1] : a0[1], oddc ? b1[1] : a1[1]);
    if (j < Wo && !(dbg & 1))
      *(uint4*)((char*)(out + (((size_t)b * Ho + q) * Wo + j) * 32) + (2 * (int)oddc + h) * 16) = val;
  }

// conv3x3_body.h -- the body of conv3x3_mfma_kernel / conv3x3_mfma_ragged_kernel (conv3x3_mfma.h).  Included inside a
// kernel with the template parameters of conv3x3_mfma_kernel, `a` (ConvArgs), RAGGED (compile-time bool), `rt` (RaggedTab) and
// `hshift` (int) in scope: one source for the uniform and the ragged form.
#ifndef DFA_KERNEL_BODY_SCOPE
#error "conv3x3_body.h is a kernel body: include it inside a kernel of conv3x3_mfma.h"
#endif
  static_assert(std::is_same<decltype(RAGGED), const bool>::value, "the including kernel defines constexpr bool RAGGED");
  static_assert(MT == 1, "strips are 32 columns wide");
  using C = ConvCfg<T, CIN, NSL, MG, RP, EPI>;
  constexpr int PB = C::PB, CPP = C::CPP, SP = C::SP, BR = C::BR, NT = C::NT, NKG = C::NKG, ROWB = C::ROW_BYTES;
  static_assert(!STATS || EPI == EPI_PLAIN, "BatchNorm statistics ride on the PLAIN epilogue");
  static_assert(!RAGGED || (EPI == EPI_POOL_2X2 && !ACCIN && !STATS), "the ragged form serves the auto-encoder's encoder blocks");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nsl = (NSL == 1) ? 0 : wave % NSL;
  const int mg = (MG == 1) ? 0 : wave / NSL;
  const int r = lane & 31, h = lane >> 5;

  const int logical = xcd_logical_workgroup();   // XCD-aware block order (dfa_device.h)
  // RAGGED: workgroup slot u -> utterance through the dispatch order of the table (longest first, dealt over the eight XCD
  // ranges); H is the utterance's own height at this layer (T_b >> hshift), a.H the batch maximum that fixes the row pitch of
  // the input and of the output.  Rows at or past H stage from the zero page, as rows past the image always did.
  const int u = logical / a.nstrips;
  const int b = RAGGED ? __builtin_amdgcn_readfirstlane(rt.tab[rt.B + u]) : u;
  const int strip = logical - u * a.nstrips;
  const int f0 = strip * 32;
  const int H = RAGGED ? __builtin_amdgcn_readfirstlane(rt.tab[b]) >> hshift : a.H, W = a.W, COUT = a.COUT;
  const int Hpitch = RAGGED ? a.H : H;
  const int cout_base = blockIdx.y * (NSL * 32);
  const int nb = cout_base + nsl * 32;  // first output channel of this wave's slice

  const int ipb = a.in_pix_bytes ? a.in_pix_bytes : PB;
  const char* in_b = (const char*)a.in + (size_t)b * Hpitch * W * ipb + a.in_ch_off_bytes;

  // ---- weights: the wave's [9][NKG] 16-byte fragments stay in registers for the whole kernel
  uint4 w[9][NKG];
  {
    const uint4* wp = a.wpack + ((size_t)(blockIdx.y * NSL + nsl) * 9 * NKG) * 64 + lane;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kg = 0; kg < NKG; ++kg) w[tap][kg] = wp[(tap * NKG + kg) * 64];
  }
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;   // LDS byte address of smem
  const float rlim = relu_limit();
  // PFD > 0: asm-pipelined fragment reads, PFD reads in flight; 0: compiler-scheduled reads; -1: pipelined (depth 4) for
  // the two-waves-per-SIMD bf16 kernels.  The one-wave-per-SIMD kernels keep weights in AGPRs and spill; there the
  // compiler-scheduled form is used (an fp32 ACCIN kernel produced wrong sums with pipelined reads under that register
  // pressure) -- every pipelined instantiation is checked bit-for-bit against its PFD = 0 twin on the GPU.
  constexpr bool PIPE = PFD > 0 || (PFD < 0 && MINW >= 2 && sizeof(T) == 2);
  constexpr int PF = PIPE ? (PFD > 0 ? PFD : 4) : 1;
  constexpr bool EARLY_RELU = PIPE && (EPI == EPI_POOL_H2 || EPI == EPI_POOL_2X2 || EPI == EPI_MEAN_T);
  float* bias_lds = (float*)(smem + C::RING_BYTES);
  if (tid < NSL * 32) bias_lds[tid] = a.bias[cout_base + tid];

  // ---- per-lane fragment offsets inside a ring row (loop-invariant): slot = r + dx, logical chunk 2*kg + h.
  // xa[dx] carries the kg = 0 address; k-group kg is xa[dx] ^ (kg << 5) (see header).
  int xa[3];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int slot = r + dx, s = lds_swz<PB>(slot);
    xa[dx] = slot * PB + (((h ^ (s & 1)) << 4) | ((s >> 1) << 5));
  }

  // ---- staging constants: thread's k-th PHYSICAL chunk of a ring block (pad slots and out-of-image columns -> zeros)
  int s_off[C::NLD];     // source byte offset relative to row (BR*j - 1), -1 when the column is never valid
#pragma unroll
  for (int k = 0; k < C::NLD; ++k) {
    const int g = k * NT + tid;
    const int rowi = g / (SP * CPP), rem = g - rowi * (SP * CPP);
    const int slot = rem / CPP, cph = rem % CPP;
    const int c = cph ^ lds_swz<PB>(slot);
    const int f = f0 - 1 + slot;
    const bool ok = (g < C::NCH) && (slot < C::SLOTS) && (f >= 0) && (f < W);
    s_off[k] = ok ? (rowi * W + f) * ipb + c * 16 : -1;
  }
  uint4 stg[DMA ? 1 : C::NLD];
  auto stage_load = [&](int j) {  // global -> registers
#pragma unroll
    for (int k = 0; k < C::NLD; ++k) {
      const int t = BR * j - 1 + (k * NT + tid) / (SP * CPP);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s_off[k] >= 0 && t >= 0 && t < H) v = *(const uint4*)(in_b + (ptrdiff_t)(BR * j - 1) * W * ipb + s_off[k]);
      stg[DMA ? 0 : k] = v;
    }
  };
  auto stage_store = [&](int ringblk) {  // registers -> LDS (physical chunk order)
#pragma unroll
    for (int k = 0; k < C::NLD; ++k) {
      const int g = k * NT + tid;
      if (g < C::NCH) *(uint4*)(smem + ringblk * BR * ROWB + g * 16) = stg[DMA ? 0 : k];
    }
  };
  // LDS-DMA variant (global_load_lds_dwordx4): no staging VGPRs, no ds_write.  One wave instruction fills 64
  // consecutive PHYSICAL 16-byte chunks (wave-uniform LDS base + lane*16); the swizzle lives in the per-lane SOURCE
  // address.  Out-of-image chunks read a 16-byte zero page.  Retired by the vmcnt(0) of the iteration's barrier.
  auto stage_dma = [&](int j, int ringblk) {
#pragma unroll
    for (int k = 0; k < C::NLD; ++k) {
      const int g = k * NT + tid;
      if (g < C::NCH) {
        const int t = BR * j - 1 + g / (SP * CPP);
        const char* src = (s_off[k] >= 0 && t >= 0 && t < H) ? in_b + (ptrdiff_t)(BR * j - 1) * W * ipb + s_off[k]
                                                             : (const char*)a.zero_page;
        char* dst = smem + ringblk * BR * ROWB + (k * NT + wave * 64) * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      }
    }
  };

  // ---- epilogue state
  float cs[EPI == EPI_MEAN_T ? 16 : 1];              // MEAN_T: running column sums (pixel = lane, channel = register)
  float st1[STATS ? 16 : 1], st2[STATS ? 16 : 1];    // PLAIN: per-channel sum / sum of squares over this lane's pixels
  if (EPI == EPI_MEAN_T) {
#pragma unroll
    for (int i = 0; i < 16; ++i) cs[i] = 0.f;
  }
  if (STATS) {
#pragma unroll
    for (int i = 0; i < 16; ++i) { st1[i] = 0.f; st2[i] = 0.f; }
  }
  const int col = f0 + r;                    // this lane's output pixel column
  const bool col_ok = col < W;

  const int niter = (H + BR - 1) / BR;
#ifdef DFA_STAMPS
  long long seg[6] = {0, 0, 0, 0, 0, 0};
  long long t_prev = __builtin_amdgcn_s_memtime();
  const long long t_begin = t_prev;
  auto stamp = [&](int k) { const long long t = __builtin_amdgcn_s_memtime(); seg[k] += t - t_prev; t_prev = t; };
#else
  auto stamp = [&](int) {};
#endif
  if (DMA) {
    stage_dma(0, 0);
    stage_dma(1, 1);
  } else {
    stage_load(0);
    stage_store(0);
    stage_load(1);
    stage_store(1);
  }
  if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // one unit: output rows t0 = BR*it + 2*RPI, t0+1; PH = it % 3 (ring phase), both compile-time
  auto unit = [&](auto ph_c, auto rp_c, int it) {
    constexpr int PH = decltype(ph_c)::value, RPI = decltype(rp_c)::value;
    f32x16_t acc0, acc1;
    const int t0 = BR * it + 2 * RPI;
    if (ACCIN) {
      const float* i0 = a.acc_in + (((size_t)b * H + t0) * W + col) * COUT + nb + 4 * h;
      const float* i1 = i0 + (size_t)W * COUT;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if (col_ok && t0 < H) v0 = *(const float4*)(i0 + 8 * g);
        if (col_ok && t0 + 1 < H) v1 = *(const float4*)(i1 + 8 * g);
        acc0[4 * g] = v0.x; acc0[4 * g + 1] = v0.y; acc0[4 * g + 2] = v0.z; acc0[4 * g + 3] = v0.w;
        acc1[4 * g] = v1.x; acc1[4 * g + 1] = v1.y; acc1[4 * g + 2] = v1.z; acc1[4 * g + 3] = v1.w;
      }
    }
    constexpr int NR = 12 * NKG;   // fragment reads of a unit, in (row i, dx, kg) order
    constexpr int S_RELU0 = 9 * NKG + (NKG >= 2 ? 2 : 1);         // acc0's last MFMA is consume step 9*NKG - 1
    u32x4_t xb[PF];
    auto step = [&](auto s_c) {
      constexpr int s = decltype(s_c)::value;
      if constexpr (s < NR) {
        constexpr int i = s / (3 * NKG), dx = (s / NKG) % 3, kg = s % NKG;   // input row key q = BR*it + 2*RPI + i
        constexpr int ringrow = (BR * PH + 2 * RPI + i) % (3 * BR);
        xb[s % PF] = lds_frag<ringrow * ROWB, PIPE>(lds0 + (xa[dx] ^ (kg << 5)));
      }
      if constexpr (s >= PF - 1) {
        constexpr int c = s - (PF - 1);
        constexpr int i = c / (3 * NKG), dx = (c / NKG) % 3, kg = c % NKG;
        constexpr int young = (NR - 1 - c) < (PF - 1) ? (NR - 1 - c) : (PF - 1);
        if constexpr (PIPE) lds_wait<young>(xb[c % PF]);
        const uint4 xv = __builtin_bit_cast(uint4, xb[c % PF]);
        if constexpr (i <= 2) acc0 = Mma<T>::run(w[i * 3 + dx][kg], xv, acc0);
        if constexpr (i >= 1) acc1 = Mma<T>::run(w[(i - 1) * 3 + dx][kg], xv, acc1);
        if constexpr (EARLY_RELU && c == S_RELU0) {   // rows 0..2 of acc0 are complete: its ReLU hides under acc1's last MFMAs
#pragma unroll
          for (int e = 0; e < 16; ++e) acc0[e] = relu1(acc0[e], rlim);
        }
      }
    };
    if (!ACCIN) {  // bias is the accumulator's initial value (EPI_RAW partial sums carry it into the ACCIN launch)
      const unsigned ba = lds0 + C::RING_BYTES + (nsl * 32 + 4 * h) * 4;
      u32x4_t b0 = lds_frag<0, PIPE>(ba), b1 = lds_frag<32, PIPE>(ba), b2 = lds_frag<64, PIPE>(ba), b3 = lds_frag<96, PIPE>(ba);
      static_for(std::make_integer_sequence<int, PF - 1>{}, step);   // first fragment reads go out behind the bias reads
      if constexpr (PIPE) lds_wait4<PF - 1>(b0, b1, b2, b3);
      const u32x4_t bq[4] = {b0, b1, b2, b3};
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc0[4 * g + e] = acc1[4 * g + e] = __uint_as_float(bq[g][e]);
    } else {
      static_for(std::make_integer_sequence<int, PF - 1>{}, step);
    }
    static_for(std::make_integer_sequence<int, NR>{}, [&](auto s_c) {
      step(std::integral_constant<int, decltype(s_c)::value + PF - 1>{});
    });

    stamp(1);
    // ---- fused epilogue.  Register i <-> channel nb + (i&3) + 8*(i>>2) + 4*h of pixel (row, col).
    if (EPI == EPI_POOL_H2) {
      const int Ho = H >> 1, to = t0 >> 1;
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = (EARLY_RELU ? acc0[i] : relu1(acc0[i], rlim)) + relu1(acc1[i], rlim);   // 1/2 is in the weights
      T* o = (T*)a.out + (((size_t)b * Ho + to) * W + col) * COUT + nb;
      const bool ok = (to < Ho) && col_ok;
      if (sizeof(T) == 4) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (ok) *(float4*)((float*)o + 8 * g + 4 * h) = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
      } else {
#pragma unroll
        for (int g = 0; g < 4; g += 2) {  // groups (g, g+1): swap halves so each lane owns 8 consecutive channels
          const unsigned a0 = pack_bf16x2(v[4 * g], v[4 * g + 1]), a1 = pack_bf16x2(v[4 * g + 2], v[4 * g + 3]);
          const unsigned b0 = pack_bf16x2(v[4 * g + 4], v[4 * g + 5]), b1 = pack_bf16x2(v[4 * g + 6], v[4 * g + 7]);
          const auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          // lanes < 32: [own g | upper's g] = channels 8g..8g+7; lanes >= 32: [lower's g+1 | own g+1] = 8g+8..8g+15
          if (ok) *(uint4*)((bf16_t*)o + 8 * g + 8 * h) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
        }
      }
    } else if (EPI == EPI_POOL_2X2) {
      const int Ho = H >> 1, Wo = W >> 1, to = t0 >> 1;
      const int Hop = RAGGED ? a.H >> 1 : Ho;     // row pitch of the output
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float s = (EARLY_RELU ? acc0[i] : relu1(acc0[i], rlim)) + relu1(acc1[i], rlim);      // 1/4 is in the weights
        v[i] = s + __shfl_xor(s, 1, 64);                                  // + the neighbouring column (lane r ^ 1)
      }
      const int fo = col >> 1;
      if (to < Ho && fo < Wo && (r & 1) == 0) {
        T* o = (T*)a.out + (((size_t)b * Hop + to) * Wo + fo) * COUT + nb;
        if (sizeof(T) == 4) {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(float4*)((float*)o + 8 * g + 4 * h) = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(uint2*)((bf16_t*)o + 8 * g + 4 * h) =
                make_uint2(pack_bf16x2(v[4 * g], v[4 * g + 1]), pack_bf16x2(v[4 * g + 2], v[4 * g + 3]));
        }
      }
    } else if (EPI == EPI_MEAN_T) {
      if (t0 + 1 < H) {          // wave-uniform: only the last row pair of an odd H takes the other branch
#pragma unroll
        for (int i = 0; i < 16; ++i) cs[i] += (EARLY_RELU ? acc0[i] : relu1(acc0[i], rlim)) + relu1(acc1[i], rlim);
      } else if (t0 < H) {
#pragma unroll
        for (int i = 0; i < 16; ++i) cs[i] += (EARLY_RELU ? acc0[i] : relu1(acc0[i], rlim));
      }
    } else if (EPI == EPI_RAW) {
      float* o0 = a.raw_out + (((size_t)b * H + t0) * W + col) * COUT + nb + 4 * h;
      float* o1 = o0 + (size_t)W * COUT;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (col_ok && t0 < H)
          *(float4*)(o0 + 8 * g) = make_float4(acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]);
        if (col_ok && t0 + 1 < H)
          *(float4*)(o1 + 8 * g) = make_float4(acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]);
      }
    } else {  // EPI_PLAIN
      const bool r0ok = col_ok && t0 < H, r1ok = col_ok && t0 + 1 < H;
      float v0[16], v1[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {     // (the statistics forms are pre-BatchNorm outputs: never a ReLU, launcher-checked)
        v0[i] = (!STATS && a.relu) ? relu1(acc0[i], rlim) : acc0[i];
        v1[i] = (!STATS && a.relu) ? relu1(acc1[i], rlim) : acc1[i];
      }
      if (STATS) {
        // Per-lane sums over the rows this lane's COLUMN walks; whether the column counts is a property of the lane, applied
        // once in front of the cross-lane reduction below (a select, so whatever a masked lane accumulated -- its operands
        // are staged zeros here, but were stray LDS bytes in the 30-column experiment -- cannot reach a sum).  Rows past
        // the image are wave-uniform.  4 VALU operations per element pair instead of 7: this epilogue was as long as the
        // unit's 18 MFMAs.
        if (t0 + 1 < H) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            st1[i] += v0[i] + v1[i];
            st2[i] = fmaf(v0[i], v0[i], fmaf(v1[i], v1[i], st2[i]));
          }
        } else if (t0 < H) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            st1[i] += v0[i];
            st2[i] = fmaf(v0[i], v0[i], st2[i]);
          }
        }
      }
      T* o0 = (T*)a.out + (((size_t)b * H + t0) * W + col) * COUT + nb;
      T* o1 = o0 + (size_t)W * COUT;
      if (sizeof(T) == 4) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if (r0ok) *(float4*)((float*)o0 + 8 * g + 4 * h) = make_float4(v0[4 * g], v0[4 * g + 1], v0[4 * g + 2], v0[4 * g + 3]);
          if (r1ok) *(float4*)((float*)o1 + 8 * g + 4 * h) = make_float4(v1[4 * g], v1[4 * g + 1], v1[4 * g + 2], v1[4 * g + 3]);
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
          unsigned a0 = pack_bf16x2(v0[4 * g], v0[4 * g + 1]), a1 = pack_bf16x2(v0[4 * g + 2], v0[4 * g + 3]);
          unsigned b0 = pack_bf16x2(v0[4 * g + 4], v0[4 * g + 5]), b1 = pack_bf16x2(v0[4 * g + 6], v0[4 * g + 7]);
          auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          if (r0ok) *(uint4*)((bf16_t*)o0 + 8 * g + 8 * h) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
          a0 = pack_bf16x2(v1[4 * g], v1[4 * g + 1]); a1 = pack_bf16x2(v1[4 * g + 2], v1[4 * g + 3]);
          b0 = pack_bf16x2(v1[4 * g + 4], v1[4 * g + 5]); b1 = pack_bf16x2(v1[4 * g + 6], v1[4 * g + 7]);
          s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
          s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
          if (r1ok) *(uint4*)((bf16_t*)o1 + 8 * g + 8 * h) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
        }
      }
    }
  };

  // one iteration at ring phase PH: prefetch block it+2, run this wave's units, publish the prefetched block
  auto iteration = [&](auto ph_c, int it) {
    constexpr int PH = decltype(ph_c)::value;
    const bool pf = (it + 1 < niter);
    if (pf) {
      if (DMA) stage_dma(it + 2, (PH + 2) % 3); else stage_load(it + 2);
    }
    stamp(0);
#pragma unroll
    for (int uu = 0; uu < C::UPW; ++uu) {
      if (MG == 1) {
        if (uu == 0) unit(ph_c, std::integral_constant<int, 0>{}, it);
        if (uu == 1) unit(ph_c, std::integral_constant<int, 1>{}, it);
      } else {  // MG == 2: row pair uu*2 + mg, dispatched on the (wave-uniform) M group
        if (mg == 0) {
          if (uu == 0) unit(ph_c, std::integral_constant<int, 0>{}, it);
          if (uu == 1) unit(ph_c, std::integral_constant<int, 2>{}, it);
        } else {
          if (uu == 0) unit(ph_c, std::integral_constant<int, 1>{}, it);
          if (uu == 1) unit(ph_c, std::integral_constant<int, 3>{}, it);
        }
      }
    }
    stamp(2);
    if (pf && !DMA) stage_store((PH + 2) % 3);
    if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA pieces of block it+2 have landed
    stamp(3);
    __syncthreads();
    stamp(4);
  };
  static_assert(C::UPW <= 2 && MG <= 2, "unit dispatch above covers UPW <= 2, MG <= 2");

  stamp(5);   // prologue
  for (int it = 0; it < niter; it += 3) {
    iteration(std::integral_constant<int, 0>{}, it);
    if (it + 1 < niter) iteration(std::integral_constant<int, 1>{}, it + 1);
    if (it + 2 < niter) iteration(std::integral_constant<int, 2>{}, it + 2);
  }

#ifdef DFA_STAMPS
  if (lane == 0 && blockIdx.x < 2048 && (EPI == EPI_MEAN_T || STATS)) {
    long long* d = g_diag + ((size_t)blockIdx.x * 4 + (wave & 3)) * 8;
    for (int k = 0; k < 6; ++k) d[k] = seg[k];
    d[6] = t_begin;
    d[7] = __builtin_amdgcn_s_memtime();
  }
#endif
  if (STATS && a.stats_partial) {
    // per-channel sums: reduce over the 32 pixel lanes of each half-wave, then over the M groups through LDS
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      st1[i] = col_ok ? st1[i] : 0.f;       // lanes whose column lies outside the image (or the strip) do not count
      st2[i] = col_ok ? st2[i] : 0.f;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        st1[i] += __shfl_xor(st1[i], off, 64);
        st2[i] += __shfl_xor(st2[i], off, 64);
      }
    }
    float* red = (float*)(smem + C::RING_BYTES + C::BIAS_BYTES);
    if (r == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = (i & 3) + 8 * (i >> 2) + 4 * h;
        red[((mg * NSL + nsl) * 32 + c) * 2] = st1[i];
        red[((mg * NSL + nsl) * 32 + c) * 2 + 1] = st2[i];
      }
    }
    __syncthreads();
    if (tid < NSL * 32) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int g = 0; g < MG; ++g) { s1 += red[(g * NSL * 32 + tid) * 2]; s2 += red[(g * NSL * 32 + tid) * 2 + 1]; }
      float* dst = a.stats_partial + ((size_t)(blockIdx.x * gridDim.y + blockIdx.y) * (NSL * 32) + tid) * 2;
      dst[0] = s1;
      dst[1] = s2;
    }
  }
  if (EPI == EPI_MEAN_T) {
    // embedding rows: for each channel the 32 lanes of a half-wave hold 32 consecutive feature columns
    if (col_ok) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = nb + (i & 3) + 8 * (i >> 2) + 4 * h;
        a.emb[((size_t)b * COUT + c) * W + col] = cs[i] * a.inv_h;
      }
    }
  }

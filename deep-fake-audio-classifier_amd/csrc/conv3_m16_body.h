// conv3_m16_body.h -- the body of conv3_m16.hip's block-3 kernels, included INSIDE each __global__ function with PIPE, TRAIN,
// RAGGED (compile-time bools), `a` (ConvArgs) and `rt` (RaggedTab) in scope: one source for the uniform, train and ragged
// forms.  (As a __device__ function inlined into the kernels the same body compiled to different registers -- 52 bytes of
// scratch per lane in the pipelined eval kernel against 12 -- so it is textual; the uniform kernels are instruction for
// instruction what they were as single functions.)
#ifndef DFA_KERNEL_BODY_SCOPE
#error "conv3_m16_body.h is a kernel body: include it only inside the __global__ functions of conv3_m16.hip"
#endif
  static_assert(std::is_same<decltype(RAGGED), const bool>::value, "the including kernel defines constexpr bool RAGGED");
  using namespace m16;
  constexpr int PF = 4;                  // fragment reads in flight (train form: 2 -> 4 was worth 2 % once the file was built without SLP)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nsl = wave;
  const int p = lane & 15, q = lane >> 4;

  const int logical = xcd_logical_workgroup();
  const int u = logical / a.nstrips, strip = logical - u * a.nstrips;
  const int b = RAGGED ? __builtin_amdgcn_readfirstlane(rt.tab[rt.B + u]) : u;
  const int f0 = strip * SW;
  const int H = RAGGED ? __builtin_amdgcn_readfirstlane(rt.tab[b]) / 4 : a.H, W = a.W, COUT = a.COUT;
  const int cout_base = blockIdx.y * (NSL * 32);
  const char* in_b = (const char*)a.in + (size_t)b * a.H * W * PB;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const float rlim = relu_limit();

  // ---- weights [tap][kk][ca]: 36 fragments = 144 VGPRs for the kernel's lifetime
  uint4 w[9][2][2];
  {
    const uint4* wp = a.wpack + (size_t)(blockIdx.y * NSL + nsl) * 9 * 2 * 2 * 64 + lane;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int ca = 0; ca < 2; ++ca) w[tap][kk][ca] = wp[((tap * 2 + kk) * 2 + ca) * 64];
  }
  float* bias_lds = (float*)(smem + RING_BYTES);
  if (tid < NSL * 32) bias_lds[tid] = a.bias[cout_base + tid];

  // per-lane fragment offsets inside a ring row: slot = p + dx (+16 for the second pixel tile = +2048 bytes, swizzle
  // unchanged), logical chunk 4*kk + q -> kk is one XOR with 64
  int xa[3];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx) {
    const int slot = p + dx;
    xa[dx] = slot * PB + ((q ^ swz(slot)) << 4);
  }

  // ---- LDS-DMA staging of a ring block (as conv3x3_mfma.h): thread's k-th PHYSICAL chunk, swizzle in the source address
  int s_off[NLD];
#pragma unroll
  for (int k = 0; k < NLD; ++k) {
    const int g = k * NT + tid;
    const int rowi = g / (SP * CPP), rem = g - rowi * (SP * CPP);
    const int slot = rem / CPP, cph = rem % CPP;
    const int c = cph ^ swz(slot);
    const int f = f0 - 1 + slot;
    const bool ok = (f >= 0) && (f < W);
    s_off[k] = ok ? (rowi * W + f) * PB + c * 16 : -1;
  }
  auto stage_dma = [&](int j, int ringblk) {
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
      const int g = k * NT + tid;
      static_assert(NCH == NLD * NT, "a ring block is exactly NLD 1-KiB pieces per wave: no conditional piece");
      {
        const int t = BR * j - 1 + g / (SP * CPP);
        const char* src = (s_off[k] >= 0 && t >= 0 && t < H) ? in_b + (ptrdiff_t)(BR * j - 1) * W * PB + s_off[k]
                                                             : (const char*)a.zero_page;
        char* dst = smem + ringblk * BR * ROWB + (k * NT + wave * 64) * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      }
    }
  };

  f32x4_t cs[2][2];     // eval: running column sums [channel tile][pixel tile]; TRAIN: [0][ca] = sum, [1][ca] = sum of squares
#pragma unroll
  for (int ca = 0; ca < 2; ++ca)
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) cs[ca][pb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int niter_all = (H + BR - 1) / BR;
  const int rchunk = RAGGED ? __builtin_amdgcn_readfirstlane(rt.tab[3 * rt.B + b]) : 0;   // the utterance's canonical chunk
  const int seg = RAGGED ? rchunk : a.seg_iters;
  // small batches: blockIdx.z walks its own segment [it0, niter) of the time axis (it0 a multiple of the ring period)
  const int it0 = a.seg_iters ? (int)blockIdx.z * seg : 0;
  const int niter = a.seg_iters ? min(niter_all, it0 + seg) : niter_all;
  if constexpr (RAGGED) {     // a chunk past the end of a short utterance: nothing to do (workgroup-uniform)
    if (it0 >= niter_all) return;
  }
  stage_dma(it0, 0);
  stage_dma(it0 + 1, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  auto unit = [&](auto ph_c, int it) {
    constexpr int PH = decltype(ph_c)::value;
    const int t0 = BR * it;
    f32x4_t acc0[2][2], acc1[2][2];
    constexpr int NR = 4 * 3 * 2 * 2;   // fragment reads in (row i, dx, kk, pb) order
    constexpr int C_RELU0 = 36 + 3;     // acc0's last MFMAs belong to read 35
    constexpr int S_BAR = 4;
    u32x4_t xbuf[PF];
    auto step = [&](auto s_c) {
      constexpr int s = decltype(s_c)::value;
      if constexpr (s < NR) {
        constexpr int i = s / 12, dx = (s / 4) % 3, kk = (s / 2) % 2, pb = s % 2;
        constexpr int ringrow = (BR * PH + i) % (3 * BR);
        xbuf[s % PF] = lds_frag<ringrow * ROWB + pb * 16 * PB, PIPE>(lds0 + (xa[dx] ^ (kk << 6)));
        if constexpr (s == S_BAR) {
          // The iteration's barrier stands here, behind the unit's first fragment reads (rows of ring block `it`, published
          // two barriers ago), so the pipeline fill overlaps the wait for the slower waves.  Behind it: the LDS-DMA of block
          // it+2 (overwrites the block the previous unit read) and, from read 24 on, the rows of block it+1 (DMA'd during the
          // previous unit: every wave waits for its own pieces, vmcnt(0), before the barrier).
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if constexpr (PIPE) asm volatile("s_barrier" ::: "memory");
          else __syncthreads();
          if (it + 1 < niter) stage_dma(it + 2, (PH + 2) % 3);
        }
      }
      if constexpr (s >= PF - 1) {
        constexpr int c = s - (PF - 1);
        constexpr int i = c / 12, dx = (c / 4) % 3, kk = (c / 2) % 2, pb = c % 2;
        constexpr int young = (NR - 1 - c) < (PF - 1) ? (NR - 1 - c) : (PF - 1);
        if constexpr (PIPE) lds_wait<young>(xbuf[c % PF]);
        const uint4 xv = __builtin_bit_cast(uint4, xbuf[c % PF]);
#pragma unroll
        for (int ca = 0; ca < 2; ++ca) {
          if constexpr (i <= 2) acc0[ca][pb] = mma16(w[i * 3 + dx][kk][ca], xv, acc0[ca][pb]);
          if constexpr (i >= 1) acc1[ca][pb] = mma16(w[(i - 1) * 3 + dx][kk][ca], xv, acc1[ca][pb]);
        }
        if constexpr (!TRAIN && c == C_RELU0) {   // rows 0..2 done for acc0: its ReLU hides under acc1's last MFMAs
#pragma unroll
          for (int ca = 0; ca < 2; ++ca)
#pragma unroll
            for (int pb2 = 0; pb2 < 2; ++pb2)
#pragma unroll
              for (int e = 0; e < 4; ++e) acc0[ca][pb2][e] = relu1(acc0[ca][pb2][e], rlim);
        }
      }
    };
    {   // bias = accumulator init: channels 16*ca + 4*q + e of this wave's slice
      const unsigned ba = lds0 + RING_BYTES + (nsl * 32 + 4 * q) * 4;
      u32x4_t b0 = lds_frag<0, PIPE>(ba), b1 = lds_frag<64, PIPE>(ba);
      static_for(std::make_integer_sequence<int, PF - 1>{}, step);
      if constexpr (PIPE) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(b0), "+v"(b1) : "n"(PF - 1));
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        acc0[0][pb] = acc1[0][pb] = __builtin_bit_cast(f32x4_t, b0);
        acc0[1][pb] = acc1[1][pb] = __builtin_bit_cast(f32x4_t, b1);
      }
    }
    static_for(std::make_integer_sequence<int, NR>{}, [&](auto s_c) {
      step(std::integral_constant<int, decltype(s_c)::value + PF - 1>{});
    });
    if constexpr (TRAIN) {
      const bool r0 = t0 < H, r1 = t0 + 1 < H;                    // wave-uniform
      // statistics of the fp32 accumulators (as the 32x32x16 kernel); rows / columns outside the image do not count
#pragma unroll
      for (int pb = 0; pb < 2; ++pb) {
        const bool cok = 16 * pb + p < SW && f0 + 16 * pb + p < W;
#pragma unroll
        for (int ca = 0; ca < 2; ++ca) {
          if (cok && r0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { cs[0][ca][e] += acc0[ca][pb][e]; cs[1][ca][e] = fmaf(acc0[ca][pb][e], acc0[ca][pb][e], cs[1][ca][e]); }
          }
          if (cok && r1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { cs[0][ca][e] += acc1[ca][pb][e]; cs[1][ca][e] = fmaf(acc1[ca][pb][e], acc1[ca][pb][e], cs[1][ca][e]); }
          }
        }
      }
      // z stores: v_permlane16_swap between the two pixel tiles hands every lane 8 consecutive channels of ONE pixel --
      // quarter-wave rows q = 0 / 2 keep tile 0 (channels 8*(q/2) .. +7 of the 16-channel tile), rows 1 / 3 take tile 1 --
      // so z leaves as 16-byte stores (4 per lane and unit instead of 8 of 8 bytes)
      const int tile = q & 1;
      const int col = f0 + 16 * tile + p;
      bf16_t* zb = (bf16_t*)a.out + (((size_t)b * H + t0) * W + col) * COUT + cout_base + nsl * 32 + 8 * (q >> 1);
#pragma unroll
      for (int ca = 0; ca < 2; ++ca) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const f32x4_t v0 = r ? acc1[ca][0] : acc0[ca][0], v1 = r ? acc1[ca][1] : acc0[ca][1];
          const auto d0 = __builtin_amdgcn_permlane16_swap(pack_bf16x2(v0[0], v0[1]), pack_bf16x2(v1[0], v1[1]), false, false);
          const auto d1 = __builtin_amdgcn_permlane16_swap(pack_bf16x2(v0[2], v0[3]), pack_bf16x2(v1[2], v1[3]), false, false);
          if (16 * tile + p < SW && col < W && (r ? r1 : r0)) *(uint4*)(zb + (size_t)r * W * COUT + 16 * ca) = make_uint4(d0[0], d1[0], d0[1], d1[1]);
        }
      }
    } else
    if (t0 + 1 < H) {   // wave-uniform
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int e = 0; e < 4; ++e) cs[ca][pb][e] += acc0[ca][pb][e] + relu1(acc1[ca][pb][e], rlim);
    } else if (t0 < H) {
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
          for (int e = 0; e < 4; ++e) cs[ca][pb][e] += acc0[ca][pb][e];
    }
  };

  auto iteration = [&](auto ph_c, int it) { unit(ph_c, it); };      // (DMA issue, DMA wait and the barrier are inside the unit)
  // eval: total over the canonical chunks.  Element k of thread tid lives at [k][tid] (16-byte stride between lanes): the
  // [tid][k] order of round 2 put lanes 64 B apart, a 4-way bank conflict on every ds_read/write_b128 -- the source of block 3's
  // SQ_LDS_BANK_CONFLICT (4.4 M of 55 M LDS cycles, profiles/r02_sq_summary.csv; the fragment reads are conflict-free).
  f32x4_t* const tot = (f32x4_t*)(smem + RING_BYTES + BIAS_BYTES) + tid;
  if constexpr (!TRAIN) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k * NT] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  // outer loop over the canonical chunks of the time mean (chunk_iters iterations, a multiple of 6; one chunk = the whole
  // walk when unset), inner loop = the ring walk itself, unchanged; a chunk's sum is flushed once, outside the hot loop
  const int chunk = RAGGED ? rchunk : (!TRAIN && a.chunk_iters > 0) ? a.chunk_iters : niter_all + 3;
#ifdef DFA_STAMPS
  const long long st_c = __builtin_amdgcn_s_memtime(), st_r = __builtin_amdgcn_s_memrealtime();
#else
  long long st_c = 0, st_r = 0;          // production build: the runtime held-clock probe (ConvArgs::clock_stamps)
  const bool probe = !TRAIN && a.clock_stamps != nullptr;
  if (probe) {
    st_c = __builtin_amdgcn_s_memtime();
    st_r = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): no scalar-memory return may be outstanding inside the counted LDS pipeline
  }
#endif
  for (int c0 = it0; c0 < niter; c0 += chunk) {
    const int cend = min(niter, c0 + chunk);
    for (int it = c0; it < cend; it += 3) {
      iteration(std::integral_constant<int, 0>{}, it);
      if (it + 1 < cend) iteration(std::integral_constant<int, 1>{}, it + 1);
      if (it + 2 < cend) iteration(std::integral_constant<int, 2>{}, it + 2);
    }
    if constexpr (!TRAIN) {
      if (a.seg_iters) {                                 // split: the chunk sum (unscaled) goes to its own slab
        float* e0 = a.emb + (size_t)(c0 / chunk) * a.emb_seg_stride;
#pragma unroll
        for (int ca = 0; ca < 2; ++ca)
#pragma unroll
          for (int pb = 0; pb < 2; ++pb) {
            const int col = f0 + 16 * pb + p;
            if (16 * pb + p < SW && col < W) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                e0[((size_t)b * COUT + cout_base + nsl * 32 + 16 * ca + 4 * q + e) * W + col] = cs[ca][pb][e];
            }
          }
      } else {
#pragma unroll
        for (int ca = 0; ca < 2; ++ca)
#pragma unroll
          for (int pb = 0; pb < 2; ++pb) tot[(ca * 2 + pb) * NT] += cs[ca][pb];
      }
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) cs[ca][pb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
  }
#ifdef DFA_STAMPS
  if (tid == 0 && blockIdx.y == 0 && blockIdx.z == 0 && blockIdx.x < 4096) {
    g_diag16[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - st_c;
    g_diag16[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - st_r;
  }
#else
  if (probe && tid == 0 && blockIdx.y == 0 && blockIdx.z == 0 && blockIdx.x < 1024) {
    a.clock_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - st_c;
    a.clock_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - st_r;
  }
#endif

  if constexpr (TRAIN) {
    // per-channel sums over this workgroup's pixels: the 16 pixel lanes of a quarter-wave hold the same 8 channels
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = cs[k][ca][e];
#pragma unroll
          for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
          cs[k][ca][e] = v;
        }
    if (p == 0 && a.stats_partial) {
      float* dst = a.stats_partial + ((size_t)(blockIdx.x * gridDim.y + blockIdx.y) * (NSL * 32) + nsl * 32 + 4 * q) * 2;
#pragma unroll
      for (int ca = 0; ca < 2; ++ca)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dst[(16 * ca + e) * 2] = cs[0][ca][e];
          dst[(16 * ca + e) * 2 + 1] = cs[1][ca][e];
        }
    }
    return;
  }
  if (a.seg_iters) return;       // split: the chunk sums are out; the classifier kernel adds and scales them
  const float inv_h = RAGGED ? __uint_as_float(rt.tab[2 * rt.B + b]) : a.inv_h;
  // embedding rows [b][channel][col]: 16 consecutive columns per (channel, quarter-wave)
#pragma unroll
  for (int ca = 0; ca < 2; ++ca)
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
      const int col = f0 + 16 * pb + p;
      const f32x4_t tv = tot[(ca * 2 + pb) * NT];
      if (16 * pb + p < SW && col < W) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = cout_base + nsl * 32 + 16 * ca + 4 * q + e;
          a.emb[((size_t)b * COUT + c) * W + col] = tv[e] * inv_h;
        }
      }
    }

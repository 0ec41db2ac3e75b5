// cnn1d_x3_body.h -- the body of cnn1d_fused_x3.hip's two forward kernels, included INSIDE each __global__ function with `a`
// (Cnn1dX3Args) in scope and C1X_RAGGED defined as 0 (cnn1d_fused_x3_kernel: every utterance has a.T frames and the contiguous
// [F][T] storage) or 1 (cnn1d_ragged_x3_kernel, with `rg` (Cnn1dRaggedArgs) in scope as well: the workgroup's utterance and its
// length T_b come from the ragged table, rows are read at the pitch of the padded batch, and an utterance longer than one LDS
// window is walked in time segments).  One source for both forms, textual rather than a __device__ function so that the uniform kernel stays
// instruction for instruction what it was.
//
// Ragged form, per segment (cnn1d_ragged_segment, a function of T_b and F only): the window [w0, w0 + T) of the utterance is
// what the uniform body calls the utterance -- `T` below is the WINDOW length and every LDS offset is that of
// cnn1d_x3_layout(T) -- and only the layer-3 frames [olo, ohi) of the window (the frames the segment owns) enter the sums.
// Frames outside [0, T_b) are the zero slots the body keeps anyway; at an interior window edge those zeros are wrong inputs,
// which reach at most 3 frames into the window, and the owned range starts 4 frames / ends 3 frames inside such an edge.
//
// C1X_K1 = taps of layer 1: 3, or 5 for the k = (5, 3, 3) variant (cnn1d_fused_x3.hip has what that changes; here every such
// place is an #if, so that the three-tap kernels keep their text).  With five taps the wrong inputs of an interior edge reach
// 4 frames, and the owned range ends 4 frames inside one.
#ifndef DFA_KERNEL_BODY_SCOPE
#error "cnn1d_x3_body.h is a kernel body: include it only inside the __global__ functions of cnn1d_fused_x3.hip"
#endif
  using namespace c1x;
  extern __shared__ __attribute__((aligned(16))) char smem[];
#if C1X_RAGGED
  const int b = __builtin_amdgcn_readfirstlane(rg.rt.tab[rg.rt.B + blockIdx.x]);   // dispatch slot -> utterance (longest first)
  const int TB = __builtin_amdgcn_readfirstlane(rg.rt.tab[b]);                     // its own length: wave-uniform, like all below
  const int nseg = cnn1d_ragged_nseg(TB, rg.seg_step, rg.wcap);
  float part = 0.f;                                        // the classifier's partial dot product runs on across the segments
  for (int seg = 0; seg < nseg; ++seg) {
  // The thread index is made opaque per segment: everything a lane derives from it (addresses, swizzles, masks) is then computed
  // inside the segment where the uniform kernel computes it.  Seen as loop-invariant it was all hoisted in front of the loop and,
  // on a kernel that already fills its 256 registers, spilled (392 bytes of scratch per lane).
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));
  __builtin_assume(tid_ >= 0 && tid_ < NTH);
  const int tid = tid_, lane = tid & 63;
  int w0, T, olo, ohi;                                     // window start (a multiple of 4), window length, owned frames of the window
#if C1X_K1 == 5
  cnn1d_ragged_segment(TB, rg.seg_step, rg.wcap, seg, &w0, &T, &olo, &ohi, 4);
#else
  cnn1d_ragged_segment(TB, rg.seg_step, rg.wcap, seg, &w0, &T, &olo, &ohi);
#endif
  const int NT = (T + 31) / 32, P = (T + 3) & ~3, n4r = P >> 2;   // P: row pitch of a slab in LDS, n4r float4 per row
  int offB, offS, offH2, slab_fl, lds_total;
#if C1X_K1 == 5
  cnn1d_x3_layout(T, a.F, 1, &offB, &lds_total, &slab_fl, &offS, &offH2, 5);
#else
  cnn1d_x3_layout(T, a.F, 1, &offB, &lds_total, &slab_fl, &offS, &offH2);
#endif
  const bool first_seg = seg == 0, last_seg = seg == nseg - 1;
  // (loads through these pointers stay inside the segment: hoisted out of the loop, the 176 registers of weight fragments,
  //  biases and classifier weights were spilled to scratch at the top of the kernel)
  const uint4 *w2p = a.w2, *w3p = a.w3;
  const float *b3p = a.b3, *cwp = a.cw;
  asm volatile("" : "+s"(w2p), "+s"(w3p), "+s"(b3p), "+s"(cwp));
#define C1X_OFFB offB
#define C1X_OFFS offS
#define C1X_OFFH2 offH2
#define C1X_SLAB slab_fl
#define C1X_W2 w2p
#define C1X_W3 w3p
#define C1X_B3 b3p
#define C1X_CW cwp
#else
  const int b = blockIdx.x;
  const int T = a.T, NT = a.NT;
  const int TB = T, P = T;
  const int tid = threadIdx.x, lane = tid & 63;
  constexpr bool first_seg = true, last_seg = true;
#define C1X_OFFB a.offB
#define C1X_OFFS a.offS
#define C1X_OFFH2 a.offH2
#define C1X_SLAB a.slab_floats
#define C1X_W2 a.w2
#define C1X_W3 a.w3
#define C1X_B3 a.b3
#define C1X_CW a.cw
#endif
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int nslots = 32 * NT + 2;
#if C1X_K1 == 5
  constexpr int KT = 5, HL = 2;                             // layer 1: taps, halo slots per side of a split image
  const int nslots1 = 32 * NT + 4;
#else
  constexpr int KT = 3, HL = 1;
#define nslots1 nslots                                      // (a name, not a second variable: the three-tap kernels compile to what they were)
#endif
  float* const slab0 = (float*)smem;                      // two slabs of slab_floats floats: [4 pad][16 x T][4 pad]
  char* const h1S = smem;                                 // region A again, after layer 1: [nslots][128 B]
  char* const w1S = smem + C1X_OFFB;                        // region B: layer-1 A fragments [3][nks1][2][64] x 16 B ...
  char* const h2S = smem + C1X_OFFH2;                       // h2 [nslots][256 B]: behind h1, over the (then dead) slab / weight regions
  float* const red = (float*)(smem + C1X_OFFH2 + nslots * 256);
  const bool stamp = a.stamps != nullptr && tid == 0 && b < 128;
  if (stamp && first_seg) { a.stamps[8 * b] = __builtin_amdgcn_s_memtime(); a.stamps[8 * b + 5] = __builtin_amdgcn_s_memrealtime(); }

  // ------------------------------------------------------------------------------------------------ layer 1: F -> 32
  // A slab (16 channels x T frames, fp32, contiguous) goes global -> registers -> LDS as it is (F buffers), is then SPLIT ONCE
  // into a pixel image S[slot = frame + 1][hi: 16 ch bf16 | lo: 16 ch bf16] (64 bytes per frame, the chunk swizzle of the
  // h1 / h2 images; halo slots and the slots beyond T stay zero), and the tiles read their three taps from that image as two
  // ds_read_b128 each.  The first version split x[c][t-1..t+1] per lane and tap -- every element three times, plus six masks per
  // tile -- and layer 1 was bound by that vector work (51 k of the kernel's 86 k cycles for 13.8 k cycles of matrix-pipe time).
  // Pipeline per trip s (one barrier): compute slab s from S[s & 1] | split slab s + 1: F[(s+1) & 1] -> S[(s+1) & 1] | park slab
  // s + 2 (registers) in F[s & 1] | request slab s + 4.
  const int nks1 = a.nks1;
  f32x16_t acc1[MAXT1];
  {
#if C1X_RAGGED
    // utterance b's rows start at x + b stride_b, one every stride_f floats (the padded batch's pitch); the window starts w0 in
    const float4* xg = (const float4*)(a.x + (size_t)b * rg.stride_b + w0);
    const int sf4 = rg.stride_f >> 2;
    const unsigned rdiv = ((1u << 20) + n4r - 1) / n4r;      // i / n4r = (i * rdiv) >> 20 for i < 1536, n4r <= 96
#else
    const float4* xg = (const float4*)(a.x + (size_t)b * a.F * T);
#endif
    const int SL = C1X_SLAB;
    char* const S0 = smem + C1X_OFFS;                          // two split images of nslots x 64 bytes
    const int SB = nslots1 * 64;
    constexpr int NLD = 3;                                   // 16 T / 4 float4 per slab <= 1536 = 3 x 512
    float4 xrA[NLD], xrB[NLD];                                // even / odd slabs in flight
    const int nreal = (a.F + 15) / 16;                        // slabs that exist (nks1 may be one more: a zero slab)
#if C1X_RAGGED
    auto slab_n4 = [&](int s) { return max(0, min(16, a.F - 16 * s)) * n4r; };
#else
    auto slab_n4 = [&](int s) { return max(0, min(16, a.F - 16 * s)) * T / 4; };
#endif
    auto slab_load = [&](int s, float4 (&xr)[NLD]) {          // unconditional, clamped index (a conditional load is an exec branch
      const int sc = min(s, nreal - 1), n4 = slab_n4(sc);    //  and hipcc's vmcnt bookkeeping across a branch is conservative)
#if C1X_RAGGED
      // item i = (row r, float4 q of the row): 16-byte loads at row pitch.  The last float4 of a row may cover up to three
      // padding floats of the SAME row (stride_f >= 4 ceil(T_b / 4)); slab_park masks them.  Rows the slab lacks re-read row r & 3
      // (F % 4 == 0: it exists), items past the slab its last one: never another utterance, never past a row's pitch.
      const float4* src = xg + (size_t)(16 * sc) * sf4;
      const int nch = min(16, a.F - 16 * sc);
      (void)n4;
#pragma unroll
      for (int k = 0; k < NLD; ++k) {
        const int i = min(k * NTH + tid, 16 * n4r - 1);
        const int r = (int)(((unsigned)i * rdiv) >> 20), q = i - r * n4r;
        xr[k] = src[(r < nch ? r : (r & 3)) * sf4 + q];
      }
#else
      const float4* src = xg + (size_t)4 * sc * T;
#pragma unroll
      for (int k = 0; k < NLD; ++k) xr[k] = src[min(k * NTH + tid, n4 - 1)];
#endif
    };
    auto slab_park = [&](int s, const float4 (&xr)[NLD]) {    // registers -> F[s & 1]; channels a short / padded slab lacks become zeros
      float* dst = slab0 + (s & 1) * SL + 4;
      const int n4 = slab_n4(s);
#pragma unroll
      for (int k = 0; k < NLD; ++k) {
        const int i = k * NTH + tid;
        const unsigned m = i < n4 ? 0xffffffffu : 0u;
        const float4 v = xr[k];
#if C1X_RAGGED
        // row r of the slab sits at dst + r P, so item i = r n4r + q lands at dst + 4 i; frames >= T of the row's last float4
        // (its own padding, possibly NaN / Inf, or frames past the window) are ANDed to zero
        const int r = (int)(((unsigned)i * rdiv) >> 20), left = T - 4 * (i - r * n4r);
        const unsigned my = left > 1 ? m : 0u, mz = left > 2 ? m : 0u, mw = left > 3 ? m : 0u;
        if (i < 16 * n4r)
          *(uint4*)(dst + 4 * i) = make_uint4(__float_as_uint(v.x) & m, __float_as_uint(v.y) & my, __float_as_uint(v.z) & mz, __float_as_uint(v.w) & mw);
#else
        if (i < 4 * T)
          *(uint4*)(dst + 4 * i) = make_uint4(__float_as_uint(v.x) & m, __float_as_uint(v.y) & m, __float_as_uint(v.z) & m, __float_as_uint(v.w) & m);
#endif
      }
    };
    auto slab_split = [&](int s) {                            // F[s & 1] -> S[s & 1]: item = (frame t, channel octet g), lanes run along t
      const float* fb = slab0 + (s & 1) * SL + 4;
      char* sb = S0 + (s & 1) * SB;
      // 2 T <= 768 items: one per thread, the remaining 2 T - 512 go to the waves that own ONE frame tile (waves NT - 8 ...: the
      // first NT - 8 waves carry two tiles per trip and would otherwise also carry two items -- every trip ends in a barrier)
      const int t2 = tid - 64 * max(0, NT - NW);
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const int it = pass == 0 ? tid : (t2 >= 0 ? NTH + t2 : 2 * T);
        if (it < 2 * T) {
          const int g = it >= T ? 1 : 0, t = it - g * T;
          float v[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) v[c] = fb[(8 * g + c) * P + t];
          uint4 hi, lo;
          split8(v, hi, lo);
          const int slot = t + HL, sw = lds_swz<64>(slot);
          *(uint4*)(sb + slot * 64 + ((g ^ sw) << 4)) = hi;
          *(uint4*)(sb + slot * 64 + (((2 + g) ^ sw) << 4)) = lo;
        }
      }
    };
#if C1X_K1 == 5
    // one k-step of A fragments = [5 taps][hi | lo][64 lanes] uint4 = 640, contiguous in the k-step-major image: item tid and, for
    // the first 128 threads, item 512 + tid.  Unconditional clamped loads like the slabs'; past the last k-step the last one again.
    constexpr int WKS = KT * 2 * 64;
    uint4 wr0, wr1;                                           // (two scalars: as an array the pair was kept in scratch)
    auto w_load = [&](int s) {
      const uint4* src = a.w1 + (size_t)min(s, nks1 - 1) * WKS;
      wr0 = src[tid];
      wr1 = src[min(NTH + tid, WKS - 1)];
    };
    auto w_park = [&](int s) {                                // registers -> W[s & 1]
      char* dst = w1S + (s & 1) * (WKS * 16);
      *(uint4*)(dst + (size_t)tid * 16) = wr0;
      if (tid < WKS - NTH) *(uint4*)(dst + (size_t)(NTH + tid) * 16) = wr1;
    };
    w_load(0);
#endif
    slab_load(0, xrA);
    slab_load(1, xrB);
    // layer-1 A fragments -> LDS (contiguous copy); the never-written slots of both split images (0 and T + 1 ...) -> zero
    {
#if C1X_K1 == 5
      w_park(0);                                              // (five taps: k-step 0 only; the halo is slots 0, 1 and T + 2 ...)
      w_load(1);
      const int nz = (nslots1 - T) * 4;
      for (int i = tid; i < 2 * nz; i += NTH) {
        const int img = i >= nz, q = i - img * nz, zs = q >> 2;
        const int slot = zs < HL ? zs : T + zs;
        *(uint4*)(S0 + img * SB + slot * 64 + (q & 3) * 16) = make_uint4(0u, 0u, 0u, 0u);
      }
#else
      const int n = 3 * nks1 * 2 * 64;
      for (int i = tid; i < n; i += NTH) *(uint4*)(w1S + (size_t)i * 16) = a.w1[i];
      const int nz = (nslots - T) * 4;                        // 16-byte chunks of the zero slots, per image
      for (int i = tid; i < 2 * nz; i += NTH) {
        const int img = i >= nz, q = i - img * nz, zs = q >> 2;
        const int slot = zs == 0 ? 0 : T + zs;
        *(uint4*)(S0 + img * SB + slot * 64 + (q & 3) * 16) = make_uint4(0u, 0u, 0u, 0u);
      }
#endif
    }
    slab_park(0, xrA);
    slab_load(2, xrA);
    __syncthreads();
    slab_split(0);
    slab_park(1, xrB);
    slab_load(3, xrB);
    __syncthreads();

    const int nmine = (NT - wave + NW - 1) / NW;
#pragma unroll
    for (int j = 0; j < MAXT1; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[j][r] = 0.f;
    auto trip = [&](int s, float4 (&xr)[NLD]) {               // xr: the register set of this trip's parity (holds slab s + 2)
      const char* sb = S0 + (s & 1) * SB;
      uint4 wh[KT], wl[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) {
#if C1X_K1 == 5
        wh[k] = *(const uint4*)(w1S + ((size_t)(((s & 1) * KT + k) * 2) * 64 + lane) * 16);
        wl[k] = *(const uint4*)(w1S + ((size_t)(((s & 1) * KT + k) * 2 + 1) * 64 + lane) * 16);
#else
        wh[k] = *(const uint4*)(w1S + ((size_t)((k * nks1 + s) * 2) * 64 + lane) * 16);
        wl[k] = *(const uint4*)(w1S + ((size_t)((k * nks1 + s) * 2 + 1) * 64 + lane) * 16);
#endif
      }
#if C1X_K1 == 5
      // (five taps: the fragments of BOTH frame tiles are 80 registers and spilled; one tile's are read while the other's MFMAs run)
#pragma unroll
      for (int j = 0; j < MAXT1; ++j) {
        uint4 xh5[KT], xl5[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const int slot = min(TW * (wave + NW * j) + col + k, nslots1 - 1);      // (tiles this wave does not have: clamped, unused)
          const int sw = lds_swz<64>(slot);
          xh5[k] = *(const uint4*)(sb + slot * 64 + ((h ^ sw) << 4));
          xl5[k] = *(const uint4*)(sb + slot * 64 + (((2 + h) ^ sw) << 4));
        }
        if (j < nmine) {
#pragma unroll
          for (int k = 0; k < KT; ++k) {
            acc1[j] = mma32(wh[k], xh5[k], acc1[j]);
            acc1[j] = mma32(wl[k], xh5[k], acc1[j]);
            acc1[j] = mma32(wh[k], xl5[k], acc1[j]);
          }
        }
      }
#else
      uint4 xh[MAXT1][KT], xl[MAXT1][KT];
#pragma unroll
      for (int j = 0; j < MAXT1; ++j)
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const int slot = min(TW * (wave + NW * j) + col + k, nslots1 - 1);      // (tiles this wave does not have: clamped, unused)
          const int sw = lds_swz<64>(slot);
          xh[j][k] = *(const uint4*)(sb + slot * 64 + ((h ^ sw) << 4));
          xl[j][k] = *(const uint4*)(sb + slot * 64 + (((2 + h) ^ sw) << 4));
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < MAXT1; ++j)
        if (j < nmine) {
#pragma unroll
          for (int k = 0; k < KT; ++k) {
            acc1[j] = mma32(wh[k], xh[j][k], acc1[j]);
            acc1[j] = mma32(wl[k], xh[j][k], acc1[j]);
            acc1[j] = mma32(wh[k], xl[j][k], acc1[j]);
          }
        }
#endif
      __builtin_amdgcn_sched_barrier(0);
      slab_split(s + 1);                                      // (past the last slab: a stale buffer into an image nobody reads)
      slab_park(s + 2, xr);
#if C1X_K1 == 5
      w_park(s + 1);                                          // W[(s + 1) & 1] was last read in trip s - 1, behind that trip's barrier
      w_load(s + 2);
#endif
      slab_load(s + 4, xr);                                   // (clamped: past the end it re-reads the last slab, never parked as data)
      __syncthreads();
    };
    for (int s = 0; s < nks1; s += 2) {                       // nks1 is even
      trip(s, xrA);
      trip(s + 1, xrB);
    }
  }
  if (stamp) a.stamps[8 * b + 1] = __builtin_amdgcn_s_memtime();
  // (the barrier that closed the loop: every wave is done with the slabs and the layer-1 weights)
  {
    // h1 halo: slot 0 (frame -1); frames >= T are written as zeros by the epilogue below, slot 32 NT + 1 here
    if (tid < 16) *(uint4*)(h1S + (tid < 8 ? 0 : (nslots - 1) * 128) + (tid & 7) * 16) = make_uint4(0u, 0u, 0u, 0u);
    const int nmine = (NT - wave + NW - 1) / NW;
#pragma unroll
    for (int j = 0; j < MAXT1; ++j)
      if (j < nmine) store_split<32>(acc1[j], a.b1, 0, h1S, TW * (wave + NW * j) + col, T, h);
  }
  // hi / lo weight fragments of layer 2 (this wave's 32 output channels): requested in front of the barrier
  uint4 w2h[6], w2l[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    w2h[i] = C1X_W2[((size_t)((wave & 1) * 6 + i) * 2) * 64 + lane];
    w2l[i] = C1X_W2[((size_t)((wave & 1) * 6 + i) * 2 + 1) * 64 + lane];
  }
  __syncthreads();

  // ------------------------------------------------------------------------------------------------ layer 2: 32 -> 64
  {
    const int m = wave & 1, par = wave >> 1;                 // 32 of the 64 channels; tiles par, par + 4, par + 8
    constexpr int ST = NW / 2;
    if (tid < 32) *(uint4*)(h2S + (tid < 16 ? 0 : (nslots - 1) * 256) + (tid & 15) * 16) = make_uint4(0u, 0u, 0u, 0u);
    // tile i's bias + ReLU + split + store rides on tile i + 1's steps (one 4-channel group per step)
    f32x16_t accA, accB;
    int tile = par;
    if (tile < NT) {
      split_gemm<32>(w2h, w2l, h1S, TW * tile, col, h, accA, [](int) {});
      for (tile += ST; tile + ST < NT; tile += 2 * ST) {
        split_gemm<32>(w2h, w2l, h1S, TW * tile, col, h, accB,
                       [&](int i) { if (i >= 1 && i < 5) store_split_g<64>(accA, a.b2, 32 * m, h2S, TW * (tile - ST) + col, T, h, i - 1); });
        split_gemm<32>(w2h, w2l, h1S, TW * (tile + ST), col, h, accA,
                       [&](int i) { if (i >= 1 && i < 5) store_split_g<64>(accB, a.b2, 32 * m, h2S, TW * tile + col, T, h, i - 1); });
      }
      if (tile < NT) {
        split_gemm<32>(w2h, w2l, h1S, TW * tile, col, h, accB,
                       [&](int i) { if (i >= 1 && i < 5) store_split_g<64>(accA, a.b2, 32 * m, h2S, TW * (tile - ST) + col, T, h, i - 1); });
        store_split<64>(accB, a.b2, 32 * m, h2S, TW * tile + col, T, h);
      } else {
        store_split<64>(accA, a.b2, 32 * m, h2S, TW * (tile - ST) + col, T, h);
      }
    }
  }
  // layer 3's fragments (32 of the 128 channels per wave; two waves share a channel tile and split its frame tiles)
  uint4 w3h[12], w3l[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    w3h[i] = C1X_W3[((size_t)((wave & 3) * 12 + i) * 2) * 64 + lane];
    w3l[i] = C1X_W3[((size_t)((wave & 3) * 12 + i) * 2 + 1) * 64 + lane];
  }
  __syncthreads();
  if (stamp) a.stamps[8 * b + 2] = __builtin_amdgcn_s_memtime();

  // ------------------------------------------------------------------------------------------------ layer 3: 64 -> 128, frame mean, classifier
  {
    const int m = wave & 3, par = wave >> 2;                 // tiles par, par + 2, ...
    float bias[16], sum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      bias[r] = C1X_B3[32 * m + (r & 3) + 8 * (r >> 2) + 4 * h];
      sum[r] = 0.f;
    }
    auto add_regs = [&](const f32x16_t& v, int tile, int r0) {       // two accumulator registers per step
#if C1X_RAGGED
      const bool inside = TW * tile + col >= olo && TW * tile + col < ohi;      // the frames this segment owns
#else
      const bool inside = TW * tile + col < T;
#endif
#pragma unroll
      for (int r = r0; r < r0 + 2; ++r) sum[r] += inside ? fmaxf(v[r] + bias[r], 0.f) : 0.f;
    };
    f32x16_t accA, accB;
    int tile = par;
    if (tile < NT) {
      split_gemm<64>(w3h, w3l, h2S, TW * tile, col, h, accA, [](int) {});
      for (tile += 2; tile + 2 < NT; tile += 4) {
        split_gemm<64>(w3h, w3l, h2S, TW * tile, col, h, accB, [&](int i) { if (i >= 2 && i < 10) add_regs(accA, tile - 2, 2 * (i - 2)); });
        split_gemm<64>(w3h, w3l, h2S, TW * (tile + 2), col, h, accA, [&](int i) { if (i >= 2 && i < 10) add_regs(accB, tile, 2 * (i - 2)); });
      }
      if (tile < NT) {
        split_gemm<64>(w3h, w3l, h2S, TW * tile, col, h, accB, [&](int i) { if (i >= 2 && i < 10) add_regs(accA, tile - 2, 2 * (i - 2)); });
#pragma unroll
        for (int r = 0; r < 16; r += 2) add_regs(accB, tile, r);
      } else {
#pragma unroll
        for (int r = 0; r < 16; r += 2) add_regs(accA, tile - 2, r);
      }
    }
#if !C1X_RAGGED
    float part = 0.f;
#endif
    const float inv_t = 1.0f / (float)TB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s = sum[r];
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      part = fmaf(s * inv_t, C1X_CW[32 * m + (r & 3) + 8 * (r >> 2) + 4 * h], part);
    }
#if C1X_RAGGED
    // (per lane, `part` holds the sum over the segments so far; the halves are joined into red[] without touching it)
    const float part2 = part + __shfl_xor(part, 32, 64);
    if (lane == 0) red[wave] = part2;
#else
    part += __shfl_xor(part, 32, 64);
    if (lane == 0) red[wave] = part;
#endif
  }
  __syncthreads();     // (ragged: also closes the segment -- every wave is done with h2 before the next window is staged)
  if (stamp && last_seg) { a.stamps[8 * b + 3] = __builtin_amdgcn_s_memtime(); a.stamps[8 * b + 6] = __builtin_amdgcn_s_memrealtime(); }
#if C1X_RAGGED
  if (stamp && last_seg) { a.stamps[8 * b + 4] = TB; a.stamps[8 * b + 7] = nseg; }
#endif
  if (tid == 0 && last_seg) a.logits[b] = (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]))) + a.cb[0];
#if C1X_RAGGED
  }   // segments
#endif
#if C1X_K1 != 5
#undef nslots1
#endif
#undef C1X_OFFB
#undef C1X_OFFS
#undef C1X_OFFH2
#undef C1X_SLAB
#undef C1X_W2
#undef C1X_W3
#undef C1X_B3
#undef C1X_CW

// dfa_device.h -- the device primitives every kernel file shares: vector types, bf16 conversion, loads and stores that
// widen / narrow between the storage type (float or bf16_t) and float registers, the MFMA wrappers on 16-byte operands, the
// fp32 -> bf16 term split and the transposed LDS read.  Nothing here belongs to one model or one layer; a new kernel file
// takes these from here and adds no copy of its own (source layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dfa {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

struct bf16_t {
  unsigned short v;
};

__device__ __forceinline__ float bf16_to_float(bf16_t x) { return __uint_as_float(((unsigned)x.v) << 16); }
__device__ __forceinline__ bf16_t float_to_bf16(float f) {
  __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: round-to-nearest-even, NaN preserved
  bf16_t r;
  r.v = __builtin_bit_cast(unsigned short, b);
  return r;
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  bf16x2_t v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}
template <typename T>
__device__ __forceinline__ T cvt_out(float f);
template <>
__device__ __forceinline__ float cvt_out<float>(float f) { return f; }
template <>
__device__ __forceinline__ bf16_t cvt_out<bf16_t>(float f) { return float_to_bf16(f); }

// ReLU as ONE instruction: v_med3_f32(x, 0, lim) with lim = +inf held in an SGPR the compiler cannot see through
// (relu_limit()).  fmaxf(x, 0) costs two -- the compiler canonicalises the operand first -- and so does a med3 against a
// literal +inf, which it folds back into that max.  Not inline asm either: the MFMA -> VALU hazard nops do not cover asm.
__device__ __forceinline__ float relu_limit() {
  float lim = __builtin_inff();
  asm volatile("" : "+s"(lim));
  return lim;
}
__device__ __forceinline__ float relu1(float x, float lim) { return __builtin_amdgcn_fmed3f(x, 0.f, lim); }

// ---- XCD-aware workgroup order.  Workgroups with equal blockIdx.x % 8 share an XCD (and its L2): each XCD gets a contiguous
// range of logical workgroup numbers, so that neighbouring (utterance, strip) ids, which share halo columns, meet in one L2.
__device__ __forceinline__ int xcd_logical_workgroup() {
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = bid & 7, xi = bid >> 3;
  return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + xi;
}

// ---- loads and stores between storage (float / bf16_t) and float registers
// one element
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return bf16_to_float(*p); }

// 8 consecutive elements (16 / 32 bytes, 16-byte aligned)
template <typename T>
__device__ __forceinline__ void ld8(const T* p, float* v);
template <>
__device__ __forceinline__ void ld8<float>(const float* p, float* v) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <>
__device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, float* v) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[2 * e] = __uint_as_float(u[e] << 16); v[2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u); }
}
template <typename T>
__device__ __forceinline__ void st8(T* p, const float* v);
template <>
__device__ __forceinline__ void st8<float>(float* p, const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
template <>
__device__ __forceinline__ void st8<bf16_t>(bf16_t* p, const float* v) {
  bf16_t o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = float_to_bf16(v[j]);
  *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(o);
}
template <typename T>
__device__ __forceinline__ void cp8(const T* src, T* dst);
template <>
__device__ __forceinline__ void cp8<float>(const float* src, float* dst) {
  reinterpret_cast<float4*>(dst)[0] = reinterpret_cast<const float4*>(src)[0];
  reinterpret_cast<float4*>(dst)[1] = reinterpret_cast<const float4*>(src)[1];
}
template <>
__device__ __forceinline__ void cp8<bf16_t>(const bf16_t* src, bf16_t* dst) {
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
}
// 4 consecutive elements, stored
__device__ __forceinline__ void st4(bf16_t* p, const float* v) {
  *(uint2*)p = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
}
__device__ __forceinline__ void st4(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }

// 32 consecutive elements (one 32-channel pixel)
template <typename T>
__device__ __forceinline__ void ld32(const T* p, float* v);
template <>
__device__ __forceinline__ void ld32<float>(const float* p, float* v) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 q = reinterpret_cast<const float4*>(p)[k];
    v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
  }
}
template <>
__device__ __forceinline__ void ld32<bf16_t>(const bf16_t* p, float* v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 q = reinterpret_cast<const uint4*>(p)[k];
    const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[8 * k + 2 * e] = __uint_as_float(u[e] << 16); v[8 * k + 2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u); }
  }
}

// ---- MFMA on 16-byte operands (8 bf16 per lane): c += a . b
// v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ f32x16_t mma32(const uint4& a, const uint4& b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
// v_mfma_f32_16x16x32_bf16
__device__ __forceinline__ f32x4_t mma16(const uint4& a, const uint4& b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// ---- fp32 -> bf16 term split.  t0 = bf16(v), t1 = bf16(v - t0), t2 = bf16(v - t0 - t1): every term takes the 8 leading
// significant bits of what is left and the subtractions are exact, so two terms carry 16 significant bits of v (v = t0 + t1
// to 2^-17 relative) and THREE TERMS CARRY THE 24-BIT MANTISSA: v = t0 + t1 + t2 exactly (barring bf16 underflow of the last
// term).  Products of bf16 terms are exact in the fp32 accumulator of the MFMA, so a product of two three-term operands summed
// over its term pairs of order <= 2 (six MFMAs; the dropped pairs are below 2^-24 of the product) is an fp32-grade product:
// the fp32 paths of CNN1D and of the DeepfakeDetector rest on this, and refer here.
// two floats -> the packed bf16 pairs of their three terms
__device__ __forceinline__ void split3_pair(float u0, float u1, unsigned& w0, unsigned& w1, unsigned& w2) {
  w0 = pack_bf16x2(u0, u1);
  const float r0 = u0 - __uint_as_float(w0 << 16), r1 = u1 - __uint_as_float(w0 & 0xffff0000u);
  w1 = pack_bf16x2(r0, r1);
  w2 = pack_bf16x2(r0 - __uint_as_float(w1 << 16), r1 - __uint_as_float(w1 & 0xffff0000u));
}
// 8 floats -> TERMS bf16 fragments (element j in bf16 position j): v = f[0] + f[1] (+ f[2])
template <int TERMS>
__device__ __forceinline__ void split8n(const float (&v)[8], uint4 (&f)[TERMS]) {
  unsigned q[TERMS][4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float r0 = v[2 * p], r1 = v[2 * p + 1];
#pragma unroll
    for (int t = 0; t < TERMS; ++t) {
      q[t][p] = pack_bf16x2(r0, r1);
      if (t + 1 < TERMS) { r0 -= __uint_as_float(q[t][p] << 16); r1 -= __uint_as_float(q[t][p] & 0xffff0000u); }
    }
  }
#pragma unroll
  for (int t = 0; t < TERMS; ++t) f[t] = make_uint4(q[t][0], q[t][1], q[t][2], q[t][3]);
}
// the two-term form on named fragments
__device__ __forceinline__ void split8(const float (&v)[8], uint4& hi, uint4& lo) {
  uint4 f[2];
  split8n<2>(v, f);
  hi = f[0];
  lo = f[1];
}

// ---- ds_read_b64_tr_b16, compiler-scheduled: the lane's 4 x 16-bit column of a 16-lane group's 4 x 16 block at LDS byte
// address addr (wgrad_mfma.hip has the layout)
__device__ __forceinline__ u32x2_t lds_read_tr16(unsigned addr) {
  return __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(size_t)addr));
}

}  // namespace dfa

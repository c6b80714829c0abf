// widen.h -- fp16 / bf16 / fp8 -> f32 widening of feature-map elements, shared by the translation units that read
// the resident batch in its stored type (kernels.hip: dropout and widen passes; featnorm.hip: the normalisation).
// Device code only; tests/test_gpu_feat16.py and tests/test_gpu_fp8.py pin the bits.
#ifndef RAU_WIDEN_H
#define RAU_WIDEN_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rau.h"

namespace rau {

// ---- element type of the resident feature map (rau_feat_type): f32, IEEE fp16, bf16, or OCP fp8 (e4m3fn,
// e5m2).  Widening a narrow value to f32 is exact, so every pass below does exactly the f32 arithmetic of the
// f32 form on the widened value.  fp16 is widened by integer operations: subnormal halves are normal f32 numbers
// and come out unchanged under any denorm mode (no f16 / f32 denormal ever enters a float op).
__device__ __forceinline__ float widen_f16(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  if (e == 0) {   // +-0 and subnormals: m * 2^-24, an exact product with a normal f32 result
    const float v = (float)m * 0x1p-24f;
    return __uint_as_float(__float_as_uint(v) | sign);
  }
  return __uint_as_float(sign | (e == 31 ? 0x7f800000u : (e + 112u) << 23) | (m << 13));
}
// OCP e4m3fn (bias 7, no infinities, S.1111.111 the only NaN), the same way: a subnormal is m * 2^-9, an exact
// product of two normal f32 numbers.  (The hardware converts v_cvt_pk_f32_fp8 / _bf8 are not used: this form is
// the contract, and it costs nothing beside the pass's memory time.)
__device__ __forceinline__ float widen_e4m3(uint32_t c) {
  const uint32_t sign = (c & 0x80u) << 24, e = (c >> 3) & 0xfu, m = c & 7u;
  if (e == 0) {
    const float v = (float)m * 0x1p-9f;
    return __uint_as_float(__float_as_uint(v) | sign);
  }
  if ((c & 0x7fu) == 0x7fu) return __uint_as_float(sign | 0x7fc00000u);
  return __uint_as_float(sign | ((e + 120u) << 23) | (m << 20));
}
// one element's bit pattern (16 or 8 bits, in the low end of h) -> f32.  e5m2 is the upper byte of a binary16.
template <int FT>
__device__ __forceinline__ float widen1(uint32_t h) {
  if (FT == RAU_FEAT_F16) return widen_f16(h);
  if (FT == RAU_FEAT_E4M3) return widen_e4m3(h);
  if (FT == RAU_FEAT_E5M2) return widen_f16(h << 8);
  return __uint_as_float(h << 16);
}
// element i of X (f32, or 16-bit / 8-bit bit patterns)
template <int FT>
__device__ __forceinline__ float load_feat(const void* __restrict__ X, size_t i) {
  if (FT == RAU_FEAT_F32) return reinterpret_cast<const float*>(X)[i];
  if (FT == RAU_FEAT_E4M3 || FT == RAU_FEAT_E5M2) return widen1<FT>(reinterpret_cast<const uint8_t*>(X)[i]);
  return widen1<FT>(reinterpret_cast<const uint16_t*>(X)[i]);
}
// quad q of X (elements 4q .. 4q+3): one 16-byte load for f32, one 8-byte load for 16-bit data, one 4-byte
// load for fp8 (rows are at pitch Sp % 4 == 0 and buffers are 256-byte aligned, so each is aligned to its size)
template <int FT>
__device__ __forceinline__ float4 load_feat4(const void* __restrict__ X, size_t q) {
  if (FT == RAU_FEAT_F32) return reinterpret_cast<const float4*>(X)[q];
  if (FT == RAU_FEAT_E4M3 || FT == RAU_FEAT_E5M2) {
    const uint32_t v = reinterpret_cast<const uint32_t*>(X)[q];
    return make_float4(widen1<FT>(v & 0xffu), widen1<FT>((v >> 8) & 0xffu), widen1<FT>((v >> 16) & 0xffu),
                       widen1<FT>(v >> 24));
  }
  const uint2 v = reinterpret_cast<const uint2*>(X)[q];
  return make_float4(widen1<FT>(v.x & 0xffffu), widen1<FT>(v.x >> 16), widen1<FT>(v.y & 0xffffu),
                     widen1<FT>(v.y >> 16));
}

}  // namespace rau

#endif  // RAU_WIDEN_H

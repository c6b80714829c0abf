// narrow.h -- f32 -> fp16 / bf16 / fp8 narrowing in integer arithmetic, shared by the translation units that
// narrow feature maps on their way into a bank (bank.hip: dense maps, packed.hip: packed region rows).  Device
// code only; tests/test_gpu_bank.py and tests/test_gpu_fp8.py pin the bits.
#ifndef RAU_NARROW_H
#define RAU_NARROW_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/rau.h"

namespace rau {

// f32 -> fp16 / bf16, round to nearest even, in integer arithmetic (independent of the wave's denormal and
// rounding modes): the bits numpy's float16 conversion gives -- subnormals kept, overflow to infinity, NaN stays
// NaN -- and feat16.bf16_bits' for bf16.
__device__ __forceinline__ uint32_t narrow_f16_bits(uint32_t x) {
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7e00u | ((a >> 13) & 0x1ffu);   // NaN (quiet)
  if (a >= 0x477ff000u) return sign | 0x7c00u;                          // >= 65520: infinity
  if (a >= 0x38800000u) {                                               // normal fp16: rebias 127 -> 15
    const uint32_t r = a - 0x38000000u, rem = r & 0x1fffu;
    uint32_t h = r >> 13;
    h += (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ? 1u : 0u;     // a carry runs into the exponent
    return sign | h;
  }
  const uint32_t e = a >> 23;
  if (e < 102u) return sign;                                            // below 2^-25: +-0
  const uint32_t m = (a & 0x7fffffu) | 0x800000u, sh = 126u - e;        // subnormal: units of 2^-24, sh in 14..24
  const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
  uint32_t h = m >> sh;
  h += (rem > half || (rem == half && (h & 1u))) ? 1u : 0u;             // may round up to the smallest normal
  return sign | h;
}
__device__ __forceinline__ uint32_t narrow_bf16_bits(uint32_t x) {
  return (x + (((x >> 16) & 1u) + 0x7fffu)) >> 16;
}
// f32 -> OCP fp8, round to nearest even and SATURATING, in integer arithmetic: MB mantissa bits, exponent bias
// BIAS, MAXC the code of the largest finite value (e4m3fn: 3, 7, 0x7e = 448; e5m2: 2, 15, 0x7b = 57344).  Every
// result beyond the largest finite value, +-inf included, is that value with the input's sign; NaN is the code
// S.1111111 (a NaN in both formats); magnitudes at or below half the smallest subnormal are +-0.  The bits of
// feat16.fp8_bits.
template <int MB, int BIAS, uint32_t MAXC>
__device__ __forceinline__ uint32_t narrow_fp8_bits(uint32_t x) {
  const uint32_t sign = (x >> 24) & 0x80u, a = x & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7fu;
  const uint32_t e = a >> 23;
  uint32_t h;
  if (e >= 128u - BIAS) {                                   // normal in the target: rebias 127 -> BIAS
    const uint32_t r = a - ((127u - BIAS) << 23), sh = 23 - MB;
    const uint32_t rem = r & ((1u << sh) - 1u), half = 1u << (sh - 1);
    h = r >> sh;
    h += (rem > half || (rem == half && (h & 1u))) ? 1u : 0u;   // a carry runs into the exponent
    h = min(h, MAXC);
  } else {                                                  // subnormal: units of 2^(1 - BIAS - MB)
    const uint32_t sh = (151u - BIAS - MB) - e;             // >= 24 - MB
    if (sh > 24u) return sign;                              // below half a unit (f32 subnormals and 0 too)
    const uint32_t m = (a & 0x7fffffu) | 0x800000u;
    const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    h = m >> sh;
    h += (rem > half || (rem == half && (h & 1u))) ? 1u : 0u;   // may round up to the smallest normal
  }
  return sign | h;
}
template <int FT>
__device__ __forceinline__ uint32_t narrow1(uint32_t x) {
  if (FT == RAU_FEAT_F16) return narrow_f16_bits(x) & 0xffffu;
  if (FT == RAU_FEAT_E4M3) return narrow_fp8_bits<3, 7, 0x7eu>(x);
  if (FT == RAU_FEAT_E5M2) return narrow_fp8_bits<2, 15, 0x7bu>(x);
  return narrow_bf16_bits(x) & 0xffffu;
}

}  // namespace rau

#endif  // RAU_NARROW_H

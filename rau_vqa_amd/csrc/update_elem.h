// update_elem.h -- the element arithmetic of the parameter update, stated once with its roundings.
//
// rau_noise_clip_adam (kernels.hip: one launch per group and phase) and rau_update (update.hip: all
// groups per launch, 16-byte accesses) must give the same bits on the same state.  What decides the
// bits is which products are fused into the following addition, so every statement below says so
// itself instead of leaving it to the compiler's contraction pass:
//   noise   v = fma(nstd, z, g), acc = fma(v, v, acc)            (fused)
//   Adam    m = (m b1) + ((1-b1) g), v = (v b2) + (((1-b2) g) g)  (every product and sum rounded)
//   decay   x = x f                                               (rau_update_ex; skipped when f == 1)
//   average e = (d e) + ((1-d) x)                                 (rau_update_ex; every product and the sum rounded)
// The first two are the roundings the kernels had before this file existed.
#pragma once
#include "common.h"
#include "philox.h"

namespace rau {

__device__ __forceinline__ float2 box_muller(uint32_t a, uint32_t b) {
#pragma clang fp contract(off)
  const float u1 = ((a >> 8) + 1) * (1.0f / 16777216.0f);  // (0,1]
  const float u2 = (b >> 8) * (1.0f / 16777216.0f);
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
  sincosf(6.28318530717958647692f * u2, &s, &c);
  return make_float2(r * c, r * s);
}
// The four normals of elements 4q .. 4q+3 of parameter group `stream`: Philox counter (q, stream, 0xA5A5),
// key `seed`, two Box-Muller pairs per 128-bit block.  nstd == 0: zeros, no draw.
__device__ __forceinline__ void noise_quad(size_t q, uint32_t stream, uint64_t seed, float nstd, float z[4]) {
  z[0] = z[1] = z[2] = z[3] = 0.f;
  if (nstd > 0.f) {
    const Philox4 o = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), stream, 0xA5A5u,
                                    (uint32_t)seed, (uint32_t)(seed >> 32));
    const float2 n0 = box_muller(o.v[0], o.v[1]), n1 = box_muller(o.v[2], o.v[3]);
    z[0] = n0.x; z[1] = n0.y; z[2] = n1.x; z[3] = n1.y;
  }
}
// g + z nstd, and its square added to the thread's partial
__device__ __forceinline__ float noise_elem(float g, float z, float nstd, float& acc) {
  const float v = __builtin_fmaf(nstd, z, g);
  acc = __builtin_fmaf(v, v, acc);
  return v;
}
// the project's clip: norm > clip ? clip / norm : 1 (not torch's clip / (norm + 1e-6))
__device__ __forceinline__ float clip_scale(float norm, float clip) {
  return norm > clip ? clip / norm : 1.f;
}
// Adam on the clipped gradient gi, epsilon outside the sqrt (utils/optim_updates.lua:59-87)
__device__ __forceinline__ void adam_elem(float gi, float& m, float& v, float& x, float stepsize,
                                          float beta1, float beta2, float eps) {
#pragma clang fp contract(off)
  const float mi = m * beta1 + (1.f - beta1) * gi;
  const float vi = v * beta2 + (1.f - beta2) * gi * gi;
  m = mi;
  v = vi;
  x = x - stepsize * mi / (sqrtf(vi) + eps);
}
// Adamax (torch.optim.Adamax's statement): u is the exponentially weighted infinity norm, kept where Adam
// keeps v; u >= eps after the first step, so a zero gradient gives a finite step of 0
__device__ __forceinline__ void adamax_elem(float gi, float& m, float& u, float& x, float stepsize,
                                            float beta1, float beta2, float eps) {
#pragma clang fp contract(off)
  const float mi = m * beta1 + (1.f - beta1) * gi;
  const float ui = fmaxf(u * beta2, fabsf(gi) + eps);
  m = mi;
  u = ui;
  x = x - stepsize * mi / ui;
}
// Decoupled weight decay (rau_update_ex), BEFORE the rule's step as in torch.optim.AdamW: x = x f, one rounded
// product; f = (float)(1 - group_lr lr_scale weight_decay decay) comes from the host's double.  f == 1: x keeps
// its bits without a multiplication
__device__ __forceinline__ void decay_elem(float& x, float f) {
  if (f != 1.f) x = x * f;
}
// The weight average (rau_update_ex), AFTER the rule's step, on the new x: e = (d e) + ((1-d) x), both products and
// the sum rounded; omd = 1 - d is formed once on the host in float
__device__ __forceinline__ void ema_elem(float& e, float x, float d, float omd) {
#pragma clang fp contract(off)
  e = d * e + omd * x;
}

}  // namespace rau

// att_bias.hip -- the caller's additive attention bias (rau_set_att_bias_dev, rau_att_bias_grad_dev): its way into the
// buffer the three forward attention kernels read (AttPartials::zadd), and its gradient's way out.
//   att_bias_attach   dst[r][s] = widen(src[r][s]), s < SL: the caller's dense rows [rows][SL] (f32 copied, fp16 / bf16
//                     widened exactly, widen.h) re-pitched to the attention's row pitch; the pad columns [SL, pitch)
//                     are written +0.  -inf passes through as it is (16-bit infinities widen to f32 infinities).
//   att_bias_grad     out[r][s] = ((dz_0 + dz_1) + ..) + dz_{hops-1} at [r][s], the softmax backward's dz of the hops
//                     the backward ran, ascending, each addition rounded once; +0 with hops = 0 and in the pad columns.
// One launch each; a thread owns one quad of a row: a 16-byte store, and 16-byte loads wherever the source rows are
// quad-aligned (always for dz, whose rows have the pitch; for the caller's rows when SL % 4 == 0 -- else element
// loads).  64-bit element offsets.  One writer per element and a fixed expression: no atomics, no LDS, no private
// memory, repeated calls give the same bits.  pitch % 4 == 0 and every base but `src` on a 16-byte boundary; src as
// its type's quad needs it (the entry point asks 16 bytes of the caller).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "widen.h"

namespace rau {
namespace {

template <int FT>
__global__ __launch_bounds__(256) void k_att_bias_attach(size_t quads, int SL, int P4, const void* __restrict__ src,
    float4* __restrict__ dst) {
  RAU_CHAIN_PRIO();
  const size_t step = (size_t)gridDim.x * blockDim.x;
  const bool row_quads = (SL & 3) == 0;   // every source row starts on a quad of its type
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < quads; i += step) {
    const size_t r = i / (size_t)P4;
    const int s = (int)(i - r * (size_t)P4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_quads) {
      if (s < SL) v = load_feat4<FT>(src, (r * (size_t)SL + s) >> 2);
    } else {
      const size_t e = r * (size_t)SL + s;
      if (s + 0 < SL) v.x = load_feat<FT>(src, e + 0);
      if (s + 1 < SL) v.y = load_feat<FT>(src, e + 1);
      if (s + 2 < SL) v.z = load_feat<FT>(src, e + 2);
      if (s + 3 < SL) v.w = load_feat<FT>(src, e + 3);
    }
    dst[i] = v;
  }
}

// dz: hop h's quad i at dz[h * hop_quads + i]
__global__ __launch_bounds__(256) void k_att_bias_grad(size_t quads, int hops, int SL, int P4, size_t hop_quads,
    const float4* __restrict__ dz, float4* __restrict__ out) {
  RAU_CHAIN_PRIO();
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < quads; i += step) {
    const int s = (int)(i % (size_t)P4) * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (hops > 0 && s < SL) a = dz[i];
    for (int h = 1; h < hops && s < SL; ++h) {
      const float4 p = dz[(size_t)h * hop_quads + i];
      a.x = __fadd_rn(a.x, p.x);
      a.y = __fadd_rn(a.y, p.y);
      a.z = __fadd_rn(a.z, p.z);
      a.w = __fadd_rn(a.w, p.w);
    }
    // the quad that straddles SL: its pad columns are +0 whatever dz holds there
    if (s + 1 >= SL) a.y = 0.f;
    if (s + 2 >= SL) a.z = 0.f;
    if (s + 3 >= SL) a.w = 0.f;
    out[i] = a;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
dim3 grid_for(size_t quads) { return dim3((unsigned)std::min<size_t>(std::max<size_t>((quads + 255) / 256, 1), 256 * 8)); }

}  // namespace

hipError_t att_bias_attach(hipStream_t st, int rows, int SL, int pitch, const void* src, int type, float* dst) {
  if (rows <= 0) return hipSuccess;
  if (SL < 1 || pitch < SL || (pitch & 3) || !src || !dst || !aligned16(src) || !aligned16(dst))
    return hipErrorInvalidValue;
  const int P4 = pitch / 4;
  const size_t quads = (size_t)rows * P4;
  float4* d4 = reinterpret_cast<float4*>(dst);
  if (type == RAU_FEAT_F32)
    hipLaunchKernelGGL(k_att_bias_attach<RAU_FEAT_F32>, grid_for(quads), dim3(256), 0, st, quads, SL, P4, src, d4);
  else if (type == RAU_FEAT_F16)
    hipLaunchKernelGGL(k_att_bias_attach<RAU_FEAT_F16>, grid_for(quads), dim3(256), 0, st, quads, SL, P4, src, d4);
  else if (type == RAU_FEAT_BF16)
    hipLaunchKernelGGL(k_att_bias_attach<RAU_FEAT_BF16>, grid_for(quads), dim3(256), 0, st, quads, SL, P4, src, d4);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t att_bias_grad(hipStream_t st, int hops, int rows, int SL, int pitch, const float* dz, size_t hop_stride,
                         float* out) {
  if (rows <= 0) return hipSuccess;
  if (hops < 0 || SL < 1 || pitch < SL || (pitch & 3) || (hop_stride & 3) || (hops > 0 && !dz) || !out ||
      !aligned16(dz) || !aligned16(out) || (hops > 1 && hop_stride < (size_t)rows * pitch))
    return hipErrorInvalidValue;
  const int P4 = pitch / 4;
  const size_t quads = (size_t)rows * P4;
  hipLaunchKernelGGL(k_att_bias_grad, grid_for(quads), dim3(256), 0, st, quads, hops, SL, P4, hop_stride / 4,
                     reinterpret_cast<const float4*>(dz), reinterpret_cast<float4*>(out));
  return hipGetLastError();
}

}  // namespace rau

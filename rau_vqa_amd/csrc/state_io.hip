// state_io.hip -- the two ends of the hop recurrence that the caller may hold (rau_set_state_dev,
// rau_state_grad_dev): the initial state (c0, h0) on its way in, the gradient at it on its way out.
//   state_attach        cc[0][b][r] = widen(c0[b][r]), hh[0][b][r] = widen(h0[b][r]): the two slot-0 row blocks the
//                       hop chain reads as prev_c / prev_h of hop 0.  f32 is copied, fp16 / bf16 widened exactly
//                       (widen.h: integer operations, no denormal enters a float op).  Its detaching form (both
//                       sources null) writes zero bits: the initial state of a context without one.
//   state_grad_finish   d_h0[b][r] = ((p_0 + p_1) + ..) + p_{ns-1}, hop 0's K-split dh_prev partials [ns][n][R] in
//                       ascending split order -- the order lstm_bwd sums the partials of every other hop in -- each
//                       addition rounded once; exact +0 with ns = 0.  d_c0[b][r] = dc_prev[b][r] of hop 0's cell.
// One launch each (blockIdx.y selects the c or the h half), 16 bytes per global access, 64-bit element offsets.
// Every element has one writer and a fixed expression: no atomics, no LDS, no private memory, repeated calls give
// the same bits.  n R % 4 == 0 (rau_create: R % 4 == 0) and every base is 16-byte aligned: the partials start in a
// quarter share of the chain workspace, whose size plan_batch keeps a multiple of 16 floats, behind a whole number of
// [n][M] blocks (M % 4 == 0); a span that is not is refused, nothing launched.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "widen.h"

namespace rau {
namespace {

// 16-bit sources: elements 8o .. 8o+7 of one 16-byte load
template <int FT>
__device__ __forceinline__ void widen8(const uint4 v, float4& lo, float4& hi) {
  lo = make_float4(widen1<FT>(v.x & 0xffffu), widen1<FT>(v.x >> 16), widen1<FT>(v.y & 0xffffu), widen1<FT>(v.y >> 16));
  hi = make_float4(widen1<FT>(v.z & 0xffffu), widen1<FT>(v.z >> 16), widen1<FT>(v.w & 0xffffu), widen1<FT>(v.w >> 16));
}

// n4 quads per half.  FT: RAU_FEAT_F32, RAU_FEAT_F16, RAU_FEAT_BF16, or -1 = the detaching form.
template <int FT>
__global__ __launch_bounds__(256) void k_state_attach(size_t n4, const void* __restrict__ c0,
    const void* __restrict__ h0, float4* __restrict__ cc, float4* __restrict__ hh) {
  RAU_CHAIN_PRIO();
  const void* src = blockIdx.y ? h0 : c0;
  float4* dst = blockIdx.y ? hh : cc;
  const size_t t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  if (FT < 0) {
    for (size_t i = t0; i < n4; i += step) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else if (FT == RAU_FEAT_F32) {
    for (size_t i = t0; i < n4; i += step) dst[i] = reinterpret_cast<const float4*>(src)[i];
  } else {
    const size_t n8 = n4 >> 1;
    for (size_t o = t0; o < n8; o += step) {
      float4 lo, hi;
      widen8<FT>(reinterpret_cast<const uint4*>(src)[o], lo, hi);
      dst[2 * o] = lo;
      dst[2 * o + 1] = hi;
    }
    if ((n4 & 1) && t0 == 0) dst[n4 - 1] = load_feat4<FT>(src, n4 - 1);   // the odd last quad: one 8-byte load
  }
}

// part: [ns][n4] quads; blockIdx.y = 0: d_c0 = dc_prev, 1: d_h0 = the partials' sum
__global__ __launch_bounds__(256) void k_state_grad_finish(size_t n4, int ns, const float4* __restrict__ part,
    const float4* __restrict__ dc_prev, float4* __restrict__ d_c0, float4* __restrict__ d_h0) {
  RAU_CHAIN_PRIO();
  const size_t t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  if (blockIdx.y == 0) {
    for (size_t i = t0; i < n4; i += step) d_c0[i] = dc_prev[i];
    return;
  }
  for (size_t i = t0; i < n4; i += step) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ns > 0) a = part[i];
    for (int s = 1; s < ns; ++s) {
      const float4 p = part[(size_t)s * n4 + i];
      a.x = __fadd_rn(a.x, p.x);
      a.y = __fadd_rn(a.y, p.y);
      a.z = __fadd_rn(a.z, p.z);
      a.w = __fadd_rn(a.w, p.w);
    }
    d_h0[i] = a;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
dim3 grid_for(size_t n4) { return dim3((unsigned)std::min<size_t>(std::max<size_t>((n4 + 255) / 256, 1), 256 * 8), 2); }

}  // namespace

hipError_t state_attach(hipStream_t st, size_t n_elems, const void* c0, const void* h0, int type, float* cc,
                        float* hh) {
  if (n_elems == 0) return hipSuccess;
  if ((n_elems & 3) || !cc || !hh || !aligned16(cc) || !aligned16(hh) || !aligned16(c0) || !aligned16(h0) ||
      (c0 == nullptr) != (h0 == nullptr))
    return hipErrorInvalidValue;
  const size_t n4 = n_elems / 4;
  float4 *c4 = reinterpret_cast<float4*>(cc), *h4 = reinterpret_cast<float4*>(hh);
  const dim3 block(256);
  if (!c0)
    hipLaunchKernelGGL(k_state_attach<-1>, grid_for(n4), block, 0, st, n4, c0, h0, c4, h4);
  else if (type == RAU_FEAT_F32)
    hipLaunchKernelGGL(k_state_attach<RAU_FEAT_F32>, grid_for(n4), block, 0, st, n4, c0, h0, c4, h4);
  else if (type == RAU_FEAT_F16)
    hipLaunchKernelGGL(k_state_attach<RAU_FEAT_F16>, grid_for((n4 + 1) / 2), block, 0, st, n4, c0, h0, c4, h4);
  else if (type == RAU_FEAT_BF16)
    hipLaunchKernelGGL(k_state_attach<RAU_FEAT_BF16>, grid_for((n4 + 1) / 2), block, 0, st, n4, c0, h0, c4, h4);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t state_grad_finish(hipStream_t st, size_t n_elems, const float* part, int ns, const float* dc_prev,
                             float* d_c0, float* d_h0) {
  if (n_elems == 0) return hipSuccess;
  if (!split_span_ok(part, ns, n_elems)) return kSplitStateError;
  if ((n_elems & 3) || ns < 0 || (ns > 0 && !part) || !dc_prev || !d_c0 || !d_h0 || !aligned16(part) ||
      !aligned16(dc_prev) || !aligned16(d_c0) || !aligned16(d_h0))
    return hipErrorInvalidValue;
  const size_t n4 = n_elems / 4;
  const float4* dc4 = reinterpret_cast<const float4*>(dc_prev);
  float4 *oc = reinterpret_cast<float4*>(d_c0), *oh = reinterpret_cast<float4*>(d_h0);
  hipLaunchKernelGGL(k_state_grad_finish, grid_for(n4), dim3(256), 0, st, n4, ns,
                     reinterpret_cast<const float4*>(part), dc4, oc, oh);
  return hipGetLastError();
}

}  // namespace rau

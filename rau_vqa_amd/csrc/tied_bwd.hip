// tied_bwd.hip -- the hop reduction of the tied feature-map dropout backward (rau_set_feat_dropout,
// RAU_XDROP_TIED).  With one dropout mask for all hops, I = tanh(Wi X' + bi) and P = Wp I + bp do not depend on the
// hop, and the three 1x1-conv gradients
//   dZ_h = Wp^T dS_h + dj_h (x) a_h,   dWp += dS_h I^T,   dWi += (dZ_h (.) (1 - I^2)) X'^T
// are linear in what hop h hands back (dS_h, dj_h (x) a_h).  The step-level backward therefore sums over the
// active hops first and runs each conv gradient once:
//   hop_sum    dS_sum[b,k,s] = sum_{h < HA} dS_h[b,k,s]                     -> conv_att_dgrad, conv_att_wgrad
//   outer_sum  dZ[b,m,s]    += sum_{1 <= h < HA} dj_h[b,m] a_h[b,s]         behind conv_att_dgrad, which added hop 0's
// Both are bandwidth kernels (HA + 1 and 2 passes over a [B][.][Sp] tensor): one 16-byte quad per lane and
// iteration, rows at the position pitch Sp (% 4 == 0, so every quad is aligned and inside one row), the hops added
// in ascending order in f32 by the one lane that owns the quad.  No atomics, no cross-lane sums: every call gives
// the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "kernels.h"

namespace rau {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 8;   // a few workgroups per CU; the loops stride over the rest

inline int quad_grid(size_t nquad) {
  size_t g = (nquad + kBlock - 1) / kBlock;
  return (int)std::min<size_t>(std::max<size_t>(g, 1), kMaxBlocks);
}

// out[r][s] = sum_h T[h][r][s] for s < SL, 0 for SL <= s < Sp; r < rows, hop stride = rows * Sp floats.
// Sq = Sp / 4 quads per row.
__global__ __launch_bounds__(kBlock) void k_hop_sum(int HA, size_t rows, int Sq, int SL,
                                                    const float4* __restrict__ T, float4* __restrict__ out) {
  const size_t nquad = rows * (size_t)Sq;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nquad; q += (size_t)gridDim.x * blockDim.x) {
    float4 acc = T[q];
#pragma unroll 4
    for (int h = 1; h < HA; ++h) {
      const float4 v = T[(size_t)h * nquad + q];
      acc.x = __fadd_rn(acc.x, v.x);
      acc.y = __fadd_rn(acc.y, v.y);
      acc.z = __fadd_rn(acc.z, v.z);
      acc.w = __fadd_rn(acc.w, v.w);
    }
    const int s = (int)(q % (size_t)Sq) * 4;   // pad columns of a pitched map stay zero whatever T holds there
    if (s + 3 >= SL) {
      if (s >= SL) acc.x = 0.f;
      if (s + 1 >= SL) acc.y = 0.f;
      if (s + 2 >= SL) acc.z = 0.f;
      acc.w = 0.f;
    }
    out[q] = acc;
  }
}

// dZ[b][m][s] = fmaf(dj[h][b][m], a[h][b][s], dZ[b][m][s]) for h = 1 .. HA-1 in that order.  dj hop stride B * M,
// a hop stride B * Sp; a's pad columns hold zeros, so dZ's stay what they were.
__global__ __launch_bounds__(kBlock) void k_outer_sum(int HA, int B, int M, int Sq, const float* __restrict__ dj,
                                                      const float4* __restrict__ a, float4* __restrict__ dZ) {
  const size_t rows = (size_t)B * M, nquad = rows * (size_t)Sq, a_hop = (size_t)B * Sq;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nquad; q += (size_t)gridDim.x * blockDim.x) {
    const size_t row = q / (size_t)Sq;
    const int sq = (int)(q - row * (size_t)Sq);
    const size_t b = row / (size_t)M;
    float4 z = dZ[q];
#pragma unroll 4
    for (int h = 1; h < HA; ++h) {
      const float d = dj[(size_t)h * rows + row];
      const float4 av = a[(size_t)h * a_hop + b * (size_t)Sq + sq];
      z.x = __fmaf_rn(d, av.x, z.x);
      z.y = __fmaf_rn(d, av.y, z.y);
      z.z = __fmaf_rn(d, av.z, z.z);
      z.w = __fmaf_rn(d, av.w, z.w);
    }
    dZ[q] = z;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t hop_sum(hipStream_t st, int HA, int B, int A, int SL, int Sp, const float* T, float* out) {
  if (HA < 1 || B < 1 || A < 1 || Sp < 4 || Sp % 4 != 0 || SL < 1 || SL > Sp || !aligned16(T) || !aligned16(out))
    return hipErrorInvalidValue;
  const size_t rows = (size_t)B * A;
  hipLaunchKernelGGL(k_hop_sum, dim3(quad_grid(rows * (Sp / 4))), dim3(kBlock), 0, st, HA, rows, Sp / 4, SL,
                     reinterpret_cast<const float4*>(T), reinterpret_cast<float4*>(out));
  return hipGetLastError();
}

hipError_t outer_sum(hipStream_t st, int HA, int B, int M, int Sp, const float* dj, const float* a, float* dZ) {
  if (HA < 2 || B < 1 || M < 1 || Sp < 4 || Sp % 4 != 0 || !aligned16(a) || !aligned16(dZ))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_outer_sum, dim3(quad_grid((size_t)B * M * (Sp / 4))), dim3(kBlock), 0, st, HA, B, M, Sp / 4,
                     dj, reinterpret_cast<const float4*>(a), reinterpret_cast<float4*>(dZ));
  return hipGetLastError();
}

}  // namespace rau

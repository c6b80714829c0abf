// bank.hip -- the two kernels of the device-resident feature bank (rau_bank_*, include/rau.h): the gather
// of whole maps out of the bank into the batch buffers, and the f32 -> fp16 / bf16 / fp8 narrowing of rau_bank_put.
// Both are byte movers bound by HBM; they live in a translation unit of their own so that the code object of
// kernels.hip is the same with and without them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "narrow.h"

namespace rau {

static inline int grid_for(size_t n, int block = 256, int cap = 256 * 8) {
  size_t g = (n + block - 1) / block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// Feature bank -> batch buffers: out[i] = bank[rows[i]] for i < n, whole maps as above.  The bank may be far
// larger than 4 GiB: the map's offset is formed in 64 bits from the wave-uniform row number, everything inside
// a map is addressed relative to it.  rows is a DEVICE index the host has checked against the bank's capacity;
// `capacity` bounds it once more here so that a stale index can never address outside the allocation.
template <typename V>
__global__ __launch_bounds__(256) void k_bank_gather(size_t nvec, const V* __restrict__ bank, int32_t capacity,
                                                     const int32_t* __restrict__ rows, V* __restrict__ out) {
  const int i = blockIdx.y;
  int r = __builtin_amdgcn_readfirstlane(rows[i]);
  r = min(max(r, 0), capacity - 1);
  const V* src = bank + (size_t)r * nvec;
  V* dst = out + (size_t)i * nvec;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  // four independent 16-byte loads in flight per lane before the first store
  for (; v + 3 * step < nvec; v += 4 * step) {
    const V a = *(src + v), b = *(src + v + step),
            c = *(src + v + 2 * step), d = *(src + v + 3 * step);
    dst[v] = a; dst[v + step] = b; dst[v + 2 * step] = c; dst[v + 3 * step] = d;
  }
  for (; v < nvec; v += step) dst[v] = *(src + v);
}
// (map_bytes % 8: D % 4 == 0 and Sp % 4 == 0 make every map, fp8 included, a multiple of 16 bytes -- see
// expand_features)
hipError_t bank_gather(hipStream_t st, int n, size_t map_bytes, const void* bank, int32_t capacity,
                       const int32_t* rows, void* out) {
  if (n <= 0 || n > 65535 || capacity <= 0 || !bank || !rows || !out || map_bytes % 8 != 0)
    return hipErrorInvalidValue;
  const bool v16 = map_bytes % 16 == 0;
  const size_t nvec = map_bytes / (v16 ? 16 : 8);
  const int slices = (int)std::min<size_t>(16, (nvec + 1023) / 1024);
  const dim3 grid(std::max(slices, 1), n);
  if (v16)
    hipLaunchKernelGGL(k_bank_gather<uint4>, grid, dim3(256), 0, st, nvec, static_cast<const uint4*>(bank),
                       capacity, rows, static_cast<uint4*>(out));
  else
    hipLaunchKernelGGL(k_bank_gather<uint2>, grid, dim3(256), 0, st, nvec, static_cast<const uint2*>(bank),
                       capacity, rows, static_cast<uint2*>(out));
  return hipGetLastError();
}

// dense f32 rows [rows][SL] -> 16-bit or fp8 rows at pitch Sp (a multiple of 4), pad columns zero; one thread
// forms four neighbouring outputs and stores them as 8 bytes (fp8: as one 32-bit word)
template <int FT>
__global__ __launch_bounds__(256) void k_narrow_features(size_t nquad, int SL, int Sp,
                                                         const float* __restrict__ src, void* __restrict__ out) {
  const int qpr = Sp / 4;   // quads per row
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nquad; q += (size_t)gridDim.x * blockDim.x) {
    const size_t r = q / qpr;
    const int s0 = (int)(q - r * qpr) * 4;
    const float* p = src + r * SL + s0;
    uint32_t h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = s0 + k < SL ? __float_as_uint(p[k]) : 0u;
      h[k] = narrow1<FT>(x);
    }
    if (FT == RAU_FEAT_E4M3 || FT == RAU_FEAT_E5M2)
      static_cast<uint32_t*>(out)[q] = h[0] | (h[1] << 8) | (h[2] << 16) | (h[3] << 24);
    else
      static_cast<uint2*>(out)[q] = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
  }
}
hipError_t narrow_features(hipStream_t st, size_t rows, int SL, int Sp, const float* src, void* out, int ft) {
  if (!feat_type_ok(ft) || ft == RAU_FEAT_F32 || Sp % 4 != 0 || SL > Sp || SL <= 0 || !src || !out)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  const size_t nquad = rows * (Sp / 4);
  const dim3 grid(grid_for(nquad));
  switch (ft) {
    case RAU_FEAT_F16:
      hipLaunchKernelGGL(k_narrow_features<RAU_FEAT_F16>, grid, dim3(256), 0, st, nquad, SL, Sp, src, out);
      break;
    case RAU_FEAT_BF16:
      hipLaunchKernelGGL(k_narrow_features<RAU_FEAT_BF16>, grid, dim3(256), 0, st, nquad, SL, Sp, src, out);
      break;
    case RAU_FEAT_E4M3:
      hipLaunchKernelGGL(k_narrow_features<RAU_FEAT_E4M3>, grid, dim3(256), 0, st, nquad, SL, Sp, src, out);
      break;
    default:
      hipLaunchKernelGGL(k_narrow_features<RAU_FEAT_E5M2>, grid, dim3(256), 0, st, nquad, SL, Sp, src, out);
      break;
  }
  return hipGetLastError();
}

}  // namespace rau

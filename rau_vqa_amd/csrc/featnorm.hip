// featnorm.hip -- per-position L2 normalisation of feature maps (rau_set_feat_norm) and its gradient:
//
//   nrm[s]   = sqrt(sum_d x[d,s]^2)                 x widened exactly to f32 first (widen.h)
//   xn[d,s]  = x[d,s] * (1 / max(nrm[s], eps))      torch.nn.functional.normalize(x, p=2, dim=channel, eps)
//
//   c[s]     = sum_d G[d,s] xn[d,s],   r[s] = 1 / max(nrm[s], eps)
//   dX[d,s]  = r[s] (G[d,s] - xn[d,s] c[s])         where nrm[s] >= eps
//   dX[d,s]  = r[s] G[d,s]  (= G / eps)             where nrm[s] <  eps: the forward is linear there
//
// Outside the contract: non-finite inputs, and inputs whose sum of squares overflows f32.
//
// Layout.  A map is [D][Sp] with the positions contiguous, so the lanes of a workgroup run along positions and the
// reduction over D strides by Sp.  A workgroup of 256 threads owns `QT` neighbouring columns of one map -- a column
// is a quad of four positions (V = 4: pitch % 4 == 0, every access to f32 data 16 bytes wide; 16-bit maps are read 8
// bytes and fp8 maps 4 bytes per quad, load_feat4's forms) or a single position (V = 1: the dense [D][S] tensors of
// the rau_dev_* helpers where S % 4 != 0) -- and all D channels of them: thread t is column t % QT, channel lane
// t / QT of C = 256 / QT lanes.  The columns of a map are split evenly over ceil(ncol / 32) workgroups (V = 1: 64).
//
// Order of the sum, a function of (D, S, pitch) alone: channel lane k adds the squares of channels k, k + C,
// k + 2C, .. in ascending order, each square and each sum rounded once (__fmul_rn, __fadd_rn: nothing contracts into
// an fma); the C partial sums meet in LDS and are added in ascending k by the lane-0 thread of the column.  No
// atomics, nothing depends on the map's index, the number of maps, the stored type or how the launch was made: the
// same map gives the same bits as a sample's map, a row of an image table or a bank row, eagerly or in a replay.
//
// The scaling pass reads the workgroup's tile a second time, out of whichever cache still holds it.  The tile is
// D x QT columns x 16 bytes in f32: 205 KB at D = 512 and 819 KB at D = 2048 with the 25 quads of a 14 x 14 map.
// Keeping it in LDS instead would cap the tile at 160 KB, i.e. 5 quads at D = 2048: rows of 80 bytes per wave
// instruction and one workgroup per CU.  The measured rates of this form are in LOG.md.  No private-memory array,
// no scratch in device memory.
//
// In-place use (rau_dev_l2norm with y == x, l2norm_backward always): a thread reads the elements it later writes,
// and workgroups own disjoint tiles; X and xn carry no __restrict__.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "widen.h"

// Every product and every sum of this file is rounded on its own.  hipcc's default (-ffp-contract=fast) contracts
// __fadd_rn(acc, __fmul_rn(x, x)) into one v_pk_fma_f32 -- the intrinsics are plain operators inlined out of the HIP
// headers, which a pragma here does not reach -- so the Makefile compiles this file with -ffp-contract=off; the
// pragma covers the operators written in this file.  (The fma left in the code object belong to the correctly
// rounded division.)
#pragma clang fp contract(off)

namespace rau {

namespace {

constexpr int kThreads = 256;

// columns per workgroup, channel lanes, workgroups per map
struct NormTile {
  int QT, C, nblk;
};
inline NormTile norm_tile(int ncol, int V) {
  NormTile t;
  const int cap = V == 4 ? 32 : 64;
  t.nblk = (ncol + cap - 1) / cap;
  t.QT = (ncol + t.nblk - 1) / t.nblk;
  t.C = kThreads / t.QT;
  return t;
}

// the V elements of column c (quad or position) in the row that starts at element e0 of X; lanes 1..3 of a V = 1
// column are zeros
template <int FT, int V>
__device__ __forceinline__ float4 load_col(const void* X, size_t e0, int c) {
  if (V == 4) return load_feat4<FT>(X, (e0 >> 2) + c);
  return make_float4(load_feat<FT>(X, e0 + c), 0.f, 0.f, 0.f);
}
template <int V>
__device__ __forceinline__ void store_col(float* Y, size_t e0, int c, const float4& v) {
  if (V == 4) reinterpret_cast<float4*>(Y)[(e0 >> 2) + c] = v;
  else Y[e0 + c] = v.x;
}
// positions at and behind SL (pad columns of a pitched row) count as zeros
__device__ __forceinline__ float4 keep4(const float4& v, int s0, int SL) {
  return make_float4(s0 < SL ? v.x : 0.f, s0 + 1 < SL ? v.y : 0.f, s0 + 2 < SL ? v.z : 0.f, s0 + 3 < SL ? v.w : 0.f);
}
__device__ __forceinline__ float4 add_sq(const float4& a, const float4& x) {
  return make_float4(__fadd_rn(a.x, __fmul_rn(x.x, x.x)), __fadd_rn(a.y, __fmul_rn(x.y, x.y)),
                     __fadd_rn(a.z, __fmul_rn(x.z, x.z)), __fadd_rn(a.w, __fmul_rn(x.w, x.w)));
}
__device__ __forceinline__ float4 add_prod(const float4& a, const float4& x, const float4& y) {
  return make_float4(__fadd_rn(a.x, __fmul_rn(x.x, y.x)), __fadd_rn(a.y, __fmul_rn(x.y, y.y)),
                     __fadd_rn(a.z, __fmul_rn(x.z, y.z)), __fadd_rn(a.w, __fmul_rn(x.w, y.w)));
}
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
// x * r, and exact +0 where the position's norm is zero (every x there is +-0)
__device__ __forceinline__ float scale1(float x, float r, float n) { return n == 0.f ? 0.f : __fmul_rn(x, r); }
__device__ __forceinline__ float inv_norm(float n, float eps) { return __fdiv_rn(1.f, fmaxf(n, eps)); }

// grid.x = maps * nblk; thread t: column blk * QT + t % QT, channel lane t / QT
template <int FT, int V>
__global__ __launch_bounds__(kThreads) void k_l2norm_features(int D, int SL, int Sp, int QT, int C, int nblk,
                                                              const void* X, float eps, float* xn, float* nrm) {
  __shared__ float4 part[kThreads];
  __shared__ float4 nrm_s[64], inv_s[64];
  const int t = threadIdx.x, col = t % QT, ch = t / QT;
  const int map = blockIdx.x / nblk, c0 = (blockIdx.x - map * nblk) * QT + col;
  const int ncol = Sp / V, s0 = c0 * V;
  const bool live = ch < C && c0 < ncol;
  const size_t m0 = (size_t)map * D * Sp;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc = zero;
  if (live) {
    // four rows in flight.  A row behind D is loaded from row D - 1 and then replaced by zeros (a select on the
    // value, not a branch around the load): it adds the square of +0.
    for (int d = ch; d < D; d += 4 * C) {
      const float4 x0 = load_col<FT, V>(X, m0 + (size_t)d * Sp, c0);
      const float4 x1 = load_col<FT, V>(X, m0 + (size_t)min(d + C, D - 1) * Sp, c0);
      const float4 x2 = load_col<FT, V>(X, m0 + (size_t)min(d + 2 * C, D - 1) * Sp, c0);
      const float4 x3 = load_col<FT, V>(X, m0 + (size_t)min(d + 3 * C, D - 1) * Sp, c0);
      acc = add_sq(acc, keep4(x0, s0, SL));
      acc = add_sq(acc, keep4(x1, d + C < D ? s0 : SL, SL));
      acc = add_sq(acc, keep4(x2, d + 2 * C < D ? s0 : SL, SL));
      acc = add_sq(acc, keep4(x3, d + 3 * C < D ? s0 : SL, SL));
    }
  }
  part[t] = acc;
  __syncthreads();
  if (ch == 0) {
    float4 tot = part[col];
    for (int k = 1; k < C; ++k) tot = add4(tot, part[k * QT + col]);
    const float4 n = make_float4(__fsqrt_rn(tot.x), __fsqrt_rn(tot.y), __fsqrt_rn(tot.z), __fsqrt_rn(tot.w));
    nrm_s[col] = n;
    inv_s[col] = make_float4(inv_norm(n.x, eps), inv_norm(n.y, eps), inv_norm(n.z, eps), inv_norm(n.w, eps));
    if (nrm && c0 < ncol) store_col<V>(nrm, (size_t)map * Sp, c0, n);   // pad positions: sqrt(+0) = +0
  }
  __syncthreads();
  if (!live) return;
  const float4 n = nrm_s[col], r = inv_s[col];
  auto put = [&](int d, const float4& x) {
    const float4 v = keep4(x, s0, SL);   // pad positions have n = 0: +0 out
    store_col<V>(xn, m0 + (size_t)d * Sp, c0,
                 make_float4(scale1(v.x, r.x, n.x), scale1(v.y, r.y, n.y), scale1(v.z, r.z, n.z), scale1(v.w, r.w, n.w)));
  };
  for (int d = ch; d < D; d += 4 * C) {   // the loads of four rows, then their stores
    const bool h1 = d + C < D, h2 = d + 2 * C < D, h3 = d + 3 * C < D;
    const float4 x0 = load_col<FT, V>(X, m0 + (size_t)d * Sp, c0);
    const float4 x1 = load_col<FT, V>(X, m0 + (size_t)min(d + C, D - 1) * Sp, c0);
    const float4 x2 = load_col<FT, V>(X, m0 + (size_t)min(d + 2 * C, D - 1) * Sp, c0);
    const float4 x3 = load_col<FT, V>(X, m0 + (size_t)min(d + 3 * C, D - 1) * Sp, c0);
    put(d, x0);
    if (h1) put(d + C, x1);
    if (h2) put(d + 2 * C, x2);
    if (h3) put(d + 3 * C, x3);
  }
}

// In place on dX [rows][D][Sp].  img_start / img_samples (both or neither): row i is an image slot, reads the xn and
// nrm of the first sample of its list and is left alone where the list is empty (uniform over the workgroup).
template <int V>
__global__ __launch_bounds__(kThreads) void k_l2norm_backward(int D, int SL, int Sp, int QT, int C, int nblk,
                                                              const float* __restrict__ xn,
                                                              const float* __restrict__ nrm, float eps, float* dX,
                                                              const int32_t* __restrict__ img_start,
                                                              const int32_t* __restrict__ img_samples) {
  __shared__ float4 part[kThreads];
  __shared__ float4 dot_s[64], inv_s[64];
  const int t = threadIdx.x, col = t % QT, ch = t / QT;
  const int row = blockIdx.x / nblk, c0 = (blockIdx.x - row * nblk) * QT + col;
  int src = row;
  if (img_start) {
    const int b0 = img_start[row];
    if (b0 == img_start[row + 1]) return;   // no sample names this image: its row is zeros and stays so
    src = img_samples[b0];
  }
  const int ncol = Sp / V, s0 = c0 * V;
  const bool live = ch < C && c0 < ncol;
  const size_t g0 = (size_t)row * D * Sp, y0 = (size_t)src * D * Sp;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc = zero;
  if (live) {
    for (int d = ch; d < D; d += 2 * C) {   // two rows of each operand in flight
      const size_t o0 = (size_t)d * Sp, o1 = (size_t)min(d + C, D - 1) * Sp;   // (behind D: row D - 1, as zeros)
      const float4 ga = load_col<RAU_FEAT_F32, V>(dX, g0 + o0, c0), ya = load_col<RAU_FEAT_F32, V>(xn, y0 + o0, c0);
      const float4 gb = load_col<RAU_FEAT_F32, V>(dX, g0 + o1, c0), yb = load_col<RAU_FEAT_F32, V>(xn, y0 + o1, c0);
      acc = add_prod(acc, keep4(ga, s0, SL), ya);
      acc = add_prod(acc, keep4(gb, d + C < D ? s0 : SL, SL), yb);
    }
  }
  part[t] = acc;
  __syncthreads();
  if (ch == 0) {
    float4 tot = part[col];
    for (int k = 1; k < C; ++k) tot = add4(tot, part[k * QT + col]);
    const float4 n = c0 < ncol ? load_col<RAU_FEAT_F32, V>(nrm, (size_t)src * Sp, c0) : zero;
    // under eps the forward is x / eps: no projection term
    dot_s[col] = make_float4(n.x < eps ? 0.f : tot.x, n.y < eps ? 0.f : tot.y, n.z < eps ? 0.f : tot.z,
                             n.w < eps ? 0.f : tot.w);
    inv_s[col] = make_float4(inv_norm(n.x, eps), inv_norm(n.y, eps), inv_norm(n.z, eps), inv_norm(n.w, eps));
  }
  __syncthreads();
  if (!live) return;
  const float4 c = dot_s[col], r = inv_s[col];
  for (int d = ch; d < D; d += 2 * C) {
    const size_t o0 = (size_t)d * Sp, o1 = (size_t)min(d + C, D - 1) * Sp;
    const bool two = d + C < D;
    const float4 ga = load_col<RAU_FEAT_F32, V>(dX, g0 + o0, c0), ya = load_col<RAU_FEAT_F32, V>(xn, y0 + o0, c0);
    const float4 gb = load_col<RAU_FEAT_F32, V>(dX, g0 + o1, c0), yb = load_col<RAU_FEAT_F32, V>(xn, y0 + o1, c0);
    auto grad = [&](const float4& g, const float4& y) {
      const float4 o = make_float4(__fmul_rn(r.x, __fsub_rn(g.x, __fmul_rn(y.x, c.x))),
                                   __fmul_rn(r.y, __fsub_rn(g.y, __fmul_rn(y.y, c.y))),
                                   __fmul_rn(r.z, __fsub_rn(g.z, __fmul_rn(y.z, c.z))),
                                   __fmul_rn(r.w, __fsub_rn(g.w, __fmul_rn(y.w, c.w))));
      return keep4(o, s0, SL);   // pad columns leave as +0
    };
    store_col<V>(dX, g0 + o0, c0, grad(ga, ya));
    if (two) store_col<V>(dX, g0 + o1, c0, grad(gb, yb));
  }
}

template <int V>
void launch_features(hipStream_t st, int ft, dim3 grid, int D, int SL, int Sp, const NormTile& t, const void* X,
                     float eps, float* xn, float* nrm) {
#define NORM_FT(FT)                                                                                           \
  hipLaunchKernelGGL((k_l2norm_features<FT, V>), grid, dim3(kThreads), 0, st, D, SL, Sp, t.QT, t.C, t.nblk, X, \
                     eps, xn, nrm)
  switch (ft) {
    case RAU_FEAT_F16: NORM_FT(RAU_FEAT_F16); break;
    case RAU_FEAT_BF16: NORM_FT(RAU_FEAT_BF16); break;
    case RAU_FEAT_E4M3: NORM_FT(RAU_FEAT_E4M3); break;
    case RAU_FEAT_E5M2: NORM_FT(RAU_FEAT_E5M2); break;
    default: NORM_FT(RAU_FEAT_F32); break;
  }
#undef NORM_FT
}
inline bool norm_shape_ok(int n, int D, int SL, int Sp, float eps) {
  // pitched rows are whole quads; a pitch that is no multiple of 4 is a dense tensor's (rau_dev_l2norm); the grid
  // (at most one workgroup per column and map) stays inside 31 bits
  return n >= 0 && D > 0 && SL > 0 && SL <= Sp && (Sp % 4 == 0 || SL == Sp) && std::isfinite(eps) && eps > 0.f &&
         (size_t)n * (size_t)Sp < 0x7fffffffu;
}

}  // namespace

hipError_t l2norm_features(hipStream_t st, int n_maps, int D, int SL, int Sp, const void* X, int ft, float eps,
                           float* xn, float* nrm) {
  if (!norm_shape_ok(n_maps, D, SL, Sp, eps) || !feat_type_ok(ft) || !X || !xn) return hipErrorInvalidValue;
  if (n_maps == 0) return hipSuccess;
  const int V = Sp % 4 == 0 ? 4 : 1;
  const NormTile t = norm_tile(Sp / V, V);
  const dim3 grid((unsigned)n_maps * t.nblk);
  if (V == 4) launch_features<4>(st, ft, grid, D, SL, Sp, t, X, eps, xn, nrm);
  else launch_features<1>(st, ft, grid, D, SL, Sp, t, X, eps, xn, nrm);
  return hipGetLastError();
}

hipError_t l2norm_backward(hipStream_t st, int rows, int D, int SL, int Sp, const float* xn, const float* nrm,
                           float eps, float* dX, const int32_t* img_start, const int32_t* img_samples) {
  if (!norm_shape_ok(rows, D, SL, Sp, eps) || !xn || !nrm || !dX || (img_start == nullptr) != (img_samples == nullptr))
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  const int V = Sp % 4 == 0 ? 4 : 1;
  const NormTile t = norm_tile(Sp / V, V);
  const dim3 grid((unsigned)rows * t.nblk);
  if (V == 4)
    hipLaunchKernelGGL(k_l2norm_backward<4>, grid, dim3(kThreads), 0, st, D, SL, Sp, t.QT, t.C, t.nblk, xn, nrm, eps,
                       dX, img_start, img_samples);
  else
    hipLaunchKernelGGL(k_l2norm_backward<1>, grid, dim3(kThreads), 0, st, D, SL, Sp, t.QT, t.C, t.nblk, xn, nrm, eps,
                       dX, img_start, img_samples);
  return hipGetLastError();
}

}  // namespace rau

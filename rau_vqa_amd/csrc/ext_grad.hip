// ext_grad.hip -- caller-supplied gradients at the step's three outputs in the step-level backward
// (rau_backward_ext): where dF/dlogits, dF/ddo_pred and dF/dattprob of an objective F the library does not
// implement join the built-in terms.  All float32, every operation rounded once, in this order:
//   ext_dl      x = dl[h,b,k] * hop_w[h]  (scale_hops' product, the same bits), then x = x + d_logits[h,b,k];
//               when the forward wrote no dl (a batch without labels or answer set) x = d_logits[h,b,k] exactly,
//               or +0 without a d_logits: dl is written, never read.  One pass: it takes scale_hops' place.
//   ext_signal  s_ext = (d_dopred[h,b] * x) * (1 - x), x = do_pred[h,b]: the gradient through the sigmoid, the last
//               line of k_select_signal.  s = s_sel + s_ext behind select_signal (acc), else s = s_ext; then
//               add[r][m] = s * wd[m], the rank-1 addend of the head_dgrad GEMM.
//   ext_da      da[h,b,s] = att_sup's value + d_attprob[h,b,s] behind att_sup_grad (acc), else d_attprob[h,b,s]
//               exactly; +0 behind the sample's region count and in the pitch padding.  d_attprob is DENSE
//               [H,n,S]; da is the attention-backward kernels' pitched addend (HopGrad::da_out).
// Every element has one writer and a fixed expression: no atomics, no device scratch, repeated calls give the
// same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace rau {
namespace {

// per4 = quads per hop, n4 = quads in all: a quad never straddles two hops (K % 4 == 0)
template <bool HAVE_DL, bool HAVE_D>
__global__ __launch_bounds__(256) void k_ext_dl(size_t per4, size_t n4, const float* __restrict__ w,
    const float4* __restrict__ d, float4* __restrict__ x) {
  RAU_CHAIN_PRIO();
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HAVE_DL) {
      const float wh = w[i / per4];
      v = x[i];
      v.x = __fmul_rn(v.x, wh);
      v.y = __fmul_rn(v.y, wh);
      v.z = __fmul_rn(v.z, wh);
      v.w = __fmul_rn(v.w, wh);
      if (HAVE_D) {
        const float4 e = d[i];
        v.x = __fadd_rn(v.x, e.x);
        v.y = __fadd_rn(v.y, e.y);
        v.z = __fadd_rn(v.z, e.z);
        v.w = __fadd_rn(v.w, e.w);
      }
    } else if (HAVE_D) {
      v = d[i];
    }
    x[i] = v;
  }
}

// The ragged form (K % 4 != 0): d is dense [H][rows][K], x has rows at pitch ld = K rounded up to a multiple of 4.
// One thread per element of x; the pad columns K..ld-1 are written +0 whatever they held.  The arithmetic of an
// element is k_ext_dl's.
template <bool HAVE_DL, bool HAVE_D>
__global__ __launch_bounds__(256) void k_ext_dl_rag(size_t rows_per_hop, int K, int ld, size_t n,
    const float* __restrict__ w, const float* __restrict__ d, float* __restrict__ x) {
  RAU_CHAIN_PRIO();
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / (size_t)ld;
    const int k = (int)(i - row * (size_t)ld);
    float v = 0.f;
    if (k < K) {
      if (HAVE_DL) {
        v = __fmul_rn(x[i], w[row / rows_per_hop]);
        if (HAVE_D) v = __fadd_rn(v, d[row * (size_t)K + k]);
      } else if (HAVE_D) {
        v = d[row * (size_t)K + k];
      }
    }
    x[i] = v;
  }
}

// one 256-thread workgroup per row r = h * Bper + b, as k_select_signal; every thread forms the row's (uniform) s
template <bool ACC>
__global__ __launch_bounds__(256) void k_ext_signal(int M, const float* __restrict__ dopred,
    const float* __restrict__ ddp, const float* __restrict__ wd, float* __restrict__ s_io,
    float* __restrict__ add) {
  RAU_CHAIN_PRIO();
  const int r = blockIdx.x;
  const float x = dopred[r];
  float s = __fmul_rn(__fmul_rn(ddp[r], x), __fsub_rn(1.f, x));
  if (ACC) s = __fadd_rn(s_io[r], s);
  for (int m = threadIdx.x; m < M; m += 256) add[(size_t)r * M + m] = __fmul_rn(s, wd[m]);
  if (ACC) __syncthreads();   // every thread has read the row's s_sel before thread 0 replaces it
  if (threadIdx.x == 0) s_io[r] = s;
}

constexpr int kRowsPerWg = 4;   // one wave per (hop, sample) row, as k_att_grad

// Row r = h * Bper + b: d rows dense at pitch S, da rows at pitch d_rs >= S, written over the whole pitch.
// VEC: S and d_rs are multiples of 4 and both bases 16-byte aligned.
template <bool VEC, bool ACC>
__global__ __launch_bounds__(64 * kRowsPerWg) void k_ext_da(int rows, int Bper, int S, const float* __restrict__ d,
    const int32_t* __restrict__ nreg, float* __restrict__ da, int d_rs) {
  RAU_CHAIN_PRIO();
  const int r = blockIdx.x * kRowsPerWg + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (r >= rows) return;
  const int b = r % Bper;
  const int nv = nreg ? min(max(nreg[b], 1), S) : S;   // clamped like the attention kernels' counts
  const float* sr = d + (size_t)r * S;
  float* dr = da + (size_t)r * d_rs;
  if (VEC) {
    for (int q = l; q < d_rs / 4; q += 64) {
      const int s = q * 4;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s < nv) {   // s < S, and S % 4 == 0: the whole quad lies inside the dense row
        const float4 e = reinterpret_cast<const float4*>(sr)[q];
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ACC) p = reinterpret_cast<const float4*>(dr)[q];
        o.x = ACC ? __fadd_rn(p.x, e.x) : e.x;
        if (s + 1 < nv) o.y = ACC ? __fadd_rn(p.y, e.y) : e.y;
        if (s + 2 < nv) o.z = ACC ? __fadd_rn(p.z, e.z) : e.z;
        if (s + 3 < nv) o.w = ACC ? __fadd_rn(p.w, e.w) : e.w;
      }
      reinterpret_cast<float4*>(dr)[q] = o;
    }
  } else {
    for (int s = l; s < d_rs; s += 64) {
      float o = 0.f;
      if (s < nv) o = ACC ? __fadd_rn(dr[s], sr[s]) : sr[s];
      dr[s] = o;
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
int grid_for(size_t n) { return (int)std::min<size_t>(std::max<size_t>((n + 255) / 256, 1), 256 * 8); }

}  // namespace

hipError_t ext_dl(hipStream_t st, int H, size_t rows_per_hop, int K, int ld, const float* w_dev, const float* d,
                  float* dl) {
  if (K < 1 || ld < K) return hipErrorInvalidValue;
  if (ld != K) {   // dense ragged d into the pitched dl
    const size_t n = rows_per_hop * H * (size_t)ld;
    if (n == 0) return hipSuccess;
    const dim3 grid(grid_for(n)), block(256);
    if (w_dev && d) hipLaunchKernelGGL((k_ext_dl_rag<true, true>), grid, block, 0, st, rows_per_hop, K, ld, n, w_dev, d, dl);
    else if (w_dev) hipLaunchKernelGGL((k_ext_dl_rag<true, false>), grid, block, 0, st, rows_per_hop, K, ld, n, w_dev, d, dl);
    else if (d) hipLaunchKernelGGL((k_ext_dl_rag<false, true>), grid, block, 0, st, rows_per_hop, K, ld, n, w_dev, d, dl);
    else hipLaunchKernelGGL((k_ext_dl_rag<false, false>), grid, block, 0, st, rows_per_hop, K, ld, n, w_dev, d, dl);
    return hipGetLastError();
  }
  const size_t per_hop = rows_per_hop * (size_t)K;
  const size_t n = per_hop * H;
  if (n == 0) return hipSuccess;
  if ((per_hop & 3) || !aligned16(dl) || (d && !aligned16(d))) return hipErrorInvalidValue;
  const size_t per4 = per_hop / 4, n4 = n / 4;
  const dim3 grid(grid_for(n4)), block(256);
  const float4* d4 = reinterpret_cast<const float4*>(d);
  float4* x4 = reinterpret_cast<float4*>(dl);
  if (w_dev && d) hipLaunchKernelGGL((k_ext_dl<true, true>), grid, block, 0, st, per4, n4, w_dev, d4, x4);
  else if (w_dev) hipLaunchKernelGGL((k_ext_dl<true, false>), grid, block, 0, st, per4, n4, w_dev, d4, x4);
  else if (d) hipLaunchKernelGGL((k_ext_dl<false, true>), grid, block, 0, st, per4, n4, w_dev, d4, x4);
  else hipLaunchKernelGGL((k_ext_dl<false, false>), grid, block, 0, st, per4, n4, w_dev, d4, x4);
  return hipGetLastError();
}

hipError_t ext_signal(hipStream_t st, int rows, int M, const float* dopred, const float* ddp, const float* wd,
                      bool acc, float* s, float* add) {
  if (rows <= 0) return hipSuccess;
  if (M < 1 || !dopred || !ddp || !wd || !s || !add) return hipErrorInvalidValue;
  if (acc) hipLaunchKernelGGL(k_ext_signal<true>, dim3(rows), dim3(256), 0, st, M, dopred, ddp, wd, s, add);
  else hipLaunchKernelGGL(k_ext_signal<false>, dim3(rows), dim3(256), 0, st, M, dopred, ddp, wd, s, add);
  return hipGetLastError();
}

hipError_t ext_da(hipStream_t st, int hops, int Bper, int S, const float* d, const int32_t* nreg, bool acc,
                  float* da, int d_rs) {
  const int rows = hops * Bper;
  if (rows <= 0) return hipSuccess;
  if (Bper < 1 || S < 1 || d_rs < S || !d || !da) return hipErrorInvalidValue;
  const dim3 grid((rows + kRowsPerWg - 1) / kRowsPerWg), block(64 * kRowsPerWg);
  const bool vec = ((S | d_rs) & 3) == 0 && aligned16(d) && aligned16(da);
#define RAU_EXT_DA(V, A) \
  hipLaunchKernelGGL((k_ext_da<V, A>), grid, block, 0, st, rows, Bper, S, d, nreg, da, d_rs)
  if (vec && acc) RAU_EXT_DA(true, true);
  else if (vec) RAU_EXT_DA(true, false);
  else if (acc) RAU_EXT_DA(false, true);
  else RAU_EXT_DA(false, false);
#undef RAU_EXT_DA
  return hipGetLastError();
}

}  // namespace rau

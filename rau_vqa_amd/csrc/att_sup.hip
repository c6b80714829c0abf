// att_sup.hip -- attention supervision: the loss of the attprob output against per-sample target maps, its gradient
// in the step-level backward (rau_backward_att) and the statistics a training loop logs (rau_att_stats); the same
// kernels serve the module-level criterion (rau_att_criterion_forward / _backward).
// For hop h, sample b, position s, with a = attprob[h,b,s], t = the batch's target map t[b,s] >= 0, n = samples per
// hop, n_reg[b] the sample's region count (S without counts), eps = 1e-12f:
//   ATT_h      = (1/n) sum_b sum_{s < n_reg[b]} t * ( -log(a + eps) )
//   da[h,b,s]  = -( (w[h] * t) / (a + eps) ) / n          float32, every step rounded once, in this order
// and exactly +0 where t == 0, where s >= n_reg[b] and in the pitch padding.  eps keeps the value finite for every
// a >= 0; the softmax gradient multiplies it by a, so where a has underflowed to 0 nothing flows back.
// With sample weights s (rau_set_sample_weights) w[h] is replaced by __fmul_rn(w[h], s_b) in da and a row's loss sum
// enters ATT_h as __fmul_rn(s_b, sum); mass, hits and the supervised-row count stay unweighted.
// k_att_grad writes da for all active hops in one launch, over the whole pitch (zeros included): the buffer is the
// attention-backward kernels' pitched addend (HopGrad::da_out) and needs no clearing.
// Statistics: a row is SUPERVISED when some t[b,s] > 0 with s < n_reg[b].  k_att_rows forms per (hop, sample) row
// the loss sum, the attention mass on the positions with t > 0, and whether the first-max attention position has
// t > 0 (the pointing game); k_att_finish adds the rows of a hop.  Lane l of the one wave that owns a row (a hop)
// takes elements l, l + 64, .. in ascending order and the 64 lane values meet in a fixed butterfly: no atomics,
// repeated calls give the same bits.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace rau {
namespace {

constexpr int kRowsPerWg = 4;   // one wave per row: HA * B rows of a few hundred floats is a latency-sized job

__device__ __forceinline__ float att_grad_1(float w, float t, float a, float n) {
  if (!(t > 0.f)) return 0.f;
  return __fdiv_rn(-__fdiv_rn(__fmul_rn(w, t), __fadd_rn(a, 1e-12f)), n);
}

// Row r = h * Bper + b.  a / da rows at pitch a_rs / d_rs (hop-major, rows contiguous), t rows at pitch t_rs; the
// row has S positions and da is written over d_rs.  w_dev [hops] device, or null: `scale` for every hop.
// VEC: all three pitches are multiples of 4 and the bases 16-byte aligned (the step path: everything at pitch Sp).
template <bool VEC>
__global__ __launch_bounds__(64 * kRowsPerWg) void k_att_grad(int rows, int Bper, int S, const float* __restrict__ a,
    int a_rs, const float* __restrict__ t, int t_rs, const int32_t* __restrict__ nreg,
    const float* __restrict__ w_dev, float scale, float* __restrict__ da, int d_rs,
    const float* __restrict__ sw) {
  RAU_CHAIN_PRIO();
  const int r = blockIdx.x * kRowsPerWg + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (r >= rows) return;
  const int h = r / Bper, b = r - h * Bper;
  const int nv = nreg ? min(max(nreg[b], 1), S) : S;   // clamped like the attention kernels' counts
  // the hop weight times the sample weight, one rounded product (no weights: times 1, exact); one load per row
  const float w = __fmul_rn(w_dev ? w_dev[h] : scale, sw ? sw[b] : 1.f), n = (float)Bper;
  const float* ar = a + (size_t)r * a_rs;
  const float* tr = t + (size_t)b * t_rs;
  float* dr = da + (size_t)r * d_rs;
  if (VEC) {
    for (int q = l; q < d_rs / 4; q += 64) {
      const int s = q * 4;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s < nv) {
        const float4 av = reinterpret_cast<const float4*>(ar)[q], tv = reinterpret_cast<const float4*>(tr)[q];
        o.x = att_grad_1(w, tv.x, av.x, n);
        if (s + 1 < nv) o.y = att_grad_1(w, tv.y, av.y, n);
        if (s + 2 < nv) o.z = att_grad_1(w, tv.z, av.z, n);
        if (s + 3 < nv) o.w = att_grad_1(w, tv.w, av.w, n);
      }
      reinterpret_cast<float4*>(dr)[q] = o;
    }
  } else {
    for (int s = l; s < d_rs; s += 64) dr[s] = s < nv ? att_grad_1(w, tr[s], ar[s], n) : 0.f;
  }
}

// (value, index) butterfly of the first maximum: the larger value wins, equal values the lower index
__device__ __forceinline__ void wave_first_max(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}
__device__ __forceinline__ float wave_sum_rn(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

// rowf [2][rows]: loss sum | mass; rowi [2][rows]: supervised | hit
__global__ __launch_bounds__(64 * kRowsPerWg) void k_att_rows(int rows, int Bper, int S, const float* __restrict__ a,
    int a_rs, const float* __restrict__ t, int t_rs, const int32_t* __restrict__ nreg, float* __restrict__ rowf,
    int32_t* __restrict__ rowi, const float* __restrict__ sw) {
  const int r = blockIdx.x * kRowsPerWg + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (r >= rows) return;
  const int b = r % Bper;
  const int nv = nreg ? min(max(nreg[b], 1), S) : S;
  const float* ar = a + (size_t)r * a_rs;
  const float* tr = t + (size_t)b * t_rs;
  float loss = 0.f, mass = 0.f, best = -1.f;
  int arg = 0x7fffffff, sup = 0;
  for (int s = l; s < nv; s += 64) {
    const float av = ar[s], tv = tr[s];
    if (tv > 0.f) {
      loss = __fadd_rn(loss, __fmul_rn(tv, -logf(__fadd_rn(av, 1e-12f))));
      mass = __fadd_rn(mass, av);
      sup = 1;
    }
    if (av > best) { best = av; arg = s; }   // ascending s: the lane's first maximum
  }
  loss = wave_sum_rn(loss);
  mass = wave_sum_rn(mass);
  wave_first_max(best, arg);
  sup = __any(sup) ? 1 : 0;
  if (l == 0) {
    rowf[r] = __fmul_rn(sw ? sw[b] : 1.f, loss);
    rowf[rows + r] = mass;
    rowi[r] = sup;
    rowi[rows + r] = (sup && arg < nv && tr[arg] > 0.f) ? 1 : 0;
  }
}

// One wave per hop.  outf [2][hops]: loss = sum / Bper | mass = sum over the supervised rows / their number (0 when
// there is none); outi [2][hops]: hits | supervised rows (the same for every hop).
__global__ __launch_bounds__(64) void k_att_finish(int hops, int Bper, const float* __restrict__ rowf,
    const int32_t* __restrict__ rowi, float* __restrict__ outf, int32_t* __restrict__ outi) {
  const int h = blockIdx.x, l = threadIdx.x, rows = hops * Bper;
  float loss = 0.f, mass = 0.f;
  int hits = 0, nsup = 0;
  for (int b = l; b < Bper; b += 64) {
    const int r = h * Bper + b;
    if (!rowi[r]) continue;
    loss = __fadd_rn(loss, rowf[r]);
    mass = __fadd_rn(mass, rowf[rows + r]);
    hits += rowi[rows + r];
    ++nsup;
  }
  loss = wave_sum_rn(loss);
  mass = wave_sum_rn(mass);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hits += __shfl_xor(hits, o, 64);
    nsup += __shfl_xor(nsup, o, 64);
  }
  if (l != 0) return;
  outf[h] = __fdiv_rn(loss, (float)Bper);
  outf[hops + h] = nsup > 0 ? __fdiv_rn(mass, (float)nsup) : 0.f;
  outi[h] = hits;
  outi[hops + h] = nsup;
}

bool vec_ok(const void* a, int a_rs, const void* t, int t_rs, const void* d, int d_rs) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(t) | reinterpret_cast<uintptr_t>(d);
  return ((a_rs | t_rs | d_rs) & 3) == 0 && (p & 15u) == 0;
}

}  // namespace

hipError_t att_sup_grad(hipStream_t st, int hops, int Bper, int S, const float* a, int a_rs, const float* t,
                        int t_rs, const int32_t* nreg, const float* w_dev, float scale, float* da, int d_rs,
                        const float* sw) {
  const int rows = hops * Bper;
  if (rows <= 0) return hipSuccess;
  if (Bper < 1 || S < 1 || a_rs < S || t_rs < S || d_rs < S) return hipErrorInvalidValue;
  const dim3 grid((rows + kRowsPerWg - 1) / kRowsPerWg), block(64 * kRowsPerWg);
  // VEC reads a and t in whole quads below the count: both rows must reach the end of the quad that holds S - 1
  if (vec_ok(a, a_rs, t, t_rs, da, d_rs))
    hipLaunchKernelGGL(k_att_grad<true>, grid, block, 0, st, rows, Bper, S, a, a_rs, t, t_rs, nreg, w_dev, scale, da,
                       d_rs, sw);
  else
    hipLaunchKernelGGL(k_att_grad<false>, grid, block, 0, st, rows, Bper, S, a, a_rs, t, t_rs, nreg, w_dev, scale, da,
                       d_rs, sw);
  return hipGetLastError();
}

hipError_t att_sup_stats(hipStream_t st, int hops, int Bper, int S, const float* a, int a_rs, const float* t,
                         int t_rs, const int32_t* nreg, float* rowf, int32_t* rowi, float* outf, int32_t* outi,
                         const float* sw) {
  const int rows = hops * Bper;
  if (rows <= 0) return hipSuccess;
  if (Bper < 1 || S < 1 || a_rs < S || t_rs < S) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_att_rows, dim3((rows + kRowsPerWg - 1) / kRowsPerWg), dim3(64 * kRowsPerWg), 0, st, rows,
                     Bper, S, a, a_rs, t, t_rs, nreg, rowf, rowi, sw);
  hipLaunchKernelGGL(k_att_finish, dim3(hops), dim3(64), 0, st, hops, Bper, rowf, rowi, outf, outi);
  return hipGetLastError();
}

}  // namespace rau

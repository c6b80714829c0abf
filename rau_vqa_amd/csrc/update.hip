// update.hip -- rau_update: gradient noise, norm clip and the optimizer rule for all three parameter groups in
// two launches, and the optimizer state's way in and out (include/rau.h "update with a rule and a clip scope").
//
// The update is three bandwidth passes with a grid-wide dependency between them: every element's clip scale
// depends on the norm of all elements.  rau_noise_clip_adam walks that per group with scalar accesses and a
// single-workgroup launch in the middle: nine launches.  Here
//   1. k_upd_noise_sqnorm  grid (kUpdParts, 3): noise into the gradients, kUpdParts partial sums of squares per group
//   2. k_upd_apply         grid (<= kUpdParts, 3): EVERY workgroup first sums the 3 x kUpdParts partials itself
//                          (12 KB out of L2, in finish_norm's order, so all workgroups hold the same bits), then
//                          clips and applies the rule; workgroup (0, g) also writes the norms out
// so the single-workgroup finish is not a launch of its own, and nothing waits on another workgroup: the only
// ordering is the stream's.  No cooperative launch, no float atomics.  blockIdx.y is the group; the groups'
// pointers, lengths, step sizes and noise keys travel by value (UpdGroups).
// x, g, m, v move as float4 where the group's pointers are 16-byte aligned; a group whose length is not a multiple
// of 4 finishes with scalar accesses, and a misaligned group is scalar throughout.  The element order of the
// sums is add_noise_sqnorm's (thread t of workgroup b owns quads b*256 + t + k*kUpdParts*256), and the element
// arithmetic is update_elem.h's, shared with the per-group kernels: RAU_OPT_ADAM with RAU_CLIP_GROUP gives
// rau_noise_clip_adam's bits.
//
// rau_update_ex (decoupled weight decay, per-layer step sizes, frozen layers, a weight average) is the same two
// launches under names of their own, k_upd_ex_sqnorm and k_upd_ex_apply, beside the two above, which it leaves
// untouched.  Its coefficients are per SEGMENT (the weight or the bias part of a layout entry; kernels.h UpdSegs).
// Segment ends are not multiples of 4, so a quad can span several segments and every coefficient is looked up per
// element; loads and stores stay 16 bytes wide.  The table travels by value and is copied to LDS at kernel start: the
// per-thread cursor (a thread's quads rise, so it only moves forward) indexes LDS, which costs no private memory.
// Frozen elements add nothing to a sum and draw no noise, so with no options set the element order, the partials
// and the finish give rau_update's bits.  k_upd_ex_apply is templated on the rule and on "has average": without one
// it moves 28 bytes per element, with one 36.  rau_ema_swap is a third kernel, k_ema_swap: one launch, grid y = group.
#include <cmath>

#include "rau_ctx.h"
#include "update_elem.h"

namespace rau {
namespace {

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
template <int RULE>
__device__ __forceinline__ void rule_elem(float gi, float& m, float& v, float& x, float stepsize, float beta1,
                                          float beta2, float eps) {
  if constexpr (RULE == RAU_OPT_ADAM) adam_elem(gi, m, v, x, stepsize, beta1, beta2, eps);
  else adamax_elem(gi, m, v, x, stepsize, beta1, beta2, eps);
}
// Quads first, first + stride, .. of one flat vector: g scaled by sc (and written back when WRITE_G), then the rule.
// vec: all four pointers are 16-byte aligned.  Every access is below n.
template <int RULE, bool WRITE_G, typename GT>
__device__ __forceinline__ void apply_quads(size_t n, float* __restrict__ x, GT* __restrict__ g,
                                            float* __restrict__ m, float* __restrict__ v, bool vec, float sc,
                                            float stepsize, float beta1, float beta2, float eps, size_t first,
                                            size_t stride) {
  for (size_t q = first; q * 4 < n; q += stride) {
    const size_t e = q * 4;
    if (vec && e + 4 <= n) {
      float4 g4 = *reinterpret_cast<const float4*>(g + e);
      float4 m4 = *reinterpret_cast<const float4*>(m + e);
      float4 v4 = *reinterpret_cast<const float4*>(v + e);
      float4 x4 = *reinterpret_cast<const float4*>(x + e);
      g4.x *= sc; g4.y *= sc; g4.z *= sc; g4.w *= sc;
      rule_elem<RULE>(g4.x, m4.x, v4.x, x4.x, stepsize, beta1, beta2, eps);
      rule_elem<RULE>(g4.y, m4.y, v4.y, x4.y, stepsize, beta1, beta2, eps);
      rule_elem<RULE>(g4.z, m4.z, v4.z, x4.z, stepsize, beta1, beta2, eps);
      rule_elem<RULE>(g4.w, m4.w, v4.w, x4.w, stepsize, beta1, beta2, eps);
      if constexpr (WRITE_G) *reinterpret_cast<float4*>(g + e) = g4;
      *reinterpret_cast<float4*>(m + e) = m4;
      *reinterpret_cast<float4*>(v + e) = v4;
      *reinterpret_cast<float4*>(x + e) = x4;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) {
          const float gi = g[e + j] * sc;
          if constexpr (WRITE_G) g[e + j] = gi;
          float mi = m[e + j], vi = v[e + j], xi = x[e + j];
          rule_elem<RULE>(gi, mi, vi, xi, stepsize, beta1, beta2, eps);
          m[e + j] = mi;
          v[e + j] = vi;
          x[e + j] = xi;
        }
    }
  }
}

__global__ void __launch_bounds__(256) k_upd_noise_sqnorm(UpdGroups G, float nstd, float* __restrict__ partial) {
  RAU_CHAIN_PRIO();
  __shared__ float s_sum[4];
  const int gi = blockIdx.y;
  const size_t n = G.n[gi];
  float* __restrict__ g = G.g[gi];
  const uint64_t seed = G.seed[gi];
  const bool vec = ((uintptr_t)g & 15) == 0;
  float acc = 0.f;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q * 4 < n; q += (size_t)gridDim.x * blockDim.x) {
    float z[4];
    noise_quad(q, (uint32_t)gi, seed, nstd, z);
    const size_t e = q * 4;
    if (vec && e + 4 <= n) {
      float4 v = *reinterpret_cast<const float4*>(g + e);
      v.x = noise_elem(v.x, z[0], nstd, acc);
      v.y = noise_elem(v.y, z[1], nstd, acc);
      v.z = noise_elem(v.z, z[2], nstd, acc);
      v.w = noise_elem(v.w, z[3], nstd, acc);
      *reinterpret_cast<float4*>(g + e) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) g[e + j] = noise_elem(g[e + j], z[j], nstd, acc);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[(size_t)gi * kUpdParts + blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

template <int RULE>
__global__ void __launch_bounds__(256) k_upd_apply(UpdGroups G, int global_clip, float clip, float beta1, float beta2,
                                                   float eps, const float* __restrict__ partial,
                                                   float* __restrict__ norms) {
  RAU_CHAIN_PRIO();
  const int gi = blockIdx.y;
  const size_t n = G.n[gi];
  // a workgroup whose first quad lies behind a short group has nothing to do (workgroup 0 writes the norm)
  if (blockIdx.x != 0 && (size_t)blockIdx.x * blockDim.x * 4 >= n) return;
  __shared__ float s_sum[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // finish_norm's order, per group
    float acc = 0.f;
    for (int i = threadIdx.x; i < kUpdParts; i += 256) acc += partial[k * kUpdParts + i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_sum[k][threadIdx.x >> 6] = acc;
  }
  __syncthreads();
  const float s0 = (s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]);
  const float s1 = (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]);
  const float s2 = (s_sum[2][0] + s_sum[2][1]) + (s_sum[2][2] + s_sum[2][3]);
  const float own = sqrtf(gi == 0 ? s0 : gi == 1 ? s1 : s2);
  const float all = sqrtf((s0 + s1) + s2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    norms[gi] = own;
    if (gi == 0) norms[3] = all;
  }
  const float sc = clip_scale(global_clip ? all : own, clip);
  float *x = G.x[gi], *g = G.g[gi], *m = G.m[gi], *v = G.v[gi];
  apply_quads<RULE, true>(n, x, g, m, v, aligned16(x, g, m, v), sc, G.step[gi], beta1, beta2, eps,
                          blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// ---- rau_update_ex: the same two passes with per-segment coefficients (kernels.h UpdSegs)
// The group's segments go to LDS once per workgroup, so the per-thread cursor below indexes LDS, not the by-value
// argument.  Returns the group's segment count; ends with a barrier.
__device__ __forceinline__ int load_segs(const UpdSegs& T, int gi, size_t* s_end, float* s_step, float* s_f,
                                         uint32_t* s_frozen) {
  const int base = T.first[gi], cnt = T.first[gi + 1] - base;
  if ((int)threadIdx.x < cnt) {
    const int i = base + (int)threadIdx.x;
    s_end[threadIdx.x] = T.end[i];
    if (s_step) s_step[threadIdx.x] = T.step[i];
    if (s_f) s_f[threadIdx.x] = T.f[i];
    s_frozen[threadIdx.x] = T.frozen[i];
  }
  __syncthreads();
  return cnt;
}
// The segments of elements e .. e+3.  A thread's quads rise, so `cur` (the segment of the thread's last quad's first
// element) only moves forward: amortised O(1).  An element at or behind the group's end gets the last segment.
__device__ __forceinline__ void quad_segs(const size_t* s_end, int cnt, size_t e, int& cur, int idx[4]) {
  while (cur + 1 < cnt && e >= s_end[cur]) ++cur;
  int c = cur;
  idx[0] = idx[1] = idx[2] = idx[3] = c;
  if (c + 1 >= cnt || e + 3 < s_end[c]) return;   // the common case: the quad lies in one segment
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    while (c + 1 < cnt && e + j >= s_end[c]) ++c;
    idx[j] = c;
  }
}

__global__ void __launch_bounds__(256) k_upd_ex_sqnorm(UpdGroups G, UpdSegs T, float nstd,
                                                       float* __restrict__ partial) {
  RAU_CHAIN_PRIO();
  __shared__ float s_sum[4];
  __shared__ size_t s_end[kUpdGroupSegs];
  __shared__ uint32_t s_frozen[kUpdGroupSegs];
  const int gi = blockIdx.y;
  const int cnt = load_segs(T, gi, s_end, nullptr, nullptr, s_frozen);
  const size_t n = G.n[gi];
  float* __restrict__ g = G.g[gi];
  const uint64_t seed = G.seed[gi];
  const bool vec = ((uintptr_t)g & 15) == 0;
  float acc = 0.f;
  int cur = 0;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q * 4 < n; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q * 4;
    int idx[4];
    quad_segs(s_end, cnt, e, cur, idx);
    const bool one = idx[3] == idx[0];   // one segment: one lookup
    const bool fr0 = s_frozen[idx[0]] != 0, fr1 = one ? fr0 : s_frozen[idx[1]] != 0,
               fr2 = one ? fr0 : s_frozen[idx[2]] != 0, fr3 = one ? fr0 : s_frozen[idx[3]] != 0;
    if (fr0 && fr1 && fr2 && fr3) continue;   // nothing drawn, nothing read
    float z[4];
    noise_quad(q, (uint32_t)gi, seed, nstd, z);
    if (vec && e + 4 <= n) {
      float4 v = *reinterpret_cast<const float4*>(g + e);
      if (!fr0) v.x = noise_elem(v.x, z[0], nstd, acc);
      if (!fr1) v.y = noise_elem(v.y, z[1], nstd, acc);
      if (!fr2) v.z = noise_elem(v.z, z[2], nstd, acc);
      if (!fr3) v.w = noise_elem(v.w, z[3], nstd, acc);
      *reinterpret_cast<float4*>(g + e) = v;   // a frozen element gets its own bits back
    } else {
      const bool fr[4] = {fr0, fr1, fr2, fr3};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n && !fr[j]) g[e + j] = noise_elem(g[e + j], z[j], nstd, acc);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[(size_t)gi * kUpdParts + blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

// one element: clip, decay, rule, average -- in that order
template <int RULE, bool EMA>
__device__ __forceinline__ void ex_elem(float& g, float& m, float& v, float& x, float& a, float sc, float stepsize,
                                        float f, float beta1, float beta2, float eps, float d, float omd) {
  g = g * sc;
  decay_elem(x, f);
  rule_elem<RULE>(g, m, v, x, stepsize, beta1, beta2, eps);
  if constexpr (EMA) ema_elem(a, x, d, omd);
}

template <int RULE, bool EMA>
__global__ void __launch_bounds__(256) k_upd_ex_apply(UpdGroups G, UpdSegs T, int global_clip, float clip,
                                                      float beta1, float beta2, float eps, float* ema0, float* ema1,
                                                      float* ema2, float d, float omd,
                                                      const float* __restrict__ partial, float* __restrict__ norms) {
  RAU_CHAIN_PRIO();
  const int gi = blockIdx.y;
  const size_t n = G.n[gi];
  // a workgroup whose first quad lies behind a short group has nothing to do (workgroup 0 writes the norm)
  if (blockIdx.x != 0 && (size_t)blockIdx.x * blockDim.x * 4 >= n) return;
  __shared__ float s_sum[3][4];
  __shared__ size_t s_end[kUpdGroupSegs];
  __shared__ float s_step[kUpdGroupSegs], s_f[kUpdGroupSegs];
  __shared__ uint32_t s_frozen[kUpdGroupSegs];
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // finish_norm's order, per group
    float acc = 0.f;
    for (int i = threadIdx.x; i < kUpdParts; i += 256) acc += partial[k * kUpdParts + i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_sum[k][threadIdx.x >> 6] = acc;
  }
  const int cnt = load_segs(T, gi, s_end, s_step, s_f, s_frozen);   // its barrier covers s_sum as well
  const float s0 = (s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]);
  const float s1 = (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]);
  const float s2 = (s_sum[2][0] + s_sum[2][1]) + (s_sum[2][2] + s_sum[2][3]);
  const float own = sqrtf(gi == 0 ? s0 : gi == 1 ? s1 : s2);
  const float all = sqrtf((s0 + s1) + s2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    norms[gi] = own;
    if (gi == 0) norms[3] = all;
  }
  const float sc = clip_scale(global_clip ? all : own, clip);
  float *x = G.x[gi], *g = G.g[gi], *m = G.m[gi], *v = G.v[gi];
  float* a = EMA ? (gi == 0 ? ema0 : gi == 1 ? ema1 : ema2) : nullptr;
  const bool vec = aligned16(x, g, m, v) && (!EMA || ((uintptr_t)a & 15) == 0);
  int cur = 0;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q * 4 < n; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q * 4;
    int idx[4];
    quad_segs(s_end, cnt, e, cur, idx);
    bool fr[4];
    float st[4], f[4];
    const bool one = idx[3] == idx[0];   // one segment: one lookup
    fr[0] = s_frozen[idx[0]] != 0;
    st[0] = s_step[idx[0]];
    f[0] = s_f[idx[0]];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      fr[j] = one ? fr[0] : s_frozen[idx[j]] != 0;
      st[j] = one ? st[0] : s_step[idx[j]];
      f[j] = one ? f[0] : s_f[idx[j]];
    }
    if (fr[0] && fr[1] && fr[2] && fr[3]) continue;   // nothing read, nothing written
    if (vec && e + 4 <= n) {
      float4 g4 = *reinterpret_cast<const float4*>(g + e);
      float4 m4 = *reinterpret_cast<const float4*>(m + e);
      float4 v4 = *reinterpret_cast<const float4*>(v + e);
      float4 x4 = *reinterpret_cast<const float4*>(x + e);
      float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (EMA) a4 = *reinterpret_cast<const float4*>(a + e);
      if (!fr[0]) ex_elem<RULE, EMA>(g4.x, m4.x, v4.x, x4.x, a4.x, sc, st[0], f[0], beta1, beta2, eps, d, omd);
      if (!fr[1]) ex_elem<RULE, EMA>(g4.y, m4.y, v4.y, x4.y, a4.y, sc, st[1], f[1], beta1, beta2, eps, d, omd);
      if (!fr[2]) ex_elem<RULE, EMA>(g4.z, m4.z, v4.z, x4.z, a4.z, sc, st[2], f[2], beta1, beta2, eps, d, omd);
      if (!fr[3]) ex_elem<RULE, EMA>(g4.w, m4.w, v4.w, x4.w, a4.w, sc, st[3], f[3], beta1, beta2, eps, d, omd);
      *reinterpret_cast<float4*>(g + e) = g4;   // a frozen element gets its own bits back, in all five
      *reinterpret_cast<float4*>(m + e) = m4;
      *reinterpret_cast<float4*>(v + e) = v4;
      *reinterpret_cast<float4*>(x + e) = x4;
      if constexpr (EMA) *reinterpret_cast<float4*>(a + e) = a4;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n && !fr[j]) {
          float gj = g[e + j], mj = m[e + j], vj = v[e + j], xj = x[e + j], aj = 0.f;
          if constexpr (EMA) aj = a[e + j];
          ex_elem<RULE, EMA>(gj, mj, vj, xj, aj, sc, st[j], f[j], beta1, beta2, eps, d, omd);
          g[e + j] = gj;
          m[e + j] = mj;
          v[e + j] = vj;
          x[e + j] = xj;
          if constexpr (EMA) a[e + j] = aj;
        }
    }
  }
}

// x <-> e of group blockIdx.y: float4 where both pointers allow, the n % 4 tail (or everything) scalar
__global__ void __launch_bounds__(256) k_ema_swap(float* x0, float* x1, float* x2, float* e0, float* e1, float* e2,
                                                  size_t n0, size_t n1, size_t n2) {
  const int gi = blockIdx.y;
  float* __restrict__ x = gi == 0 ? x0 : gi == 1 ? x1 : x2;
  float* __restrict__ a = gi == 0 ? e0 : gi == 1 ? e1 : e2;
  const size_t n = gi == 0 ? n0 : gi == 1 ? n1 : n2;
  const bool vec = (((uintptr_t)x | (uintptr_t)a) & 15) == 0;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q * 4 < n; q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q * 4;
    if (vec && e + 4 <= n) {
      const float4 xv = *reinterpret_cast<const float4*>(x + e);
      const float4 av = *reinterpret_cast<const float4*>(a + e);
      *reinterpret_cast<float4*>(x + e) = av;
      *reinterpret_cast<float4*>(a + e) = xv;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) {
          const float t = x[e + j];
          x[e + j] = a[e + j];
          a[e + j] = t;
        }
    }
  }
}

__global__ void __launch_bounds__(256) k_adamax_vec(size_t n, float* __restrict__ x, const float* __restrict__ dx,
                                                    float* __restrict__ m, float* __restrict__ u, float stepsize,
                                                    float beta1, float beta2, float eps) {
  apply_quads<RAU_OPT_ADAMAX, false>(n, x, dx, m, u, aligned16(x, dx, m, u), 1.f, stepsize, beta1, beta2, eps,
                                     blockIdx.x * (size_t)blockDim.x + threadIdx.x,
                                     (size_t)gridDim.x * blockDim.x);
}

// workgroups of 256 threads, a quad per thread and round, capped
inline int quad_blocks(size_t n, int cap) {
  const size_t q = (n + 3) / 4, b = (q + 255) / 256;
  return (int)std::min<size_t>(std::max<size_t>(b, 1), (size_t)cap);
}

}  // namespace

hipError_t upd_noise_sqnorm(hipStream_t st, const UpdGroups& G, float nstd, float* partial) {
  hipLaunchKernelGGL(k_upd_noise_sqnorm, dim3(kUpdParts, 3), dim3(256), 0, st, G, nstd, partial);
  return hipGetLastError();
}
hipError_t upd_apply(hipStream_t st, const UpdGroups& G, int rule, bool global_clip, float clip, float beta1,
                     float beta2, float eps, const float* partial, float* norms) {
  const dim3 grid(quad_blocks(std::max(G.n[0], std::max(G.n[1], G.n[2])), kUpdParts), 3);
  if (rule == RAU_OPT_ADAM)
    hipLaunchKernelGGL(k_upd_apply<RAU_OPT_ADAM>, grid, dim3(256), 0, st, G, global_clip ? 1 : 0, clip, beta1, beta2,
                       eps, partial, norms);
  else
    hipLaunchKernelGGL(k_upd_apply<RAU_OPT_ADAMAX>, grid, dim3(256), 0, st, G, global_clip ? 1 : 0, clip, beta1,
                       beta2, eps, partial, norms);
  return hipGetLastError();
}
hipError_t upd_ex_sqnorm(hipStream_t st, const UpdGroups& G, const UpdSegs& T, float nstd, float* partial) {
  hipLaunchKernelGGL(k_upd_ex_sqnorm, dim3(kUpdParts, 3), dim3(256), 0, st, G, T, nstd, partial);
  return hipGetLastError();
}
template <int RULE>
static void launch_ex_apply(hipStream_t st, dim3 grid, const UpdGroups& G, const UpdSegs& T, int global_clip,
                            float clip, float beta1, float beta2, float eps, float* const ema[3], float d, float omd,
                            const float* partial, float* norms) {
  if (ema)
    hipLaunchKernelGGL((k_upd_ex_apply<RULE, true>), grid, dim3(256), 0, st, G, T, global_clip, clip, beta1, beta2,
                       eps, ema[0], ema[1], ema[2], d, omd, partial, norms);
  else
    hipLaunchKernelGGL((k_upd_ex_apply<RULE, false>), grid, dim3(256), 0, st, G, T, global_clip, clip, beta1, beta2,
                       eps, (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.f, 1.f, partial, norms);
}
hipError_t upd_ex_apply(hipStream_t st, const UpdGroups& G, const UpdSegs& T, int rule, bool global_clip, float clip,
                        float beta1, float beta2, float eps, float* const ema[3], float d, float omd,
                        const float* partial, float* norms) {
  const dim3 grid(quad_blocks(std::max(G.n[0], std::max(G.n[1], G.n[2])), kUpdParts), 3);
  if (rule == RAU_OPT_ADAM)
    launch_ex_apply<RAU_OPT_ADAM>(st, grid, G, T, global_clip ? 1 : 0, clip, beta1, beta2, eps, ema, d, omd, partial,
                                  norms);
  else
    launch_ex_apply<RAU_OPT_ADAMAX>(st, grid, G, T, global_clip ? 1 : 0, clip, beta1, beta2, eps, ema, d, omd, partial,
                                    norms);
  return hipGetLastError();
}
hipError_t ema_swap(hipStream_t st, float* const x[3], float* const e[3], const size_t n[3]) {
  const dim3 grid(quad_blocks(std::max(n[0], std::max(n[1], n[2])), 2048), 3);
  hipLaunchKernelGGL(k_ema_swap, grid, dim3(256), 0, st, x[0], x[1], x[2], e[0], e[1], e[2], n[0], n[1], n[2]);
  return hipGetLastError();
}
hipError_t adamax_vec(hipStream_t st, size_t n, float* x, const float* dx, float* m, float* u, float stepsize,
                      float beta1, float beta2, float eps) {
  hipLaunchKernelGGL(k_adamax_vec, dim3(quad_blocks(n, 2048)), dim3(256), 0, st, n, x, dx, m, u, stepsize, beta1,
                     beta2, eps);
  return hipGetLastError();
}

}  // namespace rau

namespace {
bool known_rule(int r) { return r == RAU_OPT_ADAM || r == RAU_OPT_ADAMAX; }
// both moments of a group exist (zero-filled when new)
int need_moments(rau_ctx* ctx, Group& g) {
  if (g.m) return RAU_OK;
  float *m = nullptr, *v = nullptr;
  if (int rc = dalloc(ctx, &m, g.n, false)) return rc;
  if (int rc = dalloc(ctx, &v, g.n, false)) return rc;
  g.m = m;
  g.v = v;
  return RAU_OK;
}
// What rau_update and rau_update_ex refuse before anything is allocated or launched
int update_args(rau_ctx* ctx, int64_t step_t, const rau_update_opts* o) {
  NEED(ctx && o, "null argument");
  NEED(known_rule(o->rule), "rau_update: unknown rule %d", o->rule);
  NEED(o->clip_scope == RAU_CLIP_GROUP || o->clip_scope == RAU_CLIP_GLOBAL, "rau_update: unknown clip scope %d",
       o->clip_scope);
  NEED(step_t >= 0 && o->gamma > 0.f && o->eta >= 0.f && o->clip > 0.f, "bad update hyper-parameters");
  if (ctx->ema_swapped)
    return fail(RAU_ERR_STATE, "rau_update: the weights are swapped with their average (rau_ema_swap); swap back first");
  for (int gi = 0; gi < 3; ++gi)
    if (ctx->grp[gi].adam_t > 0 && ctx->grp[gi].opt_rule != o->rule)
      return fail(RAU_ERR_STATE, "rau_update: group %d holds the other rule's state (t = %lld); reset it with "
                  "rau_set_opt_state first", gi, (long long)ctx->grp[gi].adam_t);
  return RAU_OK;
}
bool finite_nonneg(float v) { return std::isfinite(v) && v >= 0.f; }
int units_of(const Group& g) { return ((int)g.layout.size() + 1) / 2; }
LayerOpt unit_opt(const Group& g, int u) { return g.lopt.empty() ? LayerOpt{} : g.lopt[u]; }
// all three groups' averages exist; new ones start as the current weights
int need_ema(rau_ctx* ctx) {
  if (ctx->grp[0].ema) return RAU_OK;
  float* e[3] = {nullptr, nullptr, nullptr};
  for (int gi = 0; gi < 3; ++gi)
    if (int rc = dalloc(ctx, &e[gi], ctx->grp[gi].n, false)) {
      for (int k = 0; k < gi; ++k) dfree(ctx, e[k]);
      return rc;
    }
  for (int gi = 0; gi < 3; ++gi) {
    HIPC(hipMemcpyAsync(e[gi], ctx->grp[gi].w, ctx->grp[gi].n * sizeof(float), hipMemcpyDeviceToDevice, ctx->st));
    ctx->grp[gi].ema = e[gi];
  }
  return RAU_OK;
}
}  // namespace

extern "C" {

void rau_update_opts_default(rau_update_opts* o) {
  if (!o) return;
  o->rule = RAU_OPT_ADAM;
  o->clip_scope = RAU_CLIP_GROUP;
  o->lr = 3e-3f;
  o->mult_lr = 3e-4f;
  o->beta1 = 0.9f;
  o->beta2 = 0.999f;
  o->eps = 1e-8f;
  o->eta = 0.01f;
  o->gamma = 0.55f;
  o->clip = 0.1f;
  o->noise_seed = 0;
}

int rau_update(rau_ctx* ctx, int64_t step_t, const rau_update_opts* o, float* out_norms) {
  if (int rc = update_args(ctx, step_t, o)) return rc;
  if (int rc = update_guard(ctx, false, out_norms, 4)) return rc < 0 ? rc : RAU_OK;   // rau_set_update_guard
  for (int gi = 0; gi < 3; ++gi)
    if (int rc = need_moments(ctx, ctx->grp[gi])) return rc;
  // SS:598-599: var = eta / ((step_t+1) * gamma)
  const float nstd = o->eta > 0.f ? std::sqrt(o->eta / ((float)(step_t + 1) * o->gamma)) : 0.f;
  UpdGroups G;
  double elems = 0;
  for (int gi = 0; gi < 3; ++gi) {
    const Group& g = ctx->grp[gi];
    G.x[gi] = g.w;
    G.g[gi] = g.g;
    G.m[gi] = g.m;
    G.v[gi] = g.v;
    G.n[gi] = g.n;
    G.seed[gi] = o->noise_seed + (uint64_t)step_t * 3 + gi;
    const int64_t t = g.adam_t + 1;
    const double bc1 = 1.0 - std::pow((double)o->beta1, (double)t);
    const double bc2 = 1.0 - std::pow((double)o->beta2, (double)t);
    const float group_lr = gi == RAU_GROUP_MULT ? o->mult_lr : o->lr;  // SS:770-772
    G.step[gi] = o->rule == RAU_OPT_ADAM ? (float)(group_lr * std::sqrt(bc2) / bc1) : (float)(group_lr / bc1);
    elems += (double)g.n;
  }
  RUN("upd_noise_sqnorm", 0, elems * 8.0, upd_noise_sqnorm(ctx->st, G, nstd, ctx->upd_part));
  RUN("upd_apply", 0, elems * 28.0,
      upd_apply(ctx->st, G, o->rule, o->clip_scope == RAU_CLIP_GLOBAL, o->clip, o->beta1, o->beta2, o->eps,
                ctx->upd_part, ctx->norms_d));
  for (int gi = 0; gi < 3; ++gi) {
    ctx->grp[gi].adam_t += 1;
    ctx->grp[gi].opt_rule = o->rule;
  }
  if (out_norms) return d2h(ctx, out_norms, ctx->norms_d, 4 * sizeof(float));
  return RAU_OK;
}

// ---- rau_update_ex: decoupled decay, per-layer step sizes, the weight average (include/rau.h)
void rau_update_extras_default(rau_update_extras* e) {
  if (!e) return;
  e->weight_decay = 0.f;
  e->ema_decay = 0.f;
}

int rau_update_ex(rau_ctx* ctx, int64_t step_t, const rau_update_opts* o, const rau_update_extras* e,
                  float* out_norms) {
  if (int rc = update_args(ctx, step_t, o)) return rc;
  const float wd = e ? e->weight_decay : 0.f, d = e ? e->ema_decay : 0.f;
  NEED(finite_nonneg(wd), "rau_update_ex: weight_decay %g is not >= 0", (double)wd);
  NEED(d >= 0.f && d < 1.f, "rau_update_ex: ema_decay %g is not in [0, 1)", (double)d);
  if (d > 0.f && !ctx->grp[0].ema)
    return fail(RAU_ERR_STATE, "rau_update_ex: ema_decay > 0 without an average; start one with rau_ema_reset or "
                "rau_set_ema");
  int segs = 0;
  for (int gi = 0; gi < 3; ++gi) {
    NEED((int)ctx->grp[gi].layout.size() <= kUpdGroupSegs, "rau_update_ex: group %d has too many segments", gi);
    segs += (int)ctx->grp[gi].layout.size();
  }
  NEED(segs <= kUpdSegs, "rau_update_ex: too many segments");
  if (int rc = update_guard(ctx, true, out_norms, 4)) return rc < 0 ? rc : RAU_OK;   // rau_set_update_guard
  for (int gi = 0; gi < 3; ++gi)
    if (int rc = need_moments(ctx, ctx->grp[gi])) return rc;
  const float nstd = o->eta > 0.f ? std::sqrt(o->eta / ((float)(step_t + 1) * o->gamma)) : 0.f;
  UpdGroups G;
  UpdSegs T;
  std::memset(&T, 0, sizeof(T));
  double elems = 0;
  int si = 0;
  for (int gi = 0; gi < 3; ++gi) {
    const Group& g = ctx->grp[gi];
    G.x[gi] = g.w;
    G.g[gi] = g.g;
    G.m[gi] = g.m;
    G.v[gi] = g.v;
    G.n[gi] = g.n;
    G.seed[gi] = o->noise_seed + (uint64_t)step_t * 3 + gi;
    const int64_t t = g.adam_t + 1;
    const double bc1 = 1.0 - std::pow((double)o->beta1, (double)t);
    const double bc2 = 1.0 - std::pow((double)o->beta2, (double)t);
    const float group_lr = gi == RAU_GROUP_MULT ? o->mult_lr : o->lr;  // SS:770-772
    G.step[gi] = 0.f;   // not read: the segments carry the step sizes
    T.first[gi] = si;
    for (size_t li = 0; li < g.layout.size(); ++li, ++si) {   // entry 2u is unit u's weight, 2u + 1 its bias
      const LayerOpt lo = unit_opt(g, (int)li / 2);
      const bool bias = (li & 1) != 0;
      T.end[si] = li + 1 < g.layout.size() ? g.layout[li + 1].off : g.n;
      T.step[si] = o->rule == RAU_OPT_ADAM ? (float)(group_lr * (double)lo.lr_scale * std::sqrt(bc2) / bc1)
                                           : (float)(group_lr * (double)lo.lr_scale / bc1);
      T.f[si] = (float)(1.0 - (double)group_lr * (double)lo.lr_scale * (double)wd *
                                  (double)(bias ? lo.decay_b : lo.decay_w));
      T.frozen[si] = lo.lr_scale == 0.f ? 1u : 0u;
    }
    elems += (double)g.n;
  }
  T.first[3] = si;
  float* ema[3] = {ctx->grp[0].ema, ctx->grp[1].ema, ctx->grp[2].ema};
  RUN("upd_ex_sqnorm", 0, elems * 8.0, upd_ex_sqnorm(ctx->st, G, T, nstd, ctx->upd_part));
  RUN("upd_ex_apply", 0, elems * (d > 0.f ? 36.0 : 28.0),
      upd_ex_apply(ctx->st, G, T, o->rule, o->clip_scope == RAU_CLIP_GLOBAL, o->clip, o->beta1, o->beta2, o->eps,
                   d > 0.f ? ema : nullptr, d, 1.f - d, ctx->upd_part, ctx->norms_d));
  for (int gi = 0; gi < 3; ++gi) {
    ctx->grp[gi].adam_t += 1;
    ctx->grp[gi].opt_rule = o->rule;
  }
  if (out_norms) return d2h(ctx, out_norms, ctx->norms_d, 4 * sizeof(float));
  return RAU_OK;
}

int rau_set_layer_opts(rau_ctx* ctx, int group, int index, float lr_scale, float decay_weight, float decay_bias) {
  NEED(ctx, "null ctx");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  Group& g = ctx->grp[group];
  NEED(index >= 0 && index < units_of(g), "rau_set_layer_opts: group %d has no layer %d", group, index);
  NEED(finite_nonneg(lr_scale) && finite_nonneg(decay_weight) && finite_nonneg(decay_bias),
       "rau_set_layer_opts: lr_scale %g, decay_weight %g, decay_bias %g must be finite and >= 0", (double)lr_scale,
       (double)decay_weight, (double)decay_bias);
  if (g.lopt.empty()) g.lopt.resize(units_of(g));
  g.lopt[index] = LayerOpt{lr_scale, decay_weight, decay_bias};
  return RAU_OK;
}

int rau_get_layer_opts(rau_ctx* ctx, int group, int index, float* lr_scale, float* decay_weight, float* decay_bias) {
  NEED(ctx, "null ctx");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  const Group& g = ctx->grp[group];
  NEED(index >= 0 && index < units_of(g), "rau_get_layer_opts: group %d has no layer %d", group, index);
  const LayerOpt lo = unit_opt(g, index);
  if (lr_scale) *lr_scale = lo.lr_scale;
  if (decay_weight) *decay_weight = lo.decay_w;
  if (decay_bias) *decay_bias = lo.decay_b;
  return RAU_OK;
}

int rau_ema_reset(rau_ctx* ctx) {
  NEED(ctx, "null ctx");
  if (ctx->ema_swapped) return fail(RAU_ERR_STATE, "rau_ema_reset: weights and average are swapped; swap back first");
  if (!ctx->grp[0].ema) return need_ema(ctx);
  for (int gi = 0; gi < 3; ++gi)
    HIPC(hipMemcpyAsync(ctx->grp[gi].ema, ctx->grp[gi].w, ctx->grp[gi].n * sizeof(float), hipMemcpyDeviceToDevice,
                        ctx->st));
  return RAU_OK;
}

int rau_ema_swap(rau_ctx* ctx) {
  NEED(ctx, "null ctx");
  if (!ctx->grp[0].ema) return fail(RAU_ERR_STATE, "rau_ema_swap: no average (rau_ema_reset / rau_set_ema)");
  float* x[3] = {ctx->grp[0].w, ctx->grp[1].w, ctx->grp[2].w};
  float* a[3] = {ctx->grp[0].ema, ctx->grp[1].ema, ctx->grp[2].ema};
  const size_t n[3] = {ctx->grp[0].n, ctx->grp[1].n, ctx->grp[2].n};
  RUN("ema_swap", 0, ((double)n[0] + (double)n[1] + (double)n[2]) * 16.0, ema_swap(ctx->st, x, a, n));
  ctx->ema_swapped = !ctx->ema_swapped;
  return RAU_OK;
}

int rau_ema_state(rau_ctx* ctx, int* has, int* swapped) {
  NEED(ctx, "null ctx");
  if (has) *has = ctx->grp[0].ema ? 1 : 0;
  if (swapped) *swapped = ctx->ema_swapped ? 1 : 0;
  return RAU_OK;
}

int rau_get_ema(rau_ctx* ctx, int group, float* host, size_t n) {
  NEED(ctx && host, "null argument");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  const Group& g = ctx->grp[group];
  NEED(n == g.n, "group %d has %zu floats, caller passed %zu", group, g.n, n);
  if (!g.ema) return fail(RAU_ERR_STATE, "rau_get_ema: no average (rau_ema_reset / rau_set_ema)");
  return d2h(ctx, host, g.ema, n * sizeof(float));
}

int rau_set_ema(rau_ctx* ctx, int group, const float* host, size_t n) {
  NEED(ctx && host, "null argument");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  NEED(n == ctx->grp[group].n, "group %d has %zu floats, caller passed %zu", group, ctx->grp[group].n, n);
  if (ctx->ema_swapped) return fail(RAU_ERR_STATE, "rau_set_ema: weights and average are swapped; swap back first");
  if (int rc = need_ema(ctx)) return rc;
  HIPC(hipMemcpyAsync(ctx->grp[group].ema, host, n * sizeof(float), hipMemcpyHostToDevice, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return RAU_OK;
}

int rau_get_opt_state(rau_ctx* ctx, int group, float* m, float* v, int64_t* t, int32_t* rule) {
  NEED(ctx, "null ctx");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  const Group& g = ctx->grp[group];
  float* host[2] = {m, v};
  const float* dev[2] = {g.m, g.v};
  for (int k = 0; k < 2; ++k) {
    if (!host[k]) continue;
    if (dev[k]) HIPC(hipMemcpyAsync(host[k], dev[k], g.n * sizeof(float), hipMemcpyDeviceToHost, ctx->st));
    else std::memset(host[k], 0, g.n * sizeof(float));   // before the first update: zeros, nothing allocated
  }
  HIPC(hipStreamSynchronize(ctx->st));
  if (t) *t = g.adam_t;
  if (rule) *rule = g.opt_rule;
  return RAU_OK;
}

int rau_set_opt_state(rau_ctx* ctx, int group, const float* m, const float* v, int64_t t, int32_t rule) {
  NEED(ctx, "null ctx");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  NEED(known_rule(rule), "rau_set_opt_state: unknown rule %d", rule);
  NEED(t >= 0, "rau_set_opt_state: t = %lld", (long long)t);
  NEED(t == 0 || (m && v), "rau_set_opt_state: t = %lld needs both moment vectors", (long long)t);
  Group& g = ctx->grp[group];
  if (m || v)
    if (int rc = need_moments(ctx, g)) return rc;
  const float* host[2] = {m, v};
  float* dev[2] = {g.m, g.v};
  for (int k = 0; k < 2 && g.m; ++k) {
    if (host[k]) HIPC(hipMemcpyAsync(dev[k], host[k], g.n * sizeof(float), hipMemcpyHostToDevice, ctx->st));
    else HIPC(hipMemsetAsync(dev[k], 0, g.n * sizeof(float), ctx->st));
  }
  HIPC(hipStreamSynchronize(ctx->st));
  g.adam_t = t;
  g.opt_rule = rule;
  return RAU_OK;
}

}  // extern "C"

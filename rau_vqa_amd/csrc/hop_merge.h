// hop_merge.h -- the rows predict_result and feval read out of the resident hop outputs, for the
// kernels that consume them (hop_merge.hip: statistics, first-max answers; topk.hip: ranked answers; cand_rank.hip:
// ranked candidates and MC statistics), and the
// arithmetic of the per-answer sigmoid criterion (bce_head.hip: the step's head; hop_merge.hip: its statistics).
// One definition of the merge arithmetic, so that every consumer sees the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace rau {

constexpr int kMT = 256;   // threads per sample: 4 waves

// workgroup sum in k_ce_fwd's order: wave_sum, then (w0 + w1) + (w2 + w3)
__device__ __forceinline__ float block_sum(float v, float* s_sum) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  v = wave_sum(v);
  if (l == 0) s_sum[w] = v;
  __syncthreads();
  const float r = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
  __syncthreads();
  return r;
}

// torch.max's first-max over the workgroup (k_ce_fwd's rule): the largest value, lowest index on ties
__device__ __forceinline__ void block_first_max(float& mx, int& ai, float* s_val, int* s_idx) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(ai, o, 64);
    if (ov > mx || (ov == mx && oi < ai)) { mx = ov; ai = oi; }
  }
  if (l == 0) { s_val[w] = mx; s_idx[w] = ai; }
  __syncthreads();
  mx = s_val[0]; ai = s_idx[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (s_val[i] > mx || (s_val[i] == mx && s_idx[i] < ai)) { mx = s_val[i]; ai = s_idx[i]; }
  __syncthreads();   // the slots are reused by the next reduction
}

// Entry k of row r of one sample (lg = its logits row of hop 0, hop stride hs):
//   r < H    hop r's logits;
//   r == H   uni, SS:482 + 522: uni_pred:zero(), :add(l_h) for h = 1..H, :div(nHop) -- sequential
//            adds from +0, then a true division;
//   r == H+1 select, SS:505-507: select_pred:zero():add(l_h * cur_h); at most one cur_h is 1, the
//            others add +-0, so the row is 0 + l_hsel (all +0 when no hop fired, hsel < 0).
__device__ __forceinline__ float row_val(const float* __restrict__ lg, size_t hs, int H, int r, int hsel,
                                         int k) {
  if (r < H) return lg[(size_t)r * hs + k];
  if (r == H) {
    float s = 0.f;
    for (int h = 0; h < H; ++h) s += lg[(size_t)h * hs + k];
    return __fdiv_rn(s, (float)H);
  }
  return hsel >= 0 ? 0.f + lg[(size_t)hsel * hs + k] : 0.f;
}

// First hop whose do_pred fires (do_pred > 0.5, SS:501): the clamp(do - did) / clamp(did + do)
// recurrence of SS:505, 515 selects exactly that one.  force_last: predict_result's rule (SS:685).
__device__ __forceinline__ int select_hop(const float* __restrict__ dopred, int H, int B, int b,
                                          bool force_last) {
  for (int h = 0; h < H; ++h)
    if (dopred[(size_t)h * B + b] > 0.5f || (force_last && h == H - 1)) return h;
  return -1;
}

// The per-answer sigmoid criterion (RAU_LOSS_BCE; bce_head.hip spells out the rounding), shared by the step's head
// and the statistics of the merged rows.  The set in LDS: ng entries, s_id 0-based (-1 = empty), s_w its weight.
// bce_target: t[k] = min(1, the matching entries' weights added from +0 in entry order).
__device__ __forceinline__ float bce_target(const int* s_id, const float* s_w, int ng, int k) {
  float t = 0.f;
  for (int g = 0; g < ng; ++g)
    if (s_id[g] == k) t = __fadd_rn(t, s_w[g]);
  return fminf(t, 1.f);
}
// bce_term: (max(x,0) - x t) + log1p(e), e = expf(-|x|); every step rounded once, no fused multiply-add
__device__ __forceinline__ float bce_term(float x, float t, float e) {
  return __fadd_rn(__fsub_rn(fmaxf(x, 0.f), __fmul_rn(x, t)), log1pf(e));
}
// a row is labelled when its set has a non-empty entry
__device__ __forceinline__ bool bce_labelled(const int* s_id, int ng) {
  bool any = false;
  for (int g = 0; g < ng; ++g) any = any || s_id[g] >= 0;
  return any;
}

// The TOTAL order of include/rau.h (rau_dev_topk) as a 64-bit key: the high word is the monotone unsigned image of
// the float (-0 canonicalised to +0, NaN below -inf), the low word is 0xffffffff - index.  A larger key ranks first:
// larger value, equal values by the lower index, NaN last by index.  Shared by topk.hip and cand_rank.hip.
__device__ __forceinline__ uint32_t order_bits(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;   // NaN: after everything, -inf (0x007fffff) included
  if (u == 0x80000000u) u = 0u;                     // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t make_key(float v, int c) {
  return ((uint64_t)order_bits(v) << 32) | (uint64_t)(0xffffffffu - (uint32_t)c);
}

}  // namespace rau

// ce_set.hip -- the classifier loss head against an ANSWER SET (rau_set_answers): k_ce_fwd's contract (one
// 256-thread workgroup per (hop, sample) row; finishing of K-split partials plus bias; first-max argmax; lse;
// do_pred; chain priority) with a soft target in place of the one label.  A row's set is G entries (ids 1..K,
// 0 = empty; weights w >= 0).  With W = sum of the non-empty weights in entry order:
//   lossrow = sum_g w_g (lse - lg[y_g])                       accumulated from 0 in entry order
//   dl[k]   = (expf(lg[k] - mx) / den) (W invB), then for g = 0..G-1 in order: if (y_g == k) dl[k] -= w_g invB
// With a sample weight s_b (rau_set_sample_weights) invB is __fmul_rn(s_b, 1 / Bper) in both products and the loss
// row written is __fmul_rn(s_b, lossrow); without weights s_b = 1 and both are exact.  One load per workgroup.
// The rounding of every step is spelled out, so duplicates are deterministic: the products w_g invB, W invB and
// w_g (lse - lg[y_g]) and every sum are rounded once, and the FIRST matching entry of a logit is subtracted inside
// the product's fused multiply-add, fma(e, W invB, -w_g invB) -- which is what k_ce_fwd's
// `p = e * invB; if (k == y) p -= invB;` compiles to.  So G = 1, w = 1 gives k_ce_fwd's bits: W invB = invB,
// 0 + 1 (lse - lg[y]) = lse - lg[y].
// The set sits in LDS once per workgroup: at most 16 compares per logit, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include "common.h"
#include "hop_merge.h"   // block_sum, block_first_max: k_ce_fwd's reduction orders
#include "kernels.h"

namespace rau {
namespace {

__global__ __launch_bounds__(256) void k_ce_set_fwd(int nB, int K, int M, const float* __restrict__ logits,
    const int32_t* __restrict__ ids, const float* __restrict__ w, int G, const float* __restrict__ mf,
    const float* __restrict__ wd, const float* __restrict__ bd, float* __restrict__ dl,
    float* __restrict__ lossrow, int32_t* __restrict__ argmax, float* __restrict__ dopred,
    const float* __restrict__ part, int nsplit, const float* __restrict__ bias, float* __restrict__ logits_out,
    int Bper, int ld, const float* __restrict__ sw) {
  RAU_CHAIN_PRIO();
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ float s_sum[4];
  __shared__ int s_id[kMaxAnswers];      // 0-based answer, -1 = empty entry
  __shared__ float s_w[kMaxAnswers];     // its weight (0 for an empty entry)
  __shared__ float s_wb[kMaxAnswers];    // w * invB
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float sb = sw ? sw[b % Bper] : 1.f;
  const float invB = __fmul_rn(sb, 1.f / (float)Bper);
  if (tid < G) {
    // rows = [hop][sample]: the sets repeat every Bper rows; ids clamped like k_ce_fwd's labels
    const size_t e = (size_t)(b % Bper) * G + tid;
    const int id = min(max(ids[e], 0), K);
    const float wv = id > 0 ? w[e] : 0.f;
    s_id[tid] = id - 1;
    s_w[tid] = wv;
    s_wb[tid] = __fmul_rn(wv, invB);
  }
  if (nsplit) {  // logits arrive as K-split partials [split][nB][K] of mf Wc^T: finish them here
    for (int k = tid; k < K; k += 256) {
      float v = bias[k];
      for (int sp = 0; sp < nsplit; ++sp) v += part[((size_t)sp * nB + b) * K + k];
      logits_out[(size_t)b * ld + k] = v;
    }
    for (int k = K + tid; k < ld; k += 256) logits_out[(size_t)b * ld + k] = 0.f;   // the row's pad
    logits = logits_out;
  }
  __syncthreads();   // the set, and the finished logits thread 0 reads below
  const float* lg = logits + (size_t)b * ld;
  float mx = -INFINITY;
  int ai = 0x7fffffff;
  for (int k = tid; k < K; k += 256) {
    const float v = lg[k];
    if (v > mx) { mx = v; ai = k; }
  }
  block_first_max(mx, ai, s_val, s_idx);
  float den = 0.f;
  for (int k = tid; k < K; k += 256) den += expf(lg[k] - mx);
  den = block_sum(den, s_sum);
  const float lse = mx + logf(den);
  if (tid == 0) argmax[b] = ai + 1;
  float W = 0.f;
  for (int g = 0; g < G; ++g) W = __fadd_rn(W, s_w[g]);
  const float scale = __fmul_rn(W, invB);
  for (int k = tid; k < K; k += 256) {
    const float e = expf(lg[k] - mx) / den;
    float p = __fmul_rn(e, scale);
    bool hit = false;
    for (int g = 0; g < G; ++g)
      if (s_id[g] == k) {
        p = hit ? __fsub_rn(p, s_wb[g]) : __fmaf_rn(e, scale, -s_wb[g]);
        hit = true;
      }
    dl[(size_t)b * ld + k] = p;
  }
  for (int k = K + tid; k < ld; k += 256) dl[(size_t)b * ld + k] = 0.f;   // the row's pad
  if (tid == 0) {
    float acc = 0.f;
    for (int g = 0; g < G; ++g)
      if (s_id[g] >= 0) acc = __fadd_rn(acc, __fmul_rn(s_w[g], lse - lg[s_id[g]]));
    lossrow[b] = __fmul_rn(sb, acc);
  }
  // do_pred
  if (!mf) return;   // criterion-only use (uniform per launch)
  float acc = 0.f;
  for (int m = tid; m < M; m += 256) acc += mf[(size_t)b * M + m] * wd[m];
  acc = block_sum(acc, s_sum);
  if (tid == 0) dopred[b] = sigmoidf_(acc + bd[0]);
}

}  // namespace

hipError_t ce_set_fwd(hipStream_t st, int nB, int K, int M, const float* logits, const int32_t* ids,
                      const float* w, int G, const float* mf, const float* wd, const float* bd, float* dl,
                      float* lossrow, int32_t* argmax, float* dopred, const float* part, int nsplit,
                      const float* bias, float* logits_out, int Bper, int ld, const float* sw) {
  if (G < 1 || G > kMaxAnswers || !ids || !w) return hipErrorInvalidValue;
  if (!split_span_ok(part, nsplit, (size_t)nB * K)) return kSplitStateError;
  if (ld != 0 && ld < K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ce_set_fwd, dim3(nB), dim3(256), 0, st, nB, K, M, logits, ids, w, G, mf, wd, bd, dl,
                     lossrow, argmax, dopred, part, nsplit, bias, logits_out, Bper > 0 ? Bper : nB, ld ? ld : K,
                     sw);
  return hipGetLastError();
}

}  // namespace rau

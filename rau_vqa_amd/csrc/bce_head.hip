// bce_head.hip -- the classifier loss head as a PER-ANSWER SIGMOID with binary cross-entropy against soft targets
// (rau_set_answer_loss, RAU_LOSS_BCE): k_ce_fwd's / k_ce_set_fwd's launch contract (one 256-thread workgroup per
// (hop, sample) row; finishing of K-split partials plus bias; first-max argmax; do_pred; chain priority; no loss
// and no dl without a ground truth; no do_pred without mf) with another criterion.  With x the row's logits and
// invB = 1 / Bper:
//   target   labels:      t[k] = [k == y]                                   (y clamped like k_ce_fwd's label)
//            answer set:  t[k] = min(1, sum_g w_g [y_g == k])               (ids clamped like k_ce_set_fwd's)
//   lossrow  = sum_k ( max(x,0) - x t + log1p(exp(-|x|)) )                  summed over K, NOT divided by K
//   dl[k]    = (sigmoid(x) - t) invB
// With a sample weight s_b (rau_set_sample_weights) invB is __fmul_rn(s_b, 1 / Bper) and the loss row written is
// __fmul_rn(s_b, lossrow); without weights s_b = 1 and both are exact.  One 4-byte load per workgroup.
// The rounding of every step is spelled out, so duplicates are deterministic and repeated calls give the same bits:
//   t        the matching non-empty entries' weights are added from +0 in entry order, each sum rounded once
//            (__fadd_rn), then fminf(., 1); labels are the set {(y, 1)}, so t is exactly 0 or 1
//   e        = expf(-|x|)                          in (0, 1] for every finite x: nothing overflows
//   term     = (fmaxf(x,0) - x t) + log1pf(e)      the product, the difference and the sum each rounded once
//            (__fmul_rn, __fsub_rn, __fadd_rn: no fused multiply-add); every term is >= 0
//   lossrow  thread tid adds the terms of k = tid, tid + 256, .. in ascending k from +0 (__fadd_rn), the 256
//            partials go through block_sum: wave_sum, then (w0 + w1) + (w2 + w3) -- hop_merge.h's order
//   sigmoid  d = 1 + e (__fadd_rn); x >= 0 ? 1 / d : e / d (__fdiv_rn): never 1 / (1 + exp(-x)) with an infinite
//            exp, no NaN or Inf for any finite x
//   dl       (sigmoid - t) and its product with invB each rounded once (__fsub_rn, __fmul_rn)
// A row whose set has no non-empty entry is an unlabelled sample: lossrow = 0, dl = +0 for every k.  A row whose
// entries all carry weight 0 is labelled with the all-zero target: every answer is pushed down.
// The set sits in LDS once per workgroup: at most 16 compares per logit, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include "common.h"
#include "hop_merge.h"   // block_sum, block_first_max: k_ce_fwd's reduction orders; bce_target, bce_term
#include "kernels.h"

namespace rau {
namespace {

__global__ __launch_bounds__(256) void k_bce_fwd(int nB, int K, int M, const float* __restrict__ logits,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ ids, const float* __restrict__ w, int G,
    const float* __restrict__ mf, const float* __restrict__ wd, const float* __restrict__ bd,
    float* __restrict__ dl, float* __restrict__ lossrow, int32_t* __restrict__ argmax, float* __restrict__ dopred,
    const float* __restrict__ part, int nsplit, const float* __restrict__ bias, float* __restrict__ logits_out,
    int Bper, int ld, const float* __restrict__ sw) {
  RAU_CHAIN_PRIO();
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ float s_sum[4];
  __shared__ int s_id[kMaxAnswers];     // 0-based answer, -1 = empty entry
  __shared__ float s_w[kMaxAnswers];    // its weight (0 for an empty entry)
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const bool truth = G > 0 || labels;   // uniform per launch
  const int ng = G > 0 ? G : 1;         // labels: the one-entry set {(y, 1)}
  if (G > 0) {
    if (tid < G) {
      // rows = [hop][sample]: the sets repeat every Bper rows; ids clamped like k_ce_set_fwd's
      const size_t e = (size_t)(b % Bper) * G + tid;
      const int id = min(max(ids[e], 0), K);
      s_id[tid] = id - 1;
      s_w[tid] = id > 0 ? w[e] : 0.f;
    }
  } else if (labels && tid == 0) {
    s_id[0] = min(max(labels[b % Bper], 1), K) - 1;   // clamped like k_ce_fwd's label
    s_w[0] = 1.f;
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
  __syncthreads();   // the set; each thread reads back only the logits it finished itself
  const float* lg = logits + (size_t)b * ld;
  float mx = -INFINITY;
  int ai = 0x7fffffff;
  for (int k = tid; k < K; k += 256) {
    const float v = lg[k];
    if (v > mx) { mx = v; ai = k; }
  }
  block_first_max(mx, ai, s_val, s_idx);
  if (tid == 0) argmax[b] = ai + 1;
  if (truth) {
    const bool labelled = bce_labelled(s_id, ng);
    const float sb = sw ? sw[b % Bper] : 1.f;
    const float invB = __fmul_rn(sb, 1.f / (float)Bper);
    float acc = 0.f;
    for (int k = tid; k < K; k += 256) {
      if (!labelled) {   // an unlabelled sample (uniform per workgroup)
        dl[(size_t)b * ld + k] = 0.f;
        continue;
      }
      const float t = bce_target(s_id, s_w, ng, k);
      const float x = lg[k];
      const float e = expf(-fabsf(x));
      acc = __fadd_rn(acc, bce_term(x, t, e));
      const float d = __fadd_rn(1.f, e);
      const float sg = x >= 0.f ? __fdiv_rn(1.f, d) : __fdiv_rn(e, d);
      dl[(size_t)b * ld + k] = __fmul_rn(__fsub_rn(sg, t), invB);
    }
    for (int k = K + tid; k < ld; k += 256) dl[(size_t)b * ld + k] = 0.f;   // the row's pad
    acc = block_sum(acc, s_sum);
    if (tid == 0) lossrow[b] = __fmul_rn(sb, acc);
  }
  // do_pred
  if (!mf) return;   // criterion-only use (uniform per launch)
  float acc = 0.f;
  for (int m = tid; m < M; m += 256) acc += mf[(size_t)b * M + m] * wd[m];
  acc = block_sum(acc, s_sum);
  if (tid == 0) dopred[b] = sigmoidf_(acc + bd[0]);
}

}  // namespace

hipError_t bce_fwd(hipStream_t st, int nB, int K, int M, const float* logits, const int32_t* labels,
                   const int32_t* ids, const float* w, int G, const float* mf, const float* wd, const float* bd,
                   float* dl, float* lossrow, int32_t* argmax, float* dopred, const float* part, int nsplit,
                   const float* bias, float* logits_out, int Bper, int ld, const float* sw) {
  if (G < 0 || G > kMaxAnswers || (G > 0 && (!ids || !w))) return hipErrorInvalidValue;
  if (!split_span_ok(part, nsplit, (size_t)nB * K)) return kSplitStateError;
  if (ld != 0 && ld < K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bce_fwd, dim3(nB), dim3(256), 0, st, nB, K, M, logits, labels, ids, w, G, mf, wd, bd, dl,
                     lossrow, argmax, dopred, part, nsplit, bias, logits_out, Bper > 0 ? Bper : nB, ld ? ld : K,
                     sw);
  return hipGetLastError();
}

}  // namespace rau

// cand_head.hip -- the classifier loss head RESTRICTED TO A ROW'S CANDIDATES (rau_set_candidates): k_ce_fwd's /
// k_ce_set_fwd's / k_bce_fwd's launch contract (one 256-thread workgroup per (hop, sample) row; finishing of K-split
// partials plus bias, the row's pad written +0; first-max argmax OVER ALL K -- the open-ended answer; do_pred; chain
// priority; no loss and no dl without a ground truth; no do_pred without mf) with the criterion normalised over the
// candidates only.  A row's list is C entries (ids 1..K, 0 = empty); an entry equal to an earlier entry of the row is
// dead, so a duplicate id counts once.  L = the live entries, x = the finished logits.
//   kept truth  set entries -- or the label as the set {(y, 1)} -- whose id is not in L become empty entries
//   softmax     m = max_{c in L} x_c;  den = sum_{c in L} expf(x_c - m) added from +0 in entry order;
//               lse = m + logf(den);  W = the kept weights added from +0 in entry order
//               lossrow = sum_g w_g (lse - x[y_g]) over the kept entries, from +0 in entry order
//               dl[k]   = (expf(x_k - m) / den) (W invB), then for the kept g in order: if (y_g == k) dl[k] -= w_g invB
//               for k in L, +0 elsewhere; a row without a kept entry is unlabelled: lossrow 0, dl +0
//   sigmoid     t_c = bce_target over the kept entries;  lossrow = sum_{c in L} bce_term(x_c, t_c, expf(-|x_c|)) from
//               +0 in entry order;  dl[k_c] = (sigmoid(x_c) - t_c) invB, +0 elsewhere; a row is labelled when its
//               kept set has a non-empty entry (hop_merge.h's bce_labelled), else lossrow 0, dl +0
// invB = __fmul_rn(s_b, 1 / Bper) and the row written is __fmul_rn(s_b, lossrow), s_b the sample weight or 1.  Every
// rounding is spelled out as in ce_set.hip / bce_head.hip: the products w_g invB, W invB, w_g (lse - x[y_g]) and
// every sum are rounded once, and the FIRST kept match of a candidate is subtracted inside the product's fused
// multiply-add.  A row whose one live candidate is its truth has den = 1, lse = x, so loss and gradient are 0 up to
// the rounding of expf(0).
// The list (at most 32) and the set (at most 16) sit in LDS once per workgroup; the threads tid < C mark the dead
// entries, each comparing its entry with the earlier ones.  The restricted sums (den, W, the loss row) are formed
// SERIALLY in entry order from LDS: den and W by every thread on its own (broadcast reads, no reduction tree, no
// further barrier), the loss row by thread 0.  The workgroup clears its dl row with 16-byte stores over the pitch
// (next to the stores that finish the logits, so one barrier waits for both), and behind it the lanes that own a
// live candidate write their one element: live candidates are distinct, so no atomics, no scratch, the same bits on
// every call.
#include <hip/hip_runtime.h>

#include "common.h"
#include "hop_merge.h"   // block_sum, block_first_max: k_ce_fwd's reduction orders; bce_target, bce_term, bce_labelled
#include "kernels.h"

namespace rau {
namespace {

template <int KIND>   // 0: softmax (RAU_LOSS_CE), 1: per-answer sigmoid (RAU_LOSS_BCE)
__global__ __launch_bounds__(256) void k_cand_fwd(int nB, int K, int M, const float* __restrict__ logits,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ ids, const float* __restrict__ w, int G,
    const int32_t* __restrict__ cand, int C, const float* __restrict__ mf, const float* __restrict__ wd,
    const float* __restrict__ bd, float* __restrict__ dl, float* __restrict__ lossrow, int32_t* __restrict__ argmax,
    float* __restrict__ dopred, const float* __restrict__ part, int nsplit, const float* __restrict__ bias,
    float* __restrict__ logits_out, int Bper, int ld, const float* __restrict__ sw) {
  RAU_CHAIN_PRIO();
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ float s_sum[4];
  __shared__ int s_id[kMaxAnswers];        // 0-based answer, -1 = empty or dropped entry
  __shared__ float s_w[kMaxAnswers];       // its weight (0 for such an entry)
  __shared__ int s_raw[kMaxCandidates];    // 0-based candidate as given, -1 = empty
  __shared__ int s_c[kMaxCandidates];      // ... -1 = empty or dead
  __shared__ float s_x[kMaxCandidates];    // its logit (0 for a dead entry)
  __shared__ float s_e[kMaxCandidates];    // softmax: expf(x - m); sigmoid: the entry's loss term
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int bs = b % Bper;                 // rows = [hop][sample]: labels, sets and lists repeat every Bper rows
  const bool truth = G > 0 || labels;      // uniform per launch
  const int ng = G > 0 ? G : 1;            // labels: the one-entry set {(y, 1)}
  if (G > 0) {
    if (tid < G) {
      const size_t e = (size_t)bs * G + tid;
      const int id = min(max(ids[e], 0), K);   // clamped like k_ce_set_fwd's
      s_id[tid] = id - 1;
      s_w[tid] = id > 0 ? w[e] : 0.f;
    }
  } else if (labels && tid == 0) {
    s_id[0] = min(max(labels[bs], 1), K) - 1;  // clamped like k_ce_fwd's label
    s_w[0] = 1.f;
  }
  if (tid < C) s_raw[tid] = min(max(cand[(size_t)bs * C + tid], 0), K) - 1;
  if (nsplit) {  // logits arrive as K-split partials [split][nB][K] of mf Wc^T: finish them here
    for (int k = tid; k < K; k += 256) {
      float v = bias[k];
      for (int sp = 0; sp < nsplit; ++sp) v += part[((size_t)sp * nB + b) * K + k];
      logits_out[(size_t)b * ld + k] = v;
    }
    for (int k = K + tid; k < ld; k += 256) logits_out[(size_t)b * ld + k] = 0.f;   // the row's pad
    logits = logits_out;
  }
  if (truth) {   // the dl row: +0, the pad included (in front of the barrier, which waits for these stores anyway)
    float4* d4 = reinterpret_cast<float4*>(dl + (size_t)b * ld);
    for (int i = tid; i < ld / 4; i += 256) d4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();   // the set, the list, and the finished logits the candidates' owners read below, the cleared row
  const float* lg = logits + (size_t)b * ld;
  if (tid < C) {     // an entry equal to an earlier one is dead
    const int c = s_raw[tid];
    bool live = c >= 0;
    for (int j = 0; j < tid; ++j) live = live && s_raw[j] != c;
    s_c[tid] = live ? c : -1;
    s_x[tid] = live ? lg[c] : 0.f;
  }
  float mx = -INFINITY;
  int ai = 0x7fffffff;
  for (int k = tid; k < K; k += 256) {
    const float v = lg[k];
    if (v > mx) { mx = v; ai = k; }
  }
  block_first_max(mx, ai, s_val, s_idx);   // (its barriers publish s_c and s_x)
  if (tid == 0) argmax[b] = ai + 1;
  if (truth) {
    if (tid < ng) {   // kept truth: an entry whose id is not a live candidate becomes an empty entry
      const int id = s_id[tid];
      bool in = false;
      for (int c = 0; c < C; ++c) in = in || (id >= 0 && s_c[c] == id);
      if (!in) { s_id[tid] = -1; s_w[tid] = 0.f; }
    }
    float* drow = dl + (size_t)b * ld;
    const float sb = sw ? sw[bs] : 1.f;
    const float invB = __fmul_rn(sb, 1.f / (float)Bper);
    const int mine = tid < C ? s_c[tid] : -1;
    if (KIND == 0) {
      float m = -INFINITY;
      for (int c = 0; c < C; ++c)
        if (s_c[c] >= 0) m = fmaxf(m, s_x[c]);
      if (tid < C) s_e[tid] = mine >= 0 ? expf(s_x[tid] - m) : 0.f;
      __syncthreads();   // the kept set, s_e
      const bool labelled = bce_labelled(s_id, ng);   // uniform per workgroup
      if (labelled) {
        float den = 0.f;
        for (int c = 0; c < C; ++c)
          if (s_c[c] >= 0) den = __fadd_rn(den, s_e[c]);
        const float lse = m + logf(den);
        float W = 0.f;
        for (int g = 0; g < ng; ++g) W = __fadd_rn(W, s_w[g]);
        const float scale = __fmul_rn(W, invB);
        if (mine >= 0) {
          const float e = s_e[tid] / den;   // expf(x - m) / den, as the full-vocabulary heads form it
          float p = __fmul_rn(e, scale);
          bool hit = false;
          for (int g = 0; g < ng; ++g)
            if (s_id[g] == mine) {
              const float wb = __fmul_rn(s_w[g], invB);
              p = hit ? __fsub_rn(p, wb) : __fmaf_rn(e, scale, -wb);
              hit = true;
            }
          drow[mine] = p;
        }
        if (tid == 0) {
          float acc = 0.f;
          for (int g = 0; g < ng; ++g)
            if (s_id[g] >= 0) acc = __fadd_rn(acc, __fmul_rn(s_w[g], lse - lg[s_id[g]]));
          lossrow[b] = __fmul_rn(sb, acc);
        }
      } else if (tid == 0) {
        lossrow[b] = 0.f;
      }
    } else {
      __syncthreads();   // the kept set
      const bool labelled = bce_labelled(s_id, ng);   // uniform per workgroup
      if (tid < C) {
        float term = 0.f;
        if (labelled && mine >= 0) {
          const float t = bce_target(s_id, s_w, ng, mine);
          const float x = s_x[tid];
          const float e = expf(-fabsf(x));
          term = bce_term(x, t, e);
          const float d = __fadd_rn(1.f, e);
          const float sg = x >= 0.f ? __fdiv_rn(1.f, d) : __fdiv_rn(e, d);
          drow[mine] = __fmul_rn(__fsub_rn(sg, t), invB);
        }
        s_e[tid] = term;
      }
      __syncthreads();
      if (tid == 0) {
        float acc = 0.f;
        for (int c = 0; c < C; ++c)
          if (s_c[c] >= 0) acc = __fadd_rn(acc, s_e[c]);
        lossrow[b] = labelled ? __fmul_rn(sb, acc) : 0.f;
      }
    }
  }
  // do_pred
  if (!mf) return;   // criterion-only use (uniform per launch)
  float acc = 0.f;
  for (int m = tid; m < M; m += 256) acc += mf[(size_t)b * M + m] * wd[m];
  acc = block_sum(acc, s_sum);
  if (tid == 0) dopred[b] = sigmoidf_(acc + bd[0]);
}

}  // namespace

hipError_t cand_fwd(hipStream_t st, int kind, int nB, int K, int M, const float* logits, const int32_t* labels,
                    const int32_t* ids, const float* w, int G, const int32_t* cand, int C, const float* mf,
                    const float* wd, const float* bd, float* dl, float* lossrow, int32_t* argmax, float* dopred,
                    const float* part, int nsplit, const float* bias, float* logits_out, int Bper, int ld,
                    const float* sw) {
  if (C < 1 || C > kMaxCandidates || !cand) return hipErrorInvalidValue;
  if (G < 0 || G > kMaxAnswers || (G > 0 && (!ids || !w))) return hipErrorInvalidValue;
  if (!split_span_ok(part, nsplit, (size_t)nB * K)) return kSplitStateError;
  if (ld == 0) ld = K;
  if (ld < K) return hipErrorInvalidValue;
  // the row clear: 16-byte stores over the pitch
  if ((G > 0 || labels) && (ld % 4 != 0 || (reinterpret_cast<uintptr_t>(dl) & 15u) != 0)) return hipErrorInvalidValue;
  if (Bper <= 0) Bper = nB;
  if (kind == 0)
    hipLaunchKernelGGL(k_cand_fwd<0>, dim3(nB), dim3(256), 0, st, nB, K, M, logits, labels, ids, w, G, cand, C, mf, wd,
                       bd, dl, lossrow, argmax, dopred, part, nsplit, bias, logits_out, Bper, ld, sw);
  else
    hipLaunchKernelGGL(k_cand_fwd<1>, dim3(nB), dim3(256), 0, st, nB, K, M, logits, labels, ids, w, G, cand, C, mf, wd,
                       bd, dl, lossrow, argmax, dopred, part, nsplit, bias, logits_out, Bper, ld, sw);
  return hipGetLastError();
}

}  // namespace rau

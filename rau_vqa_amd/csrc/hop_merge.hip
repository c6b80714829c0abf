// hop_merge.hip -- the bookkeeping feval and predict_result do on top of the hop outputs, on the
// resident outputs of the last step-level forward (logits [H,B,K], do_pred [H,B], argmax [H,B],
// lossrow [H,B], attention [H,B,Sp]):
//   step_stats   -- feval's joint-loss statistics (SS:476-556): CE of the uni and select merges (under
//                   RAU_LOSS_BCE their per-answer sigmoid criterion, k_step_stats_bce),
//                   the BCE of every hop's do_pred against (argmax_h == y), the accuracy counters;
//   predict_rows -- predict_result's merges (SS:633-705) and the eval loop's open-ended and
//                   multiple-choice answers (SS:877-900).
// One workgroup of 256 threads per sample; merged rows are recomputed from the hop logits in
// every pass (no LDS staging, so no limit on K).  The batch reduction is a second, single-
// workgroup launch in a fixed order: no float atomics, repeated queries give the same bits.
#include <hip/hip_runtime.h>

#include "common.h"
#include "hop_merge.h"   // kMT, block_sum, block_first_max, row_val, select_hop: shared with topk.hip, ce_set.hip
#include "kernels.h"

namespace rau {
namespace {

// CrossEntropyCriterion of row r against label y (0-based) with k_ce_fwd's formulation: max, sum of
// exp(l - max) in the same thread-strided order, lse - l_y.  Also the row's first-max index.
__device__ void row_ce(const float* __restrict__ lg, size_t hs, int H, int K, int r, int hsel, int y,
                       float* s_val, int* s_idx, float* s_sum, float& ce, int& ans) {
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  int ai = 0x7fffffff;
  for (int k = tid; k < K; k += kMT) {
    const float v = row_val(lg, hs, H, r, hsel, k);
    if (v > mx) { mx = v; ai = k; }
  }
  block_first_max(mx, ai, s_val, s_idx);
  float den = 0.f;
  for (int k = tid; k < K; k += kMT) den += expf(row_val(lg, hs, H, r, hsel, k) - mx);
  den = block_sum(den, s_sum);
  const float lse = mx + logf(den);
  ce = lse - row_val(lg, hs, H, r, hsel, y);
  ans = ai;
}

// One workgroup per sample: rowf[b] = {uni CE, select CE, BCE[H]},
// rowi[b] = correct[H+2] | do_pred_correct[H] | did_correct | fired[H] | selected[H].
__global__ __launch_bounds__(kMT) void k_step_stats_rows(int H, int B, int K, int ld,
    const float* __restrict__ logits, const float* __restrict__ dopred,
    const int32_t* __restrict__ argmax, const int32_t* __restrict__ labels,
    float* __restrict__ rowf, int32_t* __restrict__ rowi) {
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ float s_sum[4];
  const int b = blockIdx.x;
  const size_t hs = (size_t)B * ld;   // rows at pitch ld >= K
  const float* lg = logits + (size_t)b * ld;
  const int y = min(max(labels[b], 1), K) - 1;   // checked at upload; clamped like k_ce_fwd
  const int hsel = select_hop(dopred, H, B, b, false);   // feval: the last hop is not forced
  float ce_u, ce_s;
  int a_u, a_s;
  row_ce(lg, hs, H, K, H, hsel, y, s_val, s_idx, s_sum, ce_u, a_u);       // SS:522-530
  row_ce(lg, hs, H, K, H + 1, hsel, y, s_val, s_idx, s_sum, ce_s, a_s);   // SS:532-540
  if (threadIdx.x != 0) return;
  float* f = rowf + (size_t)b * (H + 2);
  int32_t* c = rowi + (size_t)b * (4 * H + 3);
  f[0] = ce_u;
  f[1] = ce_s;
  int did = 0;   // did_correct, SS:513
  for (int h = 0; h < H; ++h) {
    const int gt = argmax[(size_t)h * B + b] == y + 1;   // do_pred_gt = (argmax_h == y), SS:490, 497
    c[h] = gt;
    did |= gt;
  }
  c[H] = a_u == y;
  c[H + 1] = a_s == y;
  c[2 * H + 2] = did;
  for (int h = 0; h < H; ++h) {
    const float x = dopred[(size_t)h * B + b];
    const int fire = x > 0.5f;
    const float t = c[h] ? 1.f : 0.f;
    // nn.BCECriterion, SS:555: -(t log(x + eps) + (1 - t) log(1 - x + eps)), eps = 1e-12
    f[2 + h] = -(t * logf(x + 1e-12f) + (1.f - t) * logf(1.f - x + 1e-12f));
    c[H + 2 + h] = (fire == c[h]) && did;   // SS:552, masked by did_correct
    c[2 * H + 3 + h] = fire;
    c[3 * H + 3 + h] = h == hsel;
  }
}

// max, first-max index and log-sum-exp of row r, in row_ce's order
__device__ void row_lse(const float* __restrict__ lg, size_t hs, int H, int K, int r, int hsel, float* s_val,
                        int* s_idx, float* s_sum, float& lse, int& ans) {
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  int ai = 0x7fffffff;
  for (int k = tid; k < K; k += kMT) {
    const float v = row_val(lg, hs, H, r, hsel, k);
    if (v > mx) { mx = v; ai = k; }
  }
  block_first_max(mx, ai, s_val, s_idx);
  float den = 0.f;
  for (int k = tid; k < K; k += kMT) den += expf(row_val(lg, hs, H, r, hsel, k) - mx);
  den = block_sum(den, s_sum);
  lse = mx + logf(den);
  ans = ai;
}

// metric score of the 0-based answer a against the set in LDS: sum of the matching entries' scores in entry order
__device__ __forceinline__ float set_score(const int* s_id, const float* s_sc, int G, int a) {
  float s = 0.f;
  for (int g = 0; g < G; ++g)
    if (s_id[g] == a) s = __fadd_rn(s, s_sc[g]);
  return s;
}

// k_step_stats_rows for a batch with an answer set (rau_set_answers): the label y becomes the set.  An answer
// is correct when it carries a positive score (scores are >= 0: some matching non-empty entry has score > 0),
// the uni / select CE are the soft CE of ce_set.hip, sum_g w_g (lse - row[y_g]) from 0 in entry order.  Also
// rowscore [H+2][B]: the score of every row's answer.
__global__ __launch_bounds__(kMT) void k_step_stats_rows_set(int H, int B, int K, int ld,
    const float* __restrict__ logits, const float* __restrict__ dopred, const int32_t* __restrict__ argmax,
    const int32_t* __restrict__ ids, const float* __restrict__ w, const float* __restrict__ score, int G,
    float* __restrict__ rowf, int32_t* __restrict__ rowi, float* __restrict__ rowscore) {
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ float s_sum[4];
  __shared__ int s_id[kMaxAnswers];
  __shared__ float s_w[kMaxAnswers];
  __shared__ float s_sc[kMaxAnswers];
  const int b = blockIdx.x;
  const size_t hs = (size_t)B * ld;   // rows at pitch ld >= K
  const float* lg = logits + (size_t)b * ld;
  if (threadIdx.x < G) {
    const size_t e = (size_t)b * G + threadIdx.x;
    const int id = min(max(ids[e], 0), K);
    s_id[threadIdx.x] = id - 1;
    s_w[threadIdx.x] = id > 0 ? w[e] : 0.f;
    s_sc[threadIdx.x] = id > 0 ? score[e] : 0.f;
  }
  __syncthreads();
  const int hsel = select_hop(dopred, H, B, b, false);   // feval: the last hop is not forced
  float lse_u, lse_s;
  int a_u, a_s;
  row_lse(lg, hs, H, K, H, hsel, s_val, s_idx, s_sum, lse_u, a_u);
  row_lse(lg, hs, H, K, H + 1, hsel, s_val, s_idx, s_sum, lse_s, a_s);
  if (threadIdx.x != 0) return;
  float* f = rowf + (size_t)b * (H + 2);
  int32_t* c = rowi + (size_t)b * (4 * H + 3);
  float ce_u = 0.f, ce_s = 0.f;
  for (int g = 0; g < G; ++g) {
    if (s_id[g] < 0) continue;
    ce_u = __fadd_rn(ce_u, __fmul_rn(s_w[g], lse_u - row_val(lg, hs, H, H, hsel, s_id[g])));
    ce_s = __fadd_rn(ce_s, __fmul_rn(s_w[g], lse_s - row_val(lg, hs, H, H + 1, hsel, s_id[g])));
  }
  f[0] = ce_u;
  f[1] = ce_s;
  int did = 0;
  for (int h = 0; h < H; ++h) {
    const float sc = set_score(s_id, s_sc, G, argmax[(size_t)h * B + b] - 1);
    rowscore[(size_t)h * B + b] = sc;
    const int gt = sc > 0.f;
    c[h] = gt;
    did |= gt;
  }
  const float sc_u = set_score(s_id, s_sc, G, a_u), sc_s = set_score(s_id, s_sc, G, a_s);
  rowscore[(size_t)H * B + b] = sc_u;
  rowscore[(size_t)(H + 1) * B + b] = sc_s;
  c[H] = sc_u > 0.f;
  c[H + 1] = sc_s > 0.f;
  c[2 * H + 2] = did;
  for (int h = 0; h < H; ++h) {
    const float x = dopred[(size_t)h * B + b];
    const int fire = x > 0.5f;
    const float t = c[h] ? 1.f : 0.f;
    f[2 + h] = -(t * logf(x + 1e-12f) + (1.f - t) * logf(1.f - x + 1e-12f));
    c[H + 2 + h] = (fire == c[h]) && did;
    c[2 * H + 3 + h] = fire;
    c[3 * H + 3 + h] = h == hsel;
  }
}

// RAU_LOSS_BCE: the uni / select losses of rowf[b] become the per-answer sigmoid criterion of those rows against
// the same target, in bce_head.hip's formulation and summation order (thread-strided in ascending k, block_sum);
// a row whose set has no non-empty entry: 0.  Runs behind k_step_stats_rows(_set), which leaves everything else --
// the counts, the do_pred BCE, the scores depend on logits and argmax only.  labels: G = 0.
__global__ __launch_bounds__(kMT) void k_step_stats_bce(int H, int B, int K, int ld, const float* __restrict__ logits,
    const float* __restrict__ dopred, const int32_t* __restrict__ labels, const int32_t* __restrict__ ids,
    const float* __restrict__ w, int G, float* __restrict__ rowf) {
  __shared__ float s_sum[4];
  __shared__ int s_id[kMaxAnswers];
  __shared__ float s_w[kMaxAnswers];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t hs = (size_t)B * ld;   // rows at pitch ld >= K
  const float* lg = logits + (size_t)b * ld;
  const int ng = G > 0 ? G : 1;
  if (G > 0) {
    if (tid < G) {
      const size_t e = (size_t)b * G + tid;
      const int id = min(max(ids[e], 0), K);
      s_id[tid] = id - 1;
      s_w[tid] = id > 0 ? w[e] : 0.f;
    }
  } else if (tid == 0) {
    s_id[0] = min(max(labels[b], 1), K) - 1;
    s_w[0] = 1.f;
  }
  __syncthreads();
  const int hsel = select_hop(dopred, H, B, b, false);   // feval: the last hop is not forced
  const bool labelled = bce_labelled(s_id, ng);
  for (int r = H; r < H + 2; ++r) {
    float acc = 0.f;
    if (labelled)
      for (int k = tid; k < K; k += kMT) {
        const float x = row_val(lg, hs, H, r, hsel, k);
        acc = __fadd_rn(acc, bce_term(x, bce_target(s_id, s_w, ng, k), expf(-fabsf(x))));
      }
    acc = block_sum(acc, s_sum);
    if (tid == 0) rowf[(size_t)b * (H + 2) + (r - H)] = acc;
  }
}

// out[r][b] = score of the 1-based answer ans[r][b] against sample b's set; one thread per (r, b)
__global__ __launch_bounds__(kMT) void k_answer_scores(int R, int B, int K, const int32_t* __restrict__ ans,
    const int32_t* __restrict__ ids, const float* __restrict__ score, int G, float* __restrict__ out) {
  const int i = blockIdx.x * kMT + threadIdx.x;
  if (i >= R * B) return;
  const int b = i % B, a = ans[i];
  float s = 0.f;
  for (int g = 0; g < G; ++g) {
    const int id = min(max(ids[(size_t)b * G + g], 0), K);
    if (id > 0 && id == a) s = __fadd_rn(s, score[(size_t)b * G + g]);
  }
  out[i] = s;
}

// One workgroup: tot[r] = sum_b x[r][b], lane-strided over the batch then wave_sum: a fixed order
__global__ __launch_bounds__(kMT) void k_score_totals(int R, int B, const float* __restrict__ x,
                                                      float* __restrict__ tot) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = w; r < R; r += 4) {
    float acc = 0.f;
    for (int b = l; b < B; b += 64) acc += x[(size_t)r * B + b];
    acc = wave_sum(acc);
    if (l == 0) tot[r] = acc;
  }
}

// One workgroup: out = loss[H+2] | loss_do_pred[H] (floats) | counts[4H+3] (int32).  Float columns
// are reduced like k_loss_reduce (lane-strided over the batch, wave_sum, / B), so the per-hop CE is
// bitwise the step's own rau_get_losses.  sw (rau_set_sample_weights, or null): the uni / select losses and the
// do_pred BCE enter their sums as __fmul_rn(sw[b], row) -- lossrow already holds the weighted rows; the counts stay
// unweighted.
__global__ __launch_bounds__(kMT) void k_step_stats_reduce(int H, int B, const float* __restrict__ lossrow,
    const float* __restrict__ rowf, const int32_t* __restrict__ rowi, float* __restrict__ out,
    const float* __restrict__ sw) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int NF = H + 2, NL = 2 * H + 2, NC = 4 * H + 3;
  for (int j = w; j < NL; j += 4) {
    float acc = 0.f;
    for (int b = l; b < B; b += 64)
      acc += j < H ? lossrow[(size_t)j * B + b]
                   : sw ? __fmul_rn(sw[b], rowf[(size_t)b * NF + (j - H)]) : rowf[(size_t)b * NF + (j - H)];
    acc = wave_sum(acc);
    if (l == 0) out[j] = acc / (float)B;
  }
  int32_t* cnt = reinterpret_cast<int32_t*>(out + NL);
  for (int j = threadIdx.x; j < NC; j += kMT) {
    int s = 0;
    for (int b = 0; b < B; ++b) s += rowi[(size_t)b * NC + j];
    cnt[j] = s;
  }
}

// One workgroup per sample: for each row r of {hops, uni, select} (predict rule: last hop forced)
// the first-max answer of the row (oe) and of row * mc_mask (mc: the reference multiplies the RAW
// logits by a 0/1 mask, SS:893-894, so masked-out entries are +-0 and +0 / -0 tie at the lower
// index); the merged rows go to pred [2][B][K] and att_out [2][B][Sp] (select without any carry).
__global__ __launch_bounds__(kMT) void k_predict_rows(int H, int B, int K, int ld, int Sp,
    const float* __restrict__ logits, const float* __restrict__ dopred, const float* __restrict__ att,
    const int32_t* __restrict__ mc, int n_mc, int32_t* __restrict__ oe, int32_t* __restrict__ mco,
    float* __restrict__ pred, float* __restrict__ att_out) {
  extern __shared__ uint32_t s_mask[];   // candidate bit set of the sample, (K + 31) / 32 words (mc only)
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t hs = (size_t)B * ld;   // rows at pitch ld >= K
  const float* lg = logits + (size_t)b * ld;
  const int hsel = select_hop(dopred, H, B, b, true);   // >= 0: the last hop always fires
  if (mc) {   // test_mc_mask, SS:885-892: 0 = empty slot
    const int nw = (K + 31) / 32;
    for (int i = tid; i < nw; i += kMT) s_mask[i] = 0u;
    __syncthreads();
    for (int j = tid; j < n_mc; j += kMT) {
      const int a = mc[(size_t)b * n_mc + j];
      if (a >= 1 && a <= K) atomicOr(&s_mask[(a - 1) >> 5], 1u << ((a - 1) & 31));
    }
    __syncthreads();
  }
  for (int r = 0; r < H + 2; ++r) {
    float mx = -INFINITY, mm = -INFINITY;
    int ai = 0x7fffffff, mi = 0x7fffffff;
    float* prow = (r >= H && pred) ? pred + ((size_t)(r - H) * B + b) * ld : nullptr;
    if (prow)   // the merged row's pad
      for (int k = K + tid; k < ld; k += kMT) prow[k] = 0.f;
    for (int k = tid; k < K; k += kMT) {
      const float v = row_val(lg, hs, H, r, hsel, k);
      if (prow) prow[k] = v;
      if (v > mx) { mx = v; ai = k; }
      if (mc) {
        const float vm = v * (((s_mask[k >> 5] >> (k & 31)) & 1u) ? 1.f : 0.f);
        if (vm > mm) { mm = vm; mi = k; }
      }
    }
    block_first_max(mx, ai, s_val, s_idx);
    if (mc) block_first_max(mm, mi, s_val, s_idx);
    if (tid == 0) {
      oe[(size_t)r * B + b] = ai + 1;
      if (mc) mco[(size_t)r * B + b] = mi + 1;
    }
  }
  if (!att_out) return;
  // SS:681, 688, 700: uni = (0 + a_1 + .. + a_H) / H, select = 0 + a_hsel
  const float* ab = att + (size_t)b * Sp;
  const size_t as = (size_t)B * Sp;
  for (int s = tid; s < Sp; s += kMT) {
    float u = 0.f;
    for (int h = 0; h < H; ++h) u += ab[(size_t)h * as + s];
    att_out[(size_t)b * Sp + s] = __fdiv_rn(u, (float)H);
    att_out[as + (size_t)b * Sp + s] = 0.f + ab[(size_t)hsel * as + s];
  }
}

}  // namespace

hipError_t step_stats(hipStream_t st, int H, int B, int K, const float* logits, const float* dopred,
                      const int32_t* argmax, const float* lossrow, const Truth& t, float* rowf, int32_t* rowi,
                      float* out, float* rowscore, float* tot, int ld) {
  if (ld == 0) ld = K;
  if (ld < K) return hipErrorInvalidValue;
  if (t.G > 0 && (t.G > kMaxAnswers || !t.ids || !t.w || !t.score)) return hipErrorInvalidValue;
  if (t.G > 0)
    hipLaunchKernelGGL(k_step_stats_rows_set, dim3(B), dim3(kMT), 0, st, H, B, K, ld, logits, dopred, argmax, t.ids,
                       t.w, t.score, t.G, rowf, rowi, rowscore);
  else
    hipLaunchKernelGGL(k_step_stats_rows, dim3(B), dim3(kMT), 0, st, H, B, K, ld, logits, dopred, argmax, t.labels,
                       rowf, rowi);
  if (t.bce())   // the two merged rows' losses under the sigmoid criterion, in place of the softmax CE just written
    hipLaunchKernelGGL(k_step_stats_bce, dim3(B), dim3(kMT), 0, st, H, B, K, ld, logits, dopred, t.labels, t.ids, t.w,
                       t.G, rowf);
  hipLaunchKernelGGL(k_step_stats_reduce, dim3(1), dim3(kMT), 0, st, H, B, lossrow, rowf, rowi, out, t.sw);
  if (t.G > 0) hipLaunchKernelGGL(k_score_totals, dim3(1), dim3(kMT), 0, st, H + 2, B, rowscore, tot);
  return hipGetLastError();
}

hipError_t answer_scores(hipStream_t st, int R, int B, int K, const int32_t* ans, const Truth& t, float* out,
                         float* tot) {
  if (t.G < 1 || t.G > kMaxAnswers || !t.ids || !t.score) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_answer_scores, dim3((R * B + kMT - 1) / kMT), dim3(kMT), 0, st, R, B, K, ans, t.ids, t.score,
                     t.G, out);
  hipLaunchKernelGGL(k_score_totals, dim3(1), dim3(kMT), 0, st, R, B, out, tot);
  return hipGetLastError();
}

size_t predict_rows_lds(int K) { return (size_t)((K + 31) / 32) * sizeof(uint32_t); }

hipError_t predict_rows(hipStream_t st, int H, int B, int K, int Sp, const float* logits, const float* dopred,
                        const float* att, const int32_t* mc, int n_mc, int32_t* oe, int32_t* mco, float* pred,
                        float* att_out, int ld) {
  if (ld == 0) ld = K;
  if (ld < K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_predict_rows, dim3(B), dim3(kMT), mc ? predict_rows_lds(K) : 0, st, H, B, K, ld, Sp, logits,
                     dopred, att, mc, n_mc, oe, mco, pred, att_out);
  return hipGetLastError();
}

}  // namespace rau

// select_bwd.hip -- the step-selection head's own gradient in the step-level backward (rau_backward_select).
// The head is do_pred = sigmoid(wd . mf + bd) per (hop, sample) row (SS:281, computed by the criterion-head
// kernel); its loss is nn.BCECriterion (sizeAverage) against do_pred_gt, SS:555, 565, scaled per hop by
// select_w[h] where the reference has d_do_pred:mul(0), SS:566.  With x = do_pred, n = samples per hop,
// eps = 1e-12f, every step rounded once in float32, in this order:
//   t   = do_pred_gt: the row's first-max answer equals the label, or (answer set) carries a positive score --
//         k_step_stats_rows' / k_step_stats_rows_set's rule; a constant
//   ddp = select_w[h] * ( -(t - x) / ((1 - x + eps) * (x + eps)) ) / n
//   s   = ddp * x * (1 - x)                                   (through the sigmoid)
// With a sample weight s_b (rau_set_sample_weights) select_w[h] is replaced by __fmul_rn(select_w[h], s_b), the rest
// of the formula unchanged; without weights s_b = 1 and the product is select_w[h] exactly.
// k_select_signal writes s [rows] and the rank-1 term add[r][m] = s[r] wd[m] that enters dmf in front of the
// merge_feat dropout mask (the addend of the head_dgrad GEMM); k_select_wgrad adds sum_r s[r] mf[r][:] to the
// head's weight gradient and sum_r s[r] to its bias gradient in one pass, summed in a fixed order: no atomics,
// repeated calls give the same bits.
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace rau {
namespace {

// one 256-thread workgroup per row r = h * Bper + b; every thread forms the row's (uniform) s
__global__ __launch_bounds__(256) void k_select_signal(int Bper, int K, int M, const float* __restrict__ dopred,
    const int32_t* __restrict__ argmax, const int32_t* __restrict__ labels, const int32_t* __restrict__ ids,
    const float* __restrict__ score, int G, const float* __restrict__ selw, const float* __restrict__ wd,
    float* __restrict__ s_out, float* __restrict__ add, const float* __restrict__ sw) {
  RAU_CHAIN_PRIO();
  const int r = blockIdx.x;
  const int h = r / Bper, b = r - h * Bper;
  const int a = argmax[r];   // 1-based first-max answer of the row
  bool gt;
  if (G > 0) {   // metric score of the answer: the matching non-empty entries' scores, from 0 in entry order
    float sc = 0.f;
    for (int g = 0; g < G; ++g) {
      const size_t e = (size_t)b * G + g;
      const int id = min(max(ids[e], 0), K);
      if (id > 0 && id == a) sc = __fadd_rn(sc, score[e]);
    }
    gt = sc > 0.f;
  } else {
    gt = a == min(max(labels[b], 1), K);   // clamped like k_ce_fwd's labels
  }
  const float t = gt ? 1.f : 0.f;
  const float x = dopred[r];
  const float eps = 1e-12f;
  const float num = -__fsub_rn(t, x);
  const float den = __fmul_rn(__fadd_rn(__fsub_rn(1.f, x), eps), __fadd_rn(x, eps));
  const float wh = __fmul_rn(selw[h], sw ? sw[b] : 1.f);   // one 4-byte load per workgroup
  const float ddp = __fdiv_rn(__fmul_rn(wh, __fdiv_rn(num, den)), (float)Bper);
  const float s = __fmul_rn(__fmul_rn(ddp, x), __fsub_rn(1.f, x));
  if (threadIdx.x == 0) s_out[r] = s;
  for (int m = threadIdx.x; m < M; m += 256) add[(size_t)r * M + m] = __fmul_rn(s, wd[m]);
}

// Columns 0..M-1 are the head's weight gradient, column M (mf == 1) its bias gradient.  A workgroup owns 32
// columns; its 8 row groups take rows rg, rg + 8, .. in ascending order and are then added in group order.
__global__ __launch_bounds__(256) void k_select_wgrad(int rows, int M, const float* __restrict__ s,
    const float* __restrict__ mf, float* __restrict__ dW, float* __restrict__ db) {
  __shared__ float red[8][32];
  const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + c;
  float acc = 0.f;
  if (col < M)
    for (int r = rg; r < rows; r += 8) acc = __fmaf_rn(s[r], mf[(size_t)r * M + col], acc);
  else if (col == M)
    for (int r = rg; r < rows; r += 8) acc = __fadd_rn(acc, s[r]);
  red[rg][c] = acc;
  __syncthreads();
  if (rg != 0 || col > M) return;
  float tot = red[0][c];
  for (int g = 1; g < 8; ++g) tot = __fadd_rn(tot, red[g][c]);
  float* dst = col < M ? dW + col : db;
  *dst = __fadd_rn(*dst, tot);
}

}  // namespace

hipError_t select_signal(hipStream_t st, int rows, int Bper, int K, int M, const float* dopred,
                         const int32_t* argmax, const Truth& t, const float* selw, const float* wd, float* s,
                         float* add) {
  if (rows <= 0) return hipSuccess;
  if (Bper < 1 || rows % Bper || t.G < 0 || t.G > kMaxAnswers || (t.G > 0 ? !t.ids || !t.score : !t.labels))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_select_signal, dim3(rows), dim3(256), 0, st, Bper, K, M, dopred, argmax, t.labels, t.ids,
                     t.score, t.G, selw, wd, s, add, t.sw);
  return hipGetLastError();
}

hipError_t select_wgrad(hipStream_t st, int rows, int M, const float* s, const float* mf, float* dW,
                        float* db) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_select_wgrad, dim3((M + 1 + 31) / 32), dim3(256), 0, st, rows, M, s, mf, dW, db);
  return hipGetLastError();
}

}  // namespace rau

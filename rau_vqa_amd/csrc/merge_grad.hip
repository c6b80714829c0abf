// merge_grad.hip -- the cross-entropies of the two MERGED answer rows as training terms (rau_backward_merged,
// rau_merge_criterion_backward).  feval logs CE(uni row) and CE(select row) (SS:521-557, rau_step_stats' loss[H] and
// loss[H+1]); with merge_w = {w_uni, w_sel} the step's objective gains  w_uni CE(uni) + w_sel CE(select), and this
// kernel adds their gradient to the hop logits' gradient dl [H][B][K]:
//   uni     every hop h receives (w_uni / H) g(uni row)[b,:]                     (the row is the mean of the hop logits)
//   select  hop hsel(b) receives  w_sel g(select row)[b,:]; a row on which no hop fired receives nothing: its select
//           row is the constant zero row.  The gate do_pred > 0.5 is a constant.
// The rows are hop_merge.h's row_val(r = H) / row_val(r = H + 1) under select_hop(force_last = false) -- the feval
// rule, the bits rau_step_stats reads -- and g(row) is the criterion's own gradient at that row, ce_set.hip's
// formulation with every rounding spelled out:
//   g[k] = (expf(row[k] - mx) / den) (W invB), then for g = 0..G-1 in order: if (y_g == k) g[k] -= w_g invB
// (the first matching entry inside the product's fused multiply-add); a label is the set {y} with w = 1, which gives
// k_ce_fwd's  (expf(row[k] - mx) / den) invB - [k == y] invB.  With a sample weight s_b (rau_set_sample_weights) invB is
// __fmul_rn(s_b, 1 / B) in both products, as in the criterion heads; without weights s_b = 1 and it is 1 / B exactly.
// The update of one element, each step rounded once:
//   x = dl[h,b,k];  x = x + (w_uni / H) g_u[k];  if (h == hsel) x = x + w_sel g_s[k]
// A term whose weight is zero is SKIPPED, not added as zero: dl keeps its bits (the sign of a -0 included).
//
// One launch for all hops, one workgroup of kMT threads per sample.  Pass 1 builds the two rows (H loads per
// entry; the H K logits of a sample, 32 KB at H = 8, K = 1000, stay in L2 for pass 2's neighbours) and reduces
// their max and sum of expf(v - max) in the criterion's order (thread-strided, block_sum).  Where 2 K floats fit in
// kMergeLds bytes the rows are kept in LDS and pass 2 reads them back 16 bytes wide; otherwise pass 2 recomputes
// them.  8 KB of LDS at K = 1000 leaves the workgroups per CU to the wave slots, not to the LDS.  Pass 2 is the
// read-modify-write of dl[h,b,:] for every hop that receives a term, 16 bytes per access over the row pitch ld (a
// multiple of 4; K itself where K % 4 == 0).  kRag (ld > K): the last quad's lanes behind K take no term and leave
// as +0; the staged rows sit at pitch ld, so what decides the staging is 2 ld floats.  A workgroup owns its sample's
// rows of dl: no atomics, no scratch in device memory, the same bits on every call.
#include <hip/hip_runtime.h>

#include "common.h"
#include "hop_merge.h"   // kMT, block_sum, block_first_max, row_val, select_hop
#include "kernels.h"

namespace rau {
namespace {

constexpr size_t kMergeLds = 32768;   // bytes of LDS the two staged rows may take: a pitch of up to 4096

template <bool kStage, bool kRag>
__global__ __launch_bounds__(kMT) void k_merge_grad(int H, int B, int K, int ld, const float* __restrict__ logits,
    const float* __restrict__ dopred, const int32_t* __restrict__ labels, const int32_t* __restrict__ ids,
    const float* __restrict__ w, int G, const float* __restrict__ mw_dev, float w_uni, float w_sel,
    float* __restrict__ dl, const float* __restrict__ sw) {
  RAU_CHAIN_PRIO();
  extern __shared__ float4 s_rows4[];   // kStage: the uni row [ld], then the select row [ld]
  __shared__ float s_val[4];
  __shared__ int s_idx[4];
  __shared__ float s_sum[4];
  __shared__ int s_id[kMaxAnswers];      // 0-based answer, -1 = empty entry
  __shared__ float s_w[kMaxAnswers];     // its weight (0 for an empty entry)
  __shared__ float s_wb[kMaxAnswers];    // w * invB
  float* s_rows = reinterpret_cast<float*>(s_rows4);
  const int b = blockIdx.x, tid = threadIdx.x;
  const float wu = mw_dev ? mw_dev[0] : w_uni, ws = mw_dev ? mw_dev[1] : w_sel;
  const int hsel = select_hop(dopred, H, B, b, false);   // feval: the last hop is not forced
  const bool term[2] = {wu != 0.f, ws != 0.f && hsel >= 0};
  if (!term[0] && !term[1]) return;   // uniform over the workgroup
  const size_t hs = (size_t)B * ld;
  const float* lg = logits + (size_t)b * ld;
  const float invB = __fmul_rn(sw ? sw[b] : 1.f, 1.f / (float)B);   // one 4-byte load per workgroup
  const int Gs = G > 0 ? G : 1;   // a label is a set of one entry with weight 1
  if (tid < Gs) {
    int id;
    float wv;
    if (G > 0) {   // ids clamped like ce_set.hip's
      const size_t e = (size_t)b * G + tid;
      id = min(max(ids[e], 0), K);
      wv = id > 0 ? w[e] : 0.f;
    } else {       // clamped like k_ce_fwd's labels
      id = min(max(labels[b], 1), K);
      wv = 1.f;
    }
    s_id[tid] = id - 1;
    s_w[tid] = wv;
    s_wb[tid] = __fmul_rn(wv, invB);
  }
  __syncthreads();
  float W = 0.f;
  for (int g = 0; g < Gs; ++g) W = __fadd_rn(W, s_w[g]);
  const float scale = __fmul_rn(W, invB);
  // ---- pass 1: the rows, their max and softmax denominator in row_ce's order
  float rmx[2] = {0.f, 0.f}, rden[2] = {1.f, 1.f};
  for (int r = 0; r < 2; ++r) {
    if (!term[r]) continue;
    float mx = -INFINITY;
    int ai = 0x7fffffff;
    for (int k = tid; k < K; k += kMT) {
      const float v = row_val(lg, hs, H, H + r, hsel, k);
      if (kStage) s_rows[(size_t)r * ld + k] = v;
      if (v > mx) { mx = v; ai = k; }
    }
    block_first_max(mx, ai, s_val, s_idx);
    float den = 0.f;
    for (int k = tid; k < K; k += kMT)   // (a thread re-reads the entries it staged itself)
      den += expf((kStage ? s_rows[(size_t)r * ld + k] : row_val(lg, hs, H, H + r, hsel, k)) - mx);
    den = block_sum(den, s_sum);   // its barriers also publish the staged row to the workgroup
    rmx[r] = mx;
    rden[r] = den;
  }
  // ---- pass 2: dl[h,b,:] of every hop that receives a term
  const float cu = __fdiv_rn(wu, (float)H);
  float* dlb = dl + (size_t)b * ld;
  for (int k0 = tid * 4; k0 < ld; k0 += kMT * 4) {
    float g[2][4] = {};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (!term[r]) continue;
      float v[4];
      if (kStage) {
        const float4 q = s_rows4[((size_t)r * ld + k0) >> 2];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = row_val(lg, hs, H, H + r, hsel, k0 + j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (kRag && k0 + j >= K) continue;   // a pad lane: no term (g stays 0; what v holds there is not a logit)
        const float e = expf(v[j] - rmx[r]) / rden[r];
        float p = __fmul_rn(e, scale);
        bool hit = false;
        for (int a = 0; a < Gs; ++a)
          if (s_id[a] == k0 + j) {
            p = hit ? __fsub_rn(p, s_wb[a]) : __fmaf_rn(e, scale, -s_wb[a]);
            hit = true;
          }
        g[r][j] = p;
      }
    }
    for (int h = 0; h < H; ++h) {
      const bool sel_here = term[1] && h == hsel;
      if (!term[0] && !sel_here) continue;
      float4* p4 = reinterpret_cast<float4*>(dlb + (size_t)h * hs + k0);
      const float4 q = *p4;
      float x[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (term[0]) x[j] = __fadd_rn(x[j], __fmul_rn(cu, g[0][j]));
        if (sel_here) x[j] = __fadd_rn(x[j], __fmul_rn(ws, g[1][j]));
        if (kRag && k0 + j >= K) x[j] = 0.f;   // the pad leaves as +0
      }
      *p4 = make_float4(x[0], x[1], x[2], x[3]);
    }
  }
}

}  // namespace

hipError_t merge_grad(hipStream_t st, int H, int B, int K, const float* logits, const float* dopred, const Truth& t,
                      const float* mw_dev, float w_uni, float w_sel, float* dl, int ld) {
  if (B <= 0) return hipSuccess;
  if (ld == 0) ld = K;
  if (H < 1 || K < 1 || ld < K || (ld & 3) || t.G < 0 || t.G > kMaxAnswers || (t.G > 0 ? !t.ids || !t.w : !t.labels))
    return hipErrorInvalidValue;
  const size_t rows = (size_t)2 * ld * sizeof(float);   // what is staged: the two rows at the pitch
  const bool stage = rows <= kMergeLds;
#define RAU_MERGE_GRAD(S, R)                                                                                       \
  hipLaunchKernelGGL((k_merge_grad<S, R>), dim3(B), dim3(kMT), S ? rows : 0, st, H, B, K, ld, logits, dopred,      \
                     t.labels, t.ids, t.w, t.G, mw_dev, w_uni, w_sel, dl, t.sw)
  if (ld == K) {
    if (stage) RAU_MERGE_GRAD(true, false);
    else RAU_MERGE_GRAD(false, false);
  } else {
    if (stage) RAU_MERGE_GRAD(true, true);
    else RAU_MERGE_GRAD(false, true);
  }
#undef RAU_MERGE_GRAD
  return hipGetLastError();
}

}  // namespace rau

// cand_rank.hip -- a batch's multiple-choice candidates (rau_set_candidates) against the merged rows of the last
// step-level forward: the ranked candidates of every row (rau_topk_cand) and the MC statistics (rau_cand_stats).  The
// rows are hop_merge.h's (row_val, select_hop): nothing of the merge arithmetic is restated here.
//
// One wave per (row of H+2, sample), four waves per workgroup; lane c < C holds candidate c: its 0-based id, whether
// it is live (non-empty and equal to no earlier entry of the list: a duplicate counts once) and the row's value
// there.  Everything a lane needs of the others travels by wave shuffles in entry order -- no LDS, no barrier, no
// atomics, the same bits on every call:
//   rank   the number of live candidates whose key (hop_merge.h's make_key: larger value first, ties by the lower
//          answer id, NaN last) is above the lane's: live ids are distinct, so the ranks 0 .. nlive-1 are too
//   m      max over the live values;  den = sum of expf(v - m) over the live entries, added from +0 in entry order
//          (cand_head.hip's formulation);  conf = expf(v - m) / den
// k_cand_topk (predict rule: the last hop is forced) writes the k best as ids / score / conf [H+2][B][k]; ranks at and
// behind the live count are id 0, score -inf, conf +0.
// k_cand_stats (feval rule) forms per (row, sample): the restricted criterion of the uni and select rows against the
// kept truth (cand_head.hip's: set entries outside the live candidates are empty entries; softmax or per-answer
// sigmoid), whether the rank-0 candidate is correct (the label, or a positive metric score in the set) and its score
// (labels: 1 when correct).  Rows without a kept entry are unlabelled: loss 0, never correct, score 0.
// k_cand_reduce, one workgroup: means and totals in k_step_stats_reduce's / k_score_totals' fixed orders, so loss[:H]
// is bitwise rau_get_losses.
#include <hip/hip_runtime.h>

#include "common.h"
#include "hop_merge.h"
#include "kernels.h"

namespace rau {
namespace {

struct CandLane {
  int id;        // 0-based answer of this lane's candidate, -1 when the lane holds no live candidate
  float v;       // the row's value there (0 for such a lane)
  int rank;      // live candidates ranked before it
  int nlive;
  float m, den;  // over the live candidates (wave-uniform)
};

// cand: the sample's list [C]; lg / hs / r / hsel: row_val's arguments
__device__ __forceinline__ CandLane cand_lane(const int32_t* __restrict__ cand, int C, int K,
                                              const float* __restrict__ lg, size_t hs, int H, int r, int hsel) {
  const int lane = threadIdx.x & 63;
  const int raw = lane < C ? min(max(cand[lane], 0), K) - 1 : -1;
  bool live = raw >= 0;
  for (int j = 0; j < C; ++j) {
    const int o = __shfl(raw, j, 64);
    if (j < lane && o == raw) live = false;
  }
  CandLane L;
  L.id = live ? raw : -1;
  L.v = live ? row_val(lg, hs, H, r, hsel, raw) : 0.f;
  const uint64_t key = make_key(L.v, L.id);
  L.rank = 0;
  L.nlive = 0;
  L.m = -INFINITY;
  for (int j = 0; j < C; ++j) {
    const int oid = __shfl(L.id, j, 64);
    const float ov = __shfl(L.v, j, 64);
    if (oid < 0) continue;   // wave-uniform
    ++L.nlive;
    L.m = fmaxf(L.m, ov);
    if (make_key(ov, oid) > key) ++L.rank;
  }
  const float e = live ? expf(L.v - L.m) : 0.f;
  L.den = 0.f;
  for (int j = 0; j < C; ++j) {
    const int oid = __shfl(L.id, j, 64);
    const float oe = __shfl(e, j, 64);
    if (oid >= 0) L.den = __fadd_rn(L.den, oe);
  }
  return L;
}

__global__ __launch_bounds__(kMT) void k_cand_topk(int H, int B, int K, int ld, int C, int k,
    const float* __restrict__ logits, const float* __restrict__ dopred, const int32_t* __restrict__ cand,
    int32_t* __restrict__ ids, float* __restrict__ score, float* __restrict__ conf) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= (H + 2) * B) return;   // whole waves
  const int r = wv / B, b = wv % B;
  const size_t hs = (size_t)B * ld;
  const float* lg = logits + (size_t)b * ld;
  const int hsel = select_hop(dopred, H, B, b, true);   // predict rule: >= 0
  const CandLane L = cand_lane(cand + (size_t)b * C, C, K, lg, hs, H, r, hsel);
  const size_t o = (size_t)wv * k;
  if (L.id >= 0 && L.rank < k) {
    ids[o + L.rank] = L.id + 1;
    score[o + L.rank] = L.v;   // the row's value, bit for bit
    conf[o + L.rank] = __fdiv_rn(expf(L.v - L.m), L.den);
  }
  if (lane < k && lane >= L.nlive) {   // behind the live count
    ids[o + lane] = 0;
    score[o + lane] = -INFINITY;
    conf[o + lane] = 0.f;
  }
}

// rowf [2][B] uni / select criterion | rowsc [H+2][B] (floats, contiguous); rowc [H+2][B] correct | lab [B]
__global__ __launch_bounds__(kMT) void k_cand_stats(int H, int B, int K, int ld, int C, int bce,
    const float* __restrict__ logits, const float* __restrict__ dopred, const int32_t* __restrict__ cand,
    const int32_t* __restrict__ labels, const int32_t* __restrict__ ids, const float* __restrict__ w,
    const float* __restrict__ sc, int G, float* __restrict__ rows, int32_t* __restrict__ rowi) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= (H + 2) * B) return;   // whole waves
  const int r = wv / B, b = wv % B;
  const size_t hs = (size_t)B * ld;
  const float* lg = logits + (size_t)b * ld;
  const int hsel = select_hop(dopred, H, B, b, false);   // feval: the last hop is not forced
  const CandLane L = cand_lane(cand + (size_t)b * C, C, K, lg, hs, H, r, hsel);
  // lane g < ng holds set entry g (labels: the one-entry set {(y, 1)} with score 1)
  const int ng = G > 0 ? G : 1;
  int sid = -1;
  float sw_ = 0.f, ssc = 0.f;
  if (lane < ng) {
    if (G > 0) {
      const size_t e = (size_t)b * G + lane;
      const int id = min(max(ids[e], 0), K);
      sid = id - 1;
      sw_ = id > 0 ? w[e] : 0.f;
      ssc = id > 0 ? sc[e] : 0.f;
    } else {
      sid = min(max(labels[b], 1), K) - 1;
      sw_ = 1.f;
      ssc = 1.f;
    }
  }
  // kept truth: an entry whose id is no live candidate becomes an empty entry
  bool in = false;
  for (int j = 0; j < C; ++j) {
    const int oid = __shfl(L.id, j, 64);
    in = in || (sid >= 0 && oid == sid);
  }
  if (!in) { sid = -1; sw_ = 0.f; ssc = 0.f; }
  const bool labelled = __ballot(sid >= 0) != 0ull;
  // the rank-0 candidate (none when the list has no live entry)
  const unsigned long long first = __ballot(L.id >= 0 && L.rank == 0);
  const int a0 = first ? __shfl(L.id, __ffsll((long long)first) - 1, 64) : -1;
  float score0 = 0.f;   // set_score's order: the matching entries' scores added from +0 in entry order
  for (int g = 0; g < ng; ++g) {
    const int gid = __shfl(sid, g, 64);
    const float gs = __shfl(ssc, g, 64);
    if (gid >= 0 && gid == a0) score0 = __fadd_rn(score0, gs);
  }
  float loss = 0.f;
  if (r >= H && labelled) {   // (hop rows: the head's own loss rows are read by the reduction)
    if (!bce) {
      const float lse = L.m + logf(L.den);
      for (int g = 0; g < ng; ++g) {
        const int gid = __shfl(sid, g, 64);
        const float gw = __shfl(sw_, g, 64);
        if (gid >= 0) loss = __fadd_rn(loss, __fmul_rn(gw, lse - row_val(lg, hs, H, r, hsel, gid)));
      }
    } else {
      float t = 0.f;   // bce_target over the kept entries
      for (int g = 0; g < ng; ++g) {
        const int gid = __shfl(sid, g, 64);
        const float gw = __shfl(sw_, g, 64);
        if (gid >= 0 && gid == L.id) t = __fadd_rn(t, gw);
      }
      t = fminf(t, 1.f);
      const float term = L.id >= 0 ? bce_term(L.v, t, expf(-fabsf(L.v))) : 0.f;
      for (int j = 0; j < C; ++j) {
        const int oid = __shfl(L.id, j, 64);
        const float ot = __shfl(term, j, 64);
        if (oid >= 0) loss = __fadd_rn(loss, ot);
      }
    }
  }
  if (lane != 0) return;
  float* rowf = rows;
  float* rowsc = rows + (size_t)2 * B;
  int32_t* rowc = rowi;
  int32_t* lab = rowi + (size_t)(H + 2) * B;
  if (r >= H) rowf[(size_t)(r - H) * B + b] = loss;
  rowsc[(size_t)r * B + b] = labelled ? score0 : 0.f;
  rowc[(size_t)r * B + b] = labelled && score0 > 0.f;
  if (r == 0) lab[b] = labelled;
}

// One workgroup.  out: loss [H+2] | score [H+2] floats, then correct [H+2] | n_lab int32
__global__ __launch_bounds__(kMT) void k_cand_reduce(int H, int B, const float* __restrict__ lossrow,
    const float* __restrict__ rows, const int32_t* __restrict__ rowi, const float* __restrict__ sw,
    float* __restrict__ out) {
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int R = H + 2;
  const float* rowf = rows;
  const float* rowsc = rows + (size_t)2 * B;
  for (int j = wv; j < 2 * R; j += 4) {
    float acc = 0.f;
    if (j < R) {   // k_step_stats_reduce's order: lane-strided over the batch, wave_sum, / B
      for (int b = l; b < B; b += 64)
        acc += j < H ? lossrow[(size_t)j * B + b]
                     : sw ? __fmul_rn(sw[b], rowf[(size_t)(j - H) * B + b]) : rowf[(size_t)(j - H) * B + b];
      acc = wave_sum(acc);
      if (l == 0) out[j] = acc / (float)B;
    } else {       // k_score_totals' order
      for (int b = l; b < B; b += 64) acc += rowsc[(size_t)(j - R) * B + b];
      acc = wave_sum(acc);
      if (l == 0) out[j] = acc;
    }
  }
  int32_t* cnt = reinterpret_cast<int32_t*>(out + 2 * R);
  for (int j = threadIdx.x; j < R + 1; j += kMT) {
    int s = 0;
    for (int b = 0; b < B; ++b) s += rowi[(size_t)j * B + b];
    cnt[j] = s;
  }
}

}  // namespace

hipError_t cand_topk(hipStream_t st, int H, int B, int K, int k, const float* logits, const float* dopred,
                     const int32_t* cand, int C, int32_t* ids, float* score, float* conf, int ld) {
  if (ld == 0) ld = K;
  if (ld < K || C < 1 || C > kMaxCandidates || k < 1 || k > C || !cand) return hipErrorInvalidValue;
  const int waves = (H + 2) * B;
  hipLaunchKernelGGL(k_cand_topk, dim3((waves + 3) / 4), dim3(kMT), 0, st, H, B, K, ld, C, k, logits, dopred, cand,
                     ids, score, conf);
  return hipGetLastError();
}

hipError_t cand_stats(hipStream_t st, int H, int B, int K, const float* logits, const float* dopred,
                      const float* lossrow, const Truth& t, float* rows, int32_t* rowi, float* out, int ld) {
  if (ld == 0) ld = K;
  if (ld < K || t.C < 1 || t.C > kMaxCandidates || !t.cand || !t.present()) return hipErrorInvalidValue;
  if (t.G > 0 && (t.G > kMaxAnswers || !t.ids || !t.w || !t.score)) return hipErrorInvalidValue;
  const int waves = (H + 2) * B;
  hipLaunchKernelGGL(k_cand_stats, dim3((waves + 3) / 4), dim3(kMT), 0, st, H, B, K, ld, t.C, t.bce() ? 1 : 0, logits,
                     dopred, t.cand, t.labels, t.ids, t.w, t.score, t.G, rows, rowi);
  hipLaunchKernelGGL(k_cand_reduce, dim3(1), dim3(kMT), 0, st, H, B, lossrow, rows, rowi, t.sw, out);
  return hipGetLastError();
}

}  // namespace rau

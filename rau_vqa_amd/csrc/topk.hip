// topk.hip -- torch.topk(x, k, 2, true, true) on device rows (rau_dev_topk), and the k best answers
// of every predict_result row of the last step-level forward with their scores and softmax
// confidences (rau_topk; the rows are hop_merge.h's row_val / select_hop, as rau_predict's).
//
// One workgroup of 256 threads per row.  Every entry has a 64-bit key: the high word is the monotone
// unsigned image of the float (-0 canonicalised to +0, NaN below -inf), the low word is
// 0xffffffff - index, so keys are distinct and their order is the TOTAL order of include/rau.h:
// larger value first, equal values by the lower index, NaN last by index.  Rank j is the largest
// key strictly below rank j-1's: k rounds of a strided scan, a wave shuffle tree and four wave
// results through LDS.  There is no exclusion list, duplicates cost nothing, and an index is only
// ever decoded from the key of an entry the scan has visited, so it is in range whatever the row
// holds.  No atomics, fixed reduction order: repeated calls give the same bits.
//
// Rows of up to kStageFloats entries are staged in LDS once, so a round reads LDS only; longer rows
// are re-read (merged rows: recomputed) from global memory in every round.
#include <hip/hip_runtime.h>

#include "common.h"
#include "hop_merge.h"   // order_bits, make_key: the total order's keys
#include "kernels.h"

namespace rau {
namespace {

constexpr int kStageFloats = 4096;   // 16 KiB of LDS per workgroup at the most
constexpr int kHeadBytes = 80;       // s_key [2][4] uint64 | s_sum [4] float; the staged row follows, 16-byte aligned

// The largest key strictly below `prev` over the workgroup; 0 (no entry has that key: it would need
// index 0xffffffff) when there is none.  s_key is one of two alternating slots of four, so one barrier
// per round is enough: a wave can only write a slot again after every wave has passed the next
// round's barrier, that is, after every wave has read it.
template <class Val>
__device__ __forceinline__ uint64_t next_key(Val val, int cols, uint64_t prev, uint64_t* s_key) {
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  uint64_t best = 0;
  for (int c = tid; c < cols; c += kMT) {
    const uint64_t key = make_key(val(c), c);
    if (key < prev && key > best) best = key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t oh = __shfl_xor((uint32_t)(best >> 32), o, 64);
    const uint32_t ol = __shfl_xor((uint32_t)best, o, 64);
    const uint64_t ok = ((uint64_t)oh << 32) | ol;
    if (ok > best) best = ok;
  }
  if (l == 0) s_key[w] = best;
  __syncthreads();
  best = s_key[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (s_key[i] > best) best = s_key[i];
  return best;
}

// The k best entries of one row; row(c) is entry c from global memory.  out_* point at this row's k
// slots (any may be null).  conf: softmax probability in row_ce's formulation -- mx = the row maximum
// (rank 0's value: the first maximum, what block_first_max returns), den = sum of expf(v - mx) in the
// thread-strided order through block_sum, conf = expf(score - mx) / den.
template <class Row>
__device__ __forceinline__ void topk_row(Row row, int cols, int k, bool staged, unsigned char* smem,
                                         float* out_val, int32_t* out_idx, float* out_conf) {
  uint64_t* s_key = reinterpret_cast<uint64_t*>(smem);
  float* s_sum = reinterpret_cast<float*>(smem + 64);
  float* s_row = reinterpret_cast<float*>(smem + kHeadBytes);
  const int tid = threadIdx.x;
  if (staged) {
    for (int c = tid; c < cols; c += kMT) s_row[c] = row(c);
    __syncthreads();
  }
  auto val = [&](int c) { return staged ? s_row[c] : row(c); };
  uint64_t prev = ~0ull;   // above every key: NaN never maps to the top of the high word
  float mx = 0.f, den = 0.f;
  for (int j = 0; j < k; ++j) {
    const uint64_t best = next_key(val, cols, prev, s_key + (j & 1) * 4);
    const uint32_t c = 0xffffffffu - (uint32_t)best;
    // k <= cols, so every round finds an entry; the test keeps the gather in range regardless
    const bool found = best != 0 && c < (uint32_t)cols;
    const float v = found ? val((int)c) : 0.f;   // the entry itself, bit for bit (the key is canonicalised)
    if (out_conf && j == 0) {
      mx = v;
      for (int i = tid; i < cols; i += kMT) den += expf(val(i) - mx);
      den = block_sum(den, s_sum);
    }
    if (tid == 0) {
      if (out_idx) out_idx[j] = found ? (int32_t)c + 1 : 0;
      if (out_val) out_val[j] = v;
      if (out_conf) out_conf[j] = __fdiv_rn(expf(v - mx), den);
    }
    prev = best;
  }
}

__global__ __launch_bounds__(kMT) void k_topk_rows(int cols, int k, int staged, const float* __restrict__ x,
                                                   float* __restrict__ val, int32_t* __restrict__ idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const float* xr = x + (size_t)blockIdx.x * cols;
  const size_t o = (size_t)blockIdx.x * k;
  topk_row([&](int c) { return xr[c]; }, cols, k, staged != 0, smem, val ? val + o : nullptr,
           idx ? idx + o : nullptr, nullptr);
}

// Workgroup r * B + b: row r of {hops, uni, select} of sample b (predict rule: last hop forced, so
// hsel >= 0 and a row where no hop fired cannot occur); outputs [H+2][B][k].
__global__ __launch_bounds__(kMT) void k_topk_merged(int H, int B, int K, int ld, int k, int staged,
    const float* __restrict__ logits, const float* __restrict__ dopred, int32_t* __restrict__ ids,
    float* __restrict__ score, float* __restrict__ conf) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int r = blockIdx.x / B, b = blockIdx.x % B;
  const size_t hs = (size_t)B * ld;   // rows at pitch ld >= K
  const float* lg = logits + (size_t)b * ld;
  const int hsel = select_hop(dopred, H, B, b, true);
  const size_t o = (size_t)blockIdx.x * k;
  topk_row([&](int c) { return row_val(lg, hs, H, r, hsel, c); }, K, k, staged != 0, smem, score + o, ids + o,
           conf + o);
}

inline size_t topk_lds(int cols) { return kHeadBytes + (cols <= kStageFloats ? (size_t)cols * 4 : 0); }

}  // namespace

hipError_t topk_rows(hipStream_t st, const float* x, int rows, int cols, int k, float* val, int32_t* idx) {
  hipLaunchKernelGGL(k_topk_rows, dim3(rows), dim3(kMT), topk_lds(cols), st, cols, k, cols <= kStageFloats ? 1 : 0,
                     x, val, idx);
  return hipGetLastError();
}

hipError_t topk_merged(hipStream_t st, int H, int B, int K, int k, const float* logits, const float* dopred,
                       int32_t* ids, float* score, float* conf, int ld) {
  if (ld == 0) ld = K;
  if (ld < K) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_topk_merged, dim3((H + 2) * B), dim3(kMT), topk_lds(K), st, H, B, K, ld, k,
                     K <= kStageFloats ? 1 : 0, logits, dopred, ids, score, conf);
  return hipGetLastError();
}

}  // namespace rau

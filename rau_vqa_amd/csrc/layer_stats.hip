// layer_stats.hip -- rau_layer_stats: sum of squares, largest magnitude and non-finite count of every layout entry of
// the flat gradient / weight vectors and of the rule's direction, computed on the device; and the update guard
// (rau_set_update_guard), which is the count-only form of the same pass in front of the three update calls.
//
// A memory-bound segmented reduction: 4 bytes per element for the gradients or the weights, 8 more for the direction
// (m and v).  Two launches on the context's stream, no cooperative launch, no atomics.
//
// Work items.  Entry e of a group covers the elements [off_e, off_{e+1}) of the group's flat vector.  It is tiled by
// items of at most kStatChunk elements, item j of the entry being [off_e + j kStatChunk, min(off_e + (j + 1)
// kStatChunk, off_{e+1})): no item crosses an entry.  The table (StatItem, StatEntry; kernels.h) is built on the
// host at the context's first call, lives in device memory and is freed by rau_destroy with the context's other
// allocations.  The layout is fixed for a context's life, and so is the table.
//
// Order of the sums, stated once.  It is a function of the layout alone -- offsets and lengths -- and so the same on
// every call and for every source.
//   Pass 1, k_layer_stats_part: one workgroup of 256 threads per item [s, e).  With a0 = min(s rounded up to a
//   multiple of 4, e) and a1 = max(e rounded down to a multiple of 4, a0), every thread starts from +0 and adds, in
//   this order, the squares of
//     1. the head: element s + t, for t < a0 - s (at most 3 elements, threads 0..2);
//     2. the aligned middle, one 16-byte load per quad: quads a0 / 4 + t, + 256, + 512, .. below a1 / 4, and within a
//        quad its elements in ascending order;
//     3. the tail: element a1 + t, for t < e - a1 (at most 3 elements, threads 0..2).
//   Each square is rounded once and each addition is rounded once (__fmul_rn, __fadd_rn; the Makefile compiles this
//   file with -ffp-contract=off, as it does featnorm.hip).  A non-finite element counts as +0 in the sum and in the
//   maximum, which leaves both unchanged, and as 1 in the integer count.  The 256 partial sums are added in
//   hop_merge.h's block_sum order: wave_sum (6 butterfly levels), then (w0 + w1) + (w2 + w3).  Thread 0 writes the
//   item's partial record with three 16-byte stores.
//   Pass 2, k_layer_stats_finish: per (entry, source), the items' partial sums are added in ascending item order
//   from +0; the maxima and the integer counts are order-free.
//
// Chain length.  The longest chain of additions behind sumsq of an entry of n elements has at most
//     L(n) = 4 ceil(floor(c / 4) / 256) + 2  +  8  +  ceil(n / kStatChunk),      c = min(n, kStatChunk)
// links: the serial additions of one thread (its quads, plus a head and a tail element), the 6 + 2 levels of the
// workgroup tree, and the items of the entry.  L(1) = 11, L(255) = L(256) = L(257) = 15, L(kStatChunk - 1) =
// L(kStatChunk) = 43, L(kStatChunk + 1) = 44, L(3 kStatChunk + 5) = 46.  All terms are non-negative, so against
// the exact sum of the squares the relative error is at most (L(n) + 2) 2^-24: L(n) roundings of sums, one of the
// square, and one for the second-order terms.  rau_vqa_amd/layer_stats.py restates L(n) and the bar for the tests.
//
// Alignment.  The flat vectors start on 256-byte boundaries (hipMalloc), entry offsets are not multiples of 4 and
// attscore's bias is one element, so which elements are head, middle and tail depends on the offsets only.
//
// The direction (RAU_STAT_DIR) is formed per element from the moments as they stand with update_elem.h's operations:
// Adam m / (sqrtf(v) + eps), Adamax m / u, every operation rounded once, by the rule that owns the group's state.
//
// No LDS beyond the reduction scratch (pass 2 stages 64 partial records), no private-memory arrays, no scratch memory
// besides the partial records.
#include <cmath>
#include <vector>

#include "rau_ctx.h"
#include "hop_merge.h"

#pragma clang fp contract(off)

namespace rau {
namespace {

static_assert(sizeof(StatItem) == 16 && sizeof(StatEntry) == 16, "the work table is read 16 bytes at a time");
static_assert(sizeof(rau_layer_stat) == 56, "rau_layer_stat: 6 floats and 4 int64");

struct Acc {
  float s = 0.f, a = 0.f;
  uint32_t c = 0u;
};
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
template <bool COUNT>
__device__ __forceinline__ void acc_elem(Acc& A, float x) {
  const bool fin = finite_bits(x);
  A.c += fin ? 0u : 1u;
  if constexpr (!COUNT) {
    const float xs = fin ? x : 0.f;
    A.s = __fadd_rn(A.s, __fmul_rn(xs, xs));
    A.a = fmaxf(A.a, fabsf(xs));
  }
}
// update_elem.h's direction: adam_elem's m / (sqrtf(v) + eps), adamax_elem's m / u
__device__ __forceinline__ float dir_elem(bool adamax, float m, float v, float eps) {
  return adamax ? __fdiv_rn(m, v) : __fdiv_rn(m, __fadd_rn(sqrtf(v), eps));
}
template <bool COUNT>
__device__ __forceinline__ void acc_quad(Acc& A, const float4& x) {
  acc_elem<COUNT>(A, x.x);
  acc_elem<COUNT>(A, x.y);
  acc_elem<COUNT>(A, x.z);
  acc_elem<COUNT>(A, x.w);
}
__device__ __forceinline__ float block_max(float v, float* s_f) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
  __syncthreads();
  return r;
}
__device__ __forceinline__ uint32_t block_count(uint32_t v, uint32_t* s_u) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_u[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t r = (s_u[0] + s_u[1]) + (s_u[2] + s_u[3]);
  __syncthreads();
  return r;
}

// G, P, D: the sources read; COUNT: the non-finite counts alone
template <bool G, bool P, bool D, bool COUNT>
__global__ void __launch_bounds__(256) k_layer_stats_part(StatSrc S, const StatItem* __restrict__ items,
                                                          uint32_t* __restrict__ partial) {
  __shared__ float s_f[4];
  __shared__ uint32_t s_u[4];
  const StatItem it = items[blockIdx.x];
  const int gi = it.group;
  const bool skip = ((S.skip >> it.entry) & 1ull) != 0;
  const float* __restrict__ g = S.g[gi];
  const float* __restrict__ x = S.x[gi];
  const float* __restrict__ m = S.m[gi];
  const float* __restrict__ v = S.v[gi];
  const bool adamax = S.rule[gi] == RAU_OPT_ADAMAX;
  const float eps = S.eps;
  Acc ag, ap, ad;
  if (!skip) {
    const size_t s = it.start, e = s + it.len;
    const size_t up = (s + 3) & ~(size_t)3, down = e & ~(size_t)3;
    const size_t a0 = up < e ? up : e, a1 = down > a0 ? down : a0;
    const size_t t = threadIdx.x;
    if (t < a0 - s) {
      if constexpr (G) acc_elem<COUNT>(ag, g[s + t]);
      if constexpr (P) acc_elem<COUNT>(ap, x[s + t]);
      if constexpr (D) acc_elem<COUNT>(ad, dir_elem(adamax, m[s + t], v[s + t], eps));
    }
#pragma unroll 4
    for (size_t q = a0 / 4 + t; q < a1 / 4; q += 256) {
      if constexpr (G) acc_quad<COUNT>(ag, reinterpret_cast<const float4*>(g)[q]);
      if constexpr (P) acc_quad<COUNT>(ap, reinterpret_cast<const float4*>(x)[q]);
      if constexpr (D) {
        const float4 m4 = reinterpret_cast<const float4*>(m)[q];
        const float4 v4 = reinterpret_cast<const float4*>(v)[q];
        acc_elem<COUNT>(ad, dir_elem(adamax, m4.x, v4.x, eps));
        acc_elem<COUNT>(ad, dir_elem(adamax, m4.y, v4.y, eps));
        acc_elem<COUNT>(ad, dir_elem(adamax, m4.z, v4.z, eps));
        acc_elem<COUNT>(ad, dir_elem(adamax, m4.w, v4.w, eps));
      }
    }
    if (t < e - a1) {
      if constexpr (G) acc_elem<COUNT>(ag, g[a1 + t]);
      if constexpr (P) acc_elem<COUNT>(ap, x[a1 + t]);
      if constexpr (D) acc_elem<COUNT>(ad, dir_elem(adamax, m[a1 + t], v[a1 + t], eps));
    }
  }
  // a skipped item goes through the same barriers with zeros
  if constexpr (G) {
    if constexpr (!COUNT) { ag.s = block_sum(ag.s, s_f); ag.a = block_max(ag.a, s_f); }
    ag.c = block_count(ag.c, s_u);
  }
  if constexpr (P) {
    if constexpr (!COUNT) { ap.s = block_sum(ap.s, s_f); ap.a = block_max(ap.a, s_f); }
    ap.c = block_count(ap.c, s_u);
  }
  if constexpr (D) {
    if constexpr (!COUNT) { ad.s = block_sum(ad.s, s_f); ad.a = block_max(ad.a, s_f); }
    ad.c = block_count(ad.c, s_u);
  }
  if (threadIdx.x == 0) {
    uint4* out = reinterpret_cast<uint4*>(partial + (size_t)blockIdx.x * kStatPartWords);
    out[0] = make_uint4(__float_as_uint(ag.s), __float_as_uint(ap.s), __float_as_uint(ad.s), __float_as_uint(ag.a));
    out[1] = make_uint4(__float_as_uint(ap.a), __float_as_uint(ad.a), ag.c, ap.c);
    out[2] = make_uint4(ad.c, 0u, 0u, 0u);
  }
}

// Workgroups 0 .. n_out - 1: entry b's record.  The partial records go through LDS 64 at a time; thread k < 9 owns
// word k of the records (sumsq, absmax, count of the three sources) and walks the items in ascending order.
// Workgroups n_out .. n_out + 2: the non-finite counts of one group's items per source (integers: any order).
__global__ void __launch_bounds__(64) k_layer_stats_finish(const StatEntry* __restrict__ entries, int n_out, int gf0,
                                                           int gf1, int gf2, int gf3,
                                                           const uint32_t* __restrict__ partial,
                                                           rau_layer_stat* __restrict__ out,
                                                           int64_t* __restrict__ totals) {
  __shared__ __attribute__((aligned(16))) uint32_t s_p[64 * kStatPartWords];
  const int t = threadIdx.x;
  if ((int)blockIdx.x >= n_out) {
    const int gi = (int)blockIdx.x - n_out;
    const int first = gi == 0 ? gf0 : gi == 1 ? gf1 : gf2, last = gi == 0 ? gf1 : gi == 1 ? gf2 : gf3;
    long long c0 = 0, c1 = 0, c2 = 0;
    for (int i = first + t; i < last; i += 64) {
      const uint32_t* p = partial + (size_t)i * kStatPartWords;
      c0 += p[6];
      c1 += p[7];
      c2 += p[8];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      c0 += __shfl_xor(c0, o, 64);
      c1 += __shfl_xor(c1, o, 64);
      c2 += __shfl_xor(c2, o, 64);
    }
    if (t < 3) totals[t * 3 + gi] = t == 0 ? c0 : t == 1 ? c1 : c2;
    return;
  }
  const StatEntry en = entries[blockIdx.x];
  float f = 0.f;       // threads 0..2 a sum, 3..5 a maximum
  long long c = 0;     // threads 6..8 a count
  for (uint32_t base = 0; base < en.items; base += 64) {
    const uint32_t cnt = en.items - base < 64u ? en.items - base : 64u;
    if ((uint32_t)t < cnt) {
      const uint4* p = reinterpret_cast<const uint4*>(partial + (size_t)(en.first + base + t) * kStatPartWords);
      uint4* d = reinterpret_cast<uint4*>(s_p + t * kStatPartWords);
      d[0] = p[0];
      d[1] = p[1];
      d[2] = p[2];
    }
    __syncthreads();
    if (t < 9)
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t w = s_p[j * kStatPartWords + t];
        if (t < 3) f = __fadd_rn(f, __uint_as_float(w));
        else if (t < 6) f = fmaxf(f, __uint_as_float(w));
        else c += w;
      }
    __syncthreads();
  }
  rau_layer_stat& o = out[blockIdx.x];
  if (t < 3) o.sumsq[t] = f;
  else if (t < 6) o.absmax[t - 3] = f;
  else if (t < 9) o.nonfinite[t - 6] = c;
  else if (t == 9) o.n = (int64_t)en.n;
}

template <bool COUNT>
void launch_part(hipStream_t st, const StatSrc& S, int what, const StatItem* items, int n_items, uint32_t* partial) {
  const dim3 grid(n_items), block(256);
#define RAU_STAT_CASE(w, G, P, D)                                                                          \
  case w:                                                                                                  \
    hipLaunchKernelGGL((k_layer_stats_part<G, P, D, COUNT>), grid, block, 0, st, S, items, partial);       \
    break;
  switch (what) {
    RAU_STAT_CASE(1, true, false, false)
    RAU_STAT_CASE(2, false, true, false)
    RAU_STAT_CASE(3, true, true, false)
    RAU_STAT_CASE(4, false, false, true)
    RAU_STAT_CASE(5, true, false, true)
    RAU_STAT_CASE(6, false, true, true)
    RAU_STAT_CASE(7, true, true, true)
  }
#undef RAU_STAT_CASE
}

}  // namespace

hipError_t layer_stats_part(hipStream_t st, const StatSrc& S, int what, bool count_only, const StatItem* items,
                            int n_items, uint32_t* partial) {
  if (what < 1 || what > 7 || n_items < 1) return hipErrorInvalidValue;
  if (count_only) {
    if (what != RAU_STAT_GRAD) return hipErrorInvalidValue;   // the guard's form: the one that is instantiated
    hipLaunchKernelGGL((k_layer_stats_part<true, false, false, true>), dim3(n_items), dim3(256), 0, st, S, items,
                       partial);
  } else {
    launch_part<false>(st, S, what, items, n_items, partial);
  }
  return hipGetLastError();
}
hipError_t layer_stats_finish(hipStream_t st, const StatEntry* entries, int n_entries, const int group_first[4],
                              const uint32_t* partial, rau_layer_stat* out, int64_t* totals) {
  const int n_out = out ? n_entries : 0;
  hipLaunchKernelGGL(k_layer_stats_finish, dim3(n_out + 3), dim3(64), 0, st, entries, n_out, group_first[0],
                     group_first[1], group_first[2], group_first[3], partial, out, totals);
  return hipGetLastError();
}

}  // namespace rau

namespace {
int stat_entries(const rau_ctx* ctx) {
  return (int)(ctx->grp[0].layout.size() + ctx->grp[1].layout.size() + ctx->grp[2].layout.size());
}
// The work table and the result buffers exist: built from the layout at the first call
int need_table(rau_ctx* ctx) {
  rau_ctx::LayerStats& ls = ctx->ls;
  if (ls.items) return RAU_OK;
  NEED(stat_entries(ctx) <= kStatMaxEntries, "layer statistics: %d layout entries, at most %d", stat_entries(ctx),
       kStatMaxEntries);
  std::vector<StatItem> items;
  std::vector<StatEntry> entries;
  int gfirst[4];
  for (int gi = 0; gi < 3; ++gi) {
    const Group& g = ctx->grp[gi];
    gfirst[gi] = (int)items.size();
    for (size_t li = 0; li < g.layout.size(); ++li) {
      const size_t off = g.layout[li].off, end = li + 1 < g.layout.size() ? g.layout[li + 1].off : g.n;
      StatEntry en;
      en.first = (uint32_t)items.size();
      en.n = end - off;
      for (size_t s = off; s < end; s += kStatChunk) {
        StatItem it;
        it.start = s;
        it.len = (uint32_t)std::min<size_t>(kStatChunk, end - s);
        it.group = (uint16_t)gi;
        it.entry = (uint16_t)entries.size();
        items.push_back(it);
      }
      en.items = (uint32_t)items.size() - en.first;
      entries.push_back(en);
    }
  }
  gfirst[3] = (int)items.size();
  NEED(!items.empty(), "layer statistics: the layout has no elements");
  // the context's kind of allocation: kept through rau_set_batch_size, freed by rau_destroy
  StatItem* d_items = nullptr;
  StatEntry* d_entries = nullptr;
  uint32_t* d_partial = nullptr;
  rau_layer_stat* d_out = nullptr;
  int64_t* d_totals = nullptr;
  if (int rc = dalloc(ctx, &d_items, items.size(), false)) return rc;
  if (int rc = dalloc(ctx, &d_entries, entries.size(), false)) return rc;
  if (int rc = dalloc(ctx, &d_partial, items.size() * kStatPartWords, false)) return rc;
  if (int rc = dalloc(ctx, &d_out, entries.size(), false)) return rc;
  if (int rc = dalloc(ctx, &d_totals, (size_t)9, false)) return rc;
  HIPC(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(StatItem), hipMemcpyHostToDevice, ctx->st));
  HIPC(hipMemcpyAsync(d_entries, entries.data(), entries.size() * sizeof(StatEntry), hipMemcpyHostToDevice,
                      ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));   // the host vectors end with this call
  ls.entries = d_entries;
  ls.partial = d_partial;
  ls.out = d_out;
  ls.totals = d_totals;
  ls.n_items = (int)items.size();
  ls.n_entries = (int)entries.size();
  std::copy(gfirst, gfirst + 4, ls.group_first);
  ls.items = d_items;
  return RAU_OK;
}
StatSrc stat_src(const rau_ctx* ctx, float eps, uint64_t skip) {
  StatSrc S;
  for (int gi = 0; gi < 3; ++gi) {
    const Group& g = ctx->grp[gi];
    S.g[gi] = g.g;
    S.x[gi] = g.w;
    S.m[gi] = g.m;
    S.v[gi] = g.v;
    S.rule[gi] = g.opt_rule;
  }
  S.eps = eps;
  S.skip = skip;
  return S;
}
double stat_elems(const rau_ctx* ctx) { return (double)ctx->grp[0].n + (double)ctx->grp[1].n + (double)ctx->grp[2].n; }

// validation, then the two launches; nothing is launched in an error case
int stats_run(rau_ctx* ctx, int what, float eps) {
  NEED(ctx, "null ctx");
  NEED(what != 0 && (what & ~(RAU_STAT_GRAD | RAU_STAT_PARAM | RAU_STAT_DIR)) == 0,
       "rau_layer_stats: what = %d is not a sum of RAU_STAT_GRAD, RAU_STAT_PARAM, RAU_STAT_DIR", what);
  NEED(std::isfinite(eps) && eps >= 0.f, "rau_layer_stats: eps %g is not finite and >= 0", (double)eps);
  if (what & RAU_STAT_DIR) {
    for (int gi = 0; gi < 3; ++gi)
      if (ctx->grp[gi].adam_t == 0 || !ctx->grp[gi].m)
        return fail(RAU_ERR_STATE, "rau_layer_stats: RAU_STAT_DIR needs the moments, and group %d has had no update "
                    "(t = 0)", gi);
  }
  if (int rc = need_table(ctx)) return rc;
  const rau_ctx::LayerStats& ls = ctx->ls;
  const StatSrc S = stat_src(ctx, eps, 0);
  const double bytes = stat_elems(ctx) * (4.0 * ((what & RAU_STAT_GRAD ? 1 : 0) + (what & RAU_STAT_PARAM ? 1 : 0)) +
                                          (what & RAU_STAT_DIR ? 8.0 : 0.0));
  RUN("layer_stats_part", 0, bytes, layer_stats_part(ctx->st, S, what, false, ls.items, ls.n_items, ls.partial));
  RUN("layer_stats_finish", 0, (double)ls.n_items * kStatPartWords * 4.0,
      layer_stats_finish(ctx->st, ls.entries, ls.n_entries, ls.group_first, ls.partial, ls.out, ls.totals));
  return RAU_OK;
}
}  // namespace

int update_guard(rau_ctx* ctx, bool ex, float* out_norms, int n_norms) {
  if (ctx->guard_mode == RAU_GUARD_OFF) {
    ctx->guard_last_skipped = 0;
    return 0;
  }
  if (int rc = need_table(ctx)) return rc;
  const rau_ctx::LayerStats& ls = ctx->ls;
  uint64_t skip = 0;   // rau_update_ex: a frozen unit's two entries
  if (ex) {
    int e = 0;
    for (int gi = 0; gi < 3; ++gi) {
      const Group& g = ctx->grp[gi];
      for (size_t li = 0; li < g.layout.size(); ++li, ++e)
        if (!g.lopt.empty() && g.lopt[li / 2].lr_scale == 0.f) skip |= 1ull << e;
    }
  }
  const StatSrc S = stat_src(ctx, 0.f, skip);
  RUN("layer_stats_part", 0, stat_elems(ctx) * 4.0,
      layer_stats_part(ctx->st, S, RAU_STAT_GRAD, true, ls.items, ls.n_items, ls.partial));
  RUN("layer_stats_finish", 0, (double)ls.n_items * kStatPartWords * 4.0,
      layer_stats_finish(ctx->st, ls.entries, ls.n_entries, ls.group_first, ls.partial, nullptr, ls.totals));
  int64_t tot[3];
  if (int rc = d2h(ctx, tot, ls.totals, sizeof(tot))) return rc;   // row 0 of totals: the gradients, per group
  if (tot[0] == 0 && tot[1] == 0 && tot[2] == 0) {
    ctx->guard_last_skipped = 0;
    return 0;
  }
  ctx->guard_skipped += 1;
  ctx->guard_last_skipped = 1;
  std::copy(tot, tot + 3, ctx->guard_last_nonfinite);
  if (out_norms)
    for (int i = 0; i < n_norms; ++i) out_norms[i] = std::nanf("");
  return 1;
}

extern "C" {

int rau_layer_stats_count(const rau_ctx* ctx) {
  if (!ctx) return fail(RAU_ERR_INVALID, "null ctx");
  return stat_entries(ctx);
}

int rau_layer_stats_dev(rau_ctx* ctx, int what, float eps, const rau_layer_stat** dev) {
  NEED(ctx && dev, "null argument");
  if (int rc = stats_run(ctx, what, eps)) return rc;
  *dev = ctx->ls.out;
  return RAU_OK;
}

int rau_layer_stats(rau_ctx* ctx, int what, float eps, rau_layer_stat* out) {
  NEED(ctx && out, "null argument");
  if (int rc = stats_run(ctx, what, eps)) return rc;
  return d2h(ctx, out, ctx->ls.out, (size_t)ctx->ls.n_entries * sizeof(rau_layer_stat));
}

int rau_set_update_guard(rau_ctx* ctx, int mode) {
  NEED(ctx, "null ctx");
  NEED(mode == RAU_GUARD_OFF || mode == RAU_GUARD_SKIP, "rau_set_update_guard: unknown mode %d", mode);
  ctx->guard_mode = mode;
  return RAU_OK;
}

int rau_update_guard(rau_ctx* ctx, int* mode, int64_t* skipped, int32_t* last_skipped, int64_t last_nonfinite[3]) {
  NEED(ctx, "null ctx");
  if (mode) *mode = ctx->guard_mode;
  if (skipped) *skipped = ctx->guard_skipped;
  if (last_skipped) *last_skipped = ctx->guard_last_skipped;
  if (last_nonfinite) std::copy(ctx->guard_last_nonfinite, ctx->guard_last_nonfinite + 3, last_nonfinite);
  return RAU_OK;
}

}  // extern "C"

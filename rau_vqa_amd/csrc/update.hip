// update.hip -- rau_update: gradient noise, norm clip and the optimizer rule for all three parameter groups in
// two launches, and the optimizer state's way in and out (include/rau.h "update with a rule and a clip scope").
//
// The update is three bandwidth passes with a grid-wide dependency between them: every element's clip scale
// depends on the norm of all elements.  rau_noise_clip_adam walks that per group with scalar accesses and a
// single-workgroup launch in the middle: nine launches.  Here
//   1. k_upd_noise_sqnorm  grid (kUpdParts, 3): noise into the gradients, kUpdParts partial sums of squares per group
//   2. k_upd_apply         grid (<= kUpdParts, 3): EVERY workgroup first sums the 3 x kUpdParts partials itself
//                          (12 KB out of L2, in finish_norm's order, so all workgroups hold the same bits), then
//                          clips and applies the rule; workgroup (0, g) also writes the norms out
// so the single-workgroup finish is not a launch of its own, and nothing waits on another workgroup: the only
// ordering is the stream's.  No cooperative launch, no float atomics.  blockIdx.y is the group; the groups'
// pointers, lengths, step sizes and noise keys travel by value (UpdGroups).
// x, g, m, v move as float4 where the group's pointers are 16-byte aligned; a group whose length is not a multiple
// of 4 finishes with scalar accesses, and a misaligned group is scalar throughout.  The element order of the
// sums is add_noise_sqnorm's (thread t of workgroup b owns quads b*256 + t + k*kUpdParts*256), and the element
// arithmetic is update_elem.h's, shared with the per-group kernels: RAU_OPT_ADAM with RAU_CLIP_GROUP gives
// rau_noise_clip_adam's bits.
#include <cmath>

#include "rau_ctx.h"
#include "update_elem.h"

namespace rau {
namespace {

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}
template <int RULE>
__device__ __forceinline__ void rule_elem(float gi, float& m, float& v, float& x, float stepsize, float beta1,
                                          float beta2, float eps) {
  if constexpr (RULE == RAU_OPT_ADAM) adam_elem(gi, m, v, x, stepsize, beta1, beta2, eps);
  else adamax_elem(gi, m, v, x, stepsize, beta1, beta2, eps);
}
// Quads first, first + stride, .. of one flat vector: g scaled by sc (and written back when WRITE_G), then the rule.
// vec: all four pointers are 16-byte aligned.  Every access is below n.
template <int RULE, bool WRITE_G, typename GT>
__device__ __forceinline__ void apply_quads(size_t n, float* __restrict__ x, GT* __restrict__ g,
                                            float* __restrict__ m, float* __restrict__ v, bool vec, float sc,
                                            float stepsize, float beta1, float beta2, float eps, size_t first,
                                            size_t stride) {
  for (size_t q = first; q * 4 < n; q += stride) {
    const size_t e = q * 4;
    if (vec && e + 4 <= n) {
      float4 g4 = *reinterpret_cast<const float4*>(g + e);
      float4 m4 = *reinterpret_cast<const float4*>(m + e);
      float4 v4 = *reinterpret_cast<const float4*>(v + e);
      float4 x4 = *reinterpret_cast<const float4*>(x + e);
      g4.x *= sc; g4.y *= sc; g4.z *= sc; g4.w *= sc;
      rule_elem<RULE>(g4.x, m4.x, v4.x, x4.x, stepsize, beta1, beta2, eps);
      rule_elem<RULE>(g4.y, m4.y, v4.y, x4.y, stepsize, beta1, beta2, eps);
      rule_elem<RULE>(g4.z, m4.z, v4.z, x4.z, stepsize, beta1, beta2, eps);
      rule_elem<RULE>(g4.w, m4.w, v4.w, x4.w, stepsize, beta1, beta2, eps);
      if constexpr (WRITE_G) *reinterpret_cast<float4*>(g + e) = g4;
      *reinterpret_cast<float4*>(m + e) = m4;
      *reinterpret_cast<float4*>(v + e) = v4;
      *reinterpret_cast<float4*>(x + e) = x4;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) {
          const float gi = g[e + j] * sc;
          if constexpr (WRITE_G) g[e + j] = gi;
          float mi = m[e + j], vi = v[e + j], xi = x[e + j];
          rule_elem<RULE>(gi, mi, vi, xi, stepsize, beta1, beta2, eps);
          m[e + j] = mi;
          v[e + j] = vi;
          x[e + j] = xi;
        }
    }
  }
}

__global__ void __launch_bounds__(256) k_upd_noise_sqnorm(UpdGroups G, float nstd, float* __restrict__ partial) {
  RAU_CHAIN_PRIO();
  __shared__ float s_sum[4];
  const int gi = blockIdx.y;
  const size_t n = G.n[gi];
  float* __restrict__ g = G.g[gi];
  const uint64_t seed = G.seed[gi];
  const bool vec = ((uintptr_t)g & 15) == 0;
  float acc = 0.f;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q * 4 < n; q += (size_t)gridDim.x * blockDim.x) {
    float z[4];
    noise_quad(q, (uint32_t)gi, seed, nstd, z);
    const size_t e = q * 4;
    if (vec && e + 4 <= n) {
      float4 v = *reinterpret_cast<const float4*>(g + e);
      v.x = noise_elem(v.x, z[0], nstd, acc);
      v.y = noise_elem(v.y, z[1], nstd, acc);
      v.z = noise_elem(v.z, z[2], nstd, acc);
      v.w = noise_elem(v.w, z[3], nstd, acc);
      *reinterpret_cast<float4*>(g + e) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) g[e + j] = noise_elem(g[e + j], z[j], nstd, acc);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[(size_t)gi * kUpdParts + blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

template <int RULE>
__global__ void __launch_bounds__(256) k_upd_apply(UpdGroups G, int global_clip, float clip, float beta1, float beta2,
                                                   float eps, const float* __restrict__ partial,
                                                   float* __restrict__ norms) {
  RAU_CHAIN_PRIO();
  const int gi = blockIdx.y;
  const size_t n = G.n[gi];
  // a workgroup whose first quad lies behind a short group has nothing to do (workgroup 0 writes the norm)
  if (blockIdx.x != 0 && (size_t)blockIdx.x * blockDim.x * 4 >= n) return;
  __shared__ float s_sum[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k) {   // finish_norm's order, per group
    float acc = 0.f;
    for (int i = threadIdx.x; i < kUpdParts; i += 256) acc += partial[k * kUpdParts + i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_sum[k][threadIdx.x >> 6] = acc;
  }
  __syncthreads();
  const float s0 = (s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]);
  const float s1 = (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]);
  const float s2 = (s_sum[2][0] + s_sum[2][1]) + (s_sum[2][2] + s_sum[2][3]);
  const float own = sqrtf(gi == 0 ? s0 : gi == 1 ? s1 : s2);
  const float all = sqrtf((s0 + s1) + s2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    norms[gi] = own;
    if (gi == 0) norms[3] = all;
  }
  const float sc = clip_scale(global_clip ? all : own, clip);
  float *x = G.x[gi], *g = G.g[gi], *m = G.m[gi], *v = G.v[gi];
  apply_quads<RULE, true>(n, x, g, m, v, aligned16(x, g, m, v), sc, G.step[gi], beta1, beta2, eps,
                          blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

__global__ void __launch_bounds__(256) k_adamax_vec(size_t n, float* __restrict__ x, const float* __restrict__ dx,
                                                    float* __restrict__ m, float* __restrict__ u, float stepsize,
                                                    float beta1, float beta2, float eps) {
  apply_quads<RAU_OPT_ADAMAX, false>(n, x, dx, m, u, aligned16(x, dx, m, u), 1.f, stepsize, beta1, beta2, eps,
                                     blockIdx.x * (size_t)blockDim.x + threadIdx.x,
                                     (size_t)gridDim.x * blockDim.x);
}

// workgroups of 256 threads, a quad per thread and round, capped
inline int quad_blocks(size_t n, int cap) {
  const size_t q = (n + 3) / 4, b = (q + 255) / 256;
  return (int)std::min<size_t>(std::max<size_t>(b, 1), (size_t)cap);
}

}  // namespace

hipError_t upd_noise_sqnorm(hipStream_t st, const UpdGroups& G, float nstd, float* partial) {
  hipLaunchKernelGGL(k_upd_noise_sqnorm, dim3(kUpdParts, 3), dim3(256), 0, st, G, nstd, partial);
  return hipGetLastError();
}
hipError_t upd_apply(hipStream_t st, const UpdGroups& G, int rule, bool global_clip, float clip, float beta1,
                     float beta2, float eps, const float* partial, float* norms) {
  const dim3 grid(quad_blocks(std::max(G.n[0], std::max(G.n[1], G.n[2])), kUpdParts), 3);
  if (rule == RAU_OPT_ADAM)
    hipLaunchKernelGGL(k_upd_apply<RAU_OPT_ADAM>, grid, dim3(256), 0, st, G, global_clip ? 1 : 0, clip, beta1, beta2,
                       eps, partial, norms);
  else
    hipLaunchKernelGGL(k_upd_apply<RAU_OPT_ADAMAX>, grid, dim3(256), 0, st, G, global_clip ? 1 : 0, clip, beta1,
                       beta2, eps, partial, norms);
  return hipGetLastError();
}
hipError_t adamax_vec(hipStream_t st, size_t n, float* x, const float* dx, float* m, float* u, float stepsize,
                      float beta1, float beta2, float eps) {
  hipLaunchKernelGGL(k_adamax_vec, dim3(quad_blocks(n, 2048)), dim3(256), 0, st, n, x, dx, m, u, stepsize, beta1,
                     beta2, eps);
  return hipGetLastError();
}

}  // namespace rau

namespace {
bool known_rule(int r) { return r == RAU_OPT_ADAM || r == RAU_OPT_ADAMAX; }
// both moments of a group exist (zero-filled when new)
int need_moments(rau_ctx* ctx, Group& g) {
  if (g.m) return RAU_OK;
  float *m = nullptr, *v = nullptr;
  if (int rc = dalloc(ctx, &m, g.n, false)) return rc;
  if (int rc = dalloc(ctx, &v, g.n, false)) return rc;
  g.m = m;
  g.v = v;
  return RAU_OK;
}
}  // namespace

extern "C" {

void rau_update_opts_default(rau_update_opts* o) {
  if (!o) return;
  o->rule = RAU_OPT_ADAM;
  o->clip_scope = RAU_CLIP_GROUP;
  o->lr = 3e-3f;
  o->mult_lr = 3e-4f;
  o->beta1 = 0.9f;
  o->beta2 = 0.999f;
  o->eps = 1e-8f;
  o->eta = 0.01f;
  o->gamma = 0.55f;
  o->clip = 0.1f;
  o->noise_seed = 0;
}

int rau_update(rau_ctx* ctx, int64_t step_t, const rau_update_opts* o, float* out_norms) {
  NEED(ctx && o, "null argument");
  NEED(known_rule(o->rule), "rau_update: unknown rule %d", o->rule);
  NEED(o->clip_scope == RAU_CLIP_GROUP || o->clip_scope == RAU_CLIP_GLOBAL, "rau_update: unknown clip scope %d",
       o->clip_scope);
  NEED(step_t >= 0 && o->gamma > 0.f && o->eta >= 0.f && o->clip > 0.f, "bad update hyper-parameters");
  for (int gi = 0; gi < 3; ++gi)
    if (ctx->grp[gi].adam_t > 0 && ctx->grp[gi].opt_rule != o->rule)
      return fail(RAU_ERR_STATE, "rau_update: group %d holds the other rule's state (t = %lld); reset it with "
                  "rau_set_opt_state first", gi, (long long)ctx->grp[gi].adam_t);
  for (int gi = 0; gi < 3; ++gi)
    if (int rc = need_moments(ctx, ctx->grp[gi])) return rc;
  // SS:598-599: var = eta / ((step_t+1) * gamma)
  const float nstd = o->eta > 0.f ? std::sqrt(o->eta / ((float)(step_t + 1) * o->gamma)) : 0.f;
  UpdGroups G;
  double elems = 0;
  for (int gi = 0; gi < 3; ++gi) {
    const Group& g = ctx->grp[gi];
    G.x[gi] = g.w;
    G.g[gi] = g.g;
    G.m[gi] = g.m;
    G.v[gi] = g.v;
    G.n[gi] = g.n;
    G.seed[gi] = o->noise_seed + (uint64_t)step_t * 3 + gi;
    const int64_t t = g.adam_t + 1;
    const double bc1 = 1.0 - std::pow((double)o->beta1, (double)t);
    const double bc2 = 1.0 - std::pow((double)o->beta2, (double)t);
    const float group_lr = gi == RAU_GROUP_MULT ? o->mult_lr : o->lr;  // SS:770-772
    G.step[gi] = o->rule == RAU_OPT_ADAM ? (float)(group_lr * std::sqrt(bc2) / bc1) : (float)(group_lr / bc1);
    elems += (double)g.n;
  }
  RUN("upd_noise_sqnorm", 0, elems * 8.0, upd_noise_sqnorm(ctx->st, G, nstd, ctx->upd_part));
  RUN("upd_apply", 0, elems * 28.0,
      upd_apply(ctx->st, G, o->rule, o->clip_scope == RAU_CLIP_GLOBAL, o->clip, o->beta1, o->beta2, o->eps,
                ctx->upd_part, ctx->norms_d));
  for (int gi = 0; gi < 3; ++gi) {
    ctx->grp[gi].adam_t += 1;
    ctx->grp[gi].opt_rule = o->rule;
  }
  if (out_norms) return d2h(ctx, out_norms, ctx->norms_d, 4 * sizeof(float));
  return RAU_OK;
}

int rau_get_opt_state(rau_ctx* ctx, int group, float* m, float* v, int64_t* t, int32_t* rule) {
  NEED(ctx, "null ctx");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  const Group& g = ctx->grp[group];
  float* host[2] = {m, v};
  const float* dev[2] = {g.m, g.v};
  for (int k = 0; k < 2; ++k) {
    if (!host[k]) continue;
    if (dev[k]) HIPC(hipMemcpyAsync(host[k], dev[k], g.n * sizeof(float), hipMemcpyDeviceToHost, ctx->st));
    else std::memset(host[k], 0, g.n * sizeof(float));   // before the first update: zeros, nothing allocated
  }
  HIPC(hipStreamSynchronize(ctx->st));
  if (t) *t = g.adam_t;
  if (rule) *rule = g.opt_rule;
  return RAU_OK;
}

int rau_set_opt_state(rau_ctx* ctx, int group, const float* m, const float* v, int64_t t, int32_t rule) {
  NEED(ctx, "null ctx");
  NEED(group >= 0 && group < 3, "bad group %d", group);
  NEED(known_rule(rule), "rau_set_opt_state: unknown rule %d", rule);
  NEED(t >= 0, "rau_set_opt_state: t = %lld", (long long)t);
  NEED(t == 0 || (m && v), "rau_set_opt_state: t = %lld needs both moment vectors", (long long)t);
  Group& g = ctx->grp[group];
  if (m || v)
    if (int rc = need_moments(ctx, g)) return rc;
  const float* host[2] = {m, v};
  float* dev[2] = {g.m, g.v};
  for (int k = 0; k < 2 && g.m; ++k) {
    if (host[k]) HIPC(hipMemcpyAsync(dev[k], host[k], g.n * sizeof(float), hipMemcpyHostToDevice, ctx->st));
    else HIPC(hipMemsetAsync(dev[k], 0, g.n * sizeof(float), ctx->st));
  }
  HIPC(hipStreamSynchronize(ctx->st));
  g.adam_t = t;
  g.opt_rule = rule;
  return RAU_OK;
}

}  // extern "C"

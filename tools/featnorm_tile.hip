// featnorm_tile.hip -- where the scaling pass of the L2 normalisation takes its second look at the tile from
// (development tool, not part of librau.so).  A stand-alone restatement of featnorm.hip's f32 kernel with the tile
// width as a run-time argument and two forms of the second pass:
//   reread   the shipped form: the scaling pass loads the tile again (from whichever cache still has it);
//   lds      the first pass also parks the tile in LDS (D x QT x 16 bytes of dynamic LDS, at most 160 KB), the
//            scaling pass reads it from there: one read of the map from memory, by construction.
// 256 maps of [D][196] f32, D = 512 and 2048 (bench.py's configs[1] and configs[2]); per variant 3 warm-up launches
// and 20 timed ones between two events; prints microseconds per launch and algorithmic bytes (one read + one write)
// per second, and checks every variant's bits against the library's launcher (rau::l2norm_features).
//   make -C tools featnorm_tile && tools/featnorm_tile
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rau_vqa_amd/csrc/kernels.h"

#define CHECK(e)                                                                        \
  do {                                                                                  \
    hipError_t e_ = (e);                                                                \
    if (e_ != hipSuccess) {                                                             \
      std::fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__); \
      std::exit(1);                                                                     \
    }                                                                                   \
  } while (0)

#pragma clang fp contract(off)
__device__ __forceinline__ float4 sq_add(const float4& a, const float4& x) {
  return make_float4(a.x + x.x * x.x, a.y + x.y * x.y, a.z + x.z * x.z, a.w + x.w * x.w);
}

// thread t: quad blk * QT + t % QT of the row, channel lane t / QT of C; Sp % 4 == 0, no pad columns (S = Sp)
template <bool LDS>
__global__ __launch_bounds__(256) void k_norm_tile(int D, int Sp, int QT, int C, int nblk, const float4* X, float eps,
                                                   float4* xn, float4* nrm) {
  extern __shared__ float4 tile[];   // LDS form: [D][QT], then the 256 partials and 2 x 64 results
  float4* part = tile + (LDS ? (size_t)D * QT : 0);
  float4* nrm_s = part + 256;
  float4* inv_s = nrm_s + 64;
  const int t = threadIdx.x, col = t % QT, ch = t / QT;
  const int map = blockIdx.x / nblk, c0 = (blockIdx.x - map * nblk) * QT + col;
  const int nq = Sp / 4;
  const bool live = ch < C && c0 < nq;
  const size_t m0 = (size_t)map * D * nq;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live)
    for (int d = ch; d < D; d += C) {
      const float4 x = X[m0 + (size_t)d * nq + c0];
      if (LDS) tile[(size_t)d * QT + col] = x;
      acc = sq_add(acc, x);
    }
  part[t] = acc;
  __syncthreads();
  if (ch == 0) {
    float4 tot = part[col];
    for (int k = 1; k < C; ++k) {
      const float4 p = part[k * QT + col];
      tot = make_float4(tot.x + p.x, tot.y + p.y, tot.z + p.z, tot.w + p.w);
    }
    const float4 n = make_float4(__fsqrt_rn(tot.x), __fsqrt_rn(tot.y), __fsqrt_rn(tot.z), __fsqrt_rn(tot.w));
    nrm_s[col] = n;
    inv_s[col] = make_float4(1.f / fmaxf(n.x, eps), 1.f / fmaxf(n.y, eps), 1.f / fmaxf(n.z, eps), 1.f / fmaxf(n.w, eps));
    if (c0 < nq) nrm[(size_t)map * nq + c0] = n;
  }
  __syncthreads();
  if (!live) return;
  const float4 n = nrm_s[col], r = inv_s[col];
  for (int d = ch; d < D; d += C) {
    const float4 x = LDS ? tile[(size_t)d * QT + col] : X[m0 + (size_t)d * nq + c0];
    xn[m0 + (size_t)d * nq + c0] = make_float4(n.x == 0.f ? 0.f : x.x * r.x, n.y == 0.f ? 0.f : x.y * r.y,
                                               n.z == 0.f ? 0.f : x.z * r.z, n.w == 0.f ? 0.f : x.w * r.w);
  }
}

int main() {
  const int n = 256, S = 196, nq = S / 4;
  const float eps = 1e-12f;
  for (int D : {512, 2048}) {
    const size_t elems = (size_t)n * D * S;
    std::vector<float> h(elems);
    unsigned s = 12345u;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = (float)((int)(s >> 8) - (1 << 23)) * (1.f / (1 << 22)); }
    float *X, *Y, *Yref, *N;
    CHECK(hipMalloc(&X, elems * 4)); CHECK(hipMalloc(&Y, elems * 4)); CHECK(hipMalloc(&Yref, elems * 4));
    CHECK(hipMalloc(&N, (size_t)n * S * 4));
    CHECK(hipMemcpy(X, h.data(), elems * 4, hipMemcpyHostToDevice));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
    auto timed = [&](const char* what, auto launch, float* out) {
      for (int i = 0; i < 3; ++i) launch(out);
      CHECK(hipDeviceSynchronize());
      CHECK(hipEventRecord(a, 0));
      for (int i = 0; i < 20; ++i) launch(out);
      CHECK(hipEventRecord(b, 0));
      CHECK(hipEventSynchronize(b));
      CHECK(hipGetLastError());
      float ms = 0;
      CHECK(hipEventElapsedTime(&ms, a, b));
      int same = -1;
      if (out != Yref) {   // every variant sums in its own order: equal bits only where QT is the library's
        std::vector<float> g(elems), r(elems);
        CHECK(hipMemcpy(g.data(), out, elems * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(r.data(), Yref, elems * 4, hipMemcpyDeviceToHost));
        same = std::memcmp(g.data(), r.data(), elems * 4) == 0;
      }
      std::printf("D=%d %-22s %8.1f us  %6.3f TB/s  same_bits_as_library=%d\n", D, what, ms / 20 * 1e3,
                  elems * 8.0 / (ms / 20 * 1e-3) / 1e12, same);
    };
    timed("library", [&](float* out) { CHECK(rau::l2norm_features(0, n, D, S, S, X, RAU_FEAT_F32, eps, out, N)); }, Yref);
    for (int LDS = 0; LDS < 2; ++LDS)
      for (int QT : {4, 7, 13, 17, 25, 49}) {
        const int C = 256 / QT, nblk = (nq + QT - 1) / QT;
        const size_t lds = ((LDS ? (size_t)D * QT : 0) + 256 + 128) * sizeof(float4);
        if (lds > 160 * 1024) continue;
        auto kern = LDS ? k_norm_tile<true> : k_norm_tile<false>;
        CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds));
        char what[64];
        std::snprintf(what, sizeof what, "%s QT=%d C=%d", LDS ? "lds" : "reread", QT, C);
        timed(what, [&](float* out) {
          hipLaunchKernelGGL(kern, dim3(n * nblk), dim3(256), lds, 0, D, S, QT, C, nblk,
                             reinterpret_cast<const float4*>(X), eps, reinterpret_cast<float4*>(out),
                             reinterpret_cast<float4*>(N));
        }, Y);
      }
    CHECK(hipFree(X)); CHECK(hipFree(Y)); CHECK(hipFree(Yref)); CHECK(hipFree(N));
  }
  return 0;
}

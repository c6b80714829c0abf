// xgrad.hip -- the feature-map gradient of the step-level backward (rau_set_feat_grad):
//
//   dX[b, d, s] = sum_h keep_h[b, d, s] * s_x * ( sum_m Wi[m, d] * dZ_h[b, m, s] )
//
// The reference forms this gradient and discards it (SS:579); with the switch on the step path leaves it behind
// for a trainable image side in front of the library.  Two paths:
//
//   k_xgrad_accum  the default, every shape and dtype: an existing GEMM tile forms one hop's product in a temporary
//                  of one hop's size and this pass adds it, masked and scaled, into dX with 16-byte accesses.
//   k_xgrad_fused  RAU_XGRAD_FUSED=1, exact f32, 14 x 14 class (176 < S <= 208, S % 4 == 0, D % 4 == 0).
//                  gemm_sample.hip's tiling: a workgroup owns 128 channel rows x all positions of one sample and
//                  runs v_mfma_f32_16x16x4_f32.  The hops of a launch group are looped INSIDE the workgroup: per
//                  hop a K loop over M into one accumulator set, then a masked, scaled add into a second set, and
//                  after the last hop one 16-byte store per lane (groups behind the backward's first: one
//                  read-modify-write).  No temporary and no pass over the result per hop -- but two sets of
//                  2 x 13 x 4 registers do not fit a 256-register budget: the kernel is compiled for one workgroup
//                  per CU (256 VGPRs + 108-164 AGPRs, one wave per SIMD), runs at 0.37-0.41 of the f32 matrix
//                  peak where the per-sample GEMM runs at 0.53, and loses to the unfused path by 0.39 ms per step at
//                  configs[1]: a concluded negative, kept behind the knob with its tests.
//
//   k_xgrad_accum_img  RAU_FEAT_GRAD_IMAGES on an image-table batch: the accumulate pass per IMAGE.  It reads the same
//                  per-sample product G [B][D][Sp] and writes dT [slots][D][Sp], dT[i] (=, +=) the terms of the
//                  samples that name image i, in ascending sample order.  A workgroup owns (one image slot, 16
//                  channel rows): the image's sample list -- a CSR pair in device memory, built by the batch code
//                  with a stable counting sort -- is uniform over the workgroup and read through scalar loads, and
//                  every access to G and dT is a 16-byte one over a contiguous run of quads.  The launch covers
//                  every image slot of the CAPACITY and reads the lists from memory, so neither the geometry nor an
//                  argument depends on N or on image_of: a captured step replays on any later table batch.  A slot
//                  without samples (an unnamed image, a slot behind N) is written with zeros by the backward's
//                  first launch and left alone by the others.  Per launch 4 B D S + (4 or 8) N D S bytes instead
//                  of (8 or 12) B D S.
//                  Regenerated bits are drawn per QUAD (philox_keep16 of the quad's 16-element block, its nibble),
//                  the generic k_xgrad_accum<2>'s form, not with k_xgrad_accum_gen's wave-cooperative draw.  That
//                  draw needs runs that start on a 16-element block and hold a multiple of four quads; a workgroup's
//                  run here starts at element (b D + d0) S for each sample b of its list, which is on a block only
//                  where D S % 16 == 0, so the per-quad form would have to stay as the fallback anyway.  Drawing a
//                  block four times costs about 80 integer instructions per 16-byte quad and sample, arithmetic
//                  that hides behind the pass's memory traffic.  The bits are the contract: the same function of
//                  (seed, site, step, element) either way.
//
// Keep bits: read from the site's bit-packed mask where it is in memory (caller-supplied, or filled by fill_masks),
// regenerated with philox_keep16 from the same (seed, site, step, element) where the forward drew them inside its
// dropout pass (philox.h: the backward regenerates).  They are never inferred from the masked map: a zero feature
// under a kept bit keeps its gradient.  The hop sum is a fixed-order f32 sum, no atomics.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace rau {

namespace {

// keep bits of elements e .. e+3 (e % 4 == 0) in bits 0..3
template <int KIND>
__device__ __forceinline__ uint32_t keep_nib(const XMask& m, uint64_t seed, uint32_t step, size_t e) {
  if (KIND == 1) return mask_nib(m.bits, e);
  if (KIND == 2) return (philox_keep16(seed, m.site, step, e >> 4, m.thr) >> (uint32_t)(e & 15)) & 0xFu;
  return 0xFu;
}

template <int KIND>
__global__ void k_xgrad_accum(size_t rows, int SL, int Sp, const float4* __restrict__ G,
                              float4* __restrict__ dX, const XMask m, int store) {
  uint64_t seed = m.seed;
  uint32_t step = m.step;
  if (KIND == 2 && m.key) {
    seed = m.key[0];
    step = (uint32_t)m.key[1];
  }
  const int qpr = Sp >> 2;
  const size_t n4 = rows * (size_t)qpr;
  for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < n4; q += (size_t)gridDim.x * blockDim.x) {
    const size_t r = q / qpr;
    const int s = (int)(q - r * qpr) * 4;
    // positions of this quad that exist (pad columns of a pitched map do not)
    const uint32_t valid = s + 4 <= SL ? 0xFu : s < SL ? (1u << (SL - s)) - 1u : 0u;
    uint32_t nib;
    if (KIND == 1 && SL != Sp) {   // the mask is indexed over the logical [.., SL] tensor
      nib = 0;
      for (int i = 0; i < 4; ++i)
        if (s + i < SL) nib |= mask_bit(m.bits, m.e0 + r * SL + s + i) << i;
    } else {
      nib = keep_nib<KIND>(m, seed, step, m.e0 + r * SL + s) & valid;
    }
    const float4 g = G[q];
    float4 o = store ? make_float4(0.f, 0.f, 0.f, 0.f) : dX[q];
    o.x += (nib & 1u) ? g.x * m.scale : 0.f;
    o.y += (nib & 2u) ? g.y * m.scale : 0.f;
    o.z += (nib & 4u) ? g.z * m.scale : 0.f;
    o.w += (nib & 8u) ? g.w * m.scale : 0.f;
    if (!valid) o = make_float4(0.f, 0.f, 0.f, 0.f);
    else if (valid != 0xFu) {
      if (!(valid & 2u)) o.y = 0.f;
      if (!(valid & 4u)) o.z = 0.f;
      if (!(valid & 8u)) o.w = 0.f;
    }
    dX[q] = o;
  }
}

// The regenerate form of the same pass (dense maps, n % 16 == 0, e0 % 16 == 0): one Philox block covers 16
// consecutive elements, so a wave takes 64 blocks -- lane l draws block base + l once -- and moves the data in the
// order memory likes, as k_dropout_features_gen does: in round r lane l handles quad l & 3 of block
// base + 16 r + (l >> 2) and gets the owner's bits by shuffle.  (One Philox per quad, the generic kernel's form,
// draws every block four times.)  Same arithmetic per element: the same bits.
__global__ void k_xgrad_accum_gen(size_t n16, const float4* __restrict__ G, float4* __restrict__ dX, const XMask m,
                                  int store) {
  uint64_t seed = m.seed;
  uint32_t step = m.step;
  if (m.key) {
    seed = m.key[0];
    step = (uint32_t)m.key[1];
  }
  const int l = threadIdx.x & 63, quad = l & 3, sub = l >> 2;
  const size_t blk0 = m.e0 >> 4;
  for (size_t base = blockIdx.x * (size_t)blockDim.x + (threadIdx.x & ~63u); base < n16;
       base += (size_t)gridDim.x * blockDim.x) {
    const size_t mine = base + l < n16 ? base + l : n16 - 1;
    const uint32_t bits = philox_keep16(seed, m.site, step, blk0 + mine, m.thr);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t nib = ((uint32_t)__shfl((int)bits, 16 * r + sub, 64) >> (4 * quad)) & 0xFu;
      const size_t blk = base + 16 * r + sub;
      if (blk >= n16) continue;
      const size_t q = 4 * blk + quad;
      const float4 g = G[q];
      float4 o = store ? make_float4(0.f, 0.f, 0.f, 0.f) : dX[q];
      o.x += (nib & 1u) ? g.x * m.scale : 0.f;
      o.y += (nib & 2u) ? g.y * m.scale : 0.f;
      o.z += (nib & 4u) ? g.z * m.scale : 0.f;
      o.w += (nib & 8u) ? g.w * m.scale : 0.f;
      dX[q] = o;
    }
  }
}

// The per-image form of k_xgrad_accum (file header).  grid = (ceil(D / XIMG_ROWS), image slots); the arithmetic per
// term is k_xgrad_accum's -- keep ? g * scale : 0 rounded once, then added -- with the mask indexed by SAMPLE.
constexpr int XIMG_ROWS = 16;
template <int KIND>
__global__ __launch_bounds__(256) void k_xgrad_accum_img(int D, int SL, int Sp, const float4* __restrict__ G,
                                                         float4* __restrict__ dT,
                                                         const int32_t* __restrict__ img_start,
                                                         const int32_t* __restrict__ img_samples, const XMask m,
                                                         int store) {
  const int img = blockIdx.y;
  const int beg = img_start[img], end = img_start[img + 1];
  if (beg >= end && !store) return;   // nothing to add: the stored value stands
  uint64_t seed = m.seed;
  uint32_t step = m.step;
  if (KIND == 2 && m.key) {
    seed = m.key[0];
    step = (uint32_t)m.key[1];
  }
  const int qpr = Sp >> 2;
  const int d0 = blockIdx.x * XIMG_ROWS;
  const int nq = min(XIMG_ROWS, D - d0) * qpr;
  float4* out = dT + ((size_t)img * D + d0) * qpr;
  for (int ql = threadIdx.x; ql < nq; ql += blockDim.x) {
    const int dr = ql / qpr;
    const int s = (ql - dr * qpr) * 4;
    // positions of this quad that exist (pad columns of a pitched map do not)
    const uint32_t valid = s + 4 <= SL ? 0xFu : s < SL ? (1u << (SL - s)) - 1u : 0u;
    float4 o = store ? make_float4(0.f, 0.f, 0.f, 0.f) : out[ql];
    for (int j = beg; j < end; ++j) {
      const size_t r = (size_t)img_samples[j] * D + d0 + dr;   // the sample's row of G and of the logical mask
      uint32_t nib;
      if (KIND == 1 && SL != Sp) {   // the mask is indexed over the logical [.., SL] tensor
        nib = 0;
        for (int i = 0; i < 4; ++i)
          if (s + i < SL) nib |= mask_bit(m.bits, m.e0 + r * SL + s + i) << i;
      } else {
        nib = keep_nib<KIND>(m, seed, step, m.e0 + r * SL + s) & valid;
      }
      const float4 g = G[r * qpr + (s >> 2)];
      o.x += (nib & 1u) ? g.x * m.scale : 0.f;
      o.y += (nib & 2u) ? g.y * m.scale : 0.f;
      o.z += (nib & 4u) ? g.z * m.scale : 0.f;
      o.w += (nib & 8u) ? g.w * m.scale : 0.f;
    }
    if (!valid) o = make_float4(0.f, 0.f, 0.f, 0.f);
    else if (valid != 0xFu) {
      if (!(valid & 2u)) o.y = 0.f;
      if (!(valid & 4u)) o.z = 0.f;
      if (!(valid & 8u)) o.w = 0.f;
    }
    out[ql] = o;
  }
}

constexpr int XBK = 16, XNCB = 13, XBN = XNCB * 16;   // 208 columns
constexpr int XLDB = XBN + 32;                         // 240 = 16 mod 32
constexpr int XRB = 2, XBM = 64 * XRB;                 // 128 rows: 4 waves x 2 row blocks of 16
constexpr int XLDA = XBM + 16;                         // 144 = 16 mod 32
constexpr int XSTAGE = XBK * (XLDA + XLDB);            // floats per stage

struct XgParams {
  int D, K, S, nB, tiles_m, nh;
  const float* Wi;          // [K][D]
  const float* dZ;          // [nh][nB][K][S]
  float* dX;                // [nB][D][S]
  XMask m;
  int store;
};

template <int KIND>
__global__ __launch_bounds__(256, 1) void k_xgrad_fused(const XgParams P) {
  __shared__ __attribute__((aligned(16))) float smem[2 * XSTAGE];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int lr = l & 15, lq = l >> 4;
  const int nwg = P.tiles_m * P.nB;
  const int id = xcd_remap(blockIdx.x, nwg);      // tiles of one sample share an XCD's L2
  const int tm = id % P.tiles_m, b = id / P.tiles_m;
  const int m0 = tm * XBM;
  const int S = P.S, S4 = S >> 2;
  uint64_t seed = P.m.seed;
  uint32_t step = P.m.step;
  if (KIND == 2 && P.m.key) {
    seed = P.m.key[0];
    step = (uint32_t)P.m.key[1];
  }

  // staging maps (the same every K-step): A = 16 k-rows x 32 float4 of Wi, B = 16 k-rows x S4 float4 of dZ
  constexpr int ACL = XBM / 4, ARS = 256 / ACL;
  const int a_row = tid / ACL, a_c4 = (tid % ACL) * 4;
  const bool a_ok = m0 + a_c4 < P.D;                            // D % 4 == 0
  const float* a_ptr = P.Wi + (size_t)a_row * P.D + m0 + (a_ok ? a_c4 : 0);
  int b_row[4], b_q[4];
  bool b_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int item = tid + i * 256;
    b_row[i] = item / S4;
    b_q[i] = item - b_row[i] * S4;
    b_ok[i] = b_row[i] < XBK;
    if (!b_ok[i]) { b_row[i] = 0; b_q[i] = 0; }
  }
  // zero the pad columns [S, 208) of both B stages once: no load ever writes them
  for (int e = tid; e < 2 * XBK * (XBN - S); e += 256) {
    const int st = e / (XBK * (XBN - S)), r = e % (XBK * (XBN - S));
    smem[st * XSTAGE + XBK * XLDA + (r / (XBN - S)) * XLDB + S + r % (XBN - S)] = 0.f;
  }

  f32x4 sum[XRB][XNCB];
#pragma unroll
  for (int i = 0; i < XRB; ++i)
#pragma unroll
    for (int j = 0; j < XNCB; ++j) sum[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsteps = (P.K + XBK - 1) / XBK;
#pragma unroll 1
  for (int hop = 0; hop < P.nh; ++hop) {
    const float* Zb = P.dZ + ((size_t)hop * P.nB + b) * (size_t)P.K * S;
    f32x4 acc[XRB][XNCB];
#pragma unroll
    for (int i = 0; i < XRB; ++i)
#pragma unroll
      for (int j = 0; j < XNCB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 ra[XRB], rb[4];
    auto load = [&](int T) {
      const int k0 = T * XBK;
#pragma unroll
      for (int i = 0; i < XRB; ++i) {
        const int k = k0 + a_row + ARS * i;
        ra[i] = (a_ok && k < P.K) ? *reinterpret_cast<const float4*>(a_ptr + (size_t)(k0 + ARS * i) * P.D)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + b_row[i];
        rb[i] = (b_ok[i] && k < P.K) ? *reinterpret_cast<const float4*>(Zb + (size_t)k * S + b_q[i] * 4)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    auto store = [&](int stage) {
      float* As = smem + stage * XSTAGE;
      float* Bs = As + XBK * XLDA;
#pragma unroll
      for (int i = 0; i < XRB; ++i)
        *reinterpret_cast<float4*>(As + (a_row + ARS * i) * XLDA + a_c4) = ra[i];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (b_ok[i]) *reinterpret_cast<float4*>(Bs + b_row[i] * XLDB + b_q[i] * 4) = rb[i];
    };
    auto compute = [&](int stage) {
      const float* As = smem + stage * XSTAGE + lq * XLDA + w * 16 * XRB + lr;
      const float* Bs = smem + stage * XSTAGE + XBK * XLDA + lq * XLDB + lr;
#pragma unroll
      for (int kb = 0; kb < XBK / 4; ++kb) {
        float a[XRB], bb[XNCB];
#pragma unroll
        for (int i = 0; i < XRB; ++i) a[i] = As[kb * 4 * XLDA + i * 16];
#pragma unroll
        for (int j = 0; j < XNCB; ++j) bb[j] = Bs[kb * 4 * XLDB + j * 16];
#pragma unroll
        for (int j = 0; j < XNCB; ++j)
#pragma unroll
          for (int i = 0; i < XRB; ++i)
            // dZ as the MFMA's A operand, Wi as its B operand: a lane's 4 registers are 4 consecutive
            // positions of one channel row (gemm_sample.hip)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bb[j], a[i], acc[i][j], 0, 0, 0);
      }
    };
    if (nsteps > 0) {
      load(0);
      store(0);
    }
    __syncthreads();
    for (int T = 0; T + 1 < nsteps; ++T) {
      const int cur = T & 1;
      load(T + 1);
      compute(cur);
      store(cur ^ 1);
      __syncthreads();
    }
    if (nsteps > 0) compute((nsteps - 1) & 1);
    __syncthreads();   // the next hop's first store overwrites stage 0

    // ---- masked, scaled add: accumulator (i, j) register r = (d = m0 + w*32 + i*16 + lr, s = j*16 + 4*lq + r)
    const size_t e_hop = P.m.e0 + (size_t)hop * P.m.hop_stride + (size_t)b * P.D * S;
#pragma unroll
    for (int i = 0; i < XRB; ++i) {
      const int d = m0 + w * 16 * XRB + i * 16 + lr;
      if (d >= P.D) continue;
#pragma unroll
      for (int j = 0; j < XNCB; ++j) {
        const int s = j * 16 + 4 * lq;
        if (s >= S) continue;   // S % 4 == 0: a quad is all valid or all pad
        const uint32_t nib = keep_nib<KIND>(P.m, seed, step, e_hop + (size_t)d * S + s);
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[i][j][r] += ((nib >> r) & 1u) ? acc[i][j][r] * P.m.scale : 0.f;
      }
    }
  }

  float* Xb = P.dX + (size_t)b * P.D * S;
#pragma unroll
  for (int i = 0; i < XRB; ++i) {
    const int d = m0 + w * 16 * XRB + i * 16 + lr;
    if (d >= P.D) continue;
#pragma unroll
    for (int j = 0; j < XNCB; ++j) {
      const int s = j * 16 + 4 * lq;
      if (s >= S) continue;
      float4* p = reinterpret_cast<float4*>(Xb + (size_t)d * S + s);
      float4 v = make_float4(sum[i][j][0], sum[i][j][1], sum[i][j][2], sum[i][j][3]);
      if (!P.store) {
        const float4 o = *p;
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      *p = v;
    }
  }
}

}  // namespace

hipError_t xgrad_accum(hipStream_t st, size_t rows, int SL, int Sp, const float* G, float* dX, const XMask& m,
                       int store) {
  if (Sp % 4 != 0 || SL > Sp || (m.kind == 2 && (SL != Sp || m.e0 % 4 != 0)) || (m.kind == 1 && SL == Sp && m.e0 % 4 != 0))
    return hipErrorInvalidValue;
  const size_t n4 = rows * (size_t)(Sp / 4);
  const size_t want = (n4 + 255) / 256;
  const dim3 grid((unsigned)std::min<size_t>(std::max<size_t>(want, 1), 256 * 16)), block(256);
  const float4* G4 = reinterpret_cast<const float4*>(G);
  float4* X4 = reinterpret_cast<float4*>(dX);
  if (m.kind == 2 && n4 % 4 == 0 && m.e0 % 16 == 0) {
    const size_t n16 = n4 / 4, want16 = (n16 + 255) / 256;
    const dim3 grid16((unsigned)std::min<size_t>(std::max<size_t>(want16, 1), 256 * 16));
    hipLaunchKernelGGL(k_xgrad_accum_gen, grid16, block, 0, st, n16, G4, X4, m, store);
  } else if (m.kind == 2) hipLaunchKernelGGL(k_xgrad_accum<2>, grid, block, 0, st, rows, SL, Sp, G4, X4, m, store);
  else if (m.kind == 1) hipLaunchKernelGGL(k_xgrad_accum<1>, grid, block, 0, st, rows, SL, Sp, G4, X4, m, store);
  else hipLaunchKernelGGL(k_xgrad_accum<0>, grid, block, 0, st, rows, SL, Sp, G4, X4, m, store);
  return hipGetLastError();
}

hipError_t xgrad_accum_img(hipStream_t st, int slots, int D, int SL, int Sp, const float* G, float* dT,
                           const int32_t* img_start, const int32_t* img_samples, const XMask& m, int store) {
  if (Sp % 4 != 0 || SL > Sp || (m.kind == 2 && (SL != Sp || m.e0 % 4 != 0)) || (m.kind == 1 && SL == Sp && m.e0 % 4 != 0))
    return hipErrorInvalidValue;
  if (slots < 1 || slots > 65535 || D < 1 || !img_start || !img_samples) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((D + XIMG_ROWS - 1) / XIMG_ROWS), (unsigned)slots), block(256);
  const float4* G4 = reinterpret_cast<const float4*>(G);
  float4* T4 = reinterpret_cast<float4*>(dT);
  if (m.kind == 2)
    hipLaunchKernelGGL(k_xgrad_accum_img<2>, grid, block, 0, st, D, SL, Sp, G4, T4, img_start, img_samples, m, store);
  else if (m.kind == 1)
    hipLaunchKernelGGL(k_xgrad_accum_img<1>, grid, block, 0, st, D, SL, Sp, G4, T4, img_start, img_samples, m, store);
  else
    hipLaunchKernelGGL(k_xgrad_accum_img<0>, grid, block, 0, st, D, SL, Sp, G4, T4, img_start, img_samples, m, store);
  return hipGetLastError();
}

// on (RAU_XGRAD_FUSED=1, an A/B knob) selects the fused kernel on the shapes it takes; the default is the unfused
// path, which measured faster in the step (LOG.md: 11.85 vs 12.25 ms at configs[1]; one wave per SIMD costs the
// fused tile more than the temporary's traffic costs the other).
bool xgrad_fused_ok(bool on, int D, int M, int S) {
  return on && S % 4 == 0 && S > 176 && S <= XBN && D % 4 == 0 && D > 0 && M > 0;
}

hipError_t xgrad_fused(hipStream_t st, int nh, int nB, int D, int M, int S, const float* dZ, const float* Wi,
                       float* dX, const XMask& m, int store) {
  if (!(S % 4 == 0 && S > 176 && S <= XBN) || D % 4 != 0 || nh < 1 || nB < 1) return hipErrorInvalidValue;
  if (m.kind != 0 && (m.e0 % 4 != 0 || m.hop_stride % 4 != 0)) return hipErrorInvalidValue;
  XgParams P{};
  P.D = D; P.K = M; P.S = S; P.nB = nB; P.nh = nh;
  P.tiles_m = (D + XBM - 1) / XBM;
  P.Wi = Wi; P.dZ = dZ; P.dX = dX;
  P.m = m; P.store = store;
  const dim3 grid(P.tiles_m * nB), block(256);
  if (m.kind == 2) hipLaunchKernelGGL(k_xgrad_fused<2>, grid, block, 0, st, P);
  else if (m.kind == 1) hipLaunchKernelGGL(k_xgrad_fused<1>, grid, block, 0, st, P);
  else hipLaunchKernelGGL(k_xgrad_fused<0>, grid, block, 0, st, P);
  return hipGetLastError();
}

}  // namespace rau

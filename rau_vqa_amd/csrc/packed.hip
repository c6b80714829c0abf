// packed.hip -- packed region rows [sum(counts)][D] -> dense maps [n][D][Sp] (rau_set_batch_packed,
// rau_set_batch_async_packed, rau_bank_put_packed; include/rau.h).  Region feature files hold one row of D values
// per box; the step kernels read channel-major maps padded to Sp positions.  This is the transposition between
// the two, with the zero fill behind each map's count: a byte mover bound by HBM, like bank.hip, in a translation
// unit of its own so that the code object of kernels.hip is the same with and without it.
#include "packed.h"

#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "narrow.h"

namespace rau {

namespace {
// four neighbouring elements of ES bytes each, as one load or store
template <int ES> struct Vec4;
template <> struct Vec4<4> { using type = uint4; };
template <> struct Vec4<2> { using type = uint2; };
template <> struct Vec4<1> { using type = uint32_t; };

__device__ __forceinline__ void elems(const uint4& v, uint32_t* e) { e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; }
__device__ __forceinline__ void elems(const uint2& v, uint32_t* e) {
  e[0] = v.x & 0xffffu; e[1] = v.x >> 16; e[2] = v.y & 0xffffu; e[3] = v.y >> 16;
}
__device__ __forceinline__ void elems(const uint32_t& v, uint32_t* e) {
  e[0] = v & 0xffu; e[1] = (v >> 8) & 0xffu; e[2] = (v >> 16) & 0xffu; e[3] = v >> 24;
}
}  // namespace

// Tile: kPackTileD = 64 channels x kPackTileS = 64 positions of map blockIdx.y, 256 lanes.
//   load   lane (dl = tid % 16, sq = tid / 16) reads rows off + s0 + 4 sq + {0..3}, four channels d0 + 4 dl + {0..3}
//          of each as ONE load (16 / 8 / 4 bytes): 16 neighbouring lanes cover 64 channels, contiguous in `rows`.
//          Rows at or behind the count are not read: their elements are zero.
//   turn   the lane transposes its 4 x 4 elements in registers into four position QUADS (one per channel:
//          positions 4 sq .. 4 sq + 3, narrowed on the way in the f32 -> 16-bit / fp8 form), 16 / 8 / 4 bytes each.
//   LDS    quads go through LDS as 32-bit words: word k of the quad of channel d0 + 4 dl + j, quad column sq, lies
//          in plane k at word (16 j + dl) * kPackPitch + sq.
//   store  lane (sq' = tid % 16, rr = tid / 16 % 4, wave w) reads back the quads of four tile rows per pass and
//          stores each as ONE store of four positions: 16 neighbouring lanes cover 64 positions, contiguous in `out`.
// Pitch: ds_write_b32 / ds_read_b32 bank a word at (word address) % 32 and conflict within a 32-lane half.  With
// kPackPitch = 18 a writing half (dl = 0..15, sq in {2m, 2m+1}) hits banks 18 dl + sq + const: 18 dl mod 32 runs
// through the 16 even residues once, so the 32 banks are all different.  A reading half holds 16 neighbouring quad
// columns of two tile rows; the rows are taken 8 apart (8 * 18 = 144 = 16 mod 32), so they fill banks b .. b+15 and
// b+16 .. b+31.  Neither side conflicts, for every element size, because LDS only ever sees whole words.
// off / cnt: one wave-uniform load each (readfirstlane); offsets into `rows` are formed in 64 bits.
template <int ESI, int ESO, int FT>
__global__ __launch_bounds__(256) void k_unpack_regions(int D, int S, int Sp, const void* __restrict__ rows,
                                                        size_t total_rows, const int32_t* __restrict__ off,
                                                        const int32_t* __restrict__ cnt, void* __restrict__ out) {
  using VI = typename Vec4<ESI>::type;
  using VO = typename Vec4<ESO>::type;
  constexpr int NW = ESO;   // 32-bit words of a quad of four ESO-byte elements
  __shared__ uint32_t tile[NW][kPackTileD * kPackPitch];
  const int i = blockIdx.y;
  const int n = min(max(__builtin_amdgcn_readfirstlane(cnt[i]), 1), S);
  const size_t r0 = (size_t)max(__builtin_amdgcn_readfirstlane(off[i]), 0);
  const int d0 = blockIdx.x * kPackTileD, s0 = blockIdx.z * kPackTileS;
  const int tid = threadIdx.x;
  {
    const int dl = tid & 15, sq = tid >> 4;
    const int d = d0 + 4 * dl;
    uint32_t e[4][4];   // [position][channel]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = s0 + 4 * sq + r;
      VI v = VI();
      if (d < D && s < n && r0 + s < total_rows)
        v = *reinterpret_cast<const VI*>(static_cast<const char*>(rows) + ((r0 + s) * (size_t)D + d) * ESI);
      elems(v, e[r]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t x[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = ESI != ESO ? narrow1<FT>(e[r][j]) : e[r][j];
      const int w = (16 * j + dl) * kPackPitch + sq;
      if (ESO == 4) {
#pragma unroll
        for (int k = 0; k < NW; ++k) tile[k][w] = x[k];
      } else if (ESO == 2) {
        tile[0][w] = x[0] | (x[1] << 16);
        tile[NW - 1][w] = x[2] | (x[3] << 16);
      } else {
        tile[0][w] = x[0] | (x[1] << 8) | (x[2] << 16) | (x[3] << 24);
      }
    }
  }
  __syncthreads();
  {
    const int sq = tid & 15, rr = (tid >> 4) & 3, wv = tid >> 6;
    const int s = s0 + 4 * sq;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int x = wv + 4 * pass;                            // 0..15
      const int row = 8 * rr + (x & 7) + 32 * (x >> 3);       // tile row 16 j + dl: rr and rr + 1 are 8 rows apart
      const int d = d0 + 4 * (row & 15) + (row >> 4);
      if (d >= D || s >= Sp) continue;
      const int w = row * kPackPitch + sq;
      uint32_t q[NW];
#pragma unroll
      for (int k = 0; k < NW; ++k) q[k] = tile[k][w];
      VO* dst = reinterpret_cast<VO*>(static_cast<char*>(out) + (((size_t)i * D + d) * (size_t)Sp + s) * ESO);
      if constexpr (ESO == 4) *dst = make_uint4(q[0], q[1], q[2], q[NW - 1]);
      else if constexpr (ESO == 2) *dst = make_uint2(q[0], q[NW - 1]);
      else *dst = q[0];
    }
  }
}

hipError_t unpack_regions(hipStream_t st, int n_maps, int D, int S, int Sp, const void* rows, size_t total_rows,
                          const int32_t* off, const int32_t* cnt, void* out, int src_type, int dst_type) {
  if (n_maps <= 0 || n_maps > 65535 || D <= 0 || D % 4 != 0 || S <= 0 || S > Sp || Sp % 4 != 0 || !rows || !off ||
      !cnt || !out || !feat_type_ok(src_type) || !feat_type_ok(dst_type))
    return hipErrorInvalidValue;
  if (src_type != dst_type && src_type != RAU_FEAT_F32) return hipErrorInvalidValue;
  const dim3 grid((D + kPackTileD - 1) / kPackTileD, n_maps, (Sp + kPackTileS - 1) / kPackTileS);
  if (grid.z > 65535) return hipErrorInvalidValue;
#define RAU_UNPACK(ESI, ESO, FT)                                                                              \
  hipLaunchKernelGGL((k_unpack_regions<ESI, ESO, FT>), grid, dim3(256), 0, st, D, S, Sp, rows, total_rows, off, \
                     cnt, out)
  if (src_type == dst_type) {
    switch (feat_elem_bytes(dst_type)) {
      case 4: RAU_UNPACK(4, 4, RAU_FEAT_F32); break;
      case 2: RAU_UNPACK(2, 2, RAU_FEAT_F32); break;
      default: RAU_UNPACK(1, 1, RAU_FEAT_F32); break;
    }
  } else {
    switch (dst_type) {
      case RAU_FEAT_F16: RAU_UNPACK(4, 2, RAU_FEAT_F16); break;
      case RAU_FEAT_BF16: RAU_UNPACK(4, 2, RAU_FEAT_BF16); break;
      case RAU_FEAT_E4M3: RAU_UNPACK(4, 1, RAU_FEAT_E4M3); break;
      default: RAU_UNPACK(4, 1, RAU_FEAT_E5M2); break;
    }
  }
#undef RAU_UNPACK
  return hipGetLastError();
}

}  // namespace rau

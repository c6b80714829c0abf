// packed.h -- packed region rows -> dense feature maps (packed.hip; rau_set_batch_packed, rau_bank_put_packed).
// A header of its own so that kernels.h, and with it the code object of kernels.hip, stays as it is.
#ifndef RAU_PACKED_H
#define RAU_PACKED_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rau {

// One workgroup moves a tile of kPackTileD channels x kPackTileS positions of one map; tests/test_packed_host.py
// holds its table of edge cases to these three numbers.
constexpr int kPackTileD = 64;
constexpr int kPackTileS = 64;
constexpr int kPackPitch = 18;   // LDS words per tile row of kPackTileS / 4 position quads (see packed.hip)

// out[i][d][s] = rows[off[i] + s][d] for s < cnt[i], all bits zero for cnt[i] <= s < Sp; i < n_maps, d < D.
// rows: total_rows x D elements of src_type, row-major (one region per row); out: n_maps maps [D][Sp] of dst_type
// (Sp % 4 == 0, S <= Sp, D % 4 == 0).  dst_type == src_type moves the elements as they are (4, 2 or 1 bytes);
// src_type == RAU_FEAT_F32 into a narrower dst_type narrows on the way (narrow.h: the bits of rau_bank_put).
// off / cnt are DEVICE arrays the host has checked; the kernel clamps cnt into [1, S] and never reads a row at
// or beyond total_rows all the same.  Every element of the n_maps maps is written, pad columns included.
hipError_t unpack_regions(hipStream_t st, int n_maps, int D, int S, int Sp, const void* rows, size_t total_rows,
                          const int32_t* off, const int32_t* cnt, void* out, int src_type, int dst_type);

}  // namespace rau

#endif  // RAU_PACKED_H

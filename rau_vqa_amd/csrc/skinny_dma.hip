// skinny_dma.hip -- split-K partial products of the recurrence's Linear GEMMs (LSTM gates, hop
// projections, their input gradients): C[M,N] = A[M,K] W^T (W stored [N][K]) or A[M,K] W (W stored
// [K][N]), M = batch (<= 256), N 512..2048, K 512..2048.  Reference ops: model/DeepLSTM.lua:29-65
// (i2h / h2h Linear), train_vqa_RAU_SS.lua:448-462, 581-596 (encoder forward / backward through time).
//
// These launches sit on the step's critical path, ~100 per step, 14 us alone / 28 us in
// the step with the register-staged 64x64x16 single-stage tile of gemm_core.h (one global round
// trip and two barriers per 16-deep K-step; every XCD fetching all of W through the fabric).  Here:
//  * operands go HBM/L2 -> LDS by DMA (global_load_lds_dwordx4) into a ring of KNST stages, one
//    barrier per stage, fragments of stage s+1 read while stage s's MFMAs run.  KNST = 2: in the
//    step a 4-slot ring measures the same and an 8-slot ring +0.5 ms -- the workgroups must fit next
//    to the resident bulk tiles, and the request queue of the bulk kernels' own DMA, not this
//    kernel's prefetch depth, sets the latency a stage sees;
//  * work item g = (problem, K split, tile column, tile row) in that order, dealt to the XCDs in
//    contiguous runs (workgroup L -> XCD L & 7 -> items [ (L & 7) * per, ... )), so that one XCD
//    works on one K slice (or a column range of it): each L2 fetches its slice of W once;
//  * the LDS image is DMA's lane-linear one; the XOR swizzle that makes the fragment reads
//    conflict-free is applied on the GLOBAL side (which 16 bytes a lane fetches), not the LDS side.
// Output: raw partial sums to the slab [split][M][N]; lin_reduce_epilogue / the LSTM cell kernels
// add them in split order (deterministic), exactly as for the tile this replaces.
//
// ONE kernel template on the stage depth (NH = 16-deep halves per stage):
//  * NH = 1, 16-deep stages: 16 KB of LDS, 36 registers -- the f32 256-sample step, where the bulk
//    stream is the longer path and the recurrence's footprint beside the bulk tiles is what counts;
//  * NH = 2, 32-deep stages: a stage is 128 bytes of every [row][k] operand row (whole lines, 8
//    pieces under an 8-column XOR swizzle) and two MFMA k-groups, so a workgroup passes half as many
//    waits and barriers per K; 32 KB and 90 registers.  Stand-alone 10-18 % faster on the recurrence's
//    shapes (tools/linbench); in the step it pays where the recurrence is the longer path (bf16 mode
//    -1.1 %, 64-sample contexts -1.9 %, evaluate-mode forward +1.5-3.5 %) and costs the f32 256-sample
//    step 0.9 %, so the caller chooses per launch (LinMode::deep, computed by lin_mode() in rau_ctx.h from
//    chain_bound(); K % 64 != 0 keeps NH = 1).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace rau {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

constexpr int KT = 64;            // tile rows and columns
constexpr int KNST = 2;           // ring slots (power of two)

struct SkinnyParams {
  int M, K, nprob, splits, nst;   // nst = K-steps per split (even)
  int tiles_m, tiles_n;           // tiles_n of the widest problem
  const float* A[3]; const float* B[3];
  int N[3]; long off[3];          // problem p: N[p] columns, partials at slab + off[p] ([split][M][N[p]])
  long lda, ldb;
  float* slab;
};

template <int OFF>
__device__ __forceinline__ void lds_read128(f32x4& dst, uint32_t addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read32(float& dst, uint32_t addr) {
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}

// 16-byte column swizzle of the [row][16 NH k] image.  NH = 1 (64-byte rows): the four rows a
// ds_read_b128 lane group takes on one 64-byte bank quarter get four different columns.  NH = 2
// (128-byte rows, 8 pieces): piece p of row r sits in column p ^ ((r >> 1) & 7), so the sixteen rows a
// lane group takes at one k-group hit sixteen different 16-byte bank groups.
template <int NH>
__device__ __forceinline__ int kc_swz(int row) {
  return NH == 1 ? ((-((row & 15) >> 2)) & 3) : ((row >> 1) & 7);
}

// "s_waitcnt lgkmcnt(0)" that every fragment register of `set` depends on
template <bool BRC, int NH>
__device__ __forceinline__ void frags_landed(f32x4 (&af)[2][NH], f32x4 (&bq)[2][NH], float (&bs)[2][4 * NH]) {
  if constexpr (NH == 1) {
    if constexpr (!BRC)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(af[0][0]), "+v"(af[1][0]), "+v"(bq[0][0]), "+v"(bq[1][0]) : : "memory");
    else
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(af[0][0]), "+v"(af[1][0]), "+v"(bs[0][0]), "+v"(bs[0][1]), "+v"(bs[0][2]), "+v"(bs[0][3]),
                     "+v"(bs[1][0]), "+v"(bs[1][1]), "+v"(bs[1][2]), "+v"(bs[1][3])
                   :
                   : "memory");
  } else {
    if constexpr (!BRC)
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[1][0]), "+v"(af[1][1]),
                     "+v"(bq[0][0]), "+v"(bq[0][1]), "+v"(bq[1][0]), "+v"(bq[1][1])
                   :
                   : "memory");
    else
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(af[0][0]), "+v"(af[0][1]), "+v"(af[1][0]), "+v"(af[1][1]),
                     "+v"(bs[0][0]), "+v"(bs[0][1]), "+v"(bs[0][2]), "+v"(bs[0][3]),
                     "+v"(bs[0][4]), "+v"(bs[0][5]), "+v"(bs[0][6]), "+v"(bs[0][7]),
                     "+v"(bs[1][0]), "+v"(bs[1][1]), "+v"(bs[1][2]), "+v"(bs[1][3]),
                     "+v"(bs[1][4]), "+v"(bs[1][5]), "+v"(bs[1][6]), "+v"(bs[1][7])
                   :
                   : "memory");
  }
}

// The 4 NH reduction indices a lane holds of one 16-row block and stage, rounded to bf16 (RNE) and packed
// as one operand of v_mfma_f32_16x16x{16,32}_bf16.  Both operands of a product hold the same indices in the
// same order (k = 16 h + 4 (l >> 4) + e at position 4 h + e), which is all the instruction asks for.
template <int NH>
__device__ __forceinline__ auto pack_k(const float (&v)[4 * NH]) {
  if constexpr (NH == 1) {
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
    return o;
  } else {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
    return o;
  }
}

// What a DMA piece that lies outside its operand fetches instead (RAG kernels): sixteen zero bytes.
__device__ __attribute__((aligned(16))) float g_zero_piece[4] = {0.f, 0.f, 0.f, 0.f};

// BRC = false: W stored [N][K] (k contiguous);  true: W stored [K][N] (n contiguous)
// NH: 16-deep halves per stage (1 or 2)
// RAG: ragged shapes -- K any multiple of 4 (attprob's 196 positions, the 200-wide embedding) and, for
//      [K][N] weights, N any multiple of 4: the reduction runs over ceil(K / stage) stages (an even number
//      per split), and every 16-byte piece that starts at k >= K (or at a column >= N) is fetched from
//      g_zero_piece instead, so the staged image holds zeros there (never a neighbouring row's values,
//      never bytes behind the operand)
// BF: both operands rounded to bf16 in registers, bf16 MFMA with f32 accumulation (rau_dtype RAU_BF16: the
//     recurrence's gate / projection GEMMs, BASELINE.json configs[2]); the staging is the f32 one unchanged
template <bool BRC, int NH, bool BF, bool RAG>
__global__ __launch_bounds__(256, BF ? 4 : 1) void k_skinny_dma(const SkinnyParams P) {
  constexpr int KBK = 16 * NH;          // K-step per stage
  constexpr int KPART = KT * KBK;       // floats per operand per stage (4 / 8 KB)
  constexpr int KSTAGE = 2 * KPART;
  constexpr int PPR = 4 * NH;           // 16-byte pieces per [row][k] operand row
  RAU_CHAIN_PRIO();
  __shared__ __attribute__((aligned(16))) float smem[KNST * KSTAGE];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w & 1, wn = w >> 1;

  // ---- work item
  const int tiles = P.tiles_m * P.tiles_n;
  const int total = P.nprob * P.splits * tiles;
  int g = blockIdx.x;
  if ((total & 7) == 0) g = (g & 7) * (total >> 3) + (g >> 3);
  const int tm = g % P.tiles_m;
  g /= P.tiles_m;
  const int tn = g % P.tiles_n;
  g /= P.tiles_n;
  const int split = g % P.splits, prob = g / P.splits;
  const int PN = P.N[prob];
  const int m0 = tm * KT, n0 = tn * KT;
  if (n0 >= PN) return;                      // narrower problem of a merged launch (whole workgroup)
  const int nk = RAG ? (P.K + KBK - 1) / KBK : P.K / KBK;
  const int s0 = split * P.nst;
  int nst = nk - s0;
  if (nst <= 0) return;
  if (RAG || nst > P.nst) nst = P.nst;      // RAG: always the even count; stages past K stage zeros

  // ---- DMA sources: NH 16-byte pieces of each operand per lane and stage (pieces tid + 256 j)
  const char *ga[NH], *gb[NH];
  long stepb;
  int ka[NH], kb[NH];          // RAG: first reduction index of the piece within its stage
  bool colok[NH];              // RAG, [K][N] weights: the piece's columns lie inside N
#pragma unroll
  for (int j = 0; j < NH; ++j) {
    const int p = tid + 256 * j, row = p / PPR, c = (p % PPR) ^ kc_swz<NH>(row);
    ka[j] = c * 4; kb[j] = c * 4; colok[j] = true;
    int r = m0 + row;
    if (r > P.M - 1) r = P.M - 1;            // rows past M: a duplicate, never stored
    ga[j] = reinterpret_cast<const char*>(P.A[prob] + (long)r * P.lda + (long)s0 * KBK + c * 4);
    if (!BRC) {
      int n = n0 + row;
      if (n > PN - 1) n = PN - 1;
      gb[j] = reinterpret_cast<const char*>(P.B[prob] + (long)n * P.ldb + (long)s0 * KBK + c * 4);
      stepb = KBK * 4;
    } else {
      const int k = p >> 4, cc = (p & 15) ^ (((k >> 2) & 1) << 2);
      gb[j] = reinterpret_cast<const char*>(P.B[prob] + ((long)s0 * KBK + k) * P.ldb + n0 + cc * 4);
      stepb = (long)KBK * P.ldb * 4;
      kb[j] = k; colok[j] = n0 + cc * 4 < PN;
    }
  }
  int issued = 0;
  const char* const zero_piece = reinterpret_cast<const char*>(g_zero_piece);
  auto issue = [&]() {   // next stage, into ring slot issued % KNST
    float* dst = smem + (issued & (KNST - 1)) * KSTAGE + w * 256;
    const int kbase = (s0 + issued) * KBK;
#pragma unroll
    for (int j = 0; j < NH; ++j) {
      const char* sa = ga[j];
      const char* sb = gb[j];
      if constexpr (RAG) {
        if (kbase + ka[j] >= P.K) sa = zero_piece;
        if (kbase + kb[j] >= P.K || !colok[j]) sb = zero_piece;
      }
      __builtin_amdgcn_global_load_lds((glb_ptr_t)sa, (lds_ptr_t)(dst + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_ptr_t)sb, (lds_ptr_t)(dst + KPART + j * 1024), 16, 0, 0);
      ga[j] += KBK * 4;
      gb[j] += stepb;
    }
    ++issued;
  };

  // ---- fragment addresses (bytes, stage 0).  Lane (r = l & 15, kk = l >> 4): MFMA e (0..3) of the
  // stage's half h holds k = 16 h + 4 kk + e: one ds_read_b128 per 16-row block and half covers it
  // for [row][k] operands (piece kk + 4 h of the row); [k][n] operands take a ds_read_b32 per MFMA
  // and block.
  const int fr = l & 15, kk = l >> 4;
  const uint32_t lds0 = (uint32_t)(size_t)(lds_ptr_t)smem;
  uint32_t fa[2][NH], fb[2][NH];   // [block][half]
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ra = wm * 32 + i * 16 + fr;
#pragma unroll
    for (int h = 0; h < NH; ++h)
      fa[i][h] = lds0 + (uint32_t)(ra * (KBK * 4) + (((kk + 4 * h) ^ kc_swz<NH>(ra)) << 4));
    if (!BRC) {
      const int rb = wn * 32 + i * 16 + fr;
#pragma unroll
      for (int h = 0; h < NH; ++h)
        fb[i][h] = lds0 + (uint32_t)(KPART * 4 + rb * (KBK * 4) + (((kk + 4 * h) ^ kc_swz<NH>(rb)) << 4));
    } else {
      const int nb = (wn * 32 + i * 16 + fr) ^ ((kk & 1) << 4);
#pragma unroll
      for (int h = 0; h < NH; ++h)
        fb[i][h] = lds0 + (uint32_t)(KPART * 4 + (4 * kk * 64 + nb) * 4) + h * (16 * 64 * 4);
    }
  }

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // [set][block][half]; element e = MFMA e's value.  [k][n] operands: scalars, so that each
  // ds_read_b32 lands in the register the MFMA reads (no compiler-made copy ahead of the wait)
  f32x4 af[2][2][NH], bq[2][2][NH];
  float bs[2][2][4 * NH];

  auto read_frags = [&](int set, int slot) {
    const uint32_t so = (uint32_t)slot * (KSTAGE * 4);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      lds_read128<0>(af[set][0][h], fa[0][h] + so);
      lds_read128<0>(af[set][1][h], fa[1][h] + so);
      if constexpr (!BRC) {
        lds_read128<0>(bq[set][0][h], fb[0][h] + so);
        lds_read128<0>(bq[set][1][h], fb[1][h] + so);
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          lds_read32<0>(bs[set][j][4 * h + 0], fb[j][h] + so);
          lds_read32<256>(bs[set][j][4 * h + 1], fb[j][h] + so);
          lds_read32<512>(bs[set][j][4 * h + 2], fb[j][h] + so);
          lds_read32<768>(bs[set][j][4 * h + 3], fb[j][h] + so);
        }
      }
    }
  };
  // this wave's pieces of every issued stage but the newest have landed (a two-slot ring: the stage
  // about to be read is always the oldest one in flight)
  auto wait_landed = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

  // ---- prologue: stage 0 in flight, then its fragments in set 0 with stage 1 on its way
  issue();
  wait_landed();
  __builtin_amdgcn_s_barrier();
  if (issued < nst) issue();
  read_frags(0, 0);

  auto body = [&](auto set_tag, int s) {
    constexpr int set = decltype(set_tag)::value;
    const bool more = s + 1 < nst;
    if (more) wait_landed();
    // fragments of stage s are in registers (every consumer below depends on this wait)
    frags_landed<BRC, NH>(af[set], bq[set], bs[set]);
    __builtin_amdgcn_sched_barrier(0);
    // stage s+1 is visible to all; every wave is done with stage s's slot
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (issued < nst) issue();
    if (more) read_frags(set ^ 1, (s + 1) & (KNST - 1));
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!BF) {
#pragma unroll
      for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  af[set][i][h][e], BRC ? bs[set][j][4 * h + e] : bq[set][j][h][e], acc[i][j], 0, 0, 0);
    } else {
      float va[2][4 * NH], vb[2][4 * NH];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            va[i][4 * h + e] = af[set][i][h][e];
            vb[i][4 * h + e] = BRC ? bs[set][i][4 * h + e] : bq[set][i][h][e];
          }
      const auto a0 = pack_k<NH>(va[0]), a1 = pack_k<NH>(va[1]), b0 = pack_k<NH>(vb[0]), b1 = pack_k<NH>(vb[1]);
      if constexpr (NH == 1) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a0), __builtin_bit_cast(s16x4, b0), acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a0), __builtin_bit_cast(s16x4, b1), acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a1), __builtin_bit_cast(s16x4, b0), acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a1), __builtin_bit_cast(s16x4, b1), acc[1][1], 0, 0, 0);
      } else {
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll 1
  for (int s = 0; s < nst; s += 2) {
    body(std::integral_constant<int, 0>{}, s);
    body(std::integral_constant<int, 1>{}, s + 1);
  }

  // ---- partial sums to the slab: D[row 4 (l >> 4) + r][col l & 15]
  float* C = P.slab + P.off[prob] + (long)split * P.M * PN;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm * 32 + i * 16 + 4 * kk + r;
      if (m < P.M) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = n0 + wn * 32 + j * 16 + fr;
          if (n < PN) C[(long)m * PN + n] = acc[i][j][r];
        }
      }
    }
}

}  // namespace

// Which form a launch takes: 32-deep stages where the caller says the recurrence is the longer path
// (LinMode::deep) and K allows it, else 16-deep stages.
static int stage_depth(int deep, int K) { return (deep && K % 64 == 0) ? 32 : 16; }

// Ragged shapes (the RAG kernels): K not a whole even number of stages, or [K][N] weights whose N is not
// a multiple of the 64-column tile.  Without LinMode::ragged they go to the register-staged tile as in
// rounds 1-3.
static bool ragged(int deep, int K, bool brc, int nprob, const int* N) {
  if (K % (2 * stage_depth(deep, K)) != 0) return true;
  if (brc)
    for (int p = 0; p < nprob; ++p)
      if (N[p] % KT != 0) return true;
  return false;
}

bool skinny_dma_ok(LinMode mode, int M, int K, long lda, long ldb, bool brc, int nprob, const int* N,
                   const float* const* A, const float* const* B) {
  if (!mode.dma || M < 1 || nprob < 1 || nprob > 3) return false;
  if (K < 4 || (K & 3) || (lda & 3) || (ldb & 3)) return false;
  if (ragged(mode.deep, K, brc, nprob, N)) {
    if (!mode.ragged) return false;
    for (int p = 0; p < nprob; ++p)
      if (brc && (N[p] & 3)) return false;         // pieces are all inside or all outside a row
  }
  for (int p = 0; p < nprob; ++p) {
    if (N[p] < 1) return false;
    // global_load_lds_dwordx4 takes any dword-aligned global address (checked with tools/linbench: same
    // results, same speed); the flat parameter vector puts every weight behind attscore's 1 x A + 1 block
    // one float off a 16-byte boundary, and rounds 1-3 sent all of those GEMMs to the register-staged tile.
    // LinMode::align16 restores that.
    const uintptr_t am = mode.align16 ? 15 : 3;
    if ((reinterpret_cast<uintptr_t>(A[p]) & am) || (reinterpret_cast<uintptr_t>(B[p]) & am)) return false;
  }
  return true;
}

// K splits: about one workgroup per CU (256), an even number of K-steps per split
int skinny_dma_splits(int deep, int M, int K, int tiles_all, size_t cols_all, size_t slab_floats) {
  const int depth = stage_depth(deep, K);
  const int nk = (K + depth - 1) / depth;
  int s = (256 + tiles_all / 2) / tiles_all;   // 160 .. 512 measured equal in the step
  if (s > nk / 2) s = nk / 2;
  if (s < 1) s = 1;
  while (s > 1 && (size_t)s * M * cols_all > slab_floats) --s;
  int per = (nk + s - 1) / s;
  per += per & 1;
  return (nk + per - 1) / per;
}

hipError_t skinny_dma(hipStream_t st, LinMode mode, bool brc, int nprob, int M, int K,
                      const float* const* A, long lda, const float* const* B, long ldb, const int* N,
                      float* slab, const long* off, int splits) {
  const int depth = stage_depth(mode.deep, K);
  const bool rag = ragged(mode.deep, K, brc, nprob, N);
  if (splits < 1 || nprob < 1 || nprob > 3 || (K & 3)) return hipErrorInvalidValue;
  SkinnyParams P{};
  P.M = M; P.K = K; P.nprob = nprob; P.splits = splits;
  const int nk = (K + depth - 1) / depth;
  int per = (nk + splits - 1) / splits;
  per += per & 1;
  P.nst = per;
  if ((long)per * splits < nk) return hipErrorInvalidValue;
  int nmax = 0;
  for (int p = 0; p < nprob; ++p) {
    P.A[p] = A[p]; P.B[p] = B[p]; P.N[p] = N[p]; P.off[p] = off[p];
    nmax = N[p] > nmax ? N[p] : nmax;
  }
  P.tiles_m = (M + KT - 1) / KT;
  P.tiles_n = (nmax + KT - 1) / KT;
  P.lda = lda; P.ldb = ldb; P.slab = slab;
  const dim3 grid(nprob * splits * P.tiles_m * P.tiles_n), block(256);
  auto go = [&](auto brc_t, auto nh_t, auto bf_t) {
    if (rag)
      hipLaunchKernelGGL((k_skinny_dma<decltype(brc_t)::value, decltype(nh_t)::value, decltype(bf_t)::value, true>),
                         grid, block, 0, st, P);
    else
      hipLaunchKernelGGL((k_skinny_dma<decltype(brc_t)::value, decltype(nh_t)::value, decltype(bf_t)::value, false>),
                         grid, block, 0, st, P);
  };
  auto by_bf = [&](auto brc_t, auto nh_t) {
    if (mode.bf16) go(brc_t, nh_t, std::true_type{});
    else go(brc_t, nh_t, std::false_type{});
  };
  auto by_nh = [&](auto brc_t) {
    if (depth == 32) by_bf(brc_t, std::integral_constant<int, 2>{});
    else by_bf(brc_t, std::integral_constant<int, 1>{});
  };
  if (brc) by_nh(std::true_type{});
  else by_nh(std::false_type{});
  return hipGetLastError();
}

}  // namespace rau

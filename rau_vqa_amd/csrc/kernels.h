// kernels.h -- host-callable launchers of the HIP kernels (internal to librau.so).
// Every launcher enqueues on `st` and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rau.h"   // rau_feat_type

namespace rau {

// ------------------------------------------------ split-K partials: fail closed (split_guard.hip)
// Consumers of K-split partials read slab[split][..] for split < nsplit with no bound of their own.
// Their launchers check the span first: inside ONE registered workspace, count in [1, kMaxSplits]
// (0 = no partials, always fine); on violation they launch nothing and return kSplitStateError.
constexpr long kMaxSplits = 4096;
constexpr hipError_t kSplitStateError = hipErrorIllegalState;
void split_ws_register(const float* base, size_t floats);
void split_ws_unregister(const float* base);
bool split_span_ok(const float* slab, long nsplit, size_t per_split_floats);

// ------------------------------------------------------------ GEMM (gemm_lin.hip)
// How a Linear product is formed: an argument of every launch, computed by the caller from its context at call
// time (lin_mode, rau_ctx.h) -- there is no per-thread or per-process state behind these GEMMs.
//  bf16: rau_dtype RAU_BF16 (BASELINE.json configs[2]: "bf16 MFMA gate/classifier GEMMs"): forward y = x W^T,
//        input gradient dx = dy W and weight gradient dW += dy^T x, whichever kernel serves them, round both
//        operands to bf16 (round to nearest even) and accumulate in f32.  skinny_dma.hip does it with bf16 MFMAs;
//        the register-staged fallback tiles round while staging and keep the f32 MFMA (same products, another
//        summation order).
//  deep: skinny_dma.hip's stages are 32-deep where K % 64 == 0 (else 16-deep).  The depth also decides which
//        shapes count as ragged and how many K splits a launch makes, i.e. the summation order.
//  dma, ragged, align16: which problems skinny_dma.hip takes at all (skinny_dma_ok): none / no ragged shapes /
//        only operands on 16-byte boundaries; the others keep the register-staged tile of gemm_core.h.
struct LinMode { int bf16 = 0; int deep = 0; int dma = 1; int ragged = 1; int align16 = 0; };
struct LinOpts {
  const float* bias = nullptr;    // + bias[n]
  const float* bias2 = nullptr;   // + bias2[n]
  const float* addend = nullptr;  // + addend[m*add_rs + n]
  long add_rs = 0;
  int accumulate = 0;             // + C_old
  int act = 0;                    // 1: tanh
  const float* ymul = nullptr;    // * (1 - y^2)
  long y_rs = 0;
  const uint32_t* emask = nullptr;  // dropout on the output (bit index e0 + m*N + n)
  size_t emask_e0 = 0;
  float emscale = 1.f;
  float alpha = 1.f;
  // split-K workspace: when given, skinny problems are split over K across
  // workgroups (partials to slab, then one fused reduce + epilogue kernel)
  float* slab = nullptr;
  size_t slab_floats = 0;
  // deferred reduction: leave the K-split partials in `slab` ([splits][M*N]) and
  // report the split count; the consumer kernel (lstm_fwd / lstm_bwd) sums them
  int* defer_splits = nullptr;
  LinMode mode;
};
// C[M,N] = epi(A[M,K] * W[N,K]^T)      (Linear forward)
hipError_t gemm_nt(hipStream_t st, int M, int N, int K, const float* A, long lda,
                   const float* W, long ldw, float* C, long ldc, const LinOpts& o);
// C[M,N] = epi(A[M,K] * W[K,N])        (Linear input gradient)
hipError_t gemm_nn(hipStream_t st, int M, int N, int K, const float* A, long lda,
                   const float* W, long ldw, float* C, long ldc, const LinOpts& o);
// nb (<= 3) same-shape problems C_i = A_i W_i^T (nt) / A_i W_i (nn) in one launch; the
// K-split partials stay in `slab` as [problem][split][M*N] (*splits per problem) for a
// consumer kernel to sum -- used by the encoder's layer wavefront.
hipError_t gemm_nt_batched_deferred(hipStream_t st, LinMode mode, int nb, int M, int N, int K,
                                    const float* const* A, long lda, const float* const* W,
                                    long ldw, float* slab, size_t slab_floats, int* splits);
hipError_t gemm_nn_batched_deferred(hipStream_t st, LinMode mode, int nb, int M, int N, int K,
                                    const float* const* A, long lda, const float* const* W,
                                    long ldw, float* slab, size_t slab_floats, int* splits);
// nb (<= 3) Linear forwards x W_i^T that share x (and K) but differ in width, one launch;
// problem i's partials at slab + off[i] as [*splits][M][N[i]]
hipError_t gemm_nt_hetero_deferred(hipStream_t st, LinMode mode, int nb, int M, int K, const float* A,
                                   long lda, const float* const* W, long ldw, const int* N, float* slab,
                                   size_t slab_floats, int* splits, size_t* off);
// C[M,N] += A[K,M]^T * B[K,N]          (Linear weight gradient; deterministic split-K
// through `slab`, which must hold gemm_tn_slab_floats(M,N,K) floats)
size_t gemm_tn_slab_floats(int M, int N, int K);
// dbias (optional): dbias[m] += sum_k A[k, m], from the same pass over A (Linear bias gradient)
// bf16 != 0 (LinMode::bf16): both operands rounded to bf16 (RNE) while staged, f32 accumulate; dbias is
// summed from the UNROUNDED values
hipError_t gemm_tn_acc(hipStream_t st, int M, int N, int K, const float* A, long lda,
                       const float* B, long ldb, float* C, long ldc, float* slab,
                       float* dbias = nullptr, int bf16 = 0);

// All the Linear weight gradients of a parameter group as ONE grouped launch (+ one reduction):
// C_p[M_p,N_p] += A_p[K,M_p]^T B_p[K,N_p], dbias_p[m] += sum_k A_p[k,m]; C_p dense (ldc = N_p).
struct TnProblem {
  int M, N; const float* A; long lda; const float* B; long ldb; float* C; float* dbias;
};
size_t gemm_tn_group_slab_floats(const TnProblem* pr, int np, int K);
hipError_t gemm_tn_group_acc(hipStream_t st, const TnProblem* pr, int np, int K, float* slab,
                             size_t slab_floats, int bf16 = 0);

// ----------------------------------------------------------- conv GEMMs (gemm_conv.hip)
// I[b,m,s] = tanh(sum_d Wi[m,d] * X'[b,d,s] + bi[m])   (reference SS:238-242; X' is the
// feature map with dropout already applied, see dropout_features; nB may be H*B)
// bf16 != 0 (rau_dtype RAU_BF16) on the five hop-batched conv GEMMs: operands rounded to bf16
// while staged into LDS, f32 accumulate (v_mfma_f32_32x32x16_bf16); tensors in HBM stay f32.
// How a conv product is formed: an argument of every launcher and of every predicate that sizes a buffer for one,
// computed by the caller from its context (conv_mode, policy.h) -- the same record at both places.
struct ConvMode {
  int bf16 = 0;          // rau_dtype: 0 exact f32, 1 bf16-rounded operands, 2 split operands
  int one_per_cu = 0;    // forward convs: cap residency at one workgroup per CU
  int light = 0;         // conv_att_dgrad_dz: the caller's recurrence is the longer path, keep the f32 product on the
                         // 176-register tile instead of dgrad_dma's 240 (two per CU)
  int wide = 3;          // forward convs on the wide tiling: 1 i_embed, 2 ifeatproj
  int wide_per_cu = 1;   // ... its workgroups per CU (1 | 2)
  int sample = 12;       // products on the per-sample tiling (conv_sample_ok's `which`)
  int dgrad_ring = 3;    // dgrad_dma.hip: 0 off, else its ring depth (2 | 3)
  int wgrad_dma = 1, wgrad16 = 1;   // wgrad_dma.hip / wgrad16.hip on (else their register-staged predecessors)
  int wgrad_groups = 0;  // wgrad_dma.hip's wave groups per workgroup (1 | 2), 0 = by shape
};
hipError_t conv_embed_fwd(hipStream_t st, const ConvMode& cm, int nB, int D, int S, int M, const float* X,
                          const float* WiT /* [D][M] */, const float* bi, float* I);
// RAU_BF16 mode with the feature maps stored as bf16 (X16 [nB][D][S] bf16; S % 4 == 0)
hipError_t conv_embed_fwd_b16(hipStream_t st, int nB, int D, int S, int M, const void* X16,
                              const void* WiT16, const float* bi, float* I);
// ifeatproj in RAU_BF16 mode with the transposed weight pre-converted (WpT16 [M][A] bf16)
hipError_t conv_att_pre_b16(hipStream_t st, int nB, int M, int S, int A, const float* I,
                            const void* WpT16, const float* bp, float* Pout);
// P[b,k,s] = sum_m Wp[k,m] I[b,m,s] + bp[k]   (hop-invariant half of SS:244-252)
hipError_t conv_att_pre(hipStream_t st, const ConvMode& cm, int nB, int M, int S, int A, const float* I,
                        const float* WpT /* [M][A] */, const float* bp, float* P);
// Same three products with one sample per tile (gemm_sample.hip), used for 14 x 14 maps:
// C[b,m,s] = epi(sum_k Wt[k,m] X[b,k,s]); epi 0: act(. + bias[m]), epi 1: . + dj[b,m] a[b,s]
// which: 1 = i_embed forward, 2 = ifeatproj forward, 4 = attention dgrad, 8 = i_embed dgrad (ConvMode::sample)
bool conv_sample_ok(const ConvMode& cm, int S, int which);
hipError_t conv_sample(hipStream_t st, int epi, int nB, int M, int K, int S, const float* Wt,
                       long w_rs, const float* X, long x_bs, float* C, long c_bs,
                       const float* bias, int act, const float* dj, const float* av,
                       const float* Y = nullptr, float* rs = nullptr, int c16 = 0);
// Wide tiling for 14 x 14 maps (conv_wide.hip, round 3): 64 rows x four whole samples per tile,
// operands staged by LDS-DMA; epi 0 / 2 as conv_sample's.  nB must be a multiple of 4.
bool conv_wide_ok(int M, int K, int S, long w_rs);
hipError_t conv_wide(hipStream_t st, int epi, int nB, int M, int K, int S, const float* Wt, long w_rs,
                     const float* X, long x_bs, float* C, long c_bs, const float* bias, int act,
                     const float* dj, const float* av, const float* Y, float* rs, int c16, int per_cu);
// out[c][r] = in[r][c]  (rows x cols -> cols x rows); used once per step on the two
// 1x1-conv weights so the forward conv GEMMs get a row-contiguous A operand
hipError_t transpose2d(hipStream_t st, int rows, int cols, const float* in, float* out,
                       void* out16 = nullptr);   // out16: a bf16 copy of out (RAU_BF16 mode)
// dI[b,m,s] = sum_k Wp[k,m] dS[b,k,s] + dj[b,m] a[b,s]   (gradient at i_embed's output)
hipError_t conv_att_dgrad(hipStream_t st, const ConvMode& cm, int nB, int M, int S, int A, const float* dS,
                          const float* Wp, const float* dj, const float* a, float* dI);
// Same product with the gradient through i_embed's tanh and the bias-gradient row sums in its
// epilogue: dZ[b,m,s] = (sum_k Wp[k,m] dS[b,k,s] + dj[b,m] a[b,s]) (1 - I[b,m,s]^2),
// rs[b,m] = sum_s dZ[b,m,s].  Only where the per-sample tiling applies (conv_dz_fused_ok): the
// i_embed weight gradient then takes dZ with its plain operand loader (dz_final below).
bool conv_dz_fused_ok(const ConvMode& cm, int S, int M);
hipError_t conv_att_dgrad_dz(hipStream_t st, const ConvMode& cm, int nB, int M, int S, int A, const float* dS,
                             const float* Wp, const float* dj, const float* a, const float* I,
                             float* dZ, float* rs, int dz16 = 0,    // dz16: dZ stored as bf16
                             int ds16 = 0);   // RAU_BF16 mode: dS points at bf16 elements (dgrad16 only)
// RAU_BF16 mode, 14 x 14 maps, M % 128 == 0, K % 32 == 0 (dgrad16.hip): the product above with both GEMM
// operands rounded to bf16 while staged, f32 accumulate and epilogue; C = dZ as f32 or bf16 elements
bool dgrad16_ok(int M, int K, int S, long w_rs);
hipError_t dgrad16(hipStream_t st, int nB, int M, int K, int S, const float* Wt, long w_rs,
                   const void* X, long x_bs, void* C, long c_bs, const float* dj, const float* av,
                   const float* Y, float* rs, int c16, int x16 = 0 /* X stored as bf16 */);
// f32 mode, 14 x 14 maps, M % 128 == 0, K % 16 == 0 (dgrad_dma.hip, round 4): the same product and epilogue on
// per-sample tiles with both operands staged by LDS-DMA; bitwise the results of conv_sample's EPI 2
bool dgrad_dma_ok(const ConvMode& cm, int M, int K, int S, long w_rs);
hipError_t dgrad_dma(hipStream_t st, const ConvMode& cm, int nB, int M, int K, int S, const float* Wt, long w_rs,
                     const float* X, long x_bs, float* C, long c_bs, const float* dj, const float* av,
                     const float* Y, float* rs);
// dWp += sum dS I^T in RAU_BF16 mode with dS stored as bf16 (att_bwd_fused's dS16), I f32
hipError_t conv_att_wgrad_ds16(hipStream_t st, int nB, int M, int S, int A, const void* dS16,
                               const float* I, float* dWp, float* slab);
// dX'[b,d,s] = sum_m Wi[m,d] dZ[b,m,s]   (dead in feval, SS:579; module-level API only)
hipError_t conv_embed_dgrad(hipStream_t st, const ConvMode& cm, int nB, int D, int S, int M, const float* dZ,
                            const float* Wi, float* dX);
// The same product in the context's dtype, for the step path's feature-map gradient: cm.bf16 != 0 rounds both
// operands while they are staged (Wi from its f32 storage, dZ from f32 or, dz16, from its bf16 storage)
hipError_t conv_embed_dgrad_mode(hipStream_t st, const ConvMode& cm, int nB, int D, int S, int M, const void* dZ,
                                 int dz16, const float* Wi, float* dX);
// ---- feature-map gradient of the step path (xgrad.hip)
// Where hop h's keep bits of site RAU_MASK_X come from.  kind 0: no mask (scale 1); 1: `bits`, indexed over the
// logical [.., SL] tensor from element e0; 2: regenerated with philox_keep16 from (seed, site, step) -- read from
// `key` (device: seed, step) when it is set -- for the elements from e0 on (logical == physical layout).
struct XMask {
  int kind;
  const uint32_t* bits;
  size_t e0, hop_stride;   // first element of the first hop; elements per hop
  uint64_t seed; uint32_t site, step, thr; const uint64_t* key;
  float scale;
};
// dX[r][s] = (store ? 0 : dX[r][s]) + keep[r][s] * scale * G[r][s] for rows r < rows of pitch Sp (Sp % 4 == 0), pad
// columns s >= SL written as zeros; one hop (the mask's first)
hipError_t xgrad_accum(hipStream_t st, size_t rows, int SL, int Sp, const float* G, float* dX, const XMask& m,
                       int store);
// The same pass per IMAGE of a table: dT[i][d][s] = (store ? 0 : dT[i][d][s]) + sum over the samples b of
// img_samples[img_start[i] .. img_start[i + 1]), in that order, of keep[b][d][s] * scale * G[b][d][s], for the image
// slots i < slots (an empty list: zeros under store, else untouched).  G [.][D][Sp], dT [slots][D][Sp]; the lists are
// DEVICE arrays ([slots + 1], [samples]) read by the kernel: no argument depends on their contents.
hipError_t xgrad_accum_img(hipStream_t st, int slots, int D, int SL, int Sp, const float* G, float* dT,
                           const int32_t* img_start, const int32_t* img_samples, const XMask& m, int store);
// Exact f32, 14 x 14 class (xgrad_fused_ok): dX[b] (store ? = : +=) sum_{h < nh} keep_h * scale * Wi^T dZ_h[b] with
// the hop loop inside the workgroup.  dZ [nh][nB][M][S] f32, Wi [M][D].
bool xgrad_fused_ok(bool on /* the caller's policy: off = the unfused path */, int D, int M, int S);
hipError_t xgrad_fused(hipStream_t st, int nh, int nB, int D, int M, int S, const float* dZ, const float* Wi,
                       float* dX, const XMask& m, int store);
// dWp[k,m] += sum_{b,s} dS[b,k,s] I[b,m,s]   and, with dZ = dI (1 - I^2),
// dWi[m,d] += sum_{b,s} dZ[b,m,s] X'[b,d,s]
size_t conv_wgrad_slab_floats(int nB, int rowsA, int rowsB, int S);
// bf16-operand i_embed weight gradient on 14 x 14 maps, 256 x 256 tiles fed by LDS-DMA
// (wgrad16.hip, round 3): dW[ra][rb] += sum_{b,s} A16[b][ra][s] B16[b][rb][s], operands bf16 in HBM
// (a_bs / b_bs in elements).  _ok: cm.wgrad16, S == 196, ra and rb multiples of 256; else the 128 x 128
// register-staged tile.  The slab must hold wgrad16_slab_floats() of the same mode.
bool wgrad16_ok(const ConvMode& cm, int ra, int rb, int S);
size_t wgrad16_slab_floats(const ConvMode& cm, int nB, int ra, int rb, int S);
hipError_t wgrad16(hipStream_t st, const ConvMode& cm, int nB, int ra, int rb, int S, const void* A16, long a_bs,
                   const void* B16, long b_bs, float* dW, float* slab);
// Split-K partials of the recurrence's skinny Linear GEMMs with LDS-DMA operand staging
// (skinny_dma.hip, round 3): nprob (<= 3) problems C_p = A_p W_p^T (brc = false, W [N][K]) or
// A_p W_p (brc = true, W [K][N]) of one M and K; problem p's partials at slab + off[p] laid out
// [split][M][N[p]].  _ok: mode.dma, K % 4 == 0, dword-aligned rows (mode.align16: 16-byte), ragged shapes
// only with mode.ragged; else the register-staged tile of gemm_core.h.
// deep (LinMode::deep): 32-deep stages where K % 64 == 0, else 16-deep (one kernel template).  The three
// functions of one launch must be given the same value: raggedness and the split count depend on the depth.
bool skinny_dma_ok(LinMode mode, int M, int K, long lda, long ldb, bool brc, int nprob, const int* N,
                   const float* const* A, const float* const* B);
int skinny_dma_splits(int deep, int M, int K, int tiles_all, size_t cols_all, size_t slab_floats);
hipError_t skinny_dma(hipStream_t st, LinMode mode, bool brc, int nprob, int M, int K,
                      const float* const* A, long lda, const float* const* B, long ldb, const int* N,
                      float* slab, const long* off, int splits);
// the same products with both operands staged by LDS-DMA (wgrad_dma.hip, round 3): 14 x 14 maps,
// row counts multiples of 128, plain operands (dZ already final)
bool wgrad_dma_ok(const ConvMode& cm, int ra, int rb, int S);
hipError_t wgrad_dma(hipStream_t st, const ConvMode& cm, int nB, int ra, int rb, int S, const float* A, long a_bs,
                     const float* B, long b_bs, float* dW, float* slab, int splits);
hipError_t conv_att_wgrad(hipStream_t st, const ConvMode& cm, int nB, int M, int S, int A, const float* dS,
                          const float* I, float* dWp, float* slab);
hipError_t conv_embed_wgrad(hipStream_t st, const ConvMode& cm, int nB, int D, int S, int M, const float* dI,
                            const float* I, const float* X, float* dWi, float* slab,
                            float* dbi = nullptr /* += sum_{b,s} dZ[b,m,s] */,
                            int dz_final = 0 /* dI already holds dZ: no tanh factor, no dbi */);
// same with dZ already final and both operands stored as bf16 (conv_att_dgrad_dz with dz16)
hipError_t conv_embed_wgrad_b16(hipStream_t st, const ConvMode& cm, int nB, int D, int S, int M, const void* dZ16,
                                const void* X16, float* dWi, float* slab);

// --------------------------------------------------------- pointwise (kernels.hip)
enum GateOrder { GATES_ATT = 0 /* i g f o, ATTLSTM.lua:12-19 */,
                 GATES_DEEP = 1 /* i f o g, DeepLSTM.lua:46-54 */ };

// key_dev != nullptr: (seed, step) are read from key_dev[0], key_dev[1] on the device instead
hipError_t fill_masks(hipStream_t st, uint64_t seed, uint32_t site, uint32_t step, float p,
                      size_t n, uint32_t* bits, const uint64_t* key_dev = nullptr);
hipError_t embed_fwd(hipStream_t st, int rows, int E, int V, const float* emb, const int32_t* tokens,
                     const uint32_t* mask, float mscale, float* we, size_t mask_e0 = 0);
hipError_t embed_bwd_rows(hipStream_t st, int rows, int E, int V, const int32_t* tokens, const float* dwe,
                          const float* we, const uint32_t* mask, size_t mask_e0, float mscale,
                          float* gE);
// in place on g4: pre-activations (+ sum of `nsplit` split-K partials [nB,4R] in `slab`)
// -> activated gates; c = f c_prev + i g; h = o tanh c
hipError_t lstm_fwd(hipStream_t st, int order, int nB, int R, float* g4, const float* c_prev,
                    long cp_rs, float* c, long c_rs, float* h, long h_rs, float* tanhc,
                    float* drop_out, const uint32_t* mask, size_t mask_e0, float mscale,
                    const float* slab = nullptr, int nsplit = 0);
// dsum from (dh [+dh2], dc_next), dh optionally given as `nsplit` split-K partials [nB,R]
// in `slab`; optional row replacement by dq rows where lens[b]==t
hipError_t lstm_bwd(hipStream_t st, int order, int nB, int R, const float* gates,
                    const float* c_prev, long cp_rs, const float* tanhc, const float* dh,
                    long dh_rs, const float* dh2, const float* dc_next, float* dsum,
                    float* dc_prev, const int32_t* lens, int t, const float* dq_c,
                    const float* dq_h, long dq_rs, const float* slab = nullptr, int nsplit = 0);
// Up to two independent LSTM cells in one launch (blockIdx.y): the encoder's layer
// wavefront evaluates layer-1 cell t+1 and layer-2 cell t together.
struct LstmFwdCell {
  float* g4;                      // [nB,4R] out: activated gates; in: input part if has_input
  int has_input;                  // 1: pre-activation starts from g4, 0: from b1 + b2
  const float* b1; const float* b2;
  const float* slab; int nsplit;  // nsplit partials [nB,4R], contiguous, summed in order
  const float* c_prev; long cp_rs;
  float* c; long c_rs; float* h; long h_rs; float* tanhc;
  float* drop_out; const uint32_t* mask; size_t mask_e0; float mscale;
};
struct LstmFwdCells { int n; LstmFwdCell c[2]; };
hipError_t lstm_fwd_multi(hipStream_t st, int order, int nB, int R, const LstmFwdCells& cells);
// Weight-stationary persistent encoder forward (enc_ws.hip, round 3): all T token steps of both
// layers in one launch, recurrent weights held in registers, per-(layer, sample half) counters
// instead of a grid barrier.  cnt: 16 words (zeroed by the launcher), err: device error word.
struct EncWsParams {
  int B, R, TL, P;
  float *G1, *G2, *h1, *c1, *tc1, *x2, *h2, *c2, *tc2;
  const float *Wh1, *Wi2, *Wh2, *bi2, *bh2;
  const uint32_t* mask; float mscale;
  unsigned* cnt; int* err;
  int bf16 = 0;   // operands of the gate products rounded to bf16
};
bool enc_ws_ok(int B, int R);
int enc_ws_workgroups(int B);
// All workgroups of a launch must be co-resident (they wait on each other's progress counters):
// the pure predicate, and the same question asked of the current device (occupancy query).
bool enc_ws_coresident(int B, int blocks_per_cu, int n_cus);
bool enc_ws_fits_device(int B);
hipError_t enc_ws_forward(hipStream_t st, int order, EncWsParams Q);
struct LstmBwdCell {
  const float* gates; const float* c_prev; long cp_rs; const float* tanhc;
  const float* slabA; int nA;     // recurrent dh partials [nB,R]
  const float* slabB; int nBp;    // extra dh partials, passed through a dropout mask
  const uint32_t* maskB; size_t maskB_e0; float mscaleB;
  const float* dc_next; float* dsum; float* dc_prev;
  int t; const float* dq_c; const float* dq_h;   // rows with lens[b]==t take dq (SS:584-591)
};
struct LstmBwdCells { int n; const int32_t* lens; long dq_rs; LstmBwdCell c[2]; };
hipError_t lstm_bwd_multi(hipStream_t st, int order, int nB, int R, const LstmBwdCells& cells);
// One workgroup per sample: T = tanh(P + u[b,:,None]) (attbycontent, SS:250),
// e = ws . T + bs (SS:251), a = softmax(e + zm) (attbymemory, SS:288-289),
// jv = qf + sum_s I a (attselect SS:254-263 + first CAddTable SS:270).
// ap: u and/or zm may be handed over as K-split GEMM partials ([split][nB][A] / [split][nB][S],
// passed in the u / zm arguments) plus the Linear's bias, summed in order by the kernel itself --
// two reduce launches less on the recurrence's critical path.
// SL: logical number of positions when the tensors' pitch S is padded (7x7 maps); positions
// [SL, S) get zero attention.
// u_out: where to keep the finished u rows [nB][A] when T is not stored (T == nullptr).
struct AttPartials { int u_ns = 0; const float* u_bias = nullptr; int z_ns = 0; const float* z_bias = nullptr; int SL = 0; float* u_out = nullptr;
                     // image table (forward only): sample b reads its P and I tiles at row img[b]; null = row b
                     const int32_t* img = nullptr;
                     // per-sample region counts (forward only): sample b attends to positions [0, min(SL, nreg[b]))
                     // and gives the others attention exactly 0; indexed by the sample, never by img; null = none
                     const int32_t* nreg = nullptr;
                     // per-sample additive attention bias (forward only, rau_set_att_bias_dev): rows [nB][S] at the
                     // attention's pitch; the score of (b, s) takes zadd[b * S + s] behind the finished memory term, one
                     // f32 add; -inf = no attention there; indexed by the sample, never by img; never read at or
                     // behind the sample's region count; null = none
                     const float* zadd = nullptr; };
// Which form an attention launch takes: an argument of the four launchers and of their predicates, computed by the
// caller from its context (att_mode, policy.h).
struct AttMode {
  int dma = 1;                        // the fused family's LDS-DMA kernels on (else its register-staged ones)
  int waves_fwd = 8, waves_bwd = 16;  // waves per workgroup of the fused kernels (8 | 16)
  int chunks = 0;                     // row chunks per sample of the split family (1..8), 0 = by batch size
};
hipError_t att_fwd_fused(hipStream_t st, const AttMode& am, int nB, int M, int A, int S, const float* P,
                         const float* u, const float* ws, const float* bs, const float* zm,
                         const float* I, const float* qf, float* T, float* a, float* jv,
                         const AttPartials& ap = AttPartials());
// Which of its two kernels att_fwd_fused launches for this shape: the LDS-DMA one (true) or the register-staged
// one (T kept, S > 256 or not a multiple of 4, A or M above 512, or am.dma off).  The step's launch
// wrapper names the profile class after it: "att_fwd_fused" / "att_fwd_fused_regs".
bool att_fwd_dma_ok(const AttMode& am, int M, int A, int S, bool keep_T);
// One workgroup per sample, backward of the above: da = da_lin + sum_m dj I;
// dz = softmax'(da); T -> dS = dz ws (1-T^2) in place; du = sum_s dS; dwsp = sum_s dz T.
hipError_t att_bwd_fused(hipStream_t st, const AttMode& am, int nB, int M, int A, int S, const float* I,
                         const float* dj, const float* a, const float* da_lin,
                         const float* ws, float* T_to_dS, float* dz, float* du, float* dwsp,
                         const float* Psrc = nullptr /* T not kept: recompute tanh(Psrc + u) */,
                         const float* u = nullptr,
                         // da_ns > 0: da_lin holds K-split partials [split][nB][SL] of dj Wf (summed
                         // by the kernel, plus the optional pitched addend da_add [nB][S])
                         int da_ns = 0, int SL = 0, const float* da_add = nullptr,
                         // dS16 != nullptr (only where att_bwd_dma_ok): dS leaves as bf16 [nB][A][S] there
                         // and T_to_dS keeps P
                         void* dS16 = nullptr);
bool att_bwd_dma_ok(const AttMode& am, int M, int A, int S);
// The same two passes cut into 4-wave workgroups (NC row chunks per sample, two launches per
// pass): they always fit next to resident bulk-GEMM workgroups.  `part` is scratch of
// att_split_part_floats(nB, S) floats.  T is never kept (the backward recomputes tanh(Psrc + u)
// when Psrc is given, else reads T).
size_t att_split_part_floats(int nB, int S);
hipError_t att_fwd_split(hipStream_t st, const AttMode& am, int nB, int M, int A, int S, const float* P,
                         const float* u, const float* ws, const float* bs, const float* zm,
                         const float* I, const float* qf, float* a, float* jv, float* part,
                         const AttPartials& ap = AttPartials());
hipError_t att_bwd_split(hipStream_t st, const AttMode& am, int nB, int M, int A, int S, const float* I,
                         const float* dj, const float* a, const float* da_lin, const float* ws,
                         float* T_to_dS, float* dz, float* du, float* dwsp, const float* Psrc,
                         const float* u, float* part, int da_ns = 0, int SL = 0,
                         const float* da_add = nullptr);
// Largest position pitch at which every attention kernel of a family (split: the two above; else the two fused
// ones) gets the dynamic LDS it asks for.  Above 256 positions those are the register-staged kernels, which
// launch without hipFuncAttributeMaxDynamicSharedMemorySize and so with at most 64 KB: 4 S floats in the split
// family (4096 positions); (nw + 2) S + 2 nw + A forward and (nw + 1) S + nw backward in the fused one, nw
// waves -- the caller names the forward's at the wider of its training and evaluate-mode forms (900 positions
// at A = 128).
int att_max_pitch(bool split, int A, int waves_fwd, int waves_bwd);
// The feature-map passes below read the resident batch in its own element type ft (rau_feat_type:
// RAU_FEAT_F32, 16-bit RAU_FEAT_F16 / RAU_FEAT_BF16 or 8-bit RAU_FEAT_E4M3 / RAU_FEAT_E5M2 bit patterns laid
// out like the f32 form), widen each element exactly to f32 and then do the f32 form's arithmetic: results
// are bit-identical to an f32 batch holding the widened values.  An unknown ft (3 is reserved) is
// hipErrorInvalidValue, nothing launched.
inline bool feat_type_ok(int ft) {
  return ft == RAU_FEAT_F32 || ft == RAU_FEAT_F16 || ft == RAU_FEAT_BF16 || ft == RAU_FEAT_E4M3 ||
         ft == RAU_FEAT_E5M2;
}
// bytes of one element of a map of type ft (feat_type_ok(ft))
inline size_t feat_elem_bytes(int ft) {
  return ft == RAU_FEAT_F32 ? 4 : (ft == RAU_FEAT_E4M3 || ft == RAU_FEAT_E5M2) ? 1 : 2;
}
// the accepted types, as the error messages of the entry points list them
#define RAU_FEAT_TYPE_LIST "RAU_FEAT_F32 | _F16 | _BF16 | _E4M3 | _E5M2"
// xd[h][i] = X[i] * keep(h, i) * scale for h < H, i < per_hop (feature-map dropout, SS:239)
// SL != Sp: rows of SL logical positions at pitch Sp (mask indexed logically, pad columns zeroed)
hipError_t dropout_features(hipStream_t st, int H, size_t per_hop, const void* X,
                            const uint32_t* mask, float mscale, float* xd, size_t mask_e0 = 0,
                            int SL = 0, int Sp = 0, int ft = RAU_FEAT_F32);
// The same pass (f32 or, b16 != 0, bf16 output) drawing the site's keep bits itself instead of reading
// them: per_hop % 16 == 0, logical == physical layout; bit-identical to fill_masks + dropout_features
hipError_t dropout_features_gen(hipStream_t st, uint64_t seed, uint32_t site, uint32_t step, float p,
                                const uint64_t* key_dev, int H, size_t per_hop, const void* X,
                                float mscale, void* xd, int b16, int ft = RAU_FEAT_F32);
// RAU_BF16 mode (S % 4 == 0): the same values stored as bf16, [h][i], the form conv_embed_fwd_b16 /
// conv_embed_wgrad_b16 read
hipError_t dropout_features_b16(hipStream_t st, int H, size_t per_hop, const void* X,
                                const uint32_t* mask, float mscale, void* xd16, int ft = RAU_FEAT_F32);
// out[r][s] = widen(X[r][s]) for s < SL, 0 for SL <= s < Sp: the f32 image of a 16-bit or fp8 feature map
// (any ft but RAU_FEAT_F32) at row pitch Sp, for the readers that take the unmasked batch
hipError_t widen_features(hipStream_t st, size_t rows, int SL, int Sp, const void* X, float* out, int ft);
// Per-position L2 normalisation (featnorm.hip): for each of n_maps maps [D][Sp] of element type ft,
//   nrm[m][s] = sqrt(sum_d x[d][s]^2),  xn[m][d][s] = x[d][s] * (1 / max(nrm[m][s], eps))
// on the exactly widened values, in f32, the sum in a fixed order that depends on (D, SL, Sp) alone; an all-zero
// position gives nrm = 0 and +0 outputs; columns SL <= s < Sp of xn and nrm are written as +0.  Sp % 4 == 0, or
// SL == Sp (a dense tensor: single-element accesses).  xn may be X (f32, in place); nrm may be null.  Non-finite
// inputs and sums of squares that overflow f32 are outside the contract.  eps finite and > 0.
hipError_t l2norm_features(hipStream_t st, int n_maps, int D, int SL, int Sp, const void* X, int ft, float eps,
                           float* xn, float* nrm);
// Its gradient, in place on dX [rows][D][Sp] (on entry the gradient G at xn): with c[s] = sum_d G[d][s] xn[d][s] in the
// same fixed order and r = 1 / max(nrm, eps), dX = r (G - xn c) where nrm >= eps and r G where nrm < eps; pad
// columns leave as +0.  Row i reads map i of xn / nrm, or -- with the per-image sample lists of an image table
// (img_start [rows + 1], img_samples; both or neither) -- the map of the first sample of list i; a row whose list
// is empty is not touched.
hipError_t l2norm_backward(hipStream_t st, int rows, int D, int SL, int Sp, const float* xn, const float* nrm,
                           float eps, float* dX, const int32_t* img_start = nullptr,
                           const int32_t* img_samples = nullptr);
// Image table -> per-sample maps: out[b] = table[image_of[b]] for b < nB, maps of map_bytes bytes each
// ([D][Sp] elements of any feature type, copied as they are in 16-byte vectors; map_bytes % 8 == 0, which
// holds for every map a context can have: D % 4 == 0 and Sp % 4 == 0 make even an fp8 map a multiple of 16).
// image_of is a DEVICE index whose entries the host has range-checked against the table.
hipError_t expand_features(hipStream_t st, int nB, size_t map_bytes, const void* table, const int32_t* image_of,
                           void* out);
// Feature bank -> batch buffers: out[i] = bank[rows[i]] for i < n (n <= 65535), maps of map_bytes bytes as in
// expand_features; map offsets into the bank are 64-bit.  rows is a DEVICE index the host has checked; the
// kernel clamps it into [0, capacity) all the same.
hipError_t bank_gather(hipStream_t st, int n, size_t map_bytes, const void* bank, int32_t capacity,
                       const int32_t* rows, void* out);
// out[r][s] = narrow(src[r][s]) for s < SL, 0 for SL <= s < Sp: dense f32 rows into 16-bit or fp8 rows (any ft
// but RAU_FEAT_F32) at pitch Sp (% 4 == 0), round to nearest even -- the bits of numpy's float16 conversion
// (subnormals, overflow to infinity), of feat16.bf16_bits, and of feat16.fp8_bits (SATURATING: everything
// beyond the largest finite value, infinities included, becomes the largest finite value)
hipError_t narrow_features(hipStream_t st, size_t rows, int SL, int Sp, const float* src, void* out, int ft);
// Tied feature-map dropout backward (tied_bwd.hip): the hop sums in front of the one set of conv gradients.
// out[b][k][s] = sum_{h < HA} T[h][b][k][s] (ascending, f32), [B][A][Sp] per hop, pad columns s >= SL written as 0
hipError_t hop_sum(hipStream_t st, int HA, int B, int A, int SL, int Sp, const float* T, float* out);
// dZ[b][m][s] = fmaf(dj[h][b][m], a[h][b][s], dZ[b][m][s]) for h = 1 .. HA-1 (ascending); dj [HA][B][M],
// a [HA][B][Sp], dZ [B][M][Sp]; HA >= 2
hipError_t outer_sum(hipStream_t st, int HA, int B, int M, int Sp, const float* dj, const float* a, float* dZ);
// dst[n] += sum_rows X[row*ld + n]   (two-stage, deterministic; tmp >= 32*N floats)
hipError_t colsum_acc(hipStream_t st, int rows, int N, const float* X, long ld, float* dst,
                      float* tmp);
// per-row CE: argmax (1-based, first max), loss row, dl = (softmax - onehot)/nB, do_pred
// (labels == nullptr: no loss/dl; mf == nullptr: no do_pred)
// nsplit > 0: the logits arrive as K-split partials `part` [split][nB][K] (+ bias) and are
// finished here into logits_out
// ld: row pitch of logits / logits_out / dl (0 = K, dense); the partials stay dense in K.  With ld > K the kernel
// writes +0 into columns K..ld-1 of every row it writes (dl with a ground truth, logits_out with partials)
hipError_t ce_fwd(hipStream_t st, int nB, int K, int M, const float* logits,
                  const int32_t* labels, const float* mf, const float* wd, const float* bd,
                  float* dl, float* lossrow, int32_t* argmax, float* dopred,
                  const float* part = nullptr, int nsplit = 0, const float* bias = nullptr,
                  float* logits_out = nullptr,
                  int Bper = 0 /* rows are [hop][sample]: samples per hop (label period, 1/B) */, int ld = 0,
                  // per-sample loss weights [Bper] (device) or null: invB becomes __fmul_rn(sw[b], invB) and the loss
                  // row __fmul_rn(sw[b], row); the same argument of ce_set_fwd and bce_fwd
                  const float* sw = nullptr);
hipError_t loss_reduce(hipStream_t st, int H, int nB, const float* lossrow, float* losses);
// ce_fwd against an answer set (ce_set.hip, rau_set_answers): ids / w [Bper][G] device, ids 1..K or 0 = empty
// entry, 1 <= G <= kMaxAnswers; lossrow = sum_g w (lse - lg[y_g]), dl = softmax * (W / Bper) - sum_g onehot_g w / Bper
// with W = the row's summed weights; everything else as ce_fwd.  G = 1, w = 1 gives ce_fwd's bits.
constexpr int kMaxAnswers = 16;
hipError_t ce_set_fwd(hipStream_t st, int nB, int K, int M, const float* logits, const int32_t* ids,
                      const float* w, int G, const float* mf, const float* wd, const float* bd, float* dl,
                      float* lossrow, int32_t* argmax, float* dopred, const float* part = nullptr,
                      int nsplit = 0, const float* bias = nullptr, float* logits_out = nullptr, int Bper = 0,
                      int ld = 0, const float* sw = nullptr);
// The criterion head as a per-answer sigmoid with binary cross-entropy (bce_head.hip, RAU_LOSS_BCE): ce_fwd's /
// ce_set_fwd's contract with  t[k] = [k == y]  (labels) or  min(1, sum_g w_g [y_g == k])  (G > 0: ids / w [Bper][G]),
// lossrow = sum_k max(x,0) - x t + log1p(exp(-|x|)),  dl = (sigmoid(x) - t) / Bper; a row whose set has no non-empty
// entry: lossrow 0, dl +0.  labels == nullptr and G == 0: no loss / dl.
hipError_t bce_fwd(hipStream_t st, int nB, int K, int M, const float* logits, const int32_t* labels,
                   const int32_t* ids, const float* w, int G, const float* mf, const float* wd, const float* bd,
                   float* dl, float* lossrow, int32_t* argmax, float* dopred, const float* part = nullptr,
                   int nsplit = 0, const float* bias = nullptr, float* logits_out = nullptr, int Bper = 0, int ld = 0,
                   const float* sw = nullptr);
// The ground truth of a batch: what a criterion, a statistic or the selection head's target is read from.  A plain
// value: "no ground truth" is Truth{}; G > 0 means the answer set replaces the labels.  `loss` is the criterion the
// answers are trained with (RAU_LOSS_CE / RAU_LOSS_BCE of include/rau.h): read by criterion_head and step_stats only.
struct Truth {
  const int32_t* labels = nullptr;   // [Bper] device, or null
  const int32_t* ids = nullptr;      // answer set [Bper][G] (G > 0), device
  const float *w = nullptr, *score = nullptr;
  int G = 0;                         // 0 = labels
  int loss = 0;                      // RAU_LOSS_CE
  // per-sample loss weights [Bper] (device; rau_set_sample_weights) or null: every kernel that forms a training
  // term from this target multiplies the term's 1 / Bper (or hop weight) by sw[b]; set by step_truth() only
  const float* sw = nullptr;
  // multiple-choice candidates [Bper][C] (device; rau_set_candidates), C = 0: none.  The criterion is then restricted
  // to the row's live candidates (cand_head.hip); set by step_truth() and the module-level _cand calls only
  const int32_t* cand = nullptr;
  int C = 0;
  bool present() const { return labels || G > 0; }
  bool bce() const { return loss != 0; }
};
// The criterion head restricted to a row's candidates (cand_head.hip, rau_set_candidates): ce_fwd's / ce_set_fwd's /
// bce_fwd's launch contract -- argmax over ALL K, do_pred, finishing of the partials -- with the criterion `kind`
// (RAU_LOSS_CE / RAU_LOSS_BCE) normalised over the live candidates only.  cand [Bper][C] device, ids 1..K or 0 = empty
// entry, 1 <= C <= kMaxCandidates; the target is labels [Bper] or (G > 0) the set ids / w [Bper][G]; neither: no loss,
// no dl.  dl rows are cleared with 16-byte stores: with a target, ld (0 = K) % 4 == 0 and dl 16-byte aligned.
constexpr int kMaxCandidates = 32;
hipError_t cand_fwd(hipStream_t st, int kind, int nB, int K, int M, const float* logits, const int32_t* labels,
                    const int32_t* ids, const float* w, int G, const int32_t* cand, int C, const float* mf,
                    const float* wd, const float* bd, float* dl, float* lossrow, int32_t* argmax, float* dopred,
                    const float* part = nullptr, int nsplit = 0, const float* bias = nullptr,
                    float* logits_out = nullptr, int Bper = 0, int ld = 0, const float* sw = nullptr);
// Ranked candidates and MC statistics of the merged rows (cand_rank.hip, rau_topk_cand / rau_cand_stats): one wave
// per (row of H+2, sample), lane c holds candidate c.  Rows are hop_merge.h's; logits at pitch ld (0 = K).
// cand_topk: predict rule (last hop forced); ids / score / conf [H+2][B][k], 1 <= k <= C.
// cand_stats: feval rule; rows = rowf [2][B] | rowsc [H+2][B] floats, rowi = correct [H+2][B] | labelled [B];
// out = loss [H+2] | score [H+2] (floats) | correct [H+2] | n_lab (int32), reduced by one workgroup in a fixed order
// (loss[:H] from lossrow in loss_reduce's order).
hipError_t cand_topk(hipStream_t st, int H, int B, int K, int k, const float* logits, const float* dopred,
                     const int32_t* cand, int C, int32_t* ids, float* score, float* conf, int ld);
hipError_t cand_stats(hipStream_t st, int H, int B, int K, const float* logits, const float* dopred,
                      const float* lossrow, const Truth& t, float* rows, int32_t* rowi, float* out, int ld);
// The criterion head against whichever target `t` holds, with the criterion it names: cand_fwd when the batch names
// candidates (t.C > 0), else bce_fwd (RAU_LOSS_BCE), else ce_set_fwd (G > 0) or ce_fwd (labels, or none); the other
// arguments are the ones they share.  criterion_class names the launch for the profile.
inline const char* criterion_class(const Truth& t) {
  return t.C > 0 ? "cand_fwd" : t.bce() ? "bce_fwd" : t.G > 0 ? "ce_set_fwd" : "ce_fwd";
}
inline hipError_t criterion_head(hipStream_t st, int nB, int K, int M, const float* logits, const Truth& t,
                                 const float* mf, const float* wd, const float* bd, float* dl, float* lossrow,
                                 int32_t* argmax, float* dopred, const float* part = nullptr, int nsplit = 0,
                                 const float* bias = nullptr, float* logits_out = nullptr, int Bper = 0,
                                 int ld = 0) {
  if (t.C > 0)
    return cand_fwd(st, t.loss, nB, K, M, logits, t.labels, t.ids, t.w, t.G, t.cand, t.C, mf, wd, bd, dl, lossrow,
                    argmax, dopred, part, nsplit, bias, logits_out, Bper, ld, t.sw);
  if (t.bce())
    return bce_fwd(st, nB, K, M, logits, t.labels, t.ids, t.w, t.G, mf, wd, bd, dl, lossrow, argmax, dopred, part,
                   nsplit, bias, logits_out, Bper, ld, t.sw);
  if (t.G > 0)
    return ce_set_fwd(st, nB, K, M, logits, t.ids, t.w, t.G, mf, wd, bd, dl, lossrow, argmax, dopred, part, nsplit,
                      bias, logits_out, Bper, ld, t.sw);
  return ce_fwd(st, nB, K, M, logits, t.labels, mf, wd, bd, dl, lossrow, argmax, dopred, part, nsplit, bias,
                logits_out, Bper, ld, t.sw);
}
// The step-selection head's gradient (select_bwd.hip, rau_backward_select).  rows = active hops x Bper, hop-major.
// select_signal: s[r] = (select_w[h] * t.sw[b]) * BCE'(do_pred, do_pred_gt) / Bper * x (1 - x), add[r][m] = s[r] wd[m];
// do_pred_gt from t's labels [Bper] (G == 0) or its answer set ids / score [Bper][G] (rau_step_stats' rules).
// select_wgrad: dW[m] += sum_r s[r] mf[r][m], db[0] += sum_r s[r], one fixed-order pass (any M, any row count).
hipError_t select_signal(hipStream_t st, int rows, int Bper, int K, int M, const float* dopred,
                         const int32_t* argmax, const Truth& t, const float* selw_dev, const float* wd, float* s,
                         float* add);
hipError_t select_wgrad(hipStream_t st, int rows, int M, const float* s, const float* mf, float* dW,
                        float* db);
// Attention supervision (att_sup.hip, rau_backward_att / rau_att_stats).  Rows are [hop][sample], hop-major: a and
// da at row pitch a_rs / d_rs, the targets t [Bper] rows at pitch t_rs, nreg [Bper] region counts or null.
// att_sup_grad: da[h,b,s] = -((w[h] t) / (a + 1e-12f)) / Bper below the count, +0 elsewhere, over the whole of d_rs;
// w = w_dev [hops] (device), or with w_dev null `scale` for every hop.  One launch for all hops.
// sw [Bper] (device) or null: per-sample loss weights -- w[h] becomes __fmul_rn(w[h], sw[b]) in the gradient, a row's
// loss sum __fmul_rn(sw[b], sum) in the statistics (mass, hits and the supervised rows stay unweighted).
// att_sup_stats: outf [2][hops] = ATT_h | mean attention mass on t > 0 over the supervised rows, outi [2][hops] =
// pointing-game hits | supervised rows; rowf / rowi [2][hops * Bper] scratch.  Fixed summation order, no atomics.
hipError_t att_sup_grad(hipStream_t st, int hops, int Bper, int S, const float* a, int a_rs, const float* t,
                        int t_rs, const int32_t* nreg, const float* w_dev, float scale, float* da, int d_rs,
                        const float* sw = nullptr);
hipError_t att_sup_stats(hipStream_t st, int hops, int Bper, int S, const float* a, int a_rs, const float* t,
                         int t_rs, const int32_t* nreg, float* rowf, int32_t* rowi, float* outf, int32_t* outi,
                         const float* sw = nullptr);
// The merged answers as training terms (merge_grad.hip, rau_backward_merged / rau_merge_criterion_backward):
// dl [H][B][K] += the gradient of  w_uni CE(uni row) + w_sel CE(select row)  at the hop logits [H][B][K], the rows
// hop_merge.h's under the feval rule (do_pred [H][B], the last hop not forced), the CE against t's labels [B] or
// (G > 0) its answer set.  The two weights are read from mw_dev [2] (device), or with mw_dev null taken from
// w_uni / w_sel; a zero weight's term is skipped.  One launch, one workgroup per sample; dl 16-byte aligned.
// ld: row pitch of logits and dl (0 = K, which then must be a multiple of 4; else a multiple of 4 >= K, and the pad
// columns K..ld-1 of every row of dl the kernel touches leave as +0).
hipError_t merge_grad(hipStream_t st, int H, int B, int K, const float* logits, const float* dopred, const Truth& t,
                      const float* mw_dev, float w_uni, float w_sel, float* dl, int ld = 0);
// Caller-supplied gradients at the step's outputs (ext_grad.hip, rau_backward_ext).  Each one launch, no atomics.
// ext_dl: dl[h][r][k] = dl[h][r][k] * w_dev[h] + d[h][r][k] over H hops of rows_per_hop rows of K floats; d dense
// [H][rows][K], dl rows at pitch ld.  ld == K: 16-byte accesses (rows_per_hop K % 4 == 0, 16-byte aligned bases);
// ld > K (the answer pitch of a K % 4 != 0 context): one element per thread, +0 written into columns K..ld-1.
// d null: the product alone; w_dev null (the forward wrote no dl): dl = d exactly, or +0 with d null too.
// ext_signal: s[r] = (acc ? s[r] : nothing) + (ddp[r] * x) * (1 - x), x = dopred[r]; add[r][m] = s[r] wd[m].
// ext_da: da[h,b,s] = (acc ? da[h,b,s] : nothing) + d[h,b,s] below the count, +0 elsewhere, over the whole of d_rs;
// d dense [hops][Bper][S], da rows at pitch d_rs, nreg [Bper] region counts or null.
hipError_t ext_dl(hipStream_t st, int H, size_t rows_per_hop, int K, int ld, const float* w_dev, const float* d,
                  float* dl);
hipError_t ext_signal(hipStream_t st, int rows, int M, const float* dopred, const float* ddp, const float* wd,
                      bool acc, float* s, float* add);
hipError_t ext_da(hipStream_t st, int hops, int Bper, int S, const float* d, const int32_t* nreg, bool acc,
                  float* da, int d_rs);
// The ends of the hop recurrence (state_io.hip, rau_set_state_dev / rau_state_grad_dev).  Each one launch, no atomics.
// state_attach: cc[i] = widen(c0[i]), hh[i] = widen(h0[i]) for i < n_elems (a multiple of 4); type RAU_FEAT_F32 |
// F16 | BF16; c0 and h0 both null: the detaching form, zero bits into both.  All bases 16-byte aligned.
// state_grad_finish: d_h0[i] = part[0][i] + .. + part[ns-1][i] in ascending order (+0 with ns = 0), d_c0[i] =
// dc_prev[i]; part is a span of split-K partials (checked like every consumer's: kSplitStateError).
hipError_t state_attach(hipStream_t st, size_t n_elems, const void* c0, const void* h0, int type, float* cc,
                        float* hh);
hipError_t state_grad_finish(hipStream_t st, size_t n_elems, const float* part, int ns, const float* dc_prev,
                             float* d_c0, float* d_h0);
// The caller's attention bias (att_bias.hip, rau_set_att_bias_dev / rau_att_bias_grad_dev).  Each one launch, no atomics.
// att_bias_attach: dst[r][s] = widen(src[r][s]) for r < rows, s < SL; src dense [rows][SL] of type RAU_FEAT_F32 | F16 |
// BF16, dst rows of `pitch` floats (pitch >= SL, a multiple of 4), pad columns [SL, pitch) written +0.
// att_bias_grad: out[r][s] = ((dz_0[r][s] + dz_1[r][s]) + ..) + dz_{hops-1}[r][s], hop h's rows at dz + h * hop_stride,
// all rows of `pitch` floats; columns [SL, pitch) and every column with hops = 0 written +0.
hipError_t att_bias_attach(hipStream_t st, int rows, int SL, int pitch, const void* src, int type, float* dst);
hipError_t att_bias_grad(hipStream_t st, int hops, int rows, int SL, int pitch, const float* dz, size_t hop_stride,
                         float* out);
hipError_t scale_hops(hipStream_t st, int H, size_t per_hop, const float* w_dev, float* x);
// x_i[h][0 .. p_i) *= w[h] for three hop-major tensors in one launch
hipError_t scale_hops3(hipStream_t st, int H, const float* w_dev, size_t p0, float* x0, size_t p1, float* x1,
                       size_t p2, float* x2);
hipError_t gather_q(hipStream_t st, int nB, int Rq, int T, const int32_t* lens, const float* c1,
                    const float* h1, const float* c2, const float* h2, float* q);
hipError_t apply_mask(hipStream_t st, size_t n, size_t period, const float* x,
                      const uint32_t* mask, float mscale, float* y, size_t mask_e0 = 0);
// module-level helpers: out[r,n] = s[r] (X ? X[r,n] : 1) (v ? v[n] : 1); sigmoid / tanh backward
hipError_t row_scale(hipStream_t st, int rows, int N, const float* s, const float* X,
                     const float* v, float* out);
hipError_t sigmoid_bwd(hipStream_t st, int n, const float* dy, const float* y, float* dx);
hipError_t mul_dtanh(hipStream_t st, size_t n, const float* d, const float* y, float* out);
hipError_t scale_inplace(hipStream_t st, size_t n, float s, float* x);
// dq[i] = sum_h dQD[h][i] * mask_h[i] * scale
hipError_t dq_reduce(hipStream_t st, int H, size_t n, const float* dQD, const uint32_t* mask,
                     float mscale, float* dq);
// dx2 -> dh1 extra: y = x * mask * scale (mask may be null)
hipError_t embed_bwd(hipStream_t st, int nuniq, int E, const int32_t* utok, const int32_t* ustart,
                     const int32_t* upos, const float* dwe, const float* we,
                     const uint32_t* mask, float mscale, float* gE);
hipError_t splitk_reduce_acc(hipStream_t st, size_t n, int splits, const float* slab,
                             size_t slab_stride, float* dst);
// C = epilogue(sum_s slab[s]) with the LinOpts epilogue (bias, addend, tanh, ...)
hipError_t lin_reduce_epilogue(hipStream_t st, int M, int N, int splits, const float* slab,
                               float* C, long ldc, const LinOpts& o);
hipError_t uniform_fill(hipStream_t st, uint64_t seed, uint32_t stream, size_t n, float lo,
                        float hi, float* x);
// noise + norm + clip + adam (SS:597-630, optim_updates.lua:59-87)
hipError_t add_noise_sqnorm(hipStream_t st, size_t n, float* g, float nstd, uint64_t seed,
                            uint32_t stream, float* partial /* >= 1024 */);
hipError_t finish_norm(hipStream_t st, int nparts, const float* partial, float* norm_out);
hipError_t clip_adam(hipStream_t st, size_t n, float* x, float* g, float* m, float* v,
                     const float* norm, float clip, float stepsize, float beta1, float beta2,
                     float eps);
// The same update with all three groups in every launch (update.hip, rau_update): the groups' pointers travel
// by value and blockIdx.y names the group.  Two launches: upd_noise_sqnorm leaves kUpdParts partial sums of
// squares per group (add_noise_sqnorm's, in its order); upd_apply finishes the norms in every workgroup
// (finish_norm's order), writes norms[0..2] = group norms and norms[3] = sqrtf((s0 + s1) + s2), clips by the
// group's norm or (global_clip) by norms[3], and applies the rule.  16-byte accesses where a group's four
// pointers allow, scalar otherwise and for a tail of n % 4 elements.
constexpr int kUpdParts = 1024;
struct UpdGroups {
  float *x[3], *g[3], *m[3], *v[3];
  size_t n[3];
  float step[3];       // the rule's step size with its bias correction, formed on the host in double
  uint64_t seed[3];    // noise key of the group
};
hipError_t upd_noise_sqnorm(hipStream_t st, const UpdGroups& G, float nstd, float* partial /* [3][kUpdParts] */);
hipError_t upd_apply(hipStream_t st, const UpdGroups& G, int rule /* rau_opt_rule */, bool global_clip, float clip,
                     float beta1, float beta2, float eps, const float* partial, float* norms /* [4] */);
// rau_update_ex's two launches (update.hip): the same passes with a segment table.  A segment is the weight or the
// bias part of one layout entry; the segments of group g are first[g] .. first[g+1]-1, `end` is a segment's end offset
// in its group (the last one's is the group's n; ends are NOT multiples of 4), `step` its step size, `f` its decay
// factor (1: none), `frozen` != 0: its elements are neither read into a norm nor written.  The sums' element order,
// the partials and the finish are upd_noise_sqnorm's / upd_apply's; UpdGroups::step is not read.  ema[g] (all three
// or none) is the weight average, updated after the rule with decay d and omd = 1 - d.
constexpr int kUpdSegs = 36;       // 1 + 8 + 26 segments, padded
constexpr int kUpdGroupSegs = 26;  // the most one group has
struct UpdSegs {
  size_t end[kUpdSegs];
  float step[kUpdSegs], f[kUpdSegs];
  uint32_t frozen[kUpdSegs];
  int first[4];
};
hipError_t upd_ex_sqnorm(hipStream_t st, const UpdGroups& G, const UpdSegs& T, float nstd, float* partial);
hipError_t upd_ex_apply(hipStream_t st, const UpdGroups& G, const UpdSegs& T, int rule, bool global_clip, float clip,
                        float beta1, float beta2, float eps, float* const ema[3] /* or null */, float d, float omd,
                        const float* partial, float* norms /* [4] */);
// x[g] <-> e[g] for the three groups in one launch (rau_ema_swap): 16-byte accesses where both pointers allow
hipError_t ema_swap(hipStream_t st, float* const x[3], float* const e[3], const size_t n[3]);
// Adamax on one flat vector (rau_dev_adamax): adamax_elem on dx as it stands; any n, any 4-byte-aligned pointers
hipError_t adamax_vec(hipStream_t st, size_t n, float* x, const float* dx, float* m, float* u, float stepsize,
                      float beta1, float beta2, float eps);
// Per-layer statistics of the flat vectors and the update guard's count (layer_stats.hip, rau_layer_stats).  Every
// layout entry is tiled by ITEMS of at most kStatChunk elements that start at the entry's start plus a multiple of
// kStatChunk, so no item crosses an entry; the table is built once per context and lives in device memory.
// layer_stats_part: one 256-thread workgroup per item reads the requested sources of its elements (16-byte loads
// over the aligned middle, scalar loads for a head and a tail of at most 3) and leaves one partial record;
// layer_stats_finish adds an entry's partials in ascending item order from +0 into rau_layer_stat records, and the
// items' non-finite counts per group and source into totals [3 sources][3 groups].  The order and its chain length
// L(n) are stated in layer_stats.hip's header.
constexpr int kStatChunk = 8192;
constexpr int kStatMaxEntries = 64;   // StatSrc::skip is one bit per entry (35 today)
constexpr int kStatPartWords = 12;    // a partial record: sumsq[3] | absmax[3] | nonfinite[3] | pad[3], 32-bit words
struct StatItem {     // 16 bytes
  uint64_t start;     // first element, in its group's flat vector
  uint32_t len;       // 1 .. kStatChunk
  uint16_t group, entry;   // entry: index over the three groups' layouts, EMBED | RNN | MULT
};
struct StatEntry {    // 16 bytes
  uint32_t first, items;   // its items are first .. first + items - 1
  uint64_t n;              // elements
};
struct StatSrc {
  const float *g[3], *x[3], *m[3], *v[3];   // per group; a source that is not requested is not read
  int rule[3];        // rau_opt_rule of the group's moments (RAU_STAT_DIR)
  float eps;
  uint64_t skip;      // bit e: entry e's items read nothing and leave zeros (the guard under rau_update_ex: frozen)
};
// what: RAU_STAT_* bits; count_only: the non-finite counts alone (sumsq and absmax stay +0)
hipError_t layer_stats_part(hipStream_t st, const StatSrc& S, int what, bool count_only, const StatItem* items,
                            int n_items, uint32_t* partial /* [n_items][kStatPartWords] */);
// out == null: the totals alone (the guard)
hipError_t layer_stats_finish(hipStream_t st, const StatEntry* entries, int n_entries, const int group_first[4],
                              const uint32_t* partial, rau_layer_stat* out /* [n_entries] or null */,
                              int64_t* totals /* [3][3] */);

// feval's statistics of the resident hop outputs (hop_merge.hip, SS:476-556): per-sample rows
// rowf [B][H+2], rowi [B][4H+3], then one fixed-order batch reduction into
// out = loss[H+2] | loss_do_pred[H] | int32 counts[4H+3]
// against t's labels, or (G > 0) its answer set ids / w / score [B][G]: "correct" = the row's first-max answer
// carries a positive score, uni / select CE are the soft CE of ce_set_fwd; a set also gives the metric score of
// every row's answer, rowscore [H+2][B] (feval rule), and their fixed-order batch sums tot [H+2] (labels: unused).
// t.bce(): the uni / select losses are bce_fwd's criterion of those rows instead; nothing else changes
hipError_t step_stats(hipStream_t st, int H, int B, int K, const float* logits, const float* dopred,
                      const int32_t* argmax, const float* lossrow, const Truth& t, float* rowf, int32_t* rowi,
                      float* out, float* rowscore, float* tot, int ld = 0 /* row pitch of logits, 0 = K */);
// out[r][b] = sum_g score[b][g] * [ids[b][g] == ans[r][b]] over t's set in entry order (ans 1-based, [R][B]),
// tot[r] = the fixed-order sum of row r over the batch
hipError_t answer_scores(hipStream_t st, int R, int B, int K, const int32_t* ans, const Truth& t, float* out,
                         float* tot);
// predict_result's merges + answers (SS:633-705, 877-900): oe / mco [H+2][B] 1-based, pred [2][B][K] and
// att_out [2][B][Sp] (uni, select; either may be null); mc [B][n_mc] device ids 0..K (null: no MC).  ld: row pitch
// of logits AND of pred (0 = K); with ld > K the pad columns of pred are written +0
hipError_t predict_rows(hipStream_t st, int H, int B, int K, int Sp, const float* logits, const float* dopred,
                        const float* att, const int32_t* mc, int n_mc, int32_t* oe, int32_t* mco, float* pred,
                        float* att_out, int ld = 0);
// dynamic LDS bytes predict_rows takes with an MC list
size_t predict_rows_lds(int K);
// torch.topk(x, k, 2, true, true) of x [rows][cols] in the total order of include/rau.h (topk.hip):
// val / idx [rows][k], idx 1-based, either may be null; rows > 0, 1 <= k <= cols
hipError_t topk_rows(hipStream_t st, const float* x, int rows, int cols, int k, float* val, int32_t* idx);
// the k best answers of predict_result's rows (hops, uni, select; last hop forced): ids / score / conf
// [H+2][B][k], conf = softmax probability in row_ce's formulation; none may be null
hipError_t topk_merged(hipStream_t st, int H, int B, int K, int k, const float* logits, const float* dopred,
                       int32_t* ids, float* score, float* conf, int ld = 0 /* row pitch of logits, 0 = K */);

}  // namespace rau

/*
 * rau.h -- C ABI of librau.so: the MI355X-native Recurrent Answering Unit
 * forward/backward (hand-written HIP for gfx950 behind plain pointers).
 *
 * This is the drop-in boundary for ONE path of HyeonwooNoh/RAU_VQA: the tensor
 * half of `feval` (reference experiments/Ours_SS/LstmAttCtrlGradNoiseDontSelect.lua
 * :428-596, "SS" below) plus the network it drives (SS:198-316,
 * model/ATTLSTM.lua, model/DeepLSTM.lua).  The reference reaches that path
 * through the Torch7 nn.Module protocol, not through an FFI of its own, so each
 * entry point below cites the nn.Module call sites it replaces.  A LuaJIT
 * `ffi.cdef` shim that re-presents these calls as :forward/:backward/
 * :getParameters objects is in bindings/rau.lua; INTEGRATION.md shows the
 * reference-side patch.
 *
 * Conventions
 *  - every function returns 0 on success or a negative rau_status; the message
 *    for the calling thread's last failure is rau_last_error().  Nothing throws
 *    or longjmps across the boundary (Lua `error()` is raised by the shim).
 *  - no global state: everything hangs off an opaque rau_ctx (one per GPU,
 *    driven by one host thread at a time -- same rule as a Lua state).
 *  - the ctx owns all device memory.  Host pointers passed in are owned by the
 *    caller and are consumed before the call returns unless stated otherwise.
 *  - all work is enqueued on the ctx's HIP stream; host-visible results are
 *    valid after rau_sync() (or any call documented as synchronising).
 *  - ids are 1-based like the reference's Lua tensors: token ids 1..V with
 *    1 = ZEROPAD (utils/vqa_prepro_loader.lua:1393), answer ids 1..K, and the
 *    returned argmax ids are 1..K with torch.max's first-max tie rule (SS:488).
 *  - there is NO CPU fallback: rau_create fails if no gfx950 device is usable.
 */
#ifndef RAU_H
#define RAU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAU_ABI_VERSION 5

typedef enum rau_status {
  RAU_OK = 0,
  RAU_ERR_INVALID = -1,   /* bad argument / shape / id out of range */
  RAU_ERR_DEVICE = -2,    /* HIP error, no device, wrong architecture */
  RAU_ERR_STATE = -3,     /* call order (e.g. backward before forward) */
  RAU_ERR_NOMEM = -4
} rau_status;

typedef enum rau_group {   /* flat parameter groups, SS:322-324 getParameters() */
  RAU_GROUP_EMBED = 0,     /* protos.word_embed */
  RAU_GROUP_RNN = 1,       /* protos.rnn  (DeepLSTM) */
  RAU_GROUP_MULT = 2       /* protos.multimodal */
} rau_group;

typedef enum rau_mode {    /* m:training() / m:evaluate(), SS:449-450,479,648-649,676 */
  RAU_MODE_TRAIN = 0,
  RAU_MODE_EVAL = 1
} rau_mode;

typedef enum rau_mask_site {   /* the five nn.Dropout sites on the path */
  RAU_MASK_WE = 0,   /* [T,B,E]   word_embed Dropout(0.5), SS:205 */
  RAU_MASK_RNN = 1,  /* [T,B,Rq]  DeepLSTM inter-layer dropout, DeepLSTM.lua:39 */
  RAU_MASK_Q = 2,    /* [H,B,Q]   q_embed Dropout(0.5), SS:233 */
  RAU_MASK_X = 3,    /* [H,B,D,S] i_embed Dropout(0.5) on the feature map, SS:239 */
  RAU_MASK_MF = 4    /* [H,B,M]   classifier merge_feat Dropout(0.5), SS:277 */
} rau_mask_site;

typedef enum rau_dtype {
  RAU_F32 = 0,       /* f32 operands, f32 MFMA accumulate (exact fmaf chain) */
  RAU_BF16 = 1,      /* BASELINE.json configs[2] (Ours_ResNet 14x14x2048, "bf16 MFMA gate/classifier
                      * GEMMs"): every GEMM on the path takes bf16-rounded operands (round to nearest
                      * even) with f32 accumulation -- the five 1x1-conv GEMMs (i_embed, ifeatproj and
                      * their gradients: 94-98 % of the FLOPs) and the three products of every Linear
                      * layer (LSTM gates, hop projections, classifier: y = x W^T, dx = dy W,
                      * dW = dy^T x).  Biases, the cell / attention / softmax / loss arithmetic and
                      * the parameters, states and gradients in memory stay f32; the one-column
                      * Linears (att_score, out_do_pred) are dot products in f32.  Where the 14x14
                      * bf16 tiles do not apply (M % 128, A % 32) the attention input gradient stays
                      * exact f32; the emulating oracle (oracle/ref_torch.py bf16=True) follows the
                      * same rule. */
  RAU_F32S = 2       /* same five GEMMs with every f32 operand SPLIT into three bf16 terms
                      * (hi + mid + lo = all 24 significand bits) and six bf16 MFMA products per
                      * operand pair, f32 accumulate: f32-grade accuracy (dropped terms <= 2^-24
                      * relative) on the 16x faster bf16 matrix pipe.  Not bitwise the fmaf chain
                      * of RAU_F32; selectable, never the default. */
} rau_dtype;

/* Network hyper-parameters: the hard-coded locals of SS:202,209-229 plus the
 * data-defined sizes.  Q (question state width) is 4*Rq: 2 layers x {c,h}. */
typedef struct rau_config {
  int32_t B;    /* batch size per GPU (opt.batch_size): the context's capacity, see rau_set_batch_size */
  int32_t T;    /* seq_len: rows of the token matrix x[T,B] */
  int32_t V;    /* vocab_size incl. ZEROPAD */
  int32_t E;    /* embed_dim = 200, SS:202 */
  int32_t Rq;   /* rnn_size = 512, SS:209 (nrnn_layer fixed at 2, SS:210) */
  int32_t D;    /* cnnout_dim 512 | 2048, SS:216 */
  int32_t S;    /* cnnout_w*cnnout_h = 196 (14x14) or 49 (7x7, the scripts' default), SS:219;
                 * not a multiple of 4: padded internally (callers always see dense [.., S]) */
  int32_t M;    /* multfeat_dim = 512, SS:220 */
  int32_t A;    /* attfeat_dim = 256, SS:221 */
  int32_t R;    /* att_rnn_size = 512, SS:225 (1 layer, dropout 0) */
  int32_t K;    /* answer_size = 1000, SS:222; any K >= 2 (3129, 3113, 1842 ..): not a multiple of 4: rows padded
                 * internally (rau_logits_pitch; host-side results stay dense [.., K]) */
  int32_t H;    /* nHop */
  float p_we, p_rnn, p_q, p_x, p_mf;  /* dropout probabilities, 0.5 each (device masks resolve p to
                                       * 1/256; the 1/(1-p) scale uses the same quantised p) */
  int32_t dtype;      /* rau_dtype */
  int32_t device_id;  /* HIP device ordinal (opt.gpuid) */
} rau_config;

typedef struct rau_ctx rau_ctx;

/* Fills *cfg with the reference's defaults (Ours_SS, 14x14x512, nhop 8). */
void rau_default_config(rau_config* cfg);

const char* rau_last_error(void);
int rau_abi_version(void);

/* Builds the three protos + their clones (SS:200-347): allocates parameters,
 * gradients, activations for T tokens and H hops, and the ctx stream.
 * RAU_ERR_INVALID (before the device is touched) for a configuration outside what the kernels take: widths (E, Rq,
 * D, M, A, R) that are no positive multiple of 4, K < 2 (one answer is no classification problem), and an S above what the attention kernels' 64 KB of LDS hold -- 4096 positions
 * for contexts of up to 64 samples, (16352 - A) / 18 above (900 at A = 128); the message names the bound. */
int rau_create(const rau_config* cfg, rau_ctx** out);
void rau_destroy(rau_ctx* ctx);

/* ---- batch size: one context, batches of up to the B it was created for ------------------------
 * The B of rau_create is the context's CAPACITY: every buffer is allocated for it once.  The reference trains
 * at opt.batch_size and evaluates the same parameters at a size that divides the split (83 / 57 / 96,
 * SS:85-95, its test_* state tensors SS:387-410); rau_set_batch_size(ctx, n), 1 <= n <= capacity, makes the
 * SAME context run batches of n rows: it then behaves BIT FOR BIT like a context created with B = n in this
 * process that holds the same parameters, gradients, Adam moments and step counts, dropout seed, mode, bank
 * and communicator -- at every entry point of this header.  Every tensor shape uses n and is dense in it
 * ([H,n,K] logits, [T,n] tokens, mask sites [H,n,D,S], the staging arrays of rau_batch_slot), and every
 * batch-dependent launch decision is the one rau_create makes for n (one function serves both).
 *   kept      parameters, gradients, optimizer state, the (seed, step) of rau_set_dropout_seed, the mode, the
 *             feature bank and its rows, the communicator, rau_dev_alloc'ed memory, captured steps of other
 *             sizes (rau_graph_step keys its cache by n: a step captured at 100 is found again after an
 *             excursion to 83, never replayed at 83).
 *   cleared   the resident batch, both slots of the asynchronous path (pending uploads are dropped), explicit
 *             masks of rau_set_mask (the sites fall back to the seeded stream), the module-level output slots,
 *             the last forward's results and merged hops: entry points that need them return RAU_ERR_STATE
 *             with nothing launched, exactly as on a fresh context, until their inputs exist again.
 *   n == the current size: a no-op that keeps everything.  n < 1 or n > capacity: RAU_ERR_INVALID, nothing
 *   changes.  A split-K workspace can need MORE room at a smaller n (split counts are chosen per shape); if
 *   that allocation fails: RAU_ERR_NOMEM and the context stays at the old size.  RAU_ERR_STATE while
 *   profiling is on.  A persistent-encoder give-up (rau_sync) is a finding about the device, not the size:
 *   the context keeps the launch-per-step encoder at every later size.
 * Cost: the call drains the context's streams and clears all batch-dependent device storage, because the
 * dense layouts move and the step relies on zeros a fresh context has (initial-state rows, pad columns of
 * 7x7 maps).  Measured on an MI355X (tools/batch_size_time.py, table in LOG.md): 0.48 ms for 100 -> 83 and
 * 0.79 ms for 256 -> 96 at the default widths (contexts of 1.7 and 3.8 GB), 0.63 ms for 80 -> 32 at D = 2048
 * in bf16 mode (2.7 GB); the same in either direction, since it clears what the capacity allocated: the
 * stream drain, about a hundred memsets and one synchronise, no workspace regrowth in any of those.  That is a
 * third to a half of an evaluate-mode forward (1.5 ms at 83 rows): a per-epoch call (train / evaluate /
 * ragged tail), not a per-step call.  A context that never calls it allocates and computes exactly what it
 * did without it.  Synchronising.
 * rau_batch_size: the current size and the capacity (either may be NULL). */
int rau_set_batch_size(rau_ctx* ctx, int32_t n);
int rau_batch_size(rau_ctx* ctx, int32_t* n, int32_t* capacity);

/* ---- parameters: m:getParameters(), SS:322-324 ------------------------------
 * Flat DEVICE buffers (weights, gradients) of a group and its length in floats.
 * Layout: rau_layout_entry() lists each tensor; weight [out,in] then bias [out]
 * per layer (DESIGN.md section "Flat parameter layout"). */
int rau_params(rau_ctx* ctx, int group, float** weights, float** grads, size_t* n);
int rau_layout_count(const rau_ctx* ctx, int group);
int rau_layout_entry(const rau_ctx* ctx, int group, int index, const char** name,
                     size_t* offset, int32_t* rows, int32_t* cols);
/* host <-> device copies of a whole group (synchronising) */
int rau_set_params(rau_ctx* ctx, int group, const float* host, size_t n);
int rau_get_params(rau_ctx* ctx, int group, float* host, size_t n);
int rau_get_grads(rau_ctx* ctx, int group, float* host, size_t n);
int rau_set_grads(rau_ctx* ctx, int group, const float* host, size_t n);
/* param:uniform(lo,hi) on each flat vector, SS:352-354 (Philox, not Torch's MT) */
int rau_init_uniform(rau_ctx* ctx, uint64_t seed, float lo, float hi);
/* embed_grad:zero() rnn_grad:zero() mult_grad:zero(), SS:429-431 */
int rau_zero_grads(rau_ctx* ctx);

/* ---- mode and dropout --------------------------------------------------------
 * :training()/:evaluate() on every clone.  In TRAIN mode the five dropout sites
 * draw masks either from explicit keep flags (rau_set_mask, parity tests) or
 * from the Philox4x32-10 stream keyed by (seed, site, step) (rau_set_dropout_seed;
 * regenerated on device inside rau_forward). */
int rau_set_mode(rau_ctx* ctx, int mode);
int rau_set_dropout_seed(rau_ctx* ctx, uint64_t seed, uint32_t step);
/* keep: uint8 0/1 flags for the whole site in the shape listed at rau_mask_site;
 * n = element count.  Switches that site to explicit masks until
 * rau_set_dropout_seed is called again. */
int rau_set_mask(rau_ctx* ctx, int site, const uint8_t* keep, size_t n);
/* reads back the keep flags the next/last forward uses (tests; synchronising) */
int rau_get_mask(rau_ctx* ctx, int site, uint8_t* keep, size_t n);

/* ---- feature-map dropout: one mask per hop clone, or one mask tied across the hops ------------
 * The reference gives every hop clone its own Dropout mask on the raw feature map (SS:239, 343-347), so
 * xd[h] = X (.) mask_h and both 1x1 convolutions run once per hop.  RAU_XDROP_TIED shares ONE mask among the
 * hops (variational dropout over the steps of a weight-shared recurrence: a modelling option the reference does
 * not have).  i_embed's output and the attention pre-activation are then hop-invariant: a train-mode step
 * runs both convolutions once, and its backward sums what the hops hand back (dS_h, dj_h (x) a_h; the conv
 * gradients are linear in them) and runs the three conv gradients once.
 *   mask site    RAU_MASK_X has [B,D,S] elements in tied mode, not [H,B,D,S]: rau_set_mask / rau_get_mask check
 *                against that count.  The device-drawn tied mask of a (seed, step) is the hop-0 slice of the
 *                per-hop mask of the same (seed, step); the scale stays 1/(1-p).  Tied dropout computes what
 *                per-hop dropout computes when it is given H equal masks.
 *   the call     between steps, in either mode.  A CHANGE of kind drops a caller-supplied mask of site
 *                RAU_MASK_X (the site falls back to the seeded stream) and the last forward: a backward without a
 *                new forward is RAU_ERR_STATE.  Parameters, gradients, optimizer state, bank, batch slots and
 *                the captured steps of the other kind stay (rau_graph_step keys its cache by the kind).  A
 *                kind outside the two values: RAU_ERR_INVALID.  While a step is being captured: RAU_ERR_STATE.
 *   numerics     the summed backward adds the hops in ascending order in f32 and gives the same bits on every
 *                call; they are not the bits of the per-hop path fed H equal masks (another summation order).
 *                RAU_BF16: the hop sums are rounded once, as sums.  The evaluate-mode backward and everything
 *                under RAU_XDROP_PER_HOP compute exactly what they did without this call.
 * The module-level entry points need nothing: a host that clones modules ties the masks by handing every
 * clone the same one; rau_multimodal_forward under RAU_XDROP_TIED reads the one mask for every hop. */
#define RAU_XDROP_PER_HOP 0   /* the reference: a mask per hop clone (default) */
#define RAU_XDROP_TIED    1   /* one mask, shared by all hops */
int rau_set_feat_dropout(rau_ctx* ctx, int kind);
int rau_feat_dropout(rau_ctx* ctx, int* kind);

/* ---- answer criterion: softmax cross-entropy, or a per-answer sigmoid with binary cross-entropy --------------
 * The reference trains every hop's logits with nn.CrossEntropyCriterion (SS:310), and an answer set
 * (rau_set_answers) with its soft-target form.  RAU_LOSS_BCE is the other common VQA objective: every answer k has
 * its own sigmoid, trained with binary cross-entropy against a soft target t[k] in [0, 1] -- with rau_set_answers'
 * weights w = min(#humans / 3, 1) the recipe of the bottom-up / top-down models.  It replaces the criterion of
 * rau_forward and every rau_graph_step*; everything that reads logits and argmax only is the same under both.
 * Per (hop, sample) row, with x the row's logits, n the current batch size and invB = 1 / n:
 *   target     labels:      t[k] = [k == y]
 *              answer set:  t[k] = min(1, sum_g w[b,g] [ids[b,g] - 1 == k]) over the non-empty entries, added from 0
 *              in entry order in f32, then clamped: duplicates add up, deterministically.  Ids as at rau_set_answers.
 *   loss row   sum_k ( max(x,0) - x t + log1pf(expf(-|x|)) ), summed over K and NOT divided by K (BCE-with-logits
 *              times K); a hop's loss (rau_get_losses) is the mean of its rows over n.
 *   gradient   d_logits[k] = (sigmoid(x) - t) invB, sigmoid from e = expf(-|x|) as x >= 0 ? 1/(1+e) : e/(1+e); the
 *              difference and the product are each rounded once.  Finite for every finite x; the same bits on
 *              every call (no atomics).
 *   unlabelled a row whose set has no non-empty entry: loss 0, gradient +0, never "correct" -- as under RAU_LOSS_CE.
 *              A row whose entries all carry weight 0 IS labelled, with the all-zero target: every answer is
 *              pushed down.
 *   the call   between steps, in either mode.  A CHANGE of kind drops the last forward: rau_backward*,
 *              rau_step_stats and rau_step_scores without a new forward are RAU_ERR_STATE, nothing launched.
 *              Parameters, gradients, optimizer state, bank, batch slots, answer sets, region counts and the
 *              captured steps of the other kind stay (rau_graph_step keys its cache by the kind).  A kind outside
 *              the two values: RAU_ERR_INVALID.  While a step is being captured: RAU_ERR_STATE.  rau_config is not
 *              touched, and a context that never calls this computes exactly what it did without it.
 *   with       hop_w, select_w and att_w as before: the select head's target do_pred_gt stays "the hop's first-max
 *              answer equals the label / carries a positive score".
 *   statistics rau_step_stats: loss[0..H) is rau_get_losses bit for bit; loss[H] and loss[H+1] are the same
 *              criterion (same formula, same target) of the uni and select rows under the feval rule.  Counts,
 *              loss_do_pred, rau_step_scores, rau_predict, rau_predict_scores, rau_get_merged: untouched.
 *              rau_topk: conf stays the softmax probability; under RAU_LOSS_BCE the per-answer confidence is the
 *              sigmoid of the returned score.
 *   NOT built  training the merged rows: rau_backward_merged / rau_graph_step_merged with a non-zero merge_w under
 *              RAU_LOSS_BCE are RAU_ERR_INVALID, nothing launched (NULL or zeros stays rau_backward_att);
 *              rau_merge_criterion_backward is a cross-entropy function under either kind.
 * The module-level rau_criterion_*_bce below are this criterion whatever the kind. */
#define RAU_LOSS_CE  0   /* softmax cross-entropy: the reference, the default */
#define RAU_LOSS_BCE 1   /* per-answer sigmoid, binary cross-entropy against soft targets */
int rau_set_answer_loss(rau_ctx* ctx, int kind);
int rau_answer_loss(rau_ctx* ctx, int* kind);

/* ---- batch: what next_batch_feat returns + the H2D of SS:434-439 -------------
 * feats [B,D,S] float (NCHW with W*H flattened), tokens [T,B] int32, lens [B]
 * int32 (0..T), labels [B] int32 (1..K) or NULL for inference.  Copies to the
 * ctx's device buffers; also builds the per-token position index that makes
 * the LookupTable gradient a deterministic gather-sum. */
int rau_set_batch(rau_ctx* ctx, const float* feats, const int32_t* tokens,
                  const int32_t* lens, const int32_t* labels);
/* device pointer of the resident feature buffer (producer may write it directly).  It is returned as it
 * is: after a 16-bit batch (rau_set_batch_typed) its first B*D*Sp*2 bytes hold that batch's 16-bit
 * elements at row pitch Sp (S rounded up to a multiple of 4), not floats; after an fp8 batch its first
 * quarter (B*D*Sp bytes) holds that batch's 1-byte elements at row pitch Sp; after a batch with an image
 * table (rau_set_batch_images) it holds the table's N maps, not one map per sample. */
int rau_batch_feats(rau_ctx* ctx, float** feats_dev);

/* ---- 16-bit feature maps ---------------------------------------------------------------------------
 * The element type of a batch's feature map.  16-bit maps halve the host-to-device transfer, the pinned
 * staging and the host memory that holds the features.  Widening a 16-bit value to f32 is exact, and
 * every pass that reads the batch widens first and then does the f32 arithmetic, so a batch given as
 * fp16 or bf16 gives BIT-IDENTICAL results to the same batch given as f32 holding the widened values
 * (finite inputs; fp16 subnormals included).  The type belongs to the batch, not to the ctx: each slot
 * of the asynchronous path records the type of the batch it holds and rau_use_batch makes it current.
 * rau_set_batch / rau_set_batch_async are the RAU_FEAT_F32 case.  An unknown type is RAU_ERR_INVALID.
 *
 * fp8 maps: the two OCP 8-bit formats (NOT the MI300 "fnuz" forms), one byte per element, halve all of that
 * once more.  e4m3fn: exponent bias 7, subnormals m * 2^-9, no infinities, S.1111.111 the only NaN, largest
 * finite value 448.  e5m2: exponent bias 15, subnormals m * 2^-16, infinities and NaNs as in binary16 (a code
 * is the upper byte of a binary16), largest finite value 57344.  Widening is exact for every code: subnormals
 * become normal f32 numbers, +-0 keep their sign, e5m2 +-inf become +-inf, NaN codes become a NaN.  So the same
 * contract holds: a batch given as fp8 gives BIT-IDENTICAL results to the same batch given as f32 holding the
 * widened values (finite inputs), at every entry point that takes a feat_type, in both modes, in every context
 * dtype, under rau_graph_step and at module level with X == NULL.
 * What fp8 storage does to VQA accuracy is NOT measured and NOT claimed: the library's contract is exactness
 * with respect to the stored values.  Choosing a format is the user's decision: e4m3 has 3 significand bits
 * and range up to 448, e5m2 has 2 bits and range up to 57344.
 * The value 3 is reserved: it is an unknown type (RAU_ERR_INVALID), like every value above 5. */
typedef enum rau_feat_type {
  RAU_FEAT_F32 = 0,
  RAU_FEAT_F16 = 1,   /* IEEE binary16, passed as its bit patterns */
  RAU_FEAT_BF16 = 2,  /* bfloat16 bit patterns (the upper half of an f32) */
  RAU_FEAT_E4M3 = 4,  /* OCP e4m3fn bit patterns, one byte per element */
  RAU_FEAT_E5M2 = 5   /* OCP e5m2 bit patterns (the upper byte of an IEEE binary16) */
} rau_feat_type;
/* rau_set_batch with feats [B,D,S] of elements of feat_type (feats NULL: the resident buffer already
 * holds the map, written through rau_batch_feats, in that type) */
int rau_set_batch_typed(rau_ctx* ctx, const void* feats, int feat_type, const int32_t* tokens,
                        const int32_t* lens, const int32_t* labels);
/* rau_set_batch_async with feats of elements of feat_type; feats NULL: the slot's pinned staging
 * (rau_batch_slot) already holds B*D*S elements of feat_type at its start */
int rau_set_batch_async_typed(rau_ctx* ctx, int slot, const void* feats, int feat_type,
                              const int32_t* tokens, const int32_t* lens, const int32_t* labels,
                              int has_labels);
/* element type of the resident batch */
int rau_batch_feat_type(rau_ctx* ctx, int* feat_type);

/* ---- image tables: questions of one image share its feature map --------------------------------
 * VQA asks several questions per image, so a batch may carry each distinct map once: feats is then a
 * TABLE [n_images,D,S] (1 <= n_images <= B) of feat_type elements and image_of [B] (host, int32) gives
 * the 0-based table row sample b looks at; tokens, lens and labels stay per sample.  Only n_images*D*S
 * elements are uploaded.  The evaluate-mode forward computes i_embed and the attention pre-activation
 * once per image and its attention kernels read sample b's tiles at row image_of[b]: results are BIT-
 * IDENTICAL to the plain batch feats[image_of].  Every other consumer (train-mode forward,
 * rau_graph_step, module-level calls with X == NULL) first gathers the table into per-sample maps on
 * the device and then runs as on a plain batch; a captured step reads table and index from device
 * memory, so a new table or a new n_images replays without recapture.  rau_backward after an evaluate-
 * mode forward of a table batch is RAU_ERR_STATE (there is no per-sample I): take evaluate-mode
 * gradients on plain batches.  image_of is range-checked like the token ids: an entry outside
 * [0, n_images), or n_images outside [1, B], is RAU_ERR_INVALID and nothing is uploaded.  The index and
 * the gathered copy are allocated at a context's first table batch.
 * rau_set_batch_images is the synchronous form (feats NULL: the resident buffer already holds the
 * table).  rau_set_batch_async_images is the slot form; feats NULL: the slot's pinned staging
 * (rau_batch_slot) already holds n_images*D*S elements of feat_type at its start.  Whether a slot holds
 * a table belongs to the batch in it, like the element type: rau_use_batch makes it current.
 * rau_batch_images: 0 for a plain resident batch, else its n_images. */
int rau_set_batch_images(rau_ctx* ctx, const void* feats, int feat_type, int n_images,
                         const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                         const int32_t* labels);
int rau_set_batch_async_images(rau_ctx* ctx, int slot, const void* feats, int feat_type, int n_images,
                               const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                               const int32_t* labels, int has_labels);
int rau_batch_images(rau_ctx* ctx, int* n_images);

/* ---- feature bank: every image's map once in device memory, batches name their images by row ---
 * A context may own ONE bank of `capacity` maps of D x S elements of feat_type, stored in the layout of the
 * batch buffers (row pitch S rounded up to a multiple of 4), so a map is one contiguous run; offsets into
 * the bank are 64-bit (it may exceed 4 GiB).  After the bank has been filled, a batch is tokens, lengths,
 * labels and ROW NUMBERS: no feature byte is staged or crosses the bus during a step.
 *   rau_bank_create   a second bank is RAU_ERR_STATE; an allocation that does not fit is RAU_ERR_NOMEM and
 *                     leaves the context as it was.
 *   rau_bank_destroy  frees it (rau_destroy does too); a batch drawn from it is no longer resident.
 *   rau_bank_info     capacity, element type, number of distinct rows written so far (any may be NULL);
 *                     RAU_ERR_STATE without a bank, like every call below.
 *   rau_bank_put      host feats [count,D,S] of src_type into rows [first, first+count), in chunks through
 *                     pinned staging; synchronising.  src_type equal to the bank's type is a copy;
 *                     RAU_FEAT_F32 into a 16-bit bank is narrowed ON THE DEVICE, round to nearest even: the
 *                     bits of numpy's float16 conversion (subnormals kept, overflow to infinity) and of
 *                     bf16 rounding for every finite input.  RAU_FEAT_F32 into an fp8 bank is narrowed on the
 *                     device too, round to nearest even and SATURATING: every result beyond the largest finite
 *                     value (448 / 57344) becomes that value with the input's sign, +-inf included (a clipped
 *                     activation is usable; a NaN would poison a hop's softmax); NaN becomes a NaN code;
 *                     magnitudes at or below half the smallest subnormal become +-0.  With mbits = 3 | 2, bias =
 *                     7 | 15, emin = 1 - bias: a = |x|, e = max(floor(log2 a), emin), q = 2^(e - mbits),
 *                     r = min(rint(a / q) * q, largest finite), rint to nearest even; r is encoded, as a
 *                     subnormal when r < 2^emin, under the input's sign bit -- bit for bit what
 *                     rau_vqa_amd.feat16.fp8_bits computes, not any vendor's conversion routine.
 *                     Any other pair of types (f16 -> e4m3, e4m3 -> e5m2, ...) is RAU_ERR_INVALID, as
 *                     is a row range outside [0, capacity).  It first waits for all enqueued work that reads
 *                     the bank, so it may be called between steps to add or replace rows; a batch that was
 *                     handed over BEFORE the put and is consumed after it may see either version of a
 *                     replaced row.
 *   rau_bank_get      rows [first, first+count) as dense [count,D,S] in the bank's type; synchronising.
 * rau_set_batch_bank / rau_set_batch_async_bank mean exactly rau_set_batch_images /
 * rau_set_batch_async_images with feats = bank[bank_rows] ([n_images] host int32) in the bank's element
 * type: the same mode rules, RAU_ERR_STATE for a backward after an evaluate-mode forward, slot and
 * rau_use_batch semantics, replay under rau_graph_step without recapture, rau_batch_images and
 * rau_batch_feat_type; results are BIT-IDENTICAL to that table batch.  The slot form gathers on the copy
 * stream behind the same events as an upload and touches no feature staging.  The table itself is gathered
 * when the batch is handed over in evaluate mode (else by the first evaluate-mode forward that wants it);
 * the consumers of per-sample maps gather those from the bank in one pass, so after a bank batch
 * rau_batch_feats is defined only once an evaluate-mode forward has run.
 * Nothing is enqueued on failure: no bank -> RAU_ERR_STATE; n_images outside [1,B], an image_of entry
 * outside [0,n_images), a row outside [0,capacity) -> RAU_ERR_INVALID; a row that was never written
 * (host-side record of rau_bank_put) -> RAU_ERR_STATE. */
int rau_bank_create(rau_ctx* ctx, int32_t capacity, int feat_type);
int rau_bank_destroy(rau_ctx* ctx);
int rau_bank_info(rau_ctx* ctx, int32_t* capacity, int* feat_type, int32_t* rows_filled);
int rau_bank_put(rau_ctx* ctx, int32_t first, int32_t count, const void* feats, int src_type);
int rau_bank_get(rau_ctx* ctx, int32_t first, int32_t count, void* feats);
int rau_set_batch_bank(rau_ctx* ctx, int n_images, const int32_t* bank_rows, const int32_t* image_of,
                       const int32_t* tokens, const int32_t* lens, const int32_t* labels);
int rau_set_batch_async_bank(rau_ctx* ctx, int slot, int n_images, const int32_t* bank_rows,
                             const int32_t* image_of, const int32_t* tokens, const int32_t* lens,
                             const int32_t* labels, int has_labels);

/* ---- asynchronous, double-buffered upload: SS:434-439 behind the loader's prefetch -------------
 * The reference re-uploads feats / x / x_len / y every iteration (SS:434-439) while its loader's
 * worker thread assembles the next batch (utils/vqa_prepro_loader.lua:931-958).  Here the ctx owns
 * TWO batch slots, each with device buffers and PINNED host staging:
 *   rau_batch_slot(slot)       -> host pointers of the slot's staging (feats [B,D,S], tokens [T,B],
 *                                 lens [B], labels [B]); the loader assembles the batch in place.  The four
 *                                 pointers never move (each array has room for the capacity); a batch of the
 *                                 current size n is written DENSE in n: [n,D,S], [T,n], [n], [n].
 *                                 Waits (on the host) until the slot's previous upload has left it:
 *                                 CALL IT BEFORE EVERY IN-PLACE REFILL, never cache its pointers across
 *                                 iterations (the host may run two steps ahead of the copy stream).
 *   rau_set_batch_async(slot, feats, tokens, lens, labels, has_labels)
 *                              -> checks the ids, builds the token index (host), enqueues the H2D
 *                                 copies on a dedicated copy stream and returns; no stream is
 *                                 synchronised.  A NULL pointer = "already in the slot's staging";
 *                                 a non-NULL one is copied into it first (one host memcpy).
 *                                 has_labels tells whether in-place labels are present.
 *   rau_use_batch(slot)        -> the slot becomes the resident batch; the step's streams are ordered
 *                                 behind its upload by an event, not by a host wait.
 * Upload batch n+1 into the other slot while step n runs; the copy stream itself waits for the last
 * step that read the slot being refilled.  rau_set_batch stays the synchronous form (it writes the
 * current slot). */
int rau_batch_slot(rau_ctx* ctx, int slot, float** feats_host, int32_t** tokens_host,
                   int32_t** lens_host, int32_t** labels_host);
int rau_set_batch_async(rau_ctx* ctx, int slot, const float* feats, const int32_t* tokens,
                        const int32_t* lens, const int32_t* labels, int has_labels);
int rau_use_batch(rau_ctx* ctx, int slot);

/* ---- answer sets: multi-answer ground truth on a batch ------------------------------------------
 * Every VQA question has ten human answers.  An answer set gives a batch, per sample, up to RAU_MAX_ANSWERS
 * weighted answers in place of the one label: ids [n,G] int32 (1..K, or 0 for an empty entry), w [n,G] f32 loss
 * weights, score [n,G] f32 metric scores (NULL: use w); n = the current batch size, 1 <= G <= RAU_MAX_ANSWERS.
 * Entries with id 0 are ignored whatever their weight; duplicate ids in a row are allowed and add up; a row with
 * no entry is an unlabelled sample: zero loss, zero gradient, never "correct".
 *   slot = -1      the resident batch; synchronising, like rau_set_batch.
 *   slot = 0 | 1   a slot of the asynchronous path: call it after rau_set_batch_async* on that slot and before
 *                  rau_use_batch; the copies are enqueued on the copy stream behind the slot's batch and nothing
 *                  is synchronised (a second set for the same upload first waits for the first one's copy).
 * The set belongs to the slot's batch: any later batch upload into that slot and rau_set_batch_size clear it,
 * rau_use_batch makes it current together with the batch, an upload into the other slot leaves it alone.  It
 * REPLACES the batch's labels in the criterion head of rau_forward / rau_graph_step, in rau_step_stats, and in
 * rau_criterion_forward / _backward called with labels_dev == NULL; a batch uploaded with labels == NULL and
 * then given a set counts as labelled.  A forward that has run on the batch must be run again before
 * rau_backward or rau_step_stats.  A batch without a set computes bit for bit what it did before sets existed.
 * With lse the row's log-sum-exp, invB = 1/n and W_b = sum_g w[b,g] over the non-empty entries in order g = 0..G-1:
 *   loss row   sum_g w[b,g] (lse - logit[y_g]), accumulated from 0 in g order (rau_get_losses: their mean over n)
 *   d_logits   (expf(logit[k] - mx) / den) (W_b invB) -- mx the row's maximum, den = sum_k expf(logit[k] - mx), so that
 *              the probabilities of a row at |logit| ~ 1e4 still sum to 1 --, then for g = 0..G-1 in order: if (ids[b,g] - 1 == k) -= w[b,g] invB
 * every step's rounding is fixed (ce_set.hip: the first matching entry of a logit is subtracted inside the product's
 * fused multiply-add, as the label path does), so duplicates are deterministic and G = 1, w = 1 gives the bits of
 * the label path.  rau_graph_step keys its cache by G: a step captured without a set, or with another G, is never replayed.
 * Errors, nothing uploaded, the previous set stays in force: RAU_ERR_INVALID for G out of range, an id outside
 * 0..K, a negative or non-finite weight or score; RAU_ERR_STATE when the slot holds no batch, or (slot 0 | 1) it
 * is the current batch of a forward whose backward has not run.
 * rau_batch_answers: the G of the resident batch's set, 0 when it has none. */
#define RAU_MAX_ANSWERS 16
int rau_set_answers(rau_ctx* ctx, int slot, int32_t G, const int32_t* ids, const float* w,
                    const float* score);
int rau_batch_answers(rau_ctx* ctx, int32_t* G);

/* ---- region counts: attention over a sample's valid positions only -------------------------------
 * Region features (bottom-up attention: 10-100 boxes per image) and aspect-preserving grids are stored
 * prefix-packed and padded to S positions.  Region counts tell the attention which positions of a sample are
 * real: n [batch] int32 host, 1 <= n[b] <= S.  Sample b attends to positions 0 .. n[b]-1; positions >= n[b] get
 * attention exactly 0 in every hop, in train and evaluate mode, and with it gradient exactly 0 (the context sum,
 * the softmax gradient, both conv gradients' terms at those positions and the attbymemory / feat_attprob weight
 * gradients are all multiplied by that 0).  The features at masked positions must be finite (zero is
 * recommended); they then influence no output and no gradient.  A count of 0 is invalid -- a softmax over nothing
 * has no value: a caller with an empty image passes 1 and a zero map.
 * n is always per SAMPLE: for an image-table or bank batch the host gathers n_image[image_of[b]] (4 bytes per
 * sample, no feature byte added to the link).
 *   slot = -1      the resident batch; synchronising, like rau_set_batch.
 *   slot = 0 | 1   a slot of the asynchronous path: call it after rau_set_batch_async* on that slot and before
 *                  rau_use_batch; the copy is enqueued on the copy stream behind the slot's batch and nothing is
 *                  synchronised (a second call for the same upload first waits for the first one's copy).
 * The counts belong to the slot's batch: any later batch upload into that slot and rau_set_batch_size clear them,
 * rau_use_batch makes them current together with the batch, an upload into the other slot leaves them alone.  A
 * forward that has run on the batch must be run again before rau_backward.  A batch without counts computes bit
 * for bit, launch for launch, what it did before counts existed; counts all equal to S give the same bits too.
 * rau_graph_step keys its cache by "has counts": a step captured without them is never replayed for a batch with
 * them, nor the other way round.  The merged hops (rau_get_merged, rau_predict, rau_topk, rau_step_stats) read
 * the attention and logits the forward left and so see the masked model.
 * Errors, nothing uploaded, the previous counts stay in force: RAU_ERR_INVALID for a count outside 1..S;
 * RAU_ERR_STATE when the slot holds no batch, or (slot 0 | 1) it is the current batch of a forward whose backward
 * has not run.
 * rau_batch_regions: *has = 1 when the resident batch carries counts, else 0. */
int rau_set_regions(rau_ctx* ctx, int slot, const int32_t* n /* [batch] host */);
int rau_batch_regions(rau_ctx* ctx, int* has);

/* ---- per-sample loss weights: every training term of the step path, weighted per sample ------------
 * Every objective the step path trains is a mean over the batch, (1/n) sum_b row_b: the answer criterion (softmax
 * CE with labels, soft-target CE with an answer set, the sigmoid head), the step-selection BCE, the attention
 * supervision and the two merged rows.  With weights s [n] on the batch each becomes (1/n) sum_b s_b row_b.  The
 * library NEVER renormalises: whether sum s = n is the caller's decision.  Uses: class- or question-type-balanced
 * training, down-weighting noisy questions, importance sampling, switching single rows of a batch off (s_b = 0).
 * s [n] float32 host, n the current batch size; every entry finite and >= 0; NULL detaches the weights (nothing is
 * copied; a forward that ran with them must be run again).  The weights are always per SAMPLE, on plain, typed,
 * packed, image-table, bank and device (rau_set_batch_dev*) batches, with or without an attached question.
 * slot = -1 | 0 | 1, ownership and lifetime are exactly those of rau_set_regions: -1 is the resident batch and
 * synchronises; 0 | 1 is a slot of the asynchronous path, between rau_set_batch_async* and rau_use_batch, enqueued
 * on the copy stream, nothing synchronised; the weights belong to the slot's batch; a later upload into that slot,
 * or rau_set_batch_size, clears them; rau_use_batch makes them current with the batch.  The forward's criterion
 * head reads them: a forward that has run on the batch must be run again before rau_backward.
 * Arithmetic, float32, every product rounded once (invB = 1 / n):
 *   answer criterion and merged rows   invB is replaced by s_b * invB wherever it is used (W invB, w_g invB, the
 *                                      sigmoid head's (sigmoid - t) invB); the loss row written is s_b * row
 *   selection BCE                      select_w[h] is replaced by select_w[h] * s_b, the rest unchanged
 *   attention supervision              att_w[h] is replaced by att_w[h] * s_b, the rest unchanged
 *   statistics                         rau_get_losses, rau_get_loss_rows and rau_step_stats' loss[0..H) are the
 *                                      weighted rows' means; rau_step_stats' uni / select losses and loss_do_pred
 *                                      and rau_att_stats' loss take s_b per row (s_b * row, then the mean)
 * UNWEIGHTED, always: every count, rau_att_stats' mass, hits and n_sup, the metric scores (rau_step_scores,
 * rau_predict_scores), rau_predict, rau_topk.  Caller-supplied gradients (rau_out_grads) are the caller's and are
 * not weighted.  Module-level criteria do not read the weights (rau_dev_scale_rows weights their gradients).
 * A batch without weights computes and launches exactly what it did before weights existed; weights all equal to
 * 1 give the same bits (1 * invB is exact).  A sample with s_b = 0 contributes exactly zero to d_logits, to the
 * select signal, to the attention addend, to the merged terms and to every loss.  No atomics, no device scratch,
 * the same bits on every call; one 4-byte load per workgroup that owns a row.
 * rau_graph_step keys its cache by "has weights": a step captured without them is never replayed for a batch with
 * them, nor the other way round; a replay reads the current weights of the resident batch.
 * Errors, nothing uploaded, the previous weights stay in force: RAU_ERR_INVALID for a negative or non-finite
 * weight; RAU_ERR_STATE when the slot holds no batch, or (slot 0 | 1) it is the current batch of a forward whose
 * backward has not run.
 * rau_batch_sample_weights: *has = 1 when the resident batch carries weights, else 0. */
int rau_set_sample_weights(rau_ctx* ctx, int slot, const float* s /* [batch] host; NULL = detach */);
int rau_batch_sample_weights(rau_ctx* ctx, int* has);

/* ---- multiple-choice candidates: the criterion restricted to a sample's candidate answers ---------------
 * VQA v1 gives every question 18 candidate answers, Visual7W four; answer-type restricted evaluation has the same
 * shape.  Candidates tell the criterion head which answers a sample is normalised over: cand [n,C] int32 host,
 * cand[b,c] an answer id in 1..K or 0 for an empty entry, n the current batch size, 1 <= C <= RAU_MAX_CANDIDATES.
 * A duplicate id in a row counts once: an entry equal to an earlier entry of the row is dead.  L_b = the live
 * entries of row b.  A row with no live entry is an unlabelled sample: loss 0, gradient +0.  NULL or C == 0
 * detaches the list (nothing is copied; a forward that ran with it must be run again).
 * slot = -1 | 0 | 1, ownership and lifetime are exactly those of rau_set_answers: -1 is the resident batch and
 * synchronises; 0 | 1 is a slot of the asynchronous path, between rau_set_batch_async* and rau_use_batch, enqueued on
 * the copy stream, nothing synchronised; the list belongs to the slot's batch; a later upload into that slot, or
 * rau_set_batch_size, clears it; rau_use_batch makes it current with the batch.  A forward that has run on the batch
 * must be run again before rau_backward or the statistics.  Works on plain, typed, packed, image-table, bank and
 * device batches, with or without an attached question.
 * With candidates the criterion head of rau_forward / rau_graph_step is cand_head.hip's kernel in place of the
 * full-vocabulary one.  Unchanged: the logits, do_pred, the argmax over ALL K (rau_get_argmax, the open-ended answer,
 * the step-selection head's target).  Restricted, with x the row's logits and invB = s_b / n (s_b the sample weight,
 * or 1):
 *   kept truth  set entries (rau_set_answers), or the label as the set {(y, 1)}, whose id is not in L_b are dropped:
 *               they count as empty entries
 *   softmax     m = max_{c in L} x_c; den = sum_{c in L} expf(x_c - m), added from +0 in entry order; lse = m + logf(den);
 *               W = the kept weights added in entry order
 *               loss row   sum_g w_g (lse - x[y_g]) over the kept entries in order, times s_b last
 *               d_logits   k in L: (expf(x_k - m) / den) (W invB), then for the kept g in order: if (y_g == k) -= w_g invB
 *                          (the first match inside the product's fused multiply-add, as at rau_set_answers);
 *                          k not in L: +0.  A row without a kept entry is unlabelled.
 *   sigmoid     (RAU_LOSS_BCE) t_c = min(1, the kept matching weights added in order);
 *               loss row   sum_{c in L} max(x_c,0) - x_c t_c + log1p(exp(-|x_c|)), from +0 in entry order, times s_b
 *               d_logits   k_c in L: (sigmoid(x_c) - t_c) invB; +0 elsewhere.  A row is labelled when its kept set has
 *               a non-empty entry.
 * So a row whose one live candidate is its truth has loss 0 and gradient 0 up to the rounding of expf(0).  No atomics,
 * no device scratch, the same bits on every call.  Everything downstream of d_logits and the loss rows (hop_w,
 * select_w, att_w, rau_backward_ext, region counts, sample weights, tied dropout, the feature-map and question
 * gradients, bf16 mode, any K) works unchanged; rau_get_losses, rau_get_loss_rows and rau_step_stats' loss[0..H) are
 * the restricted rows.  Everything else of rau_step_stats, and rau_step_scores, rau_predict, rau_topk and
 * rau_predict_scores, stay open-ended statistics over all K; the MC ones are rau_cand_stats / rau_topk_cand below.
 * The deliberate gap: the merged rows' terms (merge_w) are full-vocabulary cross-entropies, so a non-zero merge_w on
 * a batch with candidates is RAU_ERR_INVALID, nothing launched, in rau_backward_merged, rau_backward_ext and
 * rau_graph_step_merged (NULL or zeros stays the path without it).
 * A batch without candidates computes and launches exactly what it did before candidates existed.  rau_graph_step
 * keys its cache by C: a step captured without candidates, or with another C, is never replayed; a replay reads the
 * current list of the resident batch.
 * Errors, nothing uploaded, the previous list stays in force: RAU_ERR_INVALID for C out of range or an id outside
 * 0..K; RAU_ERR_STATE when the slot holds no batch, or (slot 0 | 1) it is the current batch of a forward whose
 * backward has not run, or while a step is being captured.
 * rau_batch_candidates: the C of the resident batch's list, 0 when it has none. */
#define RAU_MAX_CANDIDATES 32
int rau_set_candidates(rau_ctx* ctx, int slot, int32_t C, const int32_t* cand /* [n,C] host; NULL or C == 0: detach */);
int rau_batch_candidates(rau_ctx* ctx, int32_t* C);

/* ---- packed region features: rows as the files store them, unpacked on the device ------------------
 * Region feature files hold one row of D values per box.  A packed batch hands those rows over as they are:
 * rows [sum(counts), D] of feat_type elements, row-major, map i owning counts[i] consecutive rows (1 <= counts[i]
 * <= S), n_maps maps in all.  Only sum(counts) * D elements cross the link; one kernel (packed.hip) transposes them
 * into the slot's feature buffer [n_maps, D, Sp] and writes zero bits behind each count, pad columns included, and
 * the counts become the batch's region counts in the same call.  With off the exclusive prefix sum of counts,
 *   dense[i, d, s] = rows[off[i] + s, d] for s < counts[i], all bits zero (+0 in every type) elsewhere
 * (rau_vqa_amd.feat16.unpack_regions), and a packed batch gives, BIT FOR BIT, the results of the dense batch `dense`
 * followed by rau_set_regions with counts (image_of == NULL: a plain batch, n_maps must equal the batch size) or
 * with counts[image_of[b]] (an image table of n_maps maps, image_of [batch] as at rau_set_batch_images) -- in both
 * modes, under rau_graph_step, at module level with X == NULL and in the merged hops.  rau_batch_feats,
 * rau_batch_images, rau_batch_feat_type and rau_batch_regions report what they report for that dense batch; a later
 * upload into the slot or rau_set_batch_size clears the counts, a later rau_set_regions replaces them.
 *   rau_set_batch_packed        synchronising, like rau_set_batch; rows must not be NULL.
 *   rau_set_batch_async_packed  the slot form: rows == NULL means the slot's pinned staging (rau_batch_slot) already
 *                               holds the sum(counts) * D elements at its start.  The H2D copy of the rows, the
 *                               unpack and the counts are enqueued on the copy stream behind the slot's events,
 *                               where an upload's copies go; nothing is synchronised.
 *   rau_bank_put_packed         rau_bank_put for packed rows: maps [first, first+count) from rows [sum(counts), D]
 *                               of src_type, the same type pairs (f32 is narrowed on the device with the bits of
 *                               rau_bank_put), chunking through pinned staging, quiescing and row bookkeeping.  The
 *                               bank keeps dense maps: rau_bank_get returns the unpacked [count, D, S].  Counts are
 *                               not stored in the bank; the host keeps them and passes rau_set_regions what a bank
 *                               batch needs.
 * The raw rows land in a device staging block per slot, sized for the capacity and allocated at the slot's first
 * packed batch: a context that never sends one allocates and launches exactly what it did.
 * Errors, nothing enqueued, the previous batch still resident: RAU_ERR_INVALID for a count outside 1..S, n_maps
 * outside [1, batch], n_maps != batch without image_of, an image_of entry outside [0, n_maps), an unknown type;
 * the slot and state rules of rau_set_batch_async_images; RAU_ERR_NOMEM from the staging allocation leaves the
 * context usable. */
int rau_set_batch_packed(rau_ctx* ctx, const void* rows, int feat_type, int n_maps, const int32_t* counts /* [n_maps] host */,
                         const int32_t* image_of /* NULL: plain batch */, const int32_t* tokens, const int32_t* lens,
                         const int32_t* labels);
int rau_set_batch_async_packed(rau_ctx* ctx, int slot, const void* rows, int feat_type, int n_maps,
                               const int32_t* counts, const int32_t* image_of, const int32_t* tokens,
                               const int32_t* lens, const int32_t* labels, int has_labels);
int rau_bank_put_packed(rau_ctx* ctx, int32_t first, int32_t count, const void* rows, int src_type,
                        const int32_t* counts /* [count] host */);

/* ---- the hot path ------------------------------------------------------------
 * rau_forward : SS:443-520  encoder unroll, length select, H-hop RAU, per-hop
 *               CrossEntropyCriterion forward, first-max argmax.
 * rau_backward: SS:561-596  per-hop criterion backward scaled by hop_w[h]
 *               (SS:569 nHop / MS:568-570 one / Full:587-589 0|1), RAU BPTT,
 *               gradattprob=0, dq=sum over hops, encoder BPTT, LookupTable
 *               scatter; the gradient at do_pred is the reference's zero (SS:566)
 *               here and per-hop weighted in rau_backward_select below.
 *               Gradients ACCUMULATE into the flat grad buffers like
 *               accGradParameters; call rau_zero_grads first. */
int rau_forward(rau_ctx* ctx);
int rau_backward(rau_ctx* ctx, const float* hop_w /* [H] host */);

/* ---- training the step-selection head ----------------------------------------------------------
 * do_pred = sum(sigmoid(Linear(M,1)(merge_feat))) (SS:281) decides every "select" output.  The reference forms
 * its BCE gradient (criterion SS:555, :backward SS:565) and multiplies it by 0 (SS:566, the script's "DontSelect").
 * rau_backward_select makes that multiplier a per-hop argument: select_w [H] host, NULL = zeros.
 * For hop h and row b of the last step-level forward, n = the current batch size, x = do_pred[h,b], float32:
 *   t   = rau_step_stats' do_pred_gt: 1 when the hop's first-max answer equals the label, or (answer set) is
 *         among the row's non-empty ids with a positive score; else 0.  A constant: no gradient flows through it.
 *   ddp = select_w[h] * ( -(t - x) / ((1 - x + eps) * (x + eps)) ) / n,   eps = 1e-12f, in this order
 *         (nn.BCECriterion:backward with sizeAverage, scaled where the reference scales it)
 *   s   = ddp * x * (1 - x)                                                (through the sigmoid)
 *   dmf[h,b,:] += s * do_pred.weight, in front of the merge_feat dropout mask;
 *   d(do_pred.weight) += sum_{h,b} s mf[h,b,:],  d(do_pred.bias) += sum_{h,b} s, summed in a fixed order (no
 *   float atomics: repeated calls give the same bits); f32 dot products in every dtype, like the head itself.
 * Active hops: [0, HA), HA - 1 the last hop with hop_w[h] != 0 or select_w[h] != 0; hops behind it are skipped.
 * select_w == NULL or all zeros IS rau_backward: the same launches, the same bits.  Otherwise the forward's labels
 * or answer set must still be there: RAU_ERR_STATE, nothing launched, when that batch had neither or its slot has
 * been uploaded into since (the rule of rau_step_stats); every state rule of rau_backward applies as well.  A
 * non-finite weight in either array: RAU_ERR_INVALID.  Its scratch ([H,B,M] floats) is allocated at the first
 * call with a non-zero weight.
 * rau_graph_step_select is rau_graph_step with that backward: select_w is read from device memory like hop_w, so
 * it may change between replays; whether any entry is non-zero joins the cache key with the active-hop count. */
int rau_backward_select(rau_ctx* ctx, const float* hop_w /* [H] host */, const float* select_w /* [H] host, NULL = zeros */);
int rau_graph_step_select(rau_ctx* ctx, const float* hop_w, const float* select_w, int zero_grads_first);

/* ---- attention supervision: train attprob on per-sample target maps ---------------------------------
 * The fifth output of multimodal, the attention map (SS:306-307), gets the reference's constant zero gradient
 * (gradattprob, SS:361, handed to every multimodals[h]:backward, SS:573).  With target maps on the batch -- human
 * attention maps on grids, ground-truth boxes on region features -- rau_backward_att puts a loss there.
 *
 * Targets: t [n,S] float32 host, dense; n the current batch size, S the configured position count; every entry
 * finite and >= 0.  Rows are not normalised by the library: a caller who wants a distribution passes one.  A row
 * of zeros is an UNSUPERVISED sample: zero loss, zero gradient, not counted in the statistics.  Targets are always
 * per SAMPLE, also for image-table and bank batches (a map belongs to a question).  With region counts on the
 * batch (rau_set_regions) positions s >= n_reg[b] are ignored whatever they hold.
 * slot = -1 | 0 | 1, ownership and lifetime are exactly those of rau_set_regions: the targets belong to the slot's
 * batch; a later upload into that slot, or rau_set_batch_size, clears them; rau_use_batch makes them current; the
 * slot form enqueues on the copy stream behind the slot's batch and synchronises nothing; device and pinned blocks
 * are allocated at the slot's first set.  One difference: the forward does not read targets, so setting them after
 * a forward needs no second forward.
 * Errors, nothing uploaded, the previous targets stay in force: RAU_ERR_INVALID for a negative or non-finite
 * entry; RAU_ERR_STATE when the slot holds no batch, or (slot 0 | 1) it is the current batch of a forward whose
 * backward has not run.
 * rau_batch_att_targets: *has = 1 when the resident batch carries targets, else 0.
 *
 * The loss of hop h, with a = attprob of the last step-level forward and eps = 1e-12f (nn.BCECriterion's):
 *   ATT_h = (1/n) * sum_b sum_{s < n_reg[b]} t[b,s] * ( -log(a[h,b,s] + eps) )
 * and the step's objective becomes sum_h hop_w[h]*CE_h + select_w[h]*BCE_h + att_w[h]*ATT_h.
 * The gradient at the attprob output, float32, every operation rounded once, in this order:
 *   da[h,b,s] = -( (att_w[h] * t[b,s]) / (a[h,b,s] + eps) ) / n
 * exactly +0 where t[b,s] == 0 and where s >= n_reg[b].  It enters the attention backward in front of the softmax
 * gradient, where the reference adds its zeros.  Because of eps it is finite for every a >= 0; the softmax
 * gradient multiplies it by a, so where the softmax has underflowed to 0 the gradient VANISHES: a target on a
 * position whose attention is exactly 0 (in particular one behind a region count) cannot pull it back.
 * rau_backward_att: att_w [H] host, NULL = zeros.  att_w == NULL or all zeros IS rau_backward_select with the other
 * two arguments: the same launches, the same bits, whether or not the batch carries targets.  Active hops: [0, HA),
 * HA - 1 the last hop with any of the three weights non-zero.  A non-zero att_w on a batch without targets:
 * RAU_ERR_STATE, nothing launched.  A non-finite weight: RAU_ERR_INVALID.  The scratch ([H,B,Sp] floats) is
 * allocated at the first call with a non-zero att_w.
 * rau_graph_step_att is rau_graph_step_select with that backward: att_w is read from device memory like hop_w, so
 * it may change between replays; "any att_w non-zero" and "batch has targets" join the cache key.
 *
 * rau_att_stats: what a training loop logs, of the last step-level forward (train or evaluate mode; the rule of
 * rau_step_stats) against its batch's targets; RAU_ERR_STATE without such a forward or without targets.  A row is
 * supervised when some t[b,s] > 0 with s < n_reg[b].
 *   loss[h]  = ATT_h
 *   mass[h]  = mean over the supervised rows of sum_s a[h,b,s] * [t[b,s] > 0]     (0 when there is none)
 *   hits[h]  = supervised rows whose first-max attention position has t > 0      (the pointing game)
 *   *n_sup   = supervised rows
 * Positions behind a region count are excluded from all of them.  Sums run in a fixed order without float
 * atomics: repeated calls give the same bits.  Any output may be NULL. */
int rau_set_att_targets(rau_ctx* ctx, int slot, const float* t /* [n,S] host, dense */);
int rau_batch_att_targets(rau_ctx* ctx, int* has);
int rau_backward_att(rau_ctx* ctx, const float* hop_w, const float* select_w /* NULL = zeros */, const float* att_w /* NULL = zeros */);
int rau_graph_step_att(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w, int zero_grads_first);
int rau_att_stats(rau_ctx* ctx, float* loss /* [H] */, float* mass /* [H] */, int32_t* hits /* [H] */, int32_t* n_sup);

/* ---- training the merged answers: the uni and select cross-entropies in the backward ----------------
 * The answers handed out at test time are merged over the hops: the "uni" row, the mean of the hop logits (SS:482,
 * 522), and the "select" row, the logits of the first hop whose do_pred fires (SS:505-507).  feval logs their
 * cross-entropies (SS:521-557: rau_step_stats' loss[H] and loss[H+1]) and trains neither.  With
 * merge_w = {w_uni, w_sel} (host, NULL = zeros) the step's objective becomes
 *   sum_h ( hop_w[h]*CE_h + select_w[h]*BCE_h + att_w[h]*ATT_h ) + w_uni * CE(uni row) + w_sel * CE(select row)
 * The two rows are those of rau_step_stats, bit for bit: uni = (0 + l_0 + .. + l_{H-1}) / H, select = 0 + l_hsel with
 * hsel the first hop whose do_pred > 0.5 -- the FEVAL rule: the last hop is not forced, and a row on which no hop
 * fired has the constant zero row.  So the two terms are the numbers rau_step_stats reports; there is no new getter.
 * CE is the criterion's own against the forward's labels or answer set (rau_set_answers: the soft-target CE).
 * With g(row)[b,k] = d CE(row) / d row[b,k] -- (expf(row[k] - mx) / den) (W_b invB), then for each matching entry in order
 * -= w[b,g] invB, the rule and the roundings at rau_set_answers; a label is the set {y} with weight 1; invB = 1/n --
 * the gradient at the hop logits, added to d_logits[h] behind its scaling by hop_w[h] and in front of everything
 * that consumes it (the classifier's input, weight and bias gradients; with select_w the head's addend):
 *   uni     every hop h in [0, H) receives (w_uni / H) * g(uni row)[b,:]
 *   select  hop h receives w_sel * g(select row)[b,:] on the rows b with hsel(b) == h; a row on which no hop fired
 *           receives nothing in any hop
 * each product and each sum rounded once, uni first.  The gate do_pred > 0.5 is a constant: no gradient flows through
 * it, as none flows through t in rau_backward_select.  A term whose weight is zero is skipped, not added as zeros.
 * One launch for all hops, no float atomics: repeated calls give the same bits.
 * rau_backward_merged: merge_w == NULL or both entries zero IS rau_backward_att with the other three arguments: the
 * same launches, the same bits.  Otherwise every hop is active (HA = H: the uni row reads every hop), and the
 * forward's labels or answer set must still be there: RAU_ERR_STATE, nothing launched, when that batch had neither or
 * its slot has been uploaded into since (the rule of rau_step_stats); every state rule of rau_backward applies as
 * well.  A non-finite weight in any array: RAU_ERR_INVALID.  The two terms are cross-entropies: under RAU_LOSS_BCE
 * (rau_set_answer_loss) a non-zero merge_w is RAU_ERR_INVALID, nothing launched, here and in rau_graph_step_merged.
 * They are full-vocabulary cross-entropies too: on a batch with candidates (rau_set_candidates) a non-zero merge_w
 * is RAU_ERR_INVALID, nothing launched, here, in rau_backward_ext and in rau_graph_step_merged.
 * rau_graph_step_merged is rau_graph_step_att with that backward: merge_w is uploaded next to hop_w and read from
 * device memory, so it may change between replays; "any merge_w non-zero" joins the cache key.
 * rau_merge_criterion_backward, for hosts that call the clones one by one: logits_dev [H,n,K] and dopred_dev [H,n]
 * dense in DEVICE memory (the outputs of the H multimodal clones, stacked), labels_dev [n] int32 or NULL = the
 * resident batch's labels or answer set (RAU_ERR_STATE when it has neither); the two terms' gradient is ADDED into
 * d_logits_dev [H,n,K] (16-byte aligned), which holds the caller's scaled per-hop criterion gradients and then goes
 * hop by hop into rau_multimodal_backward.  Not synchronising. */
int rau_backward_merged(rau_ctx* ctx, const float* hop_w, const float* select_w /* NULL = zeros */,
                        const float* att_w /* NULL = zeros */, const float* merge_w /* [2] host: uni, select; NULL = zeros */);
int rau_graph_step_merged(rau_ctx* ctx, const float* hop_w, const float* select_w, const float* att_w,
                          const float* merge_w, int zero_grads_first);
int rau_merge_criterion_backward(rau_ctx* ctx, const float* logits_dev /* [H,n,K] */, const float* dopred_dev /* [H,n] */,
                                 const int32_t* labels_dev /* NULL: the resident batch's labels or answer set */,
                                 const float* merge_w /* [2] host */, float* d_logits_dev /* [H,n,K], added into */);

/* ---- custom objectives: the step-level backward from caller-supplied gradients -----------------------
 * For a term F(logits, do_pred, attprob) the library does not implement (distillation, de-biasing, focal or ranking
 * losses, an attention penalty, a rule of one's own for do_pred) the caller reads the three outputs of the last
 * step-level forward on the device, computes dF/d(output) there, and hands the gradients to the backward.  The
 * step's objective becomes
 *   sum_h ( hop_w[h]*CE_h + select_w[h]*BCE_h + att_w[h]*ATT_h ) + w_uni*CE(uni) + w_sel*CE(select) + F
 * rau_outputs_dev: ctx-owned DEVICE pointers to the outputs of the last step-level forward (rau_forward or a
 * rau_graph_step*); any out argument may be NULL.  n is the CURRENT batch size (rau_set_batch_size), not the
 * capacity, and every tensor is dense in it: logits [H,n,K] with strides (n*K, K, 1), dopred [H,n] with strides
 * (n, 1), attprob [H,n,pitch] with strides (n*pitch, pitch, 1), *att_pitch = pitch = S rounded up to a multiple of
 * 4 (columns S..pitch-1 hold zeros; behind a sample's region count the probabilities are zeros).
 * rau_logits_pitch: the logits have a pitch too where K % 4 != 0.  *pitch = K where K % 4 == 0 (dense rows, the
 * strides above), else K rounded up to a multiple of 4: the logits of rau_outputs_dev then have strides
 * (n*pitch, pitch, 1) with this pitch, and columns K..pitch-1 of every row hold +0.  The host-side getters
 * (rau_get_logits, rau_get_merged, rau_topk, ...) always return dense [.., K] rows, and the gradient
 * rau_backward_ext takes stays DENSE [H,n,K] whatever the pitch (d_logits below), as d_attprob does.  The pointers stay
 * valid until the next forward or rau_set_batch_size; their contents are ordered on the ctx's stream (rau_stream),
 * and the call synchronises nothing: a caller on another stream orders itself behind an event of that stream.
 * Read-only for the caller.  RAU_ERR_STATE when there has been no step-level forward (or a module-level call has
 * overwritten its slots).
 * rau_backward_ext: rau_backward_merged with g = {dF/dlogits, dF/ddo_pred, dF/dattprob}, all float32 in DEVICE
 * memory, dense in the current batch size (d_attprob at pitch S, NOT the attention's pitch), each NULL = no such
 * term; every operation below is float32, rounded once:
 *   logits   behind the scaling by hop_w[h] (the product of rau_backward, the same bits) x = x + d_logits[h,b,k], in
 *            front of the merged rows' terms and of every consumer (the classifier's input, weight and bias
 *            gradients; the head's addend).  The forward of a batch without labels or answer set forms no criterion
 *            gradient: then x = d_logits[h,b,k] exactly, or +0 without a d_logits.  One pass over [H,n,K].
 *   do_pred  s_ext = (d_dopred[h,b] * x) * (1 - x) with x = do_pred[h,b] (through the sigmoid: the last line of the
 *            rule at rau_backward_select); s = s_sel + s_ext with a select_w term, else s = s_ext; s * wd[m] enters
 *            the gradient at merge_feat in front of its dropout mask, and s the head's weight and bias gradient,
 *            exactly as rau_backward_select's s does.
 *   attprob  da[h,b,s] = (att_w's value at rau_backward_att) + d_attprob[h,b,s] with an att_w term, else
 *            d_attprob[h,b,s] exactly; positions behind a sample's region count receive exactly +0 whatever
 *            d_attprob holds there.
 * With any pointer non-NULL every hop is active (the host cannot see which rows are zero without a synchronisation),
 * and the backward forms the head's two input-gradient products itself, as a step with a select_w does.  g == NULL
 * or three NULL pointers, with a non-NULL hop_w, IS rau_backward_merged with the other four arguments: the same
 * launches, the same bits.  hop_w may be NULL (zeros) only with a gradient in g.
 * Labels: a batch with labels or an answer set is required exactly when a built-in term reads one -- a non-zero
 * entry in hop_w, select_w or merge_w; then every state rule of rau_backward_merged applies.  An external-only
 * backward (hop_w NULL or zeros, no select_w, no merge_w) runs on a batch uploaded without labels.  A non-zero att_w
 * needs the batch's targets, as in rau_backward_att.  Evaluate mode, image-table and bank batches, region counts, the
 * tied feature-map dropout, RAU_BF16 / RAU_F32S and both answer criteria work as in rau_backward; under RAU_LOSS_BCE
 * a non-zero merge_w stays RAU_ERR_INVALID.  One backward per forward, as everywhere.  A d_logits that is not
 * 16-byte aligned: RAU_ERR_INVALID, nothing launched.  The library cannot check DEVICE values: a non-finite entry in
 * g gives non-finite gradients, not an error; the three arrays must stay unchanged until the backward's launches
 * that read them are done (they are read on the ctx's stream, before rau_backward_ext's first GEMM).
 * No atomics: repeated calls give the same bits.  There is no captured variant: the gradients are computed between
 * the forward and the backward.  No gradient enters at the last hop's c' / h' (the reference's zeros, SS:561-562) or
 * at the question state. */
typedef struct rau_out_grads {
  const float* d_logits;   /* [H,n,K] DEVICE, dense (NOT pitched), 16-byte aligned; NULL = no such term */
  const float* d_dopred;   /* [H,n]   DEVICE, dense;                  NULL = no such term */
  const float* d_attprob;  /* [H,n,S] DEVICE, dense (NOT pitched);    NULL = no such term */
} rau_out_grads;
int rau_outputs_dev(rau_ctx* ctx, const float** logits /* [H,n,K] at rau_logits_pitch */, const float** dopred /* [H,n] */,
                    const float** attprob /* [H,n,pitch] */, int32_t* att_pitch);
int rau_logits_pitch(rau_ctx* ctx, int32_t* pitch);
int rau_backward_ext(rau_ctx* ctx, const float* hop_w /* [H] host, NULL = zeros */, const float* select_w,
                     const float* att_w, const float* merge_w, const rau_out_grads* g /* NULL = none */);

/* ---- feature-map gradient: the step-level backward as the head of a model whose image side is trained ----------
 * The reference forms the gradient at the feature map and throws it away (SS:579), and so does the step path by
 * default.  rau_set_feat_grad(ctx, 1) makes every step-level backward (rau_backward, _select, _att, _merged, _ext
 * and every rau_graph_step*) also leave
 *   dX[b,d,s] = sum_{h < HA} keep_h[b,d,s] * s_x * ( sum_m Wi[m,d] * dZ_h[b,m,s] )        (all float32)
 * behind: dZ_h the gradient at i_embed's pre-activation of hop h (what the two conv weight gradients read), keep_h
 * hop h's feature-map dropout bit (site RAU_MASK_X, caller-supplied or the seeded stream's: the bits the forward
 * used), s_x = 1/(1-p_x), HA the active hops.  Tied dropout: the one mask behind the product of the summed dZ.
 * Evaluate mode: no mask, scale 1.  Behind a sample's region count dZ is exactly 0 and so is dX.  Pitched maps
 * (S % 4 != 0): the mask is indexed over the logical [.., S] tensor, the result's pad columns are zeros.  RAU_BF16:
 * the product rounds both operands to bf16 and accumulates in f32, like every GEMM of that mode; mask and scale are
 * applied in f32 behind it.  For 16-bit and fp8 batches the gradient is with respect to the widened f32 values.
 *   the switch   off by default; between steps, in either mode.  While a step is being captured: RAU_ERR_STATE.
 *                Off, every entry point computes and launches exactly what it did without this call; on, the
 *                parameter gradients keep their bits.  The switch joins rau_graph_step's key.  The result buffer
 *                [capacity, D, pitch] (and one hop's worth of scratch) is allocated at the first call with on != 0 and
 *                survives rau_set_batch_size.
 *   order        no float atomics: repeated calls give the same bits, a captured step the eager step's.  The hops
 *                are added in f32 in a fixed order that depends on the backward's launch-group partition (groups in
 *                the backward's order, last group first, the hops of a group ascending).
 *   the result   is OVERWRITTEN by each backward, never accumulated (feature maps change with every batch);
 *                rau_zero_grads does not touch it.
 *   batches      RAU_FEAT_GRAD_SAMPLES (1): one map per sample -- plain, typed and packed batches, and
 *                rau_set_batch_dev below.  The backward of an image-table or bank batch is RAU_ERR_STATE with nothing
 *                launched and no gradient changed (in this mode a caller that shares images expands them on its
 *                side, x[image_of], in front of rau_set_batch_dev; mode 2 forms the per-image sum instead).
 *                RAU_FEAT_GRAD_IMAGES (2): on a batch with one map per sample the same launches and bits as mode 1.
 *                On an IMAGE-TABLE batch (rau_set_batch_images, rau_set_batch_async_images + rau_use_batch, a packed
 *                table with an image_of, rau_set_batch_dev_images below) the result is the gradient at the TABLE,
 *                  dT[i,d,s] = sum_{h < HA} sum_{b: image_of[b] = i} keep_h[b,d,s] * s_x * (Wi^T dZ_h[b])[d,s]
 *                as [N, D, pitch]: an image no sample names gets exact zeros, pad columns are zeros, the keep bits are
 *                indexed by SAMPLE (explicit or regenerated, as in mode 1), tied dropout takes the one-mask product of
 *                the summed dZ first.  Per hop launch the accumulator starts at +0 (the backward's first writing
 *                launch) or at the stored value, an image's samples are added in ascending b, each term
 *                keep ? g * s_x : 0 rounded once: with the identity table (N = n, image_of = 0..n-1) the bits are
 *                those of the plain batch under mode 1.  The per-sample [n,D,pitch] gradient is not formed.  The
 *                evaluate-mode forward of a table batch takes the gathered per-sample path under this mode (same
 *                output bits), so its backward exists: per-image saliency.  Bank batches stay refused in both modes.
 *                Any other value of `on`: RAU_ERR_INVALID.  rau_feat_grad reports the mode.
 *   the key      where the forward drew the feature-map bits inside its dropout pass they exist nowhere, and the
 *                backward regenerates them from (seed, step): with the switch on, a rau_set_dropout_seed with another
 *                key between a forward and its backward makes that backward RAU_ERR_STATE, nothing launched (run the
 *                forward again).  A captured step holds both passes and reads the key from device memory.
 *   ext          rau_backward_ext's rule stays: no gradient enters at the question state.
 * rau_feat_grad_dev: the ctx-owned DEVICE pointer to the last backward's result [rows, D, *pitch] (rows: the current
 * batch size n, or the table's N where the gradient was formed per image; *pitch = S rounded up to a multiple of 4),
 * ordered on the ctx's stream; synchronises nothing; valid until the next forward or rau_set_batch_size.
 * RAU_ERR_STATE when the switch is off or no backward has run since the last forward.  rau_feat_grad_rows: that
 * result's map count, under the same state rules.  rau_get_feat_grad: the download, dense [rows,D,S]; synchronises.
 * rau_set_batch_dev: rau_set_batch with the maps [n,D,S] float32, dense, already in DEVICE memory: one copy on the
 * ctx's stream (re-pitching where S % 4 != 0) into the resident buffer, in the layout an f32 batch has there; the
 * rest is rau_set_batch_typed(NULL, RAU_FEAT_F32, ..).  tokens / lens / labels are HOST arrays, copied into pinned
 * staging of the ctx before the call returns; the call waits for no device work (only, from the third call on, for
 * the index copy of the call two before it).  The caller orders the producer of feats_dev in front of the ctx's
 * stream (an event of its stream, waited on by rau_stream) and keeps feats_dev unchanged until the copy has run.
 * Answer sets, region counts and attention targets attach afterwards, as to any batch.
 * rau_set_batch_dev_images: the same for an image table -- table_dev holds n_images maps [N,D,S] float32, dense, in
 * DEVICE memory, image_of [n] is a HOST array checked like rau_set_batch_images' and staged in the same pinned halves;
 * N maps are copied on the ctx's stream.  No host wait.  RAU_ERR_STATE while a step is being captured. */
#define RAU_FEAT_GRAD_OFF 0
#define RAU_FEAT_GRAD_SAMPLES 1
#define RAU_FEAT_GRAD_IMAGES 2
int rau_set_feat_grad(rau_ctx* ctx, int on);
int rau_feat_grad(rau_ctx* ctx, int* on);
int rau_feat_grad_dev(rau_ctx* ctx, const float** dX, int32_t* pitch);
int rau_feat_grad_rows(rau_ctx* ctx, int32_t* rows);
int rau_get_feat_grad(rau_ctx* ctx, float* host /* [rows,D,S] dense */);
int rau_set_batch_dev(rau_ctx* ctx, const float* feats_dev /* [n,D,S] f32, dense, DEVICE */, const int32_t* tokens,
                      const int32_t* lens, const int32_t* labels);
int rau_set_batch_dev_images(rau_ctx* ctx, const float* table_dev /* [N,D,S] f32, dense, DEVICE */, int n_images,
                             const int32_t* image_of /* host [n] */, const int32_t* tokens, const int32_t* lens,
                             const int32_t* labels);

/* ---- per-position L2 normalisation of the feature maps, on the device ---------------------------------------------
 * Grid-feature pipelines (SAN, HieCoAtt, MCB, MLB, MUTAN on res5c maps) normalise every position's channel vector
 * before attention.  rau_set_feat_norm(ctx, RAU_XNORM_L2, eps) makes every step-level forward do that first, for each
 * map x [D,S] of the batch and each position s:
 *   nrm[s]  = sqrt(sum_d x[d,s]^2)               x widened exactly to float32 first, whatever the stored type
 *   xn[d,s] = x[d,s] * (1 / max(nrm[s], eps))    torch.nn.functional.normalize(x, p=2, dim=channel, eps=eps)
 * and everything behind it -- dropout in every form, both convs, the weight gradients that read the maps -- runs on
 * xn as on a float32 batch, launch for launch: the results are bit for bit those of a context with the switch off
 * that was given xn as a plain batch.  So 16-bit and fp8 maps are stored raw, widened exactly and normalised in f32.
 *   values       an all-zero position gives nrm = 0 and +0 outputs; pad columns (S <= s < pitch) of xn and nrm are
 *                +0; region counts do not enter (all S positions are normalised, the attention ignores what lies
 *                behind a count as before).  Non-finite inputs, and inputs whose sum of squares overflows float32,
 *                are outside the contract.
 *   order        the sum over D is a fixed-order float32 sum (each square and each addition rounded once, no fma, no
 *                atomics) that depends on (D, S, pitch) alone: the same map gives the same bits as a sample's map, a
 *                row of an image table and a bank row, in every call, eagerly and in a replay.
 *   maps         the pass runs over the maps the image side reads: the N table rows in the evaluate-mode forward of
 *                an image-table or bank batch, else the n per-sample maps.
 *   gradient     with rau_set_feat_grad on, one more launch takes the feature-map gradient back through the
 *                normalisation, in place: with G the gradient at xn, c[s] = sum_d G[d,s] xn[d,s] (the same fixed
 *                order) and r = 1 / max(nrm, eps):  dX = r (G - xn c) where nrm >= eps,  dX = r G (= G / eps) where
 *                nrm < eps (the forward is linear there).  rau_feat_grad_dev / rau_get_feat_grad then hold the
 *                gradient at the RAW maps (per image under RAU_FEAT_GRAD_IMAGES: an image no sample names keeps its
 *                zero row).  Pad columns stay +0.
 *   the switch   off by default (RAU_XNORM_NONE): such a context allocates, launches and computes exactly what it did
 *                without this call.  eps must be finite and > 0 (else RAU_ERR_INVALID, like an unknown kind); while
 *                a step is being captured: RAU_ERR_STATE.  Setting the same kind and eps again changes nothing.  Any
 *                change drops the last forward: no backward, statistics or outputs until a new forward has run.
 *                xn [capacity, D, pitch] and nrm [capacity, pitch] are allocated at the first call that turns the
 *                switch on (RAU_ERR_NOMEM leaves the switch as it was) and cleared by rau_set_batch_size, which
 *                keeps the switch.  Kind and the bits of eps join rau_graph_step's key; a replay normalises what
 *                the slot holds then.  The pass runs in every forward; xn is not cached across steps.
 * rau_feat_norm reports kind and eps (either pointer may be NULL).
 * rau_norm_feats_dev: the ctx-owned DEVICE pointers to the last forward's xn [rows, D, *pitch] and nrm [rows, *pitch]
 * (rows: N after an evaluate-mode table forward, else n), ordered on the ctx's stream; synchronises nothing; any
 * output pointer may be NULL.  RAU_ERR_STATE when the switch is off or no forward has run since it was set.
 * rau_get_norm_feats: the download, dense; synchronises; same state rules. */
#define RAU_XNORM_NONE 0   /* the default */
#define RAU_XNORM_L2   1
int rau_set_feat_norm(rau_ctx* ctx, int kind, float eps);
int rau_feat_norm(rau_ctx* ctx, int* kind, float* eps);
int rau_norm_feats_dev(rau_ctx* ctx, const float** xn, const float** nrm, int32_t* pitch, int32_t* rows);
int rau_get_norm_feats(rau_ctx* ctx, float* xn_host /* [rows,D,S] dense, may be NULL */,
                       float* nrm_host /* [rows,S] dense, may be NULL */);

/* ---- question state from the caller: the step path behind another question encoder ------------------------------
 * The step path's own encoder is the reference's (LookupTable, two-layer LSTM, length select); its output q [n,Q] is
 * the only thing the hops read of it, and dq [n,Q] the only thing its backward reads of the hops.  These calls make
 * that boundary public for a caller whose encoder is something else (a language model, a GRU, an adapter over cached
 * text features).  No new GEMM or attention kernel is involved: the device work is one copy or widening pass, the
 * hot path is the existing hop chain, launch for launch.
 *   layout       Q = 4 * Rq.  q_dev is [n,Q] dense in DEVICE memory, n the current batch size (rau_set_batch_size).
 *                The library does not interpret the four quarters (in the built-in encoder they are [c1 h1 c2 h2]).
 *   type         q_type is RAU_FEAT_F32, RAU_FEAT_F16 or RAU_FEAT_BF16 (an encoder under autocast hands its output
 *                over as it is).  Widening is exact: the result is bit-identical to the f32 question that holds the
 *                widened values.  The fp8 types and unknown values: RAU_ERR_INVALID.
 *   attaching    rau_set_question_dev attaches q to the RESIDENT batch, as rau_set_answers and rau_set_regions attach
 *                theirs: one copy (f32) or widening pass (16-bit) on the ctx's stream into a ctx-owned [capacity,Q]
 *                f32 buffer.  No host wait, no synchronisation.  The caller orders its producer in front of
 *                rau_stream and keeps q_dev unchanged until the copy has run (rau_set_batch_dev's rule).  The tokens
 *                and lens the batch was uploaded with are ignored by a step while a question is attached.  The
 *                attached question survives any number of forwards.  Attaching again replaces the contents: the
 *                per-step call of a training loop.  A forward that ran before the call has no backward (run it again).
 *   detaching    q_dev == NULL detaches the question and returns the batch to the built-in encoder.  Every call that
 *                makes another batch current detaches it too: rau_set_batch* (every form, the asynchronous ones when
 *                they fill the current slot), rau_use_batch, and a rau_set_batch_size that changes the size (it drops
 *                the batch).  rau_batch_question reports whether the resident batch has one.
 *   forward      with a question attached rau_forward and every rau_graph_step* read q from that buffer; they launch
 *                nothing of the encoder (embed_fwd, enc_i2h_gemm, enc_h2h_gemm, its lstm_fwd cells or enc_ws) and no
 *                gather_q; the attention LSTM's lstm_fwd / lstm_bwd of every hop stay.
 *                Every other launch is the built-in path's, with its bits, in train and evaluate mode.
 *                rau_get_question_state returns the attached q.  Seeded dropout: under the same (seed, step) the keep
 *                bits of the q, x and mf sites are the built-in path's; the we and rnn sites are not consumed.
 *   backward     every step-level backward (rau_backward, _select, _att, _merged, _ext, the captured steps) runs the
 *                hop chain and dq_reduce as before and launches nothing of the encoder's backward: no BPTT
 *                (enc_h2h_dgrad, lstm_bwd), no enc_i2h_dgrad, no embed_bwd, no encoder weight-gradient GEMM.  The
 *                EMBED and RNN gradient buffers are not touched -- neither written nor zeroed; they keep what
 *                rau_zero_grads or earlier steps left.  The MULT group's gradients are the built-in path's bits.
 *                rau_wait_grads stays valid for all three groups, rau_allreduce_grads works unchanged.
 *   dq           dq[b,:] = sum_{h < HA} keep_q,h[b,:] * s_q * (dq~_h Wq)[b,:] in f32, hops added last first (the
 *                built-in path's dq_reduce, the buffer its BPTT would have read).  It is OVERWRITTEN by each backward,
 *                never accumulated; rau_zero_grads does not touch it.  With no active hop it is exact zeros.  No
 *                atomics: repeated calls give the same bits, a captured step the eager step's.
 *                rau_question_grad_dev hands out the ctx-owned DEVICE pointer [n,Q], ordered on the ctx's stream; it
 *                synchronises nothing; valid until the next forward or rau_set_batch_size.  rau_get_question_grad:
 *                the download, dense [n,Q]; synchronises.  Both are RAU_ERR_STATE when the last backward did not run
 *                on an attached question, or no backward has run since the last forward.
 *   captured     "a question is attached" joins rau_graph_step's key: a step captured without a question is never
 *                replayed for a batch with one, nor the reverse.  A replay reads the buffer's current contents, so
 *                attaching a new q each step needs no recapture.  rau_set_question_dev while a step is being
 *                captured: RAU_ERR_STATE.
 *   errors       nothing launched and nothing changed: a null ctx; no resident batch (RAU_ERR_STATE); a q_dev that is
 *                not 16-byte aligned (RAU_ERR_INVALID); an unknown or unsupported type (RAU_ERR_INVALID).
 *   unchanged    rau_backward_ext's rule stays: no EXTERNAL gradient enters at the question state.  The module-level
 *                calls are unchanged.  rau_update / rau_noise_clip_adam are unchanged: they still update EMBED and
 *                RNN (with noise on zero gradients) -- a caller who never uses the built-in encoder creates the
 *                context with small V / T and ignores those groups.  A context that never attaches a question
 *                computes and launches exactly what it did without these calls. */
int rau_set_question_dev(rau_ctx* ctx, const void* q_dev /* [n,Q] DEVICE, dense; NULL = detach */, int q_type);
int rau_batch_question(rau_ctx* ctx, int* has);
int rau_question_grad_dev(rau_ctx* ctx, const float** dq /* [n,Q] f32 DEVICE */);
int rau_get_question_grad(rau_ctx* ctx, float* host /* [n,Q] dense */);

/* ---- the hop recurrence's two ends: initial state in, state gradients in and out ---------------------------------
 * The answering unit is a recurrence: hop h reads the attention-LSTM state (c, h) of hop h-1.  The step path starts
 * it from zeros and hands the last hop's c' / h' zero gradients (the reference's).  These calls open both ends, as
 * every recurrent unit's interface does: (h0, c0) in, (hn, cn) out, gradients through both.  They add no parameter
 * and no layout; a context that never attaches a state or passes state gradients allocates, launches and computes
 * exactly what it did without them.
 *   attaching    rau_set_state_dev attaches (c0, h0), each [n,R] dense in DEVICE memory, 16-byte aligned, to the
 *                RESIDENT batch, by rau_set_question_dev's rules: type is RAU_FEAT_F32, RAU_FEAT_F16 or RAU_FEAT_BF16,
 *                widened exactly; one launch (state_attach) on the ctx's stream at the call, no host wait; the caller
 *                orders its producer in front of rau_stream and keeps the sources unchanged until the launch has run.
 *                The copy is taken at the call, so the sources may be the context's own rau_state_dev rows of the
 *                last hop: carrying the state into the next forward is one call.  The attached state survives any
 *                number of forwards; attaching again replaces it.  A forward that ran before the call has no backward.
 *   detaching    both pointers NULL detach: the next forward starts from zeros again (the launch's detaching form
 *                writes them; a call without an attached state launches nothing).  Every call that makes another batch
 *                current detaches too (rau_set_batch*, rau_use_batch, a rau_set_batch_size that changes the size);
 *                the next forward then writes the zeros itself, as it always has.  rau_batch_state reports the flag.
 *   forward      the hops read the state where they read the zeros; every launch is the detached path's, except that
 *                the two clears of the initial-state rows are not issued.  Train and evaluate mode, every batch form,
 *                region counts, tied dropout, bf16 mode and an attached question are unaffected.  An attached all-zero
 *                state gives the detached forward's output bits.
 *   rau_state_dev  ctx-owned DEVICE pointers to c' and h' of every hop of the last step-level forward, [H,n,R] f32
 *                dense in the current n (hop H-1's rows are the final state), ordered on the ctx's stream, no
 *                synchronisation; valid until the next forward, module-level call or rau_set_batch_size.
 *                RAU_ERR_STATE without a step-level forward to read.
 *   gradients in rau_backward_state is rau_backward_ext with sg: d_h [H,n,R] is dF/dh' of every hop, added to the
 *                recurrent gradient inside that hop's cell backward (the operand the module-level path's dh_next
 *                takes); d_c_last [n,R] is dF/dc' of the LAST hop, the recurrence's first dc_next.  Both f32 DEVICE,
 *                16-byte aligned, read on the ctx's stream during the call's launches.  With either non-NULL every hop
 *                is active (the host cannot see zero rows), hop_w may be NULL, and labels are needed only by a
 *                built-in term.  sg NULL or both members NULL IS rau_backward_ext with the other five arguments: the
 *                same launches, the same bits.  A gradient at c' of the hops BEFORE the last is not offered: it
 *                would be a new addend in the cell kernel.  There is no captured variant, as for rau_backward_ext.
 *   gradients out  with a state attached EVERY step-level backward (rau_backward, _select, _att, _merged, _ext,
 *                _state, every rau_graph_step*) also leaves d_c0 and d_h0 [n,R]: hop 0 forms its three products
 *                towards prev_h like every other hop, and one launch behind it (state_grad_finish) sums their
 *                split-K partials in ascending order into d_h0 and copies the cell's dc_prev into d_c0.  No atomics:
 *                repeated steps give the same bits, a captured step the eager step's.  Overwritten by each backward,
 *                never accumulated; rau_zero_grads does not touch them; exact zeros when no hop is active.
 *                rau_state_grad_dev hands out the ctx-owned DEVICE pointers (no synchronisation; valid until the next
 *                forward or rau_set_batch_size), rau_get_state_grad downloads them (synchronises; either may be NULL).
 *                Both are RAU_ERR_STATE without an attached state or before a backward of the current forward.
 *                Hop 0 then takes the branch of the other hops (with M == R the batched dg launch), so the
 *                parameter-gradient BITS of a step on an attached all-zero state need not equal a detached step's.
 *   captured     "a state is attached" joins rau_graph_step's key.  A captured step holds the initial-state rows'
 *                address, never their contents: a replay reads the state attached last.
 *   errors       nothing launched, the previous state stays in force: a null ctx; a step being captured or no
 *                resident batch (RAU_ERR_STATE); exactly one NULL pointer, a pointer that is not 16-byte aligned, an
 *                fp8 or unknown type (RAU_ERR_INVALID).
 *   unchanged    the module-level calls (they take the state from the caller already); the state is per sample,
 *                also on a batch with an image table. */
int rau_set_state_dev(rau_ctx* ctx, const void* c0_dev, const void* h0_dev /* [n,R] DEVICE; both NULL = detach */, int type);
int rau_batch_state(rau_ctx* ctx, int* has);
int rau_state_dev(rau_ctx* ctx, const float** c /* [H,n,R] f32 DEVICE */, const float** h /* [H,n,R] f32 DEVICE */);
typedef struct rau_state_grads {
  const float* d_h;       /* [H,n,R] DEVICE: dF/dh' of every hop;  NULL = none */
  const float* d_c_last;  /* [n,R]   DEVICE: dF/dc' of the LAST hop; NULL = none */
} rau_state_grads;
int rau_backward_state(rau_ctx* ctx, const float* hop_w /* [H] host, NULL = zeros */, const float* select_w,
                       const float* att_w, const float* merge_w, const rau_out_grads* g /* NULL = none */,
                       const rau_state_grads* sg /* NULL = none */);
int rau_state_grad_dev(rau_ctx* ctx, const float** d_c0 /* [n,R] f32 DEVICE */, const float** d_h0 /* [n,R] f32 DEVICE */);
int rau_get_state_grad(rau_ctx* ctx, float* d_c0_host /* [n,R] dense */, float* d_h0_host /* [n,R] dense */);

/* ---- attention bias from the caller: masks and priors in, its gradient out ---------------------------------------
 * Every hop adds the memory term zm[b,s] = (h_prev Wz^T)[b,s] + bz[s] to the content score before the softmax
 * (SS:287-289).  These calls add one more addend there, per SAMPLE and shared by all hops: an arbitrary mask (-inf),
 * a prior (log detector confidences, a saliency map, the previous round's attention), or the output of a small module
 * of the caller's that trains through the step -- for which every backward leaves the gradient at the bias.  No GEMM
 * and no backward kernel is involved: the forward attention kernels take one pointer, the gradient is a sum of rows
 * the backward keeps anyway.
 *   layout       bias_dev is [n,S] dense in DEVICE memory, n the current batch size (rau_set_batch_size), S the logical
 *                position count.  One bias per batch, read by every hop.  It is always per SAMPLE, also on a batch
 *                with an image table or bank rows (as the region counts are).
 *   type         RAU_FEAT_F32, RAU_FEAT_F16 or RAU_FEAT_BF16, widened exactly.  The fp8 types and unknown values:
 *                RAU_ERR_INVALID.
 *   values       finite values and -inf.  -inf means attention exactly 0 at that position, in every hop, in train and
 *                evaluate mode, and gradient exactly 0 there.  +inf and NaN are the caller's error.  A sample whose
 *                attended range (all S positions, or those below its region count) holds no finite bias is a softmax
 *                over nothing: the device form cannot check this, and that sample's attention row is then NaN (and so
 *                is everything computed from it).  Values at or behind a sample's region count are never read.
 *   arithmetic   score[b,s] = e[b,s] + bs + (zm[b,s] + bias[b,s]): one f32 add behind the finished memory term
 *                (its split-K partials and bz[s] summed as before).  Nothing else changes.  A bias of all +0 gives the
 *                bits of a step without one; a bias of -inf at s >= n[b] and 0 before gives rau_set_regions(n)'s.
 *   attaching    rau_set_att_bias_dev attaches the bias to the RESIDENT batch by rau_set_question_dev's rules: one
 *                launch (att_bias_attach) on the ctx's stream copies or widens it into a ctx-owned f32 buffer at the
 *                attention's row pitch.  No host wait, no synchronisation.  The caller orders its producer in front of
 *                rau_stream and keeps bias_dev unchanged until the launch has run.  The attached bias survives any
 *                number of forwards.  Attaching again replaces the contents: the per-step call of a training loop.  A
 *                forward that ran before the call has no backward (run it again).
 *   detaching    bias_dev == NULL detaches.  Every call that makes another batch current detaches too: rau_set_batch*
 *                (every form, the asynchronous ones when they fill the current slot), rau_use_batch, and a
 *                rau_set_batch_size that changes the size.  rau_batch_att_bias reports whether the resident batch has
 *                one.
 *   gradient     with a bias attached EVERY step-level backward (rau_backward, _select, _att, _merged, _ext, _state,
 *                every rau_graph_step*) also leaves d_bias[b,s] = sum over the backward's active hops, ascending, of
 *                dz_h[b,s], the softmax backward's result: one launch (att_bias_grad) behind the hop loop.  The per-row
 *                terms -- select_w, att_w, merge_w, external gradients, sample weights, 1/n -- are inside dz already.
 *                OVERWRITTEN by each backward, never accumulated; rau_zero_grads does not touch it; no atomics:
 *                repeated calls give the same bits, a captured step the eager step's.  With no active hop it is exact
 *                zeros.  rau_att_bias_grad_dev hands out the ctx-owned DEVICE pointer [n,pitch] and the row pitch in
 *                floats (pitch >= S; columns [S, pitch) hold +0), ordered on the ctx's stream; it synchronises nothing;
 *                valid until the next forward or rau_set_batch_size.  rau_get_att_bias_grad: the download, dense
 *                [n,S]; synchronises.  Both are RAU_ERR_STATE when the last backward did not run on an attached bias,
 *                or no backward has run since the last forward.
 *   captured     "a bias is attached" joins rau_graph_step's key: a step captured without a bias is never replayed
 *                for a batch with one, nor the reverse.  A replay reads the buffer's current contents, so attaching
 *                a new bias each step needs no recapture.  rau_set_att_bias_dev while a step is being captured:
 *                RAU_ERR_STATE.
 *   errors       nothing launched and nothing changed: a null ctx; no resident batch (RAU_ERR_STATE); a bias_dev that
 *                is not 16-byte aligned (RAU_ERR_INVALID); an fp8 or unknown type (RAU_ERR_INVALID).
 *   module level rau_multimodal_forward_bias (below) is the one-hop forward with counts and a bias in device memory.
 *                The gradient at the bias is not offered there.
 *   not offered  a bias per hop; a bias in the asynchronous upload slots or in the loader's feed; the gradient at
 *                module level; an external gradient AT the bias beyond what d_attprob of rau_backward_ext already
 *                offers.
 *   unchanged    a context that never attaches a bias allocates, launches and computes exactly what it did: no launch's
 *                grid, block or LDS request changes for anyone. */
int rau_set_att_bias_dev(rau_ctx* ctx, const void* bias_dev /* [n,S] DEVICE, dense; NULL = detach */, int type);
int rau_batch_att_bias(rau_ctx* ctx, int* has);
int rau_att_bias_grad_dev(rau_ctx* ctx, const float** d_bias /* [n,pitch] f32 DEVICE */, int32_t* pitch);
int rau_get_att_bias_grad(rau_ctx* ctx, float* host /* [n,S] dense */);

/* ---- module-level entry points: one call per nn.Module :forward / :backward -----
 * For hosts that keep feval's own loops (SS:443-596) and call the clones one by one.
 * t in [0,T) / h in [0,H) select the clone (the reference's embed_clones[t+1],
 * lstm_clones[t+1], multimodal_clones[h+1], criteria[h+1]; SS:340-347): it fixes the
 * clone's dropout-mask slice and the ctx-owned slot its activations are saved in.
 * All tensor arguments are DEVICE pointers (16-byte aligned, dense row-major), in the
 * reference's table orders; NULL for an optional input means "zeros" (or, for tokens /
 * X / labels, "the resident batch of rau_set_batch").  Outputs are returned as
 * pointers to ctx-owned slots indexed by (t|h): valid until the next :forward /
 * :backward of the same clone -- the lifetime rule of nn.Module's self.output /
 * self.gradInput.  :backward ACCUMULATES the clone's parameter gradients into the flat
 * gradient buffers (accGradParameters).  Work is enqueued on the ctx stream; nothing
 * synchronises except rau_criterion_forward when `loss` is non-NULL.
 * The step-level rau_forward/rau_backward above compute the same values faster
 * (they batch across clones); do not interleave the two within one step. */

/* word_embed = LookupTable -> Dropout(0.5) -> Tanh, SS:203-206; :forward SS:451,
 * :backward SS:593 (LookupTable has no gradInput).  tokens_dev [B] int32 1-based.
 * Ids in DEVICE tensors (tokens_dev here, labels_dev of rau_criterion_*) cannot be range-checked
 * by the call: the kernels clamp them into [1, V] / [1, K], so a bad id uses a wrong row where
 * the reference's LookupTable / ClassNLLCriterion would raise -- it never faults the GPU.  (The
 * host arrays of rau_set_batch ARE checked and rejected with RAU_ERR_INVALID.) */
int rau_embed_forward(rau_ctx* ctx, int t, const int32_t* tokens_dev, float** we /* [B,E] */);
int rau_embed_backward(rau_ctx* ctx, int t, const int32_t* tokens_dev, const float* d_we);

/* DeepLSTM.create(E, Rq, 2, 0.5), model/DeepLSTM.lua:14-71: {x [B,E], state [B,4Rq] =
 * [c1 h1 c2 h2]} -> state' [B,4Rq]; :forward SS:452, :backward SS:592 returning
 * {d_x [B,E], d_state [B,4Rq]}.  The length-select / dq row replacement of SS:455-461,
 * 584-591 stays in the host loop, as in the reference. */
int rau_deeplstm_forward(rau_ctx* ctx, int t, const float* x, const float* state,
                         float** state_out);
int rau_deeplstm_backward(rau_ctx* ctx, int t, const float* x, const float* state,
                          const float* d_state_out, float** d_x, float** d_state);

/* protos.multimodal, SS:292-307: {q [B,4Rq], X [B,D,S], c [B,R], h [B,R]} ->
 * {logits [B,K], do_pred [B], attprob [B,S], c' [B,R], h' [B,R]}; :forward SS:480,
 * :backward SS:571 with gradOutput {d_logits, d_do_pred, d_attprob, d_c, d_h}
 * (d_do_pred / d_attprob may be NULL = zeros, which is what feval passes, SS:566,573)
 * returning {d_q, d_X, d_c, d_h}.  d_X is the gradient feval discards (SS:579): pass
 * d_X = NULL to skip computing it. */
int rau_multimodal_forward(rau_ctx* ctx, int h, const float* q, const float* X,
                           const float* c_prev, const float* h_prev, float** logits,
                           float** do_pred, float** attprob, float** c_out, float** h_out);
/* rau_multimodal_forward with region counts (see rau_set_regions) in DEVICE memory: regions_dev [B] int32, NULL =
 * none (the resident batch's own counts are NOT applied here: the caller passes what the clone is to see).
 * Like ids in device tensors they cannot be range-checked by the call: the kernel clamps them into [1, S].
 * rau_multimodal_backward needs no sibling: it reads the attention this forward saved, which is exactly 0 at the
 * masked positions, and so is d_X there. */
int rau_multimodal_forward_regions(rau_ctx* ctx, int h, const float* q, const float* X,
                                   const float* c_prev, const float* h_prev, const int32_t* regions_dev,
                                   float** logits, float** do_pred, float** attprob, float** c_out,
                                   float** h_out);
/* The same with an additive attention bias (see rau_set_att_bias_dev) in DEVICE memory: bias_dev [B,S] f32 dense,
 * 16-byte aligned, NULL = none, which IS rau_multimodal_forward_regions launch for launch (the resident batch's own
 * bias is NOT applied here).  One launch re-pitches the rows into a ctx-owned buffer.  Values at or behind a sample's
 * count are never read; -inf gives attention exactly 0.  rau_multimodal_backward needs no sibling again: it reads the
 * saved attention.  The gradient at the bias is not offered at module level. */
int rau_multimodal_forward_bias(rau_ctx* ctx, int h, const float* q, const float* X,
                                const float* c_prev, const float* h_prev, const int32_t* regions_dev,
                                const float* bias_dev, float** logits, float** do_pred, float** attprob,
                                float** c_out, float** h_out);
int rau_multimodal_backward(rau_ctx* ctx, int h, const float* q, const float* X,
                            const float* c_prev, const float* h_prev, const float* d_logits,
                            const float* d_do_pred, const float* d_attprob,
                            const float* d_c, const float* d_h, float** d_q, float** d_X,
                            float** d_c_prev, float** d_h_prev);

/* nn.CrossEntropyCriterion (sizeAverage), SS:310: :forward SS:518 -> *loss (host,
 * may be NULL); :backward SS:565-569 -> d_logits [B,K] = scale*(softmax-onehot)/B,
 * scale = the dpred:mul(w) of SS:569.  labels_dev [B] int32 1-based. */
int rau_criterion_forward(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev,
                          float* loss);
int rau_criterion_backward(rau_ctx* ctx, int h, const float* logits,
                           const int32_t* labels_dev, float scale, float** d_logits);

/* The same criterion against an answer set in DEVICE memory (ids_dev / w_dev [B,G], see rau_set_answers; the
 * ids are clamped into [0, K] like labels_dev): the kernel the step's head uses with a set. */
int rau_criterion_forward_set(rau_ctx* ctx, int h, const float* logits, int32_t G, const int32_t* ids_dev,
                              const float* w_dev, float* loss);
int rau_criterion_backward_set(rau_ctx* ctx, int h, const float* logits, int32_t G, const int32_t* ids_dev,
                               const float* w_dev, float scale, float** d_logits);

/* The per-answer sigmoid criterion (RAU_LOSS_BCE at rau_set_answer_loss: target, loss row, gradient, roundings) on
 * logits the caller holds: the kernel the step's head uses under that kind, whatever kind the context is switched
 * to.  The target is labels_dev [B] int32 1-based, or with labels_dev NULL the answer set ids_dev / w_dev [B,G]
 * (1 <= G <= 16; neither: RAU_ERR_INVALID); G, ids_dev and w_dev are ignored with labels.  :forward -> *loss (host,
 * may be NULL) = the mean over B of the loss rows; :backward -> d_logits [B,K] = scale*(sigmoid - t)/B. */
int rau_criterion_forward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev /* NULL: use the set */,
                              int32_t G, const int32_t* ids_dev, const float* w_dev, float* loss);
int rau_criterion_backward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev,
                               int32_t G, const int32_t* ids_dev, const float* w_dev, float scale, float** d_logits);

/* The criterion restricted to candidates (rau_set_candidates: kept truth, loss row, gradient, roundings) on logits
 * the caller holds: the kernel the step's head uses on a batch with candidates.  cand_dev [B,C] int32 in DEVICE
 * memory (1 <= C <= RAU_MAX_CANDIDATES, ids clamped into [0, K]); the target is labels_dev [B] or with labels_dev NULL
 * the answer set ids_dev / w_dev [B,G] (neither: RAU_ERR_INVALID); kind = RAU_LOSS_CE or RAU_LOSS_BCE.  :forward ->
 * *loss (host, may be NULL) = the mean over B of the loss rows; :backward -> d_logits [B,K] = scale * the gradient. */
int rau_criterion_forward_cand(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev /* NULL: use the set */,
                               int32_t G, const int32_t* ids_dev, const float* w_dev, int32_t C, const int32_t* cand_dev,
                               int kind, float* loss);
int rau_criterion_backward_cand(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, int32_t G,
                                const int32_t* ids_dev, const float* w_dev, int32_t C, const int32_t* cand_dev, int kind,
                                float scale, float** d_logits);

/* The attention supervision above for hosts that call the clones one by one: attprob_dev [B,S] (the attprob output
 * of rau_multimodal_forward), t_dev [B,S] targets and nreg_dev [B] region counts (NULL = none, clamped into [1, S]),
 * all dense in DEVICE memory.  :forward -> *loss = ATT_h (host, may be NULL); :backward -> d_attprob [B,S]
 * (ctx-owned, valid until the next call) = -((scale * t) / (attprob + eps)) / B in that order, which goes straight
 * into rau_multimodal_backward's d_attprob.  Values in t_dev cannot be checked by the call: a negative or NaN
 * entry counts as 0. */
int rau_att_criterion_forward(rau_ctx* ctx, int h, const float* attprob_dev /* [B,S] */, const float* t_dev /* [B,S] */,
                              const int32_t* nreg_dev /* NULL */, float* loss);
int rau_att_criterion_backward(rau_ctx* ctx, int h, const float* attprob_dev, const float* t_dev,
                               const int32_t* nreg_dev, float scale, float** d_attprob /* ctx-owned [B,S] */);

/* ---- device tensors: the tensor algebra feval does BETWEEN module calls ----------------------
 * The reference's loops copy state rows where x_len[k] == t (`rnn_out[k] = lst[k]`, SS:455-461;
 * the dq row replacement, SS:584-591), accumulate (`uni_pred:add(pred[1])`, SS:522-526), take
 * `torch.max(pred[1], 2)` and `ans:eq(y):sum()` (SS:488-492) and zero-fill state tensors
 * (SS:357-413) -- on the reference's CUDA box through cutorch.  An MI355X host has no cutorch, so
 * those few operations are exported on plain device pointers (dense row-major float / int32),
 * enqueued on the ctx stream.  rau_dev_alloc'ed memory is zero-filled and owned by the ctx (freed
 * by rau_destroy, or earlier by rau_dev_free).  rau_dev_sum / _count_eq / _upload / _download
 * synchronise; the others do not. */
int rau_dev_alloc(rau_ctx* ctx, size_t n_floats, float** out);
int rau_dev_free(rau_ctx* ctx, float* p);
int rau_dev_fill(rau_ctx* ctx, float* dst, size_t n, float value);
int rau_dev_copy(rau_ctx* ctx, float* dst, const float* src, size_t n);
int rau_dev_axpy(rau_ctx* ctx, float* y, const float* x, size_t n, float alpha);   /* y += alpha x */
int rau_dev_scale(rau_ctx* ctx, float* x, size_t n, float alpha);
/* The tensor statements of the reference's optimizer call, `adam(x, dx, lr, beta1, beta2, epsilon,
 * state)` on each flat vector (SS:770-772, utils/optim_updates.lua:59-87): y += alpha x1 x2,
 * y += alpha x1 / x2, in-place sqrt, x += value -- and the whole function as one pass,
 * rau_dev_adam: m = beta1 m + (1-beta1) dx; v = beta2 v + (1-beta2) dx^2;
 * x -= lr sqrt(1-beta2^t)/(1-beta1^t) m / (sqrt(v) + eps), t = state.t after its increment (>= 1). */
int rau_dev_addcmul(rau_ctx* ctx, float* y, float alpha, const float* x1, const float* x2, size_t n);
int rau_dev_addcdiv(rau_ctx* ctx, float* y, float alpha, const float* x1, const float* x2, size_t n);
int rau_dev_sqrt(rau_ctx* ctx, float* x, size_t n);
int rau_dev_add_scalar(rau_ctx* ctx, float* x, size_t n, float value);
int rau_dev_adam(rau_ctx* ctx, float* x, const float* dx, float* m, float* v, size_t n, float lr,
                 float beta1, float beta2, float eps, int32_t t);
/* Its twin for Adamax (not in the reference; the rule of rau_update's RAU_OPT_ADAMAX, same element arithmetic):
 * m = beta1 m + (1-beta1) dx; u = max(beta2 u, |dx| + eps); x -= lr / (1-beta1^t) m / u.  Any n, any 4-byte-aligned
 * pointers (16-byte accesses when all four allow). */
int rau_dev_adamax(rau_ctx* ctx, float* x, const float* dx, float* m, float* u, size_t n, float lr,
                   float beta1, float beta2, float eps, int32_t t);
/* dst[k,:] = src[k,:] for the rows k with key_dev[k] == value (SS:455-461, 584-591) */
int rau_dev_select_rows(rau_ctx* ctx, float* dst, const float* src, int32_t rows, int32_t cols,
                        const int32_t* key_dev, int32_t value);
/* x[r, 0..cols) *= s_dev[r] for r < rows, rows of x at pitch ld >= cols (floats), each product rounded once; columns
 * cols..ld-1 are not touched.  For module-level hosts that weight a [B, K] criterion gradient per sample themselves.
 * 16-byte accesses where ld % 4 == 0 and x is 16-byte aligned; any cols.  Not synchronising. */
int rau_dev_scale_rows(rau_ctx* ctx, float* x, int32_t rows, int32_t cols, int32_t ld, const float* s_dev /* [rows] */);
/* The two kernels of rau_set_feat_norm (above) for hosts that drive the module-level calls and own their X: dense
 * float32 [n,D,S] tensors in device memory, D and S the context's, any n >= 0, on the ctx's stream, not synchronising.
 * rau_dev_l2norm: y = normalize(x) and, unless NULL, nrm [n,S].  rau_dev_l2norm_backward: dx = the gradient at x for
 * the gradient g at y, from the forward's y and nrm.  Where S % 4 == 0 every pointer must be 16-byte aligned. */
int rau_dev_l2norm(rau_ctx* ctx, const float* x_dev /* [n,D,S] dense f32 */, int32_t n, float eps,
                   float* y_dev /* may alias x_dev */, float* nrm_dev /* [n,S], may be NULL */);
int rau_dev_l2norm_backward(rau_ctx* ctx, const float* y_dev, const float* nrm_dev, float eps,
                            const float* g_dev, int32_t n, float* dx_dev /* may alias g_dev */);
/* torch.max(x, 2): per-row maximum and FIRST maximal index, 1-based (either output may be NULL) */
int rau_dev_rowmax(rau_ctx* ctx, const float* x, int32_t rows, int32_t cols, float* max_dev,
                   int32_t* argmax_dev);
/* torch.topk(x, k, 2, true, true): per row the k largest entries in descending order and their
 * 1-based indices (either output may be NULL).  x [rows, cols], val_dev [rows, k], idx_dev [rows, k];
 * rows >= 0 (0: nothing to do), cols > 0 (no alignment rule), 1 <= k <= cols, else RAU_ERR_INVALID with
 * nothing launched.  The order is TOTAL: larger value first; equal values (float equality, so +0 == -0)
 * by the LOWER index -- rau_dev_rowmax's first-max rule at every rank; +-inf order as values; NaN after
 * everything, -inf included, NaNs among themselves by the lower index.  So the k indices of a row are
 * distinct and in [1, cols] whatever the row holds, and rank 0 is rau_dev_rowmax on a row without NaN.
 * val_dev holds the selected entries bit for bit (NaN payloads, the sign of a zero).  Repeated calls
 * give the same bits.  Not synchronising. */
int rau_dev_topk(rau_ctx* ctx, const float* x, int32_t rows, int32_t cols, int32_t k,
                 float* val_dev, int32_t* idx_dev);
int rau_dev_sum(rau_ctx* ctx, const float* x, size_t n, double* out_host);
int rau_dev_count_eq(rau_ctx* ctx, const int32_t* a_dev, const int32_t* b_dev, int32_t n,
                     int32_t* count_host);
int rau_dev_upload(rau_ctx* ctx, void* dst_dev, const void* host, size_t bytes);
int rau_dev_download(rau_ctx* ctx, void* host, const void* src_dev, size_t bytes);

/* rau_zero_grads (optional) + rau_forward + rau_backward as ONE hipGraph launch: the three
 * streams, their fork/join events and all kernel arguments are captured once per step shape
 * (mode, longest question, number of active hops, explicit-mask sites) and replayed; the
 * batch, the Philox key and hop_w are read from device memory, so they may change freely
 * between launches.  Same results as the two calls, bit for bit. */
int rau_graph_step(rau_ctx* ctx, const float* hop_w /* [H] host */, int zero_grads_first);

/* ---- results (valid after rau_sync; these calls synchronise themselves) ------ */
int rau_sync(rau_ctx* ctx);
/* rau_get_losses: the per-hop means of the loss rows the last step-level forward on a batch with a ground truth
 * wrote (with sample weights: of the weighted rows).  It has NO state check: before such a forward, or after
 * something has invalidated that forward's record (rau_set_sample_weights or rau_set_answers on its slot, a
 * module-level entry point, rau_set_batch_size), it returns whatever the buffer holds -- the old means, or zeros.
 * rau_get_loss_rows is the checked form of the same data. */
int rau_get_losses(rau_ctx* ctx, float* losses /* [H] */);
/* The per-sample loss rows of the last step-level forward, dense [H,n]: the rows rau_get_losses averages (with
 * sample weights: the weighted rows).  Unlike rau_get_losses it is gated on that forward's record: RAU_ERR_STATE when
 * no step-level forward on a batch with a ground truth has run, or when its record has been invalidated since (the
 * cases listed above), where rau_get_losses would still hand back stale means. */
int rau_get_loss_rows(rau_ctx* ctx, float* rows /* [H,n] */);
int rau_get_argmax(rau_ctx* ctx, int32_t* ans /* [H,B] 1-based */);
int rau_get_logits(rau_ctx* ctx, float* logits /* [H,B,K] */);
int rau_get_dopred(rau_ctx* ctx, float* dopred /* [H,B] */);
int rau_get_attention(rau_ctx* ctx, float* att /* [H,B,S] */);
int rau_get_question_state(rau_ctx* ctx, float* q /* [B,Q] */);
int rau_get_att_state(rau_ctx* ctx, float* c /* [H,B,R] */, float* h /* [H,B,R] */);

/* ---- merged hops: feval's statistics and predict_result on the device ----------------------------
 * Computed from the resident outputs of the last rau_forward / rau_graph_step (hop_merge.hip): valid
 * from the end of that forward, through its rau_backward, until the next forward.  RAU_ERR_STATE,
 * with nothing launched, when no step-level forward has run, when a module-level entry point has run
 * since (it writes the same logits / do_pred / answer / loss slots), or when the batch slot whose
 * labels that forward read has been uploaded into again since (an upload into the OTHER slot of the
 * asynchronous path keeps them valid).
 *
 * feval's bookkeeping (SS:476-556), feval rule (last hop not forced).
 * loss [H+2]: per-hop CE (bitwise = rau_get_losses), uni CE, select CE;
 * loss_do_pred [H]: BCE of do_pred vs (argmax_h == y);
 * counts [RAU_STATS_NCOUNTS(H)]: correct[H+2] | do_pred_correct[H] (masked by did_correct) |
 *   did_correct | fired[H] (do_pred > 0.5) | selected[H] (samples whose select row is hop h).
 * Any output may be NULL.  RAU_ERR_STATE also when that forward's batch had no labels.  Synchronising. */
#define RAU_STATS_NCOUNTS(H) (4 * (H) + 3)
int rau_step_stats(rau_ctx* ctx, float* loss, float* loss_do_pred, int32_t* counts);

/* With an answer set (rau_set_answers) on that forward's batch, "argmax == y" becomes: the row's first-max
 * answer is among the row's non-empty ids with score > 0 (never on a row without entries).  rau_step_stats uses
 * that rule for correct[H+2], do_pred_gt (the BCE target) and did_correct, and the soft CE of rau_set_answers for
 * the uni and select rows; the per-hop CE stays bitwise rau_get_losses.
 * The metric score of an answer a of sample b is sum_g score[b,g] * [ids[b,g] == a], added from 0 in g order: exact
 * to restate in float32.  With score = min(#humans / 3, 1) it is the VQA accuracy the evaluation server reports.
 *   rau_step_scores     per_sample [H+2,n] (hops, uni, select; feval rule: last hop not forced), total [H+2] = their
 *                       sums over the batch.  Valid exactly when rau_step_stats is.
 *   rau_predict_scores  for the answers of the last rau_predict on the last forward (last hop forced): oe, mc
 *                       [H+2,n], totals [2,H+2] (oe row, mc row); mc and totals[1] are written only if that
 *                       rau_predict had an MC list.  RAU_ERR_STATE when no rau_predict has run on that forward.
 * Any output may be NULL.  Both return RAU_ERR_STATE, with nothing launched, when the forward's batch had no answer
 * set.  Totals are reduced by one workgroup in a fixed order (no float atomics): repeated calls give the same
 * bits.  Synchronising. */
int rau_step_scores(rau_ctx* ctx, float* per_sample /* [H+2,n] */, float* total /* [H+2] */);
int rau_predict_scores(rau_ctx* ctx, float* oe /* [H+2,n] */, float* mc /* [H+2,n] */,
                       float* totals /* [2,H+2] */);

/* predict_result + the eval loop's answer selection (SS:633-705, 877-900), last hop forced.
 * mc_ans: host [B, n_mc] candidate ids 1..K, 0 = empty slot (NULL: no MC; an id outside 0..K is
 * RAU_ERR_INVALID).  The MC answer is the first maximum of the RAW logits times the 0/1 candidate
 * mask, as in the reference: masked-out answers are +-0 and can beat negative candidates.
 * oe, mc: [H+2, B] 1-based answer ids (hops, uni, select); either may be NULL, and mc is written
 * only with an MC list.  Synchronising. */
int rau_predict(rau_ctx* ctx, const int32_t* mc_ans, int32_t n_mc, int32_t* oe, int32_t* mc);
/* merged rows of the last rau_predict: pred [2,B,K] (uni, select), att [2,B,S] (uni, select;
 * select WITHOUT the reference's never-zeroed carry, which the host adds) -- either may be NULL */
int rau_get_merged(rau_ctx* ctx, float* pred, float* att);
/* The k best answers of every row of predict_result (H hops, uni, select; last hop forced, as
 * rau_predict) of the last step-level forward, with their scores and softmax confidences.
 * ids, score, conf: host [H+2, B, k]; any may be NULL.  Synchronising.
 * ids: 1-based, in rau_dev_topk's total order, so ids[r, b, 0] is rau_predict's oe[r, b] on every
 * finite row; score: the row's raw or merged logit at that id, bit for bit; conf: its softmax
 * probability, expf(score - max) / sum expf(v - max) summed in the criterion's order (defined for
 * finite rows; a non-finite row still gives distinct ids in [1, K]; under RAU_LOSS_BCE conf is still this softmax
 * probability -- the per-answer confidence of that criterion is the sigmoid of score).  1 <= k <= K, else
 * RAU_ERR_INVALID.  Valid when rau_predict is (RAU_ERR_STATE otherwise, nothing launched), in either
 * mode; needs no labels; neither needs nor disturbs rau_predict, rau_get_merged or rau_step_stats.
 * Its device staging is allocated at the first call and regrown for a larger k (RAU_ERR_NOMEM leaves
 * the context usable).  Open-ended answers only: the reference's multiple-choice rule multiplies the
 * raw logits by a 0/1 mask, so a ranked MC list would rank the masked-out zeros among the candidates;
 * rau_predict stays the MC call of that rule, rau_topk_cand below ranks a batch's candidates among themselves. */
int rau_topk(rau_ctx* ctx, int32_t k, int32_t* ids, float* score, float* conf);

/* Multiple-choice statistics and ranked MC answers of the last step-level forward on a batch WITH candidates
 * (rau_set_candidates; cand_rank.hip).  The rows are the merged rows above (H hops, uni, select); a row's live
 * candidates are ranked among themselves in rau_dev_topk's total order: larger logit first, ties by the lower answer
 * id, NaN last.  Both return RAU_ERR_STATE, nothing launched, without such a forward or when its batch had no
 * candidates.  Any output may be NULL.  Synchronising; no float atomics, the same bits on every call.
 *   rau_topk_cand   predict rule (last hop forced, as rau_topk; valid when rau_predict is, needs no labels).  ids,
 *                   score, conf [H+2, n, k]: the k best candidates, their logits (bit for bit the row's value) and
 *                   conf = expf(v - m) / den over the live candidates (m, den as at rau_set_candidates).  Ranks at
 *                   and behind the number of live candidates: id 0, score -INFINITY, conf +0.  1 <= k <= C, else
 *                   RAU_ERR_INVALID.
 *                   Rank 0 is the first maximum of the candidates' logits: the masking rule a softmax over the
 *                   candidates implies.  It equals rau_predict's mc whenever the best candidate's logit is positive;
 *                   it differs BY DESIGN where the reference's multiply rule lets a masked-out zero win (a row whose
 *                   candidates are all negative).  rau_predict stays as it is.
 *   rau_cand_stats  feval rule (last hop not forced, as rau_step_stats); also RAU_ERR_STATE without a ground truth.
 *                   Per row of H+2: loss = the restricted criterion of rau_set_candidates (mean over n, sample weights
 *                   applied; under RAU_LOSS_BCE the restricted sigmoid criterion), loss[0..H) bitwise rau_get_losses;
 *                   correct = the labelled rows whose rank-0 candidate is the label, or carries a positive score in
 *                   the answer set; score = the summed metric score of that candidate (labels: 1 when correct),
 *                   reduced in rau_step_scores' fixed order.  n_lab = the labelled rows: those with a kept truth
 *                   entry.  Counts and scores are unweighted. */
int rau_cand_stats(rau_ctx* ctx, float* loss /* [H+2] */, int32_t* correct /* [H+2] */, float* score /* [H+2] */, int32_t* n_lab);
int rau_topk_cand(rau_ctx* ctx, int32_t k, int32_t* ids, float* score, float* conf /* [H+2, n, k] host */);

/* ---- update: SS:597-630 + utils/optim_updates.lua:59-87 (row "next-1") -------
 * Gradient noise N(0, eta/((step_t+1)*gamma)), per-group L2 clip, Adam with
 * epsilon outside the sqrt; lr applies to EMBED and RNN, mult_lr to MULT
 * (SS:770-772).  noise_seed keys the on-device normal generator; eta = 0
 * disables noise.  out_norms[3] (host, may be NULL) receives pre-clip norms. */
int rau_noise_clip_adam(rau_ctx* ctx, int64_t step_t, float lr, float mult_lr,
                        float beta1, float beta2, float eps, float eta,
                        float gamma, float clip, uint64_t noise_seed,
                        float* out_norms);

/* ---- update with a rule and a clip scope; optimizer state in and out --------------------------
 * rau_update is the same step with two choices.  RAU_OPT_ADAM with RAU_CLIP_GROUP is what the reference does
 * (SS:597-630: noise, one L2 clip per parameter group, then adam on each flat vector, SS:770-772) and gives
 * the bits of rau_noise_clip_adam on the same state and arguments: weights, gradients, moments, out_norms[0..2].
 * RAU_OPT_ADAMAX and RAU_CLIP_GLOBAL are NOT in the reference; they are the update of the bottom-up / top-down
 * recipe: Adamax, and one gradient norm clipped over the whole model.
 *   noise    the generator, counters and key (noise_seed + 3 step_t + group) of rau_noise_clip_adam in every rule
 *            and scope; eta = 0 disables it.
 *   norms    out_norms[4] (host, may be NULL): [0..2] the groups' pre-clip norms, [3] the global norm
 *            sqrtf((s_embed + s_rnn) + s_mult) of the three f32 sums of squares, written in both scopes.
 *   clip     scale = norm > clip ? clip / norm : 1 with the group's norm (GROUP) or the global norm for all three
 *            groups (GLOBAL); the clipped gradient is written back.
 *   ADAMAX   m = beta1 m + (1-beta1) g;  u = max(beta2 u, |g| + eps);  x -= (group_lr / (1 - beta1^t)) m / u, with u
 *            kept where Adam keeps v, starting at 0 (torch.optim.Adamax's statement); the step size is formed on
 *            the host in double, as Adam's is.
 * A group's optimizer state (m, v, t) belongs to the rule that last wrote it: an update with the other rule while
 * that group's t > 0 is RAU_ERR_STATE -- rau_noise_clip_adam on Adamax state included; reset the state first
 * (rau_set_opt_state).  An unknown rule or scope, clip <= 0, gamma <= 0, eta < 0, step_t < 0: RAU_ERR_INVALID.
 * In every error case nothing is launched and nothing changes.  At most two launches (update.hip), under the
 * names upd_noise_sqnorm and upd_apply in rau_prof_entry.  Synchronising only with out_norms. */
#define RAU_OPT_ADAM 0     /* the arithmetic of rau_noise_clip_adam */
#define RAU_OPT_ADAMAX 1
#define RAU_CLIP_GROUP 0   /* one norm per parameter group (the reference, SS:597-630) */
#define RAU_CLIP_GLOBAL 1  /* one norm over the three groups together */
typedef struct rau_update_opts {
  int32_t rule, clip_scope;
  float lr, mult_lr, beta1, beta2, eps, eta, gamma, clip;
  uint64_t noise_seed;
} rau_update_opts;
/* RAU_OPT_ADAM, RAU_CLIP_GROUP, lr 3e-3, mult_lr 3e-4, betas 0.9 / 0.999, eps 1e-8, eta 0.01, gamma 0.55,
 * clip 0.1, noise_seed 0 */
void rau_update_opts_default(rau_update_opts* o);
int rau_update(rau_ctx* ctx, int64_t step_t, const rau_update_opts* o, float* out_norms);
/* The optimizer state of one group, host side: m, v [n of rau_params] (v holds Adamax's u), t = updates so far,
 * rule = the rule that owns the state.  Before the first update the moments read as zeros, t = 0, rule =
 * RAU_OPT_ADAM; any output may be NULL, and a reader allocates nothing.  rau_set_opt_state allocates the moments if
 * need be; m = v = NULL with t = 0 resets the group (zero moments, t = 0) to `rule`: the way to change rule.
 * RAU_ERR_INVALID, nothing changed: t < 0, t > 0 without both vectors, an unknown rule.  Both synchronise, as
 * rau_get_params does.  The state survives rau_set_batch_size. */
int rau_get_opt_state(rau_ctx* ctx, int group, float* m, float* v, int64_t* t, int32_t* rule);
int rau_set_opt_state(rau_ctx* ctx, int group, const float* m, const float* v, int64_t t, int32_t rule);

/* ---- update with decoupled weight decay, per-layer step sizes and a weight average ---------------
 * rau_update_ex is rau_update with three more choices (none is in the reference).  rau_update_opts is unchanged and
 * means what it means to rau_update: the noise generator, keys and counters, the norms, the clip, the rule-ownership
 * rule of the optimizer state and the validation of `o` are rau_update's.  With `e` at its defaults (NULL counts as
 * defaults) and every layer at its defaults, rau_update_ex gives rau_update's bits in weights, gradients, moments and
 * all four norms, in both rules and scopes, with and without noise.  Two launches (update.hip), under the names
 * upd_ex_sqnorm and upd_ex_apply in rau_prof_entry; no atomics, no cooperative launch.  Synchronising only with
 * out_norms.
 *
 * Layers and segments.  A LAYER is one named unit of a parameter group: unit i of RNN and MULT is rau_layout_entry's
 * entries 2i ("<name>.weight", [out,in]) and 2i + 1 ("<name>.bias", [out]); EMBED has the one unit 0,
 * word_embed.weight, with no bias.  That is 1 + 4 + 13 units.  `index` below is the unit's index i.  A SEGMENT is the
 * weight part or the bias part of one unit: at most 1, 8 and 26 per group.  Segment ends are not multiples of 4 and a
 * bias can be one element; every coefficient below is per ELEMENT, by the segment the element lies in.
 *   rau_set_layer_opts  lr_scale (default 1), decay_weight (default 1), decay_bias (default 0) of one unit; kept in
 *                       the context until set again, through rau_set_batch_size as well.  lr_scale or a decay
 *                       multiplier negative or non-finite, a bad group or index: RAU_ERR_INVALID, nothing changed.
 *                       rau_update and rau_noise_clip_adam do not look at layer options.
 *   step size           a segment's step size is its group's with lr_scale multiplied in, formed on the host in
 *                       double like rau_update's: (float)(group_lr * lr_scale * sqrt(1 - beta2^t) / (1 - beta1^t)) for
 *                       RAU_OPT_ADAM, (float)(group_lr * lr_scale / (1 - beta1^t)) for RAU_OPT_ADAMAX.
 *   frozen              lr_scale == 0 freezes the unit: the x, m, v, average AND gradient of its elements keep their
 *                       bits (no noise, no clip write-back), and its elements add nothing to any norm in out_norms,
 *                       group or global -- a frozen layer is not part of the model being clipped, as in torch where
 *                       it has no .grad.  Its noise counters are simply not drawn; every other element's noise is what
 *                       it would be with nothing frozen.  The backward still forms its gradient.
 *   weight_decay        decoupled, torch.optim.AdamW's order: first x = x f (one rounded product) with
 *                       f = (float)(1 - group_lr * lr_scale * weight_decay * decay_weight) for a weight segment and
 *                       decay_bias in decay_weight's place for a bias segment, formed on the host in double; then the
 *                       rule runs on the decayed x.  A segment whose f is exactly 1 skips the multiplication.  It is
 *                       this decoupled form under RAU_OPT_ADAMAX too, NOT torch.optim.Adamax's L2 term (which adds
 *                       weight_decay x to the gradient).  The decay enters neither the gradient, nor the moments, nor
 *                       the norms.  weight_decay < 0 or non-finite: RAU_ERR_INVALID.
 *   ema_decay = d       in [0, 1), else RAU_ERR_INVALID.  d > 0: after the rule, on the new x, e = (d e) + ((1-d) x)
 *                       with both products and the sum rounded and 1-d formed once on the host in float; frozen
 *                       segments are skipped.  d == 0: the average is neither read nor written.  d > 0 without an
 *                       average (rau_ema_reset / rau_set_ema): RAU_ERR_STATE.
 * The average.  One more vector per group, of the group's length; it survives rau_set_batch_size like the optimizer
 * state.
 *   rau_ema_reset       average := current weights, all three groups (allocated at the first use; RAU_ERR_NOMEM).
 *   rau_set_ema / rau_get_ema   one group's average from / to the host, n = the group's length (else
 *                       RAU_ERR_INVALID); both synchronise, as rau_set_params does.  rau_set_ema allocates like
 *                       rau_ema_reset: when there was no average, all three start as the current weights and this
 *                       group's is then replaced.  rau_get_ema without an average: RAU_ERR_STATE.
 *   rau_ema_swap        exchanges weights and average in place: one launch over the three groups, no allocation;
 *                       RAU_ERR_STATE without an average.  It toggles `swapped`.  While swapped, rau_get_params, the
 *                       forward, the statistics and snapshots see the averaged weights, and rau_get_ema the trained
 *                       ones; rau_noise_clip_adam, rau_update and rau_update_ex return RAU_ERR_STATE with nothing
 *                       launched, and so do rau_ema_reset and rau_set_ema.  Two swaps restore every bit.
 *   rau_ema_state       has = 0 | 1 (an average exists), swapped = 0 | 1; either output may be NULL.
 * In every error case nothing is launched and nothing changes. */
typedef struct rau_update_extras {
  float weight_decay;
  float ema_decay;
} rau_update_extras;
/* 0, 0 */
void rau_update_extras_default(rau_update_extras* e);
int rau_update_ex(rau_ctx* ctx, int64_t step_t, const rau_update_opts* o, const rau_update_extras* e,
                  float* out_norms);
int rau_set_layer_opts(rau_ctx* ctx, int group, int index, float lr_scale, float decay_weight, float decay_bias);
int rau_get_layer_opts(rau_ctx* ctx, int group, int index, float* lr_scale, float* decay_weight, float* decay_bias);
int rau_ema_reset(rau_ctx* ctx);
int rau_ema_swap(rau_ctx* ctx);
int rau_ema_state(rau_ctx* ctx, int* has, int* swapped);
int rau_get_ema(rau_ctx* ctx, int group, float* host, size_t n);
int rau_set_ema(rau_ctx* ctx, int group, const float* host, size_t n);

/* ---- per-layer statistics of the flat vectors, and a non-finite guard in front of the update ------
 * rau_layer_stats reads the flat buffers on the device and returns one record per layout entry, in rau_layout_entry's
 * order group by group: EMBED, then RNN, then MULT (rau_layer_stats_count records: 35 today).  `what` is a sum of
 *   RAU_STAT_GRAD   the gradient buffers as they stand
 *   RAU_STAT_PARAM  the weight buffers as they stand (while rau_ema_swap is in force: the average)
 *   RAU_STAT_DIR    the rule's direction from the moments as they stand: m / (sqrtf(v) + eps) for a group whose state
 *                   RAU_OPT_ADAM owns, m / u for RAU_OPT_ADAMAX, with update.hip's divisions and sqrtf and the
 *                   caller's eps.  ||dx|| of a unit is its step size, formed on the host as rau_update_ex forms it,
 *                   times sqrtf(sumsq[2]).  A group with t == 0 has no moments: RAU_ERR_STATE.
 * and the fields [0], [1], [2] of a record belong to them in that order; a source that is not requested leaves its
 * three fields at 0, and eps is not read without RAU_STAT_DIR.  Frozen layers are reported like any other: this is a
 * readout, not part of the update.
 * The readout is finite-only: sumsq and absmax are taken over the finite elements and nonfinite counts the NaN and
 * +-Inf ones, so three NaNs in a large embedding do not hide the norm of the rest.  sumsq is an f32 sum and may itself
 * overflow to +Inf for finite elements above about 1e19, as torch.norm does in f32; absmax stays exact.  The sum has a
 * fixed order (layer_stats.hip states it and the length L(n) of its longest chain of additions): no atomics, the same
 * bits on every call, and a source's bits do not depend on which other sources were requested.  Against an exact sum
 * the relative error of sumsq is at most (L(n) + 2) * 2^-24.
 * Two launches on the context's stream, layer_stats_part and layer_stats_finish in rau_prof_entry; the work table is
 * built at the first call and freed by rau_destroy.  rau_layer_stats synchronises; rau_layer_stats_dev does not and
 * hands out the device array [count], ordered on the context's stream and valid until the next call of either.
 * what == 0 or with unknown bits, eps negative or non-finite (also where it is not read): RAU_ERR_INVALID.  In every error
 * case nothing is launched.
 *
 * The guard.  With RAU_GUARD_SKIP, rau_noise_clip_adam, rau_update and rau_update_ex first count the non-finite
 * elements of the three gradient buffers (the gradients only; rau_update_ex leaves frozen layers out, which are not
 * part of the model being updated): after argument validation and before anything else is launched, with the
 * count-only form of the same two launches.  The three per-group totals are downloaded, 24 bytes, WHICH SYNCHRONISES
 * THE STREAM in every guarded update.  All zero: the call proceeds exactly as without the guard, the same launches and
 * the same bits.  Otherwise nothing of the update is launched: weights, gradients, moments, the average, t and the
 * owning rule of all three groups keep their bits, out_norms (when given) receives NaN in every entry the call would
 * have written, the call returns RAU_OK, `skipped` grows by one, last_skipped = 1 and last_nonfinite holds the
 * totals.  An update that ran sets last_skipped = 0.  The next clean or unguarded update is bit for bit what it would
 * have been had the skipped call never been made.
 * Callers that accumulate gradients over several backward calls: a NaN stays in the buffer until rau_zero_grads, and
 * every guarded update is skipped until then.  With a communicator the verdict is taken on the reduced gradients, so
 * every rank decides alike (a NaN survives the average).  The mode survives rau_set_batch_size; `skipped` is neither
 * part of the optimizer state nor of snapshots.  An unknown mode: RAU_ERR_INVALID.  The guard is not offered inside
 * rau_graph_step*, which do not update. */
#define RAU_STAT_GRAD 1
#define RAU_STAT_PARAM 2
#define RAU_STAT_DIR 4
typedef struct rau_layer_stat {
  float sumsq[3];        /* [grad, param, dir]: sum of squares of the FINITE elements */
  float absmax[3];       /* largest |.| of the finite elements; +0 when there is none */
  int64_t nonfinite[3];  /* NaN and +-Inf elements */
  int64_t n;             /* elements of the entry */
} rau_layer_stat;
int rau_layer_stats_count(const rau_ctx* ctx);
int rau_layer_stats(rau_ctx* ctx, int what, float eps, rau_layer_stat* out /* host [count] */);
int rau_layer_stats_dev(rau_ctx* ctx, int what, float eps, const rau_layer_stat** dev /* device [count] */);
#define RAU_GUARD_OFF 0    /* default */
#define RAU_GUARD_SKIP 1
int rau_set_update_guard(rau_ctx* ctx, int mode);
int rau_update_guard(rau_ctx* ctx, int* mode, int64_t* skipped, int32_t* last_skipped,
                     int64_t last_nonfinite[3] /* per group; any output may be NULL */);

/* ---- data-parallel exchange (new: the reference is single-GPU) --------------------
 * One process and one rau_ctx per GPU.  Rank 0 obtains a communicator id and hands it to
 * the other ranks by any host channel (file, socket, MPI, torch.distributed); every rank
 * then calls rau_comm_init.  rau_allreduce_grads averages the three flat gradient buffers
 * in place over RCCL/xGMI after rau_backward -- the mult bucket underneath the encoder
 * BPTT, everything ordered by stream events -- after which every rank applies the
 * identical rau_noise_clip_adam (same noise_seed).  RCCL is bound at first use. */
#define RAU_COMM_ID_BYTES 128
int rau_comm_unique_id(void* id, size_t bytes /* >= RAU_COMM_ID_BYTES */);
int rau_comm_init(rau_ctx* ctx, int nranks, int rank, const void* id, size_t bytes);
int rau_allreduce_grads(rau_ctx* ctx);
int rau_comm_destroy(rau_ctx* ctx);

/* ---- timing / interop ---------------------------------------------------------
 * The ctx's hipStream_t (as void*) so a host can order its own work (e.g. an
 * RCCL all-reduce of the flat grad buffers issued through torch.distributed)
 * after the ctx's kernels without a device-wide sync. */
int rau_stream(rau_ctx* ctx, void** hip_stream);
/* Makes `hip_stream` (a hipStream_t of the same device) wait until the gradients of
 * `group` from the last rau_backward are final, without blocking the host or the ctx
 * stream.  RAU_GROUP_MULT is final BEFORE the encoder BPTT has run, so a host can put
 * that bucket's all-reduce on a side stream underneath the rest of the backward pass
 * (rau_vqa_amd/dist.py); the other two groups are final at the end of rau_backward. */
int rau_wait_grads(rau_ctx* ctx, int group, void* hip_stream);
/* HIP-event bracket on the ctx stream: kernel time of everything enqueued
 * between begin and end, in milliseconds (end synchronises). */
int rau_timer_begin(rau_ctx* ctx);
int rau_timer_end(rau_ctx* ctx, float* ms);
/* Average duration (ms) and launch count of the named kernel class since the
 * last rau_prof_reset, measured with HIP events on the ctx stream when
 * profiling is enabled (adds two events per launch; off by default).
 * on = 2: sparse -- only the launches of the bulk and weight-gradient streams and the
 * recurrence's phase markers are bracketed, so the recurrence keeps its un-profiled pace. */
int rau_prof_enable(rau_ctx* ctx, int on);
int rau_prof_reset(rau_ctx* ctx);
int rau_prof_count(rau_ctx* ctx);
int rau_prof_entry(rau_ctx* ctx, int index, const char** name, int64_t* launches,
                   double* total_ms, double* flops, double* bytes);

/* ---- diagnostics: host-side predicates of the library, callable without a device --------------
 * (what tests/test_host_logic.py pins on the CPU; nothing here touches the GPU or a ctx)
 *
 * rau_split_guard_check: the range check every consumer of split-K partial sums applies before it
 * launches (lin_reduce_epilogue, the LSTM cell kernels, the attention kernels, the criterion head,
 * splitk_reduce_acc): would a consumer reading `nsplit` partials of `per_split_floats` floats at
 * `offset` floats into a workspace of `ws_floats` floats be launched?  RAU_OK, or RAU_ERR_STATE --
 * the code rau_forward / rau_backward return instead of launching when a split count or slab
 * offset is stale.
 * rau_enc_ws_coresident: 1 if the weight-stationary persistent encoder (whose workgroups wait on each
 * other's progress counters) may be selected for `batch` samples on a device that admits
 * `blocks_per_cu` of its workgroups per CU on `n_cus` CUs, else 0.
 * rau_image_lists: the sample lists of an image table as the batch code builds them for the per-image feature-map
 * gradient (a stable counting sort over image_of): image i owns samples[start[i] .. start[i + 1]), ascending;
 * start[n_images] = n.  RAU_ERR_INVALID for n < 1, n_images outside [1, n] or an index outside [0, n_images). */
int rau_split_guard_check(size_t ws_floats, size_t offset, int nsplit, size_t per_split_floats);
int rau_enc_ws_coresident(int batch, int blocks_per_cu, int n_cus);
int rau_image_lists(int n, int n_images, const int32_t* image_of, int32_t* start /* [n_images+1] */,
                    int32_t* samples /* [n] */);

#ifdef __cplusplus
}
#endif
#endif /* RAU_H */

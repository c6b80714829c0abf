// rau_ctx.h -- the rau_ctx object shared by the translation units that implement
// include/rau.h (internal to librau.so; not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/rau.h"
#include "kernels.h"
#include "policy.h"

using namespace rau;

constexpr int kEncHeadTokens = 4;   // tokens whose layer-1 input projection stays on the chain stream
constexpr int kEncSideChunks = 4;   // the other tokens' projection: that many launches on the third stream, each with
                                    // its own event -- the recurrence waits for the chunk it is about to read, not
                                    // for all of them (one launch of 22 x 256 rows took 0.3-0.45 ms beside the bulk
                                    // tiles and held the encoder at token 5)

// ------------------------------------------------------------------ errors
// sets the calling thread's rau_last_error() message and returns `code`
__attribute__((visibility("hidden"))) int fail(int code, const char* fmt, ...);
#define HIPC(expr)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(RAU_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                  __FILE__, __LINE__);                                                    \
  } while (0)
#define NEED(cond, ...)                               \
  do {                                                \
    if (!(cond)) return fail(RAU_ERR_INVALID, __VA_ARGS__); \
  } while (0)

// ------------------------------------------------------------------ ctx
struct Lin {  // one Linear (or 1x1 conv) inside a flat group
  float *W, *b, *dW, *db;
  int out, in;
};
struct Entry {
  std::string name;
  size_t off;
  int rows, cols;
};
struct LayerOpt {   // rau_set_layer_opts
  float lr_scale = 1.f, decay_w = 1.f, decay_b = 0.f;
};
struct Group {
  float* w = nullptr;
  float* g = nullptr;
  float* m = nullptr;  // optimizer moments (allocated on first update or rau_set_opt_state); v holds Adamax's u
  float* v = nullptr;
  size_t n = 0;
  int64_t adam_t = 0;  // updates so far, of either rule
  int opt_rule = RAU_OPT_ADAM;   // the rule that owns m, v, adam_t: the other one is refused while adam_t > 0
  std::vector<Entry> layout;
  float* ema = nullptr;          // the weight average (rau_ema_reset / rau_set_ema allocate all three groups')
  std::vector<LayerOpt> lopt;    // per unit (weight + bias of one named layer); empty = every unit at its defaults
};
struct ProfRec {
  int cls;
  hipEvent_t a, b;
  int sid;   // 0 chain, 1 bulk, 2 weight-gradient stream
};
struct ProfCls {
  std::string name;
  int64_t launches = 0;
  double ms = 0, flops = 0, bytes = 0;
};

// What a batch slot holds.  A plain value: "no batch" is BatchDesc{}.
struct BatchDesc {
  int feat_type = RAU_FEAT_F32;     // rau_feat_type of the maps in `feats` (a cleared buffer counts as f32)
  // image table (rau_set_batch_images): `feats` holds n_images maps, sample b looks at map image_of_d[b];
  // 0 = a plain batch
  int n_images = 0;
  // bank batch (rau_set_batch_bank): a table batch whose maps are rows of the ctx's feature bank
  bool bank = false;
  bool table_ok = false;            // `feats` holds the gathered table (else only the index does: train-mode upload)
  std::vector<int32_t> lens;
  int max_len = 0, nuniq = 0;
  bool have = false, have_labels = false;
  // answer set (rau_set_answers): G entries per sample in the slot's ans_* buffers, 0 = none.  It replaces the
  // labels for the criterion head and the statistics; a batch with a set counts as labelled.
  int ans_G = 0;
  // region counts (rau_set_regions): sample b attends to the first nreg_d[b] positions only.  Like the answer set
  // they belong to the batch: hold() drops them.
  bool regions = false;
  // attention targets (rau_set_att_targets): the slot's att_t_d holds a target map per sample.  They belong to the
  // batch like the two above.
  bool att_targets = false;
  // per-sample loss weights (rau_set_sample_weights): the slot's sw_d holds one weight per sample, read by every
  // kernel that forms a training term (step_truth()).  They belong to the batch like the three above.
  bool sample_w = false;
  // multiple-choice candidates (rau_set_candidates): C entries per sample in the slot's cand_d, 0 = none.  The
  // criterion head and the MC statistics read them (step_truth()).  They belong to the batch like the four above.
  int cand_C = 0;
  // question state from the caller (rau_set_question_dev): the slot's q_ext holds q [n][Q] and the step reads it in
  // place of the built-in encoder's output.  It belongs to the RESIDENT batch: hold() and rau_use_batch drop it.
  bool question = false;
  // initial state of the hop chain from the caller (rau_set_state_dev): slot 0 of cc / hh holds (c0, h0) [n][R] and the
  // forward leaves it there in place of writing the zeros.  It belongs to the RESIDENT batch like the question.
  bool state = false;
  // additive attention bias from the caller (rau_set_att_bias_dev): the slot's zb_ext holds a row [Sp] per sample and
  // every hop's attention kernel adds it to the score.  It belongs to the RESIDENT batch like the two above.
  bool att_bias = false;
};
// One of the two batch slots.  slot[cur_slot] is the resident batch (cur_batch() below): the only record of it.
// Slot 0's device buffers exist from rau_create on; slot 1's, the pinned staging the loader may fill in place, the
// events and the copy stream come with the first call of the asynchronous path (rau_batch_slot /
// rau_set_batch_async / rau_use_batch).
struct BatchSlot {
  // ---- allocated once
  float* feats = nullptr;                                   // device, [B][D][Sp] (16-bit batch: its first half)
  int32_t *tokens = nullptr, *lens_d = nullptr, *labels_d = nullptr;
  int32_t *utok = nullptr, *ustart = nullptr, *upos = nullptr;
  // device, one block allocated at the slot's first table batch: image_of [cap] | img_start [cap + 1] |
  // img_samples [cap].  The last two are the table's sample lists (rau_image_lists): image slot i owns
  // img_samples[img_start[i] .. img_start[i + 1]), ascending; slots at and behind n_images are empty.  The per-image
  // feature-map gradient reads them (xgrad.hip); a captured step holds their addresses, never their contents.
  int32_t* image_of_d = nullptr;
  int32_t *img_start_d = nullptr, *img_samples_d = nullptr;
  // bank_idx_d holds rows[n_images] (padded to B) and then rows[image_of[b]] for every sample, so both gathers
  // of a bank batch are one indexed copy
  int32_t* bank_idx_d = nullptr;    // device [2B], allocated at the slot's first bank batch
  float* feats_h = nullptr;                                 // pinned host, dense [B][D][S] (16-bit: first half)
  int32_t *tokens_h = nullptr, *lens_p = nullptr, *labels_h = nullptr;
  int32_t *utok_h = nullptr, *ustart_h = nullptr, *upos_h = nullptr;
  int32_t* image_of_h = nullptr;    // pinned host, the device block's layout (3 * cap + 1 words)
  int32_t* bank_idx_h = nullptr;    // pinned host [2B]
  // answer set of the batch: ids | w | score, each [B][G] dense in the current size and G, room for
  // [capacity][kMaxAnswers]; one device block and one pinned block, allocated at the slot's first set
  int32_t* ans_ids_d = nullptr;
  float *ans_w_d = nullptr, *ans_score_d = nullptr;
  int32_t* ans_h = nullptr;         // pinned host: ids | w | score
  bool ans_pending = false;         // a copy out of ans_h is behind the last record of `uploaded`
  // region counts of the batch: [capacity] device and pinned host, allocated at the slot's first set (a captured
  // step holds nreg_d's address)
  int32_t* nreg_d = nullptr;
  int32_t* nreg_h = nullptr;
  bool reg_pending = false;         // a copy out of nreg_h is behind the last record of `uploaded`
  // attention targets of the batch: device [capacity][Sp] at the attention's pitch (pad columns stay zero), pinned
  // host [capacity][S] dense; allocated at the slot's first set (a captured step holds att_t_d's address)
  float* att_t_d = nullptr;
  float* att_t_h = nullptr;
  bool att_pending = false;         // a copy out of att_t_h is behind the last record of `uploaded`
  // per-sample loss weights of the batch: [capacity] device and pinned host, allocated at the slot's first set (a
  // captured step holds sw_d's address, never its contents)
  float* sw_d = nullptr;
  float* sw_h = nullptr;
  bool sw_pending = false;          // a copy out of sw_h is behind the last record of `uploaded`
  // candidates of the batch: [B][C] dense in the current size and C, room for [capacity][kMaxCandidates]; device and
  // pinned host, allocated at the slot's first list (a captured step holds cand_d's address, never its contents)
  int32_t* cand_d = nullptr;
  int32_t* cand_h = nullptr;
  bool cand_pending = false;        // a copy out of cand_h is behind the last record of `uploaded`
  // the caller's question state (rau_set_question_dev): device [capacity][Q] f32, allocated at the slot's first
  // attach (a captured step holds q_ext's address, never its contents)
  float* q_ext = nullptr;
  // the caller's attention bias (rau_set_att_bias_dev): device [capacity][Sp] f32 at the attention's pitch, allocated
  // at the slot's first attach (a captured step holds zb_ext's address, never its contents)
  float* zb_ext = nullptr;
  // packed region rows (rau_set_batch_packed): the raw rows [sum(counts)][D] land in pk_rows_d (room for
  // [capacity * S][D] floats) and unpack_regions transposes them into `feats`; pk_meta_d holds off[n_maps] |
  // cnt[n_maps] (room for 2 * capacity), pk_meta_h is its pinned staging on the asynchronous path.  Allocated at
  // the slot's first packed batch.
  void* pk_rows_d = nullptr;
  int32_t* pk_meta_d = nullptr;
  int32_t* pk_meta_h = nullptr;
  hipEvent_t uploaded = nullptr;    // recorded on the copy stream behind the slot's H2D copies
  hipEvent_t consumed = nullptr;    // recorded on the chain stream when the ctx switches away from the slot
  // ---- what the device buffers hold
  BatchDesc held;
  // ---- upload ordering
  bool upload_pending = false, consumed_valid = false;
};

// What a stream owns besides its queue: launches that share a workspace must be ordered by their stream, so
// whoever launches on `owner` takes the scratch from the same record (lin_opts below wires the slab into a GEMM).
struct StreamWs {
  hipStream_t owner = nullptr;   // a copy of the handle: rau_ctx::st, st2 or st3
  float* slab = nullptr;         // split-K workspace
  size_t floats = 0;             // what the current batch size asks for: the launch policy reads this
  size_t alloc = 0;              // floats really allocated (>= floats after a resize)
  float* coltmp = nullptr;       // column-sum scratch of colsum_acc (bulk and side stream)
};

// The one place that maps a slot's buffers to a target: its labels, or (G > 0) the answer set in their place
inline Truth truth_of(const BatchSlot& s) {
  return s.held.have_labels ? Truth{s.labels_d, s.ans_ids_d, s.ans_w_d, s.ans_score_d, s.held.ans_G} : Truth{};
}

// Merged hops (rau_merge.hip: rau_step_stats / rau_predict / rau_topk): what those entry points know about the
// last step-level forward.  rau_ctx::mg.
struct MergeState {
  // ---- what the last forward left (merge_record)
  bool valid = false;             // logits / dopred / argmax_d / lossrow / a hold the last step-level forward's
  Truth truth;                    // ... of a batch with this ground truth (read from the slot's device buffers)
  int slot = 0;                   // the batch slot that forward read, and its upload serial then
  uint64_t serial = 0, fwd = 0;   // ... / forwards recorded so far
  // ---- what rau_predict left
  bool merged = false;            // a rau_predict has filled pred, att
  uint64_t pred_fwd = 0;          // the forward the last rau_predict read
  bool pred_mc = false;           // that rau_predict had an MC list
  // ---- buffers, allocated once (merge_alloc; mc and topk at their first use, regrown)
  bool ready = false;
  float *rowf = nullptr, *out = nullptr, *pred = nullptr, *att = nullptr;
  int32_t *rowi = nullptr, *ans = nullptr, *mc = nullptr;
  size_t mc_cap = 0;              // int32 entries mc holds
  float* score = nullptr;         // rau_step_scores / rau_predict_scores: rows [2(H+2)][B] | totals [2(H+2)]
  // rau_topk's staging: ids | score | conf, each [H+2][B][k]; room for [H+2][cap][topk_k], allocated at
  // its first call and regrown when a larger k is asked for
  void* topk = nullptr;
  int topk_k = 0;
  // rau_topk_cand / rau_cand_stats (cand_rank.hip), one block allocated at the first call of either: the ranked
  // lists' staging ids | score | conf, room for [H+2][cap][kMaxCandidates] each, then the statistics' rows
  // (H+4) * cap floats, (H+3) * cap int32, and their results 3 (H+2) + 1 words
  uint32_t* cand = nullptr;
  // no forward result, no rau_predict result, no ground truth: a fresh context's (rau_set_batch_size)
  void invalidate() { valid = merged = false; truth = Truth{}; }
};

// The hop-weight staging (two pinned slots in rau_ctx::hopw_h, one device copy in hopw_d), defined here only:
// hop_w [H] | select_w [H] | att_w [H] | merge_w [2].  The members are offsets in floats.
struct HopwLayout {
  size_t select_w, att_w, merge_w, size;
  explicit HopwLayout(int H) : select_w(H), att_w((size_t)2 * H), merge_w((size_t)3 * H), size((size_t)3 * H + 2) {}
};
// The loss terms of one step-level backward, normalised once (step_loss in rau_ctx.hip): what backward_impl,
// graph_step_impl and upload_hop_weights read in place of the entry points' pointer arguments.
struct StepLoss {
  const float* hop_w = nullptr;      // [H] per-hop weights of the answer criterion
  // null when the term is absent or all-zero: the path without it, launch for launch
  const float* select_w = nullptr;   // [H] step-selection head's BCE (select_bwd.hip)
  const float* att_w = nullptr;      // [H] attention supervision (att_sup.hip)
  const float* merge_w = nullptr;    // [2] the merged rows' cross-entropies: uni, select (merge_grad.hip)
  // Hops behind the last one with a non-zero loss weight receive no gradient at all (zero criterion gradient,
  // zero recurrent gradient: Full/ResNet late-epoch gating, Full:587-589): their backward is identically zero
  // and is skipped -- `active` hops are "active".  H with a merge_w: the uni row reads every hop.
  int active = 0;
  // caller-supplied gradients at the outputs (rau_backward_ext, ext_grad.hip): DEVICE pointers, null = no such
  // term; step_loss() leaves the record empty when all three are null.  With any of them every hop is active.
  rau_out_grads ext{nullptr, nullptr, nullptr};
  bool has_ext() const { return ext.d_logits || ext.d_dopred || ext.d_attprob; }
  bool hop_any = false;              // hop_w has a non-zero entry (an ext backward without one needs no labels)
  // caller-supplied gradients at the hop states (rau_backward_state): DEVICE pointers, null = no such term.  d_h is
  // every hop's HopGrad::dh_next, d_c_last the hop loop's first dc_next.  With either of them every hop is active.
  rau_state_grads sg{nullptr, nullptr};
  bool has_sg() const { return sg.d_h || sg.d_c_last; }
  bool external() const { return has_ext() || has_sg(); }   // some gradient comes from the caller: needs no label
  // select_w, merge_w and the external gradients are per-row terms, which cannot be folded into what the forward
  // formed (one scale per hop): such a backward forms dpre / dhn itself from the final dl
  bool forms_dpre() const { return select_w || merge_w || has_ext(); }
};
// What shapes a captured step (rau_graph_step): one executable graph per distinct value (step_key() below).
struct StepKey {
  int mode = 0;                 // rau_mode
  int max_len = 0;              // the longest question: the encoder's token count
  int active = 0;               // StepLoss::active: the hops the backward runs
  bool zero = false;            // the gradient zeroing is in front of the step
  bool mexplicit[5] = {};       // which mask sites are caller-supplied
  int slot = 0;                 // the captured kernels hold the batch slot's device pointers
  int feat_type = 0;            // ... and read the batch in its element type
  bool table = false;           // ... through the gather of an image table (any table, any N)
  bool bank = false;            // ... of a bank batch: out of the bank (rau_bank_destroy drops these)
  // ... against an answer set of G entries (0 = labels): another head kernel (the one reader besides truth_of())
  int ans_G = 0;
  int B = 0;                    // every launch is shaped by the batch size (rau_set_batch_size)
  bool sel = false;             // ... and by the step-selection head's gradient being asked for
  // ... and the attention kernels hold the slot's region counts or a null pointer (rau_set_regions)
  bool regions = false;
  // ... and a step with a non-zero att_w has one more launch and hands every hop its da_out; the batch's targets
  // (rau_set_att_targets) are what that launch reads
  bool att = false;
  bool att_targets = false;
  bool mrg = false;             // ... and a step with a non-zero merge_w has the merge_grad launch
  // ... and under RAU_XDROP_TIED a train-mode step has one masked map, one conv group and the summed conv gradients
  bool tied_x = false;
  int ans_loss = 0;             // ... and the head kernel is the answer criterion's (rau_set_answer_loss)
  int feat_grad = 0;            // ... and with rau_set_feat_grad the conv gradients are followed by the feature-map
                                // gradient: the mode (per sample / per image of a table: another accumulate kernel)
  bool question = false;        // ... and with a question attached (rau_set_question_dev) neither pass launches the
                                // encoder: the hop chain reads the slot's q_ext
  bool sample_w = false;        // ... and the kernels that form the training terms hold the slot's sample weights
                                // or a null pointer (rau_set_sample_weights); a replay reads the current weights
  int cand_C = 0;               // ... against C candidates per sample (0 = none): another head kernel, which holds the
                                // slot's list (rau_set_candidates); a replay reads the current list
  bool state = false;           // ... and with an initial state attached (rau_set_state_dev) the forward does not clear
                                // slot 0 of cc / hh and the backward ends hop 0 with the state gradient's launch; a
                                // replay reads the slot's current contents
  bool att_bias = false;        // ... and with an attention bias attached (rau_set_att_bias_dev) the attention kernels
                                // hold the slot's zb_ext and the backward ends with the bias gradient's launch; a
                                // replay reads the buffer's current contents
  int xnorm = 0;                // ... and with rau_set_feat_norm the image side starts with the normalisation pass (and
  uint32_t xnorm_eps = 0;       // the backward may end with its gradient), which holds eps as an argument: its bits
  auto tied() const {
    return std::tie(mode, max_len, active, zero, mexplicit[0], mexplicit[1], mexplicit[2], mexplicit[3], mexplicit[4],
                    slot, feat_type, table, bank, ans_G, B, sel, regions, att, att_targets, mrg, tied_x, ans_loss,
                    feat_grad, question, sample_w, cand_C, state, att_bias, xnorm, xnorm_eps);
  }
  bool operator==(const StepKey& o) const { return tied() == o.tied(); }
};
struct StepGraph {
  StepKey key;
  hipGraphExec_t exec;
};

// What the last step-level forward left for its backward.  rau_ctx::fwd: rau_forward fills it, drop_forward()
// (below) is the one way to take the backward away, "no forward" is FwdRecord{} (rau_set_batch_size).
struct FwdRecord {
  bool done = false;              // a backward may run: a forward has, and nothing since has overwritten what it left
  bool table = false;             // it read P and I per IMAGE (evaluate-mode fast path): no per-sample I to differentiate
  // the two layout facts of the hop buffers; rau_multimodal_forward writes them too (false: it fills the hop's own rows)
  bool I_shared = false;          // evaluate mode, p_x = 0 or a tied mask: i_embed output is hop-invariant, computed once
  bool yq_shared = false;         // no dropout on q (evaluate mode): q_embed's question half is rows of hop 0 only
  bool tied = false;              // a train-mode forward under RAU_XDROP_TIED: summed conv gradients
  const float* x_shared = nullptr;  // ... and i_embed's input then: xd (the one masked map) or, without a mask, xw
  float* xw = nullptr;            // f32 image of the unmasked batch it read: feats, or (16-bit batch) the first
                                  // B*D*Sp floats of xd, widened there by that forward
  bool xgen = false;              // it drew the feature-map keep bits inside its dropout pass: they were never in
                                  // memory, the backward regenerates them (philox.h)
  uint64_t seed = 0;              // ... from the key it ran under: a rau_set_dropout_seed between it and the
  uint32_t step = 0;              // backward would regenerate other bits, and is refused with the switch on
  bool dl = false;                // it wrote dl: its batch had labels or an answer set (rau_backward_ext)
  bool dpre = false;              // it already formed dpre / dhn of every hop (unscaled by the hop weights)
  std::vector<int> groups;        // the launch partition it used (rau_ctx::groups; evaluate mode: one group of H)
  int xn_rows = 0;                // (rau_set_feat_norm) xn / nrm hold that many normalised maps of it: n, or the table's N
                                  // after an evaluate-mode table forward; 0 = none.  Outlives drop_forward().
};
// What the last step-level backward left for the getters.  rau_ctx::bwd: record_backward (rau_ctx.hip) fills it for
// backward_impl and graph_step_impl, "no backward" is BwdRecord{} (rau_set_batch_size).
struct BwdRecord {
  bool done = false;              // rau_wait_grads / rau_allreduce_grads have something to wait for
  bool graph = false;             // it ran inside a graph (its events are graph-internal: only evEnd is waitable)
  // of a backward since the last forward (rau_forward clears both, rau_set_feat_grad dX on a change of mode):
  bool dq = false;                // rau_ctx::dq holds the gradient at the ATTACHED question (rau_question_grad_dev)
  bool dX = false;                // xg_dX holds the feature-map gradient (rau_get_feat_grad) ...
  int dX_rows = 0;                // ... its map count: n, or the table's N under RAU_FEAT_GRAD_IMAGES
  bool dbias = false;             // rau_ctx::zbgrad holds the gradient at the ATTACHED attention bias (rau_att_bias_grad_dev)
  bool dstate = false;            // rau_ctx::sgrad holds the gradient at the ATTACHED initial state (rau_state_grad_dev)
};

struct rau_ctx {
  rau_config cfg;             // cfg.B is the CURRENT batch size (rau_set_batch_size): what every layout, launch and
                              // getter reads at call time -- the B of the fresh context this one is equivalent to
  int cap = 0;                // the B of rau_create: what every buffer that depends on the batch size is allocated for
  int Q;
  int Sp = 0;                 // position pitch: cfg.S rounded up to a multiple of 4 (7x7 maps: 49 -> 52);
                              // every [.., S]-shaped device tensor uses it, pad columns hold zeros
  int Kp = 0;                 // answer pitch: cfg.K rounded up to a multiple of 4 (3129 -> 3132); the row pitch of
                              // logits, dl and mg.pred, pad columns hold +0.  K % 4 == 0: Kp == K, nothing changes
  int bf16 = 0;               // cfg.dtype == RAU_BF16: bf16-operand conv GEMMs
  Policy policy;              // the A/B variables as rau_create found them: a context runs under the environment
                              // it was created in (policy.h)
  hipStream_t st = nullptr;    // chain stream: recurrences, small GEMMs; what callers order against
  hipStream_t st2 = nullptr;   // bulk stream: hop-batched 1x1-conv GEMMs, overlapped with the chain
  hipStream_t st3 = nullptr;   // weight-gradient stream: throughput GEMMs nobody waits for until the end
  StreamWs ws_chain, ws_bulk, ws_side;   // the workspaces of st, st2 and st3 (stream_ws() below lists them)
  hipEvent_t evA = nullptr, evD = nullptr, evW = nullptr, evE = nullptr, evW3 = nullptr,
             evM3 = nullptr, evEnd = nullptr, evE1 = nullptr, evHd = nullptr,
             evG0 = nullptr, evG = nullptr, evQ0 = nullptr, evQ = nullptr, evDq = nullptr;   // side-stream forks / joins
  hipEvent_t evGc[kEncSideChunks] = {};   // layer-1 input projection, chunk c done on the third stream
  int enc_chunk_tok[kEncSideChunks + 1] = {};   // first token of chunk c (last entry: TL) in the current forward
  std::vector<hipEvent_t> evH;       // per hop: forward chain done (the head stream waits on it)
  std::vector<hipEvent_t> evF, evK;  // per hop group: forward bulk done / backward chain done
  // hops per bulk launch (pipelines the bulk GEMMs with the hop loops): gsize[h] = n if hops
  // [h, h+n) form one launch group, else 0.  `groups` is the configured partition (FwdRecord::groups: the last forward's).
  std::vector<int> groups, bgroups;   // bgroups: backward partition (empty = same as forward)
  std::vector<void*> allocs;
  // what rau_set_batch_size clears: every dalloc'ed region except parameters, gradients, Adam moments, the Philox
  // key and rau_dev_alloc'ed memory.  The layouts are dense in the current batch size, so after a change stale
  // data would sit where the step expects the zeros of a fresh context (initial-state rows, pad columns).
  std::vector<std::pair<void*, size_t>> scratch;
  Group grp[3];
  // mult
  Lin q_proj, h_proj, i_embed, att_q, att_i, att_score, att_mem, feat_attprob, lstm_i2h,
      lstm_h2h, lstm_out, cls, do_pred;
  // rnn
  Lin i2h[2], h2h[2];
  // batch (the resident one is slot[cur_slot], below)
  float* feats_x = nullptr;       // [B][D][Sp] per-sample maps gathered from the table (expand_features), in the
                                  // batch's element type; allocated at the first table batch
  bool x_valid = false;           // feats_x holds the expansion of upload x_serial into slot x_slot
  int x_slot = 0;
  uint64_t x_serial = 0;
  // feature bank (rau_bank_*): every image's map once, in the batch buffers' layout [capacity][D][Sp]
  void* bank = nullptr;
  int32_t bank_cap = 0, bank_filled = 0;
  int bank_type = RAU_FEAT_F32;
  std::vector<uint8_t> bank_written;   // host record: row has been put
  void* bank_pin[2] = {nullptr, nullptr};   // pinned staging of rau_bank_put, bank_chunk bytes each
  float* bank_stage = nullptr;              // device: one chunk of f32 maps on their way to a 16-bit bank
  size_t bank_chunk = 0;
  // rau_bank_put_packed: off | cnt of one chunk's maps (kBankPackMaps each), device and pinned per staging half
  int32_t* bank_meta_d = nullptr;
  int32_t* bank_meta_pin[2] = {nullptr, nullptr};
  hipEvent_t bank_ev[2] = {nullptr, nullptr};
  // the two batch slots; the synchronous path uploads into the current one
  BatchSlot slot[2];
  uint64_t slot_serial[2] = {0, 0};   // uploads into each slot's device buffers so far
  int cur_slot = 0;
  bool async_ready = false;          // slot 1, the staging, the events and the copy stream exist
  hipStream_t stc = nullptr;         // copy stream
  hipEvent_t hopw_ev[2] = {nullptr, nullptr};   // hop-weight staging slots: H2D copy done
  // dropout
  int mode = RAU_MODE_TRAIN;
  uint32_t* mbits[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t mcount[5] = {0, 0, 0, 0, 0};
  bool mexplicit[5] = {false, false, false, false, false};
  float mp[5];        // drop probability of the device's Philox masks: p quantised to 1/256
  float mp_exact[5];  // the configured p: scale 1/(1-p) of caller-supplied masks (nn.Dropout's)
  uint64_t seed = 0;
  uint32_t step = 0;
  // encoder activations
  float *we, *G1, *G2, *c1, *h1, *c2, *h2, *tc1, *tc2, *x2, *q;
  // RAU activations
  float *xd;          // [H][B][D][S] feature map after per-hop dropout (train mode)
  void* WiT16 = nullptr;  // with xd16: bf16 copies of the transposed conv weights WiT, WpT
  void* WpT16 = nullptr;
  void* dS16 = nullptr;  // with xd16: the attention backward's dS as bf16 [H][B][A][S] (both consumers round it anyway)
  void* xd16 = nullptr;  // RAU_BF16 step path, S % 4 == 0: the same maps stored as bf16 (xd stays unwritten)
  // feature-map dropout kind (rau_set_feat_dropout): RAU_XDROP_PER_HOP, or RAU_XDROP_TIED = one mask for all hops
  int xdrop = RAU_XDROP_PER_HOP;
  // gradient at the attached initial state (rau_set_state_dev, state_io.hip): d_c0 | d_h0, [2][cap][R] with the halves
  // dense in the current n, allocated at the first attach; every backward on an attached state overwrites it
  float* sgrad = nullptr;
  // gradient at the attached attention bias (rau_set_att_bias_dev, att_bias.hip): [cap][Sp], rows dense in the current
  // n at the attention's pitch, allocated at the first attach; every backward on an attached bias overwrites it
  float* zbgrad = nullptr;
  float* m_zadd = nullptr;   // rau_multimodal_forward_bias: the caller's dense [n][S] rows at the pitch, [cap][Sp]
  float* dS_sum = nullptr;          // [cap][A][Sp] sum of the active hops' dS (tied_bwd.hip), allocated with the switch
  // feature-map gradient (rau_set_feat_grad, xgrad.hip): off = the step path as it is without it
  int feat_grad = RAU_FEAT_GRAD_OFF;   // the mode: _SAMPLES, or _IMAGES = per image where the batch has a table
  float* xg_dX = nullptr;           // [cap][D][Sp] the last backward's result (bwd.dX), allocated with the switch
  float* xg_tmp = nullptr;          // [cap][D][Sp] one hop's unmasked product (the unfused path)
  float* xg_dz = nullptr;           // [cap][M][Sp] dI (1 - I^2) where the dgrad left dI (no fused tanh derivative)
  // per-position L2 normalisation of the batch's maps (rau_set_feat_norm, featnorm.hip): off = the step path as it is
  int xnorm = RAU_XNORM_NONE;
  float xnorm_eps = 1e-12f;
  float* xn = nullptr;              // [cap][D][Sp] the last forward's normalised maps (fwd.xn_rows of them): what the
                                    // image side reads as an f32 batch; allocated with the switch, like nrm
  float* nrm = nullptr;             // [cap][Sp] their norms
  // rau_set_batch_dev: pinned staging of the index arrays, two halves alternated like hopw_h
  int32_t* bdev_h[2] = {nullptr, nullptr};
  hipEvent_t bdev_ev[2] = {nullptr, nullptr};
  int bdev_slot = 0;
  // the answer criterion of the step path (rau_set_answer_loss): RAU_LOSS_CE, or RAU_LOSS_BCE = per-answer sigmoid.
  // Read through step_truth() only; the module-level criteria name theirs themselves.
  int answer_loss = RAU_LOSS_CE;
  float *WiT, *WpT;   // i_embed / ifeatproj weights transposed ([D][M], [M][A]), refreshed per forward
  float *P0;          // [B][A][S] hop-invariant attention pre-activation (evaluate mode)
  float *qd, *Yq, *qf, *I, *T, *u, *zm, *a, *jv, *j, *g4, *cc, *hh, *tc, *mf, *logits,
      *dl, *lossrow, *dopred, *losses_d, *hopw_d;
  int32_t* argmax_d;
  float* att_part = nullptr;  // [B][chunks][S] partial column sums of the split attention kernels
  bool att_split = false;     // 4-wave row-chunk attention kernels instead of the fused ones (plan_batch: by shape)
  // persistent encoder forward (enc_ws.hip): device error word (a bounded spin gave up), copied to pinned memory behind the launch
  bool enc_ws = false;          // weight-stationary persistent encoder forward (enc_ws.hip): evaluate mode
  bool enc_ws_train = false;    // ... and in training steps
  unsigned* ws_cnt = nullptr;   // its 16 progress counters
  int* perr_d = nullptr;
  int* perr_h = nullptr;
  bool persist_used = false;
  bool persist_gave_up = false; // persist_check() turned the persistent encoder off: it stays off across resizes
  float* hopw_h = nullptr;    // pinned staging of the hop weights: 2 slots of HopwLayout::size
  int hopw_slot = 0;
  // attention supervision (rau_backward_att, att_sup.hip): the gradient at the attprob output of every hop,
  // [H][cap][Sp] at the attention's pitch, allocated at the first call with a non-zero att_w
  float* att_da = nullptr;
  // ... and its statistics' scratch (rau_att_stats, rau_att_criterion_forward): rows [2][H*cap] | results [2][H]
  float* att_sf = nullptr;
  int32_t* att_si = nullptr;
  // step-selection head's gradient (rau_backward_select, select_bwd.hip)
  float *sel_s = nullptr, *sel_add = nullptr;   // [H][cap] s rows, [H][cap][M] s (x) wd; allocated at first use
  // backward temporaries
  // dZ holds dI (gradient at i_embed's OUTPUT); the tanh derivative is applied by its consumers
  float *dpre, *dhn, *dg4, *dcn[2], *dhp[2], *dj, *da_lin, *dz, *du, *dwsp, *dZ,
      *dqt, *dQD, *dq, *tmpS, *dbi_part;
  float *dG1, *dG2, *dwe, *edc[2][2];
  // module-level entry points (rau_modules.hip); allocated on first use
  bool mod_ready = false;
  float *m_state = nullptr, *m_dstate = nullptr;   // [T][B][Q] packed DeepLSTM state slots
  float *m_tmp[4] = {nullptr, nullptr, nullptr, nullptr};  // [B][max(Rq,R,M)] scratch
  float *m_dq = nullptr, *m_dc = nullptr, *m_dh = nullptr;  // [H][B][Q], [H][B][R], [H][B][R]
  float *m_Xp = nullptr, *m_a = nullptr, *m_da = nullptr, *m_dXd = nullptr;  // re-pitching (S % 4 != 0)
  float* m_Xw = nullptr;   // [B][D][Sp]: f32 image of a 16-bit resident batch (X = NULL)
  float *m_dX = nullptr, *m_dZ = nullptr;          // [B][D][S], [B][M][S]: feature-map gradient, on request
  float *m_add = nullptr, *m_s = nullptr, *m_zero = nullptr;  // [B][M], [B], zeros [B][max(Q,R)]
  float *m_loss = nullptr;                         // [H] criterion outputs
  float *m_datt = nullptr;                         // [B][S] dense: rau_att_criterion_backward's d_attprob, on first use
  uint64_t mod_masks_seed = 0;                     // (seed, step) the device masks were drawn for
  uint32_t mod_masks_step = 0;
  bool mod_masks_valid = false;
  // native data-parallel exchange (rau_comm_*; RCCL loaded with dlopen on first use)
  void* comm = nullptr;          // ncclComm_t
  hipStream_t st_comm = nullptr;
  hipEvent_t evC = nullptr;
  int comm_ranks = 0;
  // hipGraph replay of a whole step (rau_graph_step): one executable graph per step "shape"
  uint64_t* dkey = nullptr;      // device copy of (seed, step): what fill_masks reads
  bool capturing = false;
  std::vector<StepGraph> graphs;
  MergeState mg;                 // merged hops (rau_merge.hip): what may be read of the last forward
  // update
  float *npart = nullptr, *norms_d = nullptr;
  float* upd_part = nullptr;     // rau_update's partial sums of squares, [3][kUpdParts]
  bool ema_swapped = false;      // rau_ema_swap: the weights' buffers hold the average and the other way round
  // per-layer statistics and the update guard (layer_stats.hip); everything here comes with the first use
  struct LayerStats {
    StatItem* items = nullptr;          // device: the work table, fixed for the context's life
    StatEntry* entries = nullptr;       // device [n_entries]
    uint32_t* partial = nullptr;        // device [n_items][kStatPartWords]
    rau_layer_stat* out = nullptr;      // device [n_entries]: what rau_layer_stats_dev hands out
    int64_t* totals = nullptr;          // device [3 sources][3 groups] non-finite counts of the last pass
    int n_items = 0, n_entries = 0;
    int group_first[4] = {0, 0, 0, 0};  // group g's items are group_first[g] .. group_first[g + 1] - 1
  } ls;
  int guard_mode = RAU_GUARD_OFF;       // rau_set_update_guard; survives rau_set_batch_size
  int64_t guard_skipped = 0;
  int32_t guard_last_skipped = 0;
  int64_t guard_last_nonfinite[3] = {0, 0, 0};
  FwdRecord fwd;                 // what the last step-level forward left for its backward
  BwdRecord bwd;                 // what the last step-level backward left for the getters
  // timing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool prof_on = false;
  bool prof_sparse = false;   // rau_prof_enable(ctx, 2): chain-stream launches are NOT bracketed except phase
                              // markers, so the recurrence runs at its un-profiled speed under the timeline
  std::vector<ProfCls> pcls;
  std::vector<ProfRec> precs;
  std::vector<hipEvent_t> evpool;
};

// The resident batch: what every reader of the batch goes through.
inline BatchSlot& cur_batch(rau_ctx* ctx) { return ctx->slot[ctx->cur_slot]; }
inline const BatchSlot& cur_batch(const rau_ctx* ctx) { return ctx->slot[ctx->cur_slot]; }
// The last forward has no backward any more, and nothing else: callers that also drop mg.valid say so next to this
inline void drop_forward(rau_ctx* ctx) { ctx->fwd.done = false; }
// The module-level calls that exchange dense [B,K] tensors with the caller need K % 4 == 0 (their rows feed the
// 16-byte loaders directly): on any other context they are refused before anything is launched.
#define NEED_DENSE_K(ctx, fn)                                                                              \
  NEED((ctx)->Kp == (ctx)->cfg.K, "%s: module-level calls exchange dense [B,K] rows and need K %% 4 == 0 " \
       "(K=%d); use the step-level path", fn, (ctx)->cfg.K)
// What the hop chain reads as the question state: the caller's (rau_set_question_dev) or the built-in encoder's
inline const float* question_state(const rau_ctx* ctx) {
  const BatchSlot& s = cur_batch(ctx);
  return s.held.question ? s.q_ext : ctx->q;
}
// The resident batch's feature-map gradient is formed per IMAGE: RAU_FEAT_GRAD_IMAGES on an image table.  (A bank
// batch has no gradient in either mode; on a batch with one map per sample the mode is RAU_FEAT_GRAD_SAMPLES.)
inline bool xgrad_per_image(const rau_ctx* ctx) {
  const BatchDesc& d = cur_batch(ctx).held;
  return ctx->feat_grad == RAU_FEAT_GRAD_IMAGES && d.n_images > 0 && !d.bank;
}
// The key of the step that `loss` asks for on the resident batch, as the context is configured now
inline StepKey step_key(const rau_ctx* ctx, const StepLoss& loss, bool zero) {
  const BatchDesc& d = cur_batch(ctx).held;
  StepKey key;
  key.mode = ctx->mode;
  key.max_len = d.max_len;
  key.active = loss.active;
  key.zero = zero;
  std::copy(ctx->mexplicit, ctx->mexplicit + 5, key.mexplicit);
  key.slot = ctx->cur_slot;
  key.feat_type = d.feat_type;
  key.table = d.n_images > 0;
  key.bank = d.bank;
  key.ans_G = d.ans_G;
  key.B = ctx->cfg.B;
  key.sel = loss.select_w != nullptr;
  key.regions = d.regions;
  key.att = loss.att_w != nullptr;
  key.att_targets = d.att_targets;
  key.mrg = loss.merge_w != nullptr;
  key.tied_x = ctx->xdrop == RAU_XDROP_TIED;
  key.ans_loss = ctx->answer_loss;
  key.feat_grad = ctx->feat_grad;
  key.question = d.question;
  key.sample_w = d.sample_w;
  key.cand_C = d.cand_C;
  key.state = d.state;
  key.att_bias = d.att_bias;
  key.xnorm = ctx->xnorm;
  if (ctx->xnorm) std::memcpy(&key.xnorm_eps, &ctx->xnorm_eps, sizeof(float));
  return key;
}

// Effective drop probability of a mask site.  Masks the device draws itself (Philox, 8-bit draws)
// drop with p quantised to 1/256 and scale by 1/(1-pq), so that E[mask * scale] = 1 exactly;
// caller-supplied masks (rau_set_mask) are nn.Dropout's: scale 1/(1-p) with the configured p.
// Non-recurrent GEMMs of the recurrence's stream (layer-1 input projection beyond the first tokens,
// q_embed's question half of hops 1.., the dq terms of finished backward groups) run on the
// weight-gradient stream where the recurrence is the longer path: evaluate mode, bf16 mode (forward
// phase bound by the encoder), contexts of up to 64 samples.  In the f32 step at 256 samples the bulk
// stream is the longer path and the extra concurrency costs it 1 %.
inline bool chain_bound(const rau_ctx* ctx) {
  return ctx->mode == RAU_MODE_EVAL || ctx->bf16 || ctx->cfg.B <= 64;
}
inline bool side_split(const rau_ctx* ctx) {
  if (ctx->policy.side_split >= 0) return ctx->policy.side_split != 0;
  return chain_bound(ctx);
}
// How this context's Linear GEMMs are formed NOW: bf16 products by its dtype, and the recurrence's skinny GEMMs
// with 32-deep stages (skinny_dma.hip, NH = 2) under the same predicate as the side split (Policy::skinny_deep
// overrides).  chain_bound() depends on the mode and the batch size, which change after rau_create: computed at
// every launch, never stored.
inline LinMode lin_mode(const rau_ctx* ctx) { return lin_mode(ctx->policy, ctx->bf16, chain_bound(ctx)); }
// The same for its conv products (every launcher and every predicate that sizes a buffer for one takes this) and
// for its attention kernels
inline ConvMode conv_mode(const rau_ctx* ctx) { return conv_mode(ctx->policy, ctx->bf16, chain_bound(ctx)); }
inline AttMode att_mode(const rau_ctx* ctx) {
  return att_mode(ctx->policy, ctx->bf16, ctx->mode == RAU_MODE_EVAL);
}
// The three workspaces, in the order of BatchPlan::ws (chain, bulk, side)
inline std::array<StreamWs*, 3> stream_ws(rau_ctx* ctx) { return {&ctx->ws_chain, &ctx->ws_bulk, &ctx->ws_side}; }
// Options of a Linear GEMM launched on ws.owner: the context's mode and that stream's split-K workspace.  Every
// LinOpts that reaches a GEMM starts here; callers that carve a region out of the slab, or point it at other
// scratch, overwrite slab / slab_floats afterwards.
inline LinOpts lin_opts(const rau_ctx* ctx, const StreamWs& ws) {
  LinOpts o;
  o.mode = lin_mode(ctx);
  o.slab = ws.slab;
  o.slab_floats = ws.floats;
  return o;
}
// The resident batch's ground truth with the criterion the step path trains it with (rau_set_answer_loss)
inline Truth step_truth(const rau_ctx* ctx) {
  const BatchSlot& s = cur_batch(ctx);
  Truth t = truth_of(s);
  t.loss = ctx->answer_loss;
  t.sw = s.held.sample_w ? s.sw_d : nullptr;   // the step path's terms only: module-level criteria stay unweighted
  t.cand = s.held.cand_C > 0 ? s.cand_d : nullptr;   // ... and so do the candidates (with or without a ground truth)
  t.C = s.held.cand_C;
  return t;
}
// The hop outputs now hold the results of the forward just enqueued: rau_step_stats / rau_predict may
// read them until the next forward, module-level call or upload into the batch slot it read.
inline void merge_record(rau_ctx* ctx) {
  ctx->mg.valid = true;
  ctx->mg.truth = step_truth(ctx);
  ctx->mg.slot = ctx->cur_slot;
  ctx->mg.serial = ctx->slot_serial[ctx->cur_slot];
  ++ctx->mg.fwd;
}
inline float mask_p(const rau_ctx* ctx, int site) {
  return ctx->mexplicit[site] ? ctx->mp_exact[site] : ctx->mp[site];
}
// The keep bits of every mask site -- null outside train mode and where nothing is dropped -- and its scale 1/(1-p)
struct Masks {
  const uint32_t *we, *rnn, *q, *x, *mf;
  float s_we, s_rnn, s_q, s_x, s_mf;
};
__attribute__((visibility("hidden"))) inline Masks masks_of(const rau_ctx* ctx) {
  const bool tr = ctx->mode == RAU_MODE_TRAIN;
  auto mk = [&](int site) { return (tr && mask_p(ctx, site) > 0.f) ? (const uint32_t*)ctx->mbits[site] : nullptr; };
  auto sc = [&](int site) { return 1.f / (1.f - mask_p(ctx, site)); };
  return Masks{mk(RAU_MASK_WE), mk(RAU_MASK_RNN), mk(RAU_MASK_Q), mk(RAU_MASK_X), mk(RAU_MASK_MF),
               sc(RAU_MASK_WE), sc(RAU_MASK_RNN), sc(RAU_MASK_Q), sc(RAU_MASK_X), sc(RAU_MASK_MF)};
}
// FLOPs of an [m, k] x [k, n] product, as the profile counts them
inline double gflop(double m, double n, double k) { return 2.0 * m * n * k; }

// scratch = false: the region outlives rau_set_batch_size untouched (see rau_ctx::scratch)
template <typename Tp>
static int dalloc(rau_ctx* c, Tp** p, size_t count, bool scratch = true) {
  void* d = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(Tp);
  hipError_t e = hipMalloc(&d, bytes);
  if (e != hipSuccess)
    return fail(RAU_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
  e = hipMemsetAsync(d, 0, bytes, c->st);
  if (e != hipSuccess) return fail(RAU_ERR_DEVICE, "hipMemsetAsync: %s", hipGetErrorString(e));
  c->allocs.push_back(d);
  if (scratch) c->scratch.push_back({d, bytes});
  *p = reinterpret_cast<Tp*>(d);
  return 0;
}
// Gives a dalloc'ed region back before rau_destroy: no launch may still read it, and neither rau_destroy (allocs)
// nor rau_set_batch_size (which clears scratch) may see it again.
static inline int dfree(rau_ctx* c, void* p) {
  HIPC(hipStreamSynchronize(c->st));
  hipFree(p);
  c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), p), c->allocs.end());
  auto& sc = c->scratch;
  sc.erase(std::remove_if(sc.begin(), sc.end(), [p](const auto& r) { return r.first == p; }), sc.end());
  return RAU_OK;
}

struct LayoutBuilder {
  Group* g;
  size_t off = 0;
  Lin take(const char* name, int out, int in) {
    Lin l;
    l.out = out;
    l.in = in;
    g->layout.push_back({std::string(name) + ".weight", off, out, in});
    l.W = reinterpret_cast<float*>(off);
    off += (size_t)out * in;
    g->layout.push_back({std::string(name) + ".bias", off, out, 1});
    l.b = reinterpret_cast<float*>(off);
    off += out;
    return l;
  }
};
static inline void bind(Lin& l, const Group& g) {
  const size_t ow = reinterpret_cast<size_t>(l.W), ob = reinterpret_cast<size_t>(l.b);
  l.W = g.w + ow;
  l.b = g.w + ob;
  l.dW = g.g + ow;
  l.db = g.g + ob;
}

static inline int prof_class(rau_ctx* c, const char* name) {
  for (size_t i = 0; i < c->pcls.size(); ++i)
    if (c->pcls[i].name == name) return (int)i;
  c->pcls.push_back(ProfCls{name});
  return (int)c->pcls.size() - 1;
}
static inline hipEvent_t prof_event(rau_ctx* c) {
  if (!c->evpool.empty()) {
    hipEvent_t e = c->evpool.back();
    c->evpool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

// chain-stream classes the sparse timeline keeps (one launch each per phase boundary)
static inline bool prof_marker(const char* n) {
  for (const char* m : {"embed_fwd", "gather_q", "loss_reduce", "scale_hops", "dq_reduce", "embed_bwd"})
    if (std::strcmp(n, m) == 0) return true;
  return false;
}
// Measurement hook of the DEVELOPMENT build only (make dev -> librau_dev.so, -DRAU_DEV_HOOKS; the shipped
// library compiles it to `false`): RAU_DEV_SKIP=class1,class2,.. drops every launch of the named kernel
// classes.  Timing only -- the numerics of such a run are meaningless -- used for the per-class
// sensitivity tables (tools/dev_skip.sh, profiles/r04_forward_gap.md).  Consumers of split-K partials
// whose producer was skipped see a count of 0 or fail closed (split_guard.hip), never read out of bounds.
#ifdef RAU_DEV_HOOKS
static inline bool rau_dev_skipped(const char* cname) {
  static const std::string list = [] { const char* e = std::getenv("RAU_DEV_SKIP"); return std::string(e ? e : ""); }();
  if (list.empty()) return false;
  size_t pos = 0;
  const std::string n(cname);
  while (pos <= list.size()) {
    const size_t c = list.find(',', pos);
    const std::string tok = list.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    if (tok == n) return true;
    if (c == std::string::npos) break;
    pos = c + 1;
  }
  return false;
}
#define RAU_DEV_SKIPPED(cname) rau_dev_skipped(cname)
#else
#define RAU_DEV_SKIPPED(cname) false
#endif
// Launch wrapper: counts launches/FLOPs/bytes per kernel class and, when
// profiling is on, brackets the launch with HIP events on the ctx stream.
#define RUN(cname, fl, by, expr) RUNS(ctx->st, cname, fl, by, expr)
#define RUNS(rstream, cname, fl, by, expr)                                                \
  do {                                                                                    \
    ProfRec pr_;                                                                          \
    int pc_ = -1;                                                                         \
    if (ctx->prof_on && !(ctx->prof_sparse && (rstream) == ctx->st && !prof_marker(cname))) { \
      pc_ = prof_class(ctx, cname);                                                       \
      ctx->pcls[pc_].launches++;                                                          \
      ctx->pcls[pc_].flops += (double)(fl);                                               \
      ctx->pcls[pc_].bytes += (double)(by);                                               \
      pr_.cls = pc_;                                                                      \
      pr_.a = prof_event(ctx);                                                            \
      pr_.b = prof_event(ctx);                                                            \
      pr_.sid = (rstream) == ctx->st ? 0 : (rstream) == ctx->st2 ? 1 : 2; \
      hipEventRecord(pr_.a, rstream);                                                     \
    }                                                                                     \
    hipError_t e_ = RAU_DEV_SKIPPED(cname) ? hipSuccess : (expr);                         \
    if (pc_ >= 0) {                                                                       \
      hipEventRecord(pr_.b, rstream);                                                     \
      ctx->precs.push_back(pr_);                                                          \
    }                                                                                     \
    if (e_ == kSplitStateError)   /* a consumer of split-K partials refused a stale span */ \
      return fail(RAU_ERR_STATE, "kernel %s: split-K partials outside their workspace, "  \
                  "nothing launched (%s:%d)", cname, __FILE__, __LINE__);                  \
    if (e_ != hipSuccess)                                                                 \
      return fail(RAU_ERR_DEVICE, "kernel %s: %s (%s:%d)", cname, hipGetErrorString(e_),  \
                  __FILE__, __LINE__);                                                    \
  } while (0)

// ---- shared between the step-level path (rau_ctx.hip) and the module-level entry
// points (rau_modules.hip)
struct HopGrad {
  const float* dl;        // [B,K] gradient at the logits (already scaled by the hop weight)
  const float* dc_next;   // [B,R] or null (zeros)
  const float* dh_next;
  const float* dmf_add;   // [B,M] or null: extra gradient at merge_feat before its dropout
  const float* da_out;    // [B,S] or null: gradient at the attprob output
  float* dc_out;          // [B,R] out: gradient at prev_c
  float* dh_out;          // [B,R] out: gradient at prev_h (written only when dh_part_out is null)
  // step-level fast path (rau_backward): what does not depend on the recurrence is formed for
  // all hops up front, and dh_prev travels from hop to hop as K-split partials
  int dpre_ready;         // ctx->dpre rows of this hop already hold (dl Wc) (.) mask
  const float* dhn_all;   // [H*B,R] dpre Wo for all hops (with dpre_ready)
  const float* dh_part;   // [dh_part_ns][B,R] partials of the gradient at next_h (or null)
  int dh_part_ns;
  float** dh_part_out;    // non-null: leave dh_prev as partials and report them here
  int* dh_part_ns_out;
  hipEvent_t ev_conv_ready;  // non-null: recorded on the chain stream right behind att_bwd -- everything the
                             // bulk stream's conv gradients of this hop read (dS, dj) exists from there on
  bool dh_prev_dead;      // the gradient at prev_h has no consumer (step-level hop 0: the initial state is a
                          // constant): its three products are not formed
  bool ds16;              // step-level bf16 backward on 14x14 maps: the attention backward writes dS16, not T
};
__attribute__((visibility("hidden"))) int hop_forward(rau_ctx* ctx, int h, const float* cp,
    const float* hp, float* c_out, float* h_out, const float* Ih, const float* Pin,
    const Truth& truth, const int32_t* nreg = nullptr /* device [B] region counts, see hop_forward_chain */,
    const float* zadd = nullptr /* device [B][Sp] attention bias, see hop_forward_chain */);
__attribute__((visibility("hidden"))) int hop_forward_chain(rau_ctx* ctx, int h, const float* cp,
    const float* hp, float* c_out, float* h_out, const float* Ih, const float* Pin,
    const int32_t* img = nullptr /* device index: sample b's Ih / Pin tiles are row img[b] (image table) */,
    const int32_t* nreg = nullptr /* device [B]: sample b attends to its first nreg[b] positions only */,
    const float* zadd = nullptr /* device [B][Sp]: added to sample b's attention scores (AttPartials::zadd) */);
// The resident batch as per-sample maps [B][D][Sp] in its element type: the buffer itself, or for a batch
// with an image table its expansion (expand_features on the chain stream, once per upload).
__attribute__((visibility("hidden"))) int batch_maps(rau_ctx* ctx, const float** maps);
__attribute__((visibility("hidden"))) int hop_forward_head(rau_ctx* ctx, const StreamWs& ws, int h0, int nh,
    const Truth& truth);
__attribute__((visibility("hidden"))) int hop_backward(rau_ctx* ctx, int h, const float* cp,
    const float* Ih, const HopGrad& g);
// The image side of n maps on `s`: I = tanh(Wi x + bi) and P = Wp I + bp (x_is_b16: bf16 maps and weight copies)
__attribute__((visibility("hidden"))) int image_forward(rau_ctx* ctx, hipStream_t s, int n, const void* x,
    bool x_is_b16, float* I, float* P);
// Its gradients: dZ = (Wp^T dS + dj (x) a)(1 - I^2); dWp += dS I^T; dWi += dZ X^T (+ the i_embed bias gradient).
struct ConvGrads {
  int n;                              // maps
  const void* dS; bool ds_is_b16;     // [n][A][Sp], f32 or bf16 elements
  const float *dj, *a, *I;            // [n][M], [n][Sp], [n][M][Sp]
  const void* X; bool x_is_b16;       // [n][D][Sp] what i_embed read, f32 or bf16 elements
  void* dZ; bool dz_is_b16;           // [n][M][Sp] out, stored as f32 or bf16
  int dzf;                            // conv_dz_fused_ok: the dgrad applies (1 - I^2) itself ...
  float* dbi_part;                    // ... and leaves the row sums of dZ here, [n][M]
  int tied_hops;                      // > 1: dS is the sum of that many hops, outer_sum adds dj (x) a of hops 1..
};
// element i of a map buffer that holds bf16 (b16) or f32 elements
inline void* map_elems(void* base, bool b16, size_t i) {
  return b16 ? (void*)((uint16_t*)base + i) : (void*)((float*)base + i);
}
__attribute__((visibility("hidden"))) int conv_grads(rau_ctx* ctx, hipStream_t s, const ConvGrads& g);

// ---- shared between rau_ctx.hip and the merged-hops entry points (rau_merge.hip)
extern "C" {   // defined among the result getters, inside rau_ctx.hip's extern "C" block
// the persistent encoder's error word, read after a host synchronisation; the copy to the host that ends with both
__attribute__((visibility("hidden"))) int persist_check(rau_ctx* ctx);
__attribute__((visibility("hidden"))) int d2h(rau_ctx* ctx, void* host, const void* dev, size_t bytes);
}
__attribute__((visibility("hidden"))) int merge_state(rau_ctx* ctx, const char* fn, bool need_labels);  // rau_merge.hip
// layer_stats.hip: the guard in front of an update (rau_set_update_guard), called after argument validation and before
// anything else is launched.  0: the update proceeds (guard off, or no non-finite gradient element; `ex`: frozen
// layers are not looked at).  1: it is skipped -- the first n_norms entries of out_norms (may be null) hold NaN and the
// caller returns RAU_OK with nothing launched.  < 0: an error code.
__attribute__((visibility("hidden"))) int update_guard(rau_ctx* ctx, bool ex, float* out_norms, int n_norms);
// rau_merge.hip: the statistics' scratch exists; ATT rows / results of `hops` hops of a [hops][B] attention block
__attribute__((visibility("hidden"))) int att_stats_alloc(rau_ctx* ctx);

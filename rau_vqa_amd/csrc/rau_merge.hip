// rau_merge.hip -- the merged-hops entry points of include/rau.h: what is read from the hop outputs of the last
// step-level forward after it has run (kernels: hop_merge.hip, topk.hip): feval's statistics and metric scores
// (rau_step_stats, rau_step_scores), predict_result's answers and theirs (rau_predict, rau_predict_scores), ranked
// answers (rau_topk), the merged rows (rau_get_merged), and for a batch with candidates the MC statistics and ranked MC
// answers (rau_cand_stats, rau_topk_cand; kernels: cand_rank.hip).
// What they know about that forward is one record, rau_ctx::mg (rau_ctx.h: MergeState): merge_record() fills it
// behind a forward, merge_state() decides whether it may still be read, and whoever overwrites the hop outputs or
// the targets clears `valid`.  The target is the record's Truth, taken from the batch slot when the forward ran --
// the resident batch may be another one by now.
#include "rau_ctx.h"

namespace {
int merge_alloc(rau_ctx* ctx) {
  if (ctx->mg.ready) return RAU_OK;
  const rau_config& c = ctx->cfg;
  const size_t B = ctx->cap, H = c.H;   // sized for the capacity
#define CK(x) do { if (int rc_ = (x)) return rc_; } while (0)
  CK(dalloc(ctx, &ctx->mg.rowf, B * (H + 2)));
  CK(dalloc(ctx, &ctx->mg.rowi, B * RAU_STATS_NCOUNTS(H)));
  CK(dalloc(ctx, &ctx->mg.out, (2 * H + 2) + RAU_STATS_NCOUNTS(H)));
  CK(dalloc(ctx, &ctx->mg.ans, 2 * (H + 2) * B));
  CK(dalloc(ctx, &ctx->mg.pred, 2 * B * ctx->Kp));   // rows at the answer pitch, like the logits
  CK(dalloc(ctx, &ctx->mg.att, 2 * B * ctx->Sp));
  CK(dalloc(ctx, &ctx->mg.score, 2 * (H + 2) * B + 2 * (H + 2)));
#undef CK
  ctx->mg.ready = true;
  return RAU_OK;
}
}  // namespace

// scratch of the attention-supervision statistics (att_sup.hip): rows [2][H*cap] | results [2][H], float and int32
int att_stats_alloc(rau_ctx* ctx) {
  const size_t n = 2 * (size_t)ctx->cfg.H * ctx->cap + 2 * (size_t)ctx->cfg.H;
  if (!ctx->att_sf)
    if (int rc = dalloc(ctx, &ctx->att_sf, n)) return rc;
  if (!ctx->att_si)
    if (int rc = dalloc(ctx, &ctx->att_si, n)) return rc;
  return RAU_OK;
}

// may the hop outputs of the last forward be read?  (checked before anything is launched)
int merge_state(rau_ctx* ctx, const char* fn, bool need_labels) {
  if (!ctx->mg.valid)
    return fail(RAU_ERR_STATE, "%s: no step-level forward result (none has run yet, it failed, or a module-level "
                "entry point has run since)", fn);
  if (ctx->slot_serial[ctx->mg.slot] != ctx->mg.serial)
    return fail(RAU_ERR_STATE, "%s: batch slot %d, which the last forward read, has been uploaded into since", fn,
                ctx->mg.slot);
  if (need_labels && !ctx->mg.truth.present())
    return fail(RAU_ERR_STATE, "%s: the batch of the last forward had no labels", fn);
  return RAU_OK;
}

extern "C" {

int rau_step_stats(rau_ctx* ctx, float* loss, float* loss_do_pred, int32_t* counts) {
  NEED(ctx, "null ctx");
  if (int rc = merge_state(ctx, "rau_step_stats", true)) return rc;
  if (int rc = merge_alloc(ctx)) return rc;
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B, K = c.K, NL = 2 * H + 2, NC = RAU_STATS_NCOUNTS(H);
  RUN("step_stats", 0, (double)B * (2 * H + 2) * K * 4,
      step_stats(ctx->st, H, B, K, ctx->logits, ctx->dopred, ctx->argmax_d, ctx->lossrow, ctx->mg.truth, ctx->mg.rowf,
                 ctx->mg.rowi, ctx->mg.out, ctx->mg.score, ctx->mg.score + (size_t)2 * (H + 2) * ctx->cap, ctx->Kp));
  std::vector<float> out((size_t)NL + NC);
  if (int rc = d2h(ctx, out.data(), ctx->mg.out, out.size() * 4)) return rc;
  if (loss) std::memcpy(loss, out.data(), (size_t)(H + 2) * 4);
  if (loss_do_pred) std::memcpy(loss_do_pred, out.data() + H + 2, (size_t)H * 4);
  if (counts) std::memcpy(counts, out.data() + NL, (size_t)NC * 4);
  return RAU_OK;
}

// Attention-supervision statistics of the last forward against its batch's target maps (include/rau.h)
int rau_att_stats(rau_ctx* ctx, float* loss, float* mass, int32_t* hits, int32_t* n_sup) {
  NEED(ctx, "null ctx");
  if (int rc = merge_state(ctx, "rau_att_stats", false)) return rc;
  const BatchSlot& bs = ctx->slot[ctx->mg.slot];
  if (!bs.held.att_targets)
    return fail(RAU_ERR_STATE, "rau_att_stats: the batch of the last forward has no attention targets "
                "(rau_set_att_targets)");
  if (int rc = att_stats_alloc(ctx)) return rc;
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B, S = ctx->Sp;
  float* outf = ctx->att_sf + 2 * (size_t)H * ctx->cap;
  int32_t* outi = ctx->att_si + 2 * (size_t)H * ctx->cap;
  RUN("att_sup_stats", 0, (double)H * B * S * 8,
      att_sup_stats(ctx->st, H, B, c.S, ctx->a, S, bs.att_t_d, S, bs.held.regions ? bs.nreg_d : nullptr, ctx->att_sf,
                    ctx->att_si, outf, outi, ctx->mg.truth.sw));
  std::vector<float> of(2 * (size_t)H);
  std::vector<int32_t> oi(2 * (size_t)H);
  HIPC(hipMemcpyAsync(of.data(), outf, of.size() * 4, hipMemcpyDeviceToHost, ctx->st));
  if (int rc = d2h(ctx, oi.data(), outi, oi.size() * 4)) return rc;
  if (loss) std::memcpy(loss, of.data(), (size_t)H * 4);
  if (mass) std::memcpy(mass, of.data() + H, (size_t)H * 4);
  if (hits) std::memcpy(hits, oi.data(), (size_t)H * 4);
  if (n_sup) *n_sup = oi[H];
  return RAU_OK;
}

// Metric scores of the answers (include/rau.h): rows [2(H+2)][cap] of mg.score, then 2(H+2) totals
int rau_step_scores(rau_ctx* ctx, float* per_sample, float* total) {
  NEED(ctx, "null ctx");
  if (int rc = merge_state(ctx, "rau_step_scores", true)) return rc;
  if (ctx->mg.truth.G <= 0)
    return fail(RAU_ERR_STATE, "rau_step_scores: the batch of the last forward had no answer set (rau_set_answers)");
  if (int rc = merge_alloc(ctx)) return rc;
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B, K = c.K;
  float* tot_d = ctx->mg.score + (size_t)2 * (H + 2) * ctx->cap;
  RUN("step_stats", 0, (double)B * (2 * H + 2) * K * 4,
      step_stats(ctx->st, H, B, K, ctx->logits, ctx->dopred, ctx->argmax_d, ctx->lossrow, ctx->mg.truth, ctx->mg.rowf,
                 ctx->mg.rowi, ctx->mg.out, ctx->mg.score, tot_d, ctx->Kp));
  if (per_sample)
    HIPC(hipMemcpyAsync(per_sample, ctx->mg.score, (size_t)(H + 2) * B * 4, hipMemcpyDeviceToHost, ctx->st));
  if (total) HIPC(hipMemcpyAsync(total, tot_d, (size_t)(H + 2) * 4, hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}

int rau_predict_scores(rau_ctx* ctx, float* oe, float* mc, float* totals) {
  NEED(ctx, "null ctx");
  if (int rc = merge_state(ctx, "rau_predict_scores", false)) return rc;
  if (ctx->mg.truth.G <= 0)
    return fail(RAU_ERR_STATE, "rau_predict_scores: the batch of the last forward had no answer set (rau_set_answers)");
  if (!ctx->mg.merged || ctx->mg.pred_fwd != ctx->mg.fwd)
    return fail(RAU_ERR_STATE, "rau_predict_scores: no rau_predict has run on the last forward");
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B, R = H + 2;
  const int rows = ctx->mg.pred_mc ? 2 * R : R;   // mg.ans = oe [R][B] | mc [R][B]
  float* tot_d = ctx->mg.score + (size_t)2 * R * ctx->cap;
  RUN("answer_scores", 0, (double)rows * B * 8,
      answer_scores(ctx->st, rows, B, c.K, ctx->mg.ans, ctx->mg.truth, ctx->mg.score, tot_d));
  if (oe) HIPC(hipMemcpyAsync(oe, ctx->mg.score, (size_t)R * B * 4, hipMemcpyDeviceToHost, ctx->st));
  if (mc && ctx->mg.pred_mc)
    HIPC(hipMemcpyAsync(mc, ctx->mg.score + (size_t)R * B, (size_t)R * B * 4, hipMemcpyDeviceToHost, ctx->st));
  if (totals) {
    HIPC(hipMemcpyAsync(totals, tot_d, (size_t)R * 4, hipMemcpyDeviceToHost, ctx->st));
    if (ctx->mg.pred_mc)
      HIPC(hipMemcpyAsync(totals + R, tot_d + R, (size_t)R * 4, hipMemcpyDeviceToHost, ctx->st));
  }
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}

int rau_predict(rau_ctx* ctx, const int32_t* mc_ans, int32_t n_mc, int32_t* oe, int32_t* mc) {
  NEED(ctx, "null ctx");
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B, K = c.K;
  const size_t nmc = mc_ans ? (size_t)B * n_mc : 0;
  if (mc_ans) {
    NEED(n_mc > 0, "rau_predict: n_mc=%d must be positive with an MC list", n_mc);
    NEED(predict_rows_lds(K) <= 65536, "rau_predict: K=%d too large for the MC candidate mask", K);
    for (size_t i = 0; i < nmc; ++i)
      NEED(mc_ans[i] >= 0 && mc_ans[i] <= K, "rau_predict: mc_ans[%zu]=%d out of [0,%d] (0 = empty slot)", i,
           mc_ans[i], K);
  }
  if (int rc = merge_state(ctx, "rau_predict", false)) return rc;
  if (int rc = merge_alloc(ctx)) return rc;
  if (nmc > ctx->mg.mc_cap) {   // grows only; the old buffer stays with the ctx until rau_destroy
    if (int rc = dalloc(ctx, &ctx->mg.mc, nmc)) return rc;
    ctx->mg.mc_cap = nmc;
  }
  if (nmc) HIPC(hipMemcpyAsync(ctx->mg.mc, mc_ans, nmc * 4, hipMemcpyHostToDevice, ctx->st));
  int32_t* oe_d = ctx->mg.ans;
  int32_t* mc_d = ctx->mg.ans + (size_t)(H + 2) * B;
  RUN("predict_rows", 0, (double)B * (2 * H + 1) * K * 4,
      predict_rows(ctx->st, H, B, K, ctx->Sp, ctx->logits, ctx->dopred, ctx->a, nmc ? ctx->mg.mc : nullptr,
                   n_mc, oe_d, mc_d, ctx->mg.pred, ctx->mg.att, ctx->Kp));
  ctx->mg.merged = false;
  if (oe)
    if (int rc = d2h(ctx, oe, oe_d, (size_t)(H + 2) * B * 4)) return rc;
  if (mc && nmc)
    if (int rc = d2h(ctx, mc, mc_d, (size_t)(H + 2) * B * 4)) return rc;
  HIPC(hipStreamSynchronize(ctx->st));   // the caller's mc_ans is free on return
  if (int rc = persist_check(ctx)) return rc;
  ctx->mg.merged = true;
  ctx->mg.pred_fwd = ctx->mg.fwd;
  ctx->mg.pred_mc = nmc != 0;
  return RAU_OK;
}

int rau_topk(rau_ctx* ctx, int32_t k, int32_t* ids, float* score, float* conf) {
  NEED(ctx, "null ctx");
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B, K = c.K;
  NEED(k >= 1 && k <= K, "rau_topk: k=%d out of [1,%d] (the K of rau_create)", k, K);
  if (int rc = merge_state(ctx, "rau_topk", false)) return rc;
  if (k > ctx->mg.topk_k) {   // sized for the capacity; the smaller one goes once the larger one is there
    uint32_t* fresh = nullptr;
    if (int rc = dalloc(ctx, &fresh, (size_t)3 * (H + 2) * ctx->cap * k)) {
      (void)hipGetLastError();   // the context stays as it was: nothing later may trip over this error
      return rc;
    }
    if (ctx->mg.topk)
      if (int rc = dfree(ctx, ctx->mg.topk)) return rc;
    ctx->mg.topk = fresh;
    ctx->mg.topk_k = k;
  }
  const size_t n = (size_t)(H + 2) * B * k;
  int32_t* ids_d = static_cast<int32_t*>(ctx->mg.topk);
  float* score_d = reinterpret_cast<float*>(ids_d + n);
  float* conf_d = score_d + n;
  RUN("topk_merged", 0, (double)B * (2 * H + 1) * K * 4,
      topk_merged(ctx->st, H, B, K, k, ctx->logits, ctx->dopred, ids_d, score_d, conf_d, ctx->Kp));
  if (ids) HIPC(hipMemcpyAsync(ids, ids_d, n * 4, hipMemcpyDeviceToHost, ctx->st));
  if (score) HIPC(hipMemcpyAsync(score, score_d, n * 4, hipMemcpyDeviceToHost, ctx->st));
  if (conf) HIPC(hipMemcpyAsync(conf, conf_d, n * 4, hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}

// ---- multiple-choice candidates against the merged rows (cand_rank.hip).  mg.cand, one block: the ranked lists'
// staging | the statistics' float rows | their int32 rows | their results
namespace {
struct CandBufs {
  int32_t* ids; float* score; float* conf;   // [H+2][cap][kMaxCandidates] each (dense in the call's n and k)
  float* rows; int32_t* rowi; float* out;
};
int cand_bufs(rau_ctx* ctx, CandBufs* cb) {
  const size_t R = (size_t)ctx->cfg.H + 2, cap = ctx->cap, list = R * cap * kMaxCandidates;
  if (!ctx->mg.cand)
    if (int rc = dalloc(ctx, &ctx->mg.cand, 3 * list + (R + 2) * cap + (R + 1) * cap + 3 * R + 1)) return rc;
  uint32_t* p = ctx->mg.cand;
  cb->ids = reinterpret_cast<int32_t*>(p);
  cb->score = reinterpret_cast<float*>(p + list);
  cb->conf = reinterpret_cast<float*>(p + 2 * list);
  cb->rows = reinterpret_cast<float*>(p + 3 * list);
  cb->rowi = reinterpret_cast<int32_t*>(p + 3 * list + (R + 2) * cap);
  cb->out = reinterpret_cast<float*>(p + 3 * list + (R + 2) * cap + (R + 1) * cap);
  return RAU_OK;
}
}  // namespace

int rau_cand_stats(rau_ctx* ctx, float* loss, int32_t* correct, float* score, int32_t* n_lab) {
  NEED(ctx, "null ctx");
  if (int rc = merge_state(ctx, "rau_cand_stats", true)) return rc;
  if (ctx->mg.truth.C <= 0)
    return fail(RAU_ERR_STATE, "rau_cand_stats: the batch of the last forward had no candidates (rau_set_candidates)");
  CandBufs cb;
  if (int rc = cand_bufs(ctx, &cb)) return rc;
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B, R = H + 2;
  RUN("cand_stats", 0, (double)R * B * ctx->mg.truth.C * 8,
      cand_stats(ctx->st, H, B, c.K, ctx->logits, ctx->dopred, ctx->lossrow, ctx->mg.truth, cb.rows, cb.rowi, cb.out,
                 ctx->Kp));
  std::vector<uint32_t> out((size_t)3 * R + 1);
  if (int rc = d2h(ctx, out.data(), cb.out, out.size() * 4)) return rc;
  if (loss) std::memcpy(loss, out.data(), (size_t)R * 4);
  if (score) std::memcpy(score, out.data() + R, (size_t)R * 4);
  if (correct) std::memcpy(correct, out.data() + 2 * R, (size_t)R * 4);
  if (n_lab) std::memcpy(n_lab, out.data() + 3 * R, 4);
  return RAU_OK;
}

int rau_topk_cand(rau_ctx* ctx, int32_t k, int32_t* ids, float* score, float* conf) {
  NEED(ctx, "null ctx");
  if (int rc = merge_state(ctx, "rau_topk_cand", false)) return rc;
  const int C = ctx->mg.truth.C;
  if (C <= 0)
    return fail(RAU_ERR_STATE, "rau_topk_cand: the batch of the last forward had no candidates (rau_set_candidates)");
  NEED(k >= 1 && k <= C, "rau_topk_cand: k=%d out of [1,%d] (the C of rau_set_candidates)", k, C);
  CandBufs cb;
  if (int rc = cand_bufs(ctx, &cb)) return rc;
  const rau_config& c = ctx->cfg;
  const int H = c.H, B = c.B;
  const size_t n = (size_t)(H + 2) * B * k;
  RUN("cand_topk", 0, (double)(H + 2) * B * C * 8,
      cand_topk(ctx->st, H, B, c.K, k, ctx->logits, ctx->dopred, ctx->mg.truth.cand, C, cb.ids, cb.score, cb.conf,
                ctx->Kp));
  if (ids) HIPC(hipMemcpyAsync(ids, cb.ids, n * 4, hipMemcpyDeviceToHost, ctx->st));
  if (score) HIPC(hipMemcpyAsync(score, cb.score, n * 4, hipMemcpyDeviceToHost, ctx->st));
  if (conf) HIPC(hipMemcpyAsync(conf, cb.conf, n * 4, hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return persist_check(ctx);
}

int rau_get_merged(rau_ctx* ctx, float* pred, float* att) {
  NEED(ctx, "null ctx");
  if (!ctx->mg.merged) return fail(RAU_ERR_STATE, "rau_get_merged: no rau_predict has run");
  const rau_config& c = ctx->cfg;
  if (pred) {
    if (ctx->Kp == c.K) {
      if (int rc = d2h(ctx, pred, ctx->mg.pred, (size_t)2 * c.B * c.K * 4)) return rc;
    } else {   // dense [2,n,K] on the host, rows at the answer pitch on the device
      HIPC(hipMemcpy2DAsync(pred, (size_t)c.K * 4, ctx->mg.pred, (size_t)ctx->Kp * 4, (size_t)c.K * 4, (size_t)2 * c.B,
                            hipMemcpyDeviceToHost, ctx->st));
      HIPC(hipStreamSynchronize(ctx->st));
      if (int rc = persist_check(ctx)) return rc;
    }
  }
  if (att) {
    HIPC(hipMemcpy2DAsync(att, (size_t)c.S * 4, ctx->mg.att, (size_t)ctx->Sp * 4, (size_t)c.S * 4,
                          (size_t)2 * c.B, hipMemcpyDeviceToHost, ctx->st));
    HIPC(hipStreamSynchronize(ctx->st));
  }
  return RAU_OK;
}

}  // extern "C"

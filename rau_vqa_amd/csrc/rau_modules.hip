// rau_modules.hip -- module-level entry points of include/rau.h: one call per
// nn.Module :forward / :backward of the reference's clones, so that the loops of
// feval (experiments/Ours_SS/LstmAttCtrlGradNoiseDontSelect.lua:443-596) can run
// unchanged above the C ABI:
//   embed_clones[t]   word_embed   SS:203-206   -> rau_embed_forward / _backward
//   lstm_clones[t]    DeepLSTM     SS:213       -> rau_deeplstm_forward / _backward
//   multimodal_clones[h]           SS:292-307   -> rau_multimodal_forward / _backward
//   criteria[h]       CrossEntropyCriterion SS:310 -> rau_criterion_forward / _backward
// Same kernels as the step-level path (rau_forward / rau_backward), but executed at the
// reference's granularity on the ctx stream alone: nothing is hoisted across clones, every
// weight gradient is accumulated by the clone's own :backward (accGradParameters).  The
// step-level path is the fast one; this one exists for drop-in compatibility and as a
// second, independently scheduled route to the same numbers (tests/test_gpu_modules.py).
// Everything runs on the chain stream, and every step-level call joins all three streams before it returns,
// so the bulk and side streams are idle here: that is why this file may borrow THEIR scratch (ws_side.slab /
// .coltmp for the per-clone Linear weight gradients and column sums, ws_bulk.slab for the conv weight
// gradients) while the chain stream's own slab holds the hop's partials.
#include "rau_ctx.h"

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int mod_alloc(rau_ctx* ctx) {
  ctx->mg.valid = false;   // every module-level entry point comes here: the step-level hop outputs are stale
  if (ctx->mod_ready) return 0;
  // Callers hand in / get back DENSE [.., S] tensors.  Internally every [.., S] tensor uses the
  // position pitch Sp (S rounded up to a multiple of 4: 7x7 maps 49 -> 52), so when Sp != S the
  // feature map / d_attprob are re-pitched on the way in and attprob / d_X on the way out.
  const rau_config& c = ctx->cfg;
  const size_t B = ctx->cap, Q = ctx->Q;   // sized for the capacity; contents dense in the current batch size
  const size_t wide = std::max<size_t>({(size_t)c.Rq, (size_t)c.R, (size_t)c.M});
#define CK(x) do { if (int rc_ = (x)) return rc_; } while (0)
  CK(dalloc(ctx, &ctx->m_state, (size_t)c.T * B * Q));
  CK(dalloc(ctx, &ctx->m_dstate, (size_t)c.T * B * Q));
  for (int i = 0; i < 4; ++i) CK(dalloc(ctx, &ctx->m_tmp[i], B * wide));
  CK(dalloc(ctx, &ctx->m_dq, (size_t)c.H * B * Q));
  CK(dalloc(ctx, &ctx->m_dc, (size_t)c.H * B * c.R));
  CK(dalloc(ctx, &ctx->m_dh, (size_t)c.H * B * c.R));
  CK(dalloc(ctx, &ctx->m_add, B * c.M));
  CK(dalloc(ctx, &ctx->m_s, B));
  CK(dalloc(ctx, &ctx->m_zero, B * std::max<size_t>(Q, (size_t)c.R)));
  CK(dalloc(ctx, &ctx->m_loss, (size_t)c.H));
  if (ctx->Sp != c.S) {
    CK(dalloc(ctx, &ctx->m_Xp, B * c.D * ctx->Sp));
    CK(dalloc(ctx, &ctx->m_a, (size_t)c.H * B * c.S));
    CK(dalloc(ctx, &ctx->m_da, B * ctx->Sp));
  }
#undef CK
  ctx->mod_ready = true;
  return 0;
}

// strided [B, w] block copy on the ctx stream (packs / unpacks the [c1 h1 c2 h2] state)
int copy2d(rau_ctx* ctx, float* dst, size_t dst_rs, const float* src, size_t src_rs, size_t w) {
  HIPC(hipMemcpy2DAsync(dst, dst_rs * 4, src, src_rs * 4, w * 4, ctx->cfg.B,
                        hipMemcpyDeviceToDevice, ctx->st));
  return 0;
}

// dW += dY^T X and db += column sums of dY for one Linear, rows = one clone's batch
int lin_wgrad(rau_ctx* ctx, Lin& l, const float* dY, const float* X, long ldx, bool bias = true,
              long ldy = 0) {
  const int B = ctx->cfg.B;
  RUN("wgrad_gemm", 2.0 * l.out * l.in * B, 0,
      gemm_tn_acc(ctx->st, l.out, l.in, B, dY, ldy ? ldy : l.out, X, ldx, l.dW, l.in, ctx->ws_side.slab,
                  bias ? l.db : nullptr, lin_mode(ctx).bf16));
  return 0;
}
// X = NULL ("the resident batch"): its f32 form at pitch Sp -- the buffer itself, or for a 16-bit or fp8 batch
// its exact widening into ctx-owned scratch (allocated on first use), so that the f32 kernels run on it
int resident_feats(rau_ctx* ctx, const float** X) {
  if (int rc = batch_maps(ctx, X)) return rc;   // a batch with an image table: its per-sample expansion
  if (cur_batch(ctx).held.feat_type == RAU_FEAT_F32) return 0;
  const float* src = *X;
  const rau_config& c = ctx->cfg;
  if (!ctx->m_Xw)
    if (int rc = dalloc(ctx, &ctx->m_Xw, (size_t)ctx->cap * c.D * ctx->Sp)) return rc;
  RUN("widen_features", 0, (double)c.B * c.D * ctx->Sp * (4 + feat_elem_bytes(cur_batch(ctx).held.feat_type)),
      widen_features(ctx->st, (size_t)c.B * c.D, c.S, ctx->Sp, src, ctx->m_Xw, cur_batch(ctx).held.feat_type));
  *X = ctx->m_Xw;
  return 0;
}
// [rows][w_src] -> [rows][w_dst] on the ctx stream (re-pitching of [.., S] tensors)
int repitch(rau_ctx* ctx, float* dst, size_t w_dst, const float* src, size_t w_src, size_t rows) {
  const size_t w = std::min(w_dst, w_src);
  HIPC(hipMemcpy2DAsync(dst, w_dst * 4, src, w_src * 4, w * 4, rows, hipMemcpyDeviceToDevice,
                        ctx->st));
  return 0;
}

}  // namespace

// Philox masks for the current (seed, step) if the caller has not uploaded explicit ones;
// module-level forwards of one step all see the same mask tensors, each its own slice.
static int ensure_masks(rau_ctx* ctx) {
  if (ctx->mode != RAU_MODE_TRAIN) return 0;
  if (ctx->mod_masks_seed == ctx->seed && ctx->mod_masks_step == ctx->step && ctx->mod_masks_valid)
    return 0;
  for (int i = 0; i < 5; ++i)
    if (!ctx->mexplicit[i] && ctx->mp[i] > 0.f)
      RUN("fill_masks", 0, ctx->mcount[i] / 8.0,
          fill_masks(ctx->st, ctx->seed, (uint32_t)i, ctx->step, ctx->mp[i], ctx->mcount[i],
                     ctx->mbits[i], ctx->dkey));
  ctx->mod_masks_seed = ctx->seed;
  ctx->mod_masks_step = ctx->step;
  ctx->mod_masks_valid = true;
  return 0;
}

extern "C" {

// ------------------------------------------------------------ word_embed clone t
int rau_embed_forward(rau_ctx* ctx, int t, const int32_t* tokens_dev, float** we) {
  NEED(ctx && we, "null argument");
  const rau_config& c = ctx->cfg;
  NEED(t >= 0 && t < c.T, "rau_embed_forward: t=%d out of [0,%d)", t, c.T);
  if (int rc = mod_alloc(ctx)) return rc;
  if (int rc = ensure_masks(ctx)) return rc;
  if (!tokens_dev) {
    if (!cur_batch(ctx).held.have) return fail(RAU_ERR_STATE, "rau_embed_forward: no tokens and no batch");
    tokens_dev = cur_batch(ctx).tokens + (size_t)t * c.B;
  }
  const Masks m = masks_of(ctx);
  float* out = ctx->we + (size_t)t * c.B * c.E;
  RUN("embed_fwd", 0, c.B * c.E * 8.0,
      embed_fwd(ctx->st, c.B, c.E, c.V, ctx->grp[RAU_GROUP_EMBED].w, tokens_dev, m.we, m.s_we, out,
                (size_t)t * c.B * c.E));
  *we = out;
  return RAU_OK;
}

int rau_embed_backward(rau_ctx* ctx, int t, const int32_t* tokens_dev, const float* d_we) {
  NEED(ctx && d_we, "null argument");
  const rau_config& c = ctx->cfg;
  NEED(t >= 0 && t < c.T, "rau_embed_backward: t=%d out of [0,%d)", t, c.T);
  if (int rc = mod_alloc(ctx)) return rc;
  if (!tokens_dev) {
    if (!cur_batch(ctx).held.have) return fail(RAU_ERR_STATE, "rau_embed_backward: no tokens and no batch");
    tokens_dev = cur_batch(ctx).tokens + (size_t)t * c.B;
  }
  const Masks m = masks_of(ctx);
  RUN("embed_bwd", 0, c.B * c.E * 12.0,
      embed_bwd_rows(ctx->st, c.B, c.E, c.V, tokens_dev, d_we, ctx->we + (size_t)t * c.B * c.E, m.we,
                     (size_t)t * c.B * c.E, m.s_we, ctx->grp[RAU_GROUP_EMBED].g));
  return RAU_OK;
}

// ------------------------------------------------------------ DeepLSTM clone t
int rau_deeplstm_forward(rau_ctx* ctx, int t, const float* x, const float* state,
                         float** state_out) {
  NEED(ctx && x && state_out, "null argument");
  const rau_config& c = ctx->cfg;
  NEED(t >= 0 && t < c.T, "rau_deeplstm_forward: t=%d out of [0,%d)", t, c.T);
  NEED(aligned16(x) && aligned16(state), "rau_deeplstm_forward: pointers must be 16-byte aligned");
  if (int rc = mod_alloc(ctx)) return rc;
  if (int rc = ensure_masks(ctx)) return rc;
  const int B = c.B, E = c.E, Rq = c.Rq, Q = ctx->Q;
  hipStream_t st = ctx->st;
  const Masks m = masks_of(ctx);
  if (!state) state = ctx->m_zero;   // init_state zeros, SS:358
  const size_t BRq = (size_t)B * Rq, G4 = (size_t)B * 4 * Rq;
  float* out = ctx->m_state + (size_t)t * B * Q;
  float* G1 = ctx->G1 + (size_t)t * G4;
  float* G2 = ctx->G2 + (size_t)t * G4;
  float* x2 = ctx->x2 + (size_t)t * BRq;
  {  // layer 1: i2h(x) + h2h(prev_h), DeepLSTM.lua:42-44
    LinOpts o = lin_opts(ctx, ctx->ws_chain);
    o.bias = ctx->i2h[0].b;
    o.bias2 = ctx->h2h[0].b;
    RUN("enc_i2h_gemm", gflop(B, 4 * Rq, E), 0, gemm_nt(st, B, 4 * Rq, E, x, E, ctx->i2h[0].W, E, G1, 4 * Rq, o));
    LinOpts oa = lin_opts(ctx, ctx->ws_chain);
    oa.accumulate = 1;
    RUN("enc_h2h_gemm", gflop(B, 4 * Rq, Rq), 0,
        gemm_nt(st, B, 4 * Rq, Rq, state + Rq, Q, ctx->h2h[0].W, Rq, G1, 4 * Rq, oa));
    RUN("lstm_fwd", 0, BRq * 40.0,
        lstm_fwd(st, GATES_DEEP, B, Rq, G1, state, Q, out, Q, out + Rq, Q,
                 ctx->tc1 + (size_t)t * BRq, x2, m.rnn, (size_t)t * BRq, m.s_rnn));
  }
  {  // layer 2 on dropout(h1), DeepLSTM.lua:39
    LinOpts o = lin_opts(ctx, ctx->ws_chain);
    o.bias = ctx->i2h[1].b;
    o.bias2 = ctx->h2h[1].b;
    RUN("enc_h2h_gemm", gflop(B, 4 * Rq, Rq), 0, gemm_nt(st, B, 4 * Rq, Rq, x2, Rq, ctx->i2h[1].W, Rq, G2, 4 * Rq, o));
    LinOpts oa = lin_opts(ctx, ctx->ws_chain);
    oa.accumulate = 1;
    RUN("enc_h2h_gemm", gflop(B, 4 * Rq, Rq), 0,
        gemm_nt(st, B, 4 * Rq, Rq, state + 3 * Rq, Q, ctx->h2h[1].W, Rq, G2, 4 * Rq, oa));
    RUN("lstm_fwd", 0, BRq * 40.0,
        lstm_fwd(st, GATES_DEEP, B, Rq, G2, state + 2 * Rq, Q, out + 2 * Rq, Q, out + 3 * Rq, Q,
                 ctx->tc2 + (size_t)t * BRq, nullptr, nullptr, 0, 1.f));
  }
  *state_out = out;
  return RAU_OK;
}

int rau_deeplstm_backward(rau_ctx* ctx, int t, const float* x, const float* state,
                          const float* d_state_out, float** d_x, float** d_state) {
  NEED(ctx && x && d_state_out && d_x && d_state, "null argument");
  const rau_config& c = ctx->cfg;
  NEED(t >= 0 && t < c.T, "rau_deeplstm_backward: t=%d out of [0,%d)", t, c.T);
  NEED(aligned16(x) && aligned16(state) && aligned16(d_state_out),
       "rau_deeplstm_backward: pointers must be 16-byte aligned");
  if (int rc = mod_alloc(ctx)) return rc;
  const int B = c.B, E = c.E, Rq = c.Rq, Q = ctx->Q;
  hipStream_t st = ctx->st;
  const Masks m = masks_of(ctx);
  if (!state) state = ctx->m_zero;
  const size_t BRq = (size_t)B * Rq, G4 = (size_t)B * 4 * Rq;
  float* dst = ctx->m_dstate + (size_t)t * B * Q;
  float* dG1 = ctx->dG1 + (size_t)t * G4;
  float* dG2 = ctx->dG2 + (size_t)t * G4;
  float* dxo = ctx->dwe + (size_t)t * B * E;
  float *dc_in = ctx->m_tmp[0], *dc_prev = ctx->m_tmp[1], *dx2 = ctx->m_tmp[2];
  // ---- layer 2
  if (int rc = copy2d(ctx, dc_in, Rq, d_state_out + 2 * Rq, Q, Rq)) return rc;
  RUN("lstm_bwd", 0, BRq * 48.0,
      lstm_bwd(st, GATES_DEEP, B, Rq, ctx->G2 + (size_t)t * G4, state + 2 * Rq, Q,
               ctx->tc2 + (size_t)t * BRq, d_state_out + 3 * Rq, Q, nullptr, dc_in, dG2, dc_prev,
               nullptr, 0, nullptr, nullptr, 0));
  if (int rc = copy2d(ctx, dst + 2 * Rq, Q, dc_prev, Rq, Rq)) return rc;
  {
    LinOpts o = lin_opts(ctx, ctx->ws_chain);   // grad at prev_h of layer 2
    RUN("enc_h2h_dgrad", gflop(B, Rq, 4 * Rq), 0,
        gemm_nn(st, B, Rq, 4 * Rq, dG2, 4 * Rq, ctx->h2h[1].W, Rq, dst + 3 * Rq, Q, o));
    LinOpts o2 = lin_opts(ctx, ctx->ws_chain);  // grad at layer-2 input, back through the inter-layer dropout
    o2.emask = m.rnn;
    o2.emask_e0 = (size_t)t * BRq;
    o2.emscale = m.s_rnn;
    RUN("enc_h2h_dgrad", gflop(B, Rq, 4 * Rq), 0,
        gemm_nn(st, B, Rq, 4 * Rq, dG2, 4 * Rq, ctx->i2h[1].W, Rq, dx2, Rq, o2));
  }
  // ---- layer 1: next_h of layer 1 fans out to the output state and to layer 2
  if (int rc = copy2d(ctx, dc_in, Rq, d_state_out, Q, Rq)) return rc;
  RUN("lstm_bwd", 0, BRq * 48.0,
      lstm_bwd(st, GATES_DEEP, B, Rq, ctx->G1 + (size_t)t * G4, state, Q,
               ctx->tc1 + (size_t)t * BRq, d_state_out + Rq, Q, dx2, dc_in, dG1, dc_prev, nullptr,
               0, nullptr, nullptr, 0));
  if (int rc = copy2d(ctx, dst, Q, dc_prev, Rq, Rq)) return rc;
  {
    LinOpts o = lin_opts(ctx, ctx->ws_chain);
    RUN("enc_h2h_dgrad", gflop(B, Rq, 4 * Rq), 0,
        gemm_nn(st, B, Rq, 4 * Rq, dG1, 4 * Rq, ctx->h2h[0].W, Rq, dst + Rq, Q, o));
    LinOpts o2 = lin_opts(ctx, ctx->ws_chain);
    RUN("enc_i2h_dgrad", gflop(B, E, 4 * Rq), 0,
        gemm_nn(st, B, E, 4 * Rq, dG1, 4 * Rq, ctx->i2h[0].W, E, dxo, E, o2));
  }
  // ---- accGradParameters
  if (int rc = lin_wgrad(ctx, ctx->i2h[0], dG1, x, E)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->h2h[0], dG1, state + Rq, Q)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->i2h[1], dG2, ctx->x2 + (size_t)t * BRq, Rq)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->h2h[1], dG2, state + 3 * Rq, Q)) return rc;
  *d_x = dxo;
  *d_state = dst;
  return RAU_OK;
}

// ------------------------------------------------------------ multimodal clone h
int rau_multimodal_forward(rau_ctx* ctx, int h, const float* q, const float* X, const float* c_prev,
                           const float* h_prev, float** logits, float** do_pred, float** attprob,
                           float** c_out, float** h_out) {
  return rau_multimodal_forward_regions(ctx, h, q, X, c_prev, h_prev, nullptr, logits, do_pred, attprob, c_out, h_out);
}

// regions_dev: [B] device region counts (the attention kernel clamps them into [1, S]); NULL = every position
int rau_multimodal_forward_regions(rau_ctx* ctx, int h, const float* q, const float* X, const float* c_prev,
                                   const float* h_prev, const int32_t* regions_dev, float** logits,
                                   float** do_pred, float** attprob, float** c_out, float** h_out) {
  return rau_multimodal_forward_bias(ctx, h, q, X, c_prev, h_prev, regions_dev, nullptr, logits, do_pred, attprob,
                                     c_out, h_out);
}

// bias_dev: [B,S] dense f32 device rows added to the attention scores (AttPartials::zadd; one launch re-pitches them
// into m_zadd); NULL = none, which is rau_multimodal_forward_regions launch for launch
int rau_multimodal_forward_bias(rau_ctx* ctx, int h, const float* q, const float* X, const float* c_prev,
                                const float* h_prev, const int32_t* regions_dev, const float* bias_dev,
                                float** logits, float** do_pred, float** attprob, float** c_out, float** h_out) {
  NEED(ctx && q, "null argument");
  NEED(aligned16(bias_dev), "rau_multimodal_forward_bias: bias_dev must be 16-byte aligned");
  NEED_DENSE_K(ctx, "rau_multimodal_forward");
  const rau_config& c = ctx->cfg;
  NEED(h >= 0 && h < c.H, "rau_multimodal_forward: h=%d out of [0,%d)", h, c.H);
  if (int rc = mod_alloc(ctx)) return rc;
  if (int rc = ensure_masks(ctx)) return rc;
  const bool resident = !X;   // the batch's own map, already at pitch Sp
  if (!X) {
    if (!cur_batch(ctx).held.have) return fail(RAU_ERR_STATE, "rau_multimodal_forward: no X and no batch");
    if (int rc = resident_feats(ctx, &X)) return rc;
  }
  if (!c_prev) c_prev = ctx->m_zero;   // att_c / att_h zeros, SS:362-365
  if (!h_prev) h_prev = ctx->m_zero;
  NEED(aligned16(q) && aligned16(X) && aligned16(c_prev) && aligned16(h_prev),
       "rau_multimodal_forward: pointers must be 16-byte aligned");
  const int B = c.B, D = c.D, S = ctx->Sp, SL = c.S, M = c.M, A = c.A, R = c.R, K = c.K, Q = ctx->Q;
  hipStream_t st = ctx->st;
  const Masks m = masks_of(ctx);
  const size_t BM_ = (size_t)B * M, BR_ = (size_t)B * R;
  ctx->fwd.I_shared = false;
  drop_forward(ctx);   // the step-level slots are being overwritten
  if (S != SL && !resident) {   // dense [B,D,SL] from the caller -> pitched (pad columns stay 0)
    if (int rc = repitch(ctx, ctx->m_Xp, S, X, SL, (size_t)B * D)) return rc;
    X = ctx->m_Xp;
  }
  // q_embed's input half: dropout(q) Wq^T + bq + bh   (SS:233-235)
  float* qd = ctx->qd + (size_t)h * B * Q;
  RUN("apply_mask", 0, (double)B * Q * 8,
      apply_mask(st, (size_t)B * Q, (size_t)B * Q, q, m.q, m.s_q, qd, (size_t)h * B * Q));
  ctx->fwd.yq_shared = false;   // this path fills the hop's own rows
  {
    LinOpts o = lin_opts(ctx, ctx->ws_chain);
    o.bias = ctx->q_proj.b;
    o.bias2 = ctx->h_proj.b;
    RUN("q_proj_gemm", gflop(B, M, Q), 0,
        gemm_nt(st, B, M, Q, qd, Q, ctx->q_proj.W, Q, ctx->Yq + (size_t)h * BM_, M, o));
  }
  // i_embed (SS:238-242) and attbycontent's ifeatproj (SS:247-249) for this clone
  const float* xin = X;
  if (m.x) {
    float* xd = ctx->xd + (size_t)h * B * D * S;
    RUN("dropout_features", 0, 2.0 * B * D * S * 4,
        dropout_features(st, 1, (size_t)B * D * S, X, m.x, m.s_x, xd,
                         ctx->xdrop == RAU_XDROP_TIED ? 0 : (size_t)h * B * D * SL /* tied: every hop reads the one mask */,
                         SL, S));
    xin = xd;
  }
  RUN("transpose", 0, (double)M * D * 8, transpose2d(st, M, D, ctx->i_embed.W, ctx->WiT));
  RUN("transpose", 0, (double)A * M * 8, transpose2d(st, A, M, ctx->att_i.W, ctx->WpT));
  float* Ih = ctx->I + (size_t)h * BM_ * S;
  float* Th = ctx->T + (size_t)h * B * A * S;
  if (int rc = image_forward(ctx, st, B, xin, false, Ih, Th)) return rc;
  float* co = ctx->cc + (size_t)(h + 1) * BR_;
  float* ho = ctx->hh + (size_t)(h + 1) * BR_;
  const float* zadd = nullptr;
  if (bias_dev) {
    if (!ctx->m_zadd)
      if (int rc = dalloc(ctx, &ctx->m_zadd, (size_t)ctx->cap * S)) return rc;
    RUN("att_bias_attach", 0, (double)B * SL * 8, att_bias_attach(st, B, SL, S, bias_dev, RAU_FEAT_F32, ctx->m_zadd));
    zadd = ctx->m_zadd;
  }
  if (int rc = hop_forward(ctx, h, c_prev, h_prev, co, ho, Ih, Th, Truth{}, regions_dev, zadd)) return rc;
  if (logits) *logits = ctx->logits + (size_t)h * B * K;
  if (do_pred) *do_pred = ctx->dopred + (size_t)h * B;
  if (attprob) {
    *attprob = ctx->a + (size_t)h * B * S;
    if (S != SL) {   // hand back a dense [B,SL] copy
      float* ad = ctx->m_a + (size_t)h * B * SL;
      if (int rc = repitch(ctx, ad, SL, ctx->a + (size_t)h * B * S, S, B)) return rc;
      *attprob = ad;
    }
  }
  if (c_out) *c_out = co;
  if (h_out) *h_out = ho;
  return RAU_OK;
}

int rau_multimodal_backward(rau_ctx* ctx, int h, const float* q, const float* X,
                            const float* c_prev, const float* h_prev, const float* d_logits,
                            const float* d_do_pred, const float* d_attprob, const float* d_c,
                            const float* d_h, float** d_q, float** d_X, float** d_c_prev,
                            float** d_h_prev) {
  NEED(ctx && q && d_logits, "null argument");
  NEED_DENSE_K(ctx, "rau_multimodal_backward");
  const rau_config& c = ctx->cfg;
  NEED(h >= 0 && h < c.H, "rau_multimodal_backward: h=%d out of [0,%d)", h, c.H);
  if (int rc = mod_alloc(ctx)) return rc;
  const bool resident = !X;
  if (!X) {
    if (!cur_batch(ctx).held.have) return fail(RAU_ERR_STATE, "rau_multimodal_backward: no X and no batch");
    if (int rc = resident_feats(ctx, &X)) return rc;
  }
  if (!c_prev) c_prev = ctx->m_zero;
  if (!h_prev) h_prev = ctx->m_zero;
  NEED(aligned16(q) && aligned16(X) && aligned16(c_prev) && aligned16(h_prev) &&
           aligned16(d_logits) && aligned16(d_attprob) && aligned16(d_c) && aligned16(d_h),
       "rau_multimodal_backward: pointers must be 16-byte aligned");
  const int B = c.B, D = c.D, S = ctx->Sp, SL = c.S, M = c.M, A = c.A, R = c.R, Q = ctx->Q;
  hipStream_t st = ctx->st;
  const Masks m = masks_of(ctx);
  const size_t BM_ = (size_t)B * M, BS_ = (size_t)B * S, BR_ = (size_t)B * R;
  if (S != SL) {
    if (!resident) {   // the forward of this clone re-pitched the same X
      if (int rc = repitch(ctx, ctx->m_Xp, S, X, SL, (size_t)B * D)) return rc;
      X = ctx->m_Xp;
    }
    if (d_attprob) {
      HIPC(hipMemsetAsync(ctx->m_da, 0, BS_ * sizeof(float), st));
      if (int rc = repitch(ctx, ctx->m_da, S, d_attprob, SL, B)) return rc;
      d_attprob = ctx->m_da;
    }
  }
  const float* Ih = ctx->I + (size_t)h * BM_ * S;
  const float* mfh = ctx->mf + (size_t)h * BM_;
  float* Th = ctx->T + (size_t)h * B * A * S;
  float* dZh = ctx->dZ + (size_t)h * BM_ * S;
  const float* xin = m.x ? ctx->xd + (size_t)h * B * D * S : X;

  HopGrad g{};
  g.dl = d_logits;
  g.dc_next = d_c;
  g.dh_next = d_h;
  g.da_out = d_attprob;
  g.dc_out = ctx->m_dc + (size_t)h * BR_;
  g.dh_out = ctx->m_dh + (size_t)h * BR_;
  if (d_do_pred) {
    // out_do_pred = Sigmoid(Linear(merge_feat)) (SS:281-282): s = ddp dp (1-dp);
    // dmf += s (x) wd; dwd += s^T mf; dbd += sum s.   (feval always passes zeros, SS:566)
    RUN("dopred_bwd", 0, 0, sigmoid_bwd(st, B, d_do_pred, ctx->dopred + (size_t)h * B, ctx->m_s));
    RUN("dopred_bwd", 0, 0, row_scale(st, B, M, ctx->m_s, nullptr, ctx->do_pred.W, ctx->m_add));
    g.dmf_add = ctx->m_add;
  }
  if (int rc = hop_backward(ctx, h, c_prev, Ih, g)) return rc;
  if (d_do_pred) {
    // m_add is free again once dpre has been formed: reuse it for s (.) mf rows
    RUN("dopred_bwd", 0, 0, row_scale(st, B, M, ctx->m_s, mfh, nullptr, ctx->m_add));
    RUN("colsum", 0, 0, colsum_acc(st, B, M, ctx->m_add, M, ctx->do_pred.dW, ctx->ws_side.coltmp));
    RUN("colsum", 0, 0, colsum_acc(st, B, 1, ctx->m_s, 1, ctx->do_pred.db, ctx->ws_side.coltmp));
  }
  // ---- 1x1-conv gradients of this clone: dI = Wp^T dS + dj (x) a; dWp += dS I^T;
  // dWi += (dI (1-I^2)) X'^T; bias gradients
  ConvGrads cg{};
  cg.n = B; cg.dS = Th; cg.dj = ctx->dj + (size_t)h * BM_; cg.a = ctx->a + (size_t)h * BS_; cg.I = Ih;
  cg.X = xin; cg.dZ = dZh;
  if (int rc = conv_grads(ctx, st, cg)) return rc;
  // ---- gradient w.r.t. q through q_embed's dropout
  float* dqo = ctx->m_dq + (size_t)h * B * Q;
  {
    LinOpts o = lin_opts(ctx, ctx->ws_chain);
    o.emask = m.q;
    o.emask_e0 = (size_t)h * B * Q;
    o.emscale = m.s_q;
    RUN("q_proj_dgrad", gflop(B, Q, M), 0,
        gemm_nn(st, B, Q, M, ctx->dqt + (size_t)h * BM_, M, ctx->q_proj.W, Q, dqo, Q, o));
  }
  // ---- feature-map gradient (the reference computes it and SS:579 throws it away): on request
  if (d_X) {
    if (!ctx->m_dX) {
      if (int rc = dalloc(ctx, &ctx->m_dX, (size_t)ctx->cap * D * S)) return rc;
      if (int rc = dalloc(ctx, &ctx->m_dZ, (size_t)ctx->cap * M * S)) return rc;
    }
    RUN("mul_dtanh", 0, BM_ * S * 12.0, mul_dtanh(st, BM_ * S, dZh, Ih, ctx->m_dZ));
    RUN("conv_embed_dgrad", gflop(D, (double)B * S, M), (BM_ * S + (double)B * D * S) * 4,
        conv_embed_dgrad(st, conv_mode(ctx), B, D, S, M, ctx->m_dZ, ctx->i_embed.W, ctx->m_dX));
    float* dXo = ctx->m_dX;
    if (S != SL) {   // dense [B,D,SL] for the caller (reuses the re-pitch buffer's sibling)
      if (!ctx->m_dXd)
        if (int rc = dalloc(ctx, &ctx->m_dXd, (size_t)ctx->cap * D * SL)) return rc;
      if (int rc = repitch(ctx, ctx->m_dXd, SL, ctx->m_dX, S, (size_t)B * D)) return rc;
      dXo = ctx->m_dXd;
    }
    if (m.x)   // the mask is indexed logically: applied on the dense tensor
      RUN("apply_mask", 0, (double)B * D * SL * 8,
          apply_mask(st, (size_t)B * D * SL, (size_t)B * D * SL, dXo, m.x, m.s_x, dXo,
                     ctx->xdrop == RAU_XDROP_TIED ? 0 : (size_t)h * B * D * SL));
    *d_X = dXo;
  }
  // ---- accGradParameters of the clone's Linears
  const size_t h4 = (size_t)h * B * 4 * R;
  if (int rc = lin_wgrad(ctx, ctx->cls, d_logits, mfh, M)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->lstm_out, ctx->dpre + (size_t)h * BM_, ctx->hh + (size_t)(h + 1) * BR_, R)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->lstm_i2h, ctx->dg4 + h4, ctx->j + (size_t)h * BM_, M)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->lstm_h2h, ctx->dg4 + h4, h_prev, R)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->feat_attprob, ctx->dj + (size_t)h * BM_, ctx->a + (size_t)h * BS_, S)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->att_mem, ctx->dz + (size_t)h * BS_, h_prev, R, true, S)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->att_q, ctx->du + (size_t)h * B * A, ctx->qf + (size_t)h * BM_, M)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->q_proj, ctx->dqt + (size_t)h * BM_, ctx->qd + (size_t)h * B * Q, Q)) return rc;
  if (int rc = lin_wgrad(ctx, ctx->h_proj, ctx->dqt + (size_t)h * BM_, h_prev, R)) return rc;
  // attscore: dws = sum_b dwsp[b]; dbs = sum dz.  ifeatproj bias: sum_b du[b]
  RUN("colsum", 0, (double)B * A * 4,
      colsum_acc(st, B, A, ctx->dwsp + (size_t)h * B * A, A, ctx->att_score.dW, ctx->ws_side.coltmp));
  HIPC(hipMemsetAsync(ctx->tmpS, 0, S * sizeof(float), st));
  RUN("colsum", 0, (double)B * S * 4, colsum_acc(st, B, SL, ctx->dz + (size_t)h * BS_, S, ctx->tmpS, ctx->ws_side.coltmp));
  RUN("colsum", 0, S * 4.0, colsum_acc(st, SL, 1, ctx->tmpS, 1, ctx->att_score.db, ctx->ws_side.coltmp));
  RUN("colsum", 0, (double)B * A * 4,
      colsum_acc(st, B, A, ctx->du + (size_t)h * B * A, A, ctx->att_i.db, ctx->ws_side.coltmp));
  if (d_q) *d_q = dqo;
  if (d_c_prev) *d_c_prev = g.dc_out;
  if (d_h_prev) *d_h_prev = g.dh_out;
  return RAU_OK;
}

// ------------------------------------------------------------ criteria[h]
// One body for the four entry points below (each has called mod_alloc): criteria[h] of `logits` against `t`, the
// step's head kernel without do_pred.  d_logits null: the forward (loss to *loss if asked for); else the gradient.
static int criterion(rau_ctx* ctx, int h, const float* logits, const Truth& t, float* loss, float scale,
                     float** d_logits) {
  const rau_config& c = ctx->cfg;
  float* dl = ctx->dl + (size_t)h * c.B * c.K;
  RUN(criterion_class(t), 0, (double)c.B * c.K * 12,
      criterion_head(ctx->st, c.B, c.K, c.M, logits, t, nullptr, nullptr, nullptr, dl,
                     ctx->lossrow + (size_t)h * c.B, ctx->argmax_d + (size_t)h * c.B, nullptr));
  if (d_logits) {
    if (scale != 1.f)   // dpred:mul(nHop), SS:569
      RUN("scale_hops", 0, (double)c.B * c.K * 8, scale_inplace(ctx->st, (size_t)c.B * c.K, scale, dl));
    *d_logits = dl;
    return RAU_OK;
  }
  RUN("loss_reduce", 0, 0, loss_reduce(ctx->st, 1, c.B, ctx->lossrow + (size_t)h * c.B, ctx->m_loss + h));
  if (!loss) return RAU_OK;
  HIPC(hipMemcpyAsync(loss, ctx->m_loss + h, sizeof(float), hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return RAU_OK;
}

int rau_criterion_forward(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, float* loss) {
  NEED(ctx && logits, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_forward");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_criterion_forward: h=%d out of [0,%d)", h, ctx->cfg.H);
  if (int rc = mod_alloc(ctx)) return rc;
  // labels_dev == NULL: the resident batch's ground truth, which may be its answer set
  const Truth t = labels_dev ? Truth{labels_dev} : truth_of(cur_batch(ctx));
  if (!t.present()) return fail(RAU_ERR_STATE, "rau_criterion_forward: no labels");
  return criterion(ctx, h, logits, t, loss, 1.f, nullptr);
}

int rau_criterion_backward(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev,
                           float scale, float** d_logits) {
  NEED(ctx && logits && d_logits, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_backward");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_criterion_backward: h=%d out of [0,%d)", h, ctx->cfg.H);
  if (int rc = mod_alloc(ctx)) return rc;
  const Truth t = labels_dev ? Truth{labels_dev} : truth_of(cur_batch(ctx));
  if (!t.present()) return fail(RAU_ERR_STATE, "rau_criterion_backward: no labels");
  return criterion(ctx, h, logits, t, nullptr, scale, d_logits);
}

// criteria[h] against an answer set in device memory (ids / w [B,G])
int rau_criterion_forward_set(rau_ctx* ctx, int h, const float* logits, int32_t G, const int32_t* ids_dev,
                              const float* w_dev, float* loss) {
  NEED(ctx && logits && ids_dev && w_dev, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_forward_set");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_criterion_forward_set: h=%d out of [0,%d)", h, ctx->cfg.H);
  NEED(G >= 1 && G <= kMaxAnswers, "rau_criterion_forward_set: G=%d out of [1,%d]", G, kMaxAnswers);
  if (int rc = mod_alloc(ctx)) return rc;
  return criterion(ctx, h, logits, Truth{nullptr, ids_dev, w_dev, nullptr, G}, loss, 1.f, nullptr);
}

int rau_criterion_backward_set(rau_ctx* ctx, int h, const float* logits, int32_t G, const int32_t* ids_dev,
                               const float* w_dev, float scale, float** d_logits) {
  NEED(ctx && logits && ids_dev && w_dev && d_logits, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_backward_set");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_criterion_backward_set: h=%d out of [0,%d)", h, ctx->cfg.H);
  NEED(G >= 1 && G <= kMaxAnswers, "rau_criterion_backward_set: G=%d out of [1,%d]", G, kMaxAnswers);
  if (int rc = mod_alloc(ctx)) return rc;
  return criterion(ctx, h, logits, Truth{nullptr, ids_dev, w_dev, nullptr, G}, nullptr, scale, d_logits);
}

// criteria[h] as the per-answer sigmoid criterion (bce_head.hip), whatever rau_set_answer_loss says: against labels
// in device memory, or (labels_dev NULL) an answer set in device memory
static int bce_truth(const char* fn, const int32_t* labels_dev, int32_t G, const int32_t* ids_dev, const float* w_dev,
                     Truth* t) {
  if (labels_dev) {
    *t = Truth{labels_dev};
  } else {
    NEED(ids_dev && w_dev, "%s: neither labels nor an answer set", fn);
    NEED(G >= 1 && G <= kMaxAnswers, "%s: G=%d out of [1,%d]", fn, G, kMaxAnswers);
    *t = Truth{nullptr, ids_dev, w_dev, nullptr, G};
  }
  t->loss = RAU_LOSS_BCE;
  return RAU_OK;
}

int rau_criterion_forward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, int32_t G,
                              const int32_t* ids_dev, const float* w_dev, float* loss) {
  NEED(ctx && logits, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_forward_bce");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_criterion_forward_bce: h=%d out of [0,%d)", h, ctx->cfg.H);
  Truth t;
  if (int rc = bce_truth("rau_criterion_forward_bce", labels_dev, G, ids_dev, w_dev, &t)) return rc;
  if (int rc = mod_alloc(ctx)) return rc;
  return criterion(ctx, h, logits, t, loss, 1.f, nullptr);
}

int rau_criterion_backward_bce(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, int32_t G,
                               const int32_t* ids_dev, const float* w_dev, float scale, float** d_logits) {
  NEED(ctx && logits && d_logits, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_backward_bce");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_criterion_backward_bce: h=%d out of [0,%d)", h, ctx->cfg.H);
  Truth t;
  if (int rc = bce_truth("rau_criterion_backward_bce", labels_dev, G, ids_dev, w_dev, &t)) return rc;
  if (int rc = mod_alloc(ctx)) return rc;
  return criterion(ctx, h, logits, t, nullptr, scale, d_logits);
}

// criteria[h] restricted to candidates in device memory (cand_head.hip): against labels, or (labels_dev NULL) an
// answer set, with the criterion `kind`
static int cand_truth(rau_ctx* ctx, const char* fn, int h, const int32_t* labels_dev, int32_t G, const int32_t* ids_dev,
                      const float* w_dev, int32_t C, const int32_t* cand_dev, int kind, Truth* t) {
  NEED(h >= 0 && h < ctx->cfg.H, "%s: h=%d out of [0,%d)", fn, h, ctx->cfg.H);
  NEED(kind == RAU_LOSS_CE || kind == RAU_LOSS_BCE, "%s: kind=%d (RAU_LOSS_CE or RAU_LOSS_BCE)", fn, kind);
  NEED(cand_dev, "%s: no candidates", fn);
  NEED(C >= 1 && C <= kMaxCandidates, "%s: C=%d out of [1,%d]", fn, C, kMaxCandidates);
  if (int rc = bce_truth(fn, labels_dev, G, ids_dev, w_dev, t)) return rc;
  t->loss = kind;
  t->cand = cand_dev;
  t->C = C;
  return RAU_OK;
}

int rau_criterion_forward_cand(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, int32_t G,
                               const int32_t* ids_dev, const float* w_dev, int32_t C, const int32_t* cand_dev,
                               int kind, float* loss) {
  NEED(ctx && logits, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_forward_cand");
  Truth t;
  if (int rc = cand_truth(ctx, "rau_criterion_forward_cand", h, labels_dev, G, ids_dev, w_dev, C, cand_dev, kind, &t))
    return rc;
  if (int rc = mod_alloc(ctx)) return rc;
  return criterion(ctx, h, logits, t, loss, 1.f, nullptr);
}

int rau_criterion_backward_cand(rau_ctx* ctx, int h, const float* logits, const int32_t* labels_dev, int32_t G,
                                const int32_t* ids_dev, const float* w_dev, int32_t C, const int32_t* cand_dev,
                                int kind, float scale, float** d_logits) {
  NEED(ctx && logits && d_logits, "null argument");
  NEED_DENSE_K(ctx, "rau_criterion_backward_cand");
  Truth t;
  if (int rc = cand_truth(ctx, "rau_criterion_backward_cand", h, labels_dev, G, ids_dev, w_dev, C, cand_dev, kind, &t))
    return rc;
  if (int rc = mod_alloc(ctx)) return rc;
  return criterion(ctx, h, logits, t, nullptr, scale, d_logits);
}

// ------------------------------------------------------------ the merged rows' criteria
// The step's merge_grad launch (merge_grad.hip) on hop logits and do_pred the caller holds: feval's uni and select
// rows are built from them under the feval rule and the gradient of  merge_w[0] CE(uni) + merge_w[1] CE(select)  is
// ADDED into d_logits_dev [H,n,K] -- the caller's per-hop criterion gradients, already scaled.  It touches no
// ctx-owned slot, so it may run between the hop loops of a module-level feval.
int rau_merge_criterion_backward(rau_ctx* ctx, const float* logits_dev, const float* dopred_dev,
                                 const int32_t* labels_dev, const float* merge_w, float* d_logits_dev) {
  NEED(ctx && logits_dev && dopred_dev && merge_w && d_logits_dev, "null argument");
  NEED_DENSE_K(ctx, "rau_merge_criterion_backward");
  NEED(std::isfinite(merge_w[0]) && std::isfinite(merge_w[1]), "rau_merge_criterion_backward: merge_w is not finite");
  NEED(((uintptr_t)d_logits_dev & 15) == 0, "rau_merge_criterion_backward: d_logits_dev is not 16-byte aligned");
  const Truth t = labels_dev ? Truth{labels_dev} : truth_of(cur_batch(ctx));
  if (!t.present()) return fail(RAU_ERR_STATE, "rau_merge_criterion_backward: no labels");
  if (merge_w[0] == 0.f && merge_w[1] == 0.f) return RAU_OK;   // nothing to add
  const rau_config& c = ctx->cfg;
  RUN("merge_grad", 0, (double)c.H * c.B * c.K * 16,
      merge_grad(ctx->st, c.H, c.B, c.K, logits_dev, dopred_dev, t, nullptr, merge_w[0], merge_w[1], d_logits_dev));
  return RAU_OK;
}

// ------------------------------------------------------------ attention criterion of clone h
// The step's attention supervision (att_sup.hip) on a dense attprob [B,S] the caller holds -- the attprob output of
// rau_multimodal_forward -- against dense targets and optional region counts, all in device memory.
int rau_att_criterion_forward(rau_ctx* ctx, int h, const float* attprob_dev, const float* t_dev,
                              const int32_t* nreg_dev, float* loss) {
  NEED(ctx && attprob_dev && t_dev, "null argument");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_att_criterion_forward: h=%d out of [0,%d)", h, ctx->cfg.H);
  if (int rc = mod_alloc(ctx)) return rc;
  if (int rc = att_stats_alloc(ctx)) return rc;
  const rau_config& c = ctx->cfg;
  float* outf = ctx->att_sf + 2 * (size_t)c.H * ctx->cap;
  int32_t* outi = ctx->att_si + 2 * (size_t)c.H * ctx->cap;
  RUN("att_sup_stats", 0, (double)c.B * c.S * 8,
      att_sup_stats(ctx->st, 1, c.B, c.S, attprob_dev, c.S, t_dev, c.S, nreg_dev, ctx->att_sf, ctx->att_si, outf, outi));
  if (!loss) return RAU_OK;
  HIPC(hipMemcpyAsync(loss, outf, sizeof(float), hipMemcpyDeviceToHost, ctx->st));
  HIPC(hipStreamSynchronize(ctx->st));
  return RAU_OK;
}

int rau_att_criterion_backward(rau_ctx* ctx, int h, const float* attprob_dev, const float* t_dev,
                               const int32_t* nreg_dev, float scale, float** d_attprob) {
  NEED(ctx && attprob_dev && t_dev && d_attprob, "null argument");
  NEED(h >= 0 && h < ctx->cfg.H, "rau_att_criterion_backward: h=%d out of [0,%d)", h, ctx->cfg.H);
  NEED(std::isfinite(scale), "rau_att_criterion_backward: scale is not finite");
  if (int rc = mod_alloc(ctx)) return rc;
  const rau_config& c = ctx->cfg;
  if (!ctx->m_datt)
    if (int rc = dalloc(ctx, &ctx->m_datt, (size_t)ctx->cap * ctx->Sp)) return rc;
  RUN("att_sup_grad", 0, (double)c.B * c.S * 12,
      att_sup_grad(ctx->st, 1, c.B, c.S, attprob_dev, c.S, t_dev, c.S, nreg_dev, nullptr, scale, ctx->m_datt, c.S));
  *d_attprob = ctx->m_datt;
  return RAU_OK;
}

}  // extern "C"
